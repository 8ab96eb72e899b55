"""find_peaks of the reference's real-time parser (nano_demo/fast_utils/parse/find_peaks.cpp:9-56) restated with torch on
the CPU, for planes larger than the goldens hold (several 64-column segments, several row bands).  The restatement itself is
pinned to the real reference's goldens by tests/test_fast_parse_cpu.py.  No NaNs: the window test is written as
``max(window) <= v``."""
import numpy as np
import torch
import torch.nn.functional as F


def find_peaks(det, tmap, threshold, window, M):
    """det, tmap [N,J,H,W] float32 arrays -> count [N,J] i32, val / tag [N,J,M] f32, ind [N,J,M,2] i32 = (x, y)."""
    d = torch.from_numpy(np.ascontiguousarray(det))
    N, J, H, W = d.shape
    pooled = F.max_pool2d(d, window, 1, window // 2)            # pads with -inf: the window clamped to the plane
    peak = (~(d < np.float32(threshold)) & ~(pooled > d)).numpy().reshape(N, J, H * W)
    count = np.zeros((N, J), np.int32)
    val = np.zeros((N, J, M), np.float32)
    tag = np.zeros((N, J, M), np.float32)
    ind = np.zeros((N, J, M, 2), np.int32)
    for n in range(N):
        for j in range(J):
            idx = np.flatnonzero(peak[n, j])[:M]                # the first M in raster order
            k = len(idx)
            count[n, j] = k
            val[n, j, :k] = det[n, j].reshape(-1)[idx]
            tag[n, j, :k] = tmap[n, j].reshape(-1)[idx]
            ind[n, j, :k, 0] = idx % W
            ind[n, j, :k, 1] = idx // W
    return count, val, tag, ind


def band_scene(seed, N, J, H, W, rows_per_band, M):
    """Sparse planes that make the device kernel walk its row bands: clusters of equal and near-equal values around the
    band boundaries (a peak's window reaches into the neighbouring band: the halo), planes whose peaks start far down the
    plane or in its last row, empty planes, and cells in the last columns of a row that is no multiple of 64 wide."""
    rng = np.random.default_rng(seed)
    det = np.zeros((N, J, H, W), np.float32)
    tmap = rng.integers(-40, 41, (N, J, H, W)).astype(np.float32) / 8
    levels = np.array([0.25, 0.5, 0.5, 0.75, 1.0], np.float32)
    for n in range(N):
        for j in range(J):
            kind = (n * J + j) % 5
            if kind == 4:
                continue                                         # empty plane
            if kind == 3:                                        # only the last row, last columns included
                for x in (0, W // 2, W - 2, W - 1):
                    det[n, j, H - 1, x] = levels[int(rng.integers(0, 5))]
                continue
            first = (0, H // 3, H - 3 * rows_per_band)[kind]
            bounds = [b for b in range(0, H, rows_per_band) if b >= first][:6]
            for b in bounds:
                for _ in range(3 if kind else 2):
                    y0 = min(max(b + int(rng.integers(-2, 2)), 0), H - 1)
                    x0 = int(rng.integers(0, W)) if rng.random() < 0.7 else W - 1 - int(rng.integers(0, 3))
                    for _ in range(4):                           # a cluster: neighbours suppress or tie each other
                        y = min(max(y0 + int(rng.integers(-2, 3)), 0), H - 1)
                        x = min(max(x0 + int(rng.integers(-2, 3)), 0), W - 1)
                        det[n, j, y, x] = levels[int(rng.integers(0, 5))]
    return det, tmap
