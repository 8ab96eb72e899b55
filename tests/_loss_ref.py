"""Plain fp64 restatements of the train loader's label side and of lib/core/loss.py, for the tests of lp_target_maps and
lp_pose_loss (tests/test_gpu_train_*.py, tests/test_train_cpu.py) and for the fixture tests/golden/golden_targets.npz,
which stores their values beside the real reference's.  numpy only.

The loss functions take the fp32 inputs widened to fp64 and round nothing: a device result is held to ONE fp32 rounding
of these values.  The tag terms add in a stated order (joints in slot order, pairs row by row) so that the only freedom
left to an implementation that follows it is its ``exp``."""
import numpy as np


def cells(joints, mat, flip, flip_index, R):
    """RandomAffineTransform._affine_joints + RandomHorizontalFlip on float64 [P,J,3] joints -> (cx, cy, ok) [P,J]:
    (m0*x + m1*y) + m2 per operation, output joint j from source joint flip_index[j] and x = R - x - 1 when mirrored,
    the cell truncated toward zero, ok iff v > 0 and the cell lies in the plane."""
    j = np.asarray(joints, np.float64)
    if flip:
        j = j[:, list(flip_index)]
    m = np.asarray(mat, np.float64).reshape(-1)
    x, y, v = j[..., 0], j[..., 1], j[..., 2]
    tx = (m[0] * x + m[1] * y) + m[2]
    ty = (m[3] * x + m[4] * y) + m[5]
    if flip:
        tx = (R - tx) - 1
    inside = (tx > -1) & (tx < R) & (ty > -1) & (ty < R) & (v > 0)
    cx = np.where(inside, np.trunc(np.where(inside, tx, 0)), 0).astype(np.int64)
    cy = np.where(inside, np.trunc(np.where(inside, ty, 0)), 0).astype(np.int64)
    return cx, cy, inside


def heatmaps(cx, cy, ok, table, R):
    """HeatmapGenerator.__call__ as a gather: float32 [J,R,R], per pixel the maximum of the fp32 ``table`` entries of the
    windows [c - 3 sigma - 1, c + 3 sigma + 2) that cover it."""
    side = table.shape[0]
    s3 = (side - 3) // 2
    P, J = ok.shape
    out = np.zeros((J, R, R), np.float32)
    for p in range(P):
        for j in range(J):
            if not ok[p, j]:
                continue
            ux, uy = int(cx[p, j]) - s3 - 1, int(cy[p, j]) - s3 - 1
            x0, x1, y0, y1 = max(ux, 0), min(ux + side, R), max(uy, 0), min(uy + side, R)
            out[j, y0:y1, x0:x1] = np.maximum(out[j, y0:y1, x0:x1], table[y0 - uy:y1 - uy, x0 - ux:x1 - ux])
    return out


def joints_tensor(cx, cy, ok, R, M, tag_per_joint):
    """JointsGenerator.__call__: int32 [M,J,2]."""
    P, J = ok.shape
    out = np.zeros((M, J, 2), np.int32)
    for p in range(P):
        tot = 0
        for j in range(J):
            if ok[p, j]:
                out[p, tot] = ((j * R * R if tag_per_joint else 0) + cy[p, j] * R + cx[p, j], 1)
                tot += 1
    return out


def heat_loss(pred, gt, mask, factor):
    """HeatmapLoss.forward for one image: pred, gt [J,R,R], mask [R,R] (fp32) -> fp64 mean((pred - gt)^2 * mask) * factor,
    ``factor`` the fp32 factor widened."""
    d = pred.astype(np.float64) - gt.astype(np.float64)
    return float(np.sum((d * d) * mask.astype(np.float64)[None]) / d.size * float(np.float32(factor)))


def tag_loss(tagmaps, joints, loss_type, push_factor, pull_factor):
    """AELoss.batchTagLoss for one image, before the mean over the batch: tagmaps fp32 [K,R,R], joints int [M,J,2] ->
    (push, pull) fp64, times the fp32 factors widened."""
    flat = tagmaps.astype(np.float64).reshape(-1)
    means, pulls = [], []
    for person in joints:
        tags = [flat[int(i)] for i, v in person if v > 0 and 0 <= int(i) < flat.size]
        if not tags:
            continue
        s = 0.0
        for t in tags:
            s += t
        mean = s / len(tags)
        sq = 0.0
        for t in tags:
            sq += (t - mean) * (t - mean)
        means.append(mean)
        pulls.append(sq / len(tags))
    pull = 0.0
    for v in pulls:
        pull += v
    cnt = len(means)
    pull = pull / (cnt if cnt else 1)
    push = 0.0
    if cnt >= 2:
        for a in means:
            row = 0.0
            for b in means:
                d = a - b
                row += float(np.exp(-(d * d))) if loss_type == 'exp' else max(1.0 - abs(d), 0.0)
            push += row
        push = 0.5 * (push - cnt) / max((cnt - 1) * cnt, 1)
    return push * float(np.float32(push_factor)), pull * float(np.float32(pull_factor))


def ulp32(v):
    """One fp32 unit in the last place at fp64 value ``v`` (the spacing of fp32 numbers around it)."""
    return float(np.spacing(np.float32(abs(v)))) if np.isfinite(v) else float('nan')
