"""The raster rule of utils.vis restated in plain NumPy, one boolean mask per primitive over the whole
image, with Python integers / int64 throughout.  It shares no code with the package: the tests hold lp_draw_poses,
lp_draw_poses_v and litepose_amd.utils.vis to it bitwise.

  * persons p < min(max(count, 0), pcap); joint position (int(x), int(y)), truncated toward zero
  * a joint is visible iff val > 0, x and y are finite and both truncated coordinates lie in [-16384, 16383]
  * joint mark: (px-cx)^2 + (py-cy)^2 <= Rj^2
  * link (a, b): drawn iff a < J, b < J and both joints are visible; painted iff the squared distance to the segment AB
    is <= Rl^2: with d = AP.AB, L = |AB|^2:  d <= 0: |AP|^2 <= Rl^2;  d >= L: |BP|^2 <= Rl^2;  else cross^2 <= Rl^2 L
  * person p paints palette[p % n_colors]; persons are painted in index order, so the highest index wins
"""
import math

import numpy as np

LO, HI = -16384, 16383


def joint_pos(row):
    """(cx, cy) of a visible joint row (x, y, val, ...), or None."""
    x, y, v = float(row[0]), float(row[1]), float(row[2])
    if not v > 0 or not math.isfinite(x) or not math.isfinite(y):
        return None
    cx, cy = int(x), int(y)
    if not (LO <= cx <= HI and LO <= cy <= HI):
        return None
    return cx, cy


def disc_mask(H, W, c, R):
    py, px = np.mgrid[0:H, 0:W].astype(np.int64)
    return (px - c[0]) ** 2 + (py - c[1]) ** 2 <= R * R


def capsule_mask(H, W, a, b, R):
    py, px = np.mgrid[0:H, 0:W].astype(np.int64)
    apx, apy = px - a[0], py - a[1]
    bpx, bpy = px - b[0], py - b[1]
    abx, aby = b[0] - a[0], b[1] - a[1]
    d = apx * abx + apy * aby
    L = abx * abx + aby * aby
    cross = apx * aby - apy * abx
    r2 = R * R
    return np.where(d <= 0, apx * apx + apy * apy <= r2,
                    np.where(d >= L, bpx * bpx + bpy * bpy <= r2, cross * cross <= r2 * L))


def person_mask(H, W, person, links, Rj=2, Rl=1):
    """Pixels covered by one person [J, >=3]."""
    J = person.shape[0]
    pos = [joint_pos(person[j]) for j in range(J)]
    m = np.zeros((H, W), dtype=bool)
    for c in pos:
        if c is not None:
            m |= disc_mask(H, W, c, Rj)
    for a, b in links:
        if a < J and b < J and pos[a] is not None and pos[b] is not None:
            m |= capsule_mask(H, W, pos[a], pos[b], Rl)
    return m


def draw(image, kpts, count, links, palette=((0, 0, 255),), Rj=2, Rl=1):
    """image [H,W,3] uint8, kpts [pcap,J,>=3], count: returns (drawn copy, mask of covered pixels)."""
    H, W = image.shape[:2]
    out = image.copy()
    mask = np.zeros((H, W), dtype=bool)
    P = min(max(int(count), 0), kpts.shape[0])
    for p in range(P):
        m = person_mask(H, W, kpts[p], links, Rj, Rl)
        out[m] = np.asarray(palette[p % len(palette)], dtype=np.uint8)
        mask |= m
    return out, mask
