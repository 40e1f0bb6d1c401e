"""The oracle of the surface-distance tests: medpy's assd / hd / hd95 convention restated on scipy.ndimage and numpy, in fp64 and — for unit
spacing — in exact integers (the squared distances are rebuilt from the feature-transform indices, so no comparison goes through a square root).

    surface(X, connectivity)      X & ~binary_erosion(X, structure, border_value=0)
    edt(F, spacing)               per voxel: the integer offsets to the nearest voxel of F, their integer squared length, the fp64 squared distance
    metrics(A, B, spacing, conn)  the record of include/vaeseg.h vs_surface_record
"""
import math

import numpy as np
from scipy import ndimage

FIELDS = ("count_ab", "count_ba", "sum_ab", "sum_ba", "max_sq", "lo_sq", "hi_sq", "assd", "hd", "hd95")
INT_SENTINEL = 2 ** 31 - 1


def structure(connectivity):
    assert connectivity in (6, 26)
    return ndimage.generate_binary_structure(3, 1) if connectivity == 6 else np.ones((3, 3, 3), dtype=bool)


def surface(X, connectivity=6):
    X = np.asarray(X, dtype=bool)
    return X & ~ndimage.binary_erosion(X, structure(connectivity), border_value=0)


def edt(F, spacing=None):
    """F: bool (D, H, W) with at least one True voxel -> (sq_int int64, sq fp64): squared distance to the nearest True voxel, as the integer
    sum of squared index offsets and as sum((s * offset)^2) in fp64 (equal to sq_int for unit spacing)."""
    F = np.asarray(F, dtype=bool)
    assert F.any()
    _, idx = ndimage.distance_transform_edt(~F, sampling=spacing, return_indices=True)
    delta = idx.astype(np.int64) - np.indices(F.shape, dtype=np.int64)
    sq_int = (delta ** 2).sum(0)
    s = np.ones(3) if spacing is None else np.asarray(spacing, dtype=np.float64)
    scaled = delta.astype(np.float64) * s.reshape(3, 1, 1, 1)
    sq = (scaled[0] ** 2 + scaled[1] ** 2) + scaled[2] ** 2
    return sq_int, sq


def brute_force_sq(F):
    """O(V^2): exact integer squared distance of every voxel to the nearest True voxel"""
    F = np.asarray(F, dtype=bool)
    pts = np.argwhere(F).astype(np.int64)
    grid = np.indices(F.shape, dtype=np.int64).reshape(3, -1).T
    d = ((grid[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    return d.min(1).reshape(F.shape)


def metrics(A, B, spacing=None, connectivity=6):
    """-> dict over FIELDS.  Unit spacing: max_sq / lo_sq / hi_sq are exact Python ints.  An empty surface: counts 0, everything else NaN."""
    sa, sb = surface(A, connectivity), surface(B, connectivity)
    if not sa.any() or not sb.any():
        out = {k: float("nan") for k in FIELDS}
        out["count_ab"] = out["count_ba"] = 0
        return out
    pick = 0 if spacing is None else 1
    ab = edt(sb, spacing)[pick][sa]
    ba = edt(sa, spacing)[pick][sb]
    union = np.sort(np.concatenate([ab, ba]))
    n = union.size
    h = 0.95 * (n - 1)
    k = int(math.floor(h))
    conv = int if spacing is None else float
    dist = np.sqrt(union.astype(np.float64))
    sum_ab = math.fsum(np.sqrt(ab.astype(np.float64)))
    sum_ba = math.fsum(np.sqrt(ba.astype(np.float64)))
    return {"count_ab": int(ab.size), "count_ba": int(ba.size), "sum_ab": sum_ab, "sum_ba": sum_ba,
            "max_sq": conv(union[-1]), "lo_sq": conv(union[k]), "hi_sq": conv(union[min(k + 1, n - 1)]),
            "assd": 0.5 * (sum_ab / ab.size + sum_ba / ba.size), "hd": float(dist[-1]), "hd95": float(np.percentile(dist, 95))}


# ---- the hand-derived cases (tests/test_host_surface.py states the derivations) -------------------------------------------------------------
def two_voxels():
    a, b = np.zeros((6, 7, 8), bool), np.zeros((6, 7, 8), bool)
    a[1, 1, 2] = True
    b[1, 4, 6] = True
    return a, b


def shifted_cubes(s=4, t=6):
    a, b = np.zeros((8, 9, 16), bool), np.zeros((8, 9, 16), bool)
    a[2:2 + s, 3:3 + s, 1:1 + s] = True
    b[2:2 + s, 3:3 + s, 1 + t:1 + t + s] = True
    return a, b


def anisotropic():
    a, b = np.zeros((4, 5, 6), bool), np.zeros((4, 5, 6), bool)
    a[1, 1, 1] = True
    b[2, 1, 1] = b[1, 3, 1] = True
    return a, b


ANISO_SPACING = (2.5, 0.8, 0.8)
