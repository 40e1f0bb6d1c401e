"""A numpy / scipy restatement of pasting a crop-space prediction back into scan geometry (include/vaeseg.h "vs_uncrop", data_gpu.crop_geometry,
ops.uncrop): the yardstick of tests/test_host_uncrop.py and tests/test_gpu_uncrop.py.  The reference has no counterpart.

    geometry  CropResize's integers: centre = (max + min) // 2, L = max(max - min), pad = int(0.1 L), lo = max(centre - L // 2 - pad + shift, 0),
              hi = min(centre + L // 2 + pad + shift, S), side = L + 2 pad, off = int((side - (hi - lo)) / 2)
    zoom      per class, in float64, from the patch P^3 to the cube side^3.  linear: scipy.ndimage.zoom(order=1, mode='nearest', grid_mode=True);
              nearest: the sample at floor(q + 0.5), q = (u + 0.5) P / side - 0.5, clamped to [0, P - 1]
    paste     cube rows [off, off + hi - lo) to scan rows [lo, hi); everywhere else the distribution (1, 0, ..., 0)
    label     argmax over the classes, ties to the first maximal channel
"""
import numpy as np
from scipy import ndimage as ndi


def crop_geometry(box, shape, shift=0):
    """box = (min[3], max[3]) -> (lo[3], hi[3], off[3], side)"""
    bmin, bmax = (np.asarray(b).astype(np.int64) for b in box)
    centre, L = (bmax + bmin) // 2, int(np.max(bmax - bmin))
    pad = int(L * 0.1)
    lo = [max(int(centre[d]) - L // 2 - pad + shift, 0) for d in range(3)]
    hi = [min(int(centre[d]) + L // 2 + pad + shift, int(shape[d])) for d in range(3)]
    side = L + 2 * pad
    off = [int((side - (hi[d] - lo[d])) / 2) for d in range(3)]
    return lo, hi, off, side


def box_of(label):
    idx = np.array(np.where(label > 0)).T
    return idx.min(0), idx.max(0)


def patch_coordinate(side, patch):
    """q of every cube index u, float64"""
    return (np.arange(side, dtype=np.float64) + 0.5) * patch / side - 0.5


def nearest_index(side, patch):
    return np.clip(np.floor(patch_coordinate(side, patch) + 0.5), 0, patch - 1).astype(np.int64)


def zoom_nearest(p, side):
    i = nearest_index(side, p.shape[0])
    return p[np.ix_(i, i, i)]


def zoom_linear(p, side):
    out = ndi.zoom(np.asarray(p, dtype=np.float64), side / p.shape[0], order=1, mode="nearest", grid_mode=True)
    assert out.shape == (side,) * 3, out.shape
    return out


def zoom_linear_explicit(p, side):
    """the same map written out: q clamped to [0, P - 1], the two neighbours per axis weighted by the fraction (what the header states)"""
    P = p.shape[0]
    q = np.clip(patch_coordinate(side, P), 0.0, P - 1.0)
    i0 = np.floor(q).astype(np.int64)
    i1 = np.minimum(i0 + 1, P - 1)
    t = q - i0
    out = np.asarray(p, dtype=np.float64)
    for axis in range(3):
        shape = [1, 1, 1]
        shape[axis] = side
        w = t.reshape(shape)
        out = np.take(out, i0, axis=axis) * (1.0 - w) + np.take(out, i1, axis=axis) * w
    return out


def uncrop(prob, geometry, shape, interp="linear"):
    """prob (K, P, P, P) -> {"prob": float64 (K, D, H, W), "label": uint8 (D, H, W), "inside": bool (D, H, W)}"""
    lo, hi, off, side = geometry
    prob = np.asarray(prob)
    out = np.zeros((prob.shape[0],) + tuple(shape), np.float64)
    out[0] = 1.0
    inside = np.zeros(tuple(shape), bool)
    dst = tuple(slice(lo[d], hi[d]) for d in range(3))
    src = tuple(slice(off[d], off[d] + hi[d] - lo[d]) for d in range(3))
    for k in range(prob.shape[0]):
        cube = zoom_linear(prob[k], side) if interp == "linear" else zoom_nearest(prob[k].astype(np.float64), side)
        out[k][dst] = cube[src]
    inside[dst] = True
    return {"prob": out, "label": np.argmax(out, axis=0).astype(np.uint8), "inside": inside}


def top_two_margin(prob):
    """the difference of the two largest class probabilities per voxel (inf for a single class: its label cannot flip)"""
    if prob.shape[0] < 2:
        return np.full(prob.shape[1:], np.inf)
    s = np.sort(prob, axis=0)
    return s[-1] - s[-2]


def softmax_like(k, patch, seed):
    """random smooth-ish probabilities (K, P, P, P), fp32: a softmax of scaled normal logits"""
    rng = np.random.RandomState(seed)
    logits = rng.randn(k, patch, patch, patch) * 2.0
    e = np.exp(logits - logits.max(0, keepdims=True))
    return (e / e.sum(0, keepdims=True)).astype(np.float32)


# ---- the cases of the kernel tests: (name, scan shape, patch, box (min, max) or None, geometry when there is no box) ------------------------------------
# CropResize's side is L + 2 int(0.1 L): 0..9 for L < 10, then 12, 13, ... — 10 and 11 are sides no box gives.  The side-11 case therefore hands its
# geometry to the kernel directly (an interior cube of 11 rows per axis); sides 8 and 12, its neighbours that boxes do give, stand beside it.
SCAN = (23, 30, 41)
PATCH = 16
KERNEL_CASES = [
    ("side11-direct", SCAN, PATCH, None, ([5, 8, 13], [16, 19, 24], [0, 0, 0], 11)),
    ("side8-up", SCAN, PATCH, ((6, 9, 14), (14, 16, 22)), None),
    ("side12-up", SCAN, PATCH, ((4, 10, 20), (14, 18, 29)), None),
    ("side16-identity", SCAN, PATCH, ((3, 8, 12), (17, 20, 25)), None),
    ("side37-down-clipped", SCAN, PATCH, ((2, 5, 4), (20, 25, 35)), None),          # z, y: lo = 0, hi = S, off = 7, 3
    ("side13-one-face", SCAN, PATCH, ((0, 10, 15), (9, 19, 26)), None),               # clipped at z = 0 only: off = (1, 0, 0)
    ("whole-scan", (16, 16, 16), PATCH, ((0, 0, 0), (15, 15, 15)), None),
]
KERNEL_KS = (1, 2, 3, 8)


def case_geometry(case):
    name, shape, patch, box, geometry = case
    return crop_geometry(box, shape) if box is not None else geometry


def case_seed(case, k):
    return 1000 * [c[0] for c in KERNEL_CASES].index(case[0]) + k
