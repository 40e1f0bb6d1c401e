"""A numpy / scipy restatement of the reference's dataset preparation (data/data_process.py) and of its inverse (include/vaeseg.h "vs_scan_orient",
"vs_scan_to_native", data_gpu.ScanGeometry / preprocess_scan / make_merge, ops.to_native, evaluation.predict_scan): the yardstick of
tests/test_host_scan.py and tests/test_gpu_scan.py.  Built on oracle.data_cpu.skimage_resize, the only thing taken from the oracle.

    geometry    spacing = the affine's signed diagonal in raw axis order, ind[i] = +1 if spacing[i] < 0 else -1,
                oriented = transpose(raw, [1, 0, 2])[::ind[1], ::ind[0], ::ind[2]], shape_1mm = (oriented_shape * abs(spacing)).astype(int) — the transposed
                shape times the untransposed spacing, as the reference writes it
    forward     image: skimage resize of the oriented float64 volume to shape_1mm (order 1, default anti-aliasing); label: order 0, no anti-aliasing
    cube        bounding box of label > 0 -/+ pad clipped, center = mean(bbox, 1).astype(int), L = the largest extent, rows [c - int(L/2), c - int(L/2) + L)
                clipped; merge = stack((image, label), -1).astype(int16)
    inverse     per axis q = (o + 0.5) n_1mm / n_oriented - 0.5 in float64.  linear: scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) — what
                skimage_resize(order=1, anti_aliasing=False) computes; nearest: the sample at floor(q + 0.5) clamped to [0, n_1mm - 1].  The oriented
                result is carried to the raw axes (un-flip, transpose back) and the label is the argmax over the classes, ties to the first maximal channel
"""
import itertools

import numpy as np

from oracle.data_cpu import skimage_resize
from tests.uncrop_util import softmax_like, top_two_margin  # noqa: F401


def ind_of(spacing):
    return [1 if s < 0 else -1 for s in spacing]


def geometry(raw_shape, spacing):
    """-> {"oriented_shape", "flips" (oriented axis order), "shape_1mm"}"""
    ind = ind_of(spacing)
    oriented = (raw_shape[1], raw_shape[0], raw_shape[2])
    new_size = (np.array(oriented) * np.abs(np.asarray(spacing, dtype=np.float64))).astype(int)
    return {"oriented_shape": oriented, "flips": (ind[1] < 0, ind[0] < 0, ind[2] < 0), "shape_1mm": tuple(int(v) for v in new_size)}


def orient(raw, spacing):
    ind = ind_of(spacing)
    return np.transpose(raw, [1, 0, 2])[::ind[1], ::ind[0], ::ind[2]]


def unorient(oriented, spacing):
    """the inverse of orient: raw[i0, i1, i2] = oriented[f(i1), f(i0), f(i2)] (a flip is its own inverse)"""
    ind = ind_of(spacing)
    return np.transpose(oriented[::ind[1], ::ind[0], ::ind[2]], [1, 0, 2])


def preprocess(raw, spacing, label=None, label_spacing=None):
    """-> {"image": float64 (D1, H1, W1), "label": float64 or None, "shape_1mm"}"""
    new_size = geometry(raw.shape, spacing)["shape_1mm"]
    image = skimage_resize(orient(raw, spacing).astype(np.float64), new_size)
    lab = None
    if label is not None:
        lab = skimage_resize(orient(label, spacing if label_spacing is None else label_spacing).astype(np.float64), new_size, order=0, anti_aliasing=False)
    return {"image": image, "label": lab, "shape_1mm": new_size}


def foreground_cube(label, pad=32):
    idx = np.array(np.where(label > 0))
    bbox = np.array([[max(0, idx[d].min() - pad), min(label.shape[d], idx[d].max() + pad)] for d in range(3)])
    center = np.mean(bbox, 1).astype(int)
    L = int(np.max(bbox[:, 1] - bbox[:, 0]))
    return tuple(slice(max(0, center[d] - int(L / 2)), min(label.shape[d], center[d] - int(L / 2) + L)) for d in range(3))


def make_merge(image, label, pad=32):
    """-> (slices, the float64 cube before truncation (d, h, w, 2), merge = its astype(int16))"""
    sl = foreground_cube(label, pad)
    cube = np.stack((image[sl], label[sl]), axis=-1)
    return sl, cube, cube.astype(np.int16)


def coordinate(n_out, n_in):
    """the input coordinate q of every output index, float64: a zoom from n_in to n_out rows"""
    return (np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5


def tie_distance(n_in, n_out):
    """how close the order-0 zoom's q + 0.5 comes to an integer, where floor() would turn on the last bit"""
    x = coordinate(n_out, n_in) + 0.5
    return float(np.min(np.abs(x - np.round(x))))


def forward_tie_distance(raw_shape, spacing):
    g = geometry(raw_shape, spacing)
    return min(tie_distance(g["oriented_shape"][a], g["shape_1mm"][a]) for a in range(3))


def nearest_index(n_out, n_in):
    return np.clip(np.floor(coordinate(n_out, n_in) + 0.5), 0, n_in - 1).astype(np.int64)


def zoom_linear(p, out_shape):
    out = skimage_resize(np.asarray(p, dtype=np.float64), out_shape, order=1, anti_aliasing=False)
    assert out.shape == tuple(out_shape), (out.shape, out_shape)
    return out


def zoom_nearest(p, out_shape):
    return p[np.ix_(*[nearest_index(out_shape[a], p.shape[a]) for a in range(3)])]


def to_native(src, raw_shape, spacing, interp="linear"):
    """src (K, D1, H1, W1) probabilities -> {"prob": float64 (K, X, Y, Z), "label": uint8 (X, Y, Z)}; src (D1, H1, W1) integer label -> {"label"}"""
    src = np.asarray(src)
    oriented_shape = geometry(raw_shape, spacing)["oriented_shape"]
    if src.ndim == 3:
        return {"label": np.ascontiguousarray(unorient(zoom_nearest(src, oriented_shape), spacing)).astype(np.uint8)}
    zoom = zoom_linear if interp == "linear" else zoom_nearest
    prob = np.stack([np.ascontiguousarray(unorient(zoom(src[k].astype(np.float64), oriented_shape), spacing)) for k in range(src.shape[0])])
    assert prob.shape[1:] == tuple(raw_shape)
    return {"prob": prob, "label": np.argmax(prob, axis=0).astype(np.uint8)}


# ---- the cases of the kernel tests ---------------------------------------------------------------------------------------------------------------
SIGNS = list(itertools.product((-1.0, 1.0), repeat=3))
# (name, raw shape, |spacing|); test_host_scan.py asserts the tie distances, with the zoom's output shapes
#   down-in-plane   oriented (9, 12, 7) -> 1 mm (7, 8, 17): anti-aliased in-plane, upsampled through-plane; tie distance 0.029
#   up-in-plane     oriented (6, 9, 15) -> 1 mm (10, 12, 10): the other way round; tie distance 0.1
TIE_FREE_CASES = [
    ("down-in-plane", (12, 9, 7), (0.8, 0.7, 2.5)),
    ("up-in-plane", (9, 6, 15), (1.7, 1.4, 0.7)),
]
#   tie             oriented (8, 6, 30) -> 1 mm (11, 7, 11): (o + 0.5) 30 / 11 and (o + 0.5) 8 / 11 are whole numbers at o = 5 ((o + 0.5) 6 / 7 at o = 3), so the forward order-0
#                   resize of the label turns on an exact tie there; 30 -> 11 is a pair on which only the division-first coordinate,
#                   (o + 0.5) (n_in / n_out) - 0.5, picks scipy's voxel (tests/test_host_data.py)
TIE_CASES = [
    ("tie", (6, 8, 30), (1.4, 1.2, 0.37)),
]
KERNEL_CASES = TIE_FREE_CASES + TIE_CASES
# further geometries of the inverse alone, where a forward tie plays no part: a 64-long contiguous axis, a one-row 1 mm axis, an identity grid
NATIVE_CASES = TIE_FREE_CASES + [
    ("z64", (5, 7, 64), (1.3, 0.9, 0.55)),
    ("thin", (6, 5, 3), (1.1, 2.0, 0.4)),
    ("identity", (7, 6, 9), (1.0, 1.0, 1.0)),
]
KERNEL_KS = (1, 2, 3, 8)
ORIENT_SHAPES = [(12, 9, 7), (5, 3, 1), (3, 4, 65), (7, 5, 8)]
ORIENT_DTYPES = ("int16", "uint8", "int8", "float32")


def signed(spacing, signs):
    return tuple(float(a) * float(s) for a, s in zip(spacing, signs))


def case_signs(index):
    """a sign combination per case that differs from case to case (all eight are run by the tests that say so)"""
    return SIGNS[(3 * index + 1) % 8]


def case_spacing(case, cases):
    """the case's |spacing| under its own sign combination"""
    return signed(case[2], case_signs([c[0] for c in cases].index(case[0])))


def native_input(case, k):
    """-> (signed spacing, probabilities (K, D1, H1, W1) fp32) of an inverse case: the same numbers in the host and the GPU tests"""
    spacing = case_spacing(case, NATIVE_CASES)
    index = [c[0] for c in NATIVE_CASES].index(case[0])
    return spacing, probabilities(k, geometry(case[1], spacing)["shape_1mm"], 100 * index + k)


def random_raw(shape, dtype, seed):
    rng = np.random.RandomState(seed)
    if dtype == "float32":
        return (rng.randn(*shape) * 300.0).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.randint(max(info.min, -1024), min(info.max, 3000) + 1, size=shape).astype(dtype)


def smooth_scan(shape, seed):
    """an int16 scan with structure at several scales (so that anti-aliasing and interpolation both matter) and a two-class blob label"""
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, s) for s in shape], indexing="ij")
    r = (g[0] / 0.7) ** 2 + (g[1] / 0.6) ** 2 + (g[2] / 0.8) ** 2
    img = 400.0 * np.exp(-2.0 * r) - 150.0 + 60.0 * np.sin(5.0 * g[0] + 3.0 * g[1]) + rng.randn(*shape) * 40.0
    label = np.where(r < 0.25, 2, np.where(r < 0.8, 1, 0)).astype(np.uint8)
    return np.round(img).astype(np.int16), label


def probabilities(k, shape, seed):
    """uncrop_util.softmax_like's probabilities cut to the box `shape`: (K, D1, H1, W1), fp32, still summing to one per voxel"""
    return np.ascontiguousarray(softmax_like(k, max(shape), seed)[:, :shape[0], :shape[1], :shape[2]])
