"""The oracle of the data kernels (csrc/data.hip), one plain numpy / scipy fp64 function per vs_data_* entry point, and the cases of
tests/test_gpu_data_kernels.py.  tests/test_host_data.py pins the functions and asserts, from the oracle alone, the conditions the GPU cases rely on.

    bbox, relabel, crop + pad, clip + centre     plain numpy
    gaussian_axis       scipy.ndimage.gaussian_filter1d(mode="mirror", truncate=4) with the sigma the C ABI receives, float(np.float32(sigma))
    zoom                scipy.ndimage.zoom(mode="mirror", grid_mode=True), order 0 or 1; order 1 optionally clipped to a given range
    spline3_prefilter   scipy.ndimage.spline_filter(order 3, mode="mirror"), fp64
    affine_sample       scipy.ndimage.map_coordinates(order 0 or 3, mode="constant", cval) on oracle.data_cpu.spatial_coords' coordinates, and the
                        distance of every output voxel to the nearest decision point
    minmax              np.nanmin / np.nanmax (the kernel's fminf / fmaxf skip NaN)

Tolerances (derived, not measured).  Integer and copy results and order-0 picks: equal.  fp32 results of fp64 arithmetic (gaussian, zoom order 1,
affine order 3, clip + centre): kernel and oracle each round once to fp32, so they lie at most one fp32 ulp apart: 2^-22 max(1, max |ref|).
fp64 spline coefficients: 1e-12 of the span, the bound tests/test_host_lowres.py holds the same recursion to."""
import numpy as np
from scipy import ndimage as ndi

from oracle.data_cpu import draw_spatial_params, spatial_coords

ONE_ULP = 2.0 ** -22
SPLINE_TOL = 1e-12
NEAR = 1e-9                 # an affine output voxel this close to a decision point is left out, through an explicit mask
NEAR_CAP = 8                # and at most this many per case


def fp32_bound(ref):
    return ONE_ULP * max(1.0, float(np.abs(ref).max()))


# ---- plain numpy ---------------------------------------------------------------------------------------------------------------------------------
def ref_bbox(label):
    """-> (min[3], max[3]) of label > 0, or None (NaN and negative labels are not > 0)"""
    with np.errstate(invalid="ignore"):
        idx = np.array(np.where(np.asarray(label) > 0))
    if idx.shape[1] == 0:
        return None
    return idx.min(1), idx.max(1)


def ref_relabel(x, sources, targets):
    """0 everywhere, then one assignment per (source, target) pair in order: later pairs win.  Every comparison is against the INPUT, so a chain
    [[1, 2], [2, 3]] sends 1 to 2 and 2 to 3; NaN equals nothing."""
    x = np.asarray(x)
    out = np.zeros_like(x)
    for s, t in zip(sources, targets):
        out[x == np.float32(s)] = np.float32(t)
    return out


def ref_crop_pad(src, dst_shape, lo, hi, off):
    """dst[p] = src[p - off + lo] where p - off + lo lies in [lo, hi) on every axis, 0 elsewhere"""
    src = np.asarray(src)
    out = np.zeros(dst_shape, src.dtype)
    sel_d, sel_s = [], []
    for a in range(3):
        p = np.arange(dst_shape[a])
        s = p - off[a] + lo[a]
        ok = (s >= lo[a]) & (s < hi[a])
        sel_d.append(p[ok]); sel_s.append(s[ok])
    if all(len(s) for s in sel_d):
        out[np.ix_(*sel_d)] = src[np.ix_(*sel_s)]
    return out


def ref_crop_pad_cube(vol, centre, L, pad, shift=0):
    """CropResize's cube as the reference writes it: the clipped slice, np.pad with int(d / 2) before and the rest after -> (cube, lo, hi, off)"""
    lo = [max(int(centre[a]) - L // 2 - pad + shift, 0) for a in range(3)]
    hi = [min(int(centre[a]) + L // 2 + pad + shift, vol.shape[a]) for a in range(3)]
    cut = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    diff = [L + 2 * pad - s for s in cut.shape]
    return np.pad(cut, [(int(d / 2), d - int(d / 2)) for d in diff]), lo, hi, [int(d / 2) for d in diff]


def ref_clip_center(x, lo, hi, sub, div):
    """(clip(x, lo, hi) - sub) / div in fp64 on the fp32 values the C ABI receives"""
    lo, hi, sub, div = (np.float64(np.float32(v)) for v in (lo, hi, sub, div))
    return (np.clip(np.asarray(x, np.float64), lo, hi) - sub) / div


def ref_minmax(x):
    return float(np.nanmin(x)), float(np.nanmax(x))


# ---- scipy ---------------------------------------------------------------------------------------------------------------------------------------
def sigma32(sigma):
    return float(np.float32(sigma))


def resize_sigma(n_in, n_out):
    """the sigma data_gpu.resize passes for an axis that shrinks from n_in to n_out (skimage's anti-aliasing)"""
    return max(0.0, (n_in / n_out - 1.0) / 2.0)


def ref_gaussian_axis(x, sigma, axis):
    return ndi.gaussian_filter1d(np.asarray(x).astype(np.float64), sigma32(sigma), axis=axis, mode="mirror", truncate=4)


def ref_zoom(x, out_shape, order, clip=None):
    """fp64; clip = (lo, hi) for order 1: the range the kernel is handed (fp32 values)"""
    x = np.asarray(x)
    y = ndi.zoom(x.astype(np.float64), [o / i for o, i in zip(out_shape, x.shape)], order=order, mode="mirror", grid_mode=True)
    assert y.shape == tuple(out_shape), (y.shape, out_shape)
    if clip is not None and order > 0:
        y = np.clip(y, np.float64(np.float32(clip[0])), np.float64(np.float32(clip[1])))
    return y


def ref_spline3(x):
    return ndi.spline_filter(np.asarray(x).astype(np.float64), 3, output=np.float64, mode="mirror")


def decision_distance(coords, shape, order):
    """(3, *patch) coordinates -> per output voxel the distance to the nearest point where the sampler decides: the borders c = 0 and c = n - 1 of
    mode="constant" and, for order 0, the rounding ties frac(c) = 0.5; minimised over the axes"""
    dist = np.full(coords.shape[1:], np.inf)
    for a in range(3):
        c = coords[a]
        dist = np.minimum(dist, np.minimum(np.abs(c), np.abs(c - (shape[a] - 1))))
        if order == 0:
            dist = np.minimum(dist, np.abs((c - np.floor(c)) - 0.5))
    return dist


def ref_affine(x, coords, order, cval):
    """-> (fp64 values, decision distances)"""
    x = np.asarray(x)
    out = ndi.map_coordinates(x.astype(np.float64), coords, order=order, mode="constant", cval=float(cval))
    return out, decision_distance(coords, x.shape, order)


def affine_coords(patch, angles, scale, centre):
    return spatial_coords(patch, angles, scale, centre)


# ---- the zoom's coordinate rule ------------------------------------------------------------------------------------------------------------------
def mirror(i, n):
    """scipy's 'mirror' on indices: d c b | a b c d | c b a"""
    i = np.abs(np.asarray(i, np.int64))
    if n == 1:
        return np.zeros_like(i)
    i = i % (2 * n - 2)
    return np.where(i >= n, 2 * n - 2 - i, i)


def zoom_coord(m, n, rule="division"):
    """input coordinate of every output index of an axis zoomed from m to n rows.  "division": (o + 0.5) * (m / n) - 0.5, scipy's and the kernel's;
    "product": ((o + 0.5) * m) / n - 0.5, what the kernel computed before: the two differ in the last bit, which decides exact ties"""
    o = np.arange(n, dtype=np.float64) + 0.5
    return (o * (np.float64(m) / np.float64(n)) if rule == "division" else o * np.float64(m) / np.float64(n)) - 0.5


def zoom_pick0(m, n, rule="division"):
    return mirror(np.floor(zoom_coord(m, n, rule) + 0.5).astype(np.int64), m)


def scipy_pick0(m, n):
    got = ndi.zoom(np.arange(m, dtype=np.float64), n / m, order=0, mode="mirror", grid_mode=True)
    assert got.shape == (n,), (m, n, got.shape)
    return got.astype(np.int64)


def zoom_tie_distance(m, n):
    """how close c + 0.5 of the division-first coordinate comes to an integer: 0 at an exact tie"""
    x = zoom_coord(m, n) + 0.5
    return float(np.min(np.abs(x - np.round(x))))


# ---- the inputs of the GPU cases -----------------------------------------------------------------------------------------------------------------
def ramp(shape):
    """a volume whose value is its own linear index (exact in fp32 below 2^24): a wrong pick is a wrong integer"""
    assert int(np.prod(shape)) < 2 ** 24
    return np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)


def noise(shape, seed, scale=300.0, offset=50.0):
    return (np.random.RandomState(seed).randn(*shape) * scale + offset).astype(np.float32)


TIE_PAIRS_SMALL = [(30, 11), (30, 13), (26, 23), (18, 33), (36, 33)]         # the smallest (m, n) on which the product-first rule departs from scipy
TIE_PAIRS_RUN = [(112, 40), (224, 80), (272, 56)]                            # pairs a training or preprocessing run can meet
ZOOM_CASES = [((30, 26, 18), (11, 23, 33)), ((36, 30, 112), (33, 13, 40)), ((272, 3, 2), (56, 1, 5)), ((1, 1, 9), (4, 2, 9))]
ZOOM_TIE_CASES = ZOOM_CASES[:3]                                              # every axis pair of the first two, and 272 -> 56, is a tie pair
ZOOM_SWEEP_CASE = ((3, 4, 5), (257, 256, 256))                               # 16.8 M outputs: past one sweep of the 65,535 x 256 launch grid
SWEEP = 65535 * 256

GAUSS_SHAPES = [(5, 7, 9), (1, 4, 33)]
# 3.0: radius 12, longer than every axis; then what data_gpu.resize passes for 150 -> 64 (0.671875 again), 97 -> 48 (not a float32) and 9 -> 4
GAUSS_SIGMAS = list(dict.fromkeys([0.25, 0.671875, 1.5, 3.0, resize_sigma(150, 64), resize_sigma(97, 48), resize_sigma(9, 4)]))
SPLINE_SHAPES = [(1, 2, 3), (4, 65, 2), (3, 1, 4)]

# exact affine maps: (name, volume shape, patch, angles, scale, centre); every coordinate is a dyadic rational that both implementations compute exactly
_C = lambda shape: tuple((s - 1) / 2.0 for s in shape)                       # noqa: E731
AFFINE_EXACT_CASES = [
    ("identity", (6, 7, 9), (6, 7, 9), (0.0, 0.0, 0.0), 1.0, _C((6, 7, 9))),
    ("shift+2", (6, 7, 9), (6, 7, 9), (0.0, 0.0, 0.0), 1.0, tuple(c + 2 for c in _C((6, 7, 9)))),
    ("shift-2", (6, 7, 9), (6, 7, 9), (0.0, 0.0, 0.0), 1.0, tuple(c - 2 for c in _C((6, 7, 9)))),
    ("scale0.5", (6, 7, 9), (6, 7, 9), (0.0, 0.0, 0.0), 0.5, _C((6, 7, 9))),
    ("scale2", (6, 7, 9), (6, 7, 9), (0.0, 0.0, 0.0), 2.0, _C((6, 7, 9))),
    ("patch-smaller", (6, 7, 9), (3, 4, 5), (0.0, 0.0, 0.0), 1.0, (2.0, 3.5, 4.0)),
    ("patch-larger", (6, 7, 9), (9, 10, 12), (0.0, 0.0, 0.0), 1.0, (2.0, 3.5, 4.5)),
    ("unit-axis", (1, 7, 9), (3, 7, 9), (0.0, 0.0, 0.0), 1.0, _C((1, 7, 9))),
]
AFFINE_GENERAL_SHAPE, AFFINE_GENERAL_PATCH, AFFINE_GENERAL_SEEDS = (20, 24, 28), (16, 16, 16), (0, 1, 2)
AFFINE_CVAL = {0: 0.0, 3: -1024.0}                                           # the pipeline's: label 0, image -1024


def affine_general_params(seed):
    """(angles, scale, centre) as the transform draws them: angles in +-0.2 rad, scale in [0.85, 1.15], the centre at least 5 voxels inside"""
    p = draw_spatial_params(np.random.RandomState(100 + seed), AFFINE_GENERAL_SHAPE, AFFINE_GENERAL_PATCH, [5, 5, 5])
    return p["angles"], p["scale"], p["centre"]


def affine_input(shape, order, seed):
    """order 0: integer labels 1..4 (0 is the border value, so a voxel wrongly taken for outside shows); order 3: intensities"""
    if order == 0:
        return np.random.RandomState(seed).randint(1, 5, size=shape).astype(np.float32)
    return noise(shape, seed)


COUNTS = [1, 4097, 16777216 + 300]                                           # relabel / clip + centre: one element, ragged, past one grid sweep
PAIRS_CHAINED = ([1.0, 2.0], [2.0, 3.0])
PAIRS_16 = ([float(k) for k in range(1, 17)], [float(17 - k) for k in range(1, 17)])
