"""GPU: every vs_data_* entry point of csrc/data.hip on its own, called through the library (or its thin data_gpu wrapper), against the fp64 oracle of
tests/data_util.py at the smallest shapes that can go wrong: axes of length 1, 2 and 3, axes shorter than the filter radius, samples exactly on the
volume's border, exact order-0 ties, more elements than one sweep of the 65,535 x 256 launch grid.

Tolerances are derived (tests/data_util.py): integer and copy results and order-0 picks are equal; fp32 results of fp64 arithmetic lie within
2^-22 max(1, max |ref|); fp64 spline coefficients within 1e-12 of the span.  Nothing accepts a share of mismatching voxels: the general affine maps
leave out, through an explicit mask, the voxels whose coordinate lies within 1e-9 of a decision point — at most 8 per case, which
tests/test_host_data.py asserts from the oracle alone.

The order-0 zoom cases hold exact ties on which ((o + 0.5) n_in) / n_out, the coordinate dp_zoom_kernel formed before, picks another voxel than
scipy: on that kernel test_zoom_order0_ramps fails for the first three shape pairs (a whole plane per wrong index) and passes for the fourth."""
import ctypes

import numpy as np
import pytest
import torch

from tests import data_util as U

pytestmark = pytest.mark.gpu
EINVAL, ESHAPE = -1, -2


def _lib():
    from vae_segmentation_amd._lib import check, lib
    return lib, check


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ints(v):
    return (ctypes.c_int * 3)(*[int(x) for x in v])


def _floats(v):
    return (ctypes.c_float * len(v))(*[float(x) for x in v])


def assert_close32(got, ref, what):
    """fp32 result of fp64 arithmetic against the fp64 oracle"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    err, bound = float(np.abs(got.astype(np.float64) - ref).max()), U.fp32_bound(ref)
    print(what, "max abs err %.3g, bound %.3g" % (err, bound))
    assert err <= bound, (what, err, bound)


# ---- gaussian_axis -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", U.GAUSS_SHAPES)
def test_gaussian_axis(shape):
    """every axis x every sigma; sigma 3.0 has radius 12, longer than every axis of (5, 7, 9), so the mirror wraps more than once; an axis of length 1
    returns the input"""
    lib, check = _lib()
    x = U.noise(shape, 11)
    src = dev(x)
    for sigma in U.GAUSS_SIGMAS:
        for axis in range(3):
            out = torch.full_like(src, float("nan"))
            check(lib.vs_data_gaussian_axis(src.data_ptr(), out.data_ptr(), *shape, axis, sigma, _stream()), "data_gaussian_axis")
            assert_close32(out, U.ref_gaussian_axis(x, sigma, axis), "gaussian %s sigma %g axis %d" % (shape, sigma, axis))
            if shape[axis] == 1:
                assert torch.equal(out, src)
    assert torch.equal(src, dev(x))
    assert lib.vs_data_gaussian_axis(src.data_ptr(), src.data_ptr(), *shape, 0, 1.0, _stream()) == EINVAL          # in place
    assert lib.vs_data_gaussian_axis(src.data_ptr(), out.data_ptr(), *shape, 3, 1.0, _stream()) == EINVAL
    assert lib.vs_data_gaussian_axis(src.data_ptr(), out.data_ptr(), *shape, 0, 0.0, _stream()) == EINVAL


# ---- zoom --------------------------------------------------------------------------------------------------------------------------------------------
def _zoom(x, out_shape, order, clip=(1.0, 0.0)):
    lib, check = _lib()
    src = dev(x)
    out = torch.full(out_shape, float("nan"), device="cuda")
    check(lib.vs_data_zoom(src.data_ptr(), out.data_ptr(), *x.shape, *out_shape, order, clip[0], clip[1], _stream()), "data_zoom")
    return out.cpu().numpy()


@pytest.mark.parametrize("src,dst", U.ZOOM_CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_zoom_order0_ramps(src, dst):
    """the value is the source's linear index, so a wrong pick is a wrong integer; compared with == against scipy, exact ties included"""
    x = U.ramp(src)
    got, want = _zoom(x, dst, 0), U.ref_zoom(x, dst, 0)
    wrong = got.astype(np.float64) != want
    print("zoom order 0", src, "->", dst, "voxels differing %d of %d" % (int(wrong.sum()), wrong.size))
    assert np.array_equal(got.astype(np.float64), want)


def test_zoom_order0_past_one_grid_sweep():
    """16.8 M outputs, more than 65,535 x 256 threads: the grid-stride loop's second sweep, against the index rule"""
    src, dst = U.ZOOM_SWEEP_CASE
    x = U.ramp(src)
    got = _zoom(x, dst, 0)
    want = x[np.ix_(*[U.zoom_pick0(m, n) for m, n in zip(src, dst)])]
    assert got.size > U.SWEEP and np.array_equal(got, want)
    assert np.array_equal(got.reshape(-1)[U.SWEEP - 2:], want.reshape(-1)[U.SWEEP - 2:])


@pytest.mark.parametrize("src,dst", U.ZOOM_CASES, ids=lambda s: "x".join(str(v) for v in s))
def test_zoom_order1(src, dst):
    """random data; without the clip, clipped to the input's range (what data_gpu.resize passes) and clipped to a range narrower than the data"""
    x = U.noise(src, 13)
    lo, hi = float(x.min()), float(x.max())
    narrow = (float(np.float32(lo + 0.3 * (hi - lo))), float(np.float32(hi - 0.3 * (hi - lo)))) if hi > lo else (lo, hi)
    for clip in (None, (lo, hi), narrow):
        got = _zoom(x, dst, 1, (1.0, 0.0) if clip is None else clip)
        want = U.ref_zoom(x, dst, 1, clip)
        assert_close32(got, want, "zoom order 1 %s -> %s clip %s" % (src, dst, clip))
        if clip is not None:
            assert got.min() >= np.float32(clip[0]) and got.max() <= np.float32(clip[1])
    if x.size > 1:
        assert (want == narrow[0]).any() and (want == narrow[1]).any()              # the narrow clip has work on both sides
    lib, _ = _lib()
    assert lib.vs_data_zoom(dev(x).data_ptr(), dev(x).data_ptr(), *src, *dst, 2, 1.0, 0.0, _stream()) == EINVAL
    assert lib.vs_data_zoom(dev(x).data_ptr(), dev(x).data_ptr(), *src, 0, 1, 1, 0, 1.0, 0.0, _stream()) == EINVAL


def test_resize_wrapper_takes_the_ties_as_scipy_does():
    """data_gpu.resize(order=0), the call of CropResize's label and of preprocess_scan's label, on a tie pair a run can meet: 112 -> 40"""
    from oracle import data_cpu as O
    from vae_segmentation_amd import data_gpu as D
    lab = np.random.RandomState(2).randint(0, 3, size=(112, 30, 26)).astype(np.float32)
    got = D.resize(dev(lab), (40, 11, 23), order=0, anti_aliasing=False)
    assert np.array_equal(got.cpu().numpy(), O.skimage_resize(lab, (40, 11, 23), order=0, anti_aliasing=False))


# ---- spline3_prefilter ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", U.SPLINE_SHAPES)
def test_spline3_prefilter(shape):
    """lines of length 1 (left as they are), 2, 3, 4 and 65 on each axis"""
    lib, check = _lib()
    x = U.noise(shape, 17)
    src = dev(x)
    coef = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    check(lib.vs_data_spline3_prefilter(src.data_ptr(), coef.data_ptr(), *shape, _stream()), "data_spline3_prefilter")
    got, want = coef.cpu().numpy(), U.ref_spline3(x)
    span = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print("spline3", shape, "max abs err %.3g of a span of %.4g" % (err, span))
    assert err <= U.SPLINE_TOL * span
    if shape == (1, 2, 3):
        one = torch.full((1, 1, 1), float("nan"), dtype=torch.float64, device="cuda")
        check(lib.vs_data_spline3_prefilter(src.data_ptr(), one.data_ptr(), 1, 1, 1, _stream()), "data_spline3_prefilter")
        assert one.item() == float(x.reshape(-1)[0])


# ---- affine_sample -------------------------------------------------------------------------------------------------------------------------------------
def _affine(x, patch, angles, scale, centre, order, cval):
    from vae_segmentation_amd import data_gpu as D
    return D.affine_resample(dev(x), patch, angles, scale, centre, order, cval).cpu().numpy()


@pytest.mark.parametrize("case", U.AFFINE_EXACT_CASES, ids=lambda c: c[0])
def test_affine_sample_exact_maps(case):
    """coordinates that both implementations compute without rounding, so every voxel is compared: the border voxels at 0 and n - 1, the exact .5 ties
    of scale 0.5, and the set of cval voxels, which must be exactly the oracle's"""
    name, shape, patch, angles, scale, centre = case
    coords = U.affine_coords(patch, angles, scale, centre)
    for order in (0, 3):
        x, cval = U.affine_input(shape, order, 5), U.AFFINE_CVAL[order]
        got = _affine(x, patch, angles, scale, centre, order, cval)
        want, _ = U.ref_affine(x, coords, order, cval)
        assert np.array_equal(got == np.float32(cval), want == cval), (name, order)
        if order == 0:
            assert np.array_equal(got.astype(np.float64), want), name
        else:
            assert_close32(got, want, "affine order 3 %s" % name)
        if name == "identity":
            if order == 0:
                assert np.array_equal(got, x)
            else:
                assert float(np.abs(got.astype(np.float64) - x).max()) <= U.fp32_bound(x)


@pytest.mark.parametrize("seed", U.AFFINE_GENERAL_SEEDS)
def test_affine_sample_general_maps(seed):
    """rotation, scale and an off-grid centre: the kernel's A u + ctr and the oracle's (u R) scale + ctr differ in the last bits of the coordinate, so
    the voxels within 1e-9 of a border or of an order-0 tie are left out by mask (at most 8); everywhere else order 0 is equal and order 3 within the bound"""
    angles, scale, centre = U.affine_general_params(seed)
    coords = U.affine_coords(U.AFFINE_GENERAL_PATCH, angles, scale, centre)
    for order in (0, 3):
        x, cval = U.affine_input(U.AFFINE_GENERAL_SHAPE, order, seed), U.AFFINE_CVAL[order]
        got = _affine(x, U.AFFINE_GENERAL_PATCH, angles, scale, centre, order, cval)
        want, dist = U.ref_affine(x, coords, order, cval)
        keep = dist > U.NEAR
        assert int((~keep).sum()) <= U.NEAR_CAP
        if order == 0:
            assert np.array_equal(got.astype(np.float64)[keep], want[keep]), seed
        else:
            err, bound = float(np.abs(got.astype(np.float64) - want)[keep].max()), U.fp32_bound(want)
            print("affine order 3 seed", seed, "max abs err %.3g, bound %.3g, left out %d" % (err, bound, int((~keep).sum())))
            assert err <= bound, (seed, err, bound)


def test_affine_sample_argument_errors():
    lib, _ = _lib()
    a9, c3 = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (ctypes.c_double * 3)(0, 0, 0)
    x = torch.zeros(2, 2, 2, device="cuda")
    for order in (1, 2, -1):
        assert lib.vs_data_affine_sample(x.data_ptr(), x.data_ptr(), 2, 2, 2, 2, 2, 2, a9, c3, order, 0.0, _stream()) == EINVAL
    assert lib.vs_data_affine_sample(x.data_ptr(), x.data_ptr(), 2, 2, 2, 2, 0, 2, a9, c3, 0, 0.0, _stream()) == EINVAL
    assert lib.vs_data_affine_sample(x.data_ptr(), x.data_ptr(), 2, 2, 2, 2, 2, 2, None, c3, 0, 0.0, _stream()) == EINVAL


# ---- minmax --------------------------------------------------------------------------------------------------------------------------------------------
def _minmax(x):
    lib, check = _lib()
    src = dev(np.asarray(x, np.float32))
    mm = torch.full((2,), float("nan"), device="cuda")
    check(lib.vs_data_minmax(src.data_ptr(), src.numel(), mm.data_ptr(), _stream()), "data_minmax")
    return tuple(float(v) for v in mm.cpu())


def test_minmax():
    rng = np.random.RandomState(19)
    neg = -np.abs(rng.randn(33, 5, 7).astype(np.float32)) - 1.0                     # all negative: a maximum that starts at 0 would win
    assert _minmax(neg) == U.ref_minmax(neg)
    assert _minmax([-3.5]) == (-3.5, -3.5) and _minmax([7.25]) == (7.25, 7.25)      # a single voxel
    for shape in ((4097,), (33, 47, 29)):                                           # the extremes in the last element
        for sign in (1.0, -1.0):
            x = rng.randn(*shape).astype(np.float32)
            x.reshape(-1)[-1] = sign * 100.0
            assert _minmax(x) == U.ref_minmax(x) and sign * 100.0 in _minmax(x)
    assert _minmax([0.0, -0.0, 0.0]) == (0.0, 0.0) and _minmax([-0.0]) == (0.0, 0.0)            # signed zeros compare equal
    x = rng.randn(4097).astype(np.float32)
    x[[0, 1000, 4096]] = np.nan                                                     # fminf / fmaxf skip NaN: np.nanmin / np.nanmax
    assert _minmax(x) == U.ref_minmax(x)
    lib, _ = _lib()
    assert lib.vs_data_minmax(dev(x).data_ptr(), 0, dev(x).data_ptr(), _stream()) == EINVAL


# ---- bbox ----------------------------------------------------------------------------------------------------------------------------------------------
def _bbox(label):
    lib, check = _lib()
    src = dev(np.asarray(label, np.float32))
    box = torch.full((6,), 12345, dtype=torch.int32, device="cuda")
    check(lib.vs_data_bbox(src.data_ptr(), *src.shape, box.data_ptr(), _stream()), "data_bbox")
    return box.cpu().numpy()


def test_bbox():
    from vae_segmentation_amd import data_gpu as D
    shape = (9, 10, 11)
    for corner in np.ndindex(2, 2, 2):                                              # one voxel at each of the eight corners
        lab = np.zeros(shape, np.float32)
        at = tuple(c * (s - 1) for c, s in zip(corner, shape))
        lab[at] = 2.0
        assert _bbox(lab).tolist() == list(at) + list(at)
        assert [v.tolist() for v in U.ref_bbox(lab)] == [list(at), list(at)]
    both = np.zeros(shape, np.float32)
    both[0, 9, 0] = both[8, 0, 10] = 1.0
    assert _bbox(both).tolist() == [0, 0, 0, 8, 9, 10]
    big = np.zeros((129, 64, 64), np.float32)                                       # the last element of a volume of several workgroups
    big[-1, -1, -1] = 0.5
    assert _bbox(big).tolist() == [128, 63, 63, 128, 63, 63]
    odd = -np.ones(shape, np.float32)                                               # negative and NaN labels are not > 0
    odd[1, 2, 3] = np.nan
    assert _bbox(odd).tolist() == [2 ** 31 - 1] * 3 + [-1] * 3 and D.bounding_box(dev(odd)) is None and U.ref_bbox(odd) is None
    odd[4, 5, 6] = 3.0
    odd[2, 7, 1] = 1e-30
    got, want = D.bounding_box(dev(odd)), U.ref_bbox(odd)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].tolist() == [2, 5, 1]
    assert D.bounding_box(torch.zeros(1, 1, 1, device="cuda")) is None              # an empty label
    assert _bbox(np.ones((1, 1, 1))).tolist() == [0] * 6
    lib, _ = _lib()
    assert lib.vs_data_bbox(dev(odd).data_ptr(), 9, 0, 11, dev(odd).data_ptr(), _stream()) == EINVAL


# ---- relabel, clip_center ------------------------------------------------------------------------------------------------------------------------------
def _relabel(x, sources, targets):
    lib, check = _lib()
    src = dev(x)
    out = torch.full_like(src, float("nan"))
    check(lib.vs_data_relabel(src.data_ptr(), out.data_ptr(), src.numel(), _floats(sources), _floats(targets), len(sources), _stream()), "data_relabel")
    return out.cpu().numpy()


@pytest.mark.parametrize("count", U.COUNTS)
def test_relabel(count):
    x = np.random.RandomState(23).randint(0, 20, size=count).astype(np.float32)
    for sources, targets in (U.PAIRS_CHAINED, U.PAIRS_16, ([1.0, 1.0], [4.0, 7.0]), ([], [])):
        assert np.array_equal(_relabel(x, sources, targets), U.ref_relabel(x, sources, targets)), (count, sources)
    if count == 4097:
        x[[0, 77, 4096]] = np.nan                                                   # NaN equals no source: 0
        x[1] = 1.0
        got = _relabel(x, *U.PAIRS_CHAINED)
        assert np.array_equal(got, U.ref_relabel(x, *U.PAIRS_CHAINED)) and got[[0, 77, 4096]].tolist() == [0, 0, 0] and got[1] == 2.0
        assert np.array_equal(_relabel(np.float32([1, 2, 3]), *U.PAIRS_CHAINED), np.float32([2, 3, 0]))      # the later pair does not re-map the earlier one's target


def test_relabel_argument_errors():
    from vae_segmentation_amd import data_gpu as D
    from vae_segmentation_amd._lib import VaesegError
    lib, _ = _lib()
    x = torch.zeros(2, 2, 2, device="cuda")
    seventeen = [float(k) for k in range(17)]
    assert lib.vs_data_relabel(x.data_ptr(), x.data_ptr(), 8, _floats(seventeen), _floats(seventeen), 17, _stream()) == EINVAL
    assert lib.vs_data_relabel(x.data_ptr(), x.data_ptr(), 0, _floats([1.0]), _floats([1.0]), 1, _stream()) == EINVAL
    assert lib.vs_data_relabel(x.data_ptr(), x.data_ptr(), 8, None, None, 1, _stream()) == EINVAL
    with pytest.raises(VaesegError):
        D.relabel(x, [[list(range(17)), 1]])
    assert np.array_equal(D.relabel(x + 3, [[list(range(16)), 5]]).cpu().numpy(), np.full((2, 2, 2), 5.0, np.float32))


@pytest.mark.parametrize("count", U.COUNTS)
def test_clip_center(count):
    lib, check = _lib()
    x = (np.random.RandomState(29).randn(count) * 400 + 100).astype(np.float32)
    for lo, hi, sub, div in ((-200.0, 400.0, 100.0, 300.0), (-200.0, 400.0, 0.0, 1.0), (-3.0e38, 3.0e38, 100.0, 300.0), (0.1, 0.1, -0.7, 3.0)):
        buf = dev(x)
        check(lib.vs_data_clip_center(buf.data_ptr(), count, lo, hi, sub, div, _stream()), "data_clip_center")
        assert_close32(buf, U.ref_clip_center(x, lo, hi, sub, div), "clip_center %d %s" % (count, (lo, hi, sub, div)))
        if (sub, div) == (0.0, 1.0):                                                # the clip alone is a copy or a bound
            assert np.array_equal(buf.cpu().numpy(), np.clip(x, np.float32(lo), np.float32(hi)))
    if count == 1:
        assert lib.vs_data_clip_center(buf.data_ptr(), 1, 1.0, 0.0, 0.0, 1.0, _stream()) == EINVAL          # lo > hi
        assert lib.vs_data_clip_center(buf.data_ptr(), 1, 0.0, 1.0, 0.0, 0.0, _stream()) == EINVAL          # divisor 0
        assert lib.vs_data_clip_center(buf.data_ptr(), 0, 0.0, 1.0, 0.0, 1.0, _stream()) == EINVAL


# ---- crop_pad ------------------------------------------------------------------------------------------------------------------------------------------
def _crop_pad(vol, dst_shape, lo, hi, off):
    lib, check = _lib()
    src = dev(vol)
    out = torch.full(dst_shape, float("nan"), device="cuda")
    check(lib.vs_data_crop_pad(src.data_ptr(), out.data_ptr(), *vol.shape, *dst_shape, _ints(lo), _ints(hi), _ints(off), _stream()), "data_crop_pad")
    return out.cpu().numpy()


def test_crop_pad():
    from vae_segmentation_amd import data_gpu as D
    vol = U.noise((7, 20, 21), 6) + 1000.0                                          # no zeros in the source: padding is recognisable
    # a box clipped on both sides of axis 0, 5 rows missing there: int(5 / 2) = 2 zero rows before, 3 after; with and without a shift
    for centre, L, pad, shift in (((3, 10, 10), 10, 1, 0), ((3, 4, 17), 9, 0, 0), ((3, 10, 10), 10, 1, 2)):
        want, lo, hi, off = U.ref_crop_pad_cube(vol, centre, L, pad, shift)
        got = D.crop_pad_cube(dev(vol), centre, L, pad, shift).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (centre, L, pad, shift)
        assert np.array_equal(_crop_pad(vol, want.shape, lo, hi, off), want)
    want, lo, hi, off = U.ref_crop_pad_cube(vol, (3, 10, 10), 10, 1)
    assert (lo[0], hi[0], off[0]) == (0, 7, 2) and not want[:2].any() and not want[9:].any() and (want[2:9, 1:11, 1:11] != 0).all()
    # lo == hi on one axis: an all-zero cube
    assert not _crop_pad(vol, (4, 5, 6), (1, 2, 3), (3, 2, 5), (0, 0, 0)).any()
    # a destination that is not a cube, offsets that push part of the box out of it, and unit extents
    for dst, lo, hi, off in (((3, 30, 5), (2, 0, 4), (7, 20, 21), (1, 7, 0)), ((1, 1, 1), (6, 19, 20), (7, 20, 21), (0, 0, 0)), ((9, 2, 40), (0, 5, 0), (1, 6, 21), (8, 1, 19))):
        assert np.array_equal(_crop_pad(vol, dst, lo, hi, off), U.ref_crop_pad(vol, dst, lo, hi, off)), (dst, lo, hi, off)
    lib, _ = _lib()
    src, out = dev(vol), torch.zeros(4, 4, 4, device="cuda")

    def call(s=vol.shape, d=(4, 4, 4), lo=(0, 0, 0), hi=(4, 4, 4), off=(0, 0, 0), dst=out.data_ptr()):
        return lib.vs_data_crop_pad(src.data_ptr(), dst, *s, *d, _ints(lo), _ints(hi), _ints(off), _stream())

    assert call() == 0
    assert call(lo=(-1, 0, 0)) == ESHAPE and call(hi=(8, 4, 4)) == ESHAPE and call(lo=(5, 0, 0)) == ESHAPE and call(off=(0, -1, 0)) == ESHAPE
    assert call(d=(4, 0, 4)) == EINVAL and call(s=(7, 20, 0)) == EINVAL and call(dst=None) == EINVAL
    torch.cuda.synchronize()
