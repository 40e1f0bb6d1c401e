"""CPU: tests/data_util.py — the oracle of tests/test_gpu_data_kernels.py — is pinned, and the conditions the GPU cases rely on are asserted from the
oracle alone: the zoom's coordinate rule against scipy for every pair of lengths, who owns a coordinate on the border, axes of length 1 and 2, the
tie pairs inside the zoom cases and the cap on the voxels the general affine cases leave out."""
import numpy as np
import pytest
from scipy import ndimage as ndi

from oracle import data_cpu as O
from tests import data_util as U


# ---- the zoom's coordinate rule --------------------------------------------------------------------------------------------------------------------
def test_division_first_coordinate_reproduces_scipys_order0_picks_for_all_length_pairs():
    """x = arange(m), mode="mirror", every (m, n) in 1..160: floor(c + 0.5) mirrored with c = (o + 0.5) (m / n) - 0.5 is scipy's pick everywhere; the
    product-first form ((o + 0.5) m) / n - 0.5 picks another voxel in 410 of the 25,600 pairs, the five smallest and three a run can meet among them"""
    wrong_division, wrong_product = [], set()
    for m in range(1, 161):
        for n in range(1, 161):
            want = U.scipy_pick0(m, n)
            if not np.array_equal(U.zoom_pick0(m, n, "division"), want):
                wrong_division.append((m, n))
            if not np.array_equal(U.zoom_pick0(m, n, "product"), want):
                wrong_product.add((m, n))
    print("pairs wrong: division first %d, product first %d" % (len(wrong_division), len(wrong_product)))
    assert wrong_division == []
    assert len(wrong_product) == 410
    assert set(U.TIE_PAIRS_SMALL) | set(U.TIE_PAIRS_RUN[:1]) <= wrong_product          # 224 -> 80 and 272 -> 56: the parametrised test below


@pytest.mark.parametrize("m,n,count", [(30, 11, 1), (30, 13, 1), (26, 23, 1), (18, 33, 1), (36, 33, 1), (112, 40, 1), (224, 80, 2), (272, 56, 5)])
def test_the_tie_pairs_of_the_gpu_cases(m, n, count):
    """each is an exact tie in exact arithmetic, on which the two forms of the coordinate fall on different sides: `count` output indices differ"""
    want = U.scipy_pick0(m, n)
    assert np.array_equal(U.zoom_pick0(m, n), want)
    assert int((U.zoom_pick0(m, n, "product") != want).sum()) == count
    assert any((2 * o + 1) * m % (2 * n) == 0 for o in range(n))         # (o + 0.5) m / n is an integer for some o
    assert U.zoom_tie_distance(m, n) < 1e-14


def test_zoom_cases_contain_the_ties_and_every_path():
    pairs = {(m, n) for src, dst in U.ZOOM_TIE_CASES for m, n in zip(src, dst)}
    assert set(U.TIE_PAIRS_SMALL) | {(112, 40), (272, 56)} <= pairs
    for src, dst in U.ZOOM_TIE_CASES:
        x = U.ramp(src)
        want = U.ref_zoom(x, dst, 0)
        rule = x[np.ix_(*[U.zoom_pick0(m, n) for m, n in zip(src, dst)])]
        old = x[np.ix_(*[U.zoom_pick0(m, n, "product") for m, n in zip(src, dst)])]
        assert np.array_equal(want, rule) and not np.array_equal(want, old)          # a wrong index on an axis is a whole plane
        assert float((old != want).mean()) > 1.0 / max(dst)
    assert [s for s in U.ZOOM_CASES[3][0]].count(1) == 2 and U.ZOOM_CASES[2][1][1] == 1          # unit axes in and out
    src, dst = U.ZOOM_SWEEP_CASE
    assert int(np.prod(dst)) > U.SWEEP and U.COUNTS[-1] > U.SWEEP and U.COUNTS[1] == 4097
    # order 1 is continuous in the coordinate, so the last bit of the rule cannot show there: the two forms agree far inside the bound
    x = U.noise(U.ZOOM_CASES[0][0], 3)
    want = U.ref_zoom(x, U.ZOOM_CASES[0][1], 1)
    c = [U.zoom_coord(m, n, "product") for m, n in zip(*U.ZOOM_CASES[0])]
    other = ndi.map_coordinates(x.astype(np.float64), np.array(np.meshgrid(*c, indexing="ij")), order=1, mode="mirror")
    assert np.abs(other - want).max() < 1e-3 * U.fp32_bound(want)


# ---- the affine sampler ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 3])
def test_a_coordinate_on_the_border_is_inside(order):
    x = U.affine_input((6, 7, 9), order, 1)
    centre = tuple((s - 1) / 2.0 for s in x.shape)
    coords = U.affine_coords(x.shape, (0.0, 0.0, 0.0), 1.0, centre)
    assert np.array_equal(coords, np.indices(x.shape).astype(np.float64))            # exact: 0 and n - 1 themselves
    got, dist = U.ref_affine(x, coords, order, -7.0)
    assert not (got == -7.0).any() and np.abs(got - x).max() <= (0.0 if order == 0 else 1e-9)
    border = np.zeros(x.shape, bool)
    border[[0, -1]] = border[:, [0, -1]] = border[:, :, [0, -1]] = True
    assert np.array_equal(dist == 0.0, border) and dist[~border].min() == (0.5 if order == 0 else 1.0)
    # one bit outside is outside
    for axis in range(3):
        for edge, step in ((0.0, -2.0 ** -60), (x.shape[axis] - 1.0, 2.0 ** -48)):
            c = coords.copy()
            c[axis][c[axis] == edge] = edge + step
            out, d = U.ref_affine(x, c, order, -7.0)
            moved = coords[axis] == edge
            assert np.array_equal(out == -7.0, moved) and 0 < d[moved].max() <= U.NEAR


def test_exact_affine_cases_are_exact_and_reach_both_sides_of_the_border():
    names = [c[0] for c in U.AFFINE_EXACT_CASES]
    assert names == ["identity", "shift+2", "shift-2", "scale0.5", "scale2", "patch-smaller", "patch-larger", "unit-axis"]
    for name, shape, patch, angles, scale, centre in U.AFFINE_EXACT_CASES:
        coords = U.affine_coords(patch, angles, scale, centre)
        assert np.array_equal(coords * 4.0, np.round(coords * 4.0)) and np.abs(coords).max() < 64, name      # multiples of 1/4: no rounding anywhere
        for order in (0, 3):
            x = U.affine_input(shape, order, 5)
            got, dist = U.ref_affine(x, coords, order, U.AFFINE_CVAL[order])
            outside = np.zeros(patch, bool)
            for a in range(3):
                outside |= (coords[a] < 0) | (coords[a] > shape[a] - 1)
            assert np.array_equal(got[outside], np.full(int(outside.sum()), U.AFFINE_CVAL[order])), name
            if order == 0:
                assert (got[~outside] >= 1).all(), name
            assert outside.any() == (name not in ("identity", "scale0.5", "patch-smaller")), name
            assert (~outside).any(), name
            if name in ("identity", "shift+2", "shift-2", "unit-axis"):
                assert (dist == 0.0).any(), name                           # voxels exactly on the border: inside, and compared
    # scale 0.5 puts order-0 coordinates on exact .5 ties (taken upwards by floor(c + 0.5)); both implementations see the same exact number
    coords = U.affine_coords(*U.AFFINE_EXACT_CASES[3][2:])
    assert (np.abs(coords[1] - np.floor(coords[1]) - 0.5) == 0).any()


@pytest.mark.parametrize("seed", U.AFFINE_GENERAL_SEEDS)
def test_general_affine_cases_leave_out_at_most_eight_voxels(seed):
    angles, scale, centre = U.affine_general_params(seed)
    assert all(abs(a) <= 0.2 for a in angles) and 0.85 <= scale <= 1.15 and any(a != 0 for a in angles)
    coords = U.affine_coords(U.AFFINE_GENERAL_PATCH, angles, scale, centre)
    for order in (0, 3):
        x = U.affine_input(U.AFFINE_GENERAL_SHAPE, order, seed)
        got, dist = U.ref_affine(x, coords, order, U.AFFINE_CVAL[order])
        left_out = int((dist <= U.NEAR).sum())
        outside = int((got == U.AFFINE_CVAL[order]).sum()) if order == 0 else None
        print("seed", seed, "order", order, "left out", left_out, "smallest distance %.3g" % dist.min(), "outside", outside)
        assert left_out <= U.NEAR_CAP
        if order == 0:
            assert 0 < outside < got.size // 2                             # the border is crossed, and most of the patch is inside


# ---- axes of length 1 and 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 1), (2, 1, 2), (2, 2, 2), (1, 4, 33)])
def test_every_oracle_function_accepts_short_axes(shape):
    x = U.noise(shape, 2)
    lab = (np.arange(x.size).reshape(shape) % 3).astype(np.float32)
    box = U.ref_bbox(lab)
    assert (box is None) == (x.size == 1) and U.ref_bbox(np.ones(shape, np.float32))[1].tolist() == [s - 1 for s in shape]
    assert np.array_equal(U.ref_relabel(lab, [1.0, 2.0], [2.0, 5.0]), np.where(lab == 1, 2, np.where(lab == 2, 5, 0)))
    assert np.array_equal(U.ref_crop_pad(x, shape, (0, 0, 0), shape, (0, 0, 0)), x)
    assert np.array_equal(U.ref_clip_center(x, -3e38, 3e38, 0.0, 1.0), x.astype(np.float64))
    assert U.ref_minmax(x) == (float(x.min()), float(x.max()))
    for axis in range(3):
        g = U.ref_gaussian_axis(x, 3.0, axis)                              # radius 12: the mirror wraps several times
        assert g.shape == shape and np.isfinite(g).all()
        if shape[axis] == 1:
            assert np.array_equal(g.astype(np.float32), x)
        assert float(x.min()) - 1e-9 <= g.min() and g.max() <= float(x.max()) + 1e-9      # positive weights summing to one
    coef = U.ref_spline3(x)
    assert coef.shape == shape and coef.dtype == np.float64
    if max(shape) == 1:
        assert np.array_equal(coef, x.astype(np.float64))
    for order in (0, 1):
        for out in ((3, 2, 5), (1, 1, 1)):
            z = U.ref_zoom(x, out, order)
            assert z.shape == out and float(x.min()) - 1e-9 <= z.min() and z.max() <= float(x.max()) + 1e-9
    coords = U.affine_coords(shape, (0.0, 0.0, 0.0), 1.0, tuple((s - 1) / 2.0 for s in shape))
    for order in (0, 3):
        got, dist = U.ref_affine(x, coords, order, -7.0)
        assert np.abs(got - x).max() <= (0.0 if order == 0 else 1e-9) and dist.min() == 0.0


# ---- the remaining functions against independent statements --------------------------------------------------------------------------------------------
def test_plain_numpy_functions_against_the_pipeline_oracle():
    rng = np.random.RandomState(4)
    lab = rng.randint(0, 5, size=(9, 10, 11)).astype(np.float32)
    # later pairs win, and every pair reads the input: O.load_merge assigns in the same order
    merge = np.stack([lab, lab], -1)
    assert np.array_equal(U.ref_relabel(lab, [1, 3, 2], [1, 1, 2]), O.load_merge(merge, [[[1, 3], 1], [2, 2]])[1])
    assert np.array_equal(U.ref_relabel(lab, *U.PAIRS_CHAINED), np.where(lab == 1, 2, np.where(lab == 2, 3, 0)))
    assert np.array_equal(U.ref_relabel(lab, [1, 1], [4, 7]), np.where(lab == 1, 7, 0))
    nan = lab.copy(); nan[0, 0, 0] = np.nan
    assert U.ref_relabel(nan, [1.0], [1.0])[0, 0, 0] == 0 and len(U.PAIRS_16[0]) == 16
    # bbox: NaN and negative labels are not foreground
    odd = -np.ones((4, 5, 6), np.float32); odd[1, 2, 3] = np.nan
    assert U.ref_bbox(odd) is None
    odd[3, 0, 5] = 0.5
    assert [v.tolist() for v in U.ref_bbox(odd)] == [[3, 0, 5], [3, 0, 5]]
    # crop + pad: the index form against the reference's slice + np.pad, clipped on both sides of an axis and with an odd missing width
    vol = U.noise((7, 20, 21), 6)
    for centre, L, pad, shift in (((3, 10, 10), 10, 1, 0), ((3, 4, 17), 9, 0, 0), ((3, 10, 10), 10, 1, 2)):
        cube, lo, hi, off = U.ref_crop_pad_cube(vol, centre, L, pad, shift)
        assert np.array_equal(cube, O.crop_pad_cube(vol, centre, L, pad, shift))
        assert np.array_equal(U.ref_crop_pad(vol, cube.shape, lo, hi, off), cube)
    cube, lo, hi, off = U.ref_crop_pad_cube(vol, (3, 10, 10), 10, 1)
    assert lo[0] == 0 and hi[0] == 7 and (12 - 7) % 2 == 1 and off[0] == 2              # both sides clipped; 5 missing rows: 2 before, 3 after
    assert not U.ref_crop_pad(vol, (4, 4, 4), (1, 2, 3), (3, 2, 5), (0, 0, 0)).any()     # lo == hi on an axis: nothing is copied
    # clip + centre on the fp32 arguments
    assert np.array_equal(U.ref_clip_center(np.float32([-500, 100, 900]), -200, 400, 100, 300), np.float64([-1.0, 0.0, 1.0]))
    # minmax skips NaN; signed zeros compare equal
    assert U.ref_minmax(np.float32([np.nan, -3, 2])) == (-3.0, 2.0) and U.ref_minmax(np.float32([0.0, -0.0])) == (0.0, 0.0)


def test_scipy_functions_against_independent_statements():
    x = U.noise((5, 7, 9), 8)
    # the three axis passes are scipy's gaussian_filter, which skimage's anti-aliasing calls (dyadic sigmas: float32 changes nothing)
    y = x.astype(np.float64)
    for axis, s in enumerate((0.25, 1.5, 3.0)):
        y = U.ref_gaussian_axis(y, s, axis)
    assert np.abs(y - ndi.gaussian_filter(x.astype(np.float64), (0.25, 1.5, 3.0), mode="mirror")).max() <= 1e-10
    # the radius the kernel forms in fp32, (int)(4.0f sigma + 0.5f), is scipy's int(4 sigma + 0.5) for every sigma of the GPU cases
    assert len(U.GAUSS_SIGMAS) == len(set(U.GAUSS_SIGMAS)) == 6 and U.resize_sigma(150, 64) == 0.671875 and U.resize_sigma(9, 4) == 0.625
    for s in U.GAUSS_SIGMAS:
        s32 = np.float32(s)
        assert int(np.float32(4.0) * s32 + np.float32(0.5)) == int(4.0 * float(s32) + 0.5), s
    assert int(4.0 * 3.0 + 0.5) == 12 > max(max(s) for s in U.GAUSS_SHAPES[:1])          # longer than every axis of (5, 7, 9)
    # the mirror-started coefficients are the ones map_coordinates(mode="constant") makes for itself
    coords = U.affine_coords((4, 5, 6), (0.1, -0.2, 0.15), 0.9, (2.0, 3.0, 4.0))
    a = ndi.map_coordinates(U.ref_spline3(x), coords, order=3, mode="constant", cval=-1.0, prefilter=False)
    assert np.abs(a - U.ref_affine(x, coords, 3, -1.0)[0]).max() <= 1e-9
    assert sorted({n for s in U.SPLINE_SHAPES for n in s}) == [1, 2, 3, 4, 65]
    # zoom is what skimage's resize runs (oracle.data_cpu.skimage_resize without the anti-aliasing filter), clip included
    for order in (0, 1):
        want = O.skimage_resize(x, (3, 11, 4), order=order, anti_aliasing=False)
        got = U.ref_zoom(x, (3, 11, 4), order, clip=(x.min(), x.max()))
        assert np.array_equal(got.astype(np.float32), want)
    narrow = U.ref_zoom(x, (3, 11, 4), 1, clip=(0.0, 100.0))
    assert narrow.min() == 0.0 and narrow.max() == 100.0
    # the index mirror
    assert U.mirror(np.arange(-7, 8), 4).tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1] and U.mirror([-5, 0, 9], 1).tolist() == [0, 0, 0]
