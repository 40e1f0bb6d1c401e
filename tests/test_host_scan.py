"""CPU: the host arithmetic of scan geometry (data_gpu.ScanGeometry, data_gpu.cube_slices) against known answers, and the properties of the numpy / scipy
restatement (tests/scan_util.py) that tests/test_gpu_scan.py relies on: the oracle's zoom returns the requested shapes, the forward order-0 resize of the
first two kernel cases has no tie and that of the third turns on an exact one, and the label rule of the linear inverse leaves at most 1 % of the voxels out."""
import numpy as np
import pytest

from tests import scan_util as S


def test_negative_in_plane_spacing_is_a_plain_transpose():
    """spacing (-1, -1, 1): ind = (+1, +1, -1), so the two in-plane axes are only transposed and the through-plane axis is reversed"""
    from vae_segmentation_amd import data_gpu
    g = data_gpu.ScanGeometry((4, 5, 6), (-1.0, -1.0, 1.0))
    assert g.raw_shape == (4, 5, 6) and g.oriented_shape == (5, 4, 6) and g.shape_1mm == (5, 4, 6)
    assert g.flips == (False, False, True) and g.spacing == (-1.0, -1.0, 1.0)
    assert g.as_tuple() == (4, 5, 6, 0, 0, 1, 5, 4, 6) and all(type(v) is int for v in g.as_tuple())
    raw = np.arange(4 * 5 * 6).reshape(4, 5, 6)
    assert np.array_equal(S.orient(raw, g.spacing), np.transpose(raw, [1, 0, 2])[:, :, ::-1])
    # a whole affine is accepted in place of its diagonal
    assert data_gpu.ScanGeometry((4, 5, 6), np.diag([-1.0, -1.0, 1.0, 1.0])).as_tuple() == g.as_tuple()


def test_shape_times_spacing_quirk_is_kept():
    """The reference multiplies the TRANSPOSED shape (Y, X, Z) by the UNTRANSPOSED spacing (sx, sy, sz).  With raw (10, 20, 5) at (0.5, 2.0, 1.0) that is
    (20 * 0.5, 10 * 2.0, 5) = (10, 20, 5); pairing each axis with its own spacing would give (20 * 2.0, 10 * 0.5, 5) = (40, 5, 5)."""
    from vae_segmentation_amd import data_gpu
    g = data_gpu.ScanGeometry((10, 20, 5), (0.5, 2.0, 1.0))
    assert g.oriented_shape == (20, 10, 5) and g.shape_1mm == (10, 20, 5) and g.shape_1mm != (40, 5, 5)
    assert g.flips == (True, True, True)
    # the issue's first kernel case, and truncation (not rounding) of the product
    g = data_gpu.ScanGeometry((12, 9, 7), (0.8, -0.7, 2.5))
    assert g.oriented_shape == (9, 12, 7) and g.shape_1mm == (7, 8, 17) and g.flips == (False, True, True)
    assert data_gpu.ScanGeometry((9, 6, 15), (1.7, 1.4, 0.7)).shape_1mm == (10, 12, 10)
    for bad in ((0.8, 0.0, 1.0), (0.8, float("nan"), 1.0), (0.8, 0.7), (0.01, 0.01, 0.01)):
        with pytest.raises(ValueError, match="ScanGeometry"):
            data_gpu.ScanGeometry((12, 9, 7), bad)
    with pytest.raises(ValueError, match="ScanGeometry"):
        data_gpu.ScanGeometry((12, 9), (1.0, 1.0, 1.0))


@pytest.mark.parametrize("signs", S.SIGNS, ids=lambda s: "".join("+" if v > 0 else "-" for v in s))
def test_all_sign_combinations_against_explicit_slicing(signs):
    from vae_segmentation_amd import data_gpu
    shape, spacing = (4, 5, 3), S.signed((0.8, 0.7, 2.5), signs)
    g = data_gpu.ScanGeometry(shape, spacing)
    raw = np.arange(np.prod(shape)).reshape(shape)
    want = np.transpose(raw, [1, 0, 2])
    if spacing[1] > 0:                       # ind[1] = -1 reverses the first oriented axis (raw Y)
        want = want[::-1]
    if spacing[0] > 0:
        want = want[:, ::-1]
    if spacing[2] > 0:
        want = want[:, :, ::-1]
    assert g.flips == (spacing[1] > 0, spacing[0] > 0, spacing[2] > 0)
    assert np.array_equal(S.orient(raw, spacing), want)
    # the flips in the form the kernels read them: oriented[o0][o1][o2] = raw[g1(o1)][g0(o0)][g2(o2)]
    x, y, z, f0, f1, f2 = g.as_tuple()[:6]
    o = np.indices(g.oriented_shape)
    pick = raw[np.where(f1, x - 1 - o[1], o[1]), np.where(f0, y - 1 - o[0], o[0]), np.where(f2, z - 1 - o[2], o[2])]
    assert np.array_equal(pick, want)
    assert np.array_equal(S.unorient(want, spacing), raw)
    ref = S.geometry(shape, spacing)
    assert (g.oriented_shape, g.flips, g.shape_1mm) == (ref["oriented_shape"], ref["flips"], ref["shape_1mm"])


def test_cube_slices_against_hand_computed_answers():
    from vae_segmentation_amd import data_gpu
    # interior: box [10, 14] x [20, 30] x [15, 18], pad 3 -> bbox (7, 17), (17, 33), (12, 21); center (12, 25, 16); L = 16; rows c - 8 .. c + 8
    got = data_gpu.cube_slices(((10, 20, 15), (14, 30, 18)), (40, 50, 45), pad=3)
    assert got == (slice(4, 20), slice(17, 33), slice(8, 24))
    # clipped at the z = 0 face and at the far x face: bbox (0, 9), (5, 17), (22, 30); center (4, 11, 26); L = 12 -> (0, 10), (5, 17), (20, 30)
    got = data_gpu.cube_slices(((1, 10, 27), (4, 12, 29)), (20, 25, 30), pad=5)
    assert got == (slice(0, 10), slice(5, 17), slice(20, 30))
    # the default pad is the reference's 32: a small volume is taken whole along every axis the padded box covers
    got = data_gpu.cube_slices(((5, 5, 5), (6, 6, 6)), (12, 11, 10))
    assert got == (slice(0, 12), slice(0, 11), slice(0, 10))
    # and the restatement agrees on a label (also with an odd extent, where int(L / 2) matters)
    for box, shape, pad in ((((10, 20, 15), (14, 30, 18)), (40, 50, 45), 3), (((1, 10, 27), (4, 12, 29)), (20, 25, 30), 5), (((3, 2, 6), (9, 7, 8)), (14, 9, 16), 2)):
        label = np.zeros(shape)
        label[box[0]] = label[box[1]] = 1
        assert data_gpu.cube_slices(box, shape, pad) == S.foreground_cube(label, pad), (box, shape, pad)


@pytest.mark.parametrize("case", S.TIE_FREE_CASES, ids=lambda c: c[0])
def test_kernel_cases_have_exact_shapes_and_no_forward_tie(case):
    """the order-0 forward resize turns on floor(q + 0.5): in these cases no q + 0.5 comes within 1e-6 of an integer"""
    name, shape, spacing = case
    g = S.geometry(shape, spacing)
    dist = S.forward_tie_distance(shape, spacing)
    print(name, "oriented", g["oriented_shape"], "1 mm", g["shape_1mm"], "tie distance %.4g" % dist)
    assert dist > 1e-6, (name, dist)
    raw, label = S.smooth_scan(shape, 1)
    pre = S.preprocess(raw, spacing, label)
    assert pre["image"].shape == g["shape_1mm"] and pre["label"].shape == g["shape_1mm"]
    assert set(np.unique(pre["label"])) <= {0.0, 1.0, 2.0} and pre["label"].max() > 0
    assert raw.min() <= pre["image"].min() and pre["image"].max() <= raw.max()             # skimage's clip=True
    up = [o < n for o, n in zip(g["oriented_shape"], g["shape_1mm"])]
    assert up == ([False, False, True] if name == "down-in-plane" else [True, True, False])


@pytest.mark.parametrize("case", S.TIE_CASES, ids=lambda c: c[0])
def test_tie_case_has_exact_shapes_and_an_exact_forward_tie(case):
    """the case the kernels may not step around: its tie distance is 0, the oracle (scipy) resolves the tie by the division-first coordinate, and the
    product-first one would move a whole plane of the label"""
    from tests import data_util as U
    name, shape, spacing = case
    g = S.geometry(shape, spacing)
    assert g["oriented_shape"] == (8, 6, 30) and g["shape_1mm"] == (11, 7, 11)
    assert S.forward_tie_distance(shape, spacing) == 0.0
    assert S.tie_distance(30, 11) == 0.0 and S.tie_distance(8, 11) == 0.0 and S.tie_distance(6, 7) == 0.0       # every axis: an odd output length
    assert S.KERNEL_CASES == S.TIE_FREE_CASES + S.TIE_CASES and case in S.KERNEL_CASES and case not in S.NATIVE_CASES
    raw, label = S.smooth_scan(shape, 1)
    pre = S.preprocess(raw, spacing, label)
    assert pre["image"].shape == g["shape_1mm"] and pre["label"].shape == g["shape_1mm"]
    assert set(np.unique(pre["label"])) == {0.0, 1.0, 2.0}
    # the smooth blob is mirror-symmetric about the tied plane, so the noisy scan itself goes through the label path as well (tests/test_gpu_scan.py does the same)
    for name_, vol in (("label", label), ("scan as label", raw)):
        want = S.preprocess(raw, spacing, vol)["label"]
        oriented = S.orient(vol, spacing).astype(np.float64)
        picks = {rule: oriented[np.ix_(*[U.zoom_pick0(m, n, rule) for m, n in zip(g["oriented_shape"], g["shape_1mm"])])] for rule in ("division", "product")}
        assert np.array_equal(picks["division"], want)
        differing = int((picks["product"] != want).sum())
        print(name, name_, "voxels the product-first coordinate would get wrong: %d of %d" % (differing, want.size))
    assert differing >= want.size // 11                                     # a whole plane of the 1 mm grid


def test_the_issues_rejected_candidates_do_have_ties():
    for shape, spacing in (((10, 13, 6), (0.75, 0.75, 3.0)), ((16, 11, 8), (0.6, 0.9, 1.5)), ((8, 8, 12), (1.3, 1.3, 0.7))):
        assert S.forward_tie_distance(shape, spacing) <= 1e-6, (shape, spacing)
    assert abs(S.forward_tie_distance((12, 9, 7), (0.8, 0.7, 2.5)) - 0.0294) < 1e-3


@pytest.mark.parametrize("case", S.NATIVE_CASES, ids=lambda c: c[0])
def test_inverse_restatement(case):
    """shapes of the inverse zoom, the explicit border rule against scipy's mirror mode, and the cap of the label rule on the oracle alone"""
    name, shape, spacing = case
    spacing = S.case_spacing(case, S.NATIVE_CASES)
    g = S.geometry(shape, spacing)
    n1, no = g["shape_1mm"], g["oriented_shape"]
    for k in S.KERNEL_KS:
        prob = S.native_input(case, k)[1]
        assert prob.shape == (k,) + n1 and np.allclose(prob.sum(0), 1.0, atol=1e-6)
        want = S.to_native(prob, shape, spacing, "linear")
        assert want["prob"].shape == (k,) + tuple(shape) and want["label"].shape == tuple(shape)
        undecided = float((S.top_two_margin(want["prob"]) <= 1e-4).mean())
        print(name, "K", k, "undecided share %.3g" % undecided)
        assert undecided <= 0.01, (name, k, undecided)
        # what the header states: q mirrored at the borders, the two neighbours per axis weighted by the fraction
        out = prob[0].astype(np.float64)
        for axis in range(3):
            q = S.coordinate(no[axis], n1[axis])
            top = n1[axis] - 1.0
            q = np.clip(np.where(q < 0, -q, np.where(q > top, 2 * top - q, q)), 0.0, top)
            i0 = np.floor(q).astype(np.int64)
            i1 = np.minimum(i0 + 1, n1[axis] - 1)
            w = (q - i0).reshape([-1 if a == axis else 1 for a in range(3)])
            out = np.take(out, i0, axis=axis) * (1.0 - w) + np.take(out, i1, axis=axis) * w
        assert np.abs(S.unorient(out, spacing) - want["prob"][0]).max() < 1e-12, (name, k)
        near = S.to_native(prob, shape, spacing, "nearest")
        assert np.isin(near["prob"], prob.astype(np.float64)).all()                          # a copy of samples


@pytest.mark.parametrize("signs", S.SIGNS, ids=lambda s: "".join("+" if v > 0 else "-" for v in s))
def test_unit_spacing_round_trip_of_the_restatement(signs):
    shape = (7, 6, 9)
    label = np.random.RandomState(3).randint(0, 4, size=shape).astype(np.uint8)
    pre = S.preprocess(label.astype(np.int16), signs, label, signs)
    assert pre["shape_1mm"] == (6, 7, 9)
    assert np.array_equal(S.to_native(pre["label"].astype(np.uint8), shape, signs)["label"], label)
