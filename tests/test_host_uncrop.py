"""Host: the geometry and the restatement behind ops.uncrop (tests/uncrop_util.py) against oracle/data_cpu.py, the refusals of CPU tensors and the
entry points' flag check.  No GPU is touched."""
import numpy as np
import pytest
import torch

from oracle import data_cpu as O
from tests import uncrop_util as U


def _label_with_box(shape, bmin, bmax):
    lab = np.zeros(shape, np.float32)
    lab[tuple(bmin)] = 1                                          # two corners span the box
    lab[tuple(bmax)] = 1
    return lab


# interior, clipped at one face (off > 0 on one side only), clipped on two axes, odd L, even L; each with shift 0 and 3
BOXES = [((8, 9, 12), (14, 17, 22)), ((0, 10, 15), (9, 19, 26)), ((2, 5, 4), (20, 25, 35)), ((5, 6, 7), (12, 17, 20)), ((3, 8, 12), (17, 20, 25)),
         ((12, 20, 30), (22, 29, 40))]


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("box", BOXES, ids=lambda b: "%s-%s" % b)
def test_geometry_is_what_the_oracle_crop_implies(box, shift):
    from vae_segmentation_amd import data_gpu
    shape = (23, 30, 41)
    vol = np.random.RandomState(sum(box[0])).randn(*shape).astype(np.float32) + 5.0          # no zeros: padding is recognisable
    lab = _label_with_box(shape, *box)
    centre, L, pad = O.crop_box(lab)
    cube = O.crop_pad_cube(vol, centre, L, pad, shift)
    bmin, bmax = U.box_of(lab)
    assert tuple(bmin) == box[0] and tuple(bmax) == box[1]
    lo, hi, off, side = U.crop_geometry((bmin, bmax), shape, shift)
    got = data_gpu.crop_geometry((bmin, bmax), shape, shift)
    assert (list(got[0]), list(got[1]), list(got[2]), got[3]) == (lo, hi, off, side)
    assert all(isinstance(v, int) for t in got[:3] for v in t) and isinstance(got[3], int)
    assert cube.shape == (side,) * 3 and side == L + 2 * pad
    src = tuple(slice(off[d], off[d] + hi[d] - lo[d]) for d in range(3))
    dst = tuple(slice(lo[d], hi[d]) for d in range(3))
    pasted = np.zeros(shape, np.float32)
    pasted[dst] = cube[src]
    assert np.array_equal(pasted[dst], vol[dst])
    rest = cube.copy()
    rest[src] = 0
    assert not rest.any()                                         # everything else in the cube is padding


def test_geometry_cases_cover_what_they_claim():
    geo = {c[0]: U.case_geometry(c) for c in U.KERNEL_CASES}
    assert [geo[n][3] for n in ("side11-direct", "side8-up", "side12-up", "side16-identity", "side37-down-clipped", "side13-one-face")] == [11, 8, 12, 16, 37, 13]
    lo, hi, off, side = geo["side37-down-clipped"]
    assert lo[:2] == [0, 0] and hi[:2] == [23, 30] and off[0] > 0 and off[1] > 0 and side > 23
    lo, hi, off, side = geo["side13-one-face"]
    assert lo[0] == 0 and off == [1, 0, 0] and hi[1] < 30 and hi[2] < 41 and lo[1] > 0 and lo[2] > 0
    assert {s for L in range(0, 40) for s in [L + 2 * int(0.1 * L)]}.isdisjoint({10, 11})          # why side 11 comes without a box
    for case in U.KERNEL_CASES:
        lo, hi, off, side = U.case_geometry(case)
        for d in range(3):
            assert 0 <= lo[d] < hi[d] <= case[1][d] and off[d] >= 0 and off[d] + hi[d] - lo[d] <= side


@pytest.mark.parametrize("side,patch", [(8, 16), (11, 16), (12, 16), (13, 16), (16, 16), (27, 32), (32, 32), (1, 16)])
def test_nearest_round_trip_is_the_identity_when_the_cube_is_not_larger_than_the_patch(side, patch):
    cube = np.random.RandomState(side).randint(0, 4, size=(side,) * 3).astype(np.float32)
    patch_label = O.skimage_resize(cube, (patch,) * 3, order=0, anti_aliasing=False)
    assert np.array_equal(U.zoom_nearest(patch_label, side), cube)


@pytest.mark.parametrize("side", [8, 11, 16, 37])
def test_scipy_zoom_is_the_clamped_two_point_rule(side):
    p = U.softmax_like(2, 16, side)[1]
    assert np.abs(U.zoom_linear(p, side) - U.zoom_linear_explicit(p, side)).max() <= 1e-13
    if side == 16:
        assert np.abs(U.zoom_linear(p, side) - p).max() <= 1e-13


def test_restatement_leaves_few_voxels_undecided_and_pastes_background():
    """the share of cube voxels whose two largest classes lie within 1e-5 of each other — the ones the GPU test leaves out of the label comparison —
    stays under 0.1 % for the committed seeds"""
    for case in U.KERNEL_CASES:
        name, shape, patch, _, _ = case
        geometry = U.case_geometry(case)
        for k in U.KERNEL_KS:
            want = U.uncrop(U.softmax_like(k, patch, U.case_seed(case, k)), geometry, shape, "linear")
            close = (U.top_two_margin(want["prob"]) <= 1e-5) & want["inside"]
            share = close.sum() / want["inside"].sum()
            assert share <= 1e-3, (name, k, share)
            out = ~want["inside"]
            assert (want["label"][out] == 0).all() and (want["prob"][0][out] == 1).all() and (want["prob"][1:][:, out] == 0).all()
            assert np.abs(want["prob"].sum(0) - 1).max() <= 1e-6
            near = U.uncrop(U.softmax_like(k, patch, U.case_seed(case, k)), geometry, shape, "nearest")
            assert (near["label"][out] == 0).all()


def test_tie_goes_to_the_first_channel_in_the_restatement():
    p = np.full((3, 16, 16, 16), 1.0 / 3, np.float32)
    assert not U.uncrop(p, ([0] * 3, [16] * 3, [0] * 3, 16), (16, 16, 16))["label"].any()


def test_cpu_tensors_are_refused():
    from vae_segmentation_amd import evaluation, ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.uncrop(torch.zeros(2, 16, 16, 16), ([0] * 3, [16] * 3, [0] * 3, 16), (16, 16, 16))
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluation.coarse_to_fine_predict(None, torch.zeros(32, 32, 32), 32)


def test_entry_point_flags():
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    for mod, script, side in ((main_source, "main_source.py", "source"), (main_target, "main_target.py", "target")):
        a = mod.parse(["run", "-M", "seg_train"])
        assert a.val_fine_whole is False and a.save_whole_pred is None and a.fine_interp == "linear"
        driver.check_fine_whole_flags(a, script)                                 # off: nothing to check
        a = mod.parse(["run", "-M", "seg_train", "--real_data", "--val_whole_volume", "--val_fine_whole", "--save_whole_pred", "out", "--fine_interp", "nearest"])
        assert a.val_fine_whole and a.save_whole_pred == "out" and a.fine_interp == "nearest"
        driver.check_fine_whole_flags(a, script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_whole_volume" % script):       # run() refuses before it touches a device
            driver.run(mod.parse(["run", "-M", "seg_train", "--real_data", "--val_fine_whole"]), side=side)
        with pytest.raises(SystemExit, match="inconsistent flags.*--val_fine_whole"):
            driver.run(mod.parse(["run", "-M", "seg_train", "--real_data", "--val_whole_volume", "--save_whole_pred", "out"]), side=side)
        with pytest.raises(SystemExit):
            mod.parse(["run", "--fine_interp", "cubic"])
