"""GPU: a crop-space prediction pasted back into scan geometry (csrc/uncrop.hip, ops.uncrop, data_gpu.crop_geometry, evaluation.coarse_to_fine_predict,
--val_fine_whole) against the numpy / scipy restatement of tests/uncrop_util.py, whose own checks are in tests/test_host_uncrop.py.

The issue asks for a box that gives side = 11.  CropResize's side is L + 2 int(0.1 L), which skips 10 and 11 (L = 9 -> 9, L = 10 -> 12), so that
case hands an 11-row cube to the kernel as a geometry of its own; boxes with the neighbouring sides 8 and 12 stand beside it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

from tests import uncrop_util as U

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
both_libs = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
cases = pytest.mark.parametrize("case", U.KERNEL_CASES, ids=lambda c: c[0])
_MEMO = {}                      # the restatement of a case, shared by the two library builds


def restated(case, k, interp):
    key = (case[0], k, interp)
    if key not in _MEMO:
        prob = U.softmax_like(k, case[2], U.case_seed(case, k))
        _MEMO[key] = (prob, U.uncrop(prob, U.case_geometry(case), case[1], interp))
    return _MEMO[key]


@both_libs
@cases
def test_linear_against_the_restatement(lib_mode, case):
    """Probabilities within 1e-5 absolute — the bound of the project's interpolating data kernels: fp64 coordinates and sums, one rounding to fp32 (2^-24 ~ 6e-8
    for values in [0, 1]).  Labels equal wherever the restatement's two largest classes differ by more than 1e-5; at most 0.1 % of the cube is left out by
    that rule.  Outside the cube: label 0 and the distribution (1, 0, ...), exactly.  The label is the first-max argmax of the device's own probabilities."""
    from vae_segmentation_amd import ops
    name, shape, patch, _, _ = case
    geometry = U.case_geometry(case)
    for k in U.KERNEL_KS:
        prob, want = restated(case, k, "linear")
        got = ops.uncrop(torch.from_numpy(prob).cuda(), geometry, shape, interp="linear", want_prob=True)
        p, label = got["prob"].cpu().numpy(), got["label"].cpu().numpy()
        assert p.dtype == np.float32 and p.shape == (k,) + tuple(shape) and label.dtype == np.uint8 and label.shape == tuple(shape)
        err = float(np.abs(p.astype(np.float64) - want["prob"]).max())
        inside = want["inside"]
        decided = U.top_two_margin(want["prob"]) > 1e-5
        share = float((inside & ~decided).sum()) / float(inside.sum())
        print(name, "K", k, "max abs err %.3g" % err, "undecided share %.3g" % share, "labels differing %d" % int((label != want["label"]).sum()))
        assert err <= 1e-5, (name, k, err)
        assert share <= 1e-3, (name, k, share)
        assert np.array_equal(label[decided], want["label"][decided]), (name, k)
        assert np.array_equal(label, np.argmax(p, axis=0).astype(np.uint8)), (name, k)
        out = ~inside
        assert out.any() and (label[out] == 0).all() and (p[0][out] == 1.0).all() and (p[1:][:, out] == 0.0).all(), (name, k)
        only_label = ops.uncrop(torch.from_numpy(prob).cuda(), geometry, shape, interp="linear")
        assert sorted(only_label) == ["label"] and torch.equal(only_label["label"], got["label"])


@both_libs
@cases
def test_nearest_against_the_restatement(lib_mode, case):
    """a copy of samples: labels and probabilities equal the restatement exactly"""
    from vae_segmentation_amd import ops
    name, shape, patch, _, _ = case
    geometry = U.case_geometry(case)
    for k in U.KERNEL_KS:
        prob, want = restated(case, k, "nearest")
        got = ops.uncrop(torch.from_numpy(prob).cuda(), geometry, shape, interp="nearest", want_prob=True)
        assert np.array_equal(got["label"].cpu().numpy(), want["label"]), (name, k)
        assert np.array_equal(got["prob"].cpu().numpy().astype(np.float64), want["prob"]), (name, k)


@both_libs
def test_ties_go_to_the_lower_channel(lib_mode):
    from vae_segmentation_amd import ops
    patch, shape = 16, (23, 30, 41)
    geometry = U.case_geometry(U.KERNEL_CASES[3])
    base = U.softmax_like(2, patch, 77)
    p = np.stack([base[0], base[1], base[1]])                    # channels 1 and 2 are the same numbers: 2 never wins
    for interp in ("linear", "nearest"):
        got = ops.uncrop(torch.from_numpy(p).cuda(), geometry, shape, interp=interp, want_prob=True)
        label, prob = got["label"].cpu().numpy(), got["prob"].cpu().numpy()
        assert np.array_equal(prob[1], prob[2]) and (label == 1).any() and (label == 0).any() and not (label == 2).any()
        assert np.array_equal(label == 1, prob[1] > prob[0])
    flat = torch.full((8, patch, patch, patch), 0.125, device="cuda")
    assert not ops.uncrop(flat, geometry, shape)["label"].any()
    with pytest.raises(Exception, match="uncrop"):              # a geometry that does not fit the scan is refused on the host
        ops.uncrop(flat, ([0, 0, 0], [24, 30, 41], [0, 0, 0], 41), shape)
    with pytest.raises(Exception, match="uncrop"):
        ops.uncrop(flat, ([0, 0, 0], [23, 30, 41], [0, 0, 1], 41), shape)          # off + hi - lo > side
    with pytest.raises(ValueError, match="interp"):
        ops.uncrop(flat, geometry, shape, interp="cubic")
    with pytest.raises(ValueError, match="K"):
        ops.uncrop(torch.zeros(9, patch, patch, patch, device="cuda"), geometry, shape)


def blob(shape, centre, radii):
    z, y, x = np.indices(shape)
    r = ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2
    return np.where(r < 0.3, 2.0, np.where(r < 1.0, 1.0, 0.0)).astype(np.float32)


@both_libs
@pytest.mark.parametrize("centre,radii", [((20, 24, 30), (8, 10, 12.5)), ((4, 30, 40), (9, 11, 13))], ids=["interior", "clipped-at-z0"])
def test_crop_geometry_is_what_crop_resize_did(lib_mode, centre, radii):
    """CropResize (order 0, side <= P: nothing is lost) followed by uncrop(nearest) gives the label back on [lo, hi) and background outside"""
    from vae_segmentation_amd import data_gpu, ops
    shape, patch = (40, 48, 56), 32
    lab = blob(shape, centre, radii)
    label = torch.from_numpy(lab).cuda()
    mask = (label > 0).float()
    img = torch.from_numpy(np.random.RandomState(1).randn(*shape).astype(np.float32)).cuda()
    geometry = data_gpu.crop_geometry(data_gpu.bounding_box(mask), shape)
    lo, hi, off, side = geometry
    assert side <= patch and (centre[0] > 10 or (lo[0] == 0 and off[0] > 0))
    crop = data_gpu.CropResize(["venous"], (patch,) * 3)({"venous": img, "venous_pancreas": label, "venous_pancreas_pred": mask})
    assert tuple(crop["ori_shape"]) == shape + (side,) * 3
    hot = ops.onehot(crop["venous_pancreas"][None, None], 3)[0]
    got = ops.uncrop(hot, geometry, shape, interp="nearest")["label"].cpu().numpy()
    want = np.zeros(shape, np.uint8)
    sl = tuple(slice(lo[d], hi[d]) for d in range(3))
    want[sl] = lab[sl].astype(np.uint8)
    assert np.array_equal(got, want)
    assert np.array_equal(want, lab.astype(np.uint8))             # the crop holds the whole blob here


def test_repeated_calls_and_both_builds_give_the_same_bytes():
    from vae_segmentation_amd import ops
    case = U.KERNEL_CASES[4]
    prob = torch.from_numpy(U.softmax_like(3, case[2], 5)).cuda()
    was = ops.is_deterministic()
    runs = []
    try:
        for det in (True, False, True):
            ops.set_deterministic(det)
            for interp in ("linear", "nearest"):
                for _ in range(2):
                    runs.append((interp, ops.uncrop(prob, U.case_geometry(case), case[1], interp=interp, want_prob=True)))
    finally:
        ops.set_deterministic(was)
    for interp, r in runs:
        base = next(b for i, b in runs if i == interp)
        assert torch.equal(r["label"], base["label"]) and torch.equal(r["prob"].view(torch.int32), base["prob"].view(torch.int32)), interp


# ---- the composition ------------------------------------------------------------------------------------------------------------------------
class PlantedNet:
    """a 'network' in the dict protocol of modules.Segmentation whose answer is known: probability 0.9 of class 1 where the normalised intensity is
    positive, 0.1 elsewhere (threshold: how far the organ must stand out)"""

    def __init__(self, threshold=0.0):
        self.threshold = threshold

    def __call__(self, data_dict, in_key, out_key):
        p1 = torch.where(data_dict[in_key][:, 0] > self.threshold, 0.9, 0.1)
        data_dict[out_key] = torch.stack([1 - p1, p1], 1)
        return data_dict


def _segmentation(seed=3):
    import joint_model as M
    from oracle import ref_cpu as O
    return O.deterministic_fill_(M.Segmentation(n_channels=1, n_class=2, norm_type=1), seed=seed).cuda().eval()


def synthetic_case(shape=(40, 48, 56)):
    """a bright ellipsoid (400 HU over a -200 HU background, mild noise): after Clip / CenterIntensities the organ is +1, the background -1"""
    organ = blob(shape, (18, 22, 30), (9, 8, 12)) > 0
    img = np.where(organ, 400.0, -200.0) + np.random.RandomState(4).randn(*shape) * 5.0
    return img.astype(np.float32), organ


def manual_chain(seg, img, patch, batch, interp):
    """coarse_to_fine_predict spelled out with the public pieces"""
    from vae_segmentation_amd import data_gpu, evaluation, ops
    norm = lambda d: data_gpu.CenterIntensities(["image"], subtrahend=100, divisor=300)(data_gpu.Clip(["image"], new_min=-200, new_max=400)(d))
    fn = evaluation.segmentation_model_fn(seg)
    with torch.no_grad():
        coarse = evaluation.sliding_window_predict(fn, norm({"image": img.clone()})["image"], patch, overlap=0.5, blend="gaussian", batch=batch,
                                                   cval=(0.0 - 100.0) / 300.0)
        mask = evaluation.localise(coarse["prob"], keep_largest=1, min_size=0, lo_channel=1)
        box = data_gpu.bounding_box(mask)
        if box is None:
            return coarse["label"], None, None
        geometry = data_gpu.crop_geometry(box, tuple(img.shape))
        crop = norm(data_gpu.CropResize(["image"], (patch,) * 3)({"image": img, "image_pancreas": mask, "image_pancreas_pred": mask}))
        fine = fn(crop["image"][None, None])
        return coarse["label"], geometry, ops.uncrop(fine[0], geometry, tuple(img.shape), interp=interp)["label"]


def test_coarse_to_fine_is_the_composition_of_the_public_pieces():
    from vae_segmentation_amd import evaluation, ops
    assert ops.is_deterministic()
    vol, organ = synthetic_case()
    img = torch.from_numpy(vol).cuda()
    before = img.clone()
    # the real network, fp32 kernels: bit for bit the manual chain
    seg = _segmentation()
    for interp, batch in (("linear", 2), ("nearest", 1)):
        res = evaluation.coarse_to_fine_predict(seg, img, 32, batch=batch, interp=interp)
        coarse_label, geometry, label = manual_chain(seg, img, 32, batch, interp)
        assert sorted(res) == ["coarse_label", "found", "geometry", "label"] and torch.equal(img, before)
        assert res["label"].dtype == torch.uint8 and tuple(res["label"].shape) == vol.shape and torch.equal(res["coarse_label"], coarse_label)
        assert res["found"] is (geometry is not None)
        print("network, %s: found %s, geometry %s, %d foreground voxels pasted" % (interp, res["found"], res["geometry"], int(res["label"].sum())))
        if res["found"]:
            assert res["geometry"][3] == geometry[3] and all(list(res["geometry"][i]) == list(geometry[i]) for i in range(3))
            assert torch.equal(res["label"], label)
        else:
            assert res["geometry"] is None and not res["label"].any()
    # a network whose answer is known: the pasted label is the organ up to the two resamplings' boundary shift (under one voxel each at scale <= 1.2)
    res = evaluation.coarse_to_fine_predict(PlantedNet(), img, 32, batch=3)
    assert res["found"] is True and np.array_equal(res["coarse_label"].cpu().numpy() == 1, organ)
    coarse_label, geometry, label = manual_chain(PlantedNet(), img, 32, 3, "linear")
    assert torch.equal(res["label"], label) and res["geometry"][3] == geometry[3] <= 32
    got = res["label"].cpu().numpy() == 1
    ball = ndi.generate_binary_structure(3, 3)
    assert got[ndi.binary_erosion(organ, ball, iterations=2)].all() and not got[~ndi.binary_dilation(organ, ball, iterations=2)].any()
    dice = 2.0 * (got & organ).sum() / (got.sum() + organ.sum())
    print("planted organ: dice of the pasted fine label %.4f, side %d" % (dice, geometry[3]))
    # nothing found: no box, an all-background label, no exception
    empty = evaluation.coarse_to_fine_predict(PlantedNet(threshold=5.0), img, 32)
    assert empty["found"] is False and empty["geometry"] is None and not empty["label"].any() and not empty["coarse_label"].any()
    assert empty["label"].dtype == torch.uint8 and tuple(empty["label"].shape) == vol.shape


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------
def _write_cases(root):
    rng = np.random.RandomState(0)
    (root / "data").mkdir()
    (root / "lists").mkdir()
    names, shapes = [], [(40, 48, 44), (52, 40, 46), (44, 44, 60)]
    for i, shape in enumerate(shapes):
        merge = np.zeros(shape + (2,), np.float32)
        merge[..., 0] = rng.randn(*shape) * 250 + 40
        merge[10:30, 12:34, 8:30, 1] = 1
        merge[10:30, 12:34, 8:30, 0] += 300
        np.save(root / "data" / ("case%d_merge.npy" % i), merge)
        names.append("case%d_merge.npy" % i)
    json.dump({"NIH_train": names[:1], "NIH_val": names[1:]}, open(root / "lists" / "Multi_all.json", "w"))
    return names, shapes


_CHILD = ("import sys, %s as main\n"
          "from vae_segmentation_amd import driver, ops\n"
          "driver.run(main.parse(sys.argv[1:]), side=%r)\n"
          "ops.chain_fault()\n")


def test_entry_point_writes_fine_whole_json_and_predictions(tmp_path):
    names, shapes = _write_cases(tmp_path)
    env = dict(os.environ, PYTHONPATH=REPO)
    common = ["-M", "seg_train", "-R", str(tmp_path / "data"), "-V", str(tmp_path / "data"), "--size", "32", "-b", "1", "-E", "1", "--eval_epoch", "1",
              "--save_epoch", "1", "--display_freq", "1"]
    out = subprocess.run([sys.executable, "-c", _CHILD % ("main_source", "source"), "fine", "--real_data", "--val_whole_volume", "--val_fine_whole",
                          "--save_whole_pred", str(tmp_path / "pred"), "--sw_batch", "2"] + common, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Finished Training" in out.stdout and "dice_fine_whole" in out.stdout
    fine = json.loads((tmp_path / "tensorboard" / "fine" / "fine_0.json").read_text())
    assert sorted(fine) == ["0", "1"]
    for case in fine.values():
        assert sorted(case) == ["dice_fine_whole"] and isinstance(case["dice_fine_whole"], float) and 0.0 <= case["dice_fine_whole"] <= 1.0
    whole = json.loads((tmp_path / "tensorboard" / "fine" / "whole_0.json").read_text())
    assert sorted(whole) == ["0", "1"] and all(sorted(case) == ["dice_label_free", "dice_whole"] for case in whole.values())
    for name, shape in list(zip(names, shapes))[1:]:
        pred = np.load(tmp_path / "pred" / (os.path.splitext(name)[0] + ".npy"))
        assert pred.dtype == np.uint8 and pred.shape == shape and pred.max() <= 1
    assert sorted(os.listdir(tmp_path / "pred")) == sorted(os.path.splitext(n)[0] + ".npy" for n in names[1:])
