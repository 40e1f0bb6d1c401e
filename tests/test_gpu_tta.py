"""GPU: mirror test-time augmentation inside the sliding-window kernels (csrc/window.hip vs_sw_gather_tta / vs_sw_accumulate_tta, ops.sw_gather /
sw_accumulate with flips, evaluation.SlidingWindow / sliding_window_predict / coarse_to_fine_predict with tta, --val_tta) against the numpy
restatement of tests/tta_util.py.  Weight sums, labels and gathered windows are compared exactly, the blended probabilities to the rounding bound
stated at the check; no augmentation against the plain path, batch sizes, repeated calls, the two library builds and graph replay bit for bit."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sliding_util as SW
from tests import tta_util as TTA

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
both_libs = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
_MEMO = {}                      # the restatement of a case, shared by the two library builds


def analytic_fn(batch):
    """(B, C, P, P, P) -> (B, 3, P, P, P): a softmax over three channels of x * ramp(local z, y, x) with linear terms in local z, y and x — it depends on
    where in the window a voxel sits, so a missing or wrong mirror on any single axis changes the answer"""
    p = batch.shape[-1]
    i = torch.arange(p, device=batch.device, dtype=torch.float32) / p
    z, y, x = i.view(p, 1, 1), i.view(1, p, 1), i.view(1, 1, p)
    s = batch.sum(1)
    logits = torch.stack([s * (1.0 + 2.0 * z - y), s * (0.5 - z + 1.5 * x) + 0.25 * y, -s * (0.3 + y * x) + z], 1)
    return torch.softmax(logits, 1)


def on_device(fn):
    """a torch model_fn as the numpy model_fn of the restatement: the same function on the same window values"""
    return lambda w: fn(torch.from_numpy(np.ascontiguousarray(w)).cuda()).cpu().numpy()


def volume(shape, seed):
    return (np.random.RandomState(seed).randn(*shape) * 1.5).astype(np.float32)


def restated(fn, vol, patch, overlap, blend, flips, key):
    if key not in _MEMO:
        if len(_MEMO) > 8:
            _MEMO.clear()
        _MEMO[key] = TTA.predict(on_device(fn), vol, patch, overlap, blend, 0.0, flips)
    return _MEMO[key]


def same_bits(a, b):
    return torch.equal(a["prob"].view(torch.int32), b["prob"].view(torch.int32)) and torch.equal(a["wsum"].view(torch.int32), b["wsum"].view(torch.int32)) \
        and torch.equal(a["label"], b["label"])


# (volume shape, patch, overlap, tta, batches, blends): 112 windows and 896 items, neither a multiple of 3, odd sizes and misaligned rows; S < P on two
# axes, so the padding is mirrored; two input channels under subsets of the axes; one window, 8 items, a partial last batch
CASES = [((40, 33, 57), 16, 0.5, "dhw", (1, 3), ("gaussian",)),
         ((24, 64, 20), 32, 0.75, "dhw", (3,), ("gaussian", "constant")),
         ((2, 20, 33, 18), 16, 0.5, "w", (3,), ("gaussian", "constant")),
         ((2, 20, 33, 18), 16, 0.5, "dh", (3,), ("gaussian", "constant")),
         ((32, 32, 32), 32, 0.5, "dhw", (3,), ("gaussian", "constant"))]
ids = lambda c: "%s-p%d-o%s-%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3])


@both_libs
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_kernels_against_the_restatement(lib_mode, case):
    """prob within terms * 2^-23 absolute, terms = covering windows x nf, the most a voxel sums: each fmaf rounds by at most half an ulp of a running
    sum that the weight sum bounds — terms * 2^-24 of it — and a factor 2 covers the rounding of the weight sum and the division (at 64 terms this
    is the 1e-5 of tests/test_gpu_sliding.py).  The fp32 weight sum (fp32 additions in item order: exactly defined) and the label (the first-max
    argmax of the device's own prob) exactly."""
    from vae_segmentation_amd import evaluation
    shape, patch, overlap, tta, batches, blends = case
    vol = volume(shape, sum(shape))
    dev = torch.from_numpy(vol).cuda()
    flips = TTA.flips_of(tta)
    assert evaluation.tta_flips(tta) == flips
    for blend in blends:
        want = restated(analytic_fn, vol, patch, overlap, blend, flips, (case[:4], blend))
        bound = want["terms"] * 2.0 ** -23
        for batch in batches:
            got = evaluation.sliding_window_predict(analytic_fn, dev, patch, overlap=overlap, blend=blend, batch=batch, tta=tta)
            assert got["tta"] == flips
            prob, label, wsum = got["prob"].cpu().numpy(), got["label"].cpu().numpy(), got["wsum"].cpu().numpy()
            assert prob.dtype == np.float32 and prob.shape == (3,) + tuple(shape[-3:]) and label.dtype == np.uint8 and label.shape == tuple(shape[-3:])
            err = float(np.abs(prob.astype(np.float64) - want["prob"]).max())
            print(ids(case), blend, "batch", batch, "items", len(want["origins"]) * len(flips), "terms", want["terms"], "max abs err %.3g, bound %.3g" % (err, bound))
            assert err <= bound, (case, blend, batch, err, bound)
            assert np.array_equal(wsum, want["wsum32"]), (case, blend, batch)
            assert np.array_equal(label, SW.first_argmax(prob)), (case, blend, batch)


@both_libs
def test_gather_writes_each_slot_mirrored(lib_mode):
    """every slot of a batch is np.flip of the plain window over its code's axes, bit for bit; slots past nw * nf are cval.  Windows of 16 over odd
    rows (aligned and misaligned source quads), a 10-wide window (P no multiple of 4: a partial last quad, mirrored) and S < P with cval = -7.5."""
    from vae_segmentation_amd import ops
    cval = -7.5
    for shape, patch, flips in (((2, 20, 33, 18), 16, tuple(range(8))), ((1, 12, 16, 9), 16, tuple(range(8))), ((1, 24, 64, 20), 32, (0, 1, 6, 7)),
                                ((1, 14, 13, 29), 10, (5, 3, 0))):
        vol = volume(shape, 3)
        dev = torch.from_numpy(vol).cuda()
        origins, nw = ops.sw_plan(shape[1:], patch, 0.5)
        plan = SW.plan(shape[1:], patch, 0.5)
        nf, n_items, b = len(flips), nw * len(flips), 5
        for start in range(0, n_items + b, b):                   # the last round lies wholly past the plan
            first = torch.tensor([start], dtype=torch.int32, device="cuda")
            batch = ops.sw_gather(dev, origins, first, b, patch=patch, cval=cval, flips=flips).cpu().numpy()
            for s in range(b):
                j = start + s
                if j < n_items:
                    assert np.array_equal(batch[s], TTA.gather(vol, plan[j // nf], patch, cval, flips[j % nf])), (shape, flips, j)
                else:
                    assert (batch[s] == cval).all(), (shape, flips, j)
    # accumulate: NaN in the slots past the items must not reach the sums
    shape, patch = (20, 33, 18), 16
    origins, nw = ops.sw_plan(shape, patch, 0.5)
    first = torch.tensor([2 * nw - 1], dtype=torch.int32, device="cuda")
    prob = torch.ones(3, 2, patch, patch, patch, device="cuda")
    prob[1:] = float("nan")
    acc, wsum = torch.zeros((2,) + shape, device="cuda"), torch.zeros(shape, device="cuda")
    ops.sw_accumulate(prob, acc, wsum, origins, first, ops.sw_weights(patch, "gaussian"), flips=(0, 3))
    w3 = np.zeros(shape, np.float32)
    oz, oy, ox = (int(v) for v in SW.plan(shape, patch, 0.5)[-1])
    w3[oz:oz + patch, oy:oy + patch, ox:ox + patch] = SW.window_weight(SW.weights(patch, "gaussian"))[:shape[0] - oz, :shape[1] - oy, :shape[2] - ox]
    assert np.array_equal(wsum.cpu().numpy(), w3) and np.array_equal(acc[0].cpu().numpy(), w3) and np.array_equal(acc[1].cpu().numpy(), w3)


@both_libs
def test_no_augmentation_is_the_plain_path(lib_mode):
    """tta=None, flips (0,) — the new kernels with one code that mirrors nothing — and a SlidingWindow built without the argument: the same bits"""
    from vae_segmentation_amd import evaluation, ops
    for shape, patch, overlap, batch in (((40, 33, 57), 16, 0.5, 3), ((24, 64, 20), 32, 0.75, 2), ((2, 20, 33, 18), 16, 0.5, 1)):
        dev = torch.from_numpy(volume(shape, 7)).cuda()
        plain = evaluation.SlidingWindow(analytic_fn, shape, patch, overlap=overlap, batch=batch)(dev)
        off = evaluation.sliding_window_predict(analytic_fn, dev, patch, overlap=overlap, batch=batch, tta=None)
        one = evaluation.sliding_window_predict(analytic_fn, dev, patch, overlap=overlap, batch=batch, tta=(0,))
        assert plain["tta"] is None and off["tta"] is None and one["tta"] == (0,)
        assert same_bits(off, plain) and same_bits(one, plain), (shape, patch)
        # the kernels one by one
        origins, nw = ops.sw_plan(shape[-3:], patch, overlap)
        first = torch.tensor([nw - 2], dtype=torch.int32, device="cuda")
        vol4 = dev if dev.dim() == 4 else dev[None]
        assert torch.equal(ops.sw_gather(vol4, origins, first, 3, patch=patch, cval=0.5), ops.sw_gather(vol4, origins, first, 3, patch=patch, cval=0.5, flips=(0,)))


def test_batch_sizes_repeated_calls_graph_replay_and_both_builds_give_the_same_bits():
    from vae_segmentation_amd import evaluation, ops
    shape, patch = (40, 33, 57), 16
    dev = torch.from_numpy(volume(shape, 12)).cuda()
    was = ops.is_deterministic()
    runs = []
    try:
        for det in (True, False):
            ops.set_deterministic(det)
            for batch in (1, 3, 8):
                runs.append((det, batch, "eager", evaluation.sliding_window_predict(analytic_fn, dev, patch, overlap=0.5, batch=batch, tta="dhw")))
            sw = evaluation.SlidingWindow(analytic_fn, shape, patch, overlap=0.5, batch=3, graph=True, tta="dhw")
            assert sw.nw == 112 and sw.n_items == 896 and sw.n_batches == 299
            for call in ("graph", "graph again"):
                runs.append((det, 3, call, sw(dev)))
            assert sw.graph is not None
            del sw
    finally:
        ops.set_deterministic(was)
    base = runs[0][3]
    for det, batch, how, r in runs:
        assert same_bits(r, base), (det, batch, how)
    other = evaluation.sliding_window_predict(analytic_fn, dev, patch, overlap=0.5, batch=3, tta="hw")
    assert not torch.equal(other["prob"], base["prob"])


def _segmentation(seed=3):
    import joint_model as M
    from oracle import ref_cpu as O
    from vae_segmentation_amd.modules import set_kernel_dtype
    seg = O.deterministic_fill_(M.Segmentation(n_channels=1, n_class=2, norm_type=1), seed=seed).cuda().eval()
    set_kernel_dtype(seg, torch.float32)
    return seg


def test_real_network_against_eight_plain_passes():
    """Segmentation(1, 2, InstanceNorm), fp32 kernels, deterministic library: the in-kernel TTA against what a user writes without it — one plain
    sliding-window pass per code, model_fn wrapped in torch.flip in and out, the eight probabilities averaged (float64, on the host).  The network
    sees the same window bits either way, so the difference is the blend's rounding: the bound of test_kernels_against_the_restatement."""
    from vae_segmentation_amd import evaluation, ops
    assert ops.is_deterministic()
    shape, patch = (40, 36, 44), 32
    vol = volume(shape, 21) * 0.5
    dev = torch.from_numpy(vol).cuda()
    fn = evaluation.segmentation_model_fn(_segmentation())
    flips = TTA.flips_of("dhw")

    def flipped(code):
        dims = TTA.flip_axes(code, 5)
        return (lambda b: torch.flip(fn(torch.flip(b, dims).contiguous()), dims)) if dims else fn
    with torch.no_grad():
        got = evaluation.sliding_window_predict(fn, dev, patch, overlap=0.5, blend="gaussian", batch=1, tta="dhw")
        plain = [evaluation.sliding_window_predict(flipped(c), dev, patch, overlap=0.5, blend="gaussian", batch=1)["prob"].double() for c in flips]
    want = torch.stack(plain).mean(0)
    cover = np.zeros(shape, np.int64)
    for oz, oy, ox in SW.plan(shape, patch, 0.5).tolist():
        cover[oz:oz + patch, oy:oy + patch, ox:ox + patch] += 1
    terms = int(cover.max()) * len(flips)
    err = float((got["prob"].double() - want).abs().max())
    print("fp32 network, %d terms, max abs err %.3g, bound %.3g" % (terms, err, terms * 2.0 ** -23))
    assert terms == 64 and err <= terms * 2.0 ** -23
    assert float(got["prob"][1].max() - got["prob"][1].min()) > 1e-3                             # the prediction varies over the volume
    assert float((got["prob"].double() - plain[0]).abs().max()) > 10 * terms * 2.0 ** -23        # and the augmentation changes it
    assert np.array_equal(got["label"].cpu().numpy(), SW.first_argmax(got["prob"].cpu().numpy()))


def blob(shape, centre, radii):
    z, y, x = np.indices(shape)
    r = ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2
    return np.where(r < 0.3, 2.0, np.where(r < 1.0, 1.0, 0.0)).astype(np.float32)


def synthetic_case(shape=(40, 48, 56)):
    """a bright ellipsoid (400 HU over a -200 HU background, mild noise): after Clip / CenterIntensities the organ is +1, the background -1"""
    organ = blob(shape, (18, 22, 30), (9, 8, 12)) > 0
    img = np.where(organ, 400.0, -200.0) + np.random.RandomState(4).randn(*shape) * 5.0
    return img.astype(np.float32), organ


class PlantedNet:
    """a "network" whose answer is known: foreground where the centred intensity is above the threshold, whatever way round the window arrives"""
    def __init__(self, threshold=0.0):
        self.threshold = threshold

    def __call__(self, data_dict, in_key, out_key):
        p1 = torch.where(data_dict[in_key][:, 0] > self.threshold, 0.9, 0.1)
        data_dict[out_key] = torch.stack([1 - p1, p1], 1)
        return data_dict


def manual_chain(seg, img, patch, batch, interp, tta):
    """coarse_to_fine_predict(tta=...) spelled out with the public pieces"""
    from vae_segmentation_amd import data_gpu, evaluation, ops
    norm = lambda d: data_gpu.CenterIntensities(["image"], subtrahend=100, divisor=300)(data_gpu.Clip(["image"], new_min=-200, new_max=400)(d))
    fn = evaluation.segmentation_model_fn(seg)
    with torch.no_grad():
        coarse = evaluation.sliding_window_predict(fn, norm({"image": img.clone()})["image"], patch, overlap=0.5, blend="gaussian", batch=batch,
                                                   cval=(0.0 - 100.0) / 300.0, tta=tta)
        mask = evaluation.localise(coarse["prob"], keep_largest=1, min_size=0, lo_channel=1)
        box = data_gpu.bounding_box(mask)
        if box is None:
            return coarse["label"], None, None
        geometry = data_gpu.crop_geometry(box, tuple(img.shape))
        crop = norm(data_gpu.CropResize(["image"], (patch,) * 3)({"image": img, "image_pancreas": mask, "image_pancreas_pred": mask}))
        fine = evaluation.sliding_window_predict(fn, crop["image"], patch, overlap=0.0, blend="constant", batch=batch, tta=tta)
        assert tuple(fine["wsum"].shape) == (patch,) * 3 and bool((fine["wsum"] == len(evaluation.tta_flips(tta))).all())       # one window, every flip
        return coarse["label"], geometry, ops.uncrop(fine["prob"], geometry, tuple(img.shape), interp=interp)["label"]


def test_coarse_to_fine_with_tta_is_the_composition_of_the_public_pieces():
    from vae_segmentation_amd import evaluation, ops
    assert ops.is_deterministic()
    vol, organ = synthetic_case()
    img = torch.from_numpy(vol).cuda()
    before = img.clone()
    seg = _segmentation()
    found = []
    for net, interp, batch in ((seg, "linear", 2), (seg, "nearest", 3), (PlantedNet(), "linear", 3)):
        res = evaluation.coarse_to_fine_predict(net, img, 32, batch=batch, interp=interp, tta="dhw")
        coarse_label, geometry, label = manual_chain(net, img, 32, batch, interp, "dhw")
        assert sorted(res) == ["coarse_label", "found", "geometry", "label"] and torch.equal(img, before)
        assert res["label"].dtype == torch.uint8 and tuple(res["label"].shape) == vol.shape and torch.equal(res["coarse_label"], coarse_label)
        assert res["found"] is (geometry is not None)
        print("%s, %s: found %s, geometry %s, %d foreground voxels pasted" % (type(net).__name__, interp, res["found"], res["geometry"], int(res["label"].sum())))
        if res["found"]:
            assert res["geometry"][3] == geometry[3] and all(list(res["geometry"][i]) == list(geometry[i]) for i in range(3))
            assert torch.equal(res["label"], label)
        else:
            assert res["geometry"] is None and not res["label"].any()
        found.append(res["found"])
    assert found[-1] is True                                     # the planted organ is found whatever the real network does
    # a pointwise answer commutes with the mirrors: the planted coarse label is the organ with and without augmentation
    plain = evaluation.coarse_to_fine_predict(PlantedNet(), img, 32, batch=3)
    assert torch.equal(plain["coarse_label"], res["coarse_label"]) and np.array_equal(res["coarse_label"].cpu().numpy() == 1, organ)


def _write_cases(root):
    rng = np.random.RandomState(0)
    (root / "data").mkdir()
    (root / "lists").mkdir()
    names = []
    for i, shape in enumerate([(40, 48, 44), (52, 40, 46), (44, 44, 60)]):
        merge = np.zeros(shape + (2,), np.float32)
        merge[..., 0] = rng.randn(*shape) * 250 + 40
        merge[10:30, 12:34, 8:30, 1] = 1
        merge[10:30, 12:34, 8:30, 0] += 300
        np.save(root / "data" / ("case%d_merge.npy" % i), merge)
        names.append("case%d_merge.npy" % i)
    json.dump({"NIH_train": names[:1], "NIH_val": names[1:]}, open(root / "lists" / "Multi_all.json", "w"))
    return names


_CHILD = ("import sys, %s as main\n"
          "from vae_segmentation_amd import driver, ops\n"
          "driver.run(main.parse(sys.argv[1:]), side=%r)\n"
          "ops.chain_fault()\n")


def test_entry_point_records_tta(tmp_path):
    _write_cases(tmp_path)
    env = dict(os.environ, PYTHONPATH=REPO)
    common = ["-M", "seg_train", "-R", str(tmp_path / "data"), "-V", str(tmp_path / "data"), "--size", "32", "-b", "1", "-E", "1", "--eval_epoch", "1",
              "--save_epoch", "1", "--display_freq", "1"]
    out = subprocess.run([sys.executable, "-c", _CHILD % ("main_source", "source"), "tta", "--real_data", "--val_whole_volume", "--val_fine_whole", "--val_tta", "hw",
                          "--sw_batch", "2"] + common, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]              # the child ends with ops.chain_fault(): a raised fault word is an error exit
    assert "Finished Training" in out.stdout and "mirror TTA (0, 1, 2, 3)" in out.stdout and "dice_fine_whole" in out.stdout
    whole = json.loads((tmp_path / "tensorboard" / "tta" / "whole_0.json").read_text())
    fine = json.loads((tmp_path / "tensorboard" / "tta" / "fine_0.json").read_text())
    assert whole["tta"] == [0, 1, 2, 3] and fine["tta"] == [0, 1, 2, 3]
    assert sorted(whole) == ["0", "1", "tta"] and sorted(fine) == ["0", "1", "tta"]
    for i in ("0", "1"):                                                             # the Dice keys keep their names
        assert sorted(whole[i]) == ["dice_label_free", "dice_whole"] and sorted(fine[i]) == ["dice_fine_whole"]
        assert all(isinstance(v, float) and math.isfinite(v) and 0.0 <= v <= 1.0 for v in list(whole[i].values()) + list(fine[i].values()))
