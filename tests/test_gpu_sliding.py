"""GPU: sliding-window prediction of whole volumes (csrc/window.hip, ops.sw_*, evaluation.sliding_window_predict / SlidingWindow / localise,
--val_whole_volume) against the numpy restatement of tests/sliding_util.py.  Origins, weight sums and labels are compared exactly, the blended
probabilities to the rounding bound stated at the check; batch sizes, repeated calls, the two library builds and graph replay bit for bit."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import sliding_util as SW

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
both_libs = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
_MEMO = {}                      # the restatement of a case, shared by the two library builds


def analytic_fn(batch):
    """(B, C, P, P, P) -> (B, 3, P, P, P): a softmax over three channels of x * ramp(local z, y, x) — it depends on where in the window a voxel sits, so a
    misplaced or transposed window changes the answer"""
    p = batch.shape[-1]
    i = torch.arange(p, device=batch.device, dtype=torch.float32) / p
    z, y, x = i.view(p, 1, 1), i.view(1, p, 1), i.view(1, 1, p)
    s = batch.sum(1)
    logits = torch.stack([s * (1.0 + 2.0 * z - y), s * (0.5 - z + 1.5 * x) + 0.25 * y, -s * (0.3 + y * x) + z], 1)
    return torch.softmax(logits, 1)


def pointwise_fn(batch):
    s = batch[:, 0]
    return torch.softmax(torch.stack([s, -s, 0.5 * s * s], 1), 1)


def on_device(fn):
    """a torch model_fn as the numpy model_fn of the restatement: the same function on the same window values"""
    return lambda w: fn(torch.from_numpy(np.ascontiguousarray(w)).cuda()).cpu().numpy()


def volume(shape, seed):
    return (np.random.RandomState(seed).randn(*shape) * 1.5).astype(np.float32)


def restated(fn, vol, patch, overlap, blend, key):
    if key not in _MEMO:
        if len(_MEMO) > 8:
            _MEMO.clear()
        _MEMO[key] = SW.predict(on_device(fn), vol, patch, overlap, blend)
    return _MEMO[key]


# (volume shape, patch, overlap): windows of 16 and 32 against odd sizes, S < P on two axes, a single window, two input channels.  The numbers of
# windows — 112, 8, 20, 2, 5, 1, 16 — are no multiples of 3 (except the single window's batch, which is all padding but one slot)
CASES = [((40, 33, 57), 16, 0.5), ((40, 33, 57), 32, 0), ((40, 33, 57), 32, 0.75), ((24, 64, 20), 32, 0), ((24, 64, 20), 32, 0.75), ((24, 64, 20), 32, 0.5),
         ((32, 32, 32), 32, 0.5), ((2, 20, 33, 18), 16, 0.5)]
ids = lambda c: "%s-p%d-o%s" % ("x".join(map(str, c[0])), c[1], c[2])


@both_libs
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_kernels_against_the_restatement(lib_mode, case):
    """prob within 1e-5 absolute: a voxel sums at most 4^3 = 64 fp32 terms w p with p in [0, 1] at overlap 0.75 and is divided once — about 64 * 2^-24 ~ 4e-6 of
    the weight sum against the float64 restatement.  Origins, the fp32 weight sum (fp32 additions in plan order: exactly defined) and the label
    (the first-max argmax of the device's own prob) exactly."""
    from vae_segmentation_amd import evaluation, ops
    shape, patch, overlap = case
    vol = volume(shape, sum(shape))
    dev = torch.from_numpy(vol).cuda()
    origins, nw = ops.sw_plan(shape[-3:], patch, overlap)
    want_origins = SW.plan(shape[-3:], patch, overlap)
    assert origins.dtype == torch.int32 and nw == len(want_origins) and np.array_equal(origins.cpu().numpy(), want_origins)
    if nw not in (1, 3):
        assert nw % 3 != 0
    for blend in ("gaussian", "constant"):
        want = restated(analytic_fn, vol, patch, overlap, blend, (case, blend))
        assert np.array_equal(ops.sw_weights(patch, blend).cpu().numpy(), SW.weights(patch, blend))
        for batch in (1, 3):
            got = evaluation.sliding_window_predict(analytic_fn, dev, patch, overlap=overlap, blend=blend, batch=batch)
            prob, label, wsum = got["prob"].cpu().numpy(), got["label"].cpu().numpy(), got["wsum"].cpu().numpy()
            assert prob.dtype == np.float32 and prob.shape == (3,) + tuple(shape[-3:]) and label.dtype == np.uint8 and label.shape == tuple(shape[-3:])
            err = float(np.abs(prob.astype(np.float64) - want["prob"]).max())
            print(ids(case), blend, "batch", batch, "windows", nw, "max abs err %.3g" % err)
            assert err <= 1e-5, (case, blend, batch, err)
            assert np.array_equal(wsum, want["wsum32"]), (case, blend, batch)
            assert np.array_equal(label, SW.first_argmax(prob)), (case, blend, batch)


@both_libs
def test_slots_past_the_plan_and_positions_past_the_volume(lib_mode):
    """the kernels one by one: a batch that starts at the last window holds that window and cval; its accumulation touches that window's voxels only"""
    from vae_segmentation_amd import ops
    shape, patch, cval = (2, 20, 33, 18), 16, -7.5
    vol = volume(shape, 3)
    dev = torch.from_numpy(vol).cuda()
    origins, nw = ops.sw_plan(shape[1:], patch, 0.5)
    first = torch.tensor([nw - 1], dtype=torch.int32, device="cuda")
    batch = ops.sw_gather(dev, origins, first, 3, patch=patch, cval=cval)
    last = SW.plan(shape[1:], patch, 0.5)[-1]
    assert np.array_equal(batch[0].cpu().numpy(), SW.gather(vol, last, patch, cval))
    assert (batch[1:] == cval).all()
    # S < P: a 12-wide volume under a 16-wide window reads cval beyond it
    small = volume((1, 12, 16, 9), 4)
    o2, n2 = ops.sw_plan((12, 16, 9), patch, 0.5)
    assert n2 == 1
    b2 = ops.sw_gather(torch.from_numpy(small).cuda(), o2, torch.zeros(1, dtype=torch.int32, device="cuda"), 2, patch=patch, cval=cval)
    assert np.array_equal(b2[0].cpu().numpy(), SW.gather(small, (0, 0, 0), patch, cval)) and (b2[0, :, 12:] == cval).all() and (b2[0, :, :, :, 9:] == cval).all()
    assert (b2[1] == cval).all()
    # accumulate: NaN in the slots past the plan must not reach the sums
    wt = ops.sw_weights(patch, "gaussian")
    prob = torch.ones(3, 2, patch, patch, patch, device="cuda")
    prob[1:] = float("nan")
    acc, wsum = torch.zeros((2,) + shape[1:], device="cuda"), torch.zeros(shape[1:], device="cuda")
    ops.sw_accumulate(prob, acc, wsum, origins, first, wt)
    w3 = np.zeros(shape[1:], np.float32)
    oz, oy, ox = (int(v) for v in last)
    w3[oz:oz + patch, oy:oy + patch, ox:ox + patch] = SW.window_weight(SW.weights(patch, "gaussian"))[:shape[1] - oz, :shape[2] - oy, :shape[3] - ox]
    assert np.array_equal(wsum.cpu().numpy(), w3) and np.array_equal(acc[0].cpu().numpy(), w3) and np.array_equal(acc[1].cpu().numpy(), w3)
    # finalize: label, one-hot, in one pass; ties go to the first maximal channel
    a = torch.tensor([[1.0, 2.0, 3.0, 0.0, 5.0], [1.0, 4.0, 1.0, 0.0, 5.0], [0.5, 4.0, 3.0, 0.0, 6.0]], device="cuda").view(3, 1, 1, 5)
    p, lab, hot = ops.sw_finalize(a, torch.full((1, 1, 5), 2.0, device="cuda"), label=True, onehot=True)
    assert torch.equal(p, a / 2) and lab.view(-1).tolist() == [0, 1, 0, 0, 2] and torch.equal(hot.argmax(0).to(torch.uint8), lab) and torch.equal(hot.sum(0), torch.ones_like(hot[0]))


@both_libs
def test_pointwise_model_with_constant_blend_is_the_model_on_the_whole_volume(lib_mode):
    from vae_segmentation_amd import evaluation
    for shape, patch, overlap, batch in (((40, 33, 57), 16, 0.5, 4), ((24, 64, 20), 32, 0.75, 2), ((2, 20, 33, 18), 16, 0.25, 1)):
        dev = torch.from_numpy(volume(shape, 9)).cuda()
        got = evaluation.sliding_window_predict(pointwise_fn, dev, patch, overlap=overlap, blend="constant", batch=batch)
        want = pointwise_fn(dev[None] if dev.dim() == 4 else dev[None, None])[0]
        err = float((got["prob"] - want).abs().max())
        print(shape, patch, overlap, "max abs err %.3g" % err)
        assert err <= 1e-6
        assert np.array_equal(got["label"].cpu().numpy(), SW.first_argmax(got["prob"].cpu().numpy()))


def test_batch_sizes_repeated_calls_and_both_builds_give_the_same_bits():
    from vae_segmentation_amd import evaluation, ops
    shape, patch = (40, 33, 57), 16
    dev = torch.from_numpy(volume(shape, 12)).cuda()
    was = ops.is_deterministic()
    res = {}
    try:
        for det in (True, False):
            ops.set_deterministic(det)
            for batch in (1, 2, 5, 1):
                r = evaluation.sliding_window_predict(analytic_fn, dev, patch, overlap=0.5, blend="gaussian", batch=batch)
                res.setdefault(det, []).append(r)
    finally:
        ops.set_deterministic(was)
    base = res[True][0]
    for det, runs in res.items():
        for r in runs:
            assert torch.equal(r["prob"].view(torch.int32), base["prob"].view(torch.int32)), det
            assert torch.equal(r["label"], base["label"]) and torch.equal(r["wsum"].view(torch.int32), base["wsum"].view(torch.int32)), det


def _segmentation(dtype=torch.float32):
    import joint_model as M
    from oracle import ref_cpu as O
    from vae_segmentation_amd.modules import set_kernel_dtype
    seg = O.deterministic_fill_(M.Segmentation(n_channels=1, n_class=2, norm_type=1), seed=3).cuda().eval()
    set_kernel_dtype(seg, dtype)
    return seg


def test_real_network_against_a_python_loop_over_windows():
    """Segmentation(1, 2, InstanceNorm), fp32 kernels, deterministic library: sliding_window_predict against the same model run window by window from
    Python and blended by the restatement.  1e-5 absolute, as above (12 windows, at most 8 over a voxel).  bf16 and fp16 storage: finite, and a
    convex combination of probability vectors is a probability vector."""
    from vae_segmentation_amd import evaluation, ops
    assert ops.is_deterministic()
    shape, patch = (48, 40, 56), 32
    vol = volume(shape, 21) * 0.5
    dev = torch.from_numpy(vol).cuda()
    seg = _segmentation()
    fn = evaluation.segmentation_model_fn(seg)
    with torch.no_grad():
        want = SW.predict(on_device(fn), vol, patch, 0.5, "gaussian")
        got = evaluation.sliding_window_predict(fn, dev, patch, overlap=0.5, blend="gaussian", batch=1)
    assert len(want["origins"]) == 12 and tuple(got["prob"].shape) == (2,) + shape
    err = float(np.abs(got["prob"].cpu().numpy().astype(np.float64) - want["prob"]).max())
    print("fp32 network, max abs err %.3g" % err)
    assert err <= 1e-5
    assert np.array_equal(got["wsum"].cpu().numpy(), want["wsum32"])
    assert float(got["prob"][1].max() - got["prob"][1].min()) > 1e-3             # the prediction varies over the volume
    for dtype in (torch.bfloat16, torch.float16):
        half = evaluation.segmentation_model_fn(_segmentation(dtype))
        r = evaluation.sliding_window_predict(half, dev, patch, overlap=0.5, blend="gaussian", batch=2)
        assert torch.isfinite(r["prob"]).all(), dtype
        dev1 = float((r["prob"].double().sum(0) - 1).abs().max())
        print(dtype, "max |sum_k prob - 1| %.3g" % dev1)
        assert dev1 <= 1e-5, dtype
        assert np.array_equal(r["label"].cpu().numpy(), SW.first_argmax(r["prob"].cpu().numpy()))


def test_graph_replay_equals_eager_and_follows_the_volume():
    """deterministic library: the captured batch replayed ceil(nw / B) times gives the eager bits, for the analytic function and for the network; the same
    capture then serves another volume of that shape (the window counter and the volume are read from device memory, nothing is baked in)"""
    from vae_segmentation_amd import evaluation, ops
    assert ops.is_deterministic()
    shape, patch = (48, 40, 56), 32
    v1, v2 = (torch.from_numpy(volume(shape, s) * 0.5).cuda() for s in (31, 32))
    for name, fn, batch in (("analytic", analytic_fn, 5), ("network", evaluation.segmentation_model_fn(_segmentation()), 2)):
        eager = [evaluation.sliding_window_predict(fn, v, patch, overlap=0.5, batch=batch) for v in (v1, v2)]
        one_shot = evaluation.sliding_window_predict(fn, v1, patch, overlap=0.5, batch=batch, graph=True)
        assert torch.equal(one_shot["prob"].view(torch.int32), eager[0]["prob"].view(torch.int32)), name
        sw = evaluation.SlidingWindow(fn, shape, patch, overlap=0.5, batch=batch, graph=True)
        assert sw.nw == 12 and sw.n_batches == -(-12 // batch)
        for v, want in ((v1, eager[0]), (v2, eager[1]), (v1, eager[0])):
            got = sw(v)
            assert sw.graph is not None
            assert torch.equal(got["prob"].view(torch.int32), want["prob"].view(torch.int32)), name
            assert torch.equal(got["label"], want["label"]) and torch.equal(got["wsum"], want["wsum"]), name
        assert not torch.equal(eager[0]["prob"], eager[1]["prob"])
        del sw


def planted(shape):
    """an organ (one component) and specks far from it"""
    z, y, x = np.indices(shape)
    organ = ((z - 22) / 9.0) ** 2 + ((y - 18) / 7.0) ** 2 + ((x - 30) / 12.0) ** 2 < 1.0
    specks = np.zeros(shape, bool)
    specks[2:4, 3:5, 50:52] = True
    specks[40, 30, 5] = True
    specks[5, 34, 6:8] = True
    return organ, specks


def stub_fn(batch):
    """the image carries the planted prediction: 0.9 / 0.1 probabilities where it is set, whatever window the voxel arrives in"""
    p1 = torch.where(batch[:, 0] > 0.5, 0.9, 0.1)
    return torch.stack([1 - p1, p1], 1)


@both_libs
def test_localise_finds_the_organ_and_feeds_crop_resize(lib_mode):
    from vae_segmentation_amd import data_gpu, evaluation
    shape = (44, 36, 57)
    organ, specks = planted(shape)
    img = torch.from_numpy((organ | specks).astype(np.float32)).cuda()
    res = evaluation.sliding_window_predict(stub_fn, img, 16, overlap=0.5, batch=3)
    assert np.array_equal(res["label"].cpu().numpy() == 1, organ | specks)
    organ_t = torch.from_numpy(organ.astype(np.float32)).cuda()
    for source in (res["prob"], res["label"]):
        mask = evaluation.localise(source, keep_largest=1)
        assert mask.dtype == torch.float32 and tuple(mask.shape) == shape and torch.equal(mask, organ_t)
        box, want = data_gpu.bounding_box(mask), data_gpu.bounding_box(organ_t)
        assert np.array_equal(box[0], want[0]) and np.array_equal(box[1], want[1])
    unfiltered = evaluation.localise(res["prob"], keep_largest=0)
    assert torch.equal(unfiltered, img) and data_gpu.bounding_box(unfiltered)[1][2] == 51
    assert torch.equal(evaluation.localise(res["prob"], keep_largest=2, min_size=9), organ_t)          # the largest speck has 8 voxels
    assert int(evaluation.localise(res["prob"], keep_largest=2).sum()) == int(organ.sum()) + 8
    scan = torch.from_numpy(volume(shape, 5) * 200).cuda()
    label = torch.from_numpy(np.roll(organ, 2, axis=2).astype(np.float32)).cuda()
    crops = [data_gpu.CropResize(["venous"], (32, 32, 32))({"venous": scan, "venous_pancreas": label, "venous_pancreas_pred": m})
             for m in (evaluation.localise(res["prob"]), organ_t)]
    for key in ("venous", "venous_pancreas", "venous_pancreas_pred"):
        assert torch.equal(crops[0][key], crops[1][key]), key
    assert np.array_equal(crops[0]["ori_shape"], crops[1]["ori_shape"])


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


def test_validate_then_whole_volume_pass(tmp_path, capsys):
    import main_source
    from vae_segmentation_amd import driver
    names = _write_cases(tmp_path)
    args = main_source.parse(["run", "-M", "seg_train", "--real_data", "--val_whole_volume", "--size", "32", "-R", str(tmp_path / "data"), "-V", str(tmp_path / "data")])
    loader = driver.DeviceCaseLoader(names[1:], str(tmp_path / "data"), args, 1, False, False)
    seg = _segmentation()
    plain = driver.validate("seg_train", seg, loader, 2)
    capsys.readouterr()
    again = driver.validate("seg_train", seg, loader, 2)
    log = {}
    mw, mf = driver.validate_whole_volume(seg, loader.whole_cases(), 2, args.size, overlap=args.sw_overlap, batch=args.sw_batch, blend=args.sw_blend, log=log)
    out = capsys.readouterr().out
    assert again == plain and driver.validate("seg_train", seg, loader, 2) == plain          # validation itself is unchanged, before and after the pass
    assert "dice_whole %f, dice_label_free %f over 2 cases" % (mw, mf) in out
    assert sorted(log) == [0, 1]
    for case in log.values():
        assert sorted(case) == ["dice_label_free", "dice_whole"] and all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in case.values())
    assert mw == pytest.approx(np.mean([c["dice_whole"] for c in log.values()])) and mf == pytest.approx(np.mean([c["dice_label_free"] for c in log.values()]))
    # with the component filter and a batch of windows: the same arithmetic path, finite scores
    log2 = {}
    driver.validate_whole_volume(seg, loader.whole_cases(), 2, 32, overlap=0.25, batch=3, blend="constant", keep_largest=1, log=log2)
    assert sorted(log2) == [0, 1] and all(math.isfinite(v) for c in log2.values() for v in c.values())


_CHILD = ("import sys, %s as main\n"
          "from vae_segmentation_amd import driver, ops\n"
          "driver.run(main.parse(sys.argv[1:]), side=%r)\n"
          "ops.chain_fault()\n")


def test_entry_point_writes_whole_volume_json(tmp_path):
    _write_cases(tmp_path)
    env = dict(os.environ, PYTHONPATH=REPO)
    common = ["-M", "seg_train", "-R", str(tmp_path / "data"), "-V", str(tmp_path / "data"), "--size", "32", "-b", "1", "-E", "1", "--eval_epoch", "1",
              "--save_epoch", "1", "--display_freq", "1"]
    out = subprocess.run([sys.executable, "-c", _CHILD % ("main_source", "source"), "whole", "--real_data", "--val_whole_volume", "--sw_batch", "2"] + common,
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]              # the child ends with ops.chain_fault(): a raised fault word is an error exit
    assert "Finished Training" in out.stdout and "validation on whole volumes" in out.stdout and "dice_label_free" in out.stdout
    log = json.loads((tmp_path / "tensorboard" / "whole" / "whole_0.json").read_text())
    assert sorted(log) == ["0", "1"]
    for case in log.values():
        assert sorted(case) == ["dice_label_free", "dice_whole"] and all(isinstance(v, float) and math.isfinite(v) for v in case.values())
    assert json.loads((tmp_path / "tensorboard" / "whole" / "score_0.json").read_text())
    # without --real_data the flag is refused before anything runs
    for script in ("main_source.py", "main_target.py"):
        bad = subprocess.run([sys.executable, os.path.join(REPO, script), "bad", "--val_whole_volume"] + common, cwd=str(tmp_path), env=env,
                             capture_output=True, text=True, timeout=600)
        assert bad.returncode != 0 and "inconsistent flags" in bad.stderr and "--real_data" in bad.stderr, bad.stderr[-1000:]
        assert not (tmp_path / "tensorboard" / "bad").exists()
