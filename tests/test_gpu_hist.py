"""GPU: intensity histograms, joint histograms and mutual information (csrc/hist.hip; ops.histogram, ops.joint_histogram, ops.mutual_information,
evaluation.mutual_information_3d, --val_intensity) against the numpy / scipy restatement of tests/hist_util.py.  Counts are integers: the yardstick is
equality, and edge tables are compared bit for bit.  The mutual information is a chain of fp64 sums and logarithms on both sides: relative 1e-9, the
project's fp64 gate.  Every output buffer is an uninitialised torch.empty of the caller's; the tests that hand buffers to the C ABI fill them with garbage."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import hist_util as HU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# odd and tiny; four planes, W no multiple of a wave; one voxel; 74,088 voxels (more than a 16-bit counter holds, more than one workgroup's 16,384)
SHAPES = [(1, 1, 3, 5, 7), (2, 2, 9, 17, 33), (1, 1, 1, 1, 1), (1, 1, 42, 42, 42)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
BINS_1D = [1, 2, 7, 256, 4096]                                     # 4096 bins x 2 rows = 8192 cells: the last 32-bit LDS table
BINS_2D = [(1, 1), (3, 200), (256, 256), (512, 512)]               # 32-bit LDS, 32-bit LDS, packed 16-bit LDS, global atomics
GARBAGE = 0x5A


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def volumes(shape, seed):
    """name -> (N, C, D, H, W) fp32: random, one value everywhere, one long run plus noise"""
    rng = np.random.default_rng(seed)
    run = rng.uniform(-1, 1, shape).astype(np.float32)
    flat = run.reshape(shape[0] * shape[1], -1)
    flat[:, flat.shape[1] // 10: flat.shape[1] - flat.shape[1] // 10] = 0.25
    return {"random": rng.normal(0, 0.5, shape).astype(np.float32), "constant": np.full(shape, -0.375, np.float32), "run": run}


def planes(a):
    return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:])


def check_hist(got, x, bins, bounds, labels, rows, what):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    lab = [None] * (x.shape[0] * x.shape[1]) if labels is None else planes(labels)
    for p, xp in enumerate(planes(x)):
        want = HU.ref_histogram(xp, bins, bounds, lab[p], rows)
        g = {k: planes(v)[p] for k, v in got.items()}
        assert np.array_equal(bits(g["edges"]), bits(want["edges"])), what
        assert np.array_equal(g["table"], want["table"]) and g["table"].dtype == np.int64, what
        assert int(g["outside"]) == want["outside"] and int(g["overflow"]) == want["overflow"], what
        assert g["table"].sum() + want["outside"] + want["overflow"] == xp.size, what


def check_joint(got, x, y, bins, bounds, what):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for p, (xp, yp) in enumerate(zip(planes(x), planes(y))):
        want = HU.ref_joint_histogram(xp, yp, bins, bounds)
        g = {k: planes(v)[p] for k, v in got.items()}
        assert np.array_equal(bits(g["edges_x"]), bits(want["edges_x"])) and np.array_equal(bits(g["edges_y"]), bits(want["edges_y"])), what
        assert np.array_equal(g["table"], want["table"]) and int(g["outside"]) == want["outside"], what


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_histogram_matches_the_restatement(shape):
    from vae_segmentation_amd import ops
    for name, x in volumes(shape, 11).items():
        xd = dev(x)
        for bins in BINS_1D:
            for bounds in (None, (-1.0, 1.0)):
                check_hist(ops.histogram(xd, bins, range=bounds), x, bins, bounds, None, 0, (name, bins, bounds))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_joint_histogram_matches_the_restatement(shape):
    from vae_segmentation_amd import ops
    vx, vy = volumes(shape, 21), volumes(shape, 22)
    pairs = {"random": (vx["random"], vy["random"]), "constant": (vx["constant"], vx["constant"]), "run": (vx["run"], vy["run"]),
             "shifted": (vx["random"], np.roll(vx["random"], 1, axis=-1))}
    for name, (x, y) in pairs.items():
        xd, yd = dev(x), dev(y)
        for bins in BINS_2D:
            for bounds in (None, ((-1.0, 1.0), (-0.5, 0.75))):
                check_joint(ops.joint_histogram(xd, yd, bins=bins, range=bounds), x, y, bins, bounds, (name, bins, bounds))
    if shape[-1] == 42:                                  # 74,088 voxels of one plane in ONE cell of the packed 16-bit table
        t = ops.joint_histogram(dev(pairs["constant"][0]), dev(pairs["constant"][1]), bins=(256, 256))["table"]
        assert int(t.max()) == 42 ** 3 == int(t.sum()) and 42 ** 3 > 65535


def test_every_kernel_form_gives_the_same_tables():
    """vs_config.hist_form forces the 32-bit LDS (1), packed 16-bit LDS (2) or global-atomic (3) kernel where the table fits it"""
    from vae_segmentation_amd import ops
    shape = (1, 2, 42, 42, 42)
    x, y = HU.ct_like_volume(shape, 3), HU.smooth_volume(shape, 4)
    lab = np.random.default_rng(5).integers(0, 4, shape)
    xd, yd, ld = dev(x), dev(y), dev(lab, np.int32)
    for form in (1, 2, 3):
        with ops.config(hist_form=form):
            check_joint(ops.joint_histogram(xd, yd, bins=(64, 100)), x, y, (64, 100), None, form)
            check_joint(ops.joint_histogram(xd, xd, bins=(256, 256)), x, x, (256, 256), None, form)
            check_hist(ops.histogram(xd, 256, labels=ld, rows=3), x, 256, None, lab, 3, form)
    assert ops.get_config()["hist_form"] == 0


@pytest.mark.parametrize("bins", [7, 10])
def test_values_at_and_next_to_every_edge(bins):
    """edges of linspace(-1, 1, B + 1) are not fp32 numbers for B = 7, 10: every edge cast to fp32 and both fp32 neighbours, e_0 and e_B included"""
    from vae_segmentation_amd import ops
    probe = HU.edge_probe(-1.0, 1.0, bins)
    assert probe.min() < -1.0 and probe.max() > 1.0 and (probe == -1.0).any() and (probe == 1.0).any()
    x = np.resize(probe, (1, 1, 3, 5, 7))                            # 105 voxels: every probe value at least three times
    check_hist(ops.histogram(dev(x), bins, range=(-1.0, 1.0)), x, bins, (-1.0, 1.0), None, 0, bins)
    y = x[..., ::-1].copy()
    check_joint(ops.joint_histogram(dev(x), dev(y), bins=(bins, 17 - bins), range=((-1.0, 1.0), (-1.0, 1.0))), x, y, (bins, 17 - bins),
                ((-1.0, 1.0), (-1.0, 1.0)), bins)


def test_bounds_from_the_data():
    from vae_segmentation_amd import ops
    shape = (1, 3, 4, 6, 9)
    rng = np.random.default_rng(7)
    x = rng.normal(size=shape).astype(np.float32)
    x[0, 0] = 3.25                                                   # a constant plane: (v - 0.5, v + 0.5)
    x[0, 1].flat[:6] = [np.nan, np.inf, -np.inf, -np.nan, np.inf, np.nan]
    x[0, 2] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, shape[2:])]      # no finite voxel: (-0.5, 0.5), everything outside
    got = ops.histogram(dev(x), 8)
    check_hist(got, x, 8, None, None, 0, "from data")
    e = got["edges"].cpu().numpy()
    assert e[0, 0, 0] == 2.75 and e[0, 0, -1] == 3.75 and e[0, 2, 0] == -0.5 and e[0, 2, -1] == 0.5
    assert got["outside"].cpu().tolist() == [[0, 6, 4 * 6 * 9]] and int(got["table"][0, 2].sum()) == 0
    # host bounds: out-of-range and non-finite values land in `outside`
    check_hist(ops.histogram(dev(x), 5, range=(-0.5, 0.5)), x, 5, (-0.5, 0.5), None, 0, "host bounds")
    check_joint(ops.joint_histogram(dev(x), dev(x[:, ::-1].copy()), bins=(5, 9)), x, x[:, ::-1], (5, 9), None, "joint from data")
    # lo = -0.75, hi = 1.25, B = 7: fusing i * step + lo into one rounding changes e_5 (tests/test_host_hist.py finds it on the CPU)
    z = rng.uniform(-0.75, 1.25, (1, 1, 3, 5, 7)).astype(np.float32)
    z.flat[0], z.flat[-1] = -0.75, 1.25
    got = ops.histogram(dev(z), 7)
    assert np.array_equal(bits(got["edges"].cpu().numpy()[0, 0]), bits(np.linspace(-0.75, 1.25, 8)))
    check_hist(got, z, 7, None, None, 0, "unfused edges")


@pytest.mark.parametrize("rows", [1, 3, 2047])
def test_histogram_per_label(rows):
    from vae_segmentation_amd import ops
    shape = (2, 2, 9, 17, 33)
    rng = np.random.default_rng(rows)
    x = rng.normal(0, 0.5, shape).astype(np.float32)
    lab = rng.integers(0, rows + 1, shape)
    flat = lab.reshape(-1)
    flat[::97] = rows + 1 + flat[::97]                               # above rows
    flat[5::89] = -1 - flat[5::89]                                   # negative
    x.reshape(-1)[::97][:3] = np.nan                                 # a bad label wins over a bad value: overflow, and nowhere else
    for bins in (7, 256) if rows < 2047 else (7, 2048):             # 2048 rows x 2048 bins = 2^22 cells: the limit, global atomics
        check_hist(ops.histogram(dev(x), bins, labels=dev(lab, np.int32), rows=rows), x, bins, None, lab, rows, (rows, bins))
    with pytest.raises(ValueError, match="2\\^22"):
        ops.histogram(dev(x), 2049, labels=dev(lab, np.int32), rows=2047)
    with pytest.raises(ValueError, match="2\\^22"):
        ops.joint_histogram(dev(x), dev(x), bins=(2048, 2049))


def test_cc_label_output_as_labels():
    from vae_segmentation_amd import evaluation, ops
    shape = (1, 2, 16, 16, 40)
    x = HU.smooth_volume(shape, 9)
    mask = HU.smooth_volume(shape, 10) > 0.2
    labels, counts, _ = ops.cc_label(dev(mask), connectivity=26)
    rows = max(int(counts.max()), 1)
    got = ops.histogram(dev(x), 32, range=(-1.0, 1.0), labels=labels, rows=rows)
    check_hist(got, x, 32, (-1.0, 1.0), labels.cpu().numpy(), rows, "cc labels")
    assert int(got["overflow"].sum()) == 0
    # evaluation.histogram: a 0 / 1 mask is a label with one row
    rec = evaluation.histogram(dev(x[0, 0]), 32, range=(-1.0, 1.0), mask=dev(mask[0, 0]))
    want = HU.ref_histogram(x[0, 0], 32, (-1.0, 1.0), mask[0, 0].astype(int), 1)
    assert np.array_equal(rec["table"].cpu().numpy(), want["table"][1]) and np.array_equal(rec["complement"].cpu().numpy(), want["table"][0])
    assert int(rec["table"].sum()) == int(mask[0, 0].sum()) and rec["table"].shape == (32,)
    j = evaluation.joint_histogram(dev(x[0, 0]), dev(x[0, 1]), bins=16)
    assert np.array_equal(j["table"].cpu().numpy(), HU.ref_joint_histogram(x[0, 0], x[0, 1], (16, 16))["table"])


def mi_pairs(shape):
    a, b = HU.smooth_volume(shape, 31), HU.smooth_volume(shape, 32)
    ct = HU.ct_like_volume(shape, 33)
    return {"random": (a, b), "identical": (a, a), "shifted": (a, np.roll(a, 1, axis=-1)), "ct": (ct, (0.5 * ct + 0.1 * b).astype(np.float32))}


def test_mutual_information_matches_the_restatement():
    from vae_segmentation_amd import ops
    shape = (1, 1, 24, 24, 24)
    pairs = mi_pairs(shape)
    x = np.concatenate([p[0] for p in pairs.values()], 1)           # the four pairs as four planes of one call
    y = np.concatenate([p[1] for p in pairs.values()], 1)
    for bins in ((256, 256), (40, 23)):
        table = ops.joint_histogram(dev(x), dev(y), bins=bins)["table"]
        host = table.cpu().numpy()
        for sigma in (0, 1, 2.5):
            for normalized in (True, False):
                got = ops.mutual_information(table, sigma=sigma, normalized=normalized).cpu().numpy()
                assert got.shape == (1, 4) and got.dtype == np.float64
                for p, name in enumerate(pairs):
                    want = HU.ref_mutual_information(host[0, p], sigma, normalized)
                    print("mi %s bins %s sigma %s normalized %s: device %.17g restatement %.17g" % (name, bins, sigma, normalized, got[0, p], want))
                    assert abs(got[0, p] - want) <= 1e-9 * abs(want), (name, bins, sigma, normalized, got[0, p], want)
    same = ops.mutual_information(ops.joint_histogram(dev(x[:, :1]), dev(x[:, :1]))["table"], sigma=0, normalized=True)
    assert abs(float(same) - 1.0) <= 1e-9


def test_mutual_information_3d_on_a_non_cubic_pair():
    from vae_segmentation_amd import evaluation
    for name, (a, b) in mi_pairs((5, 40, 33)).items():
        for sigma, normalized in ((1, True), (0, False), (2.5, True)):
            got = evaluation.mutual_information_3d(dev(a), dev(b), sigma=sigma, normalized=normalized)
            want = HU.ref_mutual_information_3d(a, b, sigma, normalized)
            assert got.shape == () and got.dtype == torch.float64 and got.is_cuda
            assert abs(float(got) - want) <= 1e-9 * abs(want), (name, sigma, normalized, float(got), want)


def _all_results(x, y, lab):
    from vae_segmentation_amd import ops
    j = ops.joint_histogram(x, y)
    h = ops.histogram(x, 256, labels=lab, rows=3)
    big = ops.joint_histogram(x, y, bins=(512, 512), range=((-1.0, 1.0), (-1.0, 1.0)))
    mi = ops.mutual_information(j["table"], sigma=1.0)
    return [j["table"], j["edges_x"], j["edges_y"], j["outside"], h["table"], h["edges"], h["outside"], h["overflow"], big["table"], mi]


def _equal_bits(a, b):
    return all(torch.equal(p.view(torch.int64) if p.dtype == torch.float64 else p, q.view(torch.int64) if q.dtype == torch.float64 else q) for p, q in zip(a, b))


def test_both_builds_give_the_same_bits():
    from vae_segmentation_amd import ops
    shape = (1, 2, 20, 24, 36)
    x, y = dev(HU.ct_like_volume(shape, 41)), dev(HU.smooth_volume(shape, 42))
    lab = dev(np.random.default_rng(43).integers(0, 5, shape), np.int32)
    was = ops.is_deterministic()
    try:
        ops.set_deterministic(True)
        det = [t.clone() for t in _all_results(x, y, lab)]
        ops.set_deterministic(False)
        fast = _all_results(x, y, lab)
    finally:
        ops.set_deterministic(was)
    assert _equal_bits(det, fast)


def test_graph_replay_gives_the_bits_of_eager_calls():
    """one capture, three replays with the inputs changed in place between them, each against an eager call on the same inputs"""
    from vae_segmentation_amd import ops
    shape = (1, 2, 20, 24, 36)
    x, y = dev(HU.smooth_volume(shape, 51)), dev(HU.smooth_volume(shape, 52))
    lab = dev(np.random.default_rng(53).integers(0, 5, shape), np.int32)
    _all_results(x, y, lab)                                           # warm-up: workspaces exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = _all_results(x, y, lab)
    for k in range(3):
        x.copy_(dev(HU.ct_like_volume(shape, 60 + k) if k == 1 else HU.smooth_volume(shape, 60 + k)))
        y.mul_(0.5).add_(0.1 * k)
        lab.copy_((lab + k + 1) % 6 - 1)                              # some labels out of range
        for t in captured:
            t.view(torch.uint8).fill_(GARBAGE)                        # the replay writes every output whole
        g.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        assert _equal_bits(replayed, _all_results(x, y, lab)), k


def test_c_abi_writes_every_output_over_garbage():
    """the raw calls on caller buffers filled with 0x5A bytes: table, edges, outside, overflow are written whole, whatever they held"""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import check, lib
    shape = (1, 2, 9, 17, 33)
    x = HU.smooth_volume(shape, 71)
    x[0, 1].flat[:4] = np.nan
    xd = dev(x)

    def garbage(shape_, dtype):
        t = torch.empty(shape_, dtype=dtype, device="cuda")
        t.view(torch.uint8).fill_(GARBAGE)
        return t
    st = torch.cuda.current_stream().cuda_stream
    for from_data in (0, 1):
        table, edges = garbage((1, 2, 1, 7), torch.int64), garbage((1, 2, 8), torch.float64)
        outside, overflow = garbage((1, 2), torch.int64), garbage((1, 2), torch.int32)
        check(lib.vs_histogram(xd.data_ptr(), None, *shape, 7, 0, -1.0, 1.0, from_data, edges.data_ptr(), table.data_ptr(), outside.data_ptr(),
                               overflow.data_ptr(), st), "histogram")
        check_hist({"table": table, "edges": edges, "outside": outside, "overflow": overflow}, x, 7, None if from_data else (-1.0, 1.0), None, 0, from_data)
    want = ops.joint_histogram(xd, xd, bins=(256, 256))
    mi = garbage((1, 2), torch.float64)
    ws = garbage((2 * (2 * 256 * 256 + 3 * 256),), torch.float64)
    check(lib.vs_mutual_information(want["table"].data_ptr(), 1, 2, 256, 256, 1.0, 1, ws.data_ptr(), mi.data_ptr(), st), "mutual_information")
    assert torch.equal(mi.view(torch.int64), ops.mutual_information(want["table"], sigma=1.0).view(torch.int64))


def _run(args, cwd):
    out = subprocess.run([sys.executable, os.path.join(REPO, "main_source.py")] + args, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_entry_point_writes_intensity_json(tmp_path):
    """One synthetic validation epoch with --val_intensity 32 (the same untrained network is then evaluated without the flag from its checkpoint): the
    histograms sum to the voxel counts of the masks — the synthetic image lies in [-1, 1], nothing is outside — and without the flag no file is written."""
    from vae_segmentation_amd import driver
    common = ["--method", "seg_train", "--size", "64", "-b", "1", "-E", "1", "--eval_epoch", "1", "--save_epoch", "1", "--synthetic_train", "2", "--synthetic_val", "2",
              "--max_iters", "1", "--display_freq", "1"]
    out = _run(["run"] + common + ["--val_intensity", "32"], tmp_path)
    assert "Finished Training" in out and "validation intensities:" in out
    tb = tmp_path / "tensorboard" / "run"
    log = json.load(open(tb / "intensity_0.json"))
    assert sorted(log) == ["0", "1"] == sorted(json.load(open(tb / "score_0.json")))
    for entry in log.values():
        assert tuple(entry) == driver.INTENSITY_LOG_FIELDS and entry["bins"] == 32 and entry["range"] == [-1.0, 1.0]
        assert entry["pred_outside"] == 0 == entry["label_outside"]
        for side in ("pred", "label"):
            assert [len(h) for h in entry[side + "_hist"]] == [32] * len(entry[side + "_voxels"])
            assert [sum(h) for h in entry[side + "_hist"]] == entry[side + "_voxels"]
        assert sum(entry["label_voxels"]) > 0 and all(np.isfinite(v) for v in entry["nmi"])
    out = _run(["plain", "--test_only", "--load_prefix", "run", "--checkpoint_name", "model_epoch1.ckpt"] + common, tmp_path)
    assert "validation intensities:" not in out
    assert not (tmp_path / "tensorboard" / "plain" / "intensity_0.json").exists() and (tmp_path / "tensorboard" / "plain" / "score_0.json").exists()
