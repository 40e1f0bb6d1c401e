"""GPU: binary morphology and hole filling (csrc/morph.hip) against scipy.ndimage, bit for bit — the results are sets, there is no tolerance."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import morph_util as MU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a row that crosses a word boundary; less than a word and six planes; a single row of three words; exactly one word; one voxel past a word and past 64 rows
SHAPES = [(1, 1, 5, 7, 70), (2, 3, 9, 6, 37), (1, 1, 1, 1, 130), (1, 2, 33, 20, 64), (1, 1, 12, 65, 129)]
OPS = ("dilate", "erode", "open", "close")


def masks_of(shape):
    """name -> (N, C, D, H, W) bool: every plane of a tensor holds the same kind of mask with its own seed"""
    vol = shape[2:]
    planes = shape[0] * shape[1]

    def stack(fn):
        return np.stack([fn(p) for p in range(planes)]).reshape(shape)
    out = {"random%.2f" % dens: stack(lambda p, dens=dens: MU.random_mask(vol, dens, 100 * p + int(dens * 100))) for dens in (0.05, 0.5, 0.95)}
    out["empty"] = np.zeros(shape, bool)
    out["full"] = np.ones(shape, bool)
    out["corner"] = stack(lambda p: MU.corner_voxel(vol))
    out["block"] = stack(lambda p: MU.flush_block(vol))
    if planes > 1:                                       # planes must not bleed into each other: different kinds side by side
        kinds = [out["random0.50"], out["empty"], out["full"], out["corner"], out["block"], out["random0.05"]]
        out["mixed"] = np.stack([kinds[p % len(kinds)].reshape((planes,) + vol)[p] for p in range(planes)]).reshape(shape)
    return out


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_morphology_matches_scipy(shape):
    from vae_segmentation_amd import ops
    iters = (1, 2, 3, 9) if shape[2] == 5 else (1, 2, 3)           # 9 iterations on the depth-5 shape: beyond an axis
    runs = []
    for name, m in masks_of(shape).items():
        t = dev(m)
        for op, conn, it, border in itertools.product(OPS, (6, 26), iters, (0, 1)):
            runs.append(((name, op, conn, it, border), m, ops.morph(t, op, iterations=it, connectivity=conn, border_value=border)))
    got = torch.stack([r[2] for r in runs]).cpu().numpy()            # one copy and one synchronisation for the whole table
    assert set(np.unique(got)) <= {0.0, 1.0} and got.dtype == np.float32
    for (key, m, _), g in zip(runs, got):
        name, op, conn, it, border = key
        assert np.array_equal(g, MU.ref_morph(m, op, conn, it, border)), key


def test_morphology_of_a_full_cube_and_thresholding():
    from vae_segmentation_amd import evaluation, ops
    full = torch.ones(1, 1, 4, 4, 4, device="cuda")
    assert int(ops.binary_closing(full, connectivity=26).sum()) == 8 and int(ops.binary_opening(full, connectivity=26).sum()) == 64
    assert int(ops.binary_closing(full, connectivity=6).sum()) == 8 and int(ops.binary_closing(full, border_value=1).sum()) == 64
    # foreground is value >= 0.5; a (D, H, W) volume comes back as one
    v = torch.tensor([0.49999997, 0.5, 0.0, 0.0, 0.0, 1.0, float("nan")], device="cuda").view(1, 1, 7)
    out = evaluation.binary_dilation(v)
    assert out.shape == v.shape and out.view(-1).tolist() == [1, 1, 1, 0, 1, 1, 1]
    assert evaluation.binary_erosion(v, border_value=1).view(-1).tolist() == [0, 0, 0, 0, 0, 0, 0]
    assert evaluation.fill_holes(v).view(-1).tolist() == [0, 1, 0, 0, 0, 1, 0]
    big = torch.zeros(1, 1, 3, 3, 200, device="cuda")
    big[0, 0, 1, 1, 100] = 1
    assert int(ops.binary_dilation(big, iterations=10 ** 6, connectivity=6).sum()) == big.numel()        # capped where the plane is saturated
    assert int(ops.binary_dilation(big, iterations=70, connectivity=26).sum()) == 9 * 141


def fill_cases():
    out = [("shell", MU.shell()), ("shell_corner", MU.shell("corner")), ("shell_face", MU.shell("face")), ("open_hole", MU.open_hole((9, 9, 70))),
           ("nested", MU.nested_shells((14, 15, 70))), ("random", MU.random_mask((12, 11, 70), 0.55, 2)),
           ("random_b", MU.random_mask((7, 66, 129), 0.55, 3)), ("serpentine_open", MU.serpentine_background((17, 16, 70), True)),
           ("serpentine_closed", MU.serpentine_background((17, 16, 70), False)), ("empty", np.zeros((3, 4, 65), bool)), ("full", np.ones((3, 4, 65), bool)),
           ("row", MU.random_mask((1, 1, 130), 0.5, 4))]
    return out


@pytest.mark.parametrize("conn", [6, 26])
def test_fill_holes_matches_scipy(conn):
    from vae_segmentation_amd import evaluation, ops
    got = [(name, m, evaluation.fill_holes(dev(m), connectivity=conn)) for name, m in fill_cases()]
    filled = {}
    for name, m, g in got:
        g = g.cpu().numpy()
        assert g.shape == m.shape and np.array_equal(g, MU.ref_fill_holes(m, conn)), (name, conn)
        filled[name] = int(g.sum() - m.sum())
    assert filled["shell"] == 27 and filled["shell_face"] == 0 and filled["shell_corner"] == (27 if conn == 6 else 0)
    assert filled["random"] == (102 if conn == 6 else 0) and filled["open_hole"] == 0 and filled["nested"] > 0
    assert filled["serpentine_open"] == 0 and filled["serpentine_closed"] > 7 * 7 * 68
    # six planes side by side: each is its own problem
    planes = np.stack([MU.random_mask((9, 6, 37), 0.6, s) for s in range(5)] + [np.zeros((9, 6, 37), bool)]).reshape(2, 3, 9, 6, 37)
    planes[1, 2, 2:7, 1:5, 3:30] = True
    planes[1, 2, 3:6, 2:4, 5:28] = False
    g = ops.fill_holes(dev(planes), connectivity=conn).cpu().numpy()
    assert np.array_equal(g, MU.ref_fill_holes(planes, conn)) and g[1, 2].sum() == 5 * 4 * 27


def _graph_of(fn, buf):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(buf)                                                      # the workspaces exist before the capture starts
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn(buf)
    return graph, out


def test_graph_replay_equals_eager_launches():
    """captured once, replayed on new data: no allocation, synchronisation or host read-back inside a call"""
    from vae_segmentation_amd import ops
    shape = (2, 2, 12, 13, 70)
    inputs = [dev(MU.random_mask(shape, dens, 7 + i)) for i, dens in enumerate((0.02, 0.6, 0.9))]
    calls = {"close26": lambda x: ops.binary_closing(x, iterations=2, connectivity=26), "open6": lambda x: ops.binary_opening(x, iterations=3, border_value=1),
             "erode6": lambda x: ops.binary_erosion(x, iterations=2), "dilate26": lambda x: ops.binary_dilation(x, connectivity=26, border_value=1),
             "fill6": lambda x: ops.fill_holes(x), "fill26": lambda x: ops.fill_holes(x, connectivity=26)}
    for name, fn in calls.items():
        eager = [fn(x) for x in inputs]
        buf = torch.zeros(shape, device="cuda")
        graph, out = _graph_of(fn, buf)
        for x, want in zip(inputs, eager):
            buf.copy_(x)
            graph.replay()
            assert torch.equal(out, want), name
        assert not torch.equal(eager[0], eager[2]), name


def test_both_builds_give_identical_results():
    from vae_segmentation_amd import ops
    shape = (1, 2, 12, 65, 129)
    t = dev(MU.random_mask(shape, 0.55, 11))
    was = ops.is_deterministic()
    res = {}
    try:
        for det in (True, False):
            ops.set_deterministic(det)
            assert ops.is_deterministic() == det
            res[det] = [ops.morph(t, op, iterations=2, connectivity=conn, border_value=b) for op in OPS for conn in (6, 26) for b in (0, 1)]
            res[det] += [ops.fill_holes(t, connectivity=26)]
            res[det] += [ops.fill_holes(t, connectivity=6) for _ in range(4)]              # the last four: also the same from run to run
    finally:
        ops.set_deterministic(was)
    assert all(torch.equal(a, b) for a, b in zip(res[True], res[False]))
    assert all(torch.equal(res[True][-1], r) for r in res[True][-4:]) and res[True][-1].sum() > t.sum()


def test_synthesis_mask_matches_the_reference_restatement():
    from vae_segmentation_amd import evaluation
    hu = (np.random.RandomState(5).rand(24, 20, 70) * 1400 - 700).astype(np.float32)
    hu[np.random.RandomState(6).rand(24, 20, 70) < 0.9] *= 0.25                             # bone is sparse: most voxels within (-175, 175)
    d = evaluation.get_synthesis_mask({"venous": torch.from_numpy(hu).cuda()})
    got = d["venous_syn_mask"]
    assert got.dtype == torch.float32 and got.shape == hu.shape and set(d) == {"venous", "venous_syn_mask"}
    want = MU.ref_synthesis_mask(hu)
    assert np.array_equal(got.cpu().numpy(), want) and 0 < want.sum() < want.size
    d = evaluation.get_synthesis_mask({"arterial": torch.from_numpy(hu).cuda()}, field="arterial")
    assert np.array_equal(d["arterial_syn_mask"].cpu().numpy(), want)


def three_class_onehot():
    """(1, 3, 16, 18, 70): class 1 is a thick shell whose cavity holds class-2 voxels and background; class 2 has a blob of its own with a hole; specks"""
    lab = np.zeros((16, 18, 70), np.int64)
    lab[2:14, 2:16, 4:60] = 1
    lab[5:11, 5:13, 10:54] = 0
    lab[7:9, 7:10, 20:40] = 2
    lab[6, 6, 12] = 1
    lab[3:9, 3:9, 62:69] = 2
    lab[5, 5, 65] = 0
    lab[4, 4, 30] = 0                                                   # a one-voxel pore inside the class-1 wall
    lab[14, 16, 1] = 1                                                  # a speck the component filter removes
    return np.stack([lab == c for c in range(3)]).astype(np.float32)[None]


def test_postprocess_keeps_a_one_hot_tensor_one_hot():
    from vae_segmentation_amd import evaluation, ops
    hot = three_class_onehot()
    x = dev(hot)
    for closing, fill in ((0, True), (1, False), (2, True)):
        out = evaluation.postprocess(x, closing=closing, fill_holes=fill).cpu().numpy()
        assert np.array_equal(out.sum(1), np.ones_like(out[:, 0])) and set(np.unique(out)) <= {0.0, 1.0}
        assert np.array_equal(out, MU.ref_postprocess(hot, closing, fill)), (closing, fill)
        moved = (out != hot).any(1)
        assert moved.any() and ((hot[:, 0] == 1) | (out[:, 0] == 1))[moved].all()            # only voxels that are or become background move
        if closing == 0:
            assert (hot[:, 0] == 1)[moved].all() and (out[0, 2] >= hot[0, 2]).all()           # class 2 keeps its voxels inside class 1's cavity
            assert out[0, 1, 8, 8, 12] == 1 and out[0, 2, 8, 8, 30] == 1 and out[0, 2, 5, 5, 65] == 1
    assert torch.equal(x, dev(hot))
    # the component filter comes last; alone it is the driver's call
    both = evaluation.postprocess(x, closing=1, fill_holes=True, keep_largest=1)
    want = ops.keep_largest(dev(MU.ref_postprocess(hot, 1, True)), k=1, connectivity=26, lo_channel=1, to_background=True)
    assert torch.equal(both, want) and both[0, 1, 14, 16, 1] == 0 and both[0, 0, 14, 16, 1] == 1
    assert torch.equal(evaluation.postprocess(x, keep_largest=1, min_size=3),
                       ops.keep_largest(x, k=1, min_size=3, connectivity=26, lo_channel=1, to_background=True))


class _FixedPrediction(torch.nn.Module):
    def __init__(self, pred):
        super().__init__()
        self.pred = pred

    def forward(self, batch, img_key, out_key):
        return {out_key: self.pred}


def test_validate_with_closing_and_hole_filling(capsys):
    from vae_segmentation_amd import driver
    s = 32
    z, y, x = np.indices((s, s, s))
    blob = ((z - 16) ** 2 + (y - 15) ** 2 + (x - 17) ** 2) < 81
    holed = blob.copy()
    holed[15:18, 14:17, 16:19] = False                                  # a cavity
    holed[2, 3, 28] = True                                              # a speck
    label = torch.from_numpy(blob.astype(np.float32)).view(1, 1, s, s, s)
    p1 = torch.from_numpy(np.where(holed, 0.9, 0.1).astype(np.float32)).view(1, 1, s, s, s)
    model = _FixedPrediction(torch.cat([1 - p1, p1], 1).cuda())
    loader = [{driver.IMG_KEY: torch.zeros(1, 1, s, s, s), driver.LABEL_KEY: label}]
    raw = driver.validate("seg_train", model, loader, 2)
    assert raw[0] < 1.0 and driver.validate("seg_train", model, loader, 2, closing=0, fill_holes=False) == raw
    capsys.readouterr()
    filled = driver.validate("seg_train", model, loader, 2, fill_holes=True)
    assert raw[0] < filled[0] < 1.0 and "without the component filter: %f" % raw[0] in capsys.readouterr().out
    assert driver.validate("seg_train", model, loader, 2, fill_holes=True, keep_largest=1) == {0: 1.0}
    assert driver.validate("seg_train", model, loader, 2, closing=1, fill_holes=True, keep_largest=1)[0] > raw[0]


def test_entry_point_runs_with_the_new_flags(tmp_path):
    common = ["--size", "64", "-b", "1", "-E", "1", "--eval_epoch", "1", "--save_epoch", "1", "--synthetic_train", "2", "--synthetic_val", "1",
              "--max_iters", "2", "--display_freq", "1"]
    out = subprocess.run([sys.executable, os.path.join(REPO, "main_source.py"), "run", "--method", "seg_train", "--val_closing", "1", "--val_fill_holes",
                          "--val_keep_largest", "1", "--save_eval_result"] + common, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Finished Training" in out.stdout and "without the component filter" in out.stdout and "after closing 1 and hole filling on" in out.stdout
    assert json.load(open(tmp_path / "tensorboard" / "run" / "score_0.json"))
    cc = np.load(str(tmp_path / "result" / "run" / "0_0_pred_cc.npy"))
    assert cc.shape == (1, 2, 64, 64, 64) and np.array_equal(cc.sum(1), np.ones((1, 64, 64, 64), np.float32))          # still one-hot
    assert np.array_equal(MU.ref_fill_holes(cc[:, 1:], 6), cc[:, 1:])                                                # nothing left to fill
