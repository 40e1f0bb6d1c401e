"""GPU: per-component measurements, contingency tables, the confusion matrix and lesion-wise scores (csrc/regions.hip) against the scipy / numpy
restatement of tests/regions_util.py.  Everything the kernels produce is an integer: the yardstick is equality.  The centroid is one fp64 division
of two integers below 2^53 on both sides: 1e-12 relative covers a library difference in that division and nothing else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import regions_util as RU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# W past one wave and no multiple of it (runs cross wave and row boundaries), twice; six planes with tables of their own; odd throughout; one voxel
SHAPES = [(1, 1, 7, 9, 70), (1, 1, 5, 3, 129), (2, 3, 16, 16, 16), (1, 1, 33, 47, 29), (1, 1, 1, 1, 1)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
LDS_CELLS = 4096                 # csrc/regions.hip RG_LDS_CELLS: tables up to this many cells are summed in LDS


def dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def stack(shape, fn):
    """(N, C, D, H, W): every plane made by fn(plane index)"""
    return np.stack([fn(p) for p in range(shape[0] * shape[1])]).reshape(shape)


def check_props(got, labels, rows, what):
    """got: ops.region_props' dict on the host; labels (N, C, D, H, W) int"""
    for p, lab in enumerate(RU.planes_of(labels)):
        want = RU.ref_region_props(lab, rows)
        g = {k: v.reshape((-1,) + v.shape[2:])[p] for k, v in got.items()}
        assert np.array_equal(g["count"], want["count"]), what
        assert np.array_equal(g["bbox"], want["bbox"]) and g["bbox"].dtype == np.int32, what
        assert np.array_equal(g["sums"], want["sums"]) and int(g["overflow"]) == want["overflow"], what
        there = want["count"] > 0
        assert np.isnan(g["centroid"][~there]).all() and np.allclose(g["centroid"][there], want["centroid"][there], rtol=1e-12, atol=0), what
        d, h, w = lab.shape
        assert (g["bbox"][~there] == [d, h, w, -1, -1, -1]).all() and not g["sums"][~there].any(), what


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


RATIOS = ("sensitivity", "precision", "f1", "dice", "iou")


def same_record(got, want):
    """counts are equal; a ratio is one fp64 division of the same two integers on both sides: 1e-12 relative, as for the centroid"""
    assert sorted(got) == sorted(want)
    return all(np.allclose(got[k], want[k], rtol=1e-12, atol=0) if k in RATIOS else np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_region_props_match_the_restatement(shape):
    from vae_segmentation_amd import evaluation, ops
    vol = shape[2:]
    masks = {"blobs": (stack(shape, lambda p: RU.random_blobs(vol, 12, 50 + p)), 26), "faces": (stack(shape, lambda p: RU.touching_faces(vol)), 26),
             "checkerboard": (stack(shape, lambda p: RU.checkerboard(vol)), 6), "full": (np.ones(shape, bool), 26), "empty": (np.zeros(shape, bool), 26)}
    runs = []
    for name, (m, conn) in masks.items():
        labels, counts, _ = ops.cc_label(dev(m), connectivity=conn)
        k = max(int(counts.max()), 1)
        for rows in sorted({k + 3, max(k // 2, 1)}):                 # room to spare (absent rows), and more components than rows (overflow)
            runs.append((name, rows, labels, ops.region_props(labels, max_components=rows)))
    for name, rows, labels, got in runs:
        lab = labels.cpu().numpy()
        check_props(host(got), lab, rows, (name, rows))
        if name == "checkerboard" and lab.size > 1:
            assert lab.max() == (np.prod(vol) + 1) // 2 and (int(got["overflow"].sum()) > 0) == (rows < lab.max()), (name, rows)
    # the composed call: a (D, H, W) volume, spacing, volume in mm^3, the numbering of scipy.ndimage.label
    m = masks["blobs"][0][0, 0]
    sp = (2.5, 0.75, 1.25)
    got = host(evaluation.region_props(dev(m), spacing=sp, max_components=64))
    lab, k = RU.ref_label(m)
    want = RU.ref_region_props(lab, 64)
    assert np.array_equal(got["labels"], lab) and int(got["n_components"]) == k and np.array_equal(got["count"], want["count"])
    assert np.array_equal(got["volume"], want["count"] * (sp[0] * sp[1] * sp[2])) and np.array_equal(got["bbox"], want["bbox"])
    assert np.allclose(got["centroid"][:k], want["centroid"][:k] * np.array(sp), rtol=1e-12, atol=0) and np.isnan(got["centroid"][k:]).all()


def test_two_cubes_on_the_device():
    from vae_segmentation_amd import evaluation
    mask, want = RU.two_cubes()
    got = host(evaluation.region_props(dev(mask), max_components=3))
    for i, (count, box, centroid) in enumerate(want):
        assert got["count"][i] == count and tuple(got["bbox"][i]) == box and tuple(got["centroid"][i]) == centroid and got["volume"][i] == count
    assert got["count"][2] == 0 and got["bbox"][2].tolist() == [12, 10, 70, -1, -1, -1] and int(got["overflow"]) == 0 and int(got["n_components"]) == 2


def label_pairs(shape, rows_a, rows_b, seed):
    """name -> (a, b) int32 (N, C, D, H, W): blocky random label maps (runs along x), equal maps, and labels out of range on each side"""
    rs = np.random.RandomState(seed)

    def blocky(hi):
        coarse = rs.randint(0, hi + 1, size=shape[:2] + tuple((s + 2) // 3 for s in shape[2:]))
        fine = coarse.repeat(3, 2).repeat(3, 3).repeat(3, 4)[:, :, :shape[2], :shape[3], :shape[4]]
        return np.where(rs.rand(*shape) < 0.15, rs.randint(0, hi + 1, size=shape), fine).astype(np.int32)
    a, b = blocky(rows_a), blocky(rows_b)
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[rs.rand(*shape) < 0.1] = rows_a + 1
    bad_a[rs.rand(*shape) < 0.05] = -1
    bad_b[rs.rand(*shape) < 0.1] = rows_b + 7
    bad_b[rs.rand(*shape) < 0.05] = -(2 ** 31)
    same = blocky(min(rows_a, rows_b))
    return {"random": (a, b), "equal": (same, same), "out_of_range": (bad_a, bad_b)}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_contingency_matches_bincount(shape):
    from vae_segmentation_amd import ops
    V = int(np.prod(shape[2:]))
    # 3 x 3 cells and exactly LDS_CELLS take the LDS path; one cell more and 301 x 201 the global one
    sizes = [(2, 2), (63, 63), (63, 64), (300, 200)]
    assert 64 * 64 == LDS_CELLS and 64 * 65 > LDS_CELLS
    runs = []
    for ra, rb in sizes:
        for name, (a, b) in label_pairs(shape, ra, rb, ra + rb).items():
            ta, tb = dev(a, np.int32), dev(b, np.int32)
            runs.append(((ra, rb, name), a, b, ops.contingency(ta, ta if name == "equal" else tb, ra, rb)))
    for key, a, b, (table, overflow) in runs:
        ra, rb, name = key
        table, overflow = table.cpu().numpy(), overflow.cpu().numpy()
        assert table.shape == shape[:2] + (ra + 1, rb + 1) and table.dtype == np.int64 and overflow.dtype == np.int32
        for p, (pa, pb) in enumerate(zip(RU.planes_of(a), RU.planes_of(b))):
            want, over = RU.ref_contingency(pa, pb, ra, rb)
            got = table.reshape((-1,) + table.shape[2:])[p]
            assert np.array_equal(got, want) and int(overflow.reshape(-1)[p]) == over, key
            assert got.sum() == V - over, key
            if name == "out_of_range" and V > 20:
                assert over > 0, key
            if name == "equal":
                assert over == 0 and not got[~np.eye(ra + 1, rb + 1, dtype=bool)].any(), key


def lesion_pairs():
    """(name, pred, gt) (D, H, W) bool masks: the host test's scene, random multi-lesion pairs, and the empty cases"""
    pred, gt, _ = RU.lesion_scene()
    out = [("scene", pred, gt)]
    for seed, shape in ((1, (7, 9, 70)), (2, (33, 47, 29)), (3, (16, 16, 16))):
        g = RU.random_blobs(shape, 14, seed, radius=(0.8, 2.5))
        p = np.roll(g, 1, axis=2) & (RU.random_blobs(shape, 40, seed + 10) | RU.checkerboard(shape)) | RU.random_blobs(shape, 5, seed + 20, radius=(0.8, 2.0))
        out.append(("random%d" % seed, p, g))
    empty, one = np.zeros((3, 4, 5), bool), np.zeros((3, 4, 5), bool)
    one[1, 1, 1:3] = True
    out += [("empty_empty", empty, empty), ("empty_pred", empty, one), ("empty_gt", one, empty), ("same", one, one), ("voxel", np.ones((1, 1, 1), bool), np.ones((1, 1, 1), bool))]
    return out


def test_lesion_metrics_match_the_restatement():
    from vae_segmentation_amd import evaluation
    _, _, stated = RU.lesion_scene()
    runs = []
    for name, p, g in lesion_pairs():
        for conn, min_overlap, min_size in ((26, 1, 0), (26, 3, 0), (26, 1, 2), (26, 2, 2), (26, 3, 2), (6, 2, 3)):
            runs.append(((name, conn, min_overlap, min_size), p, g,
                         evaluation.lesion_metrics(dev(p), dev(g), connectivity=conn, min_overlap=min_overlap, min_size=min_size)))
    for key, p, g, rec in runs:
        name, conn, min_overlap, min_size = key
        assert tuple(rec) == evaluation.LESION_RECORD_FIELDS
        got = evaluation.lesion_record_to_host(rec)
        want = RU.ref_lesion(p, g, connectivity=conn, min_overlap=min_overlap, min_size=min_size)
        assert same_record(got, want), (key, got, want)
        if name == "scene" and conn == 26:
            assert tuple(got[k] for k in ("n_gt", "n_pred", "tp", "fn", "fp")) == stated[(min_overlap, min_size)]
    # planes are independent problems, and a table too small for a plane's components says so
    names = [n for n, _, _ in lesion_pairs()]
    p, g = lesion_pairs()[names.index("random3")][1:]
    pp, gg = np.stack([p, g, np.zeros_like(p), p]).reshape((2, 2) + p.shape), np.stack([g, g, g, np.zeros_like(g)]).reshape((2, 2) + g.shape)
    rec = evaluation.lesion_metrics(dev(pp), dev(gg), min_size=2)
    got = evaluation.lesion_record_to_host(rec)
    for i, (a, b) in enumerate(zip(RU.planes_of(pp), RU.planes_of(gg))):
        want = RU.ref_lesion(a, b, min_size=2)
        assert same_record({k: got[k][i // 2][i % 2] for k in got}, want), i
    small = evaluation.lesion_metrics(dev(p), dev(g), max_components=2)
    assert int(small["overflow"]) > 0
    with pytest.raises(RuntimeError, match="beyond the table"):
        evaluation.lesion_record_to_host(small)


def test_confusion_matches_the_restatement():
    from vae_segmentation_amd import evaluation
    pred, gt, table = RU.three_class_pair()
    cases = [("stated", pred, gt, 3), ("stated4", pred, gt, 4), ("stated2", pred, gt, 2), ("one_class", np.zeros((2, 3, 4), int), np.zeros((2, 3, 4), int), 1)]
    rs = np.random.RandomState(9)
    for i, shape in enumerate(((7, 9, 70), (33, 47, 29))):
        cases.append(("random%d" % i, rs.randint(0, 5, size=shape), rs.randint(0, 4, size=shape), 5))
    runs = [(name, p, g, k, evaluation.confusion(dev(p, np.int64), dev(g, np.float32 if name == "stated" else np.uint8), k)) for name, p, g, k in cases]
    for name, p, g, k, got in runs:
        got, want = host(got), RU.ref_confusion(p, g, k)
        assert np.array_equal(got["table"], want["table"]) and int(got["overflow"]) == want["overflow"], name
        assert same_record(got, want) and all(got[key].dtype == np.float64 for key in ("dice", "iou", "sensitivity", "precision")), name
        if name == "stated":
            assert np.array_equal(got["table"], table)
        if name == "stated2":
            assert int(got["overflow"]) == 4
    batched = evaluation.confusion(dev(np.stack([pred, gt]).reshape(2, 1, 1, 3, 4), np.int32), dev(np.stack([gt, gt]).reshape(2, 1, 1, 3, 4), np.int32), 3)
    assert np.array_equal(batched["table"][0, 0].cpu().numpy(), table) and batched["dice"][1, 0].tolist() == [1.0, 1.0, 1.0]


def _graph_of(fn, *bufs):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(*bufs)                                                    # the workspaces exist before the capture starts
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one capture, one stream: no parallel branches
        out = fn(*bufs)
    return graph, out


def _flat(out):
    """every tensor of a result (dict, tuple or tensor) in a fixed order"""
    if isinstance(out, dict):
        return [out[k] for k in sorted(out)]
    return list(out) if isinstance(out, (tuple, list)) else [out]


def _same(xs, ys):
    return len(xs) == len(ys) and all(x.dtype == y.dtype and torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)) for x, y in zip(xs, ys))


def test_results_are_the_same_bits_in_both_builds_and_under_graph_replay():
    from vae_segmentation_amd import evaluation, ops
    shape = (2, 2, 12, 13, 70)
    g = stack(shape, lambda p: RU.random_blobs(shape[2:], 10, 30 + p))
    p = np.roll(g, 2, axis=4) | stack(shape, lambda q: RU.random_blobs(shape[2:], 3, 60 + q))
    mp, mg = dev(p), dev(g)
    labels = ops.cc_label(mp)[0]
    other = ops.cc_label(mg)[0]
    calls = {"props": (lambda a, b: ops.region_props(a, max_components=9), (labels, other)),
             "contingency_lds": (lambda a, b: ops.contingency(a, b, 20, 20), (labels, other)),
             "contingency_global": (lambda a, b: ops.contingency(a, b, 100, 90), (labels, other)),
             "lesion": (lambda a, b: evaluation.lesion_metrics(a, b, min_size=2, min_overlap=2), (mp, mg)),
             "confusion": (lambda a, b: evaluation.confusion(a, b, 3), (labels.clamp(max=3), other.clamp(max=2)))}
    was = ops.is_deterministic()
    res = {}
    try:
        for det in (True, False):
            ops.set_deterministic(det)
            assert ops.is_deterministic() == det
            res[det] = {name: _flat(fn(*args)) for name, (fn, args) in calls.items()}
            res[det, "again"] = {name: _flat(fn(*args)) for name, (fn, args) in calls.items()}
    finally:
        ops.set_deterministic(was)
    for name in calls:
        assert _same(res[True][name], res[False][name]) and _same(res[True][name], res[True, "again"][name]), name
        assert _same(res[False][name], res[False, "again"][name]), name
    # one replay of a captured call on new data against the eager call on that data
    for name, (fn, args) in calls.items():
        bufs = [torch.zeros_like(a) for a in args]
        graph, out = _graph_of(fn, *bufs)
        for buf, a in zip(bufs, args):
            buf.copy_(a)
        graph.replay()
        assert _same(_flat(out), _flat(fn(*args))), name
    assert int(res[True]["props"][_flat_index("count")].sum()) > 0


def _flat_index(key, keys=("bbox", "centroid", "count", "overflow", "sums")):
    return sorted(keys).index(key)


class _FixedPredictions(torch.nn.Module):
    """a segmentation network that answers case after case from a list"""

    def __init__(self, preds):
        super().__init__()
        self.preds, self.i = preds, 0

    def forward(self, batch, img_key, out_key):
        self.i += 1
        return {out_key: self.preds[(self.i - 1) % len(self.preds)]}


def test_validate_with_lesion_records(capsys):
    from vae_segmentation_amd import driver, evaluation
    pred, gt, stated = RU.lesion_scene()
    cases = [(pred, gt), (gt, gt)]
    s = pred.shape
    preds, loader = [], []
    for p, g in cases:
        p1 = torch.from_numpy(np.where(p, 0.9, 0.1).astype(np.float32)).view((1, 1) + s)
        preds.append(torch.cat([1 - p1, p1], 1).cuda())
        loader.append({driver.IMG_KEY: torch.zeros((1, 1) + s), driver.LABEL_KEY: torch.from_numpy(g.astype(np.float32)).view((1, 1) + s)})
    plain = driver.validate("seg_train", _FixedPredictions(preds), loader, 2)
    log = {}
    capsys.readouterr()
    scores = driver.validate("seg_train", _FixedPredictions(preds), loader, 2, lesion=True, lesion_log=log)
    assert scores == plain and sorted(log) == [0, 1] and "validation lesions: 8 of 10 reference lesions detected, 2 false detections" in capsys.readouterr().out
    for i, (p, g) in enumerate(cases):
        assert tuple(log[i]) == driver.LESION_LOG_FIELDS
        want = RU.ref_lesion(p, g)
        assert same_record({k: log[i][k] for k in evaluation.LESION_RECORD_FIELDS}, {k: [v] for k, v in want.items()})
        conf = RU.ref_confusion(p.astype(int), g.astype(int), 2)
        assert same_record({k: log[i][k] for k in ("dice", "iou")}, {k: conf[k] for k in ("dice", "iou")}) and log[i]["confusion_overflow"] == 0
        assert np.allclose(log[i]["class_sensitivity"], conf["sensitivity"], rtol=1e-12, atol=0)
        assert np.allclose(log[i]["class_precision"], conf["precision"], rtol=1e-12, atol=0)
        assert abs(log[i]["dice"][1] - scores[i]) < 1e-5              # validation's Dice carries eps = 1e-6 in numerator and denominator
    assert tuple(log[0][k][0] for k in ("n_gt", "n_pred", "tp", "fn", "fp")) == stated[(1, 0)]
    log2 = {}
    driver.validate("seg_train", _FixedPredictions(preds), loader, 2, lesion=True, lesion_log=log2, min_component=2)
    assert tuple(log2[0][k][0] for k in ("n_gt", "n_pred", "tp", "fn", "fp")) == stated[(1, 2)]
    json.dumps(log)


def _run(args, cwd):
    out = subprocess.run([sys.executable, os.path.join(REPO, "main_source.py")] + args, cwd=str(cwd), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_entry_point_writes_lesion_json(tmp_path):
    """A tiny seg_train run with --val_lesion.  The entry points take no seed (initialisation and loader order differ from process to process), so "the same
    run without the flag" is made the same by evaluating the first run's checkpoint with --test_only, once with the flag and once without."""
    from vae_segmentation_amd import driver
    common = ["--method", "seg_train", "--size", "64", "-b", "1", "-E", "1", "--eval_epoch", "1", "--save_epoch", "1", "--synthetic_train", "2", "--synthetic_val", "2",
              "--max_iters", "2", "--display_freq", "1", "--val_keep_largest", "3"]
    # the component filter bounds the prediction's components: an untrained network's speckle can exceed the lesion table, which is an error

    def check_log(tb):
        log, scores = json.load(open(tb / "lesion_0.json")), json.load(open(tb / "score_0.json"))
        assert sorted(log) == ["0", "1"] == sorted(scores)
        for i in log:
            assert tuple(log[i]) == driver.LESION_LOG_FIELDS and log[i]["overflow"] == [0]
            assert abs(log[i]["dice"][1] - scores[i]) < 1e-5
            assert log[i]["tp"][0] + log[i]["fn"][0] == log[i]["n_gt"][0] and 0 <= log[i]["fp"][0] <= log[i]["n_pred"][0]
        return scores

    out = _run(["run"] + common + ["--val_lesion"], tmp_path)
    assert "Finished Training" in out and "validation lesions:" in out
    check_log(tmp_path / "tensorboard" / "run")
    # the same network evaluated with and without the flag
    outs = {name: _run([name, "--test_only", "--load_prefix", "run", "--checkpoint_name", "model_epoch1.ckpt"] + common + extra, tmp_path)
            for name, extra in (("with", ["--val_lesion"]), ("without", []))}
    tb = {name: tmp_path / "tensorboard" / name for name in outs}
    scores = check_log(tb["with"])
    assert "validation lesions:" in outs["with"] and "validation lesions:" not in outs["without"]
    assert not (tb["without"] / "lesion_0.json").exists()
    assert sorted(os.listdir(tb["without"])) == sorted(f for f in os.listdir(tb["with"]) if f != "lesion_0.json")
    assert json.load(open(tb["without"] / "score_0.json")) == scores

    def results(text):
        return [l for l in text.splitlines() if "validation" in l and not l.startswith("validation lesions:")]
    assert results(outs["with"]) == results(outs["without"]) and len(results(outs["with"])) >= 2
