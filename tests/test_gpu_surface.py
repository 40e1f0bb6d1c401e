"""GPU: surface extraction, the exact Euclidean distance transform and the surface-distance metrics (csrc/surface.hip, ops.surface / ops.edt /
ops.surface_distances, evaluation.surface_metrics, --val_surface) against the scipy restatement of tests/surface_util.py.  Masks, counts and
squared distances are compared exactly; the floating-point fields to the rounding bounds stated at each check."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import surface_util as SU
from tests.test_gpu_cc import serpentine, shells, smooth_noise, structured_cases

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
both_libs = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)

SHAPES = [(5, 6, 7), (33, 17, 65), (1, 1, 300), (64, 64, 64), (96, 96, 96), (128, 128, 128), (40, 200, 72)]
SPACING = (2.5, 0.8, 0.8)
FEATURES = ("single", "corners", "checkerboard", "full", "sparse", "noise", "empty")
_MEMO = {}                      # the oracle of a case, shared by the two library builds


def feature_sets(shape):
    """-> bool (7, D, H, W) in the order of FEATURES"""
    rng = np.random.RandomState(sum(shape))
    out = []
    m = np.zeros(shape, bool)
    m[tuple(rng.randint(0, s) for s in shape)] = True
    out.append(m)
    m = np.zeros(shape, bool)
    for z in (0, shape[0] - 1):
        for y in (0, shape[1] - 1):
            for x in (0, shape[2] - 1):
                m[z, y, x] = True
    out.append(m)
    z, y, x = np.indices(shape)
    out.append((z + y + x) % 2 == 0)
    out.append(np.ones(shape, bool))
    m = rng.rand(*shape) < min(0.5, 20.0 / np.prod(shape))
    m[tuple(rng.randint(0, s) for s in shape)] = True
    out.append(m)
    noise = smooth_noise(shape, seed=sum(shape) + 1)
    out.append(noise >= np.float32(np.quantile(noise, 0.97)))
    out.append(np.zeros(shape, bool))
    return np.stack(out)


def oracle_edt(shape, spacing):
    key = ("edt", shape, spacing)
    if key not in _MEMO:
        _MEMO.clear()
        _MEMO[key] = [SU.edt(f, spacing) for f in feature_sets(shape)[:-1]]
    return _MEMO[key]


def cuda5(x):
    """bool / float (D, H, W) or (P, D, H, W) -> fp32 (1, P, D, H, W) on the device"""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 3:
        x = x[None]
    return torch.from_numpy(np.ascontiguousarray(x[None])).cuda()


ids = lambda s: "x".join(map(str, s))


@both_libs
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_edt_squared_is_exact(lib_mode, shape):
    from vae_segmentation_amd import ops
    feats = feature_sets(shape)
    got = ops.edt(cuda5(feats), squared=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (1, len(FEATURES)) + shape
    got = got[0].cpu().numpy()
    for name, g, (sq_int, _) in zip(FEATURES, got, oracle_edt(shape, None)):
        assert np.array_equal(g, sq_int), (name, shape, int((g != sq_int).sum()))
    assert (got[FEATURES.index("full")] == 0).all()
    assert (got[-1] == SU.INT_SENTINEL).all()                      # the definition: no feature voxel in the plane
    # the fp64 forms of the same call
    dist = ops.edt(cuda5(feats[:2]))[0].cpu().numpy()
    assert dist.dtype == np.float64 and np.array_equal(dist, np.sqrt(got[:2].astype(np.float64)))
    assert torch.isinf(ops.edt(cuda5(feats[-1:]))).all()


@both_libs
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_edt_with_spacing(lib_mode, shape):
    """fp64 squared distances against sum((s * offset)^2) formed in fp64 from the oracle's nearest-voxel indices.  rtol 1e-12: both sides
    round three products, three squares and two additions at most once each — eight roundings of 2^-53 ~ 9e-16 — and a different but equally
    near feature voxel may be chosen."""
    from vae_segmentation_amd import ops
    feats = feature_sets(shape)
    got = ops.edt(cuda5(feats), spacing=SPACING, squared=True)
    assert got.dtype == torch.float64
    got = got[0].cpu().numpy()
    for name, g, (_, sq) in zip(FEATURES, got, oracle_edt(shape, SPACING)):
        err = np.abs(g - sq) / np.maximum(sq, 1e-300)
        assert np.all((g == sq) | (err <= 1e-12)), (name, shape, float(err.max()))
    assert np.isinf(got[-1]).all() and (got[-1] > 0).all()
    root = ops.edt(cuda5(feats[:1]), spacing=SPACING)[0, 0].cpu().numpy()
    assert np.array_equal(root, np.sqrt(got[0]))


def surface_masks():
    out = [(name, m) for name, m in structured_cases()]
    for shape in ((5, 6, 7), (33, 17, 65), (1, 1, 300), (40, 44, 72)):
        for name, f in zip(FEATURES, feature_sets(shape)):
            out.append(("%s%s" % (name, shape), f))
        noise = smooth_noise(shape, seed=11)
        out.append(("dense_noise%s" % (shape,), noise >= np.float32(np.quantile(noise, 0.4))))
    out.append(("shells_big", shells((40, 42, 140))))
    out.append(("serpentine_big", serpentine((20, 30, 200))))
    return out


@both_libs
@pytest.mark.parametrize("conn", [6, 26])
def test_surface_equals_the_erosion_surface(lib_mode, conn):
    from vae_segmentation_amd import ops
    for name, m in surface_masks():
        got = ops.surface(cuda5(m), connectivity=conn)
        assert got.dtype == torch.float32
        assert np.array_equal(got[0, 0].cpu().numpy(), SU.surface(m, conn).astype(np.float32)), (name, conn)
    # the binarisation threshold, and the default connectivity
    vals = np.random.RandomState(5).choice(np.array([0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.51, -1.0, 2.0], dtype=np.float32), size=(9, 10, 66))
    assert np.array_equal(ops.surface(cuda5(vals), connectivity=conn)[0, 0].cpu().numpy(), SU.surface(vals >= 0.5, conn).astype(np.float32))
    assert torch.equal(ops.surface(cuda5(vals)), ops.surface(cuda5(vals), connectivity=6))


def organ(s, shift=(0, 0, 0), scale=1.0):
    """a clean ellipsoid, one component, away from the border"""
    ax = np.arange(s, dtype=np.float64)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    c = (s - 1) / 2
    r = ((z - c - shift[0]) / (0.30 * s * scale)) ** 2 + ((y - c - shift[1]) / (0.22 * s * scale)) ** 2 + ((x - c - shift[2]) / (0.34 * s * scale)) ** 2
    return r < 1.0


def organ_with_specks(s, seed=7):
    """a prediction: the organ a little displaced and swollen, plus 0.1 % stray voxels"""
    return organ(s, shift=(1, -2, 1), scale=1.03) | (np.random.RandomState(seed).rand(s, s, s) < 1e-3)


def run_distances(a, b, spacing=None, conn=6):
    """a, b: bool (D, H, W) or (P, D, H, W) -> list over planes of {field: python number}"""
    from vae_segmentation_amd import ops
    rec = ops.surface_distances(cuda5(a), cuda5(b), spacing=spacing, connectivity=conn)
    assert tuple(rec) == SU.FIELDS or set(rec) == set(SU.FIELDS)
    assert rec["count_ab"].dtype == torch.int64 and rec["assd"].dtype == torch.float64
    host = {k: v.cpu().numpy().reshape(-1) for k, v in rec.items()}
    return [{k: host[k][p].item() for k in SU.FIELDS} for p in range(host["assd"].size)]


def assert_record(got, want, spacing, what):
    """counts and — for unit spacing — the squared statistics exactly; the fp64 fields to rtol 1e-9, the worst case of a plain fp64 sum over at
    most 2^23 terms of relative error 2^-53 each (2^23 * 2^-53 ~ 9.3e-10), which also covers the square roots and the interpolation.
    With a spacing the squared statistics are doubles formed in another order than the oracle's: rtol 1e-12 (see test_edt_with_spacing)."""
    print(what, "device", got, "oracle", want)
    assert got["count_ab"] == want["count_ab"] and got["count_ba"] == want["count_ba"], what
    if want["count_ab"] == 0:
        assert all(math.isnan(got[k]) for k in SU.FIELDS[2:]), (what, got)
        return
    for k in ("max_sq", "lo_sq", "hi_sq"):
        if spacing is None:
            assert got[k] == want[k] and float(got[k]).is_integer(), (what, k, got[k], want[k])
        else:
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), (what, k, got[k], want[k])
    for k in ("sum_ab", "sum_ba", "assd", "hd", "hd95"):
        assert got[k] == pytest.approx(want[k], rel=1e-9, abs=0), (what, k, got[k], want[k])


def check_pair(a, b, spacing=None, conn=6, what=""):
    got = run_distances(a, b, spacing, conn)
    a4, b4 = (np.asarray(x)[None] if np.asarray(x).ndim == 3 else np.asarray(x) for x in (a, b))
    wants = [SU.metrics(x, y, spacing, conn) for x, y in zip(a4, b4)]
    for p, (g, w) in enumerate(zip(got, wants)):
        assert_record(g, w, spacing, "%s plane %d conn %d spacing %s" % (what, p, conn, spacing))
    return got, wants


@both_libs
def test_hand_derived_cases(lib_mode):
    got, _ = check_pair(*SU.two_voxels(), what="two voxels")
    assert got[0]["assd"] == 5.0 and got[0]["hd"] == 5.0 and got[0]["hd95"] == 5.0 and got[0]["max_sq"] == 25
    a, _ = SU.shifted_cubes()
    got, _ = check_pair(a, a.copy(), what="identical")
    assert got[0]["assd"] == 0.0 and got[0]["hd"] == 0.0 and got[0]["hd95"] == 0.0 and got[0]["count_ab"] == 56
    got, _ = check_pair(*SU.shifted_cubes(4, 6), what="shifted cubes")
    assert (got[0]["sum_ab"], got[0]["sum_ba"], got[0]["assd"], got[0]["hd"], got[0]["hd95"]) == (252.0, 252.0, 4.5, 6.0, 6.0)
    got, _ = check_pair(*SU.shifted_cubes(4, 5), conn=26, what="shifted cubes 26")
    assert (got[0]["assd"], got[0]["hd"], got[0]["hd95"]) == (3.5, 5.0, 5.0)
    got, _ = check_pair(*SU.anisotropic(), spacing=SU.ANISO_SPACING, what="anisotropic")
    assert got[0]["assd"] == pytest.approx(1.825, rel=1e-12) and got[0]["hd"] == pytest.approx(2.5, rel=1e-12)
    assert got[0]["hd95"] == pytest.approx(2.41, rel=1e-12)
    check_pair(*SU.anisotropic(), what="anisotropic masks, unit spacing")


@both_libs
@pytest.mark.parametrize("side", [96, 128])
def test_organ_with_specks_against_a_clean_organ(lib_mode, side):
    pred, label = organ_with_specks(side), organ(side)
    key = ("organ", side)
    got = run_distances(np.stack([pred, label]), np.stack([label, pred]))
    if key not in _MEMO:
        _MEMO.clear()
        _MEMO[key] = [SU.metrics(pred, label), SU.metrics(label, pred)]
    for p, (g, w) in enumerate(zip(got, _MEMO[key])):
        assert_record(g, w, None, "organ %d plane %d" % (side, p))
    assert got[0]["hd"] > 3 * got[0]["assd"] > 0                 # the specks dominate the maximum, hardly the mean
    assert got[0]["count_ab"] == got[1]["count_ba"] and got[0]["max_sq"] == got[1]["max_sq"] and got[0]["hd95"] == got[1]["hd95"]


@both_libs
def test_noise_border_batches_and_both_connectivities(lib_mode):
    shape = (40, 44, 72)
    n1, n2 = smooth_noise(shape, 21), smooth_noise(shape, 22)
    a, b = n1 >= np.float32(np.quantile(n1, 0.7)), n2 >= np.float32(np.quantile(n2, 0.75))
    border = np.zeros(shape, bool)
    border[0:9, 0:20, 50:72] = True                                 # touches three faces of the volume: the border counts as background
    inner = np.zeros(shape, bool)
    inner[2:12, 3:18, 45:70] = True
    for conn in (6, 26):
        check_pair(a, b, conn=conn, what="noise")
        check_pair(border, inner, conn=conn, what="border")
        # different content per plane, an odd plane size next to it (alignment of the planes' lists)
        check_pair(np.stack([a, border, inner, b, a]), np.stack([b, inner, inner, b, border]), conn=conn, what="batch")
    check_pair(a, b, spacing=SPACING, what="noise")
    check_pair(np.stack([border, a]), np.stack([inner, b]), spacing=(1.0, 1.0, 1.0), what="unit spacing given")
    odd = (11, 13, 67)
    o1, o2 = smooth_noise(odd, 31) >= 0.5, smooth_noise(odd, 32) >= 0.51
    check_pair(np.stack([o1, o2, o1]), np.stack([o2, o1, o1]), what="odd planes")
    check_pair(np.stack([o1, o2, o1]), np.stack([o2, o1, o1]), spacing=SPACING, conn=26, what="odd planes")
    # the evaluation wrappers: a single volume gives scalars
    from vae_segmentation_amd import evaluation
    ta, tb = torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()
    want = SU.metrics(a, b)
    m = evaluation.surface_metrics(ta, tb)
    assert m["assd"].shape == () and m["count_ab"].item() == want["count_ab"]
    assert evaluation.assd(ta, tb).item() == pytest.approx(want["assd"], rel=1e-9)
    assert evaluation.hd(ta, tb).item() == pytest.approx(want["hd"], rel=1e-9)
    assert evaluation.hd95(ta, tb).item() == pytest.approx(want["hd95"], rel=1e-9)
    assert evaluation.hd95(ta[None, None], tb[None, None], spacing=SPACING, connectivity=26).shape == (1, 1)


@both_libs
def test_empty_surfaces_are_nan_and_leave_other_planes_alone(lib_mode):
    shape = (12, 14, 66)
    x = smooth_noise(shape, 41) >= 0.5
    y = smooth_noise(shape, 42) >= 0.5
    zero = np.zeros(shape, bool)
    for spacing in (None, SPACING):
        got, wants = check_pair(np.stack([x, zero, x, zero, y]), np.stack([y, x, zero, zero, x]), spacing=spacing, what="empties")
        assert [g["count_ab"] for g in got][1:4] == [0, 0, 0] and got[0]["count_ab"] > 0 and got[4]["count_ab"] > 0
        assert all(math.isnan(got[p]["hd95"]) and math.isnan(got[p]["assd"]) and math.isnan(got[p]["hd"]) for p in (1, 2, 3))
        alone = run_distances(x, y, spacing)[0]
        assert alone == got[0]                                      # bit for bit what the plane gives on its own


def test_two_calls_are_bit_identical_on_the_deterministic_library():
    from vae_segmentation_amd import ops
    assert ops.is_deterministic()
    pred, label = cuda5(np.stack([organ_with_specks(96), organ(96)])), cuda5(np.stack([organ(96), organ_with_specks(96, 8)]))
    for spacing in (None, SPACING):
        first = ops.surface_distances(pred, label, spacing=spacing)
        first = {k: v.clone() for k, v in first.items()}
        again = ops.surface_distances(pred, label, spacing=spacing)
        for k in SU.FIELDS:
            assert torch.equal(first[k].view(torch.int64), again[k].view(torch.int64)), (k, spacing)


def test_both_builds_give_identical_records():
    from vae_segmentation_amd import ops
    pred, label = cuda5(organ_with_specks(96)), cuda5(organ(96))
    was = ops.is_deterministic()
    res = {}
    try:
        for det in (True, False):
            ops.set_deterministic(det)
            rec = ops.surface_distances(pred, label)
            res[det] = {k: v.clone() for k, v in rec.items()}, ops.edt(pred, squared=True), ops.edt(pred, spacing=SPACING, squared=True)
    finally:
        ops.set_deterministic(was)
    for k in SU.FIELDS:
        assert torch.equal(res[True][0][k].view(torch.int64), res[False][0][k].view(torch.int64)), k
    assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])


@both_libs
def test_surface_distances_in_a_captured_graph(lib_mode):
    """captured once on zero buffers, replayed after the buffers were overwritten: no allocation, synchronisation or host read-back inside"""
    from vae_segmentation_amd import ops
    shape = (2, 40, 44, 72)
    pairs = []
    for i in range(2):
        n1, n2 = smooth_noise(shape, 70 + i), smooth_noise(shape, 80 + i)
        pairs.append((n1 >= np.float32(0.5 + 0.01 * i), n2 >= np.float32(0.505)))
    for spacing in (None, SPACING):
        buf_a, buf_b = torch.zeros((1,) + shape, device="cuda"), torch.zeros((1,) + shape, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.surface_distances(buf_a, buf_b, spacing=spacing)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = ops.surface_distances(buf_a, buf_b, spacing=spacing)
        graph.replay()
        torch.cuda.synchronize()
        assert rec["count_ab"].sum().item() == 0 and torch.isnan(rec["hd95"]).all()
        for a, b in pairs:
            buf_a.copy_(cuda5(a))
            buf_b.copy_(cuda5(b))
            graph.replay()
            host = {k: v.cpu().numpy().reshape(-1) for k, v in rec.items()}
            for p in range(2):
                assert_record({k: host[k][p].item() for k in SU.FIELDS}, SU.metrics(a[p], b[p], spacing), spacing, "replay plane %d" % p)
        del graph


@both_libs
def test_keep_largest_brings_hd95_down_to_the_filtered_value(lib_mode):
    """what --val_surface with --val_keep_largest reports: a prediction with 0.1 % specks before and after ops.keep_largest(k=1)"""
    from scipy import ndimage
    from vae_segmentation_amd import ops
    s = 128
    pred, label = organ_with_specks(s), organ(s)
    t = cuda5(pred)
    filtered = ops.keep_largest(t, k=1)
    lab, _ = ndimage.label(pred, structure=np.ones((3, 3, 3)))
    biggest = lab == (np.argmax(np.bincount(lab.ravel())[1:]) + 1)
    assert np.array_equal(filtered[0, 0].cpu().numpy() >= 0.5, biggest) and biggest.sum() < pred.sum()
    key = ("filter", s)
    if key not in _MEMO:
        _MEMO.clear()
        _MEMO[key] = SU.metrics(pred, label), SU.metrics(biggest, label)
    want_raw, want_filt = _MEMO[key]
    raw = run_distances(pred, label)[0]
    rec = ops.surface_distances(filtered, cuda5(label))
    filt = {k: rec[k].reshape(-1)[0].item() for k in SU.FIELDS}
    assert_record(raw, want_raw, None, "unfiltered")
    assert_record(filt, want_filt, None, "filtered")
    assert filt["hd95"] < raw["hd95"] and filt["hd"] < 0.5 * raw["hd"] and filt["assd"] < raw["assd"]
    assert want_filt["hd95"] < want_raw["hd95"]


class _FixedPrediction(torch.nn.Module):
    def __init__(self, pred):
        super().__init__()
        self.pred = pred

    def forward(self, batch, img_key, out_key):
        return {out_key: self.pred}


@both_libs
def test_validate_reports_surface_distances(lib_mode, capsys):
    from vae_segmentation_amd import driver
    s = 48
    z, y, x = np.indices((s, s, s))
    blob = ((z - 24) ** 2 + (y - 22) ** 2 + (x - 26) ** 2) < 100
    noisy = blob.copy()
    noisy[2:4, 3:5, 40:42] = True
    noisy[44, 44, 5] = True
    noisy[24, 22, 36:38] = True                          # a bump on the organ itself: the filter keeps it
    label = torch.from_numpy(blob.astype(np.float32)).view(1, 1, s, s, s)
    p1 = torch.from_numpy(np.where(noisy, 0.9, 0.1).astype(np.float32)).view(1, 1, s, s, s)
    pred = torch.cat([1 - p1, p1], 1).cuda()
    empty = torch.cat([torch.ones_like(p1), torch.zeros_like(p1)], 1).cuda()
    loader = [{driver.IMG_KEY: torch.zeros(1, 1, s, s, s), driver.LABEL_KEY: label}]
    model = _FixedPrediction(pred)
    plain = driver.validate("seg_train", model, loader, 2)
    assert capsys.readouterr().out == ""
    log = {}
    assert driver.validate("seg_train", model, loader, 2, surface=True, surface_log=log) == plain
    out = capsys.readouterr().out
    want = SU.metrics(noisy, blob)
    assert "validation surface distances: ASSD %f, HD95 %f voxels (0 of 1 case x class entries undefined)" % (want["assd"], want["hd95"]) in out
    assert list(log) == [0] and log[0]["assd"] == [pytest.approx(want["assd"], rel=1e-9)] and log[0]["hd95"] == [pytest.approx(want["hd95"], rel=1e-9)]
    # with the filter: the filtered values, the unfiltered ones beside them
    filt_scores = driver.validate("seg_train", model, loader, 2, keep_largest=1)
    capsys.readouterr()
    log = {}
    assert driver.validate("seg_train", model, loader, 2, keep_largest=1, surface=True, surface_log=log) == filt_scores
    out = capsys.readouterr().out
    kept = noisy.copy()
    kept[2:4, 3:5, 40:42] = False
    kept[44, 44, 5] = False
    wf = SU.metrics(kept, blob)
    assert wf["hd"] < want["hd"]
    assert "validation surface distances: ASSD %f, HD95 %f voxels" % (wf["assd"], wf["hd95"]) in out
    assert "validation surface distances without the component filter: ASSD %f, HD95 %f voxels" % (want["assd"], want["hd95"]) in out
    assert log[0]["hd95"] == [pytest.approx(wf["hd95"], rel=1e-9)] and log[0]["hd95_unfiltered"] == [pytest.approx(want["hd95"], rel=1e-9)]
    assert log[0]["assd"] == [pytest.approx(wf["assd"], rel=1e-9)] and log[0]["assd_unfiltered"] == [pytest.approx(want["assd"], rel=1e-9)]
    # an empty prediction: undefined, counted, no exception
    log = {}
    driver.validate("seg_train", _FixedPrediction(empty), loader, 2, surface=True, surface_log=log)
    assert "undefined in all 1 entries" in capsys.readouterr().out
    assert math.isnan(log[0]["assd"][0]) and math.isnan(log[0]["hd95"][0])


def _run(args, cwd):
    out = subprocess.run([sys.executable] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_entry_point_writes_surface_json_and_leaves_the_scores_alone(tmp_path):
    """A tiny seg_train run with --val_surface, and one with --val_keep_largest 1 beside it.  The entry points take no seed (initialisation and loader order
    differ from process to process), so "the same run without the flag" is made the same by evaluating the first run's checkpoint with --test_only."""
    common = ["--size", "64", "-b", "1", "-E", "1", "--eval_epoch", "1", "--save_epoch", "1", "--synthetic_train", "2", "--synthetic_val", "2",
              "--max_iters", "2", "--display_freq", "1"]
    main = os.path.join(REPO, "main_source.py")

    def check_log(path, filtered):
        log = json.loads(path.read_text())
        assert sorted(log) == ["0", "1"]
        keys = ["assd", "hd95"] + (["assd_unfiltered", "hd95_unfiltered"] if filtered else [])
        for case in log.values():
            assert sorted(case) == sorted(keys)
            for k in keys:
                assert len(case[k]) == 1 and isinstance(case[k][0], float) and (math.isnan(case[k][0]) or 0 <= case[k][0] < 64 * 2)

    for extra, filtered in (([], False), (["--val_keep_largest", "1"], True)):
        d = tmp_path / ("train_filtered" if filtered else "train")
        d.mkdir()
        out = _run([main, "run", "--method", "seg_train", "--val_surface"] + extra + common, str(d))
        assert "Finished Training" in out and "validation surface distances" in out
        assert ("validation surface distances without the component filter" in out) == filtered
        check_log(d / "tensorboard" / "run" / "surface_0.json", filtered)
        assert (d / "tensorboard" / "run" / "score_0.json").exists()
    # the same network evaluated with and without the flag
    d = tmp_path / "train"
    outs, scores = {}, {}
    for name, extra in (("plain", []), ("surface", ["--val_surface"]), ("filtered", ["--val_keep_largest", "1"]),
                        ("surface_filtered", ["--val_surface", "--val_keep_largest", "1"])):
        outs[name] = _run([main, name, "--method", "seg_train", "--test_only", "--load_prefix", "run", "--checkpoint_name", "model_epoch1.ckpt"] + extra + common,
                          str(d))
        tb = d / "tensorboard" / name
        scores[name] = (tb / "score_0.json").read_text()
        assert (tb / "surface_0.json").exists() == ("surface" in name)
        if "surface" in name:
            check_log(tb / "surface_0.json", "filtered" in name)
        else:
            assert "surface distances" not in outs[name]
    assert scores["surface"] == scores["plain"] and scores["surface_filtered"] == scores["filtered"]
    # every printed line of a run with the flag that is not about surface distances is a line of the run without it
    strip = lambda text: [l for l in text.splitlines() if "surface distances" not in l]
    assert strip(outs["surface"]) == strip(outs["plain"]) and strip(outs["surface_filtered"]) == strip(outs["filtered"])
