"""GPU: exact percentiles and intensity standardisation on the device (csrc/quantile.hip, ops.quantile / intensity_map, data_gpu.IntensityStandardizer,
--standardize) against tests/standardize_util.py, which tests/test_host_standardize.py pins to np.percentile with ==.

Percentiles are compared for EQUALITY: two exact order statistics and three IEEE operations.  The map is compared within 2^-22 max|oracle| (one float32
rounding of an fp64 value errs by 2^-24 relative; an fp64-sized difference can move it across a rounding tie, one float32 ulp, 2^-23 relative — the
argument of tests/test_gpu_lowres.py's header).  No case is excluded: non-finite voxels are compared for identity, the others within the bound."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import standardize_util as SU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
SHAPES = [(1, 1, 1), (1, 1, 2), (5, 7, 9), (3, 17, 241), (40, 48, 56), (2, 3, 5, 7, 9)]
P_SETS = {1: (50,), 2: (0.5, 99.5), 16: (0, 100, 50, 50, 0.5, 1, 5, 10, 25, 33.3, 66.6, 75, 90, 95, 99, 99.5)}
L_SETS = {2: (0.5, 99.5), 11: (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99), 16: tuple(float(p) for p in np.linspace(0.5, 99.5, 16))}
BIG = (40, 48, 56)


def _mods():
    from vae_segmentation_amd import data_gpu as D
    from vae_segmentation_amd import ops
    assert all(hasattr(ops, n) for n in ("quantile", "intensity_map", "QUANTILE_WG_VOXELS")) and hasattr(D, "IntensityStandardizer")
    return D, ops


@functools.lru_cache(maxsize=None)
def _vol(shape, kind, seed=0, air=True):
    x = SU.volume(shape, kind, seed, air)
    x.setflags(write=False)
    return x


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).cuda()


def _planes(x):
    return np.asarray(x).reshape((-1,) + tuple(x.shape[-3:]))


@functools.lru_cache(maxsize=None)
def _want(shape, kind, ps, above=None):
    return [SU.ref_quantile(p, ps, above) for p in _planes(_vol(shape, kind))]


def _same_quantiles(got, want, lead, what):
    """got: ops.quantile's dict; want: one oracle dict per plane"""
    q = got["q"].cpu().numpy().reshape(len(want), -1)
    lo, hi = got["lo"].cpu().numpy().reshape(len(want), -1), got["hi"].cpu().numpy().reshape(len(want), -1)
    assert got["q"].dtype == torch.float64 and got["lo"].dtype == torch.float32 and got["hi"].dtype == torch.float32
    assert got["count"].dtype == torch.int64 and got["rejected"].dtype == torch.int64
    assert tuple(got["q"].shape) == lead + (q.shape[1],) and tuple(got["count"].shape) == lead and tuple(got["rejected"].shape) == lead
    assert got["count"].cpu().numpy().ravel().tolist() == [w["count"] for w in want], what
    assert got["rejected"].cpu().numpy().ravel().tolist() == [w["rejected"] for w in want], what
    for i, w in enumerate(want):
        assert np.array_equal(lo[i], w["lo"], equal_nan=True) and np.array_equal(hi[i], w["hi"], equal_nan=True), (what, i, lo[i], w["lo"], hi[i], w["hi"])
        assert np.array_equal(q[i], w["q"], equal_nan=True), (what, i, q[i], w["q"])


# ---- order statistics --------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("shape", SHAPES)
def test_percentiles_equal_the_oracles(shape, lib_mode):
    D, ops = _mods()
    assert int(np.prod(BIG)) > ops.QUANTILE_WG_VOXELS                        # that shape spans more than one workgroup's share of a plane
    for kind in SU.KINDS:
        x = _dev(_vol(shape, kind))
        for nq, ps in P_SETS.items():
            got = ops.quantile(x, ps)
            _same_quantiles(got, _want(shape, kind, ps), tuple(shape[:-3]), "%s %s Q %d" % (shape, kind, nq))


def test_selection_by_threshold_and_mask():
    D, ops = _mods()
    x = _vol(BIG, "ct")
    mask = (np.random.RandomState(5).rand(*BIG) < 0.5).astype(np.uint8)
    xd, md = _dev(x), _dev(mask)
    ps = P_SETS[2]
    for above, m, mdev in ((-500.0, None, None), (None, mask, md), (-500.0, mask, md), (None, mask, md.bool())):
        want = SU.ref_quantile(x, ps, above, m)
        assert 0.1 * x.size <= want["count"] <= 0.9 * x.size                # the selection selects: neither everything nor nothing
        _same_quantiles(ops.quantile(xd, ps, above=above, mask=mdev), [want], (), "above %r mask %s" % (above, m is not None))
    bad = _vol(BIG, "nonfinite")                                            # non-finite voxels are rejected whatever the selectors say
    want = SU.ref_quantile(bad, ps, -500.0, mask)
    assert want["rejected"] == int((~np.isfinite(bad)).sum()) > 0
    _same_quantiles(ops.quantile(_dev(bad), ps, above=-500.0, mask=md), [want], (), "nonfinite, both selectors")
    got = ops.quantile(xd, ps, mask=torch.zeros_like(md))
    assert int(got["count"]) == 0 and int(got["rejected"]) == 0
    assert bool(torch.isnan(got["q"]).all()) and bool(torch.isnan(got["lo"]).all()) and bool(torch.isnan(got["hi"]).all())
    present = float(np.sort(x[x > -1024.0])[1000])                          # a value of the data as the threshold: the comparison is strict
    assert (x == np.float32(present)).any()
    got = ops.quantile(xd, (0,), above=present)
    assert float(got["lo"]) > present and int(got["count"]) == int((x > np.float32(present)).sum())
    _same_quantiles(got, [SU.ref_quantile(x, (0,), present)], (), "strict")


# ---- the map -----------------------------------------------------------------------------------------------------------------------------------
def _close(got, want, what=""):
    got, want = got.detach().cpu().numpy(), np.asarray(want, np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    odd = ~np.isfinite(want)
    same_odd = np.array_equal(got[odd], want[odd], equal_nan=True)
    g, w = got[~odd].astype(np.float64), want[~odd].astype(np.float64)
    tol = 2.0 ** -22 * (np.abs(w).max() if w.size else 0.0)
    err = np.abs(g - w).max() if w.size else 0.0
    print("%s max abs err %.3e (bound %.3e)" % (what, err, tol))
    return same_odd and bool(np.all(np.isfinite(g))) and err <= tol


def _dst(nl):
    return np.linspace(-200.0, 400.0, nl)


@BOTH
@pytest.mark.parametrize("nl", sorted(L_SETS))
@pytest.mark.parametrize("shape", [(5, 7, 9), BIG])
def test_map_vs_oracle(shape, nl, lib_mode):
    D, ops = _mods()
    dst = torch.from_numpy(_dst(nl)).cuda()
    for kind in SU.KINDS:
        x = _vol(shape, kind)
        xd = _dev(x)
        src = ops.quantile(xd, L_SETS[nl])["q"]                             # consumed as it is: no host copy between the two calls
        want_src = _want(shape, kind, L_SETS[nl])[0]["q"]
        assert np.array_equal(src.cpu().numpy(), want_src)
        for mode in ("linear", "clamp"):
            got = ops.intensity_map(xd, src, dst, extrapolate=mode)
            assert _close(got, SU.ref_map(x, want_src, _dst(nl), mode), "%s %s L %d %s" % (shape, kind, nl, mode))
            if kind == "constant" or (kind == "ties" and nl == 16):         # repeated landmarks (16 of 11 values): segments of no width, finite output
                assert len(set(want_src.tolist())) < nl and bool(torch.isfinite(got).all())
            if mode == "clamp":
                fin = torch.isfinite(xd)
                assert float(got[fin].min()) >= -200.0 and float(got[fin].max()) <= 400.0
    out = torch.empty_like(xd)
    assert ops.intensity_map(xd, src, dst, out=out) is out and torch.equal(out.view(torch.int32), ops.intensity_map(xd, src, dst).view(torch.int32))


def test_map_leaves_nonfinite_voxels_and_unselected_planes_alone():
    D, ops = _mods()
    x = np.stack([_vol((5, 7, 9), "nonfinite", seed=1), _vol((5, 7, 9), "nonfinite", seed=2)])
    x[0].ravel()[:3] = (np.nan, np.inf, -np.inf)
    xd = _dev(x)
    odd = ~np.isfinite(x)
    assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
    mask = np.ones(x.shape, np.uint8)
    mask[1] = 0                                                             # nothing selected in plane 1: NaN landmarks, the plane is copied
    rec = ops.quantile(xd, (0.5, 99.5), mask=_dev(mask))
    assert rec["count"].tolist()[1] == 0 and bool(torch.isnan(rec["q"][1]).all()) and bool(torch.isfinite(rec["q"][0]).all())
    dst = torch.tensor([-200.0, 400.0], dtype=torch.float64, device="cuda")
    for mode in ("linear", "clamp"):
        got = ops.intensity_map(xd, rec["q"], dst, extrapolate=mode).cpu().numpy()
        assert np.array_equal(got.view(np.int32)[odd], x.view(np.int32)[odd])           # NaN, +inf and -inf: the same bits
        assert np.array_equal(got[1].view(np.int32), x[1].view(np.int32))
        want0 = SU.ref_map(x[0], SU.ref_quantile(x[0], (0.5, 99.5))["q"], (-200.0, 400.0), mode)
        assert _close(torch.from_numpy(got[0]), want0, "plane 0 %s" % mode)


# ---- invariance: the point of the feature ------------------------------------------------------------------------------------------------------
def test_transform_is_invariant_under_an_affine_change_of_units():
    D, ops = _mods()
    x = _vol((30, 30, 30), "ct", air=False)
    s = D.IntensityStandardizer((0.5, 99.5))
    want = SU.ref_map(x, SU.ref_quantile(x, (0.5, 99.5))["q"], (-200.0, 400.0))
    base = s.transform(_dev(x))
    assert _close(base, want, "unchanged units")
    for a, b in ((2, 1024), (0.5, -3), (4, 0)):
        moved = (np.float32(a) * x + np.float32(b)).astype(np.float32)      # exact: integers, halves and small offsets
        assert np.array_equal(moved.astype(np.float64), a * x.astype(np.float64) + b)
        assert _close(s.transform(_dev(moved)), want, "a %g b %g" % (a, b))
    out = s({"venous": _dev(x), "other": None})
    assert torch.equal(out["venous"], base) and out["other"] is None


# ---- Nyul and Udupa ----------------------------------------------------------------------------------------------------------------------------
def test_fit_gives_the_oracles_standard_scale_and_the_state_round_trips():
    D, ops = _mods()
    vols = [(_vol((12, 13, 14), "ct", seed=i, air=False) * np.float32(a) + np.float32(b)).astype(np.float32)
            for i, (a, b) in enumerate(((1, 0), (2, 1024), (0.5, -3)))]
    ps = L_SETS[11]
    s = D.IntensityStandardizer(ps, above=None)
    with pytest.raises(RuntimeError, match="fit"):
        s.transform(_dev(vols[0]))
    assert s.fit([_dev(v) for v in vols]) is s
    want = SU.ref_fit(vols, ps, (-200.0, 400.0))
    err = np.abs(np.array(s.scale) - want).max() / np.abs(want).max()
    print("standard scale: max rel err %.3e" % err)
    assert err <= 1e-12
    state = s.state_dict()
    assert json.loads(json.dumps(state))["scale"] == s.scale
    t = D.IntensityStandardizer().load_state_dict(state)
    assert t.state_dict() == state and t.percentiles == tuple(ps)
    got = t.transform(_dev(vols[1]))
    assert torch.equal(got, s.transform(_dev(vols[1])))
    assert _close(got, SU.ref_map(vols[1], SU.ref_quantile(vols[1], ps)["q"], np.array(s.scale)), "nyul transform")
    with pytest.raises(ValueError, match="scale"):
        D.IntensityStandardizer((10, 50, 90)).fit([_dev(_vol((5, 7, 9), "constant"))])


# ---- replay ------------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_bit_for_bit():
    D, ops = _mods()
    inputs = [_dev(_vol(BIG, kind, seed=i)) for i, kind in enumerate(("ct", "nonfinite", "wide"))]
    dst = torch.from_numpy(_dst(11)).cuda()
    ps = L_SETS[11]

    def run(x):
        rec = ops.quantile(x, ps, above=-500.0)
        return rec, ops.intensity_map(x, rec["q"], dst, extrapolate="clamp")

    eager = [run(x) for x in inputs]
    static = inputs[0].clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                           # a synchronising call would end the capture with an error
        rec, y = run(static)
    for x, (erec, ey) in zip(inputs, eager):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int32), ey.view(torch.int32))
        assert torch.equal(rec["q"].view(torch.int64), erec["q"].view(torch.int64))
        assert all(torch.equal(rec[k], erec[k]) for k in ("lo", "hi", "count", "rejected"))


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_answered_before_a_launch():
    import ctypes
    from vae_segmentation_amd import _lib
    D, ops = _mods()
    x = _dev(_vol((5, 7, 9), "ct"))
    for bad in ((), tuple(range(17)), (-1,), (100.5,), (float("nan"),), (float("inf"),)):
        with pytest.raises(ValueError, match="percentile"):
            ops.quantile(x, bad)
    with pytest.raises(ValueError):
        ops.quantile(x, (50,), above=float("nan"))
    with pytest.raises(TypeError):
        ops.quantile(x.double(), (50,))
    with pytest.raises(ValueError):
        ops.quantile(x[:, :, :0], (50,))
    with pytest.raises(ValueError, match="contiguous"):
        ops.quantile(x.permute(2, 1, 0), (50,))
    with pytest.raises(TypeError):
        ops.quantile(x, (50,), mask=torch.ones_like(x))
    with pytest.raises(ValueError):
        ops.quantile(x, (50,), mask=torch.ones((5, 7, 8), dtype=torch.uint8, device="cuda"))
    src = ops.quantile(x, (0.5, 99.5))["q"]
    dst = torch.tensor([-200.0, 400.0], dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="extrapolate"):
        ops.intensity_map(x, src, dst, extrapolate="nearest")
    with pytest.raises(TypeError):
        ops.intensity_map(x, src.float(), dst)
    with pytest.raises(TypeError):
        ops.intensity_map(x, src, [-200.0, 400.0])
    with pytest.raises(ValueError):
        ops.intensity_map(x, src, dst[:1])
    with pytest.raises(ValueError):
        ops.intensity_map(x, src, torch.zeros(17, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.intensity_map(x, torch.zeros(3, dtype=torch.float64, device="cuda"), dst)
    with pytest.raises(ValueError):
        ops.intensity_map(x, src, dst, out=torch.empty((5, 7, 8), device="cuda"))
    # the C entry points: the library's codes, from the host checks (the pointers are never followed)
    lib = _lib.lib
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    rec = ops.quantile(x, (50,))
    ws = torch.empty(int(lib.vs_quantile_workspace_bytes(1, 315, 1)) // 8 + 2, dtype=torch.float64, device="cuda")
    p01 = (ctypes.c_double * 16)(*([0.5] * 16))
    good = dict(x=x.data_ptr(), mask=None, use_above=0, above=0.0, p01=ctypes.addressof(p01), Q=1, q=rec["q"].data_ptr(), lo=rec["lo"].data_ptr(),
                hi=rec["hi"].data_ptr(), count=rec["count"].data_ptr(), rej=rec["rejected"].data_ptr(), ws=ws.data_ptr(), planes=1, d=5, h=7, w=9)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vs_quantile(a["x"], a["mask"], a["use_above"], a["above"], a["p01"], a["Q"], a["q"], a["lo"], a["hi"], a["count"], a["rej"], a["ws"],
                               a["planes"], a["d"], a["h"], a["w"], None)

    for k in ("x", "p01", "q", "lo", "hi", "count", "rej", "ws"):
        assert call(**{k: None}) == EINVAL, k
    assert call(Q=0) == EINVAL and call(Q=17) == EINVAL and call(use_above=1, above=float("nan")) == EINVAL
    for p in (float("nan"), -0.01, 1.01, float("inf")):
        assert call(p01=ctypes.addressof((ctypes.c_double * 1)(p))) == EINVAL, p
    assert call(d=0) == ESHAPE and call(planes=0) == ESHAPE and call(d=2048, h=1024, w=1024) == ESHAPE
    assert call(x=x.data_ptr() + 2) == EALIGN and call(q=rec["q"].data_ptr() + 4) == EALIGN and call(ws=ws.data_ptr() + 8) == EALIGN
    assert call(count=rec["count"].data_ptr() + 4) == EALIGN and call(lo=rec["lo"].data_ptr() + 1) == EALIGN
    assert lib.vs_quantile_workspace_bytes(1, 315, 0) == 0 and lib.vs_quantile_workspace_bytes(1, 2 ** 31, 1) == 0
    assert lib.vs_quantile_workspace_bytes(0, 315, 1) == 0 and lib.vs_quantile_workspace_bytes(2, 315, 16) == 2 * lib.vs_quantile_workspace_bytes(1, 7, 16)
    y = torch.empty_like(x)

    def imap(xp=x.data_ptr(), sp=src.data_ptr(), dp=dst.data_ptr(), nl=2, clamp=0, yp=y.data_ptr(), planes=1, d=5, h=7, w=9):
        return lib.vs_intensity_map(xp, sp, dp, nl, clamp, yp, planes, d, h, w, None)

    assert imap(xp=None) == EINVAL and imap(sp=None) == EINVAL and imap(dp=None) == EINVAL and imap(yp=None) == EINVAL
    assert imap(nl=1) == EINVAL and imap(nl=17) == EINVAL and imap(clamp=2) == EINVAL
    assert imap(w=0) == ESHAPE and imap(d=2048, h=1024, w=1024) == ESHAPE
    assert imap(xp=x.data_ptr() + 2) == EALIGN and imap(sp=src.data_ptr() + 4) == EALIGN and imap(yp=y.data_ptr() + 1) == EALIGN
    torch.cuda.synchronize()
    assert torch.equal(rec["q"], ops.quantile(x, (50,))["q"])               # no refused call touched a buffer


# ---- the entry points --------------------------------------------------------------------------------------------------------------------------
UNITS = ((1.0, 0.0), (2.0, 1024.0), (0.5, -3.0), (4.0, 0.0))


def _write_cases(root, units=None):
    """small merge arrays (image, label); units: per case (a, b), the image stored as a * image + b"""
    rng = np.random.RandomState(0)
    root.mkdir()
    names = []
    for i, shape in enumerate([(40, 48, 44), (52, 40, 46), (44, 44, 60), (48, 50, 42)]):
        merge = np.zeros(shape + (2,), np.float32)
        merge[..., 0] = np.round(rng.randn(*shape) * 250 + 40)
        if units is not None:
            merge[..., 0] = np.float32(units[i][0]) * merge[..., 0] + np.float32(units[i][1])
        merge[10:30, 12:34, 8:30, 1] = 1
        np.save(root / ("case%d_merge.npy" % i), merge)
        names.append("case%d_merge.npy" % i)
    return names


def _run(args, cwd):
    out = subprocess.run([sys.executable] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_entry_points_run_with_the_flag(tmp_path):
    names = _write_cases(tmp_path / "data", UNITS)
    (tmp_path / "lists").mkdir()
    json.dump({"NIH_train": names[:3], "NIH_val": names[3:]}, open(tmp_path / "lists" / "Multi_all.json", "w"))
    data = str(tmp_path / "data")
    out = _run([os.path.join(REPO, "main_source.py"), "std", "-M", "seg_train", "--real_data", "--standardize", "0.5,99.5", "--max_iters", "2", "-R", data,
                "-V", data, "--size", "32", "-b", "1", "-E", "1", "--eval_epoch", "1", "--save_epoch", "1", "--display_freq", "1"], str(tmp_path))
    assert "Finished Training" in out and "validation result" in out and out.count("loss:") >= 2
    out = _run([os.path.join(REPO, "main_target.py"), "stdda", "-M", "domain_adaptation", "--real_data", "--standardize", "0.5,99.5", "--standardize_above",
                "-2000", "--max_iters", "2", "-R", data, "-V", data, "--train_first_epoch", "--size", "64", "-b", "1", "-E", "1", "--eval_epoch", "1",
                "--save_epoch", "1", "--display_freq", "1"], str(tmp_path))
    assert "Finished Training" in out


def test_loader_standardises_only_with_the_flag(tmp_path):
    import main_source
    from vae_segmentation_amd import driver, evaluation
    D, ops = _mods()
    plain_names = _write_cases(tmp_path / "plain")
    moved_names = _write_cases(tmp_path / "moved", UNITS)
    common = ["run", "--real_data", "--size", "32", "-b", "2"]
    flag = ["--standardize", "0.5,99.5"]

    def loader(root, extra, train):
        return driver.DeviceCaseLoader(plain_names, str(tmp_path / root), main_source.parse(common + extra), 2, train, False, seed=4)

    a, b = loader("plain", flag, False), loader("moved", flag, False)       # the validation chain: nothing random
    assert isinstance(a.standardize, D.IntensityStandardizer) and a.standardize.percentiles == (0.5, 99.5)
    assert a.standardize.target == evaluation.INTENSITY_CLIP and a.standardize.above is None

    def same(got, want, what):
        """the map's tolerance against the unchanged dataset's result: 2^-22 max|that result|"""
        tol = 2.0 ** -22 * float(want.abs().max())
        err = float((got - want).abs().max())
        print("%s: differ by %.3e (bound %.3e)" % (what, err, tol))
        return got.shape == want.shape and bool(torch.isfinite(got).all()) and err <= tol

    for (ia, la), (ib, lb) in zip(a.whole_cases(), b.whole_cases()):
        assert torch.equal(la, lb) and same(ib, ia, "whole case")
    for ba, bb in zip(a, b):
        assert ba[driver.IMG_KEY].shape == (2, 1, 32, 32, 32) and torch.equal(ba[driver.LABEL_KEY], bb[driver.LABEL_KEY])
        assert same(bb[driver.IMG_KEY], ba[driver.IMG_KEY], "validation batch")
    ta, tb = loader("plain", flag, True), loader("moved", flag, True)       # the training loader standardises too (the same draws: the same seed)
    assert isinstance(ta.standardize, D.IntensityStandardizer) and ta.transform is not None
    for ba, bb in zip(ta, tb):
        assert torch.equal(ba[driver.LABEL_KEY], bb[driver.LABEL_KEY]) and same(bb[driver.IMG_KEY], ba[driver.IMG_KEY], "training batch")
    # without the flag: what train_sample gives when called directly, bit for bit, and nothing is built
    off = loader("moved", [], False)
    assert off.standardize is None
    for b, batch in enumerate(off):
        for k in range(2):
            merge = torch.from_numpy(np.load(tmp_path / "moved" / moved_names[2 * b + k]).astype(np.float32)).cuda()
            img, lab = D.train_sample(merge, (32,) * 3, off.mask_index, None, field=driver.IMG_KEY)
            assert torch.equal(batch[driver.IMG_KEY][k:k + 1], img) and torch.equal(batch[driver.LABEL_KEY][k:k + 1], lab)
    # with it the window sits where the data is: the unit change would otherwise saturate Clip
    on = next(iter(loader("moved", flag, False)))[driver.IMG_KEY][1]
    raw = next(iter(off))[driver.IMG_KEY][1]
    assert float((raw == 1.0).float().mean()) > 0.5 > float((on == 1.0).float().mean())
    above = driver.DeviceCaseLoader(plain_names, str(tmp_path / "plain"), main_source.parse(common + flag + ["--standardize_above", "-500"]), 2, False, False)
    assert above.standardize.above == -500.0


class PlantedNet:
    """a 'network' in the dict protocol of modules.Segmentation whose answer is known: probability 0.9 of class 1 where the normalised intensity is positive"""

    def __call__(self, data_dict, in_key, out_key):
        p1 = torch.where(data_dict[in_key][:, 0] > 0.0, 0.9, 0.1)
        data_dict[out_key] = torch.stack([1 - p1, p1], 1)
        return data_dict


def test_inference_functions_take_a_standardizer():
    from vae_segmentation_amd import evaluation
    D, ops = _mods()
    shape = (40, 48, 56)
    zz, yy, xx = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    organ = ((zz - 18) / 9.0) ** 2 + ((yy - 22) / 8.0) ** 2 + ((xx - 30) / 12.0) ** 2 < 1.0
    vol = (np.where(organ, 400.0, -200.0) + np.random.RandomState(4).randn(*shape) * 5.0).astype(np.float32)
    img = _dev(2.0 * vol + 1024.0)                                          # another unit: the window of Clip would saturate
    s = D.IntensityStandardizer((0.5, 99.5), target=evaluation.INTENSITY_CLIP)
    before = img.clone()
    got = evaluation.coarse_to_fine_predict(PlantedNet(), img, 32, batch=3, want_prob=True, standardize=s)
    want = evaluation.coarse_to_fine_predict(PlantedNet(), s.transform(img), 32, batch=3, want_prob=True)
    assert torch.equal(img, before) and got["found"] is True and want["found"] is True
    assert torch.equal(got["label"], want["label"]) and torch.equal(got["coarse_label"], want["coarse_label"]) and torch.equal(got["prob"], want["prob"])
    assert np.array_equal(got["coarse_label"].cpu().numpy() == 1, organ)    # standardised, the organ stands out again ...
    plain = evaluation.coarse_to_fine_predict(PlantedNet(), img, 32, batch=3)
    assert not np.array_equal(plain["coarse_label"].cpu().numpy() == 1, organ)          # ... which it does not in the scan's own unit
    raw = (2.0 * vol + 1024.0).astype(np.float32)
    diag = (1.0, 1.0, 1.0)
    a = evaluation.predict_scan(PlantedNet(), _dev(raw), diag, 32, batch=3, details=True, standardize=s)
    assert a["found"] is True and a["label"].dtype == torch.uint8 and tuple(a["label"].shape) == raw.shape and int(a["label"].sum()) > 0
