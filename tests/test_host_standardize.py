"""Host: the oracle of the percentile / standardisation tests is numpy's percentile, bit for bit; the integer restatement of the kernel's radix select picks
np.sort's values; the map's properties; the transform's and the parsers' argument checks.  No GPU."""
import functools

import numpy as np
import pytest

from tests import standardize_util as SU

SIZES = (1, 2, 3, 64, 65, 4097, 107520)
PS = (0, 0.5, 1, 25, 50, 95, 99.5, 100, 33.3)


@functools.lru_cache(maxsize=None)
def _vol(n, kind):
    x = SU.volume((40, 48, 56) if n == 107520 else (1, 1, n), kind, seed=n)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("kind", SU.KINDS)
def test_ref_quantile_is_numpys_percentile_exactly(kind):
    for n in SIZES:
        x = _vol(n, kind)
        sel, rejected = SU.select(x)
        assert rejected == int((~np.isfinite(x)).sum()) and sel.size == x.size - rejected
        got = SU.ref_quantile(x, PS)
        assert got["count"] == sel.size and got["rejected"] == rejected
        if sel.size == 0:
            assert np.isnan(got["q"]).all()
            continue
        for i, p in enumerate(PS):
            want = np.percentile(sel.astype(np.float64), p)
            assert got["q"][i] == want, (kind, n, p, got["q"][i], want)
            assert float(got["lo"][i]) <= want <= float(got["hi"][i])


def test_ref_quantile_selection():
    x = _vol(4097, "nonfinite")
    mask = (np.random.RandomState(3).rand(*x.shape) < 0.5).astype(np.uint8)
    fin = np.isfinite(x)
    for above, m in ((-500.0, None), (None, mask), (-500.0, mask)):
        keep = fin.copy()
        if above is not None:
            with np.errstate(invalid="ignore"):
                keep &= x > np.float32(above)
        if m is not None:
            keep &= m != 0
        got = SU.ref_quantile(x, (0.5, 99.5), above, m)
        assert got["count"] == int(keep.sum()) and got["rejected"] == int((~fin).sum())
        assert np.array_equal(got["q"], np.percentile(x[keep].astype(np.float64), (0.5, 99.5)))
    empty = SU.ref_quantile(x, (50,), mask=np.zeros(x.shape, np.uint8))
    assert empty["count"] == 0 and np.isnan(empty["q"]).all() and np.isnan(empty["lo"]).all() and np.isnan(empty["hi"]).all()
    present = float(np.sort(x[fin])[100])                                   # strict: a value equal to the threshold is not selected
    assert SU.ref_quantile(x, (0,), above=present)["lo"][0] > np.float32(present)


@pytest.mark.parametrize("kind", SU.KINDS)
def test_integer_radix_select_picks_np_sorts_values(kind):
    for n in SIZES:
        sel, _ = SU.select(_vol(n, kind))
        if sel.size == 0:
            continue
        keys, order = SU.key(sel), np.sort(sel)
        assert np.array_equal(sel[np.argsort(keys, kind="stable")], order)    # the keys' order is the values' order (-0.0 == 0.0)
        for p in PS:
            k, k1, _ = SU.ranks(sel.size, p)
            for r in (k, k1):
                assert SU.unkey(SU.radix_select(keys, r)) == order[r], (kind, n, p, r)
    for v in (0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38):
        e = int(SU.key(np.float32(v)))
        assert 0 < e < 0xFFFFFFFF and SU.unkey(e).tobytes() == np.float32(v).tobytes()


def test_ref_map_properties():
    rng = np.random.RandomState(0)
    src = np.array([-3.0, -1.0, -1.0, 0.5, 4.0, 9.0])                       # one segment of no width
    dst = np.array([0.0, 1.0, 2.0, 3.0, 5.0, 8.0])
    x = np.sort(np.concatenate([rng.uniform(-10, 15, 500), src])).astype(np.float32)
    for mode in ("linear", "clamp"):
        y = SU.ref_map(x, src, dst, mode)
        assert y.dtype == np.float32 and np.all(np.diff(y[(x < -1.0)]) >= 0) and np.all(np.diff(y[x >= -1.0]) >= 0)     # monotone on either side of the jump
        for j in (0, 1, 3, 4):                                              # it hits dst[j] at src[j]; at the repeated landmark the later one
            assert SU.ref_map(np.float32([src[j]]), src, dst, mode)[0] == np.float32(dst[2] if j == 1 else dst[j])
        inside = (x >= src[0]) & (x <= src[-1])
        assert np.all((y[inside] >= dst[0]) & (y[inside] <= dst[-1]))
    lin, cl = SU.ref_map(x, src, dst, "linear"), SU.ref_map(x, src, dst, "clamp")
    assert lin[0] < dst[0] and lin[-1] > dst[-1] and cl[0] == dst[0] and cl[-1] == dst[-1]
    assert np.array_equal(lin[(x >= src[0]) & (x <= src[-1])], cl[(x >= src[0]) & (x <= src[-1])])
    # strictly monotone landmarks: monotone everywhere
    y = SU.ref_map(x, np.array([-3.0, 0.5, 9.0]), np.array([-200.0, 0.0, 400.0]))
    assert np.all(np.diff(y) >= 0)
    # a zero-width segment has slope 0: constant data maps to the scale's first landmark, finite
    flat = SU.ref_map(np.full(5, 7.25, np.float32), np.array([7.25, 7.25]), np.array([-200.0, 400.0]))
    assert np.array_equal(flat, np.full(5, -200.0, np.float32))
    odd = np.array([np.nan, np.inf, -np.inf, 1.0], np.float32)
    got = SU.ref_map(odd, src, dst)
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == -np.inf and np.isfinite(got[3])
    assert np.array_equal(SU.ref_map(x, np.full(6, np.nan), dst), x)


def test_ref_fit_maps_the_ends_onto_the_target():
    vols = [SU.volume((9, 10, 11), "ct", seed=s, air=False) * a + b for s, (a, b) in enumerate(((1, 0), (2, 1024), (0.5, -3)))]
    ps = (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99)
    scale = SU.ref_fit(vols, ps, (-200.0, 400.0))
    assert abs(scale[0] + 200.0) < 1e-9 and abs(scale[-1] - 400.0) < 1e-9 and np.all(np.diff(scale) > 0)


def test_standardizer_constructor_and_fit_before_transform():
    import torch
    from vae_segmentation_amd import data_gpu as D
    assert hasattr(D, "IntensityStandardizer")
    s = D.IntensityStandardizer()
    assert s.percentiles == (0.5, 99.5) and s.target == (-200.0, 400.0) and s.above is None and s.scale == [-200.0, 400.0]
    for bad in (dict(percentiles=(50,)), dict(percentiles=tuple(range(17))), dict(percentiles=(10, 10)), dict(percentiles=(90, 10)),
                dict(percentiles=(-1, 50)), dict(percentiles=(0, 101)), dict(percentiles=(0, float("nan"))), dict(target=(400, -200)),
                dict(target=(1, 1)), dict(target=(0, 1, 2)), dict(above=float("nan")), dict(extrapolate="nearest")):
        with pytest.raises(ValueError):
            D.IntensityStandardizer(**bad)
    nyul = D.IntensityStandardizer((1, 10, 50, 90, 99))
    assert nyul.scale is None
    with pytest.raises(RuntimeError, match="fit"):
        nyul.transform(torch.zeros(2, 3, 4))
    state = nyul.state_dict()
    assert state["percentiles"] == (1.0, 10.0, 50.0, 90.0, 99.0) and state["scale"] is None and state["above"] is None
    state["scale"] = [-200.0, -100.0, 0.0, 300.0, 400.0]
    other = D.IntensityStandardizer().load_state_dict(state)
    assert other.percentiles == nyul.percentiles and other.scale == state["scale"] and other.state_dict() == state
    with pytest.raises(ValueError):
        D.IntensityStandardizer().load_state_dict(dict(state, scale=[0.0, 1.0]))


def test_both_parsers_take_the_flags_and_refuse_them_without_real_data(capsys):
    import main_source
    import main_target
    for mod in (main_source, main_target):
        a = mod.parse(["run", "--real_data", "--standardize", "0.5,99.5", "--standardize_above", "-500"])
        assert a.standardize == (0.5, 99.5) and a.standardize_above == -500.0
        a = mod.parse(["run", "--real_data"])
        assert a.standardize is None and a.standardize_above is None
        for bad in (["--standardize", "0.5,99.5"], ["--real_data", "--standardize", "99.5,0.5"], ["--real_data", "--standardize", "5"],
                    ["--real_data", "--standardize", "0,101"], ["--real_data", "--standardize_above", "-500"]):
            with pytest.raises(SystemExit):
                mod.parse(["run"] + bad)
    capsys.readouterr()
