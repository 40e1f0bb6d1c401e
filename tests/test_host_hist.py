"""Host: (1) the numpy / scipy restatement of tests/hist_util.py is pinned against np.histogram, np.histogram2d and known values of the mutual
information — these tests pin the ORACLE of tests/test_gpu_hist.py, not the feature, and pass without it; (2) the argument checks of ops, evaluation,
the C ABI and the entry points' --val_intensity flag that need no device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import hist_util as HU


# ---- (1) the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,bounds", [(1, (-1.0, 1.0)), (7, (-1.0, 1.0)), (10, (-1.0, 1.0)), (256, None), (4096, (-0.5, 0.75))])
def test_restatement_equals_numpy_histogram(bins, bounds):
    rng = np.random.default_rng(bins)
    x = rng.uniform(-1.2, 1.2, 5000).astype(np.float32)
    probe = HU.edge_probe(-1.0, 1.0, 7)
    x[:probe.size] = probe
    rec = HU.ref_histogram(x, bins, bounds)
    x64 = x.astype(np.float64)
    want, _ = np.histogram(x64, bins=rec["edges"])
    assert np.array_equal(rec["table"][0], want) and rec["table"].sum() + rec["outside"] == x.size and rec["overflow"] == 0
    lo, hi = HU.ref_bounds(x) if bounds is None else bounds
    assert np.array_equal(rec["edges"], np.linspace(lo, hi, bins + 1))
    assert rec["outside"] == int(((x64 < lo) | (x64 > hi)).sum())


def test_restatement_equals_numpy_histogram2d_and_handles_non_finite_values():
    rng = np.random.default_rng(1)
    x, y = rng.normal(size=4000).astype(np.float32), rng.uniform(-3, 3, 4000).astype(np.float32)
    for bins, bounds in (((3, 200), None), ((16, 16), ((-1.0, 1.0), (-2.0, 0.5))), ((1, 1), None)):
        rec = HU.ref_joint_histogram(x, y, bins, bounds)
        want, _, _ = np.histogram2d(x.astype(np.float64), y.astype(np.float64), bins=[rec["edges_x"], rec["edges_y"]])
        assert np.array_equal(rec["table"], want.astype(np.int64)) and rec["table"].sum() + rec["outside"] == x.size
    z = x.copy()
    z[:3] = [np.nan, np.inf, -np.inf]
    rec = HU.ref_histogram(z, 8)
    assert rec["outside"] == 3 and rec["table"].sum() == z.size - 3 and rec["edges"][0] == z[3:].min() and rec["edges"][-1] == z[3:].max()
    rec = HU.ref_histogram(np.full(5, np.nan, np.float32), 4)
    assert rec["outside"] == 5 and np.array_equal(rec["edges"], np.linspace(-0.5, 0.5, 5))
    rec = HU.ref_histogram(np.full(6, 3.25, np.float32), 4)
    assert np.array_equal(rec["edges"], np.linspace(2.75, 3.75, 5)) and rec["table"].sum() == 6
    lab = np.array([0, 1, 2, -1, 5, 1])
    rec = HU.ref_histogram(np.full(6, 3.25, np.float32), 4, labels=lab, rows=2)
    assert rec["overflow"] == 2 and rec["table"].sum(1).tolist() == [1, 2, 1]


def test_last_edge_belongs_to_the_last_bin_and_fusing_would_change_an_edge():
    for bins in (7, 10):
        e = HU.ref_edges(-1.0, 1.0, bins)
        assert HU.ref_bin(np.array([e[0], e[-1]]), e).tolist() == [0, bins - 1]
        probe = HU.edge_probe(-1.0, 1.0, bins)
        want, _ = np.histogram(probe.astype(np.float64), bins=e)
        assert np.array_equal(HU.ref_histogram(probe, bins, (-1.0, 1.0))["table"][0], want)
    # the triple tests/test_gpu_hist.py hard-codes: e_5 of linspace(-0.75, 1.25, 8) is not the correctly rounded 5 * step - 0.75
    from fractions import Fraction
    e, step = HU.ref_edges(-0.75, 1.25, 7), (1.25 + 0.75) / 7
    fused = [float(Fraction(i) * Fraction(step) + Fraction(-0.75)) for i in range(7)]
    assert [i for i in range(7) if fused[i] != e[i]] == [5]


def test_mutual_information_of_independent_and_identical_volumes():
    rng = np.random.default_rng(2)
    a, b = rng.uniform(size=64 ** 3).astype(np.float32), rng.uniform(size=64 ** 3).astype(np.float32)
    assert 0 <= HU.ref_mutual_information_3d(a, b, sigma=1, normalized=False) <= 0.01
    assert abs(HU.ref_mutual_information_3d(a, a, sigma=0, normalized=True) - 1.0) <= 1e-9


# ---- (2) argument checks that need no device -----------------------------------------------------------------------------------------------
def test_ops_argument_checks():
    from vae_segmentation_amd import ops
    x = torch.zeros((1, 1, 2, 3, 4))
    lab = torch.zeros((1, 1, 2, 3, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="4096 bins"):
        ops.histogram(x, 4097)
    with pytest.raises(ValueError, match="2\\^22"):
        ops.histogram(x, 4096, labels=lab, rows=1024)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="bins"):
            ops.histogram(x, bad)
    with pytest.raises(ValueError, match="lo <= hi"):
        ops.histogram(x, 8, range=(1.0, -1.0))
    with pytest.raises(ValueError, match="finite"):
        ops.histogram(x, 8, range=(0.0, float("inf")))
    with pytest.raises(ValueError, match="rows = 2 without labels"):
        ops.histogram(x, 8, rows=2)
    with pytest.raises(TypeError, match="float32"):
        ops.histogram(x.double(), 8)
    with pytest.raises(ValueError, match="planar"):
        ops.histogram(x[0], 8)
    with pytest.raises(ValueError, match="contiguous"):
        ops.histogram(x.transpose(3, 4), 8)
    with pytest.raises(TypeError, match="int32"):
        ops.histogram(x, 8, labels=lab.long(), rows=1)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.histogram(x, 8, labels=lab[:, :, :1].contiguous(), rows=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.histogram(x, 8)
    with pytest.raises(ValueError, match="2\\^22"):
        ops.joint_histogram(x, x, bins=(2049, 2048))
    with pytest.raises(ValueError, match="bins"):
        ops.joint_histogram(x, x, bins=(4, 0))
    with pytest.raises(ValueError, match="range"):
        ops.joint_histogram(x, x, range=(0.0, 1.0))
    with pytest.raises(ValueError, match="differ in shape"):
        ops.joint_histogram(x, x[..., :2].contiguous())
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.joint_histogram(x, x, bins=4, range=((0, 1), (0, 1)))
    t = torch.zeros((1, 1, 4, 4), dtype=torch.int64)
    for bad in (-1.0, float("nan"), float("inf"), 17.0, "1"):
        with pytest.raises(ValueError, match="sigma"):
            ops.mutual_information(t, sigma=bad)
    with pytest.raises(TypeError, match="int64"):
        ops.mutual_information(t.double())
    with pytest.raises(ValueError, match="bins_x, bins_y"):
        ops.mutual_information(t[0])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mutual_information(t)


def test_evaluation_argument_checks():
    from vae_segmentation_amd import evaluation
    v = torch.zeros((2, 3, 4))
    with pytest.raises(ValueError, match="mask's shape"):
        evaluation.histogram(v, 8, mask=torch.zeros((2, 3, 5)))
    with pytest.raises(ValueError, match="\\(D, H, W\\)"):
        evaluation.histogram(v[0], 8)
    with pytest.raises(TypeError, match="real-valued"):
        evaluation.histogram(v > 0, 8)
    with pytest.raises(ValueError, match="differ in shape"):
        evaluation.joint_histogram(v, torch.zeros((2, 3, 5)))
    with pytest.raises(ValueError, match="one non-empty shape"):
        evaluation.mutual_information_3d(v, torch.zeros((2, 3, 5)))
    with pytest.raises(TypeError, match="device tensors"):
        evaluation.mutual_information_3d(np.zeros(4), np.zeros(4))
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluation.mutual_information_3d(v, v)
    assert "fp64 before binning" in evaluation.mutual_information_3d.__doc__


def test_c_abi_answers_argument_errors_before_any_launch():
    """include/vaeseg.h: VS_EINVAL = -1, VS_ESHAPE = -2, VS_EALIGN = -5; the addresses are never dereferenced on these paths"""
    from vae_segmentation_amd import _lib
    lib = _lib.lib
    einval, eshape, ealign = -1, -2, -5
    A = 4096                                        # an aligned, never dereferenced address
    shape = (1, 1, 2, 3, 4)
    h = lib.vs_histogram
    assert h(None, None, *shape, 8, 0, -1.0, 1.0, 0, A, A, A, A, None) == einval
    assert h(A, None, *shape, 0, 0, -1.0, 1.0, 0, A, A, A, A, None) == einval
    assert h(A, None, *shape, 8, 1, -1.0, 1.0, 0, A, A, A, A, None) == einval            # rows without labels
    assert h(A, None, *shape, 8, 0, 1.0, -1.0, 0, A, A, A, A, None) == einval
    assert h(A, None, *shape, 8, 0, float("nan"), 1.0, 0, A, A, A, A, None) == einval
    assert h(A, None, *shape, 4097, 0, -1.0, 1.0, 0, A, A, A, A, None) == eshape
    assert h(A, A, *shape, 4096, 1024, -1.0, 1.0, 0, A, A, A, A, None) == eshape
    assert h(A, None, 1, 1, 0, 3, 4, 8, 0, -1.0, 1.0, 0, A, A, A, A, None) == eshape
    assert h(A, None, 1, 1, 2048, 1024, 1024, 8, 0, -1.0, 1.0, 0, A, A, A, A, None) == eshape
    assert h(A + 2, None, *shape, 8, 0, -1.0, 1.0, 0, A, A, A, A, None) == ealign
    assert h(A, None, *shape, 8, 0, -1.0, 1.0, 0, A + 4, A, A, A, None) == ealign
    j = lib.vs_joint_histogram
    r4 = (ctypes.c_double * 4)(-1.0, 1.0, -1.0, 1.0)
    R = ctypes.addressof(r4)
    assert j(A, None, *shape, 8, 8, R, 0, A, 2 * A, A, A, None) == einval
    assert j(A, A, *shape, 8, 8, None, 0, A, 2 * A, A, A, None) == einval                # host bounds asked for, none given
    assert j(A, A, *shape, 8, 8, R, 0, A, A, A, A, None) == einval                       # one buffer for both edge tables
    assert j(A, A, *shape, 2049, 2048, R, 0, A, 2 * A, A, A, None) == eshape
    assert j(A, A, *shape, 8, 8, R, 0, A, 2 * A, A + 4, A, None) == ealign
    bad = (ctypes.c_double * 4)(-1.0, 1.0, 2.0, 1.0)
    assert j(A, A, *shape, 8, 8, ctypes.addressof(bad), 0, A, 2 * A, A, A, None) == einval
    m = lib.vs_mutual_information
    assert m(None, 1, 1, 8, 8, 1.0, 1, A, A, None) == einval
    assert m(A, 1, 1, 8, 8, -1.0, 1, A, A, None) == einval
    assert m(A, 1, 1, 8, 8, float("nan"), 1, A, A, None) == einval
    assert m(A, 1, 1, 8, 8, 16.2, 1, A, A, None) == einval                                # radius 65
    assert m(A, 1, 1, 2049, 2048, 1.0, 1, A, A, None) == eshape
    assert m(A, 0, 1, 8, 8, 1.0, 1, A, A, None) == eshape
    assert m(A, 1, 1, 8, 8, 1.0, 1, A + 4, A, None) == ealign


def test_val_intensity_flag():
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    for mod, script in ((main_source, "main_source.py"), (main_target, "main_target.py")):
        assert mod.parse(["run"]).val_intensity == 0
        a = mod.parse(["run", "-M", "seg_train", "--val_intensity", "32", "--val_keep_largest", "1"])
        assert a.val_intensity == 32
        driver.check_intensity_flags(a, script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_intensity" % script):
            driver.check_intensity_flags(mod.parse(["run", "-M", "discriminator_train", "--val_intensity", "8"]), script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_intensity" % script):
            driver.check_intensity_flags(mod.parse(["run", "-M", "seg_train", "--val_intensity", "5000"]), script)
    with pytest.raises(SystemExit, match="--val_intensity"):
        driver.check_intensity_flags(main_target.parse(["run", "-M", "domain_adaptation", "--val_intensity", "8", "--val_finetune", "2"]), "main_target.py")
    assert driver.INTENSITY_RANGE == (-1.0, 1.0) and "nmi" in driver.INTENSITY_LOG_FIELDS
