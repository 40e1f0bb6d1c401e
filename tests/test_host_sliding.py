"""Host-side checks of the sliding-window feature (no GPU): the window plan and the importance map — the numpy restatement of tests/sliding_util.py
and the library's own host planner against it —, the C ABI's declarations and argument validation, the CPU refusals and the entry points' flags."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import sliding_util as SW

SIZES, PATCHES, OVERLAPS = (17, 32, 33, 96, 130), (16, 32), (0, 0.25, 0.5, 0.75)


@pytest.mark.parametrize("p", PATCHES)
@pytest.mark.parametrize("s", SIZES)
def test_axis_plan_properties(s, p):
    for overlap in OVERLAPS:
        o = SW.axis_origins(s, p, overlap)
        assert all(0 <= v <= max(s - p, 0) for v in o), (s, p, overlap, o)
        assert all(a <= b for a, b in zip(o, o[1:])), (s, p, overlap, o)
        if s >= p:
            assert o[-1] + p == s, (s, p, overlap, o)
        covered = np.zeros(s, bool)
        for v in o:
            covered[v:v + p] = True
        assert covered.all(), (s, p, overlap, o)
        step = max(1, int(np.floor(p * (1 - overlap))))
        assert len(o) == (1 if s <= p else -(-(s - p) // step) + 1)
        assert all(b - a <= step for a, b in zip(o, o[1:]))


@pytest.mark.parametrize("p", PATCHES)
def test_plan_covers_the_volume_and_weight_sums_are_positive(p):
    """three axes of different sizes at once: D-major order, every voxel covered, the restated weight sums > 0 everywhere for both blends"""
    for shape, overlap in (((17, 33, 40), 0.5), ((33, 17, 32), 0.25), ((40, 34, 17), 0.75), ((32, 33, 35), 0)):
        origins = SW.plan(shape, p, overlap)
        per_axis = [SW.axis_origins(s, p, overlap) for s in shape]
        assert origins.dtype == np.int32 and origins.shape == (len(per_axis[0]) * len(per_axis[1]) * len(per_axis[2]), 3)
        assert origins.tolist() == [list(t) for t in itertools.product(*per_axis)]
        assert origins.tolist() == sorted(origins.tolist())                       # non-decreasing, D-major then H then W
        for blend in ("constant", "gaussian"):
            wt = SW.weights(p, blend)
            ones = [np.ones((1, p, p, p))] * len(origins)
            prob, wsum32, acc, wsum = SW.blend(ones, origins, shape, wt)
            assert (wsum > 0).all() and (wsum32 > 0).all(), (shape, p, overlap, blend)
            assert np.allclose(prob, 1.0, rtol=0, atol=1e-12)
            if blend == "constant":                                              # the weight sum counts the windows over a voxel
                count = np.zeros(shape)
                for oz, oy, ox in origins:
                    count[oz:oz + p, oy:oy + p, ox:ox + p] += 1
                assert np.array_equal(wsum, count) and np.array_equal(wsum32, count.astype(np.float32))


@pytest.mark.parametrize("p", PATCHES + (96, 7))
def test_gaussian_table(p):
    wt = SW.weights(p, "gaussian")
    assert wt.dtype == np.float32 and wt.shape == (3, p)
    row = wt[0]
    assert np.array_equal(wt[1], row) and np.array_equal(wt[2], row)
    assert np.array_equal(row, row[::-1])
    assert row.min() >= np.float32(1e-3) and row.max() <= 1.0
    i = np.arange(p, dtype=np.float64)
    want = np.maximum(np.exp(-0.5 * ((i - (p - 1) / 2.0) / (p / 8.0)) ** 2), 1e-3)
    assert np.array_equal(row, want.astype(np.float32))
    # the Gaussian peaks at 1 at the window's centre (P - 1) / 2: on a sample for odd P; for even P the centre lies between the two middle samples, which
    # then share the maximum exp(-(4 / P)^2 / 2) of the table (0.969 at P = 16, 0.992 at P = 32) — the formula is the specification, so that is what is checked
    assert row.max() == row[p // 2] == row[(p - 1) // 2]
    assert all(a <= b for a, b in zip(row[:(p - 1) // 2], row[1:]))              # rises monotonically up to the centre
    if p % 2:
        assert row[p // 2] == 1.0
    else:
        assert row.max() == np.float32(np.exp(-0.5 * (4.0 / p) ** 2)) and row.max() < 1.0
    assert np.array_equal(SW.weights(p, "constant"), np.ones((3, p), np.float32))
    w3 = SW.window_weight(wt)
    assert w3.dtype == np.float32 and w3.min() >= np.float32(1e-3) ** 3 * 0.999 and w3.max() <= 1.0


def test_library_planner_and_weights_equal_the_restatement():
    """ops.sw_plan_host (vs_sw_plan, pure C on the host) and ops.sw_weights(device='cpu')"""
    from vae_segmentation_amd import ops
    for s, p, overlap in itertools.product(SIZES, PATCHES, OVERLAPS):
        shape = (s, SIZES[(SIZES.index(s) + 1) % len(SIZES)], 40)
        got = ops.sw_plan_host(shape, p, overlap)
        assert got.dtype == np.int32 and np.array_equal(got, SW.plan(shape, p, overlap)), (shape, p, overlap)
    assert np.array_equal(ops.sw_plan_host((20, 20, 20), 8, 0.99), SW.plan((20, 20, 20), 8, 0.99))      # step floors to 0 -> 1
    assert len(ops.sw_plan_host((20, 20, 20), 8, 0.99)) == 13 ** 3
    for p in PATCHES + (96, 7):
        for blend in ("constant", "gaussian"):
            got = ops.sw_weights(p, blend, device="cpu")
            assert got.dtype.is_floating_point and got.element_size() == 4 and np.array_equal(got.numpy(), SW.weights(p, blend))
    with pytest.raises(ValueError):
        ops.sw_weights(16, "triangle", device="cpu")


def test_header_declares_the_entry_points():
    from vae_segmentation_amd import _lib
    protos = _lib.parse_header()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert protos["vs_sw_plan"] == (ci, [ci] * 4 + [ctypes.c_double, vp, ci])
    assert protos["vs_sw_gather"] == (ci, [vp] * 4 + [ci] * 7 + [ctypes.c_float, vp])
    assert protos["vs_sw_accumulate"] == (ci, [vp] * 5 + [ci] * 7 + [vp] * 4)
    assert protos["vs_sw_finalize"] == (ci, [vp] * 5 + [ci] * 4 + [vp])
    for path in (_lib.LIB_PATH, _lib.DET_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in ("vs_sw_plan", "vs_sw_gather", "vs_sw_accumulate", "vs_sw_finalize"):
            assert hasattr(raw, name), (path, name)


def test_argument_validation_without_gpu():
    """every refusal below is decided on the host before anything is launched"""
    from vae_segmentation_amd._lib import lib
    EINVAL, ESHAPE, EWORKSPACE, EALIGN = -1, -2, -4, -5
    assert lib.vs_sw_plan(0, 8, 8, 4, 0.5, None, 0) == EINVAL
    assert lib.vs_sw_plan(8, 8, 8, 0, 0.5, None, 0) == EINVAL
    assert lib.vs_sw_plan(8, 8, 8, 4, 1.0, None, 0) == EINVAL
    assert lib.vs_sw_plan(8, 8, 8, 4, -0.1, None, 0) == EINVAL
    assert lib.vs_sw_plan(8, 8, 8, 4, float("nan"), None, 0) == EINVAL
    assert lib.vs_sw_plan(2048, 2048, 2048, 4, 0.5, None, 0) == EINVAL        # 2^33 voxels
    assert lib.vs_sw_plan(8, 8, 8, 4, 0.5, None, 0) == 27
    table = (ctypes.c_int * 81)()
    assert lib.vs_sw_plan(8, 8, 8, 4, 0.5, ctypes.addressof(table), 26) == EWORKSPACE
    assert lib.vs_sw_plan(8, 8, 8, 4, 0.5, ctypes.addressof(table), 27) == 27 and list(table[:6]) == [0, 0, 0, 0, 0, 2] and list(table[78:]) == [4, 4, 4]
    a = 1 << 20                                                               # never dereferenced: the calls return before a launch
    assert lib.vs_sw_gather(None, a, a, a, 1, 1, 1, 8, 8, 8, 4, 0.0, None) == EINVAL
    assert lib.vs_sw_gather(a, 2 * a, a, a, 0, 1, 1, 8, 8, 8, 4, 0.0, None) == EINVAL
    assert lib.vs_sw_gather(a, 2 * a, a, a, 1, 0, 1, 8, 8, 8, 4, 0.0, None) == EINVAL
    assert lib.vs_sw_gather(a, 2 * a, a, a, 1, 1, 1, 8, 0, 8, 4, 0.0, None) == ESHAPE
    assert lib.vs_sw_gather(a, 2 * a, a, a, 1, 1, 1, 2048, 2048, 2048, 4, 0.0, None) == ESHAPE
    assert lib.vs_sw_gather(a + 4, 2 * a, a, a, 1, 1, 1, 8, 8, 8, 4, 0.0, None) == EALIGN
    assert lib.vs_sw_gather(a, a, a, a, 1, 1, 1, 8, 8, 8, 4, 0.0, None) == EINVAL
    assert lib.vs_sw_accumulate(a, 2 * a, 3 * a, a, a, 1, 1, 0, 8, 8, 8, 4, a, a, a, None) == EINVAL
    assert lib.vs_sw_accumulate(a, 2 * a, 3 * a, a, a, 1, 1, 2, 8, 8, 8, 4, None, a, a, None) == EINVAL
    assert lib.vs_sw_accumulate(a, a, 3 * a, a, a, 1, 1, 2, 8, 8, 8, 4, a, a, a, None) == EINVAL
    assert lib.vs_sw_accumulate(a, 2 * a + 8, 3 * a, a, a, 1, 1, 2, 8, 8, 8, 4, a, a, a, None) == EALIGN
    assert lib.vs_sw_finalize(a, 2 * a, 3 * a, None, None, 256, 8, 8, 8, None) == EINVAL
    assert lib.vs_sw_finalize(a, 2 * a, 3 * a, None, None, 0, 8, 8, 8, None) == EINVAL
    assert lib.vs_sw_finalize(a, None, 3 * a, None, None, 2, 8, 8, 8, None) == EINVAL
    assert lib.vs_sw_finalize(a, 2 * a, 3 * a, None, None, 2, 8, -1, 8, None) == ESHAPE
    assert lib.vs_sw_finalize(a, 2 * a, 3 * a, 4 * a + 1, None, 2, 8, 8, 8, None) == EALIGN


def test_cpu_tensors_are_refused():
    import torch
    from vae_segmentation_amd import evaluation, ops
    vol = torch.zeros(1, 8, 8, 8)
    origins, first = torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    wt = ops.sw_weights(8, "constant", device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sw_gather(vol, origins, first, 1, patch=8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sw_accumulate(torch.zeros(1, 2, 8, 8, 8), torch.zeros(2, 8, 8, 8), torch.zeros(8, 8, 8), origins, first, wt)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sw_finalize(torch.zeros(2, 8, 8, 8), torch.ones(8, 8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluation.sliding_window_predict(lambda x: x, vol, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluation.localise(torch.zeros(2, 8, 8, 8))


def test_entry_point_flags():
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    for mod, script in ((main_source, "main_source.py"), (main_target, "main_target.py")):
        a = mod.parse(["run", "-M", "seg_train"])
        assert a.val_whole_volume is False and a.sw_overlap == 0.5 and a.sw_batch == 1 and a.sw_blend == "gaussian"
        driver.check_whole_volume_flags(a, script)                               # off: nothing to check
        a = mod.parse(["run", "-M", "seg_train", "--real_data", "--val_whole_volume", "--sw_overlap", "0.25", "--sw_batch", "3", "--sw_blend", "constant"])
        assert a.val_whole_volume and a.sw_overlap == 0.25 and a.sw_batch == 3 and a.sw_blend == "constant"
        driver.check_whole_volume_flags(a, script)
        with pytest.raises(SystemExit, match="inconsistent flags.*--real_data"):
            driver.check_whole_volume_flags(mod.parse(["run", "-M", "seg_train", "--val_whole_volume"]), script)
        for method in ("vae_train", "discriminator_train"):
            with pytest.raises(SystemExit, match="inconsistent flags.*segmentation network"):
                driver.check_whole_volume_flags(mod.parse(["run", "-M", method, "--real_data", "--val_whole_volume"]), script)
        with pytest.raises(SystemExit, match="inconsistent flags.*sw_overlap"):
            driver.check_whole_volume_flags(mod.parse(["run", "-M", "seg_train", "--real_data", "--val_whole_volume", "--sw_overlap", "1"]), script)
        with pytest.raises(SystemExit):
            mod.parse(["run", "--sw_blend", "triangle"])
    with pytest.raises(SystemExit, match="main_target.py: inconsistent flags"):       # run() refuses before it touches a device
        driver.run(main_target.parse(["run", "-M", "domain_adaptation", "--val_whole_volume"]), side="target")
