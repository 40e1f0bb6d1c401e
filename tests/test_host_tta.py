"""Host-side checks of mirror test-time augmentation (no GPU): evaluation.tta_flips, the flip list's validation in ops and in the C ABI, the numpy
restatement of tests/tta_util.py against tests/sliding_util.py, and the entry points' --val_tta flag."""
import ctypes

import numpy as np
import pytest

from tests import sliding_util as SW
from tests import tta_util as TTA


def test_tta_flips():
    from vae_segmentation_amd import evaluation
    f = evaluation.tta_flips
    assert f("w") == (0, 1) and f("h") == (0, 2) and f("d") == (0, 4)
    assert f("hd") == f("dh") == (0, 2, 4, 6) and f("hw") == (0, 1, 2, 3) and f("dhw") == f("wdh") == tuple(range(8))
    assert f(None) is None and f("") is None and f(()) is None
    assert f((0, 5)) == (0, 5) and f([3]) == (3,) and f((7, 0, 2)) == (7, 0, 2)               # explicit codes pass through, in their order
    for axes in ("w", "hd", "dhw", "dw"):
        assert f(axes) == TTA.flips_of(axes)
    for bad in ("x", "ww", "dhwd", "DHW", (0, 0), (8,), (-1,), tuple(range(8)) + (0,), 3, (0.5,)):
        with pytest.raises(ValueError):
            f(bad)


def test_flip_lists_are_validated_before_anything_is_launched():
    import torch
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import lib
    assert ops.sw_flips((0,)) == (1, 0) and ops.sw_flips((0, 1)) == (2, 1 << 3) and ops.sw_flips((7, 0, 2)) == (3, 7 | 2 << 6)
    assert ops.sw_flips(range(8)) == (8, sum(c << 3 * c for c in range(8)))
    vol = torch.zeros(1, 8, 8, 8)
    origins, first = torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    wt = ops.sw_weights(8, "constant", device="cpu")
    for bad in ((), (0, 0), (8,), (-1,), (0, 1, 1), tuple(range(8)) + (0,), "w"):
        with pytest.raises(ValueError, match="flips"):
            ops.sw_gather(vol, origins, first, 1, patch=8, flips=bad)
        with pytest.raises(ValueError, match="flips"):
            ops.sw_accumulate(torch.zeros(1, 2, 8, 8, 8), torch.zeros(2, 8, 8, 8), torch.zeros(8, 8, 8), origins, first, wt, flips=bad)
    with pytest.raises(RuntimeError, match="GPU only"):                                        # a good list reaches the device check, as without flips
        ops.sw_gather(vol, origins, first, 1, patch=8, flips=(0, 1))
    # the C ABI: refusals decided on the host
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    a = 1 << 20                                                                                # never dereferenced
    gather = lambda nf, codes, nw=1, vol=a: lib.vs_sw_gather_tta(vol, 2 * a, a, a, nw, 1, 1, 8, 8, 8, 4, 0.0, nf, codes, None)
    accum = lambda nf, codes, nw=1, acc=2 * a: lib.vs_sw_accumulate_tta(a, acc, 3 * a, a, a, nw, 1, 2, 8, 8, 8, 4, a, a, a, nf, codes, None)
    for call in (gather, accum):
        assert call(0, 0) == EINVAL and call(9, 0) == EINVAL and call(-1, 0) == EINVAL
        assert call(2, 0) == EINVAL                                                            # code 0 twice
        assert call(3, 1 | 2 << 3 | 1 << 6) == EINVAL
        assert call(1, 1 << 3) == EINVAL and call(2, 1 << 3 | 1 << 6) == EINVAL and call(2, -1) == EINVAL      # bits above the list
        assert call(8, sum(c << 3 * c for c in range(8)), nw=(1 << 28)) == ESHAPE              # nw * nf passes INT_MAX
    assert gather(2, 1 << 3, vol=None) == EINVAL and gather(2, 1 << 3, vol=a + 4) == EALIGN
    assert accum(2, 1 << 3, acc=a) == EINVAL and accum(2, 1 << 3, acc=2 * a + 8) == EALIGN


def test_header_declares_the_entry_points():
    from vae_segmentation_amd import _lib
    protos = _lib.parse_header()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert protos["vs_sw_gather_tta"] == (ci, [vp] * 4 + [ci] * 7 + [ctypes.c_float, ci, ci, vp])
    assert protos["vs_sw_accumulate_tta"] == (ci, [vp] * 5 + [ci] * 7 + [vp] * 3 + [ci, ci, vp])
    assert protos["vs_sw_gather"] == (ci, [vp] * 4 + [ci] * 7 + [ctypes.c_float, vp])          # the plain calls keep their signatures
    assert protos["vs_sw_accumulate"] == (ci, [vp] * 5 + [ci] * 7 + [vp] * 4)
    for path in (_lib.LIB_PATH, _lib.DET_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in ("vs_sw_gather_tta", "vs_sw_accumulate_tta"):
            assert hasattr(raw, name), (path, name)


def pointwise_np(batch):
    s = batch[:, 0].astype(np.float64)
    e = np.exp(np.stack([s, -s, 0.5 * s * s], 1))
    return e / e.sum(1, keepdims=True)


def analytic_np(batch):
    """linear terms in local z, y and x: the answer depends on where in the window a voxel sits, so every single mirror changes it"""
    p = batch.shape[-1]
    i = np.arange(p, dtype=np.float64) / p
    z, y, x = i.reshape(p, 1, 1), i.reshape(1, p, 1), i.reshape(1, 1, p)
    s = batch.sum(1).astype(np.float64)
    e = np.exp(np.stack([s * (1.0 + 2.0 * z - y), s * (0.5 - z + 1.5 * x) + 0.25 * y, -s * (0.3 + y * x) + z], 1))
    return e / e.sum(1, keepdims=True)


CASES = [((17, 21, 19), 8, 0.5, "gaussian", 0.0), ((6, 20, 5), 8, 0.75, "constant", -7.5), ((2, 9, 12, 10), 8, 0.25, "gaussian", 0.0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_restatement_against_the_plain_one(case):
    """a pointwise model commutes with every mirror, so un-mirroring its answer gives the un-mirrored answer and the average over any flips is the
    plain prediction (1e-12: float64 sums in another order); wsum32 is nf equal fp32 additions per window.  The position-dependent model does not
    commute: any single flip moves the result."""
    shape, patch, overlap, blend, cval = case
    vol = (np.random.RandomState(sum(shape)).randn(*shape) * 1.5).astype(np.float32)
    plain = SW.predict(pointwise_np, vol, patch, overlap, blend, cval)
    cover = int(round(float((SW.blend([np.ones((1, patch, patch, patch))] * len(plain["origins"]), plain["origins"], shape[-3:],
                                      SW.weights(patch, "constant"))[3]).max())))
    for flips in ((0,), (1,), (0, 2), (4, 0), (0, 1, 2, 3), tuple(range(8)), (5, 3, 6)):
        got = TTA.predict(pointwise_np, vol, patch, overlap, blend, cval, flips)
        assert np.array_equal(got["origins"], plain["origins"]) and got["terms"] == cover * len(flips)
        assert float(np.abs(got["prob"] - plain["prob"]).max()) <= 1e-12, flips
        if flips == (0,):
            assert np.array_equal(got["wsum32"], plain["wsum32"])
        # both fp32 sums round each of their at most `terms` additions by half an ulp of a running sum that the final sum bounds
        assert np.allclose(got["wsum32"], len(flips) * plain["wsum32"].astype(np.float64), rtol=got["terms"] * 2.0 ** -23, atol=0)
    base = SW.predict(analytic_np, vol, patch, overlap, blend, cval)
    same = TTA.predict(analytic_np, vol, patch, overlap, blend, cval, (0,))
    assert np.array_equal(same["prob"], base["prob"]) and np.array_equal(same["wsum32"], base["wsum32"])
    for flips in ((1,), (2,), (4,), (0, 1), (0, 2), (0, 4), tuple(range(8))):
        moved = TTA.predict(analytic_np, vol, patch, overlap, blend, cval, flips)
        assert float(np.abs(moved["prob"] - base["prob"]).max()) > 1e-3, flips


def test_gather_mirrors_the_whole_padded_window():
    vol = np.arange(2 * 5 * 8 * 3, dtype=np.float32).reshape(2, 5, 8, 3)
    plain = SW.gather(vol, (0, 0, 0), 8, -7.5)
    assert (plain[:, 5:] == -7.5).all() and (plain[:, :, :, 3:] == -7.5).all()
    for code in range(8):
        w = TTA.gather(vol, (0, 0, 0), 8, -7.5, code)
        z, y, x = np.indices((8, 8, 8))
        fz, fy, fx = (7 - z if code & 4 else z), (7 - y if code & 2 else y), (7 - x if code & 1 else x)
        assert np.array_equal(w, plain[:, fz, fy, fx])
        if code & 4:
            assert (w[:, :3] == -7.5).all() and w[0, 7, 0 if not code & 2 else 7, 0 if not code & 1 else 7] == 0.0      # the padding lands at the low end
        assert np.array_equal(TTA.mirror(w, code), plain)                                                   # a mirror is its own inverse


def test_val_tta_flag():
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    for mod, script, side in ((main_source, "main_source.py", "source"), (main_target, "main_target.py", "target")):
        a = mod.parse(["run", "-M", "seg_train"])
        assert a.val_tta is None
        driver.check_whole_volume_flags(a, script)
        a = mod.parse(["run", "-M", "seg_train", "--real_data", "--val_whole_volume", "--val_tta", "hw"])
        assert a.val_tta == "hw"
        driver.check_whole_volume_flags(a, script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_tta.*--val_whole_volume" % script):
            driver.check_whole_volume_flags(mod.parse(["run", "-M", "seg_train", "--real_data", "--val_tta", "hw"]), script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_tta" % script):     # run() refuses before it touches a device
            driver.run(mod.parse(["run", "-M", "seg_train", "--real_data", "--val_tta", "dhw"]), side=side)
        with pytest.raises(SystemExit, match="inconsistent flags.*--val_tta.*dhw"):
            driver.check_whole_volume_flags(mod.parse(["run", "-M", "seg_train", "--real_data", "--val_whole_volume", "--val_tta", "xy"]), script)
