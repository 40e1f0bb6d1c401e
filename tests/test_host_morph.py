"""Host-side checks of binary morphology and hole filling (no GPU): the mask generators of tests/morph_util.py, argument validation in ops,
evaluation and the C ABI, the entry points' --val_closing / --val_fill_holes flags and the one-hot bookkeeping of evaluation.postprocess."""
import ctypes

import numpy as np
import pytest
import torch

from tests import morph_util as MU


def test_shells_fill_as_stated():
    for drop, want6, want26 in ((None, 125, 125), ("corner", 124, 97), ("face", 97, 97)):
        m = MU.shell(drop)
        assert m.shape == (9, 9, 9) and int(m.sum()) == (98 if drop is None else 97)
        assert int(MU.ref_fill_holes(m, 6).sum()) == want6, drop
        assert int(MU.ref_fill_holes(m, 26).sum()) == want26, drop


def test_generators_give_what_they_claim():
    full = np.ones((4, 4, 4), bool)
    for conn in (6, 26):
        assert int(MU.ref_morph(full, "close", conn, 1, 0).sum()) == 8                                         # the border erodes what a dilation cannot grow
    assert int(MU.ref_morph(full, "open", 26, 1, 0).sum()) == 64 and int(MU.ref_morph(full, "open", 6, 1, 0).sum()) == 32
    assert int(MU.ref_morph(full, "close", 26, 1, 1).sum()) == 64
    m = MU.random_mask((12, 11, 70), 0.55, 2)
    assert int(MU.ref_fill_holes(m, 6).sum() - m.sum()) == 102 and int(MU.ref_fill_holes(m, 26).sum() - m.sum()) == 0
    m = MU.open_hole((9, 9, 20))
    assert np.array_equal(MU.ref_fill_holes(m, 6), m.astype(np.float32)) and (~m[4, 4, :]).sum() > 8           # the cavity is there and stays
    m = MU.nested_shells((14, 15, 16))
    want = np.zeros(m.shape, np.float32)
    want[1:-1, 1:-1, 1:-1] = 1
    assert np.array_equal(MU.ref_fill_holes(m, 6), want) and np.array_equal(MU.ref_fill_holes(m, 26), want) and m.sum() < want.sum()
    shape = (17, 16, 70)
    opened, closed = MU.serpentine_background(shape, True), MU.serpentine_background(shape, False)
    corridor = int((~closed).sum())
    assert corridor > 7 * 7 * 68 and int((~opened).sum()) == corridor + 1
    from scipy import ndimage
    assert ndimage.label(~closed, structure=MU.STRUCT[6])[1] == 1                                             # one corridor
    for conn in (6, 26):
        assert np.array_equal(MU.ref_fill_holes(opened, conn), opened.astype(np.float32))                       # reaches the border at one end only
        assert MU.ref_fill_holes(closed, conn).all()
    assert MU.corner_voxel((3, 4, 5)).sum() == 1 and MU.corner_voxel((3, 4, 5))[0, 0, 0]
    b = MU.flush_block((5, 7, 70))
    assert b[0, 0, 0] and b[0].any() and b[:, 0].any() and b[:, :, 0].any() and not b[-1].any() and not b[:, :, -1].any()


def test_bad_arguments_raise_before_the_device_check():
    from vae_segmentation_amd import evaluation, ops
    x5, x3 = torch.zeros(1, 1, 4, 5, 6), torch.zeros(4, 5, 6)
    with pytest.raises(ValueError, match="op"):
        ops.morph(x5, "dilation")
    for mod, x in ((ops, x5), (evaluation, x5), (evaluation, x3)):
        for name in ("binary_dilation", "binary_erosion", "binary_opening", "binary_closing"):
            f = getattr(mod, name)
            for kw in ({"connectivity": 18}, {"connectivity": 8}, {"connectivity": True}, {"iterations": 0}, {"iterations": -1}, {"iterations": 1.5},
                       {"iterations": None}, {"border_value": 2}):
                with pytest.raises(ValueError):
                    f(x, **kw)
            with pytest.raises(RuntimeError, match="GPU only"):
                f(x)
            with pytest.raises(RuntimeError, match="GPU only"):
                f(x, iterations=3, connectivity=26, border_value=1)
        with pytest.raises(ValueError, match="connectivity"):
            mod.fill_holes(x, connectivity=18)
        with pytest.raises(RuntimeError, match="GPU only"):
            mod.fill_holes(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.morph(x5, "close", iterations=2, connectivity=26)
    with pytest.raises(ValueError, match="shape"):
        evaluation.binary_dilation(torch.zeros(4, 5))
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluation.get_synthesis_mask({"venous": x3})
    with pytest.raises(ValueError, match="closing"):
        evaluation.postprocess(x5, closing=-1)


def test_the_library_answers_bad_arguments_on_the_host():
    from vae_segmentation_amd._lib import lib
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    a, b, ws = (ctypes.create_string_buffer(4096 + 16) for _ in range(3))
    pa, pb, pw = ((ctypes.addressof(x) + 15) & ~15 for x in (a, b, ws))
    ok = (1, 1, 2, 3, 4)

    def morph(mask=pa, out=pb, shape=ok, op=0, conn=6, it=1, border=0, w=pw):
        return lib.vs_morph(mask, out, *shape, op, conn, it, border, w, None)

    def fill(mask=pa, out=pb, shape=ok, conn=6, w=pw):
        return lib.vs_fill_holes(mask, out, *shape, conn, w, None)

    assert lib.vs_morph_workspace_bytes(*ok) > 0 and lib.vs_fill_holes_workspace_bytes(*ok, 6) >= 2 * 24 * 4
    assert lib.vs_morph_workspace_bytes(1, 2, 128, 128, 128) == 2 * 2 * 128 * 128 * 2 * 8                      # two packed planes: a bit per voxel each
    assert lib.vs_morph_workspace_bytes(1, 1, 0, 3, 4) == ESHAPE and lib.vs_morph_workspace_bytes(1, 1, 2048, 2048, 512) == ESHAPE
    assert lib.vs_fill_holes_workspace_bytes(*ok, 18) == EINVAL and lib.vs_fill_holes_workspace_bytes(1, 1, 2, 0, 4, 6) == ESHAPE
    for kw in ({"conn": 18}, {"conn": 0}, {"it": 0}, {"it": -3}, {"op": 4}, {"op": -1}, {"border": 2}, {"border": -1}, {"mask": None}, {"out": None},
               {"w": None}, {"out": pa}, {"w": pa}, {"w": pb}):
        assert morph(**kw) == EINVAL, kw
    for kw in ({"conn": 18}, {"mask": None}, {"out": None}, {"w": None}, {"out": pa}, {"w": pa}):
        assert fill(**kw) == EINVAL, kw
    assert morph(shape=(1, 1, 0, 3, 4)) == ESHAPE and fill(shape=(1, 0, 2, 3, 4)) == ESHAPE and morph(shape=(1, 1, 2048, 2048, 512)) == ESHAPE
    assert morph(w=pw + 8) == EALIGN and fill(w=pw + 8) == EALIGN


def test_val_closing_and_fill_holes_flags():
    import main_source
    import main_target
    from vae_segmentation_amd import driver
    for mod, script, side in ((main_source, "main_source.py", "source"), (main_target, "main_target.py", "target")):
        a = mod.parse(["run", "-M", "seg_train"])
        assert a.val_closing == 0 and a.val_fill_holes is False
        driver.check_whole_volume_flags(a, script)
        a = mod.parse(["run", "-M", "seg_train", "--val_closing", "2", "--val_fill_holes", "--val_keep_largest", "1"])
        assert a.val_closing == 2 and a.val_fill_holes is True and a.val_keep_largest == 1
        driver.check_whole_volume_flags(a, script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_closing" % script):
            driver.check_whole_volume_flags(mod.parse(["run", "-M", "seg_train", "--val_closing", "-1"]), script)
        with pytest.raises(SystemExit, match="%s: inconsistent flags.*--val_closing" % script):       # run() refuses before it touches a device
            driver.run(mod.parse(["run", "-M", "seg_train", "--val_closing", "-2"]), side=side)


class _CpuOps:
    """stand-ins for the three device ops of evaluation.postprocess, on CPU tensors, with a record of the calls"""

    def __init__(self):
        self.calls = []

    def binary_closing(self, x, iterations=1, connectivity=6, border_value=0):
        self.calls.append(("binary_closing", iterations, connectivity, border_value))
        return torch.from_numpy(MU.ref_morph(x.numpy(), "close", connectivity, iterations, border_value))

    def fill_holes(self, x, connectivity=6):
        self.calls.append(("fill_holes", connectivity))
        return torch.from_numpy(MU.ref_fill_holes(x.numpy(), connectivity))

    def keep_largest(self, x, **kw):
        self.calls.append(("keep_largest", kw))
        return x + 0


def _three_class_case(shape=(10, 14, 14)):
    """class 1: a shell whose cavity holds class-2 voxels and background; class 2 also has a shell of its own that encloses class-1 voxels and
    background; and one background voxel with class 1 on either side in y and class 2 on either side in x, which a closing of either would take"""
    d, h, w = shape
    lab = np.zeros(shape, np.int64)
    lab[1:8, 1:8, 1:8] = 1
    lab[2:7, 2:7, 2:7] = 0
    lab[3:5, 3:5, 3:5] = 2
    lab[1:8, 2:9, 9:13] = 2
    lab[2:7, 3:8, 10:12] = 0
    lab[4, 5, 10] = 1
    lab[5, 10, 5] = lab[5, 12, 5] = 1
    lab[5, 11, 4] = lab[5, 11, 6] = 2                                       # (5, 11, 5) lies in the closing of both
    hot = np.stack([(lab == c) for c in range(3)]).astype(np.float32)[None]
    return hot


def test_postprocess_bookkeeping(monkeypatch):
    from vae_segmentation_amd import evaluation, volume
    fake = _CpuOps()
    for name in ("binary_closing", "fill_holes", "keep_largest"):
        monkeypatch.setattr(volume, name, getattr(fake, name))
    hot = _three_class_case()
    x = torch.from_numpy(hot)
    # the no-op configuration is the driver's keep_largest call and nothing else
    out = evaluation.postprocess(x, keep_largest=2, min_size=5, lo_channel=1)
    assert fake.calls == [("keep_largest", dict(k=2, min_size=5, connectivity=26, lo_channel=1, to_background=True))]
    assert torch.equal(out, x)
    fake.calls.clear()
    assert evaluation.postprocess(x) is x and fake.calls == []
    for closing, fill in ((0, True), (1, False), (1, True), (2, True)):
        fake.calls.clear()
        out = evaluation.postprocess(x, closing=closing, fill_holes=fill, keep_largest=1).numpy()
        per_class = ([("binary_closing", closing, 26, 0)] if closing else []) + ([("fill_holes", 6)] if fill else [])
        assert fake.calls[:-1] == per_class * 2 and fake.calls[-1][0] == "keep_largest"                    # class 1, then class 2, then the filter
        assert np.array_equal(out.sum(1), np.ones_like(out[:, 0])) and set(np.unique(out)) <= {0.0, 1.0}     # one-hot
        assert np.array_equal(out, MU.ref_postprocess(hot, closing, fill))
        changed = out != hot
        assert changed.any()
        moved = changed.any(1)
        was_bg, is_bg = hot[:, 0] == 1, out[:, 0] == 1
        assert (was_bg | is_bg)[moved].all()                                                               # every move is to or from the background
        if closing == 0:
            assert was_bg[moved].all() and np.array_equal(out[:, 1:] >= hot[:, 1:], np.ones_like(out[:, 1:], bool))
    assert torch.equal(x, torch.from_numpy(hot))                                                           # the input is left alone
    # the lowest class wins a voxel both would take
    out = evaluation.postprocess(x, closing=1).numpy()
    alone2 = MU.ref_morph(hot[0, 2], "close", 26, 1, 0)
    alone1 = MU.ref_morph(hot[0, 1], "close", 26, 1, 0)
    contested = (alone1 == 1) & (alone2 == 1) & (hot[0, 0] == 1)
    assert contested[5, 11, 5] and (out[0, 1][contested] == 1).all() and (out[0, 2][contested] == 0).all()
