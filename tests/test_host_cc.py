"""Host-side checks of the connected-component feature (no GPU): the golden fixture, the C ABI's declarations and argument validation,
and the entry points' flags."""
import os

import numpy as np
from scipy import ndimage

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "cc.npz")


def load_golden():
    """-> [(name, bool mask, reference label per foreground voxel in raster order)]"""
    z = np.load(GOLDEN, allow_pickle=False)
    out = []
    for name in z["names"]:
        shape = tuple(int(s) for s in z[name + "/shape"])
        mask = np.unpackbits(z[name + "/bits"])[:int(np.prod(shape))].astype(bool).reshape(shape)
        out.append((str(name), mask, z[name + "/labels"].astype(np.int32)))
    return out


def test_golden_is_self_consistent_with_scipy():
    """The reference's check_connection(np.argwhere(mask), mask) numbers components by their first voxel in raster order, exactly as
    scipy.ndimage.label with the 3x3x3 structure does: the rule the GPU tests rely on when they compare labels bit for bit."""
    cases = load_golden()
    assert len(cases) >= 10
    assert sum(int(lab.max()) > 1 for _, _, lab in cases) >= 5             # several masks with more than one component
    for name, mask, ref in cases:
        lab, k = ndimage.label(mask, structure=np.ones((3, 3, 3)))
        assert ref.shape == (int(mask.sum()),), name
        assert k == int(ref.max()), name
        assert np.array_equal(lab[mask], ref), name


def test_header_declares_the_three_entry_points():
    import ctypes
    from vae_segmentation_amd import _lib
    protos = _lib.parse_header()
    assert protos["vs_cc_workspace_bytes"] == (ctypes.c_longlong, [ctypes.c_int] * 6)
    assert protos["vs_cc_label"] == (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2)
    assert protos["vs_cc_keep_largest"] == (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] * 10 + [ctypes.c_void_p] * 2)
    for path in (_lib.LIB_PATH, _lib.DET_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in ("vs_cc_workspace_bytes", "vs_cc_label", "vs_cc_keep_largest"):
            assert hasattr(raw, name), (path, name)


def test_argument_validation_without_gpu():
    from vae_segmentation_amd._lib import lib
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    # workspace sizing is host arithmetic: it grows with the volume, and the 6-connected size table (V / 2 rows) is the larger one
    a, b = lib.vs_cc_workspace_bytes(1, 2, 64, 64, 64, 26), lib.vs_cc_workspace_bytes(1, 2, 128, 128, 128, 26)
    assert 0 < a < b and lib.vs_cc_workspace_bytes(1, 2, 64, 64, 64, 6) > a
    assert a >= 2 * 2 * 64 ** 3 * 4                                             # parent + labels
    assert lib.vs_cc_workspace_bytes(1, 1, 5, 6, 7, 26) > 0
    assert lib.vs_cc_workspace_bytes(1, 1, 8, 8, 8, 18) == EINVAL
    assert lib.vs_cc_workspace_bytes(1, 1, 0, 8, 8, 26) == ESHAPE
    assert lib.vs_cc_workspace_bytes(1, 1, 2048, 1024, 1024, 26) == ESHAPE       # a plane of 2^31 voxels
    assert lib.vs_cc_workspace_bytes(1, 1, 2047, 1024, 1024, 26) > 0
    # null pointers, no device: the argument checks come first
    assert lib.vs_cc_label(None, None, None, 1, 1, 8, 8, 8, 18, None, None) == EINVAL
    assert lib.vs_cc_label(None, None, None, 1, 1, 8, 8, 8, 26, None, None) == EINVAL
    assert lib.vs_cc_label(None, None, None, 1, 1, 2048, 1024, 1024, 26, None, None) == ESHAPE
    assert lib.vs_cc_label(None, None, None, 0, 1, 8, 8, 8, 26, None, None) == ESHAPE
    assert lib.vs_cc_keep_largest(None, None, 1, 2, 8, 8, 8, 7, 1, 0, 0, 0, None, None) == EINVAL        # connectivity
    assert lib.vs_cc_keep_largest(None, None, 1, 2, 8, 8, 8, 26, -1, 0, 0, 0, None, None) == EINVAL      # k
    assert lib.vs_cc_keep_largest(None, None, 1, 2, 8, 8, 8, 26, 1, 0, 2, 0, None, None) == EINVAL       # lo_channel == c
    assert lib.vs_cc_keep_largest(None, None, 1, 2, 8, 8, 8, 26, 1, 0, -1, 0, None, None) == EINVAL
    assert lib.vs_cc_keep_largest(None, None, 1, 2, 8, 8, -8, 26, 1, 0, 0, 0, None, None) == ESHAPE
    assert lib.vs_cc_keep_largest(None, None, 1, 2, 2048, 1024, 1024, 26, 1, 0, 0, 0, None, None) == ESHAPE
    # fake, never dereferenced pointers: alignment and aliasing are refused before any launch
    fake = 0x10000
    assert lib.vs_cc_label(fake + 4, fake, fake, 1, 1, 8, 8, 8, 26, fake, None) == EALIGN
    assert lib.vs_cc_keep_largest(fake, fake, 1, 2, 8, 8, 8, 26, 1, 0, 0, 0, fake, None) == EINVAL       # out aliases mask


def test_cc_max_components_matches_the_header_rule():
    from vae_segmentation_amd import ops
    assert ops.cc_max_components(5, 6, 7, 26) == 3 * 3 * 4
    assert ops.cc_max_components(5, 6, 7, 6) == 105
    assert ops.cc_max_components(1, 1, 300, 26) == 150


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from vae_segmentation_amd import evaluation, ops
    x = torch.zeros(1, 1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.cc_label(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.keep_largest(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluation.keep_largest_components(x)
    import utils.evaluation as UE
    assert UE.keep_largest_components is evaluation.keep_largest_components and UE.check_connection is evaluation.check_connection


def test_save_eval_result_is_no_longer_ignored(capsys):
    import main_target
    a = main_target.parse(["r", "--save_eval_result"])
    assert a.save_eval_result
    assert "accepted and ignored" not in capsys.readouterr().err
    main_target.parse(["r", "--save_eval_result", "--save_more_reference"])
    err = capsys.readouterr().err
    assert "accepted and ignored" in err and "--save_more_reference" in err and "--save_eval_result" not in err
    assert "save_eval_result" not in main_target.__doc__.split("accepted with a warning")[0]


def test_validation_filter_flags_default_to_off():
    import main_source
    import main_target
    for mod in (main_source, main_target):
        a = mod.parse(["r"])
        assert a.val_keep_largest == 0 and a.val_min_component == 0
        a = mod.parse(["r", "--val_keep_largest", "2", "--val_min_component", "10000"])
        assert a.val_keep_largest == 2 and a.val_min_component == 10000
