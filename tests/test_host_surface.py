"""Host-side checks of the surface-distance feature (no GPU): the oracle of tests/surface_util.py against known answers and a brute force,
the C ABI's declarations and argument validation, and the entry points' flag."""
import ctypes
import math

import numpy as np
import pytest

from tests import surface_util as SU


def test_two_single_voxels_are_five_apart():
    """A = {(1, 1, 2)}, B = {(1, 4, 6)}: offsets (0, 3, 4), a 3-4-5 triangle.  A single voxel is its own surface, each directed set is {5}:
    ASSD = HD = HD95 = 5, squared statistics 25."""
    a, b = SU.two_voxels()
    for conn in (6, 26):
        m = SU.metrics(a, b, connectivity=conn)
        assert (m["count_ab"], m["count_ba"], m["max_sq"], m["lo_sq"], m["hi_sq"]) == (1, 1, 25, 25, 25)
        assert m["assd"] == 5.0 and m["hd"] == 5.0 and m["hd95"] == 5.0 and m["sum_ab"] == 5.0 and m["sum_ba"] == 5.0


def test_identical_masks_are_zero_apart():
    a = np.zeros((7, 8, 9), bool)
    a[1:6, 2:7, 3:8] = True
    m = SU.metrics(a, a.copy())
    assert m["count_ab"] == m["count_ba"] == 5 ** 3 - 3 ** 3
    assert m["assd"] == 0.0 and m["hd"] == 0.0 and m["hd95"] == 0.0 and m["max_sq"] == 0


def test_cube_against_the_cube_shifted_along_x():
    """A = a cube of side s = 4 at x in [0, 3] (coordinates relative to the cube), B = the same cube at x in [6, 9] (t = 6 >= s: disjoint).
    6-connectivity: the surface of a cube of side 4 is its shell, 4^3 - 2^3 = 56 voxels: 16 in each of the slices x = 0 and x = 3, 4 s - 4 = 12 in each of
    x = 1, 2.  The whole face x = 6 of B belongs to S(B), so the voxel of S(B) nearest to (x, y, z) in S(A) is (6, y, z): d = 6 - x.
      d(A->B): 16 x 6, 12 x 5, 12 x 4, 16 x 3   sum 96 + 60 + 48 + 48 = 252, mean 4.5;   d(B->A) is the mirror image, the same multiset.
      ASSD = 4.5, HD = 6.  Union, n = 112, ascending: 32 threes, 24 fours, 24 fives, 32 sixes; h = 0.95 * 111 = 105.45, k = 105: v[105] = v[106] = 6 -> HD95 = 6."""
    a, b = SU.shifted_cubes(4, 6)
    m = SU.metrics(a, b)
    assert (m["count_ab"], m["count_ba"]) == (56, 56)
    assert m["sum_ab"] == 252.0 and m["sum_ba"] == 252.0
    assert m["assd"] == 4.5 and m["hd"] == 6.0 and m["hd95"] == 6.0
    assert (m["max_sq"], m["lo_sq"], m["hi_sq"]) == (36, 36, 36)
    # t = 5: distances 5 - x -> 16 x 5, 12 x 4, 12 x 3, 16 x 2 per direction, sum 196, mean 3.5; k = 105 again falls into the 32 fives
    m = SU.metrics(*SU.shifted_cubes(4, 5))
    assert m["sum_ab"] == 196.0 and m["assd"] == 3.5 and m["hd"] == 5.0 and m["hd95"] == 5.0
    # 26-connectivity gives the same shell for a cube
    assert np.array_equal(SU.surface(a, 26), SU.surface(a, 6)) and int(SU.surface(a, 6).sum()) == 56


def test_anisotropic_spacing_changes_the_nearest_voxel():
    """A = {p}, B = {p + (1, 0, 0), p + (0, 2, 0)}, spacing (2.5, 0.8, 0.8): the z neighbour is 2.5 away, the y one 1.6 (unit spacing: 1 and 2).
      d(A->B) = {1.6}, d(B->A) = {2.5, 1.6}: ASSD = (1.6 + 2.05) / 2 = 1.825, HD = 2.5.
      Union ascending {1.6, 1.6, 2.5}: h = 0.95 * 2 = 1.9, k = 1 -> HD95 = 1.6 + 0.9 * 0.9 = 2.41."""
    a, b = SU.anisotropic()
    m = SU.metrics(a, b, spacing=SU.ANISO_SPACING)
    assert (m["count_ab"], m["count_ba"]) == (1, 2)
    assert m["assd"] == pytest.approx(1.825, rel=1e-14) and m["hd"] == pytest.approx(2.5, rel=1e-14) and m["hd95"] == pytest.approx(2.41, rel=1e-14)
    assert m["lo_sq"] == pytest.approx(2.56, rel=1e-14) and m["hi_sq"] == pytest.approx(6.25, rel=1e-14)
    u = SU.metrics(a, b)
    assert u["assd"] == 0.5 * (1 + 1.5) and u["hd"] == 2.0 and (u["lo_sq"], u["hi_sq"]) == (1, 4)


def test_empty_surfaces_are_undefined():
    a, _ = SU.two_voxels()
    for x, y in ((a, np.zeros_like(a)), (np.zeros_like(a), a), (np.zeros_like(a), np.zeros_like(a))):
        m = SU.metrics(x, y)
        assert m["count_ab"] == 0 and m["count_ba"] == 0
        assert all(math.isnan(m[k]) for k in SU.FIELDS[2:])


def test_oracle_edt_equals_brute_force():
    rng = np.random.RandomState(0)
    for shape, p in (((5, 6, 7), 0.05), ((12, 12, 12), 0.01), ((3, 11, 9), 0.3), ((1, 1, 12), 0.2), ((9, 1, 10), 0.1)):
        f = rng.rand(*shape) < p
        f[tuple(rng.randint(0, s) for s in shape)] = True
        sq_int, sq = SU.edt(f)
        assert np.array_equal(sq_int, SU.brute_force_sq(f)), shape
        assert np.array_equal(sq, sq_int.astype(np.float64))


def test_surface_of_the_oracle_is_the_six_neighbour_rule():
    rng = np.random.RandomState(1)
    x = rng.rand(6, 7, 8) < 0.7
    pad = np.pad(x, 1)
    inside6 = np.ones_like(x)
    for ax in range(3):
        for sh in (-1, 1):
            inside6 &= np.roll(pad, sh, ax)[1:-1, 1:-1, 1:-1]
    assert np.array_equal(SU.surface(x, 6), x & ~inside6)
    assert SU.surface(x, 26).sum() >= SU.surface(x, 6).sum()


def test_header_declares_the_entry_points():
    from vae_segmentation_amd import _lib
    protos = _lib.parse_header()
    I, P = ctypes.c_int, ctypes.c_void_p
    assert protos["vs_edt_workspace_bytes"] == (ctypes.c_longlong, [I] * 6)
    assert protos["vs_edt"] == (I, [P] * 2 + [I] * 5 + [P] * 2)
    assert protos["vs_surface_distances"] == (I, [P] * 3 + [I] * 6 + [P] * 3)
    assert protos["vs_surface"] == (I, [P] * 2 + [I] * 6 + [P])
    for path in (_lib.LIB_PATH, _lib.DET_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in ("vs_edt_workspace_bytes", "vs_edt", "vs_surface_distances", "vs_surface"):
            assert hasattr(raw, name), (path, name)


def test_argument_validation_without_gpu():
    from vae_segmentation_amd._lib import lib
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    fake = 0x10000                                                               # never dereferenced: every check comes before any launch
    sp = lambda *v: (ctypes.c_double * 3)(*v)
    ok_sp = sp(2.5, 0.8, 0.8)
    # workspace sizing is host arithmetic
    a, b = lib.vs_edt_workspace_bytes(1, 2, 64, 64, 64, 0), lib.vs_edt_workspace_bytes(1, 2, 128, 128, 128, 0)
    assert 0 < a < b and lib.vs_edt_workspace_bytes(1, 2, 64, 64, 64, 1) > a
    assert a >= 2 * 64 ** 3 * (2 + 2 * 4 + 2 * 4)                                # two surfaces, two maps, the list
    assert lib.vs_edt_workspace_bytes(1, 1, 5, 6, 7, 0) > 0
    # shapes: empty, a plane of 2^31 voxels, an axis beyond the stated limit of 1024 for d and h, the int32 range of squared distances
    for shape in ((0, 8, 8), (8, 8, -1), (1024, 1024, 2048), (1025, 8, 8), (8, 1025, 8), (2048, 1024, 1024)):
        for with_spacing in (0, 1):
            assert lib.vs_edt_workspace_bytes(1, 1, *shape, with_spacing) == ESHAPE, shape
        assert lib.vs_edt(fake, fake + 64, 1, 1, *shape, None, None) == ESHAPE
        assert lib.vs_edt(fake, fake + 64, 1, 1, *shape, ok_sp, None) == ESHAPE
        assert lib.vs_surface_distances(fake, fake + 64, fake + 128, 1, 1, *shape, 6, None, fake + 256, None) == ESHAPE
        assert lib.vs_surface(fake, fake + 64, 1, 1, *shape, 6, None) == ESHAPE
    assert lib.vs_edt_workspace_bytes(0, 1, 8, 8, 8, 0) == ESHAPE and lib.vs_edt_workspace_bytes(1, 0, 8, 8, 8, 0) == ESHAPE
    assert lib.vs_edt_workspace_bytes(1, 1, 1024, 1024, 2047, 0) > 0 and lib.vs_edt_workspace_bytes(1, 1, 1024, 8, 8, 1) > 0
    assert lib.vs_edt_workspace_bytes(1, 1, 1, 1, 46340, 0) > 0                  # 1 + 1 + 46340^2 = 2147395602 < 2^31 - 1
    assert lib.vs_edt_workspace_bytes(1, 1, 1, 1, 46341, 0) == ESHAPE            # 1 + 1 + 46341^2 = 2147488283 >= 2^31 - 1: integer path only
    assert lib.vs_edt_workspace_bytes(1, 1, 1, 1, 46341, 1) > 0
    assert lib.vs_edt(fake, fake + 64, 1, 1, 1, 1, 46341, None, None) == ESHAPE
    assert lib.vs_surface_distances(fake, fake + 64, fake + 128, 1, 1, 1, 1, 46341, 6, None, fake + 256, None) == ESHAPE
    # connectivity
    for conn in (18, 0, 8, -6):
        assert lib.vs_surface_distances(fake, fake + 64, fake + 128, 1, 1, 8, 8, 8, conn, None, fake + 256, None) == EINVAL
        assert lib.vs_surface(fake, fake + 64, 1, 1, 8, 8, 8, conn, None) == EINVAL
    # spacing: positive and finite
    for bad in (sp(0.0, 1, 1), sp(1, -0.5, 1), sp(1, 1, float("nan")), sp(float("inf"), 1, 1)):
        assert lib.vs_edt(fake, fake + 64, 1, 1, 8, 8, 8, bad, None) == EINVAL
        assert lib.vs_surface_distances(fake, fake + 64, fake + 128, 1, 1, 8, 8, 8, 6, bad, fake + 256, None) == EINVAL
    # null pointers and aliasing
    assert lib.vs_edt(None, None, 1, 1, 8, 8, 8, None, None) == EINVAL
    assert lib.vs_edt(fake, fake, 1, 1, 8, 8, 8, None, None) == EINVAL                                         # out aliases the input
    assert lib.vs_surface(fake, fake, 1, 1, 8, 8, 8, 6, None) == EINVAL
    assert lib.vs_surface_distances(None, None, None, 1, 1, 8, 8, 8, 6, None, None, None) == EINVAL
    assert lib.vs_surface_distances(fake, fake + 64, fake, 1, 1, 8, 8, 8, 6, None, fake + 256, None) == EINVAL       # out aliases pred
    assert lib.vs_surface_distances(fake, fake + 64, fake + 64, 1, 1, 8, 8, 8, 26, ok_sp, fake + 256, None) == EINVAL  # out aliases gt
    assert lib.vs_surface_distances(fake, fake + 64, fake + 128, 1, 1, 8, 8, 8, 6, None, fake + 64, None) == EINVAL  # the workspace aliases gt
    # alignment
    assert lib.vs_edt(fake + 4, fake + 64, 1, 1, 8, 8, 8, None, None) == EALIGN
    assert lib.vs_edt(fake, fake + 72, 1, 1, 8, 8, 8, ok_sp, None) == EALIGN
    assert lib.vs_surface(fake, fake + 68, 1, 1, 8, 8, 8, 26, None) == EALIGN
    assert lib.vs_surface_distances(fake + 8, fake + 64, fake + 128, 1, 1, 8, 8, 8, 6, None, fake + 256, None) == EALIGN
    assert lib.vs_surface_distances(fake, fake + 64, fake + 128, 1, 1, 8, 8, 8, 6, None, fake + 260, None) == EALIGN


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from vae_segmentation_amd import evaluation, ops
    x = torch.zeros(1, 1, 4, 4, 4)
    for call in (lambda: ops.edt(x), lambda: ops.surface(x), lambda: ops.surface_distances(x, x), lambda: evaluation.surface_metrics(x, x),
                 lambda: evaluation.assd(x[0, 0], x[0, 0]), lambda: evaluation.hd(x, x), lambda: evaluation.hd95(x, x)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(ValueError):
        evaluation.surface_metrics(torch.zeros(4, 4), torch.zeros(4, 4))
    assert ops.SURFACE_RECORD_FIELDS == SU.FIELDS


def test_val_surface_flag_defaults_to_off():
    import main_source
    import main_target
    for mod in (main_source, main_target):
        assert mod.parse(["r"]).val_surface is False
        a = mod.parse(["r", "--val_surface", "--val_keep_largest", "1"])
        assert a.val_surface is True and a.val_keep_largest == 1
