"""CPU: the integer rule of patch training as tests/patch_util.py states it — the oracle tests/test_gpu_patch.py holds the kernels to — and
the host half of the feature: PatchSampler's draws and the entry points' flags.  Everything is compared for equality."""
import importlib

import numpy as np
import pytest

from tests import patch_util as PU

S_RANGE, P_RANGE = range(1, 40), range(1, 24)
EDGE_WORDS = (0, 1, 2 ** 31, 2 ** 32 - 1)


def test_bounds_and_clamp_for_every_small_volume_and_patch():
    for s in S_RANGE:
        for p in P_RANGE:
            lb, ub = PU.bounds(s, p)
            assert lb <= ub, (s, p)
            if s >= p:
                assert (lb, ub) == (0, s - p)
            else:
                assert lb == ub and lb <= 0 and lb + p >= s             # the volume lies inside the patch, centred: the slack differs by at most one
                assert abs((0 - lb) - (lb + p - s)) <= 1
            for v in range(s):                                          # a forced origin contains its voxel
                o = PU.clamp_origin(v, s, p)
                assert lb <= o <= ub and o <= v < o + p, (s, p, v, o)
            for w in EDGE_WORDS:                                        # a free origin lies inside the bounds, and the ends of the word range reach both
                assert lb <= PU.free_origin(w, s, p) <= ub, (s, p, w)
            assert PU.free_origin(0, s, p) == lb and PU.free_origin(2 ** 32 - 1, s, p) == ub


def test_multiply_shift_is_exactly_uniform_on_stratified_words():
    ranks = [PU.scale(i * 2 ** 20, 64) for i in range(4096)]
    assert np.bincount(ranks, minlength=64).tolist() == [64] * 64
    assert ranks == sorted(ranks)                                       # and monotone: word order is rank order
    for m in (1, 2, 3, 7, 64, 1000, 2 ** 31 - 1):
        assert PU.scale(0, m) == 0 and PU.scale(2 ** 32 - 1, m) == m - 1


FREE = {0.0: [1, 2, 3, 4, 5, 6, 7, 8], 0.33: [1, 1, 2, 3, 3, 4, 5, 5], 0.5: [1, 1, 2, 2, 3, 3, 4, 4], 1.0: [0] * 8}      # floor(B (1 - p) + 0.5), B = 1..8


def test_which_samples_of_a_batch_are_forced():
    from vae_segmentation_amd import data_gpu as D
    for p, frees in FREE.items():
        for b, free in zip(range(1, 9), frees):
            assert PU.n_free(b, p) == free, (b, p)
            flags = PU.forced_flags(b, p)
            assert flags == [False] * free + [True] * (b - free)
            s = D.PatchSampler(8, p, rng=np.random.RandomState(0))
            assert [s.draw(j, b)[1] for j in range(b)] == flags, (b, p)
    assert D.PatchSampler(8).p == 0.33 and D.PatchSampler(8).margin == 0 and D.PatchSampler(8).classes is None


def test_draw_consumes_the_same_generator_values_forced_or_not():
    from vae_segmentation_amd import data_gpu as D
    a, b, ref = (np.random.RandomState(11) for _ in range(3))
    forced, free = D.PatchSampler((8, 9, 10), 1.0, rng=a), D.PatchSampler((8, 9, 10), 0.0, rng=b)
    for j in range(6):
        wf, ff = forced.draw(j % 3, 3)
        wn, fn = free.draw(j % 3, 3)
        want = ref.randint(0, 2 ** 32, size=5, dtype=np.uint64)           # exactly one such call per sample
        assert ff is True and fn is False
        assert wf.dtype == np.uint64 and np.array_equal(wf, want) and np.array_equal(wn, want)
    for g in (a, b):
        assert all(np.array_equal(x, y) for x, y in zip(g.get_state()[1:], ref.get_state()[1:]))
    with pytest.raises(ValueError):
        forced.draw(3, 3)
    for bad in (dict(oversample_foreground=1.5), dict(margin=-1), dict(classes=(1, 1)), dict(classes=(9,))):
        with pytest.raises(ValueError):
            D.PatchSampler(8, **bad)
    with pytest.raises(ValueError):
        D.PatchSampler((8, 0, 8))


def test_oracle_pick_index_and_gather_against_brute_force():
    rng = np.random.RandomState(3)
    shape, n_class, chunk = (5, 7, 9), 3, 16
    lab = PU.label_volume(shape, "odd", n_class, seed=1)
    assert np.isnan(lab).any() and (lab == 0.5).any() and (lab == n_class).any()
    table = PU.ref_index(lab, n_class, chunk)
    flat = lab.ravel()
    assert table.shape == ((flat.size + chunk - 1) // chunk + 1, n_class) and table.dtype == np.int32
    for j in range(table.shape[0]):
        for k in range(n_class):
            assert table[j, k] == sum(1 for v in flat[:j * chunk] if v == k)
    assert table[-1].sum() == np.isin(flat, [0, 1, 2]).sum() < flat.size          # NaN, 0.5, n_class, -1 and 1.5 are counted nowhere
    patch = (3, 8, 4)                                                   # larger than the volume along y
    for _ in range(50):
        words = rng.randint(0, 2 ** 32, size=5, dtype=np.uint64)
        got = PU.ref_pick(lab, n_class, (2, 1), words, True, patch)
        k = got[3]
        assert k in (1, 2) and lab[got[4], got[5], got[6]] == k and got[7] == 0
        members = [(z, y, x) for z in range(5) for y in range(7) for x in range(9) if lab[z, y, x] == k]      # ascending linear index
        assert tuple(got[4:7]) == members[(int(words[1]) * len(members)) >> 32]
        assert all(got[a] <= got[4 + a] < got[a] + patch[a] for a in range(3))
        free = PU.ref_pick(lab, n_class, (2, 1), words, False, patch)
        assert free[3:] == [-1, -1, -1, -1, 0] and free[1] == -((8 - 7) // 2) and 0 <= free[0] <= 2 and 0 <= free[2] <= 5
    nothing = PU.ref_pick(PU.label_volume(shape, "background"), n_class, (1, 2), [5, 6, 7, 8, 9], True, patch)
    assert nothing[3:] == [-1, -1, -1, -1, 0]                           # forced with no class present: a free origin
    only2 = PU.ref_pick(lab, n_class, (2,), [0, 0, 0, 0, 0], True, patch)
    assert only2[3] == 2
    vol = rng.randn(*shape).astype(np.float32)
    for origin, margin in (((0, 0, 0), 0), ((-2, 3, 7), 0), ((4, -1, 8), 2), ((-9, -9, -9), 1), ((50, 0, 0), 0)):
        got = PU.ref_gather(vol, origin, patch, margin, cval=-7.0)
        assert got.shape == tuple(p + 2 * margin for p in patch) and got.dtype == np.float32
        for z in range(got.shape[0]):
            for y in range(got.shape[1]):
                for x in range(got.shape[2]):
                    sz, sy, sx = origin[0] - margin + z, origin[1] - margin + y, origin[2] - margin + x
                    inside = 0 <= sz < 5 and 0 <= sy < 7 and 0 <= sx < 9
                    assert got[z, y, x] == (vol[sz, sy, sx] if inside else np.float32(-7.0))


def test_label_volumes_are_what_their_names_say():
    chunk = 4096
    shape = (17, 16, 257)
    n = int(np.prod(shape))
    assert n // chunk == 17 and n % chunk                               # 17 whole chunks and a partial one
    tail = PU.label_volume(shape, "tail", chunk=chunk).ravel()
    assert tail[:17 * chunk].sum() == 0 and 0 < tail.sum() < n - 17 * chunk
    sparse = np.flatnonzero(PU.label_volume(shape, "sparse64").ravel() == 2)
    assert sparse.size == 64 and len(set((sparse // chunk).tolist())) >= 3
    first, last = PU.label_volume(shape, "first").ravel(), PU.label_volume(shape, "last").ravel()
    assert np.flatnonzero(first).tolist() == [0] and np.flatnonzero(last).tolist() == [n - 1]
    assert PU.label_volume((5, 7, 9), "random", dtype=np.uint8).dtype == np.uint8


def test_ops_reexports_the_patch_names():
    from vae_segmentation_amd import ops, volume
    assert {"PATCH_CHUNK", "patch_index", "patch_pick", "patch_gather"} <= set(volume.PATCH_NAMES)
    for name in volume.PATCH_NAMES:
        assert getattr(ops, name) is getattr(volume, name), name
    assert ops.PATCH_CHUNK >= 1024 and ops.PATCH_CHUNK % 1024 == 0       # whole quarters for the four waves of a counting workgroup


def test_entry_points_parse_the_flags():
    for script in ("main_source", "main_target"):
        mod = importlib.import_module(script)
        a = mod.parse(["run", "--real_data"])
        assert a.train_patches is False and a.patch_fg == 0.33 and a.patch_margin == 16
        a = mod.parse(["run", "--real_data", "--train_patches", "--patch_fg", "0.5", "--patch_margin", "4"])
        assert a.train_patches is True and a.patch_fg == 0.5 and a.patch_margin == 4
        for bad in (["--train_patches"], ["--real_data", "--train_patches", "--patch_fg", "1.5"], ["--real_data", "--train_patches", "--patch_margin", "-1"]):
            with pytest.raises(SystemExit):
                mod.parse(["run"] + bad)
