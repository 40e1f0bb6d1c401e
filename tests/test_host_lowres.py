"""Host: (1) tests/lowres_util.py — the oracle of tests/test_gpu_lowres.py — is pinned: the coordinate rule against scipy's order-0 picks, the separable
fp64 restatement of the order-3 zoom against scipy's three-dimensional evaluation, the target-shape rule; (2) what of the feature needs no device:
data_gpu.lowres_target_shape, IntensityAugment's low-resolution draws, the entry points' --aug_lowres flag and the argument checks of the C ABI."""
import numpy as np
import pytest
from scipy import ndimage as ndi

from tests import augment_util as AU
from tests import lowres_util as LU

SHAPES = [(2, 3, 4), (5, 7, 6), (1, 1, 9), (17, 19, 23), (33, 40, 65), (24, 24, 24)]
ZOOMS = (0.5, 0.61, 0.83, 1.0)


# ---- (1) the oracle ------------------------------------------------------------------------------------------------------------------------
def test_coordinate_rule_reproduces_scipys_order0_picks_for_all_length_pairs():
    wrong, other_form = 0, 0
    for m in range(2, 48):
        x = np.arange(m, dtype=np.float64)
        for n in range(2, 48):
            want = ndi.zoom(x, n / m, order=0, mode="nearest", grid_mode=True).astype(np.int64)
            assert want.shape == (n,)
            wrong += not np.array_equal(LU.pick0(m, n), want)
            other = np.floor((np.arange(n) + 0.5) * m / n - 0.5 + 0.5).astype(np.int64)      # the product first, then the division
            other_form += not np.array_equal(other, want)
    assert wrong == 0
    assert other_form > 0                                                  # the order of the operations matters: exact ties fall the other way
    for m, n in ((26, 23), (18, 33), (30, 11), (6, 47), (12, 47), (24, 44)):
        other = np.floor((np.arange(n) + 0.5) * m / n - 0.5 + 0.5).astype(np.int64)
        assert not np.array_equal(other, LU.pick0(m, n)), (m, n)


def _down(shape, zoom):
    return tuple(max(1, int(np.round(s * zoom))) for s in shape)          # (1, 1, 9) keeps its unit axes


@pytest.mark.parametrize("shape", SHAPES)
def test_separable_restatement_is_scipys_three_dimensional_zoom(shape):
    for zoom in ZOOMS:
        for kind in LU.KINDS:
            x = LU.volume(shape, kind)
            low = LU.ref_zoom_edge(x, _down(shape, zoom), 0, clip=False)
            want, got = LU.ref_zoom_edge64(low, shape, 3), LU.sep_zoom_edge64(low, shape)
            span = max(float(low.max()) - float(low.min()), float(np.abs(low).max()))
            assert np.abs(got - want).max() <= 1e-12 * span, (zoom, kind)
            assert np.array_equal(LU.sep_zoom_edge(low, shape), LU.ref_zoom_edge(low, shape, 3, True))       # after the one rounding: the same bits
            if kind == "constant":
                assert np.array_equal(LU.ref_simulate_lowres(x, _down(shape, zoom)), x)
            if zoom == 1.0:
                assert np.array_equal(LU.ref_simulate_lowres(x, shape), x)
    # down-sampling with the cubic spline too
    x = LU.volume(shape, "offset", seed=3)
    t = _down(shape, 0.61)
    assert np.abs(LU.sep_zoom_edge64(x, t) - LU.ref_zoom_edge64(x, t, 3)).max() <= 1e-12 * float(np.abs(x).max())


def test_the_pad_is_twelve_and_the_clip_has_work():
    x = -np.ones((6, 6, 14), np.float32)
    x[:, :, 7:] = 1.0
    free = LU.ref_zoom_edge64(x, (10, 10, 24), 3)
    assert free.max() > 1.0 + 1e-3 and free.min() < -1.0 - 1e-3
    y = LU.ref_zoom_edge(x, (10, 10, 24), 3, True)
    assert y.max() == 1.0 and y.min() == -1.0
    assert abs(abs(LU.POLE) ** LU.PAD - 1.4e-7) < 1e-8                    # what a pad of another length would change: visible in float32


def test_target_shape_rule():
    from vae_segmentation_amd import data_gpu as D
    assert hasattr(D, "lowres_target_shape")
    for fn in (LU.ref_target_shape, D.lowres_target_shape):
        assert fn((17, 19, 23), 0.5) == (8, 10, 12)                        # 8.5 -> 8 and 9.5 -> 10 and 11.5 -> 12: half to even
        assert fn((5, 7, 6), 0.5) == (2, 4, 3)
        assert fn((33, 40, 65), 0.61) == (20, 24, 40)
        assert fn((33, 40, 65), 0.61, ignore_axes=(0,)) == (33, 24, 40) and fn((33, 40, 65), 0.61, (0, 2)) == (33, 24, 65)
        assert fn((24, 24, 24), 1.0) == (24, 24, 24)
        assert fn((1, 8, 8), 0.5, (0,)) == (1, 4, 4)
        with pytest.raises(ValueError, match="vanish"):
            fn((1, 8, 8), 0.5)
        with pytest.raises(ValueError, match="vanish"):
            fn((17, 19, 23), 0.02)
    for shape in SHAPES:
        for zoom in (0.5, 0.55, 0.61, 0.75, 0.83, 1.0):
            ignore = tuple(a for a in range(3) if shape[a] == 1)
            assert D.lowres_target_shape(shape, zoom, ignore) == LU.ref_target_shape(shape, zoom, ignore)
    with pytest.raises(ValueError):
        D.lowres_target_shape((8, 8, 8), 0.0)
    with pytest.raises(ValueError):
        D.lowres_target_shape((8, 8, 8), 0.5, ignore_axes=(3,))


# ---- (2) the feature, without a device -------------------------------------------------------------------------------------------------------
ALL_ON = dict(p_noise=1.0, p_blur=1.0, p_blur_per_channel=1.0, p_brightness=1.0, p_contrast=1.0, p_gamma_inverted=1.0, p_gamma=1.0, p_mirror=1.0)


def test_transform_draws_the_stage_after_contrast_and_only_when_asked():
    from vae_segmentation_amd import data_gpu as D
    channels, shape = 2, (6, 7, 8)
    t = D.IntensityAugment("data", "seg", rng=np.random.RandomState(9), noise="philox", seed=1, p_lowres=1.0, p_lowres_per_channel=1.0, **ALL_ON)
    got = t.draw(channels, shape)
    assert [op[0] for op in got] == ["noise", "blur", "brightness", "contrast", "lowres", "gamma", "gamma", "flip"]
    # the zooms are what a replay of the stream gives: count the variates before the stage
    probe = np.random.RandomState(9)
    probe.random_sample(2 + 1 + 2 * channels + 1 + channels + 1 + 2 * channels)      # noise, blur, brightness, contrast (philox: no normals)
    assert probe.uniform() < 1.0
    zooms = []
    for _ in range(channels):
        assert probe.uniform() < 1.0
        zooms.append(probe.uniform(0.5, 1.0))
    assert got[4] == ("lowres", zooms, 0, 3, ())
    # several samples, several settings: the streams stay together
    for kw in (dict(ALL_ON, p_lowres=1.0), dict(p_lowres=0.25), dict(ALL_ON, p_lowres=0.5, lowres_zoom=(0.7, 0.7), lowres_orders=(1, 1),
                                                                   lowres_ignore_axes=(0,), p_lowres_per_channel=0.3)):
        t = D.IntensityAugment("data", "seg", rng=np.random.RandomState(5), noise="philox", seed=2, **kw)
        rng = np.random.RandomState(5)
        for _ in range(6):
            want = LU.ref_draw(rng, channels, shape, noise="philox", seed=2, n_noised=t.n_noised, **kw)
            assert AU.same_ops(t.draw(channels, shape), want)
        assert t.rng.uniform() == rng.uniform()
    # without the argument: not one variate more than before the stage existed
    for kw in (ALL_ON, {}, dict(p_lowres=0.0)):
        t = D.IntensityAugment("data", "seg", rng=np.random.RandomState(7), noise="numpy", **kw)
        rng = np.random.RandomState(7)
        base = {k: v for k, v in kw.items() if k != "p_lowres"}
        for _ in range(4):
            assert AU.same_ops(t.draw(channels, shape), AU.ref_draw(rng, channels, shape, noise="numpy", **base))
        assert t.rng.uniform() == rng.uniform()
    for bad in (dict(lowres_zoom=(0.0, 1.0)), dict(lowres_zoom=(0.9, 0.5)), dict(lowres_zoom=(0.5, 1.5)), dict(lowres_orders=(0, 2)),
                dict(lowres_orders=(3,)), dict(lowres_ignore_axes=(3,))):
        with pytest.raises(ValueError, match="lowres"):
            D.IntensityAugment("data", "seg", p_noise=0, **bad)


def test_aug_lowres_flag():
    import main_source
    import main_target
    for mod in (main_source, main_target):
        assert mod.parse(["run"]).aug_lowres == 0.0
        assert mod.parse(["run", "--real_data", "--aug_intensity"]).aug_lowres == 0.0
        assert mod.parse(["run", "--real_data", "--aug_intensity", "--aug_lowres", "0.25"]).aug_lowres == 0.25
        with pytest.raises(SystemExit):
            mod.parse(["run", "--real_data", "--aug_lowres", "0.25"])
        with pytest.raises(SystemExit):
            mod.parse(["run", "--real_data", "--aug_intensity", "--aug_lowres", "1.5"])
        with pytest.raises(SystemExit):
            mod.parse(["run", "--aug_intensity", "--aug_lowres", "0.25", "--no_aug"])


def test_c_abi_answers_argument_errors_before_any_launch():
    """include/vaeseg.h: VS_EINVAL = -1, VS_ESHAPE = -2, VS_EALIGN = -5; the device addresses are never dereferenced on these paths"""
    from vae_segmentation_amd import _lib
    lib = _lib.lib
    einval, eshape, ealign = -1, -2, -5
    A, B, W = 4096, 8192, 16384
    wb, ze = lib.vs_zoom_edge_workspace_bytes, lib.vs_zoom_edge
    stats = 32 + lib.vs_aug_stats_workspace_bytes(1, 4, 5, 6)
    assert wb(4, 5, 6, 8, 9, 10, 0) == stats and wb(4, 5, 6, 8, 9, 10, 1) == stats
    assert wb(4, 5, 6, 8, 9, 10, 3) == stats + 8 * (8 * 5 * 6 + 8 * 9 * 6)
    assert wb(4, 5, 6, 8, 9, 10, 2) == 0 and wb(0, 5, 6, 8, 9, 10, 3) == 0 and wb(4, 5, 6, 8, 0, 10, 3) == 0
    assert wb(1, 2, 513, 1, 2, 512, 3) == 0 and wb(1, 2, 512, 1, 513, 2, 3) == 0 and wb(1, 2, 513, 1, 2, 600, 1) > 0
    assert wb(1, 2, 512, 1, 3, 512, 3) > 0

    def zoom(x=A, y=B, s=(4, 5, 6), d=(8, 9, 10), order=3, clip=1, ws=W):
        return ze(x, y, *s, *d, order, clip, ws, None)

    assert zoom(x=None) == einval and zoom(y=None) == einval and zoom(y=A) == einval
    for order in (-1, 2, 4, 5):
        assert zoom(order=order) == einval
    assert zoom(ws=None) == einval and zoom(order=1, ws=None) == einval and zoom(order=3, clip=0, ws=None) == einval
    assert zoom(s=(0, 5, 6)) == eshape and zoom(d=(8, 9, 0)) == eshape and zoom(s=(2048, 1024, 1024), order=0) == eshape
    assert zoom(s=(1, 2, 513), d=(1, 2, 512)) == eshape and zoom(s=(1, 2, 9), d=(1, 513, 9)) == eshape and zoom(s=(513, 1, 1), d=(1, 1, 1)) == eshape
    assert zoom(x=A + 2) == ealign and zoom(y=B + 1) == ealign and zoom(ws=W + 4) == ealign
    # the lines a workgroup holds: (m + 24) (L + 1) doubles of lines and 4 n of weights fit 80 KiB — two workgroups per CU
    bundle = lib.vs_zoom_edge_bundle
    assert bundle(0, 4) == 0 and bundle(513, 4) == 0 and bundle(4, 0) == 0 and bundle(4, 513) == 0
    assert bundle(1, 1) == 64 and bundle(64, 128) == 64 and bundle(128, 64) == 64 and bundle(128, 128) == 32 and bundle(200, 200) == 32 and bundle(256, 256) == 16
    assert bundle(300, 300) == 16 and bundle(509, 512) == 8 and bundle(512, 512) == 8
    for m in (1, 2, 63, 64, 65, 127, 128, 129, 133, 134, 255, 256, 286, 287, 511, 512):
        for n in (1, 64, 128, 256, 512):
            L = bundle(m, n)
            assert L in (64, 32, 16, 8) and ((m + 24) * (L + 1) + 4 * n) * 8 <= 80 * 1024
            assert L == 64 or ((m + 24) * (2 * L + 1) + 4 * n) * 8 > 80 * 1024              # and no more would
