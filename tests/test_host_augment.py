"""Host: (1) tests/augment_util.py — the oracle of tests/test_gpu_augment.py — is pinned against scipy, the scalar Philox form, the moments of a normal
sample and the draw order; these pass without the feature; (2) what of the feature needs no device: IntensityAugment's constructor and draws, the entry
points' --aug_intensity flag and the argument checks of the C ABI."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage as ndi

from tests import augment_util as AU
from tests import elastic_util as EU


# ---- (1) the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 4), (1, 1, 1), (9, 10, 11), (5, 1, 40)])
@pytest.mark.parametrize("sigma", [0.1, 0.5, 0.8, 1.0, 2.0])
def test_ref_blur_is_scipys_reflect_mode_filter_bit_for_bit(shape, sigma):
    rng = np.random.RandomState(int(sigma * 10) + shape[0])
    for x in ((rng.randn(*shape) + 100).astype(np.float32), (rng.rand(*shape) * 2 - 1).astype(np.float32)):
        want = ndi.gaussian_filter(x, sigma, mode="reflect")
        got = AU.ref_blur(x, sigma)
        assert want.dtype == np.float32 and got.dtype == np.float32 and np.array_equal(got, want)
        if sigma == 0.1:                                                   # radius int(0.4 + 0.5) = 0: one tap of weight 1
            assert np.array_equal(got, x)
    assert len(AU.ref_weights(sigma)) == 2 * int(4 * sigma + 0.5) + 1


def test_identities_and_restored_statistics():
    rng = np.random.RandomState(1)
    for x in ((rng.randn(7, 8, 9) + 100).astype(np.float32), (rng.rand(7, 8, 9) * 2 - 1).astype(np.float32)):
        tol = 2.0 ** -22 * np.abs(x).max()
        for invert in (False, True):
            assert np.abs(AU.ref_power(x, 1.0, invert).astype(np.float64) - x).max() <= tol
            assert np.abs(AU.ref_gamma(x, 1.0, invert, True).astype(np.float64) - x).max() <= tol
        for preserve in (False, True):
            assert np.abs(AU.ref_contrast(x, 1.0, preserve).astype(np.float64) - x).max() <= tol
        for invert in (False, True):
            y = AU.ref_gamma(x, 2.0, invert, True)
            want, got = AU.ref_stats(x), AU.ref_stats(y)
            assert abs(got[2] - want[2]) <= 1e-6 * max(1.0, abs(want[2])) and abs(got[3] - want[3]) <= 1e-6 * want[3]
            assert not np.array_equal(y, x)
        y = AU.ref_restat(x, 3.0, 0.5)
        assert abs(AU.ref_stats(y)[2] - 3.0) < 1e-6 and abs(AU.ref_stats(y)[3] - 0.5) < 1e-6
    mn, mx, mean, std = AU.ref_stats(x)
    v = x.astype(np.float64)
    assert (mn, mx) == (v.min(), v.max()) and abs(mean - v.mean()) < 1e-14 and abs(std - v.std()) < 1e-14
    # a constant plane: finite, power returns the plane, restat returns mean0
    c = np.full((3, 4, 5), 7.25, np.float32)
    assert AU.ref_stats(c) == (7.25, 7.25, 7.25, 0.0)
    for invert in (False, True):
        assert np.array_equal(AU.ref_power(c, 0.7, invert), c)
        assert np.array_equal(AU.ref_restat(c, 2.5, 1.5, invert), np.full_like(c, -2.5 if invert else 2.5))
        assert np.array_equal(AU.ref_gamma(c, 1.5, invert, True), c)
    assert np.array_equal(AU.ref_contrast(c, 1.25), c)
    # flips
    a = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    assert np.array_equal(AU.ref_flip(a, 0), a) and np.array_equal(AU.ref_flip(a, 4), a[::-1]) and np.array_equal(AU.ref_flip(a, 2), a[:, ::-1])
    assert np.array_equal(AU.ref_flip(a, 1), a[:, :, ::-1]) and np.array_equal(AU.ref_flip(a, 7), a[::-1, ::-1, ::-1])


def test_ref_normal_is_the_scalar_form_and_a_pure_function():
    import math
    seed, sample, channel = 2 ** 40 + 3, 7, 1
    a = AU.ref_normal(11, seed, sample, channel)                           # odd: the last pair is half used
    assert a.shape == (11,) and a.dtype == np.float64
    assert np.array_equal(a, AU.ref_normal(11, seed, sample, channel)) and np.array_equal(a[:6], AU.ref_normal(6, seed, sample, channel))
    for other in ((seed + 1, sample, channel), (seed + 2 ** 32, sample, channel), (seed, sample + 1, channel), (seed, sample, channel + 1)):
        assert not np.array_equal(a, AU.ref_normal(11, *other))
    # elements 6 and 7: pair 3, from the scalar Philox form
    w = EU.ref_philox4x32((3, 0, 0x100 + channel, sample), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((w[0] >> 5) * 2 ** 26 + (w[1] >> 6) + 0.5) * 2.0 ** -53
    u2 = ((w[2] >> 5) * 2 ** 26 + (w[3] >> 6)) * 2.0 ** -53
    r = math.sqrt(-2.0 * math.log(u1))
    assert abs(a[6] - r * math.cos(2 * math.pi * u2)) < 1e-15 and abs(a[7] - r * math.sin(2 * math.pi * u2)) < 1e-15
    # the stream is not the elastic one: counter word 2 starts at 0x100
    assert (w[0], w[1]) != EU.ref_philox4x32((3, 0, channel, sample), (seed & 0xFFFFFFFF, seed >> 32))[:2]


@pytest.mark.parametrize("seed,sample,channel", [(2 ** 40 + 3, 7, 0), (2 ** 40 + 3, 7, 1), (5, 0, 0)])
def test_ref_normal_has_the_moments_of_a_normal_sample(seed, sample, channel):
    """N = 2^18 against the standard errors of N iid normals, five of each"""
    n = 2 ** 18
    x = AU.ref_normal(n, seed, sample, channel)
    mean = x.mean()
    c = x - mean
    var, m3, m4 = (c ** 2).mean(), (c ** 3).mean(), (c ** 4).mean()
    print("mean %.3e (se %.3e), var - 1 %.3e (se %.3e), m3 %.3e (se %.3e), m4 - 3 %.3e (se %.3e)"
          % (mean, n ** -0.5, var - 1, (2 / n) ** 0.5, m3, (15 / n) ** 0.5, m4 - 3, (96 / n) ** 0.5))
    assert np.all(np.isfinite(x))
    assert abs(mean) < 5 / np.sqrt(n) and abs(var - 1) < 5 * np.sqrt(2 / n) and abs(m3) < 5 * np.sqrt(15 / n) and abs(m4 - 3) < 5 * np.sqrt(96 / n)


def _all_on():
    return dict(p_noise=1.0, p_blur=1.0, p_blur_per_channel=1.0, p_brightness=1.0, p_contrast=1.0, p_gamma_inverted=1.0, p_gamma=1.0, p_mirror=1.0)


def test_ref_draw_consumes_exactly_the_listed_variates():
    channels, shape = 2, (3, 4, 5)
    # every gate open: counted against a probe generator that draws what the list says
    got = AU.ref_draw(np.random.RandomState(3), channels, shape, noise="numpy", **_all_on())
    probe = np.random.RandomState(3)
    assert probe.uniform() < 1.0
    s = probe.uniform(0.0, 0.1)
    fields = np.stack([probe.normal(0.0, 1.0, shape) for _ in range(channels)])
    assert probe.uniform() < 1.0
    sig = []
    for _ in range(channels):
        assert probe.uniform() <= 1.0
        sig.append(probe.uniform(0.5, 1.0))
    assert probe.uniform() < 1.0
    m = [probe.uniform(0.75, 1.25) for _ in range(channels)]

    def range_val(lo, hi):
        return probe.uniform(lo, 1) if probe.random_sample() < 0.5 and lo < 1 else probe.uniform(max(lo, 1), hi)

    assert probe.uniform() < 1.0
    f = [range_val(0.75, 1.25) for _ in range(channels)]
    assert probe.uniform() < 1.0
    gi = [range_val(0.7, 1.5) for _ in range(channels)]
    assert probe.uniform() < 1.0
    g = [range_val(0.7, 1.5) for _ in range(channels)]
    mask = sum(bit for bit in (4, 2, 1) if probe.uniform() < 1.0)
    want = [("noise", s, fields), ("blur", sig), ("brightness", m), ("contrast", f, True), ("gamma", gi, True, True), ("gamma", g, False, True),
            ("flip", mask)]
    assert mask == 7 and AU.same_ops(got, want)
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    AU.ref_draw(a, channels, shape, noise="numpy", **_all_on())
    b.random_sample(2); b.normal(0.0, 1.0, (channels,) + shape); b.random_sample(1 + 2 * channels + 1 + channels + 3 * (1 + 2 * channels) + 3)
    assert a.uniform() == b.uniform()
    # the Philox source takes no normals from the generator
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    ops_list = AU.ref_draw(a, channels, shape, noise="philox", seed=11, n_noised=4, **_all_on())
    b.random_sample(2 + 1 + 2 * channels + 1 + channels + 3 * (1 + 2 * channels) + 3)
    assert a.uniform() == b.uniform() and ops_list[0][2] == (11, 4) and ops_list[0][1] == s
    # every gate closed: the six gates and the three mirror draws, nothing else, and no op
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    closed = {k: 0.0 for k in _all_on()}
    assert AU.ref_draw(a, channels, shape, **closed) == []
    b.random_sample(6 + 3)
    assert a.uniform() == b.uniform()
    # blur: a channel that is not chosen draws no sigma
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    only_blur = dict(closed, p_blur=1.0, p_blur_per_channel=0.0)
    assert AU.ref_draw(a, channels, shape, **only_blur) == [("blur", [None, None])]
    b.random_sample(6 + channels + 3)
    assert a.uniform() == b.uniform()


# ---- (2) the feature, without a device -------------------------------------------------------------------------------------------------------
def test_transform_constructor_errors():
    from vae_segmentation_amd import data_gpu as D
    with pytest.raises(NotImplementedError, match="noise"):
        D.IntensityAugment("data", "seg")
    for noise in ("numpy", "philox"):
        t = D.IntensityAugment("data", "seg", noise=noise, seed=5)
        assert t.noise == noise and t.seed == 5 and t.n_noised == 0
    assert D.IntensityAugment("data", "seg", p_noise=0).noise is None
    with pytest.raises(ValueError, match="noise"):
        D.IntensityAugment("data", "seg", noise="sobol")
    with pytest.raises(ValueError, match="sigma"):
        D.IntensityAugment("data", "seg", noise="philox", blur_sigma=(0.5, 2.5))
    with pytest.raises(ValueError, match="sigma"):
        D.IntensityAugment("data", "seg", noise="philox", blur_sigma=(0.0, 1.0))
    with pytest.raises(ValueError, match="gamma"):
        D.IntensityAugment("data", "seg", noise="philox", gamma=(1.5, 0.7))
    from vae_segmentation_amd import ops
    with pytest.raises(ValueError, match="sigma"):
        ops.gaussian_weights(2.01)
    for sigma in (0.1, 0.5, 1.0, 2.0):
        w = AU.ref_weights(sigma)
        assert np.array_equal(ops.gaussian_weights(sigma), w[len(w) // 2:])


def test_transform_draws_in_the_oracles_order_and_counts_philox_samples():
    from vae_segmentation_amd import data_gpu as D
    channels, shape = 2, (3, 4, 5)
    for kw in (_all_on(), {}, dict(_all_on(), p_blur_per_channel=0.5, preserve_range=False, retain_stats=False)):
        t = D.IntensityAugment("data", "seg", rng=np.random.RandomState(9), noise="numpy", **kw)
        rng = np.random.RandomState(9)
        for _ in range(4):                                                 # several samples: the streams stay together
            assert AU.same_ops(t.draw(channels, shape), AU.ref_draw(rng, channels, shape, noise="numpy", **kw))
        assert t.rng.uniform() == rng.uniform()
    t = D.IntensityAugment("data", "seg", rng=np.random.RandomState(9), noise="philox", seed=11, **_all_on())
    rng = np.random.RandomState(9)
    for n in range(3):
        got = t.draw(channels, shape)
        assert got[0][2] == (11, n) and AU.same_ops(got, AU.ref_draw(rng, channels, shape, noise="philox", seed=11, n_noised=n, **_all_on()))
    # with nnU-Net's probabilities most samples carry few ops, and only noised samples advance the counter
    t = D.IntensityAugment("data", "seg", rng=np.random.RandomState(2), noise="philox", seed=1)
    noised = sum(1 for _ in range(200) if any(op[0] == "noise" for op in t.draw(1, shape)))
    assert t.n_noised == noised and 5 <= noised <= 40


def test_aug_intensity_flag():
    import main_source
    import main_target
    for mod in (main_source, main_target):
        assert mod.parse(["run"]).aug_intensity is False
        assert mod.parse(["run", "--real_data", "--aug_intensity"]).aug_intensity is True
        assert mod.parse(["run", "--real_data", "--aug_intensity", "--aug_elastic", "0.5"]).aug_elastic == 0.5
        with pytest.raises(SystemExit):
            mod.parse(["run", "--aug_intensity", "--no_aug"])


def test_c_abi_answers_argument_errors_before_any_launch():
    """include/vaeseg.h: VS_EINVAL = -1, VS_ESHAPE = -2, VS_EALIGN = -5; the device addresses are never dereferenced on these paths"""
    from vae_segmentation_amd import _lib
    lib = _lib.lib
    einval, eshape, ealign = -1, -2, -5
    A, B, C, R = 4096, 8192, 12288, 16384
    assert lib.vs_aug_stats_workspace_bytes(1, 1, 1, 8192) == 32 and lib.vs_aug_stats_workspace_bytes(3, 1, 1, 8193) == 3 * 2 * 32
    assert lib.vs_aug_stats_workspace_bytes(1, 0, 4, 4) == 0
    st = lib.vs_aug_stats
    assert st(None, R, C, 1, 4, 5, 6, None) == einval and st(A, None, C, 1, 4, 5, 6, None) == einval and st(A, R, None, 1, 4, 5, 6, None) == einval
    assert st(A, R, C, 0, 4, 5, 6, None) == einval
    assert st(A, R, C, 1, 4, 0, 6, None) == eshape and st(A, R, C, 1, 2048, 1024, 1024, None) == eshape
    assert st(A + 2, R, C, 1, 4, 5, 6, None) == ealign and st(A, R + 4, C, 1, 4, 5, 6, None) == ealign and st(A, R, C + 4, 1, 4, 5, 6, None) == ealign
    nm = lib.vs_aug_normal_philox
    assert nm(None, 4, 5, 6, 1, 2, 0, None) == einval and nm(A, 4, 5, 6, 1, 2, -1, None) == einval
    assert nm(A, 4, 0, 6, 1, 2, 0, None) == eshape and nm(A + 4, 4, 5, 6, 1, 2, 0, None) == ealign
    sg = lib.vs_aug_stage

    def stage(x=A, y=B, d=4, h=5, w=6, flip=0, first=0, mode=0, noise=None, s=0.0, ch=0, has_m=0, m=1.0, op=0, p=1.0, flag=0, rec=None, rec0=None,
              mean0=0.0, std0=1.0, rec_out=None, ws=None):
        return sg(x, y, d, h, w, flip, first, mode, noise, s, 1, 2, ch, has_m, m, op, p, flag, rec, rec0, mean0, std0, rec_out, ws, None)

    assert stage(x=None) == einval and stage(y=None) == einval and stage(y=A) == einval
    assert stage(flip=8) == einval and stage(flip=-1) == einval and stage(mode=3) == einval and stage(op=4) == einval and stage(ch=-1) == einval
    assert stage(mode=1) == einval                                         # noise from an array, no array
    assert stage(op=1) == einval and stage(op=2) == einval                 # an op that reads statistics, no record
    assert stage(rec_out=R) == einval                                      # a record to write, no workspace
    assert stage(mode=2, s=float("nan")) == einval and stage(has_m=1, m=float("inf")) == einval and stage(op=2, rec=R, p=float("nan")) == einval
    assert stage(op=3, rec=R, mean0=float("nan")) == einval
    assert stage(d=0) == eshape and stage(d=2048, h=1024, w=1024) == eshape
    assert stage(x=A + 2) == ealign and stage(y=B + 1) == ealign and stage(mode=1, noise=C + 4) == ealign and stage(op=1, rec=R + 4) == ealign
    assert stage(op=3, rec=R, rec0=R + 4) == ealign and stage(rec_out=R + 4, ws=C) == ealign and stage(rec_out=R, ws=C + 4) == ealign
    wts = (ctypes.c_double * 9)(*([1.0] + [0.0] * 8))
    bl = lib.vs_aug_blur
    assert bl(None, B, 4, 5, 6, 1.0, wts, None) == einval and bl(A, None, 4, 5, 6, 1.0, wts, None) == einval and bl(A, A, 4, 5, 6, 1.0, wts, None) == einval
    assert bl(A, B, 4, 5, 6, 1.0, None, None) == einval
    for sigma in (0.0, -1.0, float("nan"), float("inf"), 2.0625, 1e300):   # sigma > 2: the radius the LDS tile is sized for is 8
        assert bl(A, B, 4, 5, 6, sigma, wts, None) == einval
    assert bl(A, B, 4, 5, 0, 1.0, wts, None) == eshape and bl(A, B, 1024, 1024, 2048, 1.0, wts, None) == eshape
    assert bl(A + 2, B, 4, 5, 6, 1.0, wts, None) == ealign and bl(A, B + 2, 4, 5, 6, 1.0, wts, None) == ealign
    tile = (ctypes.c_int * 3)()
    assert lib.vs_aug_blur_tile(2.5, tile) == einval and lib.vs_aug_blur_tile(1.0, None) == einval
    for sigma in (0.1, 0.5, 1.0, 1.5, 2.0):                                # the staged block of every tile fits 80 KiB: two workgroups per CU
        assert lib.vs_aug_blur_tile(sigma, tile) == 0 and tile[2] == 32
        r = int(4 * sigma + 0.5)
        assert (tile[0] + 2 * r) * (tile[1] + 2 * r) * (tile[2] + 2 * r) * 4 <= 80 * 1024
    fl = lib.vs_aug_flip
    assert fl(None, B, 1, 4, 5, 6, 3, None) == einval and fl(A, None, 1, 4, 5, 6, 3, None) == einval and fl(A, A, 1, 4, 5, 6, 3, None) == einval
    assert fl(A, B, 0, 4, 5, 6, 3, None) == einval and fl(A, B, 1, 4, 5, 6, 8, None) == einval and fl(A, B, 1, 4, 5, 6, -1, None) == einval
    assert fl(A, B, 1, 0, 5, 6, 3, None) == eshape and fl(A + 1, B, 1, 4, 5, 6, 3, None) == ealign and fl(A, B + 2, 1, 4, 5, 6, 3, None) == ealign
