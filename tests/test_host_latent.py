"""Host: (1) tests/latent_util.py — the oracle of tests/test_gpu_latent.py — is pinned against the scalar Philox form, the moments of a normal sample and
the stream's separation from its neighbours; these pass without the feature; (2) what of the feature needs no device: the entry points'
--latent_noise flag and the argument checks of the C ABI."""
import math

import numpy as np
import pytest

from tests import augment_util as AU
from tests import elastic_util as EU
from tests import latent_util as LU


# ---- (1) the oracle ------------------------------------------------------------------------------------------------------------------------
def test_ref_latent_normal_is_the_scalar_form_and_a_pure_function():
    seed, draw = 2 ** 40 + 3, 2 ** 32 + 5
    a = LU.ref_latent_normal64(11, seed, draw)                             # odd: the last pair gives its cosine only
    assert a.shape == (11,) and a.dtype == np.float64
    assert np.array_equal(a, LU.ref_latent_normal64(11, seed, draw)) and np.array_equal(a[:6], LU.ref_latent_normal64(6, seed, draw))
    # elements 6 and 7: pair 3 under counter (3, draw low, 0x200, draw high), from the scalar Philox form
    w = EU.ref_philox4x32((3, draw & 0xFFFFFFFF, 0x200, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((w[0] >> 5) * 2 ** 26 + (w[1] >> 6) + 0.5) * 2.0 ** -53
    u2 = ((w[2] >> 5) * 2 ** 26 + (w[3] >> 6)) * 2.0 ** -53
    r = math.sqrt(-2.0 * math.log(u1))
    assert abs(a[6] - r * math.cos(2 * math.pi * u2)) < 1e-15 and abs(a[7] - r * math.sin(2 * math.pi * u2)) < 1e-15
    # element 10, the last of the odd count: pair 5's cosine
    w = EU.ref_philox4x32((5, draw & 0xFFFFFFFF, 0x200, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    u1 = ((w[0] >> 5) * 2 ** 26 + (w[1] >> 6) + 0.5) * 2.0 ** -53
    u2 = ((w[2] >> 5) * 2 ** 26 + (w[3] >> 6)) * 2.0 ** -53
    assert abs(a[10] - math.sqrt(-2.0 * math.log(u1)) * math.cos(2 * math.pi * u2)) < 1e-15
    # float32 once, in the latent's shape: element i = b dim + j
    f = LU.ref_latent_normal((3, 5), seed, draw)
    assert f.dtype == np.float32 and f.shape == (3, 5) and np.array_equal(f.reshape(-1), LU.ref_latent_normal64(15, seed, draw).astype(np.float32))


def test_draws_seeds_and_neighbouring_streams_differ():
    seed, n = 2 ** 40 + 3, 64
    a = LU.ref_latent_normal64(n, seed, 5)
    assert not np.array_equal(a, LU.ref_latent_normal64(n, seed, 6))                      # draws t and t + 1
    assert not np.array_equal(a, LU.ref_latent_normal64(n, seed, 2 ** 32 + 5))            # the draw's high word is in the counter
    assert not np.array_equal(a, LU.ref_latent_normal64(n, seed + 1, 5))                  # both halves of the seed are in the key
    assert not np.array_equal(a, LU.ref_latent_normal64(n, seed + 2 ** 32, 5))
    # no element of one draw reappears in the next (a shifted copy would pass the inequality above)
    assert not np.intersect1d(a, LU.ref_latent_normal64(n, seed, 6)).size
    # counter word 2 = 0x200: not the augmentation stream's values under the same key.  With draw = (sample << 32) the two counters differ in word 2 only
    # — (j, 0, 0x100 + channel, sample) against (q, 0, 0x200, sample)
    for channel in (0, 1):
        aug = AU.ref_normal(n, seed, 7, channel)
        lat = LU.ref_latent_normal64(n, seed, 7 << 32)
        assert np.array_equal(aug, LU.ref_latent_normal64(n, seed, 7 << 32, word2=0x100 + channel))      # same form: only the word tells them apart
        assert not np.array_equal(aug, lat) and not np.intersect1d(aug, lat).size
    # nor the elastic stream's words (counter word 2 = the axis, 0 .. 2)
    w = LU.ref_latent_words(4, seed, 7 << 32)
    for axis in range(3):
        e = LU.ref_latent_words(4, seed, 7 << 32, word2=axis)
        assert not np.array_equal(w[0], e[0]) and not np.array_equal(w[1], e[1])


@pytest.mark.parametrize("seed,draw", [(2 ** 40 + 3, 7), (2 ** 40 + 3, 2 ** 32 + 5), (5, 0)])
def test_ref_latent_normal_has_the_moments_of_a_normal_sample(seed, draw):
    """N = 2^18 against the standard errors of N iid normals, five of each (the bounds of tests/test_host_augment.py)"""
    n = 2 ** 18
    x = LU.ref_latent_normal64(n, seed, draw)
    mean = x.mean()
    c = x - mean
    var, m3, m4 = (c ** 2).mean(), (c ** 3).mean(), (c ** 4).mean()
    print("mean %.3e (se %.3e), var - 1 %.3e (se %.3e), m3 %.3e (se %.3e), m4 - 3 %.3e (se %.3e)"
          % (mean, n ** -0.5, var - 1, (2 / n) ** 0.5, m3, (15 / n) ** 0.5, m4 - 3, (96 / n) ** 0.5))
    assert np.all(np.isfinite(x))
    assert abs(mean) < 5 / np.sqrt(n) and abs(var - 1) < 5 * np.sqrt(2 / n) and abs(m3) < 5 * np.sqrt(15 / n) and abs(m4 - 3) < 5 * np.sqrt(96 / n)


# ---- (2) the feature, without a device ---------------------------------------------------------------------------------------------------------
def test_latent_noise_flag():
    import main_source
    import main_target
    for mod in (main_source, main_target):
        assert mod.parse(["run"]).latent_noise == "torch"
        assert mod.parse(["run", "--latent_noise", "torch"]).latent_noise == "torch"
        assert mod.parse(["run", "--latent_noise", "philox"]).latent_noise == "philox"
        assert mod.parse(["run", "-M", "embed_train", "--latent_noise", "philox", "--no_graph"]).latent_noise == "philox"
        for bad in ("numpy", "", "Philox"):
            with pytest.raises(SystemExit):
                mod.parse(["run", "--latent_noise", bad])


def test_c_abi_answers_argument_errors_before_any_launch():
    """include/vaeseg.h: VS_EINVAL = -1, VS_ESHAPE = -2, VS_EALIGN = -5; the device addresses are never dereferenced on these paths.
    The addresses below are made up: EVERY call here must carry an argument error — a valid combination would launch on them wherever a GPU is
    present (this suite also runs there), so none may ever be added to this test."""
    from vae_segmentation_amd import _lib
    lib = _lib.lib
    einval, eshape, ealign = -1, -2, -5
    M, S, Z, N, ST = 4096, 8192, 12288, 16384, 20480
    nm = lib.vs_latent_normal_philox
    assert nm(None, 8, 1, 2, None) == einval
    assert nm(N, 0, 1, 2, None) == eshape and nm(N, -3, 1, 2, None) == eshape and nm(N, 2 ** 31, 1, 2, None) == eshape and nm(N, 2 ** 40, 1, 2, None) == eshape
    assert nm(N + 2, 8, 1, 2, None) == ealign
    assert nm(None, 0, 1, 2, None) == einval                                # the null pointer is answered first
    fw = lib.vs_reparam_philox_fwd
    assert fw(None, S, ST, 0.35, Z, N, 8, None) == einval and fw(M, None, ST, 0.35, Z, N, 8, None) == einval
    assert fw(M, S, None, 0.35, Z, N, 8, None) == einval and fw(M, S, ST, 0.35, None, N, 8, None) == einval and fw(M, S, ST, 0.35, Z, None, 8, None) == einval
    assert fw(M, S, ST, 0.35, Z, N, 0, None) == eshape and fw(M, S, ST, 0.35, Z, N, -1, None) == eshape and fw(M, S, ST, 0.35, Z, N, 2 ** 31, None) == eshape
    assert fw(M, S, ST + 4, 0.35, Z, N, 8, None) == ealign and fw(M, S, ST + 1, 0.35, Z, N, 8, None) == ealign
    assert fw(M + 2, S, ST, 0.35, Z, N, 8, None) == ealign and fw(M, S, ST, 0.35, Z, N + 1, 8, None) == ealign
    adv = lib.vs_latent_advance
    assert adv(None, None) == einval and adv(ST + 4, None) == ealign
