"""Host: (1) tests/elastic_util.py — the oracle of tests/test_gpu_elastic.py — is pinned against Philox4x32-10's known answers, scipy and the draw
order of augment_spatial; these pass without the feature; (2) what of the feature needs no device: MySpatialTransform's constructor, the entry points'
--aug_elastic flag and the argument checks of the C ABI."""
import numpy as np
import pytest

from tests import elastic_util as EU


# ---- (1) the oracle ------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    kat = [((0,) * 4, (0,) * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % w for w in EU.ref_philox4x32(ctr, key)) == want
        arr = EU.ref_philox4x32([np.array([c], np.uint64) for c in ctr], [np.array([k], np.uint64) for k in key])      # the vectorised form ref_noise uses
        assert " ".join("%08x" % int(w[0]) for w in arr) == want


def test_ref_noise_is_a_pure_function_of_its_arguments():
    patch, seed = (3, 4, 5), 2 ** 40 + 3
    a = EU.ref_noise(patch, seed, 7)
    assert a.shape == (3,) + patch and a.dtype == np.float64 and a.min() >= -1.0 and a.max() < 1.0
    assert np.array_equal(a, EU.ref_noise(patch, seed, 7))
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[1], a[2])
    assert not np.array_equal(a, EU.ref_noise(patch, seed, 8)) and not np.array_equal(a, EU.ref_noise(patch, seed + 1, 7))
    assert not np.array_equal(a, EU.ref_noise(patch, seed + 2 ** 32, 7))                       # the high key word is live
    # element (axis 1, voxel 2) from the scalar form
    w = EU.ref_philox4x32((2, 0, 1, 7), (seed & 0xFFFFFFFF, seed >> 32))
    assert a[1].reshape(-1)[2] == 2.0 * (((w[0] >> 5) * 2 ** 26 + (w[1] >> 6)) / 2.0 ** 53) - 1.0


def test_ref_field_is_scipys_constant_mode_filter():
    rng = np.random.RandomState(0)
    noise = rng.random_sample((3, 4, 5, 6)) * 2 - 1
    assert np.array_equal(EU.ref_field(noise, 7.0, 0.1), noise * 7.0)                         # radius int(0.4 + 0.5) = 0: one tap of weight 1
    ones = np.ones((3, 21, 21, 21))
    f = EU.ref_field(ones, 5.0, 2.0)                                                          # radius 8, lines longer than 2 * radius
    assert abs(f[0, 10, 10, 10] - 5.0) < 1e-12 and f[0, 10, 10, 0] < 0.6 * 5.0                # constant mode: zeros beyond the line, not its mirror
    assert f[0, 0, 0, 0] < 0.6 ** 3 * 5.0


def test_ref_draw_consumes_the_elastic_variates_first():
    from oracle import data_cpu as O
    shape = patch = (4, 5, 6)
    dist = [1, 1, 1]
    plain = np.random.RandomState(3)
    O.draw_spatial_params(plain, shape, patch, dist)
    el = np.random.RandomState(3)
    out = EU.ref_draw(el, shape, patch, dist)
    # both generators then continue identically iff the elastic draw took exactly 1 + 2 + 3 * prod(patch) more variates — but from the FRONT of the stream
    probe = np.random.RandomState(3)
    u = probe.uniform(); a = probe.uniform(0.0, 1000.0); s = probe.uniform(10.0, 13.0)
    fields = np.stack([probe.random_sample(patch) * 2 - 1 for _ in range(3)])
    rest = O.draw_spatial_params(probe, shape, patch, dist)
    assert u < 1.0 and len(out) == 5 and out[4][0] == a and out[4][1] == s and np.array_equal(out[4][2], fields)
    assert out[:4] == (rest["angles"], rest["scale"], rest["centre"], True)
    assert el.uniform() == probe.uniform()
    # counted: a sample that is not deformed takes the probability draw alone; a deformed one 2 + 3 * prod(patch) variates more, before the rotation draws
    skip = np.random.RandomState(3)
    skip.random_sample(1)
    skip.random_sample(2 + 3 * int(np.prod(patch)))
    assert O.draw_spatial_params(skip, shape, patch, dist) == rest
    undeformed = np.random.RandomState(3)
    out0 = EU.ref_draw(undeformed, shape, patch, dist, p_el=0.0)
    one = np.random.RandomState(3)
    one.random_sample(1)
    p0 = O.draw_spatial_params(one, shape, patch, dist)
    assert len(out0) == 4 and out0 == (p0["angles"], p0["scale"], p0["centre"], True) and undeformed.uniform() == one.uniform()
    assert len(EU.ref_draw(np.random.RandomState(3), shape, patch, dist, elastic=False)) == 4


# ---- (2) the feature, without a device -------------------------------------------------------------------------------------------------------
def test_transform_constructor_asks_for_a_noise_source():
    from vae_segmentation_amd import data_gpu as D
    with pytest.raises(NotImplementedError, match="noise"):
        D.MySpatialTransform((32,) * 3, do_elastic_deform=True, border_mode_data="constant")
    for noise in ("numpy", "philox"):
        t = D.MySpatialTransform((32,) * 3, do_elastic_deform=True, border_mode_data="constant", noise=noise, seed=5)
        assert t.do_elastic and t.noise == noise
    with pytest.raises(ValueError, match="noise"):
        D.MySpatialTransform((32,) * 3, do_elastic_deform=True, border_mode_data="constant", noise="sobol")
    with pytest.raises(ValueError, match="sigma"):
        D.MySpatialTransform((32,) * 3, do_elastic_deform=True, border_mode_data="constant", noise="philox", sigma=(10, 40.0))
    assert not D.MySpatialTransform((32,) * 3, do_elastic_deform=False, border_mode_data="constant").do_elastic


def test_transform_draws_in_the_oracles_order_and_counts_philox_samples():
    from vae_segmentation_amd import data_gpu as D
    patch, dist = (4, 5, 6), [1, 1, 1]
    kw = dict(random_crop=True, scale=(0.85, 1.15), angle_x=(-0.2, 0.2), angle_y=(-0.2, 0.2), angle_z=(-0.2, 0.2), border_mode_data="constant",
              alpha=(0.0, 500.0), sigma=(10.0, 30.0))
    t = D.MySpatialTransform(patch, dist, do_elastic_deform=True, noise="numpy", rng=np.random.RandomState(9), **kw)
    got = t.draw(patch)
    want = EU.ref_draw(np.random.RandomState(9), patch, patch, dist, alpha=(0.0, 500.0), sigma=(10.0, 30.0))
    assert len(got) == 5 and got[:4] == want[:4] and got[4][:2] == want[4][:2] and np.array_equal(got[4][2], want[4][2])
    t = D.MySpatialTransform(patch, dist, do_elastic_deform=True, noise="philox", seed=11, rng=np.random.RandomState(9), **kw)
    first, second = t.draw(patch), t.draw(patch)
    assert first[4][2] == (11, 0) and second[4][2] == (11, 1) and first[4][:2] == want[4][:2]       # alpha and sigma still come from rng
    t = D.MySpatialTransform(patch, dist, do_elastic_deform=True, p_el_per_sample=0, rng=np.random.RandomState(9), **kw)      # off: the 4-tuple, today's stream
    from oracle import data_cpu as O
    p = O.draw_spatial_params(np.random.RandomState(9), patch, patch, dist)
    assert t.draw(patch) == (p["angles"], p["scale"], p["centre"], True)


def test_aug_elastic_flag():
    import main_source
    import main_target
    for mod in (main_source, main_target):
        assert mod.parse(["run"]).aug_elastic == 0
        assert mod.parse(["run", "--real_data", "--aug_elastic", "0.25"]).aug_elastic == 0.25
        assert mod.parse(["run", "--aug_elastic", "1"]).aug_elastic == 1.0
        for bad in (["--aug_elastic", "1.5"], ["--aug_elastic", "-0.1"], ["--aug_elastic", "nan"], ["--aug_elastic", "0.5", "--no_aug"]):
            with pytest.raises(SystemExit):
                mod.parse(["run"] + bad)


def test_c_abi_answers_argument_errors_before_any_launch():
    """include/vaeseg.h: VS_EINVAL = -1, VS_ESHAPE = -2, VS_EALIGN = -5; the addresses are never dereferenced on these paths"""
    from vae_segmentation_amd import _lib
    lib = _lib.lib
    einval, eshape, ealign = -1, -2, -5
    A, B, C = 4096, 8192, 12288
    f = lib.vs_data_elastic_field
    assert f(None, B, C, 4, 5, 6, 10.0, 1.0, None) == einval and f(A, None, C, 4, 5, 6, 10.0, 1.0, None) == einval
    assert f(A, B, None, 4, 5, 6, 10.0, 1.0, None) == einval and f(A, A, C, 4, 5, 6, 10.0, 1.0, None) == einval
    for sigma in (0.0, -1.0, float("nan"), float("inf"), 32.125, 1e300):                     # 32.125: radius int(129.0) = 129
        assert f(A, B, C, 4, 5, 6, sigma, 1.0, None) == einval
    assert f(A, B, C, 4, 5, 6, 10.0, float("nan"), None) == einval
    assert f(A, B, C, 0, 5, 6, 10.0, 1.0, None) == eshape and f(A, B, C, 1024, 1024, 1024, 10.0, 1.0, None) == eshape
    assert f(A, B, C, 1024, 1024, 700, 10.0, 1.0, None) == eshape                            # one field fits an int, three do not
    assert f(A + 4, B, C, 4, 5, 6, 10.0, 1.0, None) == ealign
    n = lib.vs_data_noise_philox
    assert n(None, 4, 5, 6, 1, 2, None) == einval and n(A, 4, 0, 6, 1, 2, None) == eshape and n(A + 4, 4, 5, 6, 1, 2, None) == ealign
    w = lib.vs_data_warp_sample
    assert w(None, A, B, 4, 5, 6, 4, 5, 6, C, C, 3, 0.0, None) == einval and w(A, B, None, 4, 5, 6, 4, 5, 6, C, C, 3, 0.0, None) == einval
    assert w(A, B, C, 4, 5, 6, 4, 5, 6, C, C, 1, 0.0, None) == einval and w(A, B, C, 4, 5, 6, 4, 0, 6, C, C, 3, 0.0, None) == eshape
    assert w(A, B, C + 4, 4, 5, 6, 4, 5, 6, C, C, 0, 0.0, None) == ealign
