"""GPU: the intensity augmentation (csrc/augment.hip, ops.aug_stats / philox_normal / gaussian_blur3d / aug_flip, data_gpu.intensity_augment /
IntensityAugment / train_sample(intensity=...)) against tests/augment_util.py (numpy + scipy; pinned by tests/test_host_augment.py).

Tolerance of every op against the oracle on identical float32 input: 2^-22 max|oracle|.  One float32 rounding of an fp64 value errs by at most 2^-24
relative; the device's statistics, pow, log, cos differ from numpy's by fp64-sized amounts, which can move a value across a rounding tie — one float32
ulp, 2^-23 relative; the blur's three roundings add, the filter being a contraction.  No case is excluded.  Statistics: min and max exact, mean and std
to 1e-12 of max(|mean|, std) against numpy's fp64 (sums of at most 2^17 terms shifted by the first voxel err by ~1e-14 of that).  Normals: 1e-12 absolute
(|n| < 8.7, the transcendental functions err by a few ulp of 1e-15)."""
import functools

import numpy as np
import pytest
import torch

from tests import augment_util as AU

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
CHUNK = 8192                                                               # csrc/augment.hip AUG_CHUNK: the voxels one workgroup sums
SHAPES = [(1, 1, 1), (3, 5, 7), (17, 19, 23), (33, 40, 65),
          (1, 1, CHUNK - 1), (2, 64, 64), (1, 1, CHUNK + 1), (1, 47, 523)]      # one chunk - 1 / +- 0 / + 1, three chunks + 5
assert 2 * 64 * 64 == CHUNK and 47 * 523 == 3 * CHUNK + 5
KINDS = ("offset", "unit", "constant")


def _mods():
    from vae_segmentation_amd import data_gpu as D
    from vae_segmentation_amd import ops
    assert all(hasattr(ops, n) for n in ("aug_stats", "philox_normal", "gaussian_blur3d", "aug_flip")) and hasattr(D, "intensity_augment")
    return D, ops


@functools.lru_cache(maxsize=None)
def _plane(shape, kind, seed=0):
    rng = np.random.RandomState(seed + 17 * len(kind) + shape[0] + shape[2])
    if kind == "offset":
        x = rng.randn(*shape) + 100.0                                      # mean 100, std 1: the sums must not cancel
    elif kind == "unit":
        x = rng.rand(*shape) * 2 - 1
    else:
        x = np.full(shape, -3.5)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).cuda()


def _close(got, want, what=""):
    got, want = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape), np.asarray(want, np.float64)
    tol = 2.0 ** -22 * np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s max abs err %.3e (bound %.3e)" % (what, err, tol))
    return bool(np.all(np.isfinite(got))) and err <= tol


def _one(D, x, op):
    """a single op through the public function, on one plane"""
    return D.intensity_augment(_dev(x)[None], [op])[0]


# ---- statistics ------------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("shape", SHAPES)
def test_aug_stats_vs_numpy_fp64(shape, lib_mode):
    D, ops = _mods()
    x = np.stack([_plane(shape, k) for k in KINDS])
    rec = ops.aug_stats(_dev(x))
    assert rec.shape == (3, 4) and rec.dtype == torch.float64 and rec.is_cuda
    rec = rec.cpu().numpy()
    for i, kind in enumerate(KINDS):
        v = x[i].astype(np.float64)
        scale = max(abs(v.mean()), v.std())
        print(kind, shape, "mean err %.3e std err %.3e of %.3e" % (abs(rec[i, 2] - v.mean()), abs(rec[i, 3] - v.std()), scale))
        assert rec[i, 0] == v.min() and rec[i, 1] == v.max()
        assert abs(rec[i, 2] - v.mean()) <= 1e-12 * scale and abs(rec[i, 3] - v.std()) <= 1e-12 * scale
        assert np.array_equal(ops.aug_stats(_dev(x[i])).cpu().numpy(), rec[i])          # a plane's record does not depend on its neighbours
    assert rec[2, 3] == 0.0 and rec[2, 2] == -3.5


# ---- normals ---------------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 1, CHUNK + 1)])          # odd voxel counts: the last pair is half used
def test_philox_normal_vs_oracle(shape, lib_mode):
    D, ops = _mods()
    seed, sample, channel = 2 ** 40 + 3, 7, 1
    n = int(np.prod(shape))
    got = ops.philox_normal(shape, seed, sample, channel)
    assert got.shape == shape and got.dtype == torch.float64
    got = got.cpu().numpy().reshape(-1)
    err = np.abs(got - AU.ref_normal(n, seed, sample, channel)).max()
    print("normals: max abs err %.3e" % err)
    assert err <= 1e-12
    for other in ((seed - 2 ** 40, sample, channel), (seed + 1, sample, channel), (seed, 0, channel), (seed, sample, 0)):
        theirs = ops.philox_normal(shape, *other).cpu().numpy().reshape(-1)
        assert np.abs(theirs - AU.ref_normal(n, *other)).max() <= 1e-12 and np.abs(theirs - got).max() > 1e-3


# ---- every op alone --------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("shape", SHAPES)
def test_point_ops_vs_oracle(shape, lib_mode):
    D, ops = _mods()
    voxels = int(np.prod(shape))
    field = np.random.RandomState(5).normal(0.0, 1.0, (1,) + shape)
    cases = [("brightness", 0.75), ("brightness", 1.25)]
    cases += [("contrast", f, p) for f in (0.75, 1.25) for p in (False, True)]
    cases += [("gamma", g, inv, keep) for g in (0.5, 1.0, 2.0) for inv in (False, True) for keep in (False, True)]
    cases += [("power", 0.7, False), ("restat", 2.0, 0.5, False), ("restat", -1.0, 3.0, True)]
    cases += [("noise", 0.1, field), ("noise", 0.05, (2 ** 40 + 3, 7))]
    for kind in KINDS:
        x = _plane(shape, kind)
        for op in cases:
            got = _one(D, x, op)
            assert got.shape == shape and got.dtype == torch.float32
            assert _close(got, AU.ref_op(x, op), "%s %s %s" % (kind, shape, op[:2] if op[0] == "noise" else op))
    c = _plane(shape, "constant")                                          # a constant plane: power returns it, restat returns mean0
    assert torch.equal(_one(D, c, ("power", 1.5, True)), _dev(c)) and torch.equal(_one(D, c, ("gamma", 0.5, False, True)), _dev(c))
    assert torch.equal(_one(D, c, ("restat", 2.5, 1.5, False)), torch.full(shape, 2.5, device="cuda"))
    # the Philox noise is the standalone normals, and a channel's stream is its own
    x = _plane(shape, "unit")
    n1 = ops.philox_normal(shape, 9, 4, 0)
    two = D.intensity_augment(_dev(np.stack([x, x])), [("noise", 0.1, (9, 4))])
    assert torch.equal(two[0], _one(D, x, ("noise", 0.1, n1[None]))) and (voxels < 4 or not torch.equal(two[0], two[1]))


# ---- blur ------------------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("sigma", [0.1, 0.5, 1.0, 2.0])
def test_blur_vs_scipy(sigma, lib_mode):
    from scipy import ndimage as ndi
    D, ops = _mods()
    tz, ty, tx = ops.blur_tile(sigma)
    assert tx == 32
    shapes = [(1, 1, 1), (2, 3, 4), (9, 10, 11), (17, 19, 67), (tz + 1, ty + 1, tx + 1)]      # lines shorter than the radius; one voxel past the tile
    for shape in shapes:
        for kind in KINDS:
            x = _plane(shape, kind, seed=3)
            want = AU.ref_blur(x, sigma)
            got = ops.gaussian_blur3d(_dev(x), sigma)
            assert _close(got, want, "blur %s %s sigma %g" % (kind, shape, sigma))
            assert _close(got, ndi.gaussian_filter(x, sigma, mode="reflect"), "  against scipy")
            assert torch.equal(_one(D, x, ("blur", sigma)), got)
            if sigma == 0.1 or kind == "constant":
                assert torch.equal(got, _dev(x))                           # radius 0: the input's bits; a constant plane: weights that sum to 1
    with pytest.raises(ValueError, match="sigma"):
        ops.gaussian_blur3d(_dev(_plane((2, 3, 4), "unit")), 2.5)


# ---- flip ------------------------------------------------------------------------------------------------------------------------------------
@BOTH
def test_flip_all_masks_exact(lib_mode):
    D, ops = _mods()
    img = (np.random.RandomState(0).rand(2, 5, 6, 7) * 2 - 1).astype(np.float32)         # no symmetry
    lab = (np.random.RandomState(1).rand(1, 5, 6, 7) > 0.5).astype(np.float32)
    for mask in range(8):
        assert np.array_equal(ops.aug_flip(_dev(img), mask).cpu().numpy(), AU.ref_flip(img, mask))
        assert np.array_equal(ops.aug_flip(_dev(lab), mask).cpu().numpy(), AU.ref_flip(lab, mask))
        assert np.array_equal(D.intensity_augment(_dev(img), [("flip", mask)]).cpu().numpy(), AU.ref_flip(img, mask))
        one = _dev(np.full((1, 1, 1), 3.0, np.float32))
        assert torch.equal(ops.aug_flip(one, mask), one)
    big = _plane((1, 47, 523), "unit")                                     # more than one chunk
    assert np.array_equal(ops.aug_flip(_dev(big), 3).cpu().numpy(), AU.ref_flip(big, 3))
    with pytest.raises(ValueError, match="mask"):
        ops.aug_flip(_dev(img), 8)


# ---- composition -----------------------------------------------------------------------------------------------------------------------------
def _chain_input(shape=(17, 19, 23)):
    return np.stack([_plane(shape, "offset", seed=1), _plane(shape, "unit", seed=2)])


def _full_chain(noise):
    return [("noise", 0.08, noise), ("blur", [0.6, 0.9]), ("brightness", [0.8, 1.2]), ("contrast", [0.8, 1.2], True), ("gamma", [0.8, 1.4], True, True),
            ("gamma", [1.3, 0.75], False, True), ("flip", 5)]


def _op_by_op(D, x, ops_list):
    cur = x
    for op in ops_list:
        cur = D.intensity_augment(cur, [op])
    return cur


@BOTH
def test_a_chain_has_the_bits_of_the_single_op_calls(lib_mode):
    D, ops = _mods()
    x = _dev(_chain_input())
    full = _full_chain((2 ** 33 + 1, 3))
    field = np.random.RandomState(8).normal(0.0, 1.0, tuple(x.shape))
    subsets = [full,
               [("flip", 6), ("noise", 0.05, field), ("brightness", [1.1, None])],                       # the mirror first: one launch with the point ops
               [("contrast", [1.25, 0.75], False), ("flip", 3), ("gamma", 2.0, False, False), ("restat", [0.0, 1.0], [1.0, 2.0], True)],
               [("blur", [None, 2.0]), ("gamma", [0.5, 1.5], True, True), ("noise", [None, 0.02], (5, 0)), ("flip", 7), ("flip", 1), ("brightness", 0.9)]]
    for ops_list in subsets:
        got, want = D.intensity_augment(x, ops_list), _op_by_op(D, x, ops_list)
        assert got.shape == x.shape and torch.equal(got, want), [op[0] for op in ops_list]
        assert bool(torch.isfinite(got).all())
    # ... and the chain is the oracle's, op by op on identical input
    cur = x
    for op in full:
        nxt = D.intensity_augment(cur, [op])
        assert _close(nxt, AU.ref_chain(cur.cpu().numpy(), [op]), "chain step %s" % op[0])
        cur = nxt


# ---- reproducibility -------------------------------------------------------------------------------------------------------------------------
def test_same_bits_twice_under_graph_replay_and_in_both_builds():
    D, ops = _mods()
    x = _dev(_chain_input())
    chain = _full_chain((2 ** 35 + 9, 1))
    was = ops.is_deterministic()
    try:
        results = {}
        for det in (True, False):
            ops.set_deterministic(det)
            a, b = D.intensity_augment(x, chain), D.intensity_augment(x, chain)
            assert torch.equal(a, b)
            results[det] = a
            rec = ops.aug_stats(a)
            assert torch.equal(rec, ops.aug_stats(b))
        assert torch.equal(results[True], results[False])
        ops.set_deterministic(was)
        eager = results[True]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            D.intensity_augment(x, chain)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g = D.intensity_augment(x, chain)
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g, eager)
    finally:
        ops.set_deterministic(was)
    # nothing to do: the input's bits, and nothing launched — the tensor itself
    assert D.intensity_augment(x, []) is x
    closed = [("blur", [None, None]), ("flip", 0), ("brightness", None)]
    assert torch.equal(D.intensity_augment(x, closed), x)


# ---- the transform ---------------------------------------------------------------------------------------------------------------------------
ALL_ON = dict(p_noise=1.0, p_blur=1.0, p_blur_per_channel=1.0, p_brightness=1.0, p_contrast=1.0, p_gamma_inverted=1.0, p_gamma=1.0, p_mirror=1.0)


def test_transform_draws_and_applies_the_oracles_chain():
    D, ops = _mods()
    shape = (12, 13, 14)
    img = np.stack([_plane(shape, "offset", seed=4), _plane(shape, "unit", seed=5)])[None]
    lab = (np.random.RandomState(6).rand(1, 1, *shape) > 0.5).astype(np.float32)
    for noise, kw in (("numpy", ALL_ON), ("philox", ALL_ON), ("philox", {})):
        t = D.IntensityAugment("img", "lab", rng=np.random.RandomState(21), noise=noise, seed=13, **kw)
        want_ops = AU.ref_draw(np.random.RandomState(21), 2, shape, noise=noise, seed=13, n_noised=0, **kw)
        probe = D.IntensityAugment("img", "lab", rng=np.random.RandomState(21), noise=noise, seed=13, **kw)
        assert AU.same_ops(probe.draw(2, shape), want_ops)
        d = t({"img": _dev(img), "lab": _dev(lab)})                        # draws for itself: the same stream
        again = D.IntensityAugment("img", "lab", noise="philox")({"img": _dev(img), "lab": _dev(lab)}, params=[want_ops])
        assert d["img"].shape == img.shape and d["lab"].shape == lab.shape
        assert torch.equal(d["img"], again["img"]) and torch.equal(d["lab"], again["lab"])
        # stage by stage through the functional API, each op against the oracle on the device's own input
        cur = _dev(img[0])
        for op in want_ops:
            nxt = D.intensity_augment(cur, [op])
            assert _close(nxt, AU.ref_chain(cur.cpu().numpy(), [op]), "transform step %s" % op[0])
            cur = nxt
        assert torch.equal(d["img"][0], cur)
        # the label receives the mirror and nothing else
        mask = 0
        for op in want_ops:
            mask ^= op[1] if op[0] == "flip" else 0
        assert np.array_equal(d["lab"].cpu().numpy(), AU.ref_flip(lab, mask))
        if kw:
            assert mask == 7 and len(want_ops) == 7 and not torch.equal(d["img"], _dev(img))
    # every gate closed: the input's bits
    shut = D.IntensityAugment("img", "lab", rng=np.random.RandomState(3), **{k: 0.0 for k in ALL_ON})
    d = shut({"img": _dev(img), "lab": _dev(lab)})
    assert torch.equal(d["img"], _dev(img)) and torch.equal(d["lab"], _dev(lab))


def _merge(shape=(44, 50, 40)):
    rng = np.random.RandomState(7)
    merge = np.zeros(shape + (2,), np.float32)
    merge[..., 0] = rng.randn(*shape) * 300 + 50
    merge[12:30, 14:40, 8:28, 1] = rng.randint(1, 3, size=(18, 26, 20))
    return merge


def test_train_sample_applies_the_stage_after_center_intensities():
    D, ops = _mods()
    merge, patch, mask_index = _dev(_merge()), (32, 32, 32), [[[1, 2], 1]]
    base_i, base_l = D.train_sample(merge, patch, mask_index)
    none_i, none_l = D.train_sample(merge, patch, mask_index, intensity=None)
    assert torch.equal(base_i, none_i) and torch.equal(base_l, none_l)
    t = D.IntensityAugment("venous", "venous_pancreas", noise="philox", seed=3)
    ops_list = [("noise", 0.05, (3, 0)), ("blur", [0.7]), ("contrast", [1.2], True), ("gamma", [0.8], False, True), ("flip", 6)]
    got_i, got_l = D.train_sample(merge, patch, mask_index, intensity=t, intensity_params=ops_list)
    assert got_i.shape == base_i.shape and got_l.shape == base_l.shape
    assert torch.equal(got_i[0], D.intensity_augment(base_i[0], ops_list)) and torch.equal(got_l[0], ops.aug_flip(base_l[0], 6))
    assert float(base_l.sum()) > 0 and not torch.equal(got_l, base_l)
    with pytest.raises(ValueError, match="intensity"):
        D.train_sample(merge, patch, mask_index, intensity=D.IntensityAugment("data", "seg", p_noise=0))


def test_loader_builds_the_stage_only_with_the_flag(tmp_path):
    import main_source
    from vae_segmentation_amd import driver
    D, ops = _mods()
    (tmp_path / "data").mkdir()
    names = []
    for i in range(2):
        np.save(tmp_path / "data" / ("case%d_merge.npy" % i), _merge((40 + 4 * i, 44, 48)))
        names.append("case%d_merge.npy" % i)
    common = ["run", "--real_data", "-R", str(tmp_path / "data"), "--size", "32", "-b", "2"]
    plain = driver.DeviceCaseLoader(names, str(tmp_path / "data"), main_source.parse(common), 2, True, False)
    aug = driver.DeviceCaseLoader(names, str(tmp_path / "data"), main_source.parse(common + ["--aug_intensity"]), 2, True, False, seed=4)
    val = driver.DeviceCaseLoader(names, str(tmp_path / "data"), main_source.parse(common + ["--aug_intensity"]), 2, False, False)
    assert plain.intensity is None and val.intensity is None
    assert isinstance(aug.intensity, D.IntensityAugment) and aug.intensity.noise == "philox" and aug.intensity.seed == 4
    aug.intensity = D.IntensityAugment(driver.IMG_KEY, driver.LABEL_KEY, rng=np.random.RandomState(0), noise="philox", seed=4, **ALL_ON)
    batch = next(iter(aug))
    img, lab = batch[driver.IMG_KEY], batch[driver.LABEL_KEY]
    assert img.shape == (2, 1, 32, 32, 32) and lab.shape == img.shape and bool(torch.isfinite(img).all())
    assert aug.intensity.n_noised == 2 and set(np.unique(lab.cpu().numpy())) <= {0.0, 1.0}
