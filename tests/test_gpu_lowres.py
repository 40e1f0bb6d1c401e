"""GPU: zoom with edge boundaries and the simulated low resolution built on it (csrc/lowres.hip, ops.zoom_edge / simulate_lowres,
data_gpu.lowres_target_shape / intensity_augment's ("lowres", ...) / IntensityAugment(p_lowres=...), --aug_lowres) against tests/lowres_util.py: scipy's
zoom by definition (pinned by tests/test_host_lowres.py).

Tolerance against the oracle on identical float32 input: 2^-22 max|oracle| — one float32 rounding of an fp64 value errs by at most 2^-24 relative, and the
device's fp64 recursion and taps differ from scipy's three-dimensional evaluation by fp64-sized amounts, which can move a value across a rounding tie: one
float32 ulp, 2^-23 relative.  No case is excluded.  Order-0 picks and constant volumes are compared for equality."""
import functools

import numpy as np
import pytest
import torch

from tests import augment_util as AU
from tests import lowres_util as LU

pytestmark = pytest.mark.gpu
BOTH = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
BUNDLE = 64                                                                # csrc/lowres.hip lr_lanes: the lines one workgroup holds at short lengths
PAIRS0 = [(26, 23), (18, 33), (30, 11), (6, 47), (24, 44), (12, 47), (8, 4), (4, 8)]
CASES3 = [((2, 3, 4), (5, 7, 6)), ((5, 7, 6), (2, 3, 4)), ((8, 10, 12), (17, 19, 23)), ((17, 19, 23), (33, 40, 65)), ((1, 1, 1), (1, 1, 1)),
          ((1, 1, 9), (1, 1, 5)), ((1, 2, 509), (1, 3, 512)),
          ((5, 5, 13), (13, 5, 9))]                                        # 5 * 13 = BUNDLE + 1 lines in the z pass (h w) and in the x pass (d' h')
assert 5 * 13 == BUNDLE + 1


def _mods():
    from vae_segmentation_amd import data_gpu as D
    from vae_segmentation_amd import ops
    assert all(hasattr(ops, n) for n in ("zoom_edge", "simulate_lowres", "zoom_edge_bundle")) and hasattr(D, "lowres_target_shape")
    return D, ops


@functools.lru_cache(maxsize=None)
def _vol(shape, kind, seed=0):
    x = LU.volume(shape, kind, seed)
    x.setflags(write=False)
    return x


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).cuda()


def _close(got, want, what=""):
    got, want = got.detach().cpu().numpy().astype(np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    tol = 2.0 ** -22 * np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s max abs err %.3e (bound %.3e)" % (what, err, tol))
    return bool(np.all(np.isfinite(got))) and err <= tol


# ---- order 0 -----------------------------------------------------------------------------------------------------------------------------------
@BOTH
def test_order0_picks_equal_scipys_on_lines_along_every_axis(lib_mode):
    D, ops = _mods()
    for m, n in PAIRS0:
        line = (np.arange(m) * 3 + 1).astype(np.float32)
        for axis in range(3):
            shape, out = [1, 1, 1], [1, 1, 1]
            shape[axis], out[axis] = m, n
            x = line.reshape(shape)
            want = LU.ref_zoom_edge(x, tuple(out), 0, clip=False)
            for clip in (False, True):                                      # a clip of picked voxels changes nothing
                got = ops.zoom_edge(_dev(x), tuple(out), order=0, clip=clip).cpu().numpy()
                assert got.dtype == np.float32 and np.array_equal(got, want), (m, n, axis)
    x = _vol((17, 19, 23), "offset")
    assert np.array_equal(ops.zoom_edge(_dev(x), (9, 30, 12), order=0).cpu().numpy(), LU.ref_zoom_edge(x, (9, 30, 12), 0, False))


# ---- order 3 -----------------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("src,dst", CASES3)
def test_order3_vs_scipy(src, dst, lib_mode):
    D, ops = _mods()
    assert ops.zoom_edge_bundle(max(src), max(dst)) == (BUNDLE if max(src) <= 65 else 8)
    for kind in LU.KINDS:
        x = _vol(src, kind)
        for clip in (True, False):
            got = ops.zoom_edge(_dev(x), dst, order=3, clip=clip)
            assert got.dtype == torch.float32 and tuple(got.shape) == dst
            want = LU.ref_zoom_edge(x, dst, 3, clip)
            assert _close(got, want, "%s -> %s %s clip %d" % (src, dst, kind, clip))
            if kind == "constant":
                assert np.array_equal(got.cpu().numpy(), np.full(dst, 7.25, np.float32))


def test_order3_length_limit_and_argument_errors():
    D, ops = _mods()
    x = _dev(_vol((1, 2, 513), "unit"))
    with pytest.raises(ValueError, match="512"):
        ops.zoom_edge(x, (1, 2, 512), order=3)
    with pytest.raises(ValueError, match="512"):
        ops.zoom_edge(_dev(_vol((1, 2, 9), "unit")), (1, 2, 513), order=3)
    assert tuple(ops.zoom_edge(x, (1, 2, 600), order=1).shape) == (1, 2, 600)          # the limit is the cubic pass's
    y = _dev(_vol((2, 3, 4), "unit"))
    with pytest.raises(ValueError, match="order"):
        ops.zoom_edge(y, (2, 3, 4), order=2)
    with pytest.raises(ValueError, match="shape"):
        ops.zoom_edge(y, (2, 3, 0))
    with pytest.raises(ValueError, match="shape"):
        ops.zoom_edge(y, (2, 3))
    with pytest.raises(TypeError):
        ops.zoom_edge(y.double(), (2, 3, 4))
    with pytest.raises(ValueError):
        ops.zoom_edge(y[None], (2, 3, 4))
    with pytest.raises(ValueError, match="contiguous"):
        ops.zoom_edge(y.permute(2, 1, 0), (2, 3, 4))
    with pytest.raises(ValueError, match="order"):
        ops.simulate_lowres(y, (1, 2, 2), order_up=2)


# ---- order 1 -----------------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("src,dst", [((8, 10, 12), (17, 19, 23)), ((17, 19, 23), (9, 40, 12))])
def test_order1_vs_scipy(src, dst, lib_mode):
    D, ops = _mods()
    for kind in LU.KINDS:
        x = _vol(src, kind)
        for clip in (True, False):
            got = ops.zoom_edge(_dev(x), dst, order=1, clip=clip)
            assert _close(got, LU.ref_zoom_edge(x, dst, 1, clip), "order 1 %s -> %s %s" % (src, dst, kind))
            if kind == "constant":
                assert np.array_equal(got.cpu().numpy(), np.full(dst, 7.25, np.float32))


# ---- clip --------------------------------------------------------------------------------------------------------------------------------------
@BOTH
def test_clip_holds_the_overshoot_of_a_step(lib_mode):
    D, ops = _mods()
    x = -np.ones((10, 12, 14), np.float32)
    x[:, :, 7:] = 1.0
    x[:5, 6:, :] *= -1.0
    dst = tuple(int(round(s * 1.7)) for s in x.shape)
    free = LU.ref_zoom_edge64(x, dst, 3)
    assert free.max() > 1.0 + 1e-3 and free.min() < -1.0 - 1e-3            # the cubic spline overshoots the step: the clip has work to do
    got = ops.zoom_edge(_dev(x), dst, order=3, clip=True)
    assert _close(got, LU.ref_zoom_edge(x, dst, 3, True), "step, clipped")
    assert float(got.max()) == 1.0 and float(got.min()) == -1.0
    got = ops.zoom_edge(_dev(x), dst, order=3, clip=False)
    assert _close(got, LU.ref_zoom_edge(x, dst, 3, False), "step, free")
    assert float(got.max()) > 1.0 and float(got.min()) < -1.0


# ---- the composite -----------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("shape", [(17, 19, 23), (33, 40, 65)])
def test_simulate_lowres_vs_composite_oracle(shape, lib_mode):
    D, ops = _mods()
    x = _vol(shape, "offset")
    xd = _dev(x)
    for zoom, ignore in ((0.5, ()), (0.61, ()), (0.83, ()), (1.0, ()), (0.61, (0,))):
        target = D.lowres_target_shape(shape, zoom, ignore)
        assert target == LU.ref_target_shape(shape, zoom, ignore)
        got = ops.simulate_lowres(xd, target)
        assert _close(got, LU.ref_simulate_lowres(x, target), "lowres %s zoom %g ignore %s" % (shape, zoom, ignore))
        t = ops.zoom_edge(xd, target, order=0, clip=False)
        assert torch.equal(got, ops.zoom_edge(t, shape, order=3, clip=True))
        if zoom == 1.0:
            assert target == shape
    got = ops.simulate_lowres(xd, D.lowres_target_shape(shape, 0.7), order_down=1, order_up=1)
    assert _close(got, LU.ref_simulate_lowres(x, LU.ref_target_shape(shape, 0.7), 1, 1), "lowres 1 / 1")


# ---- intensity_augment -------------------------------------------------------------------------------------------------------------------------
def _chain_input(shape=(17, 19, 23)):
    return np.stack([_vol(shape, "offset", seed=1), _vol(shape, "unit", seed=2)])


@BOTH
def test_the_lowres_op_of_intensity_augment(lib_mode):
    D, ops = _mods()
    x = _dev(_chain_input())
    shape = tuple(x.shape[1:])
    got = D.intensity_augment(x, [("lowres", 0.6)])
    for c in range(2):
        assert torch.equal(got[c], ops.simulate_lowres(x[c].contiguous(), D.lowres_target_shape(shape, 0.6)))
    got = D.intensity_augment(x, [("lowres", [None, 0.75], 1, 3, (2,))])
    assert torch.equal(got[0], x[0])
    assert torch.equal(got[1], ops.simulate_lowres(x[1].contiguous(), D.lowres_target_shape(shape, 0.75, (2,)), 1, 3))
    assert D.intensity_augment(x, [("lowres", [None, None])]) is x
    # a chain has the bits of the single-op calls: the record of what lowres stores is made anew
    chain = [("lowres", [0.55, 0.9]), ("contrast", [0.8, 1.2], True), ("gamma", [0.8, 1.4], False, True)]
    cur = x
    for op in chain:
        cur = D.intensity_augment(cur, [op])
    assert torch.equal(D.intensity_augment(x, chain), cur) and bool(torch.isfinite(cur).all())
    chain = [("brightness", 1.1), ("gamma", 1.2, True, True), ("lowres", 0.7), ("flip", 3), ("lowres", [0.8, None], 0, 1)]
    cur = x
    for op in chain:
        cur = D.intensity_augment(cur, [op])
    assert torch.equal(D.intensity_augment(x, chain), cur)
    with pytest.raises(ValueError, match="vanishes"):
        D.intensity_augment(x, [("brightness", 1.1), ("lowres", 0.02)])
    with pytest.raises(ValueError, match="orders"):
        D.intensity_augment(x, [("lowres", 0.5, 2, 3)])


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------------------
def test_same_bits_twice_under_graph_replay_and_in_both_builds():
    D, ops = _mods()
    x = _dev(_vol((33, 40, 65), "offset"))
    target = D.lowres_target_shape(tuple(x.shape), 0.61)

    def run():
        return ops.simulate_lowres(x, target), ops.zoom_edge(x, (20, 50, 31), order=1, clip=True)

    was = ops.is_deterministic()
    try:
        results = {}
        for det in (True, False):
            ops.set_deterministic(det)
            a, b = run(), run()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            results[det] = a
        assert torch.equal(results[True][0], results[False][0]) and torch.equal(results[True][1], results[False][1])
        ops.set_deterministic(was)
        eager = run()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                       # one stream, no parallel branches
            g = run()
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g[0], eager[0]) and torch.equal(g[1], eager[1]) and torch.equal(eager[0], results[True][0])
    finally:
        ops.set_deterministic(was)


# ---- the transform -----------------------------------------------------------------------------------------------------------------------------
ALL_ON = dict(p_noise=1.0, p_blur=1.0, p_blur_per_channel=1.0, p_brightness=1.0, p_contrast=1.0, p_gamma_inverted=1.0, p_gamma=1.0, p_mirror=1.0)


LOWRES_ON = dict(ALL_ON, p_lowres=1.0, p_lowres_per_channel=1.0)


def test_transform_draws_and_applies_the_oracles_chain():
    D, ops = _mods()
    shape = (12, 13, 14)
    img = np.stack([_vol(shape, "offset", seed=4), _vol(shape, "unit", seed=5)])[None]
    lab = (np.random.RandomState(6).rand(1, 1, *shape) > 0.5).astype(np.float32)
    for kw in (LOWRES_ON, dict(ALL_ON, p_lowres=1.0, lowres_zoom=(0.6, 0.9), lowres_orders=(1, 3), lowres_ignore_axes=(0,)), dict(p_lowres=0.25)):
        t = D.IntensityAugment("img", "lab", rng=np.random.RandomState(21), noise="philox", seed=13, **kw)
        want_ops = LU.ref_draw(np.random.RandomState(21), 2, shape, noise="philox", seed=13, n_noised=0, **kw)
        probe = D.IntensityAugment("img", "lab", rng=np.random.RandomState(21), noise="philox", seed=13, **kw)
        got_ops = probe.draw(2, shape)
        assert AU.same_ops(got_ops, want_ops)
        if kw is LOWRES_ON:                                                 # after contrast, before the two gammas, with the stream's zooms
            assert [op[0] for op in got_ops] == ["noise", "blur", "brightness", "contrast", "lowres", "gamma", "gamma", "flip"]
            assert got_ops[4][2:] == (0, 3, ()) and all(0.5 <= z <= 1.0 for z in got_ops[4][1])
        d = t({"img": _dev(img), "lab": _dev(lab)})                        # draws for itself: the same stream
        again = D.IntensityAugment("img", "lab", noise="philox")({"img": _dev(img), "lab": _dev(lab)}, params=[want_ops])
        assert d["img"].shape == img.shape and d["lab"].shape == lab.shape
        assert torch.equal(d["img"], again["img"]) and torch.equal(d["lab"], again["lab"])
        cur = _dev(img[0])                                                  # stage by stage, each op against the oracle on the device's own input
        for op in want_ops:
            nxt = D.intensity_augment(cur, [op])
            assert _close(nxt, LU.ref_chain(cur.cpu().numpy(), [op]), "transform step %s" % op[0])
            cur = nxt
        assert torch.equal(d["img"][0], cur)
    # without the argument the stream is the one the stage's absence leaves: no variate is drawn for it
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    got = D.IntensityAugment("img", "lab", rng=a, noise="philox", **ALL_ON).draw(2, shape)
    assert AU.same_ops(got, AU.ref_draw(b, 2, shape, noise="philox", **ALL_ON)) and a.uniform() == b.uniform()
    for bad in (dict(lowres_zoom=(0.0, 1.0)), dict(lowres_zoom=(0.9, 0.5)), dict(lowres_zoom=(0.5, 1.5)), dict(lowres_orders=(0, 2)),
                dict(lowres_ignore_axes=(3,))):
        with pytest.raises(ValueError, match="lowres"):
            D.IntensityAugment("img", "lab", p_noise=0, **bad)


def _merge(shape=(44, 50, 40)):
    rng = np.random.RandomState(7)
    merge = np.zeros(shape + (2,), np.float32)
    merge[..., 0] = rng.randn(*shape) * 300 + 50
    merge[12:30, 14:40, 8:28, 1] = rng.randint(1, 3, size=(18, 26, 20))
    return merge


def test_loader_builds_the_stage_only_with_the_flag(tmp_path):
    import main_source
    from vae_segmentation_amd import driver
    D, ops = _mods()
    (tmp_path / "data").mkdir()
    names = []
    for i in range(2):
        np.save(tmp_path / "data" / ("case%d_merge.npy" % i), _merge((40 + 4 * i, 44, 48)))
        names.append("case%d_merge.npy" % i)
    common = ["run", "--real_data", "-R", str(tmp_path / "data"), "--size", "32", "-b", "2", "--aug_intensity"]
    plain = driver.DeviceCaseLoader(names, str(tmp_path / "data"), main_source.parse(common), 2, True, False, seed=4)
    low = driver.DeviceCaseLoader(names, str(tmp_path / "data"), main_source.parse(common + ["--aug_lowres", "0.25"]), 2, True, False, seed=4)
    val = driver.DeviceCaseLoader(names, str(tmp_path / "data"), main_source.parse(common + ["--aug_lowres", "0.25"]), 2, False, False)
    assert plain.intensity.p_lowres == 0.0 and val.intensity is None
    assert isinstance(low.intensity, D.IntensityAugment) and low.intensity.p_lowres == 0.25 and low.intensity.lowres_orders == (0, 3)
    # without the flag: the draws of a transform built before the stage existed
    assert AU.same_ops(plain.intensity.draw(1, (32, 32, 32)), AU.ref_draw(np.random.RandomState(4 + 500), 1, (32, 32, 32), noise="philox", seed=4))
    low.intensity = D.IntensityAugment(driver.IMG_KEY, driver.LABEL_KEY, rng=np.random.RandomState(0), noise="philox", seed=4, **LOWRES_ON)
    batch = next(iter(low))
    img, lab = batch[driver.IMG_KEY], batch[driver.LABEL_KEY]
    assert img.shape == (2, 1, 32, 32, 32) and lab.shape == img.shape and bool(torch.isfinite(img).all())
    assert set(np.unique(lab.cpu().numpy())) <= {0.0, 1.0}
