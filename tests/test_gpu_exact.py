"""The convolution and weight-gradient kernels against fp64 on inputs for which the right answer has NO rounding error: torch.equal, no tolerance.

tests/exact_util.py explains the idea and makes the data: small integers (exact in bf16, fp16, fp32; one limb in the three-limb fp32 kernels), sized so that
every partial sum stays below 2^24, so fp32 accumulation is exact in any order — whatever the tile walk, split-K, slab reduction or atomics order, in both
builds.  fp32 outputs (dW, db, the fp32 mode's y and gx, the statistics) equal the fp64 reference; 16-bit outputs equal it after one round-to-nearest-even
(exact_util.stored).  Lazy inputs are planes with mean exactly 0 and variance exactly 4 (relu((x - mean) * rstd) in {0, 0.5, 1, 2}); the 16-bit kernels stage
that value rounded to 16 bits, which absorbs eps = 1e-5; the fp32 kernels need rstd = 1/2 exactly, so the fp32 lazy cases run with ops.EPS_IN = 0 — and there the
padded input channels (zero planes in the model: variance 0, rstd = inf at eps 0) are filled with such planes too; their weights are zero.
Where the statistics bound leaves a case's weights sparse (large volumes: down to 1.2 % non-zero), the case runs a second time with every weight non-zero
and its statistics left out (test_conv_k3_dense_weights_exact), so that y and gx see every (tap, channel) product there too.
The precondition of every case is asserted when its data is built (exact_util._Case.check) and for all lists on the host (tests/test_host_exact.py).

The shape lists are those of tests/test_gpu_ops.py and tests/test_gpu_layers.py, imported.  Which case reaches which kernel or branch (16-bit modes; the fp32
mode runs igemm_k3x.h / g3_body / g3x_body on the same shapes):
  CONV_CASES            8 -> 8 and 2, 1 -> 8: Toeplitz kernel igemm_k3t.h (backward with the fused weight gradient of igemm_k3tw.h when lazy); 16 / 32-channel
                        chunks, 16- and 32-row weight blocks, one to eight chunks of 32 channels: igemm_k3b.h; padded volume <= 512 voxels — (3, 64, 32, 5, 6, 6),
                        (2, 64, 64, 1, 1, 2), 6^3, 3^3: igemm_k3s.h, the 8^3 and (7, 6, 6) volumes next to its limit stay with k3b
  CONV_CASES_LARGE      tile walks longer than the persistent grid, a sample boundary mid-walk (statistics flush), ragged edges in three axes (37, 30, 50),
                        (9, 10, 21), (7, 9, 37); the tall-tile 4x8x16 variant (2, 16, 16, 32, 64, 64), (1, 8, 8, 32, 100, 48) with a ragged y edge; 576 Toeplitz
                        tiles over a 512-workgroup grid (4, 8, 8, 24, 48, 128); 2 real input channels of 8 (2, 2, 8, 12, 20, 70)
  ODD_CHUNK_CASES       3 and 5 chunks of 32 channels in igemm_k3s.h (the last stage of an odd count runs alone); materialised only — the statistics kernel takes
                        the model's channel counts
  EXTREME_ASPECT_CASES  igemm_k3s.h voxel -> (z, y, x) by reciprocal multiplication with one long axis up to the 512-voxel padded limit
  K2_CASES / T2_CASES   g1_kernel gather (stride-2) and scatter (transposed) forms at 8 .. 256 channels, odd coarse grids (3, 5, 7), the 8-channel streaming
                        stride-2 kernel k2s2_scatter8.hip; weight and bias gradients through wgrad.hip
  GROUP_LAYERS          one backward pass of 34 layers -> vs_conv_wgrad_multi: every (channel block, kind) bucket with several layers, more than G3_GROUP_MAX in
                        the largest; under GROUP_SETTINGS the M-packed 8-channel form (g3b_body) on / off, the uber kernel or one grid per bucket, operand swap,
                        the big-tile kernel g3c_body for every layer, the transposed conv's bias gradient folded in or separate; wgrad_group_wgs = 6: every
                        workgroup walks several ragged tiles.  Grouped == per-layer launches (vs_conv_wgrad) bit for bit.
  FUSED_WGRAD_CASES     vs_conv_k3_bwd_data_wgrad (igemm_k3tw.h): backward-data result and its slabs reduced through a VS_WGRAD_SLABS descriptor — ragged,
                        3 samples, 16 samples (128 of the kernel's 192 table pairs); the two real-size shapes are left to the tolerance test

Not compared exactly, by design (not integer arithmetic; the tolerance tests keep them): the input gradient THROUGH a lazy input (InstanceNorm backward apply),
the fused-apply forms, vs_conv_k3_softmax2_bwd_data, the composed Up block, the chain kernels."""
import ctypes
import functools
import zlib

import pytest
import torch

from tests import exact_util as X
from tests.test_gpu_layers import FUSED_WGRAD_CASES
from tests.test_gpu_ops import (CONV_CASES, CONV_CASES_LARGE, EXTREME_ASPECT_CASES, GROUP_LAYERS, GROUP_SETTINGS, K2_CASES, ODD_CHUNK_CASES, T2_CASES,
                                group_config)

pytestmark = pytest.mark.gpu

both = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
DT = [torch.float32, torch.bfloat16, torch.float16]
H16 = [torch.bfloat16, torch.float16]

# (case, lazy): every 3x3x3 shape list, materialised and lazy; the odd chunk counts materialised only (no statistics kernel for 96 / 160 channels)
K3_RUNS = [(c, lz) for c in dict.fromkeys(CONV_CASES + CONV_CASES_LARGE + EXTREME_ASPECT_CASES) for lz in (False, True)] + [(c, False) for c in ODD_CHUNK_CASES]
# the runs whose statistics bound leaves the weights sparse get a dense-weight twin: y, gx and dW exactly, no statistics (tests/exact_util.py)
K3_DENSE_RUNS = [(c, lz) for c, lz in K3_RUNS if X.plan_k3(c, lz)["pw"] < 1.0]
K2_RUNS = [((n, c, c, d, h, w), lz) for n, c, d, h, w in K2_CASES for lz in (False, True)]
T2_RUNS = [((n, c, c, d, h, w), lz) for n, c, d, h, w in T2_CASES for lz in (False, True)]
SLAB_CASES = [c for c in FUSED_WGRAD_CASES if c[1] * c[2] * c[3] < 96 ** 3 and c[0] * 8 <= 192]      # minus the real sizes and the refused 25-sample shape
GROUP_RUNS = [group_config(*s) for s in GROUP_SETTINGS] + [dict(wgrad_group_wgs=6)]
SEVERAL_USES = [(2, 16, 16, 8, 8, 16), (2, 16, 16, 4, 6, 8), (2, 16, 16, 12, 4, 8)]                   # test_weight_used_several_times_in_one_backward
_KINDS = {"k3": X.K3Case, "k2": X.K2Case, "t2": X.T2Case}


def _ops():
    from vae_segmentation_amd import ops
    return ops


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (1 << 30)


@functools.lru_cache(maxsize=4)
def _case(kind, case, lazy, dense=False):
    """data and fp64 references of one case, built once and shared by the storage types and the two builds.  In file order those six runs of a case are
    neighbours (the case is the outermost parameter), so a few slots serve; they are few because the references of a large shape take up to 0.4 GB.  Under
    another run order the references (about 9 s of CPU time for all of them) are simply built again: slower, never wrong."""
    if dense:
        return _KINDS[kind](case, lazy, seed=_seed(kind, case, lazy, "dense"), dense=True).check()
    return _KINDS[kind](case, lazy, seed=_seed(kind, case, lazy)).check()


@functools.lru_cache(maxsize=1)
def _group_cases():
    return [_KINDS[kind](tuple(case), True, seed=_seed("group", i)).check() for i, (kind, *case) in enumerate(GROUP_LAYERS)]


@functools.lru_cache(maxsize=1)
def _several_cases():
    """three conv kinds, each weight used at three sizes: the uses share the weight (and bias) of the first"""
    out = {}
    for kind in _KINDS:
        uses = [_KINDS[kind](c, True, seed=_seed("several", kind, i)) for i, c in enumerate(SEVERAL_USES)]
        for u in uses[1:]:
            u.w, u.b = uses[0].w, uses[0].b
        dots = [X.dot_bounds_gather(u.a, u.w, u.gy, u.b, u.transposed) for u in uses]
        X.assert_exact_precondition("several uses, " + kind, {k: sum(d[k] for d in dots) for k in ("dw", "db")}, 0.5)      # the uses are SUMMED
        out[kind] = [u.check() for u in uses]
    return out


def _to_cl(x, cp, dtype, pad=None):
    """planar fp64 -> channels-last storage on the device, channels padded to cp with zeros (or with the planes `pad`)"""
    n, c = x.shape[:2]
    out = torch.zeros((n,) + tuple(x.shape[2:]) + (cp,), dtype=torch.float64)
    out[..., :c] = x.permute(0, 2, 3, 4, 1)
    if pad is not None:
        out[..., c:] = pad.permute(0, 2, 3, 4, 1)
    res = out.to(dtype)
    assert torch.equal(res.double(), out)                     # the operands are exact in the storage type
    return res.cuda().contiguous()


def _from_cl(y, c):
    return y.cpu()[..., :c].permute(0, 4, 1, 2, 3).contiguous()


def _same(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    if not torch.equal(got, ref):
        bad = (got.double() - ref.double()).abs()
        raise AssertionError("%s: %d of %d entries differ, the largest by %g (reference magnitude up to %g)"
                             % (what, int((bad > 0).sum()), bad.numel(), float(bad.max()), float(ref.double().abs().max())))


def _input(ops, c, dtype, monkeypatch):
    """-> (x channels-last on the device, its InstanceNorm statistics or None).  Lazy: the statistics are asserted to be exactly (0, 4 V) per real plane;
    the fp32 mode runs at eps = 0 (rstd = 1/2 exactly) with the padded channels filled with zero-mean variance-4 planes as well."""
    n, cin = c.x.shape[:2]
    cp, pad = ops.cpad(cin), None
    if c.lazy and dtype == torch.float32:
        monkeypatch.setattr(ops, "EPS_IN", 0.0)
        if cp > cin:
            pad = X.unit_planes(n, cp - cin, c.x.shape[2:], _seed("pad", c.name))
    x_cl = _to_cl(c.x, cp, dtype, pad)
    if not c.lazy:
        return x_cl, None
    xs = ops.instnorm_stats(x_cl)
    vox = c.x[0, 0].numel()
    want = torch.tensor([0.0, 4.0 * vox], dtype=torch.float64).expand(n, cin, 2)
    _same(ops.stats_total(xs).cpu()[:, :cin], want, c.name + ": statistics of the raw input")
    return x_cl, xs


@both
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case,lazy", K3_DENSE_RUNS)
def test_conv_k3_dense_weights_exact(case, lazy, dtype, lib_mode, monkeypatch):
    """the shapes whose statistics bound makes the weights of test_conv_k3_exact sparse, again with EVERY weight non-zero: y, dW and (materialised) gx equal
    the reference, so any single dropped or misplaced product of the forward or backward-data kernels shows; the statistics of these data pass 2^24 and are
    not compared"""
    _k3_exact(_case("k3", case, lazy, True), dtype, monkeypatch)


@both
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case,lazy", K3_RUNS)
def test_conv_k3_exact(case, lazy, dtype, lib_mode, monkeypatch):
    """ops.ConvK3 forward and backward as test_conv_k3_fwd_bwd drives them: y, its zero padding channels, the epilogue statistics (of the STORED values, as
    the epilogues sum them), dW; gx for a materialised input."""
    _k3_exact(_case("k3", case, lazy), dtype, monkeypatch)


def _k3_exact(c, dtype, monkeypatch):
    ops = _ops()
    case, lazy = c.case, c.lazy
    n, cin, cout = case[:3]
    x_cl, xs = _input(ops, c, dtype, monkeypatch)
    x_cl.requires_grad_(True)
    w_gpu = c.w.float().cuda().requires_grad_(True)
    y, ys = ops.ConvK3.apply(x_cl, xs, w_gpu, None)
    torch.cuda.synchronize()
    _same(_from_cl(y.detach(), cout), X.stored(c.y, dtype), c.name + ": y")
    if ops.cpad(cout) > cout:
        assert float(y.detach().float()[..., cout:].abs().max()) == 0.0
    if c.with_stats:
        _same(ops.stats_total(ys).cpu()[:, :cout], c.stats[dtype], c.name + ": epilogue statistics")
    y.backward(_to_cl(c.gy, ops.cpad(cout), dtype))
    torch.cuda.synchronize()
    _same(w_gpu.grad.cpu().double(), c.dw, c.name + ": dW")
    if lazy:
        assert bool(torch.isfinite(x_cl.grad.float()).all())            # through InstanceNorm's backward: not integer, left to the tolerance tests
    else:
        _same(_from_cl(x_cl.grad, cin), X.stored(c.gx, dtype), c.name + ": gx")


def _strided(ops, kind, c, dtype, monkeypatch):
    cin, cout = c.case[1:3]
    x_cl, xs = _input(ops, c, dtype, monkeypatch)
    x_cl.requires_grad_(True)
    w_gpu, b_gpu = c.w.float().cuda().requires_grad_(True), c.b.float().cuda().requires_grad_(True)
    y = (ops.ConvK2S2 if kind == "k2" else ops.ConvT2S2).apply(x_cl, xs, w_gpu, b_gpu)
    torch.cuda.synchronize()
    _same(_from_cl(y.detach(), cout), X.stored(c.y, dtype), c.name + ": y")
    y.backward(_to_cl(c.gy, ops.cpad(cout), dtype))
    torch.cuda.synchronize()
    _same(w_gpu.grad.cpu().double(), c.dw, c.name + ": dW")
    _same(b_gpu.grad.cpu().double(), c.db, c.name + ": db")
    if c.lazy:
        assert bool(torch.isfinite(x_cl.grad.float()).all())
    else:
        _same(_from_cl(x_cl.grad, cin), X.stored(c.gx, dtype), c.name + ": gx")


@both
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case,lazy", K2_RUNS)
def test_conv_k2s2_exact(case, lazy, dtype, lib_mode, monkeypatch):
    """ops.ConvK2S2 with an integer bias: y, dW, db; gx for a materialised input"""
    _strided(_ops(), "k2", _case("k2", case, lazy), dtype, monkeypatch)


@both
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case,lazy", T2_RUNS)
def test_conv_transpose_exact(case, lazy, dtype, lib_mode, monkeypatch):
    """ops.ConvT2S2 with an integer bias: y, dW, db; gx for a materialised input"""
    _strided(_ops(), "t2", _case("t2", case, lazy), dtype, monkeypatch)


def _layers_backward(ops, cases, kinds, dtype, monkeypatch, shared=None):
    """every layer's forward, then ONE backward pass (the engine callback at its end issues the grouped launches) -> [(dW, db or None)] on the host, fp64.
    shared: {kind: (weight, bias)} parameters used by every layer of that kind instead of one pair per layer."""
    params, total = [], None
    for kind, c in zip(kinds, cases):
        cout = c.case[2]
        x_cl, xs = _input(ops, c, dtype, monkeypatch)
        if shared is not None:
            w_gpu, b_gpu = shared[kind]
        else:
            w_gpu = c.w.float().cuda().requires_grad_(True)
            b_gpu = None if c.b is None else c.b.float().cuda().requires_grad_(True)
        if kind == "k3":
            y, _ = ops.ConvK3.apply(x_cl, xs, w_gpu, None)
        else:
            y = (ops.ConvK2S2 if kind == "k2" else ops.ConvT2S2).apply(x_cl, xs, w_gpu, b_gpu)
        term = (y.float() * _to_cl(c.gy, ops.cpad(cout), dtype).float()).sum()
        total = term if total is None else total + term
        params.append((w_gpu, b_gpu))
    total.backward()
    torch.cuda.synchronize()
    return [(w.grad.cpu().double(), None if b is None else b.grad.cpu().double()) for w, b in params]


@both
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cfg", GROUP_RUNS, ids=["-".join(s) for s in GROUP_SETTINGS] + ["group_wgs6"])
def test_grouped_weight_gradients_exact(cfg, dtype, lib_mode, monkeypatch):
    """GROUP_LAYERS in one backward pass under every setting of test_grouped_weight_gradients_many_layers and with six workgroups per layer: dW and db equal the
    fp64 reference, and the grouped launches equal the per-layer ones bit for bit."""
    ops = _ops()
    cases, kinds = _group_cases(), [g[0] for g in GROUP_LAYERS]
    with ops.config(**cfg):
        assert ops._GROUP["enabled"]
        got = _layers_backward(ops, cases, kinds, dtype, monkeypatch)
        ops.set_wgrad_grouping(False)
        try:
            single = _layers_backward(ops, cases, kinds, dtype, monkeypatch)
        finally:
            ops.set_wgrad_grouping(True)
    for (gw, gb), (sw, sb), c in zip(got, single, cases):
        _same(gw, sw, c.name + ": dW of the grouped launch against the per-layer launch")
        _same(gw, c.dw, c.name + ": grouped dW")
        _same(sw, c.dw, c.name + ": per-layer dW")
        if gb is not None:
            _same(gb, sb, c.name + ": db of the grouped launch against the per-layer launch")
            _same(gb, c.db, c.name + ": grouped db")
            _same(sb, c.db, c.name + ": per-layer db")


@both
@pytest.mark.parametrize("dtype", DT)
def test_weight_used_several_times_sums_exactly(dtype, lib_mode, monkeypatch):
    """the setup of test_weight_used_several_times_in_one_backward: each of three weights (and two biases) used at three sizes in one pass — the deferred
    launches reduce the descriptors that share a destination; the sum of the uses equals the sum of the fp64 references"""
    ops = _ops()
    by_kind = _several_cases()
    shared = {}
    for kind, uses in by_kind.items():
        b = uses[0].b
        shared[kind] = (uses[0].w.float().cuda().requires_grad_(True), None if b is None else b.float().cuda().requires_grad_(True))
    cases = [u for i in range(len(SEVERAL_USES)) for u in (by_kind["k3"][i], by_kind["k2"][i], by_kind["t2"][i])]
    ops.stats_arena_begin(torch.device("cuda", 0))
    _layers_backward(ops, cases, ["k3", "k2", "t2"] * len(SEVERAL_USES), dtype, monkeypatch, shared=shared)
    for kind, uses in by_kind.items():
        w_gpu, b_gpu = shared[kind]
        _same(w_gpu.grad.cpu().double(), sum(u.dw for u in uses), kind + ": dW summed over three uses")
        if b_gpu is not None:
            _same(b_gpu.grad.cpu().double(), sum(u.db for u in uses), kind + ": db summed over three uses")


@both
@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("case", SLAB_CASES)
def test_k3_bwd_data_with_fused_weight_gradient_exact(case, dtype, lib_mode):
    """vs_conv_k3_bwd_data_wgrad on a stored (applied) gradient, as test_k3_bwd_data_with_fused_weight_gradient calls it without the fused apply: y equals the
    exact backward-data result; the slabs, reduced through a VS_WGRAD_SLABS descriptor of vs_conv_wgrad_multi, equal the exact dW — also with fewer real
    output or input channels in the descriptor."""
    ops = _ops()
    from vae_segmentation_amd._lib import check, lib
    n, d, h, w = case
    c = _case("k3", (n, 8, 8, d, h, w), True)                # g = c.gy, the raw activation c.x (lazy), weights c.w
    g, mx = _to_cl(c.gy, 8, dtype), _to_cl(c.x, 8, dtype)
    ops.stats_arena_begin(g.device)
    mxs = ops.instnorm_stats(mx)
    dt, st = ops.vs_dtype(g), ops._stream()
    assert lib.vs_conv_k3_bwd_data_wgrad_supported(n, d, h, w, 8, 8, dt) == 1
    wpb = ops.pack_weight(c.w.float().cuda(), ops.VS_PACK_ROWS_D1_FLIP, 8, dtype)
    y, sums = torch.empty_like(mx), ops._new_stats(n, 8, g.device)
    nslabs = lib.vs_conv_k3_bwd_data_wgrad_slabs(n, d, h, w)
    assert 0 < nslabs <= 512
    slabs = torch.full((nslabs * 1728,), float("nan"), dtype=torch.float32, device="cuda")
    check(lib.vs_conv_k3_bwd_data_wgrad(g.data_ptr(), None, None, None, wpb.data_ptr(), y.data_ptr(), mx.data_ptr(), mxs.data_ptr(), sums.data_ptr(),
                                        slabs.data_ptr(), n, d, h, w, 8, 8, dt, ops.EPS_IN, st), "bwd_data + wgrad")
    torch.cuda.synchronize()
    _same(_from_cl(y, 8), X.stored(c.gx, dtype), c.name + ": backward-data result")
    for m_real, c_real in ((8, 8), (2, 8), (8, 1)):
        dw = torch.full((m_real, c_real, 27), float("nan"), dtype=torch.float32, device="cuda")
        desc = ops.WgradDesc(slabs.data_ptr(), None, None, None, dw.data_ptr(), None, None, 0, 0, 0, nslabs, 0, 0, 0, 8, 8, m_real, c_real, ops.VS_WGRAD_SLABS, 0)
        arr = (ops.WgradDesc * 1)(desc)
        nbytes = lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(arr), 1, dt)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        check(lib.vs_conv_wgrad_multi(ctypes.addressof(arr), 1, ws.data_ptr(), nbytes, dt, ops.EPS_IN, st), "wgrad_multi (slabs)")
        torch.cuda.synchronize()
        _same(dw.cpu().double(), c.dw[:m_real, :c_real].reshape(m_real, c_real, 27), "%s: dW from %d slabs, %d x %d real channels" % (c.name, nslabs, m_real, c_real))
