"""The convolution and weight-gradient kernels against fp64 on inputs for which the right answer has NO rounding error: torch.equal, no tolerance.

tests/exact_util.py explains the idea and makes the data: small integers (exact in bf16, fp16, fp32), sized so that
every partial sum stays below 2^24, so fp32 accumulation is exact in any order — whatever the tile walk, split-K, slab reduction or atomics order, in both
builds.  The fp32 parity mode's kernels split every operand into three bf16 limbs; for them the small integers (one limb) are joined by integers with two and
three non-zero limbs, paired so that the limb products the kernels drop are zero (exact_util.LimbCase; the table at the end of this text).  fp32 outputs (dW, db, the fp32 mode's y and gx, the statistics) equal the fp64 reference; 16-bit outputs equal it after one round-to-nearest-even
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
  MANY_BATCHES          58 tiny layers, 18 of them with biases, in one backward pass: more than one batch through every batching loop of vs_conv_wgrad_multi's host
                        side (G3_GROUP_MAX 24 layers per grid, G3_RED_MAX 56 reductions, G3_BIAS_MAX 16 biases per launch); bf16 in one grid, bf16 with one grid
                        per bucket, bf16 with the transposed convs' biases kept out of their layers' launches, fp32
  FUSED_WGRAD_CASES     vs_conv_k3_bwd_data_wgrad (igemm_k3tw.h): backward-data result and its slabs reduced through a VS_WGRAD_SLABS descriptor — ragged,
                        3 samples, 16 samples (128 of the kernel's 192 table pairs); the two real-size shapes are left to the tolerance test

Not compared exactly, by design (not integer arithmetic; the tolerance tests keep them): the input gradient THROUGH a lazy input (InstanceNorm backward apply),
the fused-apply forms, vs_conv_k3_softmax2_bwd_data, the composed Up block, the chain kernels.

The fp32 limb kernels on operands with SEVERAL non-zero limbs (fp32 only, both builds; LIMB_* lists below, built for the purpose).  The kernels keep
x0 w0 + x0 w1 + x1 w0 + x0 w2 + x1 w1 + x2 w0.  Every case runs in four roles, and a role pins these products (exact_util.LimbCase):
  x3   x three-limb                y: x1 w0, x2 w0 (limb planes 1 and 2 of the staged activation); dW: limbs 1, 2 of the halo operand's planes
  w3   w three-limb                y: x0 w1, x0 w2 (limb fragments 1 and 2 of the VS_F32X3 image); gx: the same in the flipped image
  g3   gy three-limb               gx: limb planes 1, 2 of the staged gradient; dW: limbs 1, 2 of the row operand's planes (the halo operand's under the exchange)
  22   x, w, gy two-limb           y, gx, dW: x1 w1 next to x0 w1 and x1 w0; the second accumulator carries all of them
Which case reaches which instantiation (forward / backward data; tests/test_host_exact.py holds the list to the dispatch's rules, k3x_instantiation; every
3x3x3 case asserts vs_conv_k3_f32_limbs == 1, none falls to k3s_kernel<float>).  vs_config.k3x_ck is 8 by default; 16 is the A/B setting:
  LIMB_K3, k3x_ck = 8   (1, 8, 8, 5, 9, 33) ragged, (3, 8, 8, 7, 9, 37) three samples: k3xt / k3xt
                        (1, 8, 16, 5, 6, 20): k3x<8,16> single chunk / MULTI with 4 x 1 x 16 tiles (YT = 1)
                        (2, 8, 32, 16, 32, 64): k3x<8,32> single chunk (256 workgroups) / k3x<8,16,MULTI>
                        (2, 16, 16, 12, 12, 12), (1, 32, 32, 7, 6, 6): the short-tile launches of <= 128 workgroups, YT = 1, two and four chunks
                        (1, 16, 16, 9, 30, 33), (3, 64, 32, 9, 10, 21): YT = 2, ragged, two and eight chunks / YT = 2 and k3x<8,16,MULTI>
                        (2, 16, 16, 20, 24, 40): k3x<8,16,MULTI>, a sample boundary in the walk; (1, 16, 32, 37, 30, 50): k3x<8,32,MULTI> / k3x<8,16,MULTI>, ragged
  LIMB_K3, k3x_ck = 16  (1, 16, 16, 5, 9, 33): k3x<16,16>; (2, 16, 32, 16, 32, 64): k3x<16,32> / k3x<16,16,MULTI>; (1, 32, 64, 16, 32, 64): k3x<16,32,MULTI> /
                        k3x<16,16,MULTI>; (3, 64, 32, 9, 10, 21): k3x<16,16,MULTI> both ways, four and two chunks, three samples, ragged
  LIMB_K3_LAZY          roles w3 and g3 through the InstanceNorm + ReLU staging of a lazy input (k3xt, 8- and 16-channel chunks); the three-limb operand is
                        the sparse one there, gx is not compared
  every LIMB_K3 run     its weight gradient through g3x_group_kernel (one layer), 16- and 8-channel blocks
  LIMB_K3_FALLBACK      two cases under f32_limbs = 0: k3_kernel<float> and g3_kernel<float>, where the same data are exact as well
  LIMB_G1               g1_kernel<float, .., LIMB>: stride-2 gather and scatter, transposed scatter and gather at 8, 16, 32, 64, 128 channels, odd coarse grids
                        (2, 3, 5), (3, 5, 7); 16- and 32-row tiles (two accumulators) by default, 64-row tiles (RB = 4: one accumulator) for the scatter launches
                        under mt_min_wgs = 1; the 64-voxel split-chunk tiles at 64 and 128 channels; one case under g1_limbs = 0
  LIMB_GROUP            eleven layers in one backward pass: g3x_group_kernel against g3x_kernel (per-layer launches) bit for bit and both against fp64; 16- and
                        8-channel blocks; the operand exchange taken by the lazy layers with Cout <= Cin, and switched off (wgrad_swap = 0); wgrad_group_wgs = 6
  FULL_CASES            not integer data: randn operands, every limb of both operands populated, against fp64 within FULL_K times torch's CPU fp32 error
The epilogue statistics and fused InstanceNorm-backward sums of these data pass 2^24 and are not compared (with_stats = False); the one-limb cases keep them."""
import ctypes
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

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
        assert ops.wgrad_grouping()
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


# More layers than one batch of any grouped launch holds (csrc/wgrad.hip: G3_GROUP_MAX = 24, G3_RED_MAX = 56, G3_BIAS_MAX = 16), all tiny: 40 3x3x3 layers 8 -> 8 on
# a (1, 4, 4, 16) grid and 18 stride-2 / transposed layers 8 -> 8 with biases on a (2, 2, 2) coarse grid, alternating.  58 weight + 18 bias reductions (two
# reduce launches), 18 biases (two bias launches where they do not ride in the all-buckets grid), 58 + 18 = 76 entries in the all-buckets grid (four G3Groups) with
# the transposed convs' biases kept out of their layers' launches, 58 + 9 = 67 (three) by default.
MANY_BATCHES = [("k3", 1, 8, 8, 4, 4, 16)] * 40 + [("k2", 1, 8, 8, 4, 4, 4) if i % 2 == 0 else ("t2", 1, 8, 8, 2, 2, 2) for i in range(18)]
MANY_BATCHES_RUNS = [(torch.bfloat16, {}), (torch.bfloat16, dict(wgrad_uber=0)), (torch.float32, {}), (torch.bfloat16, dict(wgrad_bias_fold=0))]


@functools.lru_cache(maxsize=1)
def _many_batches_cases():
    return [_KINDS[kind](tuple(case), True, seed=_seed("many", i)).check() for i, (kind, *case) in enumerate(MANY_BATCHES)]


@both
@pytest.mark.parametrize("dtype,cfg", MANY_BATCHES_RUNS, ids=["bf16", "bf16-uber0", "fp32", "bf16-fold0"])
def test_grouped_weight_gradients_many_batches_exact(dtype, cfg, lib_mode, monkeypatch):
    """MANY_BATCHES in one backward pass: every batching loop of vs_conv_wgrad_multi's host side (G3Group, G3RedGroup, G3BiasGroup fills) runs more than once —
    bf16 in the all-buckets grid, bf16 with one grid per bucket (the bias partial sums in launches of their own), and fp32 (limb groups, exact-f32 stride-2
    groups, the fp32 bias launches).  As test_grouped_weight_gradients_exact: grouped == per-layer bit for bit, and both equal the fp64 reference."""
    ops = _ops()
    cases, kinds = _many_batches_cases(), [g[0] for g in MANY_BATCHES]
    with ops.config(**cfg):
        assert ops.wgrad_grouping()
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


# ------------------------------------------------------------------------------------------------ fp32 limb kernels: operands with two and three non-zero limbs
def _cdiv(a, b):
    return -(-a // b)


def k3x_instantiation(n, c, m, d, h, w, k3x_ck=8):
    """Which kernel csrc/conv_api.hip k3_tiles + csrc/igemm_k3x.hip g1_dispatch_k3_x3 give a plain (EPI_RAW, no fused apply) fp32 3x3x3 launch with c stored
    input and m stored output channels under the default vs_config but for k3x_ck — restated here so that the case lists below can say, and
    tests/test_host_exact.py can hold them to, which instantiation each case is there for.  A backward-data launch is the same with c and m exchanged."""
    assert c in (8, 16, 32, 64) and m in (8, 16, 32, 64)
    if c % 32 == 0 and (d + 2) * (h + 2) * (w + 2) <= 512:
        return "k3s<float>"                                                # vs_conv_k3_f32_limbs == 0: not a limb kernel
    ck = min(c, k3x_ck)
    nch, rows16 = c // ck, _cdiv(m, 16) * 16
    tiles = n * _cdiv(d, 4) * _cdiv(h, 4) * _cdiv(w, 16)
    mt = 32 if rows16 % 32 == 0 and tiles * (rows16 // 32) >= 256 and (ck == 8 or 2 * n * (c + m) * 4 <= 3000) else 16
    rt = rows16 // mt
    if ck == 8 and c == 8 and m == 8:
        return "k3xt"
    if ck == 8 and nch > 1 and mt == 16:                                   # k3_short_tiles = 2
        zx = n * _cdiv(d, 4) * _cdiv(w, 16)
        if tiles * rt <= 128 and zx * _cdiv(h, 2) * rt <= 256:
            return "k3x<8,16,MULTI,YT=%d>" % (1 if zx * _cdiv(h, 2) * rt <= 128 and zx * h * rt <= 256 else 2)
    return "k3x<%d,%d%s>" % (ck, mt, ",MULTI" if nch > 1 else "")


# (k3x_ck, case, forward instantiation, backward-data instantiation): the smallest shapes that reach each instantiation of g1_dispatch_k3_x3
LIMB_K3 = [
    (8, (1, 8, 8, 5, 9, 33), "k3xt", "k3xt"),                                                # ragged in three axes
    (8, (3, 8, 8, 7, 9, 37), "k3xt", "k3xt"),                                                # three samples
    (8, (1, 8, 16, 5, 6, 20), "k3x<8,16>", "k3x<8,16,MULTI,YT=1>"),
    (8, (2, 8, 32, 16, 32, 64), "k3x<8,32>", "k3x<8,16,MULTI>"),                             # 256 workgroups of 32 rows
    (8, (2, 16, 16, 12, 12, 12), "k3x<8,16,MULTI,YT=1>", "k3x<8,16,MULTI,YT=1>"),            # the 12^3-class launches: 4 x 1 x 16 tiles
    (8, (1, 16, 16, 9, 30, 33), "k3x<8,16,MULTI,YT=2>", "k3x<8,16,MULTI,YT=2>"),             # 4 x 2 x 16 tiles, ragged
    (8, (2, 16, 16, 20, 24, 40), "k3x<8,16,MULTI>", "k3x<8,16,MULTI>"),                      # 180 tiles, a sample boundary in the walk
    (8, (1, 16, 32, 37, 30, 50), "k3x<8,32,MULTI>", "k3x<8,16,MULTI>"),                      # ragged in three axes
    (8, (1, 32, 32, 7, 6, 6), "k3x<8,16,MULTI,YT=1>", "k3x<8,16,MULTI,YT=1>"),               # four chunks; next to the small-volume kernel's limit
    (8, (3, 64, 32, 9, 10, 21), "k3x<8,16,MULTI,YT=2>", "k3x<8,16,MULTI>"),                  # eight chunks, three samples, ragged
    (16, (1, 16, 16, 5, 9, 33), "k3x<16,16>", "k3x<16,16>"),
    (16, (2, 16, 32, 16, 32, 64), "k3x<16,32>", "k3x<16,16,MULTI>"),
    (16, (1, 32, 64, 16, 32, 64), "k3x<16,32,MULTI>", "k3x<16,16,MULTI>"),
    (16, (3, 64, 32, 9, 10, 21), "k3x<16,16,MULTI>", "k3x<16,16,MULTI>"),                    # four chunks, three samples, ragged
]
LIMB_K3_LAZY = [LIMB_K3[0][:2], LIMB_K3[5][:2], LIMB_K3[9][:2], LIMB_K3[10][:2]]             # the staging of a lazy input: k3xt, 8- and 16-channel chunks
LIMB_K3_RUNS = [(ck, case, role, False) for ck, case, _, _ in LIMB_K3 for role in X.ROLES] + \
               [(ck, case, role, True) for ck, case in LIMB_K3_LAZY for role in X.LimbCase.LAZY_ROLES]
# the A/B configuration vs_config.f32_limbs = 0 (exact-f32 MFMA kernels): the same data are exact there too
LIMB_K3_FALLBACK = [(ck, case, role) for ck, case in (LIMB_K3[0][:2], LIMB_K3[5][:2]) for role in X.ROLES]
# g1_kernel<float, ..., LIMB>: (kind, case, vs_config switches).  mt_min_wgs = 1 gives the widest row tile the rows allow — 64 rows (RB = 4: ONE accumulator)
# for the scatter launches (8 C rows: backward data of the stride-2 conv, forward of the transposed one) and 32 rows for a 32-channel gather; the default
# gives 16-row tiles (RB = 1: two accumulators) at these sizes.  64 and 128 channels at <= 64 workgroups: the 64-voxel split-chunk tiles (splitw).
LIMB_G1 = [("k2", (2, 8, 8, 8, 8, 16), {}), ("k2", (2, 8, 8, 8, 8, 16), dict(mt_min_wgs=1)), ("k2", (1, 16, 16, 4, 6, 10), dict(mt_min_wgs=1)),
           ("k2", (1, 32, 32, 4, 4, 4), dict(mt_min_wgs=1)), ("k2", (1, 64, 64, 2, 2, 6), {}), ("k2", (1, 128, 128, 2, 2, 2), {}),
           ("t2", (2, 16, 16, 4, 4, 8), {}), ("t2", (1, 32, 32, 3, 5, 7), dict(mt_min_wgs=1)), ("t2", (1, 128, 128, 3, 3, 3), {}),
           ("t2", (1, 128, 128, 3, 3, 3), dict(mt_min_wgs=1)),
           ("t2", (1, 64, 64, 16, 16, 17), dict(mt_min_wgs=1))]      # 68 row-block tiles, more than the split-chunk form takes: its backward data is a 64-row GATHER tile
LIMB_G1_RUNS = [(kind, case, cfg, role) for kind, case, cfg in LIMB_G1 for role in X.ROLES]
LIMB_G1_FALLBACK = ("k2", (1, 32, 32, 4, 4, 4))
# g3x weight gradients, one backward pass: (case, role, lazy) — 16- and 8-channel blocks; the operand exchange takes the lazy layers with Cout <= Cin
LIMB_GROUP = [((2, 16, 16, 12, 12, 20), "g3", True), ((2, 16, 8, 9, 16, 33), "g3", True), ((2, 8, 16, 7, 9, 18), "g3", True), ((2, 8, 8, 7, 9, 21), "g3", True),
              ((2, 8, 8, 7, 9, 21), "x3", False), ((2, 16, 16, 5, 5, 5), "x3", False), ((1, 32, 32, 7, 6, 6), "22", False), ((1, 32, 8, 5, 7, 19), "g3", False),
              ((2, 16, 32, 8, 8, 8), "22", False), ((2, 8, 16, 5, 6, 20), "x3", False), ((2, 16, 16, 6, 5, 7), "w3", True)]
LIMB_GROUP_CFGS = [{}, dict(wgrad_swap=0), dict(wgrad_group_wgs=6)]


@functools.lru_cache(maxsize=4)
def _limb_case(kind, case, role, lazy=False):
    return X.LimbCase(kind, case, role, lazy, seed=_seed("limbs", kind, case, role, lazy)).check()


@functools.lru_cache(maxsize=1)
def _limb_group_cases():
    return [_limb_case.__wrapped__("k3", case, role, lazy) for case, role, lazy in LIMB_GROUP]


def _assert_limb_launches(ops, case, want):
    from vae_segmentation_amd._lib import lib
    n, cin, cout, d, h, w = case
    assert lib.vs_conv_k3_f32_limbs(d, h, w, ops.cpad(cin)) == want and lib.vs_conv_k3_f32_limbs(d, h, w, ops.cpad(cout)) == want, \
        "%s: not the kernel family this case is there for" % (case,)


@both
@pytest.mark.parametrize("k3x_ck,case,role,lazy", LIMB_K3_RUNS)
def test_conv_k3_limbs_exact(k3x_ck, case, role, lazy, lib_mode, monkeypatch):
    """k3xt / k3x_kernel (forward, backward data) and the g3x weight gradient on operands with two and three non-zero limbs (exact_util.LimbCase): y, dW and
    (materialised) gx equal the plain fp64 convolution.  Neither a tolerance nor a restatement of the limb arithmetic: a limb-1 or limb-2 plane staged from the
    wrong tap or channel, a wrong limb fragment of the VS_F32X3 image, a mis-paired x1 w1 or a lost second accumulator changes most entries."""
    ops = _ops()
    with ops.config(k3x_ck=k3x_ck):
        _assert_limb_launches(ops, case, 1)
        _k3_exact(_limb_case("k3", case, role, lazy), torch.float32, monkeypatch)


@both
@pytest.mark.parametrize("k3x_ck,case,role", LIMB_K3_FALLBACK)
def test_conv_k3_limb_data_exact_without_limbs(k3x_ck, case, role, lib_mode, monkeypatch):
    """the same data under vs_config.f32_limbs = 0: the exact-f32 MFMA kernels (igemm_k3.h, g3_kernel<float>) — the A/B configuration, kept correct"""
    ops = _ops()
    with ops.config(k3x_ck=k3x_ck, f32_limbs=0):
        _assert_limb_launches(ops, case, 0)
        _k3_exact(_limb_case("k3", case, role), torch.float32, monkeypatch)


@both
@pytest.mark.parametrize("kind,case,cfg,role", LIMB_G1_RUNS, ids=["%s-%s-%s-%s" % (k, "x".join(map(str, c)), "wide" if f else "default", r) for k, c, f, r in LIMB_G1_RUNS])
def test_strided_limbs_exact(kind, case, cfg, role, lib_mode, monkeypatch):
    """g1_kernel<float, ..., LIMB> (fragments split in registers, vs_limb_pair), gather and scatter forms, with two accumulators (16- and 32-row tiles) and
    with one (64-row tiles): y, dW, db and gx equal the fp64 reference"""
    ops = _ops()
    with ops.config(**cfg):
        assert ops.get_config()["f32_limbs"] == 1 and ops.get_config()["g1_limbs"] == 1
        _strided(ops, kind, _limb_case(kind, case, role), torch.float32, monkeypatch)


@both
@pytest.mark.parametrize("role", X.ROLES)
def test_strided_limb_data_exact_without_limbs(role, lib_mode, monkeypatch):
    """one stride-2 case under vs_config.g1_limbs = 0 (g1_kernel<float, ..., LIMB = false>)"""
    ops = _ops()
    kind, case = LIMB_G1_FALLBACK
    with ops.config(g1_limbs=0, mt_min_wgs=1):
        _strided(ops, kind, _limb_case(kind, case, role), torch.float32, monkeypatch)


@both
@pytest.mark.parametrize("cfg", LIMB_GROUP_CFGS, ids=["default", "swap0", "group_wgs6"])
def test_grouped_weight_gradients_limbs_exact(cfg, lib_mode, monkeypatch):
    """g3x_group_kernel and g3x_kernel, 16- and 8-channel blocks, operand exchange on and off, on gradients and activations with three and two non-zero limbs:
    LIMB_GROUP in one backward pass — grouped == per-layer bit for bit, and both equal the fp64 reference"""
    ops = _ops()
    cases = _limb_group_cases()
    with ops.config(**cfg):
        assert ops.wgrad_grouping() and ops.get_config()["f32_limbs"] == 1
        got = _layers_backward(ops, cases, ["k3"] * len(cases), torch.float32, monkeypatch)
        ops.set_wgrad_grouping(False)
        try:
            single = _layers_backward(ops, cases, ["k3"] * len(cases), torch.float32, monkeypatch)
        finally:
            ops.set_wgrad_grouping(True)
    for (gw, _), (sw, _), c in zip(got, single, cases):
        _same(gw, sw, c.name + ": dW of the grouped launch against the per-layer launch")
        _same(gw, c.dw, c.name + ": grouped dW")
        _same(sw, c.dw, c.name + ": per-layer dW")


# ------------------------------------------------------------------------------------------------ full-mantissa operands: every limb of both operands at once
FULL_CASES = [(1, 16, 16, 24, 24, 24), (1, 8, 8, 5, 9, 33)]
# Bound on (relative L2 error of the limb kernels against fp64) / (the same of torch's CPU fp32 convolution on the same operands): twice the largest ratio
# measured over y, gx and dW of both cases in both builds, rounded up to a power of two (profiles/limb_exact_accuracy.txt: 0.95 the largest, gx at 24^3); the
# factor of two is for another compiler's instruction order.  tests/test_host_exact.py shows that losing any one of the three smallest kept products puts the
# error at 9 or more times the comparator, so this bound sees such a loss as well.
FULL_K = 2.0


def _rel_l2(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


@functools.lru_cache(maxsize=2)
def full_mantissa_case(case):
    """randn operands in fp32 (weights scaled to unit output variance) -> dict: the operands, the fp64 results y / gx / dw of F.conv3d autograd, and `cpu32`, the
    relative L2 error of the same autograd pass in fp32 on the CPU — the comparator"""
    n, cin, cout, d, h, w = case
    g = X._gen(_seed("full", case))
    x = torch.randn(n, cin, d, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * (27 * cin) ** -0.5
    gy = torch.randn(n, cout, d, h, w, generator=g)
    out = {}
    for dt in (torch.float64, torch.float32):
        xr, wr = x.to(dt, copy=True).requires_grad_(True), wt.to(dt, copy=True).requires_grad_(True)
        y = F.conv3d(xr, wr, None, padding=1)
        (y * gy.to(dt)).sum().backward()
        out[dt] = dict(y=y.detach(), gx=xr.grad, dw=wr.grad)
    ref = out[torch.float64]
    return dict(x=x, w=wt, gy=gy, cpu32={k: _rel_l2(out[torch.float32][k], ref[k]) for k in ref}, **ref)


@both
@pytest.mark.parametrize("case", FULL_CASES)
def test_conv_k3_limbs_full_mantissa(case, lib_mode):
    """ordinary random fp32 operands — all limbs of both operands populated at once, the dropped products not zero: forward, backward data and weight gradient
    of the limb kernels are within FULL_K times the error torch's CPU fp32 convolution makes on the same operands (both against fp64)"""
    ops = _ops()
    n, cin, cout = case[:3]
    _assert_limb_launches(ops, case, 1)
    c = full_mantissa_case(case)
    x_cl = _to_cl(c["x"].double(), ops.cpad(cin), torch.float32).requires_grad_(True)
    w_gpu = c["w"].cuda().requires_grad_(True)
    y, _ = ops.ConvK3.apply(x_cl, None, w_gpu, None)
    y.backward(_to_cl(c["gy"].double(), ops.cpad(cout), torch.float32))
    torch.cuda.synchronize()
    got = dict(y=_from_cl(y.detach(), cout), gx=_from_cl(x_cl.grad, cin), dw=w_gpu.grad.cpu())
    errs = {k: _rel_l2(got[k], c[k]) for k in got}
    print("\nlimbs full mantissa %s %s: %s" % (case, lib_mode, ", ".join("%s %.3e / cpu fp32 %.3e = %.2f" % (k, errs[k], c["cpu32"][k], errs[k] / c["cpu32"][k]) for k in errs)))
    for k in errs:
        assert errs[k] <= FULL_K * c["cpu32"][k], "%s %s: %.3e against %g x %.3e" % (case, k, errs[k], FULL_K, c["cpu32"][k])
