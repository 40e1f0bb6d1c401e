"""InstanceNorm statistics per (sample, channel) against fp64, on data with an offset.

Every InstanceNorm of the step reads its mean / rstd from a (sum, sumsq) pair per (n, c) that a kernel epilogue accumulated, and the backward
reads (sum g mask, sum g mask xhat) the same way.  The op tests bound these pairs only globally, on centred data (U[-1, 1] inputs, zero-mean
weights, the dead conv bias never added), where a partial that is lost, doubled or credited to the neighbouring sample moves a channel sum by
about its own noise.  Here every channel gets an offset R = |mean| / std from the DATA: a non-negative input with a nonzero mean (as
post-ReLU activations) and a nonzero weight sum per output channel (mu_w added to the centre tap of zero-mean weights), mu_w solved so
that the fp64 output hits R in {0, 4, 30, 300} over the channels with alternating signs.  Each (n, c) is then checked on its own
(tests/stats_util.py): mean within 1e-5 (1 + R) std, rstd within 1e-4 (R <= 30; 5e-3 at R ~ 300, the one-pass fp32 lane sums' own
limit, or R^2 2^-23 where larger), sum within 1e-5 sqrt(N Q).  At R = 30 one lost tile of ~1700 moves the mean by ~2 % of std.

Which values the statistics are of — every producer accumulates the pair from the value it STORES (after the rounding to the storage type),
read off each epilogue.  So the pair is gated against the fp64 two-pass statistics of the kernel's own stored output, and that output
against the fp64 result on the storage-rounded operands, rounded the same way, to one storage ulp (a fixed reference rounded apart from the
kernel's would move a 64-voxel channel sum by a whole ulp per element on a rounding edge):
    igemm_k3.h   k3_kernel<float>          fp32 storage: the fp32 value              (v = E::rnd(acc + bias), rnd = identity for float)
    igemm_k3b.h  k3b_kernel<16-bit>        stored 16-bit value                        (pack2, then H16::lo / hi of the packed word)
    igemm_k3t.h  k3t_kernel<16-bit>        stored 16-bit value                        ("the statistics are those of the stored values")
    igemm_k3s.h  k3s_kernel / split reduce stored value (16-bit: the packed word; fp32: o + bias)
    igemm_k3x.h  k3x / k3xt (fp32 parity)  fp32 value                                 (v = acc + bias)
    norm.hip     vs_instnorm_stats         the stored input itself, fp64 lane sums
    backward pairs (same epilogues, SUMS)  stored 16-bit / fp32 backward-data value g; mask and xhat = (x - mean) * rstd in fp32 from the
                                           kernel's own float mean / rstd table
All inputs here are materialised (xs = None): the lazy IN+ReLU-on-load inputs round the normalised activation to 16 bits while staging, so
an fp64 reference on the rounded stored input differs from the kernel by that rounding — their per-(n, c) checks, with a gate scaled by the
storage type's tolerance, sit next to the global ones in test_gpu_ops.py / test_gpu_layers.py / test_gpu_wide.py / test_gpu_up.py.

The kernel named in each case id is the one conv_api.hip / igemm_k3_h16.inc / igemm_k3_f32.hip dispatch the case to (f32_limbs=0: the
exact-f32 MFMA k3_kernel of igemm_k3.h instead of the parity mode's limb kernels)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import stats_util as SU
from tests.test_gpu_layers import _last_call
from tests.test_gpu_ops import q, to_cl

pytestmark = pytest.mark.gpu

R_TARGETS = (0.0, 4.0, 30.0, 300.0)
BF, F32 = torch.bfloat16, torch.float32

# (kernel, storage dtype, vs_config switches, (N, Cin, Cout, D, H, W))
FWD_CASES = [
    ("k3_kernel-ragged", F32, {"f32_limbs": 0}, (3, 64, 32, 9, 10, 21)),                  # 4x1x16 tiles (under-filled launch), ragged in all three axes
    ("k3_kernel-persistent", F32, {"f32_limbs": 0}, (3, 32, 32, 36, 64, 64)),             # 1728 tiles on a grid of 1024: walks, sample boundary mid-walk
    ("k3_kernel_TY-persistent", F32, {"f32_limbs": 0}, (4, 8, 8, 24, 48, 128)),           # 8 -> 8 y-Toeplitz rows, 4 samples
    ("k3_kernel_TY-96cube", F32, {"f32_limbs": 0}, (2, 8, 8, 96, 96, 96)),
    ("k3t-96cube", BF, {}, (2, 8, 8, 96, 96, 96)),                                         # the 8 -> 8 full-resolution layers
    ("k3t-ragged", BF, {}, (4, 8, 8, 24, 48, 128)),
    ("k3b-128cube", BF, {}, (1, 16, 8, 128, 128, 128)),                                    # 8192 tiles: too many for the tall variant
    ("k3b_tall-48cube", BF, {}, (2, 16, 16, 48, 48, 48)),                                  # 16-channel chunks, <= 2048 tiles: 4x8x16 tiles
    ("k3b-48cube", BF, {}, (2, 32, 16, 48, 48, 48)),                                       # 32-channel chunks
    ("k3b-24cube", BF, {}, (2, 32, 32, 24, 24, 24)),
    ("k3b-ragged", BF, {}, (3, 64, 32, 9, 10, 21)),
    ("k3s-ragged", BF, {}, (3, 64, 32, 5, 6, 6)),                                          # small volumes: padded sample <= 512 voxels
    ("k3s-4cube", BF, {}, (2, 128, 128, 4, 4, 4)),
    ("k3s_split-512ch", BF, {}, (2, 512, 512, 4, 4, 4)),                                   # > 256 input channels: slices + k3s_split_reduce_kernel
    ("k3x-24cube", F32, {}, (2, 32, 32, 24, 24, 24)),                                      # fp32 parity mode: three-limb bf16 MFMA
    ("k3xt-48cube", F32, {}, (2, 8, 8, 48, 48, 48)),
    ("k3s_f32-4cube", F32, {}, (2, 64, 64, 4, 4, 4)),
]


def _store(y64, dtype):
    """the value a kernel stores (and takes its statistics of): fp64 -> storage type -> fp64"""
    return y64.to(torch.float32).to(dtype).double()


def _signed_targets(c):
    """R target per output channel: 0, 4, 30, 300 round-robin, the sign alternating every other channel"""
    return np.array([R_TARGETS[i % 4] * (1 if (i // 2) % 2 == 0 else -1) for i in range(c)])


def _solve_mu(y0, s, targets):
    """per output channel: mu with mean(y0 + mu s) / std(y0 + mu s) = target (pooled over the samples).  y0 (n, c, V), s (n, V) fp64"""
    mus = []
    sv = s.reshape(-1)
    ms, vs = float(sv.mean()), float(sv.var(unbiased=False))
    for c, t in enumerate(targets):
        yv = y0[:, c].reshape(-1)
        m0, v0 = float(yv.mean()), float(yv.var(unbiased=False))
        cov = float(((yv - m0) * (sv - ms)).mean())
        if t == 0.0:
            mus.append(-m0 / ms)
            continue
        r2 = t * t
        a, b, cc = ms * ms - r2 * vs, 2 * (m0 * ms - r2 * cov), m0 * m0 - r2 * v0
        assert a > 0, "offset R %g out of reach of this input (its own R is %.0f)" % (t, ms / vs ** 0.5)
        roots = [float(x.real) for x in np.roots([a, b, cc]) if abs(x.imag) < 1e-9 * max(1.0, abs(x.real))]
        roots = [m for m in roots if np.sign(m0 + m * ms) == np.sign(t)]
        mus.append(min(roots, key=abs))
    return torch.tensor(mus, dtype=torch.float64)


@_last_call
def _fwd_ref(case, dtype):
    """offset inputs and weights for a 3x3x3 case and the fp64 reference statistics of the stored output (memoised: both builds share it)"""
    n, cin, cout, d, h, w = case
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + d)
    # a non-negative input with a large mean against its spread: the centre-tap term mu_w sum_c x can then carry an offset up to
    # R ~ 700 (sqrt(cin) (b + 1/2) / 0.289) past the border structure of the zero-padded taps
    b = 0.289 * 700.0 / cin ** 0.5
    x = q(torch.rand(n, cin, d, h, w, generator=g) + b, dtype)
    w0 = (torch.rand(cout, cin, 3, 3, 3, generator=g) * 2 - 1) * (3.0 / (27 * cin)) ** 0.5
    w0 -= w0.mean((1, 2, 3, 4), keepdim=True)
    xd = x.double()
    y0 = F.conv3d(xd, q(w0, dtype).double(), padding=1).reshape(n, cout, -1)
    s = xd.sum(1).reshape(n, -1)
    mu = _solve_mu(y0, s, _signed_targets(cout))
    wt = w0.double().clone()
    wt[:, :, 1, 1, 1] += mu[:, None]
    wt = q(wt.float(), dtype)
    y_st = _store(F.conv3d(xd, wt.double(), padding=1), dtype).reshape(n, cout, -1)
    return x, wt, y_st


# one storage ulp of the largest element (bf16: up to 2^-7 of it): the stored output is the fp64 result on the rounded operands, rounded
# once (a value on a rounding edge may land one ulp away)
# fp32: K = 27 C products accumulated in fp32, whose terms are far larger than a low-R channel's outputs (the offset weights cancel): 1e-5 of
# the channel's largest value (measured 3.2e-6 at C = 32 .. 64)
Y_TOL = {BF: 2.0 ** -7, F32: 1e-5}


def _y_check(tag, y, y_st, tol):
    """y against y_st per (n, c), relative to the channel's own largest |y_st| (a low-R channel is not hidden behind a high-R one)"""
    err = (y - y_st).abs().amax(-1) / y_st.abs().amax(-1).clamp_min(1e-30)
    assert float(err.max()) <= tol * 1.01, "%s: stored output off at (n, c) %s: %.2e" % (tag, (err > tol * 1.01).nonzero()[:4].tolist(), float(err.max()))


def _fwd_check(tag, dtype, tot, y, y_st, y_tol=None, targets=True):
    """y: the kernel's stored output (n, c, V); y_st: the fp64 reference rounded to the storage type.  The statistics are gated against the
    two-pass fp64 statistics of y itself — what the kernel stored is what its pair must describe; a reference rounded apart from the kernel's
    would move a small volume's sum by a whole ulp per differing element — and y against y_st per (n, c)"""
    _y_check(tag, y, y_st, Y_TOL[dtype] if y_tol is None else y_tol)
    worst = SU.check_stats(tot, SU.two_pass(y), tag)
    if targets:
        R = SU.two_pass(y_st)["R"]
        assert float(R.max()) > 200 and float(R.min()) < 1 and bool(((R > 20) & (R < 40)).any()), "offsets not reached: R %s" % R[0].tolist()
    return worst


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("kernel,dtype,cfg,case", FWD_CASES, ids=["%s-%s-%s" % (k, str(dt).split(".")[-1], "x".join(map(str, c))) for k, dt, _, c in FWD_CASES])
def test_forward_stats_per_channel_vs_fp64(kernel, dtype, cfg, case, lib_mode):
    from vae_segmentation_amd import ops
    n, cin, cout, d, h, w = case
    x, wt, y_st = _fwd_ref(case, dtype)
    x_cl = to_cl(x, ops.cpad(cin), dtype)
    w_gpu = wt.cuda()
    with ops.config(**cfg):
        ops.clear_pack_cache()                 # the weight image depends on the switches (fp32: limb image or plain)
        ops.stats_arena_begin(x_cl.device)
        with torch.no_grad():
            y, ys = ops.ConvK3.apply(x_cl, None, w_gpu, None)
        torch.cuda.synchronize()
        ops.clear_pack_cache()
    tot = ops.stats_total(ys).cpu()[:, :cout]
    _fwd_check("%s %s %s %s" % (kernel, case, dtype, lib_mode), dtype, tot, _cl_to_ncv(y, cout), y_st)


# vs_instnorm_stats (norm.hip): the statistics of a stored tensor (the network input, skip merges, every non-conv InstanceNorm)
NORM_CASES = [(F32, (2, 16, 96)), (BF, (2, 16, 96)), (BF, (2, 512, 4)), (F32, (2, 512, 4))]


@_last_call
def _norm_ref(case, dtype):
    n, c, s = case
    g = torch.Generator().manual_seed(c + s)
    t = torch.tensor(_signed_targets(c), dtype=torch.float32)
    x = q(torch.randn(n, c, s, s, s, generator=g) * 0.8 + (t * 0.8)[None, :, None, None, None], dtype)
    return x, x.double().reshape(n, c, -1)


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("dtype,case", NORM_CASES, ids=["instnorm_stats-%s-%s" % (str(dt).split(".")[-1], "x".join(map(str, c))) for dt, c in NORM_CASES])
def test_instnorm_stats_per_channel_vs_fp64(dtype, case, lib_mode):
    from vae_segmentation_amd import ops
    x, x_st = _norm_ref(case, dtype)
    x_cl = to_cl(x, case[1], dtype)
    ops.stats_arena_begin(x_cl.device)
    tot = ops.stats_total(ops.instnorm_stats(x_cl)).cpu()
    _fwd_check("instnorm_stats %s %s %s" % (case, dtype, lib_mode), dtype, tot, _cl_to_ncv(x_cl, case[1]), x_st)


# ---- backward pairs: (sum g 1[xhat > 0], sum g 1[xhat > 0] xhat) per (n, c) of the conv's own lazy input -------------------------------------------------
# the pair against fp64 sums of the gradient the kernel stored.  xhat is formed from the kernel's float rstd, which the 16-bit kernels take
# from rsqrt + one Newton step (~1e-7 relative, csrc/common.h stats_to_mean_rstd_fast) and this reference from fp64: with g offset per channel,
# sum g m xhat is ~sqrt(N) times its scale sqrt(sum (g m xhat)^2), so that 1e-7 shows as ~1e-5 of the scale at 48^3 (measured 1.2e-5)
BWD_TOL = 1e-4


def _kernel_mean_rstd(ops, st, count):
    """the float mean / rstd table a kernel builds from a statistics buffer (fp64 pair -> float)"""
    m, r = SU.pair_mean_rstd(ops.stats_total(st).cpu(), count)
    return m.float(), r.float()


def _bwd_pairs_ref(g_st, mx, mm, mr):
    """fp64 sums of the stored gradient g_st (n, c, V) over the mask of xhat = (x - mean) * rstd, evaluated in fp32 as the kernels do"""
    xh = (mx.float() - mm[..., None]) * mr[..., None]
    gm = torch.where(xh > 0, g_st, torch.zeros_like(g_st))
    gmx = gm * xh.double()
    return torch.stack([gm.sum(-1), gmx.sum(-1)], -1), torch.stack([(gm * gm).sum(-1).sqrt(), (gmx * gmx).sum(-1).sqrt()], -1)


def _check_bwd_pairs(tag, tot, ref, scale, tol):
    err = (tot.double() - ref).abs() / scale.clamp_min(1e-300)
    print("\n%s: worst |dS1| %.1e |dS2| %.1e (of the fp64 scale)" % (tag, float(err[..., 0].max()), float(err[..., 1].max())))
    assert float(err.max()) < tol, "%s: backward pair off at (n, c) %s" % (tag, (err > tol).nonzero()[:4].tolist())


def _cl_to_ncv(t, c):
    n = t.shape[0]
    return t.double().cpu()[..., :c].reshape(n, -1, c).permute(0, 2, 1)


BWD_CASES = [("k3t_sums", BF, (2, 8, 8, 20, 12, 40)), ("k3t_sums", BF, (2, 8, 8, 48, 48, 48)), ("k3xt_sums", F32, (2, 8, 8, 20, 12, 40)),
             ("k3b_sums", BF, (2, 32, 32, 24, 24, 24)), ("k3s_sums", BF, (3, 64, 32, 5, 6, 6)), ("k3x_sums", F32, (2, 32, 32, 24, 24, 24))]


@_last_call
def _bwd_inputs(case, dtype):
    """gy (with a constant component per channel, as Dice's k1 t - k2 gives), the conv's lazy input mx with an offset, weights"""
    n, cin, cout, d, h, w = case
    g = torch.Generator().manual_seed(5 * cin + d)
    gy = q(torch.randn(n, cout, d, h, w, generator=g) + torch.tensor([3.0 * (-1) ** c for c in range(cout)])[None, :, None, None, None], dtype)
    mx = q(torch.randn(n, cin, d, h, w, generator=g) * 0.8 - 0.1, dtype)
    wt = q((torch.rand(cout, cin, 3, 3, 3, generator=g) * 2 - 1) * (3.0 / (27 * cout)) ** 0.5 + 0.02, dtype)
    g64 = F.conv_transpose3d(gy.double(), wt.double(), padding=1)
    return gy, mx, wt, _store(g64, dtype).reshape(n, cin, -1)


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("kernel,dtype,case", BWD_CASES, ids=["%s-%s-%s" % (k, str(dt).split(".")[-1], "x".join(map(str, c))) for k, dt, c in BWD_CASES])
def test_backward_data_sums_vs_fp64(kernel, dtype, case, lib_mode):
    """vs_conv_gather_bwd_data (K3) with the fused IN-backward sums of its lazy input, against fp64"""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import check, lib
    n, cin, cout, d, h, w = case
    gy, mx, wt, g_st = _bwd_inputs(case, dtype)
    gy_cl, mx_cl = to_cl(gy, cout, dtype), to_cl(mx, cin, dtype)
    ops.stats_arena_begin(gy_cl.device)
    mxs = ops.instnorm_stats(mx_cl)
    wpb = ops.pack_weight(wt.cuda(), ops.VS_PACK_ROWS_D1_FLIP, cout, ops.k3_pack_dtype(gy_cl))
    y, sums = torch.empty_like(mx_cl), ops._new_stats(n, cin, gy_cl.device)
    check(lib.vs_conv_gather_bwd_data(gy_cl.data_ptr(), wpb.data_ptr(), y.data_ptr(), mx_cl.data_ptr(), mxs.data_ptr(), sums.data_ptr(),
                                      n, d, h, w, cout, cin, ops.VS_CONV_K3, ops.vs_dtype(gy_cl), 1e-5, ops._stream()), "bwd_data")
    torch.cuda.synchronize()
    g = _cl_to_ncv(y, cin)
    _y_check("backward-data", g, g_st, Y_TOL[dtype])
    mm, mr = _kernel_mean_rstd(ops, mxs, d * h * w)
    ref, scale = _bwd_pairs_ref(g, mx.reshape(n, cin, -1), mm, mr)
    _check_bwd_pairs("%s %s %s %s" % (kernel, case, dtype, lib_mode), ops.stats_total(sums).cpu(), ref, scale, BWD_TOL)


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("dtype,case", [(BF, (2, 20, 12, 40)), (BF, (2, 96, 96, 96)), (F32, (2, 20, 12, 40))],
                         ids=["k3t_fa-bfloat16-2x20x12x40", "k3t_fa-bfloat16-2x96cube", "k3xt_fa-float32-2x20x12x40"])
def test_fused_apply_and_reduce_sums_vs_fp64(dtype, case, lib_mode):
    """vs_instnorm_relu_bwd_reduce (the pair of an un-applied gradient against its activation) and vs_conv_k3_bwd_data_fused_apply (the 8 -> 8
    backward-data with the apply pass fused into its staging; the pair of its own lazy input), each against fp64 — the latter on the applied
    gradient the kernel writes out"""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import check, lib
    n, d, h, w = case
    vox = d * h * w
    gen = torch.Generator().manual_seed(d * 7 + h)
    const = torch.tensor([2.0 * (-1) ** c for c in range(8)])
    ax = q(torch.randn(n, 8, d, h, w, generator=gen) * 1.3 + 0.2, dtype)
    gu = q(torch.randn(n, 8, d, h, w, generator=gen) + const[None, :, None, None, None], dtype)      # un-applied dL/da, a constant per channel
    mx = q(torch.randn(n, 8, d, h, w, generator=gen) * 0.8 - 0.1, dtype)
    wt = q(torch.randn(8, 8, 3, 3, 3, generator=gen) * 0.1 + 0.01, dtype)
    ax_cl, gu_cl, mx_cl = to_cl(ax, 8, dtype), to_cl(gu, 8, dtype), to_cl(mx, 8, dtype)
    ops.stats_arena_begin(ax_cl.device)
    axs, mxs = ops.instnorm_stats(ax_cl), ops.instnorm_stats(mx_cl)
    dt, st = ops.vs_dtype(ax_cl), ops._stream()
    asums = ops._new_stats(n, 8, ax_cl.device)
    check(lib.vs_instnorm_relu_bwd_reduce(gu_cl.data_ptr(), ax_cl.data_ptr(), axs.data_ptr(), asums.data_ptr(), n, vox, 8, dt, 1e-5, st), "reduce")
    wpb = ops.pack_weight(wt.cuda(), ops.VS_PACK_ROWS_D1_FLIP, 8, ops.k3_pack_dtype(gu_cl))
    y, s2, dx = torch.empty_like(gu_cl), ops._new_stats(n, 8, ax_cl.device), torch.empty_like(gu_cl)
    check(lib.vs_conv_k3_bwd_data_fused_apply(gu_cl.data_ptr(), ax_cl.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), y.data_ptr(),
                                              mx_cl.data_ptr(), mxs.data_ptr(), s2.data_ptr(), dx.data_ptr(), n, d, h, w, 8, 8, dt, 1e-5, st), "fused")
    torch.cuda.synchronize()
    tag = "%s %s %s" % (case, dtype, lib_mode)
    am, ar = _kernel_mean_rstd(ops, axs, vox)
    ref, scale = _bwd_pairs_ref(gu.double().reshape(n, 8, -1), ax.reshape(n, 8, -1), am, ar)
    _check_bwd_pairs("instnorm_relu_bwd_reduce " + tag, ops.stats_total(asums).cpu(), ref, scale, BWD_TOL)
    dxd = _cl_to_ncv(dx, 8).reshape(n, 8, d, h, w)
    g_st = _store(F.conv_transpose3d(dxd, wt.double(), padding=1), dtype).reshape(n, 8, -1)
    g = _cl_to_ncv(y, 8)
    _y_check("backward-data", g, g_st, Y_TOL[dtype])
    mm, mr = _kernel_mean_rstd(ops, mxs, vox)
    ref, scale = _bwd_pairs_ref(g, mx.reshape(n, 8, -1), mm, mr)
    _check_bwd_pairs("conv_k3_bwd_data_fused_apply " + tag, ops.stats_total(s2).cpu(), ref, scale, BWD_TOL)


# ---- the composed Up head and the chain: the other 3x3x3 forward producers -----------------------------------------------------------------------
def _centre_offset_weights(u, w0, dtype):
    """w0 (zero-mean, cout x c x 3 x 3 x 3) plus mu_w per output channel on the centre tap, solved on the fp64 conv input u so that the output hits
    the R targets; rounded to the storage type"""
    n, cout = u.shape[0], w0.shape[0]
    y0 = F.conv3d(u, q(w0, dtype).double(), padding=1).reshape(n, cout, -1)
    mu = _solve_mu(y0, u.sum(1).reshape(n, -1), _signed_targets(cout))
    wt = w0.double().clone()
    wt[:, :, 1, 1, 1] += mu[:, None]
    return q(wt.float(), dtype)


@_last_call
def _up_fwd_ref(case, dtype):
    """relu-free composed Up head on a stored input: ConvTranspose3d(c, c, 2, 2) + bias -> Conv3d(c, co, 3, pad 1).  The transposed weights are
    1 / c plus a small spread, so every channel of the fine grid carries the input's offset and the 3x3x3 conv's centre tap can reach R ~ 300"""
    n, c, co, d, h, w = case
    g = torch.Generator().manual_seed(c * 17 + co + d)
    x = q(torch.rand(n, c, d, h, w, generator=g) + 0.289 * 700.0 / c ** 0.5, dtype)
    w2 = q((torch.rand(c, c, 2, 2, 2, generator=g) - 0.5) * 0.02 * (3.0 / c) ** 0.5 + 1.0 / c, dtype)
    b2 = (torch.rand(c, generator=g) * 2 - 1) * 0.3
    w30 = (torch.rand(co, c, 3, 3, 3, generator=g) * 2 - 1) * (3.0 / (27 * c)) ** 0.5
    w30 -= w30.mean((1, 2, 3, 4), keepdim=True)
    u = F.conv_transpose3d(x.double(), w2.double(), b2.double(), stride=2)
    w3 = _centre_offset_weights(u, w30, dtype)
    y_st = _store(F.conv3d(u, w3.double(), padding=1), dtype).reshape(n, co, -1)
    return x, w2, b2, w3, y_st


UP_FWD_CASES = [(2, 32, 16, 12, 12, 12), (2, 64, 32, 6, 6, 6)]


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("case", UP_FWD_CASES, ids=["up_compose-bfloat16-%s" % "x".join(map(str, c)) for c in UP_FWD_CASES])
def test_composed_up_stats_per_channel_vs_fp64(case, lib_mode):
    """vs_up_conv_fwd (up_compose.hip): the two layers' weights are composed into one image (rounded to 16 bits once more), so y is held to the
    storage type's parity tolerance (tests/test_gpu_up.py: 2 x 1.5e-2) per channel; the pair is gated against the stored y as everywhere"""
    from vae_segmentation_amd import ops
    n, c, co, d, h, w = case
    x, w2, b2, w3, y_st = _up_fwd_ref(case, BF)
    x_cl = to_cl(x, c, BF)
    ops.stats_arena_begin(x_cl.device)
    with torch.no_grad():
        y, ys = ops.UpConvK3.apply(x_cl, None, w2.cuda(), b2.cuda(), w3.cuda())
    torch.cuda.synchronize()
    _fwd_check("up_compose %s %s" % (case, lib_mode), BF, ops.stats_total(ys).cpu()[:, :co], _cl_to_ncv(y, co), y_st, y_tol=3e-2)


CHAIN_CASES = [(BF, (2, 64, 64, 6, 6, 6)), (BF, (3, 64, 32, 5, 6, 6)), (F32, (2, 128, 128, 4, 4, 4))]


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("dtype,case", CHAIN_CASES, ids=["k3s_chain_fwd-%s-%s" % (str(dt).split(".")[-1], "x".join(map(str, c))) for dt, c in CHAIN_CASES])
def test_chain_forward_stats_per_channel_vs_fp64(dtype, case, lib_mode):
    """vs_conv_k3_chain forward, two layers in one launch: layer 0 on the offset input (its pair handed to layer 1 inside the launch), layer 1 on
    relu(instnorm(layer 0)).  Layer 1's reference applies the normalisation in fp64 while the kernel rounds the activation to the storage type
    while staging: its y is held to the storage type's parity tolerance, its pair (as every pair) to the stored y"""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import check, lib
    n, cin, cout, d, h, w = case
    x, w0, y0_st = _fwd_ref(case, dtype)
    g = torch.Generator().manual_seed(99)
    w1 = q((torch.rand(cout, cout, 3, 3, 3, generator=g) * 2 - 1) * (3.0 / (27 * cout)) ** 0.5 + 0.01, dtype)
    x_cl = to_cl(x, cin, dtype)
    assert lib.vs_conv_k3_chain_supported(n, d, h, w, max(cin, cout), ops.vs_dtype(x_cl)) == 1
    ops.stats_arena_begin(x_cl.device)
    dev = x_cl.device
    wp0 = ops.pack_weight(w0.cuda(), ops.VS_PACK_ROWS_D0, cin, ops.k3_pack_dtype(x_cl))
    wp1 = ops.pack_weight(w1.cuda(), ops.VS_PACK_ROWS_D0, cout, ops.k3_pack_dtype(x_cl))
    y0, y1 = torch.empty((n, d, h, w, cout), dtype=dtype, device=dev), torch.empty((n, d, h, w, cout), dtype=dtype, device=dev)
    s0, s1 = ops._new_stats(n, cout, dev), ops._new_stats(n, cout, dev)
    layers = (ops.ChainLayer * 2)()
    layers[0] = ops.ChainLayer(x_cl.data_ptr(), None, wp0.data_ptr(), y0.data_ptr(), s0.data_ptr(), None, None, None, cin, cout, 0, 0)
    layers[1] = ops.ChainLayer(y0.data_ptr(), s0.data_ptr(), wp1.data_ptr(), y1.data_ptr(), s1.data_ptr(), None, None, None, cout, cout, 0, 0)
    sync = ops._chain_sync(n, dev)
    check(lib.vs_conv_k3_chain(ctypes.addressof(layers), 2, 0, None, sync.data_ptr(), ops._chain_fault_word(dev).data_ptr(), n, d, h, w,
                               ops.vs_dtype(x_cl), 1e-5, ops._stream()), "chain forward")
    torch.cuda.synchronize()
    tag = "chain %s %s %s" % (case, dtype, lib_mode)
    _fwd_check(tag + " layer 0", dtype, ops.stats_total(s0).cpu(), _cl_to_ncv(y0, cout), y0_st)
    y0_own = _cl_to_ncv(y0, cout)
    m, r = SU.pair_mean_rstd(ops.stats_total(s0).cpu(), d * h * w)
    act = _store(torch.relu((y0_own - m[..., None]) * r[..., None]), dtype).reshape(n, cout, d, h, w)
    y1_st = _store(F.conv3d(act, w1.double(), padding=1), dtype).reshape(n, cout, -1)
    _fwd_check(tag + " layer 1", dtype, ops.stats_total(s1).cpu(), _cl_to_ncv(y1, cout), y1_st, y_tol=1.5e-2 if dtype == BF else 2e-5, targets=False)


# ---- backward pairs of the stride-2 launches, the epilogue-apply launches and the chain's backward bodies -------------------------------------------
def _bwd_mask_inputs(n, c, s, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return q(torch.randn(n, c, s, s, s, generator=g) * 0.8 - 0.1, dtype)


def _offset_grad(n, c, s, dtype, seed):
    """an output gradient with a constant component per channel (as Dice's k1 t - k2 adds to every voxel)"""
    g = torch.Generator().manual_seed(seed)
    return q(torch.randn(n, c, s, s, s, generator=g) + torch.tensor([3.0 * (-1) ** k for k in range(c)])[None, :, None, None, None], dtype)


# (kernel, mode, epilogue apply, (N, C, side of the gradient's grid)); scatter: backward-data of Conv3d(C, C, 2, 2) (coarse -> fine),
# gather: backward-data of ConvTranspose3d(C, C, 2, 2) (fine -> coarse)
S2_CASES = [("g1_scatter", "scatter", False, (2, 16, 12)), ("k2s2_scatter8", "scatter", False, (2, 8, 48)), ("g1_gather", "gather", False, (2, 32, 24)),
            ("g1_scatter_ea", "scatter", True, (2, 32, 12)), ("g1_gather_ea", "gather", True, (2, 32, 24))]


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("kernel,mode,ea,case", S2_CASES, ids=["%s-bfloat16-%s" % (k, "x".join(map(str, c))) for k, _, _, c in S2_CASES])
def test_stride2_backward_data_sums_vs_fp64(kernel, mode, ea, case, lib_mode):
    """vs_conv_scatter_bwd_data / vs_conv_gather_bwd_data (K2S2) with the fused IN-backward sums, and their epilogue-apply forms
    (vs_conv_s2_bwd_data_applied: the sums, then the apply pass, in one launch) — whose un-applied gradient is never stored: their pair is
    compared with the fp64 sums of the gradient the plain launch stores from the same operands"""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import check, lib
    n, c, s = case
    dtype = BF
    so = 2 * s if mode == "scatter" else s // 2
    gy = _offset_grad(n, c, s, dtype, seed=c + s)
    mx = _bwd_mask_inputs(n, c, so, dtype, seed=c * 3 + s)
    g = torch.Generator().manual_seed(c * 5 + s)
    wt = q((torch.rand(c, c, 2, 2, 2, generator=g) * 2 - 1) * (3.0 / (8 * c)) ** 0.5 + 0.02, dtype)
    if mode == "scatter":
        g_st = _store(F.conv_transpose3d(gy.double(), wt.double(), stride=2), dtype).reshape(n, c, -1)
    else:
        g_st = _store(F.conv3d(gy.double(), wt.double(), stride=2), dtype).reshape(n, c, -1)
    gy_cl, mx_cl = to_cl(gy, c, dtype), to_cl(mx, c, dtype)
    dev, dt, st = gy_cl.device, ops.vs_dtype(gy_cl), ops._stream()
    ops.stats_arena_begin(dev)
    mxs = ops.instnorm_stats(mx_cl)
    wpb = ops.pack_weight(wt.cuda(), ops.VS_PACK_SCATTER_D1 if mode == "scatter" else ops.VS_PACK_ROWS_D0, c, dtype)
    y, sums = torch.empty_like(mx_cl), ops._new_stats(n, c, dev)
    if mode == "scatter":
        check(lib.vs_conv_scatter_bwd_data(gy_cl.data_ptr(), wpb.data_ptr(), y.data_ptr(), mx_cl.data_ptr(), mxs.data_ptr(), sums.data_ptr(),
                                           n, s, s, s, c, c, dt, 1e-5, st), "scatter_bwd_data")
    else:
        check(lib.vs_conv_gather_bwd_data(gy_cl.data_ptr(), wpb.data_ptr(), y.data_ptr(), mx_cl.data_ptr(), mxs.data_ptr(), sums.data_ptr(),
                                          n, s, s, s, c, c, ops.VS_CONV_K2S2, dt, 1e-5, st), "gather_bwd_data (K2S2)")
    if ea:
        assert lib.vs_conv_s2_bwd_data_applied_supported(n, s, s, s, c, c, 1 if mode == "scatter" else 0, dt) == 1
        ya, sums_ea = torch.empty_like(mx_cl), ops._new_stats(n, c, dev)
        check(lib.vs_conv_s2_bwd_data_applied(gy_cl.data_ptr(), wpb.data_ptr(), ya.data_ptr(), mx_cl.data_ptr(), mxs.data_ptr(), sums_ea.data_ptr(), None,
                                              ops._ea_sync(n, dev).data_ptr(), ops._chain_fault_word(dev).data_ptr(), n, s, s, s, c, c,
                                              1 if mode == "scatter" else 0, dt, 1e-5, st), "s2_bwd_data_applied")
    torch.cuda.synchronize()
    g_own = _cl_to_ncv(y, c)
    _y_check(kernel, g_own, g_st, Y_TOL[dtype])
    mm, mr = _kernel_mean_rstd(ops, mxs, so ** 3)
    ref, scale = _bwd_pairs_ref(g_own, mx.reshape(n, c, -1), mm, mr)
    tag = "%s %s %s" % (kernel, case, lib_mode)
    _check_bwd_pairs(tag, ops.stats_total(sums if not ea else sums_ea).cpu(), ref, scale, BWD_TOL)


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("case", [(2, 32, 32, 24, 24, 24), (2, 64, 32, 12, 12, 12)], ids=["k3b_ea-bfloat16-2x32x32x24cube", "k3b_ea-bfloat16-2x64x32x12cube"])
def test_k3b_epilogue_apply_sums_vs_fp64(case, lib_mode):
    """vs_conv_k3_bwd_data_applied (igemm_k3b.h EA): backward-data + IN-backward sums + apply in one launch; its pair against the fp64 sums of the
    gradient the plain backward-data launch stores from the same operands (that gradient against fp64 too)"""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import check, lib
    n, cin, cout, d, h, w = case
    dtype = BF
    gy, mx, wt, g_st = _bwd_inputs(case, dtype)
    gy_cl, mx_cl = to_cl(gy, cout, dtype), to_cl(mx, cin, dtype)
    dev, dt, st = gy_cl.device, ops.vs_dtype(gy_cl), ops._stream()
    assert lib.vs_conv_k3_bwd_data_applied_supported(n, d, h, w, cout, cin, dt) == 1
    ops.stats_arena_begin(dev)
    mxs = ops.instnorm_stats(mx_cl)
    wpb = ops.pack_weight(wt.cuda(), ops.VS_PACK_ROWS_D1_FLIP, cout, ops.k3_pack_dtype(gy_cl))
    y, sums = torch.empty_like(mx_cl), ops._new_stats(n, cin, dev)
    check(lib.vs_conv_gather_bwd_data(gy_cl.data_ptr(), wpb.data_ptr(), y.data_ptr(), mx_cl.data_ptr(), mxs.data_ptr(), sums.data_ptr(),
                                      n, d, h, w, cout, cin, ops.VS_CONV_K3, dt, 1e-5, st), "bwd_data")
    ya, sums_ea = torch.empty_like(mx_cl), ops._new_stats(n, cin, dev)
    check(lib.vs_conv_k3_bwd_data_applied(gy_cl.data_ptr(), wpb.data_ptr(), ya.data_ptr(), mx_cl.data_ptr(), mxs.data_ptr(), sums_ea.data_ptr(),
                                          ops._ea_sync(n, dev).data_ptr(), ops._chain_fault_word(dev).data_ptr(), n, d, h, w, cout, cin, dt, 1e-5, st),
          "k3_bwd_data_applied")
    torch.cuda.synchronize()
    g_own = _cl_to_ncv(y, cin)
    _y_check("k3b bwd-data", g_own, g_st, Y_TOL[dtype])
    mm, mr = _kernel_mean_rstd(ops, mxs, d * h * w)
    ref, scale = _bwd_pairs_ref(g_own, mx.reshape(n, cin, -1), mm, mr)
    _check_bwd_pairs("k3b_ea %s %s" % (case, lib_mode), ops.stats_total(sums_ea).cpu(), ref, scale, BWD_TOL)


CHAIN_BWD_CASES = [(BF, (2, 64, 64, 6, 6, 6)), (F32, (2, 128, 128, 4, 4, 4))]


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("dtype,case", CHAIN_BWD_CASES, ids=["k3s_chain_bwd-%s-%s" % (str(dt).split(".")[-1], "x".join(map(str, c))) for dt, c in CHAIN_BWD_CASES])
def test_chain_backward_sums_vs_fp64(dtype, case, lib_mode):
    """vs_conv_k3_chain backward, two bodies in one launch: body 0 = backward-data of the block's second conv with the sums against the middle
    activation and the apply in place; body 1 = backward-data of the first conv on that applied gradient, with the sums against the block's lazy
    input, its gradient stored un-applied.  Body 1's pair against the fp64 sums of its own stored gradient (which is checked against fp64 of the
    applied gradient body 0 left); body 0's un-applied gradient is never stored, so its pair is compared with the fp64 sums of the fp64
    backward-data (fp32 storage only: in 16 bits a value on a rounding edge moves a 216-voxel sum by an ulp)"""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd._lib import check, lib
    n, c, _, d, h, w = case
    gy = _offset_grad(n, c, d, dtype, seed=7)
    ax0, ax1 = _bwd_mask_inputs(n, c, d, dtype, seed=8), _bwd_mask_inputs(n, c, d, dtype, seed=9)      # block input (raw), middle activation (raw)
    g = torch.Generator().manual_seed(10)
    w0, w1 = [q((torch.rand(c, c, 3, 3, 3, generator=g) * 2 - 1) * (3.0 / (27 * c)) ** 0.5 + 0.005, dtype) for _ in range(2)]
    gy_cl, ax0_cl, ax1_cl = to_cl(gy, c, dtype), to_cl(ax0, c, dtype), to_cl(ax1, c, dtype)
    dev, dt = gy_cl.device, ops.vs_dtype(gy_cl)
    assert lib.vs_conv_k3_chain_supported(n, d, h, w, c, dt) == 1
    ops.stats_arena_begin(dev)
    xs0, xs1 = ops.instnorm_stats(ax0_cl), ops.instnorm_stats(ax1_cl)
    wb1 = ops.pack_weight(w1.cuda(), ops.VS_PACK_ROWS_D1_FLIP, c, ops.k3_pack_dtype(gy_cl))
    wb0 = ops.pack_weight(w0.cuda(), ops.VS_PACK_ROWS_D1_FLIP, c, ops.k3_pack_dtype(gy_cl))
    gm, gi = torch.empty_like(gy_cl), torch.empty_like(gy_cl)
    sm, si = ops._new_stats(n, c, dev), ops._new_stats(n, c, dev)
    layers = (ops.ChainLayer * 2)()
    layers[0] = ops.ChainLayer(gy_cl.data_ptr(), None, wb1.data_ptr(), gm.data_ptr(), None, ax1_cl.data_ptr(), xs1.data_ptr(), sm.data_ptr(), c, c, 1, 0)
    layers[1] = ops.ChainLayer(gm.data_ptr(), None, wb0.data_ptr(), gi.data_ptr(), None, ax0_cl.data_ptr(), xs0.data_ptr(), si.data_ptr(), c, c, 0, 0)
    check(lib.vs_conv_k3_chain(ctypes.addressof(layers), 2, 1, None, ops._chain_sync(n, dev).data_ptr(), ops._chain_fault_word(dev).data_ptr(),
                               n, d, h, w, dt, 1e-5, ops._stream()), "chain backward")
    torch.cuda.synchronize()
    tag = "chain bwd %s %s %s" % (case, dtype, lib_mode)
    vox = d * h * w
    gm_applied = _cl_to_ncv(gm, c).reshape(n, c, d, h, w)
    g_st = _store(F.conv_transpose3d(gm_applied, w0.double(), padding=1), dtype).reshape(n, c, -1)
    g_own = _cl_to_ncv(gi, c)
    _y_check(tag + " body 1", g_own, g_st, Y_TOL[dtype])
    mm, mr = _kernel_mean_rstd(ops, xs0, vox)
    ref, scale = _bwd_pairs_ref(g_own, ax0.reshape(n, c, -1), mm, mr)
    _check_bwd_pairs(tag + " body 1", ops.stats_total(si).cpu(), ref, scale, BWD_TOL)
    if dtype == F32:
        g1 = F.conv_transpose3d(gy.double(), w1.double(), padding=1).reshape(n, c, -1)
        mm, mr = _kernel_mean_rstd(ops, xs1, vox)
        ref, scale = _bwd_pairs_ref(g1, ax1.reshape(n, c, -1), mm, mr)
        _check_bwd_pairs(tag + " body 0", ops.stats_total(sm).cpu(), ref, scale, BWD_TOL)
