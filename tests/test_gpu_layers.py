"""GPU parity at the REAL layer shapes of BASELINE configs[1] (96^3, B=2) and configs[3] (128^3, B=1): every distinct 3x3x3, stride-2 and
transposed convolution of Segmentation / VAE (joint_model.py:204-226,349-367), forward + backward-data (with the fused
InstanceNorm+ReLU-backward sums and the apply pass) + weight / bias gradient, lazy (InstanceNorm+ReLU-on-load) input, against
F.conv3d / F.conv_transpose3d autograd in fp32 on the CPU — the same tolerances as the small-shape tests in test_gpu_ops.py
(fp32 kernels 2e-5, x4 for quantities behind the lazy input; bf16 1.5e-2, fp16 2e-3, x4).

The model-level goldens at 96^3 / 128^3 bound gradients only loosely (the reference's own fp32 gradients sit 1e-2..1e-1 from fp64
there, tests/golden_util.py); this file is what pins the backward kernels at the sizes the benchmark runs."""
import pytest
import torch
import torch.nn.functional as F

from tests import stats_util as SU
from tests.test_gpu_ops import TOL, from_cl, in_relu, q, relerr, rnd, to_cl

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]

# (N, Cin, Cout, side) — configs[1]: B=2 at 96^3; configs[3]: B=1 at 128^3 (levels 128, 64; the deeper levels of 128^3 are the 96^3
# shapes with other sides, covered by the ragged cases of test_gpu_ops.py)
K3_LAYERS = [
    (2, 1, 8, 96), (2, 2, 8, 96), (2, 8, 8, 96), (2, 16, 8, 96),                      # in_block (Seg / VAE), up5
    (2, 8, 16, 48), (2, 16, 16, 48), (2, 32, 16, 48),                                 # down1, up4
    (2, 16, 32, 24), (2, 32, 32, 24), (2, 64, 32, 24),                                # down2, up3
    (2, 32, 64, 12), (2, 64, 64, 12), (2, 128, 64, 12),                               # down3, up2
    (2, 64, 128, 6), (2, 128, 128, 6), (2, 256, 128, 6),                              # down4, up1 (VAE)
    (2, 128, 256, 3), (2, 256, 256, 3),                                               # down5 (VAE)
    (1, 8, 8, 128), (1, 16, 8, 128), (1, 16, 16, 64), (1, 32, 16, 64), (1, 32, 32, 32), (1, 128, 128, 8), (1, 256, 256, 4),
]
K2_LAYERS = [(2, 8, 96), (2, 16, 48), (2, 32, 24), (2, 64, 12), (2, 128, 6), (1, 8, 128), (1, 16, 64)]           # Down: Conv3d(C, C, 2, stride 2)
T2_LAYERS = [(2, 16, 48), (2, 32, 24), (2, 64, 12), (2, 128, 6), (2, 256, 3), (1, 16, 64), (1, 32, 32)]          # Up: ConvTranspose3d(C, C, 2, stride 2), input side


def _ops():
    from vae_segmentation_amd import ops
    return ops


def _last_call(fn):
    """One-slot memo for the CPU references: the two `lib_mode` runs of a case (tests/conftest.py; innermost parameter, so they are
    neighbours) share one F.conv3d autograd pass instead of paying for it twice.  One slot: a 96^3 reference is hundreds of MB."""
    slot = {}

    def wrapped(*key):
        if slot.get("key") != key:
            slot.clear()
            slot["val"] = fn(*key)
            slot["key"] = key
        return slot["val"]
    return wrapped


def _report(tag, errs, lims):
    bad = {k: (errs[k], lims[k]) for k in errs if not errs[k] < lims[k]}
    print("\n%s: %s" % (tag, ", ".join("%s %.2e (<%.1e)" % (k, errs[k], lims[k]) for k in errs)))
    assert not bad, "%s: %s" % (tag, bad)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", K3_LAYERS)
def test_k3_layer_shapes(case, dtype):
    _k3_case(case, dtype)


# BASELINE configs[4]: 160^3, batch 2 per GPU, fp16 storage (and the fp32 parity mode): the levels 160 / 80 / 40 / 20 / 10 / 5 — the odd side 5
# and the largest tensors the 32-bit byte offsets of the 16-bit kernels must hold (2 x 160^3 x 16 channels x 2 B = 262 MB) included
K3_LAYERS_160 = [(2, 1, 8, 160), (2, 8, 8, 160), (2, 16, 8, 160), (2, 8, 16, 80), (2, 16, 16, 80), (2, 32, 16, 80), (2, 16, 32, 40), (2, 32, 32, 40),
                 (2, 64, 32, 40), (2, 64, 64, 20), (2, 128, 64, 20), (2, 128, 128, 10), (2, 256, 128, 10), (2, 128, 256, 5), (2, 256, 256, 5)]
K2_LAYERS_160 = [(2, 8, 160), (2, 16, 80), (2, 32, 40), (2, 64, 20), (2, 128, 10)]
T2_LAYERS_160 = [(2, 16, 80), (2, 32, 40), (2, 64, 20), (2, 128, 10), (2, 256, 5)]
DT160 = [torch.float32, torch.float16]


@pytest.mark.parametrize("dtype", DT160)
@pytest.mark.parametrize("case", K3_LAYERS_160)
def test_k3_layer_shapes_160(case, dtype):
    _k3_case(case, dtype)


@pytest.mark.parametrize("dtype", DT160)
@pytest.mark.parametrize("case", K2_LAYERS_160)
def test_k2s2_layer_shapes_160(case, dtype):
    test_k2s2_layer_shapes(case, dtype)


@pytest.mark.parametrize("dtype", DT160)
@pytest.mark.parametrize("case", T2_LAYERS_160)
def test_transposed_layer_shapes_160(case, dtype):
    test_transposed_layer_shapes(case, dtype)


@_last_call
def _k3_ref(case, dtype):
    n, cin, cout, s = case
    x = rnd(n, cin, s, s, s, seed=1)
    wt = rnd(cout, cin, 3, 3, 3, seed=2, scale=(3.0 / (27 * cin)) ** 0.5)
    gy = rnd(n, cout, s, s, s, seed=3)
    xq, wq, gq = q(x, dtype).requires_grad_(True), q(wt, dtype).requires_grad_(True), q(gy, dtype)
    y_ref = F.conv3d(in_relu(xq), wq, None, padding=1)
    (y_ref * gq).sum().backward()
    return x, wt, gy, xq, wq, y_ref.detach()


def _k3_case(case, dtype):
    ops = _ops()
    n, cin, cout, s = case
    x, wt, gy, xq, wq, y_ref = _k3_ref(case, dtype)

    x_cl = to_cl(x, ops.cpad(cin), dtype).requires_grad_(True)
    xs = ops.instnorm_stats(x_cl.detach())
    w_gpu = q(wt, dtype).cuda().requires_grad_(True)
    ops.stats_arena_begin(x_cl.device)
    y, ys = ops.ConvK3.apply(x_cl, xs, w_gpu, None)
    y.backward(to_cl(gy, ops.cpad(cout), dtype))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    yr = q(y_ref.detach(), dtype).double()
    st = ops.stats_total(ys).cpu()[:, :cout]
    ref_sum, ref_sq = yr.sum((2, 3, 4)), (yr * yr).sum((2, 3, 4))
    errs = {"y": relerr(from_cl(y, cout), y_ref.detach()),
            "stat_sum": float((st[..., 0] - ref_sum).abs().max() / ref_sq.sqrt().max()),
            "stat_sq": float((st[..., 1] - ref_sq).abs().max() / ref_sq.max()),
            "gx": relerr(from_cl(x_cl.grad, cin), xq.grad), "gw": relerr(w_gpu.grad.cpu(), wq.grad)}
    # the channel sum is a near-cancelling sum: its rounding noise grows like sqrt(voxels) against the sqrt(sum of squares) scale used above
    # (tests/test_gpu_ops.py, CONV_CASES_LARGE) — the 160^3 cases get the corresponding factor over the 96^3 ones
    grow = max(1.0, (s / 96.0) ** 1.5)
    lims = {"y": tol, "stat_sum": 4 * tol * grow, "stat_sq": 4 * tol, "gx": 4 * tol, "gw": 4 * tol}
    _report("k3 %s %s" % (case, dtype), errs, lims)
    # per (n, c): mean / rstd against each channel's own fp64 two-pass statistics (tests/stats_util.py); lazy input, so the storage type's tolerance
    SU.check_stats(st, SU.two_pass(yr), "k3 %s %s" % (case, dtype), mean_tol=4 * tol * grow, rstd_tol=4 * tol, sum_tol=4 * tol * grow, rstd_tol_high=4 * tol, rstd_grows_with_r=True)


@_last_call
def _k2s2_ref(case, dtype):
    n, c, s = case
    x = rnd(n, c, s, s, s, seed=4)
    wt = rnd(c, c, 2, 2, 2, seed=5, scale=(3.0 / (8 * c)) ** 0.5)
    b = rnd(c, seed=6, scale=0.1)
    gy = rnd(n, c, s // 2, s // 2, s // 2, seed=7)
    xq, wq, bq, gq = q(x, dtype).requires_grad_(True), q(wt, dtype).requires_grad_(True), b.clone().requires_grad_(True), q(gy, dtype)
    y_ref = F.conv3d(in_relu(xq), wq, bq, stride=2)
    (y_ref * gq).sum().backward()
    return x, wt, b, gy, xq, wq, bq, y_ref.detach()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", K2_LAYERS)
def test_k2s2_layer_shapes(case, dtype):
    ops = _ops()
    n, c, s = case
    x, wt, b, gy, xq, wq, bq, y_ref = _k2s2_ref(case, dtype)
    x_cl = to_cl(x, c, dtype).requires_grad_(True)
    xs = ops.instnorm_stats(x_cl.detach())
    w_gpu, b_gpu = q(wt, dtype).cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ops.stats_arena_begin(x_cl.device)
    y = ops.ConvK2S2.apply(x_cl, xs, w_gpu, b_gpu)
    y.backward(to_cl(gy, c, dtype))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    errs = {"y": relerr(from_cl(y, c), y_ref.detach()), "gx": relerr(from_cl(x_cl.grad, c), xq.grad),
            "gw": relerr(w_gpu.grad.cpu(), wq.grad), "gb": relerr(b_gpu.grad.cpu(), bq.grad)}
    _report("k2s2 %s %s" % (case, dtype), errs, {"y": tol, "gx": 4 * tol, "gw": 4 * tol, "gb": 4 * tol})


@_last_call
def _t2_ref(case, dtype):
    n, c, s = case
    x = rnd(n, c, s, s, s, seed=8)
    wt = rnd(c, c, 2, 2, 2, seed=9, scale=(3.0 / c) ** 0.5)
    b = rnd(c, seed=10, scale=0.1)
    gy = rnd(n, c, 2 * s, 2 * s, 2 * s, seed=11)
    xq, wq, bq, gq = q(x, dtype).requires_grad_(True), q(wt, dtype).requires_grad_(True), b.clone().requires_grad_(True), q(gy, dtype)
    y_ref = F.conv_transpose3d(in_relu(xq), wq, bq, stride=2)
    (y_ref * gq).sum().backward()
    return x, wt, b, gy, xq, wq, bq, y_ref.detach()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", T2_LAYERS)
def test_transposed_layer_shapes(case, dtype):
    ops = _ops()
    n, c, s = case
    x, wt, b, gy, xq, wq, bq, y_ref = _t2_ref(case, dtype)
    x_cl = to_cl(x, c, dtype).requires_grad_(True)
    xs = ops.instnorm_stats(x_cl.detach())
    w_gpu, b_gpu = q(wt, dtype).cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ops.stats_arena_begin(x_cl.device)
    y = ops.ConvT2S2.apply(x_cl, xs, w_gpu, b_gpu)
    y.backward(to_cl(gy, c, dtype))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    errs = {"y": relerr(from_cl(y, c), y_ref.detach()), "gx": relerr(from_cl(x_cl.grad, c), xq.grad),
            "gw": relerr(w_gpu.grad.cpu(), wq.grad), "gb": relerr(b_gpu.grad.cpu(), bq.grad)}
    _report("convT %s %s" % (case, dtype), errs, {"y": tol, "gx": 4 * tol, "gw": 4 * tol, "gb": 4 * tol})


@_last_call
def _out_block_ref(case, dtype):
    n, s = case
    x = rnd(n, 8, s, s, s, seed=12)
    wt = rnd(2, 8, 3, 3, 3, seed=13, scale=0.3)
    b = rnd(2, seed=14, scale=0.2)
    gp = rnd(n, 2, s, s, s, seed=15)
    xq, wq, bq = q(x, dtype).requires_grad_(True), q(wt, dtype).requires_grad_(True), b.clone().requires_grad_(True)
    p_ref = torch.softmax(F.conv3d(in_relu(xq), wq, bq, padding=1), dim=1)
    (p_ref * gp).sum().backward()
    return x, wt, b, gp, xq, wq, bq, p_ref.detach()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", [(2, 96), (1, 128)])
def test_out_block_softmax_layer_shapes(case, dtype):
    """out_block (8 -> 2, live bias) + Softmax at full resolution, with the backward through the softmax, the fused IN-backward sums and
    the weight / bias gradients (joint_model.py:366-367,386-388)."""
    ops = _ops()
    n, s = case
    x, wt, b, gp, xq, wq, bq, p_ref = _out_block_ref(case, dtype)
    x_cl = to_cl(x, 8, dtype).requires_grad_(True)
    xs = ops.instnorm_stats(x_cl.detach())
    w_gpu, b_gpu = q(wt, dtype).cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ops.stats_arena_begin(x_cl.device)
    p = ops.ConvK3Softmax.apply(x_cl, xs, w_gpu, b_gpu)
    p.backward(gp.cuda())
    torch.cuda.synchronize()
    tol = TOL[dtype]
    errs = {"p": relerr(p.cpu(), p_ref.detach()), "gx": relerr(from_cl(x_cl.grad, 8), xq.grad),
            "gw": relerr(w_gpu.grad.cpu(), wq.grad), "gb": relerr(b_gpu.grad.cpu(), bq.grad)}
    _report("out_block %s %s" % (case, dtype), errs, {"p": tol, "gx": 4 * tol, "gw": 4 * tol, "gb": 4 * tol})


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", [(2, 16, 48), (2, 32, 24), (1, 16, 64)])
def test_skip_merge_layer_shapes(case, dtype):
    """The additive U-Net skips at up3 / up4 (joint_model.py:380,382) at their real sizes: relu(IN(a)) + relu(IN(b)) and its pair backward."""
    ops = _ops()
    n, c, s = case
    x1, x2 = rnd(n, c, s, s, s, seed=16), rnd(n, c, s, s, s, seed=17) * 2 + 0.3
    g = rnd(n, c, s, s, s, seed=18)
    # fp64 reference: this op is elementwise behind two reductions, and in fp32 on the CPU a voxel whose normalised value is within
    # rounding of 0 lands on the other side of the ReLU (measured at (1, 16, 64): ONE element of 4 M, off by its whole gradient)
    a1, a2 = q(x1, dtype).double().requires_grad_(True), q(x2, dtype).double().requires_grad_(True)
    ref = in_relu(a1) + in_relu(a2)
    (ref * q(g, dtype).double()).sum().backward()
    c1, c2 = to_cl(x1, c, dtype).requires_grad_(True), to_cl(x2, c, dtype).requires_grad_(True)
    ops.stats_arena_begin(c1.device)
    out = ops.Materialize.apply(c1, ops.instnorm_stats(c1.detach()), c2, ops.instnorm_stats(c2.detach()))
    out.backward(to_cl(g, c, dtype))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    errs = {"out": relerr(from_cl(out, c).double(), ref.detach()), "g1": relerr(from_cl(c1.grad, c).double(), a1.grad),
            "g2": relerr(from_cl(c2.grad, c).double(), a2.grad)}
    _report("skip %s %s" % (case, dtype), errs, {"out": tol, "g1": 2 * tol, "g2": 2 * tol})


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _dx_agrees(dx, dx_ref, ulp):
    """The applied gradient written by a fused kernel vs the standalone apply pass: every element within an ulp of the storage type and
    almost all identical — except elements whose activation sits exactly on the ReLU edge (xhat == 0 to fp32 rounding: seen at 3^3, where a
    27-voxel mean can equal a bf16 value), where x*rstd - mean*rstd (the fused kernels, and the forward's normalise-on-load) and (x - mean)*rstd
    (the standalone pass) may land on different sides of 0; at most a handful per tensor.  -> number of such edge elements"""
    a, b = dx.float(), dx_ref.float()
    # fp32 storage: nothing rounds the result to a coarser grid, so the cancellation in rstd * (g mask - m1 - xhat m2) (terms of order 1) shows as an ABSOLUTE
    # difference of a few 1e-7 whatever the element's size — measured against the terms' scale there; 16-bit storage: against the element (one storage ulp)
    off = ((a - b).abs() / b.abs().clamp_min(1.0 if dx.dtype == torch.float32 else 1e-3)) > 2.1 * ulp
    n_off = int(off.sum())
    assert n_off <= max(2, int(2e-6 * a.numel())), "%d elements differ by more than an ulp" % n_off
    if dx.dtype != torch.float32:               # 16-bit storage: the one rounding to the storage type hides the fma association; fp32 shows it in the last bit
        assert float((a != b).float().mean()) < 0.02
    return n_off


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("case", [(2, 96, 96, 96), (1, 128, 128, 128), (2, 20, 12, 40), (3, 5, 9, 33), (1, 4, 8, 32)])
@pytest.mark.parametrize("want_dx", [True, False])
def test_k3_bwd_data_with_fused_apply(case, dtype, want_dx):
    """vs_conv_k3_bwd_data_fused_apply (the 8 -> 8 full-resolution layers: apply pass of the incoming gradient fused into the staging of the
    backward-data kernel) against the two launches it replaces — vs_instnorm_relu_bwd_apply, then vs_conv_gather_bwd_data — on the same
    operands: the applied gradient it writes out, the gradient it produces and the IN-backward sums it accumulates.  Both forms do the apply
    in fp32 and round once to the storage type; they differ in the association of one fma, i.e. by at most an ulp of the storage type
    on isolated elements of dx."""
    ops = _ops()
    from vae_segmentation_amd._lib import check, lib
    n, d, h, w = case
    dev = "cuda"
    gen = torch.Generator().manual_seed(d * 7 + h)
    ax = (torch.randn(n, d, h, w, 8, generator=gen) * 1.3 + 0.2).to(dtype).to(dev)           # raw output of this conv = the lazy activation
    g = torch.randn(n, d, h, w, 8, generator=gen).to(dtype).to(dev)                           # un-applied gradient dL/da
    mx = (torch.randn(n, d, h, w, 8, generator=gen) * 0.8 - 0.1).to(dtype).to(dev)            # the conv's own (lazy) input
    wt = (torch.randn(8, 8, 3, 3, 3, generator=gen) * 0.1).to(dev)
    ops.stats_arena_begin(ax.device)
    axs, mxs = ops.instnorm_stats(ax), ops.instnorm_stats(mx)
    vox, dt, st = d * h * w, ops.vs_dtype(ax), ops._stream()
    asums = ops._new_stats(n, 8, ax.device)
    check(lib.vs_instnorm_relu_bwd_reduce(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), n, vox, 8, dt, 1e-5, st), "reduce")
    wpb = ops.pack_weight(wt, ops.VS_PACK_ROWS_D1_FLIP, 8, ops.k3_pack_dtype(g))      # fp32 (parity mode, round 5: k3xt_kernel<..., FA>): the three-limb image
    # reference: standalone apply, then backward-data with fused sums
    dx_ref = torch.empty_like(g)
    check(lib.vs_instnorm_relu_bwd_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), dx_ref.data_ptr(), n, vox, 8, dt, 1e-5, st), "apply")
    y_ref, s_ref = torch.empty_like(g), ops._new_stats(n, 8, ax.device)
    check(lib.vs_conv_gather_bwd_data(dx_ref.data_ptr(), wpb.data_ptr(), y_ref.data_ptr(), mx.data_ptr(), mxs.data_ptr(), s_ref.data_ptr(),
                                      n, d, h, w, 8, 8, ops.VS_CONV_K3, dt, 1e-5, st), "bwd_data")
    # fused
    y, s2 = torch.empty_like(g), ops._new_stats(n, 8, ax.device)
    dx = torch.full_like(g, 7.0) if want_dx else None
    check(lib.vs_conv_k3_bwd_data_fused_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), y.data_ptr(),
                                              mx.data_ptr(), mxs.data_ptr(), s2.data_ptr(), None if dx is None else dx.data_ptr(),
                                              n, d, h, w, 8, 8, dt, 1e-5, st), "fused")
    torch.cuda.synchronize()
    ulp = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -21}[dtype]
    edge = 0
    if want_dx:
        edge = _dx_agrees(dx, dx_ref, ulp)
    assert _rel_l2(y, y_ref) < 4 * ulp and (edge or relerr(y.float().cpu(), y_ref.float().cpu()) < 4 * ulp)
    t2, tr = ops.stats_total(s2), ops.stats_total(s_ref)
    assert float((t2 - tr).abs().max() / tr.abs().max()) < (4 * ulp if not edge else 0.05)
    # the same with a stored (non-lazy) conv input: no mask tensor, no sums (VAE.in_block on the prediction)
    y_ref2 = torch.empty_like(g)
    check(lib.vs_conv_gather_fwd(dx_ref.data_ptr(), None, wpb.data_ptr(), None, y_ref2.data_ptr(), None, n, d, h, w, 8, 8, ops.VS_CONV_K3, dt, 1e-5, st), "plain")
    y3 = torch.empty_like(g)
    check(lib.vs_conv_k3_bwd_data_fused_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), y3.data_ptr(),
                                              None, None, None, None, n, d, h, w, 8, 8, dt, 1e-5, st), "fused, no sums")
    torch.cuda.synchronize()
    assert _rel_l2(y3, y_ref2) < 4 * ulp
    # shapes without a fused-apply kernel are refused (VS_ESHAPE) before anything is launched, not mis-computed: 256 channels (the per-(n,c) tables of the
    # fused kernels hold at most 192 pairs) — the planning query says the same
    assert lib.vs_conv_k3_fused_apply_supported(n, d, h, w, 256, 256, 1, dt) == 0
    assert lib.vs_conv_k3_bwd_data_fused_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), y.data_ptr(),
                                               mx.data_ptr(), mxs.data_ptr(), s2.data_ptr(), None, n, d, h, w, 256, 256, dt, 1e-5, st) == -2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("case", [(2, 48, 16, 16, True), (2, 48, 16, 16, False), (2, 48, 16, 8, False), (2, 48, 16, 32, False), (2, 96, 8, 16, False), (1, 64, 16, 16, True),
                                  (2, 80, 16, 16, True), (1, 20, 16, 16, True), (3, 12, 8, 16, False), (2, 24, 16, 32, False)])
def test_k3b_bwd_data_with_fused_apply(case, dtype):
    """the same comparison for the k3b_kernel FA instantiations (igemm_k3b.h): the single-chunk backward-data launches of the 48^3 level
    (16 -> 16 with a lazy conv input, 16 -> 8 / 16 -> 32 with a stored one), the 96^3 8 -> 16 one, and their 64^3 / 80^3 / ragged relatives;
    (n, side, gradient channels, conv-input channels, conv input is lazy)"""
    ops = _ops()
    from vae_segmentation_amd._lib import check, lib
    n, s_, c, m, lazy_in = case
    if dtype == torch.float32 and not (c == 16 and m == 16):
        pytest.skip("parity mode: the fused apply of k3x_kernel exists for the 16 -> 16 layers (k3xt_kernel takes 8 -> 8: test_k3_bwd_data_with_fused_apply)")
    d, h, w = s_, s_, s_ + (4 if s_ < 40 else 0)
    dev = "cuda"
    gen = torch.Generator().manual_seed(s_ + c)
    ax = (torch.randn(n, d, h, w, c, generator=gen) * 1.3 + 0.2).to(dtype).to(dev)
    g = torch.randn(n, d, h, w, c, generator=gen).to(dtype).to(dev)
    mx = (torch.randn(n, d, h, w, m, generator=gen) * 0.8 - 0.1).to(dtype).to(dev)
    wt = (torch.randn(c, m, 3, 3, 3, generator=gen) * 0.1).to(dev)                        # forward conv m -> c; backward-data c -> m
    ops.stats_arena_begin(ax.device)
    axs, mxs = ops.instnorm_stats(ax), ops.instnorm_stats(mx)
    vox, dt, st = d * h * w, ops.vs_dtype(ax), ops._stream()
    assert lib.vs_conv_k3_fused_apply_supported(n, d, h, w, c, m, int(lazy_in), dt) == 1
    asums = ops._new_stats(n, c, ax.device)
    check(lib.vs_instnorm_relu_bwd_reduce(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), n, vox, c, dt, 1e-5, st), "reduce")
    wpb = ops.pack_weight(wt, ops.VS_PACK_ROWS_D1_FLIP, c, ops.k3_pack_dtype(g))      # fp32: the three-limb image (k3x_kernel<8, 16, .., FA>, round 5)
    dx_ref = torch.empty_like(g)
    check(lib.vs_instnorm_relu_bwd_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), dx_ref.data_ptr(), n, vox, c, dt, 1e-5, st), "apply")
    y_ref, y = torch.empty_like(mx), torch.empty_like(mx)
    s_ref, s2 = ops._new_stats(n, m, ax.device), ops._new_stats(n, m, ax.device)
    dx = torch.full_like(g, 7.0)
    if lazy_in:
        check(lib.vs_conv_gather_bwd_data(dx_ref.data_ptr(), wpb.data_ptr(), y_ref.data_ptr(), mx.data_ptr(), mxs.data_ptr(), s_ref.data_ptr(),
                                          n, d, h, w, c, m, ops.VS_CONV_K3, dt, 1e-5, st), "bwd_data")
        check(lib.vs_conv_k3_bwd_data_fused_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), y.data_ptr(),
                                                  mx.data_ptr(), mxs.data_ptr(), s2.data_ptr(), dx.data_ptr(), n, d, h, w, c, m, dt, 1e-5, st), "fused")
    else:
        check(lib.vs_conv_gather_fwd(dx_ref.data_ptr(), None, wpb.data_ptr(), None, y_ref.data_ptr(), None, n, d, h, w, c, m, ops.VS_CONV_K3, dt, 1e-5, st), "plain")
        check(lib.vs_conv_k3_bwd_data_fused_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), y.data_ptr(),
                                                  None, None, None, dx.data_ptr(), n, d, h, w, c, m, dt, 1e-5, st), "fused")
    torch.cuda.synchronize()
    ulp = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -21}[dtype]
    edge = _dx_agrees(dx, dx_ref, ulp)
    assert _rel_l2(y, y_ref) < 4 * ulp and (edge or relerr(y.float().cpu(), y_ref.float().cpu()) < 4 * ulp)
    if lazy_in:
        t2, tr = ops.stats_total(s2), ops.stats_total(s_ref)
        assert float((t2 - tr).abs().max() / tr.abs().max()) < (4 * ulp if not edge else 0.05)
    # a shape without a fused kernel says so: the 6^3 volumes of the deep levels run k3s_kernel, which has no fused-apply form
    assert lib.vs_conv_k3_fused_apply_supported(n, 6, 6, 6, 128, 128, 1, dt) == 0
    # nor do the 32-channel chunks of the 24^3 / 12^3 levels since round 5 (the fused form measured slower twice: profiles/r04_ab_fused_apply_32ch.json)
    assert lib.vs_conv_k3_fused_apply_supported(2, 24, 24, 24, 32, 32, 1, dt) == 0


FUSED_WGRAD_CASES = [(2, 96, 96, 96), (2, 12, 16, 40), (1, 9, 11, 33), (3, 5, 9, 33), (1, 4, 8, 32), (1, 128, 128, 128), (16, 4, 8, 32), (25, 4, 8, 32)]      # (N, D, H, W)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fused_apply", [False, True])
@pytest.mark.parametrize("case", FUSED_WGRAD_CASES)
def test_k3_bwd_data_with_fused_weight_gradient(case, fused_apply, dtype):
    """vs_conv_k3_bwd_data_wgrad (igemm_k3tw.h): the backward-data launch of an 8 -> 8 layer that also forms the layer's weight gradient — against the two
    launches it replaces: backward-data output and fused sums identical to vs_conv_gather_bwd_data / vs_conv_k3_bwd_data_fused_apply (same instruction
    stream), dW (slabs through a VS_WGRAD_SLABS descriptor of vs_conv_wgrad_multi) against vs_conv_wgrad on the applied gradient; real (2 x 96^3,
    1 x 128^3), ragged and many-sample shapes; real channel counts below 8 in the descriptor (out_block-like 2 gradient channels)."""
    import ctypes
    ops = _ops()
    from vae_segmentation_amd._lib import check, lib
    n, d, h, w = case
    c = 8
    gen = torch.Generator().manual_seed(d + w)
    ax = (torch.randn(n, d, h, w, c, generator=gen) * 1.3 + 0.2).to(dtype).cuda()
    g = torch.randn(n, d, h, w, c, generator=gen).to(dtype).cuda()
    mx = (torch.randn(n, d, h, w, c, generator=gen) * 0.8 - 0.1).to(dtype).cuda()
    wt = (torch.randn(c, c, 3, 3, 3, generator=gen) * 0.1).cuda()
    ops.stats_arena_begin(ax.device)
    axs, mxs = ops.instnorm_stats(ax), ops.instnorm_stats(mx)
    vox, dt, st = d * h * w, ops.vs_dtype(ax), ops._stream()
    if n * 8 > 192:                               # the per-(n, c) tables of the kernel hold 192 pairs
        assert lib.vs_conv_k3_bwd_data_wgrad_supported(n, d, h, w, 8, 8, dt) == 0
        return
    assert lib.vs_conv_k3_bwd_data_wgrad_supported(n, d, h, w, 8, 8, dt) == 1
    assert lib.vs_conv_k3_bwd_data_wgrad_supported(n, d, h, w, 16, 16, dt) == 0 and lib.vs_conv_k3_bwd_data_wgrad_supported(n, d, h, w, 8, 8, 0) == 0
    asums = ops._new_stats(n, c, ax.device)
    check(lib.vs_instnorm_relu_bwd_reduce(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), n, vox, c, dt, 1e-5, st), "reduce")
    wpb = ops.pack_weight(wt, ops.VS_PACK_ROWS_D1_FLIP, c, dtype)
    dx_ref = torch.empty_like(g)
    check(lib.vs_instnorm_relu_bwd_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), dx_ref.data_ptr(), n, vox, c, dt, 1e-5, st), "apply")
    y_ref, y = torch.empty_like(mx), torch.empty_like(mx)
    s_ref, s2 = ops._new_stats(n, c, ax.device), ops._new_stats(n, c, ax.device)
    dx = torch.empty_like(g)
    if fused_apply:
        check(lib.vs_conv_k3_bwd_data_fused_apply(g.data_ptr(), ax.data_ptr(), axs.data_ptr(), asums.data_ptr(), wpb.data_ptr(), y_ref.data_ptr(),
                                                  mx.data_ptr(), mxs.data_ptr(), s_ref.data_ptr(), dx.data_ptr(), n, d, h, w, c, c, dt, 1e-5, st), "fused apply")
    else:
        check(lib.vs_conv_gather_bwd_data(dx_ref.data_ptr(), wpb.data_ptr(), y_ref.data_ptr(), mx.data_ptr(), mxs.data_ptr(), s_ref.data_ptr(),
                                          n, d, h, w, c, c, ops.VS_CONV_K3, dt, 1e-5, st), "bwd_data")
    nslabs = lib.vs_conv_k3_bwd_data_wgrad_slabs(n, d, h, w)
    assert 0 < nslabs <= 512
    slabs = torch.full((nslabs * 1728,), float("nan"), dtype=torch.float32, device="cuda")
    src = g if fused_apply else dx_ref
    check(lib.vs_conv_k3_bwd_data_wgrad(src.data_ptr(), ax.data_ptr() if fused_apply else None, axs.data_ptr() if fused_apply else None,
                                        asums.data_ptr() if fused_apply else None, wpb.data_ptr(), y.data_ptr(), mx.data_ptr(), mxs.data_ptr(), s2.data_ptr(),
                                        slabs.data_ptr(), n, d, h, w, c, c, dt, 1e-5, st), "bwd_data + wgrad")
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16))
    t2, tr = ops.stats_total(s2), ops.stats_total(s_ref)
    assert float((t2 - tr).abs().max() / tr.abs().max()) < 1e-6
    assert bool(torch.isfinite(slabs).all())
    applied = dx if fused_apply else dx_ref
    for m_real, c_real in ((8, 8), (2, 8), (8, 1)):
        dw = torch.full((m_real, c_real, 27), float("nan"), dtype=torch.float32, device="cuda")
        desc = ops.WgradDesc(slabs.data_ptr(), None, None, None, dw.data_ptr(), None, None, 0, 0, 0, nslabs, 0, 0, 0, 8, 8, m_real, c_real, ops.VS_WGRAD_SLABS, 0)
        arr = (ops.WgradDesc * 1)(desc)
        nbytes = lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(arr), 1, dt)
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        check(lib.vs_conv_wgrad_multi(ctypes.addressof(arr), 1, ws.data_ptr(), nbytes, dt, 1e-5, st), "wgrad_multi (slabs)")
        ref = ops.conv_wgrad(applied, None, mx, mxs, m_real, c_real, ops.VS_CONV_K3, (m_real, c_real, 3, 3, 3)).reshape(m_real, c_real, 27)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dw).all())
        assert _rel_l2(dw, ref) < 2e-5, (m_real, c_real, _rel_l2(dw, ref))
    # a slab descriptor next to a regular one in the same call; sharing its destination with another descriptor is refused
    dw_a = torch.empty(8, 8, 27, dtype=torch.float32, device="cuda")
    dw_b = torch.empty(8, 8, 27, dtype=torch.float32, device="cuda")
    d_slab = ops.WgradDesc(slabs.data_ptr(), None, None, None, dw_a.data_ptr(), None, None, 0, 0, 0, nslabs, 0, 0, 0, 8, 8, 8, 8, ops.VS_WGRAD_SLABS, 0)
    d_reg = ops.WgradDesc(applied.data_ptr(), None, mx.data_ptr(), mxs.data_ptr(), dw_b.data_ptr(), None, None, 0, 0, 0, n, d, h, w, 8, 8, 8, 8, ops.VS_CONV_K3, 0)
    arr = (ops.WgradDesc * 2)(d_slab, d_reg)
    nbytes = lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(arr), 2, dt)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    check(lib.vs_conv_wgrad_multi(ctypes.addressof(arr), 2, ws.data_ptr(), nbytes, dt, 1e-5, st), "wgrad_multi (mixed)")
    torch.cuda.synchronize()
    assert _rel_l2(dw_a, dw_b) < 2e-5
    d_reg2 = ops.WgradDesc(applied.data_ptr(), None, mx.data_ptr(), mxs.data_ptr(), dw_a.data_ptr(), None, None, 0, 0, 0, n, d, h, w, 8, 8, 8, 8, ops.VS_CONV_K3, 0)
    arr = (ops.WgradDesc * 2)(d_slab, d_reg2)
    assert lib.vs_conv_wgrad_multi(ctypes.addressof(arr), 2, ws.data_ptr(), nbytes, dt, 1e-5, st) == -1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("parts", ["planar", "cl", "both"])
@pytest.mark.parametrize("case", [(2, 96, 96, 96, 0.0), (2, 12, 16, 40, 0.3), (1, 9, 11, 33, 0.0), (3, 5, 9, 33, 0.25)])
def test_out_block_backward_as_one_launch(case, parts, dtype):
    """vs_conv_k3_softmax2_bwd_data (igemm_k3tw.h, SM staging): out_block's backward — softmax backward (planar and / or channels-last gradient parts, logit
    dropout), backward-data with the fused sums, weight gradient slabs and bias partials — against the launches it replaces: vs_softmax2_cl_bwd,
    vs_conv_gather_bwd_data, vs_conv_wgrad, vs_bias_grad.  Same arithmetic on the same rounded logit gradients: the backward-data output is bit-identical."""
    import ctypes
    ops = _ops()
    from vae_segmentation_amd._lib import check, lib
    n, d, h, w, pdrop = case
    vox, seed = d * h * w, 777
    gen = torch.Generator().manual_seed(d * 7 + w)
    logits = torch.randn(n, 2, d, h, w, generator=gen) * 2.0
    prob = torch.softmax(logits, dim=1).contiguous().cuda()
    gprob = torch.randn(n, 2, d, h, w, generator=gen).cuda() if parts != "cl" else None
    gcl = None
    if parts != "planar":
        gcl = torch.zeros(n, d, h, w, 8, dtype=dtype)
        gcl[..., :2] = torch.randn(n, d, h, w, 2, generator=gen).to(dtype)
        gcl[..., 2:] = 5.0                                       # padded channels of the channels-last part are never read
        gcl = gcl.cuda()
    mx = (torch.randn(n, d, h, w, 8, generator=gen) * 0.8 - 0.1).to(dtype).cuda()
    wt = (torch.randn(2, 8, 3, 3, 3, generator=gen) * 0.1).cuda()      # out_block: 8 -> 2
    ops.stats_arena_begin(mx.device)
    mxs = ops.instnorm_stats(mx)
    dt, st = ops.vs_dtype(mx), ops._stream()
    wpb = ops.pack_weight(wt, ops.VS_PACK_ROWS_D1_FLIP, 8, dtype)
    p_ = lambda t: None if t is None else t.data_ptr()
    gl = torch.empty(n, d, h, w, 8, dtype=dtype, device="cuda")
    check(lib.vs_softmax2_cl_bwd(prob.data_ptr(), p_(gprob), p_(gcl), gl.data_ptr(), n, vox, 8, dt, pdrop, seed, st), "softmax2_cl_bwd")
    y_ref, y = torch.empty_like(mx), torch.empty_like(mx)
    s_ref, s2 = ops._new_stats(n, 8, mx.device), ops._new_stats(n, 8, mx.device)
    check(lib.vs_conv_gather_bwd_data(gl.data_ptr(), wpb.data_ptr(), y_ref.data_ptr(), mx.data_ptr(), mxs.data_ptr(), s_ref.data_ptr(), n, d, h, w, 8, 8,
                                      ops.VS_CONV_K3, dt, 1e-5, st), "bwd_data")
    dw_ref = ops.conv_wgrad(gl, None, mx, mxs, 2, 8, ops.VS_CONV_K3, (2, 8, 3, 3, 3)).reshape(2, 8, 27)
    db_ref = ops.bias_grad(gl, 2)
    nslabs = lib.vs_conv_k3_bwd_data_wgrad_slabs(n, d, h, w)
    for want_w, want_b in ((True, True), (True, False), (False, False)):
        slabs = torch.full((nslabs * 1728,), float("nan"), dtype=torch.float32, device="cuda") if want_w else None
        bpart = torch.full((nslabs * 2,), float("nan"), dtype=torch.float64, device="cuda") if want_b else None
        s2.zero_(); y.fill_(3.0)
        check(lib.vs_conv_k3_softmax2_bwd_data(prob.data_ptr(), p_(gprob), p_(gcl), wpb.data_ptr(), y.data_ptr(), mx.data_ptr(), mxs.data_ptr(), s2.data_ptr(),
                                               p_(slabs), p_(bpart), n, d, h, w, dt, 1e-5, pdrop, seed, st), "softmax2_bwd_data")
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16))
        t2, tr = ops.stats_total(s2), ops.stats_total(s_ref)
        assert float((t2 - tr).abs().max() / tr.abs().max()) < 1e-6
        if not want_w:
            continue
        dw = torch.full((2, 8, 27), float("nan"), dtype=torch.float32, device="cuda")
        db = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
        desc = ops.WgradDesc(slabs.data_ptr(), None, None, None, dw.data_ptr(), p_(bpart), db.data_ptr() if want_b else None, nslabs if want_b else 0,
                             2 if want_b else 0, 2 if want_b else 0, nslabs, 0, 0, 0, 8, 8, 2, 8, ops.VS_WGRAD_SLABS, 0)
        arr = (ops.WgradDesc * 1)(desc)
        nbytes = lib.vs_conv_wgrad_multi_workspace_bytes(ctypes.addressof(arr), 1, dt)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        check(lib.vs_conv_wgrad_multi(ctypes.addressof(arr), 1, ws.data_ptr(), nbytes, dt, 1e-5, st), "wgrad_multi (slabs + bias partials)")
        torch.cuda.synchronize()
        assert _rel_l2(dw, dw_ref) < 2e-5
        if want_b:
            assert _rel_l2(db, db_ref) < 2e-5
    # the bias partials need the slabs; neither gradient part is refused
    assert lib.vs_conv_k3_softmax2_bwd_data(prob.data_ptr(), p_(gprob), p_(gcl), wpb.data_ptr(), y.data_ptr(), mx.data_ptr(), mxs.data_ptr(), s2.data_ptr(),
                                            None, s2.data_ptr(), n, d, h, w, dt, 1e-5, pdrop, seed, st) == -1
    assert lib.vs_conv_k3_softmax2_bwd_data(prob.data_ptr(), None, None, wpb.data_ptr(), y.data_ptr(), mx.data_ptr(), mxs.data_ptr(), s2.data_ptr(),
                                            None, None, n, d, h, w, dt, 1e-5, pdrop, seed, st) == -1


@pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", [(3, 8, 50), (2, 8, 26), (3, 8, 18), (1, 8, 34)])
def test_k2s2_scatter8_streaming_kernel_equals_the_mfma_tile_kernel(case, dtype, lib_mode):
    """the 8 -> 8 stride-2 backward-data at full resolution runs k2s2_scatter8_kernel (csrc/k2s2_scatter8.hip) by default; A/B against the
    g1_kernel<8, PW, SCATTER> it replaced (vs_config.k2s2_stream = 0) on shapes where the coarse voxel count is NOT a multiple of 32 (25^3, 13^3, 9^3, 17^3:
    partial last items, sample boundaries inside a workgroup's run with N = 3): the applied gradient (un-applied values + fused InstanceNorm-backward sums) and
    the weight gradient that reads it."""
    ops = _ops()
    n, c, s = case
    x = rnd(n, c, s, s, s, seed=31)
    wt = q(rnd(c, c, 2, 2, 2, seed=32, scale=(3.0 / (8 * c)) ** 0.5), dtype)
    gy = to_cl(rnd(n, c, s // 2, s // 2, s // 2, seed=33), c, dtype)
    res = {}
    for stream in (0, 1):
        with ops.config(k2s2_stream=stream):
            x_cl = to_cl(x, c, dtype).requires_grad_(True)
            xs = ops.instnorm_stats(x_cl.detach())
            w_gpu = wt.clone().cuda().requires_grad_(True)
            ops.stats_arena_begin(x_cl.device)
            y = ops.ConvK2S2.apply(x_cl, xs, w_gpu, None)
            y.backward(gy)
            torch.cuda.synchronize()
            res[stream] = (x_cl.grad.detach().clone(), w_gpu.grad.detach().clone())
    tol = {torch.bfloat16: 1.5e-2, torch.float16: 2e-3}[dtype]
    e = relerr(res[1][0].double().cpu(), res[0][0].double().cpu())
    # the two kernels form the 8 x 8 products in different orders (MFMA tile vs vector ALU) and sum the fused statistics in different orders: the applied
    # gradients agree to fp32 summation rounding (measured 1.2e-6 of the tensor's maximum at 25^3 x 3), far inside one rounding of the storage type
    assert e < tol, "applied gradient: %g" % e          # (fp16: a few elements round the other way, 1 ulp = 4.9e-4 of their value)
    assert relerr(res[1][1].cpu(), res[0][1].cpu()) < 2e-5, "weight gradient"
