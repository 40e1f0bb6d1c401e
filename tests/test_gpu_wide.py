"""The wide models: feature widths up to 512 channels (n_fmaps [16, 32, 64, 128, 256, 512], the setting the reference's joint_model.py
comments above its defaults).

  * layers at C/M in {256 -> 512, 512 -> 512, 512 -> 256} on 4^3, 8^3 and a ragged volume, batch 1 and 2: 3x3x3 forward and backward
    (data through the lazy InstanceNorm+ReLU input, weight, bias), stride-2 conv, transposed conv and the InstanceNorm+ReLU passes, in the three
    storage modes, against CPU fp64 autograd at the tolerances of tests/test_gpu_layers.py;
  * the reference goldens of tools/make_golden_wide.py (tests/golden/wide.npz) at the gates of their <= 256-channel siblings in test_gpu_model.py;
  * the wide step captured in train.GraphedStep, bit-identical to eager and run to run (deterministic build);
  * the fp64-atomic build (libvaeseg.so) in a child process started with VS_DETERMINISTIC=0;
  * the fused / chain / composed-Up queries decline the 512-channel shapes, and the module contract (state_dict keys and fc shapes)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import golden_util as G
from tests import stats_util as SU
from tests.test_gpu_ops import TOL, from_cl, q, rnd, to_cl

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = [torch.float32, torch.bfloat16, torch.float16]
WIDE_VAE = [16, 32, 64, 128, 256, 512]
WIDE_SEG = [32, 64, 128, 256, 512, 512]
RTOL_FP32 = 1e-3          # tests/test_gpu_model.py
RTOL_GRAD_FP32 = 2e-3

# (N, Cin, Cout, (D, H, W)): 4^3 — the small-volume kernels; 8^3 and the ragged 5 x 6 x 9 — the tiled ones
# 4^3 / 2^3 with more than 256 input channels: the split form of the small-volume kernel (csrc/igemm_k3s.h k3s_split_kernel); 384: a width between 256 and 512
K3_WIDE = [(n, ci, co, dims) for (ci, co) in ((256, 512), (512, 512), (512, 256))
           for (n, dims) in ((2, (4, 4, 4)), (1, (8, 8, 8)), (2, (5, 6, 9)))] + [(2, 512, 512, (2, 2, 2)), (2, 384, 512, (4, 4, 4)), (1, 384, 256, (8, 8, 8))]
S2_WIDE = [(2, 512, (4, 4, 4)), (1, 512, (8, 8, 8)), (2, 512, (4, 6, 2))]     # Conv3d(C, C, 2, stride 2): input dims
T2_WIDE = [(2, 512, (2, 2, 2)), (1, 512, (4, 4, 4)), (2, 512, (3, 2, 5))]     # ConvTranspose3d(C, C, 2, stride 2): input dims


def _ops():
    from vae_segmentation_amd import ops
    return ops


def _in_relu64(x):
    return torch.relu(F.instance_norm(x))


def _relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _report(tag, errs, lims):
    bad = {k: (errs[k], lims[k]) for k in errs if not errs[k] < lims[k]}
    print("\n%s: %s" % (tag, ", ".join("%s %.2e (<%.1e)" % (k, errs[k], lims[k]) for k in errs)))
    assert not bad, "%s: %s" % (tag, bad)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", K3_WIDE)
def test_k3_wide_layer(case, dtype):
    """3x3x3 conv (live bias) on a lazy InstanceNorm+ReLU input: y, its statistics, dx (through the IN+ReLU backward), dW, db."""
    ops = _ops()
    n, cin, cout, dims = case
    x = rnd(n, cin, *dims, seed=1)
    wt = rnd(cout, cin, 3, 3, 3, seed=2, scale=(3.0 / (27 * cin)) ** 0.5)
    b = rnd(cout, seed=3, scale=0.1)
    gy = rnd(n, cout, *dims, seed=4)
    xq, wq, bq = (q(x, dtype).double().requires_grad_(True), q(wt, dtype).double().requires_grad_(True),
                  b.double().requires_grad_(True))
    y_ref = F.conv3d(_in_relu64(xq), wq, bq, padding=1)
    (y_ref * q(gy, dtype).double()).sum().backward()

    x_cl = to_cl(x, cin, dtype).requires_grad_(True)
    xs = ops.instnorm_stats(x_cl.detach())
    w_gpu, b_gpu = q(wt, dtype).cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ops.stats_arena_begin(x_cl.device)
    y, ys = ops.ConvK3.apply(x_cl, xs, w_gpu, b_gpu, True)
    y.backward(to_cl(gy, cout, dtype))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    yr = q(y_ref.detach(), dtype).double()
    st = ops.stats_total(ys).cpu()[:, :cout].double()
    ref_sum, ref_sq = yr.sum((2, 3, 4)), (yr * yr).sum((2, 3, 4))
    errs = {"y": _relerr(from_cl(y, cout), y_ref.detach()),
            "stat_sum": float((st[..., 0] - ref_sum).abs().max() / ref_sq.sqrt().max()),
            "stat_sq": float((st[..., 1] - ref_sq).abs().max() / ref_sq.max()),
            "gx": _relerr(from_cl(x_cl.grad, cin), xq.grad), "gw": _relerr(w_gpu.grad.cpu(), wq.grad),
            "gb": _relerr(b_gpu.grad.cpu(), bq.grad)}
    lims = {"y": tol, "stat_sum": 4 * tol, "stat_sq": 4 * tol, "gx": 4 * tol, "gw": 4 * tol, "gb": 4 * tol}
    _report("k3 wide %s %s" % (case, dtype), errs, lims)
    # per (n, c): mean / rstd against each channel's own fp64 two-pass statistics (tests/stats_util.py); lazy input, so the storage type's tolerance
    SU.check_stats(st, SU.two_pass(yr), "k3 wide %s %s" % (case, dtype), mean_tol=4 * tol, rstd_tol=4 * tol, sum_tol=4 * tol, rstd_tol_high=4 * tol, rstd_grows_with_r=True)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", S2_WIDE)
def test_k2s2_wide_layer(case, dtype):
    ops = _ops()
    n, c, dims = case
    x = rnd(n, c, *dims, seed=5)
    wt = rnd(c, c, 2, 2, 2, seed=6, scale=(3.0 / (8 * c)) ** 0.5)
    b = rnd(c, seed=7, scale=0.1)
    gy = rnd(n, c, *[s // 2 for s in dims], seed=8)
    xq, wq, bq = q(x, dtype).double().requires_grad_(True), q(wt, dtype).double().requires_grad_(True), b.double().requires_grad_(True)
    y_ref = F.conv3d(_in_relu64(xq), wq, bq, stride=2)
    (y_ref * q(gy, dtype).double()).sum().backward()
    x_cl = to_cl(x, c, dtype).requires_grad_(True)
    xs = ops.instnorm_stats(x_cl.detach())
    w_gpu, b_gpu = q(wt, dtype).cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ops.stats_arena_begin(x_cl.device)
    y = ops.ConvK2S2.apply(x_cl, xs, w_gpu, b_gpu)
    y.backward(to_cl(gy, c, dtype))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    errs = {"y": _relerr(from_cl(y, c), y_ref.detach()), "gx": _relerr(from_cl(x_cl.grad, c), xq.grad),
            "gw": _relerr(w_gpu.grad.cpu(), wq.grad), "gb": _relerr(b_gpu.grad.cpu(), bq.grad)}
    _report("k2s2 wide %s %s" % (case, dtype), errs, {"y": tol, "gx": 4 * tol, "gw": 4 * tol, "gb": 4 * tol})


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", T2_WIDE)
def test_transposed_wide_layer(case, dtype):
    ops = _ops()
    n, c, dims = case
    x = rnd(n, c, *dims, seed=9)
    wt = rnd(c, c, 2, 2, 2, seed=10, scale=(3.0 / c) ** 0.5)
    b = rnd(c, seed=11, scale=0.1)
    gy = rnd(n, c, *[2 * s for s in dims], seed=12)
    xq, wq, bq = q(x, dtype).double().requires_grad_(True), q(wt, dtype).double().requires_grad_(True), b.double().requires_grad_(True)
    y_ref = F.conv_transpose3d(_in_relu64(xq), wq, bq, stride=2)
    (y_ref * q(gy, dtype).double()).sum().backward()
    x_cl = to_cl(x, c, dtype).requires_grad_(True)
    xs = ops.instnorm_stats(x_cl.detach())
    w_gpu, b_gpu = q(wt, dtype).cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    ops.stats_arena_begin(x_cl.device)
    y = ops.ConvT2S2.apply(x_cl, xs, w_gpu, b_gpu)
    y.backward(to_cl(gy, c, dtype))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    errs = {"y": _relerr(from_cl(y, c), y_ref.detach()), "gx": _relerr(from_cl(x_cl.grad, c), xq.grad),
            "gw": _relerr(w_gpu.grad.cpu(), wq.grad), "gb": _relerr(b_gpu.grad.cpu(), bq.grad)}
    _report("convT wide %s %s" % (case, dtype), errs, {"y": tol, "gx": 4 * tol, "gw": 4 * tol, "gb": 4 * tol})


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", [(2, 512, (4, 4, 4)), (1, 512, (8, 8, 8)), (2, 512, (5, 6, 9)), (2, 384, (4, 4, 4)), (1, 288, (5, 6, 9))])
def test_in_relu_wide(case, dtype):
    """InstanceNorm+ReLU at 512 channels: statistics, the materialising pass (with the skip add) and its backward (reduce + apply)."""
    ops = _ops()
    n, c, dims = case
    x1, x2 = rnd(n, c, *dims, seed=13), rnd(n, c, *dims, seed=14) * 2 + 0.3
    g = rnd(n, c, *dims, seed=15)
    a1, a2 = q(x1, dtype).double().requires_grad_(True), q(x2, dtype).double().requires_grad_(True)
    ref = _in_relu64(a1) + _in_relu64(a2)
    (ref * q(g, dtype).double()).sum().backward()
    c1, c2 = to_cl(x1, c, dtype).requires_grad_(True), to_cl(x2, c, dtype).requires_grad_(True)
    s1 = ops.instnorm_stats(c1.detach())
    ops.stats_arena_begin(c1.device)
    out = ops.Materialize.apply(c1, s1, c2, ops.instnorm_stats(c2.detach()))
    out.backward(to_cl(g, c, dtype))
    torch.cuda.synchronize()
    tol = TOL[dtype]
    xr = q(x1, dtype).double()
    st = ops.stats_total(s1).cpu().double()
    errs = {"sum": _relerr(st[..., 0], xr.sum((2, 3, 4))), "sumsq": _relerr(st[..., 1], (xr * xr).sum((2, 3, 4))),
            "out": _relerr(from_cl(out, c), ref.detach()), "g1": _relerr(from_cl(c1.grad, c), a1.grad), "g2": _relerr(from_cl(c2.grad, c), a2.grad)}
    _report("in_relu wide %s %s" % (case, dtype), errs, {"sum": 1e-5, "sumsq": 1e-5, "out": tol, "g1": 2 * tol, "g2": 2 * tol})


# ---- the reference goldens (tools/make_golden_wide.py) ----
def _mods():
    import joint_model
    from oracle import ref_cpu as O
    from vae_segmentation_amd import train as T
    return joint_model, O, T


def _gold(tag):
    return G.sub(G.load("wide"), tag + "/")


def test_wide_vae64_vs_reference_golden():
    M, O, T = _mods()
    g = _gold("wide_vae64")
    vae = O.deterministic_fill_(M.VAE(2, 2, norm_type=1, dim=128, n_fmaps=WIDE_VAE, spatial=64), seed=0).cuda()
    noise = torch.from_numpy(2 * O.hashed_uniform(2 * 128, 7100, 5) - 1).view(2, 128)
    final, aux = T.vae_train_losses(vae, O.synthetic_label(2, 64, 3).cuda(), scale=0.35, noise=noise.cuda())
    final.backward()
    G.scalar_close(g, "final", final.item(), RTOL_FP32)
    G.scalar_close(g, "kl", aux["kl_loss"].item(), RTOL_FP32)
    b = aux["batch"]
    assert G.rel_l2(b["mean"].detach().cpu(), g["mean@f64"]) < max(RTOL_FP32, 3 * G.rel_l2(g["mean"], g["mean@f64"]))
    assert G.rel_l2(b["std"].detach().cpu(), g["std@f64"]) < max(RTOL_FP32, 3 * G.rel_l2(g["std"], g["std@f64"]))
    G.check_tensor_f64(g, "recon", b["recon"], k=256, floor=RTOL_FP32)
    rep = G.check_grads_f64(g, "vae", [(n, p.grad) for n, p in vae.named_parameters()], floor=RTOL_GRAD_FP32, what="wide_vae64")
    G.vacuity(rep, "wide_vae64")


def test_wide_seg32_vs_reference_golden():
    M, O, T = _mods()
    g = _gold("wide_seg32")
    seg = O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1, n_fmaps=WIDE_SEG), seed=0).cuda()
    loss, aux = T.seg_train_losses(seg, O.synthetic_image(2, 32, 2).cuda(), O.synthetic_label(2, 32, 3).cuda(), eps=1e-6)
    loss.backward()
    G.scalar_close(g, "dice_loss_eps1e6", loss.item(), RTOL_FP32)
    G.check_tensor_f64(g, "pred", aux["batch"]["pred"], k=256, floor=RTOL_FP32)
    rep = G.check_grads_f64(g, "seg", [(n, p.grad) for n, p in seg.named_parameters()], floor=RTOL_GRAD_FP32, what="wide_seg32")
    G.vacuity(rep, "wide_seg32")


def _wide_joint(M, O, side):
    seg = M.Segmentation(n_channels=1, n_class=2, norm_type=1)
    vae = M.VAE(n_channels=2, n_class=2, norm_type=1, dim=128, n_fmaps=WIDE_VAE, spatial=side)
    joint = M.Joint(models=[seg, vae])
    O.deterministic_fill_(joint, seed=0)
    joint = joint.cuda()
    for p in joint.Vae.parameters():
        p.requires_grad = False
    joint.Vae.eval()
    return joint


def test_wide_joint64_vs_reference_golden():
    M, O, T = _mods()
    g = _gold("wide_joint64")
    joint = _wide_joint(M, O, 64)
    final, aux = T.joint_train_losses(joint, O.synthetic_image(2, 64, 2).cuda(), O.synthetic_label(2, 64, 3).cuda())
    final.backward()
    torch.cuda.synchronize()
    for key, val in (("final", final), ("recon_loss", aux["recon_loss"]), ("dice_loss", aux["dice_loss"])):
        G.scalar_close(g, key, val.item(), RTOL_FP32)
    b = aux["batch"]
    assert G.rel_l2(b["mean"].detach().cpu(), g["mean@f64"]) < max(RTOL_FP32, 3 * G.rel_l2(g["mean"], g["mean@f64"]))
    G.check_tensor_f64(g, "pred", b["pred"], k=512, floor=RTOL_FP32)
    G.check_tensor_f64(g, "recon", b["recon"], k=512, floor=RTOL_FP32)
    rep = G.check_grads_f64(g, "seg", [(n, p.grad) for n, p in joint.Seg.named_parameters()], floor=RTOL_GRAD_FP32, what="wide_joint64")
    G.vacuity(rep, "wide_joint64")
    assert all(p.grad is None for p in joint.Vae.parameters())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_wide_vae_graphed_step_matches_eager(dtype):
    """The wide VAE's training step captured in train.GraphedStep: bit-identical to the eager step and run to run (deterministic build)."""
    M, O, T = _mods()
    from vae_segmentation_amd import ops, optim
    assert ops.is_deterministic()
    lab = O.synthetic_label(2, 64, 3).cuda()
    noise = (2 * torch.from_numpy(O.hashed_uniform(2 * 128, 7100, 5)) - 1).view(2, 128).float().cuda()

    def build():
        vae = O.deterministic_fill_(M.VAE(2, 2, norm_type=1, dim=128, n_fmaps=WIDE_VAE, spatial=64), seed=0)
        return M.set_kernel_dtype(vae.cuda(), dtype)

    def run_graphed():
        vae = build()
        opt = optim.SGD(vae.parameters(), lr=1e-3, momentum=0.9)
        gs = T.GraphedStep(lambda: T.vae_train_losses(vae, lab, scale=0.35, noise=noise), vae.parameters(), opt, warmup=1)
        losses = [gs.step().item() for _ in range(3)]       # warmup=1: one eager step, then the capture and its replays
        return losses, [p.detach().clone() for p in vae.parameters()]

    va = build()
    opt_a = optim.SGD(va.parameters(), lr=1e-3, momentum=0.9)
    eager = []
    for _ in range(3):
        opt_a.zero_grad()
        la, _ = T.vae_train_losses(va, lab, scale=0.35, noise=noise)
        la.backward()
        opt_a.step()
        eager.append(la.item())
    l1, p1 = run_graphed()
    l2, p2 = run_graphed()
    assert l1 == l2 and all(torch.equal(a, b) for a, b in zip(p1, p2)), "graph replay not reproducible run to run"
    assert l1 == eager, (l1, eager)
    for (n, pa), pb in zip(va.named_parameters(), p1):
        assert torch.equal(pa.detach(), pb), n


def test_wide_atomic_build_in_child_process():
    """The fp64-atomic build (libvaeseg.so, the benchmarked library): the layer tests and one golden, in a child started with VS_DETERMINISTIC=0."""
    env = dict(os.environ, VS_DETERMINISTIC="0")
    sel = "k3_wide_layer or k2s2_wide_layer or transposed_wide_layer or in_relu_wide or wide_seg32"
    code = ("import sys, pytest; from vae_segmentation_amd import ops; assert not ops.is_deterministic(); "
            "sys.exit(pytest.main(['-q', '-p', 'no:cacheprovider', '-m', 'gpu', '-k', %r, %r]))" % (sel, os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1]


# ---- the paths that decline 512 channels, and the module contract ----
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_fused_chain_up_queries_decline_512_channels(dt):
    ops = _ops()
    lib = ops.lib
    d = {"bf16": ops.VS_BF16, "f16": ops.VS_F16, "f32": ops.VS_F32}[dt]
    for n, s in ((1, 4), (2, 4), (2, 2), (2, 8)):
        assert lib.vs_conv_k3_chain_supported(n, s, s, s, 512, d) == 0
        for ci, co in ((512, 512), (512, 256), (256, 512)):
            assert lib.vs_conv_k3_fused_apply_supported(n, s, s, s, ci, co, 1, d) == 0
            assert lib.vs_conv_k3_fused_apply_supported(n, s, s, s, ci, co, 0, d) == 0
            assert lib.vs_conv_k3_bwd_data_applied_supported(n, s, s, s, ci, co, d) == 0
            assert lib.vs_conv_s2_bwd_data_applied_supported(n, s, s, s, ci, co, 0, d) == 0
            assert lib.vs_conv_s2_bwd_data_applied_supported(n, s, s, s, ci, co, 1, d) == 0
    for co in (16, 64, 128, 256):
        assert lib.vs_up_supported(512, 512, co, d) == 0


@pytest.mark.parametrize("c_in", [24, 544, 1024])
def test_conv_channel_rule_refuses_other_widths(c_in):
    """check_common (csrc/conv_api.hip) refuses what is neither 8, 16 nor a multiple of 32 up to 512, before any launch (512 itself: the layer tests above)."""
    ops = _ops()
    n, s = 1, 4
    x = torch.zeros(n * s * s * s * c_in, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(27 * c_in * 16, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(n * s * s * s * 16, dtype=torch.bfloat16, device="cuda")
    rc = ops.lib.vs_conv_gather_fwd(x.data_ptr(), None, w.data_ptr(), None, y.data_ptr(), None, n, s, s, s, c_in, 16, ops.VS_CONV_K3, ops.VS_BF16,
                                    1e-5, None)
    assert rc == -2, rc                  # VS_ESHAPE (include/vaeseg.h)


@pytest.mark.parametrize("dtype", DT)
def test_k3_split_form_bit_identical_run_to_run(dtype):
    """The split form's fixed-order reduction (deterministic build): two runs of a 512 -> 512 layer at 4^3 give the same bits, forward and backward."""
    ops = _ops()
    assert ops.is_deterministic()
    n, c, dims = 2, 512, (4, 4, 4)
    x = rnd(n, c, *dims, seed=21)
    wt = rnd(c, c, 3, 3, 3, seed=22, scale=(3.0 / (27 * c)) ** 0.5)
    gy = rnd(n, c, *dims, seed=23)

    def run():
        x_cl = to_cl(x, c, dtype).requires_grad_(True)
        xs = ops.instnorm_stats(x_cl.detach())
        w_gpu = q(wt, dtype).cuda().requires_grad_(True)
        ops.stats_arena_begin(x_cl.device)
        y, ys = ops.ConvK3.apply(x_cl, xs, w_gpu, None)
        y.backward(to_cl(gy, c, dtype))
        torch.cuda.synchronize()
        return y.detach().clone(), ops.stats_total(ys).clone(), x_cl.grad.clone(), w_gpu.grad.clone()

    a, b = run(), run()
    for ta, tb, what in zip(a, b, ("y", "stats", "gx", "gw")):
        assert torch.equal(ta, tb), what


def test_wide_state_dict_matches_reference_modules():
    """state_dict keys equal those of oracle/ref_cpu.py's modules built with the same n_fmaps; fc shapes follow n_fmaps[5] * side^3 as in the
    golden (ref_cpu.VAE fixes its fc width at 256 * side^3, so its fc shapes are not the yardstick here)."""
    M, O, _ = _mods()
    g = G.load("wide")
    for side in (64, 128):
        vae = M.VAE(2, 2, norm_type=1, dim=128, n_fmaps=WIDE_VAE, spatial=side)
        ovae = O.VAE(2, 2, norm_type=1, dim=128, n_fmaps=WIDE_VAE, spatial=side)
        sd, osd = vae.state_dict(), ovae.state_dict()
        assert list(sd.keys()) == list(osd.keys())
        for k in sd:
            if k.startswith("fc"):
                assert tuple(sd[k].shape) == tuple(g["fc/vae%d/%s" % (side, k)]), k
            else:
                assert sd[k].shape == osd[k].shape, k
    seg, oseg = M.Segmentation(1, 2, norm_type=1, n_fmaps=WIDE_SEG), O.Segmentation(1, 2, norm_type=1, n_fmaps=WIDE_SEG)
    assert [(k, v.shape) for k, v in seg.state_dict().items()] == [(k, v.shape) for k, v in oseg.state_dict().items()]
    # the Encoder's expected fc shapes are by construction (tools/make_golden_wide.py: f[5] * (128 / 32)^3 in place of the reference's hard-coded 16384),
    # as is the Fusion check below (two of its widest weights): a contract guard, not a comparison with the reference's own shapes
    enc = M.Encoder(2, 128, norm_type=1, n_fmaps=WIDE_VAE, spatial=128)
    for k, v in enc.state_dict().items():
        if k.startswith("fc") and k.endswith("weight"):
            assert tuple(v.shape) == tuple(g["fc/enc128/%s" % k]), k
    fus = M.Fusion(1, 2, 2, norm_type=1, n_fmaps=WIDE_SEG)
    assert fus.down4.conv[1].conv[0].weight.shape[0] == 512 and fus.up2.conv[0].weight.shape[0] == 512
