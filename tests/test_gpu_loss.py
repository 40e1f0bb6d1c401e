"""The loss and label kernels of csrc/loss.hip and csrc/softmax.hip against their fp64 restatement (tests/loss_util.py, pinned on the host by tests/test_host_loss.py), in
both builds, at the sizes where the kernels change path.  Inputs are planar fp32 tensors (B, C, 1, 4, V / 4), so the voxel count V of a plane is set directly.

Branch reached by each DiceLossSum plane size (nblk = ceil(V / 2048) partial blocks, at most DICE_MULTI_BLOCKS = 256; the finish kernel gives 16 threads
to a statistic, each walking blk = sl, sl + 16, ...: the eight-way unrolled loop runs while blk + 112 < nblk, the remainder loop takes the rest):
  nblk   1, 2        one partial per statistic or two; only lanes 0 / 0-1 of the remainder loop add anything
  nblk  15, 16, 17   the remainder loop: one pass with the last lane idle, one full pass, a second pass for lane 0 alone
  nblk 127, 128, 129 the unrolled loop: not entered (127: 8 remainder passes, lane 15 makes 7), entered once by every lane with nothing left over,
                     entered once and lane 0 makes one remainder pass
  nblk 255, 256      the unrolled loop entered once by lane 15 and twice by the others (255); twice by every lane, at the block cap (256)
  V = 592,704        290 blocks wanted, 256 launched: the partial kernel's grid-stride loop wraps (blocks 0..33 make a second, ragged trip)
each once with the last block full (V = 2048 nblk) and once with a single quad in it (V = 2048 (nblk - 1) + 4).
  Dice, atomic build: 512 and 8,192 voxels are one block of dice_sums_kernel, 8,196 and 13,824 two (the deterministic build always launches one);
  V = 8,998,912 reaches its 1,024-block cap and the 2,048-block caps of dice_bwd_kernel and dice_multi_bwd_kernel (2,197 blocks wanted).

Tolerances (from the kernels' arithmetic, none measured): products and pair sums are formed in fp32 and accumulated in fp64, so I, S, T carry a relative
error <= 2^-23 for non-negative inputs; three casts to fp32 and about five fp32 operations follow: below 5e-7 on a Dice value in [0, 1] -> 1e-6 absolute;
a weighted sum 2e-6 sum |w_j|; gradients the norm-wise relerr < 1e-5 the existing Dice tests hold; BCE mean 2e-6 relative, KL 1e-5 relative, their
gradients 1e-5; softmax probabilities 1e-6 absolute on the storage-rounded logits, softmax gradients the per-dtype bounds of tests/test_gpu_ops.py."""
import functools

import pytest
import torch

from tests import loss_util as L

pytestmark = pytest.mark.gpu

both = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
CFGS = [(2, 0, 2), (2, 1, 2), (4, 1, 4), (8, 1, 8), (8, 2, 5)]          # (C, bot, top)
WEIGHTS = [0.1, 1.0, -0.37, 2.5]                                       # unequal, one exactly 1 (no multiply in the unfused spelling), one negative
NBLK = [1, 2, 15, 16, 17, 127, 128, 129, 255, 256]
PLANE_SIZES = sorted({2048 * n for n in NBLK} | {2048 * (n - 1) + 4 for n in NBLK} | {592704})
V17 = 2048 * 16 + 1028                                                 # 17 partial blocks, the last neither full nor nearly empty
DT = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 2e-5, torch.bfloat16: 1.5e-2, torch.float16: 2e-3}      # tests/test_gpu_ops.py


def _ops():
    from vae_segmentation_amd import ops
    return ops


def _planar(b, c, v):
    assert v % 4 == 0
    return (b, c, 1, 4, v // 4)


def _targets(g, kinds, shape, zero_plane):
    """'t': a softmax output or (every second one) a one-hot; 'l': a label volume, floats in 0..C-1"""
    b, c = shape[:2]
    out = []
    for j, kind in enumerate(kinds):
        if kind == "l":
            t = torch.randint(0, c, (b, 1) + tuple(shape[2:]), generator=g).float()
            if zero_plane is not None and c > 1:
                zb, zc = zero_plane
                t[zb][t[zb] == zc] = (zc + 1) % c
        else:
            t = torch.softmax(torch.randn(shape, generator=g) * 2, 1)
            if j % 2:
                t = L.hard_onehot(t).float()
            if zero_plane is not None:
                t[zero_plane] = 0
        out.append(t)
    return out


@functools.lru_cache(maxsize=2)
def _dls_case(shape, kinds, weights, bot, top, eps, zero_plane=None, seed=0):
    """inputs on the host and the restatement's loss, terms and gradients for them; shared by the two builds of a case"""
    g = torch.Generator().manual_seed(1000 * seed + shape[-1] + 7 * shape[0] + 13 * shape[1] + len(kinds))
    src = torch.softmax(torch.randn(shape, generator=g) * 2, 1)
    if zero_plane is not None:
        src[zero_plane] = 0
    tgts = _targets(g, kinds, shape, zero_plane)
    s64 = src.double().requires_grad_(True)
    t64 = [L.Label(t) if k == "l" else t.double().requires_grad_(True) for t, k in zip(tgts, kinds)]
    final, terms = L.dice_loss_sum(s64, t64, weights, bot, top, eps)
    final.backward()
    return {"src": src, "tgts": tgts, "final": final.item(), "terms": [t.item() for t in terms], "gs": s64.grad,
            "gts": [None if k == "l" else t.grad for t, k in zip(t64, kinds)]}


def _dls_gpu(ops, case, kinds, weights, bot, top, eps):
    s = case["src"].cuda().requires_grad_(True)
    tg = [t.cuda() if k == "l" else t.cuda().requires_grad_(True) for t, k in zip(case["tgts"], kinds)]
    final, terms = ops.dice_loss_sum(s, [(ops.LabelTarget(t) if k == "l" else t, w) for t, k, w in zip(tg, kinds, weights)], botindex=bot, topindex=top, eps=eps)
    final.backward()
    torch.cuda.synchronize()
    return final.detach(), [t.detach() for t in terms], s.grad, [None if k == "l" else t.grad for t, k in zip(tg, kinds)]


def _outside_is_zero(g, bot, top):
    return float(g[:, :bot].abs().sum()) == 0.0 and float(g[:, top:].abs().sum()) == 0.0


def _check_dls(ops, shape, kinds, weights, bot, top, eps, zero_plane=None, seed=0):
    case = _dls_case(tuple(shape), kinds, tuple(weights), bot, top, eps, zero_plane, seed)
    final, terms, gs, gts = _dls_gpu(ops, case, kinds, weights, bot, top, eps)
    what = "shape %s kinds %s w %s [%d, %d) eps %g" % (tuple(shape), kinds, weights, bot, top, eps)
    errs = [abs(a.item() - r) for a, r in zip(terms, case["terms"])]
    print(what, "final err %.3g" % abs(final.item() - case["final"]), "term errs", errs, "gs relerr %.3g" % L.relerr(gs.cpu(), case["gs"]))
    assert abs(final.item() - case["final"]) < 2e-6 * sum(abs(w) for w in weights), what
    assert max(errs) < 1e-6, what
    assert L.relerr(gs.cpu(), case["gs"]) < 1e-5 and _outside_is_zero(gs, bot, top), what
    for a, r in zip(gts, case["gts"]):
        assert (a is None) == (r is None)
        if r is not None:
            assert L.relerr(a.cpu(), r) < 1e-5 and _outside_is_zero(a, bot, top), what


# ---- DiceLossSum ---------------------------------------------------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize("v", PLANE_SIZES)
def test_dice_loss_sum_plane_sizes(v, lib_mode):
    """every count of partial blocks at which the finish kernel's loops change shape (module docstring), a tensor and a label target"""
    _check_dls(_ops(), _planar(2, 2, v), "tl", (0.1, 1.0), 1, 2, 1e-4)


@both
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_dice_loss_sum_targets_channels_batches(k, cfg, lib_mode):
    """K = 1..4 targets x every (C, bot, top) x B = 1, 2, 3, 5 at 17 partial blocks; over the grid both eps, targets that are all tensors / all
    labels / mixed, rotating unequal weights, and for B = 3 an all-zero plane pair; channels outside [bot, top) come back exactly zero"""
    c, bot, top = cfg
    for b in (1, 2, 3, 5):
        i = k + CFGS.index(cfg) + b
        kinds = ("t" * k, "l" * k, "".join("tl"[(j + i) % 2] for j in range(k)))[i % 3]
        weights = tuple((WEIGHTS[i % 4:] + WEIGHTS[:i % 4])[:k])
        _check_dls(_ops(), _planar(b, c, V17), kinds, weights, bot, top, (1e-6, 1e-4)[i % 2], zero_plane=(1, bot) if b == 3 else None)


@both
@pytest.mark.parametrize("b,cfg,k,nstat", [(5, (2, 1, 2), 1, 15), (2, (2, 1, 2), 4, 18), (1, (4, 1, 4), 3, 21), (2, (8, 0, 8), 4, 144), (1, (2, 1, 2), 1, 3)])
def test_dice_loss_sum_rounds_of_the_statistic_loop(b, cfg, k, nstat, lib_mode):
    """The finish kernel sums 16 statistics per round, batch x nc x (1 + 2K) in all.  1 + 2K is odd, so the count is never 16 (nor 17 with K <= 4): the
    nearest counts on either side of one full round are 15 (one round, a group idle) and 18 (a second round with two live groups); 144 is nine full
    rounds, 21 and 3 are ragged."""
    c, bot, top = cfg
    assert b * (top - bot) * (1 + 2 * k) == nstat
    _check_dls(_ops(), _planar(b, c, V17), "tltl"[:k], tuple(WEIGHTS[:k]), bot, top, 1e-4, seed=1)
    _check_dls(_ops(), _planar(b, c, 2048 * 129), "ttll"[:k], tuple(WEIGHTS[:k]), bot, top, 1e-6, seed=1)


@both
def test_dice_loss_sum_all_zero_plane_pair(lib_mode):
    """a (b, c) plane that is zero in the source and in every target: 0 / eps = 0, a finite loss and finite gradients equal to the restatement's"""
    ops = _ops()
    for eps in (1e-6, 1e-4):
        _check_dls(ops, _planar(2, 2, V17), "tl", (1.0, 0.1), 1, 2, eps, zero_plane=(0, 1), seed=2)
        _check_dls(ops, _planar(1, 4, 2052), "tt", (0.1, 1.0), 0, 4, eps, zero_plane=(0, 2), seed=2)


@both
def test_dice_loss_sum_limits(lib_mode):
    """batch 64 with two channels works; batch 65 and batch x nc = 129 are refused with an error, not answered"""
    from vae_segmentation_amd._lib import VaesegError
    ops = _ops()
    _check_dls(ops, _planar(64, 2, 2052), "t", (1.0,), 0, 2, 1e-4, seed=3)
    for b, c in ((65, 2), (43, 3)):
        s = torch.rand(_planar(b, c, 8), device="cuda")
        with pytest.raises(VaesegError):
            ops.dice_loss_sum(s, [(s.clone(), 1.0)], botindex=0, topindex=c, eps=1e-4)


# ---- Dice ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dice_case(shape, bot, top, eps, seed=0):
    g = torch.Generator().manual_seed(77 + seed + shape[-1] + shape[1])
    s = torch.softmax(torch.randn(shape, generator=g) * 2, 1)
    t = torch.softmax(torch.randn(shape, generator=g) * 2, 1)
    wgt = torch.tensor([0.3, -0.7, 1.1, 0.45, 2.0])[:shape[0]].double()
    ref = {}
    for rm in (True, False):
        s64, t64 = s.double().requires_grad_(True), t.double().requires_grad_(True)
        d = L.dice_planes(s64, t64, bot, top, eps)
        val = d["mean"] if rm else d["per_sample"]
        (val * (1.0 if rm else wgt)).sum().backward()
        ref[rm] = (val.detach(), s64.grad, t64.grad)
    return s, t, wgt, ref


def _check_dice(fn, shape, bot, top, eps, seed=0):
    """fn(s, t, return_mean) -> the Dice value(s); value and both gradients against the restatement, mean and weighted per-sample form"""
    s, t, wgt, ref = _dice_case(tuple(shape), bot, top, eps, seed)
    for rm in (True, False):
        sg, tg = s.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
        got = fn(sg, tg, rm)
        (got * (1.0 if rm else wgt.float().cuda())).sum().backward()
        torch.cuda.synchronize()
        val, gs, gt = ref[rm]
        what = "shape %s [%d, %d) eps %g mean %s" % (tuple(shape), bot, top, eps, rm)
        print(what, "value err %.3g" % float((got.detach().cpu().double() - val).abs().max()), "relerr %.3g %.3g" % (L.relerr(sg.grad.cpu(), gs), L.relerr(tg.grad.cpu(), gt)))
        assert got.shape == val.shape and float((got.detach().cpu().double() - val).abs().max()) < 1e-6, what
        assert L.relerr(sg.grad.cpu(), gs) < 1e-5 and L.relerr(tg.grad.cpu(), gt) < 1e-5, what
        assert _outside_is_zero(sg.grad, bot, top) and _outside_is_zero(tg.grad, bot, top), what


@both
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("v", [512, 8192, 8196, 13824])
def test_dice_plane_sizes_and_channel_ranges(v, cfg, lib_mode):
    from vae_segmentation_amd import evaluation as E
    ops = _ops()
    c, bot, top = cfg
    eps = 1e-6 if (v + c) % 8 else 1e-4
    _check_dice(lambda s, t, rm: E.avg_dsc({"s": s, "t": t}, "s", "t", botindex=bot, topindex=top, return_mean=rm, eps=eps), _planar(3, c, v), bot, top, eps)
    _check_dice(lambda s, t, rm: ops.Dice.apply(s, t, bot, top, eps, rm), _planar(2, c, v), bot, top, eps, seed=1)


def _scores_with_ties_and_nans(b, c, v, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(b, c, 1, 4, v // 4, generator=g)
    flat = x.view(b, c, v)
    flat[:, :, ::3] = torch.round(flat[:, :, ::3] * 4) / 4                  # every third voxel on a grid of five values: ties between channels, maxima included
    flat[0, :, 5] = 0.5                                                      # every channel equal
    flat[:, c - 1, 7::11] = float("nan")                                     # a NaN channel
    flat[:, 1, 7::22] = float("nan")                                         # two of them at every second such voxel: the first wins
    flat[b - 1, 0, 40] = float("inf")
    return x


@both
@pytest.mark.parametrize("c", [4, 8])
def test_hard_dice_with_ties_and_a_nan_channel(c, lib_mode):
    """avg_dsc(binary=True) — the validation number — on scores with deliberate ties and NaNs, against the restatement's argmax"""
    from vae_segmentation_amd import evaluation as E
    ops = _ops()
    s, t = _scores_with_ties_and_nans(2, c, 4100, 1), _scores_with_ties_and_nans(2, c, 4100, 2)
    hs, ht = L.hard_onehot(s), L.hard_onehot(t)
    assert torch.equal(ops.hard_onehot(s.cuda()).cpu().double(), hs) and torch.equal(ops.hard_onehot(t.cuda()).cpu().double(), ht)
    for bot, top in ((1, c), (0, c), (2, 3)):
        for rm in (True, False):
            d = L.dice_planes(hs, ht, bot, top, 1e-6)
            got = E.avg_dsc({"s": s.cuda(), "t": t.cuda()}, "s", "t", binary=True, botindex=bot, topindex=top, return_mean=rm)
            assert float((got.cpu().double() - (d["mean"] if rm else d["per_sample"])).abs().max()) < 1e-6


# ---- the one large case --------------------------------------------------------------------------------------------------------------------------
V_LARGE = 208 ** 3


@functools.lru_cache(maxsize=1)
def _large_case():
    g = torch.Generator().manual_seed(208)
    s, t = torch.rand(_planar(1, 1, V_LARGE), generator=g), (torch.rand(_planar(1, 1, V_LARGE), generator=g) > 0.7).float()
    s64, t64 = s.double().requires_grad_(True), t.double().requires_grad_(True)
    d = L.dice_planes(s64, t64, 0, 1, 1e-4)["mean"]
    d.backward()
    return s, t, d.item(), s64.grad, t64.grad


@both
def test_dice_and_dice_loss_sum_at_the_block_caps(lib_mode):
    """B = C = 1, 208^3 voxels: the 1,024-block cap of dice_sums_kernel (atomic build), the 2,048-block caps of both backward kernels, and a partial
    kernel whose every block makes 17 or 18 trips"""
    ops = _ops()
    s, t, dice, gs, gt = _large_case()
    sg, tg = s.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    got = ops.Dice.apply(sg, tg, 0, 1, 1e-4, True)
    got.backward()
    assert abs(got.item() - dice) < 1e-6
    assert L.relerr(sg.grad.cpu(), gs) < 1e-5 and L.relerr(tg.grad.cpu(), gt) < 1e-5
    sg.grad = tg.grad = None
    final, terms = ops.dice_loss_sum(sg, [(tg, 0.7)], botindex=0, topindex=1, eps=1e-4)
    final.backward()
    assert abs(terms[0].item() - (1 - dice)) < 1e-6 and abs(final.item() - 0.7 * (1 - dice)) < 2e-6 * 0.7
    assert L.relerr(sg.grad.cpu(), -0.7 * gs) < 1e-5 and L.relerr(tg.grad.cpu(), -0.7 * gt) < 1e-5


# ---- any voxel count -----------------------------------------------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize("vol", [(33, 47, 29), (5, 9, 33), (1, 1, 1), (1, 1, 2), (1, 1, 3)])
def test_voxel_counts_that_are_no_multiple_of_four(vol, lib_mode):
    """avg_dsc (soft and binary) and dice_loss_sum (tensor and label targets) on planes that are no whole number of 16-byte quads: the values and
    gradients of the restatement on the unpadded data, gradients in the caller's shape"""
    from vae_segmentation_amd import evaluation as E
    ops = _ops()
    shape = (2, 3) + vol
    _check_dice(lambda s, t, rm: E.avg_dsc({"s": s, "t": t}, "s", "t", botindex=1, topindex=3, return_mean=rm, eps=1e-6), shape, 1, 3, 1e-6)
    s, t, _, _ = _dice_case(shape, 1, 3, 1e-6)
    d = L.dice_planes(L.hard_onehot(s), L.hard_onehot(t), 1, 3, 1e-6)["mean"]
    got = E.avg_dsc({"s": s.cuda(), "t": t.cuda()}, "s", "t", binary=True, botindex=1, topindex=3)
    assert abs(got.item() - d.item()) < 1e-6
    _check_dls(ops, shape, "tl", (0.1, 1.0), 1, 3, 1e-4)
    _check_dls(ops, shape, "lt", (-0.37, 2.5), 0, 2, 1e-6)
    ops.FUSED_LOSS[0] = False                                              # the spelling with Dice.apply per term
    try:
        _check_dls(ops, shape, "tl", (0.1, 1.0), 1, 3, 1e-4)
    finally:
        ops.FUSED_LOSS[0] = True


@both
def test_whole_quads_take_the_unpadded_path_and_padding_is_the_old_padding(lib_mode):
    """a multiple-of-4 volume gives the bits of Dice.apply on the pre-flattened tensor; evaluation.dice on any size gives the bits of Dice.apply on
    the tensor padded by hand (what it did itself before ops.Dice padded)"""
    from vae_segmentation_amd import evaluation as E
    ops = _ops()
    g = torch.Generator().manual_seed(4)
    s, t = torch.softmax(torch.randn(2, 2, 6, 10, 7, generator=g), 1), torch.softmax(torch.randn(2, 2, 6, 10, 7, generator=g), 1)
    res = []
    for view in ((2, 2, 6, 10, 7), (2, 2, 1, 1, 420)):
        sg, tg = s.view(view).cuda().requires_grad_(True), t.view(view).cuda().requires_grad_(True)
        if len(res) == 0:
            got = E.avg_dsc({"s": sg, "t": tg}, "s", "t", botindex=1, topindex=2, eps=1e-4)
        else:
            got = ops.Dice.apply(sg, tg, 1, 2, 1e-4, True)
        got.backward()
        assert sg.grad.shape == sg.shape
        res.append((got.detach(), sg.grad.reshape(-1), tg.grad.reshape(-1)))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    a, b = torch.rand(5, 9, 33, generator=g).cuda().requires_grad_(True), (torch.rand(5, 9, 33, generator=g) > 0.5).float().cuda()
    got = E.dice(a, b)
    got.backward()
    ap = torch.nn.functional.pad(a.detach().reshape(1, 1, -1), (0, 3)).requires_grad_(True)
    want = ops.Dice.apply(ap, torch.nn.functional.pad(b.reshape(1, 1, -1), (0, 3)), 0, 1, 1e-6, True)
    want.backward()
    assert torch.equal(got.detach(), want.detach()) and torch.equal(a.grad.reshape(-1), ap.grad.reshape(-1)[:5 * 9 * 33])


# ---- BCE -----------------------------------------------------------------------------------------------------------------------------------------
PLANTED = [(p, t) for t in (1.0, 0.0) for p in (0.0, 1.0, 1e-45, 1.0 - 2.0 ** -24, 0.5)]


@both
@pytest.mark.parametrize("count", [1, 255, 256, 257, 4096, 4097, 70001])
def test_bce_counts_and_saturated_probabilities(count, lib_mode):
    """one block or several (atomic build: 4,097 is two, 70,001 eighteen), counts around the block size, and probabilities of exactly 0 and 1, the
    smallest subnormal, the largest value below 1 and 0.5 against both target values: the -100 clamp and the 1e-12 floor of the backward"""
    ops = _ops()
    g = torch.Generator().manual_seed(count)
    p = torch.sigmoid(torch.randn(count, generator=g) * 3)
    t = (torch.rand(count, generator=g) > 0.5).float()
    where = torch.linspace(0, count - 1, len(PLANTED)).long() if count >= len(PLANTED) else torch.zeros(1, dtype=torch.long)
    for i, (pv, tv) in zip(where.tolist(), PLANTED):
        p[i], t[i] = pv, tv
    assert count == 1 or (float(p.min()) == 0.0 and float(p.max()) == 1.0)
    pg = p.cuda().requires_grad_(True)
    got = ops.BCE.apply(pg, t.cuda())
    got.backward()
    ref, gref = L.bce(p, t), L.bce_grad(p, t)
    print(count, "bce rel err %.3g" % (abs(got.item() - ref.item()) / ref.item()), "grad relerr %.3g" % L.relerr(pg.grad.cpu(), gref))
    assert abs(got.item() - ref.item()) < 2e-6 * abs(ref.item())
    assert bool(torch.isfinite(pg.grad).all()) and L.relerr(pg.grad.cpu(), gref) < 1e-5
    inner = (p * (1 - p)) > 1e-6                                           # the saturated entries' 1e12 / N would hide every other one in the norm
    if bool(inner.any()):
        assert L.relerr(pg.grad.cpu()[inner], gref[inner]) < 1e-5


# ---- KL and reparameterisation -------------------------------------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize("batch,dim", [(1, 1), (2, 128), (3, 100), (7, 37), (16, 512)])
def test_kl_and_reparam(batch, dim, lib_mode):
    """batch x dim around the 256-thread block, stds of exactly 0 (the log(1e-5) branch, a gradient of -1e5) and 1e-7; both gradients, and each alone"""
    ops = _ops()
    g = torch.Generator().manual_seed(batch * 1000 + dim)
    mean, std, noise = torch.randn(batch, dim, generator=g), torch.rand(batch, dim, generator=g) + 0.05, torch.randn(batch, dim, generator=g)
    std.view(-1)[::7] = 0.0
    std.view(-1)[3::11] = 1e-7
    m64, s64 = mean.double().requires_grad_(True), std.double().requires_grad_(True)
    ref = L.kl(m64, s64)
    (ref * 0.6).backward()
    mg, sg = mean.cuda().requires_grad_(True), std.cuda().requires_grad_(True)
    got = ops.KL.apply(mg, sg)
    (got * 0.6).backward()
    assert abs(got.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert L.relerr(mg.grad.cpu(), m64.grad) < 1e-5 and L.relerr(sg.grad.cpu(), s64.grad) < 1e-5
    inner = std > 1e-3                                                     # without the -1e5 entries in the norm
    if bool(inner.any()):
        assert L.relerr(sg.grad.cpu()[inner], s64.grad[inner]) < 1e-5
    for which in (0, 1):                                                   # needs_input_grad on one operand only
        mo, so = mean.cuda().requires_grad_(which == 0), std.cuda().requires_grad_(which == 1)
        (ops.KL.apply(mo, so) * 0.6).backward()
        live, dead, want = (mo, so, m64.grad) if which == 0 else (so, mo, s64.grad)
        assert dead.grad is None and L.relerr(live.grad.cpu(), want) < 1e-5
    # z = mean + noise * std * scale
    m64, s64 = mean.double().requires_grad_(True), std.double().requires_grad_(True)
    gz = torch.randn(batch, dim, generator=g)
    zr = L.reparam(m64, s64, noise, 0.35)
    zr.backward(gz.double())
    mg, sg = mean.cuda().requires_grad_(True), std.cuda().requires_grad_(True)
    z = ops.Reparam.apply(mg, sg, noise.cuda(), 0.35)
    z.backward(gz.cuda())
    assert L.relerr(z.detach().cpu(), zr.detach()) < 1e-6
    assert L.relerr(mg.grad.cpu(), m64.grad) < 1e-6 and L.relerr(sg.grad.cpu(), s64.grad) < 1e-6
    mo = mean.cuda().requires_grad_(True)
    ops.Reparam.apply(mo, std.cuda(), noise.cuda(), 0.35).backward(gz.cuda())
    assert torch.equal(mo.grad, gz.cuda())


# ---- the n-class softmax pass --------------------------------------------------------------------------------------------------------------------
def _to_cl(x, cp, dtype, pad_fill):
    """planar (n, c, 1, 1, v) -> channels-last (n, 1, 1, v, cp) in the kernel dtype; the padded lanes hold NaN at even voxels and pad_fill at odd ones"""
    n, c = x.shape[:2]
    out = torch.full((n,) + tuple(x.shape[2:]) + (cp,), float("nan"), dtype=torch.float32)
    out[..., 1::2, c:] = pad_fill
    out[..., :c] = x.permute(0, 2, 3, 4, 1)
    return out.to(dtype).cuda().contiguous()


@both
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cp", [8, 16])
@pytest.mark.parametrize("nc", [1, 2, 3, 5, 8])
def test_softmax_pass_large_logits_and_garbage_in_the_padded_lanes(nc, cp, dtype, lib_mode):
    """vs_softmax_cl_fwd / _bwd, drop_p = 0: logits of magnitude 80 (and 300; 6e4 in fp16 storage) whose channels differ by a few units — the maximum
    has to be subtracted before the exponential —, NaN and the dtype's maximum in the padded input lanes, 1 / 255 / 4,097 voxels per sample"""
    ops = _ops()
    from vae_segmentation_amd._lib import check, lib
    n = 3
    big = float(torch.finfo(dtype).max)
    for vox in (1, 255, 4097):
        for scale in (80.0, 300.0) + ((6e4,) if dtype == torch.float16 else ()):
            g = torch.Generator().manual_seed(int(vox + scale + nc))
            logits = (torch.rand(n, 1, 1, 1, vox, generator=g) * 2 - 1) * scale + torch.randn(n, nc, 1, 1, vox, generator=g) * 2
            gp = torch.randn(n, nc, 1, 1, vox, generator=g)
            l_cl = _to_cl(logits, cp, dtype, big)
            lq = logits.to(dtype).double().requires_grad_(True)            # the storage-rounded logits
            p_ref = L.softmax(lq, nc)
            (p_ref * gp.double()).sum().backward()
            prob = torch.empty((n, nc, 1, 1, vox), dtype=torch.float32, device="cuda")
            check(lib.vs_softmax_cl_fwd(l_cl.data_ptr(), prob.data_ptr(), n, vox, cp, nc, ops.vs_dtype(l_cl), 0.0, 0, None), "softmax_cl_fwd")
            gl = torch.full((n, 1, 1, vox, cp), 9.0, dtype=dtype, device="cuda")
            check(lib.vs_softmax_cl_bwd(prob.data_ptr(), gp.cuda().contiguous().data_ptr(), gl.data_ptr(), n, vox, cp, nc, ops.vs_dtype(l_cl), 0.0, 0, None),
                  "softmax_cl_bwd")
            torch.cuda.synchronize()
            what = "nc %d cp %d %s vox %d scale %g" % (nc, cp, dtype, vox, scale)
            assert bool(torch.isfinite(prob).all()), what
            assert float((prob.cpu().double() - p_ref.detach()).abs().max()) < 1e-6, what
            assert float((prob.double().sum(1) - 1).abs().max()) < 1e-6, what
            got = gl.float().cpu()[..., :nc].permute(0, 4, 1, 2, 3)
            assert L.relerr(got, lq.grad) < TOL[dtype], what
            assert float(gl[..., nc:].float().abs().sum()) == 0.0, what


# ---- label helpers -------------------------------------------------------------------------------------------------------------------------------
@both
def test_label_helpers_are_exact(lib_mode):
    """onehot, hard_onehot, binarize and confident_binarize at 4,097 voxels and three samples: equality with the restatement, with labels that truncate
    (1.9 -> 1, -0.5 -> 0, -1 -> no class) and values exactly on 0.5, lo and hi and one step either side"""
    from vae_segmentation_amd import evaluation as E
    ops = _ops()
    n, v = 3, 4097
    g = torch.Generator().manual_seed(9)
    for c in (2, 4):
        lab = torch.randint(0, c, (n, 1, 1, 1, v), generator=g).float()
        lab.view(n, v)[:, 1::5] += 0.9
        lab.view(n, v)[:, 2::9] = -0.5
        lab.view(n, v)[:, 4::13] = -1.0
        lab.view(n, v)[:, v - 1] = 1.9
        hot = ops.onehot(lab.cuda(), c)
        assert hot.shape == (n, c, 1, 1, v) and torch.equal(hot.cpu().double(), L.onehot(lab, c))
    for c in (1, 3, 8):
        x = _scores_with_ties_and_nans(n, c, 4100, 30 + c).view(n, c, 1, 1, 4100)[..., :v].contiguous() if c > 1 else torch.rand(n, 1, 1, 1, v, generator=g)
        assert torch.equal(ops.hard_onehot(x.cuda()).cpu().double(), L.hard_onehot(x))
    a = torch.rand(n, 1, 1, 1, v, generator=g)
    edge = torch.tensor([0.5, 0.2, 0.8])
    marks = torch.cat([edge, torch.nextafter(edge, torch.zeros(3)), torch.nextafter(edge, torch.ones(3)), torch.tensor([0.0, 1.0, -0.0, 1.5, -2.0])])
    a.view(n, v)[:, :len(marks)] = marks
    a.view(n, v)[:, v - len(marks):] = marks
    assert torch.equal(E.binarize(a.cuda()).cpu().double(), L.binarize(a))
    assert torch.equal(E.confident_binarize(a.cuda()).cpu().double(), L.confident_binarize(a))
    assert torch.equal(E.confident_binarize(a.cuda(), max=0.7, min=0.5).cpu().double(), L.confident_binarize(a, hi=0.7, lo=0.5))


# ---- reproducibility -----------------------------------------------------------------------------------------------------------------------------
def _bits(ts):
    return [None if t is None else t.detach().clone() for t in ts]


@both
def test_dice_loss_sum_is_bit_reproducible_and_graph_replay_equals_eager(lib_mode):
    """no atomics and a fixed summation order (the comment above DICE_MULTI_BLOCKS): value, terms and gradients have the same bits on two runs and on
    the replay of a captured graph, in both builds; 129 partial blocks"""
    ops = _ops()
    shape, kinds, weights = _planar(2, 2, 2048 * 129), "tl", (0.1, 1.0)
    case = _dls_case(shape, kinds, weights, 1, 2, 1e-4)
    s = case["src"].cuda().requires_grad_(True)
    t0, lab = case["tgts"][0].cuda().requires_grad_(True), case["tgts"][1].cuda()

    def step():
        s.grad = t0.grad = None
        final, terms = ops.dice_loss_sum(s, [(t0, weights[0]), (ops.LabelTarget(lab), weights[1])], botindex=1, topindex=2, eps=1e-4)
        final.backward()
        return [final] + list(terms) + [s.grad, t0.grad]

    first = _bits(step())
    again = _bits(step())
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, out))


def test_dice_is_bit_reproducible_in_the_deterministic_build():
    ops = _ops()
    assert ops.is_deterministic()
    s, t, _, _ = _dice_case(_planar(2, 2, 13824), 0, 2, 1e-6)
    runs = []
    for _ in range(2):
        sg, tg = s.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
        per = ops.Dice.apply(sg, tg, 0, 2, 1e-6, False)
        per.sum().backward()
        runs.append(_bits([per, sg.grad, tg.grad]))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
