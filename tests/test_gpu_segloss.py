"""The compound segmentation loss (csrc/segloss.hip: ops.seg_loss, ops.SegLoss, train.seg_train_losses(loss=...), --seg_loss dice_ce) against its fp64
restatement (tests/segloss_util.py, pinned on the host by tests/test_host_segloss.py), in both builds.  Inputs are planar fp32 probabilities
(B, C, 1, 4, V / 4) and labels (B, 1, 1, 4, V / 4), so the voxel count V of a plane is set directly.

Units of work of the kernels, in quads (16 bytes = 4 voxels) of a plane: a lane takes one quad per trip, a wave 64, a workgroup 256; both grids hold
nblk = min(ceil(quads / 256), SEG_BLOCKS = 512) workgroups per sample, so a sweep of the grid-stride loop covers 131,072 quads at the cap.  The finish
kernel gives 16 threads to a statistic, each walking blk = sl, sl + 16, ...: its eight-way unrolled loop runs while blk + 112 < nblk.
Branch reached by each plane size (QUADS below, V = 4 quads):
  quads      1              V = 4: one lane of one wave works; three waves add zeros in the LDS stage; nblk 1
  quads     63, 64, 65      a wave's step: one lane idle, the wave exactly full, one lane of the second wave
  quads    255, 256, 257    a workgroup's chunk: one lane short, exactly full (nblk 1), a second workgroup holding a single quad (nblk 2)
  quads   4097              nblk 17: the finish kernel's remainder loop makes a second pass for lane 0 alone
  quads  33024              nblk 129: its unrolled loop is entered once and lane 0 makes one remainder pass
  quads 131071, 131072      nblk 512, the block cap: the last lane of the last workgroup idle / every lane exactly one trip; the unrolled loop runs 4 times
  quads 131073              one quad past the cap: the grid-stride loop wraps, lane 0 of workgroup 0 makes a second trip
The largest plane holds 524,292 voxels.

Tolerances follow from the arithmetic, none is measured: every sum is fp64 over exactly promoted fp32 values (about 1e-16 N relative, far below fp32's
6e-8) and each output is rounded to fp32 once: terms within 1e-6 max(1, |value|); final — two fp32 products and a sum of once-rounded terms — within
2e-6 (|dice_weight| + |ce_weight| max(1, ce_term)); gradients norm-wise relative error < 1e-6; exactly 0 at ignored voxels and, where ce_weight == 0, outside
[bot, top)."""
import functools
import itertools
import os
import subprocess
import sys

import pytest
import torch

from tests import segloss_util as SU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

both = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
QUADS = [1, 63, 64, 65, 255, 256, 257, 4097, 33024, 131071, 131072, 131073]
CFGS = [(1, 0, 1), (2, 1, 2), (3, 1, 3), (8, 1, 8), (8, 2, 5)]          # (C, bot, top)
MODE_A = dict(dice_weight=1.0, ce_weight=1.0, batch_dice=False, gamma=0.0, class_weights=None)
MODE_B = dict(dice_weight=0.6, ce_weight=1.7, batch_dice=True, gamma=2.0, class_weights="ramp")


def _ops():
    from vae_segmentation_amd import ops
    return ops


def _weights(kind, c):
    """None, or unequal class weights with a zero (the last class's) where there is more than one class"""
    if kind is None:
        return None
    return [0.5 + 0.75 * k if (k < c - 1 or c == 1) else 0.0 for k in range(c)]


def _labels(g, b, c, v, kind):
    lab = torch.randint(0, c, (b, 1, 1, 1, v), generator=g).float()
    r = torch.rand(lab.shape, generator=g)
    if kind == "mixed":                       # every sort of ignored value, a tenth of the voxels (at least one of each where the plane has room)
        for j, bad in enumerate((-1.0, 255.0, float("nan"), float(c), -0.5)):
            lab[(r >= 0.02 * j) & (r < 0.02 * (j + 1))] = bad
            if v > j:
                lab[0, 0, 0, 0, j] = bad
        frac = (r >= 0.5) & (r < 0.6)
        lab[frac] = lab[frac] + 0.5           # 0.5, 1.5, ...: valid, class = the truncation
        if v > 5:
            lab[-1, 0, 0, 0, 5] = 0.5
    elif kind == "half":
        lab[r < 0.5] = 255.0
    elif kind == "all_ignored":
        lab[r < 0.5] = -1.0
        lab[r >= 0.5] = float("nan")
    elif kind == "absent":                    # the last class absent from sample 0
        lab[0][lab[0] == c - 1] = 0.0
    elif kind == "background":                # the last sample entirely background
        lab[-1] = 0.0
    else:
        assert kind == "plain"
    return lab


@functools.lru_cache(maxsize=4)
def _case(b, c, v, bot, top, eps, mode, kind="mixed", hard=False, seed=0):
    """inputs on the host and the restatement's loss, terms and gradient for them; shared by the two builds of a case"""
    mode = dict(mode)
    g = torch.Generator().manual_seed(100003 * seed + v + 7 * b + 13 * c + 3 * bot)
    p = torch.softmax(torch.randn(b, c, 1, 1, v, generator=g) * 2, 1)
    lab = _labels(g, b, c, v, kind)
    if hard:                                  # exact 0 and 1 at labelled voxels: p_l = 1 on about a third, p_l = 0 on about a third (C > 1)
        r = torch.rand(b, 1, 1, 1, v, generator=g)
        valid, cls = SU.classify(lab, c)
        cls = cls.reshape(b, 1, 1, 1, v)
        hit = torch.zeros_like(p).scatter_(1, cls, 1.0)
        miss = torch.zeros_like(p).scatter_(1, (cls + 1) % c, 1.0)
        p = torch.where(r < 0.33, hit, torch.where((r < 0.66) & (c > 1), miss, p))
    shape = (b, c, 1, 4, v // 4) if v % 4 == 0 else (b, c, 1, 1, v)
    p, lab = p.reshape(shape), lab.reshape((b, 1) + shape[2:])
    mode["class_weights"] = _weights(mode["class_weights"], c)
    p64 = p.double().requires_grad_(True)
    final, (d, ce) = SU.seg_loss(p64, lab, bot=bot, top=top, eps=eps, **mode)
    final.backward()
    return {"p": p, "lab": lab, "final": final.item(), "dice": d.item(), "ce": ce.item(), "grad": p64.grad, "mode": mode,
            "valid": SU.classify(lab, c)[0].reshape((b, 1) + shape[2:])}


def _gpu(ops, case, bot, top, eps, scale=None):
    p = case["p"].cuda().requires_grad_(True)
    final, (d, ce) = ops.seg_loss(p, ops.LabelTarget(case["lab"].cuda()), botindex=bot, topindex=top, eps=eps, **case["mode"])
    assert not d.requires_grad and not ce.requires_grad
    (final if scale is None else final * scale).backward()
    torch.cuda.synchronize()
    return final.detach(), d, ce, p.grad


def _check(ops, b, c, v, bot, top, eps, mode, kind="mixed", hard=False, seed=0, scale=None):
    case = _case(b, c, v, bot, top, eps, tuple(sorted(mode.items())), kind, hard, seed)
    final, d, ce, gp = _gpu(ops, case, bot, top, eps, scale)
    m = case["mode"]
    what = "B %d C %d V %d [%d, %d) eps %g %s labels %s hard %s" % (b, c, v, bot, top, eps, m, kind, hard)
    want = case["grad"] if scale is None else case["grad"] * float(scale)
    gmax = float(want.abs().max())
    gerr = SU.relerr(gp.cpu(), want) if gmax > 0 else float(gp.abs().max())
    print(what, "final %.9g (%.3g off) dice %.9g (%.3g off) ce %.9g (%.3g off) grad relerr %.3g"
          % (final.item(), abs(final.item() - case["final"]), d.item(), abs(d.item() - case["dice"]), ce.item(), abs(ce.item() - case["ce"]), gerr))
    assert gp.shape == case["p"].shape and gp.dtype == torch.float32
    assert abs(d.item() - case["dice"]) <= 1e-6 * max(1.0, abs(case["dice"])), what
    assert abs(ce.item() - case["ce"]) <= 1e-6 * max(1.0, abs(case["ce"])), what
    assert abs(final.item() - case["final"]) <= 2e-6 * (abs(m["dice_weight"]) + abs(m["ce_weight"]) * max(1.0, case["ce"])), what
    assert torch.isfinite(gp).all(), what
    if gmax > 0:
        assert gerr < 1e-6, what
    else:
        assert float(gp.abs().max()) == 0.0, what
    assert float((gp.cpu() * (~case["valid"]).float()).abs().max()) == 0.0, what          # exactly 0 at every ignored voxel, in every channel
    if m["ce_weight"] == 0 and c > 1:
        assert float(gp[:, :bot].abs().sum()) == 0.0 and float(gp[:, top:].abs().sum()) == 0.0, what
    return case, (final, d, ce, gp)


@both
@pytest.mark.parametrize("quads", QUADS)
def test_plane_sizes(quads, lib_mode):
    ops = _ops()
    for mode in (MODE_A, MODE_B):
        _check(ops, 2, 3, 4 * quads, 1, 3, 1e-4, mode)


@both
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("b", [1, 2, 3])
def test_batch_and_channel_configurations(b, cfg, lib_mode):
    """321 quads: two workgroups per sample, the second one partly filled"""
    ops = _ops()
    c, bot, top = cfg
    for mode in (MODE_A, MODE_B):
        _check(ops, b, c, 4 * 321, bot, top, 1e-6, mode)


@both
@pytest.mark.parametrize("v", [1, 7, 4097])
def test_plane_sizes_that_are_no_multiple_of_four_are_padded(v, lib_mode):
    """ops.seg_loss pads p with 0 and the label with -1 (_pad_quads): the padding is ignored by every term and its gradient dropped"""
    ops = _ops()
    for mode in (MODE_A, MODE_B):
        _check(ops, 2, 3, v, 1, 3, 1e-6, mode, kind="plain" if v == 1 else "mixed")


@both
def test_modes(lib_mode):
    """both Dice modes x ce_weight 0 / not x dice_weight 0 / not x gamma 0 / 2 x class weights equal / unequal with a zero; 257 quads"""
    ops = _ops()
    for bd, cw, dw, gamma, w in itertools.product((False, True), (0.0, 0.7), (0.0, 1.3), (0.0, 2.0), (None, "ramp")):
        _check(ops, 2, 3, 4 * 257, 1, 3, 1e-6, dict(dice_weight=dw, ce_weight=cw, batch_dice=bd, gamma=gamma, class_weights=w))


@both
@pytest.mark.parametrize("kind", ["mixed", "half", "all_ignored", "absent", "background"])
def test_labels(kind, lib_mode):
    ops = _ops()
    for mode in (MODE_A, MODE_B, dict(MODE_A, ce_weight=0.0), dict(MODE_A, ce_weight=0.0, batch_dice=True)):
        case, (final, d, ce, gp) = _check(ops, 2, 3, 4 * 300, 1, 3, 1e-6, mode, kind=kind)
        if kind == "all_ignored":
            assert ce.item() == 0.0 and float(gp.abs().max()) == 0.0
            if not mode["batch_dice"]:
                assert d.item() == 1.0 and final.item() == torch.tensor(mode["dice_weight"], dtype=torch.float32).item()      # dice_weight * 1
        if kind == "background":
            # a sample without foreground: no gradient at all from per-sample Dice alone; batch Dice and the cross-entropy both reach it
            if mode["ce_weight"] == 0 and not mode["batch_dice"]:
                assert float(gp[-1].abs().max()) == 0.0 and float(gp[0].abs().max()) > 0
            else:
                assert float(gp[-1].abs().max()) > 0
                assert SU.relerr(gp[-1].cpu(), case["grad"][-1]) < 1e-6


@both
@pytest.mark.parametrize("cfg", [(1, 0, 1), (3, 1, 3)])
def test_probabilities_of_exactly_zero_and_one(cfg, lib_mode):
    """p_l = 0: ln p clamped at -100, the logarithm's derivative 0 there; p_l = 1: f = 0"""
    ops = _ops()
    c, bot, top = cfg
    for mode in (MODE_A, MODE_B):
        case, (final, d, ce, gp) = _check(ops, 2, c, 4 * 300, bot, top, 1e-6, mode, kind="half", hard=True)
        if c > 1:
            assert case["ce"] > 10.0           # a third of the labelled voxels cost 100 each before weighting


@both
@pytest.mark.parametrize("scale", [1024.0, 0.37])
def test_upstream_gradient_is_read_on_the_device(scale, lib_mode):
    """a LossScaler multiplies the loss by a device scalar: gout is that scalar, not 1"""
    ops = _ops()
    s = torch.tensor(scale, device="cuda")
    for mode in (MODE_A, MODE_B):
        _check(ops, 2, 3, 4 * 300, 1, 3, 1e-6, mode, scale=s, seed=1)


def _bits(ts):
    return [t.detach().clone() for t in ts]


def test_graph_replay_and_the_two_builds_give_the_bits_of_an_eager_call():
    """forward and backward captured once, replayed three times on fresh inputs: torch.equal to eager calls; and the atomic build's results are the
    deterministic build's (neither has an atomic in these kernels).  513 workgroups wanted, 512 launched: the loops wrap"""
    ops = _ops()
    b, c, v = 2, 3, 4 * 131073
    cases = [_case(b, c, v, 1, 3, 1e-4, tuple(sorted(MODE_B.items())), "mixed", False, seed) for seed in (11, 12, 13)]
    kw = dict(cases[0]["mode"], botindex=1, topindex=3, eps=1e-4)
    p = torch.zeros_like(cases[0]["p"]).cuda().requires_grad_(True)
    lab = torch.zeros_like(cases[0]["lab"]).cuda()

    def step():
        p.grad = None
        final, terms = ops.seg_loss(p, ops.LabelTarget(lab), **kw)
        final.backward()
        return [final, terms[0], terms[1], p.grad]

    def load(case):
        with torch.no_grad():
            p.copy_(case["p"])
            lab.copy_(case["lab"])

    results = {}
    for det in (True, False):
        was = ops.is_deterministic()
        ops.set_deterministic(det)
        try:
            eager = []
            for case in cases:
                load(case)
                eager.append(_bits(step()))
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = step()
            for case, want in zip(cases, eager):
                load(case)
                graph.replay()
                torch.cuda.synchronize()
                assert all(torch.equal(a, w) for a, w in zip(out, want))
            results[det] = eager
            del graph
        finally:
            ops.set_deterministic(was)
    for a, w in zip(results[True], results[False]):
        assert all(torch.equal(x, y) for x, y in zip(a, w))
    assert abs(results[True][0][0].item() - cases[0]["final"]) <= 2e-6 * (0.6 + 1.7 * max(1.0, cases[0]["ce"]))


@both
def test_argument_errors(lib_mode):
    import ctypes
    from vae_segmentation_amd._lib import VaesegError, lib
    ops = _ops()
    p = torch.softmax(torch.randn(2, 3, 1, 4, 8, device="cuda"), 1)
    lab = torch.randint(0, 3, (2, 1, 1, 4, 8), device="cuda").float()
    with pytest.raises(TypeError, match="dice_loss_sum"):
        ops.seg_loss(p, lab)
    with pytest.raises(TypeError, match="dice_loss_sum"):
        ops.seg_loss(p, ops.onehot(lab, 3))
    with pytest.raises(ValueError):
        ops.seg_loss(p, ops.LabelTarget(lab), class_weights=[1.0, 2.0])
    with pytest.raises(ValueError):
        ops.seg_loss(p, ops.LabelTarget(lab[:1]))
    for kw in (dict(class_weights=[1.0, -1.0, 1.0]), dict(class_weights=[1.0, float("nan"), 1.0]), dict(gamma=-0.5), dict(dice_weight=-1.0),
               dict(ce_weight=-1.0), dict(botindex=2, topindex=2), dict(botindex=2, topindex=1), dict(botindex=-1, topindex=2), dict(eps=-1.0)):
        with pytest.raises(VaesegError):
            ops.seg_loss(p, ops.LabelTarget(lab), **kw)
    p9 = torch.softmax(torch.randn(1, 9, 1, 4, 8, device="cuda"), 1)
    with pytest.raises(VaesegError):
        ops.seg_loss(p9, ops.LabelTarget(torch.zeros(1, 1, 1, 4, 8, device="cuda")), topindex=9)
    # the C interface itself: codes, answered on the host before any launch (nothing below may touch terms / final / gp)
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    w8 = (ctypes.c_float * 8)(*([1.0] * 8))
    wp = ctypes.addressof(w8)
    scratch = torch.empty(lib.vs_seg_loss_scratch_doubles(2, 3), dtype=torch.float64, device="cuda")
    assert lib.vs_seg_loss_scratch_doubles(2, 0) == 0 and lib.vs_seg_loss_scratch_doubles(2, 9) == 0 and lib.vs_seg_loss_scratch_doubles(0, 3) == 0
    terms = torch.full((2,), -7.0, device="cuda")
    final = torch.full((), -7.0, device="cuda")
    gout = torch.ones((), device="cuda")
    gp = torch.full_like(p, -7.0)
    st = torch.cuda.current_stream().cuda_stream
    P, L, S, TT, F, G, GP = p.data_ptr(), lab.data_ptr(), scratch.data_ptr(), terms.data_ptr(), final.data_ptr(), gout.data_ptr(), gp.data_ptr()

    def fwd(p_=P, l_=L, w_=wp, s_=S, t_=TT, f_=F, b=2, c=3, v=32, bot=1, top=3, eps=1e-6, dw=1.0, cw=1.0, bd=0, gamma=0.0):
        return lib.vs_seg_loss_fwd(p_, l_, w_, s_, t_, f_, b, c, v, bot, top, eps, dw, cw, bd, gamma, st)

    def bwd(p_=P, l_=L, w_=wp, s_=S, g_=G, gp_=GP, b=2, c=3, v=32, bot=1, top=3, eps=1e-6, dw=1.0, cw=1.0, bd=0, gamma=0.0):
        return lib.vs_seg_loss_bwd(p_, l_, w_, s_, g_, gp_, b, c, v, bot, top, eps, dw, cw, bd, gamma, st)

    neg = (ctypes.c_float * 8)(1.0, -1.0, 1.0, 1, 1, 1, 1, 1)
    for f in (fwd, bwd):
        for bad, code in ((dict(v=30), EALIGN), (dict(v=31), EALIGN), (dict(p_=P + 4), EALIGN), (dict(l_=L + 8), EALIGN), (dict(c=0), EINVAL), (dict(c=9, top=9), EINVAL),
                          (dict(bot=3, top=3), EINVAL), (dict(bot=2, top=1), EINVAL), (dict(bot=-1), EINVAL), (dict(top=4), EINVAL), (dict(gamma=-1.0), EINVAL),
                          (dict(gamma=float("nan")), EINVAL), (dict(dw=-1.0), EINVAL), (dict(cw=-0.5), EINVAL), (dict(eps=-1.0), EINVAL),
                          (dict(w_=ctypes.addressof(neg)), EINVAL), (dict(p_=None), EINVAL), (dict(l_=None), EINVAL), (dict(w_=None), EINVAL),
                          (dict(s_=None), EINVAL), (dict(b=0), EINVAL), (dict(v=0), EINVAL), (dict(b=65), ESHAPE), (dict(v=1 << 31), ESHAPE)):
            assert f(**bad) == code, (f.__name__, bad)
    assert fwd(t_=None) == EINVAL and fwd(f_=None) == EINVAL and bwd(g_=None) == EINVAL and bwd(gp_=None) == EINVAL and bwd(gp_=GP + 4) == EALIGN
    torch.cuda.synchronize()
    assert float(terms[0]) == -7.0 and float(final) == -7.0 and float((gp + 7.0).abs().max()) == 0.0
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert float(final) != -7.0 and float((gp + 7.0).abs().min()) > 0.0


def _seg(seed=0):
    import joint_model as M
    from oracle import ref_cpu as O
    return O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=seed).cuda()


def _train_inputs():
    from oracle import ref_cpu as O
    img, lab = O.synthetic_image(2, 32, 2).cuda(), O.synthetic_label(2, 32, 3).cuda()
    lab[1] = 0                                 # sample 1 all background
    assert float(lab[0].sum()) > 0
    return img, lab


LOSS = {"dice_weight": 1.0, "ce_weight": 1.0, "batch_dice": True, "class_weights": [0.5, 2.0], "gamma": 0.0}


def test_captured_training_equals_eager_training_bit_for_bit():
    """three GraphedStep replays of seg_train_losses(loss=...) on the 32^3, batch-2 Segmentation of tests/test_gpu_model.py against three eager steps:
    the same loss and weights, bit for bit; and the compound loss trains differently from the default"""
    from vae_segmentation_amd import optim
    from vae_segmentation_amd import train as T
    img, lab = _train_inputs()
    seg_a, seg_c, seg_d = _seg(), _seg(), _seg()
    opt_a = optim.SGD(seg_a.parameters(), lr=1e-2, momentum=0.9)
    opt_c = optim.SGD(seg_c.parameters(), lr=1e-2, momentum=0.9)
    opt_d = optim.SGD(seg_d.parameters(), lr=1e-2, momentum=0.9)
    gs = T.GraphedStep(lambda: T.seg_train_losses(seg_a, img, lab, loss=LOSS), list(seg_a.parameters()), opt_a, warmup=1)
    assert gs.tail
    first = None
    for i in range(3):
        la = gs.step()
        opt_c.zero_grad()
        lc, aux = T.seg_train_losses(seg_c, img, lab, loss=LOSS)
        lc.backward()
        opt_c.step()
        torch.cuda.synchronize()
        assert torch.equal(la.detach(), lc.detach()), i
        assert set(aux) == {"dice_loss", "ce_loss", "batch"} and aux["ce_loss"].item() > 0
        if i == 0:
            first = [p.detach().clone() for p in seg_c.parameters()]
    assert gs.recaptures == 0
    for (n, p), q in zip(seg_a.named_parameters(), seg_c.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    opt_d.zero_grad()
    ld, aux_d = T.seg_train_losses(seg_d, img, lab, loss=None)
    ld.backward()
    opt_d.step()
    torch.cuda.synchronize()
    assert "ce_loss" not in aux_d
    assert any(not torch.equal(p, q.detach()) for p, q in zip(first, seg_d.parameters()))


def test_joint_train_losses_with_the_compound_loss():
    """joint_train keeps lambda_vae (1 - Dice(pred, recon)) and adds seg_loss(pred, gt)"""
    import joint_model as M
    from oracle import ref_cpu as O
    from vae_segmentation_amd import ops
    from vae_segmentation_amd import train as T
    side = 64
    joint = M.Joint(models=[M.Segmentation(1, 2, norm_type=1), M.VAE(2, 2, norm_type=1, dim=128, spatial=side)])
    O.deterministic_fill_(joint, seed=0)
    joint = joint.cuda()
    img, lab = O.synthetic_image(1, side, 2).cuda(), O.synthetic_label(1, side, 3).cuda()
    final, aux = T.joint_train_losses(joint, img, lab, lambda_vae=0.1, loss=LOSS)
    final.backward()
    pred, recon = aux["batch"]["pred"].detach(), aux["batch"]["recon"].detach()
    vae_part, (r,) = ops.dice_loss_sum(pred, [(recon, 0.1)], botindex=1, topindex=2, eps=T.EPS_MAIN_SOURCE)
    seg_part, (d, ce) = ops.seg_loss(pred, ops.LabelTarget(lab), botindex=1, topindex=2, eps=T.EPS_MAIN_SOURCE, **LOSS)
    assert torch.equal(final.detach(), vae_part + seg_part)
    assert torch.equal(aux["recon_loss"], r) and torch.equal(aux["dice_loss"], d) and torch.equal(aux["ce_loss"], ce)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in joint.Seg.parameters())


def test_default_path_is_the_dice_loss_sum_call():
    """loss=None: the code path of before — the bits of a direct ops.dice_loss_sum call on the same prediction"""
    from vae_segmentation_amd import ops
    from vae_segmentation_amd import train as T
    img, lab = _train_inputs()
    seg = _seg()
    final, aux = T.seg_train_losses(seg, img, lab, loss=None)
    again, _ = T.seg_train_losses(seg, img, lab)
    direct, (term,) = ops.dice_loss_sum(aux["batch"]["pred"].detach(), [(ops.LabelTarget(lab), 1.0)], botindex=1, topindex=2, eps=T.EPS_MAIN_SOURCE)
    assert set(aux) == {"dice_loss", "batch"}
    assert torch.equal(final.detach(), direct) and torch.equal(again.detach(), direct) and torch.equal(aux["dice_loss"], term)


def test_entry_point_runs_the_compound_loss(tmp_path):
    common = ["--size", "32", "-b", "2", "-E", "1", "--eval_epoch", "1", "--save_epoch", "1", "--synthetic_train", "4", "--synthetic_val", "1",
              "--max_iters", "2", "--display_freq", "1", "--seg_loss", "dice_ce", "--batch_dice"]

    def run(method):
        return subprocess.run([sys.executable, os.path.join(REPO, "main_source.py"), "sl", "--method", method] + common, cwd=str(tmp_path),
                              env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=900)
    out = run("seg_train")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Finished Training" in out.stdout and "ce_loss" in out.stdout and "graph replay" in out.stdout
    bad = run("vae_train")
    assert bad.returncode != 0 and "seg_loss" in bad.stderr
