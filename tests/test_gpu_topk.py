"""The compound loss with a top-k cross-entropy (csrc/topk.hip: ops.seg_loss(topk=), ops.SegLossTopK, train.seg_train_losses(loss={"topk": ...}),
--ce_topk) against its fp64 restatement (tests/topk_util.py, pinned on the host by tests/test_host_topk.py), in both builds.  Inputs are planar fp32
probabilities (B, C, 1, 4, V / 4) and labels (B, 1, 1, 4, V / 4), as tests/test_gpu_segloss.py builds them, so the voxel count V of a plane is set directly.

Units of work, in quads (4 voxels) of a plane: a lane takes one quad per trip, a wave 64, a workgroup 256.  The voxel-major kernels (first pass, the
sums, the backward) hold min(ceil(quads / 256), 512) workgroups per sample — 131,072 quads is the cap, 131,073 wraps the grid-stride loop; the key-only
count passes walk the pooled keys of the batch with min(ceil(B quads / 256), 2048) workgroups — B = 2 and 131,072 quads is 1024 of them; B = 5 at that size
(655,360 pooled quads, 2560 workgroups wanted) wraps their loop: test_the_pooled_passes_wrap.

Counts — N, K, n_gt, n_eq — are integers and must EQUAL the restatement's.  The keys are fp32 roundings of fp64 products, formed on the device from a
fp64 logarithm that may differ from the host's in its last bit; such a difference moves a key only where the fp64 value lies within 1e-16 of a rounding
boundary of fp32 (about 2^-29 of the voxels), and a count only if that key is the threshold's neighbour: not in these seeded cases.  The constructed
cases use p_l in {1, 0.5, 0.25, 0} or the clamp value alone, where equal p gives equal keys whatever the logarithm.
Tolerances follow tests/test_gpu_segloss.py's header unchanged: every sum is fp64 over exactly promoted values and each output is rounded to fp32 once —
tau, terms and final within 1e-6 max(1, |value|), gradients norm-wise < 1e-6, exact zeros where the rule gives a zero."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import segloss_util as SU
from tests import topk_util as TU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

both = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
QUADS = [1, 64, 65, 256, 257, 4097, 131072, 131073]
CFGS = [(1, 0, 1), (2, 1, 2), (8, 2, 5)]                                 # (C, bot, top)
RS = [1e-9, 0.1, 0.5, 1.0]
MODE_A = dict(dice_weight=1.0, ce_weight=1.0, batch_dice=False, gamma=0.0, class_weights=None)
MODE_B = dict(dice_weight=0.6, ce_weight=1.7, batch_dice=True, gamma=2.0, class_weights="ramp")


def _ops():
    from vae_segmentation_amd import ops
    return ops


def _weights(kind, c):
    """None, or unequal class weights with a zero (the last class's) where there is more than one class"""
    if kind is None or isinstance(kind, (list, tuple)):
        return None if kind is None else list(kind)
    return [0.5 + 0.75 * k if (k < c - 1 or c == 1) else 0.0 for k in range(c)]


def _mixed_labels(g, b, c, v):
    """random classes; a tenth of the voxels carry every sort of ignored value (at least one of each where the plane has room), a tenth a fractional label"""
    lab = torch.randint(0, c, (b, 1, 1, 1, v), generator=g).float()
    r = torch.rand(lab.shape, generator=g)
    for j, bad in enumerate((-1.0, 255.0, float("nan"), float(c), -0.5)):
        lab[(r >= 0.02 * j) & (r < 0.02 * (j + 1))] = bad
        if v > j:
            lab[0, 0, 0, 0, j] = bad
    frac = (r >= 0.5) & (r < 0.6)
    lab[frac] = lab[frac] + 0.5
    if v > 5:
        lab[-1, 0, 0, 0, 5] = 0.5
    return lab


def _planar(p, lab):
    b, c, v = p.shape[0], p.shape[1], p.shape[-1]
    shape = (b, c, 1, 4, v // 4)
    return p.reshape(shape), lab.reshape((b, 1) + shape[2:])


def _oracle(p, lab, rs, mode, bot, top, eps):
    """the restatement's results for every r of rs on one pair of inputs: the Dice part and the voxel losses are formed once.
    -> {r: {"final", "dice", "ce", "grad", "ce_grad", "info", "below": (B, 1, ...) mask of the valid voxels whose key is below tau}}"""
    b, c = p.shape[:2]
    p64 = p.double().requires_grad_(True)
    d = SU.dice_term(p64, lab, 0 if c == 1 else bot, 1 if c == 1 else top, eps, mode["batch_dice"])
    (dgrad,) = torch.autograd.grad(d, p64)
    out = {}
    for r in rs:
        ce, info = TU.topk_ce(p64, lab, r, mode["class_weights"], mode["gamma"])
        (cgrad,) = torch.autograd.grad(ce, p64, allow_unused=True)
        cgrad = torch.zeros_like(dgrad) if cgrad is None else cgrad
        below = torch.zeros(info["valid"].shape, dtype=torch.bool)
        below[info["valid"]] = info["keys"] < info["tau"]
        out[r] = {"final": mode["dice_weight"] * d.item() + mode["ce_weight"] * ce.item(), "dice": d.item(), "ce": ce.item(),
                  "grad": mode["dice_weight"] * dgrad + mode["ce_weight"] * cgrad, "ce_grad": cgrad, "info": info,
                  "below": below.reshape((b, 1) + tuple(p.shape[2:])), "valid": info["valid"].reshape((b, 1) + tuple(p.shape[2:]))}
    return out


@functools.lru_cache(maxsize=4)
def _random_case(b, c, v, bot, top, eps, mode, seed=0):
    """softmax probabilities and mixed labels on the host with the restatement's results for every r of RS; shared by the two builds"""
    mode = dict(mode)
    mode["class_weights"] = _weights(mode["class_weights"], c)
    g = torch.Generator().manual_seed(100003 * seed + v + 7 * b + 13 * c + 3 * bot)
    p = torch.softmax(torch.randn(b, c, 1, 1, v, generator=g) * 2, 1)
    lab = _mixed_labels(g, b, c, v)
    p, lab = _planar(p, lab)
    return {"p": p, "lab": lab, "mode": mode, "want": _oracle(p, lab, RS, mode, bot, top, eps)}


def _gpu(ops, p, lab, r, mode, bot, top, eps, scale=None):
    pg = p.cuda().requires_grad_(True)
    record = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    final, (d, ce) = ops.seg_loss(pg, ops.LabelTarget(lab.cuda()), botindex=bot, topindex=top, eps=eps, topk=r, record=record, **mode)
    assert not d.requires_grad and not ce.requires_grad
    (final if scale is None else final * scale).backward()
    torch.cuda.synchronize()
    return final.detach().item(), d.item(), ce.item(), pg.grad.cpu(), ops.topk_record(record)


def _close(got, want):
    return abs(got - want) <= 1e-6 * max(1.0, abs(want))


def _check(ops, p, lab, r, mode, want, bot, top, eps, what):
    final, d, ce, gp, rec = _gpu(ops, p, lab, r, mode, bot, top, eps)
    info = want["info"]
    gmax = float(want["grad"].abs().max())
    gerr = SU.relerr(gp, want["grad"]) if gmax > 0 else float(gp.abs().max())
    print(what, "r %g N %d K %d tau %.9g n_gt %d n_eq %d | final %.9g (%.3g off) dice %.9g (%.3g off) ce %.9g (%.3g off) tau %.3g off grad relerr %.3g"
          % (r, rec["N"], rec["K"], rec["tau"], rec["n_gt"], rec["n_eq"], final, abs(final - want["final"]), d, abs(d - want["dice"]), ce,
             abs(ce - want["ce"]), abs(rec["tau"] - info["tau"]), gerr))
    assert (rec["N"], rec["K"], rec["n_gt"], rec["n_eq"]) == (info["N"], info["K"], info["n_gt"], info["n_eq"]), what
    assert _close(rec["tau"], info["tau"]) and _close(d, want["dice"]) and _close(ce, want["ce"]) and _close(final, want["final"]), what
    assert gp.shape == p.shape and gp.dtype == torch.float32 and torch.isfinite(gp).all(), what
    if gmax > 0:
        assert gerr < 1e-6, what
    else:
        assert float(gp.abs().max()) == 0.0, what
    assert float((gp * (~want["valid"]).float()).abs().max()) == 0.0, what                     # exactly 0 at every ignored voxel, in every channel
    # the cross-entropy part alone (dice_weight 0): exactly 0 at every voxel whose key is below tau as well
    _, _, ce0, gc, rec0 = _gpu(ops, p, lab, r, dict(mode, dice_weight=0.0), bot, top, eps)
    assert rec0 == rec and ce0 == ce, what
    assert float((gc * (want["below"] | ~want["valid"]).float()).abs().max()) == 0.0, what
    cmax = float(want["ce_grad"].abs().max())
    if cmax > 0:
        assert SU.relerr(gc, mode["ce_weight"] * want["ce_grad"]) < 1e-6, what
    else:
        assert float(gc.abs().max()) == 0.0, what
    return final, d, ce, gp, rec


@both
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("quads", QUADS)
def test_plane_sizes(quads, cfg, lib_mode):
    ops = _ops()
    c, bot, top = cfg
    for mode in (MODE_A, MODE_B):
        case = _random_case(2, c, 4 * quads, bot, top, 1e-4, tuple(sorted(mode.items())))
        for r in RS:
            what = "B 2 C %d quads %d [%d, %d) %s" % (c, quads, bot, top, case["mode"])
            rec = _check(ops, case["p"], case["lab"], r, case["mode"], case["want"][r], bot, top, 1e-4, what)[4]
            if r == 1e-9:
                assert rec["K"] == 1
            if r == 1.0:
                assert rec["K"] == rec["N"]


@both
def test_the_pooled_passes_wrap(lib_mode):
    """B = 5 at 131,072 quads: 655,360 pooled quads against the 524,288 one sweep of the count passes' 2048 workgroups covers — every workgroup below 512
    makes a second trip, across the boundary between samples 3 and 4"""
    ops = _ops()
    case = _random_case(5, 2, 4 * 131072, 1, 2, 1e-4, tuple(sorted(MODE_A.items())))
    for r in (0.1, 0.5):
        _check(ops, case["p"], case["lab"], r, case["mode"], case["want"][r], 1, 2, 1e-4, "B 5 C 2 quads 131072")


def _from_pl(pl, cls, c):
    """(B, V) probabilities of the labelled class and (B, V) classes -> planar p (B, C, 1, 4, V / 4) with p_l there and the rest spread over the others,
    labels likewise; c >= 2"""
    b, v = pl.shape
    rest = ((1 - pl) / (c - 1))[:, None].expand(b, c, v)
    p = rest.clone().scatter_(1, cls[:, None], pl[:, None])
    return _planar(p.reshape(b, c, 1, 1, v).float(), cls.float().reshape(b, 1, 1, 1, v))


def _pick(g, shape, values, shares):
    """values drawn with the given shares (they sum to 1), elementwise"""
    u = torch.rand(shape, generator=g)
    out = torch.full(shape, float(values[-1]))
    edge = 0.0
    for val, share in zip(values[:-1], shares[:-1]):
        out[(u >= edge) & (u < edge + share)] = float(val)
        edge += share
    return out


TIES = {
    # name: (quads per sample, values of p_l, their shares, r, gamma, what tau must be)
    "threshold_on_key_zero": (300, (1.0, 0.5, 0.25, 0.0), (0.9, 0.04, 0.03, 0.03), 0.5, 0.0, 0.0),
    "threshold_on_the_clamp_value": (300, (0.0, 0.5, 0.25, 1.0), (0.4, 0.2, 0.2, 0.2), 0.1, 0.0, 100.0),
    "a_group_over_workgroups_and_samples": (600, (0.5, 0.25, 1.0), (0.5, 0.2, 0.3), 0.5, 0.0, None),
    "a_group_over_workgroups_and_samples_focal": (600, (0.5, 0.25, 1.0), (0.5, 0.2, 0.3), 0.5, 2.0, None),
    "all_valid_voxels_equal": (300, (0.5,), (1.0,), 0.3, 0.0, None),
}


@both
@pytest.mark.parametrize("name", sorted(TIES))
def test_ties_by_construction(name, lib_mode):
    """p_l from {1, 0.5, 0.25, 0} only: equal p gives equal keys on the device whatever its logarithm's last bit, and tie groups hold thousands"""
    ops = _ops()
    quads, values, shares, r, gamma, tau = TIES[name]
    g = torch.Generator().manual_seed(len(name))
    b, c, v = 2, 2, 4 * quads
    pl = _pick(g, (b, v), values, shares)
    cls = torch.randint(0, c, (b, v), generator=g)
    p, lab = _from_pl(pl, cls, c)
    lab[0, 0, 0, 0, :3] = torch.tensor([-1.0, 255.0, float("nan")])
    mode = dict(MODE_A, gamma=gamma)
    want = _oracle(p, lab, (r,), mode, 1, 2, 1e-6)[r]
    rec = _check(ops, p, lab, r, mode, want, 1, 2, 1e-6, name)[4]
    assert rec["n_eq"] > 256 and rec["n_gt"] + rec["n_eq"] > rec["K"]          # the threshold's group is large and straddles K
    if tau is not None:
        assert rec["tau"] == tau
    if name == "all_valid_voxels_equal":
        assert rec["n_gt"] == 0 and rec["n_eq"] == rec["N"] == 2 * v - 3


# class weights under which the keys of clamped voxels (p_l = 0: f = 100 exactly, no logarithm) differ in one byte of their fp32 image only.
# 100 = 0x42C80000.  4^j moves the exponent by 2 j: bits 24 and up.  1 + j 2^-6 adds 204800 j ulps (bits 13 .. 20), 1 + j 2^-14 adds 800 j ulps
# (below bit 13), 1 + j 2^-22 adds round(3.125 j) ulps (below bit 5): each set agrees in every byte above the one named.
RADIX = {"top_byte": [4.0 ** j for j in range(8)], "second_byte": [1 + j * 2.0 ** -6 for j in range(8)],
         "third_byte": [1 + j * 2.0 ** -14 for j in range(8)], "lowest_byte": [1 + j * 2.0 ** -22 for j in range(8)]}


@both
@pytest.mark.parametrize("name", sorted(RADIX))
def test_each_radix_pass_decides(name, lib_mode):
    ops = _ops()
    w = RADIX[name]
    images = torch.tensor([100.0 * x for x in w], dtype=torch.float64).float().view(torch.int32)
    shift = {"top_byte": 24, "second_byte": 16, "third_byte": 8, "lowest_byte": 0}[name]
    above = images >> (shift + 8) if shift < 24 else images & 0xFFFFFF            # the top byte's set: agrees in every byte BELOW instead
    assert len(set(above.tolist())) == 1 and len(set(((images >> shift) & 255).tolist())) == 8          # the byte named decides alone
    g = torch.Generator().manual_seed(shift)
    b, c, v = 2, 8, 4 * 300
    cls = torch.randint(0, c, (b, v), generator=g)
    p, lab = _from_pl(torch.zeros(b, v), cls, c)
    mode = dict(MODE_A, class_weights=w)
    for r in (0.05, 0.4, 0.8):
        want = _oracle(p, lab, (r,), mode, 2, 5, 1e-6)[r]
        rec = _check(ops, p, lab, r, mode, want, 2, 5, 1e-6, "%s r %g" % (name, r))[4]
        assert rec["tau"] in [float(torch.tensor(100.0 * x, dtype=torch.float64).float()) for x in w]


@both
def test_the_batch_is_one_pool(lib_mode):
    """sample 0 all saturated (p_l = 1, key 0), every hard voxel in sample 1: K = N / 4 places all go to sample 1, whose mean a per-sample rule would
    not give; sample 0's cross-entropy gradient is exactly 0"""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    b, c, v = 2, 3, 4 * 300
    cls = torch.randint(0, c, (b, v), generator=g)
    pl = torch.rand(b, v, generator=g) * 0.98 + 0.01
    pl[0] = 1.0
    p, lab = _from_pl(pl, cls, c)
    want = _oracle(p, lab, (0.25,), MODE_A, 1, 3, 1e-6)[0.25]
    rec = _check(ops, p, lab, 0.25, MODE_A, want, 1, 3, 1e-6, "pool")[4]
    assert rec["K"] == (2 * v) // 4 and rec["tau"] > 0 and rec["n_gt"] == rec["K"] - 1
    _, _, _, gc, _ = _gpu(ops, p, lab, 0.25, dict(MODE_A, dice_weight=0.0), 1, 3, 1e-6)
    assert float(gc[0].abs().max()) == 0.0 and float(gc[1].abs().max()) > 0.0


@both
def test_degenerate_pools(lib_mode):
    ops = _ops()
    g = torch.Generator().manual_seed(6)
    b, c, v = 2, 3, 4 * 70
    p, _ = _planar(torch.softmax(torch.randn(b, c, 1, 1, v, generator=g), 1), torch.zeros(b, 1, 1, 1, v))
    none = torch.full((b, 1, 1, 4, v // 4), -1.0)
    none[1] = float("nan")
    for mode in (MODE_A, MODE_B):
        mode = dict(mode, class_weights=_weights(mode["class_weights"], c))
        want = _oracle(p, none, (0.1,), mode, 1, 3, 1e-6)[0.1]
        final, d, ce, gp, rec = _check(ops, p, none, 0.1, mode, want, 1, 3, 1e-6, "all ignored")
        assert rec == {"N": 0, "K": 0, "tau": 0.0, "n_gt": 0, "n_eq": 0} and ce == 0.0 and float(gp.abs().max()) == 0.0
        one = none.clone()
        one[1, 0, 0, 2, 33] = 1.0
        for r in (1e-9, 0.1, 1.0):
            want = _oracle(p, one, (r,), mode, 1, 3, 1e-6)[r]
            rec = _check(ops, p, one, r, mode, want, 1, 3, 1e-6, "one valid voxel")[4]
            assert (rec["N"], rec["K"], rec["n_gt"], rec["n_eq"]) == (1, 1, 0, 1)


@both
def test_a_record_may_be_reused_before_the_backward(lib_mode):
    """two calls fill ONE record tensor, then both backwards run: each uses its own selection (the workspace's copy), not the record's last content;
    and record=None fills nothing and changes nothing"""
    ops = _ops()
    case = _random_case(2, 3, 4 * 321, 1, 3, 1e-6, tuple(sorted(MODE_A.items())))
    p, lab, m = case["p"], case["lab"], case["mode"]
    record = torch.zeros(4, dtype=torch.float64, device="cuda")
    pa, pb, pc = (p.cuda().requires_grad_(True) for _ in range(3))
    fa, _ = ops.seg_loss(pa, ops.LabelTarget(lab.cuda()), botindex=1, topindex=3, topk=0.1, record=record, **m)
    fb, _ = ops.seg_loss(pb, ops.LabelTarget(lab.cuda()), botindex=1, topindex=3, topk=0.9, record=record, **m)
    fc, _ = ops.seg_loss(pc, ops.LabelTarget(lab.cuda()), botindex=1, topindex=3, topk=0.1, **m)
    fa.backward()
    fb.backward()
    fc.backward()
    assert ops.topk_record(record)["K"] == TU.rank_of(0.9, case["want"][0.1]["info"]["N"])
    assert torch.equal(fa, fc) and torch.equal(pa.grad, pc.grad) and not torch.equal(pa.grad, pb.grad)
    assert SU.relerr(pa.grad.cpu(), case["want"][0.1]["grad"]) < 1e-6


@both
def test_a_nan_probability_is_among_the_hardest(lib_mode):
    """a NaN key (a NaN probability under a focal exponent: fmax drops the NaN of the plain logarithm, which gives the clamp's 100) is ordered above +inf
    whatever its sign bit: it takes one of the K places and the term is NaN"""
    ops = _ops()
    case = _random_case(2, 3, 4 * 321, 1, 3, 1e-6, tuple(sorted(MODE_A.items())))
    info = case["want"][0.1]["info"]
    for nan in (float("nan"), -float("nan")):
        p = case["p"].clone()
        lab = case["lab"].clone()
        lab[1, 0, 0, 1, 7] = 0.0
        p[1, 0, 0, 1, 7] = nan
        record = torch.zeros(4, dtype=torch.float64, device="cuda")
        _, (d, ce) = ops.seg_loss(p.cuda(), ops.LabelTarget(lab.cuda()), botindex=1, topindex=3, topk=1e-9, record=record, **dict(case["mode"], gamma=2.0))
        rec = ops.topk_record(record)
        assert rec["K"] == 1 and rec["n_gt"] == 0 and rec["n_eq"] == 1 and rec["tau"] != rec["tau"] and ce.item() != ce.item()


@both
def test_keeping_everything_with_unit_weights_is_the_plain_term(lib_mode):
    """topk = 1.0: the mean over all N valid voxels; with unit weights sum w = N, the plain term's denominator"""
    ops = _ops()
    for mode in (MODE_A, dict(MODE_B, class_weights=None)):
        case = _random_case(2, 3, 4 * 321, 1, 3, 1e-6, tuple(sorted(mode.items())))
        p, lab = case["p"], case["lab"]
        final, d, ce, gp, rec = _gpu(ops, p, lab, 1.0, case["mode"], 1, 3, 1e-6)
        pg = p.cuda().requires_grad_(True)
        f0, (d0, ce0) = ops.seg_loss(pg, ops.LabelTarget(lab.cuda()), botindex=1, topindex=3, eps=1e-6, topk=None, **case["mode"])
        f0.backward()
        assert _close(d, d0.item()) and _close(ce, ce0.item()) and _close(final, f0.item())
        assert SU.relerr(gp, pg.grad.cpu()) < 1e-6


@both
def test_without_topk_the_path_is_the_parents(lib_mode):
    """topk=None: the bits of a direct ops.SegLoss call — the two launches and the one of before"""
    ops = _ops()
    case = _random_case(2, 3, 4 * 321, 1, 3, 1e-6, tuple(sorted(MODE_B.items())))
    m = case["mode"]
    pa, pb = case["p"].cuda().requires_grad_(True), case["p"].cuda().requires_grad_(True)
    lab = case["lab"].cuda()
    fa, (da, ca) = ops.seg_loss(pa, ops.LabelTarget(lab), botindex=1, topindex=3, eps=1e-6, topk=None, record=None, **m)
    fb, tb = ops.SegLoss.apply(pb, lab, 1, 3, 1e-6, m["dice_weight"], m["ce_weight"], m["batch_dice"], m["class_weights"], m["gamma"])
    fa.backward()
    fb.backward()
    assert type(fa.grad_fn).__name__.startswith("SegLossBackward")
    assert torch.equal(fa, fb) and torch.equal(da, tb[0]) and torch.equal(ca, tb[1]) and torch.equal(pa.grad, pb.grad)
    want, _ = SU.seg_loss(case["p"].double(), case["lab"], bot=1, top=3, eps=1e-6, **m)
    assert abs(fa.item() - float(want)) <= 2e-6 * (0.6 + 1.7 * max(1.0, ca.item()))


def _bits(ts):
    return [t.detach().clone() for t in ts]


def test_graph_replay_and_the_two_builds_give_the_bits_of_an_eager_call():
    """forward and backward captured once, replayed three times on fresh inputs: torch.equal to eager calls, the record included; and the atomic build's
    results are the deterministic build's (the counts are integer atomics in both, no floating-point sum uses one)"""
    ops = _ops()
    b, c, v = 2, 3, 4 * 4097
    cases = [_random_case(b, c, v, 1, 3, 1e-4, tuple(sorted(MODE_B.items())), seed) for seed in (11, 12, 13)]
    kw = dict(cases[0]["mode"], botindex=1, topindex=3, eps=1e-4, topk=0.1)
    p = torch.zeros_like(cases[0]["p"]).cuda().requires_grad_(True)
    lab = torch.zeros_like(cases[0]["lab"]).cuda()
    record = torch.zeros(4, dtype=torch.float64, device="cuda")

    def step():
        p.grad = None
        final, terms = ops.seg_loss(p, ops.LabelTarget(lab), record=record, **kw)
        final.backward()
        return [final, terms[0], terms[1], p.grad, record]

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
    assert _close(results[True][0][0].item(), cases[0]["want"][0.1]["final"])
    assert ops.topk_record(results[True][0][4])["K"] == cases[0]["want"][0.1]["info"]["K"]


@both
def test_argument_errors(lib_mode):
    import ctypes
    from vae_segmentation_amd._lib import lib
    ops = _ops()
    p = torch.softmax(torch.randn(2, 3, 1, 4, 8, device="cuda"), 1)
    lab = torch.randint(0, 3, (2, 1, 1, 4, 8), device="cuda").float()
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="topk"):
            ops.seg_loss(p, ops.LabelTarget(lab), topk=bad)
    with pytest.raises(TypeError, match="record"):
        ops.seg_loss(p, ops.LabelTarget(lab), record=torch.zeros(4, dtype=torch.float64, device="cuda"))
    for rec in (torch.zeros(4, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda"), torch.zeros(4, dtype=torch.float64)):
        with pytest.raises(ValueError, match="record"):
            ops.seg_loss(p, ops.LabelTarget(lab), topk=0.5, record=rec)
    # the C interface itself: codes, answered on the host before any launch (nothing below may touch terms / final / gp / record)
    EINVAL, ESHAPE, EALIGN = -1, -2, -5
    w8 = (ctypes.c_float * 8)(*([1.0] * 8))
    wp = ctypes.addressof(w8)
    nbytes = lib.vs_seg_topk_workspace_bytes(2, 32)
    assert nbytes >= 2 * 32 * 4 and nbytes % 16 == 0
    assert lib.vs_seg_topk_workspace_bytes(0, 32) == 0 and lib.vs_seg_topk_workspace_bytes(65, 32) == 0 and lib.vs_seg_topk_workspace_bytes(2, 0) == 0
    assert lib.vs_seg_topk_workspace_bytes(2, 1 << 25) == 0 and lib.vs_seg_topk_workspace_bytes(1, (1 << 26) - 4) > 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    record = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    terms = torch.full((2,), -7.0, device="cuda")
    final = torch.full((), -7.0, device="cuda")
    gout = torch.ones((), device="cuda")
    gp = torch.full_like(p, -7.0)
    st = torch.cuda.current_stream().cuda_stream
    P, L, W, R, TT, F, G, GP = (p.data_ptr(), lab.data_ptr(), ws.data_ptr(), record.data_ptr(), terms.data_ptr(), final.data_ptr(), gout.data_ptr(),
                                gp.data_ptr())

    def fwd(p_=P, l_=L, w_=wp, s_=W, r_=R, t_=TT, f_=F, b=2, c=3, v=32, bot=1, top=3, eps=1e-6, dw=1.0, cw=1.0, bd=0, gamma=0.0, r=0.5):
        return lib.vs_seg_loss_topk_fwd(p_, l_, w_, s_, r_, t_, f_, b, c, v, bot, top, eps, dw, cw, bd, gamma, r, st)

    def bwd(p_=P, l_=L, w_=wp, s_=W, g_=G, gp_=GP, b=2, c=3, v=32, bot=1, top=3, eps=1e-6, dw=1.0, cw=1.0, bd=0, gamma=0.0, r=0.5):
        return lib.vs_seg_loss_topk_bwd(p_, l_, w_, s_, g_, gp_, b, c, v, bot, top, eps, dw, cw, bd, gamma, r, st)

    neg = (ctypes.c_float * 8)(1.0, -1.0, 1.0, 1, 1, 1, 1, 1)
    inf = (ctypes.c_float * 8)(1.0, float("inf"), 1.0, 1, 1, 1, 1, 1)
    assert fwd(r_=R + 4) == EALIGN
    for f in (fwd, bwd):
        for bad, code in ((dict(v=30), EALIGN), (dict(p_=P + 4), EALIGN), (dict(l_=L + 8), EALIGN), (dict(s_=W + 8), EALIGN),
                          (dict(w_=ctypes.addressof(inf)), EINVAL),
                          (dict(c=0), EINVAL), (dict(c=9, top=9), EINVAL), (dict(bot=3, top=3), EINVAL), (dict(bot=-1), EINVAL), (dict(top=4), EINVAL),
                          (dict(gamma=-1.0), EINVAL), (dict(gamma=float("nan")), EINVAL), (dict(dw=-1.0), EINVAL), (dict(cw=-0.5), EINVAL),
                          (dict(eps=-1.0), EINVAL), (dict(w_=ctypes.addressof(neg)), EINVAL), (dict(p_=None), EINVAL), (dict(l_=None), EINVAL),
                          (dict(w_=None), EINVAL), (dict(s_=None), EINVAL), (dict(b=0), EINVAL), (dict(v=0), EINVAL),
                          (dict(r=0.0), EINVAL), (dict(r=-0.5), EINVAL), (dict(r=1.0000001), EINVAL), (dict(r=float("nan")), EINVAL),
                          (dict(b=65), ESHAPE), (dict(v=1 << 31), ESHAPE), (dict(v=1 << 25), ESHAPE)):
            assert f(**bad) == code, (f.__name__, bad)
    assert fwd(t_=None) == EINVAL and fwd(f_=None) == EINVAL and bwd(g_=None) == EINVAL and bwd(gp_=None) == EINVAL and bwd(gp_=GP + 4) == EALIGN
    torch.cuda.synchronize()
    assert float(terms[0]) == -7.0 and float(final) == -7.0 and float((gp + 7.0).abs().max()) == 0.0 and float((record + 7.0).abs().max()) == 0.0
    assert fwd(r_=None) == 0 and bwd() == 0                          # a null record: nothing to fill, the backward has the workspace's copy
    torch.cuda.synchronize()
    assert float(final) != -7.0 and float((gp + 7.0).abs().min()) > 0.0 and float((record + 7.0).abs().max()) == 0.0
    assert fwd(r=1.0) == 0
    torch.cuda.synchronize()
    assert ops.topk_record(record)["K"] == ops.topk_record(record)["N"] == 64


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


LOSS = {"dice_weight": 1.0, "ce_weight": 1.0, "batch_dice": True, "class_weights": [0.5, 2.0], "gamma": 0.0, "topk": 0.1}


def test_captured_training_equals_eager_training_bit_for_bit():
    """three GraphedStep replays of seg_train_losses(loss={"topk": 0.1, ...}) on the 32^3, batch-2 Segmentation of tests/test_gpu_model.py against three
    eager steps: the same loss, record and weights, bit for bit — K comes from a device count and the step is still one replayed graph; and the top-k
    term trains differently from the plain one"""
    from vae_segmentation_amd import ops, optim
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
        assert set(aux) == {"dice_loss", "ce_loss", "batch", "topk_record"} and aux["ce_loss"].item() > 0
        assert torch.equal(gs.aux["topk_record"], aux["topk_record"]), i
        rec = ops.topk_record(aux["topk_record"])
        assert rec["N"] == 2 * 32 ** 3 and rec["K"] == rec["N"] // 10 and rec["n_gt"] < rec["K"] <= rec["n_gt"] + rec["n_eq"]
        if i == 0:
            first = [p.detach().clone() for p in seg_c.parameters()]
    assert gs.recaptures == 0
    for (n, p), q in zip(seg_a.named_parameters(), seg_c.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    opt_d.zero_grad()
    ld, aux_d = T.seg_train_losses(seg_d, img, lab, loss=dict(LOSS, topk=None))
    ld.backward()
    opt_d.step()
    torch.cuda.synchronize()
    assert set(aux_d) == {"dice_loss", "ce_loss", "batch"}
    assert any(not torch.equal(p, q.detach()) for p, q in zip(first, seg_d.parameters()))


def test_entry_point_runs_the_topk_loss(tmp_path):
    common = ["--size", "32", "-b", "2", "-E", "1", "--eval_epoch", "1", "--save_epoch", "1", "--synthetic_train", "4", "--synthetic_val", "1",
              "--max_iters", "2", "--display_freq", "1", "--seg_loss", "dice_ce", "--ce_topk", "10"]
    out = subprocess.run([sys.executable, os.path.join(REPO, "main_source.py"), "tk", "--method", "seg_train"] + common, cwd=str(tmp_path),
                         env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Finished Training" in out.stdout and "ce_loss" in out.stdout and "graph replay" in out.stdout
    assert "topk %d/%d" % (2 * 32 ** 3 // 10, 2 * 32 ** 3) in out.stdout and "tau " in out.stdout
