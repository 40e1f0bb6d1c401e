"""tests/loss_util.py — the fp64 restatement the loss and label kernels are compared with (tests/test_gpu_loss.py) — pinned on the host first: against
the oracle's fp32 functions at three sizes (1e-6 absolute on Dice and BCE values, 1e-5 relative on KL), against the reference's recorded values
(tests/golden/kats.npz), and on the degenerate inputs the GPU tests rely on."""
import math

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import golden_util as G
from tests import loss_util as L

SIZES = [(2, 2, 4, 4, 4), (2, 3, 5, 6, 7), (1, 4, 8, 9, 10)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("shape", SIZES)
def test_dice_agrees_with_the_oracle(shape):
    g = _gen(shape[-1])
    s = torch.softmax(torch.randn(shape, generator=g) * 2, 1)
    t = torch.softmax(torch.randn(shape, generator=g) * 2, 1)
    c = shape[1]
    for bot, top in ((0, c), (1, c), (1, 2)):
        for eps in (1e-6, 1e-4):
            d = L.dice_planes(s, t, bot, top, eps)
            assert abs(d["mean"].item() - O.avg_dsc({"s": s, "t": t}, "s", "t", botindex=bot, topindex=top, eps=eps).item()) < 1e-6
            per = O.avg_dsc({"s": s, "t": t}, "s", "t", botindex=bot, topindex=top, eps=eps, return_mean=False)
            assert float((d["per_sample"] - per.double()).abs().max()) < 1e-6
            assert float((d["dice"] - O.dice_scores(s, t, eps).double()).abs().max()) < 1e-6
    # the hard form: the oracle's argmax -> scatter against the restatement's first maximal channel
    hard = O.avg_dsc({"s": s, "t": t}, "s", "t", binary=True, botindex=1, topindex=c)
    assert abs(L.dice_planes(L.hard_onehot(s), L.hard_onehot(t), 1, c, 1e-6)["mean"].item() - hard.item()) < 1e-6
    # the weighted sum of losses, a label target included
    lab = torch.randint(0, c, (shape[0], 1) + shape[2:], generator=g).float()
    final, terms = L.dice_loss_sum(s, [t, L.Label(lab)], [0.1, 1.0], 1, c, 1e-4)
    ref = [1 - O.avg_dsc({"s": s, "t": x}, "s", "t", botindex=1, topindex=c, eps=1e-4) for x in (t, O.one_hot(lab, c))]
    assert abs(terms[0].item() - ref[0].item()) < 1e-6 and abs(terms[1].item() - ref[1].item()) < 1e-6
    assert abs(final.item() - (0.1 * ref[0] + ref[1]).item()) < 2e-6 * 1.1


@pytest.mark.parametrize("shape", SIZES)
def test_kl_bce_onehot_agree_with_the_oracle(shape):
    g = _gen(100 + shape[-1])
    batch, dim = shape[0] + 1, shape[2] * shape[3] * shape[4]
    mean, std = torch.randn(batch, dim, generator=g), torch.rand(batch, dim, generator=g) + 1e-3
    ref = O.KLloss({"mean": mean, "std": std}).item()
    assert abs(L.kl(mean, std).item() - ref) < 1e-5 * abs(ref)
    p = torch.sigmoid(torch.randn(shape, generator=g) * 3)
    t = (torch.rand(shape, generator=g) > 0.5).float()
    assert abs(L.bce(p, t).item() - O.avg_ce({"a": p, "b": t}, "a", "b").item()) < 1e-6
    pr = p.clone().requires_grad_(True)
    O.avg_ce({"a": pr, "b": t}, "a", "b").backward()
    assert L.relerr(L.bce_grad(p, t), pr.grad) < 1e-5
    lab = torch.randint(0, shape[1], (shape[0], 1) + shape[2:], generator=g).float()
    assert torch.equal(L.onehot(lab, shape[1]).float(), O.one_hot(lab, shape[1]))
    assert torch.equal(L.onehot(lab + 0.9, shape[1]).float(), O.one_hot(lab, shape[1]))          # truncation, as .long()
    assert torch.equal(L.onehot(-0.5 * torch.ones_like(lab), shape[1])[:, 0], torch.ones_like(lab[:, 0]).double())
    x = torch.rand(shape, generator=g)
    assert torch.equal(L.binarize(x).float(), O.binarize(x))
    assert torch.equal(L.confident_binarize(x).float(), O.confident_binarize(x))


def test_recorded_reference_values():
    g = G.load("kats")
    s1 = torch.tensor([.9, .1, .8, .2, .7, .3, .6, .4]).view(1, 1, 2, 2, 2)
    t1 = torch.tensor([1., 0, 1, 0, 0, 1, 1, 0]).view(1, 1, 2, 2, 2)
    s, t = torch.cat((1 - s1, s1), 1), torch.cat((1 - t1, t1), 1)
    assert abs(L.dice_planes(s, t, 1, 2, 1e-6)["mean"].item() - float(g["dice1"])) < 1e-6
    assert abs(L.dice_planes(s, t, 1, 2, 1e-4)["mean"].item() - float(g["dice3_eps1e4"])) < 1e-6
    assert abs(L.dice_planes(s.reshape(1, 1, -1), t.reshape(1, 1, -1), 0, 1, 1e-6)["mean"].item() - float(g["dice_fn"])) < 1e-6
    assert abs(L.kl(torch.zeros(2, 3), torch.ones(2, 3)).item() - float(g["kl1"])) < 1e-5 * float(g["kl1"])
    kl2 = L.kl(torch.tensor([[1.0, -2.0, 0.5]]), torch.tensor([[0.0, 2.0, 0.5]])).item()
    assert abs(kl2 - float(g["kl2"])) < 1e-5 * float(g["kl2"])
    assert np.array_equal(L.binarize(torch.tensor([.49, .5, .81])).numpy(), g["bin"].astype(np.float64))
    assert np.array_equal(L.confident_binarize(torch.tensor([.1, .2, .5, .8, .81])).float().numpy(), g["cbin"])
    hard = L.hard_onehot(O.kat_scores(1))
    assert np.array_equal(hard.argmax(1).numpy().astype(np.int8), g["dice4_argmax_s"]) and bool((hard.sum(1) == 1).all())
    d4 = L.dice_planes(hard, L.hard_onehot(O.kat_scores(2)), 1, 4, 1e-6)
    assert abs(d4["mean"].item() - float(g["dice4_binary"])) < 1e-6
    assert abs(float(L.bce(torch.tensor([.9, .2, .6, .4]), torch.tensor([1., 0, 1, 0]))) - float(g["bce"])) < 1e-6


def test_hard_onehot_ties_and_nans():
    x = torch.tensor([[0.2, 0.7, 0.7, 0.1], [float("nan"), 3.0, float("nan"), 1.0], [1.0, float("inf"), float("nan"), float("nan")],
                      [-1.0, -1.0, -1.0, -1.0]]).t().reshape(1, 4, 4)
    assert L.hard_onehot(x).argmax(1).tolist() == [[1, 0, 2, 0]]


def test_degenerate_inputs():
    # an all-zero plane pair: Dice 0 and a finite (zero) gradient
    s = torch.rand(2, 2, 3, 4, 5, dtype=torch.float64)
    t = torch.rand(2, 2, 3, 4, 5, dtype=torch.float64)
    s[1, 1], t[1, 1] = 0, 0
    s.requires_grad_(True)
    t.requires_grad_(True)
    d = L.dice_planes(s, t, 0, 2, 1e-6)
    assert d["dice"][1, 1].item() == 0.0
    d["mean"].backward()
    assert bool(torch.isfinite(s.grad).all()) and bool(torch.isfinite(t.grad).all()) and float(s.grad[1, 1].abs().max()) == 0.0
    # saturated probabilities against either target: the -100 clamp, and the 1e-12 floor of the gradient
    p = torch.tensor([0.0, 0.0, 1.0, 1.0])
    t = torch.tensor([0.0, 1.0, 0.0, 1.0])
    assert L.bce(p, t).item() == 50.0
    assert L.bce_grad(p, t).tolist() == [0.0, -0.25e12, 0.25e12, 0.0]
    assert L.bce(torch.tensor([1e-45]), torch.tensor([1.0])).item() == 100.0
    # std = 0: the log(1e-5) value
    assert abs(L.kl(torch.zeros(1, 1), torch.zeros(1, 1)).item() + math.log(1e-5)) < 1e-12
    std = torch.zeros(1, 1, dtype=torch.float64, requires_grad=True)
    L.kl(torch.zeros(1, 1), std).backward()
    assert abs(std.grad.item() + 1e5) < 1e-6
