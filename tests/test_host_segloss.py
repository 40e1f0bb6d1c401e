"""tests/segloss_util.py — the fp64 restatement the compound-loss kernels (csrc/segloss.hip) are compared with — pinned on the host: its cross-entropy
against torch.nn.functional.nll_loss, its focal factor against the closed form on hand-written voxels, its Dice against tests/loss_util.py and a numpy sum;
the zero-gradient fact that motivates the loss; and the entry points' flags."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import loss_util as L
from tests import segloss_util as SU


def _case(b, c, v, seed=0, ignore=None):
    g = torch.Generator().manual_seed(seed)
    p = torch.softmax(torch.randn(b, c, 1, 1, v, generator=g) * 2, 1)
    lab = torch.randint(0, c, (b, 1, 1, 1, v), generator=g).float()
    if ignore is not None:
        lab[torch.rand(lab.shape, generator=g) < 0.4] = ignore
    return p, lab


@pytest.mark.parametrize("weights", [None, [0.3, 1.0, 2.5]])
@pytest.mark.parametrize("ignore", [None, 255.0, -1.0])
def test_cross_entropy_is_torch_nll_loss(weights, ignore):
    p, lab = _case(2, 3, 97, seed=3, ignore=ignore)
    p64 = p.double()
    ours = SU.ce_term(p64, lab, weights)
    w = None if weights is None else torch.tensor(weights, dtype=torch.float64)
    tgt = lab[:, 0].long()
    tgt[(lab[:, 0] < 0) | (lab[:, 0] >= 3)] = -7
    ref = torch.nn.functional.nll_loss(torch.log(p64), tgt, weight=w, ignore_index=-7)
    assert abs(float(ours) - float(ref)) < 1e-12
    final, (d, ce) = SU.seg_loss(p64, lab, dice_weight=0.0, ce_weight=1.0, class_weights=weights, bot=1, top=3)
    assert float(ce) == float(ours) and abs(float(final) - float(ref)) < 1e-12


def test_focal_gamma_two_closed_form():
    vals = [0.5, 0.25, 0.9, 1.0, 0.125]
    p = torch.tensor([[vals, [1 - x for x in vals]]], dtype=torch.float64).reshape(1, 2, 1, 1, 5)
    lab = torch.zeros(1, 1, 1, 1, 5)
    want = sum(-(1 - x) ** 2 * math.log(x) for x in vals) / len(vals)
    assert abs(float(SU.ce_term(p, lab, None, 2.0)) - want) < 1e-15
    w = [2.0, 5.0]
    lab[0, 0, 0, 0, 1] = 1                                   # voxel 1 is class 1: p_l = 0.75, weight 5
    num = sum(2.0 * -(1 - x) ** 2 * math.log(x) for i, x in enumerate(vals) if i != 1) + 5.0 * -(0.25 ** 2) * math.log(0.75)
    assert abs(float(SU.ce_term(p, lab, w, 2.0)) - num / (2.0 * 4 + 5.0)) < 1e-15
    # and its derivative: d/dp -(1 - p)^2 ln p = 2 (1 - p) ln p - (1 - p)^2 / p
    q = p.clone().requires_grad_(True)
    SU.ce_term(q, torch.zeros(1, 1, 1, 1, 5), None, 2.0).backward()
    for i, x in enumerate(vals):
        assert abs(float(q.grad[0, 0, 0, 0, i]) - (2 * (1 - x) * math.log(x) - (1 - x) ** 2 / x) / 5) < 1e-15
    assert float(q.grad[0, 1].abs().sum()) == 0.0


def test_clamp_at_zero_probability():
    p = torch.tensor([0.0, 1e-45, 0.5, 1.0], dtype=torch.float32).double().reshape(1, 1, 1, 1, 4)       # 1e-45: ln = -103.3, clamped as well
    p = torch.cat([p, 1 - p], 1).requires_grad_(True)
    lab = torch.zeros(1, 1, 1, 1, 4)
    for gamma in (0.0, 2.0):
        p.grad = None
        ce = SU.ce_term(p, lab, None, gamma)
        f2 = (0.5 ** gamma) * math.log(2.0)
        assert abs(ce.item() - (100.0 + 100.0 * (1 - float(p.detach()[0, 0, 0, 0, 1])) ** gamma + f2 + 0.0) / 4) < 1e-12
        ce.backward()
        assert torch.isfinite(p.grad).all()
        g = p.grad[0, 0, 0, 0]
        # where the clamp is active only the focal factor moves: -100 * d(1 - p)^gamma/dp * -1
        assert float(g[0]) == (0.0 if gamma == 0 else -100.0 * gamma / 4)
        assert float(g[3]) == (-1.0 / 4 if gamma == 0 else 0.0)


def test_zero_denominators():
    p, lab = _case(2, 3, 16, seed=1)
    p = p.double().requires_grad_(True)
    none_valid = torch.full_like(lab, 255.0)
    final, (d, ce) = SU.seg_loss(p, none_valid, dice_weight=0.7, ce_weight=1.3, bot=1, top=3)
    assert ce.item() == 0.0 and d.item() == 1.0 and final.item() == 0.7
    final.backward()
    assert float(p.grad.abs().sum()) == 0.0
    only0 = torch.zeros_like(lab)                             # every weight met is 0
    assert SU.ce_term(p, only0, [0.0, 1.0, 1.0]).item() == 0.0
    nan = torch.full_like(lab, float("nan"))
    assert not SU.classify(nan, 3)[0].any() and not SU.classify(torch.full_like(lab, 3.0), 3)[0].any()
    assert SU.classify(torch.full_like(lab, 2.5), 3)[0].all() and int(SU.classify(torch.full_like(lab, 2.5), 3)[1].max()) == 2


@pytest.mark.parametrize("c,bot,top", [(2, 1, 2), (3, 1, 3), (8, 2, 5)])
def test_per_sample_dice_is_loss_util_when_all_labels_are_valid(c, bot, top):
    p, lab = _case(3, c, 61, seed=5)
    ours = SU.dice_term(p.double(), lab, bot, top, 1e-4, False)
    ref, _ = L.dice_loss_sum(p.double(), [L.Label(lab)], [1.0], bot, top, 1e-4)
    assert abs(float(ours) - float(ref)) < 1e-12


def test_batch_dice_is_a_numpy_sum():
    p, lab = _case(3, 4, 53, seed=6, ignore=255.0)
    pn, ln = p.double().numpy().reshape(3, 4, -1), lab.numpy().reshape(3, -1)
    ok = (ln >= 0) & (ln < 4)
    S = np.array([(pn[:, k] * ok).sum() for k in range(4)])
    I = np.array([(pn[:, k] * (ok & (ln == k))).sum() for k in range(4)])
    T = np.array([(ok & (ln == k)).sum() for k in range(4)], dtype=np.float64)
    want = 1 - (2 * I / (S + T + 1e-6))[1:4].mean()
    assert abs(float(SU.dice_term(p.double(), lab, 1, 4, 1e-6, True)) - want) < 1e-12


def test_a_sample_without_foreground_gets_no_gradient_from_per_sample_dice():
    """The defect the compound loss answers: per-sample soft Dice over the foreground channels has an exactly zero gradient on a sample whose label
    holds no foreground.  Batch Dice and the cross-entropy both reach that sample."""
    p, lab = _case(2, 3, 40, seed=7)
    lab[1] = 0
    p64 = p.double().requires_grad_(True)
    final, _ = L.dice_loss_sum(p64, [L.Label(lab)], [1.0], 1, 3, 1e-6)
    final.backward()
    assert float(p64.grad[1].abs().max()) == 0 and float(p64.grad[0].abs().max()) > 0
    for kw in ({"ce_weight": 0.0}, {"ce_weight": 0.0, "batch_dice": True}, {"ce_weight": 1.0}):
        q = p.double().requires_grad_(True)
        f, _ = SU.seg_loss(q, lab, bot=1, top=3, **kw)
        f.backward()
        if kw == {"ce_weight": 0.0}:
            assert float(q.grad[1].abs().max()) == 0 and torch.equal(q.grad, p64.grad)
        else:
            assert float(q.grad[1].abs().max()) > 0, kw


def test_entry_point_flags():
    src, tgt = importlib.import_module("main_source"), importlib.import_module("main_target")
    a = src.parse(["run", "--method", "seg_train"])
    assert a.seg_loss == "dice" and a.ce_weight == 1.0 and a.batch_dice is False and a.focal_gamma == 0.0 and a.class_weights is None
    a = src.parse(["run", "--method", "seg_train", "--seg_loss", "dice_ce", "--batch_dice", "--ce_weight", "0.5", "--focal_gamma", "2",
                   "--class_weights", "0.5,2"])
    assert a.seg_loss == "dice_ce" and a.batch_dice is True and a.ce_weight == 0.5 and a.focal_gamma == 2.0 and a.class_weights == [0.5, 2.0]
    from vae_segmentation_amd import driver
    assert driver.seg_loss_of(a) == {"dice_weight": 1.0, "ce_weight": 0.5, "batch_dice": True, "class_weights": [0.5, 2.0], "gamma": 2.0}
    assert driver.seg_loss_of(src.parse(["run", "--method", "seg_train"])) is None
    assert src.parse(["run", "--method", "joint_train", "--seg_loss", "dice_ce", "--pan_index", "1,2", "--class_weights", "1,2,3"]).class_weights == [1, 2, 3]
    for bad in (["--method", "vae_train", "--seg_loss", "dice_ce"], ["--method", "vae_train", "--batch_dice"], ["--seg_loss", "dice_ce"],
                ["--method", "sep_joint_train", "--ce_weight", "2"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--class_weights", "1,2,3"],      # n_class is 2
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--class_weights", "1"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--class_weights", "1,-2"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--focal_gamma", "-1"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--ce_weight", "nan"],
                ["--method", "seg_train", "--seg_loss", "ce"]):
        with pytest.raises(SystemExit):
            src.parse(["run"] + bad)
    assert tgt.parse(["run", "--method", "joint_train"]).seg_loss == "dice"
    for method in ("joint_train", "domain_adaptation"):
        with pytest.raises(SystemExit):
            tgt.parse(["run", "--method", method, "--seg_loss", "dice_ce"])
