"""tests/topk_util.py — the fp64 restatement the top-k kernels (csrc/topk.hip) are compared with — pinned against torch.topk,
tests/segloss_util.py and values worked out by hand; and the --ce_topk flag of both entry points.  No GPU."""
import importlib

import pytest
import torch

from tests import segloss_util as SU
from tests import topk_util as TU


def _inputs(seed, b=2, c=3, v=500, ignore=True):
    g = torch.Generator().manual_seed(seed)
    p = torch.softmax(torch.randn(b, c, 1, 1, v, generator=g, dtype=torch.float64) * 2, 1)
    lab = torch.randint(0, c, (b, 1, 1, 1, v), generator=g).float()
    if ignore:
        r = torch.rand(lab.shape, generator=g)
        for j, bad in enumerate((-1.0, 255.0, float("nan"), float(c))):
            lab[(r >= 0.03 * j) & (r < 0.03 * (j + 1))] = bad
    return p, lab


@pytest.mark.parametrize("r", [0.1, 0.5, 0.999])
@pytest.mark.parametrize("weights,gamma", [(None, 0.0), ([0.5, 2.0, 1.25], 2.0)])
def test_tie_free_data_is_the_mean_of_torch_topk(r, weights, gamma):
    p, lab = _inputs(1)
    wf, valid = TU.voxel_losses(p, lab, weights, gamma)
    assert torch.unique(TU.keys_of(wf)).numel() == wf.numel()          # no two fp32 keys equal
    ce, info = TU.topk_ce(p, lab, r, weights, gamma)
    assert info["N"] == int(valid.sum()) == wf.numel() and info["n_eq"] == 1 and info["n_gt"] == info["K"] - 1
    want = torch.topk(wf, info["K"]).values.mean()
    assert abs(ce.item() - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


def test_a_tie_group_straddling_k_is_shared_equally():
    """one sample, 2 classes, 12 valid voxels of class 0: p_0 = 0.125 x 2, 0.5 x 6, 1 x 4, and r = 5/12: K = 5, n_gt = 2, the 6 voxels at ln 2 share 3
    places.  Every tie-break picks 3 of 6 equal values: the same value; the gradient gives each of the six 3/6 of a selected voxel's"""
    pl = torch.tensor([0.5, 1.0, 0.125, 0.5, 0.5, 1.0, 0.5, 1.0, 0.125, 0.5, 0.5, 1.0], dtype=torch.float64)
    p = torch.stack([pl, 1 - pl]).reshape(1, 2, 1, 1, 12).requires_grad_(True)
    lab = torch.zeros(1, 1, 1, 1, 12)
    ce, info = TU.topk_ce(p, lab, 5 / 12)
    assert (info["N"], info["K"], info["n_gt"], info["n_eq"]) == (12, 5, 2, 6)
    ln2 = float(torch.tensor(2.0, dtype=torch.float64).log())
    assert info["tau"] == float(torch.tensor(ln2, dtype=torch.float64).float())
    assert abs(ce.item() - (2 * 3 * ln2 + 3 * ln2) / 5) <= 1e-12
    wf, _ = TU.voxel_losses(p, lab)
    assert abs(ce.item() - float(torch.topk(wf.detach(), 5).values.mean())) <= 1e-12             # torch.topk's tie-break
    assert abs(ce.item() - float(wf.detach().sort(descending=True, stable=True).values[:5].mean())) <= 1e-12
    ce.backward()
    grad = p.grad[0, 0, 0, 0]
    want = torch.where(pl == 0.125, -1 / (5 * pl), torch.where(pl == 0.5, -(3 / 6) / (5 * pl), torch.zeros_like(pl)))
    assert float((grad - want).abs().max()) <= 1e-12
    assert float(p.grad[0, 1].abs().max()) == 0.0


def test_the_rank_rule():
    p, lab = _inputs(2, v=40)
    n = int(SU.classify(lab, 3)[0].sum())
    wf, _ = TU.voxel_losses(p, lab)
    ce, info = TU.topk_ce(p, lab, 1e-9)                                   # r N < 1: K = 1, the single hardest voxel
    assert info["K"] == 1 and abs(ce.item() - float(wf.max())) <= 1e-12
    ce, info = TU.topk_ce(p, lab, 1.0)                                    # r = 1: K = N, the plain mean
    assert info["K"] == n == info["N"] and abs(ce.item() - float(wf.mean())) <= 1e-12
    assert TU.rank_of(0.1, 19) == 1 and TU.rank_of(0.1, 20) == 2 and TU.rank_of(0.5, 7) == 3 and TU.rank_of(1.0, 7) == 7 and TU.rank_of(0.3, 0) == 0
    none = torch.full_like(lab, -1.0)
    p.requires_grad_(True)
    ce, info = TU.topk_ce(p, none, 0.1)                                   # N = 0
    ce.backward()
    assert ce.item() == 0.0 and info["N"] == 0 and info["K"] == 0 and float(p.grad.abs().max()) == 0.0


@pytest.mark.parametrize("gamma", [0.0, 2.0])
def test_unit_weights_and_r_one_is_the_plain_cross_entropy(gamma):
    p, lab = _inputs(3)
    ce, _ = TU.topk_ce(p, lab, 1.0, None, gamma)
    want = SU.ce_term(p, lab, None, gamma)
    assert abs(ce.item() - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    final, (d, c2), _ = TU.seg_loss_topk(p, lab, 1.0, dice_weight=0.6, ce_weight=1.7, batch_dice=True, gamma=gamma, bot=1, top=3, eps=1e-4)
    ref, _ = SU.seg_loss(p, lab, dice_weight=0.6, ce_weight=1.7, batch_dice=True, gamma=gamma, bot=1, top=3, eps=1e-4)
    assert abs(float(final) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))


def test_negative_zero_and_zero_keys_tie():
    """p_l = 1 gives f = -ln 1 = -0.0; a class of weight 0 gives 0 * f = 0.0: one tie group"""
    pl = torch.tensor([1.0, 1.0, 0.25, 0.5, 1.0, 0.5], dtype=torch.float64)
    p = torch.stack([pl, 1 - pl]).reshape(1, 2, 1, 1, 6)
    lab = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 1.0]).reshape(1, 1, 1, 1, 6)          # voxels 3 and 5: class 1, p_1 = 0.5, weight 0
    wf, _ = TU.voxel_losses(p, lab, [1.0, 0.0])
    assert torch.signbit(wf).tolist() == [True, True, False, False, True, False]       # the fp64 products do carry both zeros
    assert not torch.signbit(TU.keys_of(wf)).any()
    ce, info = TU.topk_ce(p, lab, 0.5, [1.0, 0.0])
    assert (info["N"], info["K"], info["tau"], info["n_gt"], info["n_eq"]) == (6, 3, 0.0, 1, 5)
    assert abs(ce.item() - float(-torch.tensor(0.25, dtype=torch.float64).log()) / 3) <= 1e-12


def test_entry_point_flags():
    src, tgt = importlib.import_module("main_source"), importlib.import_module("main_target")
    from vae_segmentation_amd import driver
    a = src.parse(["run", "--method", "seg_train", "--seg_loss", "dice_ce"])
    assert a.ce_topk is None and "topk" not in driver.seg_loss_of(a)
    a = src.parse(["run", "--method", "seg_train", "--seg_loss", "dice_ce", "--ce_topk", "10"])
    assert a.ce_topk == 10.0 and driver.seg_loss_of(a)["topk"] == 10.0 / 100.0
    a = src.parse(["run", "--method", "joint_train", "--seg_loss", "dice_ce", "--ce_topk", "100", "--batch_dice", "--focal_gamma", "2", "--class_weights",
                   "0.5,2", "--boundary_weight", "0.01"])
    assert driver.seg_loss_of(a) == {"dice_weight": 1.0, "ce_weight": 1.0, "batch_dice": True, "class_weights": [0.5, 2.0], "gamma": 2.0, "topk": 1.0}
    for bad in (["--method", "seg_train", "--ce_topk", "10"],                                           # needs --seg_loss dice_ce
                ["--method", "vae_train", "--seg_loss", "dice_ce", "--ce_topk", "10"], ["--method", "vae_train", "--ce_topk", "10"],
                ["--method", "sep_joint_train", "--ce_topk", "10"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--ce_topk", "10", "--deep_supervision", "1"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--ce_topk", "0"], ["--method", "seg_train", "--seg_loss", "dice_ce", "--ce_topk", "-5"],
                ["--method", "seg_train", "--seg_loss", "dice_ce", "--ce_topk", "100.5"], ["--method", "seg_train", "--seg_loss", "dice_ce", "--ce_topk", "nan"]):
        with pytest.raises(SystemExit):
            src.parse(["run"] + bad)
    assert tgt.parse(["run", "--method", "joint_train"]).ce_topk is None
    for method in ("joint_train", "domain_adaptation"):
        with pytest.raises(SystemExit):
            tgt.parse(["run", "--method", method, "--ce_topk", "10"])


def test_train_arguments():
    from vae_segmentation_amd import train as T
    assert T._seg_loss_args({"ce_weight": 0.5, "topk": 0.1}) == {"ce_weight": 0.5, "topk": 0.1}
    assert T._seg_loss_args({"ce_weight": 0.5, "topk": None}) == {"ce_weight": 0.5}
    with pytest.raises(TypeError):
        T._seg_loss_args({"top_k": 0.1})
    with pytest.raises(TypeError, match="deep"):
        T._deep_seg_loss(None, {}, None, None, {"topk": 0.1}, 2, 1e-6)
