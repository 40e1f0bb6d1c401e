"""The top-k cross-entropy of csrc/topk.hip restated in plain fp64 torch: the rule and nothing else.  No project code is used here;
tests/test_host_topk.py pins these functions against torch.topk and tests/segloss_util.py before a kernel is compared with them.  Gradients are fp64
autograd on the stated expression (p: an fp64 leaf with requires_grad): tau, K and the membership are constants of it.

The rule: validity, f_v and the Dice term are segloss_util's.  The pool is the valid voxels of the whole batch, N of them.
  key    g_v = fp32(w[l_v] f_v), the fp64 product rounded once; -0.0 and 0.0 are equal
  rank   K = max(1, floor(r N));  N = 0: ce_term = 0
  tau    the K-th largest key;  n_gt = #{g > tau},  n_eq = #{g = tau}
  term   ce_term = (A + (K - n_gt) (E / n_eq)) / K,  A = sum_{g > tau} w f,  E = sum_{g = tau} w f  in fp64
  final = dice_weight dice_term + ce_weight ce_term."""
import math

import torch

from tests import segloss_util as SU


def voxel_losses(p, label, class_weights=None, gamma=0.0):
    """-> (w f of the valid voxels, pooled over the batch in storage order: 1-D fp64, differentiable in p; the valid mask (B, V))"""
    b, c = p.shape[:2]
    p2 = p.double().reshape(b, c, -1)
    valid, cls = SU.classify(label, c)
    w = torch.ones(c, dtype=torch.float64) if class_weights is None else torch.tensor([float(x) for x in class_weights], dtype=torch.float64)
    pl = p2.gather(1, cls[:, None])[:, 0][valid]
    return w[cls[valid]] * SU.focal(pl, gamma), valid


def keys_of(wf):
    """the fp32 keys of fp64 voxel losses; adding 0.0 makes -0.0 a 0.0, so that the two compare AND sort as equal"""
    return wf.detach().float() + 0.0


def rank_of(r, n):
    return max(1, int(math.floor(float(r) * float(n)))) if n else 0


def topk_ce(p, label, r, class_weights=None, gamma=0.0):
    """-> (ce_term, {"N", "K", "tau", "n_gt", "n_eq", "keys": the fp32 keys of the valid voxels, "valid": the mask (B, V)})"""
    wf, valid = voxel_losses(p, label, class_weights, gamma)
    g = keys_of(wf)
    n = g.numel()
    k = rank_of(r, n)
    info = {"N": n, "K": k, "tau": 0.0, "n_gt": 0, "n_eq": 0, "keys": g, "valid": valid}
    if n == 0:
        return p.double().sum() * 0.0, info
    tau = torch.sort(g, descending=True).values[k - 1]
    above, at = g > tau, g == tau
    n_gt, n_eq = int(above.sum()), int(at.sum())
    assert n_gt < k <= n_gt + n_eq
    info.update(tau=float(tau), n_gt=n_gt, n_eq=n_eq)
    A, E = wf[above].sum(), wf[at].sum()
    return (A + (k - n_gt) * (E / n_eq)) / k, info


def seg_loss_topk(p, label, r, dice_weight=1.0, ce_weight=1.0, batch_dice=False, class_weights=None, gamma=0.0, bot=0, top=2, eps=1e-6):
    """-> (final, (dice_term, ce_term), info), all fp64; with C == 1 the channel window is (0, 1)"""
    if p.shape[1] == 1:
        bot, top = 0, 1
    d = SU.dice_term(p, label, bot, top, eps, batch_dice)
    ce, info = topk_ce(p, label, r, class_weights, gamma)
    return float(dice_weight) * d + float(ce_weight) * ce, (d, ce), info
