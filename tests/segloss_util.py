"""The compound segmentation loss of csrc/segloss.hip restated in plain fp64 torch: the rule and nothing else.  No project code is used here;
tests/test_host_segloss.py pins these functions against torch.nn.functional.nll_loss, tests/loss_util.py and hand-written values before a kernel is compared
with them.  Gradients are fp64 autograd on seg_loss (p: an fp64 leaf with requires_grad).

The rule: a voxel is valid iff 0 <= label < C (compared in fp32; NaN is not), its class is trunc(label); every other voxel adds to no sum.  Over the valid
voxels S[b][c] = sum p_c, I[b][c] = sum_{l=c} p_c, T[b][c] = #{l = c};
  per sample: dice = mean_b mean_{c in [bot, top)} 2 I / (S + T + eps);   batch: dice = mean_c 2 sum_b I / (sum_b S + sum_b T + eps);   dice_term = 1 - dice
  f_v = -(1 - p_l)^gamma max(ln p_l, -100);   ce_term = sum w[l_v] f_v / sum w[l_v], 0 when the denominator is 0
  final = dice_weight dice_term + ce_weight ce_term."""
import torch


def classify(label, channels):
    """(B, 1, ...) fp32-comparable labels -> (valid mask (B, V) bool, class index (B, V) long, 0 where not valid)"""
    l32 = label.detach().float().reshape(label.shape[0], -1)
    valid = (l32 >= 0) & (l32 < channels)
    cls = torch.where(valid, l32, torch.zeros_like(l32)).long()
    return valid, cls


def sums(p, label):
    """S, I, T as (B, C) fp64 tensors (S and I differentiable in p)"""
    b, c = p.shape[:2]
    p2 = p.double().reshape(b, c, -1)
    valid, cls = classify(label, c)
    v = valid.double()[:, None]
    hot = torch.stack([((cls == k) & valid).double() for k in range(c)], 1)
    return (p2 * v).sum(2), (p2 * hot).sum(2), hot.sum(2)


def dice_term(p, label, bot, top, eps, batch_dice):
    S, I, T = sums(p, label)
    if batch_dice:
        d = 2 * I.sum(0) / (S.sum(0) + T.sum(0) + eps)
        return 1 - d[bot:top].mean()
    d = 2 * I / (S + T + eps)
    return 1 - d[:, bot:top].mean(1).mean()


def focal(pl, gamma):
    """-(1 - p)^gamma max(ln p, -100); where the clamp is active (ln p < -100, p = 0 included) the logarithm is the constant -100: derivative 0, not 0 * inf"""
    active = torch.log(pl.detach()) < -100.0
    lg = torch.where(active, torch.full_like(pl, -100.0), torch.log(torch.where(active, torch.ones_like(pl), pl)))
    if gamma == 0:
        return -lg
    return -((1 - pl) ** float(gamma)) * lg


def ce_term(p, label, class_weights=None, gamma=0.0):
    b, c = p.shape[:2]
    p2 = p.double().reshape(b, c, -1)
    valid, cls = classify(label, c)
    w = torch.ones(c, dtype=torch.float64) if class_weights is None else torch.tensor([float(x) for x in class_weights], dtype=torch.float64)
    pl = p2.gather(1, cls[:, None])[:, 0][valid]
    wl = w[cls[valid]]
    den = wl.sum()
    if float(den) == 0.0:
        return p2.sum() * 0.0
    return (wl * focal(pl, gamma)).sum() / den


def seg_loss(p, label, dice_weight=1.0, ce_weight=1.0, batch_dice=False, class_weights=None, gamma=0.0, bot=0, top=2, eps=1e-6):
    """-> (final, (dice_term, ce_term)), all fp64; with C == 1 the channel window is (0, 1)"""
    if p.shape[1] == 1:
        bot, top = 0, 1
    d = dice_term(p, label, bot, top, eps, batch_dice)
    ce = ce_term(p, label, class_weights, gamma)
    return float(dice_weight) * d + float(ce_weight) * ce, (d, ce)


def relerr(a, b):
    """norm-wise relative error: max |a - b| / max |b|"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))
