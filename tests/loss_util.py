"""The loss and label operations of csrc/loss.hip and csrc/softmax.hip restated in plain fp64 torch / numpy: the formulas and nothing else.  No project code is used
here; tests/test_host_loss.py pins these functions against the oracle and the recorded reference values before a kernel is compared with them.
Gradients are fp64 autograd on these functions (inputs: fp64 leaves with requires_grad), except BCE's, whose clamped form nn.BCELoss defines."""
import numpy as np
import torch


class Label:
    """a Dice target given as its label volume (B, 1, ...): floats, truncated toward zero as .long() does; a value that is no class matches none"""

    def __init__(self, volume):
        self.volume = volume


def onehot(label, n_class):
    """(B, 1, ...) labels -> fp64 one-hot (B, n_class, ...), class = trunc(label)"""
    k = torch.trunc(label.detach().double())
    return torch.cat([(k == c).double() for c in range(n_class)], 1)


def dice_planes(s, t, bot, top, eps):
    """per (b, c): I = sum s t, S = sum s, T = sum t, dice = 2I / (S + T + eps); per-sample means over the channels [bot, top), and their batch mean"""
    s, t = s.double(), t.double()
    b, c = s.shape[:2]
    s2, t2 = s.reshape(b, c, -1), t.reshape(b, c, -1)
    I, S, T = (s2 * t2).sum(2), s2.sum(2), t2.sum(2)
    d = 2 * I / (S + T + eps)
    per = d[:, bot:top].mean(1)
    return {"I": I, "S": S, "T": T, "dice": d, "per_sample": per, "mean": per.mean()}


def dice_loss_sum(s, targets, weights, bot, top, eps):
    """sum_j w_j (1 - mean_{b, c in [bot, top)} dice_j) -> (final, [1 - mean dice_j ...]); a target is a tensor or a Label"""
    terms = []
    for t in targets:
        if isinstance(t, Label):
            t = onehot(t.volume, s.shape[1])
        terms.append(1 - dice_planes(s, t, bot, top, eps)["mean"])
    final = sum(float(w) * term for w, term in zip(weights, terms))
    return final, terms


def _bce_logs(p):
    p32 = p.detach().float()
    q = (1 - p32).double()                      # 1 - p is formed in fp32 (as nn.BCELoss does on fp32 input) before widening
    p64 = p32.double()
    return p64, q, torch.log(p64).clamp_min(-100.0), torch.log(q).clamp_min(-100.0)       # log(0) = -inf -> -100


def bce(p, t):
    """mean of -(t max(log p, -100) + (1 - t) max(log(1 - p), -100))"""
    _, _, lp, lq = _bce_logs(p)
    t = t.detach().double()
    return (-(t * lp + (1 - t) * lq)).mean()


def bce_grad(p, t):
    """d bce / d p = (p - t) / max(p (1 - p), 1e-12) / N: the clamped form nn.BCELoss defines (autograd of the clamped logarithms would give 0 at p = 0, 1)"""
    p64, q, _, _ = _bce_logs(p)
    return (p64 - t.detach().double()) / (p64 * q).clamp_min(1e-12) / p64.numel()


def kl(mean, std):
    """mean over the batch of 0.5 (sum std^2 + sum mean^2 - 2 sum log(std + 1e-5)); (batch, dim) inputs"""
    m, s = mean.double(), std.double()
    return (0.5 * ((s * s).sum(1) + (m * m).sum(1) - 2 * torch.log(s + 1e-5).sum(1))).mean()


def reparam(mean, std, noise, scale):
    return mean.double() + noise.double() * std.double() * scale


def softmax(logits, nc):
    """softmax over the first nc channels (dim 1) of planar logits"""
    return torch.softmax(logits.double()[:, :nc], 1)


def hard_onehot(x):
    """(B, C, ...) scores -> fp64 one-hot of the first maximal channel; a NaN counts as the maximum, and the first NaN wins"""
    a = x.detach().double().numpy()
    nan = np.isnan(a)
    arg = np.where(nan.any(1), nan.argmax(1), np.where(nan, -np.inf, a).argmax(1))
    out = np.zeros_like(a)
    np.put_along_axis(out, arg[:, None], 1.0, 1)
    return torch.from_numpy(out)


def binarize(a):
    return (a.detach().double() >= 0.5).double()


def confident_binarize(a, hi=0.8, lo=0.2):
    """above hi -> 1, below lo -> 0, the rest unchanged.  The comparison is made in the input's precision: a Python threshold compared with an fp32
    tensor is rounded to fp32 first, so the fp32 value nearest 0.8 is NOT above hi = 0.8."""
    a = a.detach()
    hi_, lo_ = torch.tensor(hi, dtype=a.dtype).double(), torch.tensor(lo, dtype=a.dtype).double()
    v = a.double()
    return torch.where(v > hi_, torch.ones_like(v), torch.where(v < lo_, torch.zeros_like(v), v))


def relerr(a, b):
    """norm-wise relative error of tests/test_gpu_ops.py: max |a - b| / max |b|"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-20))
