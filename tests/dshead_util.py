"""The deep-supervision head of csrc/dshead.hip restated in plain fp64 torch: the rule and nothing else.  No project code is used here;
tests/test_host_dshead.py pins these functions before a kernel is compared with them.  Gradients are fp64 autograd on ds_head.

The rule: coarse voxel (z, y, x) of a head at stride s takes the fine label at (s z + s/2, s y + s/2, s x + s/2); logit_k = b_k + sum_c W[k][c] f_c;
p = softmax(logit); final = scale * tests/segloss_util.seg_loss(p, picked label)."""
import torch

from tests import segloss_util as SU


def pick(label, stride):
    """(N, 1, s d, s h, s w) -> (N, 1, d, h, w): the label of every coarse voxel"""
    o = stride // 2
    return label[:, :, o::stride, o::stride, o::stride]


def probabilities(f, weight, bias):
    """channels-last f (N, d, h, w, C), weight (K, C), bias (K,) -> softmax of the 1x1x1 convolution, planar (N, K, d, h, w), fp64"""
    logit = torch.einsum("ndhwc,kc->nkdhw", f.double(), weight.double().reshape(weight.shape[0], -1)) + bias.double()[None, :, None, None, None]
    return torch.softmax(logit, 1)


def ds_head(f, weight, bias, label, stride, scale=1.0, **loss):
    """-> (final, (dice_term, ce_term)), fp64; loss: the keyword arguments of segloss_util.seg_loss"""
    final, terms = SU.seg_loss(probabilities(f, weight, bias), pick(label, stride), **loss)
    return float(scale) * final, terms


def fp32_spelling(f, weight, bias, label, stride, scale=1.0, **loss):
    """the same head as a user of torch would write it in fp32 — F.conv3d 1x1x1 and softmax on the planar fp32 feature map — followed by the oracle's
    loss: what the kernels' accuracy gates are measured against.  f, weight, bias: fp32 leaves; -> (final, (dice_term, ce_term))"""
    k = weight.shape[0]
    logit = torch.nn.functional.conv3d(f.permute(0, 4, 1, 2, 3), weight.reshape(k, -1, 1, 1, 1), bias)
    final, terms = SU.seg_loss(torch.softmax(logit, 1), pick(label, stride), **loss)
    return float(scale) * final, terms
