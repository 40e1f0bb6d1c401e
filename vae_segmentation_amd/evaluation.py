"""Loss / metric functions of the reference's utils/evaluation.py (and their duplicates in
main_source.py:133-182) on the libvaeseg kernels.  Same names, arguments and dict-in conventions;
``eps`` selects between the two epsilons that coexist in the reference:
utils/evaluation.py uses 1e-6, main_source.py's own copy 1e-4."""
import torch

from . import ops

EPS_EVALUATION = 1e-6
EPS_MAIN_SOURCE = 1e-4


def dice(A, B):
    """utils/evaluation.py:6-7 — whole-tensor soft dice (eps 1e-6)."""
    a = A.reshape(1, 1, -1)
    b = B.reshape(1, 1, -1)
    pad = (-a.shape[-1]) % 4
    if pad:
        a = torch.nn.functional.pad(a, (0, pad))
        b = torch.nn.functional.pad(b, (0, pad))
    return ops.Dice.apply(a, b, 0, 1, EPS_EVALUATION, True)


def binarize(A):
    """utils/evaluation.py:9-10."""
    return ops.binarize(A, mode=0)


def confident_binarize(A, max=0.8, min=0.2):
    """utils/evaluation.py:12-18."""
    return ops.binarize(A, mode=1, lo=min, hi=max)


def avg_ce(data_dict, source_key='align_lung', target_key='source_lung'):
    """utils/evaluation.py:29-39."""
    source_mask = data_dict[source_key]
    target_mask = data_dict[target_key]
    if not isinstance(source_mask, list):
        source_mask = [source_mask]
    total = 0
    for im in source_mask:
        total = total + ops.BCE.apply(im, target_mask)
    return total / len(source_mask)


def KLloss(data_dict, mean_key='mean', std_key='std'):
    """utils/evaluation.py:42-45."""
    return ops.KL.apply(data_dict[mean_key], data_dict[std_key])


def _hard_onehot(mask):
    """argmax over channels -> one-hot (validation path, utils/evaluation.py:58-64), any number of classes: vs_hard_onehot
    (ties go to the first maximal channel, as torch.argmax resolves them)."""
    return ops.hard_onehot(mask)


def avg_dsc(data_dict, source_key='align_lung', target_key='source_lung', binary=False, topindex=2, botindex=0,
            pad=[0, 0, 0], return_mean=True, detach=False, eps=EPS_EVALUATION):
    """utils/evaluation.py:48-80 (eps=1e-6) / main_source.py:150-182 (eps=1e-4)."""
    source_mask = data_dict[source_key]
    target_mask = data_dict[target_key]
    if detach:
        target_mask = target_mask.detach()
    if binary:
        source_mask = _hard_onehot(source_mask)
        target_mask = _hard_onehot(target_mask)
    channels = source_mask.shape[1]
    if channels > 1:
        bot, top = botindex, min(topindex, channels)
    else:
        bot, top = 0, 1
    return ops.Dice.apply(source_mask, target_mask, bot, top, eps, return_mean)


def keep_largest_components(A, k=1, min_size=0, connectivity=26):
    """utils/utils.py:776-796 (predict_vol step 2) on the device: per (n, c) plane of a planar (N, C, D, H, W) mask, binarize (>= 0.5), keep the k largest
    connected components that hold at least min_size voxels, re-binarise.  predict_vol itself hard-codes k=2, min_size=10000, full connectivity."""
    return ops.keep_largest(A, k=k, min_size=min_size, connectivity=connectivity)


def check_connection(tumor_index, image):
    """utils/utils.py:38-57 with the flood fill on the device: tumor_index is an (L, 3) host array of voxel indices into the volume `image`;
    -> numpy array of L component numbers (26-connectivity), 1, 2, ... in the order in which tumor_index first reaches each component — the
    reference's return value."""
    import numpy as np
    idx = np.asarray(tumor_index).reshape(-1, 3).astype(np.int64)
    shape = tuple(np.shape(image))
    mask = np.zeros(shape, dtype=np.float32)
    mask[idx[:, 0], idx[:, 1], idx[:, 2]] = 1
    labels, _, _ = ops.cc_label(torch.from_numpy(mask).cuda().view((1, 1) + shape), connectivity=26)
    cc = labels.view(shape).cpu().numpy()[idx[:, 0], idx[:, 1], idx[:, 2]]
    # the device numbers components by their first voxel in raster order; the reference by their first appearance in tumor_index
    _, first = np.unique(cc, return_index=True)
    order = np.empty(int(cc.max()) + 1 if cc.size else 1, dtype=np.int64)
    order[cc[np.sort(first)]] = np.arange(1, len(first) + 1)
    out = order[cc] if cc.size else cc
    return out.astype(np.asarray(image).dtype)


def _planar(X):
    if X.dim() == 3:
        return X.reshape((1, 1) + tuple(X.shape)), True
    if X.dim() == 5:
        return X, False
    raise ValueError("expected a (D, H, W) volume or a planar (N, C, D, H, W) tensor, got shape %s" % (tuple(X.shape),))


def surface_metrics(A, B, spacing=None, connectivity=6):
    """ASSD, Hausdorff distance and HD95 of the binarised (>= 0.5) masks A (prediction) against B (label) in medpy's convention
    (medpy.metric.binary.assd / hd / hd95: surfaces by binary erosion, Euclidean distances under `spacing` = (sz, sy, sx), the 95th percentile of the
    union of both directed distance sets), per (n, c) plane, on the device (csrc/surface.hip): no host copy, no synchronisation.
    A, B: (D, H, W) or (N, C, D, H, W).  -> the dict of ops.surface_distances, 0-d tensors for a single volume, (N, C) otherwise; a plane in which
    either surface is empty gives NaN where medpy raises."""
    a, single = _planar(A)
    b, _ = _planar(B)
    rec = ops.surface_distances(a.detach(), b.detach(), spacing=spacing, connectivity=connectivity)
    return {k: v.reshape(()) for k, v in rec.items()} if single else rec


def assd(A, B, spacing=None, connectivity=6):
    """average symmetric surface distance (medpy.metric.binary.assd)"""
    return surface_metrics(A, B, spacing, connectivity)["assd"]


def hd(A, B, spacing=None, connectivity=6):
    """Hausdorff distance (medpy.metric.binary.hd)"""
    return surface_metrics(A, B, spacing, connectivity)["hd"]


def hd95(A, B, spacing=None, connectivity=6):
    """95th percentile of the Hausdorff distance (medpy.metric.binary.hd95)"""
    return surface_metrics(A, B, spacing, connectivity)["hd95"]
