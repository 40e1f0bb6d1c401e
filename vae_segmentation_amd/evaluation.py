"""Loss / metric functions of the reference's utils/evaluation.py (and their duplicates in
main_source.py:133-182) on the libvaeseg kernels.  Same names, arguments and dict-in conventions;
``eps`` selects between the two epsilons that coexist in the reference:
utils/evaluation.py uses 1e-6, main_source.py's own copy 1e-4."""
import torch

from . import ops
from . import volume as V       # not `volume`: histogram, SlidingWindow.__call__ and sliding_window_predict take a parameter of that name

EPS_EVALUATION = 1e-6
EPS_MAIN_SOURCE = 1e-4


def dice(A, B):
    """utils/evaluation.py:6-7 — whole-tensor soft dice (eps 1e-6)."""
    return ops.Dice.apply(A.reshape(1, 1, -1), B.reshape(1, 1, -1), 0, 1, EPS_EVALUATION, True)


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
    return V.keep_largest(A, k=k, min_size=min_size, connectivity=connectivity)


def check_connection(tumor_index, image):
    """utils/utils.py:38-57 with the flood fill on the device: tumor_index is an (L, 3) host array of voxel indices into the volume `image`;
    -> numpy array of L component numbers (26-connectivity), 1, 2, ... in the order in which tumor_index first reaches each component — the
    reference's return value."""
    import numpy as np
    idx = np.asarray(tumor_index).reshape(-1, 3).astype(np.int64)
    shape = tuple(np.shape(image))
    mask = np.zeros(shape, dtype=np.float32)
    mask[idx[:, 0], idx[:, 1], idx[:, 2]] = 1
    labels, _, _ = V.cc_label(torch.from_numpy(mask).cuda().view((1, 1) + shape), connectivity=26)
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
    rec = V.surface_distances(a.detach(), b.detach(), spacing=spacing, connectivity=connectivity)
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


def signed_distance(label_volume, n_class, spacing=None):
    """The signed distance maps of a (D, H, W) label volume (values 0..n_class-1; anything else belongs to no class) -> fp32 (n_class, D, H, W) on the
    device (ops.signed_distance): phi_c is the Euclidean distance, under `spacing` = (sz, sy, sx), to the nearest voxel of class c outside
    the class and 1 - the distance to the nearest voxel outside it inside — Kervadec's one_hot2dist; a class that is absent or fills the volume gives 0."""
    if label_volume.dim() != 3:
        raise ValueError("expected a (D, H, W) label volume, got shape %s" % (tuple(label_volume.shape),))
    return V.signed_distance(label_volume.detach().reshape((1, 1) + tuple(label_volume.shape)), n_class, spacing=spacing)[0]


# ----------------------------------------------------------------------------------------------------
# the objects of a label: per-component measurements, the class confusion matrix and lesion-wise detection scores on the device
# (csrc/regions.hip).  The reference has no counterpart; tests/regions_util.py restates the definitions with scipy.ndimage and numpy.
# ----------------------------------------------------------------------------------------------------
LESION_RECORD_FIELDS = ("n_gt", "n_pred", "tp", "fn", "fp", "sensitivity", "precision", "f1", "overflow")
LESION_TABLE_ROWS = 2047          # components per side the lesion table can hold: (rows + 1)^2 <= 2^22 (ops.contingency)


def _spacing3(spacing, what):
    if spacing is None:
        return None
    try:
        vals = tuple(float(s) for s in spacing)
    except (TypeError, ValueError):
        vals = ()
    if len(vals) != 3 or not all(v > 0 and v < float("inf") for v in vals):
        raise ValueError("%s: spacing is (sz, sy, sx), positive and finite, got %r" % (what, spacing))
    return vals


def _components(X, connectivity, what):
    """(labels int32, sizes int32 (N, C, maxk)) of the binarised mask's components"""
    V._check_connectivity(connectivity, what)
    labels, _, sizes = V.cc_label(X.detach(), connectivity=connectivity)
    return labels, sizes


def region_props(mask, spacing=None, connectivity=26, max_components=4096):
    """The connected components of the binarised (>= 0.5) mask — (D, H, W), or per plane of a planar (N, C, D, H, W) tensor — and their measurements:
    ops.cc_label -> ops.region_props, on the device, no host copy.  -> the dict of ops.region_props for the components 1..max_components in
    scipy.ndimage.label's numbering ("count", "bbox", "centroid", "sums", "overflow": voxels of components beyond max_components) plus
    "volume" fp64 = count x sz x sy x sx (voxels without a spacing), "n_components" int32 and "labels" int32, the label volume.  With
    spacing = (sz, sy, sx) the centroid is in the spacing's unit (index x spacing), otherwise in voxels; NaN for a component that does not exist."""
    sp = _spacing3(spacing, "region_props")
    V._rows(max_components, "region_props: max_components", 1)
    x, single = _planar(mask)
    V._check_connectivity(connectivity, "region_props")
    labels, counts, _ = V.cc_label(x.detach(), connectivity=connectivity)
    out = V.region_props(labels, max_components=max_components)
    unit = 1.0
    if sp is not None:
        out["centroid"] = out["centroid"] * torch.tensor(sp, dtype=torch.float64, device=labels.device)
        unit = sp[0] * sp[1] * sp[2]
    out["volume"] = out["count"].double() * unit
    out["n_components"], out["labels"] = counts, labels
    return {k: v[0, 0] for k, v in out.items()} if single else out


def _ratio(num, den, other):
    """num / den in fp64; where den is 0 (num is then 0 too): 1.0 if the other side is empty as well, else 0.0"""
    safe = torch.where(den == 0, torch.ones_like(den), den)
    return torch.where(den == 0, (other == 0).double(), num.double() / safe.double())


def _label_map(X, what):
    x, single = _planar(X)
    if x.is_floating_point() or x.dtype == torch.bool:
        if x.dtype == torch.bool:
            raise TypeError("%s: label maps hold integers, got a bool tensor" % what)
        x = x.round()
    return x.detach().to(torch.int32).contiguous(), single


def confusion(pred_label, gt_label, n_class):
    """The confusion matrix of two label maps with classes 0..n_class-1 — (D, H, W), or per plane of (N, C, D, H, W); any integer dtype, or floats
    holding integers — from ONE read of both (ops.contingency), and the per-class scores derived from it on the device.
    -> {"table": int64 (..., n_class, n_class), table[i, j] = voxels predicted i with label j; "dice", "iou", "sensitivity", "precision": fp64
        (..., n_class); "overflow": int32, voxels whose class is outside [0, n_class) on either side (in no cell)}.
    With tp = table[k, k], p = the row sum (predicted k) and g = the column sum (labelled k): dice = 2 tp / (p + g), iou = tp / (p + g - tp),
    sensitivity = tp / g, precision = tp / p.  A class that is empty on both sides scores 1.0 everywhere; sensitivity of a class nobody labelled but
    somebody predicted — and precision the other way round — is 0.0."""
    k = V._rows(n_class, "confusion: n_class", 1)
    a, single = _label_map(pred_label, "confusion")
    b, _ = _label_map(gt_label, "confusion")
    table, overflow = V.contingency(a, b, k - 1, k - 1)
    tp = torch.diagonal(table, dim1=-2, dim2=-1)
    p, g = table.sum(-1), table.sum(-2)
    out = {"table": table, "dice": _ratio(2 * tp, p + g, p + g), "iou": _ratio(tp, p + g - tp, p + g), "sensitivity": _ratio(tp, g, p),
           "precision": _ratio(tp, p, g), "overflow": overflow}
    return {k_: v[0, 0] for k_, v in out.items()} if single else out


def lesion_metrics(pred, gt, connectivity=26, min_overlap=1, min_size=0, max_components=4096):
    """Lesion-wise detection scores of the binarised (>= 0.5) masks pred against gt — (D, H, W), or per plane of (N, C, D, H, W) — on the device, without
    a synchronisation.  P = ops.cc_label(pred), G = ops.cc_label(gt); components of fewer than min_size voxels are dropped from both sides;
    T = ops.contingency(P, G).  Reference lesion j is DETECTED iff it shares at least min_overlap voxels with the predicted components together
    (sum_i T[i, j] >= min_overlap, i >= 1); predicted component i is a FALSE POSITIVE iff it shares no voxel with any reference lesion.
    -> a dict over LESION_RECORD_FIELDS of (N, C) device tensors (0-d for a single volume): n_gt, n_pred (components that remain), tp (detected lesions),
    fn = n_gt - tp, fp — int64; sensitivity = tp / n_gt, precision = (n_pred - fp) / n_pred, f1 = 2 tp / (2 tp + fp + fn) — fp64, a ratio with
    denominator 0 being 1.0 when the other side is empty too and 0.0 otherwise; overflow — int32, voxels of components numbered above
    min(max_components, 2047), the most the table holds per side: the record is then not valid, and lesion_record_to_host raises."""
    V._check_connectivity(connectivity, "lesion_metrics")
    V._rows(max_components, "lesion_metrics: max_components", 1)
    V._rows(min_overlap, "lesion_metrics: min_overlap", 1)
    V._rows(min_size, "lesion_metrics: min_size", 0)
    a, single = _planar(pred)
    b, _ = _planar(gt)
    if a.shape != b.shape:
        raise ValueError("lesion_metrics: the two masks differ in shape: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    P, sizes_p = _components(a, connectivity, "lesion_metrics")
    G, sizes_g = _components(b, connectivity, "lesion_metrics")
    rows = min(max_components, LESION_TABLE_ROWS, sizes_p.shape[-1])
    table, overflow = V.contingency(P, G, rows, rows)
    least = max(min_size, 1)
    keep_p, keep_g = sizes_p[..., :rows] >= least, sizes_g[..., :rows] >= least            # a dropped component: its row / column is not looked at
    shared = table[..., 1:, 1:] * (keep_p.unsqueeze(-1) & keep_g.unsqueeze(-2))
    n_pred, n_gt = keep_p.sum(-1), keep_g.sum(-1)
    tp = (shared.sum(-2) >= min_overlap).sum(-1)
    fp = (keep_p & (shared.sum(-1) == 0)).sum(-1)
    fn = n_gt - tp
    out = {"n_gt": n_gt, "n_pred": n_pred, "tp": tp, "fn": fn, "fp": fp, "sensitivity": _ratio(tp, n_gt, n_pred),
           "precision": _ratio(n_pred - fp, n_pred, n_gt), "f1": _ratio(2 * tp, 2 * tp + fp + fn, n_gt + n_pred), "overflow": overflow}
    assert tuple(out) == LESION_RECORD_FIELDS
    return {k: v[0, 0] for k, v in out.items()} if single else out


def lesion_record_to_host(record):
    """a lesion_metrics record as nested Python lists (numbers for a single volume), one host copy per field; RuntimeError when a plane had more
    components than the table holds (overflow != 0): its counts would be wrong"""
    host = {k: record[k].cpu() for k in LESION_RECORD_FIELDS}
    if bool((host["overflow"] != 0).any()):
        raise RuntimeError("lesion_metrics: %d voxels belong to components beyond the table's rows: the record is not valid (max_components counts "
                           "components before the min_size filter, at most %d per side)" % (int(host["overflow"].sum()), LESION_TABLE_ROWS))
    return {k: v.tolist() for k, v in host.items()}


# ----------------------------------------------------------------------------------------------------
# the intensities of a volume: histograms, joint histograms and mutual information on the device (csrc/hist.hip).  mutual_information_3d is the
# reference's utils/utils.py:804-845; tests/hist_util.py restates the binning rule and the formula with numpy and scipy.
# ----------------------------------------------------------------------------------------------------
def _intensities(X, what):
    """(planar contiguous fp32 tensor, single): float32 is what the kernels read; other floating-point and integer dtypes are converted"""
    if not isinstance(X, torch.Tensor) or X.dtype == torch.bool or X.is_complex():
        raise TypeError("%s: expected a real-valued tensor, got %s" % (what, getattr(X, "dtype", type(X))))
    x, single = _planar(X)
    return x.detach().to(torch.float32).contiguous(), single


def histogram(volume, bins, range=None, mask=None):
    """The intensity histogram of a volume — (D, H, W), or per plane of (N, C, D, H, W) — on the device, optionally inside a mask (ops.histogram).
    Edges are np.linspace(lo, hi, bins + 1) in fp64, a voxel promoted to fp64 is in bin i iff e_i <= x < e_{i+1} (the last edge belongs to the last bin);
    range=None takes lo / hi from the finite voxels of each plane, on the device.  mask: a 0 / 1 volume of the same shape (foreground: value >= 0.5).
    -> {"table": int64 (..., bins) — with a mask the voxels inside it, and then also "complement": the voxels where the mask is 0;
        "edges": fp64 (..., bins + 1); "outside": int64, voxels that are NaN, +-inf or out of range (in no bin, whatever the mask says)}."""
    x, single = _intensities(volume, "histogram")
    lab = None
    if mask is not None:
        m, _ = _planar(mask)
        if m.shape != x.shape:
            raise ValueError("histogram: the mask's shape %s is not the volume's %s" % (tuple(mask.shape), tuple(volume.shape)))
        lab = (m.detach() >= 0.5).to(torch.int32).contiguous()
    rec = V.histogram(x, bins, range=range, labels=lab, rows=0 if lab is None else 1)
    out = {"table": rec["table"][:, :, -1], "edges": rec["edges"], "outside": rec["outside"]}
    if lab is not None:
        out["complement"] = rec["table"][:, :, 0]
    return {k: v[0, 0] for k, v in out.items()} if single else out


def joint_histogram(a, b, bins=256, range=None):
    """The joint intensity histogram of two volumes of one shape — (D, H, W), or per plane of (N, C, D, H, W) — on the device (ops.joint_histogram):
    np.histogram2d with histogram's binning rule per variable.  bins: an integer or (bins_a, bins_b); range: None (from the data) or
    ((lo_a, hi_a), (lo_b, hi_b)).  -> {"table": int64 (..., bins_a, bins_b), "edges_x", "edges_y": fp64, "outside": int64}."""
    x, single = _intensities(a, "joint_histogram")
    y, _ = _intensities(b, "joint_histogram")
    if x.shape != y.shape:
        raise ValueError("joint_histogram: the two volumes differ in shape: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    rec = V.joint_histogram(x, y, bins=bins, range=range)
    return {k: v[0, 0] for k, v in rec.items()} if single else rec


def mutual_information_3d(x, y, sigma=1, normalized=True):
    """utils/utils.py:804-845 on the device: the (normalised) mutual information of two variables from their 256 x 256 joint histogram, smoothed with a
    Gaussian of `sigma` (scipy.ndimage.gaussian_filter, mode "constant"), Studholme's measure when normalized.
    x, y: device tensors of any equal shape; they are flattened, as the reference takes 1-D arrays, and binned as ONE plane with bounds from the data.
    The kernels read float32 (another dtype is converted to it first); every value is promoted to fp64 before binning, and the edges are the fp64 values
    np.linspace(min, max, 257) — the bins numpy gives for float64 inputs.  -> a 0-d fp64 device tensor; nothing is copied to the host or synchronised."""
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError("mutual_information_3d: x and y are device tensors, got %s and %s" % (type(x).__name__, type(y).__name__))
    if x.shape != y.shape or x.numel() == 0:
        raise ValueError("mutual_information_3d: x and y have one non-empty shape, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    a, _ = _intensities(x.reshape(1, 1, 1, 1, -1), "mutual_information_3d")
    b, _ = _intensities(y.reshape(1, 1, 1, 1, -1), "mutual_information_3d")
    rec = V.joint_histogram(a, b, bins=(256, 256), range=None)
    return V.mutual_information(rec["table"], sigma=sigma, normalized=normalized)[0, 0]


# ----------------------------------------------------------------------------------------------------
# binary morphology and hole filling on the device (csrc/morph.hip): scipy.ndimage's operators without the host detour
# ----------------------------------------------------------------------------------------------------
def _morph(name, X, **kw):
    x, single = _planar(X)
    out = getattr(V, name)(x.detach(), **kw)
    return out[0, 0] if single else out


def binary_dilation(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_dilation of the binarised (>= 0.5) mask, (D, H, W) or per plane of (N, C, D, H, W): connectivity 6 is
    generate_binary_structure(3, 1), 26 is (3, 3).  -> fp32 0 / 1 of the same shape."""
    return _morph("binary_dilation", input, iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_erosion(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_erosion, as binary_dilation"""
    return _morph("binary_erosion", input, iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_opening(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_opening (erode^n then dilate^n), as binary_dilation"""
    return _morph("binary_opening", input, iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_closing(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_closing (dilate^n then erode^n), as binary_dilation"""
    return _morph("binary_closing", input, iterations=iterations, connectivity=connectivity, border_value=border_value)


def fill_holes(input, connectivity=6):
    """scipy.ndimage.binary_fill_holes of the binarised mask, (D, H, W) or per plane of (N, C, D, H, W): background that does not reach the outside of
    the volume through `connectivity`-neighbours becomes foreground."""
    return _morph("fill_holes", input, connectivity=connectivity)


def get_synthesis_mask(data_dict, field='venous'):
    """utils/utils.py:647-655 on device tensors: bone (> 200 HU) dilated twice with the 6-neighbourhood and bowel gas (< 0 HU) are excluded;
    data_dict[field + '_syn_mask'] = (1 - bowel) * (1 - bone), fp32."""
    v = data_dict[field]
    bone = binary_dilation((v > 200).float(), iterations=2)
    bowel = (v < 0).float()
    data_dict[field + '_syn_mask'] = ((1 - bowel) * (1 - bone)).float()
    return data_dict


@torch.no_grad()
def postprocess(hard, closing=0, fill_holes=False, keep_largest=0, min_size=0, lo_channel=1):
    """The usual clean-up of a one-hot prediction (N, C, D, H, W), on the device.  For every foreground class from lo_channel on, in ascending order:
    binary closing with `closing` iterations of the 26-neighbourhood (border_value 0; 0: none), then hole filling with 6-connectivity; afterwards
    ops.keep_largest(k=keep_largest, min_size, 26-connectivity, to_background=True) when keep_largest > 0.  The tensor stays one-hot: a class gains
    only voxels that are background (channel 0) at that moment — so the lowest class wins a contested voxel — and a voxel a class loses (a closing
    can erode at the volume border) goes to channel 0.  With closing 0 and fill_holes False this is exactly the keep_largest call."""
    if isinstance(closing, bool) or int(closing) != closing or closing < 0:
        raise ValueError("postprocess: closing is a number of iterations >= 0, got %r" % (closing,))
    lo = int(lo_channel)
    x = hard
    if closing > 0 or fill_holes:
        x = hard.detach().float().clone()
        for c in range(lo, x.shape[1]):
            cur = (x[:, c:c + 1] >= 0.5).float()
            new = cur
            if closing > 0:
                new = V.binary_closing(new, iterations=int(closing), connectivity=26, border_value=0)
            if fill_holes:
                new = V.fill_holes(new, connectivity=6)
            if lo < 1:                                           # no background channel to trade with
                x[:, c:c + 1] = new
                continue
            gain = new * (1 - cur) * (x[:, 0:1] >= 0.5).float()
            lose = cur * (1 - new)
            x[:, c:c + 1] = cur + gain - lose
            x[:, 0:1] += lose - gain
    if keep_largest > 0:
        x = V.keep_largest(x, k=int(keep_largest), min_size=int(min_size), connectivity=26, lo_channel=lo, to_background=True)
    return x


# ----------------------------------------------------------------------------------------------------
# whole-volume inference: sliding-window prediction on the device (csrc/window.hip).  The reference has no counterpart
# (utils/utils.py:predict_vol is a 2D slice loop); tests/sliding_util.py restates the algorithm in numpy.
# ----------------------------------------------------------------------------------------------------
TTA_AXES = {"w": 1, "h": 2, "d": 4}


def tta_flips(axes):
    """The flip codes of a mirror test-time augmentation (bit 0 mirrors W, bit 1 H, bit 2 D).  axes: a string over "dhw" -> every subset of the named
    axes, as a tuple of codes in ascending order ("w" -> (0, 1), "d" -> (0, 4), "dhw" -> (0, 1, ..., 7)).  None, "" or () -> None: no augmentation.
    A sequence of codes passes through as a tuple, validated as ops.sw_flips does.  ValueError for anything else."""
    if axes is None or (isinstance(axes, (str, tuple, list)) and len(axes) == 0):
        return None
    if isinstance(axes, str):
        if any(a not in TTA_AXES for a in axes) or len(set(axes)) != len(axes):
            raise ValueError("tta: the axes are distinct letters of \"dhw\", got %r" % (axes,))
        mask = sum(TTA_AXES[a] for a in axes)
        return tuple(c for c in range(8) if c & ~mask == 0)
    V.sw_flips(axes)
    return tuple(int(c) for c in axes)


class SlidingWindow:
    """Sliding-window predictor for volumes of one shape: the plan, the importance map, the window counter and every buffer are made once, so the
    object can be called for one volume after another.  model_fn maps a (B, C, P, P, P) fp32 batch to planar probabilities (B, K, P, P, P).

    One batch is gather -> model_fn -> accumulate -> bump the window counter.  The counter is a DEVICE word (as the captured optimiser's
    hyperparameters are), so with graph=True that batch is captured once into a HIP graph and replayed ceil(nw / B) times per volume; eagerly the
    same launches are issued in a loop.  Either way the host never waits for the device between windows.  The sums are formed without atomics in
    ascending window order: the result does not depend on B, and graph replay equals eager launches bit for bit.

    tta (tta_flips: a string over "dhw" or a tuple of flip codes) turns on mirror test-time augmentation inside the kernels: the counter walks over
    (window, flip) items, nw * nf of them, gather writes each window mirrored and accumulate reads the answer mirrored back, so the normalised
    result is the blend of the un-flipped answers averaged over the nf flips — in one pass, one set of accumulators and one capture, with the same
    guarantees.  It costs nf forwards per window.  tta=None issues exactly the launches it always did."""

    def __init__(self, model_fn, shape, patch, overlap=0.5, blend="gaussian", batch=1, cval=0.0, graph=False, device="cuda", tta=None):
        shape = tuple(int(s) for s in shape)
        if len(shape) == 3:
            shape = (1,) + shape
        if len(shape) != 4 or int(batch) < 1:
            raise ValueError("SlidingWindow: shape is (C, D, H, W) or (D, H, W) and batch >= 1, got %r, %r" % (shape, batch))
        self.model_fn, self.shape, self.patch, self.batch, self.cval = model_fn, shape, int(patch), int(batch), float(cval)
        self.device = torch.device(device)
        self.origins, self.nw = V.sw_plan(shape[1:], self.patch, overlap, device=self.device)
        self.weights = V.sw_weights(self.patch, blend, device=self.device)
        self.tta = tta_flips(tta)
        self.n_items = self.nw * (len(self.tta) if self.tta else 1)
        self.n_batches = (self.n_items + self.batch - 1) // self.batch
        self.volume = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.first = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.windows = torch.empty((self.batch, shape[0]) + (self.patch,) * 3, dtype=torch.float32, device=self.device)
        self.acc = self.wsum = None
        self.use_graph, self.graph = bool(graph), None

    def _one_batch(self):
        V.sw_gather(self.volume, self.origins, self.first, self.batch, cval=self.cval, out=self.windows, flips=self.tta)
        prob = self.model_fn(self.windows)
        if prob.dim() != 5 or prob.shape[0] != self.batch or tuple(prob.shape[2:]) != (self.patch,) * 3:
            raise ValueError("sliding window: model_fn must return (B, K, P, P, P) = (%d, K, %d, %d, %d), got %s"
                             % ((self.batch,) + (self.patch,) * 3 + (tuple(prob.shape),)))
        if self.acc is None:                                     # K is known once the model has answered
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("sliding window: the accumulators must exist before a capture starts")
            self.acc = torch.zeros((prob.shape[1],) + self.shape[1:], dtype=torch.float32, device=self.device)
            self.wsum = torch.zeros(self.shape[1:], dtype=torch.float32, device=self.device)
        V.sw_accumulate(prob, self.acc, self.wsum, self.origins, self.first, self.weights, flips=self.tta)
        self.first.add_(self.batch)

    def _reset(self):
        self.first.zero_()
        if self.acc is not None:
            self.acc.zero_()
            self.wsum.zero_()

    def _capture(self):
        """one batch run eagerly on a side stream (the model's caches and K), its sums discarded, then the same batch captured"""
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            self._one_batch()
        torch.cuda.current_stream(self.device).wait_stream(side)
        self._reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._one_batch()
        self.graph = graph

    @torch.no_grad()
    def __call__(self, volume, onehot=False):
        ops._require_cuda(volume)
        vol = volume.detach()
        if vol.dim() == 3:
            vol = vol[None]
        if tuple(vol.shape) != self.shape:
            raise ValueError("sliding window: built for volumes of shape %s, got %s" % (self.shape, tuple(volume.shape)))
        with torch.cuda.device(self.device):
            self.volume.copy_(vol)
            if self.use_graph and self.graph is None:
                self._capture()
            self._reset()
            for _ in range(self.n_batches):
                if self.graph is not None:
                    self.graph.replay()
                else:
                    self._one_batch()
            prob, label, hot = V.sw_finalize(self.acc, self.wsum, label=True, onehot=onehot)
        out = {"prob": prob, "label": label, "wsum": self.wsum.clone(), "tta": self.tta}
        if onehot:
            out["onehot"] = hot
        return out


def sliding_window_predict(model_fn, volume, patch, overlap=0.5, blend="gaussian", batch=1, cval=0.0, graph=False, tta=None):
    """Whole-volume prediction of a fully convolutional 3D network: `volume` (C, D, H, W) or (D, H, W) on the device is tiled with overlapping cubic
    windows of side `patch` (ops.sw_plan), model_fn — (B, C, P, P, P) -> planar probabilities (B, K, P, P, P) — runs on `batch` windows at a time, the
    window probabilities are blended with the importance map `blend` ("gaussian" or "constant", ops.sw_weights) and normalised.  Runs under
    torch.no_grad().  -> {"prob": (K, D, H, W) fp32, "label": (D, H, W) uint8 (argmax, ties to the first channel), "wsum": (D, H, W) fp32}.
    graph=True captures one batch into a HIP graph and replays it (SlidingWindow, which also serves further volumes of the same shape).
    tta: mirror test-time augmentation (tta_flips): every window is predicted under each flip and the un-flipped answers are averaged, inside the same
    pass; wsum is then nf times larger, the dict's "tta" is the tuple of codes (None without), and the pass costs nf forwards per window."""
    ops._require_cuda(volume)
    return SlidingWindow(model_fn, tuple(volume.shape), patch, overlap=overlap, blend=blend, batch=batch, cval=cval, graph=graph, device=volume.device,
                         tta=tta)(volume)


def segmentation_model_fn(seg):
    """model_fn of sliding_window_predict for a modules.Segmentation (or a model that has one as .Seg), in whatever storage dtype it is set to"""
    net = seg.Seg if hasattr(seg, "Seg") else seg

    def model_fn(batch):
        return net({"image": batch}, "image", "prob")["prob"]
    return model_fn


@torch.no_grad()
def localise(prob_or_label, keep_largest=1, min_size=0, lo_channel=1):
    """A coarse whole-volume prediction -> the (D, H, W) fp32 mask of where the organ is, ready to be put into a data dict as <field>_pancreas_pred for
    data_gpu.CropResize.  prob_or_label: probabilities (K, D, H, W) — hardened by argmax — or a label map (D, H, W), whose labels >= lo_channel count as one
    foreground class.  Per foreground class (channels from lo_channel on) only the keep_largest largest 26-connected components of at least min_size voxels
    stay (ops.keep_largest; 0: no filter); the mask is the union of the classes."""
    ops._require_cuda(prob_or_label)
    x = prob_or_label.detach()
    if x.dim() == 4:
        hard = ops.hard_onehot(x[None])
    elif x.dim() == 3:
        k = max(int(lo_channel) + 1, 2)
        hard = torch.stack([(x == c).float() if c < k - 1 else (x >= c).float() for c in range(k)])[None]
    else:
        raise ValueError("localise: expected probabilities (K, D, H, W) or a label map (D, H, W), got shape %s" % (tuple(x.shape),))
    lo = min(int(lo_channel), hard.shape[1] - 1)
    if keep_largest > 0:
        hard = V.keep_largest(hard, k=int(keep_largest), min_size=int(min_size), connectivity=26, lo_channel=lo)
    return hard[0, lo:].amax(0).contiguous()


# the intensity window of the training pipeline (main_source.py:207-208: Clip(-200, 400), CenterIntensities(100, 300)) and what CropResize's zero padding
# becomes under it: the value a window reads past the scan
INTENSITY_CLIP = (-200.0, 400.0)
INTENSITY_CENTRE = (100.0, 300.0)
_FIELD = "image"


def _window_intensities(data_dict):
    from . import data_gpu
    return data_gpu.CenterIntensities([_FIELD], subtrahend=INTENSITY_CENTRE[0], divisor=INTENSITY_CENTRE[1])(
        data_gpu.Clip([_FIELD], new_min=INTENSITY_CLIP[0], new_max=INTENSITY_CLIP[1])(data_dict))


@torch.no_grad()
def coarse_to_fine_predict(seg, image, patch, overlap=0.5, blend="gaussian", batch=1, keep_largest=1, min_size=0, interp="linear", graph=False, tta=None,
                           want_prob=False, standardize=None):
    """Label-free segmentation of a raw scan `image` (D, H, W) on the device, returned in the scan's own geometry.  The composition of the public pieces:
      coarse   Clip / CenterIntensities -> sliding_window_predict with cubic windows of side `patch` -> localise (keep_largest, min_size) -> data_gpu.bounding_box
               (the chain's one host synchronisation)
      fine     data_gpu.crop_geometry and data_gpu.CropResize with the PREDICTION's box -> Clip / CenterIntensities -> the network on the patch^3 crop
      paste    ops.uncrop(interp): the fine probabilities resampled onto the scan grid, argmax; background outside the crop
    -> {"label": (D, H, W) uint8, "coarse_label": (D, H, W) uint8 (the sliding-window argmax), "geometry": (lo, hi, off, side) or None, "found": bool}.
    A coarse prediction without foreground — or with a single-voxel box, of which CropResize can make no crop — gives found False, geometry None and an
    all-background label.
    tta (tta_flips): mirror test-time augmentation of both passes.  The coarse pass receives it; the fine pass is a sliding-window pass over the crop
    itself — one window, constant blend — so its probabilities are the mean of the un-flipped answers, summed in the order of the codes.
    want_prob=True adds "prob": the pasted probabilities (K, D, H, W) fp32 of ops.uncrop(want_prob=True) — (1, 0, ..., 0) outside the crop and
    everywhere when nothing was found.
    standardize (a data_gpu.IntensityStandardizer): its transform of the scan takes the scan's place before anything else — for scans whose unit is not
    the one INTENSITY_CLIP is written in; None: nothing more is launched."""
    from . import data_gpu
    ops._require_cuda(image)
    if image.dim() != 3:
        raise ValueError("coarse_to_fine_predict: expected a (D, H, W) scan, got shape %s" % (tuple(image.shape),))
    img = image.detach().float().contiguous()
    if standardize is not None:
        img = standardize.transform(img)
    model_fn = segmentation_model_fn(seg)
    lo_v, hi_v = INTENSITY_CLIP
    cval = (min(max(0.0, lo_v), hi_v) - INTENSITY_CENTRE[0]) / INTENSITY_CENTRE[1]
    whole = _window_intensities({_FIELD: img.clone()})[_FIELD]
    tta = tta_flips(tta)
    coarse = sliding_window_predict(model_fn, whole, patch, overlap=overlap, blend=blend, batch=batch, cval=cval, graph=graph, tta=tta)
    mask = localise(coarse["prob"], keep_largest=keep_largest, min_size=min_size, lo_channel=min(1, coarse["prob"].shape[0] - 1))
    box = data_gpu.bounding_box(mask)
    geometry = data_gpu.crop_geometry(box, img.shape) if box is not None else None
    if geometry is None or geometry[3] < 1:
        res = {"label": torch.zeros(tuple(img.shape), dtype=torch.uint8, device=img.device), "coarse_label": coarse["label"], "geometry": None, "found": False}
        if want_prob:
            res["prob"] = torch.zeros((coarse["prob"].shape[0],) + tuple(img.shape), dtype=torch.float32, device=img.device)
            res["prob"][0] = 1.0
        return res
    crop = data_gpu.CropResize([_FIELD], (int(patch),) * 3)({_FIELD: img, _FIELD + "_pancreas": mask, _FIELD + "_pancreas_pred": mask})
    crop = _window_intensities(crop)
    if tta is None:
        fine = model_fn(crop[_FIELD][None, None])[0]
    else:
        fine = sliding_window_predict(model_fn, crop[_FIELD], patch, overlap=0.0, blend="constant", batch=batch, tta=tta)["prob"]
    pasted = V.uncrop(fine, geometry, tuple(img.shape), interp=interp, want_prob=want_prob)
    res = {"label": pasted["label"], "coarse_label": coarse["label"], "geometry": geometry, "found": True}
    if want_prob:
        res["prob"] = pasted["prob"]
    return res


@torch.no_grad()
def predict_scan(seg, raw, affine_diag, patch, overlap=0.5, blend="gaussian", batch=1, keep_largest=1, min_size=0, interp="linear", graph=False, tta=None,
                 native_interp="linear", details=False, standardize=None):
    """A scan as the scanner wrote it in, a label on that scan's own voxel grid out, without leaving the device.  raw (X, Y, Z): CUDA int16 / uint8 /
    int8 / float32; affine_diag: the signed diagonal of its affine.  By definition the two-step composition of the public pieces:
      data_gpu.preprocess_scan               orient + resize to the 1 mm grid (data_process.py:23-34)
      standardize.transform                  only with standardize (a data_gpu.IntensityStandardizer): the 1 mm image onto the standard scale
      coarse_to_fine_predict(want_prob=True) with the options of that function: probabilities pasted onto the 1 mm grid by ops.uncrop(interp)
      ops.to_native(native_interp)           those probabilities resampled onto the raw grid, argmax
    The two resamplings (crop -> 1 mm, 1 mm -> raw) are NOT fused into one map: that would change the values.
    -> the label (X, Y, Z) uint8; with details=True a dict {"label", "label_1mm", "coarse_label", "geometry" (ScanGeometry), "crop_geometry", "found"}."""
    from . import data_gpu
    pre = data_gpu.preprocess_scan(raw, affine_diag)
    res = coarse_to_fine_predict(seg, pre["image"], patch, overlap=overlap, blend=blend, batch=batch, keep_largest=keep_largest, min_size=min_size,
                                 interp=interp, graph=graph, tta=tta, want_prob=True, standardize=standardize)
    label = V.to_native(res["prob"], pre["geometry"], interp=native_interp)["label"]
    if not details:
        return label
    return {"label": label, "label_1mm": res["label"], "coarse_label": res["coarse_label"], "geometry": pre["geometry"], "crop_geometry": res["geometry"],
            "found": res["found"]}
