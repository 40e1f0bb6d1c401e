"""Forward-only utilities on planar volumes: thin ctypes wrappers around the libvaeseg C ABI (include/vaeseg.h), one section per csrc/*.hip file.

What validation, whole-volume inference and the data pipeline (evaluation.py, driver.py, data_gpu.py) call outside the training step.  Nothing here is
differentiable and nothing synchronises; nothing has a CPU path.  ops re-exports the public names (__all__), so ``ops.<name>`` reaches them too.
"""
import ctypes as _ctypes
import math
import numbers as _numbers

import numpy as np
import torch

from . import _lib
from ._lib import _contig, _p, _require_cuda, _stream, check, lib

__all__ = ["cc_max_components", "cc_label", "keep_largest",
           "SURFACE_RECORD_FIELDS", "surface", "edt", "surface_distances",
           "MORPH_OPS", "morph", "binary_dilation", "binary_erosion", "binary_opening", "binary_closing", "fill_holes",
           "REGION_COLUMNS", "CONTINGENCY_MAX_CELLS", "region_props", "contingency",
           "HISTOGRAM_MAX_BINS", "HISTOGRAM_MAX_CELLS", "MI_MAX_RADIUS", "MI_MAX_PLANES", "histogram", "joint_histogram", "mutual_information",
           "SW_BLENDS", "SW_GAUSSIAN_FLOOR", "sw_plan_host", "sw_plan", "sw_weights", "sw_flips", "sw_gather", "sw_accumulate", "sw_finalize",
           "UNCROP_INTERPS", "uncrop",
           "SCAN_DTYPES", "scan_orient", "to_native",
           "AUG_MAX_SIGMA", "AUG_OPS", "aug_stats", "philox_normal", "gaussian_weights", "blur_tile", "gaussian_blur3d", "aug_flip", "aug_stage",
           "ZOOM_EDGE_ORDERS", "ZOOM_EDGE_MAX_LEN", "zoom_edge_bundle", "zoom_edge", "simulate_lowres",
           "QUANTILE_MAX_Q", "QUANTILE_WG_VOXELS", "INTENSITY_MAP_MAX_L", "INTENSITY_MAP_WG_VOXELS", "INTENSITY_MAP_EXTRAPOLATE", "quantile", "intensity_map"]


# what the sections share
def _aligned16(t):
    """t contiguous at a 16-byte aligned address (the kernels read quads): t itself where it already is, a copy otherwise"""
    t = _contig(t)
    return t.clone() if t.data_ptr() % 16 else t


def _mask_prepare(mask, what):
    _require_cuda(mask)
    if mask.requires_grad:
        raise RuntimeError("%s is forward only: detach the input" % what)
    if mask.dim() != 5:
        raise ValueError("expected a planar (N, C, D, H, W) tensor, got shape %s" % (tuple(mask.shape),))
    return _aligned16(mask.float())


def _workspace(cache, key, query, what, device):
    """The cached workspace of a call, allocated at its first use.  The caches (_CC_, _EDT_, _MORPH_, _FILL_, _MI_WORKSPACES) are keyed by shape, variant
    and device, and an entry is never freed or moved — as the packed weights are — so a captured graph that holds its pointer stays valid.  Calls that
    share a workspace must be ordered on one stream."""
    ws = cache.get(key)
    if ws is None:
        nbytes = query()
        check(min(nbytes, 0), what)
        ws = cache[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return ws


# connected components (csrc/cc.hip)
_CC_WORKSPACES = {}


def cc_max_components(d, h, w, connectivity=26):
    """rows per plane of the size table (include/vaeseg.h): the most components a (d, h, w) plane can hold"""
    if connectivity == 26:
        return ((d + 1) // 2) * ((h + 1) // 2) * ((w + 1) // 2)
    return (d * h * w + 1) // 2


def _cc_prepare(mask, connectivity):
    m = _mask_prepare(mask, "connected-component labelling")
    n, c, d, h, w = m.shape
    ws = _workspace(_CC_WORKSPACES, (n, c, d, h, w, int(connectivity), m.device), lambda: lib.vs_cc_workspace_bytes(n, c, d, h, w, int(connectivity)),
                    "cc_workspace_bytes", m.device)
    return m, ws


def cc_label(mask, connectivity=26):
    """Connected components of every (n, c) plane of a planar (N, C, D, H, W) mask (foreground: value >= 0.5) — utils/utils.py:20-57.
    -> labels int32 (N, C, D, H, W): 0 background, 1..K in the order of each component's first voxel in raster order (scipy.ndimage.label's
    numbering); counts int32 (N, C) = K; sizes int32 (N, C, cc_max_components(D, H, W, connectivity)): sizes[..., label - 1] voxels, 0 beyond K."""
    m, ws = _cc_prepare(mask, connectivity)
    n, c, d, h, w = m.shape
    labels = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    counts = torch.empty((n, c), dtype=torch.int32, device=m.device)
    check(lib.vs_cc_label(m.data_ptr(), labels.data_ptr(), counts.data_ptr(), n, c, d, h, w, int(connectivity), ws.data_ptr(), _stream()), "cc_label")
    maxk = cc_max_components(d, h, w, connectivity)
    sizes = ws[:n * c * maxk * 4].view(torch.int32).view(n, c, maxk).clone()       # the table sits at the start of the workspace
    return labels, counts, sizes


def keep_largest(mask, k=1, min_size=0, connectivity=26, lo_channel=0, to_background=False):
    """utils/utils.py:776-796 (predict_vol step 2) per (n, c) plane: 1.0 on the k largest components that hold at least min_size voxels (equal
    sizes: the one whose first voxel comes first), 0.0 elsewhere.  Channels below lo_channel are copied; with to_background (and lo_channel >= 1)
    channel 0 gains every removed voxel, so a one-hot tensor stays one-hot."""
    m, ws = _cc_prepare(mask, connectivity)
    n, c, d, h, w = m.shape
    out = torch.empty_like(m)
    check(lib.vs_cc_keep_largest(m.data_ptr(), out.data_ptr(), n, c, d, h, w, int(connectivity), int(k), int(min(max(min_size, 0), 2 ** 31 - 1)),
                                 int(lo_channel), int(bool(to_background)), ws.data_ptr(), _stream()), "cc_keep_largest")
    return out


# surface distances (csrc/surface.hip)
_EDT_WORKSPACES = {}
SURFACE_RECORD_FIELDS = ("count_ab", "count_ba", "sum_ab", "sum_ba", "max_sq", "lo_sq", "hi_sq", "assd", "hd", "hd95")      # vs_surface_record


def _spacing_array(spacing):
    """None, or the (sz, sy, sx) doubles the library reads on the host during the call"""
    if spacing is None:
        return None
    vals = [float(s) for s in spacing]
    if len(vals) != 3:
        raise ValueError("spacing is (sz, sy, sx), got %r" % (spacing,))
    return (_ctypes.c_double * 3)(*vals)


def surface(mask, connectivity=6):
    """S(X) = X & ~binary_erosion(X) per (n, c) plane of a planar (N, C, D, H, W) mask (foreground: value >= 0.5): fp32, 1.0 on foreground voxels that have a
    background or out-of-volume neighbour among their 6 (default, medpy's) or 26 neighbours."""
    m = _mask_prepare(mask, "surface extraction")
    n, c, d, h, w = m.shape
    out = torch.empty_like(m)
    check(lib.vs_surface(m.data_ptr(), out.data_ptr(), n, c, d, h, w, int(connectivity), _stream()), "surface")
    return out


def edt(feature, spacing=None, squared=False):
    """Exact Euclidean distance of every voxel to the nearest voxel with feature >= 0.5, per (n, c) plane of a planar (N, C, D, H, W) tensor.
    spacing None and squared: int32 squared distances (2^31 - 1 in a plane without feature voxels).  Otherwise fp64 — squared or not — with
    spacing = (sz, sy, sx) or unit spacing; +inf in a plane without feature voxels."""
    m = _mask_prepare(feature, "the distance transform")
    n, c, d, h, w = m.shape
    sp = _spacing_array(spacing)
    out = torch.empty(m.shape, dtype=torch.int32 if sp is None else torch.float64, device=m.device)
    check(lib.vs_edt(m.data_ptr(), out.data_ptr(), n, c, d, h, w, sp, _stream()), "edt")
    if sp is None:
        if squared:
            return out
        sq = out.double()
        return torch.where(out == 2 ** 31 - 1, torch.full_like(sq, float("inf")), sq).sqrt_()
    return out if squared else out.sqrt_()


def surface_distances(pred, gt, spacing=None, connectivity=6):
    """The surface-distance record of every (n, c) plane (include/vaeseg.h vs_surface_record; A = pred, B = gt): a dict of (N, C) device tensors —
    count_ab, count_ba (int64), sum_ab, sum_ba, max_sq, lo_sq, hi_sq, assd, hd, hd95 (fp64).  A plane with an empty surface has counts 0 and NaN elsewhere."""
    a, b = _mask_prepare(pred, "surface distances"), _mask_prepare(gt, "surface distances")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("surface_distances: the two masks differ in shape or device: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    n, c, d, h, w = a.shape
    sp = _spacing_array(spacing)
    ws = _workspace(_EDT_WORKSPACES, (n, c, d, h, w, sp is not None, a.device), lambda: lib.vs_edt_workspace_bytes(n, c, d, h, w, int(sp is not None)),
                    "edt_workspace_bytes", a.device)
    rec = torch.empty((n, c, len(SURFACE_RECORD_FIELDS)), dtype=torch.float64, device=a.device)
    check(lib.vs_surface_distances(a.data_ptr(), b.data_ptr(), rec.data_ptr(), n, c, d, h, w, int(connectivity), sp, ws.data_ptr(), _stream()),
          "surface_distances")
    out = {name: rec[..., i] for i, name in enumerate(SURFACE_RECORD_FIELDS)}
    counts = rec[..., :2].view(torch.int64)                     # the record's first two members are 64-bit integers
    out["count_ab"], out["count_ba"] = counts[..., 0], counts[..., 1]
    return out


# signed distance maps of a label volume (csrc/sdm.hip).  The training loss is its first caller (ops.boundary_loss): ops imports signed_distance by name
_SDM_WORKSPACES = {}


def signed_distance(label, n_class, botindex=0, topindex=None, spacing=None):
    """The signed distance maps phi_c, c in [botindex, topindex) (topindex None: n_class), of a (N, 1, D, H, W) label volume -> fp32
    (N, topindex - botindex, D, H, W), by the rule of DESIGN 3.22: a voxel's class is (int)label where 0 <= label < n_class and none otherwise; outside
    the class phi_c = +distance to its nearest voxel, inside 1 - distance to the nearest voxel outside it (Kervadec's one_hot2dist), exact Euclidean
    distances under spacing = (sz, sy, sx) or unit spacing; a plane whose class is absent or fills the whole volume is 0.  Three launches, no
    synchronisation, capturable; the workspace is cached per shape like _EDT_WORKSPACES."""
    _require_cuda(label)
    if label.requires_grad:
        raise RuntimeError("the signed distance map is forward only: detach the input")
    if label.dim() != 5 or label.shape[1] != 1:
        raise ValueError("expected a (N, 1, D, H, W) label volume, got shape %s" % (tuple(label.shape),))
    n_class = int(n_class)
    bot, top = int(botindex), n_class if topindex is None else int(topindex)
    if n_class < 1 or not 0 <= bot < top <= n_class:
        raise ValueError("signed_distance: channels [%d, %d) of %d classes" % (bot, top, n_class))
    lab = _aligned16(label.float())
    n, _, d, h, w = lab.shape
    k = top - bot
    sp = _spacing_array(spacing)
    ws = _workspace(_SDM_WORKSPACES, (n, k, d, h, w, sp is not None, lab.device),
                    lambda: lib.vs_signed_distance_workspace_bytes(n, k, d, h, w, int(sp is not None)), "signed_distance_workspace_bytes", lab.device)
    phi = torch.empty((n, k, d, h, w), dtype=torch.float32, device=lab.device)
    check(lib.vs_signed_distance(lab.data_ptr(), phi.data_ptr(), n, n_class, bot, top, d, h, w, sp, ws.data_ptr(), _stream()), "signed_distance")
    return phi


# binary morphology and hole filling (csrc/morph.hip)
MORPH_OPS = {"dilate": 0, "erode": 1, "open": 2, "close": 3}          # VS_MORPH_*
_MORPH_WORKSPACES = {}
_FILL_WORKSPACES = {}


def _check_connectivity(connectivity, what):
    if isinstance(connectivity, bool) or connectivity not in (6, 26):
        raise ValueError("%s: connectivity is 6 (generate_binary_structure(3, 1)) or 26 ((3, 3)), got %r" % (what, connectivity))
    return int(connectivity)


def morph(mask, op, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_dilation / binary_erosion / binary_opening / binary_closing (op "dilate" / "erode" / "open" / "close") per (n, c) plane of a
    planar (N, C, D, H, W) mask (foreground: value >= 0.5) -> fp32 0 / 1.  connectivity 6 is generate_binary_structure(3, 1), 26 is (3, 3); the
    structure is applied `iterations` >= 1 times (opening: erode^n then dilate^n, closing: dilate^n then erode^n); voxels outside the volume read as
    border_value (0 or 1) in both halves, as scipy passes it on.  Bit-packed on the device (csrc/morph.hip), no synchronisation."""
    if op not in MORPH_OPS:
        raise ValueError("morph: op is one of %s, got %r" % (sorted(MORPH_OPS), op))
    connectivity = _check_connectivity(connectivity, "morph")
    try:
        ok = not isinstance(iterations, bool) and int(iterations) == iterations and iterations >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("morph: iterations is an integer >= 1, got %r" % (iterations,))
    if isinstance(border_value, bool):
        border_value = int(border_value)
    if border_value not in (0, 1):
        raise ValueError("morph: border_value is 0 or 1, got %r" % (border_value,))
    m = _mask_prepare(mask, "binary morphology")
    n, c, d, h, w = m.shape
    ws = _workspace(_MORPH_WORKSPACES, (n, c, d, h, w, connectivity, m.device), lambda: lib.vs_morph_workspace_bytes(n, c, d, h, w),
                    "morph_workspace_bytes", m.device)
    out = torch.empty_like(m)
    check(lib.vs_morph(m.data_ptr(), out.data_ptr(), n, c, d, h, w, MORPH_OPS[op], connectivity, int(min(iterations, 2 ** 31 - 1)), int(border_value),
                       ws.data_ptr(), _stream()), "morph")
    return out


def binary_dilation(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_dilation(input, generate_binary_structure(3, 1 or 3), iterations, border_value=border_value) per plane (morph)"""
    return morph(input, "dilate", iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_erosion(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_erosion per plane (morph)"""
    return morph(input, "erode", iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_opening(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_opening per plane (morph)"""
    return morph(input, "open", iterations=iterations, connectivity=connectivity, border_value=border_value)


def binary_closing(input, iterations=1, connectivity=6, border_value=0):
    """scipy.ndimage.binary_closing per plane (morph)"""
    return morph(input, "close", iterations=iterations, connectivity=connectivity, border_value=border_value)


def fill_holes(mask, connectivity=6):
    """scipy.ndimage.binary_fill_holes(X, structure) per (n, c) plane of a planar (N, C, D, H, W) mask (foreground: value >= 0.5) -> fp32 0 / 1: the
    complement of the background voxels that reach the outside of the volume through `connectivity`-neighbours (6, scipy's default, or 26).
    The complement is labelled with the connected-component union-find on the device (csrc/morph.hip), no synchronisation."""
    connectivity = _check_connectivity(connectivity, "fill_holes")
    m = _mask_prepare(mask, "hole filling")
    n, c, d, h, w = m.shape
    ws = _workspace(_FILL_WORKSPACES, (n, c, d, h, w, connectivity, m.device), lambda: lib.vs_fill_holes_workspace_bytes(n, c, d, h, w, connectivity),
                    "fill_holes_workspace_bytes", m.device)
    out = torch.empty_like(m)
    check(lib.vs_fill_holes(m.data_ptr(), out.data_ptr(), n, c, d, h, w, connectivity, ws.data_ptr(), _stream()), "fill_holes")
    return out


# per-component measurements and contingency tables of label volumes (csrc/regions.hip).  No workspace: the outputs are the only buffers, and the
# kernels write their initial state themselves.
REGION_COLUMNS = ("count", "zmin", "ymin", "xmin", "zmax", "ymax", "xmax", "sum_z", "sum_y", "sum_x")      # vs_region_props
CONTINGENCY_MAX_CELLS = 1 << 22                                                                            # (rows_a + 1) * (rows_b + 1) per plane


def _rows(value, what, least):
    if isinstance(value, bool) or not isinstance(value, _numbers.Integral) or value < least or value > 2 ** 31 - 2:
        raise ValueError("%s is an integer >= %d, got %r" % (what, least, value))
    return int(value)


def _planar_volume(t, what, dtype, kind, noun):
    """every check that needs no device; the tensor is used as it is — a volume is never converted or copied behind the caller's back"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError("%s: %s, got %s" % (what, kind, getattr(t, "dtype", type(t))))
    if t.dim() != 5:
        raise ValueError("%s: expected a planar (N, C, D, H, W) %s, got shape %s" % (what, noun, tuple(t.shape)))
    if t.numel() == 0 or t.shape[2] * t.shape[3] * t.shape[4] >= 2 ** 31:
        raise ValueError("%s: an empty volume or a plane of 2^31 voxels or more, shape %s" % (what, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s: the %s must be contiguous" % (what, noun))


def _label_volume(t, what):
    _planar_volume(t, what, torch.int32, "label volumes are int32 tensors (ops.cc_label's labels)", "label volume")


def region_props(labels, max_components=4096):
    """Per-label measurements of every (n, c) plane of an int32 label volume (N, C, D, H, W) — 0 background, 1..K components, as ops.cc_label
    numbers them — for the labels 1..R, R = max_components; what scipy.ndimage.find_objects, np.bincount and center_of_mass give on the host.
    -> {"count": int64 (N, C, R) voxels; "bbox": int32 (N, C, R, 6) = (zmin, ymin, xmin, zmax, ymax, xmax), inclusive;
        "centroid": fp64 (N, C, R, 3) = (z, y, x) in voxels, sum / count; "sums": int64 (N, C, R, 3) the coordinate sums behind it;
        "overflow": int32 (N, C) voxels whose label is negative or above R — counted there and nowhere else}.
    A label that does not occur has count 0, box mins (D, H, W) and maxes -1, centroid NaN.  Two launches, no synchronisation."""
    r = _rows(max_components, "region_props: max_components", 1)
    _label_volume(labels, "region_props")
    _require_cuda(labels)
    n, c, d, h, w = labels.shape
    table = torch.empty((n, c, r, len(REGION_COLUMNS)), dtype=torch.int64, device=labels.device)
    overflow = torch.empty((n, c), dtype=torch.int32, device=labels.device)
    check(lib.vs_region_props(labels.data_ptr(), n, c, d, h, w, r, table.data_ptr(), overflow.data_ptr(), _stream()), "region_props")
    count, sums = table[..., 0], table[..., 7:10]
    return {"count": count, "bbox": table[..., 1:7].to(torch.int32), "centroid": sums.double() / count.double().unsqueeze(-1), "sums": sums,
            "overflow": overflow}


def contingency(a, b, rows_a, rows_b):
    """The contingency table of two int32 label volumes of one shape (N, C, D, H, W), per (n, c) plane:
    -> table int64 (N, C, rows_a + 1, rows_b + 1), table[..., i, j] = voxels with a == i and b == j (row / column 0: background), and
    overflow int32 (N, C): voxels with a label outside [0, rows_a] / [0, rows_b] on either side — counted there and in no cell.
    (rows_a + 1) * (rows_b + 1) <= 2^22.  Two launches, no synchronisation; np.bincount(a * (rows_b + 1) + b) without the host."""
    ra, rb = _rows(rows_a, "contingency: rows_a", 0), _rows(rows_b, "contingency: rows_b", 0)
    if (ra + 1) * (rb + 1) > CONTINGENCY_MAX_CELLS:
        raise ValueError("contingency: (rows_a + 1) * (rows_b + 1) = %d cells per plane, at most 2^22" % ((ra + 1) * (rb + 1)))
    _label_volume(a, "contingency")
    _label_volume(b, "contingency")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("contingency: the two label volumes differ in shape or device: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    _require_cuda(a, b)
    n, c, d, h, w = a.shape
    table = torch.empty((n, c, ra + 1, rb + 1), dtype=torch.int64, device=a.device)
    overflow = torch.empty((n, c), dtype=torch.int32, device=a.device)
    check(lib.vs_contingency(a.data_ptr(), b.data_ptr(), n, c, d, h, w, ra, rb, table.data_ptr(), overflow.data_ptr(), _stream()), "contingency")
    return table, overflow


# intensity histograms, joint histograms and mutual information (csrc/hist.hip).  The outputs are the only buffers of the histogram calls; the kernels
# write their initial state themselves.
HISTOGRAM_MAX_BINS = 4096                      # vs_histogram
HISTOGRAM_MAX_CELLS = 1 << 22                  # (rows + 1) * bins, bins_x * bins_y per plane
MI_MAX_RADIUS = 64                             # int(4 * sigma + 0.5) of vs_mutual_information
MI_MAX_PLANES = 65535
_MI_WORKSPACES = {}


def _bins(value, what):
    if isinstance(value, bool) or not isinstance(value, _numbers.Integral) or value < 1:
        raise ValueError("%s is an integer >= 1, got %r" % (what, value))
    return int(value)


def _intensity_volume(t, what):
    _planar_volume(t, what, torch.float32, "intensity volumes are float32 tensors", "volume")


def _bounds(pair, what):
    """(lo, hi) as two Python floats with lo <= hi, both finite"""
    try:
        lo, hi = (float(v) for v in pair)
    except (TypeError, ValueError):
        raise ValueError("%s is a pair (lo, hi) of numbers, got %r" % (what, pair)) from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("%s needs finite bounds with lo <= hi, got %r" % (what, (lo, hi)))
    return lo, hi


def histogram(x, bins, range=None, labels=None, rows=0):
    """np.histogram of every (n, c) plane of a planar fp32 volume (N, C, D, H, W) on the device, optionally one histogram per label.
    Edges: the fp64 values np.linspace(lo, hi, bins + 1) (product and sum rounded separately; lo == hi becomes lo - 0.5, hi + 0.5).  range=(lo, hi): the
    same host bounds for all planes; range=None: per plane the minimum and maximum over its finite voxels, found on the device ((0, 0) without any).
    A voxel x, promoted to fp64, is in bin i iff e_i <= x < e_{i+1}; x == e_bins is in the last bin.
    labels: an int32 volume of x's shape (ops.cc_label's labels, an argmax); row r of the table counts the voxels labelled r, 0 <= r <= rows.
    -> {"table": int64 (N, C, rows + 1, bins); "edges": fp64 (N, C, bins + 1); "outside": int64 (N, C), NaN, +-inf and out-of-range voxels, in no bin;
        "overflow": int32 (N, C), voxels whose label is negative or above rows — counted there and nowhere else}.
    bins <= 4096 and (rows + 1) * bins <= 2^22.  Three or four launches, no synchronisation (vs_histogram)."""
    b = _bins(bins, "histogram: bins")
    r = _rows(rows, "histogram: rows", 0)
    if b > HISTOGRAM_MAX_BINS or (r + 1) * b > HISTOGRAM_MAX_CELLS:
        raise ValueError("histogram: bins = %d, (rows + 1) * bins = %d; at most 4096 bins and 2^22 cells per plane" % (b, (r + 1) * b))
    lo, hi = (0.0, 0.0) if range is None else _bounds(range, "histogram: range")
    _intensity_volume(x, "histogram")
    if labels is None:
        if r != 0:
            raise ValueError("histogram: rows = %d without labels" % r)
    else:
        _label_volume(labels, "histogram")
        if labels.shape != x.shape or labels.device != x.device:
            raise ValueError("histogram: labels and x differ in shape or device: %s vs %s" % (tuple(labels.shape), tuple(x.shape)))
    _require_cuda(x, labels)
    n, c, d, h, w = x.shape
    table = torch.empty((n, c, r + 1, b), dtype=torch.int64, device=x.device)
    edges = torch.empty((n, c, b + 1), dtype=torch.float64, device=x.device)
    outside = torch.empty((n, c), dtype=torch.int64, device=x.device)
    overflow = torch.empty((n, c), dtype=torch.int32, device=x.device)
    check(lib.vs_histogram(x.data_ptr(), _p(labels), n, c, d, h, w, b, r, lo, hi, int(range is None), edges.data_ptr(), table.data_ptr(),
                           outside.data_ptr(), overflow.data_ptr(), _stream()), "histogram")
    return {"table": table, "edges": edges, "outside": outside, "overflow": overflow}


def joint_histogram(x, y, bins=(256, 256), range=None):
    """np.histogram2d of every (n, c) plane of two planar fp32 volumes of one shape (N, C, D, H, W) on the device, with histogram's binning rule per
    variable.  bins: an integer or (bins_x, bins_y); range: None (bounds from the data, per plane and variable) or ((lo_x, hi_x), (lo_y, hi_y)).
    -> {"table": int64 (N, C, bins_x, bins_y), table[..., i, j] = voxels with x in bin i and y in bin j; "edges_x": fp64 (N, C, bins_x + 1); "edges_y";
        "outside": int64 (N, C), voxels with either value NaN, +-inf or out of range — in no cell}.
    bins_x * bins_y <= 2^22.  Three or four launches, no synchronisation (vs_joint_histogram)."""
    if isinstance(bins, _numbers.Integral) and not isinstance(bins, bool):
        bins = (bins, bins)
    try:
        bx, by = bins
    except (TypeError, ValueError):
        raise ValueError("joint_histogram: bins is an integer or a pair, got %r" % (bins,)) from None
    bx, by = _bins(bx, "joint_histogram: bins_x"), _bins(by, "joint_histogram: bins_y")
    if bx * by > HISTOGRAM_MAX_CELLS:
        raise ValueError("joint_histogram: bins_x * bins_y = %d cells per plane, at most 2^22" % (bx * by))
    r4 = None
    if range is not None:
        try:
            rx, ry = range
        except (TypeError, ValueError):
            raise ValueError("joint_histogram: range is None or ((lo_x, hi_x), (lo_y, hi_y)), got %r" % (range,)) from None
        r4 = (_ctypes.c_double * 4)(*(_bounds(rx, "joint_histogram: range of x") + _bounds(ry, "joint_histogram: range of y")))
    _intensity_volume(x, "joint_histogram")
    _intensity_volume(y, "joint_histogram")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError("joint_histogram: the two volumes differ in shape or device: %s vs %s" % (tuple(x.shape), tuple(y.shape)))
    _require_cuda(x, y)
    n, c, d, h, w = x.shape
    table = torch.empty((n, c, bx, by), dtype=torch.int64, device=x.device)
    edges_x = torch.empty((n, c, bx + 1), dtype=torch.float64, device=x.device)
    edges_y = torch.empty((n, c, by + 1), dtype=torch.float64, device=x.device)
    outside = torch.empty((n, c), dtype=torch.int64, device=x.device)
    check(lib.vs_joint_histogram(x.data_ptr(), y.data_ptr(), n, c, d, h, w, bx, by, None if r4 is None else _ctypes.addressof(r4), int(r4 is None),
                                 edges_x.data_ptr(), edges_y.data_ptr(), table.data_ptr(), outside.data_ptr(), _stream()), "joint_histogram")
    return {"table": table, "edges_x": edges_x, "edges_y": edges_y, "outside": outside}


def mutual_information(table, sigma=1.0, normalized=True):
    """The tail of the reference's mutual_information_3d (utils/utils.py:824-845) on an int64 joint histogram (N, C, bins_x, bins_y), in fp64 on the
    device: scipy.ndimage.gaussian_filter(jh, sigma, mode="constant") (sigma == 0: none), + eps, division by the total, the marginals s1 and s2, then
    (sum s1 log s1 + sum s2 log s2) / sum jh log jh - 1 when normalized, otherwise sum jh log jh - sum s1 log s1 - sum s2 log s2.
    -> fp64 (N, C).  Every sum runs in a fixed order: the same bits on every run.  No synchronisation (vs_mutual_information).
    sigma is a number >= 0 with int(4 * sigma + 0.5) <= 64; N * C <= 65535."""
    if isinstance(sigma, bool) or not isinstance(sigma, _numbers.Real) or not (sigma >= 0) or math.isinf(sigma) or int(4.0 * sigma + 0.5) > MI_MAX_RADIUS:
        raise ValueError("mutual_information: sigma is a number >= 0 with a kernel radius int(4 sigma + 0.5) <= %d, got %r" % (MI_MAX_RADIUS, sigma))
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int64:
        raise TypeError("mutual_information: the table is an int64 tensor (ops.joint_histogram's), got %s" % getattr(table, "dtype", type(table)))
    if table.dim() != 4 or table.numel() == 0:
        raise ValueError("mutual_information: expected a table (N, C, bins_x, bins_y), got shape %s" % (tuple(table.shape),))
    n, c, bx, by = table.shape
    if bx * by > HISTOGRAM_MAX_CELLS or n * c > MI_MAX_PLANES:
        raise ValueError("mutual_information: at most 2^22 cells per plane and %d planes, got shape %s" % (MI_MAX_PLANES, tuple(table.shape)))
    if not table.is_contiguous():
        raise ValueError("mutual_information: the table must be contiguous")
    _require_cuda(table)
    ws = _workspace(_MI_WORKSPACES, (n, c, bx, by, table.device), lambda: 8 * n * c * (2 * bx * by + 2 * bx + by), "mutual_information workspace",
                    table.device)
    mi = torch.empty((n, c), dtype=torch.float64, device=table.device)
    check(lib.vs_mutual_information(table.data_ptr(), n, c, bx, by, float(sigma), int(bool(normalized)), ws.data_ptr(), mi.data_ptr(), _stream()),
          "mutual_information")
    return mi


# sliding-window prediction (csrc/window.hip).  evaluation.sliding_window_predict drives these; nothing here synchronises.
SW_BLENDS = ("constant", "gaussian")
SW_GAUSSIAN_FLOOR = 1e-3


def sw_plan_host(shape, patch, overlap):
    """vs_sw_plan on the host: the window origins of a (D, H, W) volume tiled with cubic `patch` windows -> numpy int32 (nw, 3), D-major, then H, then W.
    Per axis step = max(1, floor(patch (1 - overlap))), n = 1 if S <= patch else ceil((S - patch) / step) + 1, origin i = min(i step, max(S - patch, 0))."""
    d, h, w = (int(s) for s in shape)
    nw = lib.vs_sw_plan(d, h, w, int(patch), float(overlap), None, 0)
    check(min(nw, 0), "sw_plan")
    table = np.empty((nw, 3), dtype=np.int32)
    check(min(lib.vs_sw_plan(d, h, w, int(patch), float(overlap), table.ctypes.data, nw), 0), "sw_plan")
    return table


def sw_plan(shape, patch, overlap, device="cuda"):
    """-> (origins: int32 (nw, 3) tensor on `device`, nw) — sw_plan_host's table where the kernels read it"""
    table = sw_plan_host(shape, patch, overlap)
    return torch.from_numpy(table).to(device), int(table.shape[0])


def sw_weights(patch, blend="gaussian", device="cuda"):
    """The separable importance map of a window as an fp32 (3, patch) tensor (rows: z, y, x; a voxel's weight is their fp32 product).
    "constant": ones.  "gaussian": exp(-((i - (patch - 1) / 2) / sigma)^2 / 2) with sigma = patch / 8 per axis, computed in float64, floored at
    1e-3 and rounded to fp32."""
    p = int(patch)
    if p <= 0:
        raise ValueError("sw_weights: patch must be positive, got %r" % (patch,))
    if blend == "constant":
        row = np.ones(p, dtype=np.float64)
    elif blend == "gaussian":
        i = np.arange(p, dtype=np.float64)
        row = np.maximum(np.exp(-0.5 * ((i - (p - 1) / 2.0) / (p / 8.0)) ** 2), SW_GAUSSIAN_FLOOR)
    else:
        raise ValueError("sw_weights: blend is one of %s, got %r" % (SW_BLENDS, blend))
    return torch.from_numpy(np.stack([row, row, row]).astype(np.float32)).to(device)


def _sw_common(origins, first, weights, patch):
    if origins.dtype != torch.int32 or origins.dim() != 2 or origins.shape[1] != 3 or not origins.is_contiguous():
        raise ValueError("sw: origins is the contiguous int32 (nw, 3) table of sw_plan")
    if first.dtype != torch.int32 or first.numel() != 1:
        raise ValueError("sw: first is one int32 device word")
    if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (3, patch) or not weights.is_contiguous()):
        raise ValueError("sw: weights is the contiguous fp32 (3, %d) tensor of sw_weights" % patch)


def sw_flips(flips):
    """The flip codes of a mirror-TTA pass (bit 0 mirrors W, bit 1 H, bit 2 D) -> (nf, the codes packed three bits each, code i in bits [3 i, 3 i + 3)):
    how vs_sw_gather_tta and vs_sw_accumulate_tta take them.  1 to 8 distinct integers in 0..7, ValueError otherwise."""
    try:
        codes = [int(c) for c in flips]
        exact = all(c == f for c, f in zip(codes, flips))
    except (TypeError, ValueError):
        codes, exact = [], False
    if not exact or not 1 <= len(codes) <= 8 or any(c < 0 or c > 7 for c in codes) or len(set(codes)) != len(codes):
        raise ValueError("sw: flips is a sequence of 1 to 8 distinct codes in 0..7 (bit 0 mirrors W, bit 1 H, bit 2 D), got %r" % (flips,))
    return len(codes), sum(c << (3 * i) for i, c in enumerate(codes))


def sw_gather(volume, origins, first, batch, patch=None, cval=0.0, out=None, flips=None):
    """Windows [first, first + batch) of the plan, cut from the planar fp32 volume (C, D, H, W) -> (batch, C, P, P, P).  `first`: an int32 device word.
    Slots past the plan and positions past the volume read cval.  out: the batch tensor to fill (a fixed address for a captured launch).
    flips (a sequence of codes, sw_flips): `first` counts items — item j is window j // nf mirrored by flips[j % nf] — and each slot is written
    already mirrored (vs_sw_gather_tta)."""
    packed = None if flips is None else sw_flips(flips)
    _require_cuda(volume, origins, first, out)
    if volume.dim() != 4 or volume.dtype != torch.float32 or not volume.is_contiguous() or volume.data_ptr() % 16:
        raise ValueError("sw_gather: expected a contiguous, 16-byte aligned fp32 (C, D, H, W) volume, got %s %s" % (tuple(volume.shape), volume.dtype))
    c, d, h, w = volume.shape
    if out is None:
        out = torch.empty((int(batch), c) + (int(patch),) * 3, dtype=torch.float32, device=volume.device)
    p = out.shape[-1]
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (int(batch), c, p, p, p) or (patch is not None and p != int(patch)):
        raise ValueError("sw_gather: out must be a contiguous fp32 (%d, %d, P, P, P) tensor, got %s" % (int(batch), c, tuple(out.shape)))
    _sw_common(origins, first, None, p)
    if packed is None:
        check(lib.vs_sw_gather(volume.data_ptr(), out.data_ptr(), origins.data_ptr(), first.data_ptr(), origins.shape[0], int(batch), c, d, h, w, p,
                               float(cval), _stream()), "sw_gather")
    else:
        check(lib.vs_sw_gather_tta(volume.data_ptr(), out.data_ptr(), origins.data_ptr(), first.data_ptr(), origins.shape[0], int(batch), c, d, h, w, p,
                                   float(cval), packed[0], packed[1], _stream()), "sw_gather_tta")
    return out


def sw_accumulate(prob, acc, wsum, origins, first, weights, flips=None):
    """acc (K, D, H, W) += w * prob (B, K, P, P, P) and wsum (D, H, W) += w for the windows [first, first + B) that lie in the plan, in place, every voxel's
    terms in ascending window index and without atomics: bit-identical for every B.  Batches are accumulated in ascending order of `first`.
    flips (as sw_gather): the slots are items, each probability is read mirrored back and weighted at the voxel's own position, terms in ascending item
    index (vs_sw_accumulate_tta)."""
    packed = None if flips is None else sw_flips(flips)
    _require_cuda(prob, acc, wsum, origins, first, weights)
    pr = _aligned16(prob.detach().float())
    if pr.dim() != 5 or acc.dim() != 4 or wsum.dim() != 3 or pr.shape[1] != acc.shape[0] or tuple(acc.shape[1:]) != tuple(wsum.shape) or \
            not (pr.shape[2] == pr.shape[3] == pr.shape[4]):
        raise ValueError("sw_accumulate: prob (B, K, P, P, P), acc (K, D, H, W), wsum (D, H, W); got %s, %s, %s" % (tuple(prob.shape), tuple(acc.shape), tuple(wsum.shape)))
    for t in (acc, wsum):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("sw_accumulate: acc and wsum are contiguous fp32 tensors (they are updated in place)")
    b, k, p = pr.shape[0], pr.shape[1], pr.shape[2]
    _sw_common(origins, first, weights, p)
    d, h, w = wsum.shape
    if packed is None:
        check(lib.vs_sw_accumulate(pr.data_ptr(), acc.data_ptr(), wsum.data_ptr(), origins.data_ptr(), first.data_ptr(), origins.shape[0], b, k, d, h, w, p,
                                   weights[0].data_ptr(), weights[1].data_ptr(), weights[2].data_ptr(), _stream()), "sw_accumulate")
    else:
        check(lib.vs_sw_accumulate_tta(pr.data_ptr(), acc.data_ptr(), wsum.data_ptr(), origins.data_ptr(), first.data_ptr(), origins.shape[0], b, k, d, h, w,
                                       p, weights[0].data_ptr(), weights[1].data_ptr(), weights[2].data_ptr(), packed[0], packed[1], _stream()),
              "sw_accumulate_tta")


def sw_finalize(acc, wsum, label=True, onehot=False):
    """-> (prob = acc / wsum (K, D, H, W) fp32, label (D, H, W) uint8 or None, onehot (K, D, H, W) fp32 or None) in one pass.  The label is the channel
    argmax of prob, ties to the first maximal channel (vs_hard_onehot's rule)."""
    _require_cuda(acc, wsum)
    if acc.dim() != 4 or tuple(acc.shape[1:]) != tuple(wsum.shape) or acc.dtype != torch.float32 or wsum.dtype != torch.float32 or \
            not acc.is_contiguous() or not wsum.is_contiguous():
        raise ValueError("sw_finalize: acc (K, D, H, W) and wsum (D, H, W) are contiguous fp32 tensors; got %s, %s" % (tuple(acc.shape), tuple(wsum.shape)))
    k, d, h, w = acc.shape
    prob = torch.empty_like(acc)
    lab = torch.empty((d, h, w), dtype=torch.uint8, device=acc.device) if label else None
    hot = torch.empty_like(acc) if onehot else None
    check(lib.vs_sw_finalize(acc.data_ptr(), wsum.data_ptr(), prob.data_ptr(), _p(lab), _p(hot), k, d, h, w, _stream()), "sw_finalize")
    return prob, lab, hot


# a patch-space prediction pasted back into scan geometry (csrc/uncrop.hip)
UNCROP_INTERPS = ("nearest", "linear")


def uncrop(prob, geometry, shape, interp="linear", want_prob=False):
    """The probabilities (K, P, P, P), 1 <= K <= 8, that a network gave on a CropResize patch, resampled onto the scan grid `shape` = (D, H, W).
    geometry = (lo[3], hi[3], off[3], side) of data_gpu.crop_geometry: scan voxel v with lo <= v < hi has cube index u = v - lo + off and patch coordinate
    (u + 0.5) P / side - 0.5.  interp "linear": trilinear, edge replicate; "nearest": the order-0 zoom's rounding.  Outside the cube: background.
    -> {"label": (D, H, W) uint8 — argmax, ties to the first channel — and, with want_prob, "prob": (K, D, H, W) fp32, (1, 0, ..., 0) outside the cube}.
    One launch writes both outputs whole; it does not synchronise."""
    _require_cuda(prob)
    if interp not in UNCROP_INTERPS:
        raise ValueError("uncrop: interp is one of %s, got %r" % (UNCROP_INTERPS, interp))
    pr = _aligned16(prob.detach().float())
    if pr.dim() != 4 or not (pr.shape[1] == pr.shape[2] == pr.shape[3]) or not 1 <= pr.shape[0] <= 8:
        raise ValueError("uncrop: expected probabilities (K, P, P, P) with 1 <= K <= 8, got %s" % (tuple(prob.shape),))
    lo, hi, off, side = geometry
    lo, hi, off = ([int(v) for v in t] for t in (lo, hi, off))
    d, h, w = (int(s) for s in shape)
    if not (len(lo) == len(hi) == len(off) == 3):
        raise ValueError("uncrop: geometry is (lo[3], hi[3], off[3], side), got %r" % (geometry,))
    label = torch.empty((d, h, w), dtype=torch.uint8, device=pr.device)
    out = torch.empty((pr.shape[0], d, h, w), dtype=torch.float32, device=pr.device) if want_prob else None
    check(lib.vs_uncrop(pr.data_ptr(), label.data_ptr(), _p(out), pr.shape[0], pr.shape[1], d, h, w, *lo, *hi, *off, int(side),
                        UNCROP_INTERPS.index(interp), _stream()), "uncrop")
    res = {"label": label}
    if want_prob:
        res["prob"] = out
    return res


# scan geometry: the array a scanner wrote <-> the re-oriented 1 mm grid (csrc/scan.hip; data_gpu.ScanGeometry does the host arithmetic)
SCAN_DTYPES = {torch.int16: _lib.VS_SCAN_I16, torch.uint8: _lib.VS_SCAN_U8, torch.int8: _lib.VS_SCAN_I8, torch.float32: _lib.VS_SCAN_F32}


def _scan_geometry(geometry, what):
    """-> (x, y, z, flip0, flip1, flip2, d1, h1, w1): a data_gpu.ScanGeometry or its as_tuple()"""
    g = geometry.as_tuple() if hasattr(geometry, "as_tuple") else tuple(geometry)
    if len(g) != 9:
        raise ValueError("%s: geometry is a data_gpu.ScanGeometry or its as_tuple() (x, y, z, flip0, flip1, flip2, d1, h1, w1), got %r" % (what, geometry))
    g = tuple(int(v) for v in g)
    if min(g[:3] + g[6:]) < 1:
        raise ValueError("%s: empty shape in geometry %r" % (what, g))
    return g


def _scan_tensor(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s: expected a CUDA tensor (libvaeseg HIP kernels; there is no CPU fallback), got %s" %
                        (what, "a %s tensor" % t.device.type if isinstance(t, torch.Tensor) else type(t).__name__))
    return _aligned16(t.detach())


def scan_orient(raw, geometry):
    """raw (X, Y, Z) int16 / uint8 / int8 / float32 as the scanner wrote it -> the oriented float32 volume (Y, X, Z) of data_process.py:29-30,
    transpose(raw, [1, 0, 2])[::ind[1], ::ind[0], ::ind[2]], exact values, one launch (vs_scan_orient)."""
    r = _scan_tensor(raw, "scan_orient")
    if r.dtype not in SCAN_DTYPES:
        raise TypeError("scan_orient: raw is int16, uint8, int8 or float32, got %s" % r.dtype)
    if r.dim() != 3:
        raise ValueError("scan_orient: expected a raw scan (X, Y, Z), got shape %s" % (tuple(r.shape),))
    x, y, z, f0, f1, f2 = _scan_geometry(geometry, "scan_orient")[:6]
    if tuple(r.shape) != (x, y, z):
        raise ValueError("scan_orient: the geometry's raw_shape %s is not the tensor's %s" % ((x, y, z), tuple(r.shape)))
    out = torch.empty((y, x, z), dtype=torch.float32, device=r.device)
    check(lib.vs_scan_orient(r.data_ptr(), SCAN_DTYPES[r.dtype], out.data_ptr(), x, y, z, f0, f1, f2, _stream()), "scan_orient")
    return out


def to_native(src, geometry, interp="linear", want_prob=False):
    """An answer on the 1 mm grid put back onto the voxel grid of the scan it came from, in that scan's axis order, orientation and spacing.
    src: planar probabilities (K, D1, H1, W1), 1 <= K <= 8 (any float dtype; resampled in fp32), or a uint8 label (D1, H1, W1), which is a copy of
    samples and takes interp="nearest" only.  Raw voxel (i0, i1, i2) has the oriented index (f(i1), f(i0), f(i2)), f the per-axis flip, and per axis the
    1 mm coordinate q = (o + 0.5) n_1mm / n_oriented - 0.5 (fp64).  "nearest": the sample at floor(q + 0.5) clamped to [0, n_1mm - 1]; "linear":
    trilinear with q mirrored at the borders, scipy.ndimage.zoom(order=1, mode="mirror", grid_mode=True).
    -> {"label": (X, Y, Z) uint8 — argmax, ties to the first channel — and, with want_prob, "prob": (K, X, Y, Z) fp32}.  One launch writes both outputs
    whole (vs_scan_to_native); it does not synchronise and can be captured in a graph."""
    s = _scan_tensor(src, "to_native")
    if interp not in UNCROP_INTERPS:
        raise ValueError("to_native: interp is one of %s, got %r" % (UNCROP_INTERPS, interp))
    is_label = s.dtype == torch.uint8
    if is_label:
        if s.dim() != 3:
            raise ValueError("to_native: expected a uint8 label (D1, H1, W1), got shape %s" % (tuple(s.shape),))
        if interp != "nearest" or want_prob:
            raise ValueError("to_native: a uint8 label is a copy of samples: interp=\"nearest\" and no probabilities")
        k = 1
    else:
        if not s.is_floating_point():
            raise TypeError("to_native: src is floating-point probabilities (K, D1, H1, W1) or a uint8 label (D1, H1, W1), got %s" % s.dtype)
        if s.dim() != 4 or not 1 <= s.shape[0] <= 8:
            raise ValueError("to_native: expected probabilities (K, D1, H1, W1) with 1 <= K <= 8, got shape %s" % (tuple(s.shape),))
        if s.dtype != torch.float32:
            s = s.float()
        k = int(s.shape[0])
    x, y, z, f0, f1, f2, d1, h1, w1 = _scan_geometry(geometry, "to_native")
    if tuple(s.shape[-3:]) != (d1, h1, w1):
        raise ValueError("to_native: the geometry's shape_1mm %s is not the tensor's %s" % ((d1, h1, w1), tuple(s.shape[-3:])))
    label = torch.empty((x, y, z), dtype=torch.uint8, device=s.device)
    out = torch.empty((k, x, y, z), dtype=torch.float32, device=s.device) if want_prob else None
    check(lib.vs_scan_to_native(s.data_ptr(), int(is_label), label.data_ptr(), _p(out), k, d1, h1, w1, x, y, z, f0, f1, f2, UNCROP_INTERPS.index(interp),
                                _stream()), "scan_to_native")
    res = {"label": label}
    if want_prob:
        res["prob"] = out
    return res


# ---- intensity augmentation (csrc/augment.hip; the transform lives in data_gpu.py) ---------------------------------------------------------------------
AUG_MAX_SIGMA = 2.0                 # radius int(4 sigma + 0.5) <= 8: what the blur kernel's LDS tile is sized for
AUG_OPS = {"none": 0, "contrast": 1, "power": 2, "restat": 3}


def _aug_planes(x, what):
    """a contiguous CUDA float32 tensor (..., D, H, W) -> (planes, d, h, w)"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() < 3:
        raise TypeError("%s: a float32 tensor (..., D, H, W), got %s %s" % (what, getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))
    d, h, w = (int(v) for v in x.shape[-3:])
    if x.numel() == 0 or d * h * w >= 2 ** 31:
        raise ValueError("%s: an empty tensor or a plane of 2^31 voxels or more, shape %s" % (what, tuple(x.shape)))
    if not x.is_contiguous():
        raise ValueError("%s: the tensor must be contiguous" % what)
    _require_cuda(x)
    return x.numel() // (d * h * w), d, h, w


def _aug_workspace(planes, d, h, w, device):
    return torch.empty(int(lib.vs_aug_stats_workspace_bytes(planes, d, h, w)) // 8, dtype=torch.float64, device=device)


def aug_stats(x):
    """{min, max, mean, population std} of every (D, H, W) plane of a float32 tensor (..., D, H, W) -> fp64 (..., 4) on the device.  fp64 sums shifted by
    the plane's first voxel, over a fixed chunking of the linear voxel index in chunk order: a function of the plane's bits alone (two launches, no
    atomics, no synchronisation) — the record vs_aug_stage's epilogue writes for the plane it stores."""
    planes, d, h, w = _aug_planes(x, "aug_stats")
    rec = torch.empty(tuple(x.shape[:-3]) + (4,), dtype=torch.float64, device=x.device)
    ws = _aug_workspace(planes, d, h, w, x.device)
    check(lib.vs_aug_stats(x.data_ptr(), rec.data_ptr(), ws.data_ptr(), planes, d, h, w, _stream()), "aug_stats")
    return rec


def philox_normal(shape, seed, sample, channel=0):
    """the standard normals of one plane `shape` = (D, H, W), fp64 on the device: Philox4x32-10 under key `seed` and counter (pair, 0x100 + channel,
    sample), Box-Muller in fp64 (vs_aug_normal_philox) — what a noise stage with the source (seed, sample) adds, times s"""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("philox_normal: shape is (D, H, W), got %r" % (shape,))
    out = torch.empty(shape, dtype=torch.float64, device="cuda")
    check(lib.vs_aug_normal_philox(out.data_ptr(), *shape, int(seed) & (2 ** 64 - 1), int(sample) & (2 ** 64 - 1), int(channel), _stream()),
          "aug_normal_philox")
    return out


def gaussian_weights(sigma):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5)) from the centre outwards: w[k] is the weight of taps -k and +k (host, numpy)"""
    sigma = float(sigma)
    if not 0.0 < sigma <= AUG_MAX_SIGMA:
        raise ValueError("gaussian blur: 0 < sigma <= %g (radius <= 8), got %r" % (AUG_MAX_SIGMA, sigma))
    radius = int(4.0 * sigma + 0.5)
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:], dtype=np.float64)


def blur_tile(sigma):
    """the (z, y, x) tile of outputs one workgroup of the blur kernel computes at this sigma"""
    t = (_ctypes.c_int * 3)()
    check(lib.vs_aug_blur_tile(float(sigma), t), "aug_blur_tile")
    return tuple(t)


def gaussian_blur3d(x, sigma):
    """scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4) of one float32 volume (D, H, W): passes along z, y, x, fp64 accumulation,
    rounded to fp32 after each; one launch, the three passes over an LDS tile (vs_aug_blur).  0 < sigma <= 2."""
    planes, d, h, w = _aug_planes(x, "gaussian_blur3d")
    if x.dim() != 3:
        raise ValueError("gaussian_blur3d: one volume (D, H, W), got shape %s" % (tuple(x.shape),))
    wts = gaussian_weights(sigma)
    out = torch.empty_like(x)
    check(lib.vs_aug_blur(x.data_ptr(), out.data_ptr(), d, h, w, float(sigma), wts.ctypes.data, _stream()), "aug_blur")
    return out


def aug_flip(x, mask):
    """every (D, H, W) plane of a float32 tensor (..., D, H, W) mirrored along z / y / x for the bits 4 / 2 / 1 of mask: a copy (vs_aug_flip)"""
    planes, d, h, w = _aug_planes(x, "aug_flip")
    mask = int(mask)
    if not 0 <= mask <= 7:
        raise ValueError("aug_flip: mask is 0..7 (z, y, x = 4, 2, 1), got %r" % (mask,))
    out = torch.empty_like(x)
    check(lib.vs_aug_flip(x.data_ptr(), out.data_ptr(), planes, d, h, w, mask, _stream()), "aug_flip")
    return out


def aug_stage(x, flip=0, flip_first=False, noise=None, s=0.0, channel=0, mult=None, op="none", p=0.0, flag=False, rec=None, rec0=None, mean0=0.0,
              std0=1.0, want_rec=False):
    """One pass of vs_aug_stage over one float32 volume (D, H, W) -> (y, record of y or None).  noise: None, an fp64 device tensor of x's shape, or a
    tuple (seed, sample) for the Philox normals of `channel`; rec / rec0: fp64 records (4,) on the device (aug_stats); see include/vaeseg.h for the
    order of the steps.  One launch, two with want_rec; nothing is synchronised or read back."""
    planes, d, h, w = _aug_planes(x, "aug_stage")
    if x.dim() != 3:
        raise ValueError("aug_stage: one volume (D, H, W), got shape %s" % (tuple(x.shape),))
    mode, narr, seed, sample = 0, None, 0, 0
    if isinstance(noise, tuple):
        mode, seed, sample = 2, int(noise[0]) & (2 ** 64 - 1), int(noise[1]) & (2 ** 64 - 1)
    elif noise is not None:
        if not (isinstance(noise, torch.Tensor) and noise.dtype == torch.float64 and noise.shape == x.shape and noise.is_cuda and noise.is_contiguous()):
            raise TypeError("aug_stage: noise is a contiguous CUDA float64 tensor of shape %s or a tuple (seed, sample)" % (tuple(x.shape),))
        mode, narr = 1, noise
    y = torch.empty_like(x)
    rec_out = torch.empty(4, dtype=torch.float64, device=x.device) if want_rec else None
    ws = _aug_workspace(1, d, h, w, x.device) if want_rec else None
    check(lib.vs_aug_stage(x.data_ptr(), y.data_ptr(), d, h, w, int(flip), int(bool(flip_first)), mode, _p(narr), float(s), seed, sample, int(channel),
                           int(mult is not None), 1.0 if mult is None else float(mult), AUG_OPS[op], float(p), int(bool(flag)), _p(rec), _p(rec0),
                           float(mean0), float(std0), _p(rec_out), _p(ws), _stream()), "aug_stage")
    return y, rec_out


# ---- zoom with edge boundaries, simulated low resolution (csrc/lowres.hip) ---------------------------------------------------------------
ZOOM_EDGE_ORDERS = (0, 1, 3)
ZOOM_EDGE_MAX_LEN = 512             # order 3: the longest line a workgroup's LDS bundle holds


def zoom_edge_bundle(m, n):
    """the lines one workgroup of an order-3 pass holds at input length m and output length n"""
    return int(lib.vs_zoom_edge_bundle(int(m), int(n)))


def _zoom_edge_shape(shape, what):
    try:
        out = tuple(int(v) for v in shape)
    except TypeError:
        raise TypeError("%s: a shape (D, H, W), got %r" % (what, shape))
    if len(out) != 3 or min(out) < 1:
        raise ValueError("%s: a shape (D, H, W) of positive lengths, got %r" % (what, shape))
    return out


def zoom_edge(x, out_shape, order=3, clip=True):
    """scipy.ndimage.zoom(x.astype(float64), out / in, order=order, mode="nearest", grid_mode=True) of one float32 volume (D, H, W), clipped to
    [x.min(), x.max()] when clip (and order > 0), rounded to float32 once.  order 0, 1 or 3; order 3: every axis of x and of out_shape at most 512.
    One launch for orders 0 and 1, three for order 3, two more for the clip's bounds, which stay on the device; nothing is synchronised or read back."""
    planes, d, h, w = _aug_planes(x, "zoom_edge")
    if x.dim() != 3:
        raise ValueError("zoom_edge: one volume (D, H, W), got shape %s" % (tuple(x.shape),))
    out_shape = _zoom_edge_shape(out_shape, "zoom_edge")
    if order not in ZOOM_EDGE_ORDERS:
        raise ValueError("zoom_edge: order is 0, 1 or 3, got %r" % (order,))
    order = int(order)
    if order == 3 and max((d, h, w) + out_shape) > ZOOM_EDGE_MAX_LEN:
        raise ValueError("zoom_edge: order 3 takes axes of at most %d voxels, got %s -> %s" % (ZOOM_EDGE_MAX_LEN, (d, h, w), out_shape))
    if out_shape[0] * out_shape[1] * out_shape[2] >= 2 ** 31:
        raise ValueError("zoom_edge: an output of 2^31 voxels or more, shape %s" % (out_shape,))
    y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(lib.vs_zoom_edge_workspace_bytes(d, h, w, *out_shape, order)) // 8, dtype=torch.float64, device=x.device)
    check(lib.vs_zoom_edge(x.data_ptr(), y.data_ptr(), d, h, w, *out_shape, order, int(bool(clip)), ws.data_ptr(), _stream()), "zoom_edge")
    return y


def simulate_lowres(x, target_shape, order_down=0, order_up=3):
    """nnU-Net's simulated low resolution of one float32 volume (D, H, W): zoom_edge down to target_shape (order_down, clipped when order_down > 0), then
    zoom_edge back to x's shape (order_up, clipped to the down-sampled volume's range when order_up > 0).  The bits of the two calls."""
    planes, d, h, w = _aug_planes(x, "simulate_lowres")
    if x.dim() != 3:
        raise ValueError("simulate_lowres: one volume (D, H, W), got shape %s" % (tuple(x.shape),))
    target_shape = _zoom_edge_shape(target_shape, "simulate_lowres")
    for order in (order_down, order_up):
        if order not in ZOOM_EDGE_ORDERS:
            raise ValueError("simulate_lowres: an order is 0, 1 or 3, got %r" % (order,))
    t = zoom_edge(x, target_shape, order_down, clip=order_down > 0)
    return zoom_edge(t, (d, h, w), order_up, clip=order_up > 0)


# ---- exact percentiles and the piecewise-linear intensity map (csrc/quantile.hip) --------------------------------------------------------
QUANTILE_MAX_Q = 16
QUANTILE_WG_VOXELS = 16384          # csrc/quantile.hip QS_WG_VOXELS: the voxels of a plane one workgroup of a counting pass reads (a hand-kept mirror,
                                    # as INTENSITY_MAP_WG_VOXELS is of IM_WG_VOXELS: the library does not export them; change both files together)
INTENSITY_MAP_MAX_L = 16
INTENSITY_MAP_WG_VOXELS = 4096      # csrc/quantile.hip IM_WG_VOXELS
INTENSITY_MAP_EXTRAPOLATE = ("linear", "clamp")


def quantile(x, q, above=None, mask=None):
    """Exact percentiles of every (D, H, W) plane of a contiguous CUDA float32 tensor (..., D, H, W); q: 1 to 16 percentiles in [0, 100], host floats.
    A voxel is selected iff it is finite, `above` is None or x > np.float32(above) (strict), and `mask` (uint8 or bool, x's shape) is None or non-zero
    there.  With v the n selected values sorted, in fp64: h = (n - 1) * (p / 100), k = floor(h), t = h - k, a = v[k], b = v[min(k + 1, n - 1)] and
    t >= 0.5 ? b - (b - a) (1 - t) : a + (b - a) t, each operation rounded on its own — the bits of np.percentile(selected.astype(float64), p).
    -> {"q": fp64 (..., Q); "lo", "hi": float32 (..., Q), a and b; "count": int64 (...), n; "rejected": int64 (...), the non-finite voxels}, on the
    device; n == 0 gives NaN.  A radix select, nine launches whatever the data; nothing is synchronised or read back (vs_quantile)."""
    planes, d, h, w = _aug_planes(x, "quantile")
    try:
        ps = [float(v) for v in (q if hasattr(q, "__iter__") else [q])]
    except (TypeError, ValueError):
        raise ValueError("quantile: q is a percentile or a sequence of percentiles, got %r" % (q,)) from None
    if not 1 <= len(ps) <= QUANTILE_MAX_Q:
        raise ValueError("quantile: 1 to %d percentiles, got %d" % (QUANTILE_MAX_Q, len(ps)))
    if any(not math.isfinite(p) or p < 0.0 or p > 100.0 for p in ps):
        raise ValueError("quantile: percentiles are finite numbers in [0, 100], got %r" % (ps,))
    use_above, thr = 0, 0.0
    if above is not None:
        thr = float(above)
        if math.isnan(thr):
            raise ValueError("quantile: above is a number, got %r" % (above,))
        use_above = 1
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool):
            raise TypeError("quantile: mask is a uint8 or bool tensor, got %s" % getattr(mask, "dtype", type(mask)))
        if mask.shape != x.shape or mask.device != x.device or not mask.is_contiguous():
            raise ValueError("quantile: mask is a contiguous tensor of x's shape on x's device, got %s on %s" % (tuple(mask.shape), mask.device))
    nq, lead = len(ps), tuple(x.shape[:-3])
    p01 = (_ctypes.c_double * nq)(*[p / 100.0 for p in ps])
    out = {"q": torch.empty(lead + (nq,), dtype=torch.float64, device=x.device),
           "lo": torch.empty(lead + (nq,), dtype=torch.float32, device=x.device),
           "hi": torch.empty(lead + (nq,), dtype=torch.float32, device=x.device),
           "count": torch.empty(lead, dtype=torch.int64, device=x.device),
           "rejected": torch.empty(lead, dtype=torch.int64, device=x.device)}
    ws = torch.empty((int(lib.vs_quantile_workspace_bytes(planes, d * h * w, nq)) + 15) // 16 * 2, dtype=torch.float64, device=x.device)
    check(lib.vs_quantile(x.data_ptr(), _p(mask), use_above, thr, _ctypes.addressof(p01), nq, out["q"].data_ptr(), out["lo"].data_ptr(),
                          out["hi"].data_ptr(), out["count"].data_ptr(), out["rejected"].data_ptr(), ws.data_ptr(), planes, d, h, w, _stream()), "quantile")
    return out


def intensity_map(x, src, dst, extrapolate="linear", out=None):
    """The piecewise-linear map of every (D, H, W) plane of a contiguous CUDA float32 tensor (..., D, H, W) through landmarks on the device: src fp64
    (..., L), one ascending row per plane (quantile's "q", never copied to the host); dst fp64 (L,), strictly ascending, for all planes; 2 <= L <= 16.
    A finite voxel x with j the largest index in [0, L - 2] with src[j] <= x (0 below src[0]): y = dst[j] + (x - src[j]) * slope, slope =
    (dst[j+1] - dst[j]) / (src[j+1] - src[j]) or 0 for a segment of no width, in fp64, each operation rounded on its own, rounded to float32 once.
    extrapolate "linear": the end segments run on; "clamp": y is clamped to [dst[0], dst[L-1]].  A non-finite voxel and a plane with NaN landmarks
    are written unchanged.  -> float32 of x's shape (`out`, which may be x).  One launch, no synchronisation (vs_intensity_map)."""
    planes, d, h, w = _aug_planes(x, "intensity_map")
    if extrapolate not in INTENSITY_MAP_EXTRAPOLATE:
        raise ValueError("intensity_map: extrapolate is 'linear' or 'clamp', got %r" % (extrapolate,))
    for t, what in ((src, "src"), (dst, "dst")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise TypeError("intensity_map: %s is a float64 tensor on the device, got %s" % (what, getattr(t, "dtype", type(t))))
        if t.device != x.device or not t.is_contiguous():
            raise ValueError("intensity_map: %s is contiguous and on x's device" % what)
    if dst.dim() != 1 or not 2 <= dst.shape[0] <= INTENSITY_MAP_MAX_L:
        raise ValueError("intensity_map: dst has shape (L,) with 2 <= L <= %d, got %s" % (INTENSITY_MAP_MAX_L, tuple(dst.shape)))
    nl = int(dst.shape[0])
    if tuple(src.shape) != tuple(x.shape[:-3]) + (nl,):
        raise ValueError("intensity_map: src has shape %s for x %s and L = %d, got %s" % (tuple(x.shape[:-3]) + (nl,), tuple(x.shape), nl, tuple(src.shape)))
    if out is None:
        out = torch.empty_like(x)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.shape == x.shape and out.device == x.device and out.is_contiguous()):
        raise ValueError("intensity_map: out is a contiguous float32 tensor of x's shape on x's device")
    check(lib.vs_intensity_map(x.data_ptr(), src.data_ptr(), dst.data_ptr(), nl, int(extrapolate == "clamp"), out.data_ptr(), planes, d, h, w, _stream()),
          "intensity_map")
    return out


# ---- training patches: foreground-oversampled windows cut on the device (csrc/patch.hip) ------------------------------------------------
# __all__ above is the list of names that moved here from ops.py, which tests/test_host.py pins; this section's public names are PATCH_NAMES, and ops
# imports them by name.
PATCH_NAMES = ("PATCH_CHUNK", "PATCH_MAX_CLASSES", "PATCH_MAX_SOURCES", "PATCH_LABEL_DTYPES", "patch_index", "patch_pick", "patch_gather")
PATCH_CHUNK = int(lib.vs_patch_chunk())     # VS_PATCH_CHUNK: the voxels of the linear index one row of patch_index's table stands for
PATCH_MAX_CLASSES = 8
PATCH_MAX_SOURCES = 4
PATCH_LABEL_DTYPES = {torch.float32: _lib.VS_PATCH_F32, torch.uint8: _lib.VS_PATCH_U8}


def _patch_label(label, what):
    if not isinstance(label, torch.Tensor) or label.dtype not in PATCH_LABEL_DTYPES:
        raise TypeError("%s: label is a float32 or uint8 tensor (D, H, W), got %s" % (what, getattr(label, "dtype", type(label))))
    if label.dim() != 3 or label.numel() == 0 or label.numel() >= 2 ** 31:
        raise ValueError("%s: label is a non-empty (D, H, W) volume of fewer than 2^31 voxels, got shape %s" % (what, tuple(label.shape)))
    if not label.is_contiguous():
        raise ValueError("%s: label must be contiguous" % what)
    _require_cuda(label)
    return tuple(int(v) for v in label.shape)


def _patch_n_class(n_class, what):
    if not isinstance(n_class, _numbers.Integral) or not 1 <= n_class <= PATCH_MAX_CLASSES:
        raise ValueError("%s: n_class is an integer in [1, %d], got %r" % (what, PATCH_MAX_CLASSES, n_class))
    return int(n_class)


def _patch_sides(patch, what):
    try:
        sides = tuple(int(p) for p in ((patch,) * 3 if isinstance(patch, _numbers.Integral) else patch))
        exact = isinstance(patch, _numbers.Integral) or all(s == p for s, p in zip(sides, patch))
    except (TypeError, ValueError):
        sides, exact = (), False
    if not exact or len(sides) != 3 or min(sides) < 1:
        raise ValueError("%s: patch is a positive side or three of them (D, H, W), got %r" % (what, patch))
    return sides


def patch_index(label, n_class):
    """The position index of a label (D, H, W), float32 or uint8 on the device: int32 (n_chunks + 1, n_class), row j = the voxels of each class in the
    first j chunks of PATCH_CHUNK consecutive voxels of the linear index (z H + y) W + x, the last row the totals.  A voxel belongs to class k iff its
    value is the integer k in [0, n_class), n_class <= 8; NaN, fractions and larger values are counted nowhere.  Two launches, no atomics, nothing
    synchronised or read back (vs_patch_index)."""
    d, h, w = _patch_label(label, "patch_index")
    nc = _patch_n_class(n_class, "patch_index")
    table = torch.empty(((d * h * w + PATCH_CHUNK - 1) // PATCH_CHUNK + 1, nc), dtype=torch.int32, device=label.device)
    assert table.numel() * 4 == lib.vs_patch_index_bytes(d, h, w, nc)
    check(lib.vs_patch_index(label.data_ptr(), PATCH_LABEL_DTYPES[label.dtype], d, h, w, nc, table.data_ptr(), _stream()), "patch_index")
    return table


def patch_pick(label, index, classes, words, forced, patch):
    """The origins of R patch requests: words uint32-valued (R, 5) = (wc, wv, wz, wy, wx) as an int64 or int32 tensor on the device (int64
    values in [0, 2^32); int32 is taken as the same 32 bits), forced int32 (R,), classes the sampler's class list (distinct integers in [0, n_class), any
    order), patch a side or (D, H, W) sides, index = patch_index(label, n_class).  A forced request whose list has a class present takes class
    present[(wc mc) >> 32], its voxel of rank (wv n_k) >> 32 in ascending linear index, and the origin min(max(lb, v - P // 2), ub) per axis; any other
    request the free origin lb + ((w_axis (ub - lb + 1)) >> 32).  -> picks int32 (R, 8) = (oz, oy, ox, class or -1, vz, vy, vx or -1, 0), on the device.
    One launch of a wave per request; nothing synchronised or read back (vs_patch_pick)."""
    d, h, w = _patch_label(label, "patch_pick")
    sides = _patch_sides(patch, "patch_pick")
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 2 or not index.is_contiguous() or index.device != label.device or \
            index.shape[0] != (d * h * w + PATCH_CHUNK - 1) // PATCH_CHUNK + 1 or not 1 <= index.shape[1] <= PATCH_MAX_CLASSES:
        raise ValueError("patch_pick: index is patch_index(label, n_class), a contiguous int32 (n_chunks + 1, n_class) tensor on the label's device")
    nc = int(index.shape[1])
    try:
        cls = [int(c) for c in classes]
        exact = all(c == k for c, k in zip(cls, classes))
    except (TypeError, ValueError):
        cls, exact = [], False
    if not exact or len(set(cls)) != len(cls) or any(c < 0 or c >= nc for c in cls):
        raise ValueError("patch_pick: classes are distinct integers in [0, %d), got %r" % (nc, classes))
    cls.sort()
    if not isinstance(words, torch.Tensor) or words.dtype not in (torch.int64, torch.int32) or words.dim() != 2 or words.shape[1] != 5 or words.shape[0] < 1:
        raise ValueError("patch_pick: words is an int64 or int32 tensor (R, 5) with R >= 1")
    if not isinstance(forced, torch.Tensor) or forced.dtype != torch.int32 or tuple(forced.shape) != (words.shape[0],) or not forced.is_contiguous():
        raise ValueError("patch_pick: forced is a contiguous int32 tensor (R,) for words (R, 5)")
    _require_cuda(words, forced)
    w32 = _contig(words.to(torch.int32)) if words.dtype == torch.int64 else _contig(words)        # int64 -> int32 keeps the low 32 bits
    r = int(w32.shape[0])
    picks = torch.empty((r, 8), dtype=torch.int32, device=label.device)
    check(lib.vs_patch_pick(label.data_ptr(), PATCH_LABEL_DTYPES[label.dtype], index.data_ptr(), nc, len(cls), sum(c << (3 * i) for i, c in enumerate(cls)),
                            w32.data_ptr(), forced.data_ptr(), r, d, h, w, sides[0], sides[1], sides[2], picks.data_ptr(), _stream()), "patch_pick")
    return picks


def patch_gather(sources, cvals, picks, patch, margin=0):
    """The blocks of R requests cut from 1 to 4 float32 volumes of one shape (D, H, W): block i of source s is rows [o - margin, o - margin + Q) per axis,
    Q = patch + 2 margin, o = picks[i, :3] read on the device (any integers); positions outside the volume read cvals[s].  -> a tuple of (R, 1, Qd, Qh, Qw)
    tensors, one per source, views of one (n_src, R, Qd, Qh, Qw) block.  One launch, nothing synchronised or read back (vs_patch_gather)."""
    try:
        srcs = list(sources)
        cv = [float(c) for c in cvals]
    except (TypeError, ValueError):
        raise ValueError("patch_gather: sources is a sequence of volumes and cvals one number for each") from None
    if not 1 <= len(srcs) <= PATCH_MAX_SOURCES or len(cv) != len(srcs) or any(math.isnan(c) for c in cv):
        raise ValueError("patch_gather: 1 to %d sources and one cval (not NaN) for each, got %d and %r" % (PATCH_MAX_SOURCES, len(srcs), cvals))
    for t in srcs:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("patch_gather: a source is a float32 tensor (D, H, W), got %s" % getattr(t, "dtype", type(t)))
        if t.dim() != 3 or t.numel() == 0 or t.numel() >= 2 ** 31 or t.shape != srcs[0].shape or t.device != srcs[0].device:
            raise ValueError("patch_gather: the sources are non-empty (D, H, W) volumes of one shape on one device, got %s" % [tuple(s.shape) for s in srcs])
        if not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError("patch_gather: a source must be contiguous and 16-byte aligned")
    _require_cuda(*srcs)
    sides = _patch_sides(patch, "patch_gather")
    if not isinstance(margin, _numbers.Integral) or margin < 0:
        raise ValueError("patch_gather: margin is a non-negative integer, got %r" % (margin,))
    if not isinstance(picks, torch.Tensor) or picks.dtype != torch.int32 or picks.dim() != 2 or picks.shape[1] != 8 or picks.shape[0] < 1 or \
            not picks.is_contiguous() or picks.device != srcs[0].device or picks.data_ptr() % 16:
        raise ValueError("patch_gather: picks is patch_pick's contiguous int32 (R, 8) tensor on the sources' device")
    r, q = int(picks.shape[0]), tuple(s + 2 * int(margin) for s in sides)
    if q[0] * q[1] * q[2] >= 2 ** 31:
        raise ValueError("patch_gather: a block of 2^31 voxels or more, %s" % (q,))
    out = torch.empty((len(srcs), r) + q, dtype=torch.float32, device=srcs[0].device)
    ptrs = [t.data_ptr() for t in srcs] + [None] * (PATCH_MAX_SOURCES - len(srcs))
    cv = cv + [0.0] * (PATCH_MAX_SOURCES - len(cv))
    d, h, w = (int(v) for v in srcs[0].shape)
    check(lib.vs_patch_gather(ptrs[0], ptrs[1], ptrs[2], ptrs[3], cv[0], cv[1], cv[2], cv[3], len(srcs), picks.data_ptr(), r, d, h, w, sides[0], sides[1],
                              sides[2], int(margin), out.data_ptr(), _stream()), "patch_gather")
    return tuple(out[s].unsqueeze(1) for s in range(len(srcs)))
