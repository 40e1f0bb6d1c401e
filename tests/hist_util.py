"""The binning rule of csrc/hist.hip and the tail of the reference's mutual_information_3d, restated with numpy and scipy: the yardstick of
tests/test_gpu_hist.py, pinned against np.histogram / np.histogram2d by tests/test_host_hist.py.  Nothing here reads the reference or the package.

The rule: for `bins` = B and bounds lo <= hi (lo == hi becomes lo - 0.5, hi + 0.5) the edges are np.linspace(lo, hi, B + 1) on Python floats — fp64,
e_i = i * step + lo with product and sum rounded separately, e_B = hi.  A value, promoted to fp64, is in bin i iff e_i <= x < e_{i+1}; x == e_B is in bin
B - 1; NaN, +-inf and values outside [e_0, e_B] are in no bin ("outside")."""
import numpy as np
from scipy import ndimage

EPS = np.finfo(float).eps


def ref_bounds(x):
    """bounds from the data: minimum and maximum over the finite values, a zero bound being +0.0; (0, 0) without a finite value"""
    x = np.asarray(x, dtype=np.float64).ravel()
    x = x[np.isfinite(x)]
    if x.size == 0:
        return 0.0, 0.0
    return float(x.min()) + 0.0, float(x.max()) + 0.0


def ref_edges(lo, hi, bins):
    lo, hi = float(lo), float(hi)
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, int(bins) + 1)


def ref_bin(x, edges):
    """-> (bin index per value, int64, -1 where the value is in no bin)"""
    x64 = np.asarray(x).astype(np.float64).ravel()
    b = len(edges) - 1
    idx = np.searchsorted(edges, x64, side="right") - 1
    idx[x64 == edges[-1]] = b - 1
    ok = np.isfinite(x64) & (x64 >= edges[0]) & (x64 <= edges[-1])
    return np.where(ok, idx, -1).astype(np.int64)


def ref_histogram(x, bins, bounds=None, labels=None, rows=0):
    """one plane -> {"table": int64 (rows + 1, bins), "edges", "outside", "overflow"}; labels outside [0, rows] are counted in overflow and nowhere else"""
    lo, hi = ref_bounds(x) if bounds is None else bounds
    edges = ref_edges(lo, hi, bins)
    idx = ref_bin(x, edges)
    lab = np.zeros(idx.shape, np.int64) if labels is None else np.asarray(labels).astype(np.int64).ravel()
    bad = (lab < 0) | (lab > rows)
    keep = ~bad & (idx >= 0)
    table = np.bincount(lab[keep] * bins + idx[keep], minlength=(rows + 1) * bins).reshape(rows + 1, bins).astype(np.int64)
    return {"table": table, "edges": edges, "outside": int((~bad & (idx < 0)).sum()), "overflow": int(bad.sum())}


def ref_joint_histogram(x, y, bins, bounds=None):
    """one plane -> {"table": int64 (bins_x, bins_y), "edges_x", "edges_y", "outside"}; bounds = ((lo_x, hi_x), (lo_y, hi_y)) or None (from the data)"""
    bx, by = bins
    (lx, hx), (ly, hy) = (ref_bounds(x), ref_bounds(y)) if bounds is None else bounds
    ex, ey = ref_edges(lx, hx, bx), ref_edges(ly, hy, by)
    ix, iy = ref_bin(x, ex), ref_bin(y, ey)
    keep = (ix >= 0) & (iy >= 0)
    table = np.bincount(ix[keep] * by + iy[keep], minlength=bx * by).reshape(bx, by).astype(np.int64)
    return {"table": table, "edges_x": ex, "edges_y": ey, "outside": int((~keep).sum())}


def ref_mutual_information(table, sigma=1.0, normalized=True):
    """the reference's formula on a joint histogram (utils/utils.py:827-845)"""
    jh = np.asarray(table, dtype=np.float64)
    if sigma:
        jh = ndimage.gaussian_filter(jh, sigma=sigma, mode="constant")
    jh = jh + EPS
    jh = jh / np.sum(jh)
    s1, s2 = np.sum(jh, axis=0), np.sum(jh, axis=1)
    hj, h1, h2 = np.sum(jh * np.log(jh)), np.sum(s1 * np.log(s1)), np.sum(s2 * np.log(s2))
    return float((h1 + h2) / hj - 1) if normalized else float(hj - h1 - h2)


def ref_mutual_information_3d(x, y, sigma=1, normalized=True):
    rec = ref_joint_histogram(np.asarray(x).ravel(), np.asarray(y).ravel(), (256, 256))
    return ref_mutual_information(rec["table"], sigma, normalized)


# ---- test volumes -------------------------------------------------------------------------------------------------------------------------
def smooth_volume(shape, seed):
    """a smooth random volume in about [-1, 1]: white noise blurred, then scaled"""
    rng = np.random.default_rng(seed)
    v = ndimage.gaussian_filter(rng.standard_normal(shape), 1.5, mode="wrap")
    return (v / np.abs(v).max()).astype(np.float32)


def ct_like_volume(shape, seed, fill=-1.0, share=0.7):
    """`share` of the voxels at one value (the air of a CT scan) in long runs, the rest smooth"""
    rng = np.random.default_rng(seed)
    v = smooth_volume(shape, seed + 1).ravel()
    n = v.size
    start = int(rng.integers(0, max(n - int(share * n), 1)))
    v[start:start + int(share * n)] = fill
    return v.reshape(shape)


def edge_probe(lo, hi, bins):
    """every edge cast to fp32 with its two fp32 neighbours: the values at which a binning rule can go wrong"""
    e32 = ref_edges(lo, hi, bins).astype(np.float32)
    return np.unique(np.concatenate([e32, np.nextafter(e32, np.float32(-np.inf)), np.nextafter(e32, np.float32(np.inf))]))
