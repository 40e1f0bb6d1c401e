"""The oracle of the simulated-low-resolution stage (csrc/lowres.hip): scipy.ndimage.zoom with edge boundaries, by definition; the
composite with its clips; the target-shape rule; and a separable fp64 restatement of the order-3 zoom — one axis at a time, as the kernels work — which
tests/test_host_lowres.py pins against scipy's three-dimensional evaluation."""
import numpy as np
from scipy import ndimage as ndi

PAD = 12                                    # scipy's _prepad_for_spline_filter for mode="nearest"
POLE = np.sqrt(3.0) - 2.0
KINDS = ("offset", "unit", "constant")


def volume(shape, kind, seed=0):
    rng = np.random.RandomState(seed + 7 * int(np.prod(shape)))
    if kind == "offset":
        return (rng.randn(*shape) * 10 + 100).astype(np.float32)
    if kind == "unit":
        return (rng.rand(*shape) * 2 - 1).astype(np.float32)
    return np.full(shape, 7.25, np.float32)


def coord(o, m, n):
    """input coordinate of output index o on an axis of input length m and output length n: the zoom is ONE fp64 division"""
    zoom = np.float64(m) / np.float64(n)
    return (np.asarray(o, np.float64) + 0.5) * zoom - 0.5


def pick0(m, n):
    """the order-0 picks of every output index"""
    return np.floor(coord(np.arange(n), m, n) + 0.5).astype(np.int64)


def ref_zoom_edge64(x, out_shape, order):
    """the definition, before the clip and the rounding: fp64"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3
    z = [o / i for o, i in zip(out_shape, x.shape)]
    y = ndi.zoom(x.astype(np.float64), z, order=order, mode="nearest", grid_mode=True)
    assert y.shape == tuple(out_shape), (y.shape, out_shape)
    return y


def ref_zoom_edge(x, out_shape, order=3, clip=True):
    y = ref_zoom_edge64(x, out_shape, order)
    if clip:
        y = np.clip(y, np.float64(x.min()), np.float64(x.max()))
    return y.astype(np.float32)


def ref_simulate_lowres(x, target_shape, order_down=0, order_up=3):
    t = ref_zoom_edge(x, target_shape, order_down, clip=order_down > 0)
    return ref_zoom_edge(t, x.shape, order_up, clip=order_up > 0)


def ref_target_shape(shape, zoom, ignore_axes=()):
    out = []
    for axis, s in enumerate(shape):
        n = int(s) if axis in tuple(ignore_axes) else int(np.round(np.float64(s) * np.float64(zoom)))
        if n < 1:
            raise ValueError("lowres target: axis %d of length %d vanishes at zoom %r" % (axis, s, zoom))
        out.append(n)
    return tuple(out)


# ---- the separable restatement ---------------------------------------------------------------------------------------------------------------------
def _prefilter_line(c):
    """scipy's order-3 recursion with the mirror start, in place on the last axis (fp64): gain 6, causal from the full-line sum, anticausal"""
    n = c.shape[-1]
    z = POLE
    c *= 6.0
    zn1 = z ** (n - 1)
    s = c[..., 0] + zn1 * c[..., n - 1]
    zi = z
    for i in range(1, n - 1):
        s = s + zi * (c[..., i] + zn1 * c[..., n - 1 - i])
        zi *= z
    c[..., 0] = s / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[..., i] += z * c[..., i - 1]
    c[..., n - 1] = (z * c[..., n - 2] + c[..., n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[..., i] = z * (c[..., i + 1] - c[..., i])
    return c


def _zoom3_last_axis(a, n):
    m = a.shape[-1]
    c = _prefilter_line(np.pad(a, [(0, 0)] * (a.ndim - 1) + [(PAD, PAD)], mode="edge"))
    cc = coord(np.arange(n), m, n) + PAD
    f = np.floor(cc)
    t, start = cc - f, f.astype(np.int64) - 1
    u = 1.0 - t
    w = np.empty((4, n))
    w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    w[0] = u * u * u / 6.0
    w[3] = 1.0 - w[0] - w[1] - w[2]
    out = np.zeros(a.shape[:-1] + (n,))
    for k in range(4):
        out = out + w[k] * c[..., start + k]
    return out


def sep_zoom_edge64(x, out_shape):
    """order 3, one axis at a time — z, then y, then x — each: pad the line by 12 edge values, prefilter, evaluate; fp64 throughout"""
    a = np.asarray(x).astype(np.float64)
    for axis in range(3):
        a = np.moveaxis(_zoom3_last_axis(np.ascontiguousarray(np.moveaxis(a, axis, -1)), int(out_shape[axis])), -1, axis)
    return np.ascontiguousarray(a)


def sep_zoom_edge(x, out_shape, clip=True):
    y = sep_zoom_edge64(x, out_shape)
    if clip:
        y = np.clip(y, np.float64(np.min(x)), np.float64(np.max(x)))
    return y.astype(np.float32)


# ---- the transform's draws -------------------------------------------------------------------------------------------------------------------------
def ref_draw(rng, channels, shape, noise="numpy", seed=0, n_noised=0, p_lowres=0.0, p_lowres_per_channel=0.5, lowres_zoom=(0.5, 1.0), lowres_orders=(0, 3),
             lowres_ignore_axes=(), **kw):
    """IntensityAugment.draw's ops list from `rng` with the low-resolution stage: tests/augment_util.py's order, and after contrast — only when
    p_lowres > 0 — one uniform for the gate, then per channel a uniform < p_lowres_per_channel and, for a channel taken, its zoom in U(lowres_zoom)."""
    from tests import augment_util as AU
    p = dict(AU.DEFAULTS, **kw)
    ops_list = []
    if rng.uniform() < p["p_noise"]:
        s = rng.uniform(*p["noise_s"])
        spec = np.stack([rng.normal(0.0, 1.0, tuple(shape)) for _ in range(channels)]) if noise == "numpy" else (seed, n_noised)
        ops_list.append(("noise", s, spec))
    if rng.uniform() < p["p_blur"]:
        ops_list.append(("blur", [rng.uniform(*p["blur_sigma"]) if rng.uniform() <= p["p_blur_per_channel"] else None for _ in range(channels)]))
    if rng.uniform() < p["p_brightness"]:
        ops_list.append(("brightness", [rng.uniform(*p["brightness"]) for _ in range(channels)]))
    if rng.uniform() < p["p_contrast"]:
        ops_list.append(("contrast", [AU._range_val(rng, *p["contrast"]) for _ in range(channels)], p["preserve_range"]))
    if p_lowres > 0 and rng.uniform() < p_lowres:
        ops_list.append(("lowres", [rng.uniform(*lowres_zoom) if rng.uniform() < p_lowres_per_channel else None for _ in range(channels)],
                         lowres_orders[0], lowres_orders[1], tuple(lowres_ignore_axes)))
    if rng.uniform() < p["p_gamma_inverted"]:
        ops_list.append(("gamma", [AU._range_val(rng, *p["gamma"]) for _ in range(channels)], True, p["retain_stats"]))
    if rng.uniform() < p["p_gamma"]:
        ops_list.append(("gamma", [AU._range_val(rng, *p["gamma"]) for _ in range(channels)], False, p["retain_stats"]))
    mask = sum(bit for bit in (4, 2, 1) if rng.uniform() < p["p_mirror"])
    if mask:
        ops_list.append(("flip", mask))
    return ops_list


def ref_chain(x, ops_list):
    """(C, D, H, W) float32 through the ops in order: tests/augment_util.py's chain, with ("lowres", zoom, order_down, order_up, ignore_axes)"""
    from tests import augment_util as AU
    cur = np.asarray(x, np.float32)
    for op in ops_list:
        if op[0] != "lowres":
            cur = AU.ref_chain(cur, [op])
            continue
        zooms = op[1] if isinstance(op[1], (list, tuple)) else [op[1]] * cur.shape[0]
        order_down, order_up = (op[2] if len(op) > 2 else 0), (op[3] if len(op) > 3 else 3)
        ignore = op[4] if len(op) > 4 else ()
        cur = np.stack([cur[c] if z is None else ref_simulate_lowres(cur[c], ref_target_shape(cur.shape[1:], z, ignore), order_down, order_up)
                        for c, z in enumerate(zooms)])
    return cur
