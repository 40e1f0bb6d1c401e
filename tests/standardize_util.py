"""The oracle of the percentile and intensity-standardisation tests (numpy only): the two rules of DESIGN 3.18 spelt out on the host.

ref_quantile   select, sort, then h = (n - 1) p / 100, k = floor(h), t = h - k and numpy's _lerp in Python floats (IEEE fp64, one rounding per operation);
               tests/test_host_standardize.py pins it to np.percentile with ==.
ref_map        the piecewise-linear map through landmarks in numpy fp64 (numpy rounds every operation on its own).
ref_fit        the Nyul-Udupa standard scale: each case's landmarks mapped affinely onto the target's ends, averaged in list order.
key / unkey / radix_select
               a plain-integer restatement of what the kernel does: the order-preserving integer image of the fp32 bits and four 8-bit passes that
               narrow a rank down to one key.
volume         the test volumes."""
import math

import numpy as np

KINDS = ("ct", "ties", "fine", "wide", "constant", "nonfinite")


def volume(shape, kind, seed=0, air=True):
    """float32 test volumes.  ct: round(N(40, 250)) with (air) a contiguous block of -1024 over the first 40 % of the voxels; ties: integers -5..5; fine:
    1 + i 2^-23, i < 200 (the values differ in the lowest byte only); wide: +-2^e, e in [-140, 127) (both signs, every byte, subnormals); constant: 7.25;
    nonfinite: ct with about 1 % of the voxels NaN, +inf or -inf."""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    rng = np.random.RandomState(seed + 1000 * KINDS.index(kind))
    if kind in ("ct", "nonfinite"):
        x = np.round(rng.randn(n) * 250.0 + 40.0)
        if air:
            x[:int(0.4 * n)] = -1024.0
        if kind == "nonfinite":
            bad = rng.rand(n) < 0.01
            x[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    elif kind == "ties":
        x = rng.randint(-5, 6, size=n).astype(np.float64)
    elif kind == "fine":
        x = 1.0 + rng.randint(0, 200, size=n) * 2.0 ** -23
    elif kind == "wide":
        x = np.ldexp(1.0, rng.randint(-140, 127, size=n)) * rng.choice([-1.0, 1.0], size=n)
    elif kind == "constant":
        x = np.full(n, 7.25)
    else:
        raise ValueError(kind)
    return x.astype(np.float32).reshape(shape)


def select(x, above=None, mask=None):
    """-> (the selected values of one plane, float32, in storage order; the number of non-finite voxels)"""
    x = np.asarray(x, np.float32).ravel()
    fin = np.isfinite(x)
    sel = fin.copy()
    if above is not None:
        with np.errstate(invalid="ignore"):
            sel &= x > np.float32(above)
    if mask is not None:
        sel &= np.asarray(mask).ravel() != 0
    return x[sel], int((~fin).sum())


def ranks(n, p):
    """-> (k, k1, t) of percentile p among n >= 1 values"""
    p01 = float(p) / 100.0
    h = float(n - 1) * p01
    k = int(math.floor(h))
    return k, min(k + 1, n - 1), h - float(k)


def lerp(a, b, t):
    d = b - a
    if t >= 0.5:
        u = 1.0 - t
        m = d * u
        return b - m
    m = d * t
    return a + m


def ref_quantile(x, ps, above=None, mask=None):
    """one plane -> {"q": fp64 (Q,), "lo", "hi": float32 (Q,), "count", "rejected": int}"""
    v, rejected = select(x, above, mask)
    v = np.sort(v)
    n = int(v.size)
    q, lo, hi = [], [], []
    for p in ps:
        if n == 0:
            q.append(float("nan")); lo.append(np.float32("nan")); hi.append(np.float32("nan"))
            continue
        k, k1, t = ranks(n, p)
        q.append(lerp(float(v[k]), float(v[k1]), t))
        lo.append(v[k]); hi.append(v[k1])
    return {"q": np.array(q, np.float64), "lo": np.array(lo, np.float32), "hi": np.array(hi, np.float32), "count": n, "rejected": rejected}


def ref_map(x, src, dst, extrapolate="linear"):
    """one plane x float32, src and dst fp64 (L,) -> float32"""
    x = np.asarray(x, np.float32)
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    if np.isnan(src).any():
        return x.copy()
    x64 = x.astype(np.float64)
    j = np.zeros(x.shape, np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(1, len(src) - 1):
            j[src[i] <= x64] = i
    w = src[1:] - src[:-1]
    slope = np.where(w > 0, (dst[1:] - dst[:-1]) / np.where(w > 0, w, 1.0), 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        m = (x64 - src[j]) * slope[j]
        y = dst[j] + m
        if extrapolate == "clamp":
            y = np.minimum(np.maximum(y, dst[0]), dst[-1])
        out = y.astype(np.float32)
    keep = ~np.isfinite(x)
    out[keep] = x[keep]
    return out


def ref_fit(volumes, percentiles, target, above=None, masks=None):
    """the standard scale, fp64 (L,)"""
    masks = [None] * len(volumes) if masks is None else masks
    total = np.zeros(len(percentiles), np.float64)
    for x, m in zip(volumes, masks):
        s = ref_quantile(x, percentiles, above, m)["q"]
        total = total + (target[0] + (s - s[0]) * ((target[1] - target[0]) / (s[-1] - s[0])))
    return total / len(volumes)


# ---- the kernel's selection in plain integers ----------------------------------------------------------------------------------------------
def key(x):
    """float32 values -> the unsigned integers (held in int64) whose order is the values' order"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def unkey(e):
    e = int(e)
    u = (e ^ 0x80000000) if e & 0x80000000 else (~e & 0xFFFFFFFF)
    return np.array([u], np.uint32).view(np.float32)[0]


def radix_select(keys, rank):
    """the key of rank `rank` (0-based, ascending) among `keys`: four passes of 8 bits, counting only the keys under the prefix chosen so far"""
    prefix, r = 0, int(rank)
    for p in range(4):
        shift = 24 - 8 * p
        under = keys if p == 0 else keys[(keys >> (shift + 8)) == (prefix >> (shift + 8))]
        counts = np.bincount((under >> shift) & 255, minlength=256)
        digit, below = 0, 0
        while below + int(counts[digit]) <= r:
            below += int(counts[digit])
            digit += 1
        prefix |= digit << shift
        r -= below
    return prefix
