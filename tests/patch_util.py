"""The oracle of the patch-training tests (numpy only, no torch): the integer rule of DESIGN 3.19 spelt out on the host.  tests/test_host_patch.py pins it.

bounds         per axis, volume side S and patch side P: need = max(P - S, 0), lb = -(need // 2), ub = S + need // 2 + need % 2 - P
scale          a 32-bit word onto a range of m values: (w * m) >> 32 in Python integers
class_mask     the voxels of class k: the value is the integer k (NaN, fractions and values outside [0, n_class) belong to no class)
ref_index      the table of ops.patch_index: exclusive prefix counts per class over chunks of `chunk` voxels of the linear index, then the totals
members        the ascending linear indices of every class of a list that is present: np.flatnonzero(label.ravel() == k)
ref_pick       one request -> the eight integers of ops.patch_pick (ref_picks: all requests of a call)
forced_flags   which samples of a batch are forced: j >= floor(B (1 - p) + 0.5)
ref_gather     numpy pad-and-slice: the block of a request with a margin, cval outside the volume
label_volume   the test labels"""
import math

import numpy as np


def bounds(s, p):
    need = max(int(p) - int(s), 0)
    return -(need // 2), int(s) + need // 2 + need % 2 - int(p)


def scale(word, m):
    word, m = int(word), int(m)
    assert 0 <= word < 2 ** 32 and m >= 1
    return (word * m) >> 32


def class_mask(label, k, n_class):
    label = np.asarray(label)
    if not 0 <= int(k) < int(n_class):
        return np.zeros(label.shape, bool)
    with np.errstate(invalid="ignore"):
        return label == k


def ref_index(label, n_class, chunk):
    flat = np.asarray(label).ravel()
    n_chunks = (flat.size + chunk - 1) // chunk
    table = np.zeros((n_chunks + 1, n_class), np.int64)
    for k in range(n_class):
        m = class_mask(flat, k, n_class)
        counts = np.add.reduceat(m.astype(np.int64), np.arange(0, flat.size, chunk))
        table[1:, k] = np.cumsum(counts)
    return table.astype(np.int32)


def clamp_origin(v, s, p):
    lb, ub = bounds(s, p)
    return min(max(lb, int(v) - int(p) // 2), ub)


def free_origin(word, s, p):
    lb, ub = bounds(s, p)
    return lb + scale(word, ub - lb + 1)


def members(label, n_class, classes):
    """{k: np.flatnonzero(label.ravel() == k)} for the classes of the list that are present, in ascending order of k"""
    flat = np.asarray(label).ravel()
    found = {k: np.flatnonzero(class_mask(flat, k, n_class)) for k in sorted(int(c) for c in classes)}
    return {k: where for k, where in found.items() if where.size}


def _pick(shape, where, words, forced, patch):
    present = list(where)
    if forced and present:
        k = present[scale(words[0], len(present))]
        v = int(where[k][scale(words[1], where[k].size)])
        vox = [v // (shape[1] * shape[2]), v // shape[2] % shape[1], v % shape[2]]
        return [clamp_origin(vox[a], shape[a], patch[a]) for a in range(3)] + [k] + vox + [0]
    return [free_origin(words[2 + a], shape[a], patch[a]) for a in range(3)] + [-1, -1, -1, -1, 0]


def ref_pick(label, n_class, classes, words, forced, patch):
    """one request -> [oz, oy, ox, class or -1, vz, vy, vx or -1, 0]"""
    return _pick(np.asarray(label).shape, members(label, n_class, classes), words, forced, patch)


def ref_picks(label, n_class, classes, words, forced, patch):
    """ref_pick for every request of a call (the label is searched once)"""
    where = members(label, n_class, classes)
    return np.array([_pick(np.asarray(label).shape, where, w, f, patch) for w, f in zip(words, forced)], np.int32).reshape(-1, 8)


def n_free(batch_size, p):
    """the samples of a batch before the first forced one"""
    return int(math.floor(batch_size * (1.0 - p) + 0.5))


def forced_flags(batch_size, p):
    return [j >= n_free(batch_size, p) for j in range(batch_size)]


def ref_gather(vol, origin, patch, margin=0, cval=0.0):
    """rows [o - margin, o - margin + P + 2 margin) of every axis; positions outside the volume hold cval"""
    vol = np.asarray(vol)
    q = [int(p) + 2 * int(margin) for p in patch]
    lo = [int(o) - int(margin) for o in origin]
    before = [max(0, -lo[a]) for a in range(3)]                        # per axis: only as far as this block reaches
    after = [max(0, lo[a] + q[a] - vol.shape[a]) for a in range(3)]
    padded = np.pad(vol, list(zip(before, after)), mode="constant", constant_values=cval)
    return padded[tuple(slice(lo[a] + before[a], lo[a] + before[a] + q[a]) for a in range(3))].copy()


def label_volume(shape, kind, n_class=3, seed=0, dtype=np.float32, chunk=4096):
    """random: classes 0..n_class-1, mostly background; background: zeros; one: class 1 everywhere; first / last: class 1 only at the first / the last
    linear voxel; tail: class 1 only in the last, partial chunk (the last voxel when the volume is whole chunks); odd (float only): random with NaN, 0.5
    and n_class sprinkled in; sparse64: class 2 on exactly 64 voxels spread evenly over the volume, background elsewhere"""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    rng = np.random.RandomState(seed + 17 * len(kind))
    x = np.zeros(n, np.float64)
    if kind in ("random", "odd"):
        x = rng.choice(n_class, size=n, p=[0.7] + [0.3 / (n_class - 1)] * (n_class - 1)).astype(np.float64)
        if kind == "odd":
            bad = rng.rand(n) < 0.2
            x[bad] = rng.choice([np.nan, 0.5, float(n_class), -1.0, 1.5], size=int(bad.sum()))
    elif kind == "one":
        x[:] = 1
    elif kind == "first":
        x[0] = 1
    elif kind == "last":
        x[-1] = 1
    elif kind == "tail":
        start = (n - 1) // chunk * chunk
        x[start + (n - start) // 2:] = 1
    elif kind == "sparse64":
        x[np.linspace(0, n - 1, 64).astype(np.int64)] = 2
    elif kind != "background":
        raise ValueError(kind)
    return x.astype(dtype).reshape(shape)
