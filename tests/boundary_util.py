"""The signed distance maps and the boundary loss of csrc/sdm.hip restated in fp64 numpy: the rule and nothing else.  No project code is used
here; tests/test_host_boundary.py pins these functions against a brute-force nearest-voxel search and Kervadec's own expression before a kernel is compared
with them.

The rule: the class of a voxel is trunc(label) where 0 <= label < n_class (compared in fp32; NaN is not), none otherwise.  P_c = the voxels of class c, every
other voxel — the classless ones included — is outside it.  With scipy's distance_transform_edt(mask, sampling) = the distance of every nonzero voxel to the
nearest zero voxel:
  phi_c = edt(~P_c) outside P_c  and  -(edt(P_c) - 1) inside;   a plane where P_c is empty or the whole volume is 0 (scipy measures to a phantom there).
  L_B = 1 / (B K) sum_b 1 / N_b sum_{c in [bot, top)} sum_{v valid} p_c(v) phi_c(v),  N_b = the valid voxels of sample b, a sample with N_b = 0 adds 0;
  d (w L_B) / d p_c(v) = w phi_c(v) / (B K N_b) at a valid voxel of a channel of [bot, top), 0 elsewhere."""
import numpy as np


def classify(label, n_class):
    """fp32-comparable labels of any shape -> (valid bool, class int64, -1 where there is none)"""
    l32 = np.asarray(label, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        valid = (l32 >= 0) & (l32 < np.float32(n_class))
    cls = np.where(valid, np.trunc(np.where(valid, l32, 0)), -1).astype(np.int64)
    return valid, cls


def signed_distance(label, n_class, bot=0, top=None, spacing=None):
    """label (D, H, W) -> fp64 (top - bot, D, H, W)"""
    from scipy.ndimage import distance_transform_edt as edt
    top = n_class if top is None else top
    _, cls = classify(label, n_class)
    out = np.zeros((top - bot,) + cls.shape, dtype=np.float64)
    for j, c in enumerate(range(bot, top)):
        pos = cls == c
        if not pos.any() or pos.all():
            continue                                   # stays 0: defined here, not taken from scipy
        outside = edt(~pos, sampling=spacing)          # nonzero outside P_c: the distance to P_c
        inside = edt(pos, sampling=spacing)
        out[j] = np.where(pos, -(inside - 1.0), outside)
    return out


def signed_distance_batch(label, n_class, bot=0, top=None, spacing=None):
    """label (B, 1, D, H, W) -> fp64 (B, top - bot, D, H, W)"""
    return np.stack([signed_distance(l[0], n_class, bot, top, spacing) for l in np.asarray(label)])


def brute_force(label, n_class, bot=0, top=None):
    """the same at unit spacing by a search over all pairs of voxels: exact integer squares, one fp64 square root; small volumes only"""
    top = n_class if top is None else top
    _, cls = classify(label, n_class)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in cls.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    sq = ((grid[:, None, :] - grid[None, :, :]) ** 2).sum(-1)          # (V, V) int64
    flat = cls.reshape(-1)
    out = np.zeros((top - bot, flat.size), dtype=np.float64)
    for j, c in enumerate(range(bot, top)):
        pos = flat == c
        if not pos.any() or pos.all():
            continue
        to_pos = np.sqrt(sq[:, pos].min(1).astype(np.float64))
        to_neg = np.sqrt(sq[:, ~pos].min(1).astype(np.float64))
        out[j] = np.where(pos, -(to_neg - 1.0), to_pos)
    return out.reshape((top - bot,) + cls.shape)


def boundary_loss(p, label, phi, bot, top, weight=1.0, gout=1.0):
    """p (B, C, ...), label (B, 1, ...), phi (B, top - bot, ...) -> (term, weighted, gradient of gout * weighted in p), fp64"""
    p = np.asarray(p, dtype=np.float64)
    b, c = p.shape[:2]
    k = top - bot
    p2 = p.reshape(b, c, -1)
    f2 = np.asarray(phi, dtype=np.float64).reshape(b, k, -1)
    valid, _ = classify(np.asarray(label).reshape(b, -1), c)
    grad = np.zeros_like(p2)
    term = 0.0
    for s in range(b):
        n = int(valid[s].sum())
        if n == 0:
            continue
        term += float((p2[s, bot:top] * f2[s])[:, valid[s]].sum()) / n
        grad[s, bot:top] = np.where(valid[s][None], f2[s], 0.0) * (float(gout) * float(weight) / (b * k * n))
    term /= b * k
    return term, float(weight) * term, grad.reshape(p.shape)


def relerr(a, b):
    """norm-wise relative error: max |a - b| / max |b|"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def blocky_labels(rng, b, n_class, shape, block=4):
    """(B, 1, D, H, W) fp32 labels 0..n_class-1 in blocks of `block` voxels: regions a few voxels across, so distances of several voxels occur"""
    coarse = rng.integers(0, n_class, size=(b, 1) + tuple((s + block - 1) // block for s in shape))
    lab = coarse
    for ax, s in enumerate(shape):
        lab = np.repeat(lab, block, axis=2 + ax).take(np.arange(s), axis=2 + ax)
    return lab.astype(np.float32)


def sprinkle(rng, lab, n_class):
    """every sort of classless value (-1, 255, NaN, n_class, -0.5) on about a tenth of the voxels, at least one of each where there is room, and
    fractional valid labels (x.5: the class is the truncation) on another tenth"""
    lab = lab.copy()
    r = rng.random(lab.shape)
    flat = lab.reshape(-1)
    for j, bad in enumerate((-1.0, 255.0, float("nan"), float(n_class), -0.5)):
        lab[(r >= 0.02 * j) & (r < 0.02 * (j + 1))] = bad
        if flat.size > 2 * j + 1:
            flat[2 * j + 1] = bad
    frac = (r >= 0.5) & (r < 0.6)
    lab[frac] = lab[frac] + 0.5
    return lab
