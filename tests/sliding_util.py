"""A numpy restatement of the sliding-window prediction (include/vaeseg.h "sliding-window prediction", ops.sw_*, evaluation.sliding_window_predict):
the yardstick of tests/test_host_sliding.py and tests/test_gpu_sliding.py.  The reference has no counterpart.

    plan      per axis step = max(1, floor(P (1 - overlap))), n = 1 if S <= P else ceil((S - P) / step) + 1, origin i = min(i step, max(S - P, 0));
              windows D-major, then H, then W
    weights   "constant": ones; "gaussian": exp(-((i - (P - 1) / 2) / sigma)^2 / 2), sigma = P / 8, in float64, floored at 1e-3, rounded to fp32
    blend     a voxel's weight is the fp32 product (wz * wy) * wx of the fp32 tables, rounded after each product; windows are visited in plan order;
              acc += w * p and the normalisation are formed in float64.  wsum is ALSO restated in the device's own arithmetic — fp32 additions in plan
              order, which IEEE defines exactly — so that the device's weight sum can be compared bit for bit.
"""
import math

import numpy as np


def axis_origins(s, p, overlap):
    step = max(1, int(math.floor(p * (1.0 - overlap))))
    n = 1 if s <= p else -(-(s - p) // step) + 1
    return [min(i * step, max(s - p, 0)) for i in range(n)]


def plan(shape, patch, overlap):
    """-> int32 (nw, 3) origins"""
    oz, oy, ox = (axis_origins(int(s), int(patch), overlap) for s in shape)
    return np.array([(z, y, x) for z in oz for y in oy for x in ox], dtype=np.int32).reshape(-1, 3)


def weights(patch, blend):
    """-> fp32 (3, P)"""
    p = int(patch)
    if blend == "constant":
        row = np.ones(p, np.float64)
    elif blend == "gaussian":
        i = np.arange(p, dtype=np.float64)
        row = np.maximum(np.exp(-0.5 * ((i - (p - 1) / 2.0) / (p / 8.0)) ** 2), 1e-3)
    else:
        raise ValueError(blend)
    return np.stack([row, row, row]).astype(np.float32)


def window_weight(wt):
    """fp32 (P, P, P): (wz * wy) * wx, every product rounded to fp32"""
    wzy = (wt[0][:, None] * wt[1][None, :]).astype(np.float32)
    return (wzy[:, :, None] * wt[2][None, None, :]).astype(np.float32)


def gather(volume, origin, patch, cval=0.0):
    """volume (C, D, H, W) -> the (C, P, P, P) window at `origin`, cval past the volume"""
    c = volume.shape[0]
    out = np.full((c, patch, patch, patch), cval, dtype=volume.dtype)
    oz, oy, ox = (int(v) for v in origin)
    src = volume[:, oz:oz + patch, oy:oy + patch, ox:ox + patch]
    out[:, :src.shape[1], :src.shape[2], :src.shape[3]] = src
    return out


def blend(window_probs, origins, shape, wt):
    """window_probs: per window of the plan, in plan order, its (K, P, P, P) probabilities -> (prob float64 (K, D, H, W), wsum32 fp32 (D, H, W), the
    device's arithmetic, acc float64, wsum float64)"""
    d, h, w = shape
    w3 = window_weight(wt)
    acc = wsum = wsum32 = None
    for p, (oz, oy, ox) in zip(window_probs, np.asarray(origins).tolist()):
        p = np.asarray(p, dtype=np.float64)
        if acc is None:
            acc = np.zeros((p.shape[0], d, h, w), np.float64)
            wsum = np.zeros((d, h, w), np.float64)
            wsum32 = np.zeros((d, h, w), np.float32)
        nz, ny, nx = min(p.shape[1], d - oz), min(p.shape[2], h - oy), min(p.shape[3], w - ox)
        sl = (slice(oz, oz + nz), slice(oy, oy + ny), slice(ox, ox + nx))
        wv = w3[:nz, :ny, :nx]
        acc[(slice(None),) + sl] += wv.astype(np.float64)[None] * p[:, :nz, :ny, :nx]
        wsum[sl] += wv.astype(np.float64)
        wsum32[sl] = wsum32[sl] + wv                              # fp32 + fp32 -> fp32, one rounding per window, in plan order
    return acc / wsum[None], wsum32, acc, wsum


def predict(model_fn, volume, patch, overlap=0.5, blend_mode="gaussian", cval=0.0):
    """The whole algorithm with a numpy model_fn ((1, C, P, P, P) -> (1, K, P, P, P)), one window at a time.
    -> {"prob" float64 (K, D, H, W), "wsum32" fp32, "origins" int32 (nw, 3)}"""
    vol = np.asarray(volume)
    if vol.ndim == 3:
        vol = vol[None]
    shape = vol.shape[1:]
    origins = plan(shape, patch, overlap)
    wt = weights(patch, blend_mode)
    probs = [np.asarray(model_fn(gather(vol, o, patch, cval)[None]))[0] for o in origins]
    prob, wsum32, _, _ = blend(probs, origins, shape, wt)
    return {"prob": prob, "wsum32": wsum32, "origins": origins}


def first_argmax(prob):
    """argmax over axis 0, ties to the first maximal channel -> uint8"""
    return np.argmax(prob, axis=0).astype(np.uint8)
