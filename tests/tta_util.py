"""A numpy restatement of mirror test-time augmentation inside the sliding-window prediction (include/vaeseg.h vs_sw_gather_tta /
vs_sw_accumulate_tta, ops.sw_gather / sw_accumulate with flips, evaluation.SlidingWindow(tta=...)), built on tests/sliding_util.py: the yardstick of
tests/test_host_tta.py and tests/test_gpu_tta.py.  The reference has no counterpart.

    flip      a 3-bit code: bit 0 mirrors W (x), bit 1 mirrors H (y), bit 2 mirrors D (z)
    items     item j is window j // nf of the plan under flip flips[j % nf]; items are visited in ascending j
    gather    the whole padded (C, P, P, P) window of sliding_util.gather, np.flip'ed over the code's axes (cval lands at the low end)
    blend     the network's answer is np.flip'ed back and enters sliding_util.blend as one more window at the same origin: the weight is taken at the
              un-mirrored position, acc and the normalisation in float64, wsum32 as fp32 additions in item order
"""
import numpy as np

from tests import sliding_util as SW

AXES = {"w": 1, "h": 2, "d": 4}


def flips_of(axes):
    """evaluation.tta_flips for a string over "dhw": every subset of the named axes, ascending"""
    mask = sum(AXES[a] for a in axes)
    return tuple(c for c in range(8) if c & ~mask == 0)


def flip_axes(code, ndim):
    """the numpy axes of an array whose last three dimensions are (z, y, x) that `code` mirrors"""
    return tuple(ndim - 1 - bit for bit in range(3) if code >> bit & 1)


def mirror(a, code):
    a = np.asarray(a)
    return np.flip(a, flip_axes(code, a.ndim)) if code else a


def gather(volume, origin, patch, cval, code):
    """the window of item (origin, code) as the network sees it"""
    return np.ascontiguousarray(mirror(SW.gather(volume, origin, patch, cval), code))


def predict(model_fn, volume, patch, overlap=0.5, blend="gaussian", cval=0.0, flips=(0,)):
    """-> {"prob" float64 (K, D, H, W), "wsum32" fp32 (D, H, W), "origins" int32 (nw, 3), "terms": the largest number of terms a voxel sums —
    covering windows x nf}"""
    vol = np.asarray(volume)
    if vol.ndim == 3:
        vol = vol[None]
    shape = vol.shape[1:]
    origins = SW.plan(shape, patch, overlap)
    wt = SW.weights(patch, blend)
    probs, item_origins = [], []
    for o in origins:
        for code in flips:
            answer = np.asarray(model_fn(gather(vol, o, patch, cval, code)[None]))[0]
            probs.append(mirror(answer, code))
            item_origins.append(o)
    prob, wsum32, _, _ = SW.blend(probs, np.array(item_origins, dtype=np.int32).reshape(-1, 3), shape, wt)
    cover = np.zeros(shape, np.int64)
    for oz, oy, ox in origins.tolist():
        cover[oz:oz + patch, oy:oy + patch, ox:ox + patch] += 1
    return {"prob": prob, "wsum32": wsum32, "origins": origins, "terms": int(cover.max()) * len(flips)}
