"""The restatement the morphology tests compare against: scipy.ndimage per plane, plus the mask generators both test files use."""
import numpy as np
from scipy import ndimage

STRUCT = {6: ndimage.generate_binary_structure(3, 1), 26: np.ones((3, 3, 3), dtype=bool)}
SCIPY_OPS = {"dilate": ndimage.binary_dilation, "erode": ndimage.binary_erosion, "open": ndimage.binary_opening, "close": ndimage.binary_closing}


def _per_plane(x, fn):
    x = np.asarray(x)
    fg = x >= 0.5 if x.dtype != bool else x
    if fg.ndim == 3:
        return fn(fg).astype(np.float32)
    out = np.empty(fg.shape, np.float32)
    for n in range(fg.shape[0]):
        for c in range(fg.shape[1]):
            out[n, c] = fn(fg[n, c])
    return out


def ref_morph(x, op, connectivity=6, iterations=1, border_value=0):
    """scipy's operator on every (n, c) plane of a (N, C, D, H, W) array (or on one (D, H, W) volume) -> float32 0 / 1"""
    return _per_plane(x, lambda m: SCIPY_OPS[op](m, structure=STRUCT[connectivity], iterations=iterations, border_value=border_value))


def ref_fill_holes(x, connectivity=6):
    return _per_plane(x, lambda m: ndimage.binary_fill_holes(m, structure=STRUCT[connectivity]))


def ref_synthesis_mask(hu):
    """utils/utils.py:647-655 on one numpy volume"""
    bone = ndimage.binary_dilation(hu > 200, iterations=2)
    bowel = np.zeros(hu.shape)
    bowel[hu < 0] = 1
    return ((1 - bowel) * (1 - bone)).astype(np.float32)


def ref_postprocess(hot, closing=0, fill_holes=False, lo=1):
    """evaluation.postprocess without the component filter on a one-hot (N, C, D, H, W) numpy array: classes in ascending order, gains only from the
    background of the moment, losses to the background"""
    x = (np.asarray(hot) >= 0.5).copy()
    for n in range(x.shape[0]):
        for c in range(lo, x.shape[1]):
            cur = x[n, c].copy()
            new = cur
            if closing > 0:
                new = ndimage.binary_closing(new, structure=STRUCT[26], iterations=closing, border_value=0)
            if fill_holes:
                new = ndimage.binary_fill_holes(new, structure=STRUCT[6])
            gain = new & ~cur & x[n, 0]
            lose = cur & ~new
            x[n, c] = (cur | gain) & ~lose
            x[n, 0] = (x[n, 0] & ~gain) | lose
    return x.astype(np.float32)


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def random_mask(shape, density, seed):
    return np.random.RandomState(seed).rand(*shape) >= 1.0 - density


def corner_voxel(shape):
    m = np.zeros(shape, bool)
    m[(0,) * len(shape)] = True
    return m


def flush_block(shape):
    """a block that touches the low face of every axis"""
    m = np.zeros(shape, bool)
    d, h, w = shape[-3:]
    m[..., :max(1, d // 2), :max(1, h // 2), :max(1, (2 * w) // 3)] = True
    return m


def shell(drop=None, side=9, outer=5):
    """a hollow cube of side `outer` (walls one voxel thick) centred in a side^3 volume; drop: None, "corner" (one corner voxel of the wall is
    removed) or "face" (the centre voxel of one face)"""
    m = np.zeros((side,) * 3, bool)
    a = (side - outer) // 2
    b = a + outer
    m[a:b, a:b, a:b] = True
    m[a + 1:b - 1, a + 1:b - 1, a + 1:b - 1] = False
    if drop == "corner":
        m[a, a, a] = False
    elif drop == "face":
        m[a, (a + b) // 2, (a + b) // 2] = False
    elif drop is not None:
        raise ValueError(drop)
    return m


def open_hole(shape):
    """a block with a cavity that a one-voxel tunnel connects to the x = 0 face of the volume: not a hole"""
    d, h, w = shape
    m = np.zeros(shape, bool)
    m[1:d - 1, 1:h - 1, 0:w - 1] = True
    m[d // 2 - 1:d // 2 + 2, h // 2 - 1:h // 2 + 2, 4:w - 4] = False
    m[d // 2, h // 2, 0:4] = False
    return m


def nested_shells(shape):
    d, h, w = shape
    m = np.zeros(shape, bool)
    m[1:d - 1, 1:h - 1, 1:w - 1] = True
    m[2:d - 2, 2:h - 2, 2:w - 2] = False
    m[4:d - 4, 4:h - 4, 4:w - 4] = True
    m[5:d - 5, 5:h - 5, 5:w - 5] = False
    return m


def _serpentine_path(shape):
    """a one-voxel-wide path through every second row of every second slab, joined at alternating ends; it starts at (0, 0, 0)"""
    d, h, w = shape
    m = np.zeros(shape, bool)
    for zi, z in enumerate(range(0, d, 2)):
        ys = list(range(0, h, 2))
        if zi % 2:
            ys = ys[::-1]
        side = 0
        for i, y in enumerate(ys):
            m[z, y, :] = True
            if i + 1 < len(ys):
                m[z, (y + ys[i + 1]) // 2, w - 1 if side == 0 else 0] = True
                side ^= 1
        if z + 2 < d:
            m[z + 1, ys[-1], w - 1 if side == 0 else 0] = True
    return m


def serpentine_background(shape, open_end=True):
    """foreground everywhere but a serpentine corridor one voxel inside the volume; with open_end the corridor's first voxel is joined to the z = 0
    face, so the whole corridor is outside (nothing to fill) — but only by walking its full length; without, the corridor is one long hole"""
    d, h, w = shape
    m = np.ones(shape, bool)
    m[1:d - 1, 1:h - 1, 1:w - 1] = ~_serpentine_path((d - 2, h - 2, w - 2))
    if open_end:
        m[0, 1, 1] = False
    return m
