"""Reference goldens of the connected-component labelling -> tests/golden/cc.npz.

The reference's own flood fill (utils/utils.py:20-57, Tag / check_connection), unmodified and imported by path, numbers the components of
about ten small masks: ``check_connection(np.argwhere(mask), mask)`` returns one label per foreground voxel, in raster order.  The
third-party modules utils/utils.py imports at its top and this machine may lack (SimpleITK, skimage, batchgenerators, imageio, ...) are
stubbed in sys.modules — none of them is touched by the two functions used; a plain class stands in for every name imported from a stub
(SpatialTransform is subclassed at import time).

What is committed is data only: per mask its shape, its bits (np.packbits of the raveled mask) and the reference's labels as int16.

    python tools/make_golden_cc.py
"""
import importlib
import importlib.util
import os
import sys
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "cc.npz")

STUBBED = ("SimpleITK", "skimage", "skimage.transform", "skimage.measure", "imageio", "batchgenerators", "batchgenerators.transforms",
           "batchgenerators.transforms.spatial_transforms", "scipy.ndimage.morphology")


class _Stub(types.ModuleType):
    """a module every attribute of which is a plain class"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (), {})
        setattr(self, name, cls)
        return cls


def load_reference_utils():
    for name in STUBBED:
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Stub(name)
    spec = importlib.util.spec_from_file_location("_reference_utils", os.path.join(REF, "utils", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.realpath(mod.__file__).startswith(REF + os.sep)
    return mod


def smooth_noise(shape, seed, passes=2):
    """uniform noise box-filtered along every axis: thresholding it gives blobs of many sizes"""
    x = np.random.RandomState(seed).rand(*shape)
    for _ in range(passes):
        for ax in range(3):
            x = (x + np.roll(x, 1, ax) + np.roll(x, -1, ax)) / 3
    return x


def masks():
    out = {}
    out["noise_sparse"] = smooth_noise((12, 14, 16), 1, 1) > 0.56
    out["noise_mid"] = smooth_noise((16, 16, 16), 2) > 0.52
    out["noise_dense"] = smooth_noise((10, 12, 20), 3, 1) > 0.45
    out["salt"] = np.random.RandomState(4).rand(9, 10, 11) > 0.9                 # many one-voxel components, diagonal contacts
    m = np.zeros((8, 8, 70), bool)                                               # runs that cross the 64-voxel segment of a row
    m[2, 3, 5:69] = True
    m[3, 4, 60:70] = True
    m[6, 0, 69] = True
    m[6, 1, 0] = True                                                            # end of one row, start of the next: not adjacent
    out["rows"] = m
    m = np.zeros((6, 6, 6), bool)                                                # corner and edge contacts only
    m[0, 0, 0] = m[1, 1, 1] = m[2, 2, 1] = m[2, 3, 2] = m[5, 5, 5] = m[4, 5, 4] = True
    out["diagonals"] = m
    m = np.zeros((14, 14, 14), bool)                                             # two nested shells, not connected
    m[1:13, 1:13, 1:13] = True
    m[2:12, 2:12, 2:12] = False
    m[4:10, 4:10, 4:10] = True
    m[5:9, 5:9, 5:9] = False
    out["shells"] = m
    z, y, x = np.indices((8, 9, 10))
    out["checkerboard"] = (z + y + x) % 2 == 0
    m = np.zeros((5, 12, 40), bool)                                              # a one-voxel-wide serpentine
    for r in range(0, 12, 2):
        m[2, r, :] = True
        if r + 1 < 12:
            m[2, r + 1, 39 if (r // 2) % 2 == 0 else 0] = True
    out["serpentine"] = m
    out["full"] = np.ones((5, 6, 7), bool)
    return out


def main():
    ref = load_reference_utils()
    d = {"names": np.array(sorted(masks()))}
    for name, m in sorted(masks().items()):
        t0 = time.time()
        img = m.astype(np.int32)
        cc = ref.check_connection(np.argwhere(m), img)
        assert cc.shape == (int(m.sum()),) and cc.max() < 2 ** 15
        d[name + "/shape"] = np.asarray(m.shape, dtype=np.int32)
        d[name + "/bits"] = np.packbits(m.ravel())
        d[name + "/labels"] = cc.astype(np.int16)
        print("  %-14s %-14s %5d voxels, %4d components, %.2fs" % (name, m.shape, m.sum(), cc.max(), time.time() - t0))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **d)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
