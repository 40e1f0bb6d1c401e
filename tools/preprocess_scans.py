"""The reference's dataset preparation (data/data_process.py) through the device path: for every case of a directory, orient the scan and its label,
resample both to 1 mm (data_gpu.preprocess_scan) and cut the cube around the label's foreground (data_gpu.make_merge), then write what the reference
writes — <out>/<case>/img.npy (int16), label.npy (int8), merge.npy (int16, (d, h, w, 2)) — which NumpyLoader_Multi_merge / DeviceCaseLoader read.

A case is a directory <root>/<case>/ holding
    raw.npy + affine.npy [+ label.npy + label_affine.npy]     the array as the scanner wrote it (X, Y, Z) and its affine (4 x 4, 3 x 3 or the 3 diagonal entries)
or, only where `nibabel` is importable (it is an optional extra, never required),
    image.nii[.gz] [+ label.nii[.gz]]
label_affine.npy defaults to affine.npy.  A case without a label gets img.npy on the whole 1 mm grid and no merge.npy.

    python tools/preprocess_scans.py ROOT OUT [--pad 32] [--cases NAME ...]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SCAN_DTYPES = (np.int16, np.uint8, np.int8, np.float32)


def _diag(affine):
    a = np.asarray(affine, dtype=np.float64)
    return np.diagonal(a)[:3] if a.ndim == 2 else a.reshape(-1)[:3]


def _scan_array(a):
    """an array in one of the dtypes the kernel reads: other integer types go to int16 where they fit (as the files the reference writes), floats to float32"""
    a = np.asarray(a)
    if a.dtype in SCAN_DTYPES:
        return np.ascontiguousarray(a)
    if np.issubdtype(a.dtype, np.integer) and a.size and -32768 <= a.min() and a.max() <= 32767:
        return np.ascontiguousarray(a.astype(np.int16))
    return np.ascontiguousarray(a.astype(np.float32))


def _nifti(path):
    try:
        import nibabel
    except ImportError:
        raise SystemExit("%s: reading NIfTI needs nibabel, which is not installed; save raw.npy + affine.npy instead" % path)
    img = nibabel.load(path)
    return np.asanyarray(img.dataobj), img.affine


def load_case(folder):
    """-> (raw, affine_diag, label or None, label_affine_diag or None)"""
    def first(*names):
        for n in names:
            if os.path.exists(os.path.join(folder, n)):
                return os.path.join(folder, n)
        return None
    label = label_diag = None
    if first("raw.npy"):
        if not first("affine.npy"):
            raise SystemExit("%s: raw.npy without affine.npy" % folder)
        raw, diag = np.load(first("raw.npy")), _diag(np.load(first("affine.npy")))
        if first("label.npy"):
            label = np.load(first("label.npy"))
            label_diag = _diag(np.load(first("label_affine.npy"))) if first("label_affine.npy") else diag
    elif first("image.nii.gz", "image.nii"):
        raw, affine = _nifti(first("image.nii.gz", "image.nii"))
        diag = _diag(affine)
        if first("label.nii.gz", "label.nii"):
            label, laffine = _nifti(first("label.nii.gz", "label.nii"))
            label_diag = _diag(laffine)
    else:
        return None
    return _scan_array(raw), diag, None if label is None else _scan_array(label), label_diag


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("root")
    ap.add_argument("out")
    ap.add_argument("--pad", type=int, default=32)
    ap.add_argument("--cases", nargs="*", default=None)
    args = ap.parse_args()
    import torch
    from vae_segmentation_amd import data_gpu
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_scans.py runs the device path; there is no GPU here")
    names = args.cases if args.cases else sorted(n for n in os.listdir(args.root) if os.path.isdir(os.path.join(args.root, n)))
    done = 0
    for name in names:
        case = load_case(os.path.join(args.root, name))
        if case is None:
            print("%s: no raw.npy / image.nii[.gz], skipped" % name)
            continue
        raw, diag, label, label_diag = case
        pre = data_gpu.preprocess_scan(torch.from_numpy(raw).cuda(), diag, None if label is None else torch.from_numpy(label).cuda(), label_diag, truncate=True)
        dst = os.path.join(args.out, name)
        os.makedirs(dst, exist_ok=True)
        if pre["label"] is None:
            np.save(os.path.join(dst, "img.npy"), pre["image"].cpu().numpy().astype(np.int16))
            print("%s: %s at %s -> img.npy %s (no label: no cube)" % (name, raw.shape, tuple(diag), tuple(pre["image"].shape)))
        else:
            merge = data_gpu.make_merge(pre, args.pad).cpu().numpy().astype(np.int16)
            np.save(os.path.join(dst, "img.npy"), merge[..., 0])
            np.save(os.path.join(dst, "label.npy"), merge[..., 1].astype(np.int8))
            np.save(os.path.join(dst, "merge.npy"), merge)
            print("%s: %s at %s -> 1 mm %s -> cube %s" % (name, raw.shape, tuple(diag), pre["geometry"].shape_1mm, merge.shape[:3]))
        done += 1
    print("wrote %d case(s) to %s" % (done, args.out))


if __name__ == "__main__":
    main()
