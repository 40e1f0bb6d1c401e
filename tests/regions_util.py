"""The definitions behind vae_segmentation_amd's region measurements, restated with scipy.ndimage and numpy on the host — the yardstick of
tests/test_host_regions.py and tests/test_gpu_regions.py — and the hand-made scenes both files use.  Everything here is integer arithmetic
except the final divisions."""
import numpy as np
from scipy import ndimage

STRUCT = {6: ndimage.generate_binary_structure(3, 1), 26: ndimage.generate_binary_structure(3, 3)}
LESION_FIELDS = ("n_gt", "n_pred", "tp", "fn", "fp", "sensitivity", "precision", "f1", "overflow")


def planes_of(x):
    """(N, C, D, H, W) -> the list of its (D, H, W) planes"""
    return list(x.reshape((-1,) + x.shape[2:]))


def ref_label(mask, connectivity=26):
    """scipy.ndimage.label of the binarised (>= 0.5) (D, H, W) mask -> (labels int32, K)"""
    lab, k = ndimage.label(np.asarray(mask) >= 0.5, structure=STRUCT[connectivity])
    return lab.astype(np.int32), int(k)


def ref_region_props(labels, max_rows):
    """(D, H, W) integer labels -> {"count" (R,), "bbox" (R, 6), "sums" (R, 3), "centroid" (R, 3), "overflow"} for the labels 1..R = max_rows"""
    lab = np.asarray(labels).astype(np.int64)
    d, h, w = lab.shape
    ok = (lab >= 0) & (lab <= max_rows)
    inside = np.where(ok, lab, 0)
    count = np.bincount(inside.ravel(), minlength=max_rows + 1)[1:max_rows + 1].astype(np.int64)
    bbox = np.empty((max_rows, 6), np.int32)
    bbox[:, :3] = (d, h, w)
    bbox[:, 3:] = -1
    for i, sl in enumerate(ndimage.find_objects(inside.astype(np.int32), max_label=max_rows)):
        if sl is not None:
            bbox[i] = [s.start for s in sl] + [s.stop - 1 for s in sl]
    sums = np.zeros((max_rows + 1, 3), np.int64)
    z, y, x = np.indices(lab.shape)
    for axis, coord in enumerate((z, y, x)):
        np.add.at(sums[:, axis], inside.ravel(), coord.ravel())
    sums = sums[1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        centroid = sums.astype(np.float64) / count.astype(np.float64)[:, None]
    return {"count": count, "bbox": bbox, "sums": sums, "centroid": centroid, "overflow": int((~ok).sum())}


def ref_contingency(a, b, rows_a, rows_b):
    """-> (table int64 (rows_a + 1, rows_b + 1), overflow): np.bincount on a * (rows_b + 1) + b over the voxels with both labels in range"""
    a, b = np.asarray(a).astype(np.int64).ravel(), np.asarray(b).astype(np.int64).ravel()
    ok = (a >= 0) & (a <= rows_a) & (b >= 0) & (b <= rows_b)
    table = np.bincount(a[ok] * (rows_b + 1) + b[ok], minlength=(rows_a + 1) * (rows_b + 1)).reshape(rows_a + 1, rows_b + 1)
    return table.astype(np.int64), int((~ok).sum())


def ratio(num, den, other):
    """num / den; where den is 0: 1.0 if the other side is empty too, else 0.0"""
    num, den, other = (np.asarray(v, dtype=np.int64) for v in (num, den, other))
    out = np.where(other == 0, 1.0, 0.0)
    np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den != 0)
    return out


def ref_confusion(pred, gt, n_class):
    table, overflow = ref_contingency(pred, gt, n_class - 1, n_class - 1)
    tp, p, g = np.diag(table), table.sum(1), table.sum(0)
    return {"table": table, "dice": ratio(2 * tp, p + g, p + g), "iou": ratio(tp, p + g - tp, p + g), "sensitivity": ratio(tp, g, p),
            "precision": ratio(tp, p, g), "overflow": overflow}


def ref_lesion(pred, gt, connectivity=26, min_overlap=1, min_size=0):
    """the lesion-wise record of two (D, H, W) masks by the definition of evaluation.lesion_metrics, with components REMOVED from the masks"""
    sides = []
    for m in (pred, gt):
        lab, k = ref_label(m, connectivity)
        sizes = np.bincount(lab.ravel(), minlength=k + 1)
        small = np.flatnonzero(sizes < min_size)
        lab, k = ref_label(np.where(np.isin(lab, small), 0, lab) > 0, connectivity)           # removing components never merges the others
        sides.append((lab, k))
    (P, n_pred), (G, n_gt) = sides
    T, _ = ref_contingency(P, G, n_pred, n_gt)
    tp = int((T[1:, 1:].sum(0) >= min_overlap).sum())
    fp = int((T[1:, 1:].sum(1) == 0).sum())
    fn = n_gt - tp
    return {"n_gt": n_gt, "n_pred": n_pred, "tp": tp, "fn": fn, "fp": fp, "sensitivity": float(ratio(tp, n_gt, n_pred)),
            "precision": float(ratio(n_pred - fp, n_pred, n_gt)), "f1": float(ratio(2 * tp, 2 * tp + fp + fn, n_gt + n_pred)), "overflow": 0}


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
def two_cubes():
    """(12, 10, 70) mask: a 3^3 cube and a 4 x 4 x 10 block that crosses x = 64; -> (mask, [(count, box, centroid), ...]) in label order"""
    m = np.zeros((12, 10, 70), bool)
    m[1:4, 2:5, 3:6] = True
    m[6:10, 5:9, 60:70] = True
    return m, [(27, (1, 2, 3, 3, 4, 5), (2.0, 3.0, 4.0)), (160, (6, 5, 60, 9, 8, 69), (7.5, 6.5, 64.5))]


def three_class_pair():
    """two (1, 3, 4) label maps and their 3 x 3 table, table[predicted][labelled]"""
    pred = np.array([[[0, 0, 1, 1], [0, 2, 2, 1], [0, 0, 2, 2]]], np.int32)
    gt = np.array([[[0, 1, 1, 1], [0, 2, 1, 1], [0, 0, 0, 2]]], np.int32)
    table = np.array([[4, 1, 0], [0, 3, 0], [1, 1, 2]], np.int64)
    return pred, gt, table


def lesion_scene():
    """(8, 10, 40) masks.  Reference: g1, g2 (bridged by ONE predicted component, 2 shared voxels each), g3 (hit by TWO predicted components, 1 + 2
    shared voxels), g4 (missed), g5 (a single voxel, missed).  Prediction: the bridge p1, p2 (1 voxel) and p3 (2 voxels) inside g3, p4 (12 voxels)
    and p5 (1 voxel) touching nothing.  -> (pred, gt, {(min_overlap, min_size): (n_gt, n_pred, tp, fn, fp)})"""
    gt, pred = np.zeros((8, 10, 40), bool), np.zeros((8, 10, 40), bool)
    gt[1:3, 1:3, 1:4] = True
    gt[1:3, 1:3, 8:11] = True
    gt[5:7, 5:8, 1:5] = True
    gt[5:7, 1:3, 20:23] = True
    gt[0, 9, 39] = True
    pred[1, 1, 2:10] = True
    pred[5, 5, 1] = True
    pred[6, 7, 3:5] = True
    pred[1:3, 6:8, 30:33] = True
    pred[7, 0, 39] = True
    want = {(1, 0): (5, 5, 3, 2, 2), (3, 0): (5, 5, 1, 4, 2), (1, 2): (4, 3, 3, 1, 1), (2, 2): (4, 3, 3, 1, 1), (3, 2): (4, 3, 0, 4, 1)}
    return pred, gt, want


def random_blobs(shape, count, seed, radius=(1.0, 3.5)):
    """a (D, H, W) bool mask of `count` ellipsoids at seeded positions (some touch, some leave the volume)"""
    rs = np.random.RandomState(seed)
    m = np.zeros(shape, bool)
    grid = np.indices(shape)
    for _ in range(count):
        centre = [rs.uniform(0, s) for s in shape]
        r = [rs.uniform(*radius) for _ in shape]
        m |= sum(((g - c) / rr) ** 2 for g, c, rr in zip(grid, centre, r)) <= 1.0
    return m


def checkerboard(shape):
    """every other voxel: under 6-connectivity each voxel is its own component and every run has length 1"""
    z, y, x = np.indices(shape)
    return (z + y + x) % 2 == 0


def touching_faces(shape):
    """a mask with foreground on all six faces: a frame of the volume's edges plus a block in the middle"""
    m = np.zeros(shape, bool)
    m[0, :, 0] = m[-1, :, -1] = m[:, 0, 0] = m[:, -1, -1] = m[0, 0, :] = m[-1, -1, :] = True
    d, h, w = shape
    m[d // 3:d // 3 + 2, h // 3:h // 3 + 2, w // 3:w // 3 + 5] = True
    return m
