"""The training data pipeline of the reference (main_source.py:191-211) on the device: the transform classes of utils/utils.py with the
same names, constructor arguments and dict-in / dict-out protocol, operating on CUDA tensors through libvaeseg's vs_data_* kernels.

    NumpyLoader_Multi_merge   utils/utils.py:220-276   (the relabelling; file I/O stays with the caller: hand it the merge array)
    CropResize                utils/utils.py:326-383   (bounding box of the label or of a coarse prediction, cube crop + zero pad, resize)
    MySpatialTransform        utils/utils.py:927-968   (batchgenerators augment_spatial: elastic deformation — which main_source.py:198 switches off;
                                                        here it needs a noise source chosen, see the class — rotation, scale, random crop)
    Clip, CenterIntensities   utils/utils.py:508-533, 575-618
    IntensityStandardizer     no counterpart in the reference, whose window is a constant: a scan's own percentiles mapped onto that window (or, with fit(),
                              onto a Nyul-Udupa standard scale) before everything else, exact order statistics found on the device
    IntensityAugment          no counterpart in the reference's loaders: the batchgenerators / nnU-Net intensity transforms it inherits and leaves off
                              (noise, blur, brightness, contrast, simulated low resolution, gamma, mirror), applied after CenterIntensities; intensity_augment is its functional form
    PatchSampler, train_patch no counterpart in the reference, which trains on CropResize'd crops only: nnU-Net's patch sampling — windows of the unscaled case, a share of
                              each batch forced onto a random foreground voxel — cut on the device in place of CropResize, nothing read back (train_patch is train_sample's companion)

The reference runs this chain on 16 CPU workers per loader (skimage resize + scipy map_coordinates of 128^3 volumes: seconds per
sample); here a sample costs a handful of kernel launches.  One host synchronisation per sample remains: the crop cube's side depends
on the label's bounding box, so six integers come back before the crop buffers are sized.  Random parameters are drawn on the host
from numpy's RandomState in augment_spatial's order (a dozen scalars per sample).  Arithmetic parity: tests/test_gpu_data.py against
oracle/data_cpu.py (scipy.ndimage)."""
import ctypes

import numpy as np
import torch

from . import volume
from ._lib import check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _vol(t):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()):
        raise TypeError("expected a contiguous CUDA float32 volume (D, H, W), got %s %s on %s" % (tuple(t.shape), t.dtype, t.device))
    return t


def _ints(vals):
    return (ctypes.c_int * 3)(*[int(v) for v in vals])


def relabel(label_map, mask_index):
    """NumpyLoader_Multi_merge's mask_index handling (utils/utils.py:253-262): pairs ([source labels], target)"""
    _vol(label_map)
    src, dst = [], []
    for sources, target in mask_index:
        for s in (sources if isinstance(sources, (list, tuple)) else [sources]):
            src.append(float(s)); dst.append(float(target))
    out = torch.empty_like(label_map)
    check(lib.vs_data_relabel(label_map.data_ptr(), out.data_ptr(), label_map.numel(), (ctypes.c_float * len(src))(*src),
                              (ctypes.c_float * len(dst))(*dst), len(src), _stream()), "data_relabel")
    return out


def bounding_box(label):
    """-> (min[3], max[3]) of label > 0 as numpy ints, or None when the label is empty (one host synchronisation)"""
    _vol(label)
    box = torch.empty(6, dtype=torch.int32, device=label.device)
    check(lib.vs_data_bbox(label.data_ptr(), *label.shape, box.data_ptr(), _stream()), "data_bbox")
    b = box.cpu().numpy()
    return None if b[3] < 0 else (b[:3].astype(np.int64), b[3:].astype(np.int64))


def crop_pad_cube(vol, centre, L, pad, shift=0):
    _vol(vol)
    lo = [max(int(centre[d]) - L // 2 - pad + shift, 0) for d in range(3)]
    hi = [min(int(centre[d]) + L // 2 + pad + shift, vol.shape[d]) for d in range(3)]
    side = L + 2 * pad
    off = [int((side - (hi[d] - lo[d])) / 2) for d in range(3)]
    out = torch.empty((side, side, side), dtype=torch.float32, device=vol.device)
    check(lib.vs_data_crop_pad(vol.data_ptr(), out.data_ptr(), *vol.shape, side, side, side, _ints(lo), _ints(hi), _ints(off), _stream()), "data_crop_pad")
    return out


def crop_geometry(box, shape, shift=0):
    """Where CropResize puts a scan of `shape` whose box is `box` = (min[3], max[3]) (bounding_box): -> (lo[3], hi[3], off[3], side), plain ints.  The
    scan rows [lo, hi) of every axis land at [off, off + hi - lo) of a zero cube of side `side`, which is then resized to the patch — the integers of
    CropResize.__call__ and crop_pad_cube.  Host arithmetic only; ops.uncrop takes the tuple to paste a patch-space prediction back into the scan."""
    bmin, bmax = (np.asarray(b).astype(np.int64) for b in box)
    centre, L = (bmax + bmin) // 2, int(np.max(bmax - bmin))
    pad = int(L * 0.1)
    lo = [max(int(centre[d]) - L // 2 - pad + shift, 0) for d in range(3)]
    hi = [min(int(centre[d]) + L // 2 + pad + shift, int(shape[d])) for d in range(3)]
    side = L + 2 * pad
    off = [int((side - (hi[d] - lo[d])) / 2) for d in range(3)]
    return lo, hi, off, side


def resize(vol, output_size, order=1, anti_aliasing=None):
    """skimage.transform.resize(vol, output_size, order=order, anti_aliasing=anti_aliasing) with its other defaults, for a float volume
    (see oracle/data_cpu.py:skimage_resize for the restated algorithm)"""
    _vol(vol)
    out_shape = tuple(int(s) for s in output_size)
    if anti_aliasing is None:
        anti_aliasing = any(o < i for o, i in zip(out_shape, vol.shape))
    lo, hi = 1.0, 0.0                                    # lo > hi: no clipping
    if order > 0:
        mm = torch.empty(2, dtype=torch.float32, device=vol.device)
        check(lib.vs_data_minmax(vol.data_ptr(), vol.numel(), mm.data_ptr(), _stream()), "data_minmax")
        lo, hi = [float(v) for v in mm.cpu()]            # clip=True: to the input's range
    src = vol
    if anti_aliasing and order > 0:
        for axis in range(3):
            sigma = max(0.0, (vol.shape[axis] / out_shape[axis] - 1.0) / 2.0)
            if sigma > 0.0:
                nxt = torch.empty_like(src)
                check(lib.vs_data_gaussian_axis(src.data_ptr(), nxt.data_ptr(), *src.shape, axis, sigma, _stream()), "data_gaussian_axis")
                src = nxt
    out = torch.empty(out_shape, dtype=torch.float32, device=vol.device)
    check(lib.vs_data_zoom(src.data_ptr(), out.data_ptr(), *src.shape, *out_shape, 0 if order == 0 else 1, lo, hi, _stream()), "data_zoom")
    return out


# ---- raw scans: the reference's one-off dataset preparation (data/data_process.py) on the device ---------------------------------------------------
class ScanGeometry:
    """The integers of data_process.py:24-33 for a scan of `raw_shape` = (X, Y, Z) whose affine has the signed diagonal `affine_diag` (a 4 x 4 or
    3 x 3 affine is accepted too: its diagonal is taken).  Host arithmetic only, restated exactly as the reference writes it:
        spacing  = the three diagonal entries, in raw axis order
        ind[i]   = +1 if spacing[i] < 0 else -1
        oriented = transpose(raw, [1, 0, 2])[::ind[1], ::ind[0], ::ind[2]]            shape (Y, X, Z)
        new_size = (oriented_shape * abs(spacing)).astype(int)
    The last line multiplies the TRANSPOSED shape by the UNTRANSPOSED spacing: with spacing (sx, sy, sz) the 1 mm grid is (int(Y sx), int(X sy),
    int(Z sz)).  For the square in-plane spacing of CT it makes no difference; it is kept because the reference's volumes are the yardstick.
    raw_shape, oriented_shape, shape_1mm: int tuples; flips: three bools in oriented axis order (ind[1] < 0, ind[0] < 0, ind[2] < 0);
    as_tuple(): (x, y, z, flip0, flip1, flip2, d1, h1, w1), the plain-int form ops.scan_orient / ops.to_native take."""

    def __init__(self, raw_shape, affine_diag):
        shape = tuple(int(s) for s in raw_shape)
        spacing = np.asarray(affine_diag, dtype=np.float64)
        if spacing.ndim == 2:
            spacing = np.diagonal(spacing)[:3]
        if len(shape) != 3 or spacing.shape != (3,) or min(shape) < 1:
            raise ValueError("ScanGeometry: raw_shape (X, Y, Z) and three affine diagonal entries, got %r, %r" % (raw_shape, affine_diag))
        if not np.all(np.isfinite(spacing)) or np.any(spacing == 0):
            raise ValueError("ScanGeometry: spacing must be finite and non-zero, got %r" % (affine_diag,))
        ind = [1 if s < 0 else -1 for s in spacing]
        self.raw_shape = shape
        self.spacing = tuple(float(s) for s in spacing)
        self.oriented_shape = (shape[1], shape[0], shape[2])
        self.flips = (ind[1] < 0, ind[0] < 0, ind[2] < 0)
        self.shape_1mm = tuple(int(v) for v in (np.array(self.oriented_shape) * np.abs(spacing)).astype(int))
        if min(self.shape_1mm) < 1:
            raise ValueError("ScanGeometry: the 1 mm grid %s of shape %s at spacing %s is empty" % (self.shape_1mm, shape, self.spacing))

    def as_tuple(self):
        return self.raw_shape + tuple(int(f) for f in self.flips) + self.shape_1mm

    def __repr__(self):
        return "ScanGeometry(raw_shape=%s, spacing=%s, flips=%s, shape_1mm=%s)" % (self.raw_shape, self.spacing, self.flips, self.shape_1mm)


def cube_slices(box, shape, pad=32):
    """The three slices of data_process.py:45-68 for the foreground box `box` = (min[3], max[3]) of a label of `shape`: box -/+ pad clipped to the volume
    (the upper bound is max + pad, as the reference writes it), center = mean(bbox, 1).astype(int), L = the largest extent, rows
    [center - int(L / 2), center - int(L / 2) + L) clipped again.  Host arithmetic only."""
    pad = [int(pad)] * 3 if np.isscalar(pad) else [int(p) for p in pad]
    shape = [int(s) for s in shape]
    bbox = np.array([[max(0, int(box[0][d]) - pad[d]), min(shape[d], int(box[1][d]) + pad[d])] for d in range(3)])
    center = np.mean(bbox, 1).astype(int)
    L = int(np.max(bbox[:, 1] - bbox[:, 0]))
    return tuple(slice(max(0, int(center[d]) - int(L / 2)), min(shape[d], int(center[d]) - int(L / 2) + L)) for d in range(3))


def foreground_cube(label_1mm, pad=32):
    """cube_slices of the bounding box of label_1mm > 0 (bounding_box: the one host synchronisation).  An empty label raises ValueError (the reference
    fails on np.min of an empty array there)."""
    box = bounding_box(label_1mm)
    if box is None:
        raise ValueError("foreground_cube: the label has no foreground")
    return cube_slices(box, label_1mm.shape, pad)


def preprocess_scan(raw, affine_diag, label=None, label_affine_diag=None, truncate=False):
    """data_process.py:23-42 on the device.  raw (X, Y, Z): a CUDA int16 / uint8 / int8 / float32 tensor as the scanner wrote it; affine_diag: the
    signed diagonal of its affine.  The scan is oriented (ops.scan_orient) and resized to ScanGeometry.shape_1mm with skimage's defaults (order 1,
    anti-aliasing where an axis shrinks).  label (optional, same dtypes): oriented by ITS affine's diagonal (label_affine_diag, default the image's) and
    resized with order 0 / no anti-aliasing to the IMAGE's shape_1mm, as the reference does.
    -> {"image": (D1, H1, W1) fp32, "label": fp32 or None, "geometry": the image's ScanGeometry}, on the device.
    truncate=True applies the astype(int16) / astype(int8) truncation towards zero that img.npy / label.npy / merge.npy store; the tensors stay float32
    and hold those integers (values inside the integer types' range, which CT intensities and labels are)."""
    geometry = ScanGeometry(tuple(raw.shape), affine_diag)
    image = resize(volume.scan_orient(raw, geometry), geometry.shape_1mm)
    lab = None
    if label is not None:
        lgeo = ScanGeometry(tuple(label.shape), affine_diag if label_affine_diag is None else label_affine_diag)
        lab = resize(volume.scan_orient(label, lgeo), geometry.shape_1mm, order=0, anti_aliasing=False)
    if truncate:
        image = image.trunc_()
        lab = None if lab is None else lab.trunc_()
    return {"image": image, "label": lab, "geometry": geometry}


def make_merge(pre, pad=32):
    """preprocess_scan's dict -> the (d, h, w, 2) cube of data_process.py:57-75 that merge.npy holds: image and label cut to foreground_cube(label, pad),
    stacked on a last axis and truncated towards zero (the file's astype(int16)), as a float32 CUDA tensor — what train_sample / DeviceCaseLoader take."""
    if pre.get("label") is None:
        raise ValueError("make_merge: the case has no label (data_process.py cuts the cube around the label's foreground)")
    sl = foreground_cube(pre["label"], pad)
    return torch.stack((pre["image"][sl], pre["label"][sl]), dim=-1).trunc_()


class BaseTransform:
    def __init__(self, fields):
        self.fields = [fields] if isinstance(fields, str) else list(fields)


class CropResize(BaseTransform):
    """utils/utils.py:326-383 (fields f, f + '_pancreas' and, when present, the coarse prediction f + '_pancreas_pred' that then defines the box)"""

    def __init__(self, fields, output_size, pad=32, shift=0):
        super().__init__(fields)
        self.output_size, self.pad, self.shift = output_size, pad, shift

    def __call__(self, data_dict):
        for f in self.fields:
            if data_dict.get(f) is None:
                continue
            img, label = data_dict[f], data_dict[f + "_pancreas"]
            pred = data_dict.get(f + "_pancreas_pred")
            if isinstance(pred, torch.Tensor):               # utils/utils.py:345-358: the box of a coarse prediction (which the reference assumes non-empty)
                box = bounding_box(pred)
                if box is None:
                    raise ValueError("CropResize: empty %s_pancreas_pred (the reference fails on np.max of an empty index array here)" % f)
            else:
                box = bounding_box(label)
            if box is not None:
                centre, L = (box[1] + box[0]) // 2, int(np.max(box[1] - box[0]))
            else:
                centre, L = np.array([64, 64, 64]), 32
            pad = int(L * 0.1)
            if isinstance(pred, torch.Tensor):
                data_dict[f + "_pancreas_pred"] = resize(crop_pad_cube(pred, centre, L, pad, 0), self.output_size, order=0, anti_aliasing=False)
            lab_c = crop_pad_cube(label, centre, L, pad, self.shift)
            data_dict["ori_shape"] = np.array(list(label.shape) + list(lab_c.shape))
            data_dict[f] = resize(crop_pad_cube(img, centre, L, pad, self.shift), self.output_size)
            data_dict[f + "_pancreas"] = resize(lab_c, self.output_size, order=0, anti_aliasing=False)
        return data_dict


def rotation_matrix(ax, ay, az):
    """batchgenerators' create_matrix_rotation_{x,y,z}_3d chained from the identity"""
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return np.identity(3) @ rx @ ry @ rz


def _resample(vol, field, patch_size, angles, scale, centre, order, cval):
    _vol(vol)
    a = (scale * rotation_matrix(*angles).T).astype(np.float64).reshape(-1)          # row vectors times R == R^T times column vectors
    a9, c3 = (ctypes.c_double * 9)(*a), (ctypes.c_double * 3)(*[float(v) for v in centre])
    out = torch.empty(tuple(int(s) for s in patch_size), dtype=torch.float32, device=vol.device)
    if order == 3:
        coef = torch.empty(vol.shape, dtype=torch.float64, device=vol.device)
        check(lib.vs_data_spline3_prefilter(vol.data_ptr(), coef.data_ptr(), *vol.shape, _stream()), "data_spline3_prefilter")
        src = coef
    elif order == 0:
        src = vol
    else:
        raise NotImplementedError("native resampling: order 3 (image) or 0 (label), the reference's settings")
    if field is None:
        check(lib.vs_data_affine_sample(src.data_ptr(), out.data_ptr(), *vol.shape, *out.shape, a9, c3, order, float(cval), _stream()), "data_affine_sample")
    else:
        if not (field.is_cuda and field.dtype == torch.float64 and tuple(field.shape) == (3,) + tuple(out.shape) and field.is_contiguous()):
            raise TypeError("expected a contiguous CUDA float64 displacement field %s, got %s %s on %s"
                            % ((3,) + tuple(out.shape), tuple(field.shape), field.dtype, field.device))
        check(lib.vs_data_warp_sample(src.data_ptr(), out.data_ptr(), field.data_ptr(), *vol.shape, *out.shape, a9, c3, order, float(cval), _stream()),
              "data_warp_sample")
    return out


def affine_resample(vol, patch_size, angles, scale, centre, order, cval):
    """one channel through augment_spatial's coordinate map: coords = (mesh - (P-1)/2) . R * scale + centre, then
    scipy.ndimage.map_coordinates(order, mode='constant', cval)"""
    return _resample(vol, None, patch_size, angles, scale, centre, order, cval)


def warp_resample(vol, field, patch_size, angles, scale, centre, order, cval):
    """affine_resample with the displacement `field` (3, *patch_size), fp64 on the device (elastic_field), added to the zero-centred mesh before
    rotation and scale, as augment_spatial adds its elastic offsets: coords = (mesh - (P-1)/2 + field) . R * scale + centre"""
    return _resample(vol, field, patch_size, angles, scale, centre, order, cval)


ELASTIC_MAX_SIGMA = 32.0          # radius int(4 sigma + 0.5) <= 128: the longest weight table the filter kernels take


def _is_counter(noise):
    return isinstance(noise, tuple) and len(noise) == 2 and all(isinstance(v, (int, np.integer)) for v in noise)


def elastic_field(patch, alpha, sigma, noise):
    """augment_spatial's elastic offsets for one sample: scipy.ndimage.gaussian_filter(noise[k], sigma, mode="constant", cval=0) * alpha for the three
    axes k -> (3, D, H, W) fp64 on the device, in voxels.  `noise`: the three fields uniform in [-1, 1) as a (3, D, H, W) float64 array or tensor (host
    or device), or a tuple (seed, sample) of ints: the fields are then made on the device by Philox4x32-10 (vs_data_noise_philox), a pure function of
    (seed, sample, axis, voxel)."""
    patch = tuple(int(s) for s in patch)
    if len(patch) != 3 or min(patch) < 1:
        raise ValueError("elastic_field: patch is (D, H, W), got %r" % (patch,))
    alpha, sigma = float(alpha), float(sigma)
    if not (0.0 < sigma <= ELASTIC_MAX_SIGMA) or not np.isfinite(alpha):
        raise ValueError("elastic_field: 0 < sigma <= %g and a finite alpha, got sigma %r, alpha %r" % (ELASTIC_MAX_SIGMA, sigma, alpha))
    shape = (3,) + patch
    if _is_counter(noise):
        src = torch.empty(shape, dtype=torch.float64, device="cuda")
        check(lib.vs_data_noise_philox(src.data_ptr(), *patch, int(noise[0]) & (2 ** 64 - 1), int(noise[1]) & (2 ** 64 - 1), _stream()), "data_noise_philox")
    else:
        src = torch.from_numpy(noise) if isinstance(noise, np.ndarray) else noise
        if not isinstance(src, torch.Tensor) or src.dtype != torch.float64 or tuple(src.shape) != shape:
            raise TypeError("elastic_field: noise is a float64 array or tensor of shape %s or a tuple (seed, sample) of ints" % (shape,))
        src = src.cuda().contiguous()
    field, tmp = torch.empty_like(src), torch.empty_like(src)
    check(lib.vs_data_elastic_field(src.data_ptr(), field.data_ptr(), tmp.data_ptr(), *patch, sigma, alpha, _stream()), "data_elastic_field")
    return field


class MySpatialTransform:
    """utils/utils.py:927-968 with the arguments main_source.py:196-205 passes.  data_dict[data_key] / [label_key]: (B, C, D, H, W) CUDA
    tensors (the reference reshapes to [-1, 1, D, H, W] first).  `rng`: a numpy RandomState (default: the global one, as batchgenerators).
    Elastic deformation (do_elastic_deform and p_el_per_sample > 0) needs `noise` chosen, because the two sources give different samples:
      noise="numpy"   alpha, sigma and then the three rng.random_sample(patch) fields are drawn from `rng` in augment_spatial's order, before the
                      rotation draws: a seeded RandomState yields the stream batchgenerators would consume; the fields cross to the device
      noise="philox"  only alpha and sigma come from `rng`; the fields are made on the device from (seed, n), n counting this transform's deformed
                      samples: nothing patch-sized leaves the device, and the stream of `rng` differs from batchgenerators' from the first sample on
    One field per sample is shared by all of its channels and by its label."""

    def __init__(self, patch_size, patch_center_dist_from_border=30, do_elastic_deform=True, alpha=(0., 1000.), sigma=(10., 13.), do_rotation=True,
                 angle_x=(0, 2 * np.pi), angle_y=(0, 2 * np.pi), angle_z=(0, 2 * np.pi), do_scale=True, scale=(0.75, 1.25), border_mode_data="nearest",
                 border_cval_data=0, order_data=3, border_mode_seg="constant", border_cval_seg=0, order_seg=0, random_crop=True, data_key="data",
                 label_key="seg", p_el_per_sample=1, p_scale_per_sample=1, p_rot_per_sample=1, independent_scale_for_each_axis=False,
                 p_rot_per_axis: float = 1, rng=None, noise=None, seed=0):
        if noise not in (None, "numpy", "philox"):
            raise ValueError("MySpatialTransform: noise is None, 'numpy' or 'philox', got %r" % (noise,))
        self.do_elastic = bool(do_elastic_deform and p_el_per_sample > 0)
        if self.do_elastic and noise is None:
            raise NotImplementedError("elastic deformation needs a noise source: choose noise='numpy' (the fields are drawn from rng, batchgenerators' "
                                      "stream) or noise='philox' (made on the device from seed); main_source.py:198 passes do_elastic_deform=False")
        if self.do_elastic and not (0 <= alpha[0] <= alpha[1] and 0 < sigma[0] <= sigma[1] <= ELASTIC_MAX_SIGMA):
            raise ValueError("MySpatialTransform: elastic deformation takes 0 <= alpha[0] <= alpha[1] and 0 < sigma[0] <= sigma[1] <= %g, got %r, %r"
                             % (ELASTIC_MAX_SIGMA, alpha, sigma))
        self.alpha, self.sigma, self.p_el, self.noise, self.seed, self.n_elastic = alpha, sigma, p_el_per_sample, noise, int(seed), 0
        if border_mode_data != "constant" or border_mode_seg != "constant" or independent_scale_for_each_axis:
            raise NotImplementedError("native resampling: constant borders, isotropic scale (main_source.py:196-205)")
        self.patch_size = patch_size
        self.dist = patch_center_dist_from_border if isinstance(patch_center_dist_from_border, (list, tuple, np.ndarray)) else 3 * [patch_center_dist_from_border]
        self.do_rotation, self.angle = do_rotation, (angle_x, angle_y, angle_z)
        self.do_scale, self.scale = do_scale, scale
        self.cval_data, self.cval_seg, self.order_data, self.order_seg = border_cval_data, border_cval_seg, order_data, order_seg
        self.random_crop, self.data_key, self.label_key = random_crop, data_key, label_key
        self.p_scale, self.p_rot, self.p_rot_axis = p_scale_per_sample, p_rot_per_sample, p_rot_per_axis
        self.rng = rng if rng is not None else np.random

    def draw(self, shape):
        """the random draws of one sample in augment_spatial's order -> (angles, scale, centre, modified), and for a deformed sample a fifth element
        (alpha, sigma, noise_spec): noise_spec is what elastic_field takes, the (3, D, H, W) fields (noise='numpy') or (seed, n) (noise='philox')"""
        r = self.rng
        angles, sc, modified, elastic = [0.0, 0.0, 0.0], 1.0, False, None
        if self.do_elastic and r.uniform() < self.p_el:
            a, s = r.uniform(self.alpha[0], self.alpha[1]), r.uniform(self.sigma[0], self.sigma[1])
            if self.noise == "numpy":
                patch = tuple(self.patch_size) if self.patch_size is not None else tuple(shape)
                spec = np.stack([r.random_sample(patch) * 2 - 1 for _ in range(3)])
            else:
                spec = (self.seed, self.n_elastic)
            self.n_elastic += 1
            elastic, modified = (a, s, spec), True
        if self.do_rotation and r.uniform() < self.p_rot:
            for d in range(3):
                angles[d] = r.uniform(self.angle[d][0], self.angle[d][1]) if r.uniform() <= self.p_rot_axis else 0.0
            modified = True
        if self.do_scale and r.uniform() < self.p_scale:
            if r.random_sample() < 0.5 and self.scale[0] < 1:
                sc = r.uniform(self.scale[0], 1)
            else:
                sc = r.uniform(max(self.scale[0], 1), self.scale[1])
            modified = True
        if self.random_crop:
            centre = [r.uniform(self.dist[d], shape[d] - self.dist[d]) for d in range(3)]
        else:
            centre = [shape[d] / 2.0 - 0.5 for d in range(3)]
        if elastic is not None:
            return tuple(angles), sc, tuple(centre), modified, elastic
        return tuple(angles), sc, tuple(centre), modified

    def __call__(self, data_dict, params=None):
        data, seg = data_dict.get(self.data_key), data_dict.get(self.label_key)
        patch = tuple(self.patch_size) if self.patch_size is not None else tuple(data.shape[2:])
        out_d = torch.empty((data.shape[0], data.shape[1]) + patch, dtype=torch.float32, device=data.device)
        out_s = None if seg is None else torch.empty((seg.shape[0], seg.shape[1]) + patch, dtype=torch.float32, device=seg.device)
        for b in range(data.shape[0]):
            prm = params[b] if params is not None else self.draw(data.shape[2:])
            angles, sc, centre, modified = prm[:4]
            field = elastic_field(patch, *prm[4]) if len(prm) > 4 and prm[4] is not None else None        # one field for the sample's channels and its label
            if not modified and not self.random_crop and tuple(data.shape[2:]) == patch:
                out_d[b] = data[b]
                if seg is not None:
                    out_s[b] = seg[b]
                continue
            for c in range(data.shape[1]):
                out_d[b, c] = _resample(data[b, c].contiguous(), field, patch, angles, sc, centre, self.order_data, self.cval_data)
            if seg is not None:
                for c in range(seg.shape[1]):
                    out_s[b, c] = _resample(seg[b, c].contiguous(), field, patch, angles, sc, centre, self.order_seg, self.cval_seg)
        data_dict[self.data_key] = out_d
        if seg is not None:
            data_dict[self.label_key] = out_s
        return data_dict


class Clip(BaseTransform):
    """utils/utils.py:508-533"""

    def __init__(self, fields, new_min=0.0, new_max=1.0):
        super().__init__(fields)
        self._new_min, self._new_max = new_min, new_max

    def __call__(self, data_dict):
        for f in self.fields:
            if data_dict.get(f) is not None:
                x = data_dict[f].contiguous()
                check(lib.vs_data_clip_center(x.data_ptr(), x.numel(), float(self._new_min), float(self._new_max), 0.0, 1.0, _stream()), "data_clip_center")
                data_dict[f] = x
        return data_dict


class CenterIntensities(BaseTransform):
    """utils/utils.py:575-618 (scalar subtrahend / divisor, as main_source.py:210 passes)"""

    def __init__(self, fields, subtrahend, divisor=1.0):
        super().__init__(fields)
        if isinstance(subtrahend, (list, tuple, np.ndarray)) or isinstance(divisor, (list, tuple, np.ndarray)):
            raise NotImplementedError("per-channel subtrahend / divisor lists: the reference passes scalars (main_source.py:210)")
        self.subtrahend, self.divisor = subtrahend, divisor

    def __call__(self, data_dict):
        for f in self.fields:
            if data_dict.get(f) is not None:
                x = data_dict[f].contiguous()
                check(lib.vs_data_clip_center(x.data_ptr(), x.numel(), -3.0e38, 3.0e38, float(self.subtrahend), float(self.divisor), _stream()), "data_clip_center")
                data_dict[f] = x
        return data_dict


class IntensityStandardizer(BaseTransform):
    """Intensity standardisation of scans by their own order statistics, on the device (no counterpart in the reference, whose window is written for one
    protocol): the exact `percentiles` of a scan — of its voxels above `above`, under `mask` — are landmarks, and the scan is mapped piecewise linearly so
    that they land on the standard scale (ops.quantile -> ops.intensity_map, the landmarks never leave the device).  Two percentiles (nnU-Net: 0.5, 99.5):
    the standard scale IS `target`, e.g. the window Clip expects, and nothing is fitted.  More (Nyul and Udupa, e.g. (1, 10, 20, ..., 90, 99)): fit() forms
    the scale from training scans.  extrapolate: "linear" lets the end segments run on, "clamp" holds the ends of the scale.  fields: what __call__
    standardises in a data dict (the BaseTransform convention).  DESIGN 3.18 holds the two rules."""

    def __init__(self, percentiles=(0.5, 99.5), target=(-200.0, 400.0), above=None, extrapolate="linear", fields="venous"):
        super().__init__(fields)
        try:
            ps, tg = tuple(float(p) for p in percentiles), tuple(float(t) for t in target)
        except (TypeError, ValueError):
            raise ValueError("IntensityStandardizer: percentiles and target are sequences of numbers, got %r and %r" % (percentiles, target)) from None
        if not 2 <= len(ps) <= volume.INTENSITY_MAP_MAX_L:
            raise ValueError("IntensityStandardizer: 2 to %d percentiles, got %d" % (volume.INTENSITY_MAP_MAX_L, len(ps)))
        if not all(np.isfinite(p) and 0.0 <= p <= 100.0 for p in ps) or any(b <= a for a, b in zip(ps, ps[1:])):
            raise ValueError("IntensityStandardizer: percentiles are strictly ascending in [0, 100], got %r" % (ps,))
        if len(tg) != 2 or not all(np.isfinite(t) for t in tg) or not tg[0] < tg[1]:
            raise ValueError("IntensityStandardizer: target is an ascending pair of finite numbers, got %r" % (tg,))
        if above is not None and not np.isfinite(float(above)):
            raise ValueError("IntensityStandardizer: above is a finite number or None, got %r" % (above,))
        if extrapolate not in volume.INTENSITY_MAP_EXTRAPOLATE:
            raise ValueError("IntensityStandardizer: extrapolate is 'linear' or 'clamp', got %r" % (extrapolate,))
        self.percentiles, self.target, self.extrapolate = ps, tg, extrapolate
        self.above = None if above is None else float(above)
        self.scale = list(tg) if len(ps) == 2 else None           # the standard scale, host floats; None until fit()
        self._dst = {}

    def landmarks(self, x, mask=None):
        """the percentiles of every (D, H, W) plane of x -> fp64 (..., L) on the device (NaN rows where nothing is selected)"""
        return volume.quantile(x, self.percentiles, above=self.above, mask=mask)["q"]

    def fit(self, volumes, masks=None):
        """The standard scale from training scans (Nyul and Udupa): the landmarks s of each scan mapped affinely so that s[0] -> target[0] and
        s[L-1] -> target[1], averaged over the scans in list order, in fp64 on the device.  One read-back, at the end, checks the scale."""
        volumes = list(volumes)
        masks = [None] * len(volumes) if masks is None else list(masks)
        if not volumes or len(masks) != len(volumes):
            raise ValueError("IntensityStandardizer.fit: at least one volume, and a mask (or None) for each")
        total, cases = None, 0
        for x, m in zip(volumes, masks):
            s = self.landmarks(x, m).reshape(-1, len(self.percentiles))
            mapped = self.target[0] + (s - s[:, :1]) * ((self.target[1] - self.target[0]) / (s[:, -1:] - s[:, :1]))
            for row in mapped:
                total = row.clone() if total is None else total + row
                cases += 1
        scale = (total / cases).cpu().tolist()
        if not all(np.isfinite(v) for v in scale) or any(b <= a for a, b in zip(scale, scale[1:])):
            raise ValueError("IntensityStandardizer.fit: the fitted scale is not finite and strictly ascending (a scan without selected voxels, or "
                             "percentiles that coincide in every scan): %r" % (scale,))
        self.scale, self._dst = scale, {}
        return self

    def _scale_on(self, device):
        if self.scale is None:
            raise RuntimeError("IntensityStandardizer: %d percentiles need a standard scale: call fit() or load_state_dict() before transform()"
                               % len(self.percentiles))
        key = str(device)
        if key not in self._dst:
            self._dst[key] = torch.tensor(self.scale, dtype=torch.float64, device=device)
        return self._dst[key]

    def transform(self, x, mask=None):
        """x float32 (..., D, H, W) on the device -> its standardised copy; ten launches, nothing synchronised or read back"""
        dst = self._scale_on(x.device)
        return volume.intensity_map(x, self.landmarks(x, mask), dst, extrapolate=self.extrapolate)

    def state_dict(self):
        return {"percentiles": tuple(self.percentiles), "target": tuple(self.target), "above": self.above, "extrapolate": self.extrapolate,
                "scale": None if self.scale is None else list(self.scale)}

    def load_state_dict(self, state):
        other = IntensityStandardizer(state["percentiles"], state["target"], state["above"], state.get("extrapolate", "linear"), self.fields)
        scale = state["scale"]
        if scale is not None:
            scale = [float(v) for v in scale]
            if len(scale) != len(other.percentiles) or not all(np.isfinite(v) for v in scale) or any(b <= a for a, b in zip(scale, scale[1:])):
                raise ValueError("IntensityStandardizer.load_state_dict: the scale has one finite value per percentile, strictly ascending, got %r" % (scale,))
            other.scale = scale
        self.percentiles, self.target, self.above, self.extrapolate, self.scale, self._dst = (other.percentiles, other.target, other.above,
                                                                                              other.extrapolate, other.scale, {})
        return self

    def __call__(self, data_dict):
        for f in self.fields:
            if data_dict.get(f) is not None:
                data_dict[f] = self.transform(data_dict[f].contiguous())
        return data_dict


# ---- intensity augmentation (csrc/augment.hip; DESIGN "Intensity augmentation" holds the rules) --------------------------------------------------------
_STAT_OPS = ("contrast", "power", "restat", "restat_rec")


def _per_channel(v, channels, what):
    if isinstance(v, (list, tuple, np.ndarray)):
        if len(v) != channels:
            raise ValueError("intensity_augment: %s has %d per-channel values for %d channels" % (what, len(v), channels))
        return list(v)
    return [v] * channels


def lowres_target_shape(shape, zoom, ignore_axes=()):
    """the shape nnU-Net's simulated low resolution down-samples `shape` to: np.round(shape * zoom).astype(int) per axis (round-half-even), the axes in
    ignore_axes keeping their length.  ValueError when an axis would vanish — before anything is launched.  Host arithmetic only."""
    shape, ignore = tuple(int(v) for v in shape), tuple(int(a) for a in ignore_axes)
    zoom = float(zoom)
    if not (np.isfinite(zoom) and zoom > 0):
        raise ValueError("lowres_target_shape: zoom is a positive number, got %r" % (zoom,))
    if any(not 0 <= a < len(shape) for a in ignore):
        raise ValueError("lowres_target_shape: ignore_axes index the %d axes of the shape, got %r" % (len(shape), ignore_axes))
    out = tuple(s if a in ignore else int(np.round(np.float64(s) * np.float64(zoom))) for a, s in enumerate(shape))
    if min(out) < 1:
        raise ValueError("lowres_target_shape: an axis of %s vanishes at zoom %r (target %s)" % (shape, zoom, out))
    return out


def _plane_ops(ops_list, channels, c, shape):
    """the ops of channel c with scalar parameters; gamma becomes power (+ restat from the record of power's input); ops that leave the plane as it is
    (a channel's parameter None, flip 0) are dropped"""
    out = []
    for op in ops_list:
        name, args = op[0], op[1:]
        if name == "noise":
            s, spec = _per_channel(args[0], channels, "noise s")[c], args[1]
            if s is None:
                continue
            if _is_counter(spec):
                n = (int(spec[0]), int(spec[1]))
            else:
                n = torch.from_numpy(spec) if isinstance(spec, np.ndarray) else spec
                if not isinstance(n, torch.Tensor) or n.dtype != torch.float64 or tuple(n.shape) != (channels,) + shape:
                    raise TypeError("intensity_augment: noise is a float64 array or tensor of shape %s or a tuple (seed, sample) of ints"
                                    % ((channels,) + shape,))
                n = n[c].cuda().contiguous()
            out.append(("noise", float(s), n))
        elif name == "blur":
            sigma = _per_channel(args[0], channels, "blur sigma")[c]
            if sigma is not None:
                volume.gaussian_weights(sigma)                                # the range check, before anything is launched
                out.append(("blur", float(sigma)))
        elif name == "lowres":
            zoom = _per_channel(args[0], channels, "lowres zoom")[c]
            order_down, order_up = (int(args[1]) if len(args) > 1 else 0), (int(args[2]) if len(args) > 2 else 3)
            if order_down not in volume.ZOOM_EDGE_ORDERS or order_up not in volume.ZOOM_EDGE_ORDERS:
                raise ValueError("intensity_augment: lowres orders are 0, 1 or 3, got %r" % ((order_down, order_up),))
            if zoom is not None:
                target = lowres_target_shape(shape, zoom, args[3] if len(args) > 3 else ())      # the range check, before anything is launched
                if 3 in (order_down, order_up) and max(shape + target) > volume.ZOOM_EDGE_MAX_LEN:
                    raise ValueError("intensity_augment: lowres with order 3 takes axes of at most %d voxels, got %s" % (volume.ZOOM_EDGE_MAX_LEN, shape))
                out.append(("lowres", target, order_down, order_up))
        elif name == "brightness":
            m = _per_channel(args[0], channels, "brightness m")[c]
            if m is not None:
                out.append(("brightness", float(m)))
        elif name == "contrast":
            f = _per_channel(args[0], channels, "contrast f")[c]
            if f is not None:
                out.append(("contrast", float(f), bool(args[1]) if len(args) > 1 else True))
        elif name in ("gamma", "power"):
            g = _per_channel(args[0], channels, "gamma")[c]
            if g is not None:
                invert = bool(args[1]) if len(args) > 1 else False
                out.append(("power", float(g), invert))
                if name == "gamma" and (bool(args[2]) if len(args) > 2 else False):
                    out.append(("restat_rec", invert))
        elif name == "restat":
            m0 = _per_channel(args[0], channels, "restat mean0")[c]
            if m0 is not None:
                out.append(("restat", float(m0), float(_per_channel(args[1], channels, "restat std0")[c]), bool(args[2]) if len(args) > 2 else False))
        elif name == "flip":
            if not 0 <= int(args[0]) <= 7:
                raise ValueError("intensity_augment: flip mask is 0..7 (z, y, x = 4, 2, 1), got %r" % (args[0],))
            if int(args[0]):
                out.append(("flip", int(args[0])))
        else:
            raise ValueError("intensity_augment: unknown op %r (noise, blur, lowres, brightness, contrast, gamma, power, restat, flip)" % (name,))
    return out


def _augment_plane(x, plane_ops, channel):
    """One plane through its ops.  Neighbouring ops share a launch (ops.aug_stage) only where the result keeps the bits of the op-by-op chain:
        [flip] [noise] [brightness] [flip]     point ops, each rounded to fp32 inside the kernel; at most one mirror, on the read
        contrast | power | restat  [flip]      the op is driven by the record of the stage's input, so nothing may precede it in its stage
    A stage whose successor needs statistics writes the record of what it stores; after a blur or a lowres (stages of their own), or at the start,
    ops.aug_stats makes the same record."""
    cur, rec, rec_power_in, k, n = x, None, None, 0, len(plane_ops)
    while k < n:
        name = plane_ops[k][0]
        if name == "blur":
            cur, rec, k = volume.gaussian_blur3d(cur, plane_ops[k][1]), None, k + 1
            continue
        if name == "lowres":
            cur, rec, k = volume.simulate_lowres(cur, *plane_ops[k][1:]), None, k + 1
            continue
        st = {}
        if name in _STAT_OPS:
            if rec is None:
                rec = volume.aug_stats(cur)
            op = plane_ops[k]
            if name == "contrast":
                st.update(op="contrast", p=op[1], flag=op[2], rec=rec)
            elif name == "power":
                st.update(op="power", p=op[1], flag=op[2], rec=rec)
                rec_power_in = rec
            elif name == "restat":
                st.update(op="restat", mean0=op[1], std0=op[2], flag=op[3], rec=rec)
            else:
                st.update(op="restat", flag=op[1], rec=rec, rec0=rec_power_in)
            k += 1
        else:
            if name == "flip":
                st.update(flip=plane_ops[k][1], flip_first=True)
                k += 1
            if k < n and plane_ops[k][0] == "noise":
                st.update(s=plane_ops[k][1], noise=plane_ops[k][2], channel=channel)
                k += 1
            if k < n and plane_ops[k][0] == "brightness":
                st.update(mult=plane_ops[k][1])
                k += 1
        if "flip" not in st and k < n and plane_ops[k][0] == "flip":
            st.update(flip=plane_ops[k][1], flip_first=False)
            k += 1
        cur, rec = volume.aug_stage(cur, want_rec=k < n and plane_ops[k][0] in _STAT_OPS, **st)
    return cur


def intensity_augment(x, ops_list):
    """x: (C, D, H, W) CUDA float32; ops_list: tuples applied in order, a parameter being one value for all channels or a per-channel sequence in which
    None leaves that channel as it is:
        ("noise", s, n)                         x + s n; n: the normals, float64 (C, D, H, W) (numpy or tensor), or (seed, sample): Philox on the device
        ("blur", sigma)                         scipy.ndimage.gaussian_filter(mode="reflect"), 0 < sigma <= 2
        ("lowres", zoom, order_down=0, order_up=3, ignore_axes=())      ops.simulate_lowres to lowres_target_shape(plane, zoom, ignore_axes) and back
        ("brightness", m)                       x m
        ("contrast", f, preserve_range=True)    (x - mean) f + mean, clipped to the plane's range
        ("gamma", g, invert=False, retain_stats=False)      power, then restat to the mean and std of power's input
        ("power", g, invert=False)              ((x' - min) / (max - min + 1e-7))^g (max - min) + min on x' = -x when invert, negated back
        ("restat", mean0, std0, invert=False)   (x' - mean) / (std + 1e-8) std0 + mean0
        ("flip", mask)                          mirror along z / y / x for the bits 4 / 2 / 1
    Every op is computed in fp64 from the fp32 plane and the fp64 statistics of that plane and rounded to fp32 once; the result has the bits of the
    single-op calls applied one after another, eagerly and under graph replay.  No call synchronises or reads back.  Without ops: x itself."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise TypeError("intensity_augment: expected a contiguous CUDA float32 tensor (C, D, H, W), got %s %s" % (tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x))))
    channels, shape = int(x.shape[0]), tuple(int(v) for v in x.shape[1:])
    plans = [_plane_ops(ops_list, channels, c, shape) for c in range(channels)]
    if not any(plans):
        return x
    planes = [_augment_plane(x[c], plans[c], c) if plans[c] else x[c] for c in range(channels)]
    return planes[0][None] if channels == 1 else torch.stack(planes)


class IntensityAugment:
    """The batchgenerators / nnU-Net intensity stage on the device: per sample, each behind its own gate, Gaussian noise (p_noise, s in U(noise_s)),
    Gaussian blur (p_blur; every channel with p_blur_per_channel, sigma in U(blur_sigma)), brightness (p_brightness, m in U(brightness) per channel),
    contrast (p_contrast, preserve_range), gamma on the inverted image and gamma (p_gamma_inverted, p_gamma; retain_stats), and a mirror per axis
    (p_mirror).  data_dict[data_key]: (B, C, D, H, W) CUDA float32; data_dict[label_key] receives the mirror and nothing else.
    `rng`: a numpy RandomState (default: the global one).  The noise source has to be chosen when p_noise > 0:
      noise="numpy"   the normals are drawn from `rng` (rng.normal(0, 1, plane) per channel) and cross to the device
      noise="philox"  they are made on the device from (seed, n), n counting this transform's noised samples
    draw(channels, shape) -> the sample's ops for intensity_augment, drawn from `rng` in the fixed order noise gate, s, [fields]; blur gate, per channel
    (uniform <= p, sigma); brightness gate, m per channel; contrast gate, f per channel; inverted gamma gate, g per channel; gamma gate, g per channel;
    one uniform per axis z, y, x.  Every gate is drawn whatever its probability — with one exception:
    nnU-Net's simulated low resolution (p_lowres; every channel with p_lowres_per_channel, zoom in U(lowres_zoom), down with lowres_orders[0] and back up with
    lowres_orders[1], the axes in lowres_ignore_axes keeping their resolution) sits between contrast and the inverted gamma, and its draws — the gate, then
    per channel (uniform < p_lowres_per_channel, for a channel taken its zoom) — are made only when p_lowres > 0, so that a transform built without the
    argument keeps the random stream it had before the stage existed."""

    def __init__(self, data_key="data", label_key="seg", rng=None, noise=None, seed=0, p_noise=0.1, noise_s=(0.0, 0.1), p_blur=0.2, blur_sigma=(0.5, 1.0),
                 p_blur_per_channel=0.5, p_brightness=0.15, brightness=(0.75, 1.25), p_contrast=0.15, contrast=(0.75, 1.25), preserve_range=True,
                 p_gamma_inverted=0.1, p_gamma=0.3, gamma=(0.7, 1.5), retain_stats=True, p_mirror=0.5, p_lowres=0.0, lowres_zoom=(0.5, 1.0),
                 p_lowres_per_channel=0.5, lowres_orders=(0, 3), lowres_ignore_axes=()):
        if noise not in (None, "numpy", "philox"):
            raise ValueError("IntensityAugment: noise is None, 'numpy' or 'philox', got %r" % (noise,))
        if p_noise > 0 and noise is None:
            raise NotImplementedError("IntensityAugment: Gaussian noise needs a noise source: choose noise='numpy' (the normals are drawn from rng) or "
                                      "noise='philox' (made on the device from seed), or pass p_noise=0")
        if not 0 < blur_sigma[0] <= blur_sigma[1] <= volume.AUG_MAX_SIGMA:
            raise ValueError("IntensityAugment: blur takes 0 < sigma[0] <= sigma[1] <= %g, got %r" % (volume.AUG_MAX_SIGMA, blur_sigma))
        for name, (lo, hi) in (("noise_s", noise_s), ("brightness", brightness), ("contrast", contrast), ("gamma", gamma)):
            if not (np.isfinite(lo) and np.isfinite(hi) and 0 <= lo <= hi):
                raise ValueError("IntensityAugment: %s is a range 0 <= lo <= hi, got %r" % (name, (lo, hi)))
        if not (len(lowres_zoom) == 2 and 0 < lowres_zoom[0] <= lowres_zoom[1] <= 1):
            raise ValueError("IntensityAugment: lowres_zoom is a range 0 < lo <= hi <= 1, got %r" % (lowres_zoom,))
        if len(lowres_orders) != 2 or any(o not in volume.ZOOM_EDGE_ORDERS for o in lowres_orders):
            raise ValueError("IntensityAugment: lowres_orders are (down, up), each 0, 1 or 3, got %r" % (lowres_orders,))
        if any(a not in (0, 1, 2) for a in lowres_ignore_axes):
            raise ValueError("IntensityAugment: lowres_ignore_axes index the axes (0, 1, 2) of a plane, got %r" % (lowres_ignore_axes,))
        self.p_lowres, self.lowres_zoom, self.p_lowres_ch = p_lowres, tuple(lowres_zoom), p_lowres_per_channel
        self.lowres_orders, self.lowres_ignore_axes = tuple(int(o) for o in lowres_orders), tuple(int(a) for a in lowres_ignore_axes)
        self.data_key, self.label_key, self.noise, self.seed, self.n_noised = data_key, label_key, noise, int(seed), 0
        self.p_noise, self.noise_s, self.p_blur, self.blur_sigma, self.p_blur_ch = p_noise, noise_s, p_blur, blur_sigma, p_blur_per_channel
        self.p_brightness, self.brightness, self.p_contrast, self.contrast, self.preserve_range = p_brightness, brightness, p_contrast, contrast, preserve_range
        self.p_gamma_inv, self.p_gamma, self.gamma, self.retain_stats, self.p_mirror = p_gamma_inverted, p_gamma, gamma, retain_stats, p_mirror
        self.rng = rng if rng is not None else np.random

    def _range_val(self, lo, hi):
        """batchgenerators' contrast / gamma rule: below 1 and above 1 with equal probability"""
        r = self.rng
        if r.random_sample() < 0.5 and lo < 1:
            return r.uniform(lo, 1)
        return r.uniform(max(lo, 1), hi)

    def draw(self, channels, shape):
        r, ops_list = self.rng, []
        if r.uniform() < self.p_noise:
            s = r.uniform(self.noise_s[0], self.noise_s[1])
            if self.noise == "numpy":
                spec = np.stack([r.normal(0.0, 1.0, tuple(shape)) for _ in range(channels)])
            else:
                spec = (self.seed, self.n_noised)
            self.n_noised += 1
            ops_list.append(("noise", s, spec))
        if r.uniform() < self.p_blur:
            ops_list.append(("blur", [r.uniform(self.blur_sigma[0], self.blur_sigma[1]) if r.uniform() <= self.p_blur_ch else None for _ in range(channels)]))
        if r.uniform() < self.p_brightness:
            ops_list.append(("brightness", [r.uniform(self.brightness[0], self.brightness[1]) for _ in range(channels)]))
        if r.uniform() < self.p_contrast:
            ops_list.append(("contrast", [self._range_val(*self.contrast) for _ in range(channels)], self.preserve_range))
        if self.p_lowres > 0 and r.uniform() < self.p_lowres:           # the one gate that is not drawn when its probability is 0 (class docstring)
            ops_list.append(("lowres", [r.uniform(self.lowres_zoom[0], self.lowres_zoom[1]) if r.uniform() < self.p_lowres_ch else None
                                        for _ in range(channels)], self.lowres_orders[0], self.lowres_orders[1], self.lowres_ignore_axes))
        if r.uniform() < self.p_gamma_inv:
            ops_list.append(("gamma", [self._range_val(*self.gamma) for _ in range(channels)], True, self.retain_stats))
        if r.uniform() < self.p_gamma:
            ops_list.append(("gamma", [self._range_val(*self.gamma) for _ in range(channels)], False, self.retain_stats))
        mask = sum(bit for bit in (4, 2, 1) if r.uniform() < self.p_mirror)
        if mask:
            ops_list.append(("flip", mask))
        return ops_list

    def __call__(self, data_dict, params=None):
        data, seg = data_dict.get(self.data_key), data_dict.get(self.label_key)
        out_d, out_s = [], []
        for b in range(data.shape[0]):
            ops_list = params[b] if params is not None else self.draw(int(data.shape[1]), tuple(data.shape[2:]))
            out_d.append(intensity_augment(data[b].contiguous(), ops_list))
            if seg is not None:
                mask = 0
                for op in ops_list:
                    if op[0] == "flip":
                        mask ^= int(op[1])                   # mirrors compose by exclusive or
                out_s.append(volume.aug_flip(seg[b].contiguous(), mask) if mask else seg[b])
        data_dict[self.data_key] = out_d[0][None] if len(out_d) == 1 else torch.stack(out_d)
        if seg is not None:
            data_dict[self.label_key] = out_s[0][None] if len(out_s) == 1 else torch.stack(out_s)
        return data_dict


def train_sample(merge, patch_size, mask_index=None, transform=None, params=None, field="venous", shift=0, intensity=None, intensity_params=None):
    """One training sample through main_source.py:191-211 on the device: merge (D, H, W, >= 2) CUDA float32 tensor (what
    NumpyLoader_Multi_merge loads) -> (image (1, 1, P, P, P), label (1, 1, P, P, P)).  `transform`: a MySpatialTransform (None: no
    augmentation, --no_aug); `params`: its per-sample (angles, scale, centre, modified[, (alpha, sigma, noise_spec)]) instead of random draws.
    `intensity`: an IntensityAugment over (field, field + "_pancreas") applied after CenterIntensities (None: nothing more is launched);
    `intensity_params`: its ops for this sample (IntensityAugment.draw) instead of random draws."""
    img = merge[..., 0].contiguous()
    lab = merge[..., 1].contiguous()
    if mask_index is not None:
        lab = relabel(lab, mask_index)
    d = {field: img, field + "_pancreas": lab}
    d = CropResize([field], patch_size, shift=shift)(d)                 # --shift: main_target.py:81,204 (training crops only)
    d[field], d[field + "_pancreas"] = d[field][None, None], d[field + "_pancreas"][None, None]
    if transform is not None:
        d = transform(d, params=None if params is None else [params])
    d = Clip([field], new_min=-200, new_max=400)(d)
    d = CenterIntensities([field], subtrahend=100, divisor=300)(d)
    if intensity is not None:
        if (intensity.data_key, intensity.label_key) != (field, field + "_pancreas"):
            raise ValueError("train_sample: the intensity transform reads %r / %r, the sample is under %r / %r"
                             % (intensity.data_key, intensity.label_key, field, field + "_pancreas"))
        d = intensity(d, params=None if intensity_params is None else [intensity_params])
    return d[field], d[field + "_pancreas"]


# ---- patch training: foreground-oversampled windows of the unscaled volume (csrc/patch.hip; DESIGN 3.19 holds the rule) -------------------------------
class PatchSampler:
    """nnU-Net's patch sampling on the device: a batch is made of windows of `patch` voxels (a side or (D, H, W)) of the unscaled volume, and the last
    samples of every batch — sample j of B iff j >= floor(B (1 - oversample_foreground) + 0.5) — are forced to contain a uniformly chosen voxel of a
    uniformly chosen class of `classes` that is present (None: 1 .. n_class - 1).  The rule is integer throughout (ops.patch_pick).
    draw(batch_index, batch_size) -> (five words, forced): exactly one rng.randint(0, 2**32, size=5, dtype=np.uint64) per sample, forced or not, so the
    stream does not depend on the data.  `rng`: a numpy RandomState (default: the global one).
    __call__(image, label, n_class, requests) -> (image blocks (R, 1, Q, Q, Q), label blocks (R, 1, Q, Q, Q), picks int32 (R, 8)) with Q = patch +
    2 margin per axis: index, pick and gather, four launches and one small upload, nothing synchronised or read back.  Outside the volume the image reads
    `cval` and the label 0."""

    def __init__(self, patch, oversample_foreground=0.33, classes=None, margin=0, rng=None, cval=-1024.0):
        self.patch = volume._patch_sides(patch, "PatchSampler")
        p = float(oversample_foreground)
        if not 0.0 <= p <= 1.0:
            raise ValueError("PatchSampler: oversample_foreground is a share in [0, 1], got %r" % (oversample_foreground,))
        if not isinstance(margin, (int, np.integer)) or margin < 0:
            raise ValueError("PatchSampler: margin is a non-negative integer, got %r" % (margin,))
        if classes is not None:
            classes = tuple(int(c) for c in classes)
            if len(set(classes)) != len(classes) or any(not 0 <= c < volume.PATCH_MAX_CLASSES for c in classes):
                raise ValueError("PatchSampler: classes are distinct integers in [0, %d), got %r" % (volume.PATCH_MAX_CLASSES, classes))
        self.p, self.classes, self.margin, self.cval = p, classes, int(margin), float(cval)
        self.rng = rng if rng is not None else np.random

    def n_free(self, batch_size):
        """the samples of a batch before the first forced one"""
        return int(np.floor(int(batch_size) * (1.0 - self.p) + 0.5))

    def draw(self, batch_index, batch_size):
        if not 0 <= int(batch_index) < int(batch_size):
            raise ValueError("PatchSampler.draw: sample %r of a batch of %r" % (batch_index, batch_size))
        words = self.rng.randint(0, 2 ** 32, size=5, dtype=np.uint64)
        return words, bool(int(batch_index) >= self.n_free(batch_size))

    def __call__(self, image, label, n_class, requests):
        _vol(image)
        classes = tuple(range(1, int(n_class))) if self.classes is None else self.classes
        words = torch.from_numpy(np.stack([np.asarray(w, dtype=np.uint64) for w, _ in requests]).astype(np.int64)).to(label.device, non_blocking=True)
        forced = torch.tensor([int(bool(f)) for _, f in requests], dtype=torch.int32).to(label.device, non_blocking=True)
        index = volume.patch_index(label, int(n_class))
        picks = volume.patch_pick(label, index, classes, words, forced, self.patch)
        lab = label if label.dtype == torch.float32 else label.float()
        img_p, lab_p = volume.patch_gather((image, lab), (self.cval, 0.0), picks, self.patch, self.margin)
        return img_p, lab_p, picks


def train_patch(merge, patch_size, sampler, n_class, j, batch_size, mask_index=None, transform=None, params=None, field="venous", intensity=None,
                intensity_params=None, request=None):
    """train_sample's companion for patch training: sample `j` of a batch of `batch_size` cut from the UNSCALED case by `sampler` (a PatchSampler over
    patch_size) in place of CropResize -> (image (1, 1, P, P, P), label (1, 1, P, P, P), picks int32 (1, 8)).  `request`: the sample's (words, forced)
    instead of sampler.draw(j, batch_size).  `transform`: a MySpatialTransform(patch_size, random_crop=False): it resamples the gathered block of side
    P + 2 margin about its centre down to P^3, so rotation and scale read real voxels of the margin, not cval (None: no augmentation; the sampler's
    margin must then be 0).  Clip, CenterIntensities and `intensity` follow as in train_sample."""
    patch = volume._patch_sides(patch_size, "train_patch")
    if patch != sampler.patch:
        raise ValueError("train_patch: the sampler cuts %s, the sample is %s" % (sampler.patch, patch))
    if transform is None and sampler.margin:
        raise ValueError("train_patch: a margin of %d needs a spatial transform that resamples the block down to the patch" % sampler.margin)
    if transform is not None and (transform.random_crop or tuple(transform.patch_size) != patch):
        raise ValueError("train_patch: the spatial transform must be built with random_crop=False and patch_size %s" % (patch,))
    img = merge[..., 0].contiguous()
    lab = merge[..., 1].contiguous()
    if mask_index is not None:
        lab = relabel(lab, mask_index)
    if request is None:
        request = sampler.draw(j, batch_size)
    img_p, lab_p, picks = sampler(img, lab, n_class, [request])
    d = {field: img_p, field + "_pancreas": lab_p}
    if transform is not None:
        d = transform(d, params=None if params is None else [params])
    d = Clip([field], new_min=-200, new_max=400)(d)
    d = CenterIntensities([field], subtrahend=100, divisor=300)(d)
    if intensity is not None:
        if (intensity.data_key, intensity.label_key) != (field, field + "_pancreas"):
            raise ValueError("train_patch: the intensity transform reads %r / %r, the sample is under %r / %r"
                             % (intensity.data_key, intensity.label_key, field, field + "_pancreas"))
        d = intensity(d, params=None if intensity_params is None else [intensity_params])
    return d[field], d[field + "_pancreas"], picks
