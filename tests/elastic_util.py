"""The oracle of the elastic deformation tests (tests/test_host_elastic.py pins it, tests/test_gpu_elastic.py uses it): numpy and scipy only.

batchgenerators is not installed; what its augment_spatial does with do_elastic_deform is restated from its published algorithm on scipy.ndimage:

    coords = zero-centred mesh of the patch
    if do_elastic_deform and rng.uniform() < p_el_per_sample:
        a = rng.uniform(alpha[0], alpha[1]); s = rng.uniform(sigma[0], sigma[1])
        for axis in 0, 1, 2:
            off[axis] = scipy.ndimage.gaussian_filter(rng.random_sample(patch) * 2 - 1, s, mode="constant", cval=0) * a
        coords = coords + off; modified = True
    ... rotation draws and rotation, scale draws and scale, centre draws, + centre (oracle/data_cpu.py) ...
    map_coordinates(order 3 image / order 0 label, mode="constant", cval)
"""
import numpy as np
from scipy import ndimage as ndi

from oracle import data_cpu as O

M32 = 0xFFFFFFFF


def ref_philox4x32(counter4, key2):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): four 32-bit counter words, two key words -> four output words.  Plain integer arithmetic;
    Python ints give Python ints, equally shaped uint64 arrays (values below 2^32) give uint64 arrays."""
    c0, c1, c2, c3 = counter4
    k0, k1 = key2
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2              # 64-bit products of 32-bit words
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def ref_noise(patch, seed, sample):
    """(3, D, H, W) float64 in [-1, 1): key (seed low, seed high), counter (voxel low, voxel high, axis, sample low), u from the first two words"""
    v = np.arange(int(np.prod(patch)), dtype=np.uint64)
    out = np.empty((3,) + tuple(patch), np.float64)
    for axis in range(3):
        ctr = (v & np.uint64(M32), v >> np.uint64(32), np.full_like(v, axis), np.full_like(v, sample & M32))
        key = (np.full_like(v, seed & M32), np.full_like(v, (seed >> 32) & M32))
        w0, w1, _, _ = ref_philox4x32(ctr, key)
        u = ((w0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w1 >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
        out[axis] = (2.0 * u - 1.0).reshape(patch)
    return out


def ref_field(noise, alpha, sigma):
    return np.stack([ndi.gaussian_filter(np.asarray(noise[k], np.float64), sigma, mode="constant", cval=0) * alpha for k in range(3)])


def ref_draw(rng, shape, patch, dist_from_border, alpha=(0.0, 1000.0), sigma=(10.0, 13.0), p_el=1.0, elastic=True, **kw):
    """MySpatialTransform.draw's tuples from `rng` in augment_spatial's order: the elastic draws (probability, alpha, sigma, three fields) come first,
    then oracle.data_cpu.draw_spatial_params (rotation, scale, centre).  kw: scale / angle / p_rot / p_scale of draw_spatial_params."""
    el = None
    if elastic and rng.uniform() < p_el:
        a, s = rng.uniform(alpha[0], alpha[1]), rng.uniform(sigma[0], sigma[1])
        el = (a, s, np.stack([rng.random_sample(tuple(patch)) * 2 - 1 for _ in range(3)]))
    p = O.draw_spatial_params(rng, shape, patch, dist_from_border, **kw)
    out = (p["angles"], p["scale"], p["centre"], p["modified"] or el is not None)
    return out if el is None else out + (el,)


def ref_coords(field, patch, angles, scale, centre):
    """oracle.data_cpu.spatial_coords with `field` added to the zero-centred mesh: the map after the mesh is linear, so the field goes through the
    rotation and the scale on its own and is added to the coordinates of the undeformed mesh"""
    c = O.spatial_coords(patch, angles, scale, centre)
    return c + (np.asarray(field, np.float64).reshape(3, -1).T @ O.rotation_matrix(*angles)).T.reshape(c.shape) * scale


def ref_warp(img, lab, field, patch, angles, scale, centre, cval_img=-1024.0, cval_seg=0.0, perturb=None):
    """oracle.data_cpu.spatial_transform on the deformed coordinates; perturb: an array added to the coordinates (the tie check of the label test)"""
    c = ref_coords(field, patch, angles, scale, centre)
    if perturb is not None:
        c = c + perturb
    out_i = None if img is None else ndi.map_coordinates(img.astype(float), c, order=3, mode="constant", cval=cval_img).astype(img.dtype)
    out_l = None if lab is None else ndi.map_coordinates(lab.astype(float), c, order=0, mode="constant", cval=cval_seg).astype(lab.dtype)
    return out_i, out_l
