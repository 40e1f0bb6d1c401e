"""GPU: elastic deformation of the spatial augmentation (csrc/elastic.hip, data_gpu.elastic_field / warp_resample / MySpatialTransform(noise=...)) against
tests/elastic_util.py (numpy + scipy.ndimage; pinned by tests/test_host_elastic.py).  Shapes are the smallest at which each mechanism can break.
Tolerances: the noise is exact; the field is held to 1e-9 voxels absolute — fp64 sums of at most 257 products with |x| <= 1 and weights summing to 1
err by a few 1e-14, alpha <= 1000 scales that to a few 1e-11; the warped image to test_gpu_data.py's 1e-5 of the value range (same sampler, and 1e-9
voxels of coordinate difference add far less); nearest-neighbour labels to its 1e-5 share of voxels, after checking on the host that no coordinate of
the chosen seeds lies within 1e-9 of a rounding tie."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import elastic_util as EU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(random_crop=True, scale=(0.85, 1.15), do_rotation=True, angle_x=(-0.2, 0.2), angle_y=(-0.2, 0.2), angle_z=(-0.2, 0.2),
          border_mode_data="constant", border_cval_data=-1024, data_key="venous", label_key="venous_pancreas", p_scale_per_sample=1, p_rot_per_sample=1)


def _mods():
    from oracle import data_cpu as O
    from vae_segmentation_amd import data_gpu as D
    return O, D


def _close(a, b, tol):
    a, b = a.detach().cpu().double().numpy().reshape(b.shape), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b).max()
    print("max abs err %.3e (bound %.3e)" % (err, tol * max(1.0, np.abs(b).max())))
    return err <= tol * max(1.0, np.abs(b).max())


def _noise(patch, seed):
    return np.random.RandomState(seed).random_sample((3,) + tuple(patch)) * 2 - 1


def _no_ties(field, patch, angles, scale, centre, lab):
    """ref_warp's label against itself with every coordinate moved by +-1e-9: no voxel may change, or the device's 1e-9 of field error could flip one"""
    base = EU.ref_warp(None, lab, field, patch, angles, scale, centre)[1]
    return all(np.array_equal(base, EU.ref_warp(None, lab, field, patch, angles, scale, centre, perturb=e)[1]) for e in (1e-9, -1e-9))


# ---- noise -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch", [(5, 6, 7), (3, 4, 130)])
def test_philox_noise_equals_the_oracle_bit_for_bit(patch):
    from vae_segmentation_amd._lib import check, lib
    seed, sample = 2 ** 40 + 3, 7                                      # the high key word and the sample word are both live
    buf = torch.empty((3,) + patch, dtype=torch.float64, device="cuda")
    check(lib.vs_data_noise_philox(buf.data_ptr(), *patch, seed, sample, torch.cuda.current_stream().cuda_stream), "data_noise_philox")
    got = buf.cpu().numpy()
    assert np.array_equal(got, EU.ref_noise(patch, seed, sample))
    assert not np.array_equal(got, EU.ref_noise(patch, seed - 2 ** 40, sample)) and not np.array_equal(got, EU.ref_noise(patch, seed, 0))


# ---- field -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("patch,sigma,alpha", [((20, 24, 28), 10.0, 1000.0),      # radius 40 exceeds every axis; three extents catch axis mix-ups
                                               ((40, 40, 40), 1.5, 40.0),         # interior taps
                                               ((6, 7, 300), 3.0, 100.0),         # lines longer than one tile along x
                                               ((6, 300, 7), 3.0, 100.0),         # ... along y
                                               ((300, 6, 7), 3.0, 100.0),         # ... along z
                                               ((16, 16, 16), 32.0, 500.0),       # the radius cap, 128
                                               ((9, 70, 33), 0.1, 3.0)])          # radius 0; a column tile of one element
def test_elastic_field_vs_scipy(patch, sigma, alpha):
    O, D = _mods()
    noise = _noise(patch, patch[0])
    want = EU.ref_field(noise, alpha, sigma)
    for src in (noise, torch.from_numpy(noise).cuda()):
        got = D.elastic_field(patch, alpha, sigma, src)
        assert got.shape == (3,) + patch and got.dtype == torch.float64 and got.is_cuda
        err = np.abs(got.cpu().numpy() - want).max()
        print("field %s sigma %g alpha %g: max abs err %.3e voxels, max |field| %.3f" % (patch, sigma, alpha, err, np.abs(want).max()))
        assert err <= 1e-9
    zero = D.elastic_field(patch, 0.0, sigma, noise)
    assert np.array_equal(zero.cpu().numpy(), np.zeros((3,) + patch))


def test_elastic_field_from_the_philox_source_and_argument_errors():
    O, D = _mods()
    patch, seed = (12, 9, 40), 2 ** 33 + 5
    got = D.elastic_field(patch, 80.0, 2.5, (seed, 3))
    assert np.abs(got.cpu().numpy() - EU.ref_field(EU.ref_noise(patch, seed, 3), 80.0, 2.5)).max() <= 1e-9
    assert torch.equal(got, D.elastic_field(patch, 80.0, 2.5, (np.int64(seed), 3)))
    with pytest.raises(ValueError, match="sigma"):
        D.elastic_field(patch, 80.0, 33.0, (seed, 3))
    with pytest.raises(TypeError, match="float64"):
        D.elastic_field(patch, 80.0, 2.5, _noise(patch, 0).astype(np.float32))
    with pytest.raises(TypeError, match="shape"):
        D.elastic_field(patch, 80.0, 2.5, _noise((9, 12, 40), 0))


# ---- warp ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _warp_case(shape, patch, seed):
    O, _ = _mods()
    rng = np.random.RandomState(seed)
    img = (rng.randn(*shape) * 300).astype(np.float32)
    lab = (rng.rand(*shape) > 0.5).astype(np.float32)
    p = O.draw_spatial_params(np.random.RandomState(seed + 10), shape, patch, [min(patch) // 2 - 5] * 3)
    noise = _noise(patch, seed + 20)
    field = EU.ref_field(noise, 60.0, 4.0)
    ref_i, ref_l = EU.ref_warp(img, lab, field, patch, p["angles"], p["scale"], p["centre"])
    return img, lab, p, noise, field, ref_i, ref_l


@pytest.mark.parametrize("shape,patch,seed", [((40, 40, 40), (32, 32, 32), 3), ((36, 30, 44), (20, 24, 28), 4)])
def test_warp_resample_vs_scipy(shape, patch, seed):
    O, D = _mods()
    img, lab, p, noise, field, ref_i, ref_l = _warp_case(shape, patch, seed)
    print("displacements: std %.2f, max %.2f voxels" % (field.std(), np.abs(field).max()))
    assert np.abs(field).max() > 1.0                                   # the field moves voxels, or the test shows nothing
    assert _no_ties(field, patch, p["angles"], p["scale"], p["centre"], lab)
    dfield = D.elastic_field(patch, 60.0, 4.0, noise)
    args = (patch, p["angles"], p["scale"], p["centre"])
    got_i = D.warp_resample(torch.from_numpy(img).cuda(), dfield, *args, 3, -1024.0)
    got_l = D.warp_resample(torch.from_numpy(lab).cuda(), dfield, *args, 0, 0.0)
    assert _close(got_i, ref_i, 1e-5)
    share = (got_l.cpu().numpy() != ref_l).mean()
    print("label voxels that differ: %.3e" % share)
    assert share < 1e-5
    assert not np.array_equal(ref_i, O.spatial_transform(img, lab, patch, p["angles"], p["scale"], p["centre"])[0])      # ... and the field changed the picture
    zero = torch.zeros((3,) + patch, dtype=torch.float64, device="cuda")
    for vol, order, cval in ((img, 3, -1024.0), (lab, 0, 0.0)):
        v = torch.from_numpy(vol).cuda()
        assert torch.equal(D.warp_resample(v, zero, *args, order, cval), D.affine_resample(v, *args, order, cval))
    with pytest.raises(TypeError, match="displacement field"):
        D.warp_resample(torch.from_numpy(img).cuda(), dfield.float(), *args, 3, -1024.0)


# ---- transform -------------------------------------------------------------------------------------------------------------------------------
def _transform_inputs(seed=5, side=40):
    rng = np.random.RandomState(seed)
    img = (rng.randn(1, 2, side, side, side) * 300).astype(np.float32)
    lab = (rng.rand(1, 1, side, side, side) > 0.5).astype(np.float32)
    return img, lab


def test_transform_with_numpy_noise_reproduces_the_oracle_stream():
    O, D = _mods()
    img, lab = _transform_inputs()
    patch, dist, el = (32, 32, 32), [11] * 3, dict(alpha=(30.0, 60.0), sigma=(3.0, 5.0))
    prm = EU.ref_draw(np.random.RandomState(21), img.shape[2:], patch, dist, **el)
    a, s, noise = prm[4]
    field = EU.ref_field(noise, a, s)
    assert _no_ties(field, patch, prm[0], prm[1], prm[2], lab[0, 0])
    t = D.MySpatialTransform(patch, dist, do_elastic_deform=True, noise="numpy", rng=np.random.RandomState(21), **el, **KW)
    d = t({"venous": torch.from_numpy(img).cuda(), "venous_pancreas": torch.from_numpy(lab).cuda()})
    assert d["venous"].shape == (1, 2) + patch and d["venous_pancreas"].shape == (1, 1) + patch
    for c in range(2):                                                 # both channels and the label saw one and the same field
        assert _close(d["venous"][0, c], EU.ref_warp(img[0, c], None, field, patch, prm[0], prm[1], prm[2])[0], 1e-5)
    assert (d["venous_pancreas"][0, 0].cpu().numpy() != EU.ref_warp(None, lab[0, 0], field, patch, prm[0], prm[1], prm[2])[1]).mean() < 1e-5


def test_transform_with_philox_noise_is_reproducible_eagerly_and_under_graph_replay():
    O, D = _mods()
    img, lab = _transform_inputs()
    patch, dist, el = (32, 32, 32), [11] * 3, dict(alpha=(30.0, 60.0), sigma=(3.0, 5.0))
    x, y = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()

    def make():
        return D.MySpatialTransform(patch, dist, do_elastic_deform=True, noise="philox", seed=2 ** 35 + 9, rng=np.random.RandomState(4), **el, **KW)

    def run(t, params=None):
        d = t({"venous": x, "venous_pancreas": y}, params=params)
        return d["venous"], d["venous_pancreas"]

    t1, t2 = make(), make()
    a1, b1 = run(t1)
    a2, b2 = run(t2)
    assert torch.equal(a1, a2) and torch.equal(b1, b2)                 # fresh transforms, same seed: the same bits
    a3, _ = run(t1)
    assert not torch.equal(a1, a3)                                     # the second sample of one transform differs from its first
    # the same parameters with the field of sample 0 and of sample 1: only the field differs
    prm = make().draw(img.shape[2:])
    assert prm[4][2] == (2 ** 35 + 9, 0)
    other = prm[:4] + ((prm[4][0], prm[4][1], (2 ** 35 + 9, 1)),)
    e0, l0 = run(make(), [prm])
    assert torch.equal(e0, a1) and not torch.equal(e0, run(make(), [other])[0])
    # eager == replayed from a captured graph; the host draws were made before the capture and travel as params
    t = make()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(t, [prm])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_img, g_lab = run(t, [prm])
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_img, e0) and torch.equal(g_lab, l0)


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------------
def test_train_sample_with_an_elastic_transform_vs_oracle_chain():
    O, D = _mods()
    shape, patch = (60, 70, 50), (32, 32, 32)
    rng = np.random.RandomState(7)
    merge = np.zeros(shape + (2,), np.float32)
    merge[..., 0] = rng.randn(*shape) * 300 + 50
    merge[18:42, 24:56, 10:30, 1] = rng.randint(1, 4, size=(24, 32, 20))
    mask_index = [[[1, 2, 3], 1]]
    p = O.draw_spatial_params(np.random.RandomState(5), patch, patch, [11] * 3)
    noise, alpha, sigma = _noise(patch, 8), 45.0, 4.0
    img, lab = O.load_merge(merge, mask_index)
    img, lab = O.crop_resize(img, lab, patch)
    field = EU.ref_field(noise, alpha, sigma)
    ref_i, ref_l = EU.ref_warp(img, lab, field, patch, p["angles"], p["scale"], p["centre"])
    ref_i = O.center_intensities(O.clip(ref_i)).astype(np.float32)
    t = D.MySpatialTransform(patch, [11] * 3, do_elastic_deform=True, noise="numpy", **KW)
    got_i, got_l = D.train_sample(torch.from_numpy(merge).cuda(), patch, mask_index, t, (p["angles"], p["scale"], p["centre"], True, (alpha, sigma, noise)))
    assert got_i.shape == (1, 1) + patch and got_l.shape == (1, 1) + patch
    assert _close(got_i[0, 0], ref_i, 2e-5)
    share = (got_l[0, 0].cpu().numpy() != ref_l.astype(np.float32)).mean()
    print("label voxels that differ: %.3e" % share)
    assert share < 1e-4
    # the 4-tuple still means: not deformed
    plain_i, _ = D.train_sample(torch.from_numpy(merge).cuda(), patch, mask_index, t, (p["angles"], p["scale"], p["centre"], True))
    assert _close(plain_i[0, 0], O.train_sample(merge, patch, p, mask_index)[0], 2e-5)


# ---- entry point -----------------------------------------------------------------------------------------------------------------------------
# What `main_source.py real -M seg_train --real_data --size 32 -b 1 -E 1 ...` below prints as its first step's loss on the commit before --aug_elastic
# existed (torch seeded with 0 before the model is built, deterministic build of the library, the cases of _cases()).  Four decimals are printed; a
# last-bit difference can move the last printed digit by one, hence 1.5e-4.
PARENT_FIRST_STEP = [0.4285]                                           # "[  1,   1] loss: dice_loss 0.4285"
RUNNER = ("import sys, torch; torch.manual_seed(0); import main_source; from vae_segmentation_amd import driver; "
          "driver.run(main_source.parse(sys.argv[1:]), side='source')")


def _cases(tmp_path):
    rng = np.random.RandomState(0)
    (tmp_path / "data").mkdir(); (tmp_path / "lists").mkdir()
    names = []
    for i, shape in enumerate([(40, 48, 44), (52, 40, 46), (44, 44, 60)]):
        merge = np.zeros(shape + (2,), np.float32)
        merge[..., 0] = rng.randn(*shape) * 250 + 40
        merge[10:30, 12:34, 8:30, 1] = 1
        np.save(tmp_path / "data" / ("case%d_merge.npy" % i), merge)
        names.append("case%d_merge.npy" % i)
    json.dump({"NIH_train": names[:2], "NIH_val": names[2:]}, open(tmp_path / "lists" / "Multi_all.json", "w"))


def _step_losses(out):
    """the numbers of every '[epoch, step] loss: name value, ...' line"""
    return [[float(v) for v in re.findall(r" (-?\d+\.\d{4}|nan|inf)", ln.split("loss:")[1])] for ln in out.splitlines() if "loss:" in ln]


def test_real_data_run_with_aug_elastic(tmp_path):
    _cases(tmp_path)
    common = ["real", "-M", "seg_train", "--real_data", "-R", str(tmp_path / "data"), "-V", str(tmp_path / "data"), "--size", "32", "-b", "1", "-E", "1",
              "--eval_epoch", "1", "--save_epoch", "1", "--display_freq", "1", "--max_iters", "2"]
    env = dict(os.environ, PYTHONPATH=REPO, VS_DETERMINISTIC="1")
    outs = {}
    for tag, extra in (("elastic", ["--aug_elastic", "1.0"]), ("plain", [])):
        r = subprocess.run([sys.executable, "-c", RUNNER] + common + extra, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Finished Training" in r.stdout and r.stdout.count("loss:") >= 2
        outs[tag] = _step_losses(r.stdout)
        print(tag, outs[tag])
        assert all(np.isfinite(v) for step in outs[tag] for v in step) and all(len(step) >= 1 for step in outs[tag])
    assert outs["elastic"][0] != outs["plain"][0]                      # the flag reached the samples
    assert len(outs["plain"][0]) == len(PARENT_FIRST_STEP)
    assert all(abs(a - b) <= 1.5e-4 for a, b in zip(outs["plain"][0], PARENT_FIRST_STEP))
