"""GPU: patch training — the position index, the ranked pick and the gather of csrc/patch.hip (ops.patch_index / patch_pick / patch_gather),
data_gpu.PatchSampler / train_patch and --train_patches — against tests/patch_util.py, which tests/test_host_patch.py pins.

The feature is integers and copies: every comparison is for equality, there is no tolerance anywhere in this file."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import patch_util as PU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = pytest.mark.parametrize("lib_mode", ["det", "atomic"], indirect=True)
SHAPES = [(1, 1, 1), (1, 1, 2), (5, 7, 9), (3, 17, 241), (17, 16, 257), (40, 48, 56)]
CHUNKED = (17, 16, 257)                                                 # 17 chunks and a partial one
BIG = (40, 48, 56)
NC = 3
FULL = 2 ** 32 - 1


def _mods():
    from vae_segmentation_amd import data_gpu as D
    from vae_segmentation_amd import ops
    assert all(hasattr(ops, n) for n in ("patch_index", "patch_pick", "patch_gather", "PATCH_CHUNK"))
    assert hasattr(D, "PatchSampler") and hasattr(D, "train_patch")
    return D, ops


@functools.lru_cache(maxsize=None)
def _label(shape, kind, dtype="float32", n_class=NC):
    from vae_segmentation_amd import ops
    x = PU.label_volume(shape, kind, n_class, dtype=np.dtype(dtype), chunk=ops.PATCH_CHUNK)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _odd_bytes(shape):
    """a uint8 label with values that belong to no class: n_class itself and 255"""
    x = np.array(_label(shape, "random", "uint8"))
    rng = np.random.RandomState(9)
    bad = rng.rand(*shape) < 0.2
    x[bad] = rng.choice([NC, 255], size=int(bad.sum())).astype(np.uint8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _image(shape, seed=0):
    x = np.round(np.random.RandomState(seed).randn(*shape) * 250.0 + 40.0).astype(np.float32)
    x.setflags(write=False)
    return x


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True, order="C")).cuda()


def _words(n, seed):
    """(0, ..., 0), (2^32 - 1, ...) and n seeded random requests, as an int64 array"""
    rng = np.random.RandomState(seed)
    return np.concatenate([np.zeros((1, 5), np.int64), np.full((1, 5), FULL, np.int64), rng.randint(0, 2 ** 32, size=(n, 5), dtype=np.uint64).astype(np.int64)])


def _pick(ops, lab, n_class, classes, words, forced, patch, index=None):
    labd = _dev(lab)
    index = ops.patch_index(labd, n_class) if index is None else index
    return ops.patch_pick(labd, index, classes, _dev(words), _dev(np.asarray(forced, np.int32)), patch)


# ---- index -------------------------------------------------------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("shape", SHAPES)
def test_index_equals_the_oracles_table(shape, lib_mode):
    D, ops = _mods()
    chunk = ops.PATCH_CHUNK
    assert int(np.prod(CHUNKED)) // chunk == 17 and int(np.prod(CHUNKED)) % chunk and int(np.prod(BIG)) > 8 * chunk
    labels = [(kind, _label(shape, kind, dt)) for dt in ("float32", "uint8") for kind in ("random", "background", "one", "first", "last", "tail")]
    labels += [("odd", _label(shape, "odd")), ("odd bytes", _odd_bytes(shape))]
    if int(np.prod(shape)) > 64:
        flat = labels[-2][1].ravel()
        assert np.isnan(flat).any() and (flat == 0.5).any() and (flat == NC).any()
    for kind, lab in labels:
        got = ops.patch_index(_dev(lab), NC)
        want = PU.ref_index(lab, NC, chunk)
        assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (shape, kind, lab.dtype)
    for n_class in (1, 8):                                              # the least and the most classes a table holds
        lab = _label(shape, "random", "float32", 8)
        assert np.array_equal(ops.patch_index(_dev(lab), n_class).cpu().numpy(), PU.ref_index(lab, n_class, chunk)), (shape, n_class)


# ---- pick --------------------------------------------------------------------------------------------------------------------------------------
def _patches(shape):
    """smaller than the volume, equal to it, larger on one axis, larger on all"""
    return [tuple(max(1, s // 2) for s in shape), tuple(shape), (shape[0], shape[1] + 3, shape[2]), (shape[0] + 2, shape[1] + 3, shape[2] + 5)]


@BOTH
@pytest.mark.parametrize("shape", SHAPES)
def test_picks_equal_the_oracles(shape, lib_mode):
    D, ops = _mods()
    words = _words(64, seed=sum(shape))
    words = np.concatenate([words, words])                              # every request once forced and once free
    forced = [1] * 66 + [0] * 66
    cases = [("random", "float32", (1, 2), p) for p in _patches(shape)]
    cases += [("random", "uint8", (2, 1), _patches(shape)[0]),
              ("random", "float32", (2,), _patches(shape)[0]),          # a class list that is a subset
              ("random", "float32", (0, 1, 2), _patches(shape)[2]),     # the background is a class like any other when it is asked for
              ("last", "float32", (1, 2), _patches(shape)[0]),          # n_k = 1, class 2 absent
              ("first", "uint8", (1,), _patches(shape)[3]),
              ("tail", "float32", (1,), _patches(shape)[0]),
              ("odd", "float32", (1, 2), _patches(shape)[0]),
              ("background", "float32", (1, 2), _patches(shape)[0])]    # forced with no class present: a free origin, class -1
    for kind, dt, classes, patch in cases:
        lab = _label(shape, kind, dt)
        got = _pick(ops, lab, NC, classes, words, forced, patch).cpu().numpy()
        want = PU.ref_picks(lab, NC, classes, words, forced, patch)
        assert got.dtype == np.int32 and got.shape == (132, 8)
        assert np.array_equal(got, want), (shape, kind, dt, classes, patch, got[got != want][:8], want[got != want][:8])
        if kind == "background":
            assert (got[:, 3:7] == -1).all()
        if kind == "last":
            assert (got[:66, 3] == 1).all() and (got[:66, 4:7] == np.array(shape) - 1).all() and (got[66:, 3] == -1).all()


def test_stratified_words_pick_every_voxel_of_a_class_equally_often():
    D, ops = _mods()
    lab = _label(CHUNKED, "sparse64")
    where = np.flatnonzero(lab.ravel() == 2)
    assert where.size == 64 and len(set((where // ops.PATCH_CHUNK).tolist())) >= 3
    words = np.zeros((4096, 5), np.int64)
    words[:, 1] = np.arange(4096, dtype=np.int64) * 2 ** 20
    got = _pick(ops, lab, NC, (1, 2), words, [1] * 4096, (8, 8, 8)).cpu().numpy()
    assert (got[:, 3] == 2).all()
    lin = (got[:, 4].astype(np.int64) * CHUNKED[1] + got[:, 5]) * CHUNKED[2] + got[:, 6]
    assert np.array_equal(lin, where[(words[:, 1] * 64) >> 32])         # rank order is voxel order ...
    values, counts = np.unique(lin, return_counts=True)
    assert np.array_equal(values, where) and counts.tolist() == [64] * 64          # ... and every voxel comes out exactly 64 times


# ---- gather ------------------------------------------------------------------------------------------------------------------------------------
def _picks_of(origins):
    rows = np.zeros((len(origins), 8), np.int32)
    rows[:, :3] = origins
    rows[:, 3:7] = -1
    return rows


@BOTH
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_equals_pad_and_slice(shape, lib_mode):
    D, ops = _mods()
    vols = [_image(shape, seed) for seed in range(4)]
    cvals = [-1024.0, 0.0, 7.5, -0.25]
    devs = [_dev(v) for v in vols]
    lab = _label(shape, "random")
    words = _words(3, seed=1)
    for patch in _patches(shape):
        origins = PU.ref_picks(lab, NC, (1, 2), words, [1, 0, 1, 0, 1], patch)[:, :3]         # the oracle's origins: R = 5
        origins = np.concatenate([origins, [[-2, 1, -3], [shape[0] - 1, shape[1] + 2, shape[2] - 2], [0, 0, 5], [1, -1, 3], [0, 0, -patch[2] - 4]]])
        assert (origins[:, 2] % 4 != 0).any()
        for margin in (0, 3):
            for n_src, rows in ((2, origins[:5]), (4, origins[5:]), (2, origins[6:7])):          # R = 5, 5 and 1
                got = ops.patch_gather(devs[:n_src], cvals[:n_src], _dev(_picks_of(rows)), patch, margin)
                assert len(got) == n_src
                for s in range(n_src):
                    assert got[s].dtype == torch.float32 and tuple(got[s].shape) == (len(rows), 1) + tuple(p + 2 * margin for p in patch)
                    want = np.stack([PU.ref_gather(vols[s], o, patch, margin, cvals[s]) for o in rows])[:, None]
                    assert np.array_equal(got[s].cpu().numpy().view(np.int32), want.view(np.int32)), (shape, patch, margin, n_src, s)
    far = _picks_of([[2 ** 31 - 1, 0, 0], [0, -2 ** 31, 0], [0, 0, 2 ** 31 - 1], [0, 0, -2 ** 31]])      # any integer is an origin: nothing is read
    got = ops.patch_gather(devs[:1], [3.0], _dev(far), 4, 1)[0]
    assert tuple(got.shape) == (4, 1, 6, 6, 6) and bool((got == 3.0).all())


# ---- graph -------------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_bit_for_bit():
    D, ops = _mods()
    lab, img = _dev(_label(BIG, "random")), _dev(_image(BIG))
    requests = [(_words(6, seed), np.random.RandomState(seed).randint(0, 2, size=8).astype(np.int32)) for seed in (1, 2, 3)]
    patch, margin = (16, 20, 12), 3

    def run(label, words, forced):
        index = ops.patch_index(label, NC)
        picks = ops.patch_pick(label, index, (1, 2), words, forced, patch)
        return index, picks, ops.patch_gather((img, label), (-1024.0, 0.0), picks, patch, margin)

    eager = [run(lab, _dev(w), _dev(f)) for w, f in requests]
    s_lab, s_words, s_forced = lab.clone(), _dev(requests[0][0]), _dev(requests[0][1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(s_lab, s_words, s_forced)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # a synchronising call would end the capture with an error
        index, picks, blocks = run(s_lab, s_words, s_forced)
    for (w, f), (e_index, e_picks, e_blocks) in zip(requests, eager):
        s_words.copy_(_dev(w))
        s_forced.copy_(_dev(f))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(index, e_index) and torch.equal(picks, e_picks)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(blocks, e_blocks))
        assert np.array_equal(picks.cpu().numpy(), PU.ref_picks(_label(BIG, "random"), NC, (1, 2), w, f, patch))


# ---- train_patch -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _merge():
    merge = np.zeros(BIG + (2,), np.float32)
    merge[..., 0] = _image(BIG, seed=5)
    merge[10:30, 12:34, 8:30, 1] = 1
    merge[14:20, 30:40, 40:50, 1] = 2                                   # relabelled to 0 below: pan_index 1
    merge.setflags(write=False)
    return merge


MASK_INDEX = [[0, 0], [1, 1]]


def _relabelled(merge):
    lab = np.zeros(merge.shape[:3], np.float32)
    lab[merge[..., 1] == 1] = 1
    return lab


def _window(D, img):
    d = D.CenterIntensities(["venous"], subtrahend=100, divisor=300)(D.Clip(["venous"], new_min=-200, new_max=400)({"venous": img}))
    return d["venous"]


def test_train_patch_without_a_transform_is_cut_clip_centre():
    D, ops = _mods()
    merge = _merge()
    lab = _relabelled(merge)
    patch = (16, 24, 20)
    for seed, forced in ((1, True), (2, False), (3, True)):
        words = np.random.RandomState(seed).randint(0, 2 ** 32, size=5, dtype=np.uint64)
        sampler = D.PatchSampler(patch, 0.33, rng=np.random.RandomState(0))
        img, seg, picks = D.train_patch(_dev(merge), patch, sampler, 2, 0, 1, MASK_INDEX, request=(words, forced))
        want = PU.ref_pick(lab, 2, (1,), words, forced, patch)
        assert picks.cpu().numpy().tolist() == [want] and (want[3] == 1) == forced
        want_img = _window(D, _dev(PU.ref_gather(merge[..., 0], want[:3], patch, 0, -1024.0))[None, None])
        assert tuple(img.shape) == (1, 1) + patch and torch.equal(img.view(torch.int32), want_img.view(torch.int32))
        assert np.array_equal(seg.cpu().numpy()[0, 0], PU.ref_gather(lab, want[:3], patch, 0, 0.0))
    with pytest.raises(ValueError, match="margin"):
        D.train_patch(_dev(merge), patch, D.PatchSampler(patch, margin=3), 2, 0, 1, MASK_INDEX)
    with pytest.raises(ValueError, match="sampler"):
        D.train_patch(_dev(merge), (16, 16, 16), sampler, 2, 0, 1, MASK_INDEX)


def _spatial(D, patch, random_crop=False):
    return D.MySpatialTransform(patch, [p // 2 - 5 for p in patch], random_crop=random_crop, scale=(0.85, 1.15), do_elastic_deform=False, do_rotation=True,
                                angle_x=(-0.2, 0.2), angle_y=(-0.2, 0.2), angle_z=(-0.2, 0.2), border_mode_data="constant", border_cval_data=-1024,
                                data_key="venous", label_key="venous_pancreas", rng=np.random.RandomState(7))


def test_train_patch_with_a_transform_resamples_the_oracles_block():
    D, ops = _mods()
    merge = _merge()
    lab = _relabelled(merge)
    patch, margin = (16, 16, 16), 3
    q = tuple(p + 2 * margin for p in patch)
    words = np.random.RandomState(4).randint(0, 2 ** 32, size=5, dtype=np.uint64)
    params = ((0.15, -0.1, 0.05), 1.1, tuple(s / 2.0 - 0.5 for s in q), True)
    sampler = D.PatchSampler(patch, 0.33, margin=margin)
    img, seg, picks = D.train_patch(_dev(merge), patch, sampler, 2, 0, 1, MASK_INDEX, transform=_spatial(D, patch), params=params, request=(words, True))
    want = PU.ref_pick(lab, 2, (1,), words, True, patch)
    assert picks.cpu().numpy().tolist() == [want]
    block = {"venous": _dev(PU.ref_gather(merge[..., 0], want[:3], patch, margin, -1024.0))[None, None],
             "venous_pancreas": _dev(PU.ref_gather(lab, want[:3], patch, margin, 0.0))[None, None]}
    assert tuple(block["venous"].shape) == (1, 1) + q
    ref = _spatial(D, patch)(block, params=[params])
    assert tuple(img.shape) == (1, 1) + patch
    assert torch.equal(img.view(torch.int32), _window(D, ref["venous"]).view(torch.int32)) and torch.equal(seg, ref["venous_pancreas"])
    drawn = D.train_patch(_dev(merge), patch, sampler, 2, 0, 1, MASK_INDEX, transform=_spatial(D, patch), request=(words, True))      # its own draws: about the centre
    assert tuple(drawn[0].shape) == (1, 1) + patch and bool(torch.isfinite(drawn[0]).all())
    with pytest.raises(ValueError, match="random_crop"):
        D.train_patch(_dev(merge), patch, sampler, 2, 0, 1, MASK_INDEX, transform=_spatial(D, patch, random_crop=True))


def test_the_last_sample_of_a_batch_of_two_is_forced_onto_the_foreground():
    D, ops = _mods()
    merge = _merge()
    lab = _relabelled(merge)
    patch = (12, 12, 12)
    sampler = D.PatchSampler(patch, 0.33, rng=np.random.RandomState(21))
    ref = np.random.RandomState(21)
    for _ in range(4):                                                  # four batches of two
        free = D.train_patch(_dev(merge), patch, sampler, 2, 0, 2, MASK_INDEX)
        forced = D.train_patch(_dev(merge), patch, sampler, 2, 1, 2, MASK_INDEX)
        w0, w1 = (ref.randint(0, 2 ** 32, size=5, dtype=np.uint64) for _ in range(2))
        p0, p1 = free[2].cpu().numpy()[0], forced[2].cpu().numpy()[0]
        assert p0.tolist() == PU.ref_pick(lab, 2, (1,), w0, False, patch) and p0[3] == -1
        assert p1.tolist() == PU.ref_pick(lab, 2, (1,), w1, True, patch) and p1[3] == 1
        local = p1[4:7] - p1[:3]
        assert (local >= 0).all() and (local < 12).all() and float(forced[1][0, 0, local[0], local[1], local[2]]) == 1.0


# ---- the entry points --------------------------------------------------------------------------------------------------------------------------
RUNNER = ("import sys, torch; torch.manual_seed(0); import main_source; from vae_segmentation_amd import driver; "
          "driver.run(main_source.parse(sys.argv[1:]), side='source')")


def _cases(tmp_path):
    rng = np.random.RandomState(0)
    (tmp_path / "data").mkdir(); (tmp_path / "lists").mkdir()
    names = []
    for i, shape in enumerate([(40, 48, 56), (44, 40, 52), (48, 52, 40)]):
        merge = np.zeros(shape + (2,), np.float32)
        merge[..., 0] = np.round(rng.randn(*shape) * 250 + 40)
        merge[10:30, 12:34, 8:30, 1] = 1
        np.save(tmp_path / "data" / ("case%d_merge.npy" % i), merge)
        names.append("case%d_merge.npy" % i)
    json.dump({"NIH_train": names[:2], "NIH_val": names[2:]}, open(tmp_path / "lists" / "Multi_all.json", "w"))
    return names


def test_main_source_trains_on_patches(tmp_path):
    _cases(tmp_path)
    args = ["patches", "-M", "seg_train", "--real_data", "--train_patches", "--max_iters", "2", "--size", "32", "-R", str(tmp_path / "data"), "-V",
            str(tmp_path / "data"), "-b", "1", "-E", "1", "--eval_epoch", "1", "--save_epoch", "1", "--display_freq", "1"]
    r = subprocess.run([sys.executable, "-c", RUNNER] + args, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO, VS_DETERMINISTIC="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [[float(v) for v in re.findall(r" (-?\d+\.\d{4}|nan|inf)", ln.split("loss:")[1])] for ln in r.stdout.splitlines() if "loss:" in ln]
    print(losses)
    assert "Finished Training" in r.stdout and len(losses) >= 2 and all(len(step) >= 1 and all(np.isfinite(v) for v in step) for step in losses)


def test_loader_cuts_patches_only_with_the_flag(tmp_path):
    import main_source
    from vae_segmentation_amd import driver
    D, ops = _mods()
    names = _cases(tmp_path)
    root = str(tmp_path / "data")
    common = ["run", "--real_data", "-R", root, "--size", "32", "-b", "2"]
    with pytest.raises(SystemExit):
        main_source.parse(["run", "--train_patches"])                   # the flag needs --real_data

    def loader(extra, train=True, seed=4):
        return driver.DeviceCaseLoader(names[:2], root, main_source.parse(common + extra), 2, train, False, seed=seed)

    on = loader(["--train_patches"])
    assert isinstance(on.sampler, D.PatchSampler) and on.sampler.patch == (32, 32, 32) and on.sampler.p == 0.33 and on.sampler.margin == 16
    assert on.transform is not None and on.transform.random_crop is False
    batches = list(on)
    assert len(batches) == 1 and tuple(batches[0][driver.IMG_KEY].shape) == (2, 1, 32, 32, 32) and bool(torch.isfinite(batches[0][driver.IMG_KEY]).all())
    assert float(batches[0][driver.LABEL_KEY][1].max()) == 1.0          # sample 1 of 2 is forced: its patch holds foreground (before the transform, and a
    #                                                                     rotation of at most 0.2 rad and a scale within 15 % about the centre keep a 20-voxel organ in view)
    # the generators: the sampler's own stream took one draw per sample, the spatial transform's stream exactly its own two draws
    ref = np.random.RandomState(4 + 900)
    for _ in range(2):
        ref.randint(0, 2 ** 32, size=5, dtype=np.uint64)
    assert all(np.array_equal(a, b) for a, b in zip(on.sampler.rng.get_state()[1:], ref.get_state()[1:]))
    twin = _spatial(D, (32, 32, 32))
    twin.rng = np.random.RandomState(4)
    for _ in range(2):
        twin.draw((64, 64, 64))
    assert all(np.array_equal(a, b) for a, b in zip(on.transform.rng.get_state()[1:], twin.rng.get_state()[1:]))
    opts = loader(["--train_patches", "--patch_fg", "1.0", "--patch_margin", "4", "--no_aug"])
    assert opts.sampler.p == 1.0 and opts.sampler.margin == 0 and opts.transform is None
    for batch in opts:
        assert (batch[driver.LABEL_KEY].amax(dim=(1, 2, 3, 4)) == 1.0).all()            # every sample forced
    assert loader(["--train_patches", "--patch_margin", "4"]).sampler.margin == 4
    val = loader(["--train_patches"], train=False)                      # validation is unchanged: CropResize
    assert val.sampler is None
    # without the flag: what train_sample gives when called directly, bit for bit, and nothing is built
    for extra in ([], ["--no_aug"]):
        off = loader(extra)
        assert off.sampler is None
        twin = loader(extra).transform                                  # the same seed: the same draws
        for batch in off:
            for k in range(2):
                merge = torch.from_numpy(np.load(tmp_path / "data" / names[k]).astype(np.float32)).cuda()
                img, lab = D.train_sample(merge, (32,) * 3, off.mask_index, twin, field=driver.IMG_KEY)
                assert torch.equal(batch[driver.IMG_KEY][k:k + 1], img) and torch.equal(batch[driver.LABEL_KEY][k:k + 1], lab)
    vimg, vlab = D.train_sample(torch.from_numpy(np.load(tmp_path / "data" / names[0]).astype(np.float32)).cuda(), (32,) * 3, val.mask_index, None,
                                field=driver.IMG_KEY)
    first = next(iter(val))
    assert torch.equal(first[driver.IMG_KEY][:1], vimg) and torch.equal(first[driver.LABEL_KEY][:1], vlab)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_answered_before_a_launch():
    from vae_segmentation_amd import _lib
    D, ops = _mods()
    lab = _dev(_label((5, 7, 9), "random"))
    img = _dev(_image((5, 7, 9)))
    index = ops.patch_index(lab, NC)
    words, forced = _dev(_words(2, 0)), _dev(np.array([1, 0, 1, 0], np.int32))
    picks = ops.patch_pick(lab, index, (1, 2), words, forced, 4)
    with pytest.raises(TypeError):
        ops.patch_index(lab.double(), NC)
    for bad in (0, 9, 2.0):
        with pytest.raises(ValueError, match="n_class"):
            ops.patch_index(lab, bad)
    with pytest.raises(ValueError):
        ops.patch_index(lab[:, :, :0], NC)
    with pytest.raises(ValueError, match="contiguous"):
        ops.patch_index(lab.permute(2, 1, 0), NC)
    for bad in ((1, 1), (3,), (-1,), (1.5,)):
        with pytest.raises(ValueError, match="classes"):
            ops.patch_pick(lab, index, bad, words, forced, 4)
    with pytest.raises(ValueError, match="index"):
        ops.patch_pick(lab, index[:1], (1,), words, forced, 4)
    with pytest.raises(ValueError, match="words"):
        ops.patch_pick(lab, index, (1,), words[:, :4], forced, 4)
    with pytest.raises(ValueError, match="forced"):
        ops.patch_pick(lab, index, (1,), words, forced[:3], 4)
    for bad in (0, (4, 4), (4, 0, 4), 2.5):
        with pytest.raises(ValueError, match="patch"):
            ops.patch_pick(lab, index, (1,), words, forced, bad)
    with pytest.raises(ValueError):
        ops.patch_gather([], [], picks, 4)
    with pytest.raises(ValueError):
        ops.patch_gather([img] * 5, [0.0] * 5, picks, 4)
    with pytest.raises(ValueError):
        ops.patch_gather([img], [float("nan")], picks, 4)
    with pytest.raises(ValueError):
        ops.patch_gather([img, img[:4]], [0.0, 0.0], picks, 4)
    with pytest.raises(TypeError):
        ops.patch_gather([img.double()], [0.0], picks, 4)
    with pytest.raises(ValueError, match="margin"):
        ops.patch_gather([img], [0.0], picks, 4, margin=-1)
    with pytest.raises(ValueError, match="picks"):
        ops.patch_gather([img], [0.0], picks[:, :7], 4)
    # the C entry points: the library's codes, from the host checks (the pointers are never followed)
    lib = _lib.lib
    EINVAL, ESHAPE, EDTYPE, EALIGN = -1, -2, -3, -5
    w32 = words.to(torch.int32)
    out = torch.empty((1, 4, 4, 4, 4), device="cuda")
    assert lib.vs_patch_chunk() == ops.PATCH_CHUNK
    assert lib.vs_patch_index_bytes(5, 7, 9, NC) == 2 * NC * 4 and lib.vs_patch_index_bytes(17, 16, 257, 8) == 19 * 8 * 4
    assert lib.vs_patch_index_bytes(0, 7, 9, NC) == 0 and lib.vs_patch_index_bytes(5, 7, 9, 9) == 0 and lib.vs_patch_index_bytes(2048, 1024, 1024, NC) == 0

    def index_call(lp=lab.data_ptr(), dt=0, d=5, h=7, w=9, nc=NC, tp=index.data_ptr()):
        return lib.vs_patch_index(lp, dt, d, h, w, nc, tp, None)

    assert index_call(lp=None) == EINVAL and index_call(tp=None) == EINVAL and index_call(nc=0) == EINVAL and index_call(nc=9) == EINVAL
    assert index_call(dt=2) == EDTYPE and index_call(d=0) == ESHAPE and index_call(d=2048, h=1024, w=1024) == ESHAPE
    assert index_call(lp=lab.data_ptr() + 2) == EALIGN and index_call(tp=index.data_ptr() + 2) == EALIGN

    def pick_call(lp=lab.data_ptr(), dt=0, tp=index.data_ptr(), nc=NC, ns=2, cl=1 | (2 << 3), wp=w32.data_ptr(), fp=forced.data_ptr(), r=4, d=5, h=7, w=9,
                  p=(4, 4, 4), pp=picks.data_ptr()):
        return lib.vs_patch_pick(lp, dt, tp, nc, ns, cl, wp, fp, r, d, h, w, p[0], p[1], p[2], pp, None)

    for k in ("lp", "tp", "wp", "fp", "pp"):
        assert pick_call(**{k: None}) == EINVAL, k
    assert pick_call(r=0) == EINVAL and pick_call(p=(4, 0, 4)) == EINVAL and pick_call(ns=9) == EINVAL and pick_call(ns=-1) == EINVAL
    assert pick_call(cl=2 | (1 << 3)) == EINVAL and pick_call(cl=1 | (1 << 3)) == EINVAL and pick_call(cl=1 | (3 << 3)) == EINVAL          # descending, repeated, >= n_class
    assert pick_call(ns=1, cl=1 | (2 << 3)) == EINVAL                   # bits above the list
    assert pick_call(dt=7) == EDTYPE and pick_call(w=0) == ESHAPE and pick_call(d=2048, h=1024, w=1024) == ESHAPE
    assert pick_call(pp=picks.data_ptr() + 4) == EALIGN and pick_call(wp=w32.data_ptr() + 2) == EALIGN and pick_call(tp=index.data_ptr() + 1) == EALIGN

    def gather_call(s0=img.data_ptr(), s1=None, c0=0.0, n=1, pk=picks.data_ptr(), r=1, d=5, h=7, w=9, p=(4, 4, 4), m=0, op=out.data_ptr()):
        return lib.vs_patch_gather(s0, s1, None, None, c0, 0.0, 0.0, 0.0, n, pk, r, d, h, w, p[0], p[1], p[2], m, op, None)

    assert gather_call(s0=None) == EINVAL and gather_call(n=2) == EINVAL and gather_call(n=0) == EINVAL and gather_call(n=5) == EINVAL
    assert gather_call(pk=None) == EINVAL and gather_call(op=None) == EINVAL and gather_call(r=0) == EINVAL and gather_call(m=-1) == EINVAL
    assert gather_call(p=(0, 4, 4)) == EINVAL and gather_call(c0=float("nan")) == EINVAL and gather_call(op=img.data_ptr()) == EINVAL
    assert gather_call(h=0) == ESHAPE and gather_call(d=2048, h=1024, w=1024) == ESHAPE and gather_call(p=(2048, 1024, 1024)) == ESHAPE
    assert gather_call(m=2 ** 30) == ESHAPE
    assert gather_call(s0=img.data_ptr() + 4) == EALIGN and gather_call(op=out.data_ptr() + 8) == EALIGN and gather_call(pk=picks.data_ptr() + 4) == EALIGN
    torch.cuda.synchronize()
    assert torch.equal(index, ops.patch_index(lab, NC)) and torch.equal(picks, ops.patch_pick(lab, index, (1, 2), words, forced, 4))      # no refused call touched a buffer
