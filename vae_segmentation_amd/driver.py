"""Shared machinery of the main_source.py / main_target.py entry points.

The reference's scripts (main_source.py 853 lines, main_target.py 1063 lines) are argparse + a NumPy/SimpleITK data
pipeline + the train / validate / checkpoint loop.  The data pipeline, TensorBoard writer and plotting are out of scope
 and their dependencies are absent, so the entry points here keep the reference's flag names and
loop semantics (methods, loss bodies, frozen sub-nets, optimiser groups, epoch arithmetic, checkpoint dict layout, score
JSON) and feed the step from a deterministic synthetic dataset (`--synthetic`, the default) or, with `--real_data`, from merge.npy cases
run through the device data pipeline (data_gpu.py).

One process per GPU: under torchrun (WORLD_SIZE > 1) every rank builds the same replica, takes its own shard of the
synthetic volumes and averages gradients with one RCCL all-reduce per step (vae_segmentation_amd.ddp) — the replacement
for the reference's nn.DataParallel wrap (main_source.py:354, main_target.py:436-438).
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

from . import data_gpu, ddp, ops, optim, volume
from . import train as T
from .evaluation import (EPS_EVALUATION, EPS_MAIN_SOURCE, INTENSITY_CLIP, LESION_RECORD_FIELDS, avg_dsc, binarize, coarse_to_fine_predict, confusion,
                         lesion_metrics, lesion_record_to_host, localise, mutual_information_3d, postprocess, segmentation_model_fn,
                         sliding_window_predict, tta_flips)
from .modules import DeepSupervision, Embed, Encoder, Fusion, Joint, Joint2, Segmentation, VAE, set_kernel_dtype, set_recompute

LABEL_KEY, IMG_KEY = "venous_pancreas", "venous"          # main_source.py:355-356


# ----------------------------------------------------------------------------------------------------
# synthetic data (stands in for BaseDataset + the transform stack of main_source.py:189-243)
# ----------------------------------------------------------------------------------------------------
def _hash_uniform(n, stream, seed):
    idx = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0x9E3779B97F4A7C15 + stream * 0xD1B54A32D192ED03 + 12345) % (1 << 64))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return ((x >> np.uint64(40)).astype(np.float64) / float(1 << 24)).astype(np.float32)


class SyntheticVolumes(torch.utils.data.Dataset):
    """Image ~ clip(N(0,1) + blob contrast, -1, 1) as after Clip / CenterIntensities (main_source.py:211-212); label = a
    jittered ellipsoid (1 = organ).  Item i is a pure function of (seed, i): every rank / run sees the same volumes."""

    def __init__(self, count, side, seed=0):
        self.count, self.side, self.seed = count, side, seed

    def __len__(self):
        return self.count

    def __getitem__(self, i):
        s = self.side
        u = _hash_uniform(8, 17, self.seed * 100003 + i)
        ax = (np.arange(s, dtype=np.float32) + 0.5) / s - 0.5
        z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
        c = (u[0:3] - 0.5) * 0.2
        r = 0.18 + 0.14 * u[3:6]
        d2 = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2
        label = (d2 < 1.0).astype(np.float32)
        n = s ** 3
        u1 = np.maximum(_hash_uniform(n, 1, self.seed * 7919 + i), 1e-7).astype(np.float64)
        u2 = _hash_uniform(n, 2, self.seed * 7919 + i).astype(np.float64)
        noise = (np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)).astype(np.float32).reshape(s, s, s)
        img = np.clip(0.6 * noise + 0.8 * label - 0.2, -1, 1)
        return {IMG_KEY: torch.from_numpy(img[None]), LABEL_KEY: torch.from_numpy(label[None])}


# ----------------------------------------------------------------------------------------------------
# real data: merge.npy cases from a json list, transformed on the device (main_source.py:125-131,186-243 with data_gpu.py's pipeline)
# ----------------------------------------------------------------------------------------------------
def filedict_from_json(json_path, key, epoch=1):
    """main_source.py:123-131: the case names under `key`, repeated `epoch` times"""
    with open(json_path, "r") as f:
        names = json.load(f).get(key, [])
    return list(names) * epoch


def mask_index_of(args):
    """main_source.py:92-95"""
    if str(args.pan_index) != "10":
        return [[0, 0]] + [[int(f), i + 1] for i, f in enumerate(str(args.pan_index).split(","))]
    return [[0, 0], [[1, 2], 1]]


class DeviceCaseLoader:
    """What BaseDataset + the transform stack + DataLoader deliver in the reference (main_source.py:186-243), with the transforms on the
    device: np.load of each case's merge array is the only host work; relabel / CropResize / MySpatialTransform / Clip / CenterIntensities
    run as vs_data_* kernels (data_gpu.py).  Yields {IMG_KEY, LABEL_KEY: (B, 1, S, S, S) CUDA tensors}.  With --train_patches a training loader cuts
    S^3 windows of the unscaled case (data_gpu.PatchSampler / train_patch) in place of CropResize; validation loaders never do."""

    def __init__(self, names, root, args, batch_size, train, shuffle, rank=0, world=1, seed=0):
        names = list(names)
        if train and world > 1:
            names = names[:len(names) // world * world]          # every rank the same number of steps (the all-reduce is collective)
        self.names, self.root, self.bs, self.shuffle = names[rank::world], root, batch_size, shuffle
        self.patch, self.mask_index, self.epoch, self.seed = (args.size,) * 3, mask_index_of(args), 0, seed + rank
        self.drop_last = train
        self.shift = int(args.shift) if train else 0           # main_target.py:204 (training crops only; validation: CropResize default)
        # --train_patches: a training loader cuts windows of the unscaled case in place of CropResize (self.sampler, below).  The sampler has then already
        # chosen where the patch lies, and the spatial transform resamples the gathered block about its centre: random_crop=False
        patches = bool(train and args.train_patches)
        self.transform = None
        if train and not args.no_aug:                       # main_source.py:195-205
            p_el = float(args.aug_elastic or 0.0)            # --aug_elastic: the stage main_source.py:198 leaves one flag away from on
            elastic = {"noise": "philox", "seed": seed + 1000 * rank} if p_el > 0 else {}
            self.transform = data_gpu.MySpatialTransform(
                self.patch, [d // 2 - 5 for d in self.patch], random_crop=not patches, scale=(0.85, 1.15), do_elastic_deform=p_el > 0, alpha=(0, 500),
                do_rotation=True, sigma=(10, 30.), angle_x=(-0.2, 0.2), angle_y=(-0.2, 0.2), angle_z=(-0.2, 0.2), border_mode_data="constant",
                border_cval_data=-1024, data_key=IMG_KEY, p_el_per_sample=p_el, label_key=LABEL_KEY, p_scale_per_sample=1, p_rot_per_sample=1,
                rng=np.random.RandomState(seed + 1000 * rank), **elastic)
        self.intensity = None
        if train and args.aug_intensity and not args.no_aug:
            # --aug_intensity: nnU-Net's intensity stage after CenterIntensities; its own generator, so the spatial draws keep their stream
            p_lr = float(args.aug_lowres or 0.0)            # --aug_lowres: the stage's simulated low resolution, off unless asked for
            lowres = {"p_lowres": p_lr} if p_lr > 0 else {}
            self.intensity = data_gpu.IntensityAugment(IMG_KEY, LABEL_KEY, rng=np.random.RandomState(seed + 1000 * rank + 500), noise="philox",
                                                       seed=seed + 1000 * rank, **lowres)
        self.standardize = None
        if args.standardize is not None:
            # --standardize: the case's percentile window onto Clip's, before anything else sees the image; the pipeline behind it keeps its constants
            self.standardize = data_gpu.IntensityStandardizer(tuple(args.standardize), target=INTENSITY_CLIP,
                                                              above=args.standardize_above)
        self.sampler = None
        if patches:
            # the sampler has a generator of its own, so the spatial and intensity draws keep their streams; without augmentation nothing resamples a margin away
            self.n_class = n_class_of(args)
            self.sampler = data_gpu.PatchSampler(self.patch, float(args.patch_fg), rng=np.random.RandomState(seed + 1000 * rank + 900),
                                                 margin=int(args.patch_margin) if self.transform is not None else 0)

    def _load(self, name):
        """a case's merge array on the device; with --standardize its image channel standardised"""
        merge = torch.from_numpy(np.load(os.path.join(self.root, name)).astype(np.float32)).cuda(non_blocking=True)
        if self.standardize is not None:
            merge[..., 0] = self.standardize.transform(merge[..., 0].contiguous())
        return merge

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return len(self.names) // self.bs if self.drop_last else (len(self.names) + self.bs - 1) // self.bs

    def whole_cases(self):
        """--val_whole_volume: every case as it is on disk — (raw image (D, H, W), relabelled label (D, H, W)) on the device, in list order, uncropped"""
        for name in self.names:
            merge = self._load(name)
            yield merge[..., 0].contiguous(), data_gpu.relabel(merge[..., 1].contiguous(), self.mask_index)

    def __iter__(self):
        order = np.arange(len(self.names))
        if self.shuffle:
            np.random.RandomState(self.seed + self.epoch).shuffle(order)
        for b in range(len(self)):
            imgs, labs = [], []
            for j, i in enumerate(order[b * self.bs:(b + 1) * self.bs]):
                merge = self._load(self.names[i])
                extra = {} if self.intensity is None else {"intensity": self.intensity}
                if self.sampler is not None:
                    img, lab, _ = data_gpu.train_patch(merge, self.patch, self.sampler, self.n_class, j, self.bs, self.mask_index, self.transform, field=IMG_KEY,
                                                       **extra)
                else:
                    img, lab = data_gpu.train_sample(merge, self.patch, self.mask_index, self.transform, field=IMG_KEY, shift=self.shift, **extra)
                imgs.append(img); labs.append(lab)
            yield {IMG_KEY: torch.cat(imgs), LABEL_KEY: torch.cat(labs)}


def make_loaders(args, rank, world):
    if args.real_data:
        json_path = os.path.join("lists", args.data_path)
        train = DeviceCaseLoader(filedict_from_json(json_path, args.train_list, args.eval_epoch), args.data_root, args, args.batch_size, True,
                                 shuffle=args.method != "domain_adaptation", rank=rank, world=world)       # main_source.py:232-236
        val = DeviceCaseLoader(filedict_from_json(json_path, args.val_list), args.val_data_root, args, 1, False, False)
        return train, val, train                      # the loader doubles as the 'sampler': set_epoch reshuffles
    train = SyntheticVolumes(args.synthetic_train, args.size, seed=1)
    val = SyntheticVolumes(args.synthetic_val, args.size, seed=2)
    sampler = None
    if world > 1:
        sampler = torch.utils.data.distributed.DistributedSampler(train, num_replicas=world, rank=rank, shuffle=True, drop_last=True)
    tl = torch.utils.data.DataLoader(train, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler,
                                     num_workers=0, pin_memory=True, drop_last=True)        # drop_last: main_source.py:237
    vl = torch.utils.data.DataLoader(val, batch_size=1, shuffle=False, num_workers=0, pin_memory=True)
    return tl, vl, sampler


def make_pseudo_loader(args, rank, world):
    """main_target.py:228-258,299-307: the second, pseudo-labelled training loader of a --pseudo_list run — its own case list, data root and structure indices
    (--pseudo_data_root, --pseudo_pan_index), the training transform stack, shuffled, drop_last."""
    if args.real_data:
        pargs = copy.copy(args)
        pargs.pan_index = args.pseudo_pan_index                # main_target.py:233: NumpyLoader_Multi_merge(mask_index=pseudo_mask_index)
        return DeviceCaseLoader(filedict_from_json(os.path.join("lists", args.data_path), args.pseudo_list, args.eval_epoch), args.pseudo_data_root, pargs,
                                args.batch_size, True, shuffle=True, rank=rank, world=world, seed=7)
    ds = SyntheticVolumes(args.synthetic_train, args.size, seed=3)
    return torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=True, num_workers=0, pin_memory=True, drop_last=True)


# ----------------------------------------------------------------------------------------------------
# model / optimiser construction (main_source.py:245-294, 300-346; main_target.py:314-352, 395-433)
# ----------------------------------------------------------------------------------------------------
def n_class_of(args):
    return 1 + len(str(args.pan_index).split(",")) if str(args.pan_index) != "10" else 2


def build_joint(args):
    nc = n_class_of(args)
    seg = Segmentation(n_channels=1, n_class=nc, norm_type=1)
    vae = VAE(n_channels=nc, n_class=nc, norm_type=1, dim=128, spatial=args.size)
    return Joint(models=[seg, vae], vae_forward_scale=args.vae_forward_scale,                 # main_target.py:324
                 vae_decoder_dropout=args.vae_decoder_dropout, seg_dropout=args.seg_dropout)


def freeze(module):
    for p in module.parameters():
        p.requires_grad = False
    module.eval()
    return module


def load_prefix(module, prefix, name="best_model.ckpt"):
    """--load_prefix* : '3dmodel/<prefix>/<name>' holding {'epoch','model_state_dict','optimizer_state_dict'}."""
    path = os.path.join("3dmodel", prefix, name)
    sd = torch.load(path, map_location="cpu")["model_state_dict"]
    module.load_state_dict(sd)
    ops.clear_pack_cache()
    print("loaded %s" % path)


def make_optimizer(args, groups):
    """--adam / --momentum / --weight_decay / --nesterov / --grad_clip; without them the reference's SGD(momentum 0.9) or Adam, launched as it always was"""
    max_norm = args.grad_clip or None                 # 0 = off
    if args.adam:
        return optim.Adam(groups, lr=args.lr_seg, betas=(0.9, 0.999), weight_decay=args.weight_decay, max_norm=max_norm)
    return optim.SGD(groups, lr=args.lr_seg, momentum=args.momentum, weight_decay=args.weight_decay, nesterov=bool(args.nesterov), max_norm=max_norm)


def load_ds_heads(deep, prefix, name="best_model.ckpt"):
    """the deep-supervision heads of '3dmodel/<prefix>/<name>' (save_checkpoint's "ds_heads_state_dict"); a checkpoint written without
    --deep_supervision has none: the heads keep their fresh initialisation, and the run says so"""
    path = os.path.join("3dmodel", prefix, name)
    sd = torch.load(path, map_location="cpu").get("ds_heads_state_dict")
    if sd is None:
        print("%s holds no ds_heads_state_dict: the deep-supervision heads start fresh" % path)
        return False
    deep.load_state_dict(sd)
    print("loaded the deep-supervision heads of %s" % path)
    return True


def save_checkpoint(prefix, epoch_label, model, optimizer, best, deep=None):
    path = os.path.join("3dmodel", prefix)
    os.makedirs(path, exist_ok=True)
    blob = {"epoch": epoch_label, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict()}
    if deep is not None:
        blob["ds_heads_state_dict"] = deep.state_dict()      # a key of its own: model_state_dict loads into a plain network
    torch.save(blob, os.path.join(path, "model_epoch%d.ckpt" % epoch_label))
    if best:
        torch.save(blob, os.path.join(path, "best_model.ckpt"))


# ----------------------------------------------------------------------------------------------------
# validation (main_source.py:688-822): batch 1, hard Dice of the argmax prediction against the label
# ----------------------------------------------------------------------------------------------------
def _cleaned(hard, nc, keep_largest, min_component, closing, fill_holes):
    """--val_closing / --val_fill_holes / --val_keep_largest: the hard prediction after evaluation.postprocess, or None with all three off"""
    if not (keep_largest > 0 or closing > 0 or fill_holes):
        return None
    return postprocess(hard, closing=closing, fill_holes=fill_holes, keep_largest=keep_largest, min_size=min_component, lo_channel=min(1, nc - 1))


def _log_options(log, tta, closing, fill_holes):
    """what whole_<epoch>.json and fine_<epoch>.json say about the options that shaped their scores"""
    if tta:
        log["tta"] = list(tta)
    if closing > 0 or fill_holes:
        log["closing"], log["fill_holes"] = int(closing), bool(fill_holes)


# the optional measurements of validate(): per case a collector, whose record stays on the device, and after the last case a reporter, which brings
# the records to the host once, prints the summary line and fills the log dict
def _surface_case(hard, unfiltered, gt, lo):
    """-> (distances of the scored prediction, those of the unfiltered one or None when no clean-up is on)"""
    raw = None if unfiltered is None else volume.surface_distances(unfiltered[:, lo:], gt[:, lo:])
    return volume.surface_distances(hard[:, lo:], gt[:, lo:]), raw


def _surface_report(surf, surface_log):
    for which, tag in ((0, ""), (1, " without the component filter")):
        recs = {i: rec[which] for i, rec in surf.items() if rec[which] is not None}
        if not recs:
            continue
        a, h = (torch.stack([recs[i][name].reshape(-1) for i in sorted(recs)]).cpu().numpy() for name in ("assd", "hd95"))     # one host copy per metric
        undefined = int(np.isnan(a).sum())
        if undefined == a.size:
            print("validation surface distances%s: undefined in all %d entries (an empty surface)" % (tag, a.size))
        else:
            print("validation surface distances%s: ASSD %f, HD95 %f voxels (%d of %d case x class entries undefined)"
                  % (tag, float(np.nanmean(a)), float(np.nanmean(h)), undefined, a.size))
        if surface_log is not None:
            suffix = "_unfiltered" if tag else ""
            for row, i in enumerate(sorted(recs)):
                entry = surface_log.setdefault(i, {})
                entry["assd" + suffix] = [float(v) for v in a[row]]
                entry["hd95" + suffix] = [float(v) for v in h[row]]


def _lesion_case(hard, gt, lo, nc, min_component):
    return (lesion_metrics(hard[:, lo:], gt[:, lo:], connectivity=26, min_size=int(min_component)),
            confusion(hard.argmax(1, keepdim=True), gt.argmax(1, keepdim=True), nc))


def _lesion_report(les, lesion_log, min_component):
    for i in sorted(les):
        rec, conf = les[i]
        entry = {k: v[0] for k, v in lesion_record_to_host(rec).items()}                  # batch 1: lists over the foreground classes
        assert tuple(entry) == LESION_RECORD_FIELDS
        for name in CONFUSION_LOG_FIELDS:
            entry[name] = conf[name.replace("class_", "")][0, 0].cpu().tolist()            # over all classes, background first
        entry["confusion_overflow"] = int(conf["overflow"][0, 0])
        lesion_log[i] = entry
    tp, n_gt, fp = (sum(sum(lesion_log[i][k]) for i in lesion_log) for k in ("tp", "n_gt", "fp"))
    print("validation lesions: %d of %d reference lesions detected, %d false detections (components of at least %d voxels)"
          % (tp, n_gt, fp, max(int(min_component), 1)))


def _intensity_case(image, pred, hard, gt, lo, nc, bins):
    sides = {}
    for name, hot in (("pred", hard), ("label", gt)):
        rec = volume.histogram(image, bins, range=INTENSITY_RANGE, labels=hot.argmax(1, keepdim=True).to(torch.int32), rows=nc - 1)
        sides[name] = (rec["table"][:, 0, lo:], rec["outside"][:, 0], hot[:, lo:].sum((2, 3, 4)))
    return sides, torch.stack([mutual_information_3d(pred[:, k], gt[:, k]) for k in range(lo, nc)])


def _intensity_report(inten, intensity_log, bins):
    for i in sorted(inten):
        sides, nmi = inten[i]
        entry = {"bins": bins, "range": list(INTENSITY_RANGE)}
        for name in ("pred", "label"):                                                     # batch 1: lists over the foreground classes
            table, outside, voxels = sides[name]
            entry[name + "_hist"] = table[0].cpu().tolist()
            entry[name + "_voxels"] = [int(v) for v in voxels[0].cpu().tolist()]
            entry[name + "_outside"] = int(outside[0])
        entry["nmi"] = [float(v) for v in nmi.cpu().tolist()]
        assert tuple(entry) == INTENSITY_LOG_FIELDS
        intensity_log[i] = entry
    print("validation intensities: %d-bin histograms of the image inside prediction and label, mean normalised mutual information of probability and "
          "label %f" % (bins, float(np.mean([np.mean(intensity_log[i]["nmi"]) for i in intensity_log]))))


@torch.no_grad()
def validate(method, model, loader, nc, keep_largest=0, min_component=0, save_dir=None, epoch=0, surface=False, surface_log=None, closing=0,
             fill_holes=False, lesion=False, lesion_log=None, intensity=0, intensity_log=None):
    """main_source.py:688-822 / main_target.py:754-805: batch-1 forwards and hard Dice per case.  Forward only (no autograd graph is recorded: nothing is kept
    for a backward pass — the per-(n, c) statistics the conv epilogues accumulate are the FORWARD's own, the next layer normalises with them).
    keep_largest = k > 0: the hard prediction is cleaned up first as utils/utils.py:776-796 (predict_vol step 2) does — per foreground channel only the k largest
    26-connected components of at least min_component voxels stay, what is removed becomes background (ops.keep_largest on the device: no host copy and no
    synchronisation per case beyond the score's .item()) — the returned scores are the filtered ones and the unfiltered mean is printed beside them.
    save_dir (--save_eval_result; main_source.py:721-727,751-757 / main_target.py:922-930): per case {epoch}_{idx}_pred.join / _pic / _gt (+ _pred_cc, the
    filtered mask, when the filter is on) are written there with np.save.
    surface (--val_surface): additionally ASSD and HD95 (evaluation.surface_metrics: medpy's convention, unit spacing, on the device) of the hard prediction —
    the filtered one when the filter is on, the unfiltered values are then reported beside them — against the label for every foreground class; their nanmean and
    the number of undefined (empty-surface) entries are printed, the per-case values go to the dict surface_log.  The returned scores are not affected.
    closing (--val_closing N) / fill_holes (--val_fill_holes): evaluation.postprocess runs in the filter's place — per foreground class a binary closing of N
    iterations (26-neighbourhood), then hole filling (6-connectivity), then the component filter if it is on; everything said of the filter above holds for it.
    lesion (--val_lesion): additionally, for the hard prediction after whatever clean-up is on, the lesion-wise detection record of every foreground class
    (evaluation.lesion_metrics: 26-connected components, min_size = min_component) and the per-class scores of the confusion matrix
    (evaluation.confusion) — on the device, brought to the host once after the last case; the per-case values go to the dict lesion_log
    (LESION_LOG_FIELDS).  The returned scores are not affected, and with lesion False nothing of this is launched.
    intensity (--val_intensity BINS) > 0: additionally, per case, the histogram (BINS bins over INTENSITY_RANGE, what Clip and CenterIntensities leave) of
    the network's input image inside every foreground class of the hard prediction — after whatever clean-up is on — and inside every foreground class of
    the label (ops.histogram with the class map as labels: one pass over the image per side), and the normalised mutual information of every foreground
    probability with its label channel (evaluation.mutual_information_3d) — on the device, brought to the host once after the last case; the per-case
    values go to the dict intensity_log (INTENSITY_LOG_FIELDS).  The returned scores are not affected, and with intensity 0 nothing of this is launched."""
    clean = (keep_largest, min_component, closing, fill_holes)
    want_hard = surface or lesion or intensity > 0 or keep_largest > 0 or closing > 0 or fill_holes         # a measurement or a clean-up reads it
    scores, raw, surf, les, inten = {}, {}, {}, {}, {}
    lo = min(1, nc - 1)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    for i, batch in enumerate(loader):
        gt = ops.onehot(batch[LABEL_KEY].cuda(non_blocking=True), nc)
        if method == "vae_train":
            pred, _, _ = model(gt, if_random=False)
        elif method == "discriminator_train":                              # no segmentation to score: report 1 - squared error of the score
            tgt = batch[LABEL_KEY].float().mean((1, 2, 3, 4)).view(-1, 1).cuda() * 4
            scores[i] = float(1 - ((model(batch[LABEL_KEY].cuda().float()) - tgt) ** 2).mean().item())
            continue
        elif method in ("embed_train", "refine_vae"):                      # main_source.py:735-745: Embed in test mode
            pred = model({IMG_KEY: batch[IMG_KEY].cuda(non_blocking=True), "venous_pancreas_only": gt}, IMG_KEY, "pred", test_mode=True)["pred"]
        else:
            seg = model.Seg if hasattr(model, "Seg") else model
            pred = seg({IMG_KEY: batch[IMG_KEY].cuda(non_blocking=True)}, IMG_KEY, "pred")["pred"]
        unfiltered = ops.hard_onehot(pred) if want_hard else None       # the one hard prediction of the case: clean-up and every measurement read it
        filtered = _cleaned(unfiltered, nc, *clean) if want_hard else None
        if filtered is not None:
            raw[i] = avg_dsc({"p": pred, "g": gt}, "p", "g", binary=True, botindex=1, topindex=nc)
        hard = unfiltered if filtered is None else filtered             # what is scored and measured
        scores[i] = avg_dsc({"p": pred if filtered is None else filtered, "g": gt}, "p", "g", binary=True, botindex=1, topindex=nc).item()
        if surface:
            surf[i] = _surface_case(hard, unfiltered if filtered is not None else None, gt, lo)
        if lesion:
            les[i] = _lesion_case(hard, gt, lo, nc, min_component)
        if intensity > 0:
            inten[i] = _intensity_case(batch[IMG_KEY].cuda(non_blocking=True).float()[:, :1].contiguous(), pred, hard, gt, lo, nc, int(intensity))
        if save_dir is not None:
            stem = os.path.join(save_dir, "%d_%d_" % (epoch, i))
            np.save(stem + "pred.join", binarize(pred).cpu().numpy())
            np.save(stem + "pic", batch[IMG_KEY].cpu().numpy())
            np.save(stem + "gt", binarize(gt).cpu().numpy())
            if filtered is not None:
                np.save(stem + "pred_cc", filtered.cpu().numpy())
    if raw:
        print("validation without the component filter: %f (keeping the %d largest components of at least %d voxels per class%s)"
              % (float(np.mean([v.item() for v in raw.values()])), keep_largest, min_component,
                 ", after closing %d and hole filling %s" % (closing, "on" if fill_holes else "off") if closing > 0 or fill_holes else ""))
    if surf:
        _surface_report(surf, surface_log)
    if les and lesion_log is not None:
        _lesion_report(les, lesion_log, min_component)
    if inten and intensity_log is not None:
        _intensity_report(inten, intensity_log, int(intensity))
    return scores


# intensity_<epoch>.json, per case: the image's histogram inside every foreground class of the hard prediction and of the label (lists over the foreground
# classes, then over the bins), the voxels of those classes (the histograms sum to them when nothing is outside the range), the image voxels of the whole
# case outside the range, and the normalised mutual information of every foreground probability with its label channel
INTENSITY_RANGE = (-1.0, 1.0)                       # Clip(-200, 400) then CenterIntensities(100, 300)
INTENSITY_LOG_FIELDS = ("bins", "range", "pred_hist", "pred_voxels", "pred_outside", "label_hist", "label_voxels", "label_outside", "nmi")


# lesion_<epoch>.json, per case: evaluation.LESION_RECORD_FIELDS as lists over the foreground classes, then the voxel-wise scores of evaluation.confusion as
# lists over ALL classes (its sensitivity / precision under a class_ prefix: the record has lesion-wise ones of the same name) and its overflow count
CONFUSION_LOG_FIELDS = ("dice", "iou", "class_sensitivity", "class_precision")
LESION_LOG_FIELDS = ("n_gt", "n_pred", "tp", "fn", "fp", "sensitivity", "precision", "f1", "overflow") + CONFUSION_LOG_FIELDS + ("confusion_overflow",)


def validate_finetune(runner, loader):
    """main_target.py:807-953 with --val_finetune k: per case, test-time training of a copy of the model, then hard Dice of the
    finetuned and of the untouched network.  -> (scores, scores_noft)"""
    scores, scores_noft = {}, {}
    for i, batch in enumerate(loader):
        _, noft, ft, _ = runner.run(batch[IMG_KEY].cuda(non_blocking=True), batch[LABEL_KEY].cuda(non_blocking=True))
        scores[i], scores_noft[i] = ft.item(), noft.item()
    return scores, scores_noft


def _hard_dice(pred_hot, gt_hot, lo, nc):
    """hard Dice of two planar one-hot tensors (K, ...) over the classes [lo, nc), avg_dsc(binary=True)'s arithmetic; a volume of any size
    (ops.Dice pads a plane that is no whole number of 16-byte quads with voxels that belong to no class on either side)"""
    a, b = pred_hot.reshape(1, pred_hot.shape[0], -1), gt_hot.reshape(1, gt_hot.shape[0], -1)
    return ops.Dice.apply(a, b, lo, nc, EPS_EVALUATION, True)


WHOLE_VOLUME_CVAL = (0.0 - 100.0) / 300.0          # what CropResize's zero padding becomes after Clip(-200, 400) and CenterIntensities(100, 300)


@torch.no_grad()
def validate_whole_volume(model, cases, nc, patch, overlap=0.5, batch=1, blend="gaussian", keep_largest=0, min_component=0, log=None, tta=None,
                          closing=0, fill_holes=False):
    """--val_whole_volume: label-free coarse-to-fine inference, scored.  `cases` yields (raw image, relabelled label) (D, H, W) device tensors
    (DeviceCaseLoader.whole_cases).  Per case:
      dice_whole       the clipped and centred WHOLE volume is predicted by sliding window with the segmentation network (evaluation.sliding_window_predict,
                       cubic windows of side `patch`); hard Dice per foreground class of that prediction — after ops.keep_largest when keep_largest > 0 —
                       against the whole label
      dice_label_free  the case is cropped by CropResize with the box of the PREDICTION (evaluation.localise -> <field>_pancreas_pred) instead of the
                       label's, the fine forward runs on the crop, hard Dice in crop space.  A coarse prediction without foreground gives no box: 0.
    Both means are printed; the per-case values go to the dict `log`.  -> (mean dice_whole, mean dice_label_free)
    tta (--val_tta, evaluation.tta_flips): mirror test-time augmentation of the sliding-window pass; the crop-space fine forward stays a single one.
    The codes are then recorded as log["tta"].
    closing / fill_holes (--val_closing, --val_fill_holes): evaluation.postprocess cleans the sliding-window prediction up before dice_whole — closing, hole
    filling, then the component filter if it is on; recorded as log["closing"] / log["fill_holes"] when set."""
    tta = tta_flips(tta)
    seg = model.Seg if hasattr(model, "Seg") else model
    model_fn = segmentation_model_fn(seg)
    lo = min(1, nc - 1)
    whole, free = {}, {}
    for i, (img, lab) in enumerate(cases):
        d = {IMG_KEY: img.clone()}
        d = data_gpu.CenterIntensities([IMG_KEY], subtrahend=100, divisor=300)(data_gpu.Clip([IMG_KEY], new_min=-200, new_max=400)(d))
        res = sliding_window_predict(model_fn, d[IMG_KEY], patch, overlap=overlap, blend=blend, batch=batch, cval=WHOLE_VOLUME_CVAL, tta=tta)
        if res["prob"].shape[0] != nc:
            raise ValueError("whole-volume validation: the network predicts %d classes, the labels have %d" % (res["prob"].shape[0], nc))
        hard = ops.hard_onehot(res["prob"][None])
        cleaned = _cleaned(hard, nc, keep_largest, min_component, closing, fill_holes)
        gt = ops.onehot(lab[None, None], nc)
        whole[i] = _hard_dice((hard if cleaned is None else cleaned)[0], gt[0], lo, nc)
        mask = localise(res["prob"], keep_largest=max(keep_largest, 1), min_size=min_component, lo_channel=lo)
        if data_gpu.bounding_box(mask) is None:
            free[i] = torch.zeros((), device=img.device)
            continue
        c = data_gpu.CropResize([IMG_KEY], (patch,) * 3)({IMG_KEY: img, LABEL_KEY: lab, IMG_KEY + "_pancreas_pred": mask})
        c = data_gpu.CenterIntensities([IMG_KEY], subtrahend=100, divisor=300)(data_gpu.Clip([IMG_KEY], new_min=-200, new_max=400)(c))
        fine = seg({IMG_KEY: c[IMG_KEY][None, None]}, IMG_KEY, "pred")["pred"]
        free[i] = avg_dsc({"p": fine, "g": ops.onehot(c[LABEL_KEY][None, None], nc)}, "p", "g", binary=True, botindex=1, topindex=nc)
    w = {i: float(v.item()) for i, v in whole.items()}                    # host copies after the last case
    f = {i: float(v.item()) for i, v in free.items()}
    mw, mf = (float(np.mean(list(x.values()))) if x else 0.0 for x in (w, f))
    print("validation on whole volumes (sliding window %d^3, overlap %g, %s blend%s): dice_whole %f, dice_label_free %f over %d cases"
          % (patch, overlap, blend, ", mirror TTA %s" % (tta,) if tta else "", mw, mf, len(w)))
    if log is not None:
        for i in w:
            log[i] = {"dice_whole": w[i], "dice_label_free": f[i]}
        _log_options(log, tta, closing, fill_holes)
    return mw, mf


@torch.no_grad()
def validate_fine_whole(model, cases, nc, patch, overlap=0.5, batch=1, blend="gaussian", keep_largest=0, min_component=0, interp="linear", log=None,
                        save_dir=None, names=None, tta=None, closing=0, fill_holes=False):
    """--val_fine_whole: the label-free FINE prediction scored where the scan lives.  `cases` as for validate_whole_volume.  Per case
    evaluation.coarse_to_fine_predict returns the fine pass pasted back onto the scan grid (ops.uncrop); dice_fine_whole is the hard Dice per foreground
    class of that label — after ops.keep_largest when keep_largest > 0 — against the whole label, so it compares with dice_whole and with scores
    published on the scan grid.  A case whose coarse prediction is empty scores its all-background label.  The mean is printed, the per-case values
    go to the dict `log`; with save_dir the scored label of case i is written to <save_dir>/<names[i] without its extension>.npy (uint8, scan shape).
    tta (--val_tta, evaluation.tta_flips): mirror test-time augmentation of the coarse and the fine pass; the codes are then recorded as log["tta"].
    closing / fill_holes (--val_closing, --val_fill_holes): evaluation.postprocess cleans the pasted label up before it is scored and saved — closing, hole
    filling, then the component filter if it is on; recorded as log["closing"] / log["fill_holes"] when set.
    -> mean dice_fine_whole"""
    tta = tta_flips(tta)
    seg = model.Seg if hasattr(model, "Seg") else model
    lo = min(1, nc - 1)
    fine, found = {}, {}
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
    for i, (img, lab) in enumerate(cases):
        res = coarse_to_fine_predict(seg, img, patch, overlap=overlap, blend=blend, batch=batch, keep_largest=max(keep_largest, 1), min_size=min_component,
                                     interp=interp, tta=tta)
        label = res["label"]
        hard = ops.onehot(label.float()[None, None], nc)
        cleaned = _cleaned(hard, nc, keep_largest, min_component, closing, fill_holes)
        if cleaned is not None:
            hard, label = cleaned, cleaned[0].argmax(0).to(torch.uint8)
        fine[i] = _hard_dice(hard[0], ops.onehot(lab[None, None], nc)[0], lo, nc)
        found[i] = bool(res["found"])
        if save_dir is not None:
            stem = os.path.splitext(os.path.basename(names[i]))[0] if names is not None else "case%d" % i
            np.save(os.path.join(save_dir, stem + ".npy"), label.cpu().numpy())
    f = {i: float(v.item()) for i, v in fine.items()}                     # host copies after the last case
    mean = float(np.mean(list(f.values()))) if f else 0.0
    print("validation of the fine pass on whole volumes (%s paste%s): dice_fine_whole %f over %d cases, %d without a coarse box"
          % (interp, ", mirror TTA %s" % (tta,) if tta else "", mean, len(f), sum(not v for v in found.values())))
    if log is not None:
        for i in f:
            log[i] = {"dice_fine_whole": f[i]}
        _log_options(log, tta, closing, fill_holes)
    return mean


def _need(script, cond, what):
    """the reference asserts its flag combinations; `python -O` strips asserts, an entry point must not"""
    if not cond:
        raise SystemExit("%s: inconsistent flags — %s" % (script, what))


def check_fine_whole_flags(a, script="main_source.py"):
    """--val_fine_whole rides on the whole-volume pass; --save_whole_pred saves what --val_fine_whole makes"""
    if a.val_fine_whole:
        _need(script, a.val_whole_volume, "--val_fine_whole scores the fine pass of the whole-volume chain: it needs --val_whole_volume")
    if a.save_whole_pred:
        _need(script, a.val_fine_whole, "--save_whole_pred writes the labels that --val_fine_whole pastes: it needs --val_fine_whole")


def check_lesion_flags(a, script="main_source.py"):
    """--val_lesion scores the objects of the prediction validation already makes: it needs a validation pass that makes one"""
    if not a.val_lesion:
        return
    _need(script, a.method != "discriminator_train", "--val_lesion scores a segmentation, --method discriminator_train predicts none")
    _need(script, not a.val_finetune, "--val_lesion rides on the plain validation pass: it cannot be combined with --val_finetune")
    _need(script, a.val_min_component >= 0, "--val_min_component is a number of voxels: it cannot be negative")


def check_intensity_flags(a, script="main_source.py"):
    """--val_intensity reads the image inside the prediction validation already makes: it needs a validation pass that makes one"""
    if not a.val_intensity:
        return
    _need(script, 1 <= a.val_intensity <= volume.HISTOGRAM_MAX_BINS, "--val_intensity is a number of bins between 1 and %d" % volume.HISTOGRAM_MAX_BINS)
    _need(script, a.method != "discriminator_train", "--val_intensity reads the image inside a segmentation, --method discriminator_train predicts none")
    _need(script, not a.val_finetune, "--val_intensity rides on the plain validation pass: it cannot be combined with --val_finetune")


def check_whole_volume_flags(a, script="main_source.py"):
    """--val_whole_volume reads whole cases from disk and needs a segmentation network; --val_tta augments its sliding-window passes;
    --val_closing counts iterations"""
    _need(script, a.val_closing >= 0, "--val_closing is a number of closing iterations: it cannot be negative")
    if a.val_tta:
        _need(script, a.val_whole_volume, "--val_tta mirrors the windows of the whole-volume chain: it needs --val_whole_volume")
        try:
            tta_flips(a.val_tta)
        except ValueError as e:
            _need(script, False, "--val_tta: %s" % e)
    if not a.val_whole_volume:
        return
    _need(script, a.real_data, "--val_whole_volume predicts whole merge.npy cases: it needs --real_data")
    _need(script, a.method not in ("vae_train", "discriminator_train", "embed_train", "refine_vae"),
          "--val_whole_volume needs a segmentation network, --method %s has none" % a.method)
    _need(script, 0.0 <= a.sw_overlap < 1.0, "--sw_overlap must be in [0, 1)")
    _need(script, a.sw_batch >= 1, "--sw_batch must be at least 1")



# ----------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------
def start_process(args, side):
    """the flag checks — ahead of the GPU check: they need no device — then this process's place among the ranks -> (rank, world)"""
    for check in (check_fine_whole_flags, check_whole_volume_flags, check_lesion_flags, check_intensity_flags):
        check(args, "main_%s.py" % side)
    rank, world, local = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))
    if not torch.cuda.is_available():
        raise SystemExit("the native kernels need a GPU (there is no CPU path)")
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    if args.save_epoch % args.eval_epoch != 0:                            # main_source.py asserts this; an assert would vanish under python -O
        raise SystemExit("--save_epoch must be a multiple of --eval_epoch")
    return rank, world


def build_models(args, nc):
    """-> (model, the part of it that trains, the teacher or None) of --method, on the host and as initialised"""
    method, teacher = args.method, None
    if method == "vae_train":
        model = VAE(n_channels=nc, n_class=nc, norm_type=1, dim=128, soft=bool(args.softrelu), spatial=args.size)
    elif method == "seg_train":
        model = Segmentation(n_channels=1, n_class=nc, norm_type=1)
    elif method in ("joint_train", "domain_adaptation", "sep_joint_train"):
        model = build_joint(args)
        if method != "joint_train":
            teacher = build_joint(args)                                     # main_target.py:323-328 / main_source.py:270-273 (tea_model)
    elif method in ("embed_train", "refine_vae"):                          # main_source.py:259-264
        model = Embed(models=[Encoder(n_channels=1, dim=128, norm_type=1, spatial=args.size),
                              VAE(n_channels=nc, n_class=nc, norm_type=1, dim=128, spatial=args.size),
                              Fusion(n_channels_img=1, n_channels_mask=nc, n_class=nc, norm_type=1)])
    elif method == "discriminator_train":                                  # main_target.py:318-319
        model = Encoder(n_channels=1, dim=1, norm_type=1, spatial=args.size)
    elif method == "domain_adaptation_dis":                                # main_target.py:337-342
        model = Joint2(models=[Segmentation(n_channels=1, n_class=nc, norm_type=1), Encoder(n_channels=1, dim=1, norm_type=1, spatial=args.size)],
                       seg_dropout=args.seg_dropout)
        teacher = Segmentation(n_channels=1, n_class=nc, norm_type=1)
    else:
        raise ValueError("Try a valid method.")                           # main_source.py:275 / main_target.py:343
    return model, (model.Seg if isinstance(model, (Joint, Joint2)) else model), teacher


def load_and_freeze(args, model, trainable, teacher, dtype):
    """the checkpoints of --load_prefix*, the frozen sub-networks, the teacher's weights -> (model, trainable, teacher) on the device:
    --only_pseudo swaps model and teacher"""
    method = args.method
    model = model.cuda()
    from_scratch = bool(args.from_scratch) and method == "domain_adaptation"
    if from_scratch:
        teacher = teacher.cuda()
    if args.load_prefix:                                                    # main_target.py:355-366: --from_scratch loads the TEACHER's Seg, the student keeps its initialisation
        target = teacher if from_scratch else model
        load_prefix(target.Seg if hasattr(target, "Seg") else target, args.load_prefix, args.checkpoint_name)
    if args.load_prefix_vae and hasattr(model, "Vae"):
        if from_scratch:
            load_prefix(teacher.Vae, args.load_prefix_vae)                  # :370-371
        load_prefix(model.Vae, args.load_prefix_vae)
    if args.load_prefix_encoder:                                            # :384-390
        if method == "discriminator_train":
            load_prefix(model, args.load_prefix_encoder)
        elif hasattr(model, "Dis"):
            load_prefix(model.Dis, args.load_prefix_encoder)
    if args.load_prefix_joint and hasattr(model, "Seg"):
        load_prefix(model, args.load_prefix_joint, args.checkpoint_name)
    if hasattr(model, "Vae") and method != "refine_vae":
        freeze(model.Vae)                                                   # main_source.py:343-346
    if args.fix_layer and method in ("joint_train", "domain_adaptation"):   # main_target.py:400-406: only the last decoder block and the head train
        for prm in model.Seg.parameters():
            prm.requires_grad = False
        for prm in list(model.Seg.up5.parameters()) + list(model.Seg.out_block.parameters()):
            prm.requires_grad = True
    if method == "refine_vae":                                              # main_source.py:347-353: VAE encoder half frozen, decoder trained
        for name, prm in model.Vae.named_parameters():
            prm.requires_grad = name.split(".")[0] not in ("in_block", "down1", "down2", "down3", "down4", "down5", "fc_mean", "fc_std")
        for prm in model.Encoder.parameters():                              # :596-597
            prm.requires_grad = False
    if method == "domain_adaptation_dis":
        freeze(model.Dis)                                                   # main_target.py:407-411
    if teacher is not None:
        teacher = teacher.cuda()
        if method in ("sep_joint_train", "domain_adaptation_dis"):
            teacher.load_state_dict(model.state_dict() if method == "sep_joint_train" else model.Seg.state_dict())   # main_source.py:330-340 / main_target.py:366
        elif args.only_pseudo:
            # main_target.py:421-425: the loaded network becomes the frozen pseudo-label teacher, a freshly initialised one is trained
            model, teacher = teacher, model
            freeze(model.Vae)
            trainable = model.Seg
        elif args.test_only or not from_scratch:                            # main_target.py:427: a --from_scratch teacher keeps what --load_prefix* gave it
            teacher.load_state_dict(model.state_dict())                     # main_target.py:426-427 / :379-380
        freeze(teacher)
        set_kernel_dtype(teacher, dtype)
    set_kernel_dtype(model, dtype)
    set_recompute(bool(args.recompute))
    return model, trainable, teacher


def build_optimizer(args, model, trainable, teacher, world):
    """-> (the --deep_supervision heads or None, optimizer, the step's live parameters, the gradient all-reduce or None); under torchrun every replica
    leaves with rank 0's tensors"""
    deep = None                                                             # --deep_supervision L: auxiliary heads on the decoder's coarse levels
    if args.deep_supervision and args.method in SEG_LOSS_METHODS:
        deep = DeepSupervision(trainable, args.deep_supervision).cuda()
        resumed = args.load_prefix if args.method == "seg_train" else (args.load_prefix_joint or args.load_prefix)
        if resumed:
            load_ds_heads(deep, resumed, args.checkpoint_name)
    if hasattr(model, "Seg") and hasattr(model, "Vae"):
        groups = [{"params": list(model.Seg.parameters()), "lr": args.lr_seg, "model": "Seg"},
                  {"params": list(model.Vae.parameters()), "lr": args.lr_vae, "model": "Vae"}]
    else:
        groups = [{"params": list(model.parameters()), "lr": args.lr_seg}]
    if deep is not None:
        groups.append({"params": list(deep.parameters()), "lr": args.lr_seg, "model": "DeepSupervision"})
    optimizer = make_optimizer(args, groups)
    params = [p for p in trainable.parameters() if p.requires_grad]
    if deep is not None:
        params += list(deep.parameters())
    if world == 1:
        return deep, optimizer, params, None
    sync = ddp.FlatGradSync(params)
    sync.broadcast_parameters(0)
    # the trainable list is not the whole replica: frozen or freshly initialised layers (--fix_layer, --from_scratch, a VAE without a checkpoint) and
    # the teacher must agree across ranks too, or the replicas differ from the first forward on
    seen = {id(p) for p in params}
    for mod in (model, teacher):
        if mod is None:
            continue
        for t in list(mod.parameters()) + list(mod.buffers()):
            if id(t) not in seen and t.is_cuda:
                seen.add(id(t))
                dist.broadcast(t.data, 0)
    ddp.note_eager_collective()
    ops.weights_changed()
    return deep, optimizer, params, sync


def loss_key(args, method, epoch):
    """what of the loss expression depends on the epoch (main_target.py:583-592): a captured step is rebuilt when it changes"""
    if method == "domain_adaptation_dis":                               # main_target.py:720-723: lambda ramps with the epoch during the warm-up
        return min(epoch, args.lambda_vae_warmup)
    if method == "embed_train":                                         # the Encoder's requires_grad follows the epoch's parity: another live parameter set
        return epoch % 2
    if method != "domain_adaptation" or args.domain_loss_type != 0 or args.only_pseudo:
        return 0
    if args.turn_epoch != -1:
        return (epoch // args.turn_epoch) % 2
    return min(epoch, args.lambda_vae_warmup)


def _monte_carlo(draw, n):
    """main_target.py:530-603 (--vae_mont_number N): N forward passes of student and teacher per step (they differ by their dropout draws),
    the four loss terms averaged, one backward through all of them"""
    final, aux = draw()
    if n == 1:
        return final, aux
    tot = {k: v for k, v in aux.items() if k != "batch" and k != "kl_loss"}
    for _ in range(n - 1):
        f, aux = draw()
        final = final + f
        tot = {k: tot[k] + aux[k] for k in tot}
    out = {k: v / n for k, v in tot.items()}
    out["kl_loss"], out["batch"] = aux["kl_loss"], aux["batch"]             # the reference logs the LAST pass's KL (:605)
    return final / n, out


class TrainState:
    """What a training step reads and the loop changes under it.  loss() is the step's loss expression — what a train.GraphedStep captures — so a
    capture bakes in lambda_vae, the epoch-dependent branch (loss_key) and the live parameter list; whoever changes one of them sets stepper_key
    to None, and the step is captured again before it next runs."""

    def __init__(self, args, side, nc, rank, model, trainable, teacher, deep, optimizer, params, sync, scaler, pseudo_loader):
        self.args, self.method, self.nc, self.rank = args, args.method, nc, rank
        self.eps = EPS_MAIN_SOURCE if side == "source" else EPS_EVALUATION          # the two scripts use different epsilons
        self.model, self.trainable, self.teacher, self.optimizer, self.sync, self.scaler = model, trainable, teacher, optimizer, sync, scaler
        self.base_lrs = [grp["lr"] for grp in optimizer.param_groups]
        self.n_outer = max(1, args.max_epoch // args.eval_epoch)
        self.epoch, self.lambda_vae, self.params = 0, args.lambda_vae, params
        self.stepper, self.stepper_key = None, None
        self.pseudo_loader, self.pseudo_itr, self.pseudo_cycles = pseudo_loader, None, 0
        bs, s = args.batch_size, args.size
        self.img = torch.zeros(bs, 1, s, s, s, device="cuda")               # fixed-address inputs of the captured step
        self.lab = torch.zeros(bs, 1, s, s, s, device="cuda")
        self.score = torch.zeros(bs, 1, device="cuda")                      # discriminator_train's regression target (venous_score)
        self.pimg = self.plab = None                                        # the logged-only pseudo-labelled batch, made on first use
        self.use_graph = not args.no_graph and not (args.seg_dropout or args.vae_decoder_dropout)   # dropout draws fresh masks per call: eager (train.GraphedStep)
        # the sampling methods draw VAE noise per call.  --latent_noise torch (the default): torch.randn, launched eagerly.  --latent_noise philox: one
        # ops.LatentStream per rank, drawn inside the forward launch from a device-resident counter, so the step is captured like every other method's;
        # embed_train's requires_grad toggle by epoch parity rebuilds the captured step (loss_key)
        self.latent = None
        if self.method in ("embed_train", "refine_vae", "vae_train"):
            if args.latent_noise == "philox":
                # 1000 rank + 700: the loaders' per-rank Philox streams are seeded base + 1000 rank (+ 500) with their own fixed bases; this one's base is 0
                # (the entry points have no --seed flag)
                self.latent = ops.LatentStream(1000 * rank + 700)
            else:
                self.use_graph = False
        self.seg_loss = seg_loss_of(args)                                   # --seg_loss dice_ce: ops.seg_loss's arguments; None: the reference's Dice
        self.seg_kw = {} if deep is None else {"deep": deep}
        # --boundary_weight: the boundary term's weight is ONE device scalar, refilled at the top of every outer epoch (train.boundary_weight): the captured
        # launches read it, so the ramp needs no re-capture.  With the flags at their defaults nothing is built and loss() passes nothing on
        self.boundary_w = None
        if boundary_enabled(args) and self.method in SEG_LOSS_METHODS and self.seg_loss is not None:
            self.boundary_w = torch.zeros((), dtype=torch.float32, device="cuda")
            self.seg_kw["boundary"] = {"weight": self.boundary_w, "spacing": None}

    def loss(self):
        a, m, model, teacher, img, lab = self.args, self.method, self.model, self.teacher, self.img, self.lab
        kw = {"eps": self.eps, "n_class": self.nc}
        if m == "vae_train":
            return T.vae_train_losses(model, lab, scale=0.35, noise=self.latent, **kw)
        if m == "seg_train":
            return T.seg_train_losses(model, img, lab, loss=self.seg_loss, **kw, **self.seg_kw)
        if m == "joint_train":
            return T.joint_train_losses(model, img, lab, lambda_vae=self.lambda_vae, loss=self.seg_loss, **kw, **self.seg_kw)
        if m == "sep_joint_train":
            return T.sep_joint_train_losses(model, teacher, img, lab, **kw)
        if m in ("embed_train", "refine_vae"):
            return (T.embed_train_losses if m == "embed_train" else T.refine_vae_losses)(model, img, lab, noise=self.latent, **kw)
        if m == "discriminator_train":
            return T.discriminator_train_loss(model, lab, self.score)
        kw.update(lambda_vae=self.lambda_vae, use_confident_binarize=a.use_confident_binarize)
        if m == "domain_adaptation_dis":
            return T.domain_adaptation_dis_losses(model, teacher, img, lab, epoch=self.epoch, lambda_vae_warmup=a.lambda_vae_warmup, **kw)
        if self.pseudo_loader is not None:                                  # main_target.py:615-661: a --pseudo_list run has its own loss ladder
            return T.domain_adaptation_pseudo_losses(model, teacher, img, lab, domain_loss_type=a.domain_loss_type, host_schedule=not self.use_graph, **kw)
        return _monte_carlo(lambda: T.domain_adaptation_losses(model, teacher, img, lab, domain_loss_type=a.domain_loss_type, kl=a.kl,
                                                               only_pseudo=a.only_pseudo, epoch=self.epoch, turn_epoch=a.turn_epoch,
                                                               lambda_vae_warmup=a.lambda_vae_warmup, host_schedule=not self.use_graph, **kw),
                            max(1, int(a.vae_mont_number)))

    def begin_epoch(self, epoch):
        a = self.args
        self.epoch = epoch
        if a.lr_schedule == "poly":                                         # a captured step follows through sync_hyper(): no re-capture
            for grp, base in zip(self.optimizer.param_groups, self.base_lrs):
                grp["lr"] = optim.poly_lr(base, epoch, self.n_outer, a.poly_power)
        if self.boundary_w is not None:                                     # likewise: the captured launches read the scalar
            self.boundary_w.fill_(T.boundary_weight(epoch, a.boundary_weight, a.boundary_ramp, a.boundary_max))
        if self.method == "embed_train":                                    # main_source.py:550-554: the image encoder trains on odd epochs only
            for prm in self.model.Encoder.parameters():
                prm.requires_grad = epoch % 2 == 1
            self.params = [p for p in self.trainable.parameters() if p.requires_grad]

    def zero_grads(self):
        """optimizer.zero_grad() over ALL parameters, as the reference does every iteration (main_source.py:660): a GraphedStep drops the gradients of
        ITS parameters only, and an eager optimiser tail steps every parameter that holds one — a parameter frozen for this epoch (embed_train's
        Encoder on even epochs) must not keep the gradient its last trained step, or the previous capture's last replay, left it"""
        for grp in self.optimizer.param_groups:
            for p in grp["params"]:
                p.grad = None

    def divide_lambda(self):
        """--tag (main_target.py:635,712): ahead of this iteration's loss; lambda is baked into a captured loss expression"""
        self.lambda_vae /= 10
        self.stepper_key = None

    def capture(self, zero_grads=False):
        self.stepper = None                                                 # release the old capture's memory pool first
        if zero_grads:
            self.zero_grads()
        self.stepper = T.GraphedStep(self.loss, self.params, self.optimizer, grad_sync=self.sync, warmup=1, scaler=self.scaler)
        self.stepper_key = loss_key(self.args, self.method, self.epoch)

    def step(self):
        """one optimiser step on what the input buffers hold -> the step's aux dict"""
        if self.stepper is not None:
            self.stepper.step()
            return self.stepper.aux
        self.zero_grads()
        loss, aux = self.loss()
        if self.scaler is not None:
            loss.backward(gradient=self.scaler.seed)
        else:
            loss.backward()
        skw = {} if self.scaler is None else {"scaler": self.scaler}
        if self.sync is not None:
            self.sync()
            self.optimizer.step_with(*self.sync.live(), **skw)
        else:
            self.optimizer.step(**skw)
        return aux


def _refresh_teacher(st, epoch, idx, n_iter):
    """--pseudo_save_epoch: the three ways a pseudo-label network follows its student, ahead of the iteration's step -> the weights to load into the
    teacher AFTER the step, or None"""
    a, model, teacher = st.args, st.model, st.teacher
    if not a.pseudo_save_epoch:
        return None
    due = epoch % a.pseudo_save_epoch == 0
    if st.pseudo_loader is not None:
        if due:
            # main_target.py:633-635 (--pseudo_list runs): the pseudo-label network is re-loaded from the student AFTER this iteration's two forwards and
            # BEFORE its optimizer step, i.e. the next iteration's pseudo-labels come from the weights this one started with: keep them, load after the step
            with torch.no_grad():
                teacher_next = {k: v.clone() for k, v in model.state_dict().items()}
            if a.tag:
                st.divide_lambda()
            return teacher_next
    elif st.method == "domain_adaptation":
        # EMA teacher (main_target.py:508-518): every `pseudo_save_epoch` epochs, at the first iteration of an epoch slice or
        # every iteration; never in epoch 0
        every = max(1, a.pseudo_save_epoch // a.eval_epoch)
        if epoch != 0 and epoch % every == 0 and (a.update_every_iteration or idx % max(1, n_iter // a.eval_epoch) == 0):
            optim.ema_update(teacher.Seg, model.Seg, a.alpha)
    elif st.method == "domain_adaptation_dis" and due:
        # main_target.py:710-712: the pseudo-label network is re-loaded from the student (in place: a captured graph replays it)
        _load_teacher(teacher, model.Seg.state_dict())
        if a.tag:
            st.divide_lambda()
    return None


def _load_teacher(teacher, state):
    with torch.no_grad():
        teacher.load_state_dict(state)                                      # in place: a captured graph replays the same storage
    ops.clear_pack_cache()
    ops.refresh_frozen_packs(teacher)


def _pseudo_batch_losses(st):
    """main_target.py:663-687: the next batch of the pseudo-labelled loader (cycled), student forward, two Dice terms — logged, never stepped on"""
    pb = next(st.pseudo_itr, None) if st.pseudo_itr is not None else None
    if pb is None:
        st.pseudo_cycles += 1
        if hasattr(st.pseudo_loader, "set_epoch"):
            st.pseudo_loader.set_epoch(st.pseudo_cycles)                    # a DataLoader(shuffle=True) draws a new order per pass (main_target.py:299-307)
        st.pseudo_itr = iter(st.pseudo_loader)
        pb = next(st.pseudo_itr)
    if st.pimg is None:
        st.pimg, st.plab = torch.zeros_like(st.img), torch.zeros_like(st.lab)
    st.pimg.copy_(pb[IMG_KEY], non_blocking=True)
    st.plab.copy_(pb[LABEL_KEY], non_blocking=True)
    return T.pseudo_batch_losses(st.model, st.pimg, st.plab, eps=st.eps, n_class=st.nc)


def train_epoch(st, loader, epoch):
    a, method, model, optimizer = st.args, st.method, st.model, st.optimizer
    model.train()
    if hasattr(model, "Vae"):
        model.Vae.eval()
    if st.use_graph and (st.stepper is None or st.stepper_key != loss_key(a, method, epoch)):
        st.capture(zero_grads=True)
        if st.rank == 0:
            print("train step captured as a HIP graph (%s)" % ("2 graphs + bucketed all-reduce" if st.stepper.graph2 is not None else "1 graph"))
    t0, seen = time.time(), 0
    n_iter = len(loader)
    for idx, batch in enumerate(loader):
        st.img.copy_(batch[IMG_KEY], non_blocking=True)
        st.lab.copy_(batch[LABEL_KEY], non_blocking=True)
        if method == "discriminator_train":          # synthetic stand-in for the venous_score field: a function of the mask
            st.score.copy_(batch[LABEL_KEY].float().mean((1, 2, 3, 4)).view(-1, 1) * 4, non_blocking=True)
        teacher_next = _refresh_teacher(st, epoch, idx, n_iter)
        if st.use_graph and st.stepper is not None and st.stepper_key is None:       # --tag divided lambda_vae: the step that follows already runs with it
            st.capture()
        aux = st.step()
        if teacher_next is not None:
            _load_teacher(st.teacher, teacher_next)
        if st.pseudo_loader is not None:
            aux = dict(aux, **_pseudo_batch_losses(st))
        seen += a.batch_size
        if st.rank == 0 and idx % a.display_freq == 0:              # logging syncs the host every display_freq steps only
            parts = ", ".join("%s %.4f" % (k, v.item()) for k, v in aux.items() if k not in ("batch", "ds_losses", "topk_record"))
            if "topk_record" in aux:                                  # --ce_topk: the selection of the last step
                rec = ops.topk_record(aux["topk_record"])
                parts += ", topk %d/%d, tau %.4g" % (rec["K"], rec["N"], rec["tau"])
            for lvl, (d_i, ce_i) in enumerate(aux.get("ds_losses", ()), 1):      # --deep_supervision: the coarse levels' terms
                parts += ", ds%d_dice_loss %.4f, ds%d_ce_loss %.4f" % (lvl, d_i.item(), lvl, ce_i.item())
            if optimizer.max_norm is not None and optimizer.grad_norm is not None:
                parts += ", grad_norm %.4f" % optimizer.grad_norm.item()      # the last step's unclipped global norm, read where the losses are read
            print("[%3d, %3d] loss: %s" % ((epoch + 1) * a.eval_epoch, idx + 1, parts))
        if a.max_iters and idx + 1 >= a.max_iters:
            break
    torch.cuda.synchronize()
    if st.rank == 0:
        print("epoch %d: %.2f volumes/s per rank (%s)" % (epoch + 1, seen / max(time.time() - t0, 1e-9), "graph replay" if st.stepper is not None else "eager"))


def _write_json(prefix, name, epoch, obj):
    os.makedirs(os.path.join("tensorboard", prefix), exist_ok=True)
    with open(os.path.join("tensorboard", prefix, "%s_%d.json" % (name, epoch)), "w") as f:
        json.dump(obj, f)


def validate_epoch(args, model, val_loader, nc, runner, epoch):
    """rank 0's validation of one outer epoch and its tensorboard/<prefix>/*_<epoch>.json files -> the mean score"""
    model.eval()
    logs = {"surface": {}, "lesion": {}, "intensity": {}}                  # --val_surface / --val_lesion / --val_intensity: per-case records, filled by validate
    clean = {"keep_largest": args.val_keep_largest, "min_component": args.val_min_component, "closing": args.val_closing,
             "fill_holes": bool(args.val_fill_holes)}
    if runner is not None and (epoch != 0 or args.test_only):             # main_target.py:811
        scores, scores_noft = validate_finetune(runner, val_loader)
        print("epoch %d validation result without finetuning: %f" % (epoch + 1, float(np.mean(list(scores_noft.values())))))
    else:
        save_dir = os.path.join("result", args.prefix) if args.save_eval_result and epoch % 10 == 0 else None
        scores = validate(args.method, model, val_loader, nc, save_dir=save_dir, epoch=epoch, surface=bool(args.val_surface), surface_log=logs["surface"],
                          lesion=bool(args.val_lesion), lesion_log=logs["lesion"], intensity=int(args.val_intensity or 0),
                          intensity_log=logs["intensity"], **clean)
    _write_json(args.prefix, "score", epoch, scores)
    for name, log in logs.items():
        if log:
            _write_json(args.prefix, name, epoch, log)
    if args.val_whole_volume:                                              # after validation, which it leaves as it is
        sw = {"overlap": args.sw_overlap, "batch": args.sw_batch, "blend": args.sw_blend, "tta": args.val_tta}
        whole_log = {}
        validate_whole_volume(model, val_loader.whole_cases(), nc, args.size, log=whole_log, **sw, **clean)
        _write_json(args.prefix, "whole", epoch, whole_log)
        if args.val_fine_whole:
            fine_log = {}
            validate_fine_whole(model, val_loader.whole_cases(), nc, args.size, interp=args.fine_interp, log=fine_log, save_dir=args.save_whole_pred,
                                names=val_loader.names, **sw, **clean)
            _write_json(args.prefix, "fine", epoch, fine_log)
    return float(np.mean(list(scores.values()))) if scores else 0.0


def run(args, side="source"):
    """start_process -> build_models -> load_and_freeze -> build_optimizer -> a TrainState, then per outer epoch train_epoch on every rank and
    validate_epoch and the checkpoint on rank 0 -> the best validation score"""
    rank, world = start_process(args, side)
    nc, method = n_class_of(args), args.method
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[args.dtype]
    model, trainable, teacher = load_and_freeze(args, *build_models(args, nc), dtype)
    deep, optimizer, params, sync = build_optimizer(args, model, trainable, teacher, world)
    # fp16 storage: Dice gradients are O(1e-6), below fp16's normal range — dynamic loss scaling on the device (optim.LossScaler)
    scaler = optim.LossScaler() if dtype == torch.float16 else None

    runner = None
    if method == "domain_adaptation" and args.val_finetune and rank == 0:
        model_ft = build_joint(args).cuda()
        set_kernel_dtype(model_ft, dtype)
        runner = T.TestTimeFinetune(model, model_ft, teacher, args.size, steps=args.val_finetune, lr=args.lr_finetune, lambda_vae=args.lambda_vae,
                                    domain_loss_type=args.domain_loss_type, kl=args.kl, only_pseudo=args.only_pseudo,
                                    use_confident_binarize=args.use_confident_binarize, n_class=nc)

    train_loader, val_loader, sampler = make_loaders(args, rank, world)
    pseudo_loader = make_pseudo_loader(args, rank, world) if method == "domain_adaptation" and args.pseudo_list is not None else None
    st = TrainState(args, side, nc, rank, model, trainable, teacher, deep, optimizer, params, sync, scaler, pseudo_loader)
    best = 0.0
    for epoch in range(st.n_outer):
        st.begin_epoch(epoch)
        if sampler is not None:
            sampler.set_epoch(epoch)
        skip_da = method in ("domain_adaptation", "domain_adaptation_dis") and epoch == 0 and not args.train_first_epoch    # main_target.py:506,697: `if epoch == 0: continue`
        if not args.test_only and not skip_da:
            train_epoch(st, train_loader, epoch)
        if rank == 0:
            mean = validate_epoch(args, model, val_loader, nc, runner, epoch)
            print("epoch %d validation result: %f, best result %f." % (epoch + 1, mean, best))
            if not args.test_only and (epoch + 1) % max(1, args.save_epoch // args.eval_epoch) == 0:
                save_checkpoint(args.prefix, (epoch + 1) * args.eval_epoch, model, optimizer, mean > best, deep=deep)
            best = max(best, mean)
        if world > 1:
            dist.barrier()
            ddp.note_eager_collective()         # the next epoch may rebuild / re-capture its GraphedStep: ddp.quiesce_before_capture waits on this
        if args.test_only:
            break
    if world > 1:
        dist.destroy_process_group()
    if rank == 0:
        print("Finished Training")
    return best


def check_target_flags(a):
    """main_target.py:145-170: the reference's own consistency asserts, plus what this entry point does with the flags it does not act on."""
    if a.vae_mont_number != 1:
        _need("main_target.py", a.vae_forward_scale != 0.0, "--vae_mont_number != 1 needs a non-zero --vae_forward_scale")                                 # main_target.py:145
    if a.from_scratch:
        _need("main_target.py", a.method == "domain_adaptation" and not a.test_only, "--from_scratch belongs to --method domain_adaptation, not to --test_only")   # :157-159
    if a.kl:
        _need("main_target.py", a.method == "domain_adaptation" and a.domain_loss_type in (0, 8), "--kl belongs to domain_adaptation with --domain_loss_type 0 or 8")   # :162-164
    if a.update_every_iteration:
        _need("main_target.py", a.pseudo_save_epoch == 1, "--update_every_iteration needs --pseudo_save_epoch 1")                                           # :168
    if a.generate_bounding_boxes:
        _need("main_target.py", a.method == "domain_adaptation", "--generate_bounding_boxes belongs to --method domain_adaptation")                        # :170
    if a.pseudo_list is not None:
        _need("main_target.py", a.method == "domain_adaptation", "--pseudo_list is read by --method domain_adaptation only (main_target.py:615; domain_adaptation_dis runs "
                                              "without it, :689)")
    ignored = [n for n in ("save_more_reference", "analysis_figure_name", "generate_bounding_boxes", "resume") if getattr(a, n)]
    if ignored:
        print("main_target.py: accepted and ignored (they drive figure / volume dumps the native entry point does not write): %s"
              % ", ".join("--" + n for n in ignored), file=sys.stderr)


def _typed(text, convert, accept, what):
    """an argparse type: convert(text) where accept() holds for it, else the error `what, got <text>`"""
    try:
        v = convert(text)
        if accept(v):
            return v
    except ValueError:
        pass
    raise argparse.ArgumentTypeError("%s, got %r" % (what, text))


def _probability(text):
    return _typed(text, float, lambda v: 0.0 <= v <= 1.0, "a probability in [0, 1]")


def _margin(text):
    return _typed(text, int, lambda v: v >= 0, "a non-negative number of voxels")


def _percentile_pair(text):
    return _typed(text, lambda t: tuple(float(v) for v in t.split(",")), lambda p: len(p) == 2 and 0.0 <= p[0] < p[1] <= 100.0,
                  "two ascending percentiles P_LO,P_HI in [0, 100]")


def _percent(text):
    return _typed(text, float, lambda v: 0.0 < v <= 100.0, "a percentage in (0, 100]")


def _nonnegative(text):
    return _typed(text, float, lambda v: 0.0 <= v < float("inf"), "a finite number >= 0")


def _class_weights(text):
    try:
        ws = [_nonnegative(t) for t in text.split(",")]
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError("comma-separated finite numbers >= 0, got %r" % text)
    return ws


SEG_LOSS_METHODS = ("seg_train", "joint_train")


def check_seg_loss_flags(parser, a, methods=SEG_LOSS_METHODS):
    """--seg_loss and the flags that shape the compound loss belong to the methods whose loss is a Dice against the label: seg_train and joint_train
    of main_source.py (main_target.py passes methods=())"""
    given = [n for n, default in (("seg_loss", "dice"), ("ce_weight", 1.0), ("batch_dice", False), ("focal_gamma", 0.0), ("class_weights", None),
                                  ("deep_supervision", 0), ("ce_topk", None))
             if getattr(a, n) != default]
    if not given:
        return a
    if a.method not in methods:
        parser.error("%s: the compound segmentation loss belongs to --method seg_train and joint_train of main_source.py, not to --method %s"
                     % (", ".join("--" + n for n in given), a.method))
    if a.seg_loss != "dice_ce":
        parser.error("%s shape(s) the compound loss: add --seg_loss dice_ce" % ", ".join("--" + n for n in given))
    nc = n_class_of(a)
    if nc > 8:
        parser.error("--seg_loss dice_ce handles at most 8 classes, the background included")
    if a.class_weights is not None and len(a.class_weights) != nc:
        parser.error("--class_weights takes exactly %d numbers (one per class, the background included), got %d" % (nc, len(a.class_weights)))
    if a.ce_topk is not None and a.deep_supervision:
        parser.error("--ce_topk selects among stored probabilities, and the heads of --deep_supervision store none: the two cannot be combined")
    return a


BOUNDARY_FLAGS = (("boundary_weight", 0.0), ("boundary_ramp", 0.0), ("boundary_max", None))


def boundary_enabled(args):
    """--boundary_weight / --boundary_ramp switch the boundary term on (a ramp from weight 0 is a schedule too)"""
    return args.boundary_weight > 0 or args.boundary_ramp > 0


def check_boundary_flags(parser, a, methods=SEG_LOSS_METHODS):
    """--boundary_weight, --boundary_ramp and --boundary_max add the boundary term to the compound loss: they belong where --seg_loss dice_ce does
    (seg_train and joint_train of main_source.py; main_target.py passes methods=())"""
    given = [n for n, default in BOUNDARY_FLAGS if getattr(a, n) != default]
    if not given:
        return a
    names = ", ".join("--" + n for n in given)
    if a.method not in methods:
        parser.error("%s: the boundary loss belongs to --method seg_train and joint_train of main_source.py, not to --method %s" % (names, a.method))
    if a.seg_loss != "dice_ce":
        parser.error("%s add(s) the boundary term to the compound loss: add --seg_loss dice_ce" % names)
    if not boundary_enabled(a):
        parser.error("%s: the boundary term is off — give --boundary_weight or --boundary_ramp above 0" % names)
    return a


def seg_loss_of(args):
    """the `loss` argument of train.seg_train_losses / joint_train_losses from the flags; None for --seg_loss dice (the default): the reference's Dice"""
    if args.seg_loss != "dice_ce":
        return None
    kw = {"dice_weight": 1.0, "ce_weight": args.ce_weight, "batch_dice": bool(args.batch_dice), "class_weights": args.class_weights,
          "gamma": args.focal_gamma}
    if args.ce_topk is not None:                                            # off: the dict is what it was, and so is every launch
        kw["topk"] = args.ce_topk / 100.0
    return kw


# the flags main_target.py declares and main_source.py lacks, with main_target.py's defaults (tests/test_host_driver.py holds the two against each other):
# check_aug_flags, the tail of both parse() functions, gives a namespace those it lacks, so every read below is a plain attribute
TARGET_ONLY_DEFAULTS = {
    "pseudo_data_root": "../nih_data/numpy_data/", "pseudo_list": None, "load_prefix_encoder": None, "pseudo_pan_index": "1", "domain_loss_type": 0, "kl": False,
    "use_confident_binarize": False, "pseudo_save_epoch": 0, "update_every_iteration": False, "alpha": 0.995, "seg_dropout": 0.0, "vae_decoder_dropout": 0.0,
    "val_finetune": 0, "lr_finetune": 1e-2, "only_pseudo": False, "fix_layer": False, "vae_mont_number": 1, "vae_forward_scale": 0.0, "tag": False,
    "from_scratch": False, "shift": 0}


def check_aug_flags(parser, a, seg_loss_methods=SEG_LOSS_METHODS):
    """--aug_elastic and --aug_intensity act on the augmented training samples: with --no_aug there are none; --standardize reads real cases;
    the compound-loss flags belong to seg_loss_methods (check_seg_loss_flags).  -> a, completed by TARGET_ONLY_DEFAULTS"""
    check_seg_loss_flags(parser, a, seg_loss_methods)
    check_boundary_flags(parser, a, seg_loss_methods)
    if a.aug_elastic > 0 and a.no_aug:
        parser.error("--aug_elastic deforms the augmented training samples: it cannot be combined with --no_aug")
    if a.aug_intensity and a.no_aug:
        parser.error("--aug_intensity changes the grey values of the augmented training samples: it cannot be combined with --no_aug")
    if a.aug_lowres > 0 and not a.aug_intensity:
        parser.error("--aug_lowres is a stage of the intensity augmentation: it needs --aug_intensity")
    if a.standardize is not None and not a.real_data:
        parser.error("--standardize reads the percentiles of merge.npy cases: it needs --real_data")
    if a.standardize_above is not None and a.standardize is None:
        parser.error("--standardize_above selects the voxels --standardize reads: it needs --standardize")
    if a.nesterov and a.adam:
        parser.error("--nesterov is a form of SGD's momentum: it cannot be combined with --adam")
    if a.nesterov and not a.momentum > 0:
        parser.error("--nesterov needs a --momentum above 0")
    if a.train_patches and not a.real_data:
        parser.error("--train_patches cuts its windows from merge.npy cases: it needs --real_data")
    if a.train_patches and len(str(a.pan_index).split(",")) + 1 > 8:
        parser.error("--train_patches indexes at most 8 classes, the background included")
    for name, default in TARGET_ONLY_DEFAULTS.items():
        if not hasattr(a, name):
            setattr(a, name, default)
    return a


def add_native_flags(parser):
    g = parser.add_argument_group("native (MI355X) additions")
    g.add_argument("--synthetic", action="store_true", default=True, help="synthetic volumes (default: no dataset ships with this repository)")
    g.add_argument("--real_data", action="store_true", help="train / validate on the merge.npy cases of lists/<data_path>[train_list | val_list] under "
                   "data_root / val_data_root, transformed on the device (data_gpu.py) — the reference's loader stack (main_source.py:186-243)")
    g.add_argument("--aug_elastic", type=_probability, default=0.0, metavar="P", help="with --real_data: elastic deformation of a training sample with "
                   "probability P before rotation and scale (augment_spatial's first stage with the alpha=(0, 500), sigma=(10, 30) the reference's entry "
                   "points pass, noise from Philox on the device: data_gpu.MySpatialTransform(noise='philox')); 0 = off, the reference's setting")
    g.add_argument("--aug_intensity", action="store_true", help="with --real_data: the nnU-Net intensity stage on every training sample after "
                   "CenterIntensities — Gaussian noise, Gaussian blur, brightness, contrast, gamma (inverted and plain, statistics retained) and a "
                   "mirror per axis, each behind its gate, on the device (data_gpu.IntensityAugment(noise='philox')); off: the reference's setting")
    g.add_argument("--aug_lowres", type=_probability, default=0.0, metavar="P", help="with --aug_intensity: nnU-Net's simulated low resolution of a training "
                   "sample with probability P (nnU-Net: 0.25), between contrast and the gammas — per channel with probability 0.5 a zoom from U(0.5, 1), "
                   "down by nearest neighbour, back up by a cubic spline with edge boundaries, clipped, on the device (ops.simulate_lowres); 0 = off")
    g.add_argument("--standardize", type=_percentile_pair, default=None, metavar="P_LO,P_HI", help="with --real_data: map every case's image, right after "
                   "the load and before every other transform, linearly so that its P_LO and P_HI percentiles (nnU-Net: 0.5,99.5) land on the window "
                   "Clip expects (-200, 400), exact percentiles found on the device (data_gpu.IntensityStandardizer) — for scans whose unit is not "
                   "Hounsfield; training, validation and pseudo-label loaders alike; off: the reference's setting")
    g.add_argument("--standardize_above", type=float, default=None, metavar="T", help="with --standardize: the percentiles are those of the voxels above T "
                   "(strictly), e.g. to leave the air around the body out")
    g.add_argument("--train_patches", action="store_true", help="with --real_data: patch training — every training sample is a --size window of the UNSCALED "
                   "case in place of the label-centred, rescaled crop of CropResize (nnU-Net's loader: the windows --val_whole_volume predicts on), the "
                   "last samples of each batch forced onto a random foreground voxel, cut on the device (data_gpu.PatchSampler); validation is unchanged")
    g.add_argument("--patch_fg", type=_probability, default=0.33, metavar="P", help="with --train_patches: the share of a batch forced to contain foreground — "
                   "sample j of B iff j >= floor(B (1 - P) + 0.5) (nnU-Net: 0.33)")
    g.add_argument("--patch_margin", type=_margin, default=16, metavar="M", help="with --train_patches: voxels cut around each window for rotation and scale to "
                   "read in place of the border value; 0 under --no_aug")
    g.add_argument("--seg_loss", default="dice", choices=["dice", "dice_ce"], help="seg_train / joint_train: the loss against the label — dice: the "
                   "reference's per-sample soft Dice, whose gradient is zero on a sample without foreground; dice_ce: Dice plus a voxel-wise cross-entropy, "
                   "fused on the device (ops.seg_loss, DESIGN 3.20)")
    g.add_argument("--ce_weight", type=_nonnegative, default=1.0, metavar="W", help="with --seg_loss dice_ce: the weight of the cross-entropy term")
    g.add_argument("--batch_dice", action="store_true", help="with --seg_loss dice_ce: pool the Dice sums over the rank's batch (nnU-Net's batch Dice), so "
                   "a sample without foreground still receives a Dice gradient")
    g.add_argument("--focal_gamma", type=_nonnegative, default=0.0, metavar="G", help="with --seg_loss dice_ce: the focal exponent of the cross-entropy, "
                   "-(1 - p)^G ln p; 0 = plain cross-entropy")
    g.add_argument("--class_weights", type=_class_weights, default=None, metavar="W0,W1,...", help="with --seg_loss dice_ce: one cross-entropy weight "
                   ">= 0 per class, the background first — exactly n_class numbers (torch's weighted mean); default all 1")
    g.add_argument("--ce_topk", type=_percent, default=None, metavar="PCT", help="with --seg_loss dice_ce: the cross-entropy term is the mean over the "
                   "hardest PCT percent of the rank's valid voxels only (nnU-Net's DC_and_topk_loss: 10), selected on the device inside the captured step "
                   "(ops.seg_loss(topk=), DESIGN 3.23); the loss line then also prints K/N and the threshold.  Not with --deep_supervision.  Default: off")
    g.add_argument("--deep_supervision", type=int, default=0, choices=[0, 1, 2], metavar="L", help="with --seg_loss dice_ce: the same loss on L coarser "
                   "levels of the decoder — 1: the half-resolution skip sum, 2: the quarter-resolution one as well — through 1x1x1 heads fused with their "
                   "loss (ops.ds_head, DESIGN 3.21), against the label picked at stride 2 / 4, the levels weighted 2^-i and normalised (L = 2: 4/7, "
                   "2/7, 1/7); the heads train with the network, are saved beside it and are never used for prediction.  0 (default) = off")
    g.add_argument("--boundary_weight", type=_nonnegative, default=0.0, metavar="A", help="with --seg_loss dice_ce: add A times the boundary loss (Kervadec et "
                   "al., MIDL 2019) of the full-resolution prediction — the mean of p_c * phi_c over the foreground channels, phi_c the signed distance map of "
                   "the label, made on the device in every step (ops.boundary_loss, DESIGN 3.22).  0 (default) = off")
    g.add_argument("--boundary_ramp", type=_nonnegative, default=0.0, metavar="STEP", help="with --seg_loss dice_ce: the boundary weight of outer epoch e is "
                   "min(A + e * STEP, --boundary_max), refilled on the device at the top of the epoch: a captured step is not rebuilt")
    g.add_argument("--boundary_max", type=_nonnegative, default=None, metavar="M", help="with --boundary_ramp: the cap of the boundary weight (default: none)")
    g.add_argument("--momentum", type=_nonnegative, default=0.9, metavar="M", help="SGD's momentum (the reference: 0.9; nnU-Net: 0.99 with --nesterov)")
    g.add_argument("--weight_decay", type=_nonnegative, default=0.0, metavar="W", help="L2 weight decay of SGD / Adam (the reference: 0; nnU-Net: 3e-5)")
    g.add_argument("--nesterov", action="store_true", help="SGD with Nesterov momentum: the step is lr * (g + momentum * buf) instead of lr * buf")
    g.add_argument("--grad_clip", type=_nonnegative, default=0.0, metavar="N", help="clip the global 2-norm of the gradients — over every param group, "
                   "after the all-reduce and after unscaling — to N on the device, inside the (captured) optimiser step; the loss line then also prints "
                   "the last step's unclipped norm.  0 (default) = off; nnU-Net: 12")
    g.add_argument("--lr_schedule", default="constant", choices=["constant", "poly"], help="poly: at the top of every outer epoch each group's learning "
                   "rate becomes its initial rate * (1 - epoch / epochs) ** --poly_power (nnU-Net's schedule); constant (default): the reference's")
    g.add_argument("--poly_power", type=_nonnegative, default=0.9, metavar="P", help="with --lr_schedule poly: the exponent")
    g.add_argument("--latent_noise", default="torch", choices=["torch", "philox"], help="vae_train / embed_train / refine_vae: where the VAE's latent noise "
                   "comes from — torch: torch.randn per call, the step launched eagerly (the reference's draw); philox: a stated Philox4x32-10 stream per "
                   "rank (ops.LatentStream, seed 1000 rank + 700) drawn inside the forward launch from a counter in device memory, so the step is captured "
                   "as a HIP graph and every replay draws a fresh sample")
    g.add_argument("--size", type=int, default=128, help="cubic patch side (reference: patch_size 128, main_source.py:117)")
    g.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "fp16"], help="kernel storage dtype")
    g.add_argument("--synthetic_train", type=int, default=16)
    g.add_argument("--synthetic_val", type=int, default=2)
    g.add_argument("--max_iters", type=int, default=0, help="stop each epoch after this many steps (0 = whole loader)")
    g.add_argument("--display_freq", type=int, default=10)
    g.add_argument("--no_graph", action="store_true", help="eager launches instead of the HIP-graph replayed step")
    g.add_argument("--recompute", action="store_true", help="activation recomputation (checkpointing) of the Down / Up blocks: interior activations are "
                   "re-computed in backward instead of kept (BASELINE configs[4]); trades bandwidth for memory")
    g.add_argument("--val_keep_largest", type=int, default=0, help="validation: keep only the K largest 26-connected components of every foreground class of the "
                   "hard prediction before the Dice score (utils/utils.py:776-796, on the device); 0 = off, the reference's validation")
    g.add_argument("--val_min_component", type=int, default=0, help="with --val_keep_largest: components of fewer voxels are dropped as well (predict_vol uses 10000)")
    g.add_argument("--val_closing", type=int, default=0, metavar="N", help="validation: binary closing of every foreground class of the hard prediction with N "
                   "iterations of the 26-neighbourhood (scipy.ndimage.binary_closing, on the device) before the component filter and the score; 0 = off; "
                   "whole_<epoch>.json and fine_<epoch>.json record it as \"closing\"")
    g.add_argument("--val_fill_holes", action="store_true", help="validation: fill the holes of every foreground class of the hard prediction "
                   "(scipy.ndimage.binary_fill_holes, 6-connected background, on the device) after --val_closing and before the component filter; only "
                   "background voxels change class; recorded as \"fill_holes\"")
    g.add_argument("--val_surface", action="store_true", help="validation: also report ASSD and HD95 (medpy's convention, in voxels) of the hard prediction against "
                   "the label per foreground class, computed on the device; per-case values go to tensorboard/<prefix>/surface_<epoch>.json")
    g.add_argument("--val_lesion", action="store_true", help="validation: also report lesion-wise detection — per foreground class the 26-connected components of "
                   "the hard prediction (after --val_closing / --val_fill_holes / --val_keep_largest) against those of the label: lesions found and missed, false "
                   "detections, sensitivity, precision, F1 — and per-class Dice, IoU, sensitivity and precision from the confusion matrix, computed on the "
                   "device; --val_min_component drops smaller components from both sides; per-case values go to tensorboard/<prefix>/lesion_<epoch>.json")
    g.add_argument("--val_intensity", type=int, default=0, metavar="BINS", help="validation: also write, per case and foreground class, the BINS-bin histogram over "
                   "[-1, 1] of the network's input image inside the hard prediction (after --val_closing / --val_fill_holes / --val_keep_largest) and inside the "
                   "label, and the normalised mutual information of the foreground probability with the label, computed on the device, to "
                   "tensorboard/<prefix>/intensity_<epoch>.json; 0 = off")
    g.add_argument("--val_whole_volume", action="store_true", help="validation (with --real_data): additionally predict every WHOLE validation case by sliding window "
                   "with the segmentation network (windows of --size) and report dice_whole — hard Dice against the whole label — and dice_label_free — the fine "
                   "pass on a crop chosen by the prediction's box instead of the label's; per-case values go to tensorboard/<prefix>/whole_<epoch>.json")
    g.add_argument("--val_fine_whole", action="store_true", help="with --val_whole_volume: also paste the label-free fine prediction back onto the scan grid "
                   "(evaluation.coarse_to_fine_predict, on the device) and report dice_fine_whole — hard Dice against the whole label, comparable with dice_whole; "
                   "per-case values go to tensorboard/<prefix>/fine_<epoch>.json")
    g.add_argument("--fine_interp", default="linear", choices=["linear", "nearest"], help="--val_fine_whole: how the fine probabilities are resampled onto the scan")
    g.add_argument("--save_whole_pred", default=None, metavar="DIR", help="--val_fine_whole: write every case's pasted label to DIR/<case>.npy (uint8, the scan's shape)")
    g.add_argument("--val_tta", default=None, metavar="AXES", help="--val_whole_volume: mirror test-time augmentation of the sliding-window passes — AXES is a "
                   "string over \"dhw\"; every window is predicted under each subset of those flips and the un-flipped probabilities are averaged, in the "
                   "same pass (2^len(AXES) forwards per window); whole_<epoch>.json and fine_<epoch>.json record the flip codes as \"tta\"")
    g.add_argument("--sw_overlap", type=float, default=0.5, help="--val_whole_volume: overlap of neighbouring windows as a fraction of the window, in [0, 1)")
    g.add_argument("--sw_batch", type=int, default=1, help="--val_whole_volume: windows per forward pass")
    g.add_argument("--sw_blend", default="gaussian", choices=["gaussian", "constant"], help="--val_whole_volume: importance map of a window")
    g.add_argument("--train_first_epoch", action="store_true", help="domain_adaptation: also train in epoch 0 (the reference only "
                   "validates there, main_target.py:506)")
