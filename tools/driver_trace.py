#!/usr/bin/env python3
"""Record what the entry points print, write and save over a set of short runs that between them reach every stage of
vae_segmentation_amd/driver.py's run() — the check that a change to the DRIVER leaves every method's run as it was.

    python tools/driver_trace.py run OUT.json [SCENARIO ...]        every scenario (or the named ones), on the deterministic build; needs a GPU
    python tools/driver_trace.py compare A.json B.json [--loose S1,S2]   exit status 1 on any difference

Every scenario runs in a fresh child process with a time limit of its own, torch.manual_seed(0) ahead of driver.run, VS_DETERMINISTIC=1 and one
scratch working directory for the whole run (the domain-adaptation scenarios load the checkpoint the joint_train scenario wrote there).  The run stops
at the first child that fails, runs into its time limit or dies on a signal.  Per scenario the record holds
    stdout   the lines, with the `volumes/s` figure masked
    json     every tensorboard/<prefix>/*.json, parsed
    ckpt     per checkpoint under 3dmodel/<prefix>/ the shape and sha256 of every tensor it holds and the value of everything else, optimiser state included
compare --loose names the scenarios that are not bit-reproducible on ONE revision (two runs of the parent differ): for them every number on stdout is
masked, the JSON files are compared by their keys and the checkpoints by tensor names and shapes, and the summary says so.

The tool touches nothing of the package but main_source.parse / main_target.parse and driver.run, so the same file runs against any revision.
It is a tool, not a test: the runs take minutes, and a feature that changes what a run prints would have to change a pinned record with it."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300

COMMON = ["-b", "1", "--eval_epoch", "1", "--save_epoch", "1", "--max_iters", "2", "--display_freq", "1", "--synthetic_train", "2", "--synthetic_val", "1"]
VAE64 = ["--size", "64"] + COMMON                                   # 64^3: the smallest volume a VAE accepts
FROM_SRC = ["--load_prefix_joint", "joint_train", "--checkpoint_name", "model_epoch1.ckpt", "--train_first_epoch"]
REAL = ["--real_data", "-R", "data", "-V", "data", "--size", "32"] + COMMON

# name -> (side, flags); the name is the run's prefix.  joint_train comes first: FROM_SRC loads its first checkpoint
SCENARIOS = {
    "joint_train": ("source", ["-M", "joint_train", "-E", "2", "--seg_loss", "dice_ce", "--deep_supervision", "2", "--boundary_ramp", "0.1", "--grad_clip", "12",
                               "--lr_schedule", "poly"] + VAE64),
    "seg_real": ("source", ["-M", "seg_train", "-E", "2", "--val_keep_largest", "1", "--val_closing", "1", "--val_fill_holes", "--val_surface", "--val_lesion",
                            "--val_intensity", "8", "--val_whole_volume", "--val_fine_whole", "--val_tta", "w"] + REAL),
    "vae_train": ("source", ["-M", "vae_train", "-E", "1", "--latent_noise", "philox"] + VAE64),
    "embed_train": ("source", ["-M", "embed_train", "-E", "2", "--latent_noise", "philox"] + VAE64),           # two epochs: the parity re-capture
    "da_ema": ("target", ["-M", "domain_adaptation", "-E", "2", "--domain_loss_type", "8", "--pseudo_save_epoch", "1", "--update_every_iteration"] + FROM_SRC + VAE64),
    "da_pseudo_tag": ("target", ["-M", "domain_adaptation", "-E", "1", "--pseudo_list", "synthetic_pseudo", "--pseudo_save_epoch", "1", "--tag"] + FROM_SRC + VAE64),
    "da_pseudo_tag_eager": ("target", ["-M", "domain_adaptation", "-E", "1", "--pseudo_list", "synthetic_pseudo", "--pseudo_save_epoch", "1", "--tag", "--no_graph"]
                            + FROM_SRC + VAE64),
    "da_dropout": ("target", ["-M", "domain_adaptation", "-E", "1", "--seg_dropout", "0.1"] + FROM_SRC + VAE64),
    "da_dis": ("target", ["-M", "domain_adaptation_dis", "-E", "1", "--tag", "--pseudo_save_epoch", "1", "--train_first_epoch"] + VAE64),
    "da_finetune": ("target", ["-M", "domain_adaptation", "-E", "1", "--domain_loss_type", "8", "--val_finetune", "1", "--test_only"] + FROM_SRC + VAE64),
}

CHILD = ("import sys, torch; torch.manual_seed(0); sys.path.insert(0, %r); import main_%s as m; from vae_segmentation_amd import driver; "
         "driver.run(m.parse(sys.argv[1:]), side=%r)")


def make_cases(work):
    """three synthetic merge.npy cases and their list, as the suite's real-data tests make them"""
    import numpy as np
    rng = np.random.RandomState(0)
    os.makedirs(os.path.join(work, "data"))
    os.makedirs(os.path.join(work, "lists"))
    names = []
    for i, shape in enumerate([(40, 48, 56), (44, 40, 52), (48, 52, 40)]):
        merge = np.zeros(shape + (2,), np.float32)
        merge[..., 0] = np.round(rng.randn(*shape) * 250 + 40)
        merge[10:30, 12:34, 8:30, 1] = 1
        np.save(os.path.join(work, "data", "case%d_merge.npy" % i), merge)
        names.append("case%d_merge.npy" % i)
    with open(os.path.join(work, "lists", "Multi_all.json"), "w") as f:
        json.dump({"NIH_train": names[:2], "NIH_val": names[2:]}, f)


def _tensors(obj, path, out):
    import torch
    if isinstance(obj, torch.Tensor):
        t = obj.detach().cpu().contiguous()
        out[path] = [list(t.shape), hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:16]]
    elif isinstance(obj, dict):
        for k in obj:
            _tensors(obj[k], "%s/%s" % (path, k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _tensors(v, "%s/%d" % (path, i), out)
    else:
        out[path] = [None, repr(obj)]
    return out


def collect(work, name, stdout):
    import torch
    rec = {"stdout": [re.sub(r"\d+\.\d+ volumes/s", "# volumes/s", ln) for ln in stdout.splitlines()], "json": {}, "ckpt": {}}
    tb = os.path.join(work, "tensorboard", name)
    for fn in sorted(os.listdir(tb)) if os.path.isdir(tb) else ():
        with open(os.path.join(tb, fn)) as f:
            rec["json"][fn] = json.load(f)
    ck = os.path.join(work, "3dmodel", name)
    for fn in sorted(os.listdir(ck)) if os.path.isdir(ck) else ():
        rec["ckpt"][fn] = _tensors(torch.load(os.path.join(ck, fn), map_location="cpu"), "", {})
    return rec


def run(path, only=None):
    result, status = {}, 0
    env = dict(os.environ, PYTHONPATH=ROOT, VS_DETERMINISTIC="1")
    with tempfile.TemporaryDirectory() as work:
        make_cases(work)
        for name, (side, flags) in SCENARIOS.items():
            if only and name not in only and name != "joint_train":
                continue
            try:
                r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, side, side), name] + flags, cwd=work, env=env, capture_output=True, text=True,
                                   timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                print("%-22s ran into its %d s time limit: stopping" % (name, CHILD_TIMEOUT), flush=True)
                status = 3
                break
            if r.returncode != 0:
                print("%-22s exit status %d: stopping\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-3000:]), flush=True)
                status = 3 if r.returncode < 0 or r.returncode in (134, 139) else 1
                break
            result[name] = collect(work, name, r.stdout)
            print("%-22s %3d lines, %d json files, %d checkpoints" % (name, len(result[name]["stdout"]), len(result[name]["json"]), len(result[name]["ckpt"])),
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f)
    return status


def _keys(obj):
    """a parsed JSON value with every leaf replaced by its type's name"""
    if isinstance(obj, dict):
        return {k: _keys(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_keys(v) for v in obj]
    return type(obj).__name__


def _loosen(rec):
    return {"stdout": [re.sub(r"-?\d+\.\d+(e-?\d+)?|nan|inf", "#", ln) for ln in rec["stdout"]], "json": _keys(rec["json"]),
            "ckpt": {fn: {k: v[0] for k, v in ts.items()} for fn, ts in rec["ckpt"].items()}}


def compare(pa, pb, loose=()):
    with open(pa) as f:
        a = json.load(f)
    with open(pb) as f:
        b = json.load(f)
    bad = 0
    print("%-22s %6s %5s %8s  %s" % ("scenario", "lines", "json", "entries", "verdict"))
    for name in sorted(set(a) | set(b), key=lambda n: list(SCENARIOS).index(n) if n in SCENARIOS else len(SCENARIOS)):
        if name not in a or name not in b:
            print("%-22s in one record only" % name)
            bad += 1
            continue
        ra, rb = (_loosen(r) if name in loose else r for r in (a[name], b[name]))
        how = " (numbers masked: not reproducible on one revision)" if name in loose else ""
        diffs = [part for part in ("stdout", "json", "ckpt") if ra[part] != rb[part]]
        print("%-22s %6d %5d %8d  %s" % (name, len(ra["stdout"]), len(ra["json"]), sum(len(t) for t in ra["ckpt"].values()),
                                        ("DIFFERENT in " + ", ".join(diffs) if diffs else "identical") + how))
        bad += len(diffs)
        if "stdout" in diffs:
            for i, (la, lb) in enumerate(zip(ra["stdout"], rb["stdout"])):
                if la != lb:
                    print("    first different line %d:\n      A %s\n      B %s" % (i, la, lb))
                    break
            else:
                print("    A has %d lines, B %d" % (len(ra["stdout"]), len(rb["stdout"])))
        if "json" in diffs:
            print("    files: %s" % ", ".join(fn for fn in sorted(set(ra["json"]) | set(rb["json"])) if ra["json"].get(fn) != rb["json"].get(fn)))
        if "ckpt" in diffs:
            for fn in sorted(set(ra["ckpt"]) | set(rb["ckpt"])):
                ta, tb = ra["ckpt"].get(fn, {}), rb["ckpt"].get(fn, {})
                names = [k for k in sorted(set(ta) | set(tb)) if ta.get(k) != tb.get(k)]
                if names:
                    print("    %s: %d of %d entries differ, first %s" % (fn, len(names), len(set(ta) | set(tb)), names[0]))
    print("%d difference(s)" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        sys.exit(run(sys.argv[2], set(sys.argv[3:]) or None))
    if len(sys.argv) in (4, 6) and sys.argv[1] == "compare" and (len(sys.argv) == 4 or sys.argv[4] == "--loose"):
        sys.exit(compare(sys.argv[2], sys.argv[3], set(sys.argv[5].split(",")) if len(sys.argv) == 6 else ()))
    sys.exit(__doc__)
