"""Training patches cut on the device against the two detours -> profiles/patch_bench.json.

A CT-like image and a label with two foreground ellipsoids, 96^3 patches in a 160^3 volume and 128^3 patches in 256 x 256 x 192, R = 1, 2 and 8 forced
requests per call, in ONE process on ONE machine:
  index, pick, gather   each call alone (ops.patch_index / patch_pick / patch_gather of image and label, margin 0): eager_ms — issued eagerly, device
                events around it — and graph_ms — captured in a HIP graph and replayed; medians of REPS after WARMUP
  chain         index -> pick -> gather as PatchSampler issues them: the same two figures
  gather.rate   the bytes the gather must move (every output voxel written once and read once from a source) over its replayed time, and that rate over
                the copy rate measured in this run (copy_bytes_per_s: a 256 MiB device-to-device copy, bytes read plus bytes written over its median time)
  host_ms       label.cpu() -> per request np.argwhere(label == k), a choice, slice / np.pad of image and label -> .cuda(): host clock around work that
                ends in a synchronise, median of REPS after WARMUP
  torch_ms      torch.nonzero(label == k) on the device, the chosen row read back (the slice bounds must reach the host: it synchronises), slices of image
                and label stacked on the device: host clock around work that ends in a synchronise, the same median
  equal         whether the device picks of this run equalled the oracle's (tests/patch_util.ref_picks) with ==
No time or ratio is fixed in advance; the file records what was measured.

    python tools/bench_patch.py [--out profiles/patch_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

CONFIGS = (((160, 160, 160), 96), ((256, 256, 192), 128))
REQUESTS = (1, 2, 8)
N_CLASS = 3
WARMUP, REPS = 5, 20


def timed(fn, reps=REPS, warmup=WARMUP):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def host_timed(fn, reps=REPS, warmup=WARMUP):
    """fn ends in a synchronise"""
    ms = []
    for rep in range(warmup + reps):
        t = time.perf_counter()
        fn()
        if rep >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def eager_and_graph(fn):
    """-> (eager result, {"eager_ms", "graph_ms"})"""
    import torch
    eager = fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return eager, {"eager_ms": timed(fn), "graph_ms": timed(graph.replay)}


def copy_rate():
    import torch
    a = torch.empty(256 << 18, dtype=torch.float32, device="cuda").normal_()          # 256 MiB
    b = torch.empty_like(a)
    ms = timed(lambda: b.copy_(a))
    return 2.0 * a.numel() * 4 / (ms * 1e-3)


def case(shape, seed=1):
    """-> (image, label) float32: round(N(40, 250)) and two ellipsoids of classes 1 and 2"""
    rng = np.random.RandomState(seed)
    img = np.round(rng.randn(*shape) * 250.0 + 40.0).astype(np.float32)
    zz, yy, xx = np.meshgrid(*(np.arange(s, dtype=np.float32) for s in shape), indexing="ij")
    lab = np.zeros(shape, np.float32)
    for k, (c, r) in enumerate((((0.45, 0.5, 0.55), (0.16, 0.12, 0.2)), ((0.6, 0.35, 0.4), (0.06, 0.08, 0.05))), start=1):
        inside = sum(((g - ci * s) / (ri * s)) ** 2 for g, ci, ri, s in zip((zz, yy, xx), c, r, shape)) < 1.0
        lab[inside] = k
    return img, lab


def origin_of(v, shape, patch):
    return [min(max(0, int(v[a]) - patch // 2), shape[a] - patch) for a in range(3)]      # the volume is larger than the patch on every axis here


def cut(vol, o, patch, cval):
    """the host loader's cut: the part of the window inside the volume sliced, then padded to the patch"""
    lo = [max(o[a], 0) for a in range(3)]
    hi = [min(o[a] + patch, vol.shape[a]) for a in range(3)]
    part = vol[tuple(slice(lo[a], hi[a]) for a in range(3))]
    return np.pad(part, [(lo[a] - o[a], o[a] + patch - hi[a]) for a in range(3)], mode="constant", constant_values=cval)


def host_detour(img_d, lab_d, requests, patch):
    """what a host loader does for the same requests: download, np.argwhere + choice per request, slice / pad, upload"""
    import torch
    img, lab = img_d.cpu().numpy(), lab_d.cpu().numpy()
    imgs, labs = [], []
    for k, u in requests:
        where = np.argwhere(lab == k)
        o = origin_of(where[int(u * len(where))], lab.shape, patch)
        imgs.append(cut(img, o, patch, -1024.0))
        labs.append(cut(lab, o, patch, 0.0))
    out = torch.from_numpy(np.stack(imgs)).cuda(), torch.from_numpy(np.stack(labs)).cuda()
    torch.cuda.synchronize()
    return out


def torch_detour(img_d, lab_d, requests, patch):
    """the same on the device with torch: nonzero compacts and synchronises, the chosen voxel comes back for the slice bounds"""
    import torch
    imgs, labs = [], []
    for k, u in requests:
        where = torch.nonzero(lab_d == k)
        o = origin_of(where[int(u * where.shape[0])].tolist(), lab_d.shape, patch)
        sl = tuple(slice(o[a], o[a] + patch) for a in range(3))
        imgs.append(img_d[sl])
        labs.append(lab_d[sl])
    out = torch.stack(imgs), torch.stack(labs)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "patch_bench.json"))
    args = ap.parse_args()
    import torch
    from tests import patch_util as PU
    from vae_segmentation_amd import ops
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    rate = copy_rate()
    rows = []
    for shape, patch in CONFIGS:
        img, lab = case(shape)
        img_d, lab_d = torch.from_numpy(img).cuda(), torch.from_numpy(lab).cuda()
        _, t_index = eager_and_graph(lambda: ops.patch_index(lab_d, N_CLASS))
        index = ops.patch_index(lab_d, N_CLASS)
        for r in REQUESTS:
            words = np.random.RandomState(r).randint(0, 2 ** 32, size=(r, 5), dtype=np.uint64).astype(np.int64)
            forced = np.ones(r, np.int32)
            words_d, forced_d = torch.from_numpy(words).to(torch.int32).cuda(), torch.from_numpy(forced).cuda()        # the 32 bits the kernel reads
            picks, t_pick = eager_and_graph(lambda: ops.patch_pick(lab_d, index, (1, 2), words_d, forced_d, patch))
            _, t_gather = eager_and_graph(lambda: ops.patch_gather((img_d, lab_d), (-1024.0, 0.0), picks, patch))

            def chain():
                table = ops.patch_index(lab_d, N_CLASS)
                return ops.patch_gather((img_d, lab_d), (-1024.0, 0.0), ops.patch_pick(lab_d, table, (1, 2), words_d, forced_d, patch), patch)

            _, t_chain = eager_and_graph(chain)
            want = PU.ref_picks(lab, N_CLASS, (1, 2), words, forced, (patch,) * 3)
            equal = bool(np.array_equal(picks.cpu().numpy(), want))
            requests = [(int(row[3]), (int(w[1]) + 0.5) / 2.0 ** 32) for row, w in zip(want, words)]      # the same classes, a choice of the same kind
            moved = 2 * 2 * r * patch ** 3 * 4
            t_gather["bytes"] = moved
            t_gather["bytes_per_s"] = moved / (t_gather["graph_ms"] * 1e-3)
            t_gather["share_of_copy_rate"] = t_gather["bytes_per_s"] / rate
            row = {"shape": list(shape), "voxels": int(lab.size), "patch": patch, "requests": r, "equal": equal, "index": t_index, "pick": t_pick,
                   "gather": t_gather, "chain": t_chain, "host_ms": host_timed(lambda: host_detour(img_d, lab_d, requests, patch)),
                   "torch_ms": host_timed(lambda: torch_detour(img_d, lab_d, requests, patch))}
            print(json.dumps(row), flush=True)
            rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS, "copy_bytes_per_s": rate, "chunk": ops.PATCH_CHUNK, "n_class": N_CLASS,
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
