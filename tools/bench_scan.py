"""Scan geometry on the device against the host path it replaces -> profiles/scan_bench.json.

One 512 x 512 x 200 int16 scan at spacing (0.7, 0.7, 1.5) (1 mm grid 358 x 358 x 300), in ONE process on ONE machine:
  preprocess_scan   eager_ms: data_gpu.preprocess_scan(raw, affine_diag) — orient, anti-aliasing, zoom, with resize's one host read of the min / max —
                    host clock around calls that end in a synchronise, median of REPLAYS.  Not captured: that host read is inside the call.
  scan_orient       eager_ms / graph_ms: the one vs_scan_orient launch by device events, eagerly and replayed from a HIP graph; bytes per second
                    (2 bytes read + 4 written per voxel) beside the 6.3 TB/s copy ceiling
  to_native         eager_ms / graph_ms for K = 2 probabilities on the 1 mm grid, linear and nearest, with and without the probability output
  host_ms           the scipy restatement on the same box (tests/scan_util.py: numpy transpose + oracle.data_cpu.skimage_resize in float64; the inverse as
                    .cpu() -> zoom per class -> argmax -> .cuda()), host clock, HOST_REPS runs; labels differing between the two paths are counted
    python tools/bench_scan.py [--out profiles/scan_bench.json] [--shape 512 512 200] [--spacing 0.7 0.7 1.5] [--no-host]
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

REPLAYS, HOST_REPS = 20, 1
COPY_CEILING = 6.3e12


def synthetic_scan(shape, seed=0):
    rng = np.random.RandomState(seed)
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, s, dtype=np.float32) for s in shape], indexing="ij")
    r = (g[0] / 0.6) ** 2 + (g[1] / 0.5) ** 2 + (g[2] / 0.7) ** 2
    return (np.where(r < 1.0, 120.0, -400.0) + rng.randn(*shape).astype(np.float32) * 30.0).astype(np.int16)


def device_events(fn, n=REPLAYS):
    import torch
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def host_clock(fn, n):
    import torch
    ms, out = [], None
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def eager_and_graph(fn):
    """fn() -> tensors, reading only buffers that exist already -> (eager ms list, graph ms list, the captured call's outputs)"""
    import torch
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    return device_events(fn), device_events(graph.replay), out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scan_bench.json"))
    ap.add_argument("--shape", type=int, nargs=3, default=[512, 512, 200])
    ap.add_argument("--spacing", type=float, nargs=3, default=[0.7, 0.7, 1.5])
    ap.add_argument("--no-host", action="store_true", help="skip the scipy path (minutes at the default shape)")
    args = ap.parse_args()
    import torch
    from tests import scan_util as S
    from vae_segmentation_amd import data_gpu, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan.py measures on the GPU; there is none here")
    shape, spacing = tuple(args.shape), tuple(args.spacing)
    raw_np = synthetic_scan(shape)
    raw = torch.from_numpy(raw_np).cuda()
    g = data_gpu.ScanGeometry(shape, spacing)
    voxels = int(np.prod(shape))
    result = {"what": "data_gpu.preprocess_scan / ops.scan_orient / ops.to_native vs the numpy + scipy restatement, same process", "device": torch.cuda.get_device_name(0),
              "raw_shape": list(shape), "spacing": list(spacing), "shape_1mm": list(g.shape_1mm), "replays": REPLAYS, "host_reps": HOST_REPS, "cases": {}}

    def record(key, rec):
        result["cases"][key] = rec
        print(key, json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:                       # kept current: a run that is cut short leaves what it measured
            json.dump(result, f, indent=1)

    data_gpu.preprocess_scan(raw, spacing)
    ms, pre = host_clock(lambda: data_gpu.preprocess_scan(raw, spacing), REPLAYS)
    record("preprocess_scan", {"eager": summary(ms), "captured": False, "why_not": "resize reads the volume's min / max on the host"})
    e_ms, g_ms, _ = eager_and_graph(lambda: ops.scan_orient(raw, g))
    moved = voxels * (raw.element_size() + 4)
    record("scan_orient", {"eager": summary(e_ms), "graph": summary(g_ms), "bytes": moved, "bytes_per_s": moved / (statistics.median(g_ms) * 1e-3),
                           "share_of_copy_ceiling": moved / (statistics.median(g_ms) * 1e-3) / COPY_CEILING})
    # a two-class answer on the 1 mm grid: a soft ball
    z = torch.stack(torch.meshgrid(*[torch.linspace(-1.0, 1.0, s, device="cuda") for s in g.shape_1mm], indexing="ij")).pow(2).sum(0)
    p1 = torch.sigmoid((0.5 - z) * 8.0)
    prob = torch.stack([1.0 - p1, p1]).contiguous()
    outs = {}
    for interp in ("linear", "nearest"):
        for want_prob in (False, True):
            e_ms, g_ms, out = eager_and_graph(lambda: ops.to_native(prob, g, interp=interp, want_prob=want_prob))
            written = voxels * (1 + (4 * prob.shape[0] if want_prob else 0))
            outs[interp] = out["label"].clone()
            record("to_native/%s/%s" % (interp, "label+prob" if want_prob else "label"),
                   {"eager": summary(e_ms), "graph": summary(g_ms), "k": int(prob.shape[0]), "bytes_written": written,
                    "written_bytes_per_s": written / (statistics.median(g_ms) * 1e-3)})
    if not args.no_host:
        ms, ref = host_clock(lambda: S.preprocess(raw.cpu().numpy(), spacing), HOST_REPS)
        span = float(ref["image"].max() - ref["image"].min())
        err = float(np.abs(pre["image"].cpu().numpy().astype(np.float64) - ref["image"]).max())
        record("preprocess_scan/host", {"host": summary(ms), "ratio_host_over_device": statistics.median(ms) / result["cases"]["preprocess_scan"]["eager"]["median_ms"],
                                        "max_abs_err": err, "value_range": span})
        for interp in ("linear", "nearest"):
            ms, ref = host_clock(lambda: torch.from_numpy(S.to_native(prob.cpu().numpy(), shape, spacing, interp)["label"]).cuda(), HOST_REPS)
            record("to_native/%s/host" % interp, {"host": summary(ms), "labels_differing": int((ref != outs[interp]).sum()), "voxels": voxels,
                                                  "ratio_host_over_graph": statistics.median(ms) / result["cases"]["to_native/%s/label" % interp]["graph"]["median_ms"]})
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
