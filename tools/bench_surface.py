"""Surface-distance metrics on the device against the host detour they replace -> profiles/surface_bench.json.

Shapes (1, 2, S, S, S), S = 96, 128, 160: an organ-plus-specks prediction (a displaced, slightly swollen ellipsoid with 0.1 % stray voxels) against
the clean organ label, two planes with different specks.  Per case, in ONE process on ONE machine:
  device_ms     ops.surface_distances captured in a HIP graph, median of REPLAYS replays timed by device events (steady state: warmed, replayed)
  host_ms       what a user does without it: both masks .cpu() -> scipy binary_erosion surfaces -> scipy distance_transform_edt of both surfaces ->
                ASSD / HD / HD95 with numpy, per plane; host clock around work that starts from synchronised device tensors, median of HOST_REPS
  ratio         host_ms / device_ms; the two results are compared in the same run (counts and squared statistics exactly — the host side rebuilds
                the integer squared distances from the feature-transform indices — the fp64 fields to rtol 1e-9)
  kernels       per-kernel medians from one `rocprofv3 --kernel-trace` run of a child process (eager calls, a run of its own), with the bytes each
                phase has to move (from the shapes) and the rate that makes

    python tools/bench_surface.py [--out profiles/surface_bench.json] [--no-trace]
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SIDES = (96, 128, 160)
REPLAYS, HOST_REPS, TRACE_CALLS = 30, 3, 5
PHASES = ("sf_surface_kernel", "sf_xpass_kernel", "sf_line_kernel", "sf_line_kernel", "sf_chunk_kernel", "sf_scan_kernel", "sf_chunk_kernel", "sf_select_kernel")
PHASE_NAMES = ("surface", "x_pass", "y_pass", "z_pass", "count", "scan", "scatter", "select")
FIELDS = ("count_ab", "count_ba", "sum_ab", "sum_ba", "max_sq", "lo_sq", "hi_sq", "assd", "hd", "hd95")


def organ(s, shift=(0, 0, 0), scale=1.0):
    ax = np.arange(s, dtype=np.float64)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    c = (s - 1) / 2
    r = ((z - c - shift[0]) / (0.30 * s * scale)) ** 2 + ((y - c - shift[1]) / (0.22 * s * scale)) ** 2 + ((x - c - shift[2]) / (0.34 * s * scale)) ** 2
    return r < 1.0


def make_pair(s):
    """-> (pred, label) float32 (1, 2, s, s, s)"""
    label = organ(s)
    pred = [organ(s, shift=(1, -2, 1), scale=1.03) | (np.random.RandomState(10 + c).rand(s, s, s) < 1e-3) for c in range(2)]
    return np.stack(pred).astype(np.float32)[None], np.stack([label, label]).astype(np.float32)[None]


def host_path(pred, label):
    """the detour: device -> host, scipy erosion and EDT, numpy metrics; -> list over planes of {field: number}"""
    from scipy import ndimage
    a_all, b_all = pred.cpu().numpy() >= 0.5, label.cpu().numpy() >= 0.5
    struct = ndimage.generate_binary_structure(3, 1)
    out = []
    for a, b in zip(a_all.reshape((-1,) + a_all.shape[2:]), b_all.reshape((-1,) + b_all.shape[2:])):
        sa, sb = a & ~ndimage.binary_erosion(a, struct), b & ~ndimage.binary_erosion(b, struct)
        grid = np.indices(a.shape, dtype=np.int64)
        sq = []
        for src, dst in ((sa, sb), (sb, sa)):
            _, idx = ndimage.distance_transform_edt(~dst, return_indices=True)
            sq.append((((idx.astype(np.int64) - grid) ** 2).sum(0))[src])
        union = np.sort(np.concatenate(sq))
        n = union.size
        k = int(math.floor(0.95 * (n - 1)))
        sums = [math.fsum(np.sqrt(v.astype(np.float64))) for v in sq]
        out.append({"count_ab": int(sq[0].size), "count_ba": int(sq[1].size), "sum_ab": sums[0], "sum_ba": sums[1], "max_sq": int(union[-1]),
                    "lo_sq": int(union[k]), "hi_sq": int(union[min(k + 1, n - 1)]), "assd": 0.5 * (sums[0] / sq[0].size + sums[1] / sq[1].size),
                    "hd": float(np.sqrt(union[-1])), "hd95": float(np.percentile(np.sqrt(union.astype(np.float64)), 95))})
    return out


def same_results(rec, host):
    dev = {k: v.cpu().numpy().reshape(-1) for k, v in rec.items()}
    for p, want in enumerate(host):
        for k in FIELDS[:2] + FIELDS[4:7]:
            if dev[k][p] != want[k]:
                return False
        for k in ("sum_ab", "sum_ba", "assd", "hd", "hd95"):
            if abs(dev[k][p] - want[k]) > 1e-9 * abs(want[k]):
                return False
    return True


def phase_bytes(voxels, surf):
    """bytes each phase has to move for `voxels` voxels in all planes of ONE mask (the pass handles two masks) and `surf` surface voxels in all"""
    v2 = 2 * voxels
    return {"surface": v2 * (4 + 1), "x_pass": v2 * (1 + 4), "y_pass": v2 * 8, "z_pass": v2 * 8, "count": v2 * 1 + surf * 4, "scan": 0,
            "scatter": v2 * 1 + surf * 8, "select": surf * 4}


def trace_child():
    """run under rocprofv3: TRACE_CALLS eager calls per case, in the fixed case order"""
    import torch
    from vae_segmentation_amd import ops
    for s in SIDES:
        pred, label = (torch.from_numpy(x).cuda() for x in make_pair(s))
        for _ in range(TRACE_CALLS):
            ops.surface_distances(pred, label)
        torch.cuda.synchronize()


def read_trace(directory):
    """-> per case {phase: median microseconds} from the kernel trace of trace_child()"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = [r for r in csv.DictReader(open(files[0])) if "sf_" in r["Kernel_Name"] and "_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_case = len(PHASES) * TRACE_CALLS
    if len(rows) != per_case * len(SIDES):
        return None
    out, at = {}, 0
    for s in SIDES:
        chunk, at = rows[at:at + per_case], at + per_case
        med = {}
        for j, (kern, name) in enumerate(zip(PHASES, PHASE_NAMES)):
            calls = chunk[j::len(PHASES)]
            assert all(kern in r["Kernel_Name"] for r in calls), (kern, calls[0]["Kernel_Name"])
            med[name] = statistics.median(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in calls) / 1e3
        out[str(s)] = med
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface_bench.json"))
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child()
    import torch
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py measures on the GPU; there is none here")
    cases = {}
    for s in SIDES:
        pred_np, label_np = make_pair(s)
        pred, label = torch.from_numpy(pred_np).cuda(), torch.from_numpy(label_np).cuda()
        eager = {k: v.clone() for k, v in ops.surface_distances(pred, label).items()}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.surface_distances(pred, label)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            rec = ops.surface_distances(pred, label)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        dev = []
        for _ in range(REPLAYS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        host_path(pred, label)
        host = []
        for _ in range(HOST_REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = host_path(pred, label)
            host.append((time.perf_counter() - t0) * 1e3)
        same = same_results(rec, ref) and all(torch.equal(eager[k].view(torch.int64), rec[k].view(torch.int64)) for k in FIELDS)
        d, h = statistics.median(dev), statistics.median(host)
        cases[str(s)] = {"shape": [1, 2, s, s, s], "surface_voxels": int(sum(r["count_ab"] + r["count_ba"] for r in ref)),
                         "assd": [r["assd"] for r in ref], "hd95": [r["hd95"] for r in ref], "hd": [r["hd"] for r in ref],
                         "device_ms": d, "device_ms_min": min(dev), "device_ms_max": max(dev), "host_ms": h, "host_ms_min": min(host),
                         "ratio_host_over_device": h / d, "device_equals_host": bool(same)}
        print("%-4d device %.3f ms  host %.1f ms  x%.0f  same=%s" % (s, d, h, h / d, same), flush=True)
        del graph
    result = {"what": "ops.surface_distances(connectivity=6, unit spacing) replayed from a HIP graph vs .cpu() + scipy binary_erosion + distance_transform_edt + "
                      "numpy metrics, same process",
              "device": torch.cuda.get_device_name(0), "replays": REPLAYS, "host_reps": HOST_REPS, "cases": cases}
    if not args.no_trace:
        if args.trace_dir is None:
            import tempfile
            args.trace_dir = tempfile.mkdtemp(prefix="surface_trace_")
        os.makedirs(args.trace_dir, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.trace_dir, "--", sys.executable, os.path.abspath(__file__), "--trace-child"]
        rc = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        split = read_trace(args.trace_dir) if rc.returncode == 0 else None
        if split is None:
            result["kernels"] = "not measured: the trace run gave no usable kernel list (exit %d)" % rc.returncode
        else:
            for key, med in split.items():
                c = cases[key]
                nbytes = phase_bytes(2 * c["shape"][2] ** 3, c["surface_voxels"])
                c["kernels_us"] = med
                c["kernel_sum_us"] = sum(med.values())
                c["dominant_phase"] = max(med, key=med.get)
                c["phase_bytes"] = nbytes
                c["phase_GBps"] = {k: (nbytes[k] / (med[k] * 1e-6) / 1e9 if med[k] > 0 else None) for k in med}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
