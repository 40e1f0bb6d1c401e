"""Connected-component post-processing on the device against the host detour it replaces -> profiles/cc_bench.json.

Shapes (1, 2, S, S, S), S = 96, 128, 160; three masks per shape:
  label_specks  the synthetic organ label plus 0.1 % random specks (what a prediction looks like)
  noise         thresholded smooth noise, hundreds of components
  serpentine    a one-voxel-wide path through the whole volume (the deepest union-find chains)
Per case, in ONE process on ONE machine:
  device_ms     ops.keep_largest(k=1) captured in a HIP graph, median of REPLAYS replays timed by device events (steady state: warmed, replayed)
  host_ms       what a user does without it: pred.cpu() -> scipy.ndimage.label + np.bincount + select per channel -> .cuda(), host clock around
                work that ends in a synchronise, median of HOST_REPS
  ratio         host_ms / device_ms; the two results are compared bit for bit
  kernels       per-kernel medians from one `rocprofv3 --kernel-trace` run of a child process (eager calls, a run of its own), with the bytes each
                phase has to move (from the shapes) and the rate that makes
Also driver.validate per case at 128^3 with the filter off and on (a record, not a gate).

    python tools/bench_cc.py [--out profiles/cc_bench.json] [--no-trace]
"""
import argparse
import csv
import glob
import json
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
MASKS = ("label_specks", "noise", "serpentine")
REPLAYS, HOST_REPS, TRACE_CALLS = 30, 3, 5
PHASES = ("cc_init_kernel", "cc_merge_kernel", "cc_flatten_kernel", "cc_chunk_kernel", "cc_scan_kernel", "cc_chunk_kernel", "cc_relabel_kernel",
          "cc_select_kernel", "cc_apply_kernel")
PHASE_NAMES = ("init", "merge", "flatten", "count", "scan", "rank", "relabel", "select", "apply")


def smooth_noise(shape, seed, passes=2):
    x = np.random.RandomState(seed).rand(*shape).astype(np.float32)
    for _ in range(passes):
        for ax in range(3):
            x = (x + np.roll(x, 1, ax) + np.roll(x, -1, ax)) / 3
    return x


def serpentine(s):
    m = np.zeros((s, s, s), bool)
    for zi, z in enumerate(range(0, s, 2)):
        ys = list(range(0, s, 2))[::-1 if zi % 2 else 1]
        side = 0
        for i, y in enumerate(ys):
            m[z, y, :] = True
            if i + 1 < len(ys):
                m[z, (y + ys[i + 1]) // 2, s - 1 if side == 0 else 0] = True
                side ^= 1
        if z + 2 < s:
            m[z + 1, ys[-1], 0] = True
    return m


def make_mask(kind, s):
    """-> float32 (1, 2, s, s, s)"""
    from vae_segmentation_amd import synthetic
    if kind == "label_specks":
        chans = []
        for c in range(2):
            lab = synthetic.synthetic_label(1, s, 3 + c).numpy().reshape(s, s, s) > 0.5
            chans.append(lab | (np.random.RandomState(10 + c).rand(s, s, s) < 1e-3))
        return np.stack(chans).astype(np.float32)[None]
    if kind == "noise":
        return np.stack([smooth_noise((s, s, s), 20 + c) >= 0.505 for c in range(2)]).astype(np.float32)[None]
    m = serpentine(s)
    return np.stack([m, m[::-1].copy()]).astype(np.float32)[None]


def host_path(pred, k=1):
    """the detour: device -> host, scipy labelling, size ranking, selection, host -> device"""
    import torch
    from scipy import ndimage
    x = pred.cpu().numpy()
    out = np.zeros_like(x)
    for n in range(x.shape[0]):
        for c in range(x.shape[1]):
            lab, cnt = ndimage.label(x[n, c] >= 0.5, structure=np.ones((3, 3, 3)))
            sizes = np.bincount(lab.ravel(), minlength=cnt + 1)[1:]
            order = sorted(range(cnt), key=lambda i: (-int(sizes[i]), i))[:k]
            out[n, c] = np.isin(lab, [i + 1 for i in order])
    res = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    return res


def phase_bytes(v_planes, fg, comps, conn_rows=4):
    """bytes each phase has to move for v_planes voxels in all, fg of them foreground, comps components (int32 / fp32 everywhere)"""
    return {"init": 8 * v_planes, "merge": 4 * v_planes * (1 + conn_rows), "flatten": 8 * v_planes, "count": 4 * v_planes, "scan": 0,
            "rank": 4 * v_planes + 4 * comps, "relabel": 8 * v_planes + 4 * fg, "select": 8 * comps, "apply": 8 * v_planes + 4 * fg}


def trace_child():
    """run under rocprofv3: TRACE_CALLS eager calls per case, in the fixed case order"""
    import torch
    from vae_segmentation_amd import ops
    for s in SIDES:
        for kind in MASKS:
            x = torch.from_numpy(make_mask(kind, s)).cuda()
            for _ in range(TRACE_CALLS):
                ops.keep_largest(x, k=1)
            torch.cuda.synchronize()


def read_trace(directory):
    """-> per case {phase: median microseconds} from the kernel trace of trace_child()"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = [r for r in csv.DictReader(open(files[0])) if "cc_" in r["Kernel_Name"] and "_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_case = len(PHASES) * TRACE_CALLS
    if len(rows) != per_case * len(SIDES) * len(MASKS):
        return None
    out, at = {}, 0
    for s in SIDES:
        for kind in MASKS:
            chunk, at = rows[at:at + per_case], at + per_case
            med = {}
            for j, (kern, name) in enumerate(zip(PHASES, PHASE_NAMES)):
                calls = chunk[j::len(PHASES)]
                assert all(kern in r["Kernel_Name"] for r in calls), (kern, calls[0]["Kernel_Name"])
                med[name] = statistics.median(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in calls) / 1e3
            out["%d/%s" % (s, kind)] = med
    return out


def bench_validate():
    import torch
    import joint_model as M
    from vae_segmentation_amd import driver, synthetic
    seg = M.Segmentation(n_channels=1, n_class=2, norm_type=1)
    synthetic.deterministic_fill_(seg, seed=0)
    seg = seg.cuda().eval()
    loader = list(torch.utils.data.DataLoader(driver.SyntheticVolumes(2, 128, seed=2), batch_size=1))
    res = {}
    for name, k in (("filter_off", 0), ("filter_on", 1)):
        driver.validate("seg_train", seg, loader, 2, keep_largest=k)
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            driver.validate("seg_train", seg, loader, 2, keep_largest=k)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / len(loader) * 1e3)
        res[name + "_ms_per_case"] = statistics.median(times)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cc_bench.json"))
    ap.add_argument("--trace-dir", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child()
    import torch
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_cc.py measures on the GPU; there is none here")
    cases = {}
    for s in SIDES:
        for kind in MASKS:
            x_np = make_mask(kind, s)
            buf = torch.from_numpy(x_np).cuda()
            labels, counts, _ = ops.cc_label(buf)
            eager = ops.keep_largest(buf, k=1)
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.keep_largest(buf, k=1)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = ops.keep_largest(buf, k=1)
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
            host_path(buf)
            host = []
            for _ in range(HOST_REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = host_path(buf)
                host.append((time.perf_counter() - t0) * 1e3)
            same = bool(torch.equal(ref, out)) and bool(torch.equal(eager, out))
            d, h = statistics.median(dev), statistics.median(host)
            cases["%d/%s" % (s, kind)] = {"shape": [1, 2, s, s, s], "foreground_voxels": int((x_np >= 0.5).sum()), "components": int(counts.sum().item()),
                                          "device_ms": d, "device_ms_min": min(dev), "device_ms_max": max(dev), "host_ms": h, "host_ms_min": min(host),
                                          "ratio_host_over_device": h / d, "device_equals_host": same}
            print("%-18s device %.3f ms  host %.1f ms  x%.0f  same=%s" % ("%d/%s" % (s, kind), d, h, h / d, same), flush=True)
            del graph
    result = {"what": "ops.keep_largest(k=1, connectivity=26) replayed from a HIP graph vs .cpu() + scipy.ndimage.label + bincount + select + .cuda(), same process",
              "device": torch.cuda.get_device_name(0), "replays": REPLAYS, "host_reps": HOST_REPS, "cases": cases, "validate_128": bench_validate()}
    if not args.no_trace:
        if args.trace_dir is None:
            import tempfile
            args.trace_dir = tempfile.mkdtemp(prefix="cc_trace_")
        os.makedirs(args.trace_dir, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.trace_dir, "--", sys.executable, os.path.abspath(__file__), "--trace-child"]
        rc = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
        split = read_trace(args.trace_dir) if rc.returncode == 0 else None
        if split is None:
            result["kernels"] = "not measured: the trace run gave no usable kernel list (exit %d)" % rc.returncode
        else:
            for key, med in split.items():
                c = cases[key]
                nbytes = phase_bytes(2 * c["shape"][2] ** 3, c["foreground_voxels"], c["components"])
                c["kernels_us"] = med
                c["kernel_sum_us"] = sum(med.values())
                c["phase_bytes"] = nbytes
                c["phase_GBps"] = {k: (nbytes[k] / (med[k] * 1e-6) / 1e9 if med[k] > 0 else None) for k in med}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
