"""Exact percentiles and intensity standardisation on the device against the alternatives -> profiles/standardize_bench.json.

One CT-like volume (tests/standardize_util.volume "ct": round(N(40, 250)) with 40 % air at -1024) of 96^3, 128^3 and 256 x 256 x 192 voxels, Q = 2
(0.5, 99.5) and Q = 11 (1, 10, ..., 90, 99) percentiles, of the whole plane and of the voxels above -500, in ONE process on ONE machine:
  quantile      ops.quantile alone: eager_ms — issued eagerly, device events around it — and graph_ms — captured in a HIP graph and replayed; medians of
                REPS after WARMUP
  transform     IntensityStandardizer.transform's two calls, ops.quantile -> ops.intensity_map onto a standard scale of Q landmarks: the same two figures
  host_ms       x.cpu() -> np.percentile of the selected voxels + np.interp -> .cuda(), host clock around work that ends in a synchronise, median of REPS
                after WARMUP as well
  torch_ms      torch.quantile on the device, device events, median of REPS after WARMUP — or the text of the error where it refuses the input.  With
                the threshold it is torch.quantile(x[x > above]): the boolean index compacts on the device and synchronises with the host, inside the
                timed window, as a caller would pay for it
  floor_us      the bytes the launches must move — four counting passes read the plane, the map reads and writes it — at the copy rate measured in this
                run (copy_bytes_per_s: a 256 MiB device-to-device copy, bytes read plus bytes written over its median time)
  equal         whether the device percentiles of this run equalled the oracle's (tests/standardize_util.ref_quantile) with ==
No time or ratio is fixed in advance; the file records what was measured.

    python tools/bench_standardize.py [--out profiles/standardize_bench.json] [--shapes 96,96,96 128,128,128 256,256,192]
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

SHAPES = ((96, 96, 96), (128, 128, 128), (256, 256, 192))
PERCENTILES = {2: (0.5, 99.5), 11: (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99)}
ABOVE = (None, -500.0)
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


def eager_and_graph(fn):
    """-> (eager result, median eager ms, median replay ms)"""
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
    return eager, timed(fn), timed(graph.replay)


def copy_rate():
    import torch
    a = torch.empty(256 << 18, dtype=torch.float32, device="cuda").normal_()          # 256 MiB
    b = torch.empty_like(a)
    ms = timed(lambda: b.copy_(a))
    return 2.0 * a.numel() * 4 / (ms * 1e-3)


def host_detour(x, ps, above, dst):
    import torch
    v = x.cpu().numpy()
    sel = v[np.isfinite(v)] if above is None else v[np.isfinite(v) & (v > np.float32(above))]
    q = np.percentile(sel.astype(np.float64), ps)
    out = torch.from_numpy(np.interp(v.astype(np.float64), q, dst).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    return out


def torch_quantile(x, ps, above):
    """-> (median ms, None) or (None, the error's text)"""
    import torch
    q = torch.tensor([p / 100.0 for p in ps], dtype=torch.float32, device=x.device)

    def run():
        v = x.reshape(-1)
        return torch.quantile(v if above is None else v[v > above], q)

    try:
        return timed(run), None
    except RuntimeError as e:
        return None, str(e).splitlines()[0][:200]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "standardize_bench.json"))
    ap.add_argument("--shapes", nargs="+", default=[",".join(str(s) for s in shape) for shape in SHAPES])
    args = ap.parse_args()
    import torch
    from tests import standardize_util as SU
    from vae_segmentation_amd import data_gpu, ops
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    rate = copy_rate()
    rows = []
    for text in args.shapes:
        shape = tuple(int(s) for s in text.split(","))
        host = SU.volume(shape, "ct", seed=1)
        x = torch.from_numpy(host).cuda()
        v = host.size
        for nq, ps in PERCENTILES.items():
            std = data_gpu.IntensityStandardizer(ps, target=(-200.0, 400.0))
            std.scale = [float(s) for s in np.linspace(-200.0, 400.0, nq)]            # a standard scale of Q landmarks (what fit() would leave)
            for above in ABOVE:
                std.above = above
                std.transform(x)                                                        # builds the scale on the device before anything is captured
                rec, q_eager, q_graph = eager_and_graph(lambda: ops.quantile(x, ps, above=above))
                _, t_eager, t_graph = eager_and_graph(lambda: std.transform(x))
                want = SU.ref_quantile(host, ps, above)
                equal = bool(np.array_equal(rec["q"].cpu().numpy(), want["q"]) and int(rec["count"]) == want["count"])
                t0 = []
                for rep in range(WARMUP + REPS):
                    t = time.perf_counter()
                    host_detour(x, ps, above, np.array(std.scale))
                    if rep >= WARMUP:
                        t0.append((time.perf_counter() - t) * 1e3)
                torch_ms, torch_error = torch_quantile(x, ps, above)
                row = {"shape": list(shape), "voxels": v, "Q": nq, "above": above, "selected": want["count"], "equal": equal,
                       "quantile": {"eager_ms": q_eager, "graph_ms": q_graph, "floor_us": 4 * 4 * v / rate * 1e6},
                       "transform": {"eager_ms": t_eager, "graph_ms": t_graph, "floor_us": (4 * 4 * v + 2 * 4 * v) / rate * 1e6},
                       "host_ms": statistics.median(t0), "torch_ms": torch_ms, "torch_error": torch_error}
                print(json.dumps(row), flush=True)
                rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "reps": REPS,
           "copy_bytes_per_s": rate, "percentiles": {str(k): list(p) for k, p in PERCENTILES.items()}, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
