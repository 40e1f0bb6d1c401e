"""Simulated low resolution on the device against the host detour -> profiles/lowres_bench.json.

One channel of P^3 voxels, P = 64, 96, 128 (mean 0, std 0.5, as CenterIntensities leaves a CT patch), zoom 0.5, 0.75, 1.0, in ONE process on ONE machine:
  lowres        ops.simulate_lowres (down order 0, up order 3 with the clip) alone: eager_ms — issued eagerly, device events around it, median of REPLAYS
                calls — and graph_ms — captured in a HIP graph, median of REPLAYS replays
  chain         data_gpu.intensity_augment with every gate of IntensityAugment open (noise, blur, brightness, contrast, [lowres,] inverted gamma, gamma,
                flip), the same two figures with and without the low-resolution stage
  host_ms       x.cpu() -> two scipy.ndimage.zoom calls and the clip -> .cuda(), host clock around work that ends in a synchronise, median of HOST_REPS
  floor_us      the bytes the six launches must move — the gather: read what it picks, write the target; the record of the target: read it; the z, y, x
                passes: read and write their volumes, fp64 between them — at the copy rate profiles/sliding_bench.json records
No time or ratio is fixed in advance; the file records what was measured.

    python tools/bench_lowres.py [--out profiles/lowres_bench.json] [--sides 64 96 128]
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

from tools.bench_augment import OPS, eager_and_graph  # noqa: E402

SIDES, ZOOMS = (64, 96, 128), (0.5, 0.75, 1.0)
REPLAYS, HOST_REPS = 20, 3
COPY_BYTES_PER_S = 6.3e12                   # profiles/sliding_bench.json copy_ceiling_bytes_per_s


def floor_bytes(shape, target):
    """what the launches of simulate_lowres(order 0, order 3 + clip) must move, per launch"""
    sd, sh, sw = shape
    td, th, tw = target
    t, v = td * th * tw, sd * sh * sw
    return {"gather": 4 * t + 4 * t, "stats": 4 * t, "z_pass": 4 * t + 8 * sd * th * tw, "y_pass": 8 * sd * th * tw + 8 * sd * sh * tw,
            "x_pass": 8 * sd * sh * tw + 4 * v}


def host_lowres(x, target):
    import torch
    from scipy import ndimage
    v = x.cpu().numpy()
    low = ndimage.zoom(v.astype(np.float64), [t / s for t, s in zip(target, v.shape)], order=0, mode="nearest", grid_mode=True).astype(np.float32)
    up = ndimage.zoom(low.astype(np.float64), [s / t for t, s in zip(target, v.shape)], order=3, mode="nearest", grid_mode=True)
    out = torch.from_numpy(np.clip(up, low.min(), low.max()).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lowres_bench.json"))
    ap.add_argument("--sides", type=int, nargs="+", default=list(SIDES))
    args = ap.parse_args()
    import torch
    from vae_segmentation_amd import data_gpu as D
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_lowres.py measures on the GPU; there is none here")
    cases = {}
    result = {"what": "ops.simulate_lowres (order 0 down, order 3 up, clipped) and the full intensity chain with and without it, eager and replayed from a "
                      "HIP graph, vs .cpu() + scipy.ndimage.zoom twice + .cuda(); same process, one channel", "device": torch.cuda.get_device_name(0),
              "replays": REPLAYS, "host_reps": HOST_REPS, "copy_bytes_per_s": COPY_BYTES_PER_S, "cases": cases}
    names = list(OPS)
    at = names.index("contrast") + 1
    for s in args.sides:
        x = torch.from_numpy((np.random.RandomState(s).randn(1, s, s, s) * 0.5).astype(np.float32)).cuda()
        base_chain = [OPS[k] for k in names]
        _, _, e_ms, g_ms = eager_and_graph(lambda: D.intensity_augment(x, base_chain))
        base = {"eager_ms": statistics.median(e_ms), "graph_ms": statistics.median(g_ms)}
        for zoom in ZOOMS:
            target = D.lowres_target_shape((s, s, s), zoom)
            rec = {"shape": [s, s, s], "zoom": zoom, "target": list(target), "bundle": ops.zoom_edge_bundle(target[0], s)}
            eager, replayed, e_ms, g_ms = eager_and_graph(lambda: ops.simulate_lowres(x[0], target))
            rec["lowres"] = {"eager_ms": statistics.median(e_ms), "graph_ms": statistics.median(g_ms), "graph_ms_min": min(g_ms), "graph_ms_max": max(g_ms),
                             "graph_equals_eager": bool(torch.equal(eager, replayed))}
            chain = base_chain[:at] + [("lowres", zoom)] + base_chain[at:]
            eager, replayed, e_ms, g_ms = eager_and_graph(lambda: D.intensity_augment(x, chain))
            rec["chain_with"] = {"eager_ms": statistics.median(e_ms), "graph_ms": statistics.median(g_ms),
                                 "graph_equals_eager": bool(torch.equal(eager, replayed))}
            rec["chain_without"] = base
            host = []
            for _ in range(HOST_REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ref = host_lowres(x[0], target)
                host.append((time.perf_counter() - t0) * 1e3)
            rec["host_ms"] = statistics.median(host)
            rec["host_max_abs_diff"] = float((ref - ops.simulate_lowres(x[0], target)).abs().max())
            fb = floor_bytes((s, s, s), target)
            rec["floor_bytes"], rec["floor_us"] = fb, sum(fb.values()) / COPY_BYTES_PER_S * 1e6
            rec["ratio_host_over_graph"] = rec["host_ms"] / rec["lowres"]["graph_ms"]
            rec["ratio_graph_over_floor"] = rec["lowres"]["graph_ms"] * 1e3 / rec["floor_us"]
            cases["%d/%g" % (s, zoom)] = rec
            print("%-10s lowres eager %.3f graph %.3f ms   chain %.3f -> %.3f ms (graph)   host %.1f ms   floor %.1f us   same=%s  host diff %.2e"
                  % ("%d/%g" % (s, zoom), rec["lowres"]["eager_ms"], rec["lowres"]["graph_ms"], base["graph_ms"], rec["chain_with"]["graph_ms"],
                     rec["host_ms"], rec["floor_us"], rec["lowres"]["graph_equals_eager"], rec["host_max_abs_diff"]), flush=True)
            with open(args.out, "w") as f:                   # kept current: a run that is cut short leaves what it measured
                json.dump(result, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
