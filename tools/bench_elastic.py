"""Elastic deformation on the device against the two ways to get it without the new kernels -> profiles/elastic_bench.json.

Patches P^3, P = 64, 96, 128, sigma in {10, 13, 30} (radius 40, 52, 120), alpha 500.  Per case, in ONE process on ONE machine:
  field_numpy     data_gpu.elastic_field from a (3, P, P, P) fp64 noise tensor already on the device: the three filter passes alone
  field_philox    the same from (seed, sample): the Philox launch plus the filter
  warp            data_gpu.warp_resample of one P^3 fp32 volume (order 3: spline prefilter + sampler) with that field
  each as  eager_ms  issued eagerly, device events around it, median of REPLAYS calls
           graph_ms  captured in a HIP graph, median of REPLAYS replays (steady state: warmed, replayed)
  host_ms         (a) what a user does without it: noise.cpu() -> scipy.ndimage.gaussian_filter x 3, image.cpu() -> map_coordinates(order 3) -> .cuda(),
                  host clock around work that ends in a synchronise, median of HOST_REPS; split into host_field_ms and host_warp_ms
  conv3d_ms       (b) the same filter as three fp64 torch.nn.functional.conv3d calls with 1-D kernels (zero padding) on the device, eager, device events
  max_abs_err     of the device field against scipy's, in voxels

    python tools/bench_elastic.py [--out profiles/elastic_bench.json] [--sides 64 96 128] [--sigmas 10 13 30]
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

SIDES, SIGMAS, ALPHA = (64, 96, 128), (10.0, 13.0, 30.0), 500.0
REPLAYS, HOST_REPS = 20, 2


def timed(fn, reps=REPLAYS):
    import torch
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def eager_and_graph(fn):
    """-> (eager result, graph result, eager_ms, graph_ms lists)"""
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
        out = fn()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    return eager, out, timed(fn), timed(graph.replay)


def summary(prefix, e_ms, g_ms):
    return {prefix + "_eager_ms": statistics.median(e_ms), prefix + "_graph_ms": statistics.median(g_ms), prefix + "_graph_ms_min": min(g_ms),
            prefix + "_graph_ms_max": max(g_ms)}


def conv3d_field(noise, sigma, alpha):
    import torch
    import torch.nn.functional as F
    r = int(4.0 * sigma + 0.5)
    k = torch.arange(-r, r + 1, dtype=torch.float64, device=noise.device)
    w = torch.exp(-0.5 / (sigma * sigma) * k * k)
    w = w / w.sum()
    x = noise[:, None]                                         # (3, 1, D, H, W): the three fields as a batch
    x = F.conv3d(x, w.view(1, 1, -1, 1, 1), padding=(r, 0, 0))
    x = F.conv3d(x, w.view(1, 1, 1, -1, 1), padding=(0, r, 0))
    x = F.conv3d(x, w.view(1, 1, 1, 1, -1), padding=(0, 0, r))
    return x[:, 0] * alpha


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "elastic_bench.json"))
    ap.add_argument("--sides", type=int, nargs="+", default=list(SIDES))
    ap.add_argument("--sigmas", type=float, nargs="+", default=list(SIGMAS))
    args = ap.parse_args()
    import torch
    from scipy import ndimage
    from oracle import data_cpu as O
    from vae_segmentation_amd import data_gpu as D
    if not torch.cuda.is_available():
        raise SystemExit("bench_elastic.py measures on the GPU; there is none here")
    cases = {}
    result = {"what": "data_gpu.elastic_field / warp_resample eager and replayed from a HIP graph vs .cpu() + scipy.ndimage + .cuda() and vs fp64 conv3d, same process",
              "device": torch.cuda.get_device_name(0), "alpha": ALPHA, "replays": REPLAYS, "host_reps": HOST_REPS, "cases": cases}
    angles, scale = (0.1, -0.15, 0.05), 1.05
    for s in args.sides:
        patch = (s, s, s)
        rng = np.random.RandomState(s)
        noise = torch.from_numpy(rng.random_sample((3,) + patch) * 2 - 1).cuda()
        image = torch.from_numpy((rng.randn(*patch) * 300).astype(np.float32)).cuda()
        centre = tuple(s / 2.0 - 0.5 for _ in range(3))
        for sigma in args.sigmas:
            rec = {"shape": list(patch), "sigma": sigma, "radius": int(4.0 * sigma + 0.5)}
            field, g_field, e_ms, g_ms = eager_and_graph(lambda: D.elastic_field(patch, ALPHA, sigma, noise))
            rec.update(summary("field_numpy", e_ms, g_ms))
            rec["graph_equals_eager"] = bool(torch.equal(field, g_field))
            _, _, e_ms, g_ms = eager_and_graph(lambda: D.elastic_field(patch, ALPHA, sigma, (7, 3)))
            rec.update(summary("field_philox", e_ms, g_ms))
            warped, g_warped, e_ms, g_ms = eager_and_graph(lambda: D.warp_resample(image, field, patch, angles, scale, centre, 3, -1024.0))
            rec.update(summary("warp", e_ms, g_ms))
            rec["graph_equals_eager"] = rec["graph_equals_eager"] and bool(torch.equal(warped, g_warped))
            try:                                             # an fp64 convolution with a 241-tap kernel is not a path every backend has
                conv = conv3d_field(noise, sigma, ALPHA)
                torch.cuda.synchronize()
                rec["conv3d_ms"] = statistics.median(timed(lambda: conv3d_field(noise, sigma, ALPHA), reps=5))
                rec["conv3d_max_abs_diff"] = float((conv - field).abs().max())
            except RuntimeError as e:
                rec["conv3d_ms"], rec["conv3d_error"] = float("nan"), str(e)[:200]
            h_field, h_warp = [], []
            for _ in range(HOST_REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n_host = noise.cpu().numpy()
                f_host = np.stack([ndimage.gaussian_filter(n_host[k], sigma, mode="constant", cval=0) * ALPHA for k in range(3)])
                t1 = time.perf_counter()
                c = O.spatial_coords(patch, angles, scale, centre) + (f_host.reshape(3, -1).T @ O.rotation_matrix(*angles)).T.reshape(f_host.shape) * scale
                out = torch.from_numpy(ndimage.map_coordinates(image.cpu().numpy().astype(float), c, order=3, mode="constant", cval=-1024.0)
                                       .astype(np.float32)).cuda()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                h_field.append((t1 - t0) * 1e3); h_warp.append((t2 - t1) * 1e3)
            rec["host_field_ms"], rec["host_warp_ms"] = statistics.median(h_field), statistics.median(h_warp)
            rec["host_ms"] = rec["host_field_ms"] + rec["host_warp_ms"]
            rec["max_abs_err"] = float(np.abs(field.cpu().numpy() - f_host).max())
            rec["warp_max_abs_err"] = float((warped - out).abs().max())
            rec["ratio_host_over_graph"] = rec["host_ms"] / (rec["field_philox_graph_ms"] + rec["warp_graph_ms"])
            rec["ratio_conv3d_over_graph"] = rec["conv3d_ms"] / rec["field_numpy_graph_ms"]
            key = "%d/sigma%g" % (s, sigma)
            cases[key] = rec
            print("%-14s field %.3f / %.3f ms (numpy noise, eager / graph)  philox %.3f  warp %.3f  conv3d %.2f  host %.0f + %.0f ms  err %.1e  same=%s"
                  % (key, rec["field_numpy_eager_ms"], rec["field_numpy_graph_ms"], rec["field_philox_graph_ms"], rec["warp_graph_ms"], rec["conv3d_ms"],
                     rec["host_field_ms"], rec["host_warp_ms"], rec["max_abs_err"], rec["graph_equals_eager"]), flush=True)
            with open(args.out, "w") as f:                   # kept current: a run that is cut short leaves what it measured
                json.dump(result, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
