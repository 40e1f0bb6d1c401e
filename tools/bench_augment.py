"""Intensity augmentation on the device against the two ways to get it without the new kernels -> profiles/augment_bench.json.

One channel of P^3 voxels, P = 64, 96, 128 (mean 0, std 0.5, as CenterIntensities leaves a CT patch).  Per op — noise (s 0.05, Philox), blur (sigma 1,
radius 4), brightness, contrast (preserve_range), inverted gamma and gamma (retain_stats), flip (all axes) — and for the full chain of the seven with every
gate open, in ONE process on ONE machine:
  eager_ms   data_gpu.intensity_augment issued eagerly, device events around it, median of REPLAYS calls
  graph_ms   captured in a HIP graph, median of REPLAYS replays
  torch_ms   (a) the same op or chain written with torch calls on the device (torch.randn noise, symmetric padding + three conv3d for the blur,
             x.min() / x.mean() / x.std() kept as device tensors so that nothing synchronises), eager, device events, median of REPLAYS
  host_ms    (b) x.cpu() -> numpy / scipy.ndimage.gaussian_filter -> .cuda(), host clock around work that ends in a synchronise, median of HOST_REPS
No ratio is fixed in advance; the file records what was measured.

    python tools/bench_augment.py [--out profiles/augment_bench.json] [--sides 64 96 128]
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

SIDES = (64, 96, 128)
REPLAYS, HOST_REPS = 20, 3
OPS = {"noise": ("noise", 0.05, (7, 3)), "blur": ("blur", 1.0), "brightness": ("brightness", 1.1), "contrast": ("contrast", 1.2, True),
       "gamma_inverted": ("gamma", 0.8, True, True), "gamma": ("gamma", 1.3, False, True), "flip": ("flip", 7)}


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


# ---- (a) the chain in torch on the device ----------------------------------------------------------------------------------------------------
def _sym_pad(x, r, dim):
    import torch
    n = x.shape[dim]
    idx = torch.arange(-r, n + r, device=x.device) % (2 * n)
    idx = torch.where(idx < n, idx, 2 * n - 1 - idx)
    return x.index_select(dim, idx)


def torch_op(x, op):
    """x: (1, D, H, W) float32 on the device; fp64 arithmetic and one float32 rounding per op, as the kernels compute"""
    import torch
    import torch.nn.functional as F
    name = op[0]
    v = x.double()
    if name == "noise":
        return (v + op[1] * torch.randn(x.shape, dtype=torch.float64, device=x.device)).float()
    if name == "blur":
        sigma = op[1]
        r = int(4.0 * sigma + 0.5)
        k = torch.arange(-r, r + 1, dtype=torch.float64, device=x.device)
        w = torch.exp(-0.5 / (sigma * sigma) * k * k)
        w = w / w.sum()
        y = x
        for dim, shape in ((1, (1, 1, -1, 1, 1)), (2, (1, 1, 1, -1, 1)), (3, (1, 1, 1, 1, -1))):
            y = F.conv3d(_sym_pad(y.double(), r, dim)[None], w.view(shape))[0].float()
        return y
    if name == "brightness":
        return (v * op[1]).float()
    if name == "contrast":
        mean = v.mean()
        y = (v - mean) * op[1] + mean
        return (torch.minimum(torch.maximum(y, v.min()), v.max()) if op[2] else y).float()
    if name == "gamma":
        g, invert, retain = op[1], op[2], op[3]
        if invert:
            v = -v
        mean0, std0 = v.mean(), v.std(unbiased=False)
        mn = v.min()
        rng = v.max() - mn
        y = torch.pow((v - mn) / (rng + 1e-7), g) * rng + mn
        if retain:
            y = y.float().double()
            y = (y - y.mean()) / (y.std(unbiased=False) + 1e-8) * std0 + mean0
        return (-y if invert else y).float()
    if name == "flip":
        return torch.flip(x, [d for d, bit in zip((1, 2, 3), (4, 2, 1)) if op[1] & bit]).contiguous()
    raise ValueError(name)


def torch_chain(x, ops_list):
    for op in ops_list:
        x = torch_op(x, op)
    return x


# ---- (b) the host detour ---------------------------------------------------------------------------------------------------------------------
def host_chain(x, ops_list, rng):
    import torch
    from scipy import ndimage
    v = x.cpu().numpy()[0]
    for op in ops_list:
        name = op[0]
        if name == "noise":
            v = (v + op[1] * rng.normal(0.0, 1.0, v.shape)).astype(np.float32)
        elif name == "blur":
            v = ndimage.gaussian_filter(v, op[1], mode="reflect")
        elif name == "brightness":
            v = (v * np.float64(op[1])).astype(np.float32)
        elif name == "contrast":
            d = v.astype(np.float64)
            y = (d - d.mean()) * op[1] + d.mean()
            v = (np.clip(y, d.min(), d.max()) if op[2] else y).astype(np.float32)
        elif name == "gamma":
            d = -v.astype(np.float64) if op[2] else v.astype(np.float64)
            mean0, std0, mn, r = d.mean(), d.std(), d.min(), d.max() - d.min()
            y = np.power((d - mn) / (r + 1e-7), op[1]) * r + mn
            if op[3]:
                y = y.astype(np.float32).astype(np.float64)
                y = (y - y.mean()) / (y.std() + 1e-8) * std0 + mean0
            v = (-y if op[2] else y).astype(np.float32)
        elif name == "flip":
            v = np.ascontiguousarray(np.flip(v, [a for a, bit in zip((0, 1, 2), (4, 2, 1)) if op[1] & bit]))
    out = torch.from_numpy(v[None]).cuda()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "augment_bench.json"))
    ap.add_argument("--sides", type=int, nargs="+", default=list(SIDES))
    args = ap.parse_args()
    import torch
    from vae_segmentation_amd import data_gpu as D
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU; there is none here")
    cases = {}
    result = {"what": "data_gpu.intensity_augment eager and replayed from a HIP graph vs the same ops in torch on the device and vs .cpu() + numpy / scipy + "
                      ".cuda(), same process, one channel", "device": torch.cuda.get_device_name(0), "replays": REPLAYS, "host_reps": HOST_REPS,
              "ops": {k: [v[0]] + [list(a) if isinstance(a, tuple) else a for a in v[1:]] for k, v in OPS.items()}, "cases": cases}
    for s in args.sides:
        x = torch.from_numpy((np.random.RandomState(s).randn(1, s, s, s) * 0.5).astype(np.float32)).cuda()
        for name, ops_list in list((k, [v]) for k, v in OPS.items()) + [("chain", list(OPS.values()))]:
            rec = {"shape": [s, s, s]}
            eager, replayed, e_ms, g_ms = eager_and_graph(lambda: D.intensity_augment(x, ops_list))
            rec.update(eager_ms=statistics.median(e_ms), graph_ms=statistics.median(g_ms), graph_ms_min=min(g_ms), graph_ms_max=max(g_ms),
                       graph_equals_eager=bool(torch.equal(eager, replayed)))
            ref = torch_chain(x, ops_list)
            torch.cuda.synchronize()
            rec["torch_ms"] = statistics.median(timed(lambda: torch_chain(x, ops_list)))
            if not any(op[0] == "noise" for op in ops_list):                 # the torch form draws other normals
                rec["torch_max_abs_diff"] = float((ref - eager).abs().max())
            host = []
            for _ in range(HOST_REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_chain(x, ops_list, np.random.RandomState(0))
                host.append((time.perf_counter() - t0) * 1e3)
            rec["host_ms"] = statistics.median(host)
            rec["ratio_torch_over_graph"], rec["ratio_host_over_graph"] = rec["torch_ms"] / rec["graph_ms"], rec["host_ms"] / rec["graph_ms"]
            cases["%d/%s" % (s, name)] = rec
            print("%-20s eager %.3f  graph %.3f ms   torch %.3f ms   host %.1f ms   same=%s  torch diff %s"
                  % ("%d/%s" % (s, name), rec["eager_ms"], rec["graph_ms"], rec["torch_ms"], rec["host_ms"], rec["graph_equals_eager"],
                     rec.get("torch_max_abs_diff", "-")), flush=True)
            with open(args.out, "w") as f:                   # kept current: a run that is cut short leaves what it measured
                json.dump(result, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
