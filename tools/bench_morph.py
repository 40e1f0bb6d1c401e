"""Binary morphology and hole filling on the device against the host detour they replace -> profiles/morph_bench.json.

Shapes (1, 2, S, S, S), S = 96, 128, 160.  Per case, in ONE process on ONE machine:
  eager_ms      the op issued eagerly, device events around it, median of REPLAYS calls
  graph_ms      the same call captured in a HIP graph, median of REPLAYS replays timed by device events (steady state: warmed, replayed)
  host_ms       what a user does without it: mask.cpu() -> scipy.ndimage per plane -> .cuda(), host clock around work that ends in a synchronise,
                median of HOST_REPS
  ratio         host_ms / graph_ms; the two results are compared bit for bit
Morphology: op x connectivity x iterations in {1, 2, 5} on a thresholded smooth-noise mask.  Hole filling, connectivity 6 and 26: the synthetic organ
label with random pores ("blob") and a serpentine background corridor that reaches the border at one end only (the deepest union-find chains).

    python tools/bench_morph.py [--out profiles/morph_bench.json] [--sides 96 128 160]
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

SIDES = (96, 128, 160)
OPS = ("dilate", "erode", "open", "close")
ITERATIONS = (1, 2, 5)
REPLAYS, HOST_REPS = 20, 2


def smooth_noise(shape, seed, passes=2):
    x = np.random.RandomState(seed).rand(*shape).astype(np.float32)
    for _ in range(passes):
        for ax in range(3):
            x = (x + np.roll(x, 1, ax) + np.roll(x, -1, ax)) / 3
    return x


def serpentine(shape):
    d, h, w = shape
    m = np.zeros(shape, bool)
    for zi, z in enumerate(range(0, d, 2)):
        ys = list(range(0, h, 2))[::-1 if zi % 2 else 1]
        side = 0
        for i, y in enumerate(ys):
            m[z, y, :] = True
            if i + 1 < len(ys):
                m[z, (y + ys[i + 1]) // 2, w - 1 if side == 0 else 0] = True
                side ^= 1
        if z + 2 < d:
            m[z + 1, ys[-1], w - 1 if side == 0 else 0] = True
    return m


def make_mask(kind, s):
    """-> float32 (1, 2, s, s, s)"""
    from vae_segmentation_amd import synthetic
    if kind == "noise":
        return np.stack([smooth_noise((s, s, s), 20 + c) >= 0.505 for c in range(2)]).astype(np.float32)[None]
    if kind == "blob":
        chans = []
        for c in range(2):
            lab = synthetic.synthetic_label(1, s, 3 + c).numpy().reshape(s, s, s) > 0.5
            chans.append(lab & ~(np.random.RandomState(10 + c).rand(s, s, s) < 2e-2))
        return np.stack(chans).astype(np.float32)[None]
    m = np.ones((s, s, s), bool)
    m[1:-1, 1:-1, 1:-1] = ~serpentine((s - 2,) * 3)
    m[0, 1, 1] = False
    return np.stack([m, m[::-1].copy()]).astype(np.float32)[None]


def host_path(x, fn):
    import torch
    a = x.cpu().numpy() >= 0.5
    out = np.empty(a.shape, np.float32)
    for n in range(a.shape[0]):
        for c in range(a.shape[1]):
            out[n, c] = fn(a[n, c])
    res = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    return res


def timed(fn):
    import torch
    ms = []
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def measure(buf, dev_fn, host_fn):
    import torch
    eager = dev_fn(buf)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev_fn(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dev_fn(buf)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    e_ms = timed(lambda: dev_fn(buf))
    g_ms = timed(graph.replay)
    host = []
    for _ in range(HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = host_path(buf, host_fn)
        host.append((time.perf_counter() - t0) * 1e3)
    same = bool(torch.equal(ref, out)) and bool(torch.equal(eager, out))
    g, h = statistics.median(g_ms), statistics.median(host)
    return {"eager_ms": statistics.median(e_ms), "graph_ms": g, "graph_ms_min": min(g_ms), "graph_ms_max": max(g_ms), "host_ms": h, "host_ms_min": min(host),
            "ratio_host_over_graph": h / g, "device_equals_host": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "morph_bench.json"))
    ap.add_argument("--sides", type=int, nargs="+", default=list(SIDES))
    args = ap.parse_args()
    import torch
    from scipy import ndimage
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_morph.py measures on the GPU; there is none here")
    struct = {6: ndimage.generate_binary_structure(3, 1), 26: np.ones((3, 3, 3), bool)}
    scipy_op = {"dilate": ndimage.binary_dilation, "erode": ndimage.binary_erosion, "open": ndimage.binary_opening, "close": ndimage.binary_closing}
    cases = {}

    def record(key, rec, shape):
        rec["shape"] = list(shape)
        cases[key] = rec
        print("%-28s eager %.3f ms  graph %.3f ms  host %.1f ms  x%.0f  same=%s"
              % (key, rec["eager_ms"], rec["graph_ms"], rec["host_ms"], rec["ratio_host_over_graph"], rec["device_equals_host"]), flush=True)
        with open(args.out, "w") as f:                       # kept current: a run that is cut short leaves what it measured
            json.dump(result, f, indent=1)

    result = {"what": "ops.morph / ops.fill_holes eager and replayed from a HIP graph vs .cpu() + scipy.ndimage per plane + .cuda(), same process",
              "device": torch.cuda.get_device_name(0), "replays": REPLAYS, "host_reps": HOST_REPS, "cases": cases}
    for s in args.sides:
        buf = torch.from_numpy(make_mask("noise", s)).cuda()
        for op in OPS:
            for conn in (6, 26):
                for it in ITERATIONS:
                    rec = measure(buf, lambda x: ops.morph(x, op, iterations=it, connectivity=conn),
                                  lambda m: scipy_op[op](m, structure=struct[conn], iterations=it))
                    record("%d/%s/c%d/n%d" % (s, op, conn, it), rec, buf.shape)
        for kind in ("blob", "serpentine"):
            x_np = make_mask(kind, s)
            buf = torch.from_numpy(x_np).cuda()
            for conn in (6, 26):
                rec = measure(buf, lambda x: ops.fill_holes(x, connectivity=conn), lambda m: ndimage.binary_fill_holes(m, structure=struct[conn]))
                rec["background_voxels"] = int((x_np < 0.5).sum())
                record("%d/fill_holes/%s/c%d" % (s, kind, conn), rec, buf.shape)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
