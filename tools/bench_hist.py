"""Histograms, joint histograms and mutual information on the device against what they replace -> profiles/hist_bench.json.

Volumes (1, 1, S, S, S), S = 96, 128, 160, of two kinds: "smooth" (blurred noise: neighbouring voxels fall into neighbouring cells) and "ct" (70 % of the
voxels at one value in long runs, the air of a CT scan, the rest smooth).  Per case, in ONE process on ONE machine:
  (a) fused      ops.joint_histogram (256 x 256, bounds from the data) + ops.mutual_information; ops.histogram with 256 bins, with and without a label
                 volume of 4 classes.  Every counting kernel that can hold the table is timed (vs_config.hist_form: lds32 / packed / global) next to
                 the one the library picks ("auto"), and their tables are compared for equality; further joint tables of 64 x 64 and 512 x 512 cells.
  (b) composed   what the parent commit offers: torch.bucketize of both volumes against the same edges, then ops.contingency.
  (c) host       x.cpu() -> np.histogram2d -> scipy.ndimage.gaussian_filter -> numpy, host clock around work that starts on the device.
eager_ms: the calls issued eagerly, device events around BATCH calls, median of SAMPLES; graph_ms: the same calls captured in a HIP graph, events around
BATCH replays, median of SAMPLES.  No ratio is asserted.

    python tools/bench_hist.py [--out profiles/hist_bench.json] [--sides 96 128 160]
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
FORMS = {"auto": 0, "lds32": 1, "packed": 2, "global": 3}
LDS32_CELLS, PACKED_CELLS = 8192, 65536          # csrc/hist.hip HS_LDS32_CELLS, HS_PACKED_CELLS
BATCH, SAMPLES, HOST_REPS = 10, 7, 2


def smooth(shape, seed, passes=2):
    x = np.random.RandomState(seed).randn(*shape).astype(np.float32)
    for _ in range(passes):
        for ax in range(3):
            x = (x + np.roll(x, 1, ax) + np.roll(x, -1, ax)) / 3
    return x / np.abs(x).max()


def make(kind, s, seed):
    v = smooth((s, s, s), seed)
    if kind == "ct":
        flat = v.reshape(-1)
        n = int(0.7 * flat.size)
        flat[flat.size // 8: flat.size // 8 + n] = -1.0
    return np.ascontiguousarray(v.reshape(1, 1, s, s, s))


def forms_for(cells):
    return ["auto"] + [f for f, cap in (("lds32", LDS32_CELLS), ("packed", PACKED_CELLS), ("global", None)) if cap is None or cells <= cap]


def served_by(cells):
    return "lds32" if cells <= LDS32_CELLS else "packed" if cells <= PACKED_CELLS else "global"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hist_bench.json"))
    ap.add_argument("--sides", type=int, nargs="+", default=list(SIDES))
    args = ap.parse_args()
    import torch
    from scipy import ndimage
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_hist.py measures on the GPU: no device visible")

    def events(fn):
        out = []
        for _ in range(SAMPLES):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BATCH):
                fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) / BATCH)
        return statistics.median(out)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        eager = events(fn)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        return {"eager_ms": round(eager, 5), "graph_ms": round(events(g.replay), 5)}

    def host_mi(xd, yd):
        x, y = xd.cpu().numpy().ravel(), yd.cpu().numpy().ravel()
        jh = np.histogram2d(x, y, bins=(256, 256))[0]
        jh = ndimage.gaussian_filter(jh, sigma=1, mode="constant") + np.finfo(float).eps
        jh = jh / jh.sum()
        s1, s2 = jh.sum(0), jh.sum(1)
        return (np.sum(s1 * np.log(s1)) + np.sum(s2 * np.log(s2))) / np.sum(jh * np.log(jh)) - 1

    results = []
    for s in args.sides:
        for kind in ("smooth", "ct"):
            x, y = torch.from_numpy(make(kind, s, 1)).cuda(), torch.from_numpy(make(kind, s, 2)).cuda()
            lab = torch.from_numpy(np.random.RandomState(3).randint(0, 4, (1, 1, s, 1, 1)).astype(np.int32)).cuda().expand(1, 1, s, s, s).contiguous()
            cases = {"joint256+mi": (65536, lambda: ops.mutual_information(ops.joint_histogram(x, y)["table"], sigma=1.0)),
                     "joint256": (65536, lambda: ops.joint_histogram(x, y)["table"]),
                     "joint64": (4096, lambda: ops.joint_histogram(x, y, bins=(64, 64))["table"]),
                     "joint512": (512 * 512, lambda: ops.joint_histogram(x, y, bins=(512, 512))["table"]),
                     "hist256": (256, lambda: ops.histogram(x, 256)["table"]),
                     "hist256_labels4": (1024, lambda: ops.histogram(x, 256, labels=lab, rows=3)["table"])}
            for name, (cells, fn) in cases.items():
                rec = {"side": s, "content": kind, "case": name, "cells": cells, "default_form": served_by(cells), "forms": {}}
                tables = []
                for form in forms_for(cells):
                    with ops.config(hist_form=FORMS[form]):
                        rec["forms"][form] = timed(fn)
                        tables.append(fn().clone())
                rec["forms_agree"] = all(torch.equal(tables[0].view(torch.int64), t.view(torch.int64)) for t in tables[1:])
                results.append(rec)
                print(json.dumps(rec), flush=True)
            # (b) bucketize against the fused call's own edges, then the contingency table of the two bin volumes
            fused = ops.joint_histogram(x, y)
            ex, ey = fused["edges_x"][0, 0, 1:-1].float().contiguous(), fused["edges_y"][0, 0, 1:-1].float().contiguous()

            def composed():
                a = torch.bucketize(x, ex, right=True).to(torch.int32)
                b = torch.bucketize(y, ey, right=True).to(torch.int32)
                return ops.contingency(a, b, 255, 255)[0]
            rec = {"side": s, "content": kind, "case": "composed_bucketize+contingency256", "cells": 65536, **timed(composed)}
            rec["total_agrees"] = int(composed().sum()) == int(fused["table"].sum())
            results.append(rec)
            print(json.dumps(rec), flush=True)
            # (c) the host detour
            torch.cuda.synchronize()
            ts = []
            for _ in range(HOST_REPS):
                t0 = time.perf_counter()
                host = host_mi(x, y)
                ts.append((time.perf_counter() - t0) * 1e3)
            dev_mi = float(ops.mutual_information(fused["table"], sigma=1.0))
            rec = {"side": s, "content": kind, "case": "host_histogram2d+scipy", "host_ms": round(statistics.median(ts), 3), "host_nmi": float(host),
                   "device_nmi": dev_mi}
            results.append(rec)
            print(json.dumps(rec), flush=True)
    doc = {"tool": "tools/bench_hist.py", "device": torch.cuda.get_device_name(0), "batch": BATCH, "samples": SAMPLES,
           "form_by_cells": {"lds32": "<= %d" % LDS32_CELLS, "packed": "<= %d" % PACKED_CELLS, "global": "larger"}, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
