"""Per-component measurements, contingency tables and lesion-wise scores on the device against the host detour they replace
-> profiles/regions_bench.json.

Shapes (1, 1, S, S, S), S = 96, 128, 160; masks: one blob, many lesions, thresholded noise.  Per case, in ONE process on ONE machine:
  eager_ms      the call issued eagerly, device events around it, median of REPLAYS calls
  graph_ms      the same call captured in a HIP graph, median of REPLAYS replays timed by device events (steady state: warmed, replayed)
  host_ms       what a user does without it: .cpu() -> scipy.ndimage / numpy -> .cuda(), host clock around work that ends in a synchronise,
                median of HOST_REPS
  ratio         host_ms / graph_ms; the two results are compared for equality
    region_props   labels (from ops.cc_label, not timed) -> count, box, coordinate sums;  host: find_objects + bincount + index sums
    contingency    two label volumes -> the table;                                       host: np.bincount(a * (rows_b + 1) + b)
    lesion_metrics two masks -> the record (labelling included on both sides);           host: scipy.ndimage.label twice + bincount

    python tools/bench_regions.py [--out profiles/regions_bench.json] [--sides 96 128 160]
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
KINDS = ("blob", "lesions", "noise")
REPLAYS, HOST_REPS = 20, 2
ROWS = 2047                      # rows of the tables: what evaluation.lesion_metrics uses


def smooth_noise(shape, seed, passes=2):
    x = np.random.RandomState(seed).rand(*shape).astype(np.float32)
    for _ in range(passes):
        for ax in range(3):
            x = (x + np.roll(x, 1, ax) + np.roll(x, -1, ax)) / 3
    return x


def make_masks(kind, s):
    """-> (pred, gt) bool (s, s, s): the second is the first moved by two voxels, so the two label volumes overlap without being equal"""
    if kind == "blob":
        z, y, x = np.indices((s, s, s))
        m = ((z - s / 2) ** 2 + (y - s / 2) ** 2 + (x - s / 2) ** 2) < (0.35 * s) ** 2
    elif kind == "lesions":
        rs = np.random.RandomState(s)
        m = np.zeros((s, s, s), bool)
        for _ in range(400):
            c = rs.randint(4, s - 4, size=3)
            r = rs.randint(1, 4)
            m[c[0] - r:c[0] + r, c[1] - r:c[1] + r, c[2] - r:c[2] + r] = True
    else:
        m = smooth_noise((s, s, s), 20, passes=3) >= 0.52          # specks: fewer than ROWS components at these sizes is not guaranteed — recorded
    return np.roll(m, 2, axis=2), m


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


def flat(out):
    import torch
    ts = [out[k] for k in sorted(out)] if isinstance(out, dict) else list(out)
    return [torch.nan_to_num(t.double(), nan=-7.0) for t in ts]


def measure(bufs, dev_fn, host_fn):
    """dev_fn(*bufs) -> dict / tuple of device tensors; host_fn(*bufs) -> the same from the host detour, on the device again"""
    import torch
    eager = flat(dev_fn(*bufs))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev_fn(*bufs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = dev_fn(*bufs)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    e_ms = timed(lambda: dev_fn(*bufs))
    g_ms = timed(graph.replay)
    host = []
    for _ in range(HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = host_fn(*bufs)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    got = flat(out)
    same = all(torch.equal(a, b) for a, b in zip(got, eager)) and all(torch.equal(a, b.to(a.device)) for a, b in zip(got, flat(ref)))
    g, h = statistics.median(g_ms), statistics.median(host)
    return {"eager_ms": statistics.median(e_ms), "graph_ms": g, "graph_ms_min": min(g_ms), "graph_ms_max": max(g_ms), "host_ms": h, "host_ms_min": min(host),
            "ratio_host_over_graph": h / g, "device_equals_host": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "regions_bench.json"))
    ap.add_argument("--sides", type=int, nargs="+", default=list(SIDES))
    args = ap.parse_args()
    import torch
    from scipy import ndimage
    from vae_segmentation_amd import evaluation, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions.py measures on the GPU; there is none here")
    full = ndimage.generate_binary_structure(3, 3)
    cases = {}
    result = {"what": "ops.region_props / ops.contingency / evaluation.lesion_metrics eager and replayed from a HIP graph vs .cpu() + scipy.ndimage / numpy + .cuda(), "
                      "same process", "device": torch.cuda.get_device_name(0), "replays": REPLAYS, "host_reps": HOST_REPS, "rows": ROWS, "cases": cases}

    def record(key, rec, **more):
        rec.update(more)
        cases[key] = rec
        print("%-28s eager %.3f ms  graph %.3f ms  host %.1f ms  x%.0f  same=%s"
              % (key, rec["eager_ms"], rec["graph_ms"], rec["host_ms"], rec["ratio_host_over_graph"], rec["device_equals_host"]), flush=True)
        with open(args.out, "w") as f:                       # kept current: a run that is cut short leaves what it measured
            json.dump(result, f, indent=1)

    def host_props(labels):
        lab = labels.cpu().numpy()[0, 0]
        d, h, w = lab.shape
        inside = np.where(lab <= ROWS, lab, 0)
        count = np.bincount(inside.ravel(), minlength=ROWS + 1)[1:ROWS + 1]
        bbox = np.empty((ROWS, 6), np.int32)
        bbox[:, :3], bbox[:, 3:] = (d, h, w), -1
        for i, sl in enumerate(ndimage.find_objects(inside, max_label=ROWS)):
            if sl is not None:
                bbox[i] = [s.start for s in sl] + [s.stop - 1 for s in sl]
        flat_lab = inside.ravel()
        sums = np.stack([np.bincount(flat_lab, weights=c.ravel(), minlength=ROWS + 1)[1:ROWS + 1] for c in np.indices(lab.shape)], -1).astype(np.int64)
        return {"bbox": torch.from_numpy(bbox).cuda(), "count": torch.from_numpy(count).cuda(), "overflow": torch.tensor(int((lab > ROWS).sum())).cuda(),
                "sums": torch.from_numpy(sums).cuda()}

    def dev_props(labels):
        out = ops.region_props(labels, max_components=ROWS)
        return {k: out[k][0, 0] for k in ("bbox", "count", "overflow", "sums")}

    def host_contingency(a, b):
        x, y = a.cpu().numpy().ravel().astype(np.int64), b.cpu().numpy().ravel().astype(np.int64)
        ok = (x <= ROWS) & (y <= ROWS)
        table = np.bincount(x[ok] * (ROWS + 1) + y[ok], minlength=(ROWS + 1) ** 2).reshape(ROWS + 1, ROWS + 1)
        return torch.from_numpy(table).cuda(), torch.tensor(int((~ok).sum())).cuda()

    def dev_contingency(a, b):
        table, overflow = ops.contingency(a, b, ROWS, ROWS)
        return table[0, 0], overflow[0, 0]

    def host_lesion(p, g):
        P, n_pred = ndimage.label(p.cpu().numpy()[0, 0] >= 0.5, structure=full)
        G, n_gt = ndimage.label(g.cpu().numpy()[0, 0] >= 0.5, structure=full)
        T = np.bincount(P.ravel().astype(np.int64) * (n_gt + 1) + G.ravel(), minlength=(n_pred + 1) * (n_gt + 1)).reshape(n_pred + 1, n_gt + 1)[1:, 1:]
        tp, fp = int((T.sum(0) >= 1).sum()), int((T.sum(1) == 0).sum())
        return {k: torch.tensor(v).cuda() for k, v in (("fn", n_gt - tp), ("fp", fp), ("n_gt", n_gt), ("n_pred", n_pred), ("tp", tp))}

    def dev_lesion(p, g):
        rec = evaluation.lesion_metrics(p, g)
        return {k: rec[k][0, 0] for k in ("fn", "fp", "n_gt", "n_pred", "tp")}

    for s in args.sides:
        for kind in KINDS:
            pred, gt = make_masks(kind, s)
            mp, mg = (torch.from_numpy(m.astype(np.float32)).cuda().view(1, 1, s, s, s) for m in (pred, gt))
            lp, counts_p, _ = ops.cc_label(mp)
            lg, counts_g, _ = ops.cc_label(mg)
            more = {"shape": [1, 1, s, s, s], "components": [int(counts_p.max()), int(counts_g.max())]}
            record("%d/%s/region_props" % (s, kind), measure((lp,), dev_props, host_props), **more)
            record("%d/%s/contingency" % (s, kind), measure((lp, lg), dev_contingency, host_contingency), **more)
            record("%d/%s/lesion_metrics" % (s, kind), measure((mp, mg), dev_lesion, host_lesion), **more)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
