"""The signed distance maps (ops.signed_distance) and the boundary loss (ops.boundary_loss, csrc/sdm.hip) against what one could spell without
them -> profiles/boundary_bench.json.

ONE process on ONE machine.  Labels are (B, 1, S, S, S) volumes with one ellipsoid per foreground class on a background of class 0 — distances of tens of
voxels, as an organ gives; the maps are those of the foreground channels [1, C), K = C - 1, as the training path asks for them.
  (a) signed_distance   ops.signed_distance(label, C, 1, C), against
        composed   the spelling of the parent commit: ops.onehot, the complement, ops.edt(..., squared=True) on the 2 K planes, fp64 sqrt, combine
                   (checked here to give the same bits)
        host       label.cpu() -> two scipy.ndimage.distance_transform_edt per sample and class -> .cuda(), wall clock, HOST_SAMPLES calls after one
        floor      (8 + 36 K) V bytes per sample — the label read twice, both int32 maps written by the x pass, read and written by the y pass, read by
                   the z pass, phi written — over the copy rate measured in the same run (256 MiB device to device, read + write counted)
  (b) boundary loss     forward + backward of ops.BoundaryLoss on given maps, against the torch spelling (p[:, 1:] * phi).mean() with autograd
  (c) the seg_train step at 96^3, batch 2, bf16 kernels, graph-replayed (train.GraphedStep): --seg_loss dice_ce alone against the same with the boundary
      term, alternating; the added time beside the map's and the loss's own graph-replayed times at that shape
eager_ms: the calls issued eagerly, device events around BATCH calls; graph_ms: the same calls captured in a HIP graph, events around BATCH replays; both
medians of SAMPLES after WARMUP.  No ratio is asserted.

    python tools/bench_boundary.py [--out profiles/boundary_bench.json] [--no_step] [--no_host]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = ((2, 2, 96), (2, 4, 96), (1, 2, 128), (2, 8, 128))          # (B, C, side)
BATCH, SAMPLES, WARMUP, HOST_SAMPLES = 10, 20, 5, 3


def ellipsoid_labels(torch, b, c, s):
    """class k = 1..c-1: an ellipsoid of its own centre and radii (about s / 6), later classes over earlier ones; sample j shifted by 3 j voxels"""
    ax = torch.arange(s, device="cuda", dtype=torch.float32)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    lab = torch.zeros(b, 1, s, s, s, device="cuda")
    for j in range(b):
        for k in range(1, c):
            t = k / c
            cz, cy, cx = s * (0.25 + 0.5 * t) + 3 * j, s * (0.3 + 0.4 * ((3 * t) % 1.0)), s * (0.3 + 0.4 * ((5 * t) % 1.0))
            rz, ry, rx = s / 6.0, s / 7.0 + k, s / 5.0 - k
            inside = ((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
            lab[j, 0][inside] = float(k)
    return lab


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "boundary_bench.json"))
    ap.add_argument("--no_step", action="store_true", help="leave the seg_train step out")
    ap.add_argument("--no_host", action="store_true", help="leave the scipy detour out")
    args = ap.parse_args()
    import torch
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_boundary.py measures on the GPU: no device visible")

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
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        eager = events(fn)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        for _ in range(WARMUP):
            g.replay()
        torch.cuda.synchronize()
        return {"eager_ms": round(eager, 5), "graph_ms": round(events(g.replay), 5)}

    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(WARMUP):
        dst.copy_(src)
    copy_ms = events(lambda: dst.copy_(src))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)
    del src, dst
    doc = {"tool": "tools/bench_boundary.py", "device": torch.cuda.get_device_name(0), "batch": BATCH, "samples": SAMPLES, "warmup": WARMUP,
           "host_samples": HOST_SAMPLES, "copy_bytes_per_s": copy_rate, "results": []}
    print("copy rate %.3g B/s" % copy_rate, flush=True)
    for b, c, s in SHAPES:
        k, v = c - 1, s ** 3
        lab = ellipsoid_labels(torch, b, c, s)
        g = torch.Generator(device="cuda").manual_seed(s + c)
        p = torch.softmax(torch.randn(b, c, s, s, s, device="cuda", generator=g) * 2, 1).requires_grad_(True)

        def composed():
            pos = ops.onehot(lab, c)[:, 1:]
            sq = ops.edt(torch.cat([pos, 1.0 - pos], 1), squared=True)
            none = sq == 2 ** 31 - 1
            d = sq.double().sqrt_()
            to_pos, to_neg = d[:, :k], d[:, k:]
            phi = torch.where(pos >= 0.5, 1.0 - to_neg, to_pos)
            return torch.where(none[:, :k] | none[:, k:], torch.zeros_like(phi), phi).float()

        def host():
            from scipy.ndimage import distance_transform_edt as edt
            import numpy as np
            l = lab.cpu().numpy()
            out = np.zeros((b, k, s, s, s), np.float32)
            for j in range(b):
                for i in range(k):
                    pos = l[j, 0] == i + 1
                    if pos.any() and not pos.all():
                        out[j, i] = np.where(pos, -(edt(pos) - 1.0), edt(~pos))
            return torch.from_numpy(out).cuda()

        phi = ops.signed_distance(lab, c, 1, c)
        same = bool(torch.equal(phi, composed()))
        nbytes = b * (8 + 36 * k) * v
        rec = {"batch": b, "channels": c, "side": s, "planes": k, "bytes": nbytes, "floor_ms": round(nbytes / copy_rate * 1e3, 5),
               "composition_gives_the_same_bits": same, "max_abs_phi": float(phi.abs().max()),
               "signed_distance": timed(lambda: ops.signed_distance(lab, c, 1, c)), "composed_parent_spelling": timed(composed)}
        if not args.no_host:
            same_host = bool(torch.equal(phi, host()))
            walls = []
            for _ in range(HOST_SAMPLES):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host()
                torch.cuda.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3)
            rec["host_scipy_detour"] = {"wall_ms": round(statistics.median(walls), 2), "gives_the_same_bits": same_host}
        wt = torch.full((), 0.01, device="cuda")

        def fused():
            p.grad = None
            weighted, _ = ops.BoundaryLoss.apply(p, lab, phi, wt, 1, c)
            weighted.backward()

        def spelled():
            p.grad = None
            (wt * (p[:, 1:] * phi).mean()).backward()

        rec["boundary_loss_fwd_bwd"] = timed(fused)
        rec["torch_mean_spelling_fwd_bwd"] = timed(spelled)
        rec["loss_bytes"] = b * v * 4 * ((1 + 2 * k) + (1 + k + c))          # forward: label, p and phi planes; backward: label, phi planes, every plane of gp
        rec["loss_floor_ms"] = round(rec["loss_bytes"] / copy_rate * 1e3, 5)
        doc["results"].append(rec)
        print(json.dumps(rec), flush=True)
        del p, lab, phi

    if not args.no_step:
        import joint_model as M
        from oracle import ref_cpu as O
        from vae_segmentation_amd import optim
        from vae_segmentation_amd import train as T
        from vae_segmentation_amd.modules import set_kernel_dtype
        side, bs = 96, 2
        img, lab = O.synthetic_image(bs, side, 2).cuda(), O.synthetic_label(bs, side, 3).cuda()
        loss = {"ce_weight": 1.0}
        wt = torch.full((), 0.01, device="cuda")
        steps = {}
        for name, kw in (("dice_ce", {}), ("dice_ce_boundary", {"boundary": {"weight": wt, "spacing": None}})):
            seg = O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=0).cuda()
            set_kernel_dtype(seg, torch.bfloat16)
            opt = optim.SGD(seg.parameters(), lr=1e-2, momentum=0.9)
            steps[name] = T.GraphedStep(lambda seg=seg, kw=kw: T.seg_train_losses(seg, img, lab, loss=loss, **kw), list(seg.parameters()), opt, warmup=2)
        for gs in steps.values():
            for _ in range(WARMUP):
                gs.step()
        torch.cuda.synchronize()
        samples = {name: [] for name in steps}
        for _ in range(SAMPLES):                  # alternating: the two forms share whatever else the machine is doing
            for name, gs in steps.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(BATCH):
                    gs.step()
                b.record()
                b.synchronize()
                samples[name].append(a.elapsed_time(b) / BATCH)
        med = {name: statistics.median(v) for name, v in samples.items()}
        pred = torch.softmax(torch.randn(bs, 2, side, side, side, device="cuda"), 1).requires_grad_(True)
        phi = ops.signed_distance(lab, 2, 1, 2)

        def loss_only():
            pred.grad = None
            weighted, _ = ops.BoundaryLoss.apply(pred, lab, phi, wt, 1, 2)
            weighted.backward()
        doc["seg_train_step_96_b2_bf16_ms"] = {name: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                                               for name, v in samples.items()}
        doc["seg_train_step_96_b2_bf16_ms"].update({
            "added_ms": round(med["dice_ce_boundary"] - med["dice_ce"], 5),
            "added_percent": round(100.0 * (med["dice_ce_boundary"] - med["dice_ce"]) / med["dice_ce"], 3),
            "map_alone_on_the_step_label": timed(lambda: ops.signed_distance(lab, 2, 1, 2)),
            "loss_fwd_bwd_alone": timed(loss_only)})
        print(json.dumps(doc["seg_train_step_96_b2_bf16_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
