"""The compound loss with a top-k cross-entropy (ops.seg_loss(topk=), csrc/topk.hip) against what it adds to and replaces -> profiles/topk_bench.json.

Forward plus backward of the loss alone on softmax outputs (B, C, S, S, S) and label volumes (B, 1, S, S, S), in ONE process on ONE machine:
  (a) topk      ops.seg_loss(topk=r), r = 0.1 and 1: seven forward launches, one backward
  (b) plain     ops.seg_loss without topk — the parent's cost
  (c) composed  what one could write on the parent commit: the Dice of ops.seg_loss(ce_weight=0) plus torch.topk over -(w log p_l) flattened, K taken from
                a count read back to the host.  It synchronises, so it cannot be captured: its time is the eager one.  It stands for the COST of that
                spelling only: its value is not the rule's (K = int(r N), no focal factor, clamp_min(tiny) for the -100 clamp, torch.topk's tie-break),
                so its output is not compared with (a)'s
  (d) floor     the bytes the eight launches must move over the copy rate measured in the same run (a device-to-device copy of 256 MiB, read + write
                counted): the first pass reads (C + 1) and writes 1 plane of 4 B V bytes, three count passes and the sums read 1 each, the backward reads
                C + 2 and writes C — (3 C + 8) 4 B V; what the sums read of label and p on top (r-dependent) is not counted
eager_ms: the calls issued eagerly, device events around BATCH calls; graph_ms: the same calls captured in a HIP graph, events around BATCH replays; both
medians of SAMPLES after WARMUP.  "saturated" repeats the first shape with p_l = 1 at 95 % of the voxels: the keys nearly all 0, the tables' worst case.
  (e) the seg_train step at 96^3, batch 2, bf16 kernels, graph-replayed (train.GraphedStep), with --seg_loss dice_ce and with --ce_topk 10 on top,
      alternating.  No ratio is asserted.

    python tools/bench_topk.py [--out profiles/topk_bench.json] [--no_step]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = ((2, 2, 96), (2, 4, 96), (1, 2, 128), (2, 8, 128))          # (B, C, side)
RS = (0.1, 1.0)
BATCH, SAMPLES, WARMUP = 10, 20, 5


def floor_bytes(b, c, v):
    return (3 * c + 8) * 4 * b * v


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "topk_bench.json"))
    ap.add_argument("--no_step", action="store_true", help="leave the seg_train step out")
    args = ap.parse_args()
    import torch
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk.py measures on the GPU: no device visible")

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

    def timed(fn, graph=True):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        out = {"eager_ms": round(events(fn), 5)}
        if graph:
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
            out["graph_ms"] = round(events(g.replay), 5)
        return out

    # the copy rate of this run: 256 MiB device to device, bytes read + bytes written
    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(WARMUP):
        dst.copy_(src)
    copy_ms = events(lambda: dst.copy_(src))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)
    del src, dst
    doc = {"tool": "tools/bench_topk.py", "device": torch.cuda.get_device_name(0), "batch": BATCH, "samples": SAMPLES, "warmup": WARMUP,
           "copy_bytes_per_s": copy_rate, "results": []}
    print("copy rate %.3g B/s" % copy_rate, flush=True)
    tiny = torch.finfo(torch.float32).tiny
    for kind, (b, c, s) in [("softmax", shape) for shape in SHAPES] + [("saturated", SHAPES[0])]:
        g = torch.Generator(device="cuda").manual_seed(s + c)
        lab = torch.randint(0, c, (b, 1, s, s, s), device="cuda", generator=g).float()
        lab_long = lab.long()
        p = torch.softmax(torch.randn(b, c, s, s, s, device="cuda", generator=g) * 2, 1)
        if kind == "saturated":
            hot = torch.zeros_like(p).scatter_(1, lab_long, 1.0)
            p = torch.where(torch.rand(b, 1, s, s, s, device="cuda", generator=g) < 0.95, hot, p)
        p.requires_grad_(True)
        tgt = ops.LabelTarget(lab)
        w = torch.ones(c, device="cuda")

        def fused(**kw):
            def fn():
                p.grad = None
                final, _ = ops.seg_loss(p, tgt, botindex=1, topindex=c, eps=1e-4, **kw)
                final.backward()
            return fn

        def composed(r):
            def fn():
                p.grad = None
                final, _ = ops.seg_loss(p, tgt, botindex=1, topindex=c, eps=1e-4, ce_weight=0.0)
                valid = (lab >= 0) & (lab < c)
                loss = -(w[lab_long] * torch.log(p.gather(1, lab_long).clamp_min(tiny)))[valid]
                k = max(1, int(r * int(valid.sum().item())))               # the read-back: K depends on a device count
                final = final + torch.topk(loss, k, sorted=False).values.mean()
                final.backward()
            return fn

        nbytes = floor_bytes(b, c, s ** 3)
        rec = {"input": kind, "batch": b, "channels": c, "side": s, "bytes": nbytes, "d_floor_ms": round(nbytes / copy_rate * 1e3, 5),
               "workspace_bytes": ops.lib.vs_seg_topk_workspace_bytes(b, s ** 3), "b_seg_loss": timed(fused())}
        for r in RS:
            rec["a_topk_r%g" % r] = timed(fused(topk=r))
            rec["c_dice_plus_torch_topk_r%g" % r] = timed(composed(r), graph=False)
        doc["results"].append(rec)
        print(json.dumps(rec), flush=True)
        del p, lab, lab_long, tgt

    if not args.no_step:
        import joint_model as M
        from oracle import ref_cpu as O
        from vae_segmentation_amd import optim
        from vae_segmentation_amd import train as T
        from vae_segmentation_amd.modules import set_kernel_dtype
        side, bs = 96, 2
        img, lab = O.synthetic_image(bs, side, 2).cuda(), O.synthetic_label(bs, side, 3).cuda()
        steps = {}
        for name, loss in (("dice_ce", {"ce_weight": 1.0}), ("dice_ce_topk10", {"ce_weight": 1.0, "topk": 0.1})):
            seg = O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=0).cuda()
            set_kernel_dtype(seg, torch.bfloat16)
            opt = optim.SGD(seg.parameters(), lr=1e-2, momentum=0.9)
            steps[name] = T.GraphedStep(lambda seg=seg, loss=loss: T.seg_train_losses(seg, img, lab, loss=loss), list(seg.parameters()), opt, warmup=2)
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
        doc["seg_train_step_96_b2_bf16_ms"] = {name: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
                                               for name, v in samples.items()}
        print(json.dumps(doc["seg_train_step_96_b2_bf16_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
