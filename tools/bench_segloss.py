"""The compound segmentation loss (ops.seg_loss, csrc/segloss.hip) against what it replaces -> profiles/segloss_bench.json.

Forward plus backward of the loss alone on softmax outputs (B, C, S, S, S) and label volumes (B, 1, S, S, S), in ONE process on ONE machine:
  seg_loss      ops.seg_loss: Dice + cross-entropy, per-sample and batch Dice, gamma 0 and 2
  (a) dice      ops.dice_loss_sum with the label target alone — what the step pays today
  (b) composed  the same Dice plus torch.nn.functional.nll_loss(torch.log(p.clamp_min(tiny)), label.long()) — the compound loss as one could spell it
                on the parent commit
  (c) floor     the bytes over the copy rate measured in the same run (a device-to-device copy of 256 MiB, read + write counted): forward reads
                (C + 1) 4 B V bytes, backward reads that and writes C 4 B V
eager_ms: the calls issued eagerly, device events around BATCH calls; graph_ms: the same calls captured in a HIP graph, events around BATCH replays; both
medians of SAMPLES after WARMUP.  Then the seg_train step at 96^3, batch 2, bf16 kernels, graph-replayed (train.GraphedStep), with the default loss and with
--seg_loss dice_ce (plain, and with --batch_dice), alternating.  No ratio is asserted.

    python tools/bench_segloss.py [--out profiles/segloss_bench.json] [--no_step]
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
BATCH, SAMPLES, WARMUP = 10, 20, 5


def loss_bytes(b, c, v):
    fwd = (c + 1) * 4 * b * v
    return fwd, fwd + c * 4 * b * v


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "segloss_bench.json"))
    ap.add_argument("--no_step", action="store_true", help="leave the seg_train step out")
    args = ap.parse_args()
    import torch
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_segloss.py measures on the GPU: no device visible")

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

    # the copy rate of this run: 256 MiB device to device, bytes read + bytes written
    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(WARMUP):
        dst.copy_(src)
    copy_ms = events(lambda: dst.copy_(src))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)
    del src, dst
    doc = {"tool": "tools/bench_segloss.py", "device": torch.cuda.get_device_name(0), "batch": BATCH, "samples": SAMPLES, "warmup": WARMUP,
           "copy_bytes_per_s": copy_rate, "results": []}
    print("copy rate %.3g B/s" % copy_rate, flush=True)
    tiny = torch.finfo(torch.float32).tiny
    for b, c, s in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(s + c)
        p = torch.softmax(torch.randn(b, c, s, s, s, device="cuda", generator=g) * 2, 1).requires_grad_(True)
        lab = torch.randint(0, c, (b, 1, s, s, s), device="cuda", generator=g).float()
        lab_long = lab[:, 0].long()
        tgt = ops.LabelTarget(lab)

        def fused(**kw):
            def fn():
                p.grad = None
                final, _ = ops.seg_loss(p, tgt, botindex=1, topindex=c, eps=1e-4, **kw)
                final.backward()
            return fn

        def dice():
            p.grad = None
            final, _ = ops.dice_loss_sum(p, [(tgt, 1.0)], botindex=1, topindex=c, eps=1e-4)
            final.backward()

        def composed():
            p.grad = None
            final, _ = ops.dice_loss_sum(p, [(tgt, 1.0)], botindex=1, topindex=c, eps=1e-4)
            final = final + torch.nn.functional.nll_loss(torch.log(p.clamp_min(tiny)), lab_long)
            final.backward()

        fwd_b, bwd_b = loss_bytes(b, c, s ** 3)
        rec = {"batch": b, "channels": c, "side": s, "bytes_fwd": fwd_b, "bytes_bwd": bwd_b,
               "floor_ms": round((fwd_b + bwd_b) / copy_rate * 1e3, 5),
               "seg_loss": timed(fused()), "seg_loss_batch_dice": timed(fused(batch_dice=True)), "seg_loss_gamma2": timed(fused(gamma=2.0)),
               "a_dice_loss_sum": timed(dice), "b_dice_plus_torch_nll": timed(composed)}
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
        for name, loss in (("dice", None), ("dice_ce", {"ce_weight": 1.0}), ("dice_ce_batch_dice", {"ce_weight": 1.0, "batch_dice": True})):
            seg = O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=0).cuda()
            set_kernel_dtype(seg, torch.bfloat16)
            opt = optim.SGD(seg.parameters(), lr=1e-2, momentum=0.9)
            steps[name] = T.GraphedStep(lambda seg=seg, loss=loss: T.seg_train_losses(seg, img, lab, loss=loss), list(seg.parameters()), opt, warmup=2)
        for gs in steps.values():
            for _ in range(WARMUP):
                gs.step()
        torch.cuda.synchronize()
        samples = {name: [] for name in steps}
        for _ in range(SAMPLES):                  # alternating: the three forms share whatever else the machine is doing
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
