"""The fused deep-supervision head (ops.ds_head, csrc/dshead.hip) against what one could write without it -> profiles/dshead_bench.json.

(a) Forward plus backward of ONE head on a channels-last bf16 feature map (B, d, d, d, C) against the full-resolution label (B, 1, s d, s d, s d), in ONE
process on ONE machine:
  ds_head   ops.ds_head: 1x1x1 convolution + softmax + Dice + cross-entropy, two launches each way, gradients to the feature map, the weight and the bias
  torch     the spelling available without it: ops.UnpackPlanar (channels-last 16-bit -> planar fp32) -> F.conv3d 1x1x1 -> softmax -> ops.seg_loss against
            the strided slice of the label
  floor     the bytes over the copy rate measured in the same run (a device-to-device copy of 256 MiB, read + write counted): the feature map read twice
            (forward, backward), df written, and each way the label ROWS that hold a picked voxel (B d d rows of s d floats: every 128-byte line of such a
            row is touched at s <= 8)
eager_ms: the calls issued eagerly, device events around BATCH calls; graph_ms: the same calls captured in a HIP graph, events around BATCH replays; both
medians of SAMPLES after WARMUP.
(b) The seg_train step at 96^3, batch 2, bf16 kernels, graph-replayed (train.GraphedStep), with --seg_loss dice_ce alone and with --deep_supervision 1
and 2, alternating in one run; median, min and max of SAMPLES.  No ratio is asserted.

    python tools/bench_dshead.py [--out profiles/dshead_bench.json] [--no_step]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPES = ((2, 16, 48, 2), (2, 32, 24, 4), (2, 16, 80, 2), (2, 32, 40, 4))          # (B, C, coarse side, stride)
CLASSES = 2
BATCH, SAMPLES, WARMUP = 10, 20, 5


def head_bytes(b, c, d, s, esize=2):
    feat = b * d ** 3 * c * esize
    rows = b * d * d * s * d * 4
    return 2 * feat + feat + 2 * rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dshead_bench.json"))
    ap.add_argument("--no_step", action="store_true", help="leave the seg_train step out")
    args = ap.parse_args()
    import torch
    from vae_segmentation_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_dshead.py measures on the GPU: no device visible")

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
    doc = {"tool": "tools/bench_dshead.py", "device": torch.cuda.get_device_name(0), "batch": BATCH, "samples": SAMPLES, "warmup": WARMUP,
           "copy_bytes_per_s": copy_rate, "classes": CLASSES, "storage": "bf16", "results": []}
    print("copy rate %.3g B/s" % copy_rate, flush=True)
    k = CLASSES
    for b, c, d, s in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(d + c)
        feat = torch.randn(b, d, d, d, c, device="cuda", generator=g).to(torch.bfloat16).requires_grad_(True)
        wt = (torch.randn(k, c, 1, 1, 1, device="cuda", generator=g) / c ** 0.5).requires_grad_(True)
        bias = torch.zeros(k, device="cuda").requires_grad_(True)
        lab = torch.randint(0, k, (b, 1, s * d, s * d, s * d), device="cuda", generator=g).float()
        tgt = ops.LabelTarget(lab)
        o = s // 2

        def fused():
            feat.grad = wt.grad = bias.grad = None
            final, _ = ops.ds_head(feat, wt, bias, tgt, s, botindex=1, topindex=k, eps=1e-4)
            final.backward()

        def spelled():
            feat.grad = wt.grad = bias.grad = None
            p = torch.softmax(torch.nn.functional.conv3d(ops.UnpackPlanar.apply(feat, c), wt, bias), 1)
            final, _ = ops.seg_loss(p, ops.LabelTarget(lab[:, :, o::s, o::s, o::s]), botindex=1, topindex=k, eps=1e-4)
            final.backward()

        nbytes = head_bytes(b, c, d, s)
        rec = {"batch": b, "channels": c, "coarse_side": d, "stride": s, "bytes": nbytes, "floor_ms": round(nbytes / copy_rate * 1e3, 5),
               "ds_head": timed(fused), "torch_spelling": timed(spelled)}
        doc["results"].append(rec)
        print(json.dumps(rec), flush=True)
        del feat, wt, bias, lab, tgt

    if not args.no_step:
        import joint_model as M
        from oracle import ref_cpu as O
        from vae_segmentation_amd import optim
        from vae_segmentation_amd import train as T
        from vae_segmentation_amd.modules import DeepSupervision, set_kernel_dtype
        side, bs = 96, 2
        img, lab = O.synthetic_image(bs, side, 2).cuda(), O.synthetic_label(bs, side, 3).cuda()
        loss = {"ce_weight": 1.0}
        steps = {}
        for name, levels in (("dice_ce", 0), ("deep_supervision_1", 1), ("deep_supervision_2", 2)):
            seg = O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=0).cuda()
            set_kernel_dtype(seg, torch.bfloat16)
            deep = O.deterministic_fill_(DeepSupervision(seg, levels), seed=1).cuda() if levels else None
            params = list(seg.parameters()) + (list(deep.parameters()) if deep is not None else [])
            opt = optim.SGD(params, lr=1e-2, momentum=0.9)
            steps[name] = T.GraphedStep(lambda seg=seg, deep=deep: T.seg_train_losses(seg, img, lab, loss=loss, deep=deep), params, opt, warmup=2)
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
        doc["seg_train_step_96_b2_bf16_ms"] = {name: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5),
                                                      "captured_tail": bool(steps[name].tail)} for name, v in samples.items()}
        print(json.dumps(doc["seg_train_step_96_b2_bf16_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
