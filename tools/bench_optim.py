"""The clipped / Nesterov optimiser step (optim.SGD(nesterov=, max_norm=), csrc/optim.hip) against the plain one and against what one could write without
it -> profiles/optim_clip_bench.json.

ONE process on ONE machine, device events around BATCH calls, medians of SAMPLES after WARMUP:
  (a) the optimiser tail alone on the parameters of Segmentation(1, 2) with random gradients, captured in a HIP graph and replayed: plain SGD, Nesterov,
      Nesterov + clip (two more launches: vs_grad_sqnorm_multi, vs_grad_clip_finish).  floor_ms: the bytes each form moves — parameter, gradient and
      momentum buffer read, parameter and buffer written, the gradient read once more for the norm — over the copy rate measured in the same run (a
      device-to-device copy of 256 MiB, read + write counted).
  (b) the seg_train step at 96^3, batch 2, bf16 kernels through train.GraphedStep (captured tail): plain against Nesterov + clip, alternating.
  (c) the same step with the tail left eager (capture_tail=False, what VS_GRAPH_TAIL=0 selects) and torch.nn.utils.clip_grad_norm_ between the replay and
      optimizer.step() — clipping as one could write it without this feature.
No ratio is asserted.

    python tools/bench_optim.py [--out profiles/optim_clip_bench.json] [--no_step]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

BATCH, SAMPLES, WARMUP = 10, 20, 5
MAX_NORM = 12.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim_clip_bench.json"))
    ap.add_argument("--no_step", action="store_true", help="leave the seg_train steps (b), (c) out")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py measures on the GPU: no device visible")
    import joint_model as M
    from oracle import ref_cpu as O
    from vae_segmentation_amd import optim
    from vae_segmentation_amd import train as T
    from vae_segmentation_amd.modules import set_kernel_dtype

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
        return out

    def summary(v):
        return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}

    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(WARMUP):
        dst.copy_(src)
    copy_ms = statistics.median(events(lambda: dst.copy_(src)))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)
    del src, dst
    doc = {"tool": "tools/bench_optim.py", "device": torch.cuda.get_device_name(0), "batch": BATCH, "samples": SAMPLES, "warmup": WARMUP,
           "max_norm": MAX_NORM, "copy_bytes_per_s": copy_rate}
    print("copy rate %.3g B/s" % copy_rate, flush=True)

    # (a) the tail alone
    tail = {}
    for name, kw, words in (("plain", {}, 5), ("nesterov", {"nesterov": True}, 5), ("nesterov_clip", {"nesterov": True, "max_norm": MAX_NORM}, 6)):
        seg = O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=0).cuda()
        params = list(seg.parameters())
        g = torch.Generator(device="cuda").manual_seed(1)
        grads = [torch.randn(p.shape, device="cuda", generator=g) * 1e-3 for p in params]
        opt = optim.SGD(params, lr=1e-4, momentum=0.99, weight_decay=3e-5, **kw)
        opt.prepare(params, grads)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            opt.step_with(params, grads, device_hyper=True)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step_with(params, grads, device_hyper=True)
        for _ in range(WARMUP):
            graph.replay()
        torch.cuda.synchronize()
        n = sum(p.numel() for p in params)
        rec = summary(events(graph.replay))
        rec.update(parameters=n, bytes=words * 4 * n, floor_ms=round(words * 4 * n / copy_rate * 1e3, 5))
        tail[name] = rec
        print(name, json.dumps(rec), flush=True)
        del graph, opt, seg, params, grads
    doc["a_tail_graph_ms"] = tail

    if not args.no_step:
        side_, bs = 96, 2
        img, lab = O.synthetic_image(bs, side_, 2).cuda(), O.synthetic_label(bs, side_, 3).cuda()

        def model():
            seg = O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=0).cuda()
            set_kernel_dtype(seg, torch.bfloat16)
            return seg

        steps = {}
        for name, kw in (("b_plain", {}), ("b_nesterov_clip", {"nesterov": True, "max_norm": MAX_NORM})):
            seg = model()
            opt = optim.SGD(seg.parameters(), lr=1e-2, momentum=0.99, weight_decay=3e-5, **kw)
            gs = T.GraphedStep(lambda seg=seg: T.seg_train_losses(seg, img, lab), list(seg.parameters()), opt, warmup=2)
            assert gs.tail
            steps[name] = gs.step
        seg = model()
        params = list(seg.parameters())
        opt = optim.SGD(params, lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=True)
        gs = T.GraphedStep(lambda seg=seg: T.seg_train_losses(seg, img, lab), params, opt, warmup=2, capture_tail=False)
        assert not gs.tail

        def eager_clip(gs=gs, opt=opt, params=params):
            gs.graph.replay()
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
        steps["c_eager_tail_torch_clip"] = eager_clip
        for fn in steps.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in steps}
        for _ in range(SAMPLES):                  # alternating: the forms share whatever else the machine is doing
            for name, fn in steps.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(BATCH):
                    fn()
                b.record()
                b.synchronize()
                samples[name].append(a.elapsed_time(b) / BATCH)
        doc["seg_train_step_96_b2_bf16_ms"] = {name: summary(v) for name, v in samples.items()}
        print(json.dumps(doc["seg_train_step_96_b2_bf16_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
