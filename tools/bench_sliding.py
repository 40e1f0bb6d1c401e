"""Sliding-window prediction of a whole volume on the device -> profiles/sliding_bench.json.

Volume 256 x 256 x 192 (one channel), cubic windows of 96 and 128, overlap 0.5, Gaussian blend, bf16 Segmentation(1, 2), one window per forward pass.
Per window size, in ONE process on ONE machine, every figure the median of REPS repetitions after WARMUP (device events around the work):
  eager_ms        evaluation.SlidingWindow called eagerly: the volume copy, per batch gather -> network -> accumulate -> counter bump, finalize
  graph_ms        the same object with graph=True: the batch captured once, replayed ceil(nw / B) times (results compared bit for bit with eager)
  network_ms      the network forward alone on a fixed window buffer, as many times as there are batches
  kernels_ms      gather + accumulate per batch and one finalize alone (the network's answer is a fixed tensor)
  torch_blend_ms  the same gather / blend / normalise / argmax written with plain torch slicing ops on the same tensors (no network either), and
                  the largest difference of its probabilities from the kernels'
  kernels         per kernel: microseconds per launch from back-to-back launches between two events, the bytes the launch has to move (from the
                  shapes) and the rate that makes, beside the copy rate the project uses as its practical ceiling (6.3 TB/s)

    python tools/bench_sliding.py [--out profiles/sliding_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SHAPE = (256, 256, 192)
PATCHES = (96, 128)
OVERLAP, BLEND, BATCH = 0.5, "gaussian", 1
REPS, WARMUP, KERNEL_LAUNCHES = 20, 3, 50
COPY_CEILING = 6.3e12


def timed(fn, reps=REPS, warmup=WARMUP):
    """median / min / max milliseconds of fn() between two device events"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def torch_blend(vol, origins, w3, prob, patch, acc, wsum):
    """the blend with slicing ops: what a user writes without the kernels (one window at a time, the host knows the origins)"""
    import torch
    acc.zero_()
    wsum.zero_()
    buf = torch.empty((1, vol.shape[0]) + (patch,) * 3, device=vol.device)
    for oz, oy, ox in origins:
        sl = (slice(oz, oz + patch), slice(oy, oy + patch), slice(ox, ox + patch))
        buf[0].copy_(vol[(slice(None),) + sl])
        acc[(slice(None),) + sl] += w3 * prob[0]
        wsum[sl] += w3
    out = acc / wsum
    return out, out.argmax(0).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sliding_bench.json"))
    args = ap.parse_args()
    import torch
    import joint_model as M
    from vae_segmentation_amd import evaluation, ops
    from vae_segmentation_amd.modules import set_kernel_dtype
    if not torch.cuda.is_available():
        raise SystemExit("bench_sliding.py measures on the GPU; there is none here")
    torch.manual_seed(0)
    seg = M.Segmentation(n_channels=1, n_class=2, norm_type=1).cuda().eval()
    set_kernel_dtype(seg, torch.bfloat16)
    model_fn = evaluation.segmentation_model_fn(seg)
    vol = torch.randn((1,) + SHAPE, device="cuda")
    voxels = SHAPE[0] * SHAPE[1] * SHAPE[2]
    cases = {}
    for patch in PATCHES:
        eager = evaluation.SlidingWindow(model_fn, vol.shape, patch, overlap=OVERLAP, blend=BLEND, batch=BATCH)
        graphed = evaluation.SlidingWindow(model_fn, vol.shape, patch, overlap=OVERLAP, blend=BLEND, batch=BATCH, graph=True)
        ref = eager(vol)
        same = torch.equal(graphed(vol)["prob"].view(torch.int32), ref["prob"].view(torch.int32))
        k = ref["prob"].shape[0]
        t_eager, t_graph = timed(lambda: eager(vol)), timed(lambda: graphed(vol))
        nb, nw = eager.n_batches, eager.nw
        with torch.no_grad():
            t_net = timed(lambda: [model_fn(eager.windows) for _ in range(nb)])
            fixed = model_fn(eager.windows).float().contiguous()

        def kernels_only():
            eager._reset()
            for _ in range(nb):
                ops.sw_gather(eager.volume, eager.origins, eager.first, BATCH, out=eager.windows)
                ops.sw_accumulate(fixed, eager.acc, eager.wsum, eager.origins, eager.first, eager.weights)
                eager.first.add_(BATCH)
            return ops.sw_finalize(eager.acc, eager.wsum)
        t_kern = timed(kernels_only)
        kprob = kernels_only()[0]
        origins = eager.origins.cpu().tolist()
        wt = eager.weights
        w3 = (wt[0].view(-1, 1, 1) * wt[1].view(1, -1, 1)) * wt[2].view(1, 1, -1)
        acc_t, wsum_t = torch.zeros_like(eager.acc), torch.zeros_like(eager.wsum)
        t_torch = timed(lambda: torch_blend(eager.volume, origins, w3, fixed, patch, acc_t, wsum_t))
        diff = float((torch_blend(eager.volume, origins, w3, fixed, patch, acc_t, wsum_t)[0] - kprob).abs().max())

        pv = patch ** 3
        launches = {
            "sw_gather_kernel": (lambda: ops.sw_gather(eager.volume, eager.origins, eager.first, BATCH, out=eager.windows), BATCH * 1 * pv * 4 * 2),
            "sw_accumulate_kernel": (lambda: ops.sw_accumulate(fixed, eager.acc, eager.wsum, eager.origins, eager.first, eager.weights), BATCH * pv * 4 * (3 * k + 2)),
            "sw_finalize_kernel": (lambda: ops.sw_finalize(eager.acc, eager.wsum), voxels * (4 * (2 * k + 1) + 1)),
        }
        eager.first.zero_()
        kernels = {}
        for name, (fn, nbytes) in launches.items():
            t = timed(lambda: [fn() for _ in range(KERNEL_LAUNCHES)], reps=REPS, warmup=1)
            us = t["median"] * 1e3 / KERNEL_LAUNCHES
            rate = nbytes / (us * 1e-6)
            kernels[name] = {"us_per_launch": us, "bytes": nbytes, "bytes_per_s": rate, "share_of_copy_ceiling": rate / COPY_CEILING}
        cases[str(patch)] = {"windows": nw, "batches": nb, "classes": k, "eager_ms": t_eager, "graph_ms": t_graph, "graph_equals_eager": bool(same),
                             "network_ms": t_net, "kernels_ms": t_kern, "torch_blend_ms": t_torch, "torch_blend_max_abs_diff": diff,
                             "kernels": kernels}
        print("patch %d: %d windows, eager %.1f ms, graph %.1f ms (same bits: %s), network %.1f ms, kernels %.2f ms, torch blend %.2f ms"
              % (patch, nw, t_eager["median"], t_graph["median"], same, t_net["median"], t_kern["median"], t_torch["median"]), flush=True)
        del eager, graphed
    result = {"what": "evaluation.SlidingWindow on a %dx%dx%d volume, overlap %g, %s blend, batch %d, bf16 Segmentation(1, 2); milliseconds, median of %d "
                      "repetitions after %d warm-up calls, device events" % (SHAPE + (OVERLAP, BLEND, BATCH, REPS, WARMUP)),
              "device": torch.cuda.get_device_name(0), "copy_ceiling_bytes_per_s": COPY_CEILING, "kernel_launches_per_timing": KERNEL_LAUNCHES,
              "note": "us_per_launch is the time of back-to-back launches on one stream divided by their number: it holds the launch gap as well as the kernel, and the launches "
                      "re-read what the one before left in the 256 MiB last-level cache (a rate above the HBM copy ceiling says so)",
              "cases": cases}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
