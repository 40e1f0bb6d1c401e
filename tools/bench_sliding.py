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

With --tta AXES (a string over "dhw") the same configuration is run with mirror test-time augmentation inside the kernels -> profiles/sliding_tta_bench.json.
Per window size, again in one process:
  graph_ms             SlidingWindow(graph=True, tta=AXES): nw * nf items, one capture (compared bit for bit with one eager call)
  plain_graph_ms       the same object without tta, for scale
  naive_ms             what a user writes without it: nf plain graphed passes, model_fn wrapped in torch.flip in and out, and the mean of the nf
                       probability volumes; and the largest difference of that mean from the in-kernel result
  kernels_ms           gather + accumulate per item and one finalize alone, mirrored (tta) and un-mirrored (plain, per window), and both divided by
                       their number of items: the share the comparison is about
  kernels              microseconds per launch of the mirrored gather and accumulate with the counter parked on an item of a given flip code, beside
                       the plain kernels, measured the same way

    python tools/bench_sliding.py --tta dhw [--out profiles/sliding_tta_bench.json]
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


def main_tta(args):
    import torch
    import joint_model as M
    from vae_segmentation_amd import evaluation, ops
    from vae_segmentation_amd.modules import set_kernel_dtype
    if not torch.cuda.is_available():
        raise SystemExit("bench_sliding.py measures on the GPU; there is none here")
    flips = evaluation.tta_flips(args.tta)
    if not flips or not isinstance(args.tta, str):
        raise SystemExit("--tta takes a non-empty string over \"dhw\"")
    nf = len(flips)
    torch.manual_seed(0)
    seg = M.Segmentation(n_channels=1, n_class=2, norm_type=1).cuda().eval()
    set_kernel_dtype(seg, torch.bfloat16)
    model_fn = evaluation.segmentation_model_fn(seg)
    vol = torch.randn((1,) + SHAPE, device="cuda")

    def flipped(code):
        dims = tuple(4 - bit for bit in range(3) if code >> bit & 1)
        return (lambda b: torch.flip(model_fn(torch.flip(b, dims)), dims)) if dims else model_fn
    cases = {}
    for patch in PATCHES:
        kw = dict(overlap=OVERLAP, blend=BLEND, batch=BATCH)
        tta = evaluation.SlidingWindow(model_fn, vol.shape, patch, graph=True, tta=flips, **kw)
        plain = evaluation.SlidingWindow(model_fn, vol.shape, patch, graph=True, **kw)
        ref = evaluation.SlidingWindow(model_fn, vol.shape, patch, tta=flips, **kw)(vol)
        got = tta(vol)
        same = torch.equal(got["prob"].view(torch.int32), ref["prob"].view(torch.int32)) and torch.equal(got["wsum"], ref["wsum"])
        prob_tta = got["prob"].clone()
        del ref, got
        plain(vol)
        t_tta, t_plain = timed(lambda: tta(vol)), timed(lambda: plain(vol))
        naive = [evaluation.SlidingWindow(flipped(c), vol.shape, patch, graph=True, **kw) for c in flips]
        naive_pass = lambda: torch.stack([sw(vol)["prob"] for sw in naive]).mean(0)
        diff = float((naive_pass() - prob_tta).abs().max())
        t_naive = timed(naive_pass)
        del naive
        with torch.no_grad():
            fixed = model_fn(tta.windows).float().contiguous()

        def kernels_only(sw, fl):
            sw._reset()
            for _ in range(sw.n_batches):
                ops.sw_gather(sw.volume, sw.origins, sw.first, BATCH, out=sw.windows, flips=fl)
                ops.sw_accumulate(fixed, sw.acc, sw.wsum, sw.origins, sw.first, sw.weights, flips=fl)
                sw.first.add_(BATCH)
            return ops.sw_finalize(sw.acc, sw.wsum)
        # alternating, so that a drift of the box touches both alike
        t_kt, t_kp = [], []
        for _ in range(3):
            t_kt.append(timed(lambda: kernels_only(tta, flips), reps=REPS // 2)["median"])
            t_kp.append(timed(lambda: kernels_only(plain, None), reps=REPS // 2)["median"])
        k_tta = {"median": statistics.median(t_kt), "min": min(t_kt), "max": max(t_kt)}
        k_plain = {"median": statistics.median(t_kp), "min": min(t_kp), "max": max(t_kp)}
        kernels = {}
        for name, fl, first in [("plain", None, 0)] + [("tta_code_%d" % c, flips, i) for i, c in enumerate(flips) if c in (0, 1, 2, 4, 7)]:
            plain.first.fill_(first)
            for kname, fn in (("sw_gather_kernel", lambda: ops.sw_gather(plain.volume, plain.origins, plain.first, BATCH, out=plain.windows, flips=fl)),
                              ("sw_accumulate_kernel", lambda: ops.sw_accumulate(fixed, plain.acc, plain.wsum, plain.origins, plain.first, plain.weights, flips=fl))):
                t = timed(lambda: [fn() for _ in range(KERNEL_LAUNCHES)], reps=REPS, warmup=1)
                kernels.setdefault(kname, {})[name] = t["median"] * 1e3 / KERNEL_LAUNCHES
        cases[str(patch)] = {"windows": tta.nw, "flips": list(flips), "items": tta.n_items, "batches": tta.n_batches, "graph_ms": t_tta, "graph_equals_eager": bool(same),
                             "plain_graph_ms": t_plain, "graph_ms_over_plain": t_tta["median"] / t_plain["median"],
                             "naive_ms": t_naive, "naive_over_tta": t_naive["median"] / t_tta["median"], "naive_max_abs_diff": diff,
                             "kernels_ms": {"tta": k_tta, "plain": k_plain},
                             "kernels_us_per_item": {"tta": k_tta["median"] * 1e3 / tta.n_items, "plain": k_plain["median"] * 1e3 / plain.n_items},
                             "kernels_share_of_graph_ms": k_tta["median"] / t_tta["median"],
                             "kernel_us_per_launch": kernels}
        print("patch %d: %d items, tta graph %.1f ms (same bits as eager: %s), plain graph %.1f ms, naive %.1f ms (x%.2f, max diff %.3g), kernels per item %.2f us "
              "mirrored / %.2f us plain" % (patch, tta.n_items, t_tta["median"], same, t_plain["median"], t_naive["median"], t_naive["median"] / t_tta["median"], diff,
                                            k_tta["median"] * 1e3 / tta.n_items, k_plain["median"] * 1e3 / plain.n_items), flush=True)
        del tta, plain
    result = {"what": "evaluation.SlidingWindow(tta=%r) on a %dx%dx%d volume, overlap %g, %s blend, batch %d, bf16 Segmentation(1, 2), graph replay; milliseconds, "
                      "median of %d repetitions after %d warm-up calls, device events" % ((args.tta,) + SHAPE + (OVERLAP, BLEND, BATCH, REPS, WARMUP)),
              "device": torch.cuda.get_device_name(0), "kernel_launches_per_timing": KERNEL_LAUNCHES,
              "note": "kernels_ms: gather + accumulate per item and one finalize, the network's answer a fixed tensor; three alternating rounds of the mirrored and the "
                      "plain loop, median / min / max of the rounds' medians.  kernel_us_per_launch: back-to-back launches with the item counter parked on an item of "
                      "the named flip code (bit 0 mirrors x); it holds the launch gap and re-reads the last-level cache, as in sliding_bench.json",
              "cases": cases}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote %s" % args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tta", default=None, metavar="AXES", help="measure mirror test-time augmentation over these axes (a string over \"dhw\") instead")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "sliding_tta_bench.json" if args.tta else "sliding_bench.json")
    if args.tta:
        return main_tta(args)
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
