"""A patch-space prediction pasted back onto the scan grid (vs_uncrop) against the host detour it replaces -> profiles/uncrop_bench.json.

Scan 256 x 256 x 192, K = 2 classes, patches of 96 and 128, a box whose crop cube has side 150 (the patch is a downsampled crop) and one of side 60
(upsampled).  Per combination, in ONE process on ONE machine:
  device_ms        one ops.uncrop(interp="linear") — one vs_uncrop launch writing the uint8 label — between two device events, the median of REPS runs
                   after WARMUP; device_prob_ms: the same with the fp32 probabilities (K, D, H, W) written as well
  us_per_launch    back-to-back launches between two events divided by their number, the bytes a launch has to move (from the shapes: the patch read
                   once, every output written once) and the rate that makes, beside the copy rate the project uses as its practical ceiling
  host_ms          the same result through .cpu() -> scipy.ndimage.zoom per class (order 1, mode 'nearest', grid_mode) -> numpy paste and argmax ->
                   .cuda(), wall clock around the whole detour with the device idle before and after; and how many labels differ from the device's
  finalize         vs_sw_finalize on a volume of the same size and K, measured the same way: the project's other launch that writes a uint8 label
                   per voxel (it reads K + 1 and writes K fp32 planes besides)

    python tools/bench_uncrop.py [--out profiles/uncrop_bench.json]
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

SHAPE = (256, 256, 192)
K = 2
PATCHES = (96, 128)
BOXES = {"side150_downsampled": ((60, 60, 30), (186, 180, 150)), "side60_upsampled": ((100, 100, 70), (150, 140, 110))}
REPS, WARMUP, KERNEL_LAUNCHES, HOST_REPS = 20, 3, 50, 3
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


def per_launch(fn, nbytes):
    t = timed(lambda: [fn() for _ in range(KERNEL_LAUNCHES)], reps=REPS, warmup=1)
    us = t["median"] * 1e3 / KERNEL_LAUNCHES
    rate = nbytes / (us * 1e-6)
    return {"us_per_launch": us, "bytes": nbytes, "bytes_per_s": rate, "share_of_copy_ceiling": rate / COPY_CEILING}


def host_detour(prob, geometry, shape):
    """what a user writes without the kernel"""
    import numpy as np
    import torch
    from scipy import ndimage as ndi
    lo, hi, off, side = geometry
    p = prob.cpu().numpy()
    out = np.zeros((p.shape[0],) + tuple(shape), np.float32)
    out[0] = 1.0
    dst = tuple(slice(lo[d], hi[d]) for d in range(3))
    src = tuple(slice(off[d], off[d] + hi[d] - lo[d]) for d in range(3))
    for k in range(p.shape[0]):
        out[k][dst] = ndi.zoom(p[k], side / p.shape[1], order=1, mode="nearest", grid_mode=True)[src]
    return torch.from_numpy(out.argmax(0).astype(np.uint8)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "uncrop_bench.json"))
    args = ap.parse_args()
    import torch
    from vae_segmentation_amd import data_gpu, ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncrop.py measures on the GPU; there is none here")
    torch.manual_seed(0)
    voxels = SHAPE[0] * SHAPE[1] * SHAPE[2]
    acc, wsum = torch.rand((K,) + SHAPE, device="cuda"), torch.rand(SHAPE, device="cuda") + 0.5
    fin = {"ms": timed(lambda: ops.sw_finalize(acc, wsum)), **per_launch(lambda: ops.sw_finalize(acc, wsum), voxels * (4 * (2 * K + 1) + 1))}
    print("sw_finalize: %.1f us per launch, %.2f TB/s" % (fin["us_per_launch"], fin["bytes_per_s"] / 1e12), flush=True)
    del acc, wsum
    cases = {}
    for patch in PATCHES:
        prob = torch.softmax(torch.randn((K,) + (patch,) * 3, device="cuda") * 2.0, 0).contiguous()
        for name, box in BOXES.items():
            geometry = data_gpu.crop_geometry(box, SHAPE)
            label_only = lambda: ops.uncrop(prob, geometry, SHAPE, interp="linear")
            with_prob = lambda: ops.uncrop(prob, geometry, SHAPE, interp="linear", want_prob=True)
            rec = {"geometry": {"lo": geometry[0], "hi": geometry[1], "off": geometry[2], "side": geometry[3]},
                   "device_ms": timed(label_only), "device_prob_ms": timed(with_prob),
                   "label_only": per_launch(label_only, voxels + K * patch ** 3 * 4),
                   "label_and_prob": per_launch(with_prob, voxels * (1 + 4 * K) + K * patch ** 3 * 4)}
            got = label_only()["label"]
            torch.cuda.synchronize()
            host = []
            for _ in range(HOST_REPS):
                t0 = time.perf_counter()
                want = host_detour(prob, geometry, SHAPE)
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e3)
            rec["host_ms"] = {"median": statistics.median(host), "min": min(host), "max": max(host), "repetitions": HOST_REPS}
            rec["labels_differing_from_host"] = int((got != want).sum())
            rec["host_over_device"] = rec["host_ms"]["median"] / rec["device_ms"]["median"]
            rec["us_per_launch_over_sw_finalize"] = rec["label_only"]["us_per_launch"] / fin["us_per_launch"]
            cases["patch%d_%s" % (patch, name)] = rec
            print("patch %d, %s: device %.3f ms (%.1f us back to back, %.2f TB/s; with prob %.1f us, %.2f TB/s), host detour %.0f ms, %d labels differ"
                  % (patch, name, rec["device_ms"]["median"], rec["label_only"]["us_per_launch"], rec["label_only"]["bytes_per_s"] / 1e12,
                     rec["label_and_prob"]["us_per_launch"], rec["label_and_prob"]["bytes_per_s"] / 1e12, rec["host_ms"]["median"],
                     rec["labels_differing_from_host"]), flush=True)
    result = {"what": "ops.uncrop (one vs_uncrop launch, linear) onto a %dx%dx%d scan, K = %d; device events, median of %d runs after %d warm-up calls; the host "
                      "detour by wall clock, median of %d" % (SHAPE + (K, REPS, WARMUP, HOST_REPS)),
              "device": torch.cuda.get_device_name(0), "copy_ceiling_bytes_per_s": COPY_CEILING, "kernel_launches_per_timing": KERNEL_LAUNCHES,
              "note": "device_ms is ONE launch between two events and holds the events' own cost; us_per_launch is the time of back-to-back launches on one stream "
                      "divided by their number: it holds the launch gap as well as the kernel, and the launches re-read what the one before left in the last-level cache",
              "sw_finalize": fin, "cases": cases}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
