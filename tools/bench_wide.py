"""Wide-VAE step time: vae_train of VAE(2, 2, norm_type=1, dim=128, n_fmaps=[16, 32, 64, 128, 256, 512]) at 128^3, batch 2, bf16 storage,
one captured graph per step (train.GraphedStep).  Prints one JSON line.

    python tools/bench_wide.py --steps 20 --warmup 3
    rocprofv3 --kernel-trace --stats -d DIR -o wide -- python tools/bench_wide.py --steps 5 --warmup 2    (the per-kernel table; a separate run)
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

WIDE_VAE = [16, 32, 64, 128, 256, 512]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    a = ap.parse_args()
    import joint_model as M
    from oracle import ref_cpu as O
    from vae_segmentation_amd import optim
    from vae_segmentation_amd import train as T

    torch.cuda.set_device(0)
    vae = O.deterministic_fill_(M.VAE(2, 2, norm_type=1, dim=128, n_fmaps=WIDE_VAE, spatial=a.side), seed=0)
    vae = M.set_kernel_dtype(vae.cuda(), torch.bfloat16)
    lab = O.synthetic_label(a.batch, a.side, 3).cuda()
    noise = (2 * torch.from_numpy(O.hashed_uniform(a.batch * 128, 7100, 5)) - 1).view(a.batch, 128).float().cuda()
    opt = optim.SGD(vae.parameters(), lr=1e-4, momentum=0.9)
    gs = T.GraphedStep(lambda: T.vae_train_losses(vae, lab, scale=0.35, noise=noise), vae.parameters(), opt, warmup=1)
    for _ in range(a.warmup):
        loss = gs.step()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = gs.step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    params = sum(p.numel() for p in vae.parameters())
    print(json.dumps({"workload": "vae_train wide n_fmaps=%s" % WIDE_VAE, "side": a.side, "batch": a.batch, "dtype": "bf16",
                      "steps": a.steps, "step_ms_median": times[len(times) // 2], "step_ms_min": times[0], "step_ms_max": times[-1],
                      "loss": float(loss.item()), "params": params}))


if __name__ == "__main__":
    main()
