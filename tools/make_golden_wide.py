"""Reference goldens of the wide models (n_fmaps up to 512 channels) -> tests/golden/wide.npz.

The reference's own modules (joint_model.py), unmodified, in fp32 and fp64 on the CPU, through the helpers of oracle/make_golden.py:
  wide_vae64/    vae_train step of VAE(2, 2, norm_type=1, dim=128, n_fmaps=[16, 32, 64, 128, 256, 512]) at 64^3, batch 2, injected noise;
                 the reference VAE hard-codes Linear(16384, dim) / view(256, 4, 4, 4), so its blocks are composed around fc layers of width
                 512 * side^3 (make_golden.composed_vae with the top width of n_fmaps)
  wide_seg32/    seg_train step of Segmentation(1, 2, norm_type=1, n_fmaps=[32, 64, 128, 256, 512, 512]) at 32^3, batch 2 (512-channel 2^3 bottleneck)
  wide_joint64/  joint_train step (frozen VAE) of the default Segmentation and the wide VAE at 64^3, batch 2
  fc/            the fc weight shapes of the wide VAE at 64^3 and 128^3 and of the wide Encoder at 128^3 (tests/test_gpu_wide.py state_dict check)

    python tools/make_golden_wide.py
"""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import make_golden as MG  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

WIDE_VAE = [16, 32, 64, 128, 256, 512]
WIDE_SEG = [32, 64, 128, 256, 512, 512]


def composed_wide_vae(ref_vae, side, top):
    """make_golden.composed_vae with the bottleneck width `top` (n_fmaps[5]) in place of 256."""
    flat = top * side ** 3
    dim = ref_vae.fc_mean.out_features
    ref_vae.fc_mean = torch.nn.Linear(flat, dim)
    ref_vae.fc_std = torch.nn.Linear(flat, dim)
    ref_vae.fc2 = torch.nn.Linear(dim, flat)

    def fwd(x, if_random=False, scale=1, noise=None):
        v = ref_vae
        x = v.down5(v.down4(v.down3(v.down2(v.down1(v.in_block(x))))))
        x = x.view(x.size(0), flat)
        mean = v.fc_mean(x)
        std = torch.relu(v.fc_std(x))
        z = mean + noise * std * scale if if_random else mean
        x = v.fc2(z).view(x.size(0), top, side, side, side)
        x = v.up5(v.up4(v.up3(v.up2(v.up1(x)))))
        return v.final(v.out_block(x)), mean, std
    return fwd


def _wide_vae64(dt):
    d = {}
    vae = MG.RM.VAE(n_channels=2, n_class=2, norm_type=1, dim=128, n_fmaps=WIDE_VAE)
    fwd = composed_wide_vae(vae, 2, WIDE_VAE[5])
    O.deterministic_fill_(vae, seed=0)
    vae.to(dt)
    gt = O.one_hot(O.synthetic_label(2, 64, seed=3)).to(dt)
    noise = torch.from_numpy(2 * O.hashed_uniform(2 * 128, 7100, 5) - 1).view(2, 128).to(dt)
    recon, mean, std = fwd(gt, if_random=True, scale=0.35, noise=noise)
    b = {"recon": recon, "gt": gt, "mean": mean, "std": std}
    kl = MG.REV.KLloss(b)
    dsc = 1 - MG.main_source_avg_dsc(recon, gt, 1, 2)
    final = dsc + 0.00002 * kl
    final.backward()
    d["kl"], d["dice_loss"], d["final"] = kl.detach().numpy(), dsc.detach().numpy(), final.detach().numpy()
    d["mean"], d["std"] = mean.detach().numpy(), std.detach().numpy()
    MG.put(d, "recon", recon, 256)
    MG.put_grads(d, "vae", vae)
    return d


def _wide_seg32(dt):
    d = {}
    seg = MG.RM.Segmentation(n_channels=1, n_class=2, norm_type=1, n_fmaps=WIDE_SEG)
    O.deterministic_fill_(seg, seed=0)
    seg = seg.to(dt)
    img, lab = O.synthetic_image(2, 32, seed=2).to(dt), O.synthetic_label(2, 32, seed=3)
    batch = {"img": img, "gt": O.one_hot(lab).to(dt)}
    batch = seg(batch, "img", "pred")
    dsc = 1 - MG.REV.avg_dsc(batch, "pred", "gt", botindex=1, topindex=2)
    dsc.backward()
    d["dice_loss_eps1e6"] = dsc.detach().numpy()
    MG.put(d, "pred", batch["pred"], 256)
    MG.put_grads(d, "seg", seg)
    return d


def _wide_joint64(dt):
    d = {}
    seg = MG.RM.Segmentation(n_channels=1, n_class=2, norm_type=1)
    vae = MG.RM.VAE(n_channels=2, n_class=2, norm_type=1, dim=128, n_fmaps=WIDE_VAE)
    joint = MG.RM.Joint(models=[seg, vae])
    fwd = composed_wide_vae(vae, 2, WIDE_VAE[5])
    O.deterministic_fill_(joint, seed=0)
    joint.to(dt)
    for p in joint.Vae.parameters():
        p.requires_grad = False
    joint.Vae.eval()
    img, lab = O.synthetic_image(2, 64, seed=2).to(dt), O.synthetic_label(2, 64, seed=3)
    batch = {"img": img, "gt": O.one_hot(lab).to(dt)}
    batch = joint.Seg(batch, "img", "pred")
    batch["recon"], batch["mean"], batch["std"] = fwd(batch["pred"])
    recon_loss = 1 - MG.main_source_avg_dsc(batch["pred"], batch["recon"], 1, 2)
    dsc_loss = 1 - MG.main_source_avg_dsc(batch["pred"], batch["gt"], 1, 2)
    final = 0.1 * recon_loss + dsc_loss
    final.backward()
    d["recon_loss"], d["dice_loss"], d["final"] = recon_loss.detach().numpy(), dsc_loss.detach().numpy(), final.detach().numpy()
    d["mean"], d["std"] = batch["mean"].detach().numpy(), batch["std"].detach().numpy()
    MG.put(d, "pred", batch["pred"], 512)
    MG.put(d, "recon", batch["recon"], 512)
    MG.put_grads(d, "seg", joint.Seg)
    return d


def _fc_shapes():
    d = {}
    for side in (64, 128):
        vae = MG.RM.VAE(n_channels=2, n_class=2, norm_type=1, dim=128, n_fmaps=WIDE_VAE)
        composed_wide_vae(vae, side // 32, WIDE_VAE[5])
        for name, p in vae.named_parameters():
            if name.startswith("fc"):
                d["fc/vae%d/%s" % (side, name)] = np.asarray(p.shape, dtype=np.int64)
    enc = MG.RM.Encoder(n_channels=2, dim=128, norm_type=1, n_fmaps=WIDE_VAE)
    enc.fc1 = torch.nn.Linear(WIDE_VAE[5] * 4 ** 3, 1024)          # the reference hard-codes 16384 (256 * 4^3) here as in the VAE
    for name, p in enc.named_parameters():
        if name.startswith("fc"):
            d["fc/enc128/%s" % name] = np.asarray(p.shape, dtype=np.int64)
    return d


def main():
    d = {}
    for tag, fn in (("wide_vae64", _wide_vae64), ("wide_seg32", _wide_seg32), ("wide_joint64", _wide_joint64)):
        t0 = time.time()
        for k, v in MG.both_precisions(fn).items():
            d[tag + "/" + k] = v
        print("  %s %.1fs" % (tag, time.time() - t0))
    d.update(_fc_shapes())
    MG.save("wide", d)


if __name__ == "__main__":
    main()
