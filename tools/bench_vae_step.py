"""The vae_train step launched eagerly with torch.randn against the same step captured with an ops.LatentStream -> profiles/vae_graph_bench.json.

The step of `main_source.py -M vae_train` (VAE(dim=128), SGD momentum 0.9, (1 - Dice) + 2e-5 KL at scale 0.35), batch 2, bf16 storage, spatial 128 (the
reference's VAE) and 64, in ONE process on ONE machine, two model copies with the same weights:
  eager_ms   --latent_noise torch, today's entry-point path: gradients dropped, vae_train_losses(noise=None) -> torch.randn, backward, optimiser step, all
             issued eagerly
  graph_ms   --latent_noise philox: train.GraphedStep(vae_train_losses(noise=LatentStream)).step()
Each sample is a host clock around ONE step that ends in a device synchronise; the two variants alternate sample by sample, STEPS samples of each after
WARMUP untimed steps of each; medians (and the extremes) are recorded.
  launches_per_step   what the host issues per step.  eager: the C-ABI calls of libvaeseg.so that launch (prototypes ending in `void* stream`; a few
                      launch more than one kernel), counted in one untimed step — torch's own launches (randn, the loss arithmetic, autograd's
                      accumulations) come on top and are not counted.  graph: one graph launch plus the library calls issued around it, counted the same way
  noise_equals_oracle the stream advanced by exactly one draw per step, and ops.latent_normal of the first and the last timed draw is the numpy oracle's
                      sample (tests/latent_util.py) within 2^-22 max(1, |value|)
No time or ratio is fixed in advance; the file records what was measured.

    python tools/bench_vae_step.py [--out profiles/vae_graph_bench.json] [--sides 128 64]
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

SIDES, BATCH, STEPS, WARMUP = (128, 64), 2, 20, 5
SEED = 700                                  # what driver.run gives rank 0's stream


def launching_entry_points():
    """the names of include/vaeseg.h whose last parameter is `void* stream`"""
    from vae_segmentation_amd import _lib
    src = re.sub(r"/\*.*?\*/", " ", open(_lib.HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return {m.group(1) for m in re.finditer(r"\b(vs_\w+)\s*\(([^)]*)\)\s*;", src) if re.search(r"void\s*\*\s*stream\s*$", m.group(2).strip())}


class LibraryCalls:
    """with LibraryCalls() as c: ...  — c.n = the launching C-ABI calls made inside the block (a counting wrapper around the binding's attribute lookup)"""

    def __enter__(self):
        from vae_segmentation_amd import _lib
        self.n, self._cls, self._orig = 0, _lib._Lib, _lib._Lib.__getattr__
        names, orig, me = launching_entry_points(), self._orig, self

        def lookup(obj, name):
            fn = orig(obj, name)
            if name not in names:
                return fn

            def call(*a):
                me.n += 1
                return fn(*a)
            return call
        self._cls.__getattr__ = lookup
        return self

    def __exit__(self, *exc):
        self._cls.__getattr__ = self._orig
        return False


def timed_step(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vae_graph_bench.json"))
    ap.add_argument("--sides", type=int, nargs="+", default=list(SIDES))
    args = ap.parse_args()
    import torch
    import joint_model as M
    from oracle import ref_cpu as O
    from tests import latent_util as LU
    from vae_segmentation_amd import ops, optim
    from vae_segmentation_amd import train as T
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_step.py measures on the GPU; there is none here")
    cases = {}
    result = {"what": "one vae_train step (VAE dim 128, SGD momentum 0.9, batch %d, bf16): eager with torch.randn (the entry point's default path) vs "
                      "train.GraphedStep with an ops.LatentStream; host clock around one step ending in a synchronise, the variants alternating, "
                      "medians of %d after %d warm-up steps; same process" % (BATCH, STEPS, WARMUP),
              "device": torch.cuda.get_device_name(0), "deterministic_build": bool(ops.is_deterministic()), "batch": BATCH, "dtype": "bf16",
              "steps": STEPS, "warmup": WARMUP, "cases": cases}
    for side in args.sides:
        lab = O.synthetic_label(BATCH, side, 3).cuda()

        def build():
            vae = O.deterministic_fill_(M.VAE(2, 2, norm_type=1, dim=128, spatial=side), seed=0).cuda()
            return M.set_kernel_dtype(vae, torch.bfloat16)

        va, vb = build(), build()
        opt_a = optim.SGD(va.parameters(), lr=1e-2, momentum=0.9)
        opt_b = optim.SGD(vb.parameters(), lr=1e-2, momentum=0.9)
        stream = ops.LatentStream(SEED)
        gs = T.GraphedStep(lambda: T.vae_train_losses(va, lab, scale=0.35, noise=stream), list(va.parameters()), opt_a, warmup=1)

        def eager_step():
            for p in vb.parameters():
                p.grad = None
            loss, _ = T.vae_train_losses(vb, lab, scale=0.35)
            loss.backward()
            opt_b.step()

        for _ in range(WARMUP):
            eager_step()
            gs.step()
        torch.cuda.synchronize()
        with LibraryCalls() as c_eager:
            eager_step()
        with LibraryCalls() as c_graph:
            gs.step()
        torch.cuda.synchronize()
        first = stream.state()
        e_ms, g_ms = [], []
        for _ in range(STEPS):
            e_ms.append(timed_step(eager_step))
            g_ms.append(timed_step(gs.step))
        last = stream.state()
        ok = first[0] == SEED and last == (SEED, first[1] + STEPS)
        for t in (first[1], last[1] - 1):
            want = LU.ref_latent_normal((BATCH, 128), SEED, t).astype(np.float64)
            got = ops.latent_normal((BATCH, 128), SEED, t).cpu().numpy().astype(np.float64)
            ok = ok and bool((np.abs(got - want) <= 2.0 ** -22 * np.maximum(1.0, np.abs(want))).all())
        rec = {"side": side, "eager_ms": statistics.median(e_ms), "eager_ms_min": min(e_ms), "eager_ms_max": max(e_ms),
               "graph_ms": statistics.median(g_ms), "graph_ms_min": min(g_ms), "graph_ms_max": max(g_ms),
               "launches_per_step": {"eager_library_calls": c_eager.n, "eager_torch_launches": "not counted",
                                     "graph_launches": 1, "graph_library_calls_around_it": c_graph.n},
               "tail_captured": bool(gs.tail), "draws": [first[1], last[1]], "noise_equals_oracle": bool(ok),
               "loss_eager": float(T.vae_train_losses(vb, lab, scale=0.35)[0].item()), "loss_graph": float(gs.loss.item())}
        rec["ratio_eager_over_graph"] = rec["eager_ms"] / rec["graph_ms"]
        cases[str(side)] = rec
        print("side %3d  eager %.3f ms (%.3f .. %.3f)  graph %.3f ms (%.3f .. %.3f)  ratio %.2f  library calls %d -> 1 graph launch + %d  noise ok %s"
              % (side, rec["eager_ms"], rec["eager_ms_min"], rec["eager_ms_max"], rec["graph_ms"], rec["graph_ms_min"], rec["graph_ms_max"],
                 rec["ratio_eager_over_graph"], c_eager.n, c_graph.n, ok), flush=True)
        with open(args.out, "w") as f:                       # kept current: a run that is cut short leaves what it measured
            json.dump(result, f, indent=1)
        del gs
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
