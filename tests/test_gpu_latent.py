"""GPU: the VAE's latent noise drawn on the device (include/vaeseg.h "VAE latent": vs_latent_normal_philox, vs_reparam_philox_fwd, vs_latent_advance;
ops.latent_normal / LatentStream / ReparamPhilox; VAE.forward(noise=LatentStream); --latent_noise philox) against tests/latent_util.py: the stated
Philox stream, its semantics eagerly and under graph replay, the captured vae_train step against the eager one, and the entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import latent_util as LU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEEDS = (0x9E3779B97F4A7C15, 2 ** 40 + 3)              # bits in both halves; the first has bit 63 set
DRAWS = (0, 1, 2 ** 32 + 5)


@pytest.mark.parametrize("shape", [(1, 2), (2, 128), (3, 1025), (4, 1024)])
def test_latent_normal_matches_the_oracle(shape):
    """|got - want| <= 2^-22 max(1, |want|): one fp32 rounding is 2^-24 |want|; the device's fp64 log / sqrt / sin / cos are a few fp64 ulp off numpy's,
    so only a value next to a rounding tie can land on the neighbouring float — one more ulp, 2^-23 |want| at the most."""
    from vae_segmentation_amd import ops
    worst = 0.0
    for seed in SEEDS:
        for draw in DRAWS:
            got = ops.latent_normal(shape, seed, draw)
            assert got.dtype == torch.float32 and tuple(got.shape) == shape and got.is_cuda
            want = LU.ref_latent_normal(shape, seed, draw).astype(np.float64)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
            worst = max(worst, float(err.max()))
            assert err.max() <= 2.0 ** -22, (seed, draw, float(err.max()))
    print("worst |got - want| / max(1, |want|) = %.3e (bound %.3e)" % (worst, 2.0 ** -22))


def test_stream_semantics_eager():
    """three draws of one stream are draws 0, 1, 2 of its seed, the counter ends at 3, and z and both gradients have ops.Reparam's bits for that noise"""
    from vae_segmentation_amd import ops
    seed, shape, scale = SEEDS[0], (3, 1025), 0.35
    g = torch.Generator().manual_seed(3)
    stream = ops.LatentStream(seed)
    assert stream.state() == (seed, 0)
    for t in range(3):
        mean = torch.randn(shape, generator=g).cuda().requires_grad_()
        std = (torch.rand(shape, generator=g) + 0.1).cuda().requires_grad_()
        gz = torch.randn(shape, generator=g).cuda()
        z, noise = ops.ReparamPhilox.apply(mean, std, stream, scale)
        assert torch.equal(noise, ops.latent_normal(shape, seed, t)) and not noise.requires_grad
        z.backward(gz)
        m2, s2 = mean.detach().clone().requires_grad_(), std.detach().clone().requires_grad_()
        z2 = ops.Reparam.apply(m2, s2, noise, scale)
        z2.backward(gz)
        assert torch.equal(z.detach(), z2.detach())
        assert torch.equal(mean.grad, m2.grad) and torch.equal(std.grad, s2.grad)
    assert stream.state() == (seed, 3)
    stream.set(SEEDS[1], 2 ** 32 + 5)                                      # the high word of the draw reaches the kernel through device memory
    assert stream.state() == (SEEDS[1], 2 ** 32 + 5)
    mean, std = torch.zeros(shape, device="cuda"), torch.ones(shape, device="cuda")
    z, noise = ops.ReparamPhilox.apply(mean, std, stream, 1.0)
    assert torch.equal(noise, ops.latent_normal(shape, SEEDS[1], 2 ** 32 + 5)) and torch.equal(z, noise)
    assert stream.state() == (SEEDS[1], 2 ** 32 + 6)


def test_captured_forward_draws_afresh_on_every_replay():
    """a captured ReparamPhilox forward, replayed three times: three different samples, the ones an eager stream draws from the same state"""
    from vae_segmentation_amd import ops
    seed, shape, scale = SEEDS[1], (2, 129), 0.5
    g = torch.Generator().manual_seed(4)
    mean, std = torch.randn(shape, generator=g).cuda(), (torch.rand(shape, generator=g) + 0.1).cuda()
    stream = ops.LatentStream(seed, 2 ** 32 - 2)                           # the replays carry the counter across 2^32
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ReparamPhilox.apply(mean, std, stream, scale)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # succeeds: nothing in the two launches synchronises or allocates outside torch
        z, noise = ops.ReparamPhilox.apply(mean, std, stream, scale)
    before = stream.state()
    assert before == (seed, 2 ** 32 - 1)                                   # the warm-up drew once; the capture itself ran nothing
    got = []
    for _ in range(3):
        graph.replay()
        got.append((noise.clone(), z.clone()))
    torch.cuda.synchronize()
    assert stream.state() == (seed, before[1] + 3)
    for a in range(3):
        for b in range(a + 1, 3):
            assert not torch.equal(got[a][0], got[b][0])
    twin = ops.LatentStream(1)
    twin.set(*before)
    for n_replayed, z_replayed in got:
        z2, n2 = ops.ReparamPhilox.apply(mean, std, twin, scale)
        assert torch.equal(n_replayed, n2) and torch.equal(z_replayed, z2)
    assert twin.state() == stream.state()


def test_vae_train_step_captured_with_a_stream_matches_eager():
    """three GraphedStep replays of vae_train_losses(noise=LatentStream) against three eager steps from the same stream state: bit-equal losses and
    weights (tests/test_gpu_optim.py's comparison of captured and eager steps), and exactly one draw per step"""
    import joint_model as M
    from oracle import ref_cpu as O
    from vae_segmentation_amd import ops, optim
    from vae_segmentation_amd import train as T
    assert ops.is_deterministic()
    lab = O.synthetic_label(1, 64, 3).cuda()

    def build():
        return O.deterministic_fill_(M.VAE(2, 2, norm_type=1, dim=128, spatial=64), seed=0).cuda()

    va, vb = build(), build()
    for p, q in zip(va.parameters(), vb.parameters()):
        assert torch.equal(p, q)
    sa = ops.LatentStream(SEEDS[0])
    opt_a = optim.SGD(va.parameters(), lr=1e-2, momentum=0.9)
    gs = T.GraphedStep(lambda: T.vae_train_losses(va, lab, noise=sa), list(va.parameters()), opt_a, warmup=1)
    start = sa.state()                                                      # the warm-up consumed draws: read, not assumed
    assert start[0] == SEEDS[0] and start[1] >= 1
    captured = [gs.step().item() for _ in range(3)]
    assert sa.state() == (SEEDS[0], start[1] + 3)
    sb = ops.LatentStream(0)
    sb.set(*start)
    opt_b = optim.SGD(vb.parameters(), lr=1e-2, momentum=0.9)
    eager = []
    for _ in range(3):
        opt_b.zero_grad()
        loss, _ = T.vae_train_losses(vb, lab, noise=sb)
        loss.backward()
        opt_b.step()
        eager.append(loss.item())
    torch.cuda.synchronize()
    assert sb.state() == sa.state()
    print("captured", captured, "eager", eager)
    assert captured == eager and len(set(captured)) == 3
    for (n, p), q in zip(va.named_parameters(), vb.parameters()):
        assert torch.equal(p.detach(), q.detach()), n


def _run(args, cwd):
    out = subprocess.run([sys.executable] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


CAPTURED = "train step captured as a HIP graph"


def test_entry_point_vae_train_is_captured_with_philox_noise(tmp_path):
    cmd = [os.path.join(REPO, "main_source.py"), "vae", "-M", "vae_train", "--size", "64", "-b", "1", "-E", "1", "--max_iters", "2",
           "--synthetic_train", "2", "--synthetic_val", "1"]
    out = _run(cmd + ["--latent_noise", "philox"], str(tmp_path))
    assert CAPTURED in out and "Finished Training" in out and "graph replay" in out
    out = _run(cmd, str(tmp_path))                                         # without the flag: as before, eager
    assert CAPTURED not in out and "Finished Training" in out and "(eager)" in out


def test_entry_point_embed_train_recaptures_when_the_encoder_thaws(tmp_path):
    """two epochs: the Encoder's requires_grad flips once (main_source.py:550-554) and the step is captured again"""
    cmd = [os.path.join(REPO, "main_source.py"), "emb", "-M", "embed_train", "--size", "64", "-b", "1", "-E", "2", "--eval_epoch", "1", "--save_epoch", "50",
           "--max_iters", "2", "--synthetic_train", "2", "--synthetic_val", "1"]
    out = _run(cmd + ["--latent_noise", "philox"], str(tmp_path))
    assert out.count(CAPTURED) == 2 and "Finished Training" in out and out.count("graph replay") == 2
    out = _run(cmd, str(tmp_path))
    assert CAPTURED not in out and "Finished Training" in out and out.count("(eager)") == 2


@pytest.mark.parametrize("extra", [[], ["--adam"]], ids=["sgd", "adam"])
def test_entry_point_embed_train_frozen_encoder_does_not_move(tmp_path, extra):
    """three epochs: the Encoder trains in epoch 1 and is frozen again in epoch 2, where the gradient its last trained step left must not reach the
    optimiser (whose tail is eager for this model, and always with Adam) — its weights in the checkpoints after epochs 1 and 2 are equal, and they
    did move in epoch 1"""
    cmd = [os.path.join(REPO, "main_source.py"), "emb3", "-M", "embed_train", "--size", "64", "-b", "1", "-E", "3", "--eval_epoch", "1", "--save_epoch", "1",
           "--max_iters", "2", "--synthetic_train", "2", "--synthetic_val", "1", "--latent_noise", "philox"] + extra
    out = _run(cmd, str(tmp_path))
    assert out.count(CAPTURED) == 3 and "Finished Training" in out
    sd = [torch.load(str(tmp_path / "3dmodel" / "emb3" / ("model_epoch%d.ckpt" % e)), map_location="cpu")["model_state_dict"] for e in (1, 2, 3)]
    enc = [k for k in sd[0] if k.startswith("Encoder.") and sd[0][k].dtype.is_floating_point]
    fus = [k for k in sd[0] if k.startswith("Fusion.") and sd[0][k].dtype.is_floating_point]
    assert enc and fus
    assert any(not torch.equal(sd[0][k], sd[1][k]) for k in enc)             # epoch 1 (odd): the Encoder trains
    moved = [k for k in enc if not torch.equal(sd[1][k], sd[2][k])]
    assert not moved, moved[:5]                                              # epoch 2 (even): frozen, bit for bit
    assert any(not torch.equal(sd[1][k], sd[2][k]) for k in fus)             # while the Fusion network goes on training
