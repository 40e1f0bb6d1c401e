"""GPU: global gradient-norm clipping, Nesterov momentum and their captured form (vae_segmentation_amd/optim.py, csrc/optim.hip
vs_grad_sqnorm_multi / vs_grad_clip_finish / vs_sgd_step_*_multi / vs_adam_clip_multi) against the numpy oracle (tests/optim_util.py) and
torch.nn.utils.clip_grad_norm_ + torch.optim on the CPU.

Shapes: ragged chunks on both sides of the 4096-element chunk; one tensor of 300 * 4096 + 5 elements (301 partials: the finish kernel's 256 threads loop);
one tensor that starts one element into a larger buffer (not 16-byte aligned: dword loads next to the other tensors' vector loads).
Norm bound 2^-22 * norm: the squares are exact in fp64 and their fp64 sum over 1.5 M terms is off by < 2e-10 relative, the square root and the one
rounding to fp32 by 2^-24 each."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import optim_util as OU

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1,), (2,), (4095,), (4096,), (4097,), (3, 4100), (128, 64, 3, 3, 3), (300 * 4096 + 5,)]
N_VIEW = 3 * 4100                        # the misaligned tensor: as many elements as SHAPES[5], so the two can trade values
I_TWIN, I_VIEW = 5, len(SHAPES)
NORM_RTOL = 2.0 ** -22


def _tensors(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * scale for s in SHAPES] + [torch.randn(N_VIEW, generator=g) * scale]


def _to_gpu(ts):
    """cuda copies; the last one lives one element into a larger buffer"""
    out = [t.clone().cuda() for t in ts[:-1]]
    buf = torch.zeros(N_VIEW + 8, device="cuda")
    view = buf[1:1 + N_VIEW]
    view.copy_(ts[-1])
    assert view.data_ptr() % 16 == 4 and out[-1].data_ptr() % 16 == 0
    return out + [view]


def _params(ts):
    return [torch.nn.Parameter(t) for t in _to_gpu(ts)]


def _set_grads(params, ts):
    for p, g in zip(params, _to_gpu(ts)):
        p.grad = g


def _bits(t):
    return t.detach().reshape(-1).view(torch.int32)


def _norm_of(opt):
    return float(opt.grad_norm.item())


def test_grad_norm_one_group_two_groups_and_reproducible():
    from vae_segmentation_amd import optim
    grads = _tensors(7, 0.3)
    want = OU.global_norm([g.numpy() for g in grads])
    ps = _params(_tensors(1))
    one = optim.SGD(ps, lr=1e-2, momentum=0.9, max_norm=1e30)
    assert one.grad_norm is None
    _set_grads(ps, grads)
    one.step()
    got = _norm_of(one)
    assert one.grad_norm.is_cuda and one.grad_norm.dim() == 0
    assert one._partials.numel() > 256                               # the finish kernel's threads walk more than one partial each
    assert abs(got - want) <= NORM_RTOL * want, (got, want)
    # two groups with different learning rates: the norm is the norm of BOTH
    qs = _params(_tensors(1))
    two = optim.SGD([{"params": qs[:4], "lr": 1e-2}, {"params": qs[4:], "lr": 1e-3}], lr=1e-2, momentum=0.9, max_norm=1e30)
    _set_grads(qs, grads)
    two.step()
    got2 = _norm_of(two)
    assert abs(got2 - want) <= NORM_RTOL * want, (got2, want)
    assert OU.global_norm([g.numpy() for g in grads[4:]]) < want * (1 - 1e-4)          # (a per-group norm would have been told apart)
    # the same bits from a second run on the same values
    _set_grads(ps, grads)
    one.step()
    torch.cuda.synchronize()
    assert np.float32(got).tobytes() == np.float32(_norm_of(one)).tobytes()


def test_grad_norm_does_not_depend_on_which_tensor_is_misaligned():
    """the aligned (3, 4100) tensor and the misaligned view trade values: vector-path and dword-path chunks swap roles"""
    from vae_segmentation_amd import optim
    grads = _tensors(8, 0.3)
    swapped = list(grads)
    swapped[I_TWIN], swapped[I_VIEW] = grads[I_VIEW].reshape(3, 4100), grads[I_TWIN].reshape(-1)
    want = OU.global_norm([g.numpy() for g in grads])
    got = []
    for gs in (grads, swapped):
        ps = _params(_tensors(1))
        opt = optim.SGD(ps, lr=1e-2, momentum=0.9, max_norm=1e30)
        _set_grads(ps, gs)
        opt.step()
        got.append(_norm_of(opt))
    for g in got:
        assert abs(g - want) <= NORM_RTOL * want, (got, want)


def test_sqnorm_partials_are_a_function_of_the_chunk_values_alone():
    """vs_grad_sqnorm_multi on the same values at a 16-byte-aligned address (vector loads) and one element further (dword loads): the same partials,
    bit for bit, full chunks and the ragged one; and each partial is the fp64 sum of its chunk's squares within fp64 rounding"""
    from vae_segmentation_amd._lib import check, lib
    from vae_segmentation_amd.optim import _Tables
    n = 5 * 4096 + 123
    vals = torch.randn(n, generator=torch.Generator().manual_seed(3)) * 0.7
    a = vals.cuda()
    buf = torch.zeros(n + 8, device="cuda")
    b = buf[1:1 + n]
    b.copy_(vals)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4
    outs = []
    for t in (a, b):
        (gp, sizes, bm), nb = _Tables().get([[t]], t.device)
        part = torch.full((nb,), -1.0, dtype=torch.float64, device="cuda")
        check(lib.vs_grad_sqnorm_multi(gp.data_ptr(), sizes.data_ptr(), bm.data_ptr(), nb, part.data_ptr(), torch.cuda.current_stream().cuda_stream), "sqnorm")
        outs.append(part.cpu())
    assert outs[0].numel() == 6 and torch.equal(outs[0], outs[1])
    v64 = vals.double()
    want = torch.stack([(v64[i:i + 4096] ** 2).sum() for i in range(0, n, 4096)])
    assert float(((outs[0] - want).abs() / want).max()) < 1e-13


def _cpu_reference(make_opt, max_norm, steps=3):
    ref = [torch.nn.Parameter(t.clone()) for t in _tensors(1)]
    o_ref = make_opt(ref)
    for step in range(steps):
        for p, g in zip(ref, _step_grads(step)):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref, max_norm)
        o_ref.step()
    return ref, o_ref


def _step_grads(step):
    return _tensors(20 + step, 0.1 if step < 2 else 0.01)            # the third step's gradients are ten times smaller: it is not clipped


def _traj_max_norm():
    """half the first step's norm: steps 0 and 1 clip, step 2 does not (checked through the oracle)"""
    norms = [OU.global_norm([g.numpy() for g in _step_grads(s)]) for s in range(3)]
    max_norm = 0.5 * norms[0]
    coefs = [float(OU.clip_coef(np.float32(n), max_norm)) for n in norms]
    assert coefs[0] < 0.51 and coefs[1] < 1.0 and coefs[2] == 1.0
    return max_norm, norms


@pytest.mark.parametrize("momentum,wd,nesterov", [(0.9, 0.0, True), (0.99, 3e-5, True), (0.9, 3e-5, False), (0.99, 0.0, False)])
def test_clipped_sgd_trajectory_matches_torch(momentum, wd, nesterov):
    from vae_segmentation_amd import optim
    max_norm, norms = _traj_max_norm()
    ref, _ = _cpu_reference(lambda ps: torch.optim.SGD(ps, lr=1e-2, momentum=momentum, weight_decay=wd, nesterov=nesterov), max_norm)
    mine = _params(_tensors(1))
    opt = optim.SGD(mine, lr=1e-2, momentum=momentum, weight_decay=wd, nesterov=nesterov, max_norm=max_norm)
    for step in range(3):
        _set_grads(mine, _step_grads(step))
        opt.step()
        assert abs(_norm_of(opt) - norms[step]) <= NORM_RTOL * norms[step]
    for p, q in zip(ref, mine):
        assert float((q.detach().cpu() - p.detach()).abs().max()) <= 1e-6 * float(p.detach().abs().max()) + 1e-7


def test_clipped_adam_trajectory_matches_torch():
    """No weight decay here, on purpose: Adam's first step is lr * gi / (|gi| + eps), and with gi = g * coef + wd * p an element whose two terms cancel to
    a few eps (1e-8) turns ONE ulp of the sum (2e-9) into 1e-2 of the step.  Among 1.5 M elements a few such elements exist in every draw, and there
    the fp32 reference is no more right than the kernel (measured with wd = 1e-2: 1.7e-5 on one element of the (128, 64, 3, 3, 3) tensor against a bound
    of 9.4e-6).  g * coef alone is one rounding of its own size, so the comparison is well conditioned; weight decay is covered by the SGD trajectories."""
    from vae_segmentation_amd import optim
    max_norm, norms = _traj_max_norm()
    ref, _ = _cpu_reference(lambda ps: torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), max_norm)
    mine = _params(_tensors(1))
    opt = optim.Adam(mine, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=max_norm)
    for step in range(3):
        _set_grads(mine, _step_grads(step))
        opt.step()
        assert abs(_norm_of(opt) - norms[step]) <= NORM_RTOL * norms[step]
    for p, q in zip(ref, mine):
        assert float((q.detach().cpu() - p.detach()).abs().max()) <= 2e-6 * float(p.detach().abs().max()) + 1e-7


@pytest.mark.parametrize("nesterov", [False, True])
def test_inactive_clip_is_free_of_rounding(nesterov):
    """max_norm = 1e30 never clips: coef is exactly 1 and the step gives the bits of max_norm = None — for nesterov = False that is the plain
    launch (vs_sgd_momentum_scaled_multi) against the extended one, on vector-path, ragged and misaligned chunks"""
    from vae_segmentation_amd import optim
    runs = []
    for max_norm in (None, 1e30):
        ps = _params(_tensors(1))
        opt = optim.SGD(ps, lr=1e-2, momentum=0.9, weight_decay=3e-5, nesterov=nesterov, max_norm=max_norm)
        for step in range(3):
            _set_grads(ps, _step_grads(step))
            opt.step()
        torch.cuda.synchronize()
        runs.append((ps, [opt.state[p]["momentum_buffer"] for p in ps]))
    for k in (0, 1):
        for a, b in zip(runs[0][k], runs[1][k]):
            assert torch.equal(a.detach(), b.detach())


class _Spy:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self.real, name)


def test_defaults_launch_the_plain_step(monkeypatch):
    """SGD(lr, momentum, wd) and Adam(...) constructed as before launch what they launched before — no norm launch, the old entry points — and SGD's
    step is bit-equal to vs_sgd_momentum_scaled_multi called directly on the same tables"""
    from vae_segmentation_amd import optim
    from vae_segmentation_amd._lib import check, lib
    spy = _Spy(optim.lib)
    monkeypatch.setattr(optim, "lib", spy)
    ps = _params(_tensors(1))
    opt = optim.SGD(ps, lr=1e-2, momentum=0.9, weight_decay=3e-5)
    qs = _params(_tensors(1))
    bufs = [torch.zeros_like(q) for q in qs]
    stream = torch.cuda.current_stream().cuda_stream
    for step in range(2):
        _set_grads(ps, _step_grads(step))
        opt.step()
        grads = _to_gpu(_step_grads(step))
        (pp, gp, bp, sizes, bm), nb = optim._Tables().get([qs, grads, bufs], qs[0].device)
        check(lib.vs_sgd_momentum_scaled_multi(pp.data_ptr(), gp.data_ptr(), bp.data_ptr(), sizes.data_ptr(), bm.data_ptr(), nb, 1e-2, 0.9, 3e-5, 0,
                                               None, None, stream), "sgd")
    torch.cuda.synchronize()
    assert spy.calls == ["vs_sgd_momentum_scaled_multi"] * 2
    for p, q, m in zip(ps, qs, bufs):
        assert torch.equal(p.detach(), q.detach()) and torch.equal(opt.state[p]["momentum_buffer"], m)
    del spy.calls[:]
    adam = optim.Adam(ps, lr=1e-3)
    adam.step()
    assert spy.calls == ["vs_adam_scaled_multi"] and opt.grad_norm is None and adam.grad_norm is None


def test_loss_scaler_norm_is_unscaled_and_overflow_skips_the_step():
    from vae_segmentation_amd import optim
    grads = _tensors(9, 0.3)
    want = OU.global_norm([g.numpy() for g in grads])
    scaler = optim.LossScaler(init_scale=65536.0)
    ps = _params(_tensors(1))
    opt = optim.SGD(ps, lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=True, max_norm=0.5 * want)
    _set_grads(ps, [g * 65536.0 for g in grads])                     # a power of two: every scaled gradient is exact
    opt.step(scaler=scaler)
    got = _norm_of(opt)
    assert abs(got - want) <= NORM_RTOL * want, (got, want)
    assert float(scaler.scale.item()) == 65536.0
    # ... and the clipped, unscaled step is the step of the unscaled gradients
    qs = _params(_tensors(1))
    plain = optim.SGD(qs, lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=True, max_norm=0.5 * want)
    _set_grads(qs, grads)
    plain.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())
    # an inf in one gradient: nothing moves, the scale is halved
    snap_p = [p.detach().clone() for p in ps]
    snap_m = [opt.state[p]["momentum_buffer"].clone() for p in ps]
    bad = [g * 65536.0 for g in _tensors(10, 0.3)]
    bad[4][17] = float("inf")
    _set_grads(ps, bad)
    opt.step(scaler=scaler)
    torch.cuda.synchronize()
    assert float(scaler.scale.item()) == 32768.0 and float(scaler.found_inf.item()) == 0.0
    for p, s, m in zip(ps, snap_p, snap_m):
        assert torch.equal(_bits(p), _bits(s)) and torch.equal(_bits(opt.state[p]["momentum_buffer"]), _bits(m))


def _seg_step_pair(side=32, seed=0):
    import joint_model as M
    from oracle import ref_cpu as O
    seg = O.deterministic_fill_(M.Segmentation(1, 2, norm_type=1), seed=seed).cuda()
    img, lab = O.synthetic_image(1, side, 2 + seed).cuda(), O.synthetic_label(1, side, 3 + seed).cuda()
    return seg, img, lab


def test_graphed_step_captures_the_clipped_nesterov_tail():
    """the captured tail follows lr AND max_norm from device memory (no re-capture) and equals the eager loop bit for bit — the flat gradient views of
    the captured step and the eager loop's own gradient tensors sit at different alignments, the norm is the same bits; switching clipping off
    removes launches: one re-capture"""
    from vae_segmentation_amd import optim
    from vae_segmentation_amd import train as T
    seg_p, img, lab = _seg_step_pair(seed=0)
    loss, _ = T.seg_train_losses(seg_p, img, lab)                   # a probe pass: the size of this model's gradient
    loss.backward()
    from vae_segmentation_amd import ops
    ops.flush_wgrads()
    torch.cuda.synchronize()
    m0 = 0.5 * OU.global_norm([p.grad.cpu().numpy() for p in seg_p.parameters() if p.grad is not None])
    assert m0 > 0 and math.isfinite(m0)
    del loss, seg_p
    seg_a, img, lab = _seg_step_pair(seed=0)
    seg_c, _, _ = _seg_step_pair(seed=0)
    kw = dict(lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=True, max_norm=m0)
    opt_a, opt_c = optim.SGD(seg_a.parameters(), **kw), optim.SGD(seg_c.parameters(), **kw)
    gs = T.GraphedStep(lambda: T.seg_train_losses(seg_a, img, lab), list(seg_a.parameters()), opt_a, warmup=1)
    assert gs.tail

    def both(lr, max_norm):
        for o in (opt_a, opt_c):
            o.param_groups[0]["lr"] = lr
            o.max_norm = max_norm
        gs.step()
        opt_c.zero_grad()
        loss, _ = T.seg_train_losses(seg_c, img, lab)
        loss.backward()
        opt_c.step()

    norms = []
    for lr, mn in [(1e-2, m0), (5e-3, m0), (5e-3, 0.5 * m0), (2e-2, 1e30), (1e-3, m0)]:
        both(lr, mn)
        norms.append((float(opt_a.grad_norm.item()), float(opt_c.grad_norm.item())))
    torch.cuda.synchronize()
    assert gs.recaptures == 0
    assert all(a == c and math.isfinite(a) for a, c in norms), norms
    assert norms[0][0] > m0                                          # the first step did clip
    for (n, p), q in zip(seg_a.named_parameters(), seg_c.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    both(1e-3, None)
    both(1e-3, None)
    torch.cuda.synchronize()
    assert gs.recaptures == 1 and gs.tail
    for (n, p), q in zip(seg_a.named_parameters(), seg_c.parameters()):
        assert torch.equal(p.detach(), q.detach()), n


def _run(args, cwd):
    return subprocess.run([sys.executable] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True, timeout=900)


def test_main_source_trains_with_the_nnunet_optimiser_flags(tmp_path):
    common = ["--size", "64", "-b", "1", "-E", "2", "--eval_epoch", "1", "--save_epoch", "2", "--synthetic_train", "2",
              "--synthetic_val", "1", "--max_iters", "2", "--display_freq", "1"]
    out = _run([os.path.join(REPO, "main_source.py"), "clip", "-M", "seg_train", "--nesterov", "--momentum", "0.99", "--weight_decay", "3e-5",
                "--grad_clip", "12", "--lr_schedule", "poly"] + common, str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Finished Training" in out.stdout and "graph replay" in out.stdout
    norms = [float(m) for m in re.findall(r"grad_norm (\S+?),?\s", out.stdout + " ")]
    assert len(norms) >= 4 and all(math.isfinite(v) and v > 0 for v in norms), out.stdout[-2000:]
    bad = _run([os.path.join(REPO, "main_source.py"), "clip", "-M", "seg_train", "--nesterov", "--adam"] + common, str(tmp_path))
    assert bad.returncode == 2 and "--nesterov" in bad.stderr
    import main_target
    a = main_target.parse(["r", "--nesterov", "--momentum", "0.99", "--weight_decay", "3e-5", "--grad_clip", "12", "--lr_schedule", "poly"])
    assert a.nesterov and a.grad_clip == 12.0 and a.lr_schedule == "poly"
    with pytest.raises(SystemExit):
        main_target.parse(["r", "--nesterov", "--adam"])
