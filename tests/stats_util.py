"""Per-(sample, channel) InstanceNorm statistics against a two-pass fp64 reference.

Every InstanceNorm reads its mean and rstd from a (sum, sumsq) pair per (n, c) that a kernel epilogue accumulated (csrc/common.h stat_add;
the deterministic build keeps the pair as four fixed-point limbs).  These helpers decode such a pair into mean / rstd with the formula of
pair_to_mean_rstd (fp64, eps 1e-5) and compare each (n, c) on its own with a two-pass fp64 reference of the same values:
  mean   |mean - mean_ref| / std_ref          <= mean_tol * (1 + R)          R = |mean_ref| / std_ref, the channel's offset
  rstd   |rstd / rstd_ref - 1|                <= rstd_tol  (R <= r_tight; above: rstd_tol_high or R^2 2^-23)
  sum    |S - S_ref| / sqrt(N * Q_ref)        <= sum_tol
The sum bound catches a workgroup partial that is lost or counted twice even where the normalised statistics hide it.
Pure torch on the CPU: the host suite tests the helpers themselves (tests/test_host.py)."""
import torch

EPS_IN = 1e-5


def pair_mean_rstd(tot, count, eps=EPS_IN):
    """(..., 2) fp64 (sum, sumsq) totals -> fp64 mean, rstd: the arithmetic of pair_to_mean_rstd (csrc/common.h)"""
    tot = tot.double()
    m = tot[..., 0] / count
    var = (tot[..., 1] / count - m * m).clamp_min(0.0)
    return m, 1.0 / torch.sqrt(var + eps)


def two_pass(y, eps=EPS_IN):
    """y (n, c, ...) -> per-(n, c) fp64 reference: count, S, Q, mean and std (two passes), rstd, R"""
    y = y.double().reshape(y.shape[0], y.shape[1], -1)
    count = y.shape[-1]
    mean = y.mean(-1)
    var = ((y - mean[..., None]) ** 2).mean(-1)
    std = var.sqrt()
    return {"count": count, "S": y.sum(-1), "Q": (y * y).sum(-1), "mean": mean, "std": std,
            "rstd": 1.0 / torch.sqrt(var + eps), "R": mean.abs() / std.clamp_min(1e-300)}


def stat_errors(tot, ref):
    """per-(n, c) errors of the decoded totals tot (n, c, 2) against two_pass(...): mean (in units of std_ref), rstd (relative), sum
    (against sqrt(N Q_ref))"""
    tot = tot.double().cpu()
    m, r = pair_mean_rstd(tot, ref["count"])
    return {"mean": (m - ref["mean"]).abs() / ref["std"].clamp_min(1e-300),
            "rstd": (r / ref["rstd"] - 1.0).abs(),
            "sum": (tot[..., 0] - ref["S"]).abs() / (ref["count"] * ref["Q"]).sqrt().clamp_min(1e-300)}


R_BANDS = ((0.0, 1.0), (1.0, 10.0), (10.0, 100.0), (100.0, float("inf")))


def band_worst(err, ref):
    """{band label: {statistic: worst error}} over the (n, c) whose R falls in each band (bands without a channel are left out)"""
    out = {}
    for lo, hi in R_BANDS:
        sel = (ref["R"] >= lo) & (ref["R"] < hi)
        if bool(sel.any()):
            out["R%g-%g" % (lo, hi)] = {k: float(v[sel].max()) for k, v in err.items()}
    return out


def check_stats(tot, ref, tag, mean_tol=1e-5, rstd_tol=1e-4, sum_tol=1e-5, r_tight=40.0, rstd_tol_high=5e-3, rstd_grows_with_r=False):
    """assert the per-(n, c) bounds of the module docstring; print the worst errors per R band.  -> band_worst(...)
    rstd_grows_with_r: the rstd bound times (1 + R) — for a reference whose values differ from the kernel's by a relative rounding e (a lazy
    input normalised and rounded on one side only): such errors follow the values, mean included, and move var by ~e R std^2"""
    err = stat_errors(tot, ref)
    R = ref["R"]
    # above r_tight: rstd_tol_high, or the one-pass limit of a pair accumulated in fp32 lanes if that is larger — var = Q/N - m^2 carries the
    # fp32 rounding of Q times R^2 (2^-24 R^2 relative, twice for the lane sum and the butterfly: 5.4e-3 of rstd at R = 300)
    high = torch.maximum(torch.full_like(R, rstd_tol_high), R * R * 2.0 ** -23)
    lim_rstd = torch.where(R <= r_tight, torch.full_like(R, rstd_tol), high)
    if rstd_grows_with_r:
        lim_rstd = lim_rstd * (1.0 + R)
    bad = {"mean": err["mean"] > mean_tol * (1.0 + R), "rstd": err["rstd"] > lim_rstd, "sum": err["sum"] > sum_tol}
    worst = band_worst(err, ref)
    print("\n%s: %s" % (tag, "; ".join("%s mean %.1e rstd %.1e sum %.1e" % (b, e["mean"], e["rstd"], e["sum"]) for b, e in worst.items())))
    msgs = []
    for k, m in bad.items():
        if bool(m.any()):
            idx = [tuple(int(i) for i in ix) for ix in m.nonzero()[:4]]
            msgs.append("%s at (n, c) %s: %s (R %s)" % (k, idx, [float(err[k][i]) for i in idx], [round(float(R[i]), 1) for i in idx]))
    assert not msgs, "%s: per-(n, c) statistics off: %s" % (tag, "; ".join(msgs))
    return worst


def pack_limbs(tot, slots=4, interleaved=False):
    """fp64 totals (n, c, 2) -> the deterministic build's buffer double[4][n][c][2] of four signed 40-bit-weighted limbs (the split of
    stat_add in csrc/common.h, here as ONE partial per pair), each stored as the int64 bit pattern in a double slot.  interleaved: the
    VS_STAT_INTERLEAVE layout double[n][c][4][2], handed back viewed as (4, n, c, 2) the way a buffer of that layout is shaped."""
    assert slots == 4
    tot = tot.double()
    n, c, _ = tot.shape
    limbs = torch.zeros(4, n, c, 2, dtype=torch.int64)
    r = tot.clone()
    for s, (up, down) in enumerate(((2.0 ** -40, 2.0 ** 40), (1.0, 1.0), (2.0 ** 40, 2.0 ** -40), (2.0 ** 80, 2.0 ** -80))):
        q = torch.trunc(r * up)
        r = r - q * down
        limbs[s] = q.to(torch.int64)
    if interleaved:
        limbs = limbs.permute(1, 2, 0, 3).contiguous().view(4, n, c, 2)
    return limbs.view(torch.float64)
