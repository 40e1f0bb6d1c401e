"""The oracle of the intensity augmentation tests (tests/test_host_augment.py pins it, tests/test_gpu_augment.py uses it): numpy and scipy only.

batchgenerators is not installed; the rules are the ones DESIGN "Intensity augmentation" states, restated here in fp64 numpy.  An op maps one float32
plane (D, H, W) to one float32 plane: it is computed in fp64 from the float32 input and from the fp64 statistics of that plane, and rounded to float32
once — so every function below takes and returns float32 and a chain of them rounds at every op boundary.

    noise        x + s n                                            (s used as the standard deviation)
    blur         scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4) of the float32 array: z, y, x passes, each rounded to float32
    brightness   x m
    contrast     (x - mean) f + mean, clipped to [min, max] with preserve_range
    power        x' = -x if invert; ((x' - min) / (max - min + 1e-7))^g (max - min) + min with the statistics of x'; negated back
    restat       (x' - mean(x')) / (std(x') + 1e-8) std0 + mean0, same negation
    gamma        power; with retain_stats followed by restat with the mean and std of the x' that entered power
    flip         mirror along z / y / x for the bits 4 / 2 / 1 of the mask
"""
import numpy as np

from tests.elastic_util import M32, ref_philox4x32


def _f32(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, "the oracle's ops take float32 planes"
    return x


def ref_stats(x):
    """(min, max, mean, population std) in fp64, the sums shifted by the plane's first voxel"""
    v = _f32(x).astype(np.float64).reshape(-1)
    dv = v - v[0]
    m1 = dv.sum() / v.size
    var = (dv * dv).sum() / v.size - m1 * m1
    return float(v.min()), float(v.max()), float(v[0] + m1), float(np.sqrt(max(var, 0.0)))


def ref_noise(x, s, n):
    return (_f32(x).astype(np.float64) + float(s) * np.asarray(n, np.float64)).astype(np.float32)


def ref_weights(sigma):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, int(4 sigma + 0.5)), all 2 radius + 1 weights"""
    radius = int(4.0 * float(sigma) + 0.5)
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return phi / phi.sum()


def ref_blur(x, sigma):
    """three passes z, y, x; each: the line mirrored as scipy's "reflect" does (d c b a | a b c d | d c b a — numpy calls it "symmetric" — repeated when
    the line is shorter than the radius), fp64 accumulation in the order of scipy's correlate1d for a symmetric kernel (centre tap, then the pairs from
    the outside in, (a + b) w), rounded to float32"""
    out = _f32(x)
    w = ref_weights(sigma)
    r = len(w) // 2
    for axis in range(3):
        v = np.moveaxis(out.astype(np.float64), axis, 0)
        n = v.shape[0]
        p = np.pad(v, [(r, r)] + [(0, 0)] * (v.ndim - 1), mode="symmetric")
        acc = p[r:r + n] * w[r]
        for j in range(-r, 0):
            acc = acc + (p[r + j:r + j + n] + p[r - j:r - j + n]) * w[r + j]
        out = np.ascontiguousarray(np.moveaxis(acc, 0, axis)).astype(np.float32)
    return out


def ref_brightness(x, m):
    return (_f32(x).astype(np.float64) * float(m)).astype(np.float32)


def ref_contrast(x, f, preserve_range=True):
    mn, mx, mean, _ = ref_stats(x)
    y = (_f32(x).astype(np.float64) - mean) * float(f) + mean
    if preserve_range:
        y = np.clip(y, mn, mx)
    return y.astype(np.float32)


def _signed(x, invert):
    return -_f32(x) if invert else _f32(x)


def ref_power(x, g, invert=False):
    xp = _signed(x, invert)
    mn, mx, _, _ = ref_stats(xp)
    r = mx - mn
    y = np.power((xp.astype(np.float64) - mn) / (r + 1e-7), float(g)) * r + mn
    return (-y if invert else y).astype(np.float32)


def ref_restat(x, mean0, std0, invert=False):
    xp = _signed(x, invert)
    _, _, mean, std = ref_stats(xp)
    y = (xp.astype(np.float64) - mean) / (std + 1e-8) * float(std0) + float(mean0)
    return (-y if invert else y).astype(np.float32)


def ref_gamma(x, g, invert=False, retain_stats=False):
    y = ref_power(x, g, invert)
    if retain_stats:
        _, _, mean0, std0 = ref_stats(_signed(x, invert))
        y = ref_restat(y, mean0, std0, invert)
    return y


def ref_flip(x, mask):
    x = np.asarray(x)
    axes = [a for a, bit in zip((-3, -2, -1), (4, 2, 1)) if mask & bit]
    return np.ascontiguousarray(np.flip(x, axes)) if axes else x


def ref_normal(n, seed, sample, channel):
    """the first n standard normals of plane (seed, sample, channel), float64: pair j under counter (j low, j high, 0x100 + channel, sample low) and key
    (seed low, seed high); u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53, u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53, r = sqrt(-2 ln u1),
    n[2j] = r cos(2 pi u2), n[2j + 1] = r sin(2 pi u2)"""
    j = np.arange((int(n) + 1) // 2, dtype=np.uint64)
    ctr = (j & np.uint64(M32), j >> np.uint64(32), np.full_like(j, 0x100 + int(channel)), np.full_like(j, int(sample) & M32))
    key = (np.full_like(j, int(seed) & M32), np.full_like(j, (int(seed) >> 32) & M32))
    w0, w1, w2, w3 = ref_philox4x32(ctr, key)
    u1 = ((w0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w1 >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = ((w2 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w3 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    r, a = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1).reshape(-1)[:int(n)]


def _of_channel(v, c):
    return v[c] if isinstance(v, (list, tuple, np.ndarray)) else v


def ref_op(x, op, channel=0, channels=1):
    """one op of an ops list (the tuples data_gpu.intensity_augment takes) on the float32 plane x of channel `channel`"""
    name, a = op[0], op[1:]
    first = _of_channel(a[0], channel) if name != "flip" else a[0]
    if first is None:
        return _f32(x)
    if name == "noise":
        spec = a[1]
        n = ref_normal(x.size, spec[0], spec[1], channel).reshape(x.shape) if isinstance(spec, tuple) else np.asarray(spec)[channel]
        return ref_noise(x, first, n)
    if name == "blur":
        return ref_blur(x, first)
    if name == "brightness":
        return ref_brightness(x, first)
    if name == "contrast":
        return ref_contrast(x, first, a[1] if len(a) > 1 else True)
    if name == "gamma":
        return ref_gamma(x, first, a[1] if len(a) > 1 else False, a[2] if len(a) > 2 else False)
    if name == "power":
        return ref_power(x, first, a[1] if len(a) > 1 else False)
    if name == "restat":
        return ref_restat(x, first, _of_channel(a[1], channel), a[2] if len(a) > 2 else False)
    if name == "flip":
        return ref_flip(_f32(x), first)
    raise ValueError(name)


def ref_chain(x, ops_list):
    """(C, D, H, W) float32 through the ops in order, every op boundary a float32 array"""
    out = []
    for c in range(x.shape[0]):
        v = _f32(x[c])
        for op in ops_list:
            v = ref_op(v, op, c, x.shape[0])
        out.append(v)
    return np.stack(out)


DEFAULTS = dict(p_noise=0.1, noise_s=(0.0, 0.1), p_blur=0.2, blur_sigma=(0.5, 1.0), p_blur_per_channel=0.5, p_brightness=0.15, brightness=(0.75, 1.25),
                p_contrast=0.15, contrast=(0.75, 1.25), preserve_range=True, p_gamma_inverted=0.1, p_gamma=0.3, gamma=(0.7, 1.5), retain_stats=True,
                p_mirror=0.5)


def _range_val(rng, lo, hi):
    if rng.random_sample() < 0.5 and lo < 1:
        return rng.uniform(lo, 1)
    return rng.uniform(max(lo, 1), hi)


def ref_draw(rng, channels, shape, noise="numpy", seed=0, n_noised=0, **kw):
    """IntensityAugment.draw's ops list from `rng`: noise gate, s, [one rng.normal(0, 1, shape) per channel with noise="numpy"]; blur gate, per channel
    uniform() <= p and then sigma; brightness gate, m per channel; contrast gate, f per channel (random_sample() < 0.5 and lo < 1 ? uniform(lo, 1) :
    uniform(max(lo, 1), hi)); inverted gamma gate, g per channel by the same rule; gamma gate, likewise; one uniform() < p_mirror per axis z, y, x.
    kw: the probabilities and ranges of DEFAULTS."""
    p = dict(DEFAULTS, **kw)
    ops_list = []
    if rng.uniform() < p["p_noise"]:
        s = rng.uniform(*p["noise_s"])
        spec = np.stack([rng.normal(0.0, 1.0, tuple(shape)) for _ in range(channels)]) if noise == "numpy" else (seed, n_noised)
        ops_list.append(("noise", s, spec))
    if rng.uniform() < p["p_blur"]:
        ops_list.append(("blur", [rng.uniform(*p["blur_sigma"]) if rng.uniform() <= p["p_blur_per_channel"] else None for _ in range(channels)]))
    if rng.uniform() < p["p_brightness"]:
        ops_list.append(("brightness", [rng.uniform(*p["brightness"]) for _ in range(channels)]))
    if rng.uniform() < p["p_contrast"]:
        ops_list.append(("contrast", [_range_val(rng, *p["contrast"]) for _ in range(channels)], p["preserve_range"]))
    if rng.uniform() < p["p_gamma_inverted"]:
        ops_list.append(("gamma", [_range_val(rng, *p["gamma"]) for _ in range(channels)], True, p["retain_stats"]))
    if rng.uniform() < p["p_gamma"]:
        ops_list.append(("gamma", [_range_val(rng, *p["gamma"]) for _ in range(channels)], False, p["retain_stats"]))
    mask = sum(bit for bit in (4, 2, 1) if rng.uniform() < p["p_mirror"])
    if mask:
        ops_list.append(("flip", mask))
    return ops_list


def same_ops(a, b):
    """two ops lists are equal, arrays compared element for element"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if len(x) != len(y) or x[0] != y[0]:
            return False
        for u, v in zip(x[1:], y[1:]):
            if isinstance(u, np.ndarray) or isinstance(v, np.ndarray):
                if not np.array_equal(np.asarray(u), np.asarray(v)):
                    return False
            elif u != v:
                return False
    return True
