"""The oracle of the latent noise tests (tests/test_host_latent.py pins it, tests/test_gpu_latent.py uses it): numpy only.

A latent stream is (seed, draw), two unsigned 64-bit integers.  Element i < count of draw t (i = b dim + j of a (B, dim) latent), pair q = i >> 1:
Philox4x32-10 under key (seed low 32, seed high 32) and counter (q, t low 32, 0x200, t high 32); u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53,
u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53, r = sqrt(-2 ln u1) in fp64 (tests/augment_util.py:ref_normal forms them the same way); even i takes
r cos(2 pi u2), odd i takes r sin(2 pi u2), rounded to float32 once.  An odd count uses only the cosine of its last pair.  Integers, then fp64, then fp32."""
import numpy as np

from tests.elastic_util import M32, ref_philox4x32

LATENT_WORD = 0x200            # counter word 2: the elastic stream has 0 .. 2 there, the augmentation stream 0x100 + channel


def ref_latent_words(pairs, seed, draw, word2=LATENT_WORD):
    """the four Philox output words of pairs 0 .. pairs - 1 of draw `draw`, uint64 arrays of values below 2^32"""
    q = np.arange(int(pairs), dtype=np.uint64)
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    ctr = (q, np.full_like(q, draw & M32), np.full_like(q, int(word2)), np.full_like(q, draw >> 32))
    key = (np.full_like(q, seed & M32), np.full_like(q, seed >> 32))
    return ref_philox4x32(ctr, key)


def ref_latent_normal64(count, seed, draw, word2=LATENT_WORD):
    """the first `count` normals of draw `draw` before the rounding to float32, float64"""
    count = int(count)
    w0, w1, w2, w3 = ref_latent_words((count + 1) // 2, seed, draw, word2)
    u1 = ((w0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w1 >> np.uint64(6)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = ((w2 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w3 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    r, a = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1).reshape(-1)[:count]


def ref_latent_normal(shape, seed, draw):
    """draw `draw` of the stream `seed` for a latent of `shape`, float32"""
    shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    return ref_latent_normal64(int(np.prod(shape)), seed, draw).astype(np.float32).reshape(shape)
