// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11): four 32-bit counter words and two key words ->
// four output words, ten rounds of two 32 x 32 -> 64 bit products.  A pure function of its arguments: no state, the same bits in every launch geometry.
// Users: elastic.hip (counter word 2 = the field's axis, 0..2; words w0, w1), augment.hip (counter word 2 = 0x100 + channel; all four words) and
// latent.hip's latent stream (counter (pair, draw low, 0x200, draw high); all four words).
#pragma once
#include <math.h>

__device__ __forceinline__ void vs_philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0, unsigned int k1,
                                                 unsigned int& w0, unsigned int& w1, unsigned int& w2, unsigned int& w3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned int)p1; c3 = (unsigned int)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w0 = c0; w1 = c1; w2 = c2; w3 = c3;
}

// two output words -> the 53-bit integer (a >> 5) 2^26 + (b >> 6) as an fp64, exact; times 2^-53: a uniform in [0, 1)
__device__ __forceinline__ double vs_philox_u53(unsigned int a, unsigned int b) {
#pragma clang fp contract(off)
    return (double)(a >> 5) * 67108864.0 + (double)(b >> 6);
}
// Box-Muller on four output words: radius r = sqrt(-2 ln u1) with u1 = (u53 + 0.5) / 2^53 in (0, 1), angle a = 2 pi u2 with u2 = u53 / 2^53; the pair of
// normals is (r cos a, r sin a).  Contraction off: augment.hip and latent.hip's latent stream are pinned bit for bit to this order of roundings.
// (elastic.hip's uniform spells its u53 out: it compiles under the default contraction, the same exact value through one fused multiply-add.)
__device__ __forceinline__ void vs_philox_box_muller(unsigned int w0, unsigned int w1, unsigned int w2, unsigned int w3, double& r, double& a) {
#pragma clang fp contract(off)
    const double u1 = (vs_philox_u53(w0, w1) + 0.5) * 0x1p-53;
    const double u2 = vs_philox_u53(w2, w3) * 0x1p-53;
    r = sqrt(-2.0 * log(u1));
    a = 2.0 * M_PI * u2;
}
