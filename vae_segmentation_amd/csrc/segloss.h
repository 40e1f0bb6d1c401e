// What the compound loss (segloss.hip) and its top-k form (topk.hip) share: the limits, the class weights as a kernel argument, the statistics' layout,
// the focal voxel loss and its derivative, the host-side validation and the grid.  Included inside each translation unit: everything here has internal
// linkage.
#pragma once
#include "common.h"

#define SEG_MAXC 8
#define SEG_BLOCKS 512                 // block cap of both grids: 512 x 256 threads = 131072 quads per sweep of the grid-stride loop
#define SEG_MAXB 64                    // seg_finish_kernel keeps batch * (3C + 2) totals in LDS

struct SegW { float w[SEG_MAXC]; };    // class weights, by value in the kernel arguments

// statistics of one sample, in this order, in the partials and at the head of scratch: S[C], I[C], T[C], sum w f, sum w
__host__ __device__ static inline int seg_nstat(int channels) { return 3 * channels + 2; }

// x^g in fp64 (g wave-uniform): g = 0, 1, 2 — plain cross-entropy and the usual focal exponents — are exact without the pow routine, which costs as much
// again as the logarithm next to it (x * x is x^2 rounded once)
__device__ __forceinline__ double seg_pow(double x, double g) {
    if (g == 0.0) return 1.0;
    if (g == 1.0) return x;
    if (g == 2.0) return x * x;
    return pow(x, g);
}
// f = -(1 - p)^gamma * max(ln p, -100) in fp64
__device__ __forceinline__ double seg_focal(double p, double gamma) {
    const double lg = fmax(log(p), -100.0);
    return gamma == 0.0 ? -lg : -(seg_pow(1.0 - p, gamma) * lg);
}
// df/dp of the same: gamma (1-p)^(gamma-1) L - (1-p)^gamma L', L' = 1/p where the clamp is inactive and 0 where it is active.  The clamp is active iff
// ln p < -100 iff p < e^-100 = 3.72e-44: for an fp32 p that is 0 and the 26 smallest denormals (26 * 2^-149 = 3.64e-44, 27 * 2^-149 = 3.78e-44 — nowhere
// near a rounding question), so plain cross-entropy needs no logarithm here.  p == 1 with gamma > 0: both terms' limit is 0.
__device__ __forceinline__ double seg_focal_grad(double p, double gamma) {
    const bool clamped = p >= 0.0 && p < 3.720075976020836e-44;
    const double dl = clamped ? 0.0 : 1.0 / p;
    if (gamma == 0.0) return -dl;
    const double om = 1.0 - p;
    if (om == 0.0) return 0.0;
    const double lg = clamped ? -100.0 : log(p);
    const double t = seg_pow(om, gamma - 1.0);
    return t * (gamma * lg - om * dl);
}

// the block's sums -> its partials part[b][q][block]: waves reduce by shuffles, the four waves through LDS, one thread per statistic stores
template <int C>
__device__ __forceinline__ void seg_store_partials(double (&aS)[C], double (&aI)[C], int (&aT)[C], double aN, double aD, double* __restrict__ part, int b) {
    constexpr int NS = 3 * C + 2;
    __shared__ double red[4][NS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double s = wave_sum_d(aS[c]), t = wave_sum_d(aI[c]), n = wave_sum_d((double)aT[c]);      // a count is exact in fp64
        if (lane == 0) { red[wave][c] = s; red[wave][C + c] = t; red[wave][2 * C + c] = n; }
    }
    aN = wave_sum_d(aN);
    aD = wave_sum_d(aD);
    if (lane == 0) { red[wave][3 * C] = aN; red[wave][3 * C + 1] = aD; }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int q = threadIdx.x;
        part[((size_t)b * NS + q) * gridDim.x + blockIdx.x] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

// one workgroup of 256: the partials added in a fixed order into s_tot[b][q] (LDS, SEG_MAXB * (3 SEG_MAXC + 2) doubles) and head[b][q];
// -> dice (not 1 - dice), in thread 0 only; the backward pools the batch in the same order
__device__ __forceinline__ double seg_totals_dice(const double* __restrict__ part, double* __restrict__ head, double* s_tot, int batch, int channels, int bot,
                                                  int top, int nblk, float eps, int batch_dice) {
    const int NS = seg_nstat(channels), nc = top - bot, total = batch * NS;
    __shared__ double s_p16[16][17];
    __shared__ double s_ratio[SEG_MAXB * SEG_MAXC];
    // 16 threads per statistic, each adding every 16th block's partial, 16 statistics per round; every order is fixed
    const int sl = threadIdx.x & 15, sg = threadIdx.x >> 4;
    for (int i0 = 0; i0 < total; i0 += 16) {
        const int i = i0 + sg;
        double t = 0.0;
        if (i < total) {
            const double* src = part + (size_t)i * nblk;
            int blk = sl;
            for (; blk + 7 * 16 < nblk; blk += 8 * 16) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = src[blk + 16 * u];
#pragma unroll
                for (int u = 0; u < 8; ++u) t += v[u];
            }
            for (; blk < nblk; blk += 16) t += src[blk];
        }
        s_p16[sg][sl] = t;
        __syncthreads();
        if (sl == 0 && i < total) {
            double tt = 0.0;
#pragma unroll
            for (int u = 0; u < 16; ++u) tt += s_p16[sg][u];
            s_tot[i] = tt;
            head[i] = tt;
        }
        __syncthreads();
    }
    const double e = (double)eps;
    const int nratio = batch_dice ? nc : batch * nc;
    for (int i = threadIdx.x; i < nratio; i += 256) {
        const int c = bot + i % nc;
        double S, I, T;
        if (batch_dice) {
            S = 0.0; I = 0.0; T = 0.0;
            for (int b = 0; b < batch; ++b) { S += s_tot[b * NS + c]; I += s_tot[b * NS + channels + c]; T += s_tot[b * NS + 2 * channels + c]; }
        } else {
            const int b = i / nc;
            S = s_tot[b * NS + c]; I = s_tot[b * NS + channels + c]; T = s_tot[b * NS + 2 * channels + c];
        }
        s_ratio[i] = 2.0 * I / (S + T + e);
    }
    __syncthreads();
    double dice = 0.0;
    if (threadIdx.x == 0) {
        if (batch_dice) {
            double m = 0.0;
            for (int ci = 0; ci < nc; ++ci) m += s_ratio[ci];
            dice = m / (double)nc;
        } else {
            double m = 0.0;
            for (int b = 0; b < batch; ++b) {
                double v = 0.0;
                for (int ci = 0; ci < nc; ++ci) v += s_ratio[b * nc + ci];
                m += v / (double)nc;
            }
            dice = m / (double)batch;
        }
    }
    return dice;
}

// dice_term = 1 - k sum 2 I/den  (k = 1/(B nc), den per sample; or k = 1/nc, den pooled)  =>  d/dp_c(v) = -k (2 [l = c]/den - 2 I/den^2) at a valid voxel:
// a2[c], plus a1[c] where l == c, times kd = gout * dice_w * k; 0 outside [bot, top)
template <int C>
__device__ __forceinline__ void seg_dice_coeffs(const double* __restrict__ head, int b, int batch, int bot, int top, float eps, double kd, int batch_dice,
                                                double (&a1)[C], double (&a2)[C]) {
    constexpr int NS = 3 * C + 2;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        a1[c] = 0.0; a2[c] = 0.0;
        if (c >= bot && c < top) {
            double S, I, T;
            if (batch_dice) {
                S = 0.0; I = 0.0; T = 0.0;
                for (int bb = 0; bb < batch; ++bb) { S += head[bb * NS + c]; I += head[bb * NS + C + c]; T += head[bb * NS + 2 * C + c]; }
            } else {
                S = head[b * NS + c]; I = head[b * NS + C + c]; T = head[b * NS + 2 * C + c];
            }
            const double den = S + T + (double)eps;
            a1[c] = -kd * 2.0 / den;
            a2[c] = kd * 2.0 * I / (den * den);
        }
    }
}

static int seg_args(const float* p, const float* label, const float* class_w, const void* scratch, int batch, int channels, long long voxels, int bot,
                    int top, float eps, float dice_w, float ce_w, float gamma, SegW& cw) {
    if (!p || !label || !class_w || !scratch) return VS_EINVAL;
    if (channels < 1 || channels > SEG_MAXC || batch <= 0 || voxels <= 0 || bot < 0 || top > channels || bot >= top) return VS_EINVAL;
    if (!(eps >= 0.f) || !(dice_w >= 0.f) || !(ce_w >= 0.f) || !(gamma >= 0.f)) return VS_EINVAL;              // NaN fails every comparison
    for (int c = 0; c < SEG_MAXC; ++c) {
        cw.w[c] = c < channels ? class_w[c] : 0.f;
        if (!(cw.w[c] >= 0.f)) return VS_EINVAL;
    }
    if (batch > SEG_MAXB || voxels >= (1ll << 31)) return VS_ESHAPE;
    if (voxels & 3) return VS_EALIGN;
    if (((uintptr_t)p & 15) || ((uintptr_t)label & 15) || ((uintptr_t)scratch & 7)) return VS_EALIGN;
    return VS_OK;
}

static unsigned seg_blocks(long long voxels) {
    long long blocks = (voxels / 4 + 255) / 256;
    return (unsigned)(blocks > SEG_BLOCKS ? SEG_BLOCKS : blocks);
}

#define SEG_DISPATCH_C(channels, CALL)                                                                                      \
    switch (channels) {                                                                                                     \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                     \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;                    \
    }
