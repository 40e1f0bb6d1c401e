// Compound segmentation loss against a label volume: soft Dice (per sample or pooled over the batch) + class-weighted, optionally focal, voxel-wise
// cross-entropy (include/vaeseg.h vs_seg_loss_*).  The rule is this library's own — neither the reference nor the oracle has one.
//
//   valid voxel: label >= 0 && label < C in fp32 (NaN fails both), class l = (int)label.  Every other voxel — the -1 of the quad padding, an ignore value
//   such as 255, NaN — is IGNORED: it adds to no sum, S included, and gets gradient 0 in every channel.  This deliberately differs from
//   vs_dice_loss_multi_labels_* (loss.hip), where a voxel whose label matches no class still counts in S.
//
// Forward = two launches.  seg_partial_kernel is voxel-major: a thread owns quads of voxels, loads the label quad and the C probability quads (16-byte loads,
// coalesced per plane), classifies each voxel once and updates 2C + 2 fp64 sums (S, I, sum w f, sum w) and C integer counts (T) — one read of p and one of the
// label serve every term, where dice_multi_partial_kernel walks the label once per channel.  Waves reduce by shuffles, the four waves through LDS, and one thread
// per statistic stores the block's partial.  seg_finish_kernel (one workgroup) adds the partials in a fixed order, leaves the totals at the head of scratch for
// the backward, and writes terms and final.  Backward = one launch that reads label and p and writes all C planes of gp as 16-byte stores.
// No atomics, no memset, nothing allocated or read back; the deterministic build compiles the same code.
//
// p_l and w[l] are selected with compare chains over registers: a register array indexed with a runtime value would be put in scratch memory.
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

template <int C>
__global__ __launch_bounds__(256) void seg_partial_kernel(const float* __restrict__ p, const float* __restrict__ label, const SegW cw,
                                                          double* __restrict__ part, long long voxels, float gamma_f) {
    const int b = blockIdx.y;
    const float* pb = p + (size_t)b * C * voxels;
    const float* lb = label + (size_t)b * voxels;
    const double gamma = (double)gamma_f;
    double aS[C], aI[C], aN = 0.0, aD = 0.0;
    int aT[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { aS[c] = 0.0; aI[c] = 0.0; aT[c] = 0; }
    const long long v4 = voxels / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
        const f32x4 l4 = *(const f32x4*)(lb + i * 4);
        f32x4 x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = *(const f32x4*)(pb + (size_t)c * voxels + i * 4);
        // straight-line code, selects instead of branches: the four voxels' logarithms are independent chains the scheduler can interleave.  An ignored voxel
        // has class -1 (it matches no channel), adds 0 to S and takes p_l = 1, w = 0: f = 0 * ... adds nothing either
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lf = l4[e];
            const bool valid = lf >= 0.f && lf < (float)C;
            const int l = valid ? (int)lf : -1;
            float pl = 1.f, wl = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float v = x[c][e];
                const bool hit = l == c;
                aS[c] += valid ? (double)v : 0.0;
                aI[c] += hit ? (double)v : 0.0;
                aT[c] += hit ? 1 : 0;
                pl = hit ? v : pl;
                wl = hit ? cw.w[c] : wl;
            }
            aN += (double)wl * seg_focal((double)pl, gamma);
            aD += (double)wl;
        }
    }
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

// dice (not 1 - dice) from the totals tot[b][q]; the backward pools the batch in the same order
__global__ __launch_bounds__(256) void seg_finish_kernel(const double* __restrict__ part, double* __restrict__ head, float* __restrict__ terms,
                                                         float* __restrict__ final_out, int batch, int channels, int bot, int top, int nblk, float eps,
                                                         float dice_w, float ce_w, int batch_dice) {
    const int NS = seg_nstat(channels), nc = top - bot, total = batch * NS;
    __shared__ double s_tot[SEG_MAXB * (3 * SEG_MAXC + 2)];
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
    if (threadIdx.x == 0) {
        double dice;
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
        double N = 0.0, D = 0.0;
        for (int b = 0; b < batch; ++b) { N += s_tot[b * NS + 3 * channels]; D += s_tot[b * NS + 3 * channels + 1]; }
        const float dterm = (float)(1.0 - dice), cterm = D > 0.0 ? (float)(N / D) : 0.f;
        terms[0] = dterm;
        terms[1] = cterm;
        final_out[0] = __fadd_rn(__fmul_rn(dice_w, dterm), __fmul_rn(ce_w, cterm));
    }
}

// dice_term = 1 - k sum 2 I/den  (k = 1/(B nc), den per sample; or k = 1/nc, den pooled)  =>  d/dp_c(v) = -k (2 [l = c]/den - 2 I/den^2) at a valid voxel;
// ce_term = N/D with D independent of p  =>  d/dp_l(v) = w_l f'(p_l) / D
template <int C>
__global__ __launch_bounds__(256) void seg_bwd_kernel(const float* __restrict__ p, const float* __restrict__ label, const SegW cw,
                                                      const double* __restrict__ head, const float* __restrict__ gout, float* __restrict__ gp, int batch,
                                                      long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice,
                                                      float gamma_f) {
    constexpr int NS = 3 * C + 2;
    const int b = blockIdx.y;
    const double g = (double)gout[0], gamma = (double)gamma_f;
    const double kd = g * (double)dice_w / (batch_dice ? (double)(top - bot) : (double)batch * (double)(top - bot));
    double a1[C], a2[C];              // the gradient of a valid voxel in channel c: a2[c], plus a1[c] where l == c
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
    double D = 0.0;
    for (int bb = 0; bb < batch; ++bb) D += head[bb * NS + 3 * C + 1];
    const double kc = D > 0.0 ? g * (double)ce_w / D : 0.0;
    const bool with_ce = kc != 0.0;

    const float* pb = p + (size_t)b * C * voxels;
    const float* lb = label + (size_t)b * voxels;
    float* gb = gp + (size_t)b * C * voxels;
    const long long v4 = voxels / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
        const f32x4 l4 = *(const f32x4*)(lb + i * 4);
        f32x4 x[C], o[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = *(const f32x4*)(pb + (size_t)c * voxels + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lf = l4[e];
            const bool valid = lf >= 0.f && lf < (float)C;
            const int l = valid ? (int)lf : -1;
            double hit = 0.0;                     // what the voxel's own channel gets on top of a2
            float pl = 0.5f, wl = 0.f;            // an ignored voxel or a class of weight 0: no cross-entropy part, whatever p_l is
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool own = l == c;
                hit = own ? a1[c] : hit;
                pl = own && cw.w[c] != 0.f ? x[c][e] : pl;
                wl = own ? cw.w[c] : wl;
            }
            if (with_ce) hit += kc * (double)wl * seg_focal_grad((double)pl, gamma);       // with_ce is uniform; the four voxels' chains are independent
#pragma unroll
            for (int c = 0; c < C; ++c) o[c][e] = valid ? (float)(l == c ? a2[c] + hit : a2[c]) : 0.f;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) *(f32x4*)(gb + (size_t)c * voxels + i * 4) = o[c];
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

extern "C" size_t vs_seg_loss_scratch_doubles(int batch, int channels) {
    if (batch <= 0 || channels < 1 || channels > SEG_MAXC) return 0;
    return (size_t)batch * seg_nstat(channels) * (1 + SEG_BLOCKS);
}

template <int C>
static void seg_launch_partial(dim3 grid, hipStream_t st, const float* p, const float* label, const SegW& cw, double* part, long long voxels, float gamma) {
    hipLaunchKernelGGL(seg_partial_kernel<C>, grid, dim3(256), 0, st, p, label, cw, part, voxels, gamma);
}
template <int C>
static void seg_launch_bwd(dim3 grid, hipStream_t st, const float* p, const float* label, const SegW& cw, const double* head, const float* gout, float* gp,
                           int batch, long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma) {
    hipLaunchKernelGGL(seg_bwd_kernel<C>, grid, dim3(256), 0, st, p, label, cw, head, gout, gp, batch, voxels, bot, top, eps, dice_w, ce_w, batch_dice, gamma);
}
#define SEG_DISPATCH_C(channels, CALL)                                                                                      \
    switch (channels) {                                                                                                     \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                     \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;                    \
    }

extern "C" int vs_seg_loss_fwd(const float* p, const float* label, const float* class_w, double* scratch, float* terms, float* final_out, int batch,
                               int channels, long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma,
                               void* stream) {
    SegW cw;
    const int rc = seg_args(p, label, class_w, scratch, batch, channels, voxels, bot, top, eps, dice_w, ce_w, gamma, cw);
    if (rc) return rc;
    if (!terms || !final_out) return VS_EINVAL;
    const unsigned blocks = seg_blocks(voxels);
    double* part = scratch + (size_t)batch * seg_nstat(channels);
    const dim3 grid(blocks, batch);
    hipStream_t st = (hipStream_t)stream;
#define SEG_CALL(CC) seg_launch_partial<CC>(grid, st, p, label, cw, part, voxels, gamma)
    SEG_DISPATCH_C(channels, SEG_CALL)
#undef SEG_CALL
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(256), 0, st, part, scratch, terms, final_out, batch, channels, bot, top, (int)blocks, eps, dice_w,
                       ce_w, batch_dice ? 1 : 0);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_seg_loss_bwd(const float* p, const float* label, const float* class_w, const double* scratch, const float* gout, float* gp, int batch,
                               int channels, long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma,
                               void* stream) {
    SegW cw;
    const int rc = seg_args(p, label, class_w, scratch, batch, channels, voxels, bot, top, eps, dice_w, ce_w, gamma, cw);
    if (rc) return rc;
    if (!gout || !gp) return VS_EINVAL;
    if ((uintptr_t)gp & 15) return VS_EALIGN;
    const dim3 grid(seg_blocks(voxels), batch);
    hipStream_t st = (hipStream_t)stream;
    const int bd = batch_dice ? 1 : 0;
#define SEG_CALL(CC) seg_launch_bwd<CC>(grid, st, p, label, cw, scratch, gout, gp, batch, voxels, bot, top, eps, dice_w, ce_w, bd, gamma)
    SEG_DISPATCH_C(channels, SEG_CALL)
#undef SEG_CALL
    VS_CHECK_LAUNCH();
    return VS_OK;
}
