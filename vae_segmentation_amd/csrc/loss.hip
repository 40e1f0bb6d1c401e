// Losses on planar fp32 probabilities: soft Dice, the weighted sum of Dice losses against several targets, BCE.
#include "common.h"
#include <math.h>

// ---- soft Dice ------------------------------------------------------------------------------------------
// grid (blocks, channel slot, b): float4 streaming over the voxels of one (b,c) plane; fp64 atomics per block.
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ s, const float* __restrict__ t, double* __restrict__ sums,
                                                        int channels, long long voxels, int bot) {
    const int c = bot + blockIdx.y, b = blockIdx.z;
    const float* sp = s + ((size_t)b * channels + c) * voxels;
    const float* tp = t + ((size_t)b * channels + c) * voxels;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const long long v4 = voxels / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
        const f32x4 x = *(const f32x4*)(sp + i * 4), y = *(const f32x4*)(tp + i * 4);
        a0 += (double)(x[0] * y[0] + x[1] * y[1]) + (double)(x[2] * y[2] + x[3] * y[3]);
        a1 += (double)(x[0] + x[1]) + (double)(x[2] + x[3]);
        a2 += (double)(y[0] + y[1]) + (double)(y[2] + y[3]);
    }
    __shared__ double red[4][3];
    a0 = wave_sum_d(a0); a1 = wave_sum_d(a1); a2 = wave_sum_d(a2);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a0; red[threadIdx.x >> 6][1] = a1; red[threadIdx.x >> 6][2] = a2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double tot = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        atomicAdd(sums + ((size_t)b * channels + c) * 3 + threadIdx.x, tot);
    }
}
__global__ void dice_finish_kernel(const double* __restrict__ sums, float* per_sample, float* mean_out, int batch, int channels, int bot, int top, float eps) {
    // single small block; thread b computes per-sample mean over channels
    __shared__ float ps[64];
    const int b = threadIdx.x;
    float v = 0.f;
    if (b < batch) {
        for (int c = bot; c < top; ++c) {
            const double* q = sums + ((size_t)b * channels + c) * 3;
            // fp32 arithmetic as torch does on the fp32 sums
            const float I = (float)q[0], S = (float)q[1], Tt = (float)q[2];
            v += 2.f * I / (S + Tt + eps);
        }
        v /= (float)(top - bot);
        if (per_sample) per_sample[b] = v;
        ps[b] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0 && mean_out) {
        float m = 0.f;
        for (int i = 0; i < batch; ++i) m += ps[i];
        mean_out[0] = m / batch;
    }
}
extern "C" int vs_dice_fwd(const float* s, const float* t, double* sums, float* per_sample, float* mean_out, int batch,
                           int channels, long long voxels, int bot, int top, float eps, void* stream) {
    if (!s || !t || !sums || batch <= 0 || batch > 64 || channels <= 0 || voxels <= 0 || bot < 0 || top > channels || bot >= top) return VS_EINVAL;
    if (((uintptr_t)s & 15) || ((uintptr_t)t & 15) || (voxels & 3)) return VS_EALIGN;
    hipError_t e = vs_zero_async(sums, sizeof(double) * 3 * batch * channels, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    long long blocks = (voxels / 4 + 256 * 8 - 1) / (256 * 8);
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    if (VS_DET_BUILD) blocks = 1;                      // deterministic mode: one block per (b, c) plane, so one fp64 atomic onto a zeroed word
    hipLaunchKernelGGL(dice_sums_kernel, dim3((unsigned)blocks, top - bot, batch), dim3(256), 0, (hipStream_t)stream, s, t, sums, channels, voxels, bot);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, per_sample, mean_out, batch, channels, bot, top, eps);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// d/ds_i [2I/(S+T+eps)] = 2 t_i/den - 2I/den^2 ; d/dt_i symmetric.  grid (blocks, channels, b)
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ s, const float* __restrict__ t, const double* __restrict__ sums,
                                                       const float* __restrict__ gout, int gout_is_mean, int batch,
                                                       float* __restrict__ gs, float* __restrict__ gt,
                                                       int channels, long long voxels, int bot, int top, float eps) {
    const int c = blockIdx.y, b = blockIdx.z;
    const size_t plane = ((size_t)b * channels + c) * voxels;
    const long long v4 = voxels / 4;
    if (c < bot || c >= top) {
        const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
            if (gs) *(f32x4*)(gs + plane + i * 4) = z;
            if (gt) *(f32x4*)(gt + plane + i * 4) = z;
        }
        return;
    }
    const double* q = sums + ((size_t)b * channels + c) * 3;
    const float I = (float)q[0], den = (float)q[1] + (float)q[2] + eps;
    const float g = (gout_is_mean ? gout[0] / (float)batch : gout[b]) / (float)(top - bot);
    const float k1 = g * 2.f / den, k2 = g * 2.f * I / (den * den);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
        if (gs) { const f32x4 y = *(const f32x4*)(t + plane + i * 4); *(f32x4*)(gs + plane + i * 4) = f32x4{k1 * y[0] - k2, k1 * y[1] - k2, k1 * y[2] - k2, k1 * y[3] - k2}; }
        if (gt) { const f32x4 x = *(const f32x4*)(s + plane + i * 4); *(f32x4*)(gt + plane + i * 4) = f32x4{k1 * x[0] - k2, k1 * x[1] - k2, k1 * x[2] - k2, k1 * x[3] - k2}; }
    }
}
extern "C" int vs_dice_bwd(const float* s, const float* t, const double* sums, const float* gout, int gout_is_mean, float* gs,
                           float* gt, int batch, int channels, long long voxels, int bot, int top, float eps, void* stream) {
    if (!s || !t || !sums || !gout || batch <= 0 || channels <= 0 || voxels <= 0 || (voxels & 3)) return VS_EINVAL;
    long long blocks = (voxels / 4 + 256 * 4 - 1) / (256 * 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(dice_bwd_kernel, dim3((unsigned)blocks, channels, batch), dim3(256), 0, (hipStream_t)stream, s, t, sums, gout, gout_is_mean, batch, gs, gt, channels, voxels, bot, top, eps);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- weighted sum of Dice losses, one source against k targets (one launch forward, one backward) -----------------
#define DICE_MULTI_MAX 4
struct DiceMulti {
    const float* s;
    const float* t[DICE_MULTI_MAX];
    const float* lab[DICE_MULTI_MAX];      // non-null: target j is the one-hot of these labels ([B][voxels] floats, truncated as vs_onehot does) — never materialised
    float* gt[DICE_MULTI_MAX];
    float w[DICE_MULTI_MAX];
    int k;
};
// scratch layout: sums[(j*B + b)*C + c][3] = (I_j, S, T_j), written by the finish kernel (the backward reads them); then
// the per-block partials part[((b*nc + ci)*NQ + q)*nblk + blk], q = 0: S, 1+2j: I_j, 2+2j: T_j.  No atomics: 27 ns per
// same-line fp64 atomic made a 432-block single-launch version (atomics + last-block ticket) cost 58 us; two small launches
// cost 12, and the fixed summation order makes the loss bitwise reproducible.
#define DICE_MULTI_BLOCKS 256
// four consecutive values of target j in channel c of sample b
__device__ __forceinline__ f32x4 dice_target4(const DiceMulti& a, int j, size_t plane, int b, int c, long long voxels, long long i) {
    if (a.lab[j] != nullptr) {
        const f32x4 l = *(const f32x4*)(a.lab[j] + (size_t)b * voxels + i * 4);
        return f32x4{(int)l[0] == c ? 1.f : 0.f, (int)l[1] == c ? 1.f : 0.f, (int)l[2] == c ? 1.f : 0.f, (int)l[3] == c ? 1.f : 0.f};
    }
    return *(const f32x4*)(a.t[j] + plane + i * 4);
}
__global__ __launch_bounds__(256) void dice_multi_partial_kernel(const DiceMulti a, double* __restrict__ part, int channels, long long voxels, int bot) {
    const int c = bot + blockIdx.y, b = blockIdx.z, K = a.k;
    const size_t plane = ((size_t)b * channels + c) * voxels;
    const float* sp = a.s + plane;
    double aS = 0.0, aI[DICE_MULTI_MAX], aT[DICE_MULTI_MAX];
#pragma unroll
    for (int j = 0; j < DICE_MULTI_MAX; ++j) { aI[j] = 0.0; aT[j] = 0.0; }
    const long long v4 = voxels / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
        const f32x4 x = *(const f32x4*)(sp + i * 4);
        aS += (double)(x[0] + x[1]) + (double)(x[2] + x[3]);
#pragma unroll
        for (int j = 0; j < DICE_MULTI_MAX; ++j) {
            if (j < K) {
                const f32x4 y = dice_target4(a, j, plane, b, c, voxels, i);
                aI[j] += (double)(x[0] * y[0] + x[1] * y[1]) + (double)(x[2] * y[2] + x[3] * y[3]);
                aT[j] += (double)(y[0] + y[1]) + (double)(y[2] + y[3]);
            }
        }
    }
    __shared__ double red[4][1 + 2 * DICE_MULTI_MAX];
    const int wave = threadIdx.x >> 6;
    aS = wave_sum_d(aS);
#pragma unroll
    for (int j = 0; j < DICE_MULTI_MAX; ++j) { aI[j] = wave_sum_d(aI[j]); aT[j] = wave_sum_d(aT[j]); }
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = aS;
#pragma unroll
        for (int j = 0; j < DICE_MULTI_MAX; ++j) { red[wave][1 + 2 * j] = aI[j]; red[wave][2 + 2 * j] = aT[j]; }
    }
    __syncthreads();
    const int NQ = 1 + 2 * K;
    if (threadIdx.x < NQ) {
        const int q = threadIdx.x;
        part[(((size_t)b * gridDim.y + blockIdx.y) * NQ + q) * gridDim.x + blockIdx.x] = red[0][q] + red[1][q] + red[2][q] + red[3][q];
    }
}

__global__ __launch_bounds__(256) void dice_multi_finish_kernel(const DiceMulti a, const double* __restrict__ part, double* __restrict__ sums,
                                                               float* __restrict__ terms, float* __restrict__ final_out, int batch,
                                                               int channels, int bot, int top, int nblk, float eps) {
    const int K = a.k, NQ = 1 + 2 * K, nc = top - bot;
    __shared__ double s_tot[64 * 2 * (1 + 2 * DICE_MULTI_MAX)];      // [b][ci][q], batch*nc <= 128 checked on the host
    __shared__ double s_p16[16][17];
    // 16 threads per statistic, each summing every 16th block (fixed order: reproducible), 16 statistics per round: the usual 10
    // statistics x 256 blocks are two rounds of 8 loads per thread instead of 32 dependent rounds in one thread
    const int sl = threadIdx.x & 15, sg = threadIdx.x >> 4;
    for (int i0 = 0; i0 < batch * nc * NQ; i0 += 16) {
        const int i = i0 + sg;
        double t = 0.0;
        if (i < batch * nc * NQ) {
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
        if (sl == 0 && i < batch * nc * NQ) {
            double tt = 0.0;
#pragma unroll
            for (int u = 0; u < 16; ++u) tt += s_p16[sg][u];
            s_tot[i] = tt;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < batch * nc * NQ; i += 256) {
        const double t = s_tot[i];
        const int q = i % NQ, bc = i / NQ, ci = bc % nc, b = bc / nc;
        if (q == 0) {
            for (int j = 0; j < K; ++j) sums[(((size_t)j * batch + b) * channels + bot + ci) * 3 + 1] = t;
        } else {
            const int j = (q - 1) >> 1;
            sums[(((size_t)j * batch + b) * channels + bot + ci) * 3 + (((q - 1) & 1) ? 2 : 0)] = t;
        }
    }
    __syncthreads();
    __shared__ float s_term[DICE_MULTI_MAX];
    if (threadIdx.x < K) {
        const int j = threadIdx.x;
        float m = 0.f;
        for (int b = 0; b < batch; ++b) {
            float v = 0.f;
            for (int ci = 0; ci < nc; ++ci) {
                const double* q = s_tot + (b * nc + ci) * NQ;
                // fp32 arithmetic as torch does on the fp32 sums
                const float I = (float)q[1 + 2 * j], S = (float)q[0], T = (float)q[2 + 2 * j];
                v += 2.f * I / (S + T + eps);
            }
            m += v / (float)nc;
        }
        const float term = 1.f - m / (float)batch;
        terms[j] = term;
        s_term[j] = term;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float f = __fmul_rn(a.w[0], s_term[0]);
        for (int j = 1; j < K; ++j) f = __fadd_rn(f, __fmul_rn(a.w[j], s_term[j]));
        final_out[0] = f;
    }
}

static int dice_multi_args(DiceMulti& a, const float* s, const float* const* t, const float* w, float* const* gt, int k, const float* const* lab = nullptr) {
    if (!s || !t || !w || k <= 0 || k > DICE_MULTI_MAX) return VS_EINVAL;
    a = DiceMulti{};
    a.s = s; a.k = k;
    if ((uintptr_t)s & 15) return VS_EALIGN;
    for (int j = 0; j < k; ++j) {
        const float* lj = lab ? lab[j] : nullptr;
        if (!t[j] && !lj) return VS_EINVAL;
        if (lj && gt && gt[j]) return VS_EINVAL;                 // a label target has no gradient
        if (((uintptr_t)t[j] & 15) || ((uintptr_t)lj & 15) || (gt && gt[j] && ((uintptr_t)gt[j] & 15))) return VS_EALIGN;
        a.t[j] = lj ? nullptr : t[j]; a.lab[j] = lj; a.w[j] = w[j]; a.gt[j] = gt ? gt[j] : nullptr;
    }
    return VS_OK;
}

extern "C" size_t vs_dice_loss_multi_scratch_doubles(int k, int batch, int channels) {
    if (k <= 0 || batch <= 0 || channels <= 0) return 0;
    return (size_t)3 * k * batch * channels + (size_t)batch * channels * (1 + 2 * k) * DICE_MULTI_BLOCKS;
}

extern "C" int vs_dice_loss_multi_fwd(const float* s, const float* const* t, const float* w, int k, double* scratch, float* terms,
                                      float* final_out, int batch, int channels, long long voxels, int bot, int top, float eps, void* stream) {
    return vs_dice_loss_multi_labels_fwd(s, t, nullptr, w, k, scratch, terms, final_out, batch, channels, voxels, bot, top, eps, stream);
}

extern "C" int vs_dice_loss_multi_labels_fwd(const float* s, const float* const* t, const float* const* labels, const float* w, int k, double* scratch,
                                             float* terms, float* final_out, int batch, int channels, long long voxels, int bot, int top, float eps,
                                             void* stream) {
    DiceMulti a;
    int rc = dice_multi_args(a, s, t, w, nullptr, k, labels);
    if (rc) return rc;
    if (!scratch || !terms || !final_out || batch <= 0 || batch > 64 || channels <= 0 || voxels <= 0 || bot < 0 || top > channels || bot >= top) return VS_EINVAL;
    if (voxels & 3) return VS_EALIGN;
    if ((long long)batch * (top - bot) > 128) return VS_ESHAPE;
    long long blocks = (voxels / 4 + 256 * 2 - 1) / (256 * 2);       // short loops: the launch is latency-, not bandwidth-bound
    if (blocks < 1) blocks = 1;
    if (blocks > DICE_MULTI_BLOCKS) blocks = DICE_MULTI_BLOCKS;
    double* part = scratch + (size_t)3 * k * batch * channels;
    hipLaunchKernelGGL(dice_multi_partial_kernel, dim3((unsigned)blocks, top - bot, batch), dim3(256), 0, (hipStream_t)stream, a, part, channels,
                       voxels, bot);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(dice_multi_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a, part, scratch, terms, final_out, batch, channels,
                       bot, top, (int)blocks, eps);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// final = sum_j w_j (1 - mean_{b,c} 2 I_j/(S+T_j+eps))  =>  d/ds_i = -sum_j w_j/(B*nc) (2 t_ji/den_j - 2 I_j/den_j^2), d/dt_ji symmetric
__global__ __launch_bounds__(256) void dice_multi_bwd_kernel(const DiceMulti a, const double* __restrict__ sums, const float* __restrict__ gout,
                                                            float* __restrict__ gs, int batch, int channels, long long voxels, int bot,
                                                            int top, float eps) {
    const int c = blockIdx.y, b = blockIdx.z, K = a.k;
    const size_t plane = ((size_t)b * channels + c) * voxels;
    const long long v4 = voxels / 4;
    if (c < bot || c >= top) {
        const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
            if (gs) *(f32x4*)(gs + plane + i * 4) = z;
#pragma unroll
            for (int j = 0; j < DICE_MULTI_MAX; ++j)
                if (j < K && a.gt[j]) *(f32x4*)(a.gt[j] + plane + i * 4) = z;
        }
        return;
    }
    float k1[DICE_MULTI_MAX], k2[DICE_MULTI_MAX], k2sum = 0.f;
    const float g0 = -gout[0] / ((float)batch * (float)(top - bot));
#pragma unroll
    for (int j = 0; j < DICE_MULTI_MAX; ++j) {
        k1[j] = 0.f; k2[j] = 0.f;
        if (j < K) {
            const double* q = sums + (((size_t)j * batch + b) * channels + c) * 3;
            const float I = (float)q[0], den = (float)q[1] + (float)q[2] + eps;
            const float g = g0 * a.w[j];
            k1[j] = g * 2.f / den;
            k2[j] = g * 2.f * I / (den * den);
            k2sum += k2[j];
        }
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
        const f32x4 x = *(const f32x4*)(a.s + plane + i * 4);
        f32x4 acc = f32x4{-k2sum, -k2sum, -k2sum, -k2sum};
#pragma unroll
        for (int j = 0; j < DICE_MULTI_MAX; ++j) {
            if (j < K) {
                if (gs) {
                    const f32x4 y = dice_target4(a, j, plane, b, c, voxels, i);
                    acc[0] += k1[j] * y[0]; acc[1] += k1[j] * y[1]; acc[2] += k1[j] * y[2]; acc[3] += k1[j] * y[3];
                }
                if (a.gt[j]) *(f32x4*)(a.gt[j] + plane + i * 4) = f32x4{k1[j] * x[0] - k2[j], k1[j] * x[1] - k2[j], k1[j] * x[2] - k2[j], k1[j] * x[3] - k2[j]};
            }
        }
        if (gs) *(f32x4*)(gs + plane + i * 4) = acc;
    }
}

extern "C" int vs_dice_loss_multi_bwd(const float* s, const float* const* t, const float* w, int k, const double* scratch, const float* gout,
                                      float* gs, float* const* gt, int batch, int channels, long long voxels, int bot, int top, float eps,
                                      void* stream) {
    return vs_dice_loss_multi_labels_bwd(s, t, nullptr, w, k, scratch, gout, gs, gt, batch, channels, voxels, bot, top, eps, stream);
}

extern "C" int vs_dice_loss_multi_labels_bwd(const float* s, const float* const* t, const float* const* labels, const float* w, int k,
                                             const double* scratch, const float* gout, float* gs, float* const* gt, int batch, int channels,
                                             long long voxels, int bot, int top, float eps, void* stream) {
    DiceMulti a;
    int rc = dice_multi_args(a, s, t, w, gt, k, labels);
    if (rc) return rc;
    if (!scratch || !gout || batch <= 0 || channels <= 0 || voxels <= 0 || (voxels & 3) || bot < 0 || top > channels || bot >= top) return VS_EINVAL;
    if (gs && ((uintptr_t)gs & 15)) return VS_EALIGN;
    long long blocks = (voxels / 4 + 256 * 4 - 1) / (256 * 4);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(dice_multi_bwd_kernel, dim3((unsigned)blocks, channels, batch), dim3(256), 0, (hipStream_t)stream, a, scratch, gout, gs,
                       batch, channels, voxels, bot, top, eps);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- BCE ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bce_sum_kernel(const float* __restrict__ p, const float* __restrict__ t, double* __restrict__ acc, long long count) {
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float lp = fmaxf(logf(p[i]), -100.f), lq = fmaxf(logf(1.f - p[i]), -100.f);
        s -= (double)(t[i] * lp + (1.f - t[i]) * lq);
    }
    __shared__ double red[4];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc, red[0] + red[1] + red[2] + red[3]);
}
__global__ void bce_finish_kernel(const double* acc, float* out, long long count) { out[0] = (float)(acc[0] / (double)count); }
__global__ void bce_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ gout, float* __restrict__ gp, long long count) {
    const float g = gout[0] / (float)count;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float d = fmaxf(p[i] * (1.f - p[i]), 1e-12f);
        gp[i] = g * (p[i] - t[i]) / d;
    }
}
extern "C" int vs_bce_fwd(const float* p, const float* t, float* out, double* scratch, long long count, void* stream) {
    if (!p || !t || !out || !scratch || count <= 0) return VS_EINVAL;
    hipError_t e = vs_zero_async(scratch, sizeof(double), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    long long blocks = (count + 256 * 16 - 1) / (256 * 16);
    if (blocks > 1024) blocks = 1024;
    if (VS_DET_BUILD) blocks = 1;                      // deterministic mode: a single block, a single atomic
    hipLaunchKernelGGL(bce_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, t, scratch, count);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, scratch, out, count);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
extern "C" int vs_bce_bwd(const float* p, const float* t, const float* gout, float* gp, long long count, void* stream) {
    if (!p || !t || !gout || !gp || count <= 0) return VS_EINVAL;
    hipLaunchKernelGGL(bce_bwd_kernel, GRID1D(count), dim3(256), 0, (hipStream_t)stream, p, t, gout, gp, count);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
