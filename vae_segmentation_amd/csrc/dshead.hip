// Deep-supervision head: a 1x1x1 convolution of a coarse channels-last feature map, the softmax of its K logits and the compound segmentation loss of
// segloss.hip against the full-resolution label, picked at stride s — fused, so that neither logits nor probabilities are ever stored
// (include/vaeseg.h vs_ds_head_*).  The loss rule is 3.20's, unchanged, and its device functions are restated here (ds_pow, ds_focal,
// ds_focal_grad, the finish arithmetic): segloss.hip stays the device code it was.
//
//   label of coarse voxel (z, y, x) = fine label at (s z + s/2, s y + s/2, s x + s/2), read in place;  logit_k = b_k + sum_c W[k][c] f_c in fp32 over the
//   stored value of f;  p = softmax(logit), max-subtracted, fp32;  sums S, I, T, sum w f, sum w in fp64 over the valid voxels;
//   final = scale * ((dice_w * dice_term) + ce_w * ce_term).
//
// Forward = two launches.  ds_partial_kernel: a lane owns one coarse voxel per trip of a grid-stride loop and reads its fragment (C values, contiguous) in
// 16-byte loads, 8 channels at a time; W and b sit in LDS and are read at wave-uniform addresses (broadcasts).  fp64 sums per thread -> wave shuffles -> the
// four waves through LDS -> one ordinary store per statistic and workgroup.  ds_finish_kernel (one workgroup) adds the partials in a fixed order, leaves the
// per-sample totals at the head of scratch and writes terms and final.
// Backward = two launches.  ds_bwd_kernel recomputes p from the same fragment, forms dlogit (fp64 factors, as 3.20), writes df (rounded once to the storage
// type) and reduces dW = sum_v dlogit_k f_c through LDS: the workgroup stages its 256 fragments (32 channels at a time) and dlogits, then thread
// (slice, c) adds every (256 / CC)-th voxel's product for its channel c and all K rows into registers that live across the trips; at the end the slices
// are added in a fixed order and ONE partial per (output, workgroup) is stored.  ds_bwd_finish_kernel adds the partials (fp64, fixed order) into dW / db.
// The matrix cores were not used for this reduction: the product is K x 256 x C with K <= 8 — a 16-row MFMA tile would be at least half empty, the
// 16-bit tiles would round dlogit to 16 bits first (the accuracy gate is fp32's), and the LDS form costs less than the fragment loads it sits behind.
// No atomics, no memset, nothing allocated or read back; the deterministic build compiles the same code.
//
// p_l, w[l] and the per-channel factors are selected with compare chains over registers: a register array indexed with a runtime value would be put in
// scratch memory (hipcc reports 0 bytes of scratch for every instantiation below).
#include "common.h"

#define DS_MAXK 8
#define DS_MAXC 64
#define DS_BLOCKS 512                  // block cap of the partial and backward grids: 512 x 256 threads = 131072 coarse voxels per sweep of the grid-stride loop
#define DS_MAXB 64                     // ds_finish_kernel keeps batch * (3K + 2) totals in LDS
#define DS_GC 32                       // channels staged per pass of the backward's LDS reduction
#define DS_ROW (DS_GC + 4)             // floats between two voxels' staged fragments: 16-byte aligned, and 16 consecutive lanes' 16-byte stores fall in 16 different bank groups

struct DsW { float w[DS_MAXK]; };      // class weights, by value in the kernel arguments
struct DsGeom { int d, h, w, s; };     // the coarse volume and the stride

__host__ __device__ static inline int ds_nstat(int classes) { return 3 * classes + 2; }

// x^g in fp64 (g wave-uniform): 0, 1, 2 exact without the pow routine
__device__ __forceinline__ double ds_pow(double x, double g) {
    if (g == 0.0) return 1.0;
    if (g == 1.0) return x;
    if (g == 2.0) return x * x;
    return pow(x, g);
}
// f = -(1 - p)^gamma * max(ln p, -100) in fp64
__device__ __forceinline__ double ds_focal(double p, double gamma) {
    const double lg = fmax(log(p), -100.0);
    return gamma == 0.0 ? -lg : -(ds_pow(1.0 - p, gamma) * lg);
}
// df/dp of the same; the clamp is active iff p < e^-100 (segloss.hip seg_focal_grad says why the threshold is no rounding question)
__device__ __forceinline__ double ds_focal_grad(double p, double gamma) {
    const bool clamped = p >= 0.0 && p < 3.720075976020836e-44;
    const double dl = clamped ? 0.0 : 1.0 / p;
    if (gamma == 0.0) return -dl;
    const double om = 1.0 - p;
    if (om == 0.0) return 0.0;
    const double lg = clamped ? -100.0 : log(p);
    const double t = ds_pow(om, gamma - 1.0);
    return t * (gamma * lg - om * dl);
}

// 8 consecutive channels of one voxel: 16 bytes of a 16-bit type, 32 of fp32
template <typename T>
__device__ __forceinline__ void ds_load8(const T* p, float (&v)[8]) {
    if constexpr (sizeof(T) == 4) {
        const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
    } else {
        const u32x4 r = *(const u32x4*)p;
        frag_unpack(r, v, (T*)nullptr);
    }
}
template <typename T>
__device__ __forceinline__ void ds_store8(T* p, const float (&v)[8]) {
    if constexpr (sizeof(T) == 4) {
        *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
        *(f32x4*)(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
        *(u32x4*)p = frag_pack(v, (T*)nullptr);            // round to nearest even, once
    }
}

// W[K][C] and b[K] into LDS (every thread of the workgroup; the caller synchronises)
__device__ __forceinline__ void ds_stage_weights(const float* __restrict__ W, const float* __restrict__ bias, float* sW, float* sB, int K, int C) {
    for (int i = threadIdx.x; i < K * C; i += 256) sW[i] = W[i];
    if (threadIdx.x < K) sB[threadIdx.x] = bias[threadIdx.x];
}

// index of coarse voxel i's label in the sample's fine volume [s d][s h][s w]
__device__ __forceinline__ size_t ds_label_index(unsigned int i, const DsGeom g) {
    const unsigned int x = i % (unsigned int)g.w, r = i / (unsigned int)g.w;
    const unsigned int y = r % (unsigned int)g.h, z = r / (unsigned int)g.h;
    const unsigned int o = (unsigned int)g.s >> 1, s = (unsigned int)g.s;
    return ((size_t)(s * z + o) * (size_t)(s * g.h) + (s * y + o)) * (size_t)(s * g.w) + (s * x + o);
}

// p = softmax(b + W f) of one voxel, fp32: the fragment 8 channels at a time, the weights from LDS at uniform addresses
template <int K, typename T>
__device__ __forceinline__ void ds_probabilities(const T* __restrict__ fv, const float* sW, const float* sB, int C, float (&p)[K]) {
    float lg[K];
#pragma unroll
    for (int k = 0; k < K; ++k) lg[k] = sB[k];
    for (int c0 = 0; c0 < C; c0 += 8) {
        float x[8];
        ds_load8<T>(fv + c0, x);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const f32x4 w0 = *(const f32x4*)(sW + k * C + c0), w1 = *(const f32x4*)(sW + k * C + c0 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lg[k] = __builtin_fmaf(w0[j], x[j], lg[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) lg[k] = __builtin_fmaf(w1[j], x[4 + j], lg[k]);
        }
    }
    float m = lg[0];
#pragma unroll
    for (int k = 1; k < K; ++k) m = fmaxf(m, lg[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { p[k] = expf(lg[k] - m); sum += p[k]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] *= inv;
}

template <int K, typename T>
__global__ __launch_bounds__(256) void ds_partial_kernel(const T* __restrict__ f, const float* __restrict__ label, const float* __restrict__ W,
                                                         const float* __restrict__ bias, const DsW cw, double* __restrict__ part, int C, const DsGeom g,
                                                         float gamma_f) {
    __shared__ __attribute__((aligned(16))) float sW[DS_MAXK * DS_MAXC];
    __shared__ float sB[DS_MAXK];
    ds_stage_weights(W, bias, sW, sB, K, C);
    __syncthreads();
    const int b = blockIdx.y;
    const unsigned int vox = (unsigned int)g.d * g.h * g.w;
    const T* fb = f + (size_t)b * vox * C;
    const float* lb = label + (size_t)b * vox * g.s * g.s * g.s;
    const double gamma = (double)gamma_f;
    double aS[K], aI[K], aN = 0.0, aD = 0.0;
    int aT[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { aS[k] = 0.0; aI[k] = 0.0; aT[k] = 0; }
    for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < vox; i += gridDim.x * 256u) {
        const float lf = lb[ds_label_index(i, g)];
        float p[K];
        ds_probabilities<K, T>(fb + (size_t)i * C, sW, sB, C, p);
        // as seg_partial_kernel: an ignored voxel has class -1, adds 0 to S and takes p_l = 1, w = 0
        const bool valid = lf >= 0.f && lf < (float)K;
        const int l = valid ? (int)lf : -1;
        float pl = 1.f, wl = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool hit = l == k;
            aS[k] += valid ? (double)p[k] : 0.0;
            aI[k] += hit ? (double)p[k] : 0.0;
            aT[k] += hit ? 1 : 0;
            pl = hit ? p[k] : pl;
            wl = hit ? cw.w[k] : wl;
        }
        aN += (double)wl * ds_focal((double)pl, gamma);
        aD += (double)wl;
    }
    constexpr int NS = 3 * K + 2;
    __shared__ double red[4][NS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum_d(aS[k]), t = wave_sum_d(aI[k]), n = wave_sum_d((double)aT[k]);      // a count is exact in fp64
        if (lane == 0) { red[wave][k] = s; red[wave][K + k] = t; red[wave][2 * K + k] = n; }
    }
    aN = wave_sum_d(aN);
    aD = wave_sum_d(aD);
    if (lane == 0) { red[wave][3 * K] = aN; red[wave][3 * K + 1] = aD; }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int q = threadIdx.x;
        part[((size_t)b * NS + q) * gridDim.x + blockIdx.x] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

// the arithmetic of seg_finish_kernel, restated, with the level's weight: final = scale * ((dice_w * dice_term) + ce_w * ce_term)
__global__ __launch_bounds__(256) void ds_finish_kernel(const double* __restrict__ part, double* __restrict__ head, float* __restrict__ terms,
                                                        float* __restrict__ final_out, int batch, int classes, int bot, int top, int nblk, float eps,
                                                        float dice_w, float ce_w, int batch_dice, float scale) {
    const int NS = ds_nstat(classes), nc = top - bot, total = batch * NS;
    __shared__ double s_tot[DS_MAXB * (3 * DS_MAXK + 2)];
    __shared__ double s_p16[16][17];
    __shared__ double s_ratio[DS_MAXB * DS_MAXK];
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
            for (int b = 0; b < batch; ++b) { S += s_tot[b * NS + c]; I += s_tot[b * NS + classes + c]; T += s_tot[b * NS + 2 * classes + c]; }
        } else {
            const int b = i / nc;
            S = s_tot[b * NS + c]; I = s_tot[b * NS + classes + c]; T = s_tot[b * NS + 2 * classes + c];
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
        for (int b = 0; b < batch; ++b) { N += s_tot[b * NS + 3 * classes]; D += s_tot[b * NS + 3 * classes + 1]; }
        const float dterm = (float)(1.0 - dice), cterm = D > 0.0 ? (float)(N / D) : 0.f;
        terms[0] = dterm;
        terms[1] = cterm;
        final_out[0] = __fmul_rn(scale, __fadd_rn(__fmul_rn(dice_w, dterm), __fmul_rn(ce_w, cterm)));
    }
}

// gp by seg_bwd_kernel's factors (times scale), dlogit_k = p_k (gp_k - sum_j gp_j p_j) in fp64, df_c = sum_k W[k][c] dlogit_k in fp32;
// part[o][workgroup], o = k C + c for dW and K C + k for db: this workgroup's sums
template <int K, typename T>
__global__ __launch_bounds__(256) void ds_bwd_kernel(const T* __restrict__ f, const float* __restrict__ label, const float* __restrict__ W,
                                                     const float* __restrict__ bias, const DsW cw, const double* __restrict__ head,
                                                     const float* __restrict__ gout, T* __restrict__ df, float* __restrict__ part, int C, const DsGeom g,
                                                     int batch, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma_f,
                                                     float scale) {
    __shared__ __attribute__((aligned(16))) float sW[DS_MAXK * DS_MAXC];
    __shared__ float sB[DS_MAXK];
    __shared__ __attribute__((aligned(16))) float sF[256 * DS_ROW];       // the trip's fragments, one pass of up to 32 channels; at the end the slices' sums
    __shared__ __attribute__((aligned(16))) float sD[256 * DS_MAXK];      // the trip's dlogits
    __shared__ float sR[4][DS_MAXK];
    ds_stage_weights(W, bias, sW, sB, K, C);
    constexpr int NS = 3 * K + 2;
    const int b = blockIdx.y;
    const double gs = (double)gout[0] * (double)scale, gamma = (double)gamma_f;
    const double kd = gs * (double)dice_w / (batch_dice ? (double)(top - bot) : (double)batch * (double)(top - bot));
    double a1[K], a2[K];              // gp of a valid voxel in channel k: a2[k], plus a1[k] where l == k
#pragma unroll
    for (int k = 0; k < K; ++k) {
        a1[k] = 0.0; a2[k] = 0.0;
        if (k >= bot && k < top) {
            double S, I, Tc;
            if (batch_dice) {
                S = 0.0; I = 0.0; Tc = 0.0;
                for (int bb = 0; bb < batch; ++bb) { S += head[bb * NS + k]; I += head[bb * NS + K + k]; Tc += head[bb * NS + 2 * K + k]; }
            } else {
                S = head[b * NS + k]; I = head[b * NS + K + k]; Tc = head[b * NS + 2 * K + k];
            }
            const double den = S + Tc + (double)eps;
            a1[k] = -kd * 2.0 / den;
            a2[k] = kd * 2.0 * I / (den * den);
        }
    }
    double D = 0.0;
    for (int bb = 0; bb < batch; ++bb) D += head[bb * NS + 3 * K + 1];
    const double kc = D > 0.0 ? gs * (double)ce_w / D : 0.0;
    const bool with_ce = kc != 0.0;

    const unsigned int vox = (unsigned int)g.d * g.h * g.w;
    const T* fb = f + (size_t)b * vox * C;
    T* dfb = df + (size_t)b * vox * C;
    const float* lb = label + (size_t)b * vox * g.s * g.s * g.s;
    const int CC = C < DS_GC ? C : DS_GC;           // channels per pass; thread (slice, cc) of the reduction owns channel cc of every (256 / CC)-th voxel
    const int cc = threadIdx.x % CC, slice = threadIdx.x / CC, nsl = 256 / CC;
    float acc[2][K], adb[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { acc[0][k] = 0.f; acc[1][k] = 0.f; adb[k] = 0.f; }
    __syncthreads();                                                   // sW, sB staged

    for (unsigned int base = blockIdx.x * 256u; base < vox; base += gridDim.x * 256u) {     // uniform trip count: the body holds barriers
        const unsigned int i = base + threadIdx.x;
        const bool in = i < vox;
        const T* fv = fb + (size_t)i * C;
        float dl[K];
#pragma unroll
        for (int k = 0; k < K; ++k) dl[k] = 0.f;
        if (in) {
            const float lf = lb[ds_label_index(i, g)];
            float p[K];
            ds_probabilities<K, T>(fv, sW, sB, C, p);
            const bool valid = lf >= 0.f && lf < (float)K;
            const int l = valid ? (int)lf : -1;
            double hit = 0.0;                     // what the voxel's own channel gets on top of a2
            float pl = 0.5f, wl = 0.f;            // an ignored voxel or a class of weight 0: no cross-entropy part, whatever p_l is
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const bool own = l == k;
                hit = own ? a1[k] : hit;
                pl = own && cw.w[k] != 0.f ? p[k] : pl;
                wl = own ? cw.w[k] : wl;
            }
            if (with_ce) hit += kc * (double)wl * ds_focal_grad((double)pl, gamma);
            double gp[K], dot = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                gp[k] = l == k ? a2[k] + hit : a2[k];
                dot += gp[k] * (double)p[k];
            }
#pragma unroll
            for (int k = 0; k < K; ++k) dl[k] = valid ? (float)((double)p[k] * (gp[k] - dot)) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) adb[k] += dl[k];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if (pass * DS_GC < C) {                                    // uniform
                __syncthreads();                                       // the previous pass's readers are done with sF (and, pass 0, with sD; sW is staged)
                if (pass == 0) {
#pragma unroll
                    for (int k = 0; k < K; ++k) sD[threadIdx.x * DS_MAXK + k] = dl[k];
                }
                const int cend = C < (pass + 1) * DS_GC ? C : (pass + 1) * DS_GC;
                for (int c0 = pass * DS_GC; c0 < cend; c0 += 8) {
                    float x[8], o[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { x[j] = 0.f; o[j] = 0.f; }
                    if (in) ds_load8<T>(fv + c0, x);                   // the lines ds_probabilities has just read
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const f32x4 w0 = *(const f32x4*)(sW + k * C + c0), w1 = *(const f32x4*)(sW + k * C + c0 + 4);
#pragma unroll
                        for (int j = 0; j < 4; ++j) { o[j] = __builtin_fmaf(w0[j], dl[k], o[j]); o[4 + j] = __builtin_fmaf(w1[j], dl[k], o[4 + j]); }
                    }
                    if (in) ds_store8<T>(dfb + (size_t)i * C + c0, o);
                    float* dst = sF + threadIdx.x * DS_ROW + (c0 - pass * DS_GC);
                    *(f32x4*)dst = f32x4{x[0], x[1], x[2], x[3]};
                    *(f32x4*)(dst + 4) = f32x4{x[4], x[5], x[6], x[7]};
                }
                __syncthreads();
                for (int v = slice; v < 256; v += nsl) {
                    const float fx = sF[v * DS_ROW + cc];
#pragma unroll
                    for (int k = 0; k < K; ++k) acc[pass][k] = __builtin_fmaf(sD[v * DS_MAXK + k], fx, acc[pass][k]);
                }
            }
        }
    }
    // the slices' sums through LDS, added in slice order; db by wave shuffles and the four waves in a fixed order
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (pass * DS_GC < C) {
#pragma unroll
            for (int k = 0; k < K; ++k) sF[((pass * nsl + slice) * K + k) * CC + cc] = acc[pass][k];
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float t = wave_sum(adb[k]);
        if (lane == 0) sR[wave][k] = t;
    }
    __syncthreads();
    const size_t nparts = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    for (int o = threadIdx.x; o < K * C; o += 256) {
        const int k = o / C, c = o % C, pass = c / DS_GC, ci = c % DS_GC;
        float t = 0.f;
        for (int sl = 0; sl < nsl; ++sl) t += sF[((pass * nsl + sl) * K + k) * CC + ci];
        part[(size_t)o * nparts + blk] = t;
    }
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        part[(size_t)(K * C + k) * nparts + blk] = (sR[0][k] + sR[1][k]) + (sR[2][k] + sR[3][k]);
    }
}

// 16 outputs per workgroup, 16 threads per output, each adding every 16th workgroup's partial in fp64; rounded to fp32 once
__global__ __launch_bounds__(256) void ds_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ dW, float* __restrict__ db, int nw, int nout,
                                                            int nparts) {
    __shared__ double s_p16[16][17];
    const int sl = threadIdx.x & 15, sg = threadIdx.x >> 4, o = blockIdx.x * 16 + sg;
    double t = 0.0;
    if (o < nout) {
        const float* src = part + (size_t)o * nparts;
        for (int blk = sl; blk < nparts; blk += 16) t += (double)src[blk];
    }
    s_p16[sg][sl] = t;
    __syncthreads();
    if (sl == 0 && o < nout) {
        double tt = 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) tt += s_p16[sg][u];
        if (o < nw) dW[o] = (float)tt;
        else db[o - nw] = (float)tt;
    }
}

static int ds_args(const void* f, int dtype, const float* W, const float* bias, const float* label, const float* class_w, const void* scratch, int batch,
                   int classes, int channels, int d, int h, int w, int stride, int bot, int top, float eps, float dice_w, float ce_w, float gamma,
                   float scale, DsW& cw) {
    if (!f || !W || !bias || !label || !class_w || !scratch) return VS_EINVAL;
    if (classes < 1 || classes > DS_MAXK || bot < 0 || top > classes || bot >= top) return VS_EINVAL;
    if (stride != 2 && stride != 4 && stride != 8) return VS_EINVAL;
    if (!(eps >= 0.f) || !(dice_w >= 0.f) || !(ce_w >= 0.f) || !(gamma >= 0.f) || !(scale >= 0.f)) return VS_EINVAL;      // NaN fails every comparison
    for (int k = 0; k < DS_MAXK; ++k) {
        cw.w[k] = k < classes ? class_w[k] : 0.f;
        if (!(cw.w[k] >= 0.f)) return VS_EINVAL;
    }
    if (!vs_dtype_ok(dtype)) return VS_EDTYPE;
    if (channels != 8 && channels != 16 && channels != 32 && channels != 64) return VS_ESHAPE;
    if (batch <= 0 || d <= 0 || h <= 0 || w <= 0 || batch > DS_MAXB) return VS_ESHAPE;
    const long long plane = (long long)d * h;                          // each product is checked before the next factor: no overflow
    if (plane >= (1ll << 31) || plane * w >= (1ll << 31) || plane * w * batch >= (1ll << 31)) return VS_ESHAPE;
    if (((uintptr_t)f & 15) || ((uintptr_t)W & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)label & 3) || ((uintptr_t)scratch & 7)) return VS_EALIGN;
    return VS_OK;
}

static unsigned ds_blocks(long long vox) {
    const long long blocks = (vox + 255) / 256;
    return (unsigned)(blocks > DS_BLOCKS ? DS_BLOCKS : blocks);
}

// doubles of the forward's part of scratch: the totals, then the per-block partials
static size_t ds_fwd_doubles(int batch, int classes) { return (size_t)batch * ds_nstat(classes) * (1 + DS_BLOCKS); }

extern "C" size_t vs_ds_head_scratch_doubles(int batch, int classes, int channels) {
    if (batch <= 0 || classes < 1 || classes > DS_MAXK || channels < 1 || channels > DS_MAXC) return 0;
    const size_t bwd_floats = (size_t)classes * (channels + 1) * batch * DS_BLOCKS;       // one fp32 partial per (output, workgroup)
    return ds_fwd_doubles(batch, classes) + (bwd_floats + 1) / 2;
}

#define DS_DISPATCH_K(classes, CALL)                                                                                        \
    switch (classes) {                                                                                                      \
        case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break;                     \
        case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; default: CALL(8); break;                    \
    }

extern "C" int vs_ds_head_fwd(const void* feat, int dtype, const float* weight, const float* bias, const float* label, const float* class_w, double* scratch,
                              float* terms, float* final_out, int batch, int classes, int channels, int d, int h, int w, int stride, int bot, int top,
                              float eps, float dice_w, float ce_w, int batch_dice, float gamma, float scale, void* stream) {
    DsW cw;
    const int rc = ds_args(feat, dtype, weight, bias, label, class_w, scratch, batch, classes, channels, d, h, w, stride, bot, top, eps, dice_w, ce_w, gamma,
                           scale, cw);
    if (rc) return rc;
    if (!terms || !final_out) return VS_EINVAL;
    const unsigned blocks = ds_blocks((long long)d * h * w);
    double* part = scratch + (size_t)batch * ds_nstat(classes);
    const dim3 grid(blocks, batch);
    const DsGeom g{d, h, w, stride};
    hipStream_t st = (hipStream_t)stream;
    dispatch_t(dtype, [&](auto tag) {
        using T = TAG_T(tag);
#define DS_CALL(KK) hipLaunchKernelGGL((ds_partial_kernel<KK, T>), grid, dim3(256), 0, st, (const T*)feat, label, weight, bias, cw, part, channels, g, gamma)
        DS_DISPATCH_K(classes, DS_CALL)
#undef DS_CALL
    });
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(ds_finish_kernel, dim3(1), dim3(256), 0, st, part, scratch, terms, final_out, batch, classes, bot, top, (int)blocks, eps, dice_w, ce_w,
                       batch_dice ? 1 : 0, scale);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_ds_head_bwd(const void* feat, int dtype, const float* weight, const float* bias, const float* label, const float* class_w, double* scratch,
                              const float* gout, void* dfeat, float* dweight, float* dbias, int batch, int classes, int channels, int d, int h, int w,
                              int stride, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma, float scale, void* stream) {
    DsW cw;
    const int rc = ds_args(feat, dtype, weight, bias, label, class_w, scratch, batch, classes, channels, d, h, w, stride, bot, top, eps, dice_w, ce_w, gamma,
                           scale, cw);
    if (rc) return rc;
    if (!gout || !dfeat || !dweight || !dbias) return VS_EINVAL;
    if (((uintptr_t)dfeat & 15) || ((uintptr_t)gout & 3) || ((uintptr_t)dweight & 3) || ((uintptr_t)dbias & 3)) return VS_EALIGN;
    const unsigned blocks = ds_blocks((long long)d * h * w);
    float* part = (float*)(scratch + ds_fwd_doubles(batch, classes));
    const dim3 grid(blocks, batch);
    const DsGeom g{d, h, w, stride};
    const int bd = batch_dice ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    dispatch_t(dtype, [&](auto tag) {
        using T = TAG_T(tag);
#define DS_CALL(KK)                                                                                                                                        \
    hipLaunchKernelGGL((ds_bwd_kernel<KK, T>), grid, dim3(256), 0, st, (const T*)feat, label, weight, bias, cw, (const double*)scratch, gout, (T*)dfeat, part, \
                       channels, g, batch, bot, top, eps, dice_w, ce_w, bd, gamma, scale)
        DS_DISPATCH_K(classes, DS_CALL)
#undef DS_CALL
    });
    VS_CHECK_LAUNCH();
    const int nw = classes * channels, nout = nw + classes;
    hipLaunchKernelGGL(ds_bwd_finish_kernel, dim3((nout + 15) / 16), dim3(256), 0, st, (const float*)part, dweight, dbias, nw, nout, (int)(blocks * batch));
    VS_CHECK_LAUNCH();
    return VS_OK;
}
