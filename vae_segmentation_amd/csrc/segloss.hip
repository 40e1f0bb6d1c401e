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
// The limits, the voxel loss, the block reduction, the totals and the Dice coefficients live in segloss.h: topk.hip uses them too.
#include "segloss.h"

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
    seg_store_partials<C>(aS, aI, aT, aN, aD, part, b);
}

// dice (not 1 - dice) from the totals tot[b][q]; the backward pools the batch in the same order
__global__ __launch_bounds__(256) void seg_finish_kernel(const double* __restrict__ part, double* __restrict__ head, float* __restrict__ terms,
                                                         float* __restrict__ final_out, int batch, int channels, int bot, int top, int nblk, float eps,
                                                         float dice_w, float ce_w, int batch_dice) {
    const int NS = seg_nstat(channels);
    __shared__ double s_tot[SEG_MAXB * (3 * SEG_MAXC + 2)];
    const double dice = seg_totals_dice(part, head, s_tot, batch, channels, bot, top, nblk, eps, batch_dice);
    if (threadIdx.x == 0) {
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
    seg_dice_coeffs<C>(head, b, batch, bot, top, eps, kd, batch_dice, a1, a2);
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
