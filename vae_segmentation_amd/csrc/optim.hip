// The multi-tensor optimiser: SGD and Adam steps, the gradients' finite check, global norm and clip record, the loss-scale update, the EMA and the
// bucket staging copies.  Every *_multi kernel walks the same tables: one workgroup per chunk of VS_MT_CHUNK elements of one tensor.
#include "common.h"
#include <math.h>

// ---- the chunk walk ---------------------------------------------------------------------------------------------
// block_map holds {tensor index, first element} per workgroup (optim._Tables builds it with vs_mt_chunk()).  Two steps, so that each kernel keeps its
// loads where they stood: the pair first, the chunk's end on the line behind the pointer-table loads (sizes[ti] requested up front costs waits and SGPRs).
constexpr int MT_CHUNK = VS_MT_CHUNK;
static_assert(MT_CHUNK % 1024 == 0, "the f32x4 loops of the *_multi kernels cover a chunk in rounds of 256 threads x 4 elements");
extern "C" int vs_mt_chunk(void) { return MT_CHUNK; }
struct MtChunk { int ti, start; };
__device__ __forceinline__ MtChunk mt_chunk(const int* block_map) { return MtChunk{block_map[2 * blockIdx.x], block_map[2 * blockIdx.x + 1]}; }
__device__ __forceinline__ long long mt_chunk_end(const long long* sizes, int ti, int start) {
    const long long n = sizes[ti];
    return (long long)start + MT_CHUNK < n ? (long long)start + MT_CHUNK : n;
}

// ---- SGD ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgd_multi_kernel(float* const* params, const float* const* grads, float* const* bufs,
                                                        const long long* sizes, const int* block_map, float lr, float momentum,
                                                        float wd, int first, const float* __restrict__ loss_scale,
                                                        const float* __restrict__ found_inf, const float* __restrict__ hyper) {
    if (found_inf != nullptr && found_inf[0] != 0.f) return;          // a non-finite gradient somewhere: the whole step is skipped
    if (hyper != nullptr) { lr = hyper[0]; momentum = hyper[1]; wd = hyper[2]; }      // device-resident hyperparameters: a captured launch follows the schedule
    const float inv_scale = loss_scale != nullptr ? 1.f / loss_scale[0] : 1.f;
    const auto [ti, start] = mt_chunk(block_map);
    float* p = params[ti];
    const float* g = grads[ti];
    float* m = bufs[ti];
    const long long end = mt_chunk_end(sizes, ti, start);
    // every operand of the chunk is requested before the first store: the compiler cannot move a load over a store that may alias, and
    // sixteen dependent load -> store rounds made this 2.3 M-parameter update 25 us
    constexpr int R = MT_CHUNK / 256;
    if (end - start == MT_CHUNK && ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0)) {      // a full, 16-byte-aligned chunk (uniform): 12 vector loads instead of 48 dword loads (same 12.5 us: the update moves 49 MB at 3.9 TB/s either way)
        constexpr int R4 = R / 4;
        f32x4 g4[R4], p4[R4], m4[R4];
        const f32x4* gq = (const f32x4*)(g + start);
        f32x4* pq = (f32x4*)(p + start);
        f32x4* mq = (f32x4*)(m + start);
#pragma unroll
        for (int r = 0; r < R4; ++r) {
            const int i = threadIdx.x + r * 256;
            g4[r] = gq[i]; p4[r] = pq[i];
            m4[r] = first ? f32x4{0.f, 0.f, 0.f, 0.f} : mq[i];
        }
#pragma unroll
        for (int r = 0; r < R4; ++r) {
            const int i = threadIdx.x + r * 256;
            f32x4 bo, po;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gi = g4[r][e] * inv_scale + wd * p4[r][e];
                const float bi = first ? gi : momentum * m4[r][e] + gi;
                bo[e] = bi;
                po[e] = p4[r][e] - lr * (momentum != 0.f ? bi : gi);
            }
            mq[i] = bo; pq[i] = po;
        }
        return;
    }
    float gv[R], pv[R], mv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        const bool ok = i < end;
        gv[r] = ok ? g[i] : 0.f; pv[r] = ok ? p[i] : 0.f; mv[r] = (ok && !first) ? m[i] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        if (i < end) {
            const float gi = gv[r] * inv_scale + wd * pv[r];
            const float bi = first ? gi : momentum * mv[r] + gi;
            m[i] = bi;
            p[i] = pv[r] - lr * (momentum != 0.f ? bi : gi);
        }
    }
}
// The step of vs_sgd_step_*_multi (clip coefficient, Nesterov momentum): one element -> {momentum buffer, parameter}.  sgd_multi_kernel above is left to the
// compiler's contraction, and which products it fuses there moves with the code around them (templating that kernel flipped gi from fma(g, 1/S, wd*p) to
// fma(wd, p, g/S): other bits), so that kernel stays word for word what it was and this one is a kernel of its own with its contraction WRITTEN OUT:
//   t = wd*p;  gi = fma(g/S, coef, t);  bi = fma(momentum, m, gi);  p = fma(-lr, nesterov ? fma(momentum, bi, gi) : bi, p)
// With coef == 1 and no Nesterov momentum that is what sgd_multi_kernel compiles to whenever g/S is exact (no scaler, or a LossScaler's power-of-two scale),
// so a clip that never bites changes no bit (tests/test_gpu_optim_clip.py).
__device__ __forceinline__ f32x2 sgd_step1(float g, float p, float m, float lr, float momentum, float wd, float inv_scale, float coef, bool nesterov) {
#pragma clang fp contract(off)
    const float t = wd * p;
    const float gs = g * inv_scale;
    const float gi = __builtin_fmaf(gs, coef, t);
    const float bi = __builtin_fmaf(momentum, m, gi);
    const float ui = nesterov ? __builtin_fmaf(momentum, bi, gi) : bi;
    return f32x2{bi, __builtin_fmaf(-lr, momentum != 0.f ? ui : gi, p)};
}
__global__ __launch_bounds__(256) void sgd_step_multi_kernel(float* const* params, const float* const* grads, float* const* bufs,
                                                             const long long* sizes, const int* block_map, float lr, float momentum,
                                                             float wd, const float* __restrict__ loss_scale,
                                                             const float* __restrict__ found_inf, const float* __restrict__ hyper,
                                                             const float* __restrict__ clip_coef, int nesterov) {
    if (found_inf != nullptr && found_inf[0] != 0.f) return;          // a non-finite gradient somewhere: the whole step is skipped
    if (hyper != nullptr) { lr = hyper[0]; momentum = hyper[1]; wd = hyper[2]; nesterov = hyper[3] != 0.f; }      // device-resident hyperparameters
    const float coef = (clip_coef != nullptr) ? clip_coef[0] : 1.f;      // written by vs_grad_clip_finish earlier on this stream; x * 1 + t rounds once
    const float inv_scale = loss_scale != nullptr ? 1.f / loss_scale[0] : 1.f;
    const auto [ti, start] = mt_chunk(block_map);
    float* p = params[ti];
    const float* g = grads[ti];
    float* m = bufs[ti];
    const long long end = mt_chunk_end(sizes, ti, start);
    // every operand of the chunk is requested before the first store: the compiler cannot move a load over a store that may alias, and
    // sixteen dependent load -> store rounds made this 2.3 M-parameter update 25 us
    constexpr int R = MT_CHUNK / 256;
    if (end - start == MT_CHUNK && ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0)) {      // a full, 16-byte-aligned chunk (uniform): 12 vector loads instead of 48 dword loads (same 12.5 us: the update moves 49 MB at 3.9 TB/s either way)
        constexpr int R4 = R / 4;
        f32x4 g4[R4], p4[R4], m4[R4];
        const f32x4* gq = (const f32x4*)(g + start);
        f32x4* pq = (f32x4*)(p + start);
        f32x4* mq = (f32x4*)(m + start);
#pragma unroll
        for (int r = 0; r < R4; ++r) {
            const int i = threadIdx.x + r * 256;
            g4[r] = gq[i]; p4[r] = pq[i];
            m4[r] = mq[i];
        }
#pragma unroll
        for (int r = 0; r < R4; ++r) {
            const int i = threadIdx.x + r * 256;
            f32x4 bo, po;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f32x2 u = sgd_step1(g4[r][e], p4[r][e], m4[r][e], lr, momentum, wd, inv_scale, coef, nesterov != 0);
                bo[e] = u[0]; po[e] = u[1];
            }
            mq[i] = bo; pq[i] = po;
        }
        return;
    }
    float gv[R], pv[R], mv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        const bool ok = i < end;
        gv[r] = ok ? g[i] : 0.f; pv[r] = ok ? p[i] : 0.f; mv[r] = ok ? m[i] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        if (i < end) {
            const f32x2 u = sgd_step1(gv[r], pv[r], mv[r], lr, momentum, wd, inv_scale, coef, nesterov != 0);
            m[i] = u[0]; p[i] = u[1];
        }
    }
}
// The one launch of the SGD family.  ext: the written-out step (sgd_step_multi_kernel: clip coefficient, Nesterov momentum), else the plain one.
// hyper != NULL: the kernel reads its hyperparameters from device memory and ignores lr / momentum / wd / nesterov.
static int sgd_launch(bool ext, float* const* params, const float* const* grads, float* const* bufs, const long long* sizes, const int* block_map,
                      int n_blocks, float lr, float momentum, float wd, int first, int nesterov, const float* hyper, const float* clip_coef,
                      const float* loss_scale, const float* found_inf, void* stream) {
    if (!params || !grads || !bufs || !sizes || !block_map || n_blocks <= 0) return VS_EINVAL;
    if (ext)
        hipLaunchKernelGGL(sgd_step_multi_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, params, grads, bufs, sizes, block_map, lr, momentum,
                           wd, loss_scale, found_inf, hyper, clip_coef, nesterov);
    else
        hipLaunchKernelGGL(sgd_multi_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, params, grads, bufs, sizes, block_map, lr, momentum,
                           wd, first, loss_scale, found_inf, hyper);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
extern "C" int vs_sgd_momentum_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                                     const int* block_map, int n_blocks, float lr, float momentum, float weight_decay,
                                     int first_step, void* stream) {
    return sgd_launch(false, params, grads, bufs, sizes, block_map, n_blocks, lr, momentum, weight_decay, first_step, 0, nullptr, nullptr, nullptr, nullptr,
                      stream);
}
extern "C" int vs_sgd_momentum_scaled_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                                            const int* block_map, int n_blocks, float lr, float momentum, float weight_decay,
                                            int first_step, const float* loss_scale, const float* found_inf, void* stream) {
    return sgd_launch(false, params, grads, bufs, sizes, block_map, n_blocks, lr, momentum, weight_decay, first_step, 0, nullptr, nullptr, loss_scale,
                      found_inf, stream);
}
extern "C" int vs_sgd_momentum_dev_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                                         const int* block_map, int n_blocks, const float* hyper, const float* loss_scale,
                                         const float* found_inf, void* stream) {
    if (!hyper) return VS_EINVAL;
    return sgd_launch(false, params, grads, bufs, sizes, block_map, n_blocks, 0.f, 0.f, 0.f, 0, 0, hyper, nullptr, loss_scale, found_inf, stream);
}
// the step with Nesterov momentum and / or a clip coefficient (clip_coef -> clip[2] of vs_grad_clip_finish, NULL = no clipping).  Momentum buffers must exist
// and hold zeros before the first step.  Neither asked for: the launch of vs_sgd_momentum_scaled_multi.
extern "C" int vs_sgd_step_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                                 const int* block_map, int n_blocks, float lr, float momentum, float weight_decay, int nesterov,
                                 const float* clip_coef, const float* loss_scale, const float* found_inf, void* stream) {
    return sgd_launch(clip_coef || nesterov, params, grads, bufs, sizes, block_map, n_blocks, lr, momentum, weight_decay, 0, nesterov, nullptr, clip_coef,
                      loss_scale, found_inf, stream);
}
// hyper[4] = {lr, momentum, weight_decay, nesterov (0 / 1)} in DEVICE memory: the host cannot tell which step the record asks for, so this is always the
// written-out form (the same bits as the plain step when the record says no Nesterov momentum and clip_coef is NULL: sgd_step1)
extern "C" int vs_sgd_step_dev_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                                     const int* block_map, int n_blocks, const float* hyper, const float* clip_coef, const float* loss_scale,
                                     const float* found_inf, void* stream) {
    if (!hyper) return VS_EINVAL;
    return sgd_launch(true, params, grads, bufs, sizes, block_map, n_blocks, 0.f, 0.f, 0.f, 0, 0, hyper, clip_coef, loss_scale, found_inf, stream);
}

// ---- Adam ---------------------------------------------------------------------------------------------------------
template <bool CLIP>      // false: the step of vs_adam_multi / vs_adam_scaled_multi, expression for expression as it was
__global__ __launch_bounds__(256) void adam_multi_kernel(float* const* params, const float* const* grads, float* const* m1, float* const* m2,
                                                         const long long* sizes, const int* block_map, float lr, float b1, float b2,
                                                         float omb1, float omb2, float eps, float wd, float bc1, float bc2,
                                                         const float* __restrict__ loss_scale, const float* __restrict__ found_inf,
                                                         const float* __restrict__ clip_coef) {
    if (found_inf != nullptr && found_inf[0] != 0.f) return;
    const float inv_scale = loss_scale != nullptr ? 1.f / loss_scale[0] : 1.f;
    const float coef = CLIP ? clip_coef[0] : 1.f;                    // written by vs_grad_clip_finish earlier on this stream
    const auto [ti, start] = mt_chunk(block_map);
    float* p = params[ti];
    const float* g = grads[ti];
    float* a = m1[ti];
    float* v = m2[ti];
    const long long end = mt_chunk_end(sizes, ti, start);
    const float step_size = lr / bc1;
    const float bc2s = sqrtf(bc2);
    constexpr int R = MT_CHUNK / 256;                    // all loads of the chunk before the first store (see sgd_multi_kernel)
    float gv[R], pv[R], av[R], vv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        const bool ok = i < end;
        gv[r] = ok ? g[i] : 0.f; pv[r] = ok ? p[i] : 0.f; av[r] = ok ? a[i] : 0.f; vv[r] = ok ? v[i] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        if (i < end) {
            float gi;
            if constexpr (CLIP) gi = (gv[r] * inv_scale) * coef + wd * pv[r];
            else gi = gv[r] * inv_scale + wd * pv[r];
            const float ai = b1 * av[r] + omb1 * gi;                 // omb = 1 - beta formed in double on the host, as torch forms it
            const float vi = b2 * vv[r] + omb2 * gi * gi;
            a[i] = ai; v[i] = vi;
            const float denom = sqrtf(vi) / bc2s + eps;
            p[i] = pv[r] - step_size * ai / denom;
        }
    }
}
// The one launch of the Adam family; clip_coef NULL: the step without the coefficient.
static int adam_launch(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long long* sizes,
                       const int* block_map, int n_blocks, float lr, double beta1, double beta2, float eps, float weight_decay, int step,
                       const float* clip_coef, const float* loss_scale, const float* found_inf, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !sizes || !block_map || n_blocks <= 0 || step < 1) return VS_EINVAL;
    // betas arrive as doubles (python floats): 1 - beta and the bias corrections are formed in double, as torch.optim.Adam forms them
    const float bc1 = (float)(1.0 - pow(beta1, (double)step)), bc2 = (float)(1.0 - pow(beta2, (double)step));
    const auto kernel = clip_coef ? adam_multi_kernel<true> : adam_multi_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, sizes, block_map, lr, (float)beta1,
                       (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay, bc1, bc2, loss_scale, found_inf, clip_coef);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
extern "C" int vs_adam_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                             const long long* sizes, const int* block_map, int n_blocks, float lr, double beta1, double beta2,
                             float eps, float weight_decay, int step, void* stream) {
    return adam_launch(params, grads, exp_avg, exp_avg_sq, sizes, block_map, n_blocks, lr, beta1, beta2, eps, weight_decay, step, nullptr, nullptr, nullptr,
                       stream);
}
extern "C" int vs_adam_scaled_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                    const long long* sizes, const int* block_map, int n_blocks, float lr, double beta1, double beta2,
                                    float eps, float weight_decay, int step, const float* loss_scale, const float* found_inf, void* stream) {
    return adam_launch(params, grads, exp_avg, exp_avg_sq, sizes, block_map, n_blocks, lr, beta1, beta2, eps, weight_decay, step, nullptr, loss_scale,
                       found_inf, stream);
}
// vs_adam_scaled_multi with the gradient multiplied by clip_coef[0] after unscaling (clip[2] of vs_grad_clip_finish); NULL = vs_adam_scaled_multi itself
extern "C" int vs_adam_clip_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                  const long long* sizes, const int* block_map, int n_blocks, float lr, double beta1, double beta2,
                                  float eps, float weight_decay, int step, const float* clip_coef, const float* loss_scale, const float* found_inf,
                                  void* stream) {
    return adam_launch(params, grads, exp_avg, exp_avg_sq, sizes, block_map, n_blocks, lr, beta1, beta2, eps, weight_decay, step, clip_coef, loss_scale,
                       found_inf, stream);
}

// ---- dynamic loss scaling (fp16 storage: Dice gradients are O(1e-6), below fp16's normal range) ---------------------------------------
__global__ __launch_bounds__(256) void grad_finite_multi_kernel(const float* const* grads, const long long* sizes, const int* block_map,
                                                                float* __restrict__ found_inf) {
    const auto [ti, start] = mt_chunk(block_map);
    const float* g = grads[ti];
    const long long end = mt_chunk_end(sizes, ti, start);
    constexpr int R = MT_CHUNK / 256;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        const float v = i < end ? g[i] : 0.f;
        bad |= !(fabsf(v) <= 3.402823466e+38f);         // inf or nan
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) found_inf[0] = 1.f;       // same value from every writer: a benign race
}
extern "C" int vs_grad_finite_multi(const float* const* grads, const long long* sizes, const int* block_map, int n_blocks,
                                    float* found_inf, void* stream) {
    if (!grads || !sizes || !block_map || n_blocks <= 0 || !found_inf) return VS_EINVAL;
    hipLaunchKernelGGL(grad_finite_multi_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, grads, sizes, block_map, found_inf);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- global gradient norm and clip coefficient ------------------------------------------------------------------------------------------
// The norm must be the same bits on every data-parallel rank (each derives its coefficient from the all-reduced gradients on its own), so the sum has ONE
// order: per thread, per wave (wave_sum_d: a butterfly whose every lane ends with the same value), the four waves in wave order, the chunks in table order.
// No atomics, nothing to zero.  -> the workgroup's sum, valid on thread 0; lds: 4 doubles
__device__ __forceinline__ double block256_sum_d_ordered(double s, double* lds) {
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}
__global__ __launch_bounds__(256) void grad_sqnorm_multi_kernel(const float* const* grads, const long long* sizes, const int* block_map,
                                                                double* __restrict__ partials) {
    __shared__ double lds[4];
    const auto [ti, start] = mt_chunk(block_map);
    const float* g = grads[ti];
    const long long end = mt_chunk_end(sizes, ti, start);
    // thread t owns elements 4*(t + 256*r) + e of the chunk (r = 0..3, e = 0..3) and adds their squares in that order: the f32x4 a full aligned chunk
    // loads.  A ragged or misaligned chunk fetches the SAME elements with dword loads (zeros past the end: s + 0 = s), so the partial is a function of
    // the chunk's values alone, not of where the tensor happens to start
    constexpr int R4 = MT_CHUNK / 1024;
    f32x4 v[R4];
    if (end - start == MT_CHUNK && (((uintptr_t)g) & 15) == 0) {
        const f32x4* gq = (const f32x4*)(g + start);
#pragma unroll
        for (int r = 0; r < R4; ++r) v[r] = gq[threadIdx.x + r * 256];
    } else {
#pragma unroll
        for (int r = 0; r < R4; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long i = (long long)start + 4 * (threadIdx.x + r * 256) + e;
                v[r][e] = i < end ? g[i] : 0.f;
            }
    }
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < R4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double d = (double)v[r][e];
            s += d * d;                                  // an fp32 x fp32 product is exact in fp64 (fused or not: the same sum)
        }
    s = block256_sum_d_ordered(s, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
extern "C" int vs_grad_sqnorm_multi(const float* const* grads, const long long* sizes, const int* block_map, int n_blocks, double* partials,
                                    void* stream) {
    if (!grads || !sizes || !block_map || n_blocks <= 0 || !partials) return VS_EINVAL;
    hipLaunchKernelGGL(grad_sqnorm_multi_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, grads, sizes, block_map, partials);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
__global__ __launch_bounds__(256) void grad_clip_finish_kernel(const double* __restrict__ partials, int n_partials, float* __restrict__ clip,
                                                               const float* __restrict__ loss_scale) {
    __shared__ double lds[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) s += partials[i];
    s = block256_sum_d_ordered(s, lds);
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const float inv_scale = loss_scale != nullptr ? 1.f / loss_scale[0] : 1.f;
        const float norm = (float)(sqrt(s) * (double)inv_scale);
        const float c = clip[0] / (norm + 1e-6f);        // torch.nn.utils.clip_grad_norm_'s rule, in fp32
        clip[1] = norm;
        clip[2] = c < 1.f ? c : 1.f;                     // a NaN norm compares false: 1; an infinite norm: 0
    }
}
extern "C" int vs_grad_clip_finish(const double* partials, int n_partials, float* clip, const float* loss_scale, void* stream) {
    if (!partials || n_partials <= 0 || !clip) return VS_EINVAL;
    hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, clip, loss_scale);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- the loss scale's update (LossScaler.update) -----------------------------------------------------------------------
__global__ void loss_scale_update_kernel(float* scale, int* growth_tracker, float* found_inf, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (found_inf[0] != 0.f) {
        scale[0] *= backoff;
        growth_tracker[0] = 0;
    } else {
        const int t = growth_tracker[0] + 1;
        if (t >= interval) { scale[0] *= growth; growth_tracker[0] = 0; }
        else growth_tracker[0] = t;
    }
    found_inf[0] = 0.f;
}
extern "C" int vs_loss_scale_update(float* scale, int* growth_tracker, float* found_inf, float growth_factor, float backoff_factor,
                                    int growth_interval, void* stream) {
    if (!scale || !growth_tracker || !found_inf || growth_factor < 1.f || backoff_factor <= 0.f || backoff_factor > 1.f || growth_interval < 1)
        return VS_EINVAL;
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale, growth_tracker, found_inf, growth_factor,
                       backoff_factor, growth_interval);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- EMA teacher update; the scaled copies that stage gradients into and out of the data-parallel buckets ------------------------------
__global__ __launch_bounds__(256) void ema_multi_kernel(float* const* teacher, const float* const* student, const long long* sizes,
                                                        const int* block_map, float alpha) {
    const auto [ti, start] = mt_chunk(block_map);
    float* t = teacher[ti];
    const float* s = student[ti];
    const long long end = mt_chunk_end(sizes, ti, start);
    constexpr int R = MT_CHUNK / 256;                    // all loads of the chunk before the first store (see sgd_multi_kernel)
    float tv[R], sv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        tv[r] = i < end ? t[i] : 0.f; sv[r] = i < end ? s[i] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        if (i < end) t[i] = alpha * tv[r] + (1.f - alpha) * sv[r];
    }
}
extern "C" int vs_ema_multi(float* const* teacher, const float* const* student, const long long* sizes, const int* block_map,
                            int n_blocks, float alpha, void* stream) {
    if (!teacher || !student || !sizes || !block_map || n_blocks <= 0) return VS_EINVAL;
    hipLaunchKernelGGL(ema_multi_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, teacher, student, sizes, block_map, alpha);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

__global__ __launch_bounds__(256) void copy_scale_multi_kernel(const float* const* srcs, float* const* dsts, const long long* sizes,
                                                               const int* block_map, float scale) {
    const auto [ti, start] = mt_chunk(block_map);
    const float* s = srcs[ti];
    float* d = dsts[ti];
    const long long end = mt_chunk_end(sizes, ti, start);
    constexpr int R = MT_CHUNK / 256;                    // all loads of the chunk before the first store (see sgd_multi_kernel)
    float sv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        sv[r] = i < end ? s[i] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long i = start + threadIdx.x + r * 256;
        if (i < end) d[i] = sv[r] * scale;
    }
}
extern "C" int vs_copy_scale_multi(const float* const* srcs, float* const* dsts, const long long* sizes, const int* block_map,
                                   int n_blocks, float scale, void* stream) {
    if (!srcs || !dsts || !sizes || !block_map || n_blocks <= 0) return VS_EINVAL;
    hipLaunchKernelGGL(copy_scale_multi_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, srcs, dsts, sizes, block_map, scale);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

__global__ void scale_copy_kernel(const float* src, float* dst, long long n, float scale) {     // src may equal dst (in-place scale)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = src[i] * scale;
}
extern "C" int vs_scale_copy(const float* src, float* dst, long long count, float scale, void* stream) {
    if (!src || !dst || count <= 0) return VS_EINVAL;
    long long blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(scale_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, count, scale);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
