// Per-voxel passes around the segmentation head: dropout, the softmax backward (2 classes) and the n-class softmax pass, label preparation.
#include "common.h"
#include <math.h>

// ---- dropout ---------------------------------------------------------------------------------------
template <typename T>
__global__ void dropout_kernel(const T* __restrict__ x, T* __restrict__ out, long long frags, float p, unsigned long long seed) {
    constexpr int EPL = ET<T>::EPL;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < frags; i += (long long)gridDim.x * blockDim.x) {
        float f[EPL];
        frag_unpack(*(const u32x4*)(x + i * EPL), f, (T*)nullptr);
#pragma unroll
        for (int j = 0; j < EPL; ++j) f[j] *= dropout_scale(seed, (unsigned long long)i * EPL + j, p);
        *(u32x4*)(out + i * EPL) = frag_pack(f, (T*)nullptr);
    }
}
extern "C" int vs_dropout(const void* x, void* out, long long count, float p, unsigned long long seed, int dtype, void* stream) {
    if (!x || !out || count <= 0 || p < 0.f || p >= 1.f) return VS_EINVAL;
    if (!vs_dtype_ok(dtype)) return VS_EDTYPE;
    const int epl = dtype == VS_F32 ? 4 : 8;
    if (count % epl) return VS_ESHAPE;
    const long long frags = count / epl;
    dispatch_t(dtype, [&](auto* tag) {
        using T = TAG_T(tag);
        hipLaunchKernelGGL(dropout_kernel<T>, GRID1D(frags), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)out, frags, p, seed);
    });
    VS_CHECK_LAUNCH();
    return VS_OK;
}

__global__ void dropout_mask_kernel(float* __restrict__ mask, long long count, float p, unsigned long long seed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x)
        mask[i] = dropout_scale(seed, (unsigned long long)i, p);
}
extern "C" int vs_dropout_mask(float* mask, long long count, float p, unsigned long long seed, void* stream) {
    if (!mask || count <= 0 || p < 0.f || p >= 1.f) return VS_EINVAL;
    hipLaunchKernelGGL(dropout_mask_kernel, GRID1D(count), dim3(256), 0, (hipStream_t)stream, mask, count, p, seed);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- softmax (2 classes) backward ----------------------------------------------------------------
template <typename T>
__global__ void softmax2_bwd_kernel(const float* __restrict__ prob, const float* __restrict__ gprob, const T* __restrict__ gcl, T* __restrict__ gl,
                                    long long voxels, int c_pad, long long total, float drop_p, unsigned long long drop_seed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / voxels, v = i - n * voxels;
        const float p0 = prob[(n * 2 + 0) * voxels + v], p1 = prob[(n * 2 + 1) * voxels + v];
        float g0 = 0.f, g1 = 0.f;
        if (gprob) { g0 = gprob[(n * 2 + 0) * voxels + v]; g1 = gprob[(n * 2 + 1) * voxels + v]; }
        if (gcl) {                  // + the gradient that arrived through the channels-last copy of the probabilities
            float f2[ET<T>::EPL];
            frag_unpack(*(const u32x4*)(gcl + i * c_pad), f2, (T*)nullptr);
            g0 += f2[0]; g1 += f2[1];
        }
        const float dot = p0 * g0 + p1 * g1;
        float f[ET<T>::EPL];
#pragma unroll
        for (int j = 0; j < ET<T>::EPL; ++j) f[j] = 0.f;
        f[0] = p0 * (g0 - dot);
        f[1] = p1 * (g1 - dot);
        if (drop_p > 0.f) {          // backward of the logit dropout fused into the out_block epilogue
            f[0] *= dropout_scale(drop_seed, ((unsigned long long)n * 2 + 0) * voxels + v, drop_p);
            f[1] *= dropout_scale(drop_seed, ((unsigned long long)n * 2 + 1) * voxels + v, drop_p);
        }
        T* o = gl + i * c_pad;
        *(u32x4*)o = frag_pack(f, (T*)nullptr);
        const u32x4 z = u32x4{0u, 0u, 0u, 0u};
        for (int c0 = ET<T>::EPL; c0 < c_pad; c0 += ET<T>::EPL) *(u32x4*)(o + c0) = z;
    }
}

extern "C" int vs_softmax2_bwd(const float* prob, const float* gprob, void* glogit, int n, long long voxels, int c_pad,
                               int dtype, void* stream) {
    return vs_softmax2_dropout_bwd(prob, gprob, glogit, n, voxels, c_pad, dtype, 0.f, 0ull, stream);
}

extern "C" int vs_softmax2_dropout_bwd(const float* prob, const float* gprob, void* glogit, int n, long long voxels, int c_pad,
                                       int dtype, float drop_p, unsigned long long drop_seed, void* stream) {
    if (!gprob) return VS_EINVAL;
    return vs_softmax2_cl_bwd(prob, gprob, nullptr, glogit, n, voxels, c_pad, dtype, drop_p, drop_seed, stream);
}

extern "C" int vs_softmax2_cl_bwd(const float* prob, const float* gprob, const void* gprob_cl, void* glogit, int n, long long voxels,
                                  int c_pad, int dtype, float drop_p, unsigned long long drop_seed, void* stream) {
    if (!prob || (!gprob && !gprob_cl) || !glogit || n <= 0 || voxels <= 0 || c_pad % 8 || c_pad <= 0) return VS_EINVAL;
    const long long total = (long long)n * voxels;
    if (!vs_dtype_ok(dtype)) return VS_EDTYPE;
    dispatch_t(dtype, [&](auto* tag) {
        using T = TAG_T(tag);
        hipLaunchKernelGGL(softmax2_bwd_kernel<T>, GRID1D(total), dim3(256), 0, (hipStream_t)stream, prob, gprob, (const T*)gprob_cl, (T*)glogit, voxels, c_pad, total, drop_p, drop_seed);
    });
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- softmax over n_class = 1..8 classes as its own pass ------------------------------------------
// The two-class case (every configuration BASELINE names) has the fused out_block epilogue; a label set with more structures
// (main_source.py:92-93: n_class = 1 + number of --pan_index entries) takes the plain 3x3x3 conv and these two kernels.
template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&f)[8]) {
    constexpr int EPL = ET<T>::EPL;
#pragma unroll
    for (int k = 0; k < 8 / EPL; ++k) {
        float part[EPL];
        frag_unpack(*(const u32x4*)(p + k * EPL), part, (T*)nullptr);
#pragma unroll
        for (int j = 0; j < EPL; ++j) f[k * EPL + j] = part[j];
    }
}
template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&f)[8]) {
    constexpr int EPL = ET<T>::EPL;
#pragma unroll
    for (int k = 0; k < 8 / EPL; ++k) {
        float part[EPL];
#pragma unroll
        for (int j = 0; j < EPL; ++j) part[j] = f[k * EPL + j];
        *(u32x4*)(p + k * EPL) = frag_pack(part, (T*)nullptr);
    }
}

template <typename T>
__global__ void softmaxn_fwd_kernel(const T* __restrict__ logits, float* __restrict__ prob, long long voxels, int c_pad, int nc, long long total,
                                    float drop_p, unsigned long long drop_seed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / voxels, v = i - n * voxels;
        float l[8];
        load8(logits + i * c_pad, l);
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (c < nc) {
                if (drop_p > 0.f) l[c] *= dropout_scale(drop_seed, ((unsigned long long)n * nc + c) * voxels + v, drop_p);
                mx = fmaxf(mx, l[c]);
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            l[c] = c < nc ? expf(l[c] - mx) : 0.f;
            sum += l[c];
        }
        const float inv = 1.f / sum;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < nc) prob[(n * nc + c) * voxels + v] = l[c] * inv;
    }
}

template <typename T>
__global__ void softmaxn_bwd_kernel(const float* __restrict__ prob, const float* __restrict__ gprob, T* __restrict__ gl, long long voxels, int c_pad, int nc,
                                    long long total, float drop_p, unsigned long long drop_seed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / voxels, v = i - n * voxels;
        float p[8], g[8], dot = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            p[c] = c < nc ? prob[(n * nc + c) * voxels + v] : 0.f;
            g[c] = c < nc ? gprob[(n * nc + c) * voxels + v] : 0.f;
            dot += p[c] * g[c];
        }
        float f[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            f[c] = p[c] * (g[c] - dot);
            if (drop_p > 0.f && c < nc) f[c] *= dropout_scale(drop_seed, ((unsigned long long)n * nc + c) * voxels + v, drop_p);
        }
        T* o = gl + i * c_pad;
        store8(o, f);
        const u32x4 z = u32x4{0u, 0u, 0u, 0u};
        for (int c0 = 8; c0 < c_pad; c0 += ET<T>::EPL) *(u32x4*)(o + c0) = z;
    }
}

static int softmaxn_check(const void* a, const void* b, int n, long long voxels, int c_pad, int n_class, int dtype, float drop_p) {
    if (!a || !b || n <= 0 || voxels <= 0 || drop_p < 0.f || drop_p >= 1.f) return VS_EINVAL;
    if (c_pad <= 0 || c_pad % 8 || n_class < 1 || n_class > 8) return VS_ESHAPE;
    if (!vs_dtype_ok(dtype)) return VS_EDTYPE;
    return VS_OK;
}

extern "C" int vs_softmax_cl_fwd(const void* logits, float* prob, int n, long long voxels, int c_pad, int n_class, int dtype, float drop_p,
                                 unsigned long long drop_seed, void* stream) {
    const int rc = softmaxn_check(logits, prob, n, voxels, c_pad, n_class, dtype, drop_p);
    if (rc) return rc;
    const long long total = (long long)n * voxels;
    dispatch_t(dtype, [&](auto* tag) {
        using T = TAG_T(tag);
        hipLaunchKernelGGL(softmaxn_fwd_kernel<T>, GRID1D(total), dim3(256), 0, (hipStream_t)stream, (const T*)logits, prob, voxels, c_pad, n_class, total, drop_p, drop_seed);
    });
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_softmax_cl_bwd(const float* prob, const float* gprob, void* glogit, int n, long long voxels, int c_pad, int n_class, int dtype,
                                 float drop_p, unsigned long long drop_seed, void* stream) {
    const int rc = softmaxn_check(prob, glogit, n, voxels, c_pad, n_class, dtype, drop_p);
    if (rc) return rc;
    if (!gprob) return VS_EINVAL;
    const long long total = (long long)n * voxels;
    dispatch_t(dtype, [&](auto* tag) {
        using T = TAG_T(tag);
        hipLaunchKernelGGL(softmaxn_bwd_kernel<T>, GRID1D(total), dim3(256), 0, (hipStream_t)stream, prob, gprob, (T*)glogit, voxels, c_pad, n_class, total, drop_p, drop_seed);
    });
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- one-hot / binarize ---------------------------------------------------------------------------
__global__ void onehot_kernel(const float* __restrict__ label, float* __restrict__ out, long long voxels, int n_class, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / voxels, v = i - n * voxels;
        const int k = (int)label[i];          // .long() truncation, as label.type(LongTensor)
        for (int c = 0; c < n_class; ++c) out[(n * n_class + c) * voxels + v] = c == k ? 1.f : 0.f;
    }
}
extern "C" int vs_onehot(const float* label, float* out, int n, long long voxels, int n_class, void* stream) {
    if (!label || !out || n <= 0 || voxels <= 0 || n_class <= 0) return VS_EINVAL;
    const long long total = (long long)n * voxels;
    hipLaunchKernelGGL(onehot_kernel, GRID1D(total), dim3(256), 0, (hipStream_t)stream, label, out, voxels, n_class, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// argmax over the channel axis of a planar (n, c, voxels) tensor -> its one-hot, the hard masks of the validation Dice (utils/evaluation.py:58-64:
// torch.argmax -> scatter_).  Ties go to the FIRST maximal channel, as torch.argmax resolves them; a NaN channel wins (as torch's max does).
__global__ void hard_onehot_kernel(const float* __restrict__ x, float* __restrict__ out, long long voxels, int c, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / voxels, v = i - b * voxels;
        const float* xp = x + (size_t)b * c * voxels + v;
        float best = xp[0];
        int arg = 0;
        for (int k = 1; k < c; ++k) {
            const float val = xp[(size_t)k * voxels];
            if (val > best || (val != val && best == best)) { best = val; arg = k; }
        }
        float* op = out + (size_t)b * c * voxels + v;
        for (int k = 0; k < c; ++k) op[(size_t)k * voxels] = k == arg ? 1.f : 0.f;
    }
}
extern "C" int vs_hard_onehot(const float* x, float* out, int n, int n_class, long long voxels, void* stream) {
    if (!x || !out || n <= 0 || voxels <= 0 || n_class <= 0) return VS_EINVAL;
    const long long total = (long long)n * voxels;
    hipLaunchKernelGGL(hard_onehot_kernel, GRID1D(total), dim3(256), 0, (hipStream_t)stream, x, out, voxels, n_class, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

__global__ void binarize_kernel(const float* __restrict__ a, float* __restrict__ out, long long count, int mode, float lo, float hi) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x) {
        const float v = a[i];
        float r;
        if (mode == 0) r = v >= 0.5f ? 1.f : 0.f;
        else r = v > hi ? 1.f : (v < lo ? 0.f : v);
        out[i] = r;
    }
}
extern "C" int vs_binarize(const float* a, float* out, long long count, int mode, float lo, float hi, void* stream) {
    if (!a || !out || count <= 0) return VS_EINVAL;
    hipLaunchKernelGGL(binarize_kernel, GRID1D(count), dim3(256), 0, (hipStream_t)stream, a, out, count, mode, lo, hi);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
