// Elastic deformation of the spatial augmentation on the device: the first stage of batchgenerators' augment_spatial, which data.hip's affine
// resampling left out.  Per sample
//     off[k] = scipy.ndimage.gaussian_filter(noise[k], sigma, mode="constant", cval=0) * alpha,   k = 0, 1, 2,   noise uniform in [-1, 1)
// is added to the zero-centred mesh before rotation and scale; sigma = 10..30 voxels, i.e. 81..241 taps per axis over three patch-sized fp64 fields.
//   vs_data_noise_philox   the noise, counter-based (Philox4x32-10): a pure function of (seed, sample, axis, voxel), no state, no host transfer
//   vs_data_elastic_field  the three separable passes of all three fields, fp64, zeros beyond the volume
//   vs_data_warp_sample    vs_data_affine_sample with the field added to the output coordinate (the sampler itself is data_sample.h's)
// The filter.  The weights are scipy's _gaussian_kernel1d, made on the host in fp64; the kernel is symmetric, so the half w[0..radius] — at most 129
// doubles, 1032 bytes — travels BY VALUE in the kernel arguments (the limit is 4096 bytes): no device table to allocate, upload or keep alive, the
// values are part of the launch and hence of a captured graph node.  The tap loop is uniform over the workgroup, so a weight is one scalar load from
// the argument segment (scalar cache) and feeds EL_A_PER / EL_X_PER multiply-adds; no kernel evaluates exp().
// A workgroup stages a tile of lines plus the halo its taps reach in LDS (zeros where the volume ends) and every thread walks the taps over it:
//   along z and y (not contiguous)  a tile of EL_TA = 64 positions along the axis x EL_TX = 32 contiguous elements (for z the (y, x) plane is one
//                                   contiguous run of h * w elements): every global load and store is a 256-byte row segment; thread (a, x) owns the
//                                   8 outputs a, a + 8, ... of its column, so a wave reads 64 consecutive doubles of LDS per tap: no bank conflict
//   along x (contiguous)            EL_XR = 8 lines x EL_XT = 128 outputs, thread (line, i) owns outputs i, i + 32, i + 64, i + 96
// The halo is clipped to the line: a tile stages only positions [p0 + klo, p0 + T + khi) with klo = max(-radius, -(last output of the tile)) and
// khi = min(radius, n - 1 - p0), so a line shorter than the radius costs its own length, not the radius; a line longer than a tile takes several
// tiles.  LDS is sized per launch: (T + 2 min(radius, n - 1)) rows.  No atomics, no memset, every output written exactly once by one thread in a
// fixed order of additions: the same bits on every run, in both builds of the library and under graph replay.
#include "common.h"
#include "data_sample.h"
#include "philox.h"
#include <math.h>

constexpr int EL_MAX_RADIUS = 128;
struct ElWeights { double w[EL_MAX_RADIUS + 1]; int radius; };       // w[k]: the weight of taps -k and +k

constexpr int EL_TA = 64, EL_TX = 32, EL_A_PER = EL_TA / 8;          // strided axes: 256 threads = 8 axis rows x 32 columns, 8 outputs each
constexpr int EL_XR = 8, EL_XT = 128, EL_X_PER = EL_XT / 32;         // contiguous axis: 256 threads = 8 lines x 32 lanes, 4 outputs each

// the block-uniform tap range of the tile whose outputs are [p0, p0 + tile) of a line of n
__device__ __forceinline__ void el_tap_range(int p0, int tile, int n, int radius, int& klo, int& khi) {
    const int plast = min(p0 + tile, n) - 1;
    klo = max(-radius, -plast);
    khi = min(radius, n - 1 - p0);
}

// src / dst: [outer][n][W] doubles, filtered along n.  blockIdx.x = (outer, axis tile, column tile), column tile fastest.
__global__ __launch_bounds__(256) void el_gauss_strided_kernel(const double* __restrict__ src, double* __restrict__ dst, int n, long long W, int n_xt,
                                                              int n_at, ElWeights g, double scale) {
    extern __shared__ __attribute__((aligned(16))) double el_tile[];
    long long b = blockIdx.x;
    const long long x0 = (b % n_xt) * EL_TX; b /= n_xt;
    const int p0 = (int)(b % n_at) * EL_TA;
    const long long base = (b / n_at) * (long long)n * W;
    int klo, khi;
    el_tap_range(p0, EL_TA, n, g.radius, klo, khi);
    const int rows = EL_TA + khi - klo;
    for (int idx = threadIdx.x; idx < rows * EL_TX; idx += 256) {
        const int a = p0 + klo + (idx >> 5);
        const long long x = x0 + (idx & 31);
        el_tile[idx] = (a >= 0 && a < n && x < W) ? src[base + (long long)a * W + x] : 0.0;
    }
    __syncthreads();
    const int ta = threadIdx.x >> 5, tx = threadIdx.x & 31;
    double acc[EL_A_PER];
#pragma unroll
    for (int j = 0; j < EL_A_PER; ++j) acc[j] = 0.0;
    for (int k = klo; k <= khi; ++k) {
        const double wk = g.w[k < 0 ? -k : k];
        const double* col = el_tile + (ta + k - klo) * EL_TX + tx;
#pragma unroll
        for (int j = 0; j < EL_A_PER; ++j) acc[j] = fma(wk, col[j * 8 * EL_TX], acc[j]);
    }
    const long long x = x0 + tx;
    if (x < W) {
#pragma unroll
        for (int j = 0; j < EL_A_PER; ++j) {
            const int a = p0 + ta + 8 * j;
            if (a < n) dst[base + (long long)a * W + x] = acc[j] * scale;
        }
    }
}

// src / dst: [lines][n] doubles, filtered along n.  blockIdx.x = (line tile, x tile), x tile fastest.
__global__ __launch_bounds__(256) void el_gauss_x_kernel(const double* __restrict__ src, double* __restrict__ dst, int n, long long lines, int n_xt,
                                                        ElWeights g, double scale) {
    extern __shared__ __attribute__((aligned(16))) double el_tile[];
    const int p0 = (int)(blockIdx.x % n_xt) * EL_XT;
    const long long line = (long long)(blockIdx.x / n_xt) * EL_XR + (threadIdx.x >> 5);
    int klo, khi;
    el_tap_range(p0, EL_XT, n, g.radius, klo, khi);
    const int pitch = EL_XT + khi - klo;
    const int i = threadIdx.x & 31;
    double* row = el_tile + (threadIdx.x >> 5) * pitch;
    const double* in = src + line * n;                         // dereferenced only where line < lines
    for (int c = i; c < pitch; c += 32) {
        const int x = p0 + klo + c;
        row[c] = (line < lines && x >= 0 && x < n) ? in[x] : 0.0;
    }
    __syncthreads();
    double acc[EL_X_PER];
#pragma unroll
    for (int j = 0; j < EL_X_PER; ++j) acc[j] = 0.0;
    for (int k = klo; k <= khi; ++k) {
        const double wk = g.w[k < 0 ? -k : k];
        const double* at = row + i + k - klo;
#pragma unroll
        for (int j = 0; j < EL_X_PER; ++j) acc[j] = fma(wk, at[32 * j], acc[j]);
    }
    if (line < lines) {
#pragma unroll
        for (int j = 0; j < EL_X_PER; ++j) {
            const int x = p0 + i + 32 * j;
            if (x < n) dst[line * n + x] = acc[j] * scale;
        }
    }
}

// ---- the noise: Philox4x32-10 (philox.h) ---------------------------------------------------------------------------------------------------------
// noise[axis][v] = 2 u - 1, u = ((w0 >> 5) 2^26 + (w1 >> 6)) / 2^53 of block (v lo, v hi, axis, sample lo) under key (seed lo, seed hi): every step exact in fp64
__global__ __launch_bounds__(256) void el_noise_kernel(double* __restrict__ noise, long long voxels, unsigned long long seed, unsigned int sample) {
    const long long total = 3 * voxels;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const unsigned int axis = (unsigned int)(i / voxels);
        const unsigned long long v = (unsigned long long)(i - (long long)axis * voxels);
        unsigned int w0, w1, w2, w3;
        vs_philox4x32_10((unsigned int)v, (unsigned int)(v >> 32), axis, sample, (unsigned int)seed, (unsigned int)(seed >> 32), w0, w1, w2, w3);
        const double u = ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) * 0x1p-53;
        noise[i] = 2.0 * u - 1.0;
    }
}

// ---- dp_affine_kernel (data.hip) with the displacement field[k][o] added to the zero-centred coordinate of output voxel o, before the matrix ----------
template <int ORDER>
__global__ __launch_bounds__(256) void el_warp_kernel(const void* __restrict__ src, float* __restrict__ dst, const double* __restrict__ field, DpAffine p,
                                                     float cval) {
    const long long total = (long long)p.pd * p.ph * p.pw;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % p.pw), oy = (int)((i / p.pw) % p.ph), oz = (int)(i / ((long long)p.pw * p.ph));
        const double uz = oz - (p.pd - 1) / 2.0 + field[i], uy = oy - (p.ph - 1) / 2.0 + field[total + i], ux = ox - (p.pw - 1) / 2.0 + field[2 * total + i];
        double cz, cy, cx;
        dp_affine_map(p, uz, uy, ux, cz, cy, cx);
        dst[i] = dp_sample<ORDER>(src, p, cz, cy, cx, cval);
    }
}

static inline bool el_dims_ok(int d, int h, int w) { return dp_dims_ok(d, h, w) && 3.0 * d * h * w < 2147483648.0; }      // the three fields index as one int

extern "C" int vs_data_noise_philox(double* noise, int d, int h, int w, unsigned long long seed, unsigned long long sample, void* stream) {
    if (!noise) return VS_EINVAL;
    if (!el_dims_ok(d, h, w)) return VS_ESHAPE;
    if ((uintptr_t)noise & 7) return VS_EALIGN;
    const long long voxels = (long long)d * h * w;
    hipLaunchKernelGGL(el_noise_kernel, dim3(dp_blocks(3 * voxels)), dim3(256), 0, (hipStream_t)stream, noise, voxels, seed, (unsigned int)sample);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_data_elastic_field(const double* noise, double* field, double* tmp, int d, int h, int w, double sigma, double alpha, void* stream) {
    if (!noise || !field || !tmp || noise == field || noise == tmp || field == tmp) return VS_EINVAL;
    if (!(sigma > 0.0) || !isfinite(sigma) || !isfinite(alpha) || 4.0 * sigma + 0.5 >= (double)(EL_MAX_RADIUS + 1)) return VS_EINVAL;
    if (!el_dims_ok(d, h, w)) return VS_ESHAPE;
    if (((uintptr_t)noise & 7) || ((uintptr_t)field & 7) || ((uintptr_t)tmp & 7)) return VS_EALIGN;
    ElWeights g{};
    g.radius = (int)(4.0 * sigma + 0.5);                                   // scipy.ndimage.gaussian_filter1d, truncate = 4
    double sum = 0.0;                                                      // scipy's _gaussian_kernel1d: exp(-0.5 / sigma^2 * k^2), divided by the sum
    for (int k = -g.radius; k <= g.radius; ++k) sum += exp(-0.5 / (sigma * sigma) * (double)(k * k));
    for (int k = 0; k <= g.radius; ++k) g.w[k] = exp(-0.5 / (sigma * sigma) * (double)(k * k)) / sum;
    static const hipError_t attr_err =
        hipFuncSetAttribute((const void*)el_gauss_strided_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (EL_TA + 2 * EL_MAX_RADIUS) * EL_TX * 8);
    if (attr_err != hipSuccess) return (int)attr_err;
    const hipStream_t st = (hipStream_t)stream;
    auto strided = [&](const double* src, double* dst, long long outer, int n, long long W) {      // blocks <= elements of the three fields < 2^31
        const int n_xt = (int)((W + EL_TX - 1) / EL_TX), n_at = (n + EL_TA - 1) / EL_TA;
        const size_t lds = (size_t)(EL_TA + 2 * (g.radius < n - 1 ? g.radius : n - 1)) * EL_TX * sizeof(double);
        hipLaunchKernelGGL(el_gauss_strided_kernel, dim3((unsigned int)(outer * n_at * n_xt)), dim3(256), lds, st, src, dst, n, W, n_xt, n_at, g, 1.0);
    };
    strided(noise, field, 3, d, (long long)h * w);                         // along z: the (y, x) plane is one contiguous run
    strided(field, tmp, 3LL * d, h, w);                                    // along y
    const long long lines = 3LL * d * h;
    const int n_xt = (w + EL_XT - 1) / EL_XT;
    const size_t lds = (size_t)EL_XR * (EL_XT + 2 * (g.radius < w - 1 ? g.radius : w - 1)) * sizeof(double);
    hipLaunchKernelGGL(el_gauss_x_kernel, dim3((unsigned int)((lines + EL_XR - 1) / EL_XR * n_xt)), dim3(256), lds, st, tmp, field, w, lines, n_xt, g, alpha);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_data_warp_sample(const void* src, float* dst, const double* field, int sd, int sh, int sw, int pd, int ph, int pw, const double* a9,
                                   const double* ctr3, int order, float cval, void* stream) {
    if (!src || !dst || !field || !a9 || !ctr3 || (order != 0 && order != 3)) return VS_EINVAL;
    if (!dp_dims_ok(sd, sh, sw) || !el_dims_ok(pd, ph, pw)) return VS_ESHAPE;
    if ((uintptr_t)field & 7) return VS_EALIGN;
    DpAffine p{};
    for (int i = 0; i < 9; ++i) p.a[i] = a9[i];            // HOST arrays
    for (int i = 0; i < 3; ++i) p.ctr[i] = ctr3[i];
    p.sd = sd; p.sh = sh; p.sw = sw; p.pd = pd; p.ph = ph; p.pw = pw;
    const int blocks = dp_blocks((long long)pd * ph * pw);
    if (order == 0) hipLaunchKernelGGL(el_warp_kernel<0>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, dst, field, p, cval);
    else hipLaunchKernelGGL(el_warp_kernel<3>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, dst, field, p, cval);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
