// Zoom with edge boundaries: scipy.ndimage.zoom(x.astype(float64), out / in, order, mode="nearest", grid_mode=True) of one fp32 volume (d, h, w),
// optionally clipped to the input's range, rounded to fp32 once — the building block of nnU-Net's simulated low resolution (DESIGN 3.17 holds the rules).
//   coordinate   output index o of an axis of input length m and output length n reads c = (o + 0.5) zoom - 0.5, zoom = m / n ONE fp64 division (host)
//   order 0      floor(c + 0.5); always inside the axis
//   order 1      c clamped to [0, m - 1], two taps per axis, the upper one clamped to m - 1; the eight products summed in fp64
//   order 3      one pass per axis, z, then y, then x.  A pass pads each line by LR_PAD = 12 edge values on both sides, runs scipy's order-3 recursion with
//                the mirror start over the padded line (pole sqrt(3) - 2, gain 6, the causal start summed over the whole line) and evaluates the four
//                B-spline taps of every output at c + 12, all in fp64.  Padding a line with its edge values commutes with a linear operation along another
//                axis, so the three passes compute what scipy's three-dimensional evaluation of the padded, prefiltered volume computes.
// An order-3 pass: one workgroup of 256 threads owns a BUNDLE of L lines and keeps them in LDS as fp64 [position][line] (pitch P doubles), so the padded
// line is never written to memory.
//   load       z, y: the lines of a bundle are L consecutive values of the contiguous inner index; thread t = (g, lane) reads positions g, g + 256 / L, ...
//              of line `lane`: a wave reads 64 / L runs of L consecutive elements.  x: the L lines of a bundle are one contiguous run of L m elements,
//              read with the flat index and transposed on the LDS write; P = L + 1 makes consecutive positions of one line land 2 (L + 1) dwords
//              apart, on distinct banks.
//   prefilter  thread `lane` < L runs the serial recursion of its line; lanes read consecutive doubles of one row: distinct banks
//   evaluate   all 256 threads again: z, y as the load; x with the flat output index, so the store is one contiguous run of L n elements
// The B-spline weights of the n outputs are the same for every line: the workgroup computes them once, [n][4] fp64 behind the lines.
// L is the largest of 64, 32, 16, 8 for which lines and weights, ((m + 24) (L + 1) + 4 n) 8 bytes, fit 80 KiB: at least two workgroups (eight waves) per
// CU at every length up to 512; 64 lines up to 128 -> 64 or 64 -> 128, 32 at 128 -> 128, 8 at 512 -> 512.  The x pass clamps to the record's [min, max] when asked and rounds to fp32; the passes before it store fp64.
// Clip bounds: the record vs_aug_stats makes of x (its two launches), read on the device.  No atomics, no memset, nothing read back.
// Compiled without floating-point contraction: products and sums round separately, as scipy's C and the numpy restatement of the tests write them.
#include "common.h"
#include "data_sample.h"
#include <math.h>
#pragma clang fp contract(off)

constexpr int LR_PAD = 12, LR_THREADS = 256, LR_MAX_LEN = 512;
constexpr int LR_LDS = 80 * 1024;
constexpr double LR_POLE = -0.26794919243112270647;                       // sqrt(3) - 2

struct LrPass {
    int m, n, inner;                   // input and output length of the axis; the number of contiguous elements between two positions of a line
    int lines, lanes, pitch;           // lines of the volume; L; P
    double zoom, zn1;                  // m / n; pole^(m + 23)
    int clip;
};

// the LDS of a workgroup that holds l lines of input length m and the weights of n outputs; the lines it holds: the most that fit LR_LDS
static inline size_t lr_lds_bytes(int m, int n, int pitch) { return ((size_t)(m + 2 * LR_PAD) * pitch + 4 * (size_t)n) * sizeof(double); }
static inline int lr_lanes(int m, int n) {
    for (int l = 64; l > 8; l >>= 1)
        if (lr_lds_bytes(m, n, l + 1) <= (size_t)LR_LDS) return l;
    return 8;
}

__device__ __forceinline__ double lr_coord(int o, double zoom) { return ((double)o + 0.5) * zoom - 0.5; }

// scipy's apply_filter for order 3 with the mirror start, in place on c[0], c[pitch], ..., c[(n - 1) pitch]; the gain is applied by the load.
// The recursion is serial, its LDS reads are not: each loop takes LR_BLK positions into registers first and then runs the dependent chain over them, so
// the chain waits for arithmetic, not for LDS.  The operations and their order are those of the plain loops.
constexpr int LR_BLK = 8;
__device__ __forceinline__ void lr_prefilter(double* __restrict__ c, int pitch, int n, double zn1) {
    const double z = LR_POLE;
    double s = c[0] + zn1 * c[(n - 1) * pitch], zi = z;
    int i = 1;
    for (; i + LR_BLK <= n - 1; i += LR_BLK) {                             // the causal start: the sum over the whole (mirrored) line
        double a[LR_BLK], b[LR_BLK];
#pragma unroll
        for (int k = 0; k < LR_BLK; ++k) { a[k] = c[(i + k) * pitch]; b[k] = c[(n - 1 - i - k) * pitch]; }
#pragma unroll
        for (int k = 0; k < LR_BLK; ++k) { s = s + zi * (a[k] + zn1 * b[k]); zi = zi * z; }
    }
    for (; i < n - 1; ++i) { s = s + zi * (c[i * pitch] + zn1 * c[(n - 1 - i) * pitch]); zi = zi * z; }
    double prev = s / (1.0 - zn1 * zn1);
    c[0] = prev;
    for (i = 1; i + LR_BLK <= n; i += LR_BLK) {                            // causal
        double a[LR_BLK];
#pragma unroll
        for (int k = 0; k < LR_BLK; ++k) a[k] = c[(i + k) * pitch];
#pragma unroll
        for (int k = 0; k < LR_BLK; ++k) { prev = a[k] + z * prev; a[k] = prev; }
#pragma unroll
        for (int k = 0; k < LR_BLK; ++k) c[(i + k) * pitch] = a[k];
    }
    for (; i < n; ++i) { prev = c[i * pitch] + z * prev; c[i * pitch] = prev; }
    prev = (z * c[(n - 2) * pitch] + prev) * z / (z * z - 1.0);
    c[(n - 1) * pitch] = prev;
    for (i = n - 2; i - LR_BLK + 1 >= 0; i -= LR_BLK) {                    // anticausal
        double a[LR_BLK];
#pragma unroll
        for (int k = 0; k < LR_BLK; ++k) a[k] = c[(i - k) * pitch];
#pragma unroll
        for (int k = 0; k < LR_BLK; ++k) { prev = z * (prev - a[k]); a[k] = prev; }
#pragma unroll
        for (int k = 0; k < LR_BLK; ++k) c[(i - k) * pitch] = a[k];
    }
    for (; i >= 0; --i) { prev = z * (prev - c[i * pitch]); c[i * pitch] = prev; }
}

// the four B-spline weights of output o, scipy's form; the same for every line of a pass, so a workgroup computes them once into LDS (three fp64
// divisions per output, which would otherwise be most of the evaluation's arithmetic)
__device__ __forceinline__ void lr_weights(int o, double zoom, double* __restrict__ w) {
    const double cc = lr_coord(o, zoom) + (double)LR_PAD, t = cc - floor(cc), u = 1.0 - t;
    const double w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0, w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0, w0 = u * u * u / 6.0;
    w[0] = w0; w[1] = w1; w[2] = w2; w[3] = 1.0 - w0 - w1 - w2;
}

// the four taps of output o on the prefiltered padded line
__device__ __forceinline__ double lr_eval(const double* __restrict__ c, int pitch, int n_pad, int o, double zoom, const double* __restrict__ w) {
    const int start = min(max((int)floor(lr_coord(o, zoom) + (double)LR_PAD) - 1, 0), n_pad - 4);      // 10 <= start <= m + 10 by the rule; the clamp only guards the LDS
    const double* a = c + start * pitch;
    double acc = 0.0;
    acc = acc + w[0] * a[0]; acc = acc + w[1] * a[pitch]; acc = acc + w[2] * a[2 * pitch]; acc = acc + w[3] * a[3 * pitch];
    return acc;
}

// blockIdx.x = bundle.  XPASS: inner == 1 (the lines are contiguous), Tout = float, rec (may be null) = {min, max, ..} of the volume the call zooms
template <bool XPASS, typename Tin, typename Tout>
__global__ __launch_bounds__(LR_THREADS) void lr_spline_pass_kernel(const Tin* __restrict__ in, Tout* __restrict__ out, const double* __restrict__ rec,
                                                                   LrPass p) {
    extern __shared__ __attribute__((aligned(16))) double lr_lines[];
    const int L = p.lanes, P = p.pitch, m = p.m, n = p.n, n_pad = m + 2 * LR_PAD;
    const int line0 = blockIdx.x * L, nl = min(L, p.lines - line0);
    const int lane = threadIdx.x & (L - 1), grp = threadIdx.x / L, ngrp = LR_THREADS / L;
    long long in_base = 0, out_base = 0;
    if (!XPASS && lane < nl) {
        const int li = line0 + lane, outer = li / p.inner, i = li - outer * p.inner;
        in_base = (long long)outer * m * p.inner + i;
        out_base = (long long)outer * n * p.inner + i;
    }
    if (XPASS) {
        const Tin* src = in + (long long)line0 * m;
        for (int idx = threadIdx.x; idx < nl * m; idx += LR_THREADS) {
            const int line = idx / m, pos = idx - line * m;
            lr_lines[(pos + LR_PAD) * P + line] = 6.0 * (double)src[idx];
        }
    } else if (lane < nl) {
        for (int pos = grp; pos < m; pos += ngrp) lr_lines[(pos + LR_PAD) * P + lane] = 6.0 * (double)in[in_base + (long long)pos * p.inner];
    }
    double* lr_w = lr_lines + n_pad * P;                                               // [n][4], behind the lines
    for (int o = threadIdx.x; o < n; o += LR_THREADS) lr_weights(o, p.zoom, lr_w + 4 * o);
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * LR_PAD * L; idx += LR_THREADS) {             // the edge values, in LDS only
        const int r = idx / L, ln = idx - r * L;
        if (ln < nl) {
            if (r < LR_PAD) lr_lines[r * P + ln] = lr_lines[LR_PAD * P + ln];
            else lr_lines[(m + r) * P + ln] = lr_lines[(m + LR_PAD - 1) * P + ln];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nl) lr_prefilter(lr_lines + threadIdx.x, P, n_pad, p.zn1);
    __syncthreads();
    if (XPASS) {
        double lo = -INFINITY, hi = INFINITY;
        if (p.clip) { lo = rec[0]; hi = rec[1]; }
        Tout* dst = out + (long long)line0 * n;
        for (int idx = threadIdx.x; idx < nl * n; idx += LR_THREADS) {
            const int line = idx / n, o = idx - line * n;
            double v = lr_eval(lr_lines + line, P, n_pad, o, p.zoom, lr_w + 4 * o);
            if (p.clip) v = fmin(fmax(v, lo), hi);
            dst[idx] = (Tout)v;
        }
    } else if (lane < nl) {
        for (int o = grp; o < n; o += ngrp) out[out_base + (long long)o * p.inner] = (Tout)lr_eval(lr_lines + lane, P, n_pad, o, p.zoom, lr_w + 4 * o);
    }
}

// orders 0 and 1: one thread per output voxel
struct LrGather { int sd, sh, sw, dd, dh, dw, order, clip; double zz, zy, zx; };

__device__ __forceinline__ void lr_linear(double c, int m, int& i0, int& i1, double& t) {
    c = fmin(fmax(c, 0.0), (double)(m - 1));
    const double fl = floor(c);
    t = c - fl; i0 = (int)fl; i1 = min(i0 + 1, m - 1);
}

__global__ __launch_bounds__(256) void lr_gather_kernel(const float* __restrict__ x, float* __restrict__ y, const double* __restrict__ rec, LrGather g) {
    const long long total = (long long)g.dd * g.dh * g.dw;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int ox = (int)(i % g.dw), oy = (int)((i / g.dw) % g.dh), oz = (int)(i / ((long long)g.dw * g.dh));
        const double cz = lr_coord(oz, g.zz), cy = lr_coord(oy, g.zy), cx = lr_coord(ox, g.zx);
        if (g.order == 0) {
            const int z = min(max((int)floor(cz + 0.5), 0), g.sd - 1), yy = min(max((int)floor(cy + 0.5), 0), g.sh - 1),
                      xx = min(max((int)floor(cx + 0.5), 0), g.sw - 1);
            y[i] = x[((long long)z * g.sh + yy) * g.sw + xx];
        } else {
            int iz[2], iy[2], ix[2];
            double tz, ty, tx;
            lr_linear(cz, g.sd, iz[0], iz[1], tz); lr_linear(cy, g.sh, iy[0], iy[1], ty); lr_linear(cx, g.sw, ix[0], ix[1], tx);
            const double wz[2] = {1.0 - tz, tz}, wy[2] = {1.0 - ty, ty}, wx[2] = {1.0 - tx, tx};
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int a = (k >> 2) & 1, b = (k >> 1) & 1, c = k & 1;
                acc = acc + (double)x[((long long)iz[a] * g.sh + iy[b]) * g.sw + ix[c]] * wz[a] * wy[b] * wx[c];
            }
            if (g.clip) acc = fmin(fmax(acc, rec[0]), rec[1]);
            y[i] = (float)acc;
        }
    }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------------
static inline bool lr_order_ok(int order) { return order == 0 || order == 1 || order == 3; }
static inline bool lr_len_ok(int sd, int sh, int sw, int dd, int dh, int dw) {
    return sd <= LR_MAX_LEN && sh <= LR_MAX_LEN && sw <= LR_MAX_LEN && dd <= LR_MAX_LEN && dh <= LR_MAX_LEN && dw <= LR_MAX_LEN;
}
// workspace: the record {min, max, mean, std} of x, vs_aug_stats' scratch, and for order 3 the fp64 volumes after the z pass and after the y pass
static inline long long lr_stats_bytes(int sd, int sh, int sw) { return 4 * (long long)sizeof(double) + vs_aug_stats_workspace_bytes(1, sd, sh, sw); }

extern "C" long long vs_zoom_edge_workspace_bytes(int sd, int sh, int sw, int dd, int dh, int dw, int order) {
    if (!dp_dims_ok(sd, sh, sw) || !dp_dims_ok(dd, dh, dw) || !lr_order_ok(order)) return 0;
    if (order == 3 && !lr_len_ok(sd, sh, sw, dd, dh, dw)) return 0;
    long long bytes = lr_stats_bytes(sd, sh, sw);
    if (order == 3) bytes += ((long long)dd * sh * sw + (long long)dd * dh * sw) * (long long)sizeof(double);
    return bytes;
}

extern "C" int vs_zoom_edge_bundle(int m, int n) { return m < 1 || m > LR_MAX_LEN || n < 1 || n > LR_MAX_LEN ? 0 : lr_lanes(m, n); }

template <bool XPASS, typename Tin, typename Tout>
static int lr_launch_pass(const Tin* in, Tout* out, const double* rec, int m, int n, int inner, long long lines, int clip, hipStream_t stream) {
    static const hipError_t attr_err = hipFuncSetAttribute((const void*)lr_spline_pass_kernel<XPASS, Tin, Tout>,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, LR_LDS);
    if (attr_err != hipSuccess) return (int)attr_err;
    LrPass p{};
    p.m = m; p.n = n; p.inner = inner; p.lines = (int)lines; p.lanes = lr_lanes(m, n); p.pitch = XPASS ? p.lanes + 1 : p.lanes;
    p.zoom = (double)m / (double)n; p.zn1 = pow(LR_POLE, (double)(m + 2 * LR_PAD - 1)); p.clip = clip;
    const size_t lds = lr_lds_bytes(m, n, p.pitch);
    const unsigned int blocks = (unsigned int)((lines + p.lanes - 1) / p.lanes);
    hipLaunchKernelGGL((lr_spline_pass_kernel<XPASS, Tin, Tout>), dim3(blocks), dim3(LR_THREADS), lds, stream, in, out, rec, p);
    return VS_OK;
}

extern "C" int vs_zoom_edge(const float* x, float* y, int sd, int sh, int sw, int dd, int dh, int dw, int order, int clip, void* workspace, void* stream) {
    if (!x || !y || x == y || !lr_order_ok(order)) return VS_EINVAL;
    clip = clip != 0 && order > 0;                                         // order 0 copies voxels: nothing to clip
    if ((order == 3 || clip) && !workspace) return VS_EINVAL;
    if (!dp_dims_ok(sd, sh, sw) || !dp_dims_ok(dd, dh, dw)) return VS_ESHAPE;
    if (order == 3 && !lr_len_ok(sd, sh, sw, dd, dh, dw)) return VS_ESHAPE;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)workspace & 7)) return VS_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    double* rec = (double*)workspace;
    if (clip) {
        const int rc = vs_aug_stats(x, rec, rec + 4, 1, sd, sh, sw, stream);
        if (rc != VS_OK) return rc;
    }
    if (order < 3) {
        LrGather g{};
        g.sd = sd; g.sh = sh; g.sw = sw; g.dd = dd; g.dh = dh; g.dw = dw; g.order = order; g.clip = clip;
        g.zz = (double)sd / (double)dd; g.zy = (double)sh / (double)dh; g.zx = (double)sw / (double)dw;
        hipLaunchKernelGGL(lr_gather_kernel, dim3(dp_blocks((long long)dd * dh * dw)), dim3(256), 0, st, x, y, (const double*)rec, g);
        VS_CHECK_LAUNCH();
        return VS_OK;
    }
    double* a = (double*)((char*)workspace + lr_stats_bytes(sd, sh, sw));  // (dd, sh, sw)
    double* b = a + (long long)dd * sh * sw;                               // (dd, dh, sw)
    int rc = lr_launch_pass<false, float, double>(x, a, nullptr, sd, dd, sh * sw, (long long)sh * sw, 0, st);
    if (rc == VS_OK) rc = lr_launch_pass<false, double, double>(a, b, nullptr, sh, dh, sw, (long long)dd * sw, 0, st);
    if (rc == VS_OK) rc = lr_launch_pass<true, double, float>(b, y, rec, sw, dw, 1, (long long)dd * dh, clip, st);
    if (rc != VS_OK) return rc;
    VS_CHECK_LAUNCH();
    return VS_OK;
}
