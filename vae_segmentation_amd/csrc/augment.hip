// Intensity augmentation on the device: the batchgenerators / nnU-Net set after the geometric stage — Gaussian noise, Gaussian blur, multiplicative
// brightness, contrast, gamma (plain and inverted, with retained statistics), mirroring.  An op maps one fp32 plane (D, H, W) to one fp32 plane: it is
// computed in fp64 from the fp32 input and from fp64 plane statistics and rounded to fp32 once (DESIGN "Intensity augmentation" holds the rules).
//   vs_aug_stats          planes -> records {min, max, mean, population std}
//   vs_aug_normal_philox  the standard normals of a plane, Philox4x32-10 + Box-Muller in fp64
//   vs_aug_stage          one pass: flip on the read, + s n, * m, one of contrast / power / restat driven by a record, the store, the record of the output
//   vs_aug_blur           scipy.ndimage.gaussian_filter(mode="reflect"), all three axis passes over one LDS tile
//   vs_aug_flip           the mirror alone (the label)
// Statistics.  A record is a function of the plane's bits alone: the linear voxel index is cut into chunks of AUG_CHUNK = 8192; one workgroup of 256
// threads sums a chunk — thread t takes voxels t, t + 256, ... of the chunk in that order, then a fixed binary tree over the 256 threads in LDS — into
// {min, max, sum (x - x0), sum (x - x0)^2}, fp64, x0 the plane's first voxel; a second kernel, one thread per plane, adds the chunks' sums one after
// another in chunk order and forms mean = x0 + s1 / N, var = s2 / N - (s1 / N)^2.  The stage kernel runs the same chunking over what it writes (aug_chunk_reduce, one definition), so
// a record made by a stage's epilogue and one made by vs_aug_stats of the stored plane have the same bits.  No atomics of any kind, no memset.
// Every kernel is compiled without floating-point contraction: products and sums round separately, as the rules and the numpy oracle write them.
#include "common.h"
#include "data_sample.h"
#include "philox.h"
#include <math.h>
#pragma clang fp contract(off)

constexpr int AUG_CHUNK = 8192, AUG_THREADS = 256, AUG_PER = AUG_CHUNK / AUG_THREADS;
constexpr int AUG_MAX_RADIUS = 8;
enum { AUG_OP_NONE = 0, AUG_OP_CONTRAST = 1, AUG_OP_POWER = 2, AUG_OP_RESTAT = 3 };
enum { AUG_NOISE_NONE = 0, AUG_NOISE_ARRAY = 1, AUG_NOISE_PHILOX = 2 };

// ---- normals -------------------------------------------------------------------------------------------------------------------------------------------
// element v of the plane: pair j = v / 2 under counter (j lo, j hi, 0x100 + channel, sample), key (seed lo, seed hi); even v takes the cosine, odd v the sine
__device__ __forceinline__ double aug_normal(unsigned long long v, unsigned long long seed, unsigned int sample, unsigned int channel) {
    const unsigned long long j = v >> 1;
    unsigned int w0, w1, w2, w3;
    vs_philox4x32_10((unsigned int)j, (unsigned int)(j >> 32), 0x100u + channel, sample, (unsigned int)seed, (unsigned int)(seed >> 32), w0, w1, w2, w3);
    double r, a;
    vs_philox_box_muller(w0, w1, w2, w3, r, a);
    return r * ((v & 1) ? sin(a) : cos(a));
}

__global__ __launch_bounds__(256) void aug_normal_kernel(double* __restrict__ n, long long voxels, unsigned long long seed, unsigned int sample,
                                                        unsigned int channel) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < voxels; i += (long long)gridDim.x * 256)
        n[i] = aug_normal((unsigned long long)i, seed, sample, channel);
}

// ---- statistics ----------------------------------------------------------------------------------------------------------------------------------------
struct AugAcc { double mn, mx, s1, s2; };
__device__ __forceinline__ void aug_acc_init(AugAcc& a) { a.mn = INFINITY; a.mx = -INFINITY; a.s1 = 0.0; a.s2 = 0.0; }
__device__ __forceinline__ void aug_acc_add(AugAcc& a, float y, double y0) {
    const double v = (double)y, dv = v - y0;
    a.mn = fmin(a.mn, v); a.mx = fmax(a.mx, v);
    a.s1 = a.s1 + dv; a.s2 = a.s2 + dv * dv;
}
// the fixed tree over the workgroup's 256 threads; thread 0 writes the chunk's four doubles
__device__ __forceinline__ void aug_chunk_reduce(const AugAcc& a, double* __restrict__ part4) {
    __shared__ double red[4][AUG_THREADS];
    const int t = threadIdx.x;
    red[0][t] = a.mn; red[1][t] = a.mx; red[2][t] = a.s1; red[3][t] = a.s2;
    __syncthreads();
    for (int half = AUG_THREADS / 2; half > 0; half >>= 1) {
        if (t < half) {
            red[0][t] = fmin(red[0][t], red[0][t + half]); red[1][t] = fmax(red[1][t], red[1][t + half]);
            red[2][t] = red[2][t] + red[2][t + half]; red[3][t] = red[3][t] + red[3][t + half];
        }
        __syncthreads();
    }
    if (t == 0) { part4[0] = red[0][0]; part4[1] = red[1][0]; part4[2] = red[2][0]; part4[3] = red[3][0]; }
}

// blockIdx.x = chunk, blockIdx.y = plane; part: [planes][chunks][4]
__global__ __launch_bounds__(AUG_THREADS) void aug_stats_kernel(const float* __restrict__ x, double* __restrict__ part, long long voxels) {
    const float* px = x + (long long)blockIdx.y * voxels;
    const double x0 = (double)px[0];
    AugAcc acc;
    aug_acc_init(acc);
    const long long base = (long long)blockIdx.x * AUG_CHUNK + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < AUG_PER; ++j) {
        const long long i = base + (long long)j * AUG_THREADS;
        if (i < voxels) aug_acc_add(acc, px[i], x0);
    }
    aug_chunk_reduce(acc, part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// blockIdx.x = plane.  The chunks' sums are added one after another in chunk order by thread 0; the workgroup only fetches them, 256 chunks at a time,
// into LDS, so that the one thread does not wait for global memory 4 * chunks times.  rec = {min, max, mean, std}
__global__ __launch_bounds__(AUG_THREADS) void aug_finalize_kernel(const float* __restrict__ x, const double* __restrict__ part, double* __restrict__ rec,
                                                                  long long voxels, int chunks) {
    __shared__ double buf[4 * AUG_THREADS];
    const double* q = part + (long long)blockIdx.x * chunks * 4;
    double mn = INFINITY, mx = -INFINITY, s1 = 0.0, s2 = 0.0;
    for (int c0 = 0; c0 < chunks; c0 += AUG_THREADS) {
        const int nb = min(AUG_THREADS, chunks - c0);
        for (int i = threadIdx.x; i < 4 * nb; i += AUG_THREADS) buf[i] = q[4LL * c0 + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int c = 0; c < nb; ++c) {
                mn = fmin(mn, buf[4 * c]); mx = fmax(mx, buf[4 * c + 1]);
                s1 = s1 + buf[4 * c + 2]; s2 = s2 + buf[4 * c + 3];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = (double)voxels, m1 = s1 / n, var = s2 / n - m1 * m1;
        double* r = rec + 4 * blockIdx.x;
        r[0] = mn; r[1] = mx; r[2] = (double)x[(long long)blockIdx.x * voxels] + m1; r[3] = sqrt(fmax(var, 0.0));
    }
}

// ---- the stage -----------------------------------------------------------------------------------------------------------------------------------------
struct AugStage {
    int d, h, w;
    int flip, flip_first;              // mask z / y / x = 4 / 2 / 1 on the read; flip_first: the mirror is the first op of the stage (noise is indexed by the
                                       // output voxel), else the last (noise is indexed by the voxel read)
    int noise_mode; double s; unsigned long long seed; unsigned int sample, channel;
    int has_mult; double m;
    int op; double p; int flag;        // contrast: p = f, flag = preserve_range; power: p = gamma, flag = invert; restat: flag = invert
    int rec0_given; double mean0, std0;
};

__device__ __forceinline__ float aug_stage_voxel(const AugStage& a, const float* __restrict__ x, const double* __restrict__ noise,
                                                 const double* __restrict__ rec, double mean0, double std0, unsigned int i) {
    unsigned int src = i;                                                  // a plane has fewer than 2^31 voxels: 32-bit index arithmetic
    if (a.flip) {
        const unsigned int w = (unsigned int)a.w, hw = (unsigned int)a.h * w;
        unsigned int z = i / hw;
        const unsigned int rem = i - z * hw;
        unsigned int y = rem / w, xx = rem - y * w;
        if (a.flip & 4) z = (unsigned int)a.d - 1u - z;
        if (a.flip & 2) y = (unsigned int)a.h - 1u - y;
        if (a.flip & 1) xx = w - 1u - xx;
        src = z * hw + y * w + xx;
    }
    float v = x[src];
    if (a.noise_mode != AUG_NOISE_NONE) {
        const unsigned int ni = a.flip_first ? i : src;
        const double nv = a.noise_mode == AUG_NOISE_ARRAY ? noise[ni] : aug_normal((unsigned long long)ni, a.seed, a.sample, a.channel);
        v = (float)((double)v + a.s * nv);
    }
    if (a.has_mult) v = (float)((double)v * a.m);
    if (a.op == AUG_OP_CONTRAST) {
        const double mean = rec[2];
        double y = ((double)v - mean) * a.p + mean;
        if (a.flag) y = fmin(fmax(y, rec[0]), rec[1]);
        v = (float)y;
    } else if (a.op == AUG_OP_POWER) {
        const double xp = a.flag ? -(double)v : (double)v, mn = a.flag ? -rec[1] : rec[0], mx = a.flag ? -rec[0] : rec[1], r = mx - mn;
        const double y = pow((xp - mn) / (r + 1e-7), a.p) * r + mn;
        v = (float)(a.flag ? -y : y);
    } else if (a.op == AUG_OP_RESTAT) {
        const double xp = a.flag ? -(double)v : (double)v, mean = a.flag ? -rec[2] : rec[2];
        const double y = (xp - mean) / (rec[3] + 1e-8) * std0 + mean0;
        v = (float)(a.flag ? -y : y);
    }
    return v;
}

// blockIdx.x = chunk of the output plane.  part (may be null): the chunk's statistics of what is stored
__global__ __launch_bounds__(AUG_THREADS) void aug_stage_kernel(const float* __restrict__ x, float* __restrict__ y, const double* __restrict__ noise,
                                                               const double* __restrict__ rec, const double* __restrict__ rec0,
                                                               double* __restrict__ part, AugStage a) {
    const unsigned int voxels = (unsigned int)a.d * (unsigned int)a.h * (unsigned int)a.w;
    double mean0 = a.mean0, std0 = a.std0;
    if (a.op == AUG_OP_RESTAT && a.rec0_given) { mean0 = a.flag ? -rec0[2] : rec0[2]; std0 = rec0[3]; }
    AugAcc acc;
    aug_acc_init(acc);
    const double y0 = part ? (double)aug_stage_voxel(a, x, noise, rec, mean0, std0, 0) : 0.0;      // the shift of the output's sums: its first voxel
    const unsigned int base = blockIdx.x * (unsigned int)AUG_CHUNK + threadIdx.x;          // < 2^31 + 8192
    for (int j = 0; j < AUG_PER; ++j) {
        const unsigned int i = base + (unsigned int)j * AUG_THREADS;
        if (i < voxels) {
            const float v = aug_stage_voxel(a, x, noise, rec, mean0, std0, i);
            y[i] = v;
            if (part) aug_acc_add(acc, v, y0);
        }
    }
    if (part) aug_chunk_reduce(acc, part + (long long)blockIdx.x * 4);
}

// ---- blur ----------------------------------------------------------------------------------------------------------------------------------------------
// One workgroup owns a tile of tz x ty x 32 outputs.  It stages the tile plus a halo of `radius` voxels on every side in LDS as fp32 — rows of
// xw = 32 + 2 radius contiguous voxels, the indices beyond the volume mirrored as scipy's "reflect" does (d c b a | a b c d | d c b a, repeated when the
// line is shorter than the halo) — and runs the three passes over it:
//   z   a thread owns a column (y', x') of the staged block and writes the tz filtered values over the column's first tz entries, front to back: output
//       z reads entries z .. z + 2 radius, all behind the ones already overwritten
//   y   likewise for the lines (z, x') of the tz filtered planes
//   x   from LDS to global memory
// Each pass accumulates in fp64 in scipy's order for a symmetric kernel — centre tap first, then the pairs from the outside in, (a + b) w — and rounds to
// fp32 when it stores.  A pass over the mirrored halo computes what the pass over the volume computes at the mirrored position, operand for operand, so
// the halo holds the bits a pass-by-pass filter of the whole volume would mirror in.
// LDS traffic: consecutive lanes take consecutive x' of one row (z, y passes: the staged rows are contiguous, pitch xw, so a flat index over (y', x')
// walks consecutive dwords; x pass: 32 lanes = one row of 32 outputs), so no 32-lane group meets a bank twice.
// The tile is chosen per radius so that the staged block stays under 80 KiB: two workgroups per CU.
struct AugWeights { double w[AUG_MAX_RADIUS + 1]; int radius; };
constexpr int AUG_TX = 32;
constexpr int AUG_BLUR_LDS = 80 * 1024;

__device__ __forceinline__ int aug_reflect(int i, int n) {
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

__device__ __forceinline__ float aug_taps(const float* at, int stride, const AugWeights& g) {
    const int r = g.radius;
    double acc = (double)at[r * stride] * g.w[0];
    for (int k = r; k >= 1; --k) acc = acc + ((double)at[(r - k) * stride] + (double)at[(r + k) * stride]) * g.w[k];
    return (float)acc;
}

__global__ __launch_bounds__(256) void aug_blur_kernel(const float* __restrict__ x, float* __restrict__ y, int d, int h, int w, int tz, int ty, int n_xt,
                                                      int n_yt, AugWeights g) {
    extern __shared__ __attribute__((aligned(16))) float aug_tile[];
    const int r = g.radius, xw = AUG_TX + 2 * r, yw = ty + 2 * r, zw = tz + 2 * r;
    int b = blockIdx.x;
    const int x0 = (b % n_xt) * AUG_TX; b /= n_xt;
    const int y0 = (b % n_yt) * ty;
    const int z0 = (b / n_yt) * tz;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // stage: a wave per row (z', y'), lanes along x'
    const int gx = aug_reflect(x0 - r + lane, w);
    for (int row = wave; row < zw * yw; row += 4) {
        const int zz = row / yw, yy = row - zz * yw;
        const long long line = ((long long)aug_reflect(z0 - r + zz, d) * h + aug_reflect(y0 - r + yy, h)) * w;
        if (lane < xw) aug_tile[row * xw + lane] = x[line + gx];
    }
    __syncthreads();
    const int plane = yw * xw;
    for (int c = threadIdx.x; c < plane; c += 256) {                               // z: columns (y', x')
        float* col = aug_tile + c;
        for (int z = 0; z < tz; ++z) col[z * plane] = aug_taps(col + z * plane, plane, g);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < tz * xw; c += 256) {                              // y: lines (z, x')
        const int z = c / xw, xx = c - z * xw;
        float* col = aug_tile + z * plane + xx;
        for (int yy = 0; yy < ty; ++yy) col[yy * xw] = aug_taps(col + yy * xw, xw, g);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < tz * ty * AUG_TX; c += 256) {                     // x: 32 lanes = one row of outputs
        const int xx = c & (AUG_TX - 1), row = c >> 5, z = row / ty, yy = row - z * ty;
        const int oz = z0 + z, oy = y0 + yy, ox = x0 + xx;
        if (oz < d && oy < h && ox < w) y[((long long)oz * h + oy) * w + ox] = aug_taps(aug_tile + z * plane + yy * xw + xx, 1, g);
    }
}

// the first tile (tz, ty) whose staged block fits AUG_BLUR_LDS
static inline void aug_blur_tile(int radius, int& tz, int& ty) {
    static const int cand[5][2] = {{16, 16}, {16, 8}, {8, 8}, {8, 4}, {4, 4}};
    for (int i = 0; i < 5; ++i) {
        tz = cand[i][0]; ty = cand[i][1];
        if ((size_t)(tz + 2 * radius) * (ty + 2 * radius) * (AUG_TX + 2 * radius) * sizeof(float) <= (size_t)AUG_BLUR_LDS) return;
    }
}

static inline bool aug_sigma_ok(double sigma) { return sigma > 0.0 && sigma <= 2.0; }      // false for NaN

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------------
static inline int aug_chunks(long long voxels) { return (int)((voxels + AUG_CHUNK - 1) / AUG_CHUNK); }

extern "C" long long vs_aug_stats_workspace_bytes(int planes, int d, int h, int w) {
    if (planes < 1 || !dp_dims_ok(d, h, w)) return 0;
    return (long long)planes * aug_chunks((long long)d * h * w) * 4 * (long long)sizeof(double);
}

extern "C" int vs_aug_stats(const float* x, double* rec, double* workspace, int planes, int d, int h, int w, void* stream) {
    if (!x || !rec || !workspace || planes < 1) return VS_EINVAL;
    if (!dp_dims_ok(d, h, w) || planes > 65535) return VS_ESHAPE;
    if (((uintptr_t)x & 3) || ((uintptr_t)rec & 7) || ((uintptr_t)workspace & 7)) return VS_EALIGN;
    const long long voxels = (long long)d * h * w;
    const int chunks = aug_chunks(voxels);
    hipLaunchKernelGGL(aug_stats_kernel, dim3(chunks, planes), dim3(AUG_THREADS), 0, (hipStream_t)stream, x, workspace, voxels);
    hipLaunchKernelGGL(aug_finalize_kernel, dim3(planes), dim3(AUG_THREADS), 0, (hipStream_t)stream, x, (const double*)workspace, rec, voxels, chunks);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_aug_normal_philox(double* n, int d, int h, int w, unsigned long long seed, unsigned long long sample, int channel, void* stream) {
    if (!n || channel < 0) return VS_EINVAL;
    if (!dp_dims_ok(d, h, w)) return VS_ESHAPE;
    if ((uintptr_t)n & 7) return VS_EALIGN;
    const long long voxels = (long long)d * h * w;
    hipLaunchKernelGGL(aug_normal_kernel, dim3(dp_blocks(voxels)), dim3(256), 0, (hipStream_t)stream, n, voxels, seed, (unsigned int)sample,
                       (unsigned int)channel);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_aug_stage(const float* x, float* y, int d, int h, int w, int flip, int flip_first, int noise_mode, const double* noise, double s,
                            unsigned long long seed, unsigned long long sample, int channel, int has_mult, double m, int op, double p, int flag,
                            const double* rec, const double* rec0, double mean0, double std0, double* rec_out, double* workspace, void* stream) {
    if (!x || !y || x == y || flip < 0 || flip > 7 || noise_mode < AUG_NOISE_NONE || noise_mode > AUG_NOISE_PHILOX || op < AUG_OP_NONE ||
        op > AUG_OP_RESTAT || channel < 0)
        return VS_EINVAL;
    if ((noise_mode == AUG_NOISE_ARRAY && !noise) || (op != AUG_OP_NONE && !rec) || (rec_out && !workspace)) return VS_EINVAL;
    if ((noise_mode != AUG_NOISE_NONE && !isfinite(s)) || (has_mult && !isfinite(m)) || (op != AUG_OP_NONE && op != AUG_OP_RESTAT && !isfinite(p)) ||
        (op == AUG_OP_RESTAT && !rec0 && !(isfinite(mean0) && isfinite(std0))))
        return VS_EINVAL;
    if (!dp_dims_ok(d, h, w)) return VS_ESHAPE;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)noise & 7) || ((uintptr_t)rec & 7) || ((uintptr_t)rec0 & 7) || ((uintptr_t)rec_out & 7) ||
        ((uintptr_t)workspace & 7))
        return VS_EALIGN;
    AugStage a{};
    a.d = d; a.h = h; a.w = w; a.flip = flip; a.flip_first = flip_first != 0;
    a.noise_mode = noise_mode; a.s = s; a.seed = seed; a.sample = (unsigned int)sample; a.channel = (unsigned int)channel;
    a.has_mult = has_mult != 0; a.m = m; a.op = op; a.p = p; a.flag = flag != 0;
    a.rec0_given = rec0 != nullptr; a.mean0 = mean0; a.std0 = std0;
    const long long voxels = (long long)d * h * w;
    const int chunks = aug_chunks(voxels);
    hipLaunchKernelGGL(aug_stage_kernel, dim3(chunks), dim3(AUG_THREADS), 0, (hipStream_t)stream, x, y, noise, rec, rec0, rec_out ? workspace : nullptr, a);
    if (rec_out)
        hipLaunchKernelGGL(aug_finalize_kernel, dim3(1), dim3(AUG_THREADS), 0, (hipStream_t)stream, (const float*)y, (const double*)workspace, rec_out,
                           voxels, chunks);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_aug_blur_tile(double sigma, int* tile3) {
    if (!tile3 || !aug_sigma_ok(sigma)) return VS_EINVAL;
    aug_blur_tile((int)(4.0 * sigma + 0.5), tile3[0], tile3[1]);
    tile3[2] = AUG_TX;
    return VS_OK;
}

extern "C" int vs_aug_blur(const float* x, float* y, int d, int h, int w, double sigma, const double* weights, void* stream) {
    if (!x || !y || x == y || !weights || !aug_sigma_ok(sigma)) return VS_EINVAL;
    if (!dp_dims_ok(d, h, w)) return VS_ESHAPE;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)weights & 7)) return VS_EALIGN;
    AugWeights g{};
    g.radius = (int)(4.0 * sigma + 0.5);                                   // scipy.ndimage.gaussian_filter1d, truncate = 4; sigma <= 2: at most 8
    for (int k = 0; k <= g.radius; ++k) {
        if (!isfinite(weights[k])) return VS_EINVAL;                       // a HOST array: the half kernel w[0 .. radius], w[k] the weight of taps -k and +k
        g.w[k] = weights[k];
    }
    static const hipError_t attr_err = hipFuncSetAttribute((const void*)aug_blur_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, AUG_BLUR_LDS);
    if (attr_err != hipSuccess) return (int)attr_err;
    int tz, ty;
    aug_blur_tile(g.radius, tz, ty);
    const int n_xt = (w + AUG_TX - 1) / AUG_TX, n_yt = (h + ty - 1) / ty, n_zt = (d + tz - 1) / tz;
    const long long blocks = (long long)n_xt * n_yt * n_zt;                // <= voxels < 2^31
    const size_t lds = (size_t)(tz + 2 * g.radius) * (ty + 2 * g.radius) * (AUG_TX + 2 * g.radius) * sizeof(float);
    hipLaunchKernelGGL(aug_blur_kernel, dim3((unsigned int)blocks), dim3(256), lds, (hipStream_t)stream, x, y, d, h, w, tz, ty, n_xt, n_yt, g);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_aug_flip(const float* x, float* y, int planes, int d, int h, int w, int mask, void* stream) {
    if (!x || !y || x == y || planes < 1 || mask < 0 || mask > 7) return VS_EINVAL;
    if (!dp_dims_ok(d, h, w)) return VS_ESHAPE;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3)) return VS_EALIGN;
    AugStage a{};
    a.d = d; a.h = h; a.w = w; a.flip = mask;
    const long long voxels = (long long)d * h * w;
    for (int p = 0; p < planes; ++p)
        hipLaunchKernelGGL(aug_stage_kernel, dim3(aug_chunks(voxels)), dim3(AUG_THREADS), 0, (hipStream_t)stream, x + p * voxels, y + p * voxels,
                           (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, (double*)nullptr, a);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
