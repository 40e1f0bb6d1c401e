// Exact order statistics of fp32 planes and the piecewise-linear intensity map through them (include/vaeseg.h: vs_quantile, vs_intensity_map).
//
// Inputs are planar fp32 (planes, d, h, w); every plane is its own problem and is read as one flat string of V = d*h*w voxels.
//
//   selection  a voxel counts iff it is finite, above the threshold (strict fp32 comparison) and under a non-zero mask byte, as far as either is given.
//   select     no sort: a radix select over key_enc's order-preserving integer image of the fp32 bits (volume.h), four passes of 8 bits.  A percentile
//              needs the order statistics of two ranks, k and k1: 2 Q targets.  In a pass every workgroup counts, in LDS, the current digit of the
//              voxels whose higher digits equal a target's prefix — one table of 256 32-bit counters per DISTINCT prefix (at most QS_MAX_TARGETS
//              tables, 32 KB; the first pass has one) — and adds its non-zero cells to the plane's tables in the workspace.  A run of equal voxels
//              along x is ONE update of the run's length (the ballot of run heads of hist.hip and regions.hip): the air of a CT volume does not
//              serialise on one LDS cell.
//   choose     a one-workgroup-per-plane launch behind each pass: a wave scans a target's table (four counters per lane), finds the digit that
//              holds the target's rank and leaves prefix and residual rank in the workspace, numbers the distinct prefixes for the next pass and
//              zeroes the tables that pass will add to.
//   finish     the last of these launches decodes the 2 Q keys and forms h = (n - 1) p, t = h - floor(h) and numpy's _lerp in fp64 with every product
//              and sum rounded separately (contraction off): n is known only on the device.
//
// Nine launches whatever the data: the initial state, then count and choose four times.  The first launch writes the workspace's initial state; no
// memset, nothing allocated, synchronised or read back.  Every count is an integer added by vector-lane atomics, so the results do not depend on the
// order of arrival: the same bits eagerly, under graph replay and in both builds of the library.
//
// vs_intensity_map: y = dst[j] + (x - src[j]) * slope_j in fp64, contraction off, rounded to fp32 once; src is a row of landmarks per plane in DEVICE
// memory (vs_quantile's q_out), so a standardisation is quantile -> map without a host copy in between.  One launch over all planes.
#include <limits.h>
#include <math.h>
#include "volume.h"

namespace {

constexpr int QS_MAX_Q = 16;
constexpr int QS_MAX_TARGETS = 2 * QS_MAX_Q;  // the ranks k and k1 of every percentile
// QS_WG_VOXELS and IM_WG_VOXELS are mirrored by hand in ops.py (QUANTILE_WG_VOXELS, INTENSITY_MAP_WG_VOXELS), which the tests size their multi-workgroup
// shapes against: whoever changes one here changes the other there.
constexpr int QS_WG_VOXELS = 16384;           // voxels a workgroup counts in LDS before its one flush
constexpr int QS_UNROLL = 4;                  // voxels per thread whose loads are issued before the first is counted
constexpr int IM_MAX_L = 16;
constexpr int IM_WG_VOXELS = 4096;            // voxels a workgroup of vs_intensity_map writes
static_assert(QS_WG_VOXELS % (256 * QS_UNROLL) == 0, "every thread of a workgroup runs the same trip count: the ballots need all lanes");
static_assert(IM_WG_VOXELS % 1024 == 0, "a thread of the map moves whole quads");

// a plane's piece of the workspace, in 32-bit words: a header, four rows of TT = 2 Q words, TT tables of 256 counters (16-byte aligned)
enum { QS_N = 0, QS_REJ = 1, QS_NTAB = 2, QS_HEADER = 4 };
__host__ __device__ __forceinline__ long long qs_stride(int TT) { return QS_HEADER + 4ll * TT + 256ll * TT; }
__device__ __forceinline__ unsigned int* qs_prefix(unsigned int* S, int TT) { return S + QS_HEADER; }             // per target: the digits chosen so far
__device__ __forceinline__ unsigned int* qs_rank(unsigned int* S, int TT) { return S + QS_HEADER + TT; }          // per target: its rank among the voxels under its prefix
__device__ __forceinline__ unsigned int* qs_slot(unsigned int* S, int TT) { return S + QS_HEADER + 2 * TT; }      // per target: the table of its prefix
__device__ __forceinline__ unsigned int* qs_tabprefix(unsigned int* S, int TT) { return S + QS_HEADER + 3 * TT; } // per table: the prefix it counts
__device__ __forceinline__ unsigned int* qs_tables(unsigned int* S, int TT) { return S + QS_HEADER + 4 * TT; }

struct qs_job {
    const float* x;
    const unsigned char* mask;     // NULL: every voxel
    unsigned int* ws;
    double* q_out;                 // (planes, Q)
    float* lo_out;
    float* hi_out;
    i64* count;                    // (planes)
    i64* rejected;
    double p01[QS_MAX_Q];
    float above;
    int use_above, Q, V;
    long long planes;
};

__global__ __launch_bounds__(256) void qs_init_kernel(qs_job j) {
    const int TT = 2 * j.Q;
    unsigned int* S = j.ws + (long long)blockIdx.x * qs_stride(TT);
    qs_tables(S, TT)[threadIdx.x] = 0u;                                   // the first pass has one table
    if (threadIdx.x < QS_HEADER) S[threadIdx.x] = threadIdx.x == QS_NTAB ? 1u : 0u;
}

// a workgroup per QS_WG_VOXELS voxels of one plane; PASS p counts bits [24 - 8 p, 32 - 8 p) of the keys under the targets' prefixes
template <int PASS>
__global__ __launch_bounds__(256) void qs_count_kernel(qs_job j, int blocks_per_plane) {
    __shared__ unsigned int cells[(PASS == 0 ? 1 : QS_MAX_TARGETS) * 256];     // the first pass has one table: it keeps its occupancy
    __shared__ unsigned int tp[QS_MAX_TARGETS];
    __shared__ unsigned int totals[2];
    constexpr int HI = 32 - 8 * PASS;                                     // the bits above the current digit (PASS > 0)
    const int lane = threadIdx.x & 63, TT = 2 * j.Q;
    const long long plane = blockIdx.x / blocks_per_plane;
    const int v0 = (int)(blockIdx.x - plane * blocks_per_plane) * QS_WG_VOXELS;
    unsigned int* S = j.ws + plane * qs_stride(TT);
    const int ntab = PASS == 0 ? 1 : min((int)S[QS_NTAB], TT);            // written by the launch before this one
    if (ntab == 0) return;                                                // nothing selected in this plane (the whole workgroup leaves)
    for (int i = threadIdx.x; i < ntab * 256; i += 256) cells[i] = 0u;
    if (PASS > 0 && (int)threadIdx.x < ntab) tp[threadIdx.x] = qs_tabprefix(S, TT)[threadIdx.x] >> (HI & 31);
    if (threadIdx.x < 2) totals[threadIdx.x] = 0u;
    __syncthreads();
    const float* X = j.x + (size_t)plane * j.V;
    const unsigned char* M = j.mask ? j.mask + (size_t)plane * j.V : nullptr;
    int nsel = 0, nrej = 0;
    for (int it = 0; it < QS_WG_VOXELS / 256; it += QS_UNROLL) {
        float xv[QS_UNROLL];
        unsigned char mk[QS_UNROLL];
#pragma unroll
        for (int u = 0; u < QS_UNROLL; ++u) {
            const long long v = (long long)v0 + (it + u) * 256 + threadIdx.x;
            const bool live = v < j.V;
            xv[u] = live ? X[v] : 0.f;
            mk[u] = live && M ? M[v] : (unsigned char)1;
        }
#pragma unroll
        for (int u = 0; u < QS_UNROLL; ++u) {
            const long long v = (long long)v0 + (it + u) * 256 + threadIdx.x;
            const bool live = v < j.V, fin = key_finite(xv[u]);
            const bool sel = live && fin && (!j.use_above || xv[u] > j.above) && mk[u] != 0;
            const unsigned int e = sel ? key_enc(xv[u]) : 0u;             // no finite value has the key 0
            if (PASS == 0) {
                nsel += __popcll(__ballot(sel));
                nrej += __popcll(__ballot(live && !fin));
            }
            const unsigned int below = (unsigned int)__shfl_up((int)e, 1);
            const bool head = lane == 0 || e != below;
            const u64 heads = __ballot(head);
            if (head && e) {
                const unsigned int len = (unsigned int)run_length(heads, lane);
                if (PASS == 0) {
                    atomicAdd(&cells[e >> 24], len);
                } else {
                    const unsigned int hi = e >> (HI & 31), digit = (e >> ((HI - 8) & 31)) & 255u;
                    for (int s = 0; s < ntab; ++s)
                        if (hi == tp[s]) atomicAdd(&cells[s * 256 + digit], len);
                }
            }
        }
    }
    if (PASS == 0 && lane == 0) {
        if (nsel) atomicAdd(&totals[0], (unsigned int)nsel);
        if (nrej) atomicAdd(&totals[1], (unsigned int)nrej);
    }
    __syncthreads();
    unsigned int* T = qs_tables(S, TT);
    for (int i = threadIdx.x; i < ntab * 256; i += 256) {
        const unsigned int c = cells[i];
        if (c) atomicAdd(T + i, c);
    }
    if (PASS == 0 && threadIdx.x < 2 && totals[threadIdx.x]) atomicAdd(S + threadIdx.x, totals[threadIdx.x]);      // QS_N, QS_REJ
}

// h = (n - 1) p and its floor, n >= 1: the two ranks a percentile interpolates and the weight of the upper one
__device__ __forceinline__ void qs_ranks(unsigned int n, double p01, unsigned int& k, unsigned int& k1, double& t) {
#pragma clang fp contract(off)
    const double h = (double)(n - 1u) * p01;
    const double f = fmin(fmax(floor(h), 0.0), (double)(n - 1u));
    k = (unsigned int)f;
    k1 = k + 1u < n ? k + 1u : n - 1u;
    t = h - f;
}

// numpy's _lerp
__device__ __forceinline__ double qs_lerp(double a, double b, double t) {
#pragma clang fp contract(off)
    const double d = b - a;
    if (t >= 0.5) {
        const double u = 1.0 - t;
        const double m = d * u;
        return b - m;
    }
    const double m = d * t;
    return a + m;
}

// a workgroup per plane behind count pass PASS: the digit of every target, the tables of the next pass; PASS 3 writes the results
template <int PASS>
__global__ __launch_bounds__(256) void qs_choose_kernel(qs_job j) {
    __shared__ unsigned int pfx[QS_MAX_TARGETS], rk[QS_MAX_TARGETS], rep[QS_MAX_TARGETS];
    __shared__ int next_tabs;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, TT = 2 * j.Q, tid = threadIdx.x;
    const long long plane = blockIdx.x;
    unsigned int* S = j.ws + plane * qs_stride(TT);
    const unsigned int n = S[QS_N];
    if (n == 0u) {                                                        // nothing selected: the whole workgroup takes this branch
        if (PASS == 0 && tid == 0) S[QS_NTAB] = 0u;
        if (PASS == 3) {
            if (tid < j.Q) {
                j.q_out[plane * j.Q + tid] = (double)NAN;
                j.lo_out[plane * j.Q + tid] = NAN;
                j.hi_out[plane * j.Q + tid] = NAN;
            }
            if (tid == 0) {
                j.count[plane] = 0;
                j.rejected[plane] = (i64)S[QS_REJ];
            }
        }
        return;
    }
    const uint4* T = reinterpret_cast<const uint4*>(qs_tables(S, TT));
    for (int t = wave; t < TT; t += 4) {                                  // wave-uniform
        unsigned int r, pre = 0u;
        int s = 0;
        if (PASS == 0) {
            unsigned int k, k1;
            double w;
            qs_ranks(n, j.p01[t >> 1], k, k1, w);
            r = (t & 1) ? k1 : k;
        } else {
            r = qs_rank(S, TT)[t];
            pre = qs_prefix(S, TT)[t];
            s = min((int)qs_slot(S, TT)[t], TT - 1);
        }
        const uint4 c = T[s * 64 + lane];                                 // the counters of digits 4 lane .. 4 lane + 3
        const unsigned int sum = c.x + c.y + c.z + c.w;
        unsigned int inc = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int up = (unsigned int)__shfl_up((int)inc, o);
            if (lane >= o) inc += up;
        }
        unsigned int exc = inc - sum;                                     // voxels under the prefix with a smaller digit than this lane's first
        const u64 reach = __ballot(exc <= r);                             // lane 0 always: the last such lane holds the rank
        const int L = 63 - __clzll((long long)reach);
        if (lane == L) {
            unsigned int d = 0u;
            if (r >= exc + c.x) {
                exc += c.x; d = 1u;
                if (r >= exc + c.y) {
                    exc += c.y; d = 2u;
                    if (r >= exc + c.z) { exc += c.z; d = 3u; }
                }
            }
            pfx[t] = pre | ((4u * (unsigned int)L + d) << (24 - 8 * PASS));
            rk[t] = r - exc;
        }
    }
    __syncthreads();                                                      // every table is read; pfx and rk are complete
    if (PASS == 3) {
        if (tid < j.Q) {
            unsigned int k, k1;
            double t;
            qs_ranks(n, j.p01[tid], k, k1, t);
            const float a = key_dec(pfx[2 * tid]), b = key_dec(pfx[2 * tid + 1]);
            j.q_out[plane * j.Q + tid] = qs_lerp((double)a, (double)b, t);
            j.lo_out[plane * j.Q + tid] = a;
            j.hi_out[plane * j.Q + tid] = b;
        }
        if (tid == 0) {
            j.count[plane] = (i64)n;
            j.rejected[plane] = (i64)S[QS_REJ];
        }
        return;
    }
    if (tid < TT) {                                                       // the first target with the same prefix stands for it
        int first = tid;
        for (int u = 0; u < tid; ++u)
            if (pfx[u] == pfx[tid]) { first = u; break; }
        rep[tid] = (unsigned int)first;
    }
    __syncthreads();
    if (tid < TT) {
        int slot = 0;
        for (int u = 0; u < (int)rep[tid]; ++u) slot += rep[u] == (unsigned int)u;
        qs_prefix(S, TT)[tid] = pfx[tid];
        qs_rank(S, TT)[tid] = rk[tid];
        qs_slot(S, TT)[tid] = (unsigned int)slot;
        if (rep[tid] == (unsigned int)tid) qs_tabprefix(S, TT)[slot] = pfx[tid];
    }
    if (tid == 0) {
        int tabs = 0;
        for (int u = 0; u < TT; ++u) tabs += rep[u] == (unsigned int)u;
        S[QS_NTAB] = (unsigned int)tabs;
        next_tabs = tabs;
    }
    __syncthreads();
    unsigned int* Z = qs_tables(S, TT);
    for (int i = tid; i < next_tabs * 256; i += 256) Z[i] = 0u;           // what the next pass adds to
}

struct im_job {
    const float* x;
    const double* src;             // (planes, L)
    const double* dst;             // (L)
    float* y;
    int L, clamp, V;
    long long planes;
};

struct im_table {
    double s[IM_MAX_L], d[IM_MAX_L], slope[IM_MAX_L];
};

__device__ __forceinline__ float im_apply(float xf, const im_table& tb, int L, int clamp) {
#pragma clang fp contract(off)
    if (!key_finite(xf)) return xf;
    const double x = (double)xf;
    int jj = 0;
    for (int i = 1; i < L - 1; ++i)
        if (tb.s[i] <= x) jj = i;
    const double m = (x - tb.s[jj]) * tb.slope[jj];
    double y = tb.d[jj] + m;
    if (clamp) y = fmin(fmax(y, tb.d[0]), tb.d[L - 1]);
    return (float)y;
}

// a workgroup per IM_WG_VOXELS voxels of one plane.  VEC: V is a multiple of 4 and the pointers are 16-byte aligned, a lane moves quads
template <bool VEC>
__global__ __launch_bounds__(256) void im_kernel(im_job j, int blocks_per_plane) {
    __shared__ im_table tb;
    __shared__ int copy;
    const long long plane = blockIdx.x / blocks_per_plane;
    const int v0 = (int)(blockIdx.x - plane * blocks_per_plane) * IM_WG_VOXELS;
    const int L = j.L, tid = threadIdx.x;
    if (tid < L) {
        tb.s[tid] = j.src[plane * L + tid];
        tb.d[tid] = j.dst[tid];
    }
    __syncthreads();
    if (tid < L - 1) {
        const double w = tb.s[tid + 1] - tb.s[tid];
        tb.slope[tid] = w > 0.0 ? (tb.d[tid + 1] - tb.d[tid]) / w : 0.0;
    }
    if (tid == 0) {
        int bad = 0;
        for (int i = 0; i < L; ++i) bad |= tb.s[i] != tb.s[i];            // NaN landmarks: nothing was selected, the plane is copied
        copy = bad;
    }
    __syncthreads();
    const float* X = j.x + (size_t)plane * j.V;
    float* Y = j.y + (size_t)plane * j.V;
    const int is_copy = copy;
    if (VEC) {
        for (int it = 0; it < IM_WG_VOXELS / 1024; ++it) {
            const long long v = (long long)v0 + (it * 256 + tid) * 4;
            if (v >= j.V) break;
            f32x4 q = *reinterpret_cast<const f32x4*>(X + v);
            if (!is_copy)
                for (int e = 0; e < 4; ++e) q[e] = im_apply(q[e], tb, L, j.clamp);
            *reinterpret_cast<f32x4*>(Y + v) = q;
        }
    } else {
        for (int it = 0; it < IM_WG_VOXELS / 256; ++it) {
            const long long v = (long long)v0 + it * 256 + tid;
            if (v >= j.V) break;
            const float q = X[v];
            Y[v] = is_copy ? q : im_apply(q, tb, L, j.clamp);
        }
    }
}

int qs_shape(int planes, int d, int h, int w, int* V) {
    if (planes <= 0 || d <= 0 || h <= 0 || w <= 0) return VS_ESHAPE;
    const long long v = (long long)d * h * w;
    if (v > INT_MAX) return VS_ESHAPE;                                    // plane-local indices and the counters are 32-bit
    *V = (int)v;
    return VS_OK;
}

}  // namespace

extern "C" size_t vs_quantile_workspace_bytes(int planes, long long V, int Q) {
    if (planes <= 0 || V <= 0 || V > INT_MAX || Q < 1 || Q > QS_MAX_Q) return 0;
    return (size_t)planes * (size_t)qs_stride(2 * Q) * sizeof(unsigned int);
}

extern "C" int vs_quantile(const float* x, const unsigned char* mask, int use_above, float above, const double* p01, int Q, double* q_out, float* lo_out,
                           float* hi_out, long long* count, long long* rejected, void* workspace, int planes, int d, int h, int w, void* stream) {
    qs_job j = {};
    const int rc = qs_shape(planes, d, h, w, &j.V);
    if (rc != VS_OK) return rc;
    if (!x || !p01 || !q_out || !lo_out || !hi_out || !count || !rejected || !workspace || Q < 1 || Q > QS_MAX_Q) return VS_EINVAL;
    if (use_above && !(above == above)) return VS_EINVAL;
    for (int i = 0; i < Q; ++i) {
        if (!(p01[i] >= 0.0 && p01[i] <= 1.0)) return VS_EINVAL;         // NaN fails both
        j.p01[i] = p01[i];
    }
    if (((uintptr_t)x & 3) || ((uintptr_t)q_out & 7) || ((uintptr_t)lo_out & 3) || ((uintptr_t)hi_out & 3) || ((uintptr_t)count & 7) ||
        ((uintptr_t)rejected & 7) || ((uintptr_t)workspace & 15)) return VS_EALIGN;
    const long long bpp = ((long long)j.V + QS_WG_VOXELS - 1) / QS_WG_VOXELS;
    if ((long long)planes * bpp > INT_MAX) return VS_ESHAPE;              // one workgroup per piece of a plane
    j.x = x; j.mask = mask;
    j.ws = (unsigned int*)workspace;
    j.q_out = q_out; j.lo_out = lo_out; j.hi_out = hi_out;
    j.count = count; j.rejected = rejected;
    j.use_above = use_above != 0; j.above = above;
    j.Q = Q;
    j.planes = planes;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 pieces((unsigned)(planes * bpp)), each((unsigned)planes), wg(256);
    hipLaunchKernelGGL(qs_init_kernel, each, wg, 0, st, j);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(qs_count_kernel<0>, pieces, wg, 0, st, j, (int)bpp);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(qs_choose_kernel<0>, each, wg, 0, st, j);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(qs_count_kernel<1>, pieces, wg, 0, st, j, (int)bpp);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(qs_choose_kernel<1>, each, wg, 0, st, j);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(qs_count_kernel<2>, pieces, wg, 0, st, j, (int)bpp);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(qs_choose_kernel<2>, each, wg, 0, st, j);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(qs_count_kernel<3>, pieces, wg, 0, st, j, (int)bpp);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(qs_choose_kernel<3>, each, wg, 0, st, j);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_intensity_map(const float* x, const double* src, const double* dst, int L, int clamp, float* y, int planes, int d, int h, int w,
                                void* stream) {
    im_job j = {};
    const int rc = qs_shape(planes, d, h, w, &j.V);
    if (rc != VS_OK) return rc;
    if (!x || !src || !dst || !y || L < 2 || L > IM_MAX_L || (clamp != 0 && clamp != 1)) return VS_EINVAL;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)src & 7) || ((uintptr_t)dst & 7)) return VS_EALIGN;
    const long long bpp = ((long long)j.V + IM_WG_VOXELS - 1) / IM_WG_VOXELS;
    if ((long long)planes * bpp > INT_MAX) return VS_ESHAPE;
    j.x = x; j.src = src; j.dst = dst; j.y = y;
    j.L = L; j.clamp = clamp;
    j.planes = planes;
    const bool vec = j.V % 4 == 0 && !((uintptr_t)x & 15) && !((uintptr_t)y & 15);
    const dim3 grid((unsigned)(planes * bpp)), wg(256);
    if (vec) hipLaunchKernelGGL(im_kernel<true>, grid, wg, 0, (hipStream_t)stream, j, (int)bpp);
    else hipLaunchKernelGGL(im_kernel<false>, grid, wg, 0, (hipStream_t)stream, j, (int)bpp);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
