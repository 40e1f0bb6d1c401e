// Training patches cut from an unscaled volume, a share of them forced onto the foreground (include/vaeseg.h: vs_patch_index, vs_patch_pick,
// vs_patch_gather; DESIGN.md 3.19 holds the rule).
//
// The one non-trivial step is "a uniformly random voxel of class k" without np.argwhere on the host or torch.nonzero on the device: a ranked select
// over the label's positions.
//
//   index    the label is read once, as one flat string of V voxels in chunks of VS_PATCH_CHUNK.  A workgroup owns whole chunks: a wave takes a quarter
//            of the chunk 64 voxels at a time, every lane classifies its voxel, and a class's count is the popcount of the ballot of its lanes; the
//            four waves' counts meet in LDS and one thread per class stores the chunk's word.  A second launch, one workgroup per class, turns the
//            column into exclusive prefix counts in place and appends the total.
//   pick     a wave per request.  The totals row gives the classes present and n_k, the request's words give k and the rank r; a binary search in the
//            class's column finds the chunk that holds rank r, and the wave walks that chunk 64 voxels at a time (eight loads in flight), subtracting
//            ballot popcounts until the r-th match lies in the current 64: the lane whose match has exactly the missing number of matches below it.
//            Every label read is one contiguous run of 64 elements.  The linear index becomes (z, y, x), the clamp makes the origin.
//   gather   vs_sw_gather's row copy (window.hip) with signed origins from device memory, a margin, per-axis patch sides and up to four sources with
//            their own cval: a thread owns four x of an output row, stores 16 bytes, loads 16 bytes where the source quad is inside the row and
//            aligned, element by element with guards otherwise.  Positions are 64-bit: an origin may be any integer.
//
// No atomics, no memset, no workspace: every word of the table and of the outputs has one writer, so the bits are the same eagerly, under graph
// replay and in both builds.
#include <limits.h>
#include "common.h"

namespace {

constexpr int PI_CHUNK = VS_PATCH_CHUNK;
constexpr int PI_MAX_CLASS = 8;
constexpr int PI_GRID_CAP = 8192;
constexpr int PP_UNROLL = 8;                   // pick: 64-voxel steps whose loads are issued together
constexpr long long PG_GRID_CAP = 1 << 20;
static_assert(PI_CHUNK % (256 * 4) == 0, "a wave of the index kernel takes a quarter of a chunk in whole groups of four 64-voxel steps");
static_assert(PI_CHUNK % (64 * PP_UNROLL) == 0, "the pick walks a chunk in whole groups of PP_UNROLL steps");

// the class of a label value: the integer itself when it is one in [0, n_class), -1 otherwise (NaN fails every comparison)
__device__ __forceinline__ int pi_class(float v, int n_class) { return (v >= 0.f && v < (float)n_class && v == truncf(v)) ? (int)v : -1; }
__device__ __forceinline__ int pi_class(unsigned char v, int n_class) { return (int)v < n_class ? (int)v : -1; }

// (w * m) >> 32 with a 64-bit product: a word onto a range of m values, m >= 1
__device__ __forceinline__ unsigned int pp_map(unsigned int w, unsigned int m) { return (unsigned int)(((unsigned long long)w * (unsigned long long)m) >> 32); }

// ---- index ----------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pi_count_kernel(const T* __restrict__ label, int* __restrict__ table, int V, int n_chunks, int n_class) {
    __shared__ int part[4][PI_MAX_CLASS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {           // workgroup-uniform: every lane reaches every ballot
        const long long base = (long long)chunk * PI_CHUNK + wave * (PI_CHUNK / 4) + lane;
        int cnt[PI_MAX_CLASS];
#pragma unroll
        for (int c = 0; c < PI_MAX_CLASS; ++c) cnt[c] = 0;
        for (int it = 0; it < PI_CHUNK / 256; it += 4) {
            int k[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long v = base + (long long)(it + u) * 64;
                k[u] = v < V ? pi_class(label[v], n_class) : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int c = 0; c < PI_MAX_CLASS; ++c)
                    if (c < n_class) cnt[c] += __popcll(__ballot(k[u] == c));
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < PI_MAX_CLASS; ++c) part[wave][c] = cnt[c];
        }
        __syncthreads();
        if ((int)threadIdx.x < n_class) {
            const int c = threadIdx.x;
            table[(size_t)chunk * n_class + c] = part[0][c] + part[1][c] + part[2][c] + part[3][c];
        }
        __syncthreads();                                                            // part is rewritten for the next chunk
    }
}

// one workgroup per class: the column of chunk counts -> exclusive prefix counts, in place; the total goes to row n_chunks
__global__ __launch_bounds__(256) void pi_scan_kernel(int* table, int n_chunks, int n_class) {
    __shared__ int lds[4];
    const int c = blockIdx.x;
    int base = 0;
    for (int t0 = 0; t0 < n_chunks; t0 += 256) {
        const int i = t0 + (int)threadIdx.x;
        const int val = i < n_chunks ? table[(size_t)i * n_class + c] : 0;
        int tot;
        const int ex = block_excl_scan<256>(val, &tot, lds);
        if (i < n_chunks) table[(size_t)i * n_class + c] = base + ex;
        base += tot;
    }
    if (threadIdx.x == 0) table[(size_t)n_chunks * n_class + c] = base;
}

// ---- pick -----------------------------------------------------------------------------------------------------------------------------------
struct pp_job {
    const int* table;
    const unsigned int* words;
    const int* forced;
    int* picks;
    int n_class, n_sel, classes;
    int d, h, w, V, n_chunks;
    int p[3];
};

// the bounds of an axis and an origin inside them
__device__ __forceinline__ void pp_bounds(int s, int p, int& lb, int& ub) {
    const int need = p > s ? p - s : 0;
    lb = -(need / 2);
    ub = s + need / 2 + need % 2 - p;
}
__device__ __forceinline__ int pp_origin(bool have, int v, unsigned int word, int s, int p) {
    int lb, ub;
    pp_bounds(s, p, lb, ub);
    if (have) {
        const int o = v - p / 2;
        return o < lb ? lb : (o > ub ? ub : o);
    }
    return lb + (int)pp_map(word, (unsigned int)(ub - lb + 1));
}

// a wave per request (blockDim.x == 64): everything but the label reads of the walk is wave-uniform
template <typename T>
__global__ __launch_bounds__(64) void pp_pick_kernel(const T* __restrict__ label, pp_job j) {
    const int lane = threadIdx.x, req = blockIdx.x;
    const unsigned int* W = j.words + 5 * (size_t)req;
    const unsigned int wc = W[0], wv = W[1];
    const int* totals = j.table + (size_t)j.n_chunks * j.n_class;
    int mc = 0;
    for (int i = 0; i < j.n_sel; ++i) mc += totals[(j.classes >> (3 * i)) & 7] > 0;
    int k = -1, vlin = -1;
    if (j.forced[req] != 0 && mc > 0) {
        const int want = (int)pp_map(wc, (unsigned int)mc);
        int nk = 0;
        for (int i = 0, seen = 0; i < j.n_sel; ++i) {                               // the want-th class of the list that is present
            const int c = (j.classes >> (3 * i)) & 7, n = totals[c];
            if (n > 0 && seen++ == want) { k = c; nk = n; }
        }
        const int r = (int)pp_map(wv, (unsigned int)nk);
        int lo = 0, hi = j.n_chunks - 1;                                            // the last chunk whose prefix count is <= r holds rank r
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (j.table[(size_t)mid * j.n_class + k] <= r) lo = mid; else hi = mid - 1;
        }
        int rem = r - j.table[(size_t)lo * j.n_class + k];
        const long long base = (long long)lo * PI_CHUNK + lane;
        for (int s0 = 0; s0 < PI_CHUNK / 64 && vlin < 0; s0 += PP_UNROLL) {
            bool match[PP_UNROLL];
#pragma unroll
            for (int u = 0; u < PP_UNROLL; ++u) {
                const long long v = base + (long long)(s0 + u) * 64;
                match[u] = v < j.V && pi_class(label[v], j.n_class) == k;
            }
#pragma unroll
            for (int u = 0; u < PP_UNROLL; ++u) {
                const unsigned long long m = __ballot(match[u]);
                const int c = __popcll(m);
                if (vlin < 0) {
                    if (rem < c) {
                        const int below = __popcll(m & ((1ull << lane) - 1ull));
                        const unsigned long long hit = __ballot(match[u] && below == rem);
                        vlin = lo * PI_CHUNK + (s0 + u) * 64 + (__ffsll((long long)hit) - 1);
                    } else {
                        rem -= c;
                    }
                }
            }
        }
        if (vlin < 0) k = -1;                                                       // a table that is not this label's: a free origin
    }
    const bool have = vlin >= 0;
    int vz = -1, vy = -1, vx = -1;
    if (have) {
        vz = vlin / (j.h * j.w);
        const int rest = vlin - vz * (j.h * j.w);
        vy = rest / j.w;
        vx = rest - vy * j.w;
    }
    if (lane == 0) {
        int4* out = reinterpret_cast<int4*>(j.picks + 8 * (size_t)req);
        out[0] = make_int4(pp_origin(have, vz, W[2], j.d, j.p[0]), pp_origin(have, vy, W[3], j.h, j.p[1]), pp_origin(have, vx, W[4], j.w, j.p[2]), k);
        out[1] = make_int4(vz, vy, vx, 0);
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------------------
struct pg_job {
    const float* src[4];
    float cval[4];
    const int* picks;
    float* out;
    int n_src, r, d, h, w, margin;
    int q[3];
};

__device__ __forceinline__ bool pg_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__global__ __launch_bounds__(256) void pg_gather_kernel(pg_job g, int nq, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % nq);
        long long t = i / nq;
        const int ly = (int)(t % g.q[1]);
        t /= g.q[1];
        const int lz = (int)(t % g.q[0]);
        t /= g.q[0];
        const int req = (int)(t % g.r), s = (int)(t / g.r);
        const int lx = 4 * q, n = g.q[2] - lx < 4 ? g.q[2] - lx : 4;
        const float* vol = s == 0 ? g.src[0] : (s == 1 ? g.src[1] : (s == 2 ? g.src[2] : g.src[3]));
        const float cval = s == 0 ? g.cval[0] : (s == 1 ? g.cval[1] : (s == 2 ? g.cval[2] : g.cval[3]));
        const int* pk = g.picks + 8 * (size_t)req;
        const long long z = (long long)pk[0] - g.margin + lz, y = (long long)pk[1] - g.margin + ly, x = (long long)pk[2] - g.margin + lx;
        float v[4] = {cval, cval, cval, cval};
        if (z >= 0 && z < g.d && y >= 0 && y < g.h && x > -4 && x < g.w) {          // the row exists and the quad touches it
            const long long row = (z * g.h + y) * g.w;
            if (n == 4 && x >= 0 && x + 4 <= g.w && pg_aligned16(vol + row + x)) {
                const float4 f = *reinterpret_cast<const float4*>(vol + row + x);
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n && x + e >= 0 && x + e < g.w) v[e] = vol[row + x + e];
            }
        }
        float* dp = g.out + ((((size_t)s * g.r + req) * g.q[0] + lz) * g.q[1] + ly) * g.q[2] + lx;
        if (n == 4 && pg_aligned16(dp)) {
            *reinterpret_cast<float4*>(dp) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) dp[e] = v[e];
        }
    }
}

// d, h, w >= 1 with fewer than 2^31 voxels
bool pi_dims_ok(int d, int h, int w) { return d > 0 && h > 0 && w > 0 && (long long)d * h * w <= INT_MAX; }
int pi_chunks(int d, int h, int w) { return (int)(((long long)d * h * w + PI_CHUNK - 1) / PI_CHUNK); }

int pi_label_check(const void* label, int dtype, int d, int h, int w, int n_class) {
    if (!label || n_class < 1 || n_class > PI_MAX_CLASS) return VS_EINVAL;
    if (dtype != VS_PATCH_F32 && dtype != VS_PATCH_U8) return VS_EDTYPE;
    if (!pi_dims_ok(d, h, w)) return VS_ESHAPE;
    if (dtype == VS_PATCH_F32 && ((uintptr_t)label & 3)) return VS_EALIGN;
    return VS_OK;
}

}  // namespace

extern "C" int vs_patch_chunk(void) { return PI_CHUNK; }

extern "C" size_t vs_patch_index_bytes(int d, int h, int w, int n_class) {
    if (!pi_dims_ok(d, h, w) || n_class < 1 || n_class > PI_MAX_CLASS) return 0;
    return ((size_t)pi_chunks(d, h, w) + 1) * (size_t)n_class * sizeof(int);
}

extern "C" int vs_patch_index(const void* label, int dtype, int d, int h, int w, int n_class, int* table, void* stream) {
    const int rc = pi_label_check(label, dtype, d, h, w, n_class);
    if (rc != VS_OK) return rc;
    if (!table || (const void*)table == label) return VS_EINVAL;
    if ((uintptr_t)table & 3) return VS_EALIGN;
    const int V = d * h * w, n_chunks = pi_chunks(d, h, w);
    const dim3 grid((unsigned)(n_chunks < PI_GRID_CAP ? n_chunks : PI_GRID_CAP)), wg(256);
    if (dtype == VS_PATCH_F32)
        hipLaunchKernelGGL(pi_count_kernel<float>, grid, wg, 0, (hipStream_t)stream, (const float*)label, table, V, n_chunks, n_class);
    else
        hipLaunchKernelGGL(pi_count_kernel<unsigned char>, grid, wg, 0, (hipStream_t)stream, (const unsigned char*)label, table, V, n_chunks, n_class);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(pi_scan_kernel, dim3((unsigned)n_class), wg, 0, (hipStream_t)stream, table, n_chunks, n_class);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_patch_pick(const void* label, int dtype, const int* table, int n_class, int n_sel, int classes, const unsigned int* words, const int* forced,
                             int r, int d, int h, int w, int pd, int ph, int pw, int* picks, void* stream) {
    const int rc = pi_label_check(label, dtype, d, h, w, n_class);
    if (rc != VS_OK) return rc;
    if (!table || !words || !forced || !picks || r < 1 || pd < 1 || ph < 1 || pw < 1) return VS_EINVAL;
    if (n_sel < 0 || n_sel > PI_MAX_CLASS || classes < 0 || (n_sel < PI_MAX_CLASS && (classes >> (3 * n_sel)) != 0)) return VS_EINVAL;
    for (int i = 0, last = -1; i < n_sel; ++i) {                                    // strictly ascending inside [0, n_class)
        const int c = (classes >> (3 * i)) & 7;
        if (c <= last || c >= n_class) return VS_EINVAL;
        last = c;
    }
    if (((uintptr_t)table & 3) || ((uintptr_t)words & 3) || ((uintptr_t)forced & 3) || ((uintptr_t)picks & 15)) return VS_EALIGN;
    pp_job j = {};
    j.table = table; j.words = words; j.forced = forced; j.picks = picks;
    j.n_class = n_class; j.n_sel = n_sel; j.classes = classes;
    j.d = d; j.h = h; j.w = w; j.V = d * h * w; j.n_chunks = pi_chunks(d, h, w);
    j.p[0] = pd; j.p[1] = ph; j.p[2] = pw;
    if (dtype == VS_PATCH_F32)
        hipLaunchKernelGGL(pp_pick_kernel<float>, dim3((unsigned)r), dim3(64), 0, (hipStream_t)stream, (const float*)label, j);
    else
        hipLaunchKernelGGL(pp_pick_kernel<unsigned char>, dim3((unsigned)r), dim3(64), 0, (hipStream_t)stream, (const unsigned char*)label, j);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_patch_gather(const float* src0, const float* src1, const float* src2, const float* src3, float cval0, float cval1, float cval2, float cval3,
                               int n_src, const int* picks, int r, int d, int h, int w, int pd, int ph, int pw, int margin, float* out, void* stream) {
    if (n_src < 1 || n_src > 4 || !picks || !out || r < 1 || pd < 1 || ph < 1 || pw < 1 || margin < 0) return VS_EINVAL;
    pg_job g = {};
    const float* src[4] = {src0, src1, src2, src3};
    const float cval[4] = {cval0, cval1, cval2, cval3};
    for (int s = 0; s < n_src; ++s) {
        if (!src[s] || src[s] == out || !(cval[s] == cval[s])) return VS_EINVAL;
        g.src[s] = src[s];
        g.cval[s] = cval[s];
    }
    if (!pi_dims_ok(d, h, w)) return VS_ESHAPE;
    const long long qd = (long long)pd + 2ll * margin, qh = (long long)ph + 2ll * margin, qw = (long long)pw + 2ll * margin;
    if (qd > INT_MAX || qh > INT_MAX || qw > INT_MAX || (double)qd * (double)qh * (double)qw >= 2147483648.0) return VS_ESHAPE;
    if ((double)n_src * (double)r * (double)qd * (double)qh * (double)qw >= 0x1p46) return VS_ESHAPE;      // the thread count stays far inside 64 bits
    for (int s = 0; s < n_src; ++s)
        if ((uintptr_t)src[s] & 15) return VS_EALIGN;
    if (((uintptr_t)out & 15) || ((uintptr_t)picks & 15)) return VS_EALIGN;
    g.picks = picks; g.out = out;
    g.n_src = n_src; g.r = r; g.d = d; g.h = h; g.w = w; g.margin = margin;
    g.q[0] = (int)qd; g.q[1] = (int)qh; g.q[2] = (int)qw;
    const int nq = (int)((qw + 3) / 4);
    const long long total = (long long)n_src * r * qd * qh * nq;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(pg_gather_kernel, dim3((unsigned)(blocks > PG_GRID_CAP ? PG_GRID_CAP : blocks)), dim3(256), 0, (hipStream_t)stream, g, nq, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
