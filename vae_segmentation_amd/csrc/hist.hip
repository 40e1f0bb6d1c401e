// Intensity histograms, joint histograms and mutual information (include/vaeseg.h: vs_histogram, vs_joint_histogram, vs_mutual_information).
//
// Inputs are planar fp32 (n, c, d, h, w); every (n, c) plane is its own problem and is read as one flat string of V = d*h*w voxels.
//
//   bounds    "from the data": the finite minimum and maximum of a plane are folded with atomicMin / atomicMax on the order-preserving integer image
//             of an fp32 value, in the first and last slot of the plane's own edge table (the caller's buffer: no workspace, nothing read back).
//   edges     one workgroup per plane and variable writes e_i = i * step + lo in fp64 with the product and the sum rounded separately
//             (hs_edge: contraction off), e_B = hi.  These are the bits of np.linspace(lo, hi, B + 1).
//   binning   a voxel is promoted to fp64, an estimate (x - e_0) * B / (e_B - e_0) proposes a bin and the edge table decides: the bin moves down
//             while x < e_i and up while x >= e_{i+1}, so e_i <= x < e_{i+1} holds on leaving (x == e_B stays in bin B - 1).
//   counting  three forms, chosen by the table's cells per plane (hs_pick_form):
//               HS_LDS32   32-bit counters in LDS (<= HS_LDS32_CELLS cells), flushed once per workgroup, non-zero cells only;
//               HS_PACKED  two 16-bit counters per LDS word (<= HS_PACKED_CELLS cells, 128 KB: one workgroup per CU).  A workgroup counts
//                          HS_WG_VOXELS voxels before it flushes and HS_WG_VOXELS < 2^16 (static_assert below), so no half can carry into the other;
//               HS_GLOBAL  a wave walks a chunk of the plane, carries ONE (cell, count) record in wave-uniform registers and issues 64-bit global
//                          atomics for the other cells.
//             In all three a run of equal cells along x is ONE update of the run's length (csrc/regions.hip's ballot of run heads): the cell
//             that holds the air of a CT volume does not serialise.
//
// Every count is an integer added by vector-lane atomics: the tables do not depend on the order of arrival — both builds of the library, eager
// launches and graph replay give the same bits.  The first launch of a call writes the initial state of every output; nothing is allocated,
// synchronised or read back and no kernel waits for another workgroup.
//
// vs_mutual_information restates the tail of the reference's mutual_information_3d (utils/utils.py:824-845) in fp64 on the int64 table: every sum
// is a per-thread strided sum followed by a fixed tree over the workgroup's 256 partials — no floating-point atomics, the same bits on every run.
#include <limits.h>
#include <math.h>
#include "volume.h"

namespace {

constexpr int HS_LDS32_CELLS = 8192;          // 32 KB of 32-bit counters
constexpr int HS_PACKED_CELLS = 65536;        // 128 KB of 16-bit counter pairs (a 256 x 256 joint histogram)
constexpr int HS_WG_VOXELS = 16384;           // voxels a workgroup counts in LDS before its one flush
constexpr int HS_UNROLL = 4;                  // voxels per thread whose loads are issued before the first is binned
constexpr int HS_CHUNK = 32;                  // 64-voxel segments a wave walks with one pending record (HS_GLOBAL)
constexpr int HS_MAX_BINS = 4096;             // vs_histogram
constexpr long long HS_MAX_CELLS = 1ll << 22;
constexpr int HS_MAX_RADIUS = 64;             // of the Gaussian of vs_mutual_information: its weights travel as a kernel argument
static_assert(HS_WG_VOXELS < 65536, "a 16-bit half of a packed LDS counter must not carry: a workgroup flushes before it has counted 2^16 voxels");
static_assert(HS_WG_VOXELS % (256 * HS_UNROLL) == 0, "every thread of a workgroup runs the same trip count");

enum { HS_AUTO = 0, HS_LDS32 = 1, HS_PACKED = 2, HS_GLOBAL = 3 };

// np.linspace's edge: the product and the sum are rounded separately
__device__ __forceinline__ double hs_edge(int i, double step, double lo) {
#pragma clang fp contract(off)
    const double p = (double)i * step;
    return p + lo;
}

struct hs_job {
    const float* x;
    const float* y;            // NULL: one variable
    const int* labels;         // NULL: one row
    double* ex;                // (planes, bx + 1)
    double* ey;                // (planes, by + 1), NULL with y
    i64* table;                // (planes, ncells)
    i64* outside;              // (planes)
    int* overflow;             // (planes), NULL without labels
    int bx, by, rows, V, ncells;
    long long planes;
    double lo_x, hi_x, lo_y, hi_y;
    int from_data;
};

struct hs_axis {
    const double* E;
    double e0, eB, inv;
    int B;
    __device__ __forceinline__ void load(const double* edges, int bins) {
        E = edges;
        B = bins;
        e0 = edges[0];
        eB = edges[bins];
        inv = (double)bins / (eB - e0);
    }
    // the bin of x, or -1 for NaN, +-inf and values outside [e_0, e_B]
    __device__ __forceinline__ int bin(float xf) const {
        const double x = (double)xf;
        if (!(x >= e0 && x <= eB)) return -1;
        int i = (int)fmin((x - e0) * inv, (double)(B - 1));            // an estimate in [0, B - 1] (a NaN estimate gives B - 1) ...
        while (i > 0 && x < E[i]) --i;                                  // ... and the edge table decides
        while (i < B - 1 && x >= E[i + 1]) ++i;
        return i;
    }
};

// the cell of a voxel: >= 0, -1 (outside the range) or -2 (a label outside [0, rows])
__device__ __forceinline__ int hs_key(const hs_job& j, const hs_axis& ax, const hs_axis& ay, float xv, float yv, int lab) {
    int base = 0;
    if (j.labels) {
        if (lab < 0 || lab > j.rows) return -2;
        base = lab * j.bx;
    }
    const int ix = ax.bin(xv);
    if (ix < 0) return -1;
    if (!j.y) return base + ix;
    const int iy = ay.bin(yv);
    return iy < 0 ? -1 : ix * j.by + iy;
}

__global__ __launch_bounds__(256) void hs_init_kernel(hs_job j) {
    const long long cells = j.planes * j.ncells;
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long i = i0; i < cells; i += stride) j.table[i] = 0;
    for (long long i = i0; i < j.planes; i += stride) {
        j.outside[i] = 0;
        if (j.overflow) j.overflow[i] = 0;
        if (j.from_data) {                                   // the slots of the running minimum / maximum: "no finite voxel yet"
            u64* sx = reinterpret_cast<u64*>(j.ex + i * (j.bx + 1));
            sx[0] = 0xffffffffull;
            sx[j.bx] = 0ull;
            if (j.y) {
                u64* sy = reinterpret_cast<u64*>(j.ey + i * (j.by + 1));
                sy[0] = 0xffffffffull;
                sy[j.by] = 0ull;
            }
        }
    }
}

__device__ __forceinline__ void hs_minmax_fold(float v, bool live, unsigned int& mn, unsigned int& mx) {
    if (live && key_finite(v)) {
        const unsigned int e = key_enc(v);
        mn = min(mn, e);
        mx = max(mx, e);
    }
}

__device__ __forceinline__ void hs_minmax_commit(unsigned int mn, unsigned int mx, u64* slots, int bins, int lane) {
    for (int s = 32; s > 0; s >>= 1) {
        mn = min(mn, (unsigned int)__shfl_xor((int)mn, s));
        mx = max(mx, (unsigned int)__shfl_xor((int)mx, s));
    }
    if (lane == 0 && mn <= mx) {
        atomicMin(slots, (u64)mn);
        atomicMax(slots + bins, (u64)mx);
    }
}

// a workgroup per HS_WG_VOXELS voxels of one plane
__global__ __launch_bounds__(256) void hs_minmax_kernel(hs_job j, int blocks_per_plane) {
    const long long plane = blockIdx.x / blocks_per_plane;
    const int v0 = (int)(blockIdx.x - plane * blocks_per_plane) * HS_WG_VOXELS;
    const float* X = j.x + (size_t)plane * j.V;
    const float* Y = j.y ? j.y + (size_t)plane * j.V : nullptr;
    unsigned int mnx = 0xffffffffu, mxx = 0u, mny = 0xffffffffu, mxy = 0u;
    for (int it = 0; it < HS_WG_VOXELS / 256; ++it) {
        const long long v = (long long)v0 + it * 256 + threadIdx.x;
        const bool live = v < j.V;
        hs_minmax_fold(live ? X[v] : 0.f, live, mnx, mxx);
        if (Y) hs_minmax_fold(live ? Y[v] : 0.f, live, mny, mxy);
    }
    const int lane = threadIdx.x & 63;
    hs_minmax_commit(mnx, mxx, reinterpret_cast<u64*>(j.ex + plane * (j.bx + 1)), j.bx, lane);
    if (Y) hs_minmax_commit(mny, mxy, reinterpret_cast<u64*>(j.ey + plane * (j.by + 1)), j.by, lane);
}

// a workgroup per plane and variable (blockIdx.y): bounds -> the B + 1 edges
__global__ __launch_bounds__(256) void hs_edges_kernel(hs_job j) {
    __shared__ double bounds[2];
    const long long plane = blockIdx.x;
    const bool second = blockIdx.y == 1;
    const int B = second ? j.by : j.bx;
    double* E = (second ? j.ey : j.ex) + plane * (B + 1);
    if (threadIdx.x == 0) {
        double lo = second ? j.lo_y : j.lo_x, hi = second ? j.hi_y : j.hi_x;
        if (j.from_data) {
            const u64 mn = reinterpret_cast<const u64*>(E)[0], mx = reinterpret_cast<const u64*>(E)[B];
            lo = hi = 0.0;
            if (mn <= mx) {                                  // + 0.0: a zero bound is +0.0 whichever zero the data held
                lo = (double)key_dec((unsigned int)mn) + 0.0;
                hi = (double)key_dec((unsigned int)mx) + 0.0;
            }
        }
        if (lo == hi) {
            lo -= 0.5;
            hi += 0.5;
        }
        bounds[0] = lo;
        bounds[1] = hi;
    }
    __syncthreads();                                         // the slots are read before any edge is written
    const double lo = bounds[0], hi = bounds[1];
    const double step = (hi - lo) / (double)B;
    for (int i = threadIdx.x; i <= B; i += 256) E[i] = i == B ? hi : hs_edge(i, step, lo);
}

// a workgroup per HS_WG_VOXELS voxels of one plane, the plane's table in LDS
template <bool PACKED>
__global__ __launch_bounds__(256) void hs_count_lds_kernel(hs_job j, int blocks_per_plane) {
    constexpr int WORDS = PACKED ? HS_PACKED_CELLS / 2 : HS_LDS32_CELLS;
    __shared__ unsigned int cells[WORDS];
    __shared__ int out_total, bad_total;
    const int lane = threadIdx.x & 63;
    const int nwords = PACKED ? (j.ncells + 1) / 2 : j.ncells;          // <= WORDS: the launcher picks this form for such tables only
    const long long plane = blockIdx.x / blocks_per_plane;
    const int v0 = (int)(blockIdx.x - plane * blocks_per_plane) * HS_WG_VOXELS;
    for (int i = threadIdx.x; i < nwords; i += 256) cells[i] = 0u;
    if (threadIdx.x == 0) out_total = bad_total = 0;
    hs_axis ax, ay;
    ax.load(j.ex + plane * (j.bx + 1), j.bx);
    ay = ax;
    if (j.y) ay.load(j.ey + plane * (j.by + 1), j.by);
    __syncthreads();
    const float* X = j.x + (size_t)plane * j.V;
    const float* Y = j.y ? j.y + (size_t)plane * j.V : nullptr;
    const int* L = j.labels ? j.labels + (size_t)plane * j.V : nullptr;
    int out = 0, bad = 0;
    // every thread runs the same trip count: the ballots need all lanes.  A workgroup adds at most HS_WG_VOXELS to all of its counters together.
    for (int it = 0; it < HS_WG_VOXELS / 256; it += HS_UNROLL) {
        float xv[HS_UNROLL], yv[HS_UNROLL];
        int lab[HS_UNROLL];
#pragma unroll
        for (int u = 0; u < HS_UNROLL; ++u) {
            const long long v = (long long)v0 + (it + u) * 256 + threadIdx.x;
            const bool live = v < j.V;
            xv[u] = live ? X[v] : 0.f;
            yv[u] = live && Y ? Y[v] : 0.f;
            lab[u] = live && L ? L[v] : 0;
        }
#pragma unroll
        for (int u = 0; u < HS_UNROLL; ++u) {
            const long long v = (long long)v0 + (it + u) * 256 + threadIdx.x;
            const int key = v < j.V ? hs_key(j, ax, ay, xv[u], yv[u], lab[u]) : -3;
            out += __popcll(__ballot(key == -1));
            bad += __popcll(__ballot(key == -2));
            const int below = __shfl_up(key, 1);
            const bool head = lane == 0 || key != below;
            const u64 heads = __ballot(head);
            if (head && key >= 0) {
                const unsigned int len = (unsigned int)run_length(heads, lane);
                if (PACKED) atomicAdd(&cells[key >> 1], len << ((key & 1) * 16));
                else atomicAdd(&cells[key], len);
            }
        }
    }
    if (lane == 0) {
        if (out) atomicAdd(&out_total, out);
        if (bad) atomicAdd(&bad_total, bad);
    }
    __syncthreads();
    i64* T = j.table + (size_t)plane * j.ncells;
    for (int i = threadIdx.x; i < nwords; i += 256) {
        const unsigned int c = cells[i];
        if (!c) continue;
        if (PACKED) {
            if (c & 0xffffu) run_add(T + 2 * i, (i64)(c & 0xffffu));
            if (c >> 16) run_add(T + 2 * i + 1, (i64)(c >> 16));        // a key 2 i + 1 was counted, so the cell exists
        } else {
            run_add(T + i, (i64)c);
        }
    }
    if (threadIdx.x == 0) {
        if (out_total) run_add(j.outside + plane, (i64)out_total);
        if (bad_total) atomicAdd(j.overflow + plane, bad_total);       // labels were given, so overflow is a buffer
    }
}

// a wave per chunk of HS_CHUNK 64-voxel segments of one plane, a pending (cell, count) in wave-uniform registers
__global__ __launch_bounds__(256) void hs_count_global_kernel(hs_job j, long long chunks) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long job = wave0; job < j.planes * chunks; job += nwaves) {
        const long long plane = job / chunks;
        const long long v0 = (job - plane * chunks) * (HS_CHUNK * 64);
        const float* X = j.x + (size_t)plane * j.V;
        const float* Y = j.y ? j.y + (size_t)plane * j.V : nullptr;
        const int* L = j.labels ? j.labels + (size_t)plane * j.V : nullptr;
        i64* T = j.table + (size_t)plane * j.ncells;
        hs_axis ax, ay;
        ax.load(j.ex + plane * (j.bx + 1), j.bx);
        ay = ax;
        if (j.y) ay.load(j.ey + plane * (j.by + 1), j.by);
        int pend_key = -1, out = 0, bad = 0;
        i64 pend_cnt = 0;
        for (int it = 0; it < HS_CHUNK; ++it) {
            const long long v = v0 + it * 64 + lane;
            if (v0 + it * 64 >= j.V) break;                               // wave-uniform
            const bool live = v < j.V;
            const int key = live ? hs_key(j, ax, ay, X[v], Y ? Y[v] : 0.f, L ? L[v] : 0) : -3;
            out += __popcll(__ballot(key == -1));
            bad += __popcll(__ballot(key == -2));
            const u64 counted = __ballot(key >= 0);
            if (!counted) continue;
            u64 m = pend_key >= 0 ? __ballot(key == pend_key) : 0ull;
            if (!m) {
                if (pend_key >= 0 && lane == 0) run_add(T + pend_key, pend_cnt);
                pend_key = __shfl(key, run_ctz(counted));
                pend_cnt = 0;
                m = __ballot(key == pend_key);
            }
            pend_cnt += __popcll(m);
            const int below = __shfl_up(key, 1);
            const bool head = lane == 0 || key != below;
            const u64 heads = __ballot(head);
            if (head && key >= 0 && key != pend_key) run_add(T + key, (i64)run_length(heads, lane));
        }
        if (lane == 0) {
            if (pend_key >= 0) run_add(T + pend_key, pend_cnt);
            if (out) run_add(j.outside + plane, (i64)out);
            if (bad) atomicAdd(j.overflow + plane, bad);
        }
    }
}

unsigned hs_grid(long long blocks) {
    const long long cap = 1 << 20;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// The form that serves a table of `ncells` cells per plane.  vs_config.hist_form forces one where the table fits it (measurements: tools/bench_hist.py).
int hs_pick_form(long long ncells) {
    const int forced = vs_cfg().hist_form;
    if (forced == HS_GLOBAL) return HS_GLOBAL;
    if (forced == HS_PACKED && ncells <= HS_PACKED_CELLS) return HS_PACKED;
    if (forced == HS_LDS32 && ncells <= HS_LDS32_CELLS) return HS_LDS32;
    if (ncells <= HS_LDS32_CELLS) return HS_LDS32;
    if (ncells <= HS_PACKED_CELLS) return HS_PACKED;
    return HS_GLOBAL;
}

int hs_bounds_ok(double lo, double hi) { return isfinite(lo) && isfinite(hi) && lo <= hi; }

// the launches of both histogram calls; j is complete and checked
int hs_run(const hs_job& j, hipStream_t st) {
    const long long bpp = ((long long)j.V + HS_WG_VOXELS - 1) / HS_WG_VOXELS;
    if (j.planes * bpp > INT_MAX) return VS_ESHAPE;                       // one workgroup per piece of a plane
    const long long cells = j.planes * j.ncells;
    hipLaunchKernelGGL(hs_init_kernel, dim3(hs_grid((cells + 255) / 256)), dim3(256), 0, st, j);
    VS_CHECK_LAUNCH();
    if (j.from_data) {
        hipLaunchKernelGGL(hs_minmax_kernel, dim3((unsigned)(j.planes * bpp)), dim3(256), 0, st, j, (int)bpp);
        VS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(hs_edges_kernel, dim3((unsigned)j.planes, j.y ? 2 : 1), dim3(256), 0, st, j);
    VS_CHECK_LAUNCH();
    const int form = hs_pick_form(j.ncells);
    if (form == HS_LDS32) {
        hipLaunchKernelGGL(hs_count_lds_kernel<false>, dim3((unsigned)(j.planes * bpp)), dim3(256), 0, st, j, (int)bpp);
    } else if (form == HS_PACKED) {
        hipLaunchKernelGGL(hs_count_lds_kernel<true>, dim3((unsigned)(j.planes * bpp)), dim3(256), 0, st, j, (int)bpp);
    } else {
        const long long chunks = ((long long)j.V + HS_CHUNK * 64 - 1) / (HS_CHUNK * 64);
        hipLaunchKernelGGL(hs_count_global_kernel, dim3(hs_grid((j.planes * chunks + 3) / 4)), dim3(256), 0, st, j, chunks);
    }
    VS_CHECK_LAUNCH();
    return VS_OK;
}

int hs_shape(int n, int c, int d, int h, int w, hs_job* j) {
    if (n <= 0 || c <= 0 || d <= 0 || h <= 0 || w <= 0) return VS_ESHAPE;
    const long long V = (long long)d * h * w;
    if (V > INT_MAX) return VS_ESHAPE;                                    // plane-local indices and the overflow counts are int32
    j->V = (int)V;
    j->planes = (long long)n * c;
    if (j->planes > INT_MAX) return VS_ESHAPE;
    return VS_OK;
}

// ---- mutual information ----------------------------------------------------------------------------------------------------------------

struct mi_weights {
    double w[HS_MAX_RADIUS + 1];      // w[k] for the offsets +-k, normalised
    int radius;
};

// the sum of one value per thread: a fixed tree over the 256 partials, the same on every run
__device__ __forceinline__ double mi_block_sum(double v, double* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    const double r = part[0];
    __syncthreads();
    return r;
}

// sum of `len` values `stride` apart: per-thread strided partials in ascending order, then the tree
__device__ __forceinline__ double mi_strided_sum(const double* p, long long len, long long stride, double* part) {
    double s = 0.0;
    for (long long i = threadIdx.x; i < len; i += 256) s += p[i * stride];
    return mi_block_sum(s, part);
}

// one thread per cell: scipy's correlate1d with the symmetric Gaussian along AXIS (0: the x bins, 1: the y bins), zeros beyond the table
// ("constant").  SRC is the int64 table (converted on load) or the fp64 result of the other axis; `add` is added to every result.
template <int AXIS, typename SRC>
__global__ __launch_bounds__(256) void mi_filter_kernel(const SRC* __restrict__ in, double* __restrict__ out, long long planes, int bx, int by,
                                                        mi_weights g, double add) {
    const long long cells = (long long)bx * by, total = planes * cells;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long plane = t / cells, cell = t - plane * cells;
        const int i = (int)(cell / by), jj = (int)(cell - (long long)i * by);
        const SRC* P = in + plane * cells;
        const int pos = AXIS == 0 ? i : jj, len = AXIS == 0 ? bx : by;
        const long long stride = AXIS == 0 ? by : 1;
        double acc = (double)P[cell] * g.w[0];
        for (int k = 1; k <= g.radius; ++k) {
            double pair = 0.0;
            if (pos - k >= 0) pair += (double)P[cell - k * stride];
            if (pos + k < len) pair += (double)P[cell + k * stride];
            acc += pair * g.w[k];
        }
        out[t] = acc + add;
    }
}

// blockIdx.x < bx: the sum of row i of the smoothed table -> rows[i]; otherwise of column blockIdx.x - bx -> cols[...]; blockIdx.y: the plane
__global__ __launch_bounds__(256) void mi_marginals_kernel(const double* __restrict__ sm, double* __restrict__ rows, double* __restrict__ cols, int bx,
                                                           int by) {
    __shared__ double part[256];
    const long long plane = blockIdx.y, cells = (long long)bx * by;
    const double* P = sm + plane * cells;
    const int b = blockIdx.x;
    if (b < bx) {
        const double s = mi_strided_sum(P + (long long)b * by, by, 1, part);
        if (threadIdx.x == 0) rows[plane * bx + b] = s;
    } else {
        const double s = mi_strided_sum(P + (b - bx), bx, by, part);
        if (threadIdx.x == 0) cols[plane * by + (b - bx)] = s;
    }
}

// a workgroup per row i: ent[i] = sum_j p log p with p = sm[i][j] / total; every workgroup sums the same total in the same order
__global__ __launch_bounds__(256) void mi_entropy_kernel(const double* __restrict__ sm, const double* __restrict__ rows, double* __restrict__ ent, int bx,
                                                         int by) {
    __shared__ double part[256];
    const long long plane = blockIdx.y;
    const double total = mi_strided_sum(rows + plane * bx, bx, 1, part);
    const double* P = sm + (plane * bx + blockIdx.x) * (long long)by;
    double s = 0.0;
    for (int jj = threadIdx.x; jj < by; jj += 256) {
        const double p = P[jj] / total;
        s += p * log(p);
    }
    s = mi_block_sum(s, part);
    if (threadIdx.x == 0) ent[plane * bx + blockIdx.x] = s;
}

__device__ __forceinline__ double mi_plogp_sum(const double* p, int len, double total, double* part) {
    double s = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) {
        const double q = p[i] / total;
        s += q * log(q);
    }
    return mi_block_sum(s, part);
}

// a workgroup per plane
__global__ __launch_bounds__(256) void mi_final_kernel(const double* __restrict__ rows, const double* __restrict__ cols, const double* __restrict__ ent,
                                                       double* __restrict__ mi, int bx, int by, int normalized) {
    __shared__ double part[256];
    const long long plane = blockIdx.x;
    const double total = mi_strided_sum(rows + plane * bx, bx, 1, part);
    const double hr = mi_plogp_sum(rows + plane * bx, bx, total, part);
    const double hc = mi_plogp_sum(cols + plane * by, by, total, part);
    const double hj = mi_strided_sum(ent + plane * bx, bx, 1, part);
    if (threadIdx.x == 0) mi[plane] = normalized ? (hc + hr) / hj - 1.0 : hj - hc - hr;
}

}  // namespace

extern "C" int vs_histogram(const float* x, const int* labels, int n, int c, int d, int h, int w, int bins, int rows, double lo, double hi, int from_data,
                            double* edges, long long* table, long long* outside, int* overflow, void* stream) {
    hs_job j = {};
    const int rc = hs_shape(n, c, d, h, w, &j);
    if (rc != VS_OK) return rc;
    if (!x || !edges || !table || !outside || !overflow || bins < 1 || rows < 0 || (!labels && rows != 0)) return VS_EINVAL;
    if (!from_data && !hs_bounds_ok(lo, hi)) return VS_EINVAL;
    if (bins > HS_MAX_BINS || ((long long)rows + 1) * bins > HS_MAX_CELLS) return VS_ESHAPE;
    if (((uintptr_t)x & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)edges & 7) || ((uintptr_t)table & 7) || ((uintptr_t)outside & 7) ||
        ((uintptr_t)overflow & 3)) return VS_EALIGN;
    j.x = x; j.labels = labels;
    j.ex = edges;
    j.table = table; j.outside = outside; j.overflow = overflow;
    j.bx = bins; j.by = 1; j.rows = rows;
    j.ncells = (rows + 1) * bins;
    j.lo_x = lo; j.hi_x = hi;
    j.from_data = from_data != 0;
    return hs_run(j, (hipStream_t)stream);
}

extern "C" int vs_joint_histogram(const float* x, const float* y, int n, int c, int d, int h, int w, int bins_x, int bins_y, const double* range4,
                                  int from_data, double* edges_x, double* edges_y, long long* table, long long* outside, void* stream) {
    hs_job j = {};
    const int rc = hs_shape(n, c, d, h, w, &j);
    if (rc != VS_OK) return rc;
    if (!x || !y || !edges_x || !edges_y || !table || !outside || bins_x < 1 || bins_y < 1 || edges_x == edges_y) return VS_EINVAL;
    if (!from_data && (!range4 || !hs_bounds_ok(range4[0], range4[1]) || !hs_bounds_ok(range4[2], range4[3]))) return VS_EINVAL;
    if ((long long)bins_x * bins_y > HS_MAX_CELLS) return VS_ESHAPE;
    if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)edges_x & 7) || ((uintptr_t)edges_y & 7) || ((uintptr_t)table & 7) ||
        ((uintptr_t)outside & 7)) return VS_EALIGN;
    j.x = x; j.y = y;
    j.ex = edges_x; j.ey = edges_y;
    j.table = table; j.outside = outside;
    j.bx = bins_x; j.by = bins_y;
    j.ncells = bins_x * bins_y;
    if (!from_data) { j.lo_x = range4[0]; j.hi_x = range4[1]; j.lo_y = range4[2]; j.hi_y = range4[3]; }
    j.from_data = from_data != 0;
    return hs_run(j, (hipStream_t)stream);
}

extern "C" int vs_mutual_information(const long long* table, int n, int c, int bins_x, int bins_y, double sigma, int normalized, double* workspace,
                                     double* mi, void* stream) {
    if (n <= 0 || c <= 0) return VS_ESHAPE;
    if (!table || !workspace || !mi || bins_x < 1 || bins_y < 1 || !(sigma >= 0.0)) return VS_EINVAL;
    const long long cells = (long long)bins_x * bins_y, planes = (long long)n * c;
    if (cells > HS_MAX_CELLS || planes > 65535) return VS_ESHAPE;         // the plane is a grid's y
    if (((uintptr_t)table & 7) || ((uintptr_t)workspace & 7) || ((uintptr_t)mi & 7)) return VS_EALIGN;
    mi_weights g;
    g.radius = (int)(4.0 * sigma + 0.5);                                  // scipy.ndimage.gaussian_filter1d, truncate = 4
    if (g.radius > HS_MAX_RADIUS) return VS_EINVAL;
    if (sigma > 0.0) {                                                    // scipy's _gaussian_kernel1d: exp(-0.5 / sigma^2 * k^2), divided by the sum
        double sum = 0.0;
        for (int k = -g.radius; k <= g.radius; ++k) sum += exp(-0.5 / (sigma * sigma) * (double)k * (double)k);
        for (int k = 0; k <= g.radius; ++k) g.w[k] = exp(-0.5 / (sigma * sigma) * (double)k * (double)k) / sum;
    } else {
        g.w[0] = 1.0;
    }
    double* half = workspace;                                             // the table smoothed along x
    double* sm = half + planes * cells;                                   // smoothed along both, + eps
    double* rows = sm + planes * cells;
    double* cols = rows + planes * bins_x;
    double* ent = cols + planes * bins_y;
    const double eps = 2.220446049250313e-16;                             // np.finfo(float).eps
    const hipStream_t st = (hipStream_t)stream;
    const unsigned fgrid = hs_grid((planes * cells + 255) / 256);
    if (sigma > 0.0) {
        hipLaunchKernelGGL((mi_filter_kernel<0, long long>), dim3(fgrid), dim3(256), 0, st, table, half, planes, bins_x, bins_y, g, 0.0);
        VS_CHECK_LAUNCH();
        hipLaunchKernelGGL((mi_filter_kernel<1, double>), dim3(fgrid), dim3(256), 0, st, (const double*)half, sm, planes, bins_x, bins_y, g, eps);
    } else {
        hipLaunchKernelGGL((mi_filter_kernel<1, long long>), dim3(fgrid), dim3(256), 0, st, table, sm, planes, bins_x, bins_y, g, eps);
    }
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mi_marginals_kernel, dim3((unsigned)(bins_x + bins_y), (unsigned)planes), dim3(256), 0, st, (const double*)sm, rows, cols, bins_x,
                       bins_y);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mi_entropy_kernel, dim3((unsigned)bins_x, (unsigned)planes), dim3(256), 0, st, (const double*)sm, (const double*)rows, ent, bins_x,
                       bins_y);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mi_final_kernel, dim3((unsigned)planes), dim3(256), 0, st, (const double*)rows, (const double*)cols, (const double*)ent, mi, bins_x,
                       bins_y, normalized);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
