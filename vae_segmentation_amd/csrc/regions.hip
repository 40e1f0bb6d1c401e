// Per-component measurements of a label volume and the contingency table of two label volumes (include/vaeseg.h: vs_region_props, vs_contingency).
//
// Both read int32 labels (n, c, d, h, w) as vs_cc_label writes them — 0 background, 1..K components — and every (n, c) plane is its own problem.
// Components are spatially coherent: along x consecutive voxels mostly share a label (or a pair of labels), so the work is done per RUN, not per voxel.
//
//   runs      a wave loads 64 consecutive voxels, one key per lane (-1: not counted).  A lane is a run's head when its key differs from the lane
//             below it; one ballot of the heads gives every head its run's length as the distance to the next set bit.  Inside a row a run's
//             count, box and coordinate sums are closed forms of (first x, length, y, z): the segmented reduction needs no shuffle tree.
//   pending   a wave walks a chunk of consecutive segments of one plane and carries ONE record in wave-uniform registers: the lanes of the
//             segment that hold the pending key are folded into it from their ballot (popcount, first / last bit, bit-position sum per run),
//             and only the heads of the OTHER runs issue global atomics.  When a segment holds foreground but none of the pending key, the
//             record is flushed (one set of atomics) and the segment's first foreground key takes its place.  A blob that spans the chunk
//             costs one flush per chunk instead of one update per row.
//   LDS       a contingency table of at most RG_LDS_CELLS cells is accumulated per workgroup in LDS (32-bit counters: a workgroup sees
//             RG_LDS_VOXELS voxels) and flushed once, non-zero cells only.
//
// Every accumulator is an integer and every update is atomicAdd / atomicMin / atomicMax on it, issued by vector lanes: the result does not
// depend on the order of arrival — both builds of the library, eager launches and graph replay give the same bits.  The first launch of a call
// writes the table's initial state (no memset node), the second accumulates; nothing waits for another workgroup, nothing is read back.
#include <limits.h>
#include "volume.h"

namespace {

constexpr int RG_CHUNK = 32;                 // 64-voxel segments a wave walks with one pending record
constexpr int RG_LDS_CELLS = 4096;           // contingency tables up to this many cells take the LDS path (16 KB of 32-bit counters)
constexpr int RG_LDS_VOXELS = 16384;         // voxels per workgroup on the LDS path: 256 threads x 64 iterations
constexpr long long RG_MAX_CELLS = 1ll << 22;
constexpr int RG_COLS = 10;                  // count, zmin, ymin, xmin, zmax, ymax, xmax, sum_z, sum_y, sum_x

__device__ __forceinline__ void rg_min(i64* p, i64 v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rg_max(i64* p, i64 v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }



// a record of voxels (z, y, x0 + bit) for the set bits of m: wave-uniform
struct rg_record {
    i64 cnt, sz, sy, sx;
    int zmin, ymin, xmin, zmax, ymax, xmax;
    __device__ __forceinline__ void clear() {
        cnt = sz = sy = sx = 0;
        zmin = ymin = xmin = INT_MAX;
        zmax = ymax = xmax = -1;
    }
    __device__ __forceinline__ void fold(u64 m, int z, int y, int x0) {
        const int k = __popcll(m);
        cnt += k;
        sz += (i64)z * k;
        sy += (i64)y * k;
        zmin = min(zmin, z); zmax = max(zmax, z);
        ymin = min(ymin, y); ymax = max(ymax, y);
        xmin = min(xmin, x0 + run_ctz(m));
        xmax = max(xmax, x0 + 63 - __clzll((long long)m));
        i64 pos = 0;                                    // sum of the set bits' positions, run by run
        while (m) {
            const int s = run_ctz(m);
            const u64 t = m >> s;
            const int len = t == ~0ull ? 64 : run_ctz(~t);
            pos += (i64)len * s + (i64)len * (len - 1) / 2;
            m &= ~((len == 64 ? ~0ull : (1ull << len) - 1ull) << s);
        }
        sx += (i64)x0 * k + pos;
    }
    __device__ __forceinline__ void flush(i64* row) const {
        run_add(row + 0, cnt);
        rg_min(row + 1, zmin); rg_min(row + 2, ymin); rg_min(row + 3, xmin);
        rg_max(row + 4, zmax); rg_max(row + 5, ymax); rg_max(row + 6, xmax);
        run_add(row + 7, sz); run_add(row + 8, sy); run_add(row + 9, sx);
    }
};

struct rg_dims {
    int d, h, w, segs;                 // segs: 64-wide segments per row
    int V;                             // voxels per plane
    long long planes, chunks;          // n * c; chunks per plane
};

__global__ __launch_bounds__(256) void rg_props_init_kernel(i64* __restrict__ table, int* __restrict__ overflow, rg_dims g, int max_rows) {
    const long long cells = g.planes * max_rows * RG_COLS;
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long i = i0; i < cells; i += stride) {
        const int col = (int)(i % RG_COLS);
        i64 v = 0;
        if (col == 1) v = g.d;
        else if (col == 2) v = g.h;
        else if (col == 3) v = g.w;
        else if (col >= 4 && col <= 6) v = -1;
        table[i] = v;
    }
    for (long long i = i0; i < g.planes; i += stride) overflow[i] = 0;
}

// a wave per chunk of RG_CHUNK row segments of one plane
__global__ __launch_bounds__(256) void rg_props_kernel(const int* __restrict__ labels, i64* __restrict__ table, int* __restrict__ overflow, rg_dims g,
                                                       int max_rows) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const long long segs_per_plane = (long long)g.d * g.h * g.segs;
    for (long long job = wave0; job < g.planes * g.chunks; job += nwaves) {
        const long long plane = job / g.chunks;
        const long long s0 = (job - plane * g.chunks) * RG_CHUNK;
        const long long s1 = s0 + RG_CHUNK < segs_per_plane ? s0 + RG_CHUNK : segs_per_plane;
        const int* L = labels + (size_t)plane * g.V;
        i64* T = table + (size_t)plane * max_rows * RG_COLS;
        rg_record pend;
        int pend_key = 0, bad = 0;
        pend.clear();
        for (long long s = s0; s < s1; ++s) {
            const long long row = s / g.segs;
            const int x0 = (int)(s - row * g.segs) * 64;
            const int z = (int)(row / g.h), y = (int)(row - (long long)z * g.h);
            const int x = x0 + lane;
            const bool live = x < g.w;
            const int lab = live ? L[(size_t)row * g.w + x] : 0;
            const bool out = live && (lab < 0 || lab > max_rows);
            bad += __popcll(__ballot(out));
            const int key = live && !out ? lab : -1;                      // 0: background, counted nowhere
            const u64 fg = __ballot(key > 0);
            if (!fg) continue;
            u64 m = pend_key ? __ballot(key == pend_key) : 0ull;
            if (!m) {
                if (pend_key && lane == 0) pend.flush(T + (size_t)(pend_key - 1) * RG_COLS);
                pend_key = __shfl(key, run_ctz(fg));
                pend.clear();
                m = __ballot(key == pend_key);
            }
            pend.fold(m, z, y, x0);
            const int below = __shfl_up(key, 1);
            const u64 heads = __ballot(lane == 0 || key != below);
            if (key > 0 && key != pend_key && (lane == 0 || key != below)) {
                const int len = run_length(heads, lane);
                i64* r = T + (size_t)(key - 1) * RG_COLS;
                run_add(r + 0, len);
                rg_min(r + 1, z); rg_min(r + 2, y); rg_min(r + 3, x);
                rg_max(r + 4, z); rg_max(r + 5, y); rg_max(r + 6, x + len - 1);
                run_add(r + 7, (i64)z * len); run_add(r + 8, (i64)y * len); run_add(r + 9, (i64)x * len + (i64)len * (len - 1) / 2);
            }
        }
        if (lane == 0) {
            if (pend_key) pend.flush(T + (size_t)(pend_key - 1) * RG_COLS);
            if (bad) atomicAdd(overflow + plane, bad);
        }
    }
}

__global__ __launch_bounds__(256) void rg_zero_kernel(i64* __restrict__ table, long long cells, int* __restrict__ overflow, long long planes) {
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long i = i0; i < cells; i += stride) table[i] = 0;
    for (long long i = i0; i < planes; i += stride) overflow[i] = 0;
}

// the cell of a voxel's label pair, or -1 when either label is out of range
__device__ __forceinline__ int rg_cell(int a, int b, int rows_a, int rows_b) {
    return a < 0 || a > rows_a || b < 0 || b > rows_b ? -1 : a * (rows_b + 1) + b;
}

// a workgroup per RG_LDS_VOXELS voxels of one plane; the plane is one flat string of voxels (no coordinates are needed)
__global__ __launch_bounds__(256) void rg_contingency_lds_kernel(const int* __restrict__ a, const int* __restrict__ b, i64* __restrict__ table,
                                                                 int* __restrict__ overflow, int V, int blocks_per_plane, int rows_a, int rows_b) {
    __shared__ unsigned int cells[RG_LDS_CELLS];
    __shared__ int bad_total;
    const int lane = threadIdx.x & 63;
    const int ncells = (rows_a + 1) * (rows_b + 1);
    const long long plane = blockIdx.x / blocks_per_plane;
    const int v0 = (int)(blockIdx.x - plane * blocks_per_plane) * RG_LDS_VOXELS;
    for (int i = threadIdx.x; i < ncells; i += 256) cells[i] = 0u;
    if (threadIdx.x == 0) bad_total = 0;
    __syncthreads();
    const int* A = a + (size_t)plane * V;
    const int* B = b + (size_t)plane * V;
    int bad = 0;
    for (int it = 0; it < RG_LDS_VOXELS / 256; ++it) {
        const long long v = (long long)v0 + it * 256 + threadIdx.x;      // the same trip count for every lane: the ballots need all of them
        const bool live = v < V;
        const int key = live ? rg_cell(A[v], B[v], rows_a, rows_b) : -1;
        bad += __popcll(__ballot(live && key < 0));
        const int below = __shfl_up(key, 1);
        const bool head = lane == 0 || key != below;
        const u64 heads = __ballot(head);
        if (head && key >= 0) atomicAdd(&cells[key], (unsigned int)run_length(heads, lane));
    }
    if (lane == 0 && bad) atomicAdd(&bad_total, bad);
    __syncthreads();
    i64* T = table + (size_t)plane * ncells;
    for (int i = threadIdx.x; i < ncells; i += 256)
        if (cells[i]) run_add(T + i, (i64)cells[i]);
    if (threadIdx.x == 0 && bad_total) atomicAdd(overflow + plane, bad_total);
}

// a wave per chunk of RG_CHUNK 64-voxel segments of one plane, a pending (cell, count) in wave-uniform registers
__global__ __launch_bounds__(256) void rg_contingency_kernel(const int* __restrict__ a, const int* __restrict__ b, i64* __restrict__ table,
                                                             int* __restrict__ overflow, int V, long long planes, long long chunks, int rows_a, int rows_b) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const long long ncells = (long long)(rows_a + 1) * (rows_b + 1);
    for (long long job = wave0; job < planes * chunks; job += nwaves) {
        const long long plane = job / chunks;
        const long long v0 = (job - plane * chunks) * (RG_CHUNK * 64);
        const int* A = a + (size_t)plane * V;
        const int* B = b + (size_t)plane * V;
        i64* T = table + (size_t)plane * ncells;
        int pend_key = -1, bad = 0;
        i64 pend_cnt = 0;
        for (int it = 0; it < RG_CHUNK; ++it) {
            const long long v = v0 + it * 64 + lane;
            if (v0 + it * 64 >= V) break;                                 // wave-uniform
            const bool live = v < V;
            const int key = live ? rg_cell(A[v], B[v], rows_a, rows_b) : -1;
            bad += __popcll(__ballot(live && key < 0));
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
            if (bad) atomicAdd(overflow + plane, bad);
        }
    }
}

unsigned rg_grid(long long blocks) {
    const long long cap = 1 << 20;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// VS_OK and the plane geometry, or the status of a rejected shape
int rg_shape(int n, int c, int d, int h, int w, rg_dims* g) {
    if (n <= 0 || c <= 0 || d <= 0 || h <= 0 || w <= 0) return VS_ESHAPE;
    const long long V = (long long)d * h * w;
    if (V > INT_MAX) return VS_ESHAPE;                                    // plane-local indices and the overflow counts are int32
    g->d = d; g->h = h; g->w = w;
    g->segs = (w + 63) / 64;
    g->V = (int)V;
    g->planes = (long long)n * c;
    if (g->planes > INT_MAX) return VS_ESHAPE;
    return VS_OK;
}

}  // namespace

extern "C" int vs_region_props(const int* labels, int n, int c, int d, int h, int w, int max_rows, long long* table, int* overflow, void* stream) {
    rg_dims g;
    const int rc = rg_shape(n, c, d, h, w, &g);
    if (rc != VS_OK) return rc;
    if (!labels || !table || !overflow || max_rows < 1) return VS_EINVAL;
    if (((uintptr_t)labels & 3) || ((uintptr_t)table & 7) || ((uintptr_t)overflow & 3)) return VS_EALIGN;
    const long long segs_per_plane = (long long)d * h * g.segs;
    g.chunks = (segs_per_plane + RG_CHUNK - 1) / RG_CHUNK;
    const hipStream_t st = (hipStream_t)stream;
    const long long cells = g.planes * max_rows * RG_COLS;
    hipLaunchKernelGGL(rg_props_init_kernel, dim3(rg_grid((cells + 255) / 256)), dim3(256), 0, st, table, overflow, g, max_rows);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(rg_props_kernel, dim3(rg_grid((g.planes * g.chunks + 3) / 4)), dim3(256), 0, st, labels, table, overflow, g, max_rows);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_contingency(const int* a, const int* b, int n, int c, int d, int h, int w, int rows_a, int rows_b, long long* table, int* overflow,
                              void* stream) {
    rg_dims g;
    const int rc = rg_shape(n, c, d, h, w, &g);
    if (rc != VS_OK) return rc;
    if (!a || !b || !table || !overflow || rows_a < 0 || rows_b < 0) return VS_EINVAL;
    const long long ncells = ((long long)rows_a + 1) * ((long long)rows_b + 1);
    if (ncells > RG_MAX_CELLS) return VS_ESHAPE;
    if (((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)table & 7) || ((uintptr_t)overflow & 3)) return VS_EALIGN;
    const long long bpp = ((long long)g.V + RG_LDS_VOXELS - 1) / RG_LDS_VOXELS;
    if (ncells <= RG_LDS_CELLS && g.planes * bpp > INT_MAX) return VS_ESHAPE;      // the LDS path: one workgroup per piece of a plane
    const hipStream_t st = (hipStream_t)stream;
    const long long cells = g.planes * ncells;
    hipLaunchKernelGGL(rg_zero_kernel, dim3(rg_grid((cells + 255) / 256)), dim3(256), 0, st, table, cells, overflow, g.planes);
    VS_CHECK_LAUNCH();
    if (ncells <= RG_LDS_CELLS) {
        hipLaunchKernelGGL(rg_contingency_lds_kernel, dim3((unsigned)(g.planes * bpp)), dim3(256), 0, st, a, b, table, overflow, g.V, (int)bpp, rows_a,
                           rows_b);
    } else {
        const long long chunks = ((long long)g.V + RG_CHUNK * 64 - 1) / (RG_CHUNK * 64);
        hipLaunchKernelGGL(rg_contingency_kernel, dim3(rg_grid((g.planes * chunks + 3) / 4)), dim3(256), 0, st, a, b, table, overflow, g.V, g.planes,
                           chunks, rows_a, rows_b);
    }
    VS_CHECK_LAUNCH();
    return VS_OK;
}
