// The label-equivalence core of the connected-component code, shared by cc.hip (labelling, keep-largest) and morph.hip (hole filling labels the
// complement of a mask): the union-find primitives over an int32 `parent` array of plane-local indices and the merge launch.  cc.hip's header
// comment describes the scheme.  Included inside each translation unit: everything here has internal linkage.
#pragma once
#include "common.h"

namespace {

constexpr int CC_SEG = 64;          // x extent a wave owns in init / merge

struct cc_dims {
    int n, c, d, h, w, lo;          // planes with channel < lo are not labelled
    int V, maxk, nb;                // voxels per plane, rows of the size table per plane, chunks per plane
    long long planes, total;        // n * c, n * c * V
};

__device__ __forceinline__ int cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of a: parent values only decrease along the walk
__device__ __forceinline__ int cc_find(const int* L, int a) {
    int p = cc_ld(L + a);
    while (p != a) {
        a = p;
        p = cc_ld(L + a);
    }
    return a;
}

// find with the start pointed at what was found (an ancestor: the displaced link's target stays reachable through its own links)
__device__ __forceinline__ int cc_find_compress(int* L, int a) {
    const int a0 = a;
    int p = cc_ld(L + a), hops = 0;
    while (p != a) {
        a = p;
        p = cc_ld(L + a);
        ++hops;
    }
    if (hops > 1) atomicMin(L + a0, a);
    return a;
}

__device__ __forceinline__ void cc_union(int* L, int a, int b) {
    for (;;) {
        a = cc_find_compress(L, a);
        b = cc_find_compress(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);      // agent scope
        if (old == a) return;                     // a was a root and now hangs under b
        a = old;                                  // a had been linked meanwhile (old < a): what it pointed to is united with b next
    }
}

// wave w -> (row, segment); rows are (plane, z, y)
struct cc_seg {
    long long row;
    int plane_c, z, y, x0;
    long long plane;
};
__device__ __forceinline__ cc_seg cc_seg_of(long long s, int segs, const cc_dims& g) {
    cc_seg r;
    r.row = s / segs;
    r.x0 = (int)(s - r.row * segs) * CC_SEG;
    const long long pz = r.row / g.h;
    r.y = (int)(r.row - pz * g.h);
    r.plane = pz / g.d;
    r.z = (int)(pz - r.plane * g.d);
    r.plane_c = (int)(r.plane % g.c);
    return r;
}

// foreground bits of one 64-wide segment of a row plus the voxel on either side of it (0 outside the row / volume: no wrap, borders are background)
struct cc_rowbits {
    unsigned long long m;
    bool left, right;
    __device__ __forceinline__ bool at(int lane) const { return (m >> lane) & 1ull; }
    __device__ __forceinline__ bool before(int lane) const { return lane ? (m >> (lane - 1)) & 1ull : left; }
    __device__ __forceinline__ bool after(int lane) const { return lane < 63 ? (m >> (lane + 1)) & 1ull : right; }
};
__device__ __forceinline__ cc_rowbits cc_load_row(const int* rowp, bool row_ok, int x0, int w, int lane) {
    const int x = x0 + lane;
    const bool fg = row_ok && x < w && rowp[x] >= 0;
    int xe = -1;
    if (lane == 0) xe = x0 - 1;
    if (lane == 1) xe = x0 + CC_SEG;
    const bool edge = row_ok && xe >= 0 && xe < w && rowp[xe] >= 0;
    cc_rowbits r;
    r.m = __ballot(fg);
    const unsigned long long e = __ballot(edge);
    r.left = e & 1ull;
    r.right = (e >> 1) & 1ull;
    return r;
}

template <int CONN>
__global__ __launch_bounds__(256) void cc_merge_kernel(int* __restrict__ parent, cc_dims g, long long nsegs, int segs) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long s = wave0; s < nsegs; s += nwaves) {
        const cc_seg q = cc_seg_of(s, segs, g);
        if (q.plane_c < g.lo) continue;
        int* L = parent + (size_t)q.plane * g.V;
        const int rowbase = (q.z * g.h + q.y) * g.w;
        const cc_rowbits own = cc_load_row(L + rowbase, true, q.x0, g.w, lane);
        if (!own.m) continue;
        const bool fg = own.at(lane);
        const int v = rowbase + q.x0 + lane;
        if (fg && lane == 0 && own.left) cc_union(L, v, v - 1);               // an x-run that crosses the segment boundary
        const bool pl = own.before(lane), pr = own.after(lane);
        constexpr int NROWS = CONN == 26 ? 4 : 2;
        const int dzs[4] = {0, -1, -1, -1}, dys[4] = {-1, 0, -1, 1};
        cc_rowbits ups[NROWS];
        int nbases[NROWS];
#pragma unroll
        for (int r = 0; r < NROWS; ++r) {         // every lane takes part in the ballots
            const int z = q.z + dzs[r], y = q.y + dys[r];
            const bool ok = z >= 0 && y >= 0 && y < g.h;
            nbases[r] = (z * g.h + y) * g.w;
            ups[r] = cc_load_row(L + (ok ? nbases[r] : 0), ok, q.x0, g.w, lane);
        }
        if (!fg) continue;
#pragma unroll
        for (int r = 0; r < NROWS; ++r) {
            const cc_rowbits up = ups[r];
            const int u = nbases[r] + q.x0 + lane;
            const bool a = up.before(lane), c = up.at(lane), e = up.after(lane);
            // The runs of both rows are already one set each, so one union per pair of touching runs is enough: the pair (v, u) is left to
            // (v - 1, u - 1) when both of those are foreground, and so on down to the first column where the two runs overlap.
            if (c) {
                if (!(pl && a)) cc_union(L, v, u);
            } else if (CONN == 26) {
                if (a && !pl) cc_union(L, v, u - 1);      // diagonal contacts; with pl set, v - 1 sits right under u - 1 and unites
                if (e && !pr) cc_union(L, v, u + 1);      // likewise v + 1 under u + 1
            }
        }
    }
}

unsigned cc_grid(long long items_per_block_units) {
    const long long cap = 1 << 20;
    return (unsigned)(items_per_block_units < 1 ? 1 : (items_per_block_units > cap ? cap : items_per_block_units));
}

}  // namespace
