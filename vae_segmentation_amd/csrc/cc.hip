// Connected-component labelling of planar fp32 masks and the keep-largest filter (include/vaeseg.h: vs_cc_*).
//
// The reference numbers components with a numpy flood fill (utils/utils.py:20-57, Tag / check_connection) and filters predictions with
// SimpleITK's ConnectedComponent + RelabelComponent (utils/utils.py:776-796, predict_vol step 2).  Here every (n, c) plane is an independent
// union-find over its voxels, kept in an int32 `parent` array of plane-local linear indices (z slowest, x fastest):
//
//   init     parent[v] = first voxel of v's x-run inside its 64-wide row segment (one wave ballot + a bit scan, no atomics); background -1
//   merge    every foreground voxel is united with the runs it touches in the rows above / behind it (and across the segment boundary of
//            its own row): find + atomicMin.  A link only ever moves to a SMALLER index, a displaced link is re-united by the thread that
//            displaced it, so the result is the same for every arrival order and the root of a component is its minimal index — its first
//            voxel in raster order.  Reads of `parent` may be stale (another XCD's L2): any value ever stored is a valid ancestor, the
//            atomics decide; a `find` walks strictly decreasing indices, so every loop ends.
//   flatten  parent[v] = root(v)
//   count / scan / rank   roots per 4096-voxel chunk, exclusive scan of the chunk counts per plane (one workgroup), label(root) = rank + 1
//   relabel  label(v) = label(root(v)); sizes[label - 1] += 1 (integer atomics, one per distinct label per wave)
//   select   per plane: which labels are among the k largest with at least min_size voxels (ties: lower label)
//   apply    the filtered mask
//
// Phase boundaries are launch boundaries: no kernel waits for another workgroup.  The same code serves both builds of the library.
#include <limits.h>
#include "cc_core.h"

namespace {

constexpr int CC_CHUNK = 4096;      // voxels per workgroup in count / rank: 256 threads x 4 iterations x 4 voxels
constexpr int CC_SEL_NT = 1024;     // threads of the per-plane workgroups (scan, select)

__global__ __launch_bounds__(256) void cc_init_kernel(const float* __restrict__ mask, int* __restrict__ parent, int* __restrict__ sizes, cc_dims g,
                                                      long long nsegs, int segs) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long i = wave0 * 64 + lane; i < g.planes * g.maxk; i += nwaves * 64) sizes[i] = 0;
    for (long long s = wave0; s < nsegs; s += nwaves) {
        const cc_seg q = cc_seg_of(s, segs, g);
        if (q.plane_c < g.lo) continue;
        const int x = q.x0 + lane;
        const size_t at = (size_t)q.row * g.w + x;
        const bool fg = x < g.w && mask[at] >= 0.5f;                       // binarize, utils/evaluation.py:9-10
        const unsigned long long b = __ballot(fg);
        const unsigned long long below = ~b & ((1ull << lane) - 1ull);     // background lanes below this one
        const int start = below ? 64 - __clzll(below) : 0;
        if (x < g.w) parent[at] = fg ? (q.z * g.h + q.y) * g.w + q.x0 + start : -1;
    }
}

// (plane, plane-local index) of a flat element index, advanced element by element
struct cc_cursor {
    long long p;
    int l;
    __device__ __forceinline__ cc_cursor(long long i, int V) : p(i / V), l((int)(i - (i / V) * V)) {}
    __device__ __forceinline__ void next(int V) {
        if (++l == V) { l = 0; ++p; }
    }
};

__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, cc_dims g) {
    const long long quads = (g.total + 3) / 4;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
        const long long i = q * 4;
        const bool full = i + 4 <= g.total;
        int par[4] = {-1, -1, -1, -1};
        if (full) {
            const int4 t = *reinterpret_cast<const int4*>(parent + i);
            par[0] = t.x; par[1] = t.y; par[2] = t.z; par[3] = t.w;
        } else {
            for (int j = 0; i + j < g.total; ++j) par[j] = parent[i + j];
        }
        cc_cursor cur(i, g.V);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < g.total && (int)(cur.p % g.c) >= g.lo) {
                if (par[j] >= 0 && par[j] != cur.l) par[j] = cc_find(parent + (size_t)cur.p * g.V, par[j]);
            } else {
                par[j] = -1;
            }
            cur.next(g.V);
        }
        if (full) {
            *reinterpret_cast<int4*>(parent + i) = make_int4(par[0], par[1], par[2], par[3]);
        } else {
            for (int j = 0; i + j < g.total; ++j) parent[i + j] = par[j];
        }
    }
}

// flags[j] = voxel e + j of the plane is a root
template <bool VEC>
__device__ __forceinline__ int cc_root_flags(const int* L, int e, int V, bool flags[4]) {
    int par[4] = {-1, -1, -1, -1};
    if (e < V) {
        if (VEC) {
            const int4 t = *reinterpret_cast<const int4*>(L + e);
            par[0] = t.x; par[1] = t.y; par[2] = t.z; par[3] = t.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e + j < V) par[j] = L[e + j];
        }
    }
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        flags[j] = par[j] == e + j;
        cnt += flags[j];
    }
    return cnt;
}

// RANK = false: chunks[plane][chunk] = roots in the chunk.  RANK = true: chunks hold the exclusive scan; labels[root] = rank + 1.
template <bool VEC, bool RANK>
__global__ __launch_bounds__(256) void cc_chunk_kernel(const int* __restrict__ parent, int* __restrict__ chunks, int* __restrict__ labels, cc_dims g) {
    __shared__ int lds[4];
    const long long p = blockIdx.x / g.nb;
    const int b = (int)(blockIdx.x - p * g.nb);
    if ((int)(p % g.c) < g.lo) return;
    const int* L = parent + (size_t)p * g.V;
    int carry = RANK ? chunks[blockIdx.x] : 0;
    for (int it = 0; it < CC_CHUNK / 1024; ++it) {
        const long long e64 = (long long)b * CC_CHUNK + it * 1024 + threadIdx.x * 4;
        const int e = e64 < g.V ? (int)e64 : g.V;
        bool flags[4];
        const int cnt = cc_root_flags<VEC>(L, e, g.V, flags);
        int tot;
        int r = carry + block_excl_scan<256>(cnt, &tot, lds);
        if (RANK) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (flags[j]) labels[(size_t)p * g.V + e + j] = ++r;
        }
        carry += tot;
    }
    if (!RANK && threadIdx.x == 0) chunks[blockIdx.x] = carry;
}

__global__ __launch_bounds__(CC_SEL_NT) void cc_scan_kernel(int* __restrict__ chunks, int* __restrict__ counts, cc_dims g) {
    __shared__ int lds[CC_SEL_NT / 64];
    const long long p = blockIdx.x;
    if ((int)(p % g.c) < g.lo) {
        if (threadIdx.x == 0) counts[p] = 0;
        return;
    }
    int* c = chunks + (size_t)p * g.nb;
    int carry = 0;
    for (int base = 0; base < g.nb; base += CC_SEL_NT) {
        const int i = base + threadIdx.x;
        const int val = i < g.nb ? c[i] : 0;
        int tot;
        const int ex = block_excl_scan<CC_SEL_NT>(val, &tot, lds);
        if (i < g.nb) c[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) counts[p] = carry;
}

__global__ __launch_bounds__(256) void cc_relabel_kernel(const int* __restrict__ parent, int* __restrict__ labels, int* __restrict__ sizes, cc_dims g) {
    const int lane = threadIdx.x & 63;
    const long long quads = (g.total + 3) / 4;
    const long long q0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    // the trip count is the same for every lane of a wave (the shuffles below need all of them)
    for (long long qw = q0 - lane; qw < quads; qw += stride) {
        const long long q = qw + lane;
        const long long i = q * 4;
        const bool live = q < quads, full = live && i + 4 <= g.total;
        int par[4] = {-1, -1, -1, -1};
        if (full) {
            const int4 t = *reinterpret_cast<const int4*>(parent + i);
            par[0] = t.x; par[1] = t.y; par[2] = t.z; par[3] = t.w;
        } else if (live) {
            for (int j = 0; i + j < g.total; ++j) par[j] = parent[i + j];
        }
        int lab[4], cnt[4];
        long long slot[4];          // row of the size table: plane * maxk + label - 1
        cc_cursor cur(live ? i : 0, g.V);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = live && i + j < g.total && (int)(cur.p % g.c) >= g.lo && par[j] >= 0;
            lab[j] = on ? labels[(size_t)cur.p * g.V + par[j]] : 0;      // a root's label was written by the rank launch
            slot[j] = on ? cur.p * g.maxk + lab[j] - 1 : -1;
            cnt[j] = on ? 1 : 0;
            cur.next(g.V);
        }
        if (full) {
            *reinterpret_cast<int4*>(labels + i) = make_int4(lab[0], lab[1], lab[2], lab[3]);
        } else if (live) {
            for (int j = 0; i + j < g.total; ++j) labels[i + j] = lab[j];
        }
        // sizes: equal neighbours fold inside the thread, then one atomic per distinct slot per wave
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (cnt[j] && slot[j] == slot[j - 1]) { cnt[j] += cnt[j - 1]; cnt[j - 1] = 0; }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned long long active = __ballot(cnt[j] > 0);
            while (active) {
                const int leader = __ffsll((long long)active) - 1;
                const long long sl = __shfl(slot[j], leader);
                const bool same = cnt[j] > 0 && slot[j] == sl;
                int sum = same ? cnt[j] : 0;
#pragma unroll
                for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
                if (lane == leader) atomicAdd(sizes + sl, sum);
                active &= ~__ballot(same);
            }
        }
    }
}

__device__ __forceinline__ int cc_block_sum(int v, int* lds) {
    int tot;
    block_excl_scan<CC_SEL_NT>(v, &tot, lds);
    return tot;
}

// keep[label - 1] = 1 for the k largest components of the plane that hold at least min_size voxels; equal sizes: the lower label first
__global__ __launch_bounds__(CC_SEL_NT) void cc_select_kernel(const int* __restrict__ sizes, const int* __restrict__ counts, int* __restrict__ keep, cc_dims g,
                                                              int k, int min_size) {
    __shared__ int lds[CC_SEL_NT / 64];
    const long long p = blockIdx.x;
    if ((int)(p % g.c) < g.lo) return;
    const int K = counts[p];
    const int* sz = sizes + (size_t)p * g.maxk;
    int* kp = keep + (size_t)p * g.maxk;
    const int m = min_size > 1 ? min_size : 1;
    auto count_ge = [&](int t) {
        int c = 0;
        for (int i = threadIdx.x; i < K; i += CC_SEL_NT) c += sz[i] >= t;
        return cc_block_sum(c, lds);
    };
    const int eligible = count_ge(m);
    if (k >= eligible || k == 0) {
        for (int i = threadIdx.x; i < K; i += CC_SEL_NT) kp[i] = k != 0 && sz[i] >= m;
        return;
    }
    int lo = m, hi = g.V;                          // the largest t with at least k components of size >= t
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (count_ge(mid) >= k) lo = mid; else hi = mid - 1;
    }
    const int t = lo;
    const int room = k - (t < g.V ? count_ge(t + 1) : 0);          // how many components of size exactly t are kept: the first ones
    int carry = 0;
    for (int base = 0; base < K; base += CC_SEL_NT) {
        const int i = base + threadIdx.x;
        const int s = i < K ? sz[i] : 0;
        int tot;
        const int ex = block_excl_scan<CC_SEL_NT>(s == t, &tot, lds);
        if (i < K) kp[i] = s > t || (s == t && carry + ex < room);
        carry += tot;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void cc_apply_kernel(const float* __restrict__ mask, float* __restrict__ out, const int* __restrict__ labels,
                                                       const int* __restrict__ keep, cc_dims g, int to_background) {
    const long long qpp = ((long long)g.V + 3) / 4, quads = qpp * g.n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
        const long long n = q / qpp;
        const int e = (int)(q - n * qpp) * 4;
        float removed[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = g.lo; c < g.c; ++c) {
            const long long p = n * g.c + c;
            const size_t at = (size_t)p * g.V + e;
            int lab[4] = {0, 0, 0, 0};
            if (VEC) {
                const int4 t = *reinterpret_cast<const int4*>(labels + at);
                lab[0] = t.x; lab[1] = t.y; lab[2] = t.z; lab[3] = t.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e + j < g.V) lab[j] = labels[at + j];
            }
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool kept = lab[j] > 0 && keep[(size_t)p * g.maxk + lab[j] - 1] != 0;
                o[j] = kept ? 1.f : 0.f;
                removed[j] += lab[j] > 0 && !kept ? 1.f : 0.f;
            }
            if (VEC) {
                *reinterpret_cast<float4*>(out + at) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e + j < g.V) out[at + j] = o[j];
            }
        }
        for (int c = 0; c < g.lo; ++c) {                 // copied through; channel 0 takes the removed voxels (a one-hot tensor stays one-hot)
            const size_t at = ((size_t)n * g.c + c) * g.V + e;
            const bool add = c == 0 && to_background;
            if (VEC) {
                float4 t = *reinterpret_cast<const float4*>(mask + at);
                if (add) { t.x += removed[0]; t.y += removed[1]; t.z += removed[2]; t.w += removed[3]; }
                *reinterpret_cast<float4*>(out + at) = t;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e + j < g.V) out[at + j] = mask[at + j] + (add ? removed[j] : 0.f);
            }
        }
    }
}

size_t cc_align(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: sizes int[planes][maxk] (FIRST: callers read it) | keep int[planes][maxk] | counts int[planes] | chunks int[planes][nb] | parent int[total] | labels int[total]
struct cc_layout {
    size_t sizes, keep, counts, chunks, parent, labels, bytes;
};
cc_layout cc_layout_of(const cc_dims& g) {
    cc_layout l;
    size_t o = 0;
    l.sizes = o;  o += cc_align((size_t)g.planes * g.maxk * 4);
    l.keep = o;   o += cc_align((size_t)g.planes * g.maxk * 4);
    l.counts = o; o += cc_align((size_t)g.planes * 4);
    l.chunks = o; o += cc_align((size_t)g.planes * g.nb * 4);
    l.parent = o; o += cc_align((size_t)g.total * 4);
    l.labels = o; o += cc_align((size_t)g.total * 4);
    l.bytes = o;
    return l;
}

// VS_OK and *g filled, or the status of a rejected call
int cc_check(int n, int c, int d, int h, int w, int connectivity, int lo, cc_dims* g) {
    if (connectivity != 6 && connectivity != 26) return VS_EINVAL;
    if (n <= 0 || c <= 0 || d <= 0 || h <= 0 || w <= 0) return VS_ESHAPE;
    if (lo < 0 || lo >= c) return VS_EINVAL;
    const long long V = (long long)d * h * w;
    if (V > INT_MAX) return VS_ESHAPE;                                   // plane-local indices are int32
    g->n = n; g->c = c; g->d = d; g->h = h; g->w = w; g->lo = lo;
    g->V = (int)V;
    // two components never share a 2x2x2 cell under 26-connectivity, nor a pair of x-neighbours under 6-connectivity
    const long long maxk = connectivity == 26 ? (long long)((d + 1) / 2) * ((h + 1) / 2) * ((w + 1) / 2) : (V + 1) / 2;
    g->maxk = (int)maxk;
    g->nb = (int)((V + CC_CHUNK - 1) / CC_CHUNK);
    g->planes = (long long)n * c;
    g->total = g->planes * V;
    if (g->planes * g->nb > INT_MAX || g->planes > INT_MAX) return VS_ESHAPE;      // one workgroup per chunk / per plane
    return VS_OK;
}

int cc_label_launch(const float* mask, int* labels, int* counts, char* ws, const cc_dims& g, int connectivity, hipStream_t st) {
    const cc_layout l = cc_layout_of(g);
    int* sizes = (int*)(ws + l.sizes);
    int* chunks = (int*)(ws + l.chunks);
    int* parent = (int*)(ws + l.parent);
    const int segs = (g.w + CC_SEG - 1) / CC_SEG;
    const long long nsegs = g.planes * g.d * g.h * segs;
    const unsigned seg_grid = cc_grid((nsegs + 3) / 4), quad_grid = cc_grid(((g.total + 3) / 4 + 255) / 256);
    hipLaunchKernelGGL(cc_init_kernel, dim3(seg_grid), dim3(256), 0, st, mask, parent, sizes, g, nsegs, segs);
    VS_CHECK_LAUNCH();
    if (connectivity == 26) hipLaunchKernelGGL(cc_merge_kernel<26>, dim3(seg_grid), dim3(256), 0, st, parent, g, nsegs, segs);
    else hipLaunchKernelGGL(cc_merge_kernel<6>, dim3(seg_grid), dim3(256), 0, st, parent, g, nsegs, segs);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(quad_grid), dim3(256), 0, st, parent, g);
    VS_CHECK_LAUNCH();
    const dim3 chunk_grid((unsigned)(g.planes * g.nb));
    const bool vec = g.V % 4 == 0;
    if (vec) hipLaunchKernelGGL((cc_chunk_kernel<true, false>), chunk_grid, dim3(256), 0, st, parent, chunks, labels, g);
    else hipLaunchKernelGGL((cc_chunk_kernel<false, false>), chunk_grid, dim3(256), 0, st, parent, chunks, labels, g);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(cc_scan_kernel, dim3((unsigned)g.planes), dim3(CC_SEL_NT), 0, st, chunks, counts, g);
    VS_CHECK_LAUNCH();
    if (vec) hipLaunchKernelGGL((cc_chunk_kernel<true, true>), chunk_grid, dim3(256), 0, st, parent, chunks, labels, g);
    else hipLaunchKernelGGL((cc_chunk_kernel<false, true>), chunk_grid, dim3(256), 0, st, parent, chunks, labels, g);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(quad_grid), dim3(256), 0, st, parent, labels, sizes, g);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

bool cc_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" long long vs_cc_workspace_bytes(int n, int c, int d, int h, int w, int connectivity) {
    cc_dims g;
    const int rc = cc_check(n, c, d, h, w, connectivity, 0, &g);
    if (rc != VS_OK) return rc;
    return (long long)cc_layout_of(g).bytes;
}

extern "C" int vs_cc_label(const float* mask, int* labels, int* counts, int n, int c, int d, int h, int w, int connectivity, void* workspace,
                           void* stream) {
    cc_dims g;
    const int rc = cc_check(n, c, d, h, w, connectivity, 0, &g);
    if (rc != VS_OK) return rc;
    if (!mask || !labels || !counts || !workspace) return VS_EINVAL;
    if (cc_misaligned(mask) || cc_misaligned(labels) || cc_misaligned(workspace)) return VS_EALIGN;
    return cc_label_launch(mask, labels, counts, (char*)workspace, g, connectivity, (hipStream_t)stream);
}

extern "C" int vs_cc_keep_largest(const float* mask, float* out, int n, int c, int d, int h, int w, int connectivity, int k, int min_size,
                                  int lo_channel, int to_background, void* workspace, void* stream) {
    cc_dims g;
    if (k < 0) return VS_EINVAL;
    const int rc = cc_check(n, c, d, h, w, connectivity, lo_channel, &g);
    if (rc != VS_OK) return rc;
    if (!mask || !out || !workspace || mask == out) return VS_EINVAL;
    if (cc_misaligned(mask) || cc_misaligned(out) || cc_misaligned(workspace)) return VS_EALIGN;
    char* ws = (char*)workspace;
    const cc_layout l = cc_layout_of(g);
    int* labels = (int*)(ws + l.labels);
    int* counts = (int*)(ws + l.counts);
    int* keep = (int*)(ws + l.keep);
    const hipStream_t st = (hipStream_t)stream;
    const int lrc = cc_label_launch(mask, labels, counts, ws, g, connectivity, st);
    if (lrc != VS_OK) return lrc;
    hipLaunchKernelGGL(cc_select_kernel, dim3((unsigned)g.planes), dim3(CC_SEL_NT), 0, st, (const int*)(ws + l.sizes), counts, keep, g, k, min_size);
    VS_CHECK_LAUNCH();
    const unsigned grid = cc_grid((((long long)g.V + 3) / 4 * g.n + 255) / 256);
    const bool to_bg = to_background && lo_channel >= 1;
    if (g.V % 4 == 0) hipLaunchKernelGGL(cc_apply_kernel<true>, dim3(grid), dim3(256), 0, st, mask, out, labels, keep, g, (int)to_bg);
    else hipLaunchKernelGGL(cc_apply_kernel<false>, dim3(grid), dim3(256), 0, st, mask, out, labels, keep, g, (int)to_bg);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
