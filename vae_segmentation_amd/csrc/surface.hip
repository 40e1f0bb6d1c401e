// Surface extraction, exact squared Euclidean distance transform and the surface-distance metrics ASSD / HD / HD95 of planar fp32 masks
// (include/vaeseg.h: vs_surface, vs_edt, vs_edt_workspace_bytes, vs_surface_distances).
//
// The reference has no such metric; the definitions are medpy's (metric/binary.py: __surface_distances, assd, hd, hd95) with scipy.ndimage's
// binary_erosion / distance_transform_edt underneath.  Every (n, c) plane is an independent problem.  T below is the value type of a squared
// distance: int32 for unit spacing (exact integers, INT32_MAX = "no feature voxel"), double for a given spacing (+inf).
//
//   surface  S(X) = X & ~erode(X): a wave owns a 64-wide row segment, takes the foreground bits of the 3 (6-connectivity: the centre row's
//            neighbours in y and z) or 9 rows around it as ballots and tests bits; rows / columns outside the volume are background
//   x pass   squared in-row distance to the nearest feature voxel: one wave per row, forward over its segments carrying the last feature
//            seen (ballot + count-leading-zeros), then backward carrying the next one (find-first-set), min of the two
//   y, z     out[i] = min_j (g[j] + (s (i - j))^2) per line, in place: a workgroup stages a slab — the whole axis x TX consecutive x columns,
//            so global accesses stay contiguous along x — in LDS; every lane scans outward from its i and stops once (s r)^2 reaches its
//            running minimum (no candidate further out can be smaller: g >= 0).  A min over exact values: independent of the evaluation order.
//   count    per 4096-voxel chunk and direction: surface voxels, sum of sqrt(d^2) (a fixed tree: no atomics) and max d^2
//   scan     per plane (one workgroup): exclusive scan of the chunk counts of both directions, the chunk sums added in a fixed order
//   scatter  the d^2 of every surface voxel into the plane's list: direction A->B first, then B->A, each in raster order
//   select   per plane (one workgroup): the order statistics v[k], v[k + 1] of the list for k = floor(0.95 (n - 1)) by bisecting the value
//            (T = double: its bit pattern) with counting passes, then the record
//
// Phase boundaries are launch boundaries, every loop is bounded by the data, there are no atomics at all: both builds of the library and every
// run give the same bits.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int SF_SEG = 64;           // x extent a wave owns in surface / x pass
constexpr int SF_CHUNK = 4096;       // voxels per workgroup in count / scatter: 256 threads x 16 iterations
constexpr int SF_SEL_NT = 1024;      // threads of the per-plane workgroups (scan, select)
constexpr int SF_MAX_AXIS = 1024;    // longest y / z axis: a slab of 8 columns of doubles is 64 KB of LDS
constexpr int SF_LDS_SOFT = 32768, SF_LDS_HARD = 65536;

struct sf_dims {
    int n, c, d, h, w;
    int V, nb;                       // voxels per plane, chunks per plane
    long long planes, total, cap;    // n * c, n * c * V, list entries per plane (2 V rounded up to 4)
};

template <typename T> struct sf_val;
template <> struct sf_val<int> {
    typedef unsigned int key_t;
    __host__ __device__ static constexpr int inf() { return INT_MAX; }
    __device__ static __forceinline__ int cost(int r, double s) { return r * r; }
    __device__ static __forceinline__ key_t key(int v) { return (key_t)v; }
    __device__ static __forceinline__ int unkey(key_t k) { return (int)k; }
};
template <> struct sf_val<double> {
    typedef unsigned long long key_t;
    __host__ __device__ static double inf() { return HUGE_VAL; }
    __device__ static __forceinline__ double cost(int r, double s) {
        const double t = s * (double)r;
        return t * t;
    }
    // non-negative doubles order like their bit patterns
    __device__ static __forceinline__ key_t key(double v) { return (key_t)__double_as_longlong(v); }
    __device__ static __forceinline__ double unkey(key_t k) { return __longlong_as_double((long long)k); }
};

__device__ __forceinline__ bool sf_on(float v) { return v >= 0.5f; }            // the binarize rule, utils/evaluation.py:9-10
__device__ __forceinline__ bool sf_on(unsigned char v) { return v != 0; }

// ---- surface -------------------------------------------------------------------------------------------------------------------------------
// foreground bits of one 64-wide segment of a row plus the voxel on either side of it (0 outside the row / volume)
struct sf_rowbits {
    unsigned long long m;
    bool left, right;
    __device__ __forceinline__ bool at(int lane) const { return (m >> lane) & 1ull; }
    __device__ __forceinline__ bool before(int lane) const { return lane ? (m >> (lane - 1)) & 1ull : left; }
    __device__ __forceinline__ bool after(int lane) const { return lane < 63 ? (m >> (lane + 1)) & 1ull : right; }
    __device__ __forceinline__ bool all3(int lane) const { return before(lane) && at(lane) && after(lane); }
};
__device__ __forceinline__ sf_rowbits sf_load_row(const float* rowp, bool row_ok, int x0, int w, int lane) {
    const int x = x0 + lane;
    const bool fg = row_ok && x < w && sf_on(rowp[x]);
    int xe = -1;
    if (lane == 0) xe = x0 - 1;
    if (lane == 1) xe = x0 + SF_SEG;
    const bool edge = row_ok && xe >= 0 && xe < w && sf_on(rowp[xe]);
    sf_rowbits r;
    r.m = __ballot(fg);
    const unsigned long long e = __ballot(edge);
    r.left = e & 1ull;
    r.right = (e >> 1) & 1ull;
    return r;
}

// masks m0 / m1 -> o0 / o1 (blockIdx.y picks the pair); OUT = float: 1.0 / 0.0, unsigned char: 1 / 0
template <int CONN, typename OUT>
__global__ __launch_bounds__(256) void sf_surface_kernel(const float* __restrict__ m0, const float* __restrict__ m1, OUT* __restrict__ o0, OUT* __restrict__ o1,
                                                         sf_dims g, long long nsegs, int segs) {
    const float* mask = blockIdx.y ? m1 : m0;
    OUT* out = blockIdx.y ? o1 : o0;
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long s = wave0; s < nsegs; s += nwaves) {
        const long long row = s / segs;                        // rows are (plane, z, y)
        const int x0 = (int)(s - row * segs) * SF_SEG;
        const long long pz = row / g.h;
        const int y = (int)(row - pz * g.h), z = (int)(pz % g.d);
        const float* rowp = mask + (size_t)row * g.w;
        const sf_rowbits own = sf_load_row(rowp, true, x0, g.w, lane);
        bool inside;                                           // every neighbour of the structure is foreground
        if (CONN == 6) {
            inside = own.before(lane) && own.after(lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {                      // every lane takes part in the ballots
                const int dz = r < 2 ? (r ? 1 : -1) : 0, dy = r < 2 ? 0 : (r == 2 ? -1 : 1);
                const bool ok = z + dz >= 0 && z + dz < g.d && y + dy >= 0 && y + dy < g.h;
                const sf_rowbits nb = sf_load_row(ok ? rowp + ((long long)dz * g.h + dy) * g.w : rowp, ok, x0, g.w, lane);
                inside = inside && nb.at(lane);
            }
        } else {
            inside = own.all3(lane);
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                if (r == 4) continue;
                const int dz = r / 3 - 1, dy = r % 3 - 1;
                const bool ok = z + dz >= 0 && z + dz < g.d && y + dy >= 0 && y + dy < g.h;
                const sf_rowbits nb = sf_load_row(ok ? rowp + ((long long)dz * g.h + dy) * g.w : rowp, ok, x0, g.w, lane);
                inside = inside && nb.all3(lane);
            }
        }
        const int x = x0 + lane;
        if (x < g.w) out[(size_t)row * g.w + x] = (OUT)(own.at(lane) && !inside ? 1 : 0);
    }
}

// ---- distance transform -------------------------------------------------------------------------------------------------------------------
template <typename SRC, typename T>
__global__ __launch_bounds__(256) void sf_xpass_kernel(const SRC* __restrict__ src, T* __restrict__ out, long long rows, int w, double sx) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const int segs = (w + SF_SEG - 1) / SF_SEG;
    for (long long row = wave0; row < rows; row += nwaves) {
        const SRC* sp = src + (size_t)row * w;
        T* op = out + (size_t)row * w;
        int carry = -1;                                        // x of the last feature voxel of the segments already passed
        for (int sg = 0; sg < segs; ++sg) {
            const int x = sg * SF_SEG + lane;
            const unsigned long long b = __ballot(x < w && sf_on(sp[x]));
            const unsigned long long upto = b & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
            const int left = upto ? sg * SF_SEG + 63 - __clzll(upto) : carry;
            if (x < w) op[x] = left >= 0 ? sf_val<T>::cost(x - left, sx) : sf_val<T>::inf();
            if (b) carry = sg * SF_SEG + 63 - __clzll(b);
        }
        carry = -1;
        for (int sg = segs - 1; sg >= 0; --sg) {
            const int x = sg * SF_SEG + lane;
            const unsigned long long b = __ballot(x < w && sf_on(sp[x]));
            const unsigned long long from = b & ~((1ull << lane) - 1ull);
            const int right = from ? sg * SF_SEG + __ffsll((long long)from) - 1 : carry;
            if (x < w && right >= 0) {
                const T v = sf_val<T>::cost(right - x, sx);
                if (v < op[x]) op[x] = v;                      // the lane's own store of the forward sweep
            }
            if (b) carry = sg * SF_SEG + __ffsll((long long)b) - 1;
        }
    }
}

// one axis of out[i] = min_j (g[j] + (s (i - j))^2), in place.  Slab q = (plane, o, x tile): element (i, col) at plane * V + o * ostride + i * stride + tile * TX + col
template <typename T>
__global__ __launch_bounds__(256) void sf_line_kernel(T* __restrict__ G, long long nslabs, int L, long long stride, int nother, long long ostride, int w, int V,
                                                      int TX, int ntiles, double s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sf_lds_raw[];
    T* lds = reinterpret_cast<T*>(sf_lds_raw);
    const int col = threadIdx.x & (TX - 1), i0 = threadIdx.x / TX, istep = 256 / TX;
    const T INF = sf_val<T>::inf();
    for (long long q = blockIdx.x; q < nslabs; q += gridDim.x) {
        const long long po = q / ntiles;
        const int tile = (int)(q - po * ntiles);
        const long long plane = po / nother;
        const int o = (int)(po - plane * nother);
        const int x = tile * TX + col;
        const bool live = x < w;
        T* base = G + (size_t)plane * V + (size_t)o * ostride + x;
        for (int i = i0; i < L; i += istep) lds[i * TX + col] = live ? base[(size_t)i * stride] : INF;
        __syncthreads();
        for (int i = i0; i < L; i += istep) {
            T best = lds[i * TX + col];
            for (int r = 1; r < L; ++r) {
                const T cost = sf_val<T>::cost(r, s);
                if (!(cost < best)) break;
                const int lo = i - r, hi = i + r;
                if (lo < 0 && hi >= L) break;
                if (lo >= 0) {
                    const T v = lds[lo * TX + col];
                    if (v < INF && v + cost < best) best = v + cost;
                }
                if (hi < L) {
                    const T v = lds[hi * TX + col];
                    if (v < INF && v + cost < best) best = v + cost;
                }
            }
            if (live) base[(size_t)i * stride] = best;
        }
        __syncthreads();
    }
}

// ---- metric reduction ----------------------------------------------------------------------------------------------------------------------

// a fixed tree: xor butterflies inside the wave, then the waves in order
template <int NT, typename T>
__device__ __forceinline__ T sf_block_sum(T v, T* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T tot = 0;
#pragma unroll
    for (int j = 0; j < NT / 64; ++j) tot += lds[j];
    __syncthreads();
    return tot;
}
template <int NT, typename T>
__device__ __forceinline__ T sf_block_max(T v, T* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T tot = lds[0];
#pragma unroll
    for (int j = 1; j < NT / 64; ++j) tot = lds[j] > tot ? lds[j] : tot;
    __syncthreads();
    return tot;
}
template <int NT, typename T>
__device__ __forceinline__ T sf_block_min(T v, T* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T tot = lds[0];
#pragma unroll
    for (int j = 1; j < NT / 64; ++j) tot = lds[j] < tot ? lds[j] : tot;
    __syncthreads();
    return tot;
}

// flags: unsigned char [2][planes][V] (surface of A, of B); maps: T [2][planes][V] (squared distance to S(A), to S(B)).
// direction 0 (A -> B): the voxels of S(A) read the distance to S(B); direction 1 the other way round.
// per (direction, plane, chunk): cnt, sum of sqrt, max.  SCATTER: the values go to list[plane][(dir ? count_ab : 0) + offs[dir][plane][chunk] + rank]
template <typename T, bool SCATTER>
__global__ __launch_bounds__(256) void sf_chunk_kernel(const unsigned char* __restrict__ flags, const T* __restrict__ maps, int* __restrict__ cnts,
                                                       double* __restrict__ sums, T* __restrict__ maxs, T* __restrict__ list, const long long* __restrict__ rec,
                                                       sf_dims g) {
    __shared__ int lds_i[4];
    __shared__ double lds_d[4];
    __shared__ T lds_t[4];
    const int dir = blockIdx.y;
    const long long p = blockIdx.x / g.nb;
    const int b = (int)(blockIdx.x - p * g.nb);
    const unsigned char* f = flags + ((size_t)dir * g.planes + p) * g.V;
    const T* m = maps + ((size_t)(1 - dir) * g.planes + p) * g.V;
    const size_t slot = ((size_t)dir * g.planes + p) * g.nb + b;
    int carry = SCATTER ? cnts[slot] : 0;
    const long long first = SCATTER && dir ? rec[p * (long long)(sizeof(vs_surface_record) / 8)] : 0;      // direction 1 follows count_ab entries
    double sum = 0.0;
    T mx = 0;
    for (int it = 0; it < SF_CHUNK / 256; ++it) {
        const long long e = (long long)b * SF_CHUNK + it * 256 + threadIdx.x;
        const bool on = e < g.V && f[e] != 0;
        const T v = on ? m[e] : (T)0;
        if (SCATTER) {
            int tot;
            const int ex = block_excl_scan<256>(on, &tot, lds_i);
            if (on) list[(size_t)p * g.cap + first + carry + ex] = v;
            carry += tot;
        } else {
            carry += on;
            sum += on ? sqrt((double)v) : 0.0;
            mx = v > mx ? v : mx;
        }
    }
    if (!SCATTER) {
        int tot;
        block_excl_scan<256>(carry, &tot, lds_i);
        const double s = sf_block_sum<256, double>(sum, lds_d);
        const T x = sf_block_max<256>(mx, lds_t);
        if (threadIdx.x == 0) {
            cnts[slot] = tot;
            sums[slot] = s;
            maxs[slot] = x;
        }
    }
}

// the record of one plane (include/vaeseg.h vs_surface_record)
struct sf_record {
    long long count_ab, count_ba;
    double sum_ab, sum_ba, max_sq, lo_sq, hi_sq, assd, hd, hd95;
};
static_assert(sizeof(sf_record) == sizeof(vs_surface_record), "record layout");

// chunk counts -> offsets into the direction's part of the plane's list; counts, sums and the maximum go to the record
template <typename T>
__global__ __launch_bounds__(SF_SEL_NT) void sf_scan_kernel(int* __restrict__ cnts, const double* __restrict__ sums, const T* __restrict__ maxs,
                                                            sf_record* __restrict__ rec, sf_dims g) {
    __shared__ int lds_i[SF_SEL_NT / 64];
    __shared__ double lds_d[SF_SEL_NT / 64];
    __shared__ T lds_t[SF_SEL_NT / 64];
    const long long p = blockIdx.x;
    int count[2];
    double total[2];
    T mx = 0;
    for (int dir = 0; dir < 2; ++dir) {
        const size_t at = ((size_t)dir * g.planes + p) * g.nb;
        int carry = 0;                                         // offsets are relative to the direction's own part of the list
        double part = 0.0;
        for (int base = 0; base < g.nb; base += SF_SEL_NT) {
            const int i = base + threadIdx.x;
            const int val = i < g.nb ? cnts[at + i] : 0;
            if (i < g.nb) {
                part += sums[at + i];
                mx = maxs[at + i] > mx ? maxs[at + i] : mx;
            }
            int tot;
            const int ex = block_excl_scan<SF_SEL_NT>(val, &tot, lds_i);
            if (i < g.nb) cnts[at + i] = carry + ex;
            carry += tot;
        }
        count[dir] = carry;
        total[dir] = sf_block_sum<SF_SEL_NT, double>(part, lds_d);
    }
    mx = sf_block_max<SF_SEL_NT>(mx, lds_t);
    if (threadIdx.x == 0) {
        sf_record r;
        r.count_ab = count[0]; r.count_ba = count[1];
        r.sum_ab = total[0]; r.sum_ba = total[1];
        r.max_sq = (double)mx;
        r.lo_sq = r.hi_sq = r.assd = r.hd = r.hd95 = 0.0;
        rec[p] = r;
    }
}

template <typename T>
__global__ __launch_bounds__(SF_SEL_NT) void sf_select_kernel(const T* __restrict__ list, sf_record* __restrict__ rec, sf_dims g) {
    typedef typename sf_val<T>::key_t key_t;
    __shared__ long long lds_l[SF_SEL_NT / 64];
    __shared__ key_t lds_k[SF_SEL_NT / 64];
    const long long p = blockIdx.x;
    sf_record r = rec[p];
    if (r.count_ab == 0 || r.count_ba == 0) {                  // an empty surface: nothing is defined
        if (threadIdx.x == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            r.count_ab = r.count_ba = 0;
            r.sum_ab = r.sum_ba = r.max_sq = r.lo_sq = r.hi_sq = r.assd = r.hd = r.hd95 = nan;
            rec[p] = r;
        }
        return;
    }
    const long long n = r.count_ab + r.count_ba;               // up to 2 V: beyond an int32 for the largest planes
    const T* v = list + (size_t)p * g.cap;
    const key_t kmax = sf_val<T>::key((T)r.max_sq);            // exact: the record holds the plane's maximum converted from T
    auto count_le = [&](key_t t) {
        long long c = 0;
        for (long long i = threadIdx.x; i < n; i += SF_SEL_NT) c += sf_val<T>::key(v[i]) <= t;
        return sf_block_sum<SF_SEL_NT, long long>(c, lds_l);
    };
    const double h = 0.95 * (double)(n - 1);                   // numpy.percentile(., 95), linear: virtual index, its floor, the fraction
    const long long k = (long long)floor(h);
    key_t lo = 0, hi = kmax;                                   // the smallest t with at least k + 1 values <= t: v[k]
    while (lo < hi) {
        const key_t mid = lo + (hi - lo) / 2;
        if (count_le(mid) >= k + 1) hi = mid; else lo = mid + 1;
    }
    key_t next = lo;                                           // v[k + 1]: the same value again, or the smallest one above it
    if (k + 1 < n && count_le(lo) < k + 2) {
        key_t mn = kmax;
        for (long long i = threadIdx.x; i < n; i += SF_SEL_NT) {
            const key_t t = sf_val<T>::key(v[i]);
            if (t > lo && t < mn) mn = t;
        }
        next = sf_block_min<SF_SEL_NT>(mn, lds_k);
    }
    if (threadIdx.x == 0) {
        r.lo_sq = (double)sf_val<T>::unkey(lo);
        r.hi_sq = (double)sf_val<T>::unkey(next);
        const double a = sqrt(r.lo_sq), b = sqrt(r.hi_sq);
        const double t = h - (double)k, diff = b - a;
        r.hd95 = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;       // numpy's _lerp
        r.hd = sqrt(r.max_sq);
        r.assd = 0.5 * (r.sum_ab / (double)r.count_ab + r.sum_ba / (double)r.count_ba);
        rec[p] = r;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
size_t sf_align(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: flags uchar[2][planes][V] | maps T[2][planes][V] | list T[planes][cap] | cnts int[2][planes][nb] | sums double[2][planes][nb] | maxs T[2][planes][nb]
struct sf_layout {
    size_t flags, maps, list, cnts, sums, maxs, bytes;
};
sf_layout sf_layout_of(const sf_dims& g, size_t sz) {
    sf_layout l;
    size_t o = 0;
    l.flags = o; o += sf_align((size_t)2 * g.total);
    l.maps = o;  o += sf_align((size_t)2 * g.total * sz);
    l.list = o;  o += sf_align((size_t)g.planes * g.cap * sz);
    l.cnts = o;  o += sf_align((size_t)2 * g.planes * g.nb * 4);
    l.sums = o;  o += sf_align((size_t)2 * g.planes * g.nb * 8);
    l.maxs = o;  o += sf_align((size_t)2 * g.planes * g.nb * sz);
    l.bytes = o;
    return l;
}

// VS_OK and *g filled, or the status of a rejected call.  integer: the unit-spacing path (squared distances must fit an int32)
int sf_check(int n, int c, int d, int h, int w, bool integer, sf_dims* g) {
    if (n <= 0 || c <= 0 || d <= 0 || h <= 0 || w <= 0) return VS_ESHAPE;
    if (d > SF_MAX_AXIS || h > SF_MAX_AXIS) return VS_ESHAPE;
    const long long V = (long long)d * h * w;
    if (V > INT_MAX) return VS_ESHAPE;                                   // plane-local indices are int32
    if (integer && (long long)d * d + (long long)h * h + (long long)w * w >= (long long)INT_MAX) return VS_ESHAPE;
    g->n = n; g->c = c; g->d = d; g->h = h; g->w = w;
    g->V = (int)V;
    g->nb = (int)((V + SF_CHUNK - 1) / SF_CHUNK);
    g->planes = (long long)n * c;
    g->total = g->planes * V;
    g->cap = (2 * V + 3) & ~3ll;
    if (g->planes * g->nb > INT_MAX) return VS_ESHAPE;                   // one workgroup per chunk
    return VS_OK;
}

int sf_check_spacing(const double* spacing) {
    if (!spacing) return VS_OK;
    for (int i = 0; i < 3; ++i)
        if (!(spacing[i] > 0.0) || !(spacing[i] < HUGE_VAL)) return VS_EINVAL;
    return VS_OK;
}

unsigned sf_grid(long long blocks) {
    const long long cap = 1 << 20;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

bool sf_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// columns per slab: a power of two up to 64, the slab within SF_LDS_SOFT bytes where 8 columns allow it (SF_MAX_AXIS keeps 8 columns within SF_LDS_HARD)
int sf_tile_x(int L, int w, size_t sz) {
    int tx = 64;
    while (tx > 8 && (size_t)L * tx * sz > (size_t)SF_LDS_SOFT) tx >>= 1;
    while (tx > 8 && tx / 2 >= w) tx >>= 1;
    return tx;
}

template <typename T>
int sf_line_launch(T* maps, long long planes, const sf_dims& g, int axis, double s, hipStream_t st) {
    const int L = axis == 1 ? g.h : g.d;
    if (L == 1) return VS_OK;
    const int tx = sf_tile_x(L, g.w, sizeof(T));
    const int ntiles = (g.w + tx - 1) / tx;
    const int nother = axis == 1 ? g.d : g.h;
    const long long stride = axis == 1 ? g.w : (long long)g.h * g.w, ostride = axis == 1 ? (long long)g.h * g.w : g.w;
    const long long nslabs = planes * nother * ntiles;
    const size_t lds = (size_t)L * tx * sizeof(T);
    if (lds > (size_t)SF_LDS_HARD) return VS_ESHAPE;
    hipLaunchKernelGGL(sf_line_kernel<T>, dim3(sf_grid(nslabs)), dim3(256), lds, st, maps, nslabs, L, stride, nother, ostride, g.w, g.V, tx, ntiles, s);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// squared distance to the feature voxels of src (planes x V elements), written to out
template <typename SRC, typename T>
int sf_edt_launch(const SRC* src, T* out, long long planes, const sf_dims& g, const double* spacing, hipStream_t st) {
    const double sz = spacing ? spacing[0] : 1.0, sy = spacing ? spacing[1] : 1.0, sx = spacing ? spacing[2] : 1.0;
    const long long rows = planes * g.d * g.h;
    hipLaunchKernelGGL((sf_xpass_kernel<SRC, T>), dim3(sf_grid((rows + 3) / 4)), dim3(256), 0, st, src, out, rows, g.w, sx);
    VS_CHECK_LAUNCH();
    int rc = sf_line_launch<T>(out, planes, g, 1, sy, st);
    if (rc != VS_OK) return rc;
    return sf_line_launch<T>(out, planes, g, 2, sz, st);
}

template <typename OUT>
int sf_surface_launch(const float* m0, const float* m1, OUT* o0, OUT* o1, const sf_dims& g, int connectivity, hipStream_t st) {
    const int segs = (g.w + SF_SEG - 1) / SF_SEG;
    const long long nsegs = g.planes * g.d * g.h * segs;
    const dim3 grid(sf_grid((nsegs + 3) / 4), m1 ? 2 : 1);
    if (connectivity == 26) hipLaunchKernelGGL((sf_surface_kernel<26, OUT>), grid, dim3(256), 0, st, m0, m1, o0, o1, g, nsegs, segs);
    else hipLaunchKernelGGL((sf_surface_kernel<6, OUT>), grid, dim3(256), 0, st, m0, m1, o0, o1, g, nsegs, segs);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

template <typename T>
int sf_distances_launch(const float* pred, const float* gt, sf_record* rec, char* ws, const sf_dims& g, int connectivity, const double* spacing, hipStream_t st) {
    const sf_layout l = sf_layout_of(g, sizeof(T));
    unsigned char* flags = (unsigned char*)(ws + l.flags);
    T* maps = (T*)(ws + l.maps);
    T* list = (T*)(ws + l.list);
    int* cnts = (int*)(ws + l.cnts);
    double* sums = (double*)(ws + l.sums);
    T* maxs = (T*)(ws + l.maxs);
    int rc = sf_surface_launch<unsigned char>(pred, gt, flags, flags + g.total, g, connectivity, st);
    if (rc != VS_OK) return rc;
    rc = sf_edt_launch<unsigned char, T>(flags, maps, 2 * g.planes, g, spacing, st);
    if (rc != VS_OK) return rc;
    const dim3 chunk_grid((unsigned)(g.planes * g.nb), 2);
    hipLaunchKernelGGL((sf_chunk_kernel<T, false>), chunk_grid, dim3(256), 0, st, flags, maps, cnts, sums, maxs, list, (const long long*)rec, g);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(sf_scan_kernel<T>, dim3((unsigned)g.planes), dim3(SF_SEL_NT), 0, st, cnts, sums, maxs, rec, g);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL((sf_chunk_kernel<T, true>), chunk_grid, dim3(256), 0, st, flags, maps, cnts, sums, maxs, list, (const long long*)rec, g);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(sf_select_kernel<T>, dim3((unsigned)g.planes), dim3(SF_SEL_NT), 0, st, list, rec, g);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

}  // namespace

extern "C" int vs_surface(const float* mask, float* out, int n, int c, int d, int h, int w, int connectivity, void* stream) {
    sf_dims g;
    if (connectivity != 6 && connectivity != 26) return VS_EINVAL;
    const int rc = sf_check(n, c, d, h, w, false, &g);
    if (rc != VS_OK) return rc;
    if (!mask || !out || mask == out) return VS_EINVAL;
    if (sf_misaligned(mask) || sf_misaligned(out)) return VS_EALIGN;
    return sf_surface_launch<float>(mask, nullptr, out, nullptr, g, connectivity, (hipStream_t)stream);
}

extern "C" long long vs_edt_workspace_bytes(int n, int c, int d, int h, int w, int with_spacing) {
    sf_dims g;
    const int rc = sf_check(n, c, d, h, w, !with_spacing, &g);
    if (rc != VS_OK) return rc;
    return (long long)sf_layout_of(g, with_spacing ? 8 : 4).bytes;
}

extern "C" int vs_edt(const float* feature, void* out, int n, int c, int d, int h, int w, const double* spacing, void* stream) {
    sf_dims g;
    const int rc = sf_check(n, c, d, h, w, !spacing, &g);
    if (rc != VS_OK) return rc;
    if (sf_check_spacing(spacing) != VS_OK) return VS_EINVAL;
    if (!feature || !out || (const void*)feature == out) return VS_EINVAL;
    if (sf_misaligned(feature) || sf_misaligned(out)) return VS_EALIGN;
    if (spacing) return sf_edt_launch<float, double>(feature, (double*)out, g.planes, g, spacing, (hipStream_t)stream);
    return sf_edt_launch<float, int>(feature, (int*)out, g.planes, g, nullptr, (hipStream_t)stream);
}

extern "C" int vs_surface_distances(const float* pred, const float* gt, vs_surface_record* out, int n, int c, int d, int h, int w, int connectivity,
                                    const double* spacing, void* workspace, void* stream) {
    sf_dims g;
    if (connectivity != 6 && connectivity != 26) return VS_EINVAL;
    const int rc = sf_check(n, c, d, h, w, !spacing, &g);
    if (rc != VS_OK) return rc;
    if (sf_check_spacing(spacing) != VS_OK) return VS_EINVAL;
    if (!pred || !gt || !out || !workspace) return VS_EINVAL;
    if ((const void*)out == (const void*)pred || (const void*)out == (const void*)gt || workspace == (const void*)pred || workspace == (const void*)gt ||
        workspace == (void*)out)
        return VS_EINVAL;
    if (sf_misaligned(pred) || sf_misaligned(gt) || sf_misaligned(out) || sf_misaligned(workspace)) return VS_EALIGN;
    if (spacing) return sf_distances_launch<double>(pred, gt, (sf_record*)out, (char*)workspace, g, connectivity, spacing, (hipStream_t)stream);
    return sf_distances_launch<int>(pred, gt, (sf_record*)out, (char*)workspace, g, connectivity, nullptr, (hipStream_t)stream);
}
