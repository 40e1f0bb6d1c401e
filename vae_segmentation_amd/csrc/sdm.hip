// Signed distance maps of a label volume and the boundary loss on them (include/vaeseg.h: vs_signed_distance*, vs_boundary_loss_*).
// The reference has no counterpart; the loss is Kervadec et al. (MIDL 2019), the map their one_hot2dist, the rule is stated in the header.
//
//   class of a voxel: (int)label where 0 <= label < n_class in fp32, none otherwise (segloss.hip's valid-label rule).  P_c = the voxels of class c; every
//   other voxel of the volume, the classless ones included, is outside P_c.  T below is the type of a squared distance: int32 for unit spacing (exact,
//   INT_MAX = "no such voxel"), double under a spacing (+inf).  The workspace holds, per (sample, class of [bot, top)), two maps of V values of T:
//   map 0 = squared distance to the nearest voxel of P_c, map 1 = to the nearest voxel outside P_c.
//
//   x pass   a wave owns a row of the LABEL: per class and 64-wide segment the membership ballots of both sets, forward over the segments carrying the last
//            voxel of each set (count-leading-zeros), then backward carrying the next one (find-first-set), min of the two.  Writes every entry of both maps
//            of every class: nothing has to be cleared first.
//   y pass   out[i] = min_j (g[j] + (s (i - j))^2) per line of both maps, in place: a workgroup stages a slab — the whole axis x TX consecutive x columns — in
//            LDS and every lane scans outward from its i, four distances per trip, until (s r)^2 reaches its running minimum.  A column of the slab without
//            a finite entry is left alone (a flag per column, set while staging).  A voxel's sign is not known from a row: both maps go on.
//   z pass   the same scan along z, but a voxel reads only the map opposite to its own membership (a voxel of P_c: map 1, any other: map 0) — the label is
//            read again for that — and stores phi as fp32: +sqrt outside, 1 - sqrt inside, 0.0 where the minimum is still the "no such voxel" value
//            (P_c empty, or the whole volume).  Square root and subtraction in fp64, one rounding.  No combine launch, no fp64 volume on the integer path.
//
// The loss: per-workgroup fp64 partials of sum p_c phi_c over the valid voxels and of their number, a one-workgroup finish in a fixed order, one backward
// launch.  No atomics, no memset, nothing allocated, synchronised or read back anywhere in this file; both builds compile the same code.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int SD_SEG = 64;                     // x extent of one ballot of the x pass
constexpr int SD_STEP = 4;                     // distances a lane of the y / z passes tries per trip of its scan
constexpr int SD_TX_MAX = 32;                  // widest slab: 32 columns = one 128-byte line of int32 per row; narrower slabs mean more workgroups
constexpr int SD_MIN_SLABS = 1024;             // slabs a y / z launch should hold before its slabs grow past 8 columns: four workgroups per CU
static_assert(256 / SD_TX_MAX >= 8, "sd_zpass_kernel keeps a lane's memberships in 128 bits");
constexpr int SD_MAX_AXIS = 1024;              // longest y / z axis: a slab of 4 columns of doubles and its flags is 32 KB of LDS
constexpr int SD_LDS_SOFT = 32768, SD_LDS_HARD = 65536;
constexpr int BL_BLOCKS = 512;                 // block cap of the loss grids: 512 x 256 elements (quads, or voxels on the unaligned path) per sweep
constexpr int BL_MAXB = 64;                    // bl_finish_kernel keeps 2 totals per sample in LDS

struct sd_dims {
    int n, k, bot, n_class, d, h, w, V;        // k = top - bot planes per sample
};

template <typename T> struct sd_val;
template <> struct sd_val<int> {
    __host__ __device__ static constexpr int inf() { return INT_MAX; }
    // 0 <= r < 46341 < 2^24: the 24-bit multiply (full rate; the 32-bit one is quarter rate, and a lane of the y / z passes squares four distances per trip)
    __device__ static __forceinline__ int cost(int r, double s) { return __mul24(r, r); }
};
template <> struct sd_val<double> {
    __host__ __device__ static double inf() { return HUGE_VAL; }
    __device__ static __forceinline__ double cost(int r, double s) {
        const double t = s * (double)r;
        return t * t;
    }
};

// the class of a label value, -1 for none (NaN fails both comparisons)
__device__ __forceinline__ int sd_class(float lf, int n_class) { return lf >= 0.f && lf < (float)n_class ? (int)lf : -1; }

// ---- x pass ---------------------------------------------------------------------------------------------------------------------------------
// rows are (sample, z, y) of the label; maps[((b * k + j) * 2 + which) * V + voxel]
template <typename T>
__global__ __launch_bounds__(256) void sd_xpass_kernel(const float* __restrict__ label, T* __restrict__ maps, long long rows, sd_dims g, double sx) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const int segs = (g.w + SD_SEG - 1) / SD_SEG, per_sample = g.d * g.h;
    const unsigned long long upto_me = lane == 63 ? ~0ull : ((2ull << lane) - 1ull), from_me = ~((1ull << lane) - 1ull);
    const T INF = sd_val<T>::inf();
    for (long long row = wave0; row < rows; row += nwaves) {
        const long long b = row / per_sample;
        const size_t in_sample = (size_t)(row - b * per_sample) * g.w;
        const float* lp = label + (size_t)row * g.w;
        for (int j = 0; j < g.k; ++j) {
            const int c = g.bot + j;
            T* m_in = maps + ((size_t)(b * g.k + j) * 2) * g.V + in_sample;        // distance to P_c
            T* m_out = m_in + g.V;                                                 // distance to its complement
            int last_in = -1, last_out = -1;                                       // x of the last voxel of either set in the segments already passed
            for (int sg = 0; sg < segs; ++sg) {
                const int x = sg * SD_SEG + lane;
                const bool live = x < g.w;
                const bool member = live && sd_class(lp[live ? x : 0], g.n_class) == c;
                const unsigned long long bi = __ballot(member), bo = __ballot(live && !member);
                const unsigned long long ui = bi & upto_me, uo = bo & upto_me;
                const int li = ui ? sg * SD_SEG + 63 - __clzll(ui) : last_in;
                const int lo = uo ? sg * SD_SEG + 63 - __clzll(uo) : last_out;
                if (live) {
                    m_in[x] = li >= 0 ? sd_val<T>::cost(x - li, sx) : INF;
                    m_out[x] = lo >= 0 ? sd_val<T>::cost(x - lo, sx) : INF;
                }
                if (bi) last_in = sg * SD_SEG + 63 - __clzll(bi);
                if (bo) last_out = sg * SD_SEG + 63 - __clzll(bo);
            }
            int next_in = -1, next_out = -1;
            for (int sg = segs - 1; sg >= 0; --sg) {
                const int x = sg * SD_SEG + lane;
                const bool live = x < g.w;
                const bool member = live && sd_class(lp[live ? x : 0], g.n_class) == c;
                const unsigned long long bi = __ballot(member), bo = __ballot(live && !member);
                const unsigned long long fi = bi & from_me, fo = bo & from_me;
                const int ri = fi ? sg * SD_SEG + __ffsll((long long)fi) - 1 : next_in;
                const int ro = fo ? sg * SD_SEG + __ffsll((long long)fo) - 1 : next_out;
                if (live) {                                                        // the lane's own stores of the forward sweep
                    if (ri >= 0) {
                        const T v = sd_val<T>::cost(ri - x, sx);
                        if (v < m_in[x]) m_in[x] = v;
                    }
                    if (ro >= 0) {
                        const T v = sd_val<T>::cost(ro - x, sx);
                        if (v < m_out[x]) m_out[x] = v;
                    }
                }
                if (bi) next_in = sg * SD_SEG + __ffsll((long long)bi) - 1;
                if (bo) next_out = sg * SD_SEG + __ffsll((long long)bo) - 1;
            }
        }
    }
}

// min_j (line[j] + (s (i - j))^2) for the lane's column of a staged slab; stops once (s r)^2 alone reaches the running minimum: every entry is >= 0, so no
// candidate further out can be smaller.  SD_STEP distances per trip: their 2 SD_STEP LDS reads are independent of the running minimum and are issued
// together, so a trip costs one LDS latency, not SD_STEP; the steps taken past the stopping distance within a trip cannot lower the minimum either
// (their cost alone is >= it).  A min over exact values: independent of the order.
template <typename T>
__device__ __forceinline__ T sd_scan(const T* lds, int i, int L, int tsh, int col, double s) {
    const T INF = sd_val<T>::inf();
    T best = lds[(i << tsh) + col];
    for (int r = 1; r < L; r += SD_STEP) {
        if (!(sd_val<T>::cost(r, s) < best)) break;
        if (i - r < 0 && i + r >= L) break;
        T a[SD_STEP], b[SD_STEP];
#pragma unroll
        for (int u = 0; u < SD_STEP; ++u) {                                        // clamped addresses: every read is inside the slab
            const int lo = i - r - u, hi = i + r + u;
            a[u] = lds[((lo >= 0 ? lo : 0) << tsh) + col];
            b[u] = lds[((hi < L ? hi : L - 1) << tsh) + col];
        }
#pragma unroll
        for (int u = 0; u < SD_STEP; ++u) {
            const T cost = sd_val<T>::cost(r + u, s);                              // r + u < L + SD_STEP: its square fits
            if (i - r - u >= 0 && a[u] < INF && a[u] + cost < best) best = a[u] + cost;      // INF never enters a sum: no integer overflow
            if (i + r + u < L && b[u] < INF && b[u] + cost < best) best = b[u] + cost;
        }
    }
    return best;
}

// stage the lane's part of a slab and learn which of its columns hold a finite entry at all: a column without one keeps INF everywhere, and none of its
// voxels has anything to scan for (most columns of the map "to P_c" of a small organ).  flag: TX ints behind the slab; every writer stores the same 1.
template <typename T>
__device__ __forceinline__ void sd_stage(T* lds, int* flag, const T* src, size_t stride, bool live, int L, int tsh, int col, int i0, int istep) {
    const T INF = sd_val<T>::inf();
    if (threadIdx.x < (1u << tsh)) flag[threadIdx.x] = 0;
    __syncthreads();
    bool any = false;
    int i = i0;
    for (; i + 3 * istep < L; i += 4 * istep) {                                    // four loads in flight: a lane's rows are a chain of memory latencies otherwise
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = live ? src[(size_t)(i + u * istep) * stride] : INF;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            lds[((i + u * istep) << tsh) + col] = v[u];
            any = any || v[u] < INF;
        }
    }
    for (; i < L; i += istep) {
        const T v = live ? src[(size_t)i * stride] : INF;
        lds[(i << tsh) + col] = v;
        any = any || v < INF;
    }
    if (any) flag[col] = 1;
    __syncthreads();
}

// ---- y pass: both maps of every (sample, class), in place.  Slab q = (map plane, z, x tile) -------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void sd_ypass_kernel(T* __restrict__ maps, long long nslabs, sd_dims g, int tsh, int ntiles, double s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sd_lds_raw[];
    T* lds = reinterpret_cast<T*>(sd_lds_raw);
    const int TX = 1 << tsh, col = threadIdx.x & (TX - 1), i0 = threadIdx.x >> tsh, istep = 256 >> tsh, L = g.h;      // a slab is TX = 2^tsh columns wide
    int* flag = reinterpret_cast<int*>(lds + (size_t)L * TX);
    for (long long q = blockIdx.x; q < nslabs; q += gridDim.x) {
        const long long pz = q / ntiles;                                           // (map plane, z)
        const int x = (int)(q - pz * ntiles) * TX + col;
        const bool live = x < g.w;
        T* base = maps + (size_t)pz * L * g.w + x;                                 // plane * V + z * h * w
        sd_stage<T>(lds, flag, base, (size_t)g.w, live, L, tsh, col, i0, istep);
        if (live && flag[col]) {                                                   // a column without a finite entry stays as the x pass left it
            for (int i = i0; i < L; i += istep) base[(size_t)i * g.w] = sd_scan<T>(lds, i, L, tsh, col, s);
        }
        __syncthreads();
    }
}

// ---- z pass: reads the label and the map opposite to each voxel's membership, writes phi.  Slab q = (sample, class, y, x tile) --------------------
template <typename T>
__global__ __launch_bounds__(256) void sd_zpass_kernel(const float* __restrict__ label, const T* __restrict__ maps, float* __restrict__ phi, long long nslabs,
                                                       sd_dims g, int tsh, int ntiles, double s) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sd_lds_raw[];
    T* lds = reinterpret_cast<T*>(sd_lds_raw);
    const int TX = 1 << tsh, col = threadIdx.x & (TX - 1), i0 = threadIdx.x >> tsh, istep = 256 >> tsh, L = g.d;
    const size_t hw = (size_t)g.h * g.w;
    const T INF = sd_val<T>::inf();
    int* flag = reinterpret_cast<int*>(lds + (size_t)L * TX);
    for (long long q = blockIdx.x; q < nslabs; q += gridDim.x) {
        const long long py = q / ntiles;                                           // (sample, class, y)
        const int x = (int)(q - py * ntiles) * TX + col;
        const long long bj = py / g.h;                                             // sample * k + class index
        const int y = (int)(py - bj * g.h);
        const long long b = bj / g.k;
        const int c = g.bot + (int)(bj - b * g.k);
        const bool live = x < g.w;
        const size_t at = (size_t)y * g.w + x;
        const float* lp = label + (size_t)b * g.V + at;
        float* op = phi + (size_t)bj * g.V + at;
        // the membership of the lane's voxels, one bit each — at most SD_MAX_AXIS / (256 / SD_TX_MAX) = 128 — read once, ahead of both maps
        unsigned long long m0 = 0, m1 = 0;
        if (live) {
            int n = 0;
#pragma unroll 4
            for (int i = i0; i < L; i += istep, ++n) {
                const unsigned long long bit = sd_class(lp[i * hw], g.n_class) == c ? 1ull : 0ull;
                if (n < 64) m0 |= bit << n; else m1 |= bit << (n - 64);
            }
        }
        for (int which = 0; which < 2; ++which) {
            const T* src = maps + ((size_t)bj * 2 + which) * g.V + at;
            sd_stage<T>(lds, flag, src, hw, live, L, tsh, col, i0, istep);
            const bool finite = flag[col] != 0;
            int n = 0;
            for (int i = i0; i < L; i += istep, ++n) {
                if (!live) continue;
                const bool member = ((n < 64 ? m0 >> n : m1 >> (n - 64)) & 1ull) != 0;
                if ((int)member != which) continue;                                // a voxel of P_c measures to the complement (map 1), any other to P_c (map 0)
                const T best = finite ? sd_scan<T>(lds, i, L, tsh, col, s) : INF;
                double r = 0.0;                                                    // still "no such voxel": P_c is empty, or the whole volume
                if (best < INF) {
                    const double e = sqrt((double)best);
                    r = member ? 1.0 - e : e;
                }
                op[i * hw] = (float)r;
            }
            __syncthreads();
        }
    }
}

// ---- boundary loss --------------------------------------------------------------------------------------------------------------------------
// An element is a quad of voxels (VEC: 16-byte loads) or one voxel.  part[(b * 2 + stat) * gridDim.x + block]: stat 0 = sum over the valid voxels and the
// channels [bot, top) of p_c phi_c — the product of two promoted fp32 values is exact in fp64 —, stat 1 = the number of valid voxels
template <bool VEC>
__global__ __launch_bounds__(256) void bl_partial_kernel(const float* __restrict__ p, const float* __restrict__ label, const float* __restrict__ phi,
                                                         double* __restrict__ part, long long voxels, int channels, int bot, int top) {
    constexpr int E = VEC ? 4 : 1;
    const int b = blockIdx.y, k = top - bot;
    const float* lb = label + (size_t)b * voxels;
    const float* pb = p + ((size_t)b * channels + bot) * voxels;
    const float* fb = phi + (size_t)b * k * voxels;
    double acc = 0.0;
    int cnt = 0;
    const long long ne = voxels / E;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < ne; i += (long long)gridDim.x * 256) {
        float l[E];
        bool valid[E];
        if (VEC) {
            const f32x4 l4 = *(const f32x4*)(lb + i * 4);
#pragma unroll
            for (int e = 0; e < E; ++e) l[e] = l4[e];
        } else {
            l[0] = lb[i];
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            valid[e] = l[e] >= 0.f && l[e] < (float)channels;
            cnt += valid[e] ? 1 : 0;
        }
        for (int j = 0; j < k; ++j) {
            if (VEC) {
                const f32x4 x = *(const f32x4*)(pb + (size_t)j * voxels + i * 4), f = *(const f32x4*)(fb + (size_t)j * voxels + i * 4);
#pragma unroll
                for (int e = 0; e < E; ++e) acc += valid[e] ? (double)x[e] * (double)f[e] : 0.0;
            } else {
                acc += valid[0] ? (double)pb[(size_t)j * voxels + i] * (double)fb[(size_t)j * voxels + i] : 0.0;
            }
        }
    }
    __shared__ double red[4][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double s = wave_sum_d(acc), n = wave_sum_d((double)cnt);                 // a count is exact in fp64
    if (lane == 0) { red[wave][0] = s; red[wave][1] = n; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        part[((size_t)b * 2 + q) * gridDim.x + blockIdx.x] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

// head[b * 2] = S_b, head[b * 2 + 1] = N_b;  terms = (L_B, w L_B), L_B = 1 / (B k) sum_b S_b / N_b (0 for N_b = 0)
__global__ __launch_bounds__(256) void bl_finish_kernel(const double* __restrict__ part, double* __restrict__ head, const float* __restrict__ weight,
                                                        float* __restrict__ terms, int batch, int k, int nblk) {
    __shared__ double s_wave[4];
    __shared__ double s_tot[BL_MAXB * 2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = 0; i < batch * 2; ++i) {                                          // every order is fixed: thread t adds blocks t, t + 256, ...
        double t = 0.0;
        for (int blk = threadIdx.x; blk < nblk; blk += 256) t += part[(size_t)i * nblk + blk];
        t = wave_sum_d(t);
        if (lane == 0) s_wave[wave] = t;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double tot = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
            s_tot[i] = tot;
            head[i] = tot;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double m = 0.0;
        for (int b = 0; b < batch; ++b) m += s_tot[b * 2 + 1] > 0.0 ? s_tot[b * 2] / s_tot[b * 2 + 1] : 0.0;
        const double L = m / ((double)batch * (double)k);
        terms[0] = (float)L;
        terms[1] = (float)((double)weight[0] * L);
    }
}

// gp[b][c][v] = gout w phi_c(v) / (B k N_b) at a valid voxel of a channel of [bot, top), formed in fp64 and rounded once; 0.0 everywhere else
template <bool VEC>
__global__ __launch_bounds__(256) void bl_bwd_kernel(const float* __restrict__ label, const float* __restrict__ phi, const float* __restrict__ weight,
                                                     const double* __restrict__ head, const float* __restrict__ gout, float* __restrict__ gp, int batch,
                                                     long long voxels, int channels, int bot, int top) {
    constexpr int E = VEC ? 4 : 1;
    const int b = blockIdx.y, k = top - bot;
    const double N = head[b * 2 + 1];
    const double coef = N > 0.0 ? (double)gout[0] * (double)weight[0] / ((double)batch * (double)k * N) : 0.0;
    const float* lb = label + (size_t)b * voxels;
    const float* fb = phi + (size_t)b * k * voxels;
    float* gb = gp + (size_t)b * channels * voxels;
    const long long ne = voxels / E;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < ne; i += (long long)gridDim.x * 256) {
        bool valid[E];
        if (VEC) {
            const f32x4 l4 = *(const f32x4*)(lb + i * 4);
#pragma unroll
            for (int e = 0; e < E; ++e) valid[e] = l4[e] >= 0.f && l4[e] < (float)channels;
        } else {
            const float l = lb[i];
            valid[0] = l >= 0.f && l < (float)channels;
        }
        for (int c = 0; c < channels; ++c) {
            const bool in_range = c >= bot && c < top;                             // uniform
            if (VEC) {
                f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
                if (in_range) {
                    const f32x4 f = *(const f32x4*)(fb + (size_t)(c - bot) * voxels + i * 4);
#pragma unroll
                    for (int e = 0; e < E; ++e) o[e] = valid[e] ? (float)(coef * (double)f[e]) : 0.f;
                }
                *(f32x4*)(gb + (size_t)c * voxels + i * 4) = o;
            } else {
                float o = 0.f;
                if (in_range && valid[0]) o = (float)(coef * (double)fb[(size_t)(c - bot) * voxels + i]);
                gb[(size_t)c * voxels + i] = o;
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
// VS_OK and *g filled, or the status of a rejected call.  integer: the unit-spacing path (squared distances must fit an int32)
int sd_check(int n, int n_class, int bot, int top, int d, int h, int w, bool integer, sd_dims* g) {
    if (n <= 0 || d <= 0 || h <= 0 || w <= 0) return VS_ESHAPE;
    if (n_class < 1 || bot < 0 || top > n_class || bot >= top) return VS_EINVAL;
    if (d > SD_MAX_AXIS || h > SD_MAX_AXIS) return VS_ESHAPE;
    const long long V = (long long)d * h * w;
    if (V > INT_MAX) return VS_ESHAPE;                                             // sample-local indices are int32
    if (integer && (long long)d * d + (long long)h * h + (long long)w * w >= (long long)INT_MAX) return VS_ESHAPE;
    g->n = n; g->k = top - bot; g->bot = bot; g->n_class = n_class; g->d = d; g->h = h; g->w = w; g->V = (int)V;
    return VS_OK;
}

int sd_check_spacing(const double* spacing) {
    if (!spacing) return VS_OK;
    for (int i = 0; i < 3; ++i)
        if (!(spacing[i] > 0.0) || !(spacing[i] < HUGE_VAL)) return VS_EINVAL;
    return VS_OK;
}

unsigned sd_grid(long long blocks) {
    const long long cap = 1 << 20;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

int sd_log2(int tx) { return tx == 4 ? 2 : tx == 8 ? 3 : tx == 16 ? 4 : 5; }

// LDS of a slab: L x tx values and the tx column flags behind them
size_t sd_lds_bytes(int L, int tx, size_t sz) { return (size_t)L * tx * sz + (size_t)tx * sizeof(int); }

// columns per slab: a power of two up to SD_TX_MAX, halved — but not below 8 — while the slab passes SD_LDS_SOFT bytes, while it is at least twice as wide
// as the row, and while the launch (`lines` lines of slabs) would hold fewer than SD_MIN_SLABS workgroups: a 96^3 volume is 576 slabs of 32 columns, two
// per CU, and a lane's scan is a chain of LDS latencies that only other waves hide.  The one case 8 columns do not fit SD_LDS_HARD — an axis of
// SD_MAX_AXIS doubles, 64 KB before the flags — takes 4.
int sd_tile_x(int L, int w, size_t sz, long long lines) {
    int tx = SD_TX_MAX;
    while (tx > 8 && sd_lds_bytes(L, tx, sz) > (size_t)SD_LDS_SOFT) tx >>= 1;
    while (tx > 8 && tx / 2 >= w) tx >>= 1;
    while (tx > 8 && lines * ((w + tx - 1) / tx) < SD_MIN_SLABS) tx >>= 1;
    while (tx > 4 && sd_lds_bytes(L, tx, sz) > (size_t)SD_LDS_HARD) tx >>= 1;
    return tx;
}

template <typename T>
int sd_launch(const float* label, float* phi, T* maps, const sd_dims& g, const double* spacing, hipStream_t st) {
    const double sz = spacing ? spacing[0] : 1.0, sy = spacing ? spacing[1] : 1.0, sx = spacing ? spacing[2] : 1.0;
    const long long ylines = (long long)g.n * g.k * 2 * g.d, zlines = (long long)g.n * g.k * g.h;
    const int txy = sd_tile_x(g.h, g.w, sizeof(T), ylines), txz = sd_tile_x(g.d, g.w, sizeof(T), zlines);
    const size_t ldsy = sd_lds_bytes(g.h, txy, sizeof(T)), ldsz = sd_lds_bytes(g.d, txz, sizeof(T));
    if (ldsy > (size_t)SD_LDS_HARD || ldsz > (size_t)SD_LDS_HARD) return VS_ESHAPE;      // before the first launch
    const long long rows = (long long)g.n * g.d * g.h;
    hipLaunchKernelGGL(sd_xpass_kernel<T>, dim3(sd_grid((rows + 3) / 4)), dim3(256), 0, st, label, maps, rows, g, sx);
    VS_CHECK_LAUNCH();
    if (g.h > 1) {
        const int ntiles = (g.w + txy - 1) / txy;
        const long long nslabs = ylines * ntiles;
        hipLaunchKernelGGL(sd_ypass_kernel<T>, dim3(sd_grid(nslabs)), dim3(256), ldsy, st, maps, nslabs, g, sd_log2(txy), ntiles, sy);
        VS_CHECK_LAUNCH();
    }
    const int ntiles = (g.w + txz - 1) / txz;
    const long long nslabs = zlines * ntiles;
    hipLaunchKernelGGL(sd_zpass_kernel<T>, dim3(sd_grid(nslabs)), dim3(256), ldsz, st, label, (const T*)maps, phi, nslabs, g, sd_log2(txz), ntiles, sz);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

int bl_args(const void* label, const void* phi, const void* weight, const void* scratch, int batch, int channels, int bot, int top, long long voxels) {
    if (!label || !phi || !weight || !scratch) return VS_EINVAL;
    if (channels < 1 || batch <= 0 || voxels <= 0 || bot < 0 || top > channels || bot >= top) return VS_EINVAL;
    if (batch > BL_MAXB || voxels >= (1ll << 31)) return VS_ESHAPE;
    if (misaligned(label, 4) || misaligned(phi, 4) || misaligned(weight, 4) || misaligned(scratch, 8)) return VS_EALIGN;
    return VS_OK;
}

unsigned bl_blocks(long long elements) {
    const long long blocks = (elements + 255) / 256;
    return (unsigned)(blocks > BL_BLOCKS ? BL_BLOCKS : (blocks < 1 ? 1 : blocks));
}

}  // namespace

extern "C" long long vs_signed_distance_workspace_bytes(int n, int classes, int d, int h, int w, int with_spacing) {
    sd_dims g;
    if (classes < 1) return VS_EINVAL;
    const int rc = sd_check(n, classes, 0, classes, d, h, w, !with_spacing, &g);
    if (rc != VS_OK) return rc;
    const long long bytes = (long long)n * classes * 2 * g.V * (with_spacing ? 8 : 4);
    return (bytes + 255) & ~255ll;
}

extern "C" int vs_signed_distance(const float* label, float* phi, int n, int n_class, int bot, int top, int d, int h, int w, const double* spacing,
                                  void* workspace, void* stream) {
    sd_dims g;
    const int rc = sd_check(n, n_class, bot, top, d, h, w, !spacing, &g);
    if (rc != VS_OK) return rc;
    if (sd_check_spacing(spacing) != VS_OK) return VS_EINVAL;
    if (!label || !phi || !workspace) return VS_EINVAL;
    if ((const void*)label == (const void*)phi || workspace == (const void*)label || workspace == (void*)phi) return VS_EINVAL;
    if (misaligned(label, 16) || misaligned(phi, 16) || misaligned(workspace, 16)) return VS_EALIGN;
    if (spacing) return sd_launch<double>(label, phi, (double*)workspace, g, spacing, (hipStream_t)stream);
    return sd_launch<int>(label, phi, (int*)workspace, g, nullptr, (hipStream_t)stream);
}

extern "C" long long vs_boundary_loss_scratch_doubles(int b, int c) {
    if (b <= 0 || b > BL_MAXB || c < 1) return 0;
    return (long long)b * 2 * (1 + BL_BLOCKS);
}

extern "C" int vs_boundary_loss_fwd(const float* p, const float* label, const float* phi, const float* weight_dev, double* scratch, float* terms, int b,
                                    int c, int bot, int top, long long voxels, void* stream) {
    const int rc = bl_args(label, phi, weight_dev, scratch, b, c, bot, top, voxels);
    if (rc) return rc;
    if (!p || !terms) return VS_EINVAL;
    if (misaligned(p, 4) || misaligned(terms, 4)) return VS_EALIGN;
    const bool vec = !(voxels & 3) && !misaligned(p, 16) && !misaligned(label, 16) && !misaligned(phi, 16);
    const unsigned blocks = bl_blocks(vec ? voxels / 4 : voxels);
    double* part = scratch + (size_t)b * 2;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(bl_partial_kernel<true>, dim3(blocks, b), dim3(256), 0, st, p, label, phi, part, voxels, c, bot, top);
    else hipLaunchKernelGGL(bl_partial_kernel<false>, dim3(blocks, b), dim3(256), 0, st, p, label, phi, part, voxels, c, bot, top);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bl_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)part, scratch, weight_dev, terms, b, top - bot, (int)blocks);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_boundary_loss_bwd(const float* label, const float* phi, const float* weight_dev, const double* scratch, const float* gout, float* gp,
                                    int b, int c, int bot, int top, long long voxels, void* stream) {
    const int rc = bl_args(label, phi, weight_dev, scratch, b, c, bot, top, voxels);
    if (rc) return rc;
    if (!gout || !gp) return VS_EINVAL;
    if (misaligned(gout, 4) || misaligned(gp, 4)) return VS_EALIGN;
    const bool vec = !(voxels & 3) && !misaligned(label, 16) && !misaligned(phi, 16) && !misaligned(gp, 16);
    const unsigned blocks = bl_blocks(vec ? voxels / 4 : voxels);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(bl_bwd_kernel<true>, dim3(blocks, b), dim3(256), 0, st, label, phi, weight_dev, scratch, gout, gp, b, voxels, c, bot, top);
    else hipLaunchKernelGGL(bl_bwd_kernel<false>, dim3(blocks, b), dim3(256), 0, st, label, phi, weight_dev, scratch, gout, gp, b, voxels, c, bot, top);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
