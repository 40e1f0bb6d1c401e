// The compound segmentation loss with a TOP-K cross-entropy: the voxel loss averaged over the hardest K = max(1, floor(r N)) of the N valid voxels of the
// rank's whole batch, K found on the device (include/vaeseg.h vs_seg_loss_topk_*).  Validity, f, S / I / T and the Dice term are
// segloss.hip's (segloss.h); the rule of the selection is this library's own:
//
//   key     g_v = (float)(w[l_v] f_v): the fp64 product rounded once, -0.0 made +0.0, ordered through key_enc's integer image (volume.h).  A NaN key (a
//           NaN probability under a focal exponent — with gamma = 0 fmax drops the logarithm's NaN and f is the clamp's 100; the weights are finite) is
//           made the positive quiet NaN, whose image lies above +inf's: such a voxel is among the hardest, and the term it enters is NaN.  An ignored voxel stores the image 0, which only the NaN of all bits set has and no
//           stored key therefore: it is in no count.
//   tau     the K-th largest key, by a radix select of four 8-bit digits from the top.  n_gt = #{g > tau}, n_eq = #{g = tau}.
//   term    ce_term = (A + (K - n_gt) (E / n_eq)) / K,  A = sum_{g > tau} w f,  E = sum_{g = tau} w f  in fp64: the mean of the K largest voxel losses, the
//           places left at the threshold shared equally by every voxel tied there — no tie-break by position.
//
// Forward = seven launches whatever the data:
//   tk_init_kernel        zeroes the four digit tables (the workspace's initial state: no memset)
//   tk_partial_kernel<C>  voxel-major, seg_partial_kernel's walk: label quad and C probability quads read once (16-byte loads), the Dice sums, the key quad
//                         written (16-byte store), the top digit counted
//   tk_count_kernel<1..3> the next digits, over the keys alone (4 bytes per voxel, no second logarithm)
//   tk_sum_kernel         A and E: keys read; label and p_l only where a quad holds a selected voxel, f formed again exactly as the first pass formed it
//   tk_finish_kernel      one workgroup: totals, Dice, the term, final and the record
// Backward = one launch reading p, label, keys and the selection the finish left in the workspace.
//
// A workgroup counts digits in 256 LDS cells and adds its non-zero cells to the table with integer atomics; a run of equal digits along the lanes is ONE
// update of the run's length (quantile.hip's ballot of run heads): a batch whose keys are nearly all 0 does not serialise on one cell.  No kernel waits for
// a "choose" launch between the passes: every wave that needs the selection so far walks the finished tables itself (tk_resolve: 64 lanes x 4 counters, one
// scan per digit), which costs less than a launch.  Counts are integers added by atomics, every fp64 sum is a per-block partial added in a fixed order:
// the same bits eagerly, under graph replay and in both builds.
#include <float.h>
#include <math.h>
#include "segloss.h"
#include "volume.h"

namespace {

constexpr long long TK_MAX_POOL = 1ll << 26;      // batch * voxels: two counts share one fp64 of the record, and the tables are 32-bit
constexpr int TK_COUNT_BLOCKS = 2048;             // block cap of the key-only passes
constexpr double TK_PACK = 67108864.0;            // 2^26: record[3] = n_gt * 2^26 + n_eq

// the workspace, in bytes: four tables of 256 counters; the selection for the backward (the record's four doubles: a caller's record may be reused before
// the backward runs, this copy is the call's own); head + per-block partials of the statistics (segloss.hip's scratch, sized for 8 classes); the per-block
// partials of A and E; the keys
__host__ __device__ inline size_t tk_stat_doubles(int batch) { return (size_t)batch * seg_nstat(SEG_MAXC) * (1 + SEG_BLOCKS); }
__host__ __device__ inline size_t tk_off_sel() { return 4 * 256 * sizeof(unsigned int); }
__host__ __device__ inline size_t tk_off_stats() { return tk_off_sel() + 4 * sizeof(double); }
__host__ __device__ inline size_t tk_off_ae(int batch) { return tk_off_stats() + tk_stat_doubles(batch) * sizeof(double); }
__host__ __device__ inline size_t tk_off_keys(int batch) { return tk_off_ae(batch) + (size_t)2 * batch * SEG_BLOCKS * sizeof(double); }

struct tk_sel {
    unsigned int N, K;          // valid voxels, rank; N == 0: nothing else is set
    unsigned int prefix;        // the digits chosen so far, in place
    unsigned int rank;          // 0-based, from the top, among the keys under the prefix
    unsigned int cnt;           // keys under the prefix (all digits chosen: n_eq)
};

// The selection after NPASS finished tables, by one wave, every lane returning the same.  A lane holds four counters of a table, the highest digits in lane 0:
// the exclusive scan along the lanes is the number of keys above the lane's digits.
template <int NPASS>
__device__ __forceinline__ tk_sel tk_resolve(const unsigned int* __restrict__ tables, double r) {
    const int lane = threadIdx.x & 63;
    tk_sel s = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        const uint4 q = reinterpret_cast<const uint4*>(tables + ps * 256)[63 - lane];
        const unsigned int c0 = q.w, c1 = q.z, c2 = q.y, c3 = q.x;                 // digits 4 (63 - lane) + 3 .. + 0: descending
        const unsigned int sum = c0 + c1 + c2 + c3;
        unsigned int inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int up = (unsigned int)__shfl_up((int)inc, o);
            if (lane >= o) inc += up;
        }
        if (ps == 0) {
            s.N = (unsigned int)__shfl((int)inc, 63);
            if (s.N == 0u) return s;
            const double k = floor(r * (double)s.N);
            s.K = k < 1.0 ? 1u : (unsigned int)k;
            s.rank = s.K - 1u;
        }
        unsigned int exc = inc - sum;
        const u64 reach = __ballot(exc <= s.rank);                                // lane 0 always: the last such lane holds the rank
        const int L = 63 - __clzll((long long)reach);
        unsigned int d = 0u, cd = c0;
        if (s.rank >= exc + c0) {
            exc += c0; d = 1u; cd = c1;
            if (s.rank >= exc + c1) {
                exc += c1; d = 2u; cd = c2;
                if (s.rank >= exc + c2) { exc += c2; d = 3u; cd = c3; }
            }
        }
        const unsigned int digit = 4u * (unsigned int)(63 - L) + 3u - (unsigned int)__shfl((int)d, L);
        s.prefix |= digit << (24 - 8 * ps);
        s.rank -= (unsigned int)__shfl((int)exc, L);
        s.cnt = (unsigned int)__shfl((int)cd, L);
    }
    return s;
}

// one digit of four keys a lane holds into the workgroup's cells: bucket 256 = not counted.  Every lane of the wave calls it.
__device__ __forceinline__ void tk_count4(unsigned int* cells, const unsigned int (&bucket)[4], int lane) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned int below = (unsigned int)__shfl_up((int)bucket[e], 1);
        const bool head = lane == 0 || bucket[e] != below;
        const u64 heads = __ballot(head);
        if (head && bucket[e] < 256u) atomicAdd(&cells[bucket[e]], (unsigned int)run_length(heads, lane));
    }
}

__global__ __launch_bounds__(256) void tk_init_kernel(unsigned int* __restrict__ tables) {
    reinterpret_cast<uint4*>(tables)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

template <int C>
__global__ __launch_bounds__(256) void tk_partial_kernel(const float* __restrict__ p, const float* __restrict__ label, const SegW cw,
                                                         double* __restrict__ part, unsigned int* __restrict__ keys, unsigned int* __restrict__ tables,
                                                         long long voxels, float gamma_f) {
    __shared__ unsigned int cells[256];
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const float* pb = p + (size_t)b * C * voxels;
    const float* lb = label + (size_t)b * voxels;
    unsigned int* kb = keys + (size_t)b * voxels;
    const double gamma = (double)gamma_f;
    double aS[C], aI[C];
    int aT[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { aS[c] = 0.0; aI[c] = 0.0; aT[c] = 0; }
    cells[threadIdx.x] = 0u;
    __syncthreads();
    const long long v4 = voxels / 4;
    // the trip count is the workgroup's, not the thread's: the ballots need every lane
    for (long long i0 = (long long)blockIdx.x * 256; i0 < v4; i0 += (long long)gridDim.x * 256) {
        const long long i = i0 + threadIdx.x;
        const bool live = i < v4;
        const long long at = live ? i : 0;
        f32x4 l4 = *(const f32x4*)(lb + at * 4);
        f32x4 x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = *(const f32x4*)(pb + (size_t)c * voxels + at * 4);
        u32x4 k4;
        unsigned int bucket[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lf = l4[e];
            const bool valid = live && lf >= 0.f && lf < (float)C;
            const int l = valid ? (int)lf : -1;
            float pl = 1.f, wl = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float v = x[c][e];
                const bool hit = l == c;
                aS[c] += valid ? (double)v : 0.0;
                aI[c] += hit ? (double)v : 0.0;
                aT[c] += hit ? 1 : 0;
                pl = hit ? v : pl;
                wl = hit ? cw.w[c] : wl;
            }
            const float g = (float)((double)wl * seg_focal((double)pl, gamma));
            // -0.0 (ln 1 negated) ties with 0.0; every NaN is the one above +inf
            const unsigned int ek = valid ? key_enc(g == 0.f ? 0.f : g != g ? __uint_as_float(0x7fc00000u) : g) : 0u;
            k4[e] = ek;
            bucket[e] = valid ? ek >> 24 : 256u;
        }
        if (live) *(u32x4*)(kb + i * 4) = k4;
        tk_count4(cells, bucket, lane);
    }
    seg_store_partials<C>(aS, aI, aT, 0.0, 0.0, part, b);              // its barrier stands behind every thread's updates of the cells
    const unsigned int c = cells[threadIdx.x];
    if (c) atomicAdd(tables + threadIdx.x, c);
}

// digit PASS (bits [24 - 8 PASS, 32 - 8 PASS)) of the keys under the prefix the tables before it select
template <int PASS>
__global__ __launch_bounds__(256) void tk_count_kernel(const unsigned int* __restrict__ keys, unsigned int* __restrict__ tables, long long quads, double r) {
    __shared__ unsigned int cells[256];
    constexpr int HI = 32 - 8 * PASS;
    const int lane = threadIdx.x & 63;
    const tk_sel s = tk_resolve<PASS>(tables, r);
    if (s.N == 0u) return;                                              // nothing valid: the whole grid leaves
    const unsigned int want = s.prefix >> HI;
    cells[threadIdx.x] = 0u;
    __syncthreads();
    for (long long i0 = (long long)blockIdx.x * 256; i0 < quads; i0 += (long long)gridDim.x * 256) {
        const long long i = i0 + threadIdx.x;
        const bool live = i < quads;
        const u32x4 k4 = *(const u32x4*)(keys + (live ? i : 0) * 4);
        unsigned int bucket[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) bucket[e] = live && k4[e] != 0u && (k4[e] >> HI) == want ? (k4[e] >> (HI - 8)) & 255u : 256u;
        tk_count4(cells, bucket, lane);
    }
    __syncthreads();
    const unsigned int c = cells[threadIdx.x];
    if (c) atomicAdd(tables + PASS * 256 + threadIdx.x, c);
}

// A = sum over g > tau, E = sum over g = tau of w f in fp64, per block; f is formed from p_l again, only where the key selects the voxel
__global__ __launch_bounds__(256) void tk_sum_kernel(const float* __restrict__ p, const float* __restrict__ label, const SegW cw,
                                                     const unsigned int* __restrict__ keys, const unsigned int* __restrict__ tables,
                                                     double* __restrict__ ae, long long voxels, int channels, float gamma_f, double r) {
    const tk_sel s = tk_resolve<4>(tables, r);
    if (s.N == 0u) return;
    const unsigned int tau = s.prefix;
    const int b = blockIdx.y;
    const float* pb = p + (size_t)b * channels * voxels;
    const float* lb = label + (size_t)b * voxels;
    const unsigned int* kb = keys + (size_t)b * voxels;
    const double gamma = (double)gamma_f;
    double A = 0.0, E = 0.0;
    const long long v4 = voxels / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
        const u32x4 k4 = *(const u32x4*)(kb + i * 4);
        if (k4[0] < tau && k4[1] < tau && k4[2] < tau && k4[3] < tau) continue;               // an ignored voxel's 0 is below every tau
        const f32x4 l4 = *(const f32x4*)(lb + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (k4[e] < tau) continue;
            const int l = (int)l4[e];                                   // selected, hence valid
            float wl = 0.f;
#pragma unroll
            for (int c = 0; c < SEG_MAXC; ++c) wl = l == c ? cw.w[c] : wl;
            const double wf = (double)wl * seg_focal((double)pb[(size_t)l * voxels + i * 4 + e], gamma);
            A += k4[e] > tau ? wf : 0.0;
            E += k4[e] > tau ? 0.0 : wf;
        }
    }
    __shared__ double red[4][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    A = wave_sum_d(A);
    E = wave_sum_d(E);
    if (lane == 0) { red[wave][0] = A; red[wave][1] = E; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int q = threadIdx.x;
        ae[((size_t)q * gridDim.y + b) * gridDim.x + blockIdx.x] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

__global__ __launch_bounds__(256) void tk_finish_kernel(const double* __restrict__ part, double* __restrict__ head, const double* __restrict__ ae,
                                                        const unsigned int* __restrict__ tables, float* __restrict__ terms, float* __restrict__ final_out,
                                                        double* __restrict__ sel, double* __restrict__ record, int batch, int channels, int bot, int top, int nblk, float eps,
                                                        float dice_w, float ce_w, int batch_dice, double r) {
    __shared__ double s_tot[SEG_MAXB * (3 * SEG_MAXC + 2)];
    __shared__ double s_ae[2][256];
    const double dice = seg_totals_dice(part, head, s_tot, batch, channels, bot, top, nblk, eps, batch_dice);
    const tk_sel s = tk_resolve<4>(tables, r);
    // every 256th partial per thread, then the 256 in order: both orders are fixed
    double a = 0.0, e = 0.0;
    if (s.N != 0u) {
        const int n = batch * nblk;
        for (int i = threadIdx.x; i < n; i += 256) { a += ae[i]; e += ae[n + i]; }
    }
    s_ae[0][threadIdx.x] = a;
    s_ae[1][threadIdx.x] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        double A = 0.0, E = 0.0, ce = 0.0, tau = 0.0, n_gt = 0.0;
        for (int i = 0; i < 256; ++i) { A += s_ae[0][i]; E += s_ae[1][i]; }
        if (s.N != 0u) {
            n_gt = (double)(s.K - 1u - s.rank);
            tau = (double)key_dec(s.prefix);
            ce = (A + ((double)s.K - n_gt) * (E / (double)s.cnt)) / (double)s.K;
        }
        const float dterm = (float)(1.0 - dice), cterm = (float)ce;
        terms[0] = dterm;
        terms[1] = cterm;
        final_out[0] = __fadd_rn(__fmul_rn(dice_w, dterm), __fmul_rn(ce_w, cterm));
        const double rec[4] = {(double)s.N, (double)s.K, tau, n_gt * TK_PACK + (double)s.cnt};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sel[i] = rec[i];
            if (record) record[i] = rec[i];
        }
    }
}

// seg_bwd_kernel with the cross-entropy part weighted per voxel: kc / K above tau, kc (K - n_gt) / (n_eq K) at tau, nothing below
template <int C>
__global__ __launch_bounds__(256) void tk_bwd_kernel(const float* __restrict__ p, const float* __restrict__ label, const SegW cw,
                                                     const double* __restrict__ head, const unsigned int* __restrict__ keys,
                                                     const double* __restrict__ sel, const float* __restrict__ gout, float* __restrict__ gp, int batch,
                                                     long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma_f) {
    const int b = blockIdx.y;
    const double g = (double)gout[0], gamma = (double)gamma_f;
    const double kd = g * (double)dice_w / (batch_dice ? (double)(top - bot) : (double)batch * (double)(top - bot));
    double a1[C], a2[C];              // the gradient of a valid voxel in channel c: a2[c], plus a1[c] where l == c
    seg_dice_coeffs<C>(head, b, batch, bot, top, eps, kd, batch_dice, a1, a2);
    const double K = sel[1], n_gt = floor(sel[3] / TK_PACK), n_eq = sel[3] - n_gt * TK_PACK;
    const double k_gt = K > 0.0 ? g * (double)ce_w / K : 0.0;
    const double k_eq = K > 0.0 ? g * (double)ce_w * ((K - n_gt) / n_eq) / K : 0.0;
    const bool with_ce = k_gt != 0.0;
    const unsigned int tau = key_enc((float)sel[2]);

    const float* pb = p + (size_t)b * C * voxels;
    const float* lb = label + (size_t)b * voxels;
    const unsigned int* kb = keys + (size_t)b * voxels;
    float* gb = gp + (size_t)b * C * voxels;
    const long long v4 = voxels / 4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v4; i += (long long)gridDim.x * 256) {
        const f32x4 l4 = *(const f32x4*)(lb + i * 4);
        const u32x4 k4 = *(const u32x4*)(kb + i * 4);
        f32x4 x[C], o[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = *(const f32x4*)(pb + (size_t)c * voxels + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float lf = l4[e];
            const bool valid = lf >= 0.f && lf < (float)C;
            const int l = valid ? (int)lf : -1;
            const bool sel = k4[e] >= tau;                // an ignored voxel's key is 0, below every tau
            double hit = 0.0;                             // what the voxel's own channel gets on top of a2
            float pl = 0.5f, wl = 0.f;                    // not selected, ignored or a class of weight 0: no cross-entropy part, whatever p_l is
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool own = l == c;
                hit = own ? a1[c] : hit;
                pl = own && sel && cw.w[c] != 0.f ? x[c][e] : pl;
                wl = own && sel ? cw.w[c] : wl;
            }
            if (with_ce) hit += (k4[e] > tau ? k_gt : k_eq) * (double)wl * seg_focal_grad((double)pl, gamma);
#pragma unroll
            for (int c = 0; c < C; ++c) o[c][e] = valid ? (float)(l == c ? a2[c] + hit : a2[c]) : 0.f;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) *(f32x4*)(gb + (size_t)c * voxels + i * 4) = o[c];
    }
}

int tk_args(const float* p, const float* label, const float* class_w, const void* workspace, const double* record, int batch, int channels, long long voxels,
            int bot, int top, float eps, float dice_w, float ce_w, float gamma, double r, SegW& cw) {
    const int rc = seg_args(p, label, class_w, workspace, batch, channels, voxels, bot, top, eps, dice_w, ce_w, gamma, cw);
    if (rc) return rc;
    if (!(r > 0.0 && r <= 1.0)) return VS_EINVAL;                        // NaN fails both
    for (int c = 0; c < channels; ++c)
        if (!(cw.w[c] <= FLT_MAX)) return VS_EINVAL;                     // an infinite weight times f = 0 would be a NaN key
    if ((long long)batch * voxels >= TK_MAX_POOL) return VS_ESHAPE;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)record & 7)) return VS_EALIGN;
    return VS_OK;
}

template <int C>
void tk_launch_partial(dim3 grid, hipStream_t st, const float* p, const float* label, const SegW& cw, double* part, unsigned int* keys, unsigned int* tables,
                       long long voxels, float gamma) {
    hipLaunchKernelGGL(tk_partial_kernel<C>, grid, dim3(256), 0, st, p, label, cw, part, keys, tables, voxels, gamma);
}
template <int C>
void tk_launch_bwd(dim3 grid, hipStream_t st, const float* p, const float* label, const SegW& cw, const double* head, const unsigned int* keys,
                   const double* sel, const float* gout, float* gp, int batch, long long voxels, int bot, int top, float eps, float dice_w, float ce_w,
                   int batch_dice, float gamma) {
    hipLaunchKernelGGL(tk_bwd_kernel<C>, grid, dim3(256), 0, st, p, label, cw, head, keys, sel, gout, gp, batch, voxels, bot, top, eps, dice_w, ce_w,
                       batch_dice, gamma);
}

}  // namespace

extern "C" size_t vs_seg_topk_workspace_bytes(int batch, long long voxels) {
    if (batch <= 0 || batch > SEG_MAXB || voxels <= 0 || (long long)batch * voxels >= TK_MAX_POOL) return 0;
    return tk_off_keys(batch) + (size_t)batch * (size_t)voxels * sizeof(unsigned int);
}

extern "C" int vs_seg_loss_topk_fwd(const float* p, const float* label, const float* class_w, void* workspace, double* record, float* terms,
                                    float* final_out, int batch, int channels, long long voxels, int bot, int top, float eps, float dice_w, float ce_w,
                                    int batch_dice, float gamma, double r, void* stream) {
    SegW cw;
    const int rc = tk_args(p, label, class_w, workspace, record, batch, channels, voxels, bot, top, eps, dice_w, ce_w, gamma, r, cw);
    if (rc) return rc;
    if (!terms || !final_out) return VS_EINVAL;
    char* ws = (char*)workspace;
    unsigned int* tables = (unsigned int*)ws;
    double* sel = (double*)(ws + tk_off_sel());
    double* head = (double*)(ws + tk_off_stats());
    double* part = head + (size_t)batch * seg_nstat(channels);
    double* ae = (double*)(ws + tk_off_ae(batch));
    unsigned int* keys = (unsigned int*)(ws + tk_off_keys(batch));
    const unsigned blocks = seg_blocks(voxels);
    const long long quads = (long long)batch * voxels / 4;
    const long long cb = (quads + 255) / 256;
    const dim3 grid(blocks, batch), wg(256), cgrid((unsigned)(cb > TK_COUNT_BLOCKS ? TK_COUNT_BLOCKS : cb));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tk_init_kernel, dim3(1), wg, 0, st, tables);
    VS_CHECK_LAUNCH();
#define TK_CALL(CC) tk_launch_partial<CC>(grid, st, p, label, cw, part, keys, tables, voxels, gamma)
    SEG_DISPATCH_C(channels, TK_CALL)
#undef TK_CALL
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tk_count_kernel<1>, cgrid, wg, 0, st, keys, tables, quads, r);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tk_count_kernel<2>, cgrid, wg, 0, st, keys, tables, quads, r);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tk_count_kernel<3>, cgrid, wg, 0, st, keys, tables, quads, r);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tk_sum_kernel, grid, wg, 0, st, p, label, cw, keys, tables, ae, voxels, channels, gamma, r);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tk_finish_kernel, dim3(1), wg, 0, st, part, head, ae, tables, terms, final_out, sel, record, batch, channels, bot, top, (int)blocks, eps,
                       dice_w, ce_w, batch_dice ? 1 : 0, r);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_seg_loss_topk_bwd(const float* p, const float* label, const float* class_w, const void* workspace, const float* gout, float* gp, int batch, int channels, long long voxels, int bot, int top, float eps, float dice_w,
                                    float ce_w, int batch_dice, float gamma, double r, void* stream) {
    SegW cw;
    const int rc = tk_args(p, label, class_w, workspace, nullptr, batch, channels, voxels, bot, top, eps, dice_w, ce_w, gamma, r, cw);
    if (rc) return rc;
    if (!gout || !gp) return VS_EINVAL;
    if ((uintptr_t)gp & 15) return VS_EALIGN;
    const char* ws = (const char*)workspace;
    const double* sel = (const double*)(ws + tk_off_sel());
    const double* head = (const double*)(ws + tk_off_stats());
    const unsigned int* keys = (const unsigned int*)(ws + tk_off_keys(batch));
    const dim3 grid(seg_blocks(voxels), batch);
    hipStream_t st = (hipStream_t)stream;
    const int bd = batch_dice ? 1 : 0;
#define TK_CALL(CC) tk_launch_bwd<CC>(grid, st, p, label, cw, head, keys, sel, gout, gp, batch, voxels, bot, top, eps, dice_w, ce_w, bd, gamma)
    SEG_DISPATCH_C(channels, TK_CALL)
#undef TK_CALL
    VS_CHECK_LAUNCH();
    return VS_OK;
}
