// Sliding-window prediction of a whole volume (include/vaeseg.h: vs_sw_plan, vs_sw_gather, vs_sw_accumulate, vs_sw_finalize, and the mirror
// test-time augmentation of the middle two, vs_sw_gather_tta, vs_sw_accumulate_tta).
//
// The reference has no counterpart (utils/utils.py:predict_vol is a 2D slice loop); this is the standard scheme for fully convolutional 3D
// networks: tile the volume (C, D, H, W) with overlapping cubic patches of side P, run the network on batches of B windows, blend the window
// probabilities with a separable importance map, normalise.
//
//   plan        host, pure C: per axis step = max(1, floor(P (1 - overlap))), n = 1 if S <= P else ceil((S - P) / step) + 1 windows, the origin of
//               window i is min(i step, max(S - P, 0)); the table lists the windows D-major, then H, then W
//   gather      windows [first, first + B) -> a (B, C, P, P, P) batch.  `first` is a DEVICE word, so one captured launch serves every batch.  A
//               thread owns four consecutive x of one batch row: a 16-byte store, a 16-byte load where the source quad happens to be aligned
//               (window origins are not multiples of 4), guarded scalar loads otherwise.  Slots past the plan and positions past the volume
//               (S < P) read cval.
//   accumulate  acc[k][v] += w prob[b][k][v - origin], wsum[v] += w.  No atomics: a thread is (slot b, row of the window, quad of four x
//               aligned in the VOLUME's row) and updates a voxel only when no earlier slot of the batch covers it; it then adds the terms of
//               every slot from b on that covers the voxel, in ascending slot order.  So every voxel has exactly one writer per launch and
//               receives its terms in ascending window index, whatever B is: the sums are bit-identical for every batch size, from run to run
//               and between the two builds.  Whole quads move as 16-byte accesses when the row is aligned; the head and tail of a window's x
//               range, and everything in a misaligned row, go element by element.
//   finalize    prob = acc / wsum (IEEE fp32 division), optionally the uint8 argmax (ties: the first maximal channel; a NaN channel wins, as
//               vs_hard_onehot) and its planar one-hot, four voxels of the flat volume per thread.
//
//   tta         mirror test-time augmentation: a flip is a 3-bit code (bit 0 mirrors x, bit 1 y, bit 2 z), a pass has nf distinct codes, and the
//               device word `first` counts ITEMS: item j is window j / nf under flip codes[j % nf].  The codes travel by value, three bits each in
//               one word.  gather writes the window already mirrored (the whole padded cube: cval lands at the low end), accumulate reads the
//               network's answer mirrored back and takes the weight at the un-mirrored position.  Both are the kernels above instantiated with
//               FLIP = true; FLIP = false compiles the item arithmetic and every mirror away.  Slots of one batch may now share an origin: the
//               first of them covers every voxel of the later ones, so it stays the only writer and adds them in ascending item order.
//
// Every term is fmaf(w, p, sum) with w = (wz[lz] * wy[ly]) * wx[lx] rounded to fp32 after each product; wsum takes fmaf(w, 1, sum) = sum + w.
// All four are bandwidth-bound: no LDS, offsets are 64-bit wherever K D H W or B C P^3 can pass 2^31.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include "common.h"

namespace {

struct sw_dims {
    int c, d, h, w, p;
    int nw, b;
};

// the flips of a TTA pass, by value: nf codes of three bits each, code i in bits [3 i, 3 i + 3) of `codes`
struct sw_flips {
    int nf;
    unsigned codes;
};

constexpr long long SW_GRID_CAP = 1 << 20;

unsigned sw_grid(long long threads) {
    const long long blocks = (threads + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > SW_GRID_CAP ? SW_GRID_CAP : blocks));
}

bool sw_dims_ok(int d, int h, int w) { return d > 0 && h > 0 && w > 0 && (double)d * h * w < 2147483648.0; }      // data.hip's dp_dims_ok
bool sw_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

__device__ __forceinline__ bool sw_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the origin of plan entry `win`, or false for a slot outside the plan or an entry that is no origin of this volume (nothing is then read or written)
__device__ __forceinline__ bool sw_window(const int* __restrict__ origins, int win, const sw_dims& g, int& oz, int& oy, int& ox) {
    if (win < 0 || win >= g.nw) return false;
    oz = origins[3 * (size_t)win];
    oy = origins[3 * (size_t)win + 1];
    ox = origins[3 * (size_t)win + 2];
    const int mz = g.d > g.p ? g.d - g.p : 0, my = g.h > g.p ? g.h - g.p : 0, mx = g.w > g.p ? g.w - g.p : 0;
    return oz >= 0 && oz <= mz && oy >= 0 && oy <= my && ox >= 0 && ox <= mx;
}

// item -> (window, flip code); false for an item before the first.  Without FLIP an item is a window and the code is 0.
template <bool FLIP>
__device__ __forceinline__ bool sw_item(int item, const sw_flips& f, int& win, int& code) {
    win = item;
    code = 0;
    if (FLIP) {
        if (item < 0) return false;
        win = item / f.nf;
        code = (int)((f.codes >> (3 * (item - win * f.nf))) & 7u);
    }
    return true;
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------------------
template <bool FLIP>
__global__ __launch_bounds__(256) void sw_gather_kernel(const float* __restrict__ vol, float* __restrict__ batch, const int* __restrict__ origins,
                                                        const int* __restrict__ firstp, sw_dims g, float cval, int nq, long long total, sw_flips f) {
    const int first = firstp[0];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % nq);
        long long r = i / nq;
        const int ly = (int)(r % g.p);
        r /= g.p;
        const int lz = (int)(r % g.p);
        r /= g.p;
        const int c = (int)(r % g.c), b = (int)(r / g.c);
        const int lx = 4 * q, n = g.p - lx < 4 ? g.p - lx : 4;
        float v[4] = {cval, cval, cval, cval};
        int oz, oy, ox, win, code;
        if (sw_item<FLIP>(first + b, f, win, code) && sw_window(origins, win, g, oz, oy, ox)) {
            const bool mx = FLIP && (code & 1);                  // a mirrored x: the four outputs are the source quad [P - 4 - lx, P - lx) in reverse
            const int z = oz + (FLIP && (code & 4) ? g.p - 1 - lz : lz), y = oy + (FLIP && (code & 2) ? g.p - 1 - ly : ly);
            const int x = ox + (mx ? g.p - 4 - lx : lx);         // n < 4 with mx: x may lie left of the window, the guarded loads skip those
            if (z < g.d && y < g.h) {
                const float* sp = vol + (((size_t)c * g.d + z) * g.h + y) * g.w;
                sp += x;
                if (n == 4 && x + 4 <= g.w && sw_aligned16(sp)) {
                    const float4 t = *reinterpret_cast<const float4*>(sp);
                    if (mx) {
                        v[0] = t.w; v[1] = t.z; v[2] = t.y; v[3] = t.x;
                    } else {
                        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int se = mx ? 3 - e : e;           // the source element of output e
                        if (e < n && x + se < g.w) v[e] = sp[se];
                    }
                }
            }
        }
        float* dp = batch + ((((size_t)b * g.c + c) * g.p + lz) * g.p + ly) * g.p + lx;
        if (n == 4 && sw_aligned16(dp)) {
            *reinterpret_cast<float4*>(dp) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) dp[e] = v[e];
        }
    }
}

// ---- accumulate -----------------------------------------------------------------------------------------------------------------------------
template <bool FLIP>
__global__ __launch_bounds__(256) void sw_accumulate_kernel(const float* __restrict__ prob, float* __restrict__ acc, float* __restrict__ wsum,
                                                            const int* __restrict__ origins, const int* __restrict__ firstp, sw_dims g, int nk,
                                                            const float* __restrict__ wz, const float* __restrict__ wy, const float* __restrict__ wx,
                                                            int nq, long long total, sw_flips f) {
    const int first = firstp[0];
    const size_t V = (size_t)g.d * g.h * g.w, PV = (size_t)g.p * g.p * g.p;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int q = (int)(i % nq);
        long long r = i / nq;
        const int ly = (int)(r % g.p);
        r /= g.p;
        const int lz = (int)(r % g.p), b = (int)(r / g.p);
        int oz, oy, ox, win, code;
        if (!sw_item<FLIP>(first + b, f, win, code) || !sw_window(origins, win, g, oz, oy, ox)) continue;
        const int z = oz + lz, y = oy + ly;
        if (z >= g.d || y >= g.h) continue;
        const int x0 = (ox & ~3) + 4 * q;                       // a quad aligned in the volume's row
        unsigned mine = 0;                                       // elements of the quad inside this window and the volume ...
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x0 + e >= ox && x0 + e < ox + g.p && x0 + e < g.w) mine |= 1u << e;
        for (int b2 = 0; b2 < b && mine; ++b2) {                 // ... that no earlier slot of the batch covers: this thread is their only writer
            int pz, py, px, w2, c2;
            if (!sw_item<FLIP>(first + b2, f, w2, c2) || !sw_window(origins, w2, g, pz, py, px)) continue;
            if (z < pz || z >= pz + g.p || y < py || y >= py + g.p) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x0 + e >= px && x0 + e < px + g.p) mine &= ~(1u << e);
        }
        if (!mine) continue;
        // the terms of the slots from b on, in ascending order: weight and offset into prob per element (weight stays 0 where a slot does not cover it)
        const size_t vrow = ((size_t)z * g.h + y) * g.w + x0;
        for (int k = 0; k <= nk; ++k) {                          // k == nk: the weight sum
            float* plane = k < nk ? acc + (size_t)k * V + vrow : wsum + vrow;
            const bool whole = mine == 0xFu && sw_aligned16(plane);
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            if (whole) {
                const float4 t = *reinterpret_cast<const float4*>(plane);
                s[0] = t.x; s[1] = t.y; s[2] = t.z; s[3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (mine & (1u << e)) s[e] = plane[e];
            }
            for (int b2 = b; b2 < g.b; ++b2) {
                int pz = oz, py = oy, px = ox, c2 = code;
                if (b2 != b) {
                    int w2;
                    if (!sw_item<FLIP>(first + b2, f, w2, c2) || !sw_window(origins, w2, g, pz, py, px)) continue;
                    if (z < pz || z >= pz + g.p || y < py || y >= py + g.p) continue;
                }
                const float wzy = wz[z - pz] * wy[y - py];               // the weight belongs to the voxel's own position, the probability to its mirror image
                const int sz = FLIP && (c2 & 4) ? g.p - 1 - (z - pz) : z - pz, sy = FLIP && (c2 & 2) ? g.p - 1 - (y - py) : y - py;
                const float* pp = prob + ((((size_t)b2 * nk + (k < nk ? k : 0)) * g.p + sz) * g.p + sy) * g.p;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int lx = x0 + e - px;
                    if ((mine & (1u << e)) && lx >= 0 && lx < g.p) {
                        const float w = wzy * wx[lx];
                        s[e] = fmaf(w, k < nk ? pp[FLIP && (c2 & 1) ? g.p - 1 - lx : lx] : 1.f, s[e]);
                    }
                }
            }
            if (whole) {
                *reinterpret_cast<float4*>(plane) = make_float4(s[0], s[1], s[2], s[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (mine & (1u << e)) plane[e] = s[e];
            }
        }
    }
}

// ---- finalize -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sw_finalize_kernel(const float* acc, const float* __restrict__ wsum, float* prob, unsigned char* __restrict__ label,
                                                          float* __restrict__ onehot, int nk, long long V, long long nquads, int vec) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nquads; i += (long long)gridDim.x * blockDim.x) {
        const long long v0 = 4 * i;
        const int n = V - v0 < 4 ? (int)(V - v0) : 4;
        const bool whole = vec && n == 4;                        // vec: every plane base and V are multiples of 16 bytes
        float ws[4] = {1.f, 1.f, 1.f, 1.f}, best[4];
        int arg[4] = {0, 0, 0, 0};
        if (whole) {
            const float4 t = *reinterpret_cast<const float4*>(wsum + v0);
            ws[0] = t.x; ws[1] = t.y; ws[2] = t.z; ws[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) ws[e] = wsum[v0 + e];
        }
        for (int k = 0; k < nk; ++k) {
            const size_t off = (size_t)k * V + v0;
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (whole) {
                const float4 t = *reinterpret_cast<const float4*>(acc + off);
                a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) a[e] = acc[off + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = a[e] / ws[e];
                if (k == 0) {
                    best[e] = a[e];
                } else if (a[e] > best[e] || (a[e] != a[e] && best[e] == best[e])) {
                    best[e] = a[e];
                    arg[e] = k;
                }
            }
            if (whole) {
                *reinterpret_cast<float4*>(prob + off) = make_float4(a[0], a[1], a[2], a[3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) prob[off + e] = a[e];
            }
        }
        if (label) {
            if (whole) {
                *reinterpret_cast<unsigned int*>(label + v0) = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) label[v0 + e] = (unsigned char)arg[e];
            }
        }
        if (onehot) {
            for (int k = 0; k < nk; ++k) {
                const size_t off = (size_t)k * V + v0;
                if (whole) {
                    *reinterpret_cast<float4*>(onehot + off) = make_float4(arg[0] == k ? 1.f : 0.f, arg[1] == k ? 1.f : 0.f, arg[2] == k ? 1.f : 0.f, arg[3] == k ? 1.f : 0.f);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < n) onehot[off + e] = arg[e] == k ? 1.f : 0.f;
                }
            }
        }
    }
}

int sw_axis_plan(int s, int p, int step, int* n) {
    *n = s <= p ? 1 : (s - p + step - 1) / step + 1;
    return s > p ? s - p : 0;
}

int sw_check(const sw_dims& g) {
    if (g.c <= 0 || g.p <= 0 || g.nw <= 0 || g.b <= 0) return VS_EINVAL;
    if (!sw_dims_ok(g.d, g.h, g.w) || !sw_dims_ok(g.p, g.p, g.p)) return VS_ESHAPE;
    return VS_OK;
}

// 1 <= nf <= 8 distinct codes, nothing set above them, and first[0] + b stays an int for every item of the pass
int sw_flips_check(const sw_dims& g, const sw_flips& f) {
    if (f.nf < 1 || f.nf > 8 || (f.nf < 8 && (f.codes >> (3 * f.nf)) != 0)) return VS_EINVAL;
    unsigned seen = 0;
    for (int i = 0; i < f.nf; ++i) {
        const unsigned bit = 1u << ((f.codes >> (3 * i)) & 7u);
        if (seen & bit) return VS_EINVAL;
        seen |= bit;
    }
    if ((long long)g.nw * f.nf + g.b > INT_MAX) return VS_ESHAPE;
    return VS_OK;
}

}  // namespace

extern "C" int vs_sw_plan(int d, int h, int w, int patch, double overlap, int* origins, int capacity) {
    if (!sw_dims_ok(d, h, w) || patch <= 0 || !(overlap >= 0.0) || !(overlap < 1.0)) return VS_EINVAL;
    const double fs = floor((double)patch * (1.0 - overlap));
    const int step = fs < 1.0 ? 1 : (int)fs;
    int nz, ny, nx;
    const int mz = sw_axis_plan(d, patch, step, &nz), my = sw_axis_plan(h, patch, step, &ny), mx = sw_axis_plan(w, patch, step, &nx);
    const long long nw = (long long)nz * ny * nx;
    if (nw > INT_MAX / 3) return VS_ESHAPE;
    if (!origins) return (int)nw;
    if (capacity < nw) return VS_EWORKSPACE;
    int* o = origins;
    for (int iz = 0; iz < nz; ++iz)
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix) {
                const long long tz = (long long)iz * step, ty = (long long)iy * step, tx = (long long)ix * step;
                *o++ = (int)(tz < mz ? tz : mz);
                *o++ = (int)(ty < my ? ty : my);
                *o++ = (int)(tx < mx ? tx : mx);
            }
    return (int)nw;
}

extern "C" int vs_sw_gather(const float* volume, float* batch, const int* origins, const int* first, int nw, int b, int c, int d, int h, int w, int patch,
                            float cval, void* stream) {
    const sw_dims g = {c, d, h, w, patch, nw, b};
    const int rc = sw_check(g);
    if (rc != VS_OK) return rc;
    if (!volume || !batch || !origins || !first || volume == batch) return VS_EINVAL;
    if (sw_misaligned(volume) || sw_misaligned(batch)) return VS_EALIGN;
    const int nq = (patch + 3) / 4;
    const long long total = (long long)b * c * patch * patch * nq;
    hipLaunchKernelGGL(sw_gather_kernel<false>, dim3(sw_grid(total)), dim3(256), 0, (hipStream_t)stream, volume, batch, origins, first, g, cval, nq, total,
                       sw_flips{1, 0u});
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_sw_gather_tta(const float* volume, float* batch, const int* origins, const int* first, int nw, int b, int c, int d, int h, int w, int patch,
                                float cval, int nf, int codes, void* stream) {
    const sw_dims g = {c, d, h, w, patch, nw, b};
    const sw_flips f = {nf, (unsigned)codes};
    int rc = sw_check(g);
    if (rc == VS_OK) rc = sw_flips_check(g, f);
    if (rc != VS_OK) return rc;
    if (!volume || !batch || !origins || !first || volume == batch) return VS_EINVAL;
    if (sw_misaligned(volume) || sw_misaligned(batch)) return VS_EALIGN;
    const int nq = (patch + 3) / 4;
    const long long total = (long long)b * c * patch * patch * nq;
    hipLaunchKernelGGL(sw_gather_kernel<true>, dim3(sw_grid(total)), dim3(256), 0, (hipStream_t)stream, volume, batch, origins, first, g, cval, nq, total, f);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_sw_accumulate(const float* prob, float* acc, float* wsum, const int* origins, const int* first, int nw, int b, int k, int d, int h, int w,
                                int patch, const float* wz, const float* wy, const float* wx, void* stream) {
    const sw_dims g = {1, d, h, w, patch, nw, b};
    const int rc = sw_check(g);
    if (rc != VS_OK) return rc;
    if (k <= 0) return VS_EINVAL;
    if (!prob || !acc || !wsum || !origins || !first || !wz || !wy || !wx || prob == acc || prob == wsum || acc == wsum) return VS_EINVAL;
    if (sw_misaligned(prob) || sw_misaligned(acc) || sw_misaligned(wsum)) return VS_EALIGN;
    const int nq = (patch + 3) / 4 + 1;                          // the volume-aligned quads that [ox, ox + P) can touch
    const long long total = (long long)b * patch * patch * nq;
    hipLaunchKernelGGL(sw_accumulate_kernel<false>, dim3(sw_grid(total)), dim3(256), 0, (hipStream_t)stream, prob, acc, wsum, origins, first, g, k, wz, wy, wx,
                       nq, total, sw_flips{1, 0u});
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_sw_accumulate_tta(const float* prob, float* acc, float* wsum, const int* origins, const int* first, int nw, int b, int k, int d, int h,
                                    int w, int patch, const float* wz, const float* wy, const float* wx, int nf, int codes, void* stream) {
    const sw_dims g = {1, d, h, w, patch, nw, b};
    const sw_flips f = {nf, (unsigned)codes};
    int rc = sw_check(g);
    if (rc == VS_OK) rc = sw_flips_check(g, f);
    if (rc != VS_OK) return rc;
    if (k <= 0) return VS_EINVAL;
    if (!prob || !acc || !wsum || !origins || !first || !wz || !wy || !wx || prob == acc || prob == wsum || acc == wsum) return VS_EINVAL;
    if (sw_misaligned(prob) || sw_misaligned(acc) || sw_misaligned(wsum)) return VS_EALIGN;
    const int nq = (patch + 3) / 4 + 1;
    const long long total = (long long)b * patch * patch * nq;
    hipLaunchKernelGGL(sw_accumulate_kernel<true>, dim3(sw_grid(total)), dim3(256), 0, (hipStream_t)stream, prob, acc, wsum, origins, first, g, k, wz, wy, wx,
                       nq, total, f);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_sw_finalize(const float* acc, const float* wsum, float* prob, unsigned char* label, float* onehot, int k, int d, int h, int w, void* stream) {
    if (!sw_dims_ok(d, h, w)) return VS_ESHAPE;
    if (k <= 0 || k > 255) return VS_EINVAL;                     // the label is a byte
    if (!acc || !wsum || !prob || (const void*)onehot == (const void*)acc || (const void*)onehot == (const void*)prob) return VS_EINVAL;
    if (sw_misaligned(acc) || sw_misaligned(wsum) || sw_misaligned(prob) || sw_misaligned(label) || sw_misaligned(onehot)) return VS_EALIGN;
    const long long V = (long long)d * h * w, nquads = (V + 3) / 4;
    hipLaunchKernelGGL(sw_finalize_kernel, dim3(sw_grid(nquads)), dim3(256), 0, (hipStream_t)stream, acc, wsum, prob, label, onehot, k, V, nquads,
                       (int)(V % 4 == 0));
    VS_CHECK_LAUNCH();
    return VS_OK;
}
