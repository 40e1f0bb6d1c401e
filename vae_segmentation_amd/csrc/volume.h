// Pieces the volume utility kernels share.  Included inside each translation unit: everything here has internal linkage.
//   runs       regions.hip and hist.hip walk 64-voxel segments run by run: the 64-bit integer atomic add, the bit scan and a run's length from the ballot of heads
//   keys       hist.hip and quantile.hip order fp32 values through an unsigned integer image of their bits
//   resample   scan.hip and uncrop.hip map a (K, D, H, W) probability volume onto another grid, four consecutive x per thread: the two source indices and the
//              weight of an axis, the trilinear blend in fp64
#pragma once
#include "common.h"

namespace {

typedef long long i64;
typedef unsigned long long u64;

__device__ __forceinline__ void run_add(i64* p, i64 v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }
__device__ __forceinline__ int run_ctz(u64 m) { return __ffsll((long long)m) - 1; }      // m != 0

// length of the run that starts at `lane`, from the ballot of the lanes whose key differs from the lane below (bit 0 always set)
__device__ __forceinline__ int run_length(u64 heads, int lane) {
    const u64 above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    return (above ? run_ctz(above) : 64) - lane;
}

// fp32 bits <-> an unsigned integer with the same order as the values (finite values never map to 0 or 0xffffffff)
__device__ __forceinline__ unsigned int key_enc(float f) {
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_dec(unsigned int e) { return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e); }
__device__ __forceinline__ bool key_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

struct rs_axis {
    int i0, i1;      // the two source indices (nearest: both the same)
    double t;        // the weight of i1
};

// source coordinate q along an axis of n rows -> indices and weight.  linear: q clamped to [0, n - 1]; nearest: floor(q + 0.5), clamped, a.t left as it is
template <int LINEAR>
__device__ __forceinline__ void rs_axis_at(double q, int n, rs_axis& a) {
    if (LINEAR) {
        const double c = fmin(fmax(q, 0.0), (double)(n - 1));
        const int i = (int)floor(c);
        a.i0 = i;
        a.i1 = i + 1 < n ? i + 1 : n - 1;
        a.t = c - (double)i;
    } else {
        const double r = fmin(fmax(floor(q + 0.5), 0.0), (double)(n - 1));
        a.i0 = a.i1 = (int)r;
    }
}

// the four source rows (offsets into a plane of rows of `w` elements, `h` rows per slice) a thread reads for its (z, y) and their weights
struct rs_rows {
    size_t r00, r01, r10, r11;
    double w00, w01, w10, w11;
    __device__ __forceinline__ rs_rows(const rs_axis& az, const rs_axis& ay, int h, int w)
        : r00(((size_t)az.i0 * h + ay.i0) * w), r01(((size_t)az.i0 * h + ay.i1) * w), r10(((size_t)az.i1 * h + ay.i0) * w), r11(((size_t)az.i1 * h + ay.i1) * w),
          w00((1.0 - az.t) * (1.0 - ay.t)), w01((1.0 - az.t) * ay.t), w10(az.t * (1.0 - ay.t)), w11(az.t * ay.t) {}
    // one class at column ax: trilinear (the four rows blended for each of the two x columns, the columns weighted by x, in fp64, rounded once) or the nearest sample
    template <int LINEAR>
    __device__ __forceinline__ float sample(const float* plane, const rs_axis& ax) const {
        if (LINEAR) {
            const int xa = ax.i0, xb = ax.i1;
            const double ta = 1.0 - ax.t, tb = ax.t;
            const double sa = w00 * (double)plane[r00 + xa] + w01 * (double)plane[r01 + xa] + w10 * (double)plane[r10 + xa] + w11 * (double)plane[r11 + xa];
            const double sb = w00 * (double)plane[r00 + xb] + w01 * (double)plane[r01 + xb] + w10 * (double)plane[r10 + xb] + w11 * (double)plane[r11 + xb];
            return (float)(ta * sa + tb * sb);
        }
        return plane[r00 + ax.i0];
    }
};

}  // namespace
