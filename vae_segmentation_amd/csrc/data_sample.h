// The sampler of scipy.ndimage.map_coordinates(mode='constant') as augment_spatial uses it, shared by the affine resampling of data.hip and the
// displacement-field resampling of elastic.hip: one body, so both give the same bits for the same input coordinate.
#pragma once
#include "common.h"

__device__ __forceinline__ int dp_mirror(int i, int n) {       // scipy 'mirror': d c b | a b c d | c b a
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i = i < 0 ? -i : i;
    i %= p;
    return i >= n ? p - i : i;
}

// input coordinate of output voxel o = A (o - (P - 1) / 2 [+ displacement]) + ctr (augment_spatial: A = scale * R^T)
struct DpAffine { double a[9]; double ctr[3]; int sd, sh, sw, pd, ph, pw; };
__device__ __forceinline__ void dp_cubic_w(double t, double (&w)[4]) {
    w[0] = (1 - t) * (1 - t) * (1 - t) / 6.0;
    w[1] = (3 * t * t * t - 6 * t * t + 4) / 6.0;
    w[2] = (-3 * t * t * t + 3 * t * t + 3 * t + 1) / 6.0;
    w[3] = t * t * t / 6.0;
}
// the zero-centred coordinate (uz, uy, ux) through the matrix
__device__ __forceinline__ void dp_affine_map(const DpAffine& p, double uz, double uy, double ux, double& cz, double& cy, double& cx) {
    cz = p.a[0] * uz + p.a[1] * uy + p.a[2] * ux + p.ctr[0];
    cy = p.a[3] * uz + p.a[4] * uy + p.a[5] * ux + p.ctr[1];
    cx = p.a[6] * uz + p.a[7] * uy + p.a[8] * ux + p.ctr[2];
}
// cval where any coordinate leaves [0, n - 1] (a NaN coordinate does); order 3 on the spline coefficients (taps mirrored), order 0 nearest
template <int ORDER>
__device__ __forceinline__ float dp_sample(const void* __restrict__ src, const DpAffine& p, double cz, double cy, double cx, float cval) {
    float v = cval;
    if (cz >= 0.0 && cz <= p.sd - 1.0 && cy >= 0.0 && cy <= p.sh - 1.0 && cx >= 0.0 && cx <= p.sw - 1.0) {
        if (ORDER == 0) {
            const int z = (int)floor(cz + 0.5), y = (int)floor(cy + 0.5), x = (int)floor(cx + 0.5);
            v = ((const float*)src)[((long long)z * p.sh + y) * p.sw + x];
        } else {
            const int z0 = (int)floor(cz), y0 = (int)floor(cy), x0 = (int)floor(cx);
            double wz[4], wy[4], wx[4];
            dp_cubic_w(cz - z0, wz); dp_cubic_w(cy - y0, wy); dp_cubic_w(cx - x0, wx);
            const double* co = (const double*)src;
            double acc = 0.0;
            for (int a = 0; a < 4; ++a) {
                const long long zo = (long long)dp_mirror(z0 - 1 + a, p.sd) * p.sh;
                for (int b = 0; b < 4; ++b) {
                    const long long yo = (zo + dp_mirror(y0 - 1 + b, p.sh)) * p.sw;
                    double row = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) row += wx[k] * co[yo + dp_mirror(x0 - 1 + k, p.sw)];
                    acc += wz[a] * wy[b] * row;
                }
            }
            v = (float)acc;
        }
    }
    return v;
}

static inline int dp_blocks(long long total) { long long b = (total + 255) / 256; return (int)(b < 1 ? 1 : (b > 65535 ? 65535 : b)); }
static inline bool dp_dims_ok(int d, int h, int w) { return d > 0 && h > 0 && w > 0 && (double)d * h * w < 2147483648.0; }
