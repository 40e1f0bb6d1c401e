// A crop-space prediction pasted back into scan geometry (include/vaeseg.h: vs_uncrop).
//
// data_gpu.CropResize cuts the scan rows [lo, hi) of every axis, puts them at [off, off + hi - lo) of a zero cube of side `side` and resizes that cube
// to P^3 (csrc/data.hip: dp_crop_pad_kernel, dp_zoom_kernel).  The network's probabilities (K, P, P, P) live on that patch grid; this kernel
// resamples them onto the scan grid (D, H, W) and takes the argmax, in one launch that writes every voxel of the outputs exactly once:
//
//   inside   lo <= v < hi on every axis: cube index u = v - lo + off, patch coordinate q = (u + 0.5) P / side - 0.5 (the inverse of dp_zoom_kernel's
//            grid, skimage / scipy.ndimage.zoom(grid_mode=True)), in fp64
//            linear   q clamped to [0, P - 1], trilinear: the four (z, y) neighbours weighted wz wy for each of the two x columns, the columns weighted
//                     by x, all in fp64, rounded to fp32 once
//                     = scipy.ndimage.zoom(p_k, side / P, order=1, mode='nearest', grid_mode=True) on the cube rows that exist in the scan
//            nearest  index floor(q + 0.5), clamped: the rounding of the order-0 zoom
//   outside  probability (1, 0, ..., 0), label 0
//   label    argmax of the fp32 probabilities, ties to the first maximal channel, a NaN channel wins (vs_hard_onehot, vs_sw_finalize)
//
// A thread owns four consecutive x of one scan row (csrc/window.hip's shape): the z and y indices and weights are computed once per thread, the four
// labels leave as one 32-bit word and the four probabilities of a class as one 16-byte store where the row is aligned, element by element otherwise.
// No memset, no atomics, no LDS: bandwidth-bound on the stores, the (K, P, P, P) reads stay in cache.  Offsets are 64-bit.  Every patch index is
// clamped to [0, P - 1] and every store is bounded by (D, H, W) alone, so no geometry can address outside either buffer.
#include <math.h>
#include <stdint.h>
#include "volume.h"

namespace {

struct uc_geom {
    int k, p, d, h, w;
    int lo[3], hi[3], off[3];
    int side;
};

constexpr long long UC_GRID_CAP = 1 << 20;

// the patch coordinate of scan index v along one axis, or false outside the cube's rows
template <int LINEAR>
__device__ __forceinline__ bool uc_coord(int v, int lo, int hi, int off, int side, int p, rs_axis& a) {
    a.i0 = a.i1 = 0;
    a.t = 0.0;
    if (v < lo || v >= hi) return false;
    const double u = (double)v - (double)lo + (double)off;
    rs_axis_at<LINEAR>((u + 0.5) * p / side - 0.5, p, a);
    return true;
}

template <int LINEAR>
__global__ __launch_bounds__(256) void uncrop_kernel(const float* __restrict__ prob, unsigned char* __restrict__ label, float* __restrict__ out, uc_geom g,
                                                     int nq, long long total) {
    const size_t V = (size_t)g.d * g.h * g.w, PV = (size_t)g.p * g.p * g.p;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int qd = (int)(i % nq);
        const long long r = i / nq;
        const int y = (int)(r % g.h), z = (int)(r / g.h);
        const int x0 = 4 * qd, n = g.w - x0 < 4 ? g.w - x0 : 4;
        const size_t vrow = ((size_t)z * g.h + y) * g.w + x0;
        rs_axis az, ay, ax[4];
        const bool in_z = uc_coord<LINEAR>(z, g.lo[0], g.hi[0], g.off[0], g.side, g.p, az);
        const bool in_zy = uc_coord<LINEAR>(y, g.lo[1], g.hi[1], g.off[1], g.side, g.p, ay) && in_z;
        unsigned in = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (uc_coord<LINEAR>(x0 + e, g.lo[2], g.hi[2], g.off[2], g.side, g.p, ax[e]) && in_zy && e < n) in |= 1u << e;
        const rs_rows rows(az, ay, g.p, g.p);                  // the four patch rows this thread reads and their weights
        float best[4];
        int arg[4] = {0, 0, 0, 0};
        for (int k = 0; k < g.k; ++k) {
            const float* plane = prob + (size_t)k * PV;
            float a[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = k == 0 ? 1.f : 0.f;
                if (in & (1u << e)) a[e] = rows.sample<LINEAR>(plane, ax[e]);
                if (k == 0) {
                    best[e] = a[e];
                } else if (a[e] > best[e] || (a[e] != a[e] && best[e] == best[e])) {
                    best[e] = a[e];
                    arg[e] = k;
                }
            }
            if (out) {
                float* op = out + (size_t)k * V + vrow;
                if (n == 4 && ((uintptr_t)op & 15) == 0) {
                    *reinterpret_cast<float4*>(op) = make_float4(a[0], a[1], a[2], a[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < n) op[e] = a[e];
                }
            }
        }
        unsigned char* lp = label + vrow;
        if (n == 4 && ((uintptr_t)lp & 3) == 0) {
            *reinterpret_cast<unsigned int*>(lp) = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) lp[e] = (unsigned char)arg[e];
        }
    }
}

bool uc_dims_ok(int d, int h, int w) { return d > 0 && h > 0 && w > 0 && (double)d * h * w < 2147483648.0; }      // data.hip's dp_dims_ok

}  // namespace

extern "C" int vs_uncrop(const float* prob, unsigned char* label, float* prob_out, int k, int patch, int d, int h, int w, int lo_z, int lo_y, int lo_x,
                         int hi_z, int hi_y, int hi_x, int off_z, int off_y, int off_x, int side, int interp, void* stream) {
    if (!uc_dims_ok(d, h, w) || patch <= 0 || !uc_dims_ok(patch, patch, patch)) return VS_ESHAPE;
    if (k < 1 || k > 8 || side <= 0 || (interp != 0 && interp != 1)) return VS_EINVAL;
    if (!prob || !label || (const void*)prob == (const void*)prob_out) return VS_EINVAL;
    if (((uintptr_t)prob & 15) != 0 || ((uintptr_t)label & 15) != 0 || ((uintptr_t)prob_out & 15) != 0) return VS_EALIGN;
    const uc_geom g = {k, patch, d, h, w, {lo_z, lo_y, lo_x}, {hi_z, hi_y, hi_x}, {off_z, off_y, off_x}, side};
    const int dims[3] = {d, h, w};
    for (int a = 0; a < 3; ++a) {                                // the rows [lo, hi) exist in the scan and fit into the cube behind `off`
        if (g.lo[a] < 0 || g.hi[a] < g.lo[a] || g.hi[a] > dims[a] || g.off[a] < 0 || g.off[a] > side || g.hi[a] - g.lo[a] > side - g.off[a]) return VS_EINVAL;
    }
    const int nq = (w + 3) / 4;
    const long long total = (long long)d * h * nq, blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(blocks > UC_GRID_CAP ? UC_GRID_CAP : blocks);
    if (interp == 0) hipLaunchKernelGGL(uncrop_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, prob, label, prob_out, g, nq, total);
    else hipLaunchKernelGGL(uncrop_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, prob, label, prob_out, g, nq, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
