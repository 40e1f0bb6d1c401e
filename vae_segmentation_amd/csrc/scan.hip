// Scan geometry on the device (include/vaeseg.h: vs_scan_orient, vs_scan_to_native): the two ends of the label-free inference chain.
//
// The reference's data/data_process.py:24-33 turns the array a scanner wrote, raw (X, Y, Z), into the volume every entry point expects:
//   oriented = transpose(raw, [1, 0, 2])[::ind[1], ::ind[0], ::ind[2]]     (Y, X, Z), ind[i] = +1 where the affine's diagonal is negative, else -1
//   1 mm     = skimage resize of the oriented volume to shape_1mm            (data.hip: vs_data_gaussian_axis, vs_data_zoom)
// data_gpu.ScanGeometry holds the integers; the kernels take them as (x, y, z) and three flips in ORIENTED axis order:
//   oriented[o0][o1][o2] = raw[g1(o1)][g0(o0)][g2(o2)],   g_a(o) = flip_a ? n_a - 1 - o : o,   (n_0, n_1, n_2) = (y, x, z)
//
// scan_orient_kernel   raw int16 / uint8 / int8 / fp32 -> contiguous fp32 oriented volume, exact values.  The contiguous axis (raw Z) stays the contiguous
//                      axis and is at most reversed: a thread owns four consecutive z of one oriented row, reads them with one 4-element load where the
//                      address is aligned (reversed in registers under a z flip) and writes one 16-byte store.
// scan_native_kernel   the way back: every raw voxel (i0, i1, i2) has the oriented index (g0(i1), g1(i0), g2(i2)) and per axis the 1 mm coordinate
//                      q = (o + 0.5) n_1mm / n_oriented - 0.5 in fp64 (the grid of scipy.ndimage.zoom(grid_mode=True), as vs_data_zoom and vs_uncrop).
//                        nearest  the sample at floor(q + 0.5) clamped to [0, n_1mm - 1]
//                        linear   q mirrored at the borders (q < 0 -> -q, q > n - 1 -> 2 (n - 1) - q: scipy's mode='mirror'), the two neighbours per axis
//                                 weighted by the fraction: the four (d, h) rows weighted once, then the two w columns, all in fp64, rounded to fp32 once
//                                 = scipy.ndimage.zoom(p_k, oriented / 1mm, order=1, mode='mirror', grid_mode=True)
//                        label    argmax of the fp32 probabilities, ties to the first maximal channel, a NaN channel wins (vs_hard_onehot, vs_uncrop)
//                      A thread owns four consecutive z of one raw row (vs_uncrop's shape): the indices and weights of the row's two slow axes are computed
//                      once per thread, those of its four z once, and all K classes reuse them.  The four labels leave as one 32-bit word, the four
//                      probabilities of a class as one 16-byte store where the row is aligned.
// scan_native_label_kernel   the same map for a uint8 label on the 1 mm grid (nearest only): a copy of samples.
// One launch each; every output element is written exactly once; no memset, no atomics, no LDS, no synchronisation.  Offsets are 64-bit.  Every source
// index is clamped into its axis and every store is bounded by (x, y, z) alone, so no geometry can address outside either buffer.
#include <math.h>
#include <stdint.h>
#include "volume.h"

namespace {

struct sc_geom {
    int k;
    int n1[3];       // the 1 mm grid (D1, H1, W1)
    int x, y, z;     // the raw grid
    int flip[3];     // oriented axis order: (y, x, z)
};

constexpr long long SC_GRID_CAP = 1 << 16;

template <typename T>
struct alignas(4 * sizeof(T)) sc_vec4 {
    T v[4];
};

// the 1 mm coordinate of oriented index o along an axis of n_o oriented and n_1 1 mm rows
template <int LINEAR>
__device__ __forceinline__ void sc_coord(int o, int n_o, int n_1, rs_axis& a) {
    const double q = ((double)o + 0.5) * n_1 / n_o - 0.5;
    if (LINEAR) {                                              // reflected at both ends before the clamp: not rs_axis_at's rule
        const double top = (double)(n_1 - 1);
        double c = q < 0.0 ? -q : (q > top ? 2.0 * top - q : q);
        c = fmin(fmax(c, 0.0), top);
        const int i = (int)floor(c);
        a.i0 = i;
        a.i1 = i + 1 < n_1 ? i + 1 : n_1 - 1;
        a.t = c - (double)i;
    } else {
        a.t = 0.0;
        rs_axis_at<0>(q, n_1, a);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void scan_orient_kernel(const T* __restrict__ raw, float* __restrict__ out, int X, int Y, int Z, int f0, int f1, int f2,
                                                          int nq, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int qd = (int)(i % nq);
        const long long r = i / nq;
        const int o1 = (int)(r % X), o0 = (int)(r / X);
        const int i0 = f1 ? X - 1 - o1 : o1, i1 = f0 ? Y - 1 - o0 : o0;
        const int z0 = 4 * qd, n = Z - z0 < 4 ? Z - z0 : 4;
        const T* row = raw + ((size_t)i0 * Y + i1) * Z;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        const T* first = row + (n < 4 ? 0 : (f2 ? Z - 4 - z0 : z0));            // the lowest address of the four (a full quad only)
        if (n == 4 && ((uintptr_t)first & (4 * sizeof(T) - 1)) == 0) {
            const sc_vec4<T> v = *reinterpret_cast<const sc_vec4<T>*>(first);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = (float)v.v[f2 ? 3 - e : e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) a[e] = (float)row[f2 ? Z - 1 - (z0 + e) : z0 + e];
        }
        float* op = out + (size_t)r * Z + z0;
        if (n == 4 && ((uintptr_t)op & 15) == 0) {
            *reinterpret_cast<float4*>(op) = make_float4(a[0], a[1], a[2], a[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) op[e] = a[e];
        }
    }
}

template <int LINEAR>
__global__ __launch_bounds__(256) void scan_native_kernel(const float* __restrict__ prob, unsigned char* __restrict__ label, float* __restrict__ out, sc_geom g,
                                                          int nq, long long total) {
    const size_t V = (size_t)g.x * g.y * g.z, PV = (size_t)g.n1[0] * g.n1[1] * g.n1[2];
    const int H1 = g.n1[1], W1 = g.n1[2];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int qd = (int)(i % nq);
        const long long r = i / nq;
        const int i1 = (int)(r % g.y), i0 = (int)(r / g.y);
        const int z0 = 4 * qd, n = g.z - z0 < 4 ? g.z - z0 : 4;
        const size_t vrow = (size_t)r * g.z + z0;
        rs_axis ad, ah, aw[4];
        sc_coord<LINEAR>(g.flip[0] ? g.y - 1 - i1 : i1, g.y, g.n1[0], ad);
        sc_coord<LINEAR>(g.flip[1] ? g.x - 1 - i0 : i0, g.x, g.n1[1], ah);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i2 = z0 + e < g.z ? z0 + e : g.z - 1;
            sc_coord<LINEAR>(g.flip[2] ? g.z - 1 - i2 : i2, g.z, g.n1[2], aw[e]);
        }
        const rs_rows rows(ad, ah, H1, W1);                    // the four 1 mm rows this thread reads and their weights
        float best[4];
        int arg[4] = {0, 0, 0, 0};
        for (int k = 0; k < g.k; ++k) {
            const float* plane = prob + (size_t)k * PV;
            float a[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = rows.sample<LINEAR>(plane, aw[e]);
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

__global__ __launch_bounds__(256) void scan_native_label_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ label, sc_geom g, int nq,
                                                                long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int qd = (int)(i % nq);
        const long long r = i / nq;
        const int i1 = (int)(r % g.y), i0 = (int)(r / g.y);
        const int z0 = 4 * qd, n = g.z - z0 < 4 ? g.z - z0 : 4;
        rs_axis ad, ah, aw;
        sc_coord<0>(g.flip[0] ? g.y - 1 - i1 : i1, g.y, g.n1[0], ad);
        sc_coord<0>(g.flip[1] ? g.x - 1 - i0 : i0, g.x, g.n1[1], ah);
        const unsigned char* row = src + ((size_t)ad.i0 * g.n1[1] + ah.i0) * g.n1[2];
        unsigned v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i2 = z0 + e < g.z ? z0 + e : g.z - 1;
            sc_coord<0>(g.flip[2] ? g.z - 1 - i2 : i2, g.z, g.n1[2], aw);
            v[e] = row[aw.i0];
        }
        unsigned char* lp = label + (size_t)r * g.z + z0;
        if (n == 4 && ((uintptr_t)lp & 3) == 0) {
            *reinterpret_cast<unsigned int*>(lp) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < n) lp[e] = (unsigned char)v[e];
        }
    }
}

bool sc_dims_ok(int d, int h, int w) { return d > 0 && h > 0 && w > 0 && (double)d * h * w < 2147483648.0; }      // data.hip's dp_dims_ok

unsigned sc_grid(long long total) {
    const long long blocks = (total + 255) / 256;
    return (unsigned)(blocks > SC_GRID_CAP ? SC_GRID_CAP : blocks);
}

template <typename T>
void sc_launch_orient(const void* raw, float* out, int x, int y, int z, int f0, int f1, int f2, hipStream_t stream) {
    const int nq = (z + 3) / 4;
    const long long total = (long long)x * y * nq;
    hipLaunchKernelGGL(scan_orient_kernel<T>, dim3(sc_grid(total)), dim3(256), 0, stream, (const T*)raw, out, x, y, z, f0, f1, f2, nq, total);
}

}  // namespace

extern "C" int vs_scan_orient(const void* raw, int dtype, float* out, int x, int y, int z, int flip0, int flip1, int flip2, void* stream) {
    if (!sc_dims_ok(x, y, z)) return VS_ESHAPE;
    if (!raw || !out || raw == (const void*)out) return VS_EINVAL;
    if (((uintptr_t)raw & 15) != 0 || ((uintptr_t)out & 15) != 0) return VS_EALIGN;
    const int f0 = flip0 != 0, f1 = flip1 != 0, f2 = flip2 != 0;
    switch (dtype) {
        case VS_SCAN_I16: sc_launch_orient<short>(raw, out, x, y, z, f0, f1, f2, (hipStream_t)stream); break;
        case VS_SCAN_U8: sc_launch_orient<unsigned char>(raw, out, x, y, z, f0, f1, f2, (hipStream_t)stream); break;
        case VS_SCAN_I8: sc_launch_orient<signed char>(raw, out, x, y, z, f0, f1, f2, (hipStream_t)stream); break;
        case VS_SCAN_F32: sc_launch_orient<float>(raw, out, x, y, z, f0, f1, f2, (hipStream_t)stream); break;
        default: return VS_EDTYPE;
    }
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_scan_to_native(const void* src, int src_is_label, unsigned char* label, float* prob_out, int k, int d1, int h1, int w1, int x, int y, int z,
                                 int flip0, int flip1, int flip2, int interp, void* stream) {
    if (!sc_dims_ok(x, y, z) || !sc_dims_ok(d1, h1, w1)) return VS_ESHAPE;
    if (interp != 0 && interp != 1) return VS_EINVAL;
    if (src_is_label ? (k != 1 || interp != 0 || prob_out != nullptr) : (k < 1 || k > 8)) return VS_EINVAL;
    if (!src || !label || src == (const void*)prob_out || src == (const void*)label) return VS_EINVAL;
    if (((uintptr_t)src & 15) != 0 || ((uintptr_t)label & 15) != 0 || ((uintptr_t)prob_out & 15) != 0) return VS_EALIGN;
    const sc_geom g = {k, {d1, h1, w1}, x, y, z, {flip0 != 0, flip1 != 0, flip2 != 0}};
    const int nq = (z + 3) / 4;
    const long long total = (long long)x * y * nq;
    const dim3 grid(sc_grid(total));
    if (src_is_label)
        hipLaunchKernelGGL(scan_native_label_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src, label, g, nq, total);
    else if (interp == 0)
        hipLaunchKernelGGL(scan_native_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, label, prob_out, g, nq, total);
    else
        hipLaunchKernelGGL(scan_native_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, label, prob_out, g, nq, total);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
