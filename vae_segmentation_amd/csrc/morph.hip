// Binary morphology (dilation, erosion, opening, closing) and hole filling of planar fp32 masks (include/vaeseg.h: vs_morph, vs_fill_holes).
//
// The reference dilates a bone mask with scipy.ndimage.binary_dilation(iterations=2) (utils/utils.py:647-655, get_synthesis_mask); the definitions
// here are scipy.ndimage's binary_dilation / binary_erosion / binary_opening / binary_closing / binary_fill_holes.  Every (n, c) plane is an
// independent problem.
//
// Morphology works on bit-packed rows: one 64-bit word per 64 x-voxels (a wave ballot, as sf_load_row takes it), so a 128^3 plane is 256 KB and a
// step is shifts and ORs of words.  Only ONE operator exists on the packed planes, dilation with a border value b (voxels outside the volume read
// as b; the pad bits of a row's last word hold b too, so a row is one infinite bit string).  Erosion is its dual — erode(X, b) = ~dilate(~X, ~b),
// the structures are symmetric — so an inversion at pack / unpack time, or on the loads of the first launch of a second phase, gives the rest:
//
//   dilate   pack          -> dilate^n (b)                          -> unpack
//   erode    pack inverted -> dilate^n (~b)                         -> unpack inverted
//   open     pack inverted -> dilate^n (~b) -> [invert] dilate^n (b)  -> unpack
//   close    pack          -> dilate^n (b)  -> [invert] dilate^n (~b) -> unpack inverted
//
//   dilate^n, connectivity 26   the box of half-width n: three axis passes (x: shifts of the row's words, y / z: ORs of the words of 2n + 1 rows),
//                               three launches whatever n is
//   dilate^n, connectivity 6    the L1 ball of radius n is not separable: n launches of one step (own word shifted both ways, the four row
//                               neighbours), ping-pong between two packed planes
//   n is capped at the extent that saturates the plane (a dilation only grows, so past the diameter it has reached its fixed point).
//
// Hole filling labels the COMPLEMENT with the union-find of cc_core.h (init: x-runs by ballot; merge: cc_merge_kernel as it stands, 6 or 26),
// marks the root of every background voxel that lies on a face of the volume, and writes out[v] = !(background(v) && marked(root(v))).
// Four launches; the only atomics are cc_core.h's atomicMin, whose result does not depend on their order; the marks are plain stores of 1.
//
// Phase boundaries are launch boundaries, every loop is bounded by the data, nothing is read back: both builds and every run give the same bits.
#include <limits.h>
#include "cc_core.h"

namespace {

typedef unsigned long long mo_word;

struct mo_dims {
    int d, h, w, segs;               // segs: words per row
    long long rows, words, total;    // planes * d * h, rows * segs, planes * d * h * w
    mo_word tail;                    // the valid bits of a row's last word
};

// pad bits (x >= w) of a row's last word hold the border value
__device__ __forceinline__ mo_word mo_pad(mo_word v, int seg, const mo_dims& g, int border) {
    if (seg != g.segs - 1) return v;
    return border ? v | ~g.tail : v & g.tail;
}

__global__ __launch_bounds__(256) void mo_pack_kernel(const float* __restrict__ mask, mo_word* __restrict__ words, mo_dims g, int invert, int border) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long s = wave0; s < g.words; s += nwaves) {
        const long long row = s / g.segs;
        const int seg = (int)(s - row * g.segs), x = seg * 64 + lane;
        const bool fg = x < g.w && mask[(size_t)row * g.w + x] >= 0.5f;      // the binarize rule, utils/evaluation.py:9-10
        mo_word b = __ballot(fg);
        if (invert) b = ~b;
        if (lane == 0) words[s] = mo_pad(b, seg, g, border);
    }
}

__global__ __launch_bounds__(256) void mo_unpack_kernel(const mo_word* __restrict__ words, float* __restrict__ out, mo_dims g, int invert) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long s = wave0; s < g.words; s += nwaves) {
        const long long row = s / g.segs;
        const int seg = (int)(s - row * g.segs), x = seg * 64 + lane;
        const bool on = (((words[s] >> lane) & 1ull) != 0) != (invert != 0);
        if (x < g.w) out[(size_t)row * g.w + x] = on ? 1.f : 0.f;
    }
}

// word i of a packed plane -> its row coordinates
struct mo_at {
    int seg, y, z;
};
__device__ __forceinline__ mo_at mo_at_of(long long i, const mo_dims& g) {
    mo_at a;
    const long long row = i / g.segs;
    a.seg = (int)(i - row * g.segs);
    const long long pz = row / g.h;
    a.y = (int)(row - pz * g.h);
    a.z = (int)(pz % g.d);
    return a;
}

// one step of the 6-neighbourhood.  xin: all ones when the input is read inverted (the first launch of a second phase), else 0
__global__ __launch_bounds__(256) void mo_step6_kernel(const mo_word* __restrict__ in, mo_word* __restrict__ out, mo_dims g, int border, mo_word xin) {
    const mo_word bw = border ? ~0ull : 0ull;
    const long long ystride = g.segs, zstride = (long long)g.h * g.segs;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.words; i += (long long)gridDim.x * 256) {
        const mo_at a = mo_at_of(i, g);
        const mo_word c = in[i] ^ xin;
        const mo_word l = a.seg > 0 ? in[i - 1] ^ xin : bw, r = a.seg < g.segs - 1 ? in[i + 1] ^ xin : bw;
        mo_word o = c | (c << 1) | (l >> 63) | (c >> 1) | (r << 63);
        o |= a.y > 0 ? in[i - ystride] ^ xin : bw;
        o |= a.y < g.h - 1 ? in[i + ystride] ^ xin : bw;
        o |= a.z > 0 ? in[i - zstride] ^ xin : bw;
        o |= a.z < g.d - 1 ? in[i + zstride] ^ xin : bw;
        out[i] = mo_pad(o, a.seg, g, border);
    }
}

// the x pass of the box: out bit x = OR of the row's bits x - r .. x + r, the row continued with the border value on both sides
__global__ __launch_bounds__(256) void mo_boxx_kernel(const mo_word* __restrict__ in, mo_word* __restrict__ out, mo_dims g, int r, int border, mo_word xin) {
    const mo_word bw = border ? ~0ull : 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.words; i += (long long)gridDim.x * 256) {
        const long long row = i / g.segs;
        const int seg = (int)(i - row * g.segs);
        const mo_word* rp = in + row * g.segs;
        auto get = [&](int j) { return j < 0 || j >= g.segs ? bw : rp[j] ^ xin; };
        mo_word o = 0;
        for (int q = 0; q * 64 <= r; ++q) {                    // shifts by 64 q + t, t = 0 .. min(63, r - 64 q)
            const mo_word al = get(seg - q), bl = get(seg - q - 1), ar = get(seg + q), br = get(seg + q + 1);
            const int tmax = r - q * 64 < 63 ? r - q * 64 : 63;
            o |= al | ar;
            for (int t = 1; t <= tmax; ++t) o |= (al << t) | (bl >> (64 - t)) | (ar >> t) | (br << (64 - t));
        }
        out[i] = mo_pad(o, seg, g, border);
    }
}

// a y (AXIS 1) or z (AXIS 2) pass of the box: the OR of the same word of the 2 r + 1 rows around; rows outside the volume are the border word
template <int AXIS>
__global__ __launch_bounds__(256) void mo_boxrow_kernel(const mo_word* __restrict__ in, mo_word* __restrict__ out, mo_dims g, int r, int border) {
    const long long stride = AXIS == 1 ? g.segs : (long long)g.h * g.segs;
    const int L = AXIS == 1 ? g.h : g.d;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.words; i += (long long)gridDim.x * 256) {
        const mo_at a = mo_at_of(i, g);
        const int p = AXIS == 1 ? a.y : a.z;
        const int lo = p - r < 0 ? -p : -r, hi = p + r > L - 1 ? L - 1 - p : r;
        mo_word o = border && (lo > -r || hi < r) ? ~0ull : 0ull;
        for (int k = lo; k <= hi; ++k) o |= in[i + k * stride];
        out[i] = o;                                            // the pad bits of every row read hold the border value already
    }
}

// ---- hole filling --------------------------------------------------------------------------------------------------------------------------
// cc_init_kernel on the complement: parent[v] = first voxel of v's BACKGROUND x-run inside its 64-wide segment, foreground -1; marks cleared
__global__ __launch_bounds__(256) void fh_init_kernel(const float* __restrict__ mask, int* __restrict__ parent, int* __restrict__ outside, cc_dims g,
                                                      long long nsegs, int segs) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long s = wave0; s < nsegs; s += nwaves) {
        const cc_seg q = cc_seg_of(s, segs, g);
        const int x = q.x0 + lane;
        const size_t at = (size_t)q.row * g.w + x;
        const bool bg = x < g.w && !(mask[at] >= 0.5f);
        const unsigned long long b = __ballot(bg);
        const unsigned long long below = ~b & ((1ull << lane) - 1ull);
        const int start = below ? 64 - __clzll(below) : 0;
        if (x < g.w) {
            parent[at] = bg ? (q.z * g.h + q.y) * g.w + q.x0 + start : -1;
            outside[at] = 0;
        }
    }
}

// outside[root(v)] = 1 for every background voxel v on a face of the volume.  Every writer stores the same value.
__global__ __launch_bounds__(256) void fh_mark_kernel(const int* __restrict__ parent, int* __restrict__ outside, cc_dims g, long long nsegs, int segs) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long s = wave0; s < nsegs; s += nwaves) {
        const cc_seg q = cc_seg_of(s, segs, g);
        const bool rowface = q.z == 0 || q.z == g.d - 1 || q.y == 0 || q.y == g.h - 1;
        if (!rowface && q.x0 != 0 && q.x0 + CC_SEG < g.w) continue;       // an inner segment of an inner row holds no face voxel
        const int x = q.x0 + lane;
        if (x >= g.w || !(rowface || x == 0 || x == g.w - 1)) continue;
        const int* L = parent + (size_t)q.plane * g.V;
        const int v = (q.z * g.h + q.y) * g.w + x;
        const int par = L[v];
        if (par >= 0) outside[(size_t)q.plane * g.V + cc_find(L, par)] = 1;
    }
}

__global__ __launch_bounds__(256) void fh_apply_kernel(const int* __restrict__ parent, const int* __restrict__ outside, float* __restrict__ out, cc_dims g) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < g.total; i += (long long)gridDim.x * 256) {
        const long long p = i / g.V;
        const int par = parent[i];
        bool open = false;                                     // background that reaches the outside of the volume
        if (par >= 0) open = outside[(size_t)p * g.V + cc_find(parent + (size_t)p * g.V, par)] != 0;
        out[i] = open ? 0.f : 1.f;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
size_t mo_align(size_t b) { return (b + 255) & ~(size_t)255; }
bool mo_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

int mo_check(int n, int c, int d, int h, int w, mo_dims* g) {
    if (n <= 0 || c <= 0 || d <= 0 || h <= 0 || w <= 0) return VS_ESHAPE;
    const long long V = (long long)d * h * w;
    if (V > INT_MAX) return VS_ESHAPE;
    g->d = d; g->h = h; g->w = w;
    g->segs = (w + 63) / 64;
    g->rows = (long long)n * c * d * h;
    g->words = g->rows * g->segs;
    g->total = (long long)n * c * V;
    g->tail = w % 64 ? (1ull << (w % 64)) - 1ull : ~0ull;
    return VS_OK;
}

// n dilations with border value `border`, ping-pong between src and other; *res: where the result is
int mo_dilate_launch(mo_word* src, mo_word* other, const mo_dims& g, int connectivity, int iterations, int border, bool invert_in, hipStream_t st,
                     mo_word** res) {
    const unsigned grid = cc_grid((g.words + 255) / 256);
    mo_word xin = invert_in ? ~0ull : 0ull;
    if (connectivity == 26) {
        const int rx = iterations < g.w ? iterations : g.w, ry = iterations < g.h ? iterations : g.h, rz = iterations < g.d ? iterations : g.d;
        hipLaunchKernelGGL(mo_boxx_kernel, dim3(grid), dim3(256), 0, st, (const mo_word*)src, other, g, rx, border, xin);
        VS_CHECK_LAUNCH();
        hipLaunchKernelGGL(mo_boxrow_kernel<1>, dim3(grid), dim3(256), 0, st, (const mo_word*)other, src, g, ry, border);
        VS_CHECK_LAUNCH();
        hipLaunchKernelGGL(mo_boxrow_kernel<2>, dim3(grid), dim3(256), 0, st, (const mo_word*)src, other, g, rz, border);
        VS_CHECK_LAUNCH();
        *res = other;
        return VS_OK;
    }
    const long long diameter = (long long)g.d + g.h + g.w;     // past it a plane is all zeros or all ones
    const int steps = iterations < diameter ? iterations : (int)diameter;
    for (int k = 0; k < steps; ++k) {
        hipLaunchKernelGGL(mo_step6_kernel, dim3(grid), dim3(256), 0, st, (const mo_word*)src, other, g, border, xin);
        VS_CHECK_LAUNCH();
        mo_word* t = src; src = other; other = t;
        xin = 0ull;
    }
    *res = src;
    return VS_OK;
}

}  // namespace

extern "C" long long vs_morph_workspace_bytes(int n, int c, int d, int h, int w) {
    mo_dims g;
    const int rc = mo_check(n, c, d, h, w, &g);
    if (rc != VS_OK) return rc;
    return (long long)(2 * mo_align((size_t)g.words * sizeof(mo_word)));
}

extern "C" int vs_morph(const float* mask, float* out, int n, int c, int d, int h, int w, int op, int connectivity, int iterations, int border_value,
                        void* workspace, void* stream) {
    mo_dims g;
    if (connectivity != 6 && connectivity != 26) return VS_EINVAL;
    if (op < VS_MORPH_DILATE || op > VS_MORPH_CLOSE || iterations < 1 || (border_value != 0 && border_value != 1)) return VS_EINVAL;
    const int rc = mo_check(n, c, d, h, w, &g);
    if (rc != VS_OK) return rc;
    if (!mask || !out || !workspace || mask == out || workspace == (const void*)mask || workspace == (void*)out) return VS_EINVAL;
    if (mo_misaligned(workspace)) return VS_EALIGN;
    const hipStream_t st = (hipStream_t)stream;
    mo_word* a = (mo_word*)workspace;
    mo_word* b = (mo_word*)((char*)workspace + mo_align((size_t)g.words * sizeof(mo_word)));
    // the first phase of erode / open runs on the inverted mask with the inverted border; open / close add a second phase on the inverted result
    const bool inv_first = op == VS_MORPH_ERODE || op == VS_MORPH_OPEN, two = op == VS_MORPH_OPEN || op == VS_MORPH_CLOSE;
    const int b1 = inv_first ? 1 - border_value : border_value;
    const unsigned seg_grid = cc_grid((g.words + 3) / 4);
    hipLaunchKernelGGL(mo_pack_kernel, dim3(seg_grid), dim3(256), 0, st, mask, a, g, (int)inv_first, b1);
    VS_CHECK_LAUNCH();
    mo_word* res;
    int lrc = mo_dilate_launch(a, b, g, connectivity, iterations, b1, false, st, &res);
    if (lrc != VS_OK) return lrc;
    bool inv_out = inv_first;
    if (two) {
        lrc = mo_dilate_launch(res, res == a ? b : a, g, connectivity, iterations, 1 - b1, true, st, &res);
        if (lrc != VS_OK) return lrc;
        inv_out = !inv_first;
    }
    hipLaunchKernelGGL(mo_unpack_kernel, dim3(seg_grid), dim3(256), 0, st, (const mo_word*)res, out, g, (int)inv_out);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

namespace {
int fh_check(int n, int c, int d, int h, int w, int connectivity, cc_dims* g) {
    if (connectivity != 6 && connectivity != 26) return VS_EINVAL;
    if (n <= 0 || c <= 0 || d <= 0 || h <= 0 || w <= 0) return VS_ESHAPE;
    const long long V = (long long)d * h * w;
    if (V > INT_MAX) return VS_ESHAPE;                         // plane-local indices are int32
    g->n = n; g->c = c; g->d = d; g->h = h; g->w = w; g->lo = 0;
    g->V = (int)V;
    g->maxk = 0; g->nb = 0;                                    // no size table, no chunks: only the union-find is used
    g->planes = (long long)n * c;
    g->total = g->planes * V;
    return VS_OK;
}
}  // namespace

extern "C" long long vs_fill_holes_workspace_bytes(int n, int c, int d, int h, int w, int connectivity) {
    cc_dims g;
    const int rc = fh_check(n, c, d, h, w, connectivity, &g);
    if (rc != VS_OK) return rc;
    return (long long)(2 * mo_align((size_t)g.total * 4));
}

extern "C" int vs_fill_holes(const float* mask, float* out, int n, int c, int d, int h, int w, int connectivity, void* workspace, void* stream) {
    cc_dims g;
    const int rc = fh_check(n, c, d, h, w, connectivity, &g);
    if (rc != VS_OK) return rc;
    if (!mask || !out || !workspace || mask == out || workspace == (const void*)mask || workspace == (void*)out) return VS_EINVAL;
    if (mo_misaligned(workspace)) return VS_EALIGN;
    const hipStream_t st = (hipStream_t)stream;
    int* parent = (int*)workspace;
    int* outside = (int*)((char*)workspace + mo_align((size_t)g.total * 4));
    const int segs = (g.w + CC_SEG - 1) / CC_SEG;
    const long long nsegs = g.planes * g.d * g.h * segs;
    const unsigned seg_grid = cc_grid((nsegs + 3) / 4);
    hipLaunchKernelGGL(fh_init_kernel, dim3(seg_grid), dim3(256), 0, st, mask, parent, outside, g, nsegs, segs);
    VS_CHECK_LAUNCH();
    if (connectivity == 26) hipLaunchKernelGGL(cc_merge_kernel<26>, dim3(seg_grid), dim3(256), 0, st, parent, g, nsegs, segs);
    else hipLaunchKernelGGL(cc_merge_kernel<6>, dim3(seg_grid), dim3(256), 0, st, parent, g, nsegs, segs);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(fh_mark_kernel, dim3(seg_grid), dim3(256), 0, st, (const int*)parent, outside, g, nsegs, segs);
    VS_CHECK_LAUNCH();
    hipLaunchKernelGGL(fh_apply_kernel, dim3(cc_grid((g.total + 255) / 256)), dim3(256), 0, st, (const int*)parent, (const int*)outside, out, g);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
