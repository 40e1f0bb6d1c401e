// The VAE bottleneck: fully connected layers, reparameterisation, the Philox latent stream, KL.
#include "common.h"
#include "philox.h"
#include <math.h>

// ---- fully connected --------------------------------------------------------------------------------
__device__ __forceinline__ long long phys_index(int k, int pc, int pv) { return pc > 0 ? (long long)(k % pv) * pc + k / pv : k; }
__device__ __forceinline__ float ld_any(const void* p, int dtype, long long i) {
    if (dtype == VS_F32) return ((const float*)p)[i];
    if (dtype == VS_BF16) return bf2f(((const unsigned short*)p)[i]);
    return (float)((const vs_half*)p)[i];
}
__device__ __forceinline__ void st_any(void* p, int dtype, long long i, float v) {
    if (dtype == VS_F32) ((float*)p)[i] = v;
    else if (dtype == VS_BF16) ((unsigned short*)p)[i] = f2bf(v);
    else ((vs_half*)p)[i] = (vs_half)v;
}
#define LIN_MAXB 16

// one workgroup per output j: y[b][j] = act(bias[j] + sum_k W[j][k] x[b][phys(k)]).  NB = batch rounded up to 1/2/4/8/16 at compile
// time (padding rows re-read row batch-1 and are dropped), k unrolled by 4: 4 weight + 4*NB activation loads are in flight per
// thread instead of one dependent load per FMA (the bottleneck GEMV is latency-, not bandwidth-bound: 27 k-steps per thread).
// Round 6: (1) 16-byte weight loads, four consecutive k per lane and load — the bottleneck widths finish in ONE round of <= 8 loads per thread (dword loads in
// two dependent rounds streamed the frozen fc2's 14 MB at 1.1 TB/s: 12.6 us); (2) a PERMUTED activation (pc > 0: the channels-last bottleneck tensor read in the
// reference's (c, z, y, x) flattening order) made every lane gather 2-byte elements pc apart; when its fp32 image fits the LDS (s_x, [NB][k_in]) the workgroup reads x
// once in PHYSICAL order (coalesced) and writes it at its logical index, and the k loop reads consecutive words.
template <int NB>
__device__ __forceinline__ void linear_fwd_body(const void* __restrict__ x, int x_dtype, const float* __restrict__ w,
                                                const float* __restrict__ bias, float* __restrict__ y, int batch, int k_in,
                                                int j_out, int pc, int pv, int relu, float* s_x) {
    const int j = blockIdx.x;
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    const float* wr = w + (size_t)j * k_in;
    const int nt = (int)blockDim.x;                       // 256, or 1024 for the wide layers (one round of loads instead of several)
    // four k per lane: every row of w and x 16-byte aligned, and (permuted x) the four k of a group in one channel (pv % 4 == 0)
    const bool vec = (k_in & 3) == 0 && ((uintptr_t)w & 15) == 0 && (pc == 0 ? ((uintptr_t)x & 15) == 0 : (pv & 3) == 0);
    if (vec) {
        constexpr int LU4 = NB <= 1 ? 8 : (NB <= 2 ? 4 : (NB <= 4 ? 4 : (NB <= 8 ? 2 : 1)));      // 1024-thread workgroups: 128 VGPRs (LU4 * NB * 4 activation values in flight)
        const int nk4 = k_in >> 2;
        const f32x4* wr4 = (const f32x4*)wr;
        if (s_x != nullptr) {                             // workgroup-uniform
            for (int qi = threadIdx.x; qi < k_in; qi += nt) {
                const int v = qi / pc, c = qi - v * pc;   // physical index qi = v * pc + c  <->  logical k = c * pv + v (phys_index's inverse)
#pragma unroll
                for (int b = 0; b < NB; ++b) s_x[b * k_in + c * pv + v] = ld_any(x, x_dtype, (long long)(b < batch ? b : batch - 1) * k_in + qi);
            }
            __syncthreads();
        }
        for (int k0 = threadIdx.x; k0 < nk4; k0 += nt * LU4) {
            f32x4 wv[LU4];
            float xv[LU4][NB][4];
#pragma unroll
            for (int u = 0; u < LU4; ++u) {
                const int k4 = k0 + u * nt;
                const bool ok = k4 < nk4;
                wv[u] = ok ? wr4[k4] : f32x4{0.f, 0.f, 0.f, 0.f};
                const int kk = 4 * (ok ? k4 : 0);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const long long row = (long long)(b < batch ? b : batch - 1) * k_in;
                    if (s_x != nullptr) {
                        const f32x4 t = *(const f32x4*)(s_x + b * k_in + kk);
                        xv[u][b][0] = t[0]; xv[u][b][1] = t[1]; xv[u][b][2] = t[2]; xv[u][b][3] = t[3];
                    } else if (pc > 0) {
                        const long long ph = phys_index(kk, pc, pv);              // k .. k + 3: the same channel, voxels v .. v + 3
#pragma unroll
                        for (int i = 0; i < 4; ++i) xv[u][b][i] = ld_any(x, x_dtype, row + ph + (long long)i * pc);
                    } else if (x_dtype == VS_F32) {
                        const f32x4 t = *(const f32x4*)((const float*)x + row + kk);
                        xv[u][b][0] = t[0]; xv[u][b][1] = t[1]; xv[u][b][2] = t[2]; xv[u][b][3] = t[3];
                    } else {
                        const u32x2 t = *(const u32x2*)((const unsigned short*)x + row + kk);
                        if (x_dtype == VS_BF16) {
                            xv[u][b][0] = H16<unsigned short>::lo(t[0]); xv[u][b][1] = H16<unsigned short>::hi(t[0]);
                            xv[u][b][2] = H16<unsigned short>::lo(t[1]); xv[u][b][3] = H16<unsigned short>::hi(t[1]);
                        } else {
                            xv[u][b][0] = H16<vs_half>::lo(t[0]); xv[u][b][1] = H16<vs_half>::hi(t[0]);
                            xv[u][b][2] = H16<vs_half>::lo(t[1]); xv[u][b][3] = H16<vs_half>::hi(t[1]);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < LU4; ++u)
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[b] += wv[u][i] * xv[u][b][i];
        }
    } else {
        // one k per lane and load (ragged widths, pv % 4 != 0): LU k-steps per round
        constexpr int LU = NB <= 2 ? 16 : (NB <= 4 ? 8 : 4);
        for (int k0 = threadIdx.x; k0 < k_in; k0 += nt * LU) {
            float wv[LU], xv[LU][NB];
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const int k = k0 + u * nt;
                const bool ok = k < k_in;
                wv[u] = ok ? wr[k] : 0.f;
                const long long ph = phys_index(ok ? k : 0, pc, pv);
#pragma unroll
                for (int b = 0; b < NB; ++b) xv[u][b] = ld_any(x, x_dtype, (long long)(b < batch ? b : batch - 1) * k_in + ph);
            }
#pragma unroll
            for (int u = 0; u < LU; ++u)
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] += wv[u] * xv[u][b];
        }
    }
    __shared__ float red[16][NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float s = wave_sum(acc[b]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][b] = s;
    }
    __syncthreads();
    if (threadIdx.x < batch) {
        float s = bias ? bias[j] : 0.f;
        for (int w2 = 0; w2 < (nt >> 6); ++w2) s += red[w2][threadIdx.x];
        if (relu && s < 0.f) s = 0.f;
        y[(size_t)threadIdx.x * j_out + j] = s;
    }
}
template <int NB>
__global__ __launch_bounds__(1024) void linear_fwd_kernel(const void* __restrict__ x, int x_dtype, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y, int batch, int k_in,
                                                         int j_out, int pc, int pv, int relu, int lds_x) {
    extern __shared__ __attribute__((aligned(16))) float s_lin[];
    linear_fwd_body<NB>(x, x_dtype, w, bias, y, batch, k_in, j_out, pc, pv, relu, lds_x ? s_lin : nullptr);
}
// fc_mean and fc_std read the same bottleneck activation (joint_model.py:241-243): blockIdx.y picks the layer, one launch for both
struct LinearPair { const float* w[2]; const float* bias[2]; float* y[2]; int relu[2]; };
template <int NB>
__global__ __launch_bounds__(1024) void linear_fwd_pair_kernel(const void* __restrict__ x, int x_dtype, const LinearPair a, int batch, int k_in,
                                                              int j_out, int pc, int pv, int lds_x) {
    extern __shared__ __attribute__((aligned(16))) float s_lin[];
    const int op = blockIdx.y;
    linear_fwd_body<NB>(x, x_dtype, a.w[op], a.bias[op], a.y[op], batch, k_in, j_out, pc, pv, a.relu[op], lds_x ? s_lin : nullptr);
}
// bytes of the LDS image of x (0: read it from memory as before — not permuted, or too large for the default 64 KB)
static inline size_t lin_lds_bytes(int nb, int k_in, int pc, int pv) {
    const size_t need = (size_t)nb * k_in * sizeof(float);
    return (pc > 0 && (k_in & 3) == 0 && (pv & 3) == 0 && need <= 64 * 1024) ? need : 0;      // only the four-k-per-lane path stages x
}

extern "C" int vs_linear_fwd(const void* x, int x_dtype, const float* wgt, const float* bias, float* y, int batch, int k_in,
                             int j_out, int pc, int pv, int relu, void* stream) {
    if (!x || !wgt || !y || batch <= 0 || batch > LIN_MAXB || k_in <= 0 || j_out <= 0) return VS_EINVAL;
    if (pc > 0 && (long long)pc * pv != k_in) return VS_ESHAPE;
    const int lin_threads = k_in >= 4096 ? 1024 : 256;
#define LIN_FWD(NB) hipLaunchKernelGGL(linear_fwd_kernel<NB>, dim3(j_out), dim3(lin_threads), lin_lds_bytes(NB, k_in, pc, pv), (hipStream_t)stream, x, x_dtype, wgt, bias, y, batch, k_in, j_out, pc, pv, relu, lin_lds_bytes(NB, k_in, pc, pv) ? 1 : 0)
    if (batch == 1) LIN_FWD(1); else if (batch == 2) LIN_FWD(2); else if (batch <= 4) LIN_FWD(4); else if (batch <= 8) LIN_FWD(8); else LIN_FWD(16);
#undef LIN_FWD
    VS_CHECK_LAUNCH();
    return VS_OK;
}

extern "C" int vs_linear_fwd_pair(const void* x, int x_dtype, const float* w1, const float* b1, float* y1, int relu1, const float* w2,
                                  const float* b2, float* y2, int relu2, int batch, int k_in, int j_out, int pc, int pv, void* stream) {
    if (!x || !w1 || !w2 || !y1 || !y2 || batch <= 0 || batch > LIN_MAXB || k_in <= 0 || j_out <= 0) return VS_EINVAL;
    if (pc > 0 && (long long)pc * pv != k_in) return VS_ESHAPE;
    LinearPair a;
    a.w[0] = w1; a.w[1] = w2; a.bias[0] = b1; a.bias[1] = b2; a.y[0] = y1; a.y[1] = y2; a.relu[0] = relu1; a.relu[1] = relu2;
    const int lin_threads = k_in >= 4096 ? 1024 : 256;
#define LIN_FWD2(NB) hipLaunchKernelGGL(linear_fwd_pair_kernel<NB>, dim3(j_out, 2), dim3(lin_threads), lin_lds_bytes(NB, k_in, pc, pv), (hipStream_t)stream, x, x_dtype, a, batch, k_in, j_out, pc, pv, lin_lds_bytes(NB, k_in, pc, pv) ? 1 : 0)
    if (batch == 1) LIN_FWD2(1); else if (batch == 2) LIN_FWD2(2); else if (batch <= 4) LIN_FWD2(4); else if (batch <= 8) LIN_FWD2(8); else LIN_FWD2(16);
#undef LIN_FWD2
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// one wave per output j (k_in is small, e.g. 128): y[b][phys(j)] = bias[j] + sum_k W[j][k] z[b][k]
__global__ __launch_bounds__(256) void linear_fwd_perm_out_kernel(const float* __restrict__ z, const float* __restrict__ w,
                                                                  const float* __restrict__ bias, void* __restrict__ y, int y_dtype,
                                                                  int batch, int k_in, int j_out, int pc, int pv) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= j_out) return;
    const float* wr = w + (size_t)j * k_in;
    const long long ph = phys_index(j, pc, pv);
    for (int b = 0; b < batch; ++b) {
        float s = 0.f;
        for (int k = lane; k < k_in; k += 64) s += wr[k] * z[(size_t)b * k_in + k];
        s = wave_sum(s);
        if (lane == 0) st_any(y, y_dtype, (long long)b * j_out + ph, s + (bias ? bias[j] : 0.f));
    }
}

extern "C" int vs_linear_fwd_perm_out(const float* z, const float* wgt, const float* bias, void* y, int y_dtype, int batch,
                                      int k_in, int j_out, int pc, int pv, void* stream) {
    if (!z || !wgt || !y || batch <= 0 || k_in <= 0 || j_out <= 0) return VS_EINVAL;
    if (pc > 0 && (long long)pc * pv != j_out) return VS_ESHAPE;
    hipLaunchKernelGGL(linear_fwd_perm_out_kernel, dim3((j_out + 3) / 4), dim3(256), 0, (hipStream_t)stream, z, wgt, bias, y, y_dtype, batch, k_in, j_out, pc, pv);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// gx[b][phys(k)] = sum_j gy'[b][j] W[j][k]   (gy' = gy masked by y>0 when y_for_relu given).  A workgroup = 64 values of k x 4 waves; wave w walks the
// weight rows j = w, w + 4, ... with 8 rows in flight per step and the waves' partial sums meet in LDS (fixed order).  (One thread per k walking all j_out rows
// — 16 dependent rounds of 8 loads on 108 waves — was 11.7 us for 3.5 MB of weights; before that, a dependent load per FMA: 64 us.)
template <int NB>
__global__ __launch_bounds__(256) void linear_bwd_x_kernel(const float* __restrict__ w, const float* __restrict__ gy, const float* __restrict__ yrelu,
                                                          void* __restrict__ gx, int x_dtype, int batch, int k_in, int j_out, int pc, int pv) {
    __shared__ float red[3][NB][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int k = blockIdx.x * 64 + lane;
    const bool kok = k < k_in;
    float s[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) s[b] = 0.f;
    for (int j0 = wave; j0 < j_out; j0 += 32) {
        float wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = (kok && j0 + 4 * u < j_out) ? w[(size_t)(j0 + 4 * u) * k_in + k] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + 4 * u < j_out ? j0 + 4 * u : j_out - 1;     // rows past the end carry a zero weight
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int bb = b < batch ? b : batch - 1;
                float g = gy[(size_t)bb * j_out + j];
                if (yrelu && !(yrelu[(size_t)bb * j_out + j] > 0.f)) g = 0.f;
                s[b] += g * wv[u];
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) red[wave - 1][b][lane] = s[b];
    }
    __syncthreads();
    if (wave == 0 && kok) {
        const long long ph = phys_index(k, pc, pv);
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b < batch) st_any(gx, x_dtype, (long long)b * k_in + ph, ((s[b] + red[0][b][lane]) + red[1][b][lane]) + red[2][b][lane]);
    }
}
// gw[j][k] = sum_b gy'[b][j] x[b][phys(k)] ; gb[j] = sum_b gy'[b][j]
__global__ void linear_bwd_w_kernel(const void* __restrict__ x, int x_dtype, const float* __restrict__ gy, const float* __restrict__ yrelu,
                                    float* __restrict__ gw, float* __restrict__ gb, int batch, int k_in, int j_out, int pc, int pv) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)j_out * k_in) return;
    const int j = (int)(i / k_in), k = (int)(i - (long long)j * k_in);
    const long long ph = phys_index(k, pc, pv);
    float s = 0.f, sb = 0.f;
    for (int b = 0; b < batch; ++b) {
        float g = gy[(size_t)b * j_out + j];
        if (yrelu && !(yrelu[(size_t)b * j_out + j] > 0.f)) g = 0.f;
        s += g * ld_any(x, x_dtype, (long long)b * k_in + ph);
        sb += g;
    }
    if (gw) gw[i] = s;
    if (gb && k == 0) gb[j] = sb;
}

extern "C" int vs_linear_bwd(const void* x, int x_dtype, const float* wgt, const float* gy, const float* y_for_relu, void* gx,
                             float* gw, float* gb, int batch, int k_in, int j_out, int pc, int pv, void* stream) {
    if (!wgt || !gy || batch <= 0 || k_in <= 0 || j_out <= 0) return VS_EINVAL;
    if (pc > 0 && (long long)pc * pv != k_in) return VS_ESHAPE;
    if (gx) {
        if (batch > LIN_MAXB) return VS_EINVAL;
#define LIN_BX(NB) hipLaunchKernelGGL(linear_bwd_x_kernel<NB>, dim3((k_in + 63) / 64), dim3(256), 0, (hipStream_t)stream, wgt, gy, y_for_relu, gx, x_dtype, batch, k_in, j_out, pc, pv)
        if (batch == 1) LIN_BX(1); else if (batch == 2) LIN_BX(2); else if (batch <= 4) LIN_BX(4); else if (batch <= 8) LIN_BX(8); else LIN_BX(16);
#undef LIN_BX
        VS_CHECK_LAUNCH();
    }
    if (gw || gb) {
        if (!x) return VS_EINVAL;
        const long long total = (long long)j_out * k_in;
        hipLaunchKernelGGL(linear_bwd_w_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, x_dtype, gy, y_for_relu, gw, gb, batch, k_in, j_out, pc, pv);
        VS_CHECK_LAUNCH();
    }
    return VS_OK;
}

// backward of y[b][phys(j)] = bias[j] + sum_k W[j][k] z[b][k]
__global__ __launch_bounds__(256) void linear_perm_out_bwd_z_kernel(const float* __restrict__ w, const void* __restrict__ gy, int y_dtype,
                                                                    float* __restrict__ gz, int batch, int k_in, int j_out, int pc, int pv) {
    // one workgroup per (b, k): reduce over j
    const int b = blockIdx.y, k = blockIdx.x;
    float s = 0.f;
    for (int j = threadIdx.x; j < j_out; j += 256)
        s += ld_any(gy, y_dtype, (long long)b * j_out + phys_index(j, pc, pv)) * w[(size_t)j * k_in + k];
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) gz[(size_t)b * k_in + k] = red[0] + red[1] + red[2] + red[3];
}
__global__ void linear_perm_out_bwd_w_kernel(const float* __restrict__ z, const void* __restrict__ gy, int y_dtype, float* __restrict__ gw,
                                             float* __restrict__ gb, int batch, int k_in, int j_out, int pc, int pv) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)j_out * k_in) return;
    const int j = (int)(i / k_in), k = (int)(i - (long long)j * k_in);
    const long long ph = phys_index(j, pc, pv);
    float s = 0.f, sb = 0.f;
    for (int b = 0; b < batch; ++b) {
        const float g = ld_any(gy, y_dtype, (long long)b * j_out + ph);
        s += g * z[(size_t)b * k_in + k];
        sb += g;
    }
    if (gw) gw[i] = s;
    if (gb && k == 0) gb[j] = sb;
}
extern "C" int vs_linear_perm_out_bwd(const float* z, const float* wgt, const void* gy, int y_dtype, float* gz, float* gw,
                                      float* gb, int batch, int k_in, int j_out, int pc, int pv, void* stream) {
    if (!wgt || !gy || batch <= 0 || k_in <= 0 || j_out <= 0) return VS_EINVAL;
    if (pc > 0 && (long long)pc * pv != j_out) return VS_ESHAPE;
    if (gz) {
        hipLaunchKernelGGL(linear_perm_out_bwd_z_kernel, dim3(k_in, batch), dim3(256), 0, (hipStream_t)stream, wgt, gy, y_dtype, gz, batch, k_in, j_out, pc, pv);
        VS_CHECK_LAUNCH();
    }
    if (gw || gb) {
        if (!z) return VS_EINVAL;
        const long long total = (long long)j_out * k_in;
        hipLaunchKernelGGL(linear_perm_out_bwd_w_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, gy, y_dtype, gw, gb, batch, k_in, j_out, pc, pv);
        VS_CHECK_LAUNCH();
    }
    return VS_OK;
}

// ---- reparameterisation / KL -----------------------------------------------------------------------
// one definition of the latent's arithmetic: vs_reparam_fwd and vs_reparam_philox_fwd give the same bits for the same noise
__device__ __forceinline__ float reparam_z(float mean, float sd, float noise, float scale) { return mean + noise * sd * scale; }
__global__ void reparam_fwd_kernel(const float* mean, const float* sd, const float* noise, float scale, float* z, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) z[i] = reparam_z(mean[i], sd[i], noise[i], scale);
}
__global__ void reparam_bwd_kernel(const float* gz, const float* noise, float scale, float* gmean, float* gstd, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        if (gmean) gmean[i] = gz[i];
        if (gstd) gstd[i] = gz[i] * noise[i] * scale;
    }
}
extern "C" int vs_reparam_fwd(const float* mean, const float* std_, const float* noise, float scale, float* z, long long count, void* stream) {
    if (!mean || !std_ || !noise || !z || count <= 0) return VS_EINVAL;
    hipLaunchKernelGGL(reparam_fwd_kernel, GRID1D(count), dim3(256), 0, (hipStream_t)stream, mean, std_, noise, scale, z, count);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
extern "C" int vs_reparam_bwd(const float* gz, const float* noise, float scale, float* gmean, float* gstd, long long count, void* stream) {
    if (!gz || !noise || count <= 0) return VS_EINVAL;
    hipLaunchKernelGGL(reparam_bwd_kernel, GRID1D(count), dim3(256), 0, (hipStream_t)stream, gz, noise, scale, gmean, gstd, count);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

// ---- the latent's noise, drawn on the device ------------------------------------------------------------
// A latent stream is (seed, draw), two unsigned 64-bit words.  Pair q of draw t: Philox4x32-10 under key (seed low, seed high) and counter
// (q, t low, 0x200, t high); u1, u2 and r = sqrt(-2 ln u1) as vs_aug_normal_philox forms them, in fp64; element 2q = r cos(2 pi u2), element
// 2q + 1 = r sin(2 pi u2), rounded to fp32 once.  An odd count uses the cosine of its last pair only.  One thread per pair.
__device__ __forceinline__ void latent_pair(unsigned int q, unsigned long long seed, unsigned long long draw, float& even, float& odd) {
#pragma clang fp contract(off)
    unsigned int w0, w1, w2, w3;
    vs_philox4x32_10(q, (unsigned int)draw, 0x200u, (unsigned int)(draw >> 32), (unsigned int)seed, (unsigned int)(seed >> 32), w0, w1, w2, w3);
    double r, a;
    vs_philox_box_muller(w0, w1, w2, w3, r, a);
    even = (float)(r * cos(a));
    odd = (float)(r * sin(a));
}
__global__ __launch_bounds__(256) void latent_normal_kernel(float* __restrict__ noise, long long n, unsigned long long seed, unsigned long long draw) {
    const long long pairs = (n + 1) >> 1;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < pairs; q += (long long)gridDim.x * 256) {
        float even, odd;
        latent_pair((unsigned int)q, seed, draw, even, odd);
        noise[2 * q] = even;
        if (2 * q + 1 < n) noise[2 * q + 1] = odd;
    }
}
// state[0] = seed, state[1] = draw, read from device memory by every thread: a replayed graph draws what the counter says at that launch
__global__ __launch_bounds__(256) void reparam_philox_fwd_kernel(const float* __restrict__ mean, const float* __restrict__ sd,
                                                                const unsigned long long* __restrict__ state, float scale, float* __restrict__ z,
                                                                float* __restrict__ noise_out, long long n) {
    const unsigned long long seed = state[0], draw = state[1];
    const long long pairs = (n + 1) >> 1;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < pairs; q += (long long)gridDim.x * 256) {
        float even, odd;
        latent_pair((unsigned int)q, seed, draw, even, odd);
        const long long i = 2 * q;
        noise_out[i] = even;
        z[i] = reparam_z(mean[i], sd[i], even, scale);
        if (i + 1 < n) {
            noise_out[i + 1] = odd;
            z[i + 1] = reparam_z(mean[i + 1], sd[i + 1], odd, scale);
        }
    }
}
// the launch behind the forward on the same stream: every read of state[1] above has completed when this one thread writes it
__global__ void latent_advance_kernel(unsigned long long* state) { state[1] = state[1] + 1ull; }

static inline int latent_count_ok(long long count) { return count > 0 && count < (1LL << 31); }
extern "C" int vs_latent_normal_philox(float* noise, long long count, unsigned long long seed, unsigned long long draw, void* stream) {
    if (!noise) return VS_EINVAL;
    if (!latent_count_ok(count)) return VS_ESHAPE;
    if ((uintptr_t)noise & 3) return VS_EALIGN;
    hipLaunchKernelGGL(latent_normal_kernel, GRID1D((count + 1) / 2), dim3(256), 0, (hipStream_t)stream, noise, count, seed, draw);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
extern "C" int vs_reparam_philox_fwd(const float* mean, const float* std_, const unsigned long long* state, float scale, float* z, float* noise_out,
                                     long long count, void* stream) {
    if (!mean || !std_ || !state || !z || !noise_out) return VS_EINVAL;
    if (!latent_count_ok(count)) return VS_ESHAPE;
    if (((uintptr_t)state & 7) || (((uintptr_t)mean | (uintptr_t)std_ | (uintptr_t)z | (uintptr_t)noise_out) & 3)) return VS_EALIGN;
    hipLaunchKernelGGL(reparam_philox_fwd_kernel, GRID1D((count + 1) / 2), dim3(256), 0, (hipStream_t)stream, mean, std_, state, scale, z, noise_out,
                       count);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
extern "C" int vs_latent_advance(unsigned long long* state, void* stream) {
    if (!state) return VS_EINVAL;
    if ((uintptr_t)state & 7) return VS_EALIGN;
    hipLaunchKernelGGL(latent_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
    VS_CHECK_LAUNCH();
    return VS_OK;
}

__global__ __launch_bounds__(256) void kl_fwd_kernel(const float* __restrict__ mean, const float* __restrict__ sd, float* __restrict__ out, int batch, int dim) {
    // single workgroup: total = sum_b 0.5*(sum sd^2 + sum mean^2 - 2 sum log(sd+1e-5)) / batch
    double s = 0.0;
    for (int i = threadIdx.x; i < batch * dim; i += 256) {
        const float m = mean[i], d = sd[i];
        s += 0.5 * ((double)d * d + (double)m * m - 2.0 * (double)logf(d + 0.00001f));
    }
    __shared__ double red[4];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (float)((red[0] + red[1] + red[2] + red[3]) / batch);
}
__global__ void kl_bwd_kernel(const float* mean, const float* sd, const float* gout, float* gmean, float* gstd, int batch, int dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * dim) return;
    const float g = gout[0] / batch;
    if (gmean) gmean[i] = g * mean[i];
    if (gstd) gstd[i] = g * (sd[i] - 1.f / (sd[i] + 0.00001f));
}
extern "C" int vs_kl_fwd(const float* mean, const float* std_, float* out, int batch, int dim, void* stream) {
    if (!mean || !std_ || !out || batch <= 0 || dim <= 0) return VS_EINVAL;
    hipLaunchKernelGGL(kl_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, mean, std_, out, batch, dim);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
extern "C" int vs_kl_bwd(const float* mean, const float* std_, const float* gout, float* gmean, float* gstd, int batch, int dim, void* stream) {
    if (!mean || !std_ || !gout || batch <= 0 || dim <= 0) return VS_EINVAL;
    hipLaunchKernelGGL(kl_bwd_kernel, dim3((batch * dim + 255) / 256), dim3(256), 0, (hipStream_t)stream, mean, std_, gout, gmean, gstd, batch, dim);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
