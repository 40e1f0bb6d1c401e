// The library's properties (build, version, statistics layout, error strings) and the zero fill.  The streaming kernels of the training step live by subject
// in softmax.hip (dropout, softmax, label prep), latent.hip (VAE bottleneck), loss.hip (Dice, BCE) and optim.hip (multi-tensor optimiser).
#include "common.h"

// ---- deterministic build (common.h): a property of the library, queried by the package ----------------------------------------------
extern "C" int vs_get_deterministic(void) { return VS_DET_BUILD; }

extern "C" int vs_version(void) { return VS_VERSION; }
extern "C" int vs_stat_slots(void) { return VS_STAT_SLOTS; }
extern "C" int vs_stat_interleaved(void) { return VS_STAT_INTERLEAVE; }
extern "C" const char* vs_strerror(int code) {
    switch (code) {
        case VS_OK: return "ok";
        case VS_EINVAL: return "invalid argument (null pointer or non-positive size)";
        case VS_ESHAPE: return "unsupported shape (channels must be 8, 16 or a multiple of 32 up to 512; even dims for stride 2; batch <= 16 for wgrad)";
        case VS_EDTYPE: return "unsupported dtype (VS_F32, VS_BF16 or VS_F16)";
        case VS_EWORKSPACE: return "workspace too small";
        case VS_EALIGN: return "pointer not 16-byte aligned";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown libvaeseg error";
    }
}

// ---- zero fill (statistics arenas): a kernel of this library, not a memset node (common.h: vs_zero_async) -------------------------
__global__ __launch_bounds__(256) void zero_fill_kernel(u32x4* __restrict__ p, long long frags) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < frags; i += (long long)gridDim.x * 256) p[i] = u32x4{0u, 0u, 0u, 0u};
}
extern "C" int vs_zero_fill(void* p, long long bytes, void* stream) {
    if (!p || bytes <= 0) return VS_EINVAL;
    if (((uintptr_t)p & 15) || (bytes & 15)) return VS_EALIGN;
    const long long frags = bytes / 16;
    long long blocks = (frags + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (u32x4*)p, frags);
    VS_CHECK_LAUNCH();
    return VS_OK;
}
