// The launches vs_conv_wgrad_multi WOULD make, recorded on a machine without a device: csrc/wgrad.hip's host side as a program of its own.
//
//   python tools/wgrad_plan_table.py --dump-lists lists.bin
//   hipcc --cuda-host-only --offload-arch=gfx950 -O1 -std=c++17 -rdynamic -Wl,--unresolved-symbols=ignore-in-object-files -I TREE/vae_segmentation_amd/csrc \
//         tools/wgrad_trace.hip TREE/vae_segmentation_amd/csrc/config.hip -o trace -ldl
//   ./trace lists.bin > launches.txt            (add -fsanitize=address,undefined to check the host code as well)
//
// Built once from the tree before a change to the host code and once from the tree after it, the two outputs must be the same file: per call the workspace
// size and the returned code, per launch the kernel, grid, block, LDS bytes and every field of the argument struct, and every hipFuncSetAttribute in between.
// hipLaunchKernelGGL, hipFuncSetAttribute and the launch check are replaced by recorders before wgrad.hip is included; nothing reaches the HIP runtime, and the
// descriptors' addresses (and the workspace's) are fakes that are printed, never read.
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdio.h>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"                     // first, under its #pragma once, so that its launch check can be replaced below

static void trace_kernel(const void* kern) {
    Dl_info info;
    std::string name = "?";
    if (dladdr(kern, &info) && info.dli_sname) {
        int status = 0;
        char* d = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
        name = status == 0 && d ? d : info.dli_sname;
        free(d);
    }
    printf("%s", name.c_str());
}
struct G3Params; struct G3Group; struct G3RedGroup; struct G3BiasGroup;
static void trace_arg(const G3Params& p);
static void trace_arg(const G3Group& g);
static void trace_arg(const G3RedGroup& g);
static void trace_arg(const G3BiasGroup& g);
template <typename A, typename = typename std::enable_if<std::is_arithmetic<A>::value || std::is_pointer<A>::value>::type>
static void trace_arg(const A& a) {
    if constexpr (std::is_pointer<A>::value) printf("  arg %p\n", (const void*)a);
    else if constexpr (std::is_floating_point<A>::value) printf("  arg %a\n", (double)a);
    else printf("  arg %lld\n", (long long)a);
}
template <typename K, typename... A>
static void trace_launch(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
    printf(" launch ");
    trace_kernel((const void*)kern);
    printf(" grid %u %u %u block %u %u %u lds %zu stream %p\n", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds, (void*)stream);
    (trace_arg(args), ...);
}
static hipError_t trace_attr(const void* kern, hipFuncAttribute attr, int value) {
    printf(" attribute ");
    trace_kernel(kern);
    printf(" %d = %d\n", (int)attr, value);
    return hipSuccess;
}
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, grid, block, lds, stream, ...) trace_launch(kern, grid, block, lds, stream, __VA_ARGS__)
#define hipFuncSetAttribute(kern, attr, value) trace_attr(kern, attr, value)
#undef VS_CHECK_LAUNCH
#define VS_CHECK_LAUNCH() do { } while (0)

#include "wgrad.hip"

static void trace_arg(const G3Params& p) {
    printf("   P %p %p Q %p %p ws %p N %d P grid %d %d %d Q grid %d %d %d ch %d %d blocks %d %d ksplit %d tiles %d %d %d %d eps %a inv %a %a up_co %d fd %u %u %u %u variant %d mp %d\n",
           p.P, (const void*)p.P_stats, p.Q, (const void*)p.Q_stats, (void*)p.ws, p.N, p.Dp, p.Hp, p.Wp, p.Dq, p.Hq, p.Wq, p.Mch, p.Cch, p.mbn, p.cbn, p.ksplit, p.total_tiles,
           p.tiles_per_sample, p.tyn, p.txn, (double)p.eps, p.inv_cnt_p, p.inv_cnt_q, p.up_co, p.fd_m[0], p.fd_m[1], p.fd_m[2], p.fd_s, p.variant, p.mp);
}
static void trace_arg(const G3Group& g) {
    printf("  G3Group n %d xcd %d wg_start", g.n, g.xcd);
    for (int j = 0; j <= G3_GROUP_MAX; ++j) printf(" %d", g.wg_start[j]);
    printf("\n");
    for (int j = 0; j < G3_GROUP_MAX; ++j) trace_arg(g.p[j]);              // all of them: the entries past n are part of the argument too
}
static void trace_arg(const G3RedGroup& g) {
    printf("  G3RedGroup n %d blk_start", g.n);
    for (int j = 0; j <= G3_RED_MAX; ++j) printf(" %d", g.blk_start[j]);
    printf("\n");
    for (int j = 0; j < G3_RED_MAX; ++j) {
        const G3RedDesc& d = g.d[j];
        printf("   ws %p dw %p real %d %d blocks %d %d nslabs %d cb %d ntaps %d ncb %d kind %d parts %d swap %d\n", (const void*)d.ws, (void*)d.dw, d.m_real, d.c_real, d.mbn, d.cbn,
               d.nslabs, d.cb, d.ntaps, d.ncb, d.kind, d.parts, d.swap);
    }
}
static void trace_arg(const G3BiasGroup& g) {
    printf("  G3BiasGroup n %d blk_start", g.n);
    for (int j = 0; j <= G3_BIAS_MAX; ++j) printf(" %d", g.blk_start[j]);
    printf("\n");
    for (int j = 0; j < G3_BIAS_MAX; ++j) {
        const G3BiasDesc& d = g.d[j];
        printf("   g %p part %p rows %lld ch %d %d nblk %d\n", d.g, (void*)d.part, d.rows, d.c_ch, d.c_real, d.nblk);
    }
}

// A host-only compilation has no device code to register: the registration calls of the kernels' host stubs end here, not in the HIP runtime
// (the code object they name is the one symbol the link line lets stay unresolved).
extern "C" void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
extern "C" void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned int, void*, void*, void*, void*, int*) {}
extern "C" void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
extern "C" void __hipUnregisterFatBinary(void**) {}

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    int entries = 0;
    if (!f || fread(&entries, 4, 1, f) != 1) { fprintf(stderr, "usage: %s LISTS (from tools/wgrad_plan_table.py --dump-lists)\n", argv[0]); return 2; }
    char* const workspace = (char*)0x7e0000000000ull;                 // a fake like the descriptors' addresses
    for (int e = 0; e < entries; ++e) {
        int head[3];
        if (fread(head, 4, 3, f) != 3 || head[2] != vs_config_bytes()) { fprintf(stderr, "entry %d: bad header\n", e); return 2; }
        vs_config cfg;
        std::vector<vs_wgrad_desc> descs(head[1]);
        if (fread(&cfg, sizeof(cfg), 1, f) != 1 || fread(descs.data(), sizeof(vs_wgrad_desc), descs.size(), f) != descs.size()) { fprintf(stderr, "entry %d: short\n", e); return 2; }
        if (vs_set_config(&cfg)) { fprintf(stderr, "entry %d: configuration refused\n", e); return 2; }
        const size_t bytes = vs_conv_wgrad_multi_workspace_bytes(descs.data(), head[1], head[0]);
        printf("call %d dtype %d descriptors %d workspace %zu\n", e, head[0], head[1], bytes);
        const int rc = vs_conv_wgrad_multi(descs.data(), head[1], workspace, bytes, head[0], 1e-5f, nullptr);
        printf(" returned %d\n", rc);
        if (bytes >= 512) {                                            // and with a workspace 256 bytes short: what is launched before the refusal
            const int rc2 = vs_conv_wgrad_multi(descs.data(), head[1], workspace, bytes - 256, head[0], 1e-5f, nullptr);
            printf(" 256 bytes short: returned %d\n", rc2);
        }
    }
    fclose(f);
    return 0;
}
