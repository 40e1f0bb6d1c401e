// shared by igemm_k3_bf16.hip and igemm_k3_f16.hip: the dispatch of the 16-bit 3x3x3 kernels, templated on the storage type
#include "igemm_dispatch.h"
#include "igemm_k3b.h"
#include "igemm_k3t.h"
#include "igemm_k3s.h"
#include "igemm_k3tw.h"

#define K3B_CASE(CKV, MTV)                                                                              \
    if (ck == CKV && mt == MTV)                                                                          \
        return p.sums ? k3b_launch<T, CKV, MTV, EPI_RAW, true>(p, tiles, row_tiles, s)                   \
                      : k3b_launch<T, CKV, MTV, EPI_RAW, false>(p, tiles, row_tiles, s);

// 16-bit (bf16 / fp16) 3x3x3 convolutions run k3b_kernel with 16- or 32-row tiles (a 64-row weight block does not fit LDS next to the
// halo tile): a 64-row request from pick_mt() is served as twice as many 32-row workgroups.
// does dispatch_k3_h16 have a fused-apply (FA) kernel for this backward-data launch?  (mirrors the routing below; p: geometry only, lazy_in: the launch has fused sums)
static inline bool k3_h16_fa_supported(const G1Params& p, int ck, int mt, bool lazy_in) {
    if (ck == 32) return false;                            // the 24^3 / 12^3 levels keep the standalone apply (a fused k3b<32,...> measured slower: round 4;
                                                           // so did 16-channel half stages of it: profiles/r05_ab_fused_apply_half_stages.json)
    if (ck == 8 && p.C == 8 && p.M == 8) return true;                          // k3t
    if (mt == 16 && k3b_use_tall(p)) return ck == 16;                          // k3b<16,16,*,8>
    if (mt == 64) mt = 32;
    return (ck == 16 && mt == 16) || (ck == 8 && mt == 16 && !lazy_in) || (ck == 16 && mt == 32 && !lazy_in);
}
// ... and an epilogue-apply (EA) kernel, k3b_kernel<32, 16, .., EA>, for one of wgs workgroups (with fused sums, without FA)?  32-channel chunks, 16-row tiles, every
// workgroup resident together (igemm_k3b.h).  Volumes up to 6^3 are k3s_kernel's and stay refused where vs_config.k3_small = 0 hands them to k3b_kernel.
static inline bool k3_h16_ea_supported(const G1Params& p, int ck, int mt, long long wgs) {
    const bool small = (long long)(p.D + 2) * (p.H + 2) * (p.W + 2) <= 512 && p.C <= 1024;
    return ck == 32 && mt == 16 && !small && wgs <= k3b_ea_max_wgs(p.N, p.C, p.M);
}

template <typename T>
static int dispatch_k3_h16(const G1Params& p, int ck, int mt, int epi, int tiles, int row_tiles, hipStream_t s) {
    if (p.fa_x != nullptr && (epi != EPI_RAW || !k3_h16_fa_supported(p, ck, mt, p.sums != nullptr))) return VS_ESHAPE;     // never run an un-applied gradient through a kernel that ignores fa_x
    if (p.wg_ws != nullptr || p.sm_prob != nullptr) {     // backward-data with the fused weight gradient / softmax backward (conv_api.hip vs_conv_k3_bwd_data_wgrad, vs_conv_k3_softmax2_bwd_data): 8 -> 8 only
        if (!(ck == 8 && p.C == 8 && p.M == 8 && epi == EPI_RAW && p.sums)) return VS_ESHAPE;
        return k3tw_launch<T>(p, s);
    }
    // Short tiles (4 x 2 x 16; round 6): a 12^3 x 64 layer is 72 workgroups of 4 x 4 x 16 tiles — 72 of 256 CUs, each walking a serial chain of staging, MFMA and epilogue.
    // Where the launch has at most 128 workgroups and twice as many still fit one per CU, the tiles are halved in y: twice the CUs, half the MFMA phase and 2/3 of the
    // staging per workgroup (vs_config.k3_short_tiles = 0: off).
    const bool short_tiles = vs_cfg().k3_short_tiles && ck == 32 && mt == 16 && epi == EPI_RAW && !p.fa_x && !k3s_takes(p, ck) &&
                             (long long)tiles * row_tiles <= 128 && (long long)p.N * ((p.D + 3) / 4) * ((p.H + 1) / 2) * p.txn * row_tiles <= 256;
    // ... and once more (4 x 1 x 16) where even the halved tiles leave at most 128 workgroups (the 8^3 / 16^3 levels of configs[3])
    const bool shorter_tiles = short_tiles && vs_cfg().k3_short_tiles >= 2 &&
                               (long long)p.N * ((p.D + 3) / 4) * ((p.H + 1) / 2) * p.txn * row_tiles <= 128 && (long long)p.N * ((p.D + 3) / 4) * p.H * p.txn * row_tiles <= 256;
    if (p.ea_sync != nullptr) {                           // backward-data + fused sums + the apply in the epilogue (igemm_k3b.h EA): the 32-channel chunks, 16-row tiles
        if (epi != EPI_RAW || p.fa_x || !p.sums || !k3_h16_ea_supported(p, ck, mt, (long long)tiles * row_tiles)) return VS_ESHAPE;
        if (shorter_tiles) return k3b_launch_t<T, 32, 16, EPI_RAW, true, 1, false, false, true>(p, tiles, row_tiles, s);
        if (short_tiles) return k3b_launch_t<T, 32, 16, EPI_RAW, true, 2, false, false, true>(p, tiles, row_tiles, s);
        return k3b_launch_t<T, 32, 16, EPI_RAW, true, 4, false, false, true>(p, tiles, row_tiles, s);
    }
    if (ck == 8 && p.C == 8 && p.M == 8) {                // the 8-channel full-resolution layers: Toeplitz kernel (weights packed to match)
        if (epi == EPI_SOFTMAX2) return k3t_launch<T, EPI_SOFTMAX2, false, 8>(p, s);
        return p.sums ? k3t_launch<T, EPI_RAW, true, 8>(p, s) : k3t_launch<T, EPI_RAW, false, 8>(p, s);
    }
    if (epi == EPI_RAW && k3s_takes(p, ck))                 // the small volumes of the deep levels: flattened columns, waves split the taps
        return p.sums ? k3s_launch<T, true>(p, s) : k3s_launch<T, false>(p, s);
    const bool tall = mt == 16 && ck < 32 && k3b_use_tall(p);
    if (epi == EPI_SOFTMAX2) return VS_ESHAPE;           // out_block is an 8-channel layer (above)
    if (tall) {
        if (ck == 8) return p.sums ? k3b_launch<T, 8, 16, EPI_RAW, true, 8>(p, tiles, row_tiles, s) : k3b_launch<T, 8, 16, EPI_RAW, false, 8>(p, tiles, row_tiles, s);
        return p.sums ? k3b_launch<T, 16, 16, EPI_RAW, true, 8>(p, tiles, row_tiles, s) : k3b_launch<T, 16, 16, EPI_RAW, false, 8>(p, tiles, row_tiles, s);
    }
    if (shorter_tiles) return p.sums ? k3b_launch<T, 32, 16, EPI_RAW, true, 1>(p, tiles, row_tiles, s) : k3b_launch<T, 32, 16, EPI_RAW, false, 1>(p, tiles, row_tiles, s);
    if (short_tiles) return p.sums ? k3b_launch<T, 32, 16, EPI_RAW, true, 2>(p, tiles, row_tiles, s) : k3b_launch<T, 32, 16, EPI_RAW, false, 2>(p, tiles, row_tiles, s);
    if (mt == 64) { mt = 32; row_tiles *= 2; }
    K3B_CASE(8, 16) K3B_CASE(8, 32) K3B_CASE(16, 16) K3B_CASE(16, 32) K3B_CASE(32, 16) K3B_CASE(32, 32)
    return VS_ESHAPE;
}

