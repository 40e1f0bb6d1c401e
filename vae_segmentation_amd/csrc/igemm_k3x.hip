// fp32 parity mode, 3x3x3 convolutions on the bf16 matrix cores through exact three-limb operand splitting (igemm_k3x.h)
#include <stdlib.h>
#include "igemm_dispatch.h"
#include "igemm_k3x.h"

// conv_api.hip asks these before it launches; the dispatcher below guards with them.  p, ck, mt as the dispatcher gets them (p.nch = C / ck; geometry only).
// fused apply (FA): k3xt_kernel for the 8 -> 8 layers, k3x_kernel<8, 16, RAW, .., MULTI, FA> for 16 -> 16 in 8-channel chunks; waves 1 .. 3 build the
// per-(n, c) tables, at most 192 entries
int k3x_fa_supported(const G1Params& p, int ck, int mt) {
    if (ck != 8 || p.N * p.C > 192) return 0;
    if (p.C == 8 && p.M == 8 && p.nch == 1 && vs_k3x_toeplitz(8, 8, 27)) return 1;
    return mt == 16 && p.nch == 2 && p.C == 16 && p.M == 16;
}
// epilogue apply (EA): k3x_kernel<8, 16, .., MULTI, .., EA> — several 8-channel chunks, 16-row workgroups, all wgs of them resident together
int k3x_ea_supported(const G1Params& p, int ck, int mt, long long wgs) { return ck == 8 && p.nch >= 2 && mt == 16 && wgs <= k3x_ea_max_wgs(p.N, p.C, p.M); }

// ck = min(C, 16); mt = 16 or 32 rows per workgroup
int g1_dispatch_k3_x3(const G1Params& p, int ck, int mt, int epi, int tiles, int row_tiles, hipStream_t s) {
    if (p.fa_x != nullptr && (epi != EPI_RAW || !k3x_fa_supported(p, ck, mt))) return VS_ESHAPE;
    if (p.ea_sync != nullptr && (epi != EPI_RAW || p.fa_x || !p.sums || !k3x_ea_supported(p, ck, mt, (long long)tiles * row_tiles))) return VS_ESHAPE;
    // 8 stored input and output channels (the full-resolution layers; out_block's two logits are stored in 8): Toeplitz rows, weights packed to match
    if (ck == 8 && p.C == 8 && p.M == 8 && p.nch == 1 && vs_k3x_toeplitz(8, 8, 27))
        return epi == EPI_SOFTMAX2 ? k3xt_launch<EPI_SOFTMAX2>(p, s) : k3xt_launch<EPI_RAW>(p, s);
    if (epi == EPI_SOFTMAX2) {
        if (ck != 8 || mt != 16 || p.nch != 1) return VS_ESHAPE;      // out_block: 8 stored channels -> 2 logits
        return k3x_launch<8, 16, EPI_SOFTMAX2, false>(p, tiles, row_tiles, s);
    }
    if (ck == 8) {
        if (p.nch == 1) {
            if (mt == 16) return k3x_launch<8, 16, EPI_RAW, false>(p, tiles, row_tiles, s);
            if (mt == 32) return k3x_launch<8, 32, EPI_RAW, false>(p, tiles, row_tiles, s);
        } else {                                          // VS_K3X_CK=8: 8-channel chunks for every layer (two workgroups per CU)
            if (mt == 16 && !p.fa_x && vs_cfg().k3_short_tiles) {
                // the under-filled launches of the 12^3-class levels (<= 128 workgroups): 4 x 2 x 16 tiles, 4 x 1 x 16 where that still leaves <= 128 (igemm_k3_h16.inc)
                const long long zx = (long long)p.N * ((p.D + 3) / 4) * p.txn;
                // (4 x 2 x 16 for EVERY launch — two waves per SIMD instead of one — measured slower: fp32 step 5.748 -> 5.846 ms; the halo grows 2.5 x -> 3.4 x)
                if ((long long)tiles * row_tiles <= 128 && zx * ((p.H + 1) / 2) * row_tiles <= 256) {
                    if (vs_cfg().k3_short_tiles >= 2 && zx * ((p.H + 1) / 2) * row_tiles <= 128 && zx * p.H * row_tiles <= 256)
                        return k3x_launch_short<8, 16, true, 1>(p, tiles, row_tiles, s);
                    return k3x_launch_short<8, 16, true, 2>(p, tiles, row_tiles, s);
                }
            }
            if (mt == 16 && p.ea_sync != nullptr) return k3x_launch_short<8, 16, true, 4>(p, tiles, row_tiles, s);
            if (mt == 16) return k3x_launch<8, 16, EPI_RAW, true>(p, tiles, row_tiles, s);
            if (mt == 32) return k3x_launch<8, 32, EPI_RAW, true>(p, tiles, row_tiles, s);
        }
        return VS_ESHAPE;
    }
    if (ck == 16) {
        if (p.nch == 1) {
            if (mt == 16) return k3x_launch<16, 16, EPI_RAW, false>(p, tiles, row_tiles, s);
            if (mt == 32) return k3x_launch<16, 32, EPI_RAW, false>(p, tiles, row_tiles, s);
        } else {
            if (mt == 16) return k3x_launch<16, 16, EPI_RAW, true>(p, tiles, row_tiles, s);
            if (mt == 32) return k3x_launch<16, 32, EPI_RAW, true>(p, tiles, row_tiles, s);
        }
    }
    return VS_ESHAPE;
}
