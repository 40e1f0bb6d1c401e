// C-ABI launchers of the implicit-GEMM convolutions (forward / backward-data).
// Planning is apart from launching: plan_gather / plan_scatter turn the VALUES of a launch (ConvAsk: shape, kind, dtype, which optional parts it has) into a
// ConvPlan — geometry, tiling, the status code the shape earns, which fused forms exist for it.  A launcher plans once, adds its pointers to the plan's
// G1Params and dispatches; a *_supported query reads the same plan.  Which kernel carries which form is asked of the dispatch units' own predicates.
#include <stdlib.h>
#include "igemm_dispatch.h"

int g1_dispatch_k3_f32(const G1Params& p, int ck, int mt, int epi, int tiles, int row_tiles, hipStream_t s);
int g1_dispatch_k3_bf16(const G1Params& p, int ck, int mt, int epi, int tiles, int row_tiles, hipStream_t s);
int g1_dispatch_k3_f16(const G1Params& p, int ck, int mt, int epi, int tiles, int row_tiles, hipStream_t s);
int g1_dispatch_k3_x3(const G1Params& p, int ck, int mt, int epi, int tiles, int row_tiles, hipStream_t s);
// is there a fused-apply (FA) / epilogue-apply (EA, with fused sums and without FA) kernel for an already tiled 3x3x3 backward-data launch of wgs workgroups?
int g1_k3_fa_supported(const G1Params& p, int ck, int mt, int lazy_in);                // igemm_k3_bf16.hip: the same for both 16-bit storage types
int g1_k3_ea_supported(const G1Params& p, int ck, int mt, long long wgs);
int k3x_fa_supported(const G1Params& p, int ck, int mt);                               // igemm_k3x.hip: the limb kernels of the fp32 parity mode
int k3x_ea_supported(const G1Params& p, int ck, int mt, long long wgs);
int k3tw_slab_count(int n, int d, int h, int w);                                       // igemm_k3_bf16.hip: workgroups (= slabs) of a k3tw_kernel launch
int k2s2_scatter8_launch(const G1Params& p, int dtype, hipStream_t stream);            // k2s2_scatter8.hip

// fp32 parity mode: the 3x3x3 convolutions run on the bf16 matrix cores through exact three-limb operand splitting (igemm_k3x.h); their packed
// weights are VS_F32X3 images (pack.hip).  VS_F32_LIMBS=0 keeps the exact-f32 MFMA kernels (igemm_k3.h) and the plain fp32 images.
extern "C" int vs_conv_k3_f32_limbs(int d, int h, int w, int c_in) {
    const int on = vs_cfg().f32_limbs;
    if (!on) return 0;
    // volumes up to 6^3 with C a multiple of 32 stay on k3s_kernel<float> (igemm_k3s.h: the whole padded sample in LDS, the waves split the taps): a
    // 4x4x16 tile is mostly padding there and the limb kernel would walk C / 16 chunk stages per workgroup (3^3 x 256: 92 us against 26)
    const int small = vs_cfg().k3_small;
    if (small && c_in % 32 == 0 && c_in <= 1024 && (long long)(d + 2) * (h + 2) * (w + 2) <= 512) return 0;
    return 1;
}

// channel chunk and row tile as a dispatcher gets them
struct ConvTiles { int ck, mt, row_tiles; bool limbs; };

// ... of a 3x3x3 launch; sets p.nch to match.  The fp32 parity mode re-plans both for the limb kernels.
static ConvTiles k3_tiles(G1Params& p, int dtype, int ck, int mt, int rows16, long long tiles) {
    ConvTiles t = {ck, mt, rows16 / mt, false};
    p.nch = p.C / ck;
    if (dtype != VS_F32 || !vs_conv_k3_f32_limbs(p.D, p.H, p.W, p.C)) return t;
    t.limbs = true;
    t.ck = vs_k3x_ck(p.C);
    p.nch = p.C / t.ck;
    // 32-row workgroups (B fragments shared by two row blocks) when that still fills the chip; chunks of 16 channels with a 32-row weight block
    // fill the 160 KB of LDS exactly, so the per-(n,c) tables must be small
    t.mt = (rows16 % 32 == 0 && tiles * (rows16 / 32) >= 256 && (t.ck == 8 || (size_t)2 * p.N * (p.C + p.M) * sizeof(float) <= 3000)) ? 32 : 16;
    t.row_tiles = rows16 / t.mt;
    return t;
}

static int dispatch_k3(const G1Params& p, int dtype, const ConvTiles& t, int epi, int tiles, hipStream_t s) {
    if (t.limbs) return g1_dispatch_k3_x3(p, t.ck, t.mt, epi, tiles, t.row_tiles, s);
    if (dtype == VS_F32) return g1_dispatch_k3_f32(p, t.ck, t.mt, epi, tiles, t.row_tiles, s);
    if (dtype == VS_BF16) return g1_dispatch_k3_bf16(p, t.ck, t.mt, epi, tiles, t.row_tiles, s);
    return g1_dispatch_k3_f16(p, t.ck, t.mt, epi, tiles, t.row_tiles, s);
}

static int pick_mt(int rows16, long long tiles) {
    // largest row tile that still leaves >= VS_MT_MIN_WGS workgroups; 16 when the layer is too small for that.
    // (more rows per wave = more MFMAs per B fragment read from LDS, fewer workgroups)
    // 1024 since round 5 (256 before; same-box A/B with the round's kernels, profiles/r05_ab_mt_min_wgs_*.json: 96^3 2.416 -> 2.406 ms, 160^3 6.03 -> 6.00, fp32 mode
    // 6.169 -> 6.148; 128 -> 2.456): the full-resolution stride-2 / transposed launches run 32-row workgroups, twice as many, instead of 64-row ones
    const int min_wgs = vs_cfg().mt_min_wgs;
    const int cands[3] = {64, 32, 16};
    for (int i = 0; i < 3; ++i) {
        const int mt = cands[i];
        if (rows16 % mt) continue;
        if (tiles * (rows16 / mt) >= min_wgs || mt == 16) return mt;
    }
    return 16;
}

// widest channel count of the conv stack (input or output): the 512-channel layers of the wide models (n_fmaps [16, .., 512]) run the per-layer kernels only
#define VS_MAX_CHANNELS 512
// the fused / epilogue-apply / composed / chain paths were sized for the default widths and decline anything wider (ops.py takes the per-layer path)
static inline bool wide_layer(int c_in, int m_out) { return c_in > 256 || m_out > 256; }

// What the input's shape earns, in the order the C ABI reports it.  A launcher's alignment check has its place in that order (misaligned); a planner has no pointers.
static int shape_status(int n, int d, int h, int w_, int c_in, int dtype, bool misaligned = false) {
    if (n <= 0 || d <= 0 || h <= 0 || w_ <= 0) return VS_ESHAPE;
    if (!(c_in == 8 || c_in == 16 || (c_in % 32 == 0 && c_in > 0 && c_in <= VS_MAX_CHANNELS))) return VS_ESHAPE;
    if (!vs_dtype_ok(dtype)) return VS_EDTYPE;
    if (misaligned) return VS_EALIGN;
    return (double)n * d * h * w_ * c_in >= 2147483648.0 ? VS_ESHAPE : VS_OK;      // kernels index activations with 32-bit element offsets
}

static int check_common(const void* x, const void* w, int n, int d, int h, int w_, int c_in, int dtype) {
    if (!x || !w) return VS_EINVAL;
    return shape_status(n, d, h, w_, c_in, dtype, ((uintptr_t)x & 15) || ((uintptr_t)w & 15));
}

// a launch without its tensors.  kind: VS_CONV_K3 / VS_CONV_K2S2 (plan_gather), VS_CONV_T2S2 (plan_scatter); parts: the optional ones it has —
// input statistics, a bias, fused IN-backward sums, the fused apply, the fused weight gradient, the epilogue apply
enum { X_STATS = 1, BIAS = 2, SUMS = 4, FA = 8, WGRAD = 16, EA = 32 };
struct ConvAsk { int n, d, h, w, c_in, m_out, kind, dtype, parts; };

struct ConvPlan {
    ConvAsk ask;
    G1Params g;                   // the geometry part; every pointer null
    ConvTiles t;
    long long tiles;
    int status;                   // VS_OK: a kernel takes this launch with every part it asks for
    bool fa_ok, ea_ok, wg_ok;     // the fused-apply / epilogue-apply / fused-weight-gradient form exists for this shape (the other parts of the ask as given)
    bool stream8;                 // stride-2 scatter: the streaming 8 -> 8 kernel goes first
};

// g1_kernel's epilogue apply (igemm.h: the stride-2 kinds, any storage type): 16-row workgroups, all wgs of the launch resident together — one per CU is certain
// (up to 256 VGPRs + AGPRs)
static void g1_ea_plan(ConvPlan& pl, long long wgs) {
    pl.ea_ok = pl.t.mt == 16 && wgs <= 256;
    if (pl.ask.parts & EA) pl.g.ea_items = pl.g.tiles_per_sample * pl.t.row_tiles;
}

// what both planners start from: the status of the shape, then the fields every kind fills alike.  rows: those of the packed weight
static ConvPlan plan_begin(const ConvAsk& a, int rows) {
    ConvPlan pl{};
    pl.ask = a;
    pl.status = shape_status(a.n, a.d, a.h, a.w, a.c_in, a.dtype);
    if (!pl.status && (a.m_out <= 0 || a.m_out % 8)) pl.status = VS_EINVAL;
    if (!pl.status && a.m_out > VS_MAX_CHANNELS) pl.status = VS_ESHAPE;
    if (pl.status) return pl;
    G1Params& p = pl.g;
    p.N = a.n; p.D = a.d; p.H = a.h; p.W = a.w;
    p.C = a.c_in; p.M = a.m_out;
    p.rb_total = (rows + 15) / 16;
    pl.t.ck = a.c_in < 32 ? a.c_in : 32;
    p.nch = a.c_in / pl.t.ck;
    p.inv_count_in = 1.0 / ((double)a.d * a.h * a.w);
    return pl;
}

// VS_CONV_K3 / VS_CONV_K2S2
static ConvPlan plan_gather(const ConvAsk& a) {
    ConvPlan pl = plan_begin(a, a.m_out);
    const bool k3 = a.kind == VS_CONV_K3, sums = a.parts & SUMS, fa = a.parts & FA, ea = a.parts & EA;
    if (!pl.status && !k3 && a.kind != VS_CONV_K2S2) pl.status = VS_EINVAL;
    if (!pl.status && wide_layer(a.c_in, a.m_out) && (a.parts & (EA | FA | WGRAD))) pl.status = VS_ESHAPE;
    if (!pl.status && !k3 && ((a.d | a.h | a.w) & 1)) pl.status = VS_ESHAPE;
    if (pl.status) return pl;
    G1Params& p = pl.g;
    const int ck = pl.t.ck;
    if (k3) {                                              // the column grid is the input grid, walked in 4 x 4 x 16 tiles
        p.Do = a.d; p.Ho = a.h; p.Wo = a.w;
        p.tyn = (a.h + 3) / 4; p.txn = (a.w + 15) / 16;
        p.tiles_per_sample = ((a.d + 3) / 4) * p.tyn * p.txn;
    } else {
        p.Do = a.d / 2; p.Ho = a.h / 2; p.Wo = a.w / 2;
        p.tiles_per_sample = vs_ceil_div((long long)p.Do * p.Ho * p.Wo, 256);
        // few workgroups and several 32-channel chunks (the deep stride-2 convs: 8-32 workgroups, one memory round trip per chunk each):
        // 64-voxel column tiles whose four waves split the chunks (g1_kernel, splitw)
        if (ck == 32 && p.nch >= 2 && (long long)p.tiles_per_sample * a.n * p.rb_total <= 64) {
            p.tiles_per_sample = vs_ceil_div((long long)p.Do * p.Ho * p.Wo, 64);
            p.tyn = 64;
        }
    }
    p.inv_count_out = 1.0 / ((double)p.Do * p.Ho * p.Wo);
    pl.tiles = (long long)p.tiles_per_sample * a.n;
    const int rows16 = p.rb_total * 16;
    int mt = (!k3 && p.tyn == 64) ? 16 : pick_mt(rows16, pl.tiles);
    // fused apply on 32-channel chunks: every row-block workgroup of a tile repeats the apply pass over the tile's halo, and the kernel runs one
    // workgroup per CU (512 VGPRs) — 32-row tiles halve both the repeats and the workgroup count (24^3 x 32: 144 workgroups, one round)
    if (k3 && fa && ck == 32 && mt == 16 && rows16 % 32 == 0) mt = 32;
    pl.t = k3 ? k3_tiles(p, a.dtype, ck, mt, rows16, pl.tiles) : ConvTiles{ck, mt, rows16 / mt, false};
    const long long wgs = pl.tiles * pl.t.row_tiles;
    if (!k3) {
        g1_ea_plan(pl, wgs);
    } else if (a.dtype != VS_F32) {
        pl.fa_ok = g1_k3_fa_supported(p, pl.t.ck, pl.t.mt, sums) != 0;
        pl.ea_ok = g1_k3_ea_supported(p, pl.t.ck, pl.t.mt, wgs) != 0;
        // the fused weight gradient (igemm_k3tw.h): 8 -> 8, the weight image is the Toeplitz one of k3t_kernel
        pl.wg_ok = vs_cfg().fuse_wgrad && a.c_in == 8 && a.m_out == 8 && a.n * 8 <= 192 && (double)a.n * a.d * a.h * a.w * 16 < 2147483648.0 &&
                   vs_k3_toeplitz(8, 8, 27, a.dtype);
    } else if (pl.t.limbs) {
        pl.fa_ok = k3x_fa_supported(p, pl.t.ck, pl.t.mt) != 0;
        pl.ea_ok = k3x_ea_supported(p, pl.t.ck, pl.t.mt, wgs) != 0;
    }
    pl.ea_ok = pl.ea_ok && sums && !fa && vs_cfg().epilogue_apply;
    if ((fa && !pl.fa_ok) || (ea && !pl.ea_ok) || ((a.parts & WGRAD) && !pl.wg_ok)) pl.status = VS_ESHAPE;
    return pl;
}

// the stride-2 scatter (backward-data of Conv3d(k2, s2), forward of ConvTranspose3d(k2, s2)): the column grid is the input grid, 8 taps x m_out rows
static ConvPlan plan_scatter(const ConvAsk& a) {
    ConvPlan pl = plan_begin(a, 8 * a.m_out);
    const bool sums = a.parts & SUMS, ea = a.parts & EA;
    if (!pl.status && wide_layer(a.c_in, a.m_out) && ea) pl.status = VS_ESHAPE;
    if (pl.status) return pl;
    G1Params& p = pl.g;
    p.Do = a.d; p.Ho = a.h; p.Wo = a.w;
    p.inv_count_out = 1.0 / (8.0 * a.d * a.h * a.w);
    p.tiles_per_sample = vs_ceil_div((long long)a.d * a.h * a.w, 256);
    pl.tiles = (long long)p.tiles_per_sample * a.n;
    // the 8 -> 8 backward-data scatter at full resolution (Down1): a streaming kernel instead of an MFMA tile per 256 coarse voxels (k2s2_scatter8.hip);
    // it has no epilogue apply (full resolution: never resident) and hands the shapes it declines back with VS_ESHAPE
    pl.stream8 = !ea && vs_cfg().k2s2_stream && sums && a.c_in == 8 && a.m_out == 8 && a.dtype != VS_F32 && !(a.parts & (BIAS | X_STATS));
    const int rows16 = p.rb_total * 16;
    const int mt = pick_mt(rows16, pl.tiles);
    pl.t = ConvTiles{pl.t.ck, mt, rows16 / mt, false};
    g1_ea_plan(pl, pl.tiles * pl.t.row_tiles);
    pl.ea_ok = pl.ea_ok && sums && vs_cfg().epilogue_apply;
    if (ea && !pl.ea_ok) pl.status = VS_ESHAPE;
    return pl;
}

// validate the pointers every launch has, then dispatch.  p: the plan's geometry with the call's pointers and eps filled in
static int launch_conv(const ConvPlan& pl, const G1Params& p, void* stream) {
    const ConvAsk& a = pl.ask;
    hipStream_t s = (hipStream_t)stream;
    int rc = check_common(p.x, p.wp, a.n, a.d, a.h, a.w, a.c_in, a.dtype);
    if (rc) return rc;
    if (!p.y || ((uintptr_t)p.y & 15)) return VS_EINVAL;
    if (pl.status) return pl.status;
    if (a.kind == VS_CONV_K3) return dispatch_k3(p, a.dtype, pl.t, EPI_RAW, (int)pl.tiles, s);
    if (a.kind == VS_CONV_K2S2) return g1_dispatch_k2s2(p, a.dtype, pl.t.ck, pl.t.mt, (int)pl.tiles, pl.t.row_tiles, s);
    if (pl.stream8) {
        rc = k2s2_scatter8_launch(p, a.dtype, s);
        if (rc != VS_ESHAPE) return rc;
    }
    return g1_dispatch_pw(p, a.dtype, pl.t.ck, pl.t.mt, (int)pl.tiles, pl.t.row_tiles, s);
}

extern "C" int vs_conv_gather_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias, void* y, double* y_stats,
                                  int n, int d, int h, int w, int c_in, int m_out, int kind, int dtype, float eps, void* stream) {
    const ConvPlan pl = plan_gather({n, d, h, w, c_in, m_out, kind, dtype, 0});
    G1Params p = pl.g;
    p.x = x; p.x_stats = x_stats; p.wp = w_packed; p.bias = bias; p.y = y; p.y_stats = y_stats; p.eps = eps;
    return launch_conv(pl, p, stream);
}

// a backward-data launch with the fused IN-backward sums: the plan's geometry plus the pointers every such entry point has
static G1Params bwd_params(const ConvPlan& pl, const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats, double* sums, float eps) {
    G1Params p = pl.g;
    p.x = x; p.wp = w_packed; p.y = y; p.mask_x = mask_x; p.mask_stats = mask_stats; p.sums = sums; p.eps = eps;
    return p;
}

extern "C" int vs_conv_gather_bwd_data(const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats, double* sums,
                                       int n, int d, int h, int w, int c_in, int m_out, int kind, int dtype, float eps, void* stream) {
    if (!mask_x || !mask_stats || !sums) return VS_EINVAL;
    const ConvPlan pl = plan_gather({n, d, h, w, c_in, m_out, kind, dtype, SUMS});
    return launch_conv(pl, bwd_params(pl, x, w_packed, y, mask_x, mask_stats, sums, eps), stream);
}

static ConvPlan plan_fused_apply(int n, int d, int h, int w, int c_in, int m_out, bool lazy_input, int dtype) {
    return plan_gather({n, d, h, w, c_in, m_out, VS_CONV_K3, dtype, X_STATS | FA | (lazy_input ? SUMS : 0)});
}
extern "C" int vs_conv_k3_bwd_data_fused_apply(const void* g, const void* act_x, const double* act_stats, const double* act_sums, const void* w_packed, void* y,
                                               const void* mask_x, const double* mask_stats, double* sums, void* dx_out, int n, int d, int h, int w, int c_in,
                                               int m_out, int dtype, float eps, void* stream) {
    if (!g || !act_x || !act_stats || !act_sums) return VS_EINVAL;
    if ((mask_x == nullptr) != (sums == nullptr) || (mask_x == nullptr) != (mask_stats == nullptr)) return VS_EINVAL;    // all three (lazy conv input) or none
    const ConvPlan pl = plan_fused_apply(n, d, h, w, c_in, m_out, mask_x != nullptr, dtype);
    if (dtype == VS_F32 && pl.status) return VS_ESHAPE;
    if (((uintptr_t)act_x & 15) || (dx_out && ((uintptr_t)dx_out & 15))) return VS_EALIGN;
    G1Params p = bwd_params(pl, g, w_packed, y, mask_x, mask_stats, sums, eps);
    p.x_stats = act_stats; p.fa_x = act_x; p.fa_sums = act_sums; p.fa_dx = dx_out;
    return launch_conv(pl, p, stream);
}

extern "C" int vs_conv_k3_fused_apply_supported(int n, int d, int h, int w, int c_in, int m_out, int lazy_input, int dtype) {
    return plan_fused_apply(n, d, h, w, c_in, m_out, lazy_input != 0, dtype).status == VS_OK;
}

// ---- backward-data whose epilogue applies the InstanceNorm+ReLU backward itself (igemm_k3b.h EA, round 6) ----
extern "C" int vs_conv_k3_bwd_data_applied_supported(int n, int d, int h, int w, int c_in, int m_out, int dtype) {
    return plan_gather({n, d, h, w, c_in, m_out, VS_CONV_K3, dtype, SUMS | EA}).status == VS_OK;
}

extern "C" int vs_conv_k3_bwd_data_applied(const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats, double* sums,
                                           unsigned int* sync, unsigned int* fault, int n, int d, int h, int w, int c_in, int m_out, int dtype, float eps, void* stream) {
    if (!mask_x || !mask_stats || !sums || !sync || !fault) return VS_EINVAL;
    if (((uintptr_t)sync & 127) || ((uintptr_t)fault & 3)) return VS_EALIGN;
    const ConvPlan pl = plan_gather({n, d, h, w, c_in, m_out, VS_CONV_K3, dtype, SUMS | EA});
    if (pl.status) return VS_ESHAPE;
    G1Params p = bwd_params(pl, x, w_packed, y, mask_x, mask_stats, sums, eps);
    p.ea_sync = sync; p.ea_fault = fault;
    return launch_conv(pl, p, stream);
}

// ---- backward-data with the layer's weight gradient fused (igemm_k3tw.h) ----
static ConvPlan plan_wgrad(int n, int d, int h, int w, int c_in, int m_out, bool act, int dtype) {
    return plan_gather({n, d, h, w, c_in, m_out, VS_CONV_K3, dtype, SUMS | WGRAD | (act ? X_STATS | FA : 0)});      // act: an un-applied gradient comes in
}
extern "C" int vs_conv_k3_bwd_data_wgrad_supported(int n, int d, int h, int w, int c_in, int m_out, int dtype) {
    return plan_wgrad(n, d, h, w, c_in, m_out, false, dtype).status == VS_OK;
}

extern "C" int vs_conv_k3_bwd_data_wgrad_slabs(int n, int d, int h, int w) {
    if (n <= 0 || d <= 0 || h <= 0 || w <= 0) return 0;
    return k3tw_slab_count(n, d, h, w);
}

extern "C" int vs_conv_k3_bwd_data_wgrad(const void* g, const void* act_x, const double* act_stats, const double* act_sums, const void* w_packed, void* y,
                                         const void* mask_x, const double* mask_stats, double* sums, float* slabs, int n, int d, int h, int w, int c_in,
                                         int m_out, int dtype, float eps, void* stream) {
    if (!g || !slabs || !mask_x || !mask_stats || !sums) return VS_EINVAL;
    if ((act_x == nullptr) != (act_stats == nullptr) || (act_x == nullptr) != (act_sums == nullptr)) return VS_EINVAL;     // all three (un-applied gradient in) or none
    const ConvPlan pl = plan_wgrad(n, d, h, w, c_in, m_out, act_x != nullptr, dtype);
    if (pl.status) return VS_ESHAPE;
    if (((uintptr_t)slabs & 15) || (act_x && ((uintptr_t)act_x & 15))) return VS_EALIGN;
    G1Params p = bwd_params(pl, g, w_packed, y, mask_x, mask_stats, sums, eps);
    p.x_stats = act_stats; p.fa_x = act_x; p.fa_sums = act_sums; p.wg_ws = slabs;
    return launch_conv(pl, p, stream);
}

// out_block's backward in one launch: softmax backward while staging, backward-data with the fused IN-backward sums [, weight gradient slabs, bias partials]
extern "C" int vs_conv_k3_softmax2_bwd_data(const float* prob, const float* gprob, const void* gprob_cl, const void* w_packed, void* y, const void* mask_x,
                                            const double* mask_stats, double* sums, float* slabs, double* bias_part, int n, int d, int h, int w, int dtype,
                                            float eps, float drop_p, unsigned long long drop_seed, void* stream) {
    if (!prob || (!gprob && !gprob_cl) || !w_packed || !y || !mask_x || !mask_stats || !sums) return VS_EINVAL;
    if (bias_part && !slabs) return VS_EINVAL;             // the bias partials travel with the weight gradient's slabs
    const ConvPlan pl = plan_wgrad(n, d, h, w, 8, 8, false, dtype);
    if (pl.status) return VS_ESHAPE;
    if (((uintptr_t)w_packed & 15) || ((uintptr_t)y & 15) || ((uintptr_t)mask_x & 15) || (gprob_cl && ((uintptr_t)gprob_cl & 15)) || (slabs && ((uintptr_t)slabs & 15)) ||
        ((uintptr_t)prob & 3) || ((uintptr_t)gprob & 3)) return VS_EALIGN;
    if (!(drop_p >= 0.f && drop_p < 1.f)) return VS_EINVAL;
    G1Params p = bwd_params(pl, nullptr, w_packed, y, mask_x, mask_stats, sums, eps);      // no x: the gradient is formed from the probabilities while staging
    p.sm_prob = prob; p.sm_gprob = gprob; p.sm_gcl = gprob_cl; p.wg_ws = slabs; p.wg_bias = bias_part;
    p.drop_p = drop_p; p.drop_seed = drop_seed;
    return dispatch_k3(p, dtype, pl.t, EPI_RAW, 0, (hipStream_t)stream);                    // k3tw_launch tiles the grid its own way
}

extern "C" int vs_conv_scatter_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias, void* y,
                                   int n, int d, int h, int w, int c_in, int m_out, int dtype, float eps, void* stream) {
    const ConvPlan pl = plan_scatter({n, d, h, w, c_in, m_out, VS_CONV_T2S2, dtype, (x_stats ? X_STATS : 0) | (bias ? BIAS : 0)});
    G1Params p = pl.g;
    p.x = x; p.x_stats = x_stats; p.wp = w_packed; p.bias = bias; p.y = y; p.eps = eps;
    return launch_conv(pl, p, stream);
}

extern "C" int vs_conv_scatter_bwd_data(const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats, double* sums,
                                        int n, int d, int h, int w, int c_in, int m_out, int dtype, float eps, void* stream) {
    if (!mask_x || !mask_stats || !sums) return VS_EINVAL;
    const ConvPlan pl = plan_scatter({n, d, h, w, c_in, m_out, VS_CONV_T2S2, dtype, SUMS});
    return launch_conv(pl, bwd_params(pl, x, w_packed, y, mask_x, mask_stats, sums, eps), stream);
}

// ---- the same for the stride-2 kinds (igemm.h g1_kernel's epilogue apply): scatter = 0: backward-data of ConvTranspose3d(k2, s2) (a stride-2 gather);
// scatter = 1: backward-data of Conv3d(k2, s2) (the scatter form).  add (nullable): a second gradient of the same raw tensor, summed in after the apply ----
static ConvPlan plan_s2_applied(int n, int d, int h, int w, int c_in, int m_out, int scatter, int dtype) {
    return scatter ? plan_scatter({n, d, h, w, c_in, m_out, VS_CONV_T2S2, dtype, SUMS | EA}) : plan_gather({n, d, h, w, c_in, m_out, VS_CONV_K2S2, dtype, SUMS | EA});
}
extern "C" int vs_conv_s2_bwd_data_applied_supported(int n, int d, int h, int w, int c_in, int m_out, int scatter, int dtype) {
    return plan_s2_applied(n, d, h, w, c_in, m_out, scatter, dtype).status == VS_OK;
}

extern "C" int vs_conv_s2_bwd_data_applied(const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats, double* sums, const void* add,
                                           unsigned int* sync, unsigned int* fault, int n, int d, int h, int w, int c_in, int m_out, int scatter, int dtype, float eps,
                                           void* stream) {
    if (!mask_x || !mask_stats || !sums || !sync || !fault) return VS_EINVAL;
    if (((uintptr_t)sync & 127) || ((uintptr_t)fault & 3) || (add && ((uintptr_t)add & 15))) return VS_EALIGN;
    const ConvPlan pl = plan_s2_applied(n, d, h, w, c_in, m_out, scatter, dtype);
    if (pl.status) return VS_ESHAPE;
    G1Params p = bwd_params(pl, x, w_packed, y, mask_x, mask_stats, sums, eps);
    p.ea_sync = sync; p.ea_fault = fault; p.ea_add = add;
    return launch_conv(pl, p, stream);
}

extern "C" int vs_conv_k3_softmax2_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias,
                                       float* prob, int n, int d, int h, int w, int c_in, int dtype, float eps,
                                       void* stream) {
    return vs_conv_k3_softmax2_dropout_fwd(x, x_stats, w_packed, bias, prob, n, d, h, w, c_in, dtype, eps, 0.f, 0ull, stream);
}

extern "C" int vs_conv_k3_softmax2_dropout_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias,
                                               float* prob, int n, int d, int h, int w, int c_in, int dtype, float eps,
                                               float drop_p, unsigned long long drop_seed, void* stream) {
    return vs_conv_k3_softmax2_cl_fwd(x, x_stats, w_packed, bias, prob, nullptr, n, d, h, w, c_in, dtype, eps, drop_p, drop_seed, stream);
}

extern "C" int vs_conv_k3_softmax2_cl_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias, float* prob, void* prob_cl,
                                          int n, int d, int h, int w, int c_in, int dtype, float eps, float drop_p, unsigned long long drop_seed, void* stream) {
    if (drop_p < 0.f || drop_p >= 1.f) return VS_EINVAL;
    if (prob_cl && dtype == VS_F32) return VS_EDTYPE;
    if (prob_cl && ((uintptr_t)prob_cl & 15)) return VS_EALIGN;
    int rc = check_common(x, w_packed, n, d, h, w, c_in, dtype);
    if (rc) return rc;
    if (!prob || c_in != 8) return VS_ESHAPE;
    const ConvPlan pl = plan_gather({n, d, h, w, 8, 8, VS_CONV_K3, dtype, 0});           // the two logits are stored in 8 channels: one 16-row block
    G1Params p = pl.g;
    p.x = x; p.x_stats = x_stats; p.wp = w_packed; p.bias = bias; p.y = prob_cl; p.prob = prob; p.eps = eps;
    p.drop_p = drop_p; p.drop_seed = drop_seed;
    return dispatch_k3(p, dtype, pl.t, EPI_SOFTMAX2, (int)pl.tiles, (hipStream_t)stream);
}
