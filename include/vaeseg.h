/* libvaeseg — C ABI of the MI355X (gfx950) kernels behind the joint_model.py surface.
 *
 * The reference (yyNoBug/VAE_segmentation) has no FFI of its own: its hot path is the stock ATen ops
 * that joint_model.py / utils/evaluation.py invoke.  Each entry point below replaces one such op (or a
 * fused group of them); the reference call site it stands in for is cited as file:line under
 * /root/reference.  INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch); nothing is allocated, freed or
 *     synchronised inside; every launch goes to `stream` (a hipStream_t passed as void*).
 *   - activations are channels-last: [N][D][H][W][C], C a multiple of 8, element type `dtype`
 *     (VS_F32, VS_BF16 or VS_F16; accumulation is always fp32).  "planar" tensors are the reference's NCDHW fp32: [N][C][D*H*W].
 *   - a *lazy* activation is a raw conv output plus `stats`: double[VS_STAT_SLOTS][N][C][2] = VS_STAT_SLOTS partial copies of
 *     (sum, sum of squares) over the D*H*W voxels of each (n,c): a producing workgroup accumulates (fp64 atomics) into copy
 *     (workgroup id mod VS_STAT_SLOTS), consumers add the copies — same-address atomics retire ~20 ns apart, and hundreds of
 *     workgroups finish together at the full-resolution levels.  The IN-backward `sums` buffers have the same shape.  Passing `stats` to a
 *     consumer makes it read relu((x-mean)*rstd) — InstanceNorm3d(affine=False, eps) + ReLU
 *     (joint_model.py:11,41-48,107-108) — without that tensor ever being materialised.  stats == NULL
 *     means "use x as is".
 *   - return value: 0 on success, negative VS_E* on a rejected call, positive = hipError_t.
 *   - the library is re-entrant: no mutable globals.
 */
#ifndef VAESEG_H
#define VAESEG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_VERSION 500

enum { VS_F32 = 0, VS_BF16 = 1, VS_F16 = 2, VS_F32X3 = 3 /* PACK-ONLY: three-bf16-limb image of an fp32 3x3x3 weight, see vs_conv_k3_f32_limbs */ };   /* storage type of activations: fp32 (parity mode), bf16, IEEE fp16 (needs loss scaling, see vs_loss_scale_*) */
#ifndef VS_STAT_SLOTS
#define VS_STAT_SLOTS 4        /* measured on one MI355X, 96^3 step: 1 copy 2.908 ms, 2: 2.820, 4: 2.797, 8: 3.021 (consumers read every copy) */
#endif
enum { VS_OK = 0, VS_EINVAL = -1, VS_ESHAPE = -2, VS_EDTYPE = -3, VS_EWORKSPACE = -4, VS_EALIGN = -5 };

/* geometry of an implicit-GEMM convolution */
enum {
    VS_CONV_K3 = 0,     /* 3x3x3, stride 1, pad 1          nn.Conv3d(...,3,padding=1)        joint_model.py:40,43,46,106,224,366 */
    VS_CONV_K2S2 = 1,   /* 2x2x2, stride 2, pad 0          nn.Conv3d(C,C,2,stride=2)         joint_model.py:130 */
    VS_CONV_T2S2 = 2,   /* 2x2x2 transposed, stride 2      nn.ConvTranspose3d(C,C,2,stride=2) joint_model.py:118 */
    VS_WGRAD_SLABS = 16, /* vs_wgrad_desc only: p = the slabs vs_conv_k3_bwd_data_wgrad wrote, n = their count (vs_conv_k3_bwd_data_wgrad_slabs); m_ch = c_ch = 8,
                            m_real / c_real / dw as for the layer; the descriptor only takes part in the grouped reduction and must be the only one for its dw */
    VS_CONV_UP = 3      /* vs_wgrad_desc only: the composed Up block (vs_up_*): p = the FINE output gradient (n,2dp,2hp,2wp,Co) read space-to-depth
                           (m_ch = m_real = 8 Co view channels (parity, co); reserved_ = Co), q = the coarse input, dw = dWeff [8 Co][c_real][27] */
};

/* how a weight tensor src[d0][d1][ntaps] (fp32, the reference's parameter layout) is packed into MFMA
 * fragment order for a GEMM whose rows are output channels m and whose k runs over (tap, channel c) */
enum {
    VS_PACK_ROWS_D0 = 0,       /* m = d0, c = d1                 : Conv3d forward; ConvTranspose3d backward-data        */
    VS_PACK_ROWS_D1_FLIP = 1,  /* m = d1, c = d0, taps mirrored  : Conv3d(k3,p1) backward-data                          */
    VS_PACK_SCATTER_D1 = 2     /* rows (tap, m = d1), k = c = d0 : ConvTranspose3d forward; Conv3d(k2,s2) backward-data */
};

int vs_version(void);
int vs_stat_slots(void);        /* VS_STAT_SLOTS the library was built with (callers size statistics buffers by it) */
int vs_stat_interleaved(void);  /* 0: double[slot][N][C][2]   1: double[N][C][slot][2] */
const char* vs_strerror(int code);
/* 1 for the deterministic build of the library (libvaeseg_det.so, -DVS_DET_BUILD=1: parity runs), 0 for the throughput build.  In the
 * deterministic build every per-(n,c) statistic — the conv epilogues' (sum, sumsq), the fused InstanceNorm-backward sums, the vs_instnorm_*
 * reductions — is accumulated with commuting integer atomics on four fixed-point limbs held in the same double[VS_STAT_SLOTS][N][C][2]
 * buffer (csrc/common.h), and the few remaining floating-point atomics (vs_dice_fwd, vs_bce_fwd, vs_bias_grad) run as one block: two runs of a
 * step on the same inputs agree bit for bit.  A statistics buffer must be produced and consumed by the same build. */
int vs_get_deterministic(void);

/* ---- composed Up block (csrc/igemm_k4.h): ConvTranspose3d(C, C, 2, stride 2) -> Conv3d(C, Co, 3, padding 1) as ONE operator -----------------
 * Replaces, for 16-bit storage, the pair vs_conv_scatter_fwd + vs_conv_gather_fwd(K3) behind `Up` (/root/reference/joint_model.py:116-120: the
 * Sequential has nothing between the two convolutions) and, backward, vs_conv_gather_bwd_data(K3) + vs_conv_gather_bwd_data(K2S2).
 * w2 = ConvTranspose3d.weight [cin][cm][2][2][2], b2 = its bias [cm] (nullable), w3 = Conv3d.weight [co][cm][3][3][3] (bias dead: InstanceNorm follows).
 * vs_up_compose_sizes -> bytes of {Weff fp32 scratch, forward image, backward-data image, forward tap lists, backward tap lists, bias table}. */
int vs_up_supported(int cin, int cm, int co, int dtype);
int vs_up_compose_sizes(int cin, int cm, int co, size_t* out6);
int vs_up_compose(const float* w2, const float* b2, const float* w3, float* weff, void* img_fwd, void* img_bwd, int* taps_fwd, int* taps_bwd,
                  float* btab, int cin, int cm, int co, int dtype, void* stream);
/* x: coarse (n,d,h,w,cin) [lazy with x_stats]; y: fine raw conv output (n,2d,2h,2w,co) + its statistics */
int vs_up_conv_fwd(const void* x, const double* x_stats, const void* img_fwd, const int* taps_fwd, const float* btab, void* y, double* y_stats,
                   int n, int d, int h, int w, int cin, int co, int dtype, float eps, void* stream);
/* Weight gradients of the composed block: vs_conv_wgrad_multi with a VS_CONV_UP descriptor gives dWeff27[(parity, co)][ci][27 coarse offsets];
 * vs_up_faces sums the output gradient over the 26 boundary classes of the fine volume (the transposed conv's bias acts only through the zero
 * padding of the 3x3x3 conv: its gradient is a boundary quantity, and the sum over the whole volume of an InstanceNorm-backward output is 0)
 * into G, a statistics-format buffer double[VS_STAT_SLOTS][27 co / 2][2] (ACCUMULATED: caller zeroes; entry cls * co + c = statistic (e & 1) of
 * pair e >> 1; a second use of the weights in the same pass simply adds); vs_up_chain applies the parameter-space chain rule:
 * dw3 [co][cm][27], dw2 [cin][cm][8], db2 [cm] (any of them nullable). */
int vs_up_faces(const void* gy, double* G, int n, int fd, int fh, int fw, int co, int dtype, void* stream);
int vs_up_chain(const float* dweff27, const double* G, const float* w2, const float* b2, const float* w3, float* dw2, float* db2, float* dw3,
                int cin, int cm, int co, void* stream);
/* gy: gradient of y (fine, applied); gx: gradient of the coarse input (n,d,h,w,cin); mask_* / sums: fused InstanceNorm-backward sums of a lazy input (all or none) */
int vs_up_conv_bwd_data(const void* gy, const void* img_bwd, const int* taps_bwd, void* gx, const void* mask_x, const double* mask_stats,
                        double* sums, int n, int d, int h, int w, int co, int cin, int dtype, float eps, void* stream);

/* ---- weights ---------------------------------------------------------------------------------- */
/* bytes of the packed image of a weight with `rows` GEMM rows (any count; padded to 16 inside),
 * `c_pad` k-side channels (multiple of 8) and ntaps taps (27, 8, or 1 for VS_PACK_SCATTER_D1). */
size_t vs_packed_weight_bytes(int rows, int c_pad, int ntaps, int dtype);
/* src: float[d0][d1][ntaps]; c_pad >= the k-side channel count, zero-filled beyond it. */
int vs_pack_weight(const float* src, void* dst, int d0, int d1, int ntaps, int c_pad, int form, int dtype, void* stream);

/* One launch packing many weights (all trainable convs of a network after an optimiser step): descs is a DEVICE array. */
typedef struct vs_pack_desc {
    const float* src;      /* float[d0][d1][ntaps] */
    void* dst;             /* packed image, vs_packed_weight_bytes() bytes */
    int d0, d1, ntaps, c_pad, form, dtype;
    int first_block;       /* index of this weight's first 256-thread block in the launch; a thread packs one 16-byte fragment (8 bf16 / 4 fp32 elements) */
    int pad_;
    long long total;       /* packed elements of this weight */
} vs_pack_desc;
int vs_pack_weight_multi(const vs_pack_desc* descs, int n_desc, int total_blocks, void* stream);

/* ---- convolutions (implicit GEMM on MFMA) ------------------------------------------------------ */
/* y[n,v,m] = bias[m] + sum_{tap,c} act(x)[n, v*s + off(tap) - p, c] * W[m][tap][c]
 *   kind K3  : x,y both (N,D,H,W);   kind K2S2: x is (N,D,H,W), y is (N,D/2,H/2,W/2).
 * Also the backward-data of K3 (with VS_PACK_ROWS_D1_FLIP weights) and of T2S2 (kind K2S2 with the
 * transposed-conv weight packed VS_PACK_ROWS_D0).
 *   x_stats  : lazy-activation stats of x or NULL         y_stats : if non-NULL, (sum,sumsq) of y are
 *   bias     : float[m_out] or NULL                                 ACCUMULATED into it (caller zeroes)
 *   c_in     : channels of x: 8, 16 or a multiple of 32 up to 512   m_out : channels of y (multiple of 8, at most 512; rows
 *              beyond the real weight rows come out as bias/zero)
 * Layers with more than 256 input or output channels (the deepest levels of the wide models, n_fmaps [16, .., 512]) run the
 * per-layer kernels only: the fused-apply, epilogue-apply, chain and composed-Up queries answer 0 for them.
 */
int vs_conv_gather_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias,
                       void* y, double* y_stats, int n, int d, int h, int w, int c_in, int m_out,
                       int kind, int dtype, float eps, void* stream);

/* y[n, 2v+off(tap), m] = bias[m] + sum_c act(x)[n,v,c] * W[tap][m][c]      (x is (N,D,H,W), y (N,2D,2H,2W))
 * ConvTranspose3d(k2,s2) forward (joint_model.py:118) and Conv3d(k2,s2) backward-data. */
int vs_conv_scatter_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias,
                        void* y, int n, int d, int h, int w, int c_in, int m_out, int dtype, float eps, void* stream);

/* Backward-data forms of the two calls above with the InstanceNorm+ReLU-backward REDUCTION fused into the epilogue:
 * y here is g = dL/da of a lazy activation a = relu(instnorm(mask_x)) (mask_x: raw tensor shaped like y, mask_stats
 * its (sum,sumsq)); besides writing g the kernel ACCUMULATES sums[n][m] = (sum g*[xhat>0], sum g*[xhat>0]*xhat)
 * (caller zeroes), i.e. exactly what vs_instnorm_relu_bwd_reduce(g, mask_x, mask_stats) would return, without re-reading g. */
int vs_conv_gather_bwd_data(const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats,
                            double* sums, int n, int d, int h, int w, int c_in, int m_out, int kind, int dtype, float eps,
                            void* stream);
int vs_conv_scatter_bwd_data(const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats,
                             double* sums, int n, int d, int h, int w, int c_in, int m_out, int dtype, float eps, void* stream);
/* vs_conv_gather_bwd_data (K3) whose INPUT gradient arrives un-applied: g = dL/da of the lazy activation a = relu(instnorm(act_x)), with
 * that activation's statistics (act_stats) and IN-backward sums (act_sums, complete: produced by the backward-data launch that wrote g).
 * The apply pass rstd * (g*[xhat>0] - m1 - xhat*m2) runs while the halo tile is staged — the standalone vs_instnorm_relu_bwd_apply launch
 * between two backward-data launches of the 8-channel full-resolution layers (3 tensor passes at 96^3) disappears; dx_out (nullable)
 * receives the applied gradient (what the weight gradient of this layer reads).  mask_x / mask_stats / sums: all three as in
 * vs_conv_gather_bwd_data (the conv's own input is a lazy activation) or all NULL (it is a stored tensor: no sums to accumulate).
 * 16-bit storage; kernels exist for the single-chunk layers of the full- and half-resolution levels (c_in 8 or 16: igemm_k3t.h, igemm_k3b.h FA);
 * any other shape returns VS_ESHAPE — ask vs_conv_k3_fused_apply_supported first (1 / 0; lazy_input: the conv's own input is a lazy activation). */
int vs_conv_k3_fused_apply_supported(int n, int d, int h, int w, int c_in, int m_out, int lazy_input, int dtype);
/* Backward-data of a 3x3x3 conv whose own input is a lazy activation (vs_conv_gather_bwd_data, K3) WITH THE LAYER'S WEIGHT GRADIENT in the same launch
 * (autograd of joint_model.py:40-48 at full resolution; csrc/igemm_k3tw.h): the launch already holds both operands of dW — the applied output gradient as
 * its halo tile, relu(instnorm(mask_x)) under every output voxel for the fused sums — so neither is read again by the grouped weight-gradient launch.
 * act_x / act_stats / act_sums: all three (g arrives un-applied, as for vs_conv_k3_bwd_data_fused_apply; the applied gradient is then never stored) or all NULL.
 * slabs: vs_conv_k3_bwd_data_wgrad_slabs(n, d, h, w) partial sums float[27][8][8] each, S[o][c][m] = sum_v Q(v)[c] g_applied(v + o)[m] = dW[m][c][-o];
 * hand them to vs_conv_wgrad_multi as a VS_WGRAD_SLABS descriptor (fixed summation order: bitwise reproducible).
 * 16-bit storage, c_in = m_out = 8 stored channels (the 96^3 / 128^3 / 160^3 levels); vs_conv_k3_bwd_data_wgrad_supported says 1 / 0 (VS_FUSE_WGRAD=0: always 0). */
int vs_conv_k3_bwd_data_wgrad_supported(int n, int d, int h, int w, int c_in, int m_out, int dtype);
int vs_conv_k3_bwd_data_wgrad_slabs(int n, int d, int h, int w);
int vs_conv_k3_bwd_data_wgrad(const void* g, const void* act_x, const double* act_stats, const double* act_sums, const void* w_packed, void* y,
                              const void* mask_x, const double* mask_stats, double* sums, float* slabs, int n, int d, int h, int w, int c_in,
                              int m_out, int dtype, float eps, void* stream);
/* out_block's backward (two classes, 8 stored channels; joint_model.py:224-225,265-266 / 366-367,386-388) as ONE launch: the gradient of the logits is formed
 * from the planar probabilities and their gradient(s) while the tile is staged — exactly vs_softmax2_cl_bwd(prob, gprob, gprob_cl), logit dropout included,
 * never stored — and multiplied out as vs_conv_gather_bwd_data would (y, fused sums against mask_x / mask_stats).  slabs (nullable): the layer's weight
 * gradient as for vs_conv_k3_bwd_data_wgrad; bias_part (nullable, needs slabs): one (sum gl0, sum gl1) pair of doubles per slab — give both to
 * vs_conv_wgrad_multi as ONE VS_WGRAD_SLABS descriptor (bias_g = bias_part, bias_rows = the slab count, bias_c_real = 2, db).  Shapes: those of
 * vs_conv_k3_bwd_data_wgrad_supported(n, d, h, w, 8, 8, dtype). */
int vs_conv_k3_softmax2_bwd_data(const float* prob, const float* gprob, const void* gprob_cl, const void* w_packed, void* y, const void* mask_x,
                                 const double* mask_stats, double* sums, float* slabs, double* bias_part, int n, int d, int h, int w, int dtype,
                                 float eps, float drop_p, unsigned long long drop_seed, void* stream);
/* The library's tuning switches, in ONE place (round 6; csrc/config.hip).  The library keeps one process-wide copy: filled on first use from the environment
 * variables named below (so A/B scripts that set them before the process starts keep working), read by every launcher on EVERY call (nothing is cached in
 * function-local statics), replaced as a whole by vs_set_config() — the only writer; set it between launches, not concurrently with one.  vs_config_bytes():
 * sizeof(vs_config) of the loaded library (bindings check their layout against it).  vs_config_from_env(): defaults + environment into *c without installing it. */
typedef struct vs_config {
    int k3_small;              /* VS_K3_SMALL 1: volumes up to 6^3 with C % 32 == 0 run k3s_kernel (whole padded sample in LDS) */
    int k3_tall;               /* VS_K3_TALL -1: 4x8x16 tiles where measured faster (auto); 0 / 1 force */
    int k3_wgs_per_cu;         /* VS_K3_WGS_PER_CU 0: persistent workgroups per CU of the 3x3x3 kernels (0 = per-kernel default: 3 for k3b, 4 for the exact-f32 k3) */
    int k3t_wgs_per_cu;        /* VS_K3T_WGS_PER_CU 2: the 8-channel full-resolution kernels (k3t, k3tw) */
    int k3f_min_wgs;           /* VS_K3F_MIN_WGS 512: exact-f32 C >= 32 layers take shorter tiles until the launch has this many workgroups */
    int mt_min_wgs;            /* VS_MT_MIN_WGS 1024: largest row tile that still leaves this many workgroups */
    int f32_limbs;             /* VS_F32_LIMBS 1: fp32 parity mode on the bf16 matrix cores (three-limb operands); 0 = exact-f32 MFMA everywhere */
    int g1_limbs;              /* VS_G1_LIMBS 1: ... in the stride-2 / transposed kernels */
    int k3x_ck;                /* VS_K3X_CK 8: channel chunk of the limb kernels (8 or 16) */
    int k3x_toeplitz;          /* VS_K3X_TOEPLITZ 1 */
    int fuse_wgrad;            /* VS_FUSE_WGRAD 1: vs_conv_k3_bwd_data_wgrad_supported may say 1 */
    int epilogue_apply;        /* VS_EPILOGUE_APPLY 1: vs_conv_k3_bwd_data_applied_supported may say 1 */
    int chain;                 /* VS_CHAIN 1: vs_conv_k3_chain_supported may say 1 */
    int k2s2_stream;           /* VS_K2S2_STREAM 1: the streaming kernel for the full-resolution stride-2 backward-data scatter */
    int k2s8_wgs_per_cu;       /* VS_K2S8_WGS_PER_CU 4 */
    int up_wgs_per_cu;         /* VS_UP_WGS_PER_CU 2: composed Up head kernels */
    int up_rb;                 /* VS_UP_RB 0: row blocks per workgroup of the composed Up forward (0 = chosen per shape) */
    int wgrad_uber;            /* VS_WGRAD_UBER 1: every bucket of a grouped weight-gradient pass in one grid */
    int wgrad_mpack;           /* VS_WGRAD_MPACK 1: M-packed rows for layers with 8 stored output channels */
    int wgrad_swap;            /* VS_WGRAD_SWAP 1: operand exchange for lazy-input 3x3x3 layers */
    int wgrad_big;             /* VS_WGRAD_BIG 1: 8x8x16 tiles for the full-resolution layers */
    int wgrad_xcd;             /* VS_WGRAD_XCD 2: a layer's workgroups re-ranked so that one XCD walks neighbouring tiles and holds all channel-block pairs of a tile (1: single-pair layers only; 0: plain order) */
    int k3_short_tiles;        /* VS_K3_SHORT_TILES 2: 4x2x16 tiles for the 32-channel 3x3x3 launches of at most 128 workgroups (the 12^3-class levels), 4x1x16 where that still leaves at most 128 (2); 1: 4x2x16 only; 0: off */
    int wgrad_bias_fold;       /* VS_WGRAD_BIAS_FOLD 1: a ConvTranspose3d's bias gradient is summed by its weight-gradient workgroups (the same tensor is their Q operand) */
    int hist_form;             /* VS_HIST_FORM 0: the counting kernel of vs_histogram / vs_joint_histogram is chosen by table size; 1 / 2 / 3 force the 32-bit LDS, the packed 16-bit LDS or the global-atomic form where the table fits it (A/B measurements; the tables are the same) */
    long long wgrad_wgs;            /* VS_WGRAD_WGS 512: workgroups per ungrouped weight-gradient launch */
    long long wgrad_f32_tiles;      /* VS_WGRAD_F32_TILES 8 */
    long long wgrad_group_wgs;      /* VS_WGRAD_GROUP_WGS 0: workgroups per bucket of a grouped pass (0 = chosen per pass) */
    long long wgrad_big_min_voxels; /* VS_WGRAD_BIG_MIN_VOXELS 400000 */
} vs_config;
int vs_config_bytes(void);
int vs_config_from_env(vs_config* c);
int vs_get_config(vs_config* out);
int vs_set_config(const vs_config* cfg);
/* vs_conv_gather_bwd_data (K3) FOLLOWED BY vs_instnorm_relu_bwd_apply of its output, in one launch (csrc/igemm_k3b.h EA, round 6): every workgroup keeps its tile's
 * rounded outputs in registers, adds its partial IN-backward sums, arrives on its SAMPLE's counter (the statistics of joint_model.py:11's InstanceNorm3d are per
 * sample: nothing of another sample is waited for), reads the complete sums back and stores y = dL/d(raw tensor) — the un-applied gradient is never written and the
 * standalone apply launch disappears.  Results equal the two launches' bit for bit in the deterministic build.  sync: n * 1024 ZEROED bytes (8 counter shards per sample), 128-byte aligned,
 * private to the call; fault: the device word of vs_conv_k3_chain.  16-bit storage, c_in a multiple of 32, volumes above 6^3 whose launch is one resident round
 * (at most 512 workgroups: the 24^3 / 12^3 levels): vs_conv_k3_bwd_data_applied_supported says 1 / 0 (env VS_EPILOGUE_APPLY=0: always 0). */
int vs_conv_k3_bwd_data_applied_supported(int n, int d, int h, int w, int c_in, int m_out, int dtype);
int vs_conv_k3_bwd_data_applied(const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats, double* sums,
                                unsigned int* sync, unsigned int* fault, int n, int d, int h, int w, int c_in, int m_out, int dtype, float eps, void* stream);
/* The same for the stride-2 kinds (csrc/igemm.h g1_kernel, round 6): scatter = 0: vs_conv_gather_bwd_data(kind K2S2) — the backward-data of
 * nn.ConvTranspose3d(C, C, 2, stride=2) (joint_model.py:118) — scatter = 1: vs_conv_scatter_bwd_data — the backward-data of nn.Conv3d(C, C, 2, stride=2)
 * (joint_model.py:130) — FOLLOWED BY vs_instnorm_relu_bwd_apply_add of its output, in one launch.  add (nullable, y's shape and type): a second gradient of the same raw
 * tensor (the U-Net skip's, joint_model.py:380,382), summed in after the apply as vs_instnorm_relu_bwd_apply_add does.  Any storage type; launches of at most 256
 * workgroups (the <= 48^3 levels at batch 2).  sync / fault / concurrency rule: as vs_conv_k3_bwd_data_applied.  Results equal the two launches' bit for bit in the
 * deterministic build. */
int vs_conv_s2_bwd_data_applied_supported(int n, int d, int h, int w, int c_in, int m_out, int scatter, int dtype);
int vs_conv_s2_bwd_data_applied(const void* x, const void* w_packed, void* y, const void* mask_x, const double* mask_stats, double* sums, const void* add,
                                unsigned int* sync, unsigned int* fault, int n, int d, int h, int w, int c_in, int m_out, int scatter, int dtype, float eps,
                                void* stream);
/* One DoubleConv (joint_model.py:35-52: three times [Conv3d 3x3x3 pad 1 -> InstanceNorm3d -> ReLU]) at the small volumes of the deep levels as ONE launch
 * (csrc/chain.h, round 6).  InstanceNorm3d is per (sample, channel) (joint_model.py:11), so layer l + 1 of sample n depends on layer l of sample n only: the
 * workgroups of a sample hand the raw output and its statistics over inside the launch (write-through stores, counter, sc1 loads) instead of ending it.
 * forward (backward = 0): layers[0..n_layers) in order; layer l = vs_conv_gather_fwd(K3) of (x, x_stats) -> (y, y_stats); for l > 0, x / x_stats ARE layer l-1's
 *   y / y_stats; layer 0's x_stats may be NULL (a stored input).
 * backward (backward = 1): layers in BACKWARD order; layer l = vs_conv_gather_bwd_data(K3) of the gradient x (layer 0: w.r.t. the block's raw output, applied;
 *   l > 0: layer l-1's y) with the transposed / mirrored weight image -> y = dL/d(activation), sums against (mask_x, mask_stats) = that activation's raw tensor and
 *   statistics; apply = 1: vs_instnorm_relu_bwd_apply runs on y IN PLACE inside the launch (y leaves as dL/d(raw tensor): what the next layer and the weight gradient read).
 *   Every layer but the last must apply; the last may have mask_x = mask_stats = sums = NULL (the block's input is a stored tensor: plain backward-data).
 *   add (nullable; needs the last layer's apply): a second gradient of the last layer's raw tensor, summed in as vs_instnorm_relu_bwd_apply_add does.
 * sync: vs_conv_k3_chain_sync_bytes(n) ZEROED bytes, 128-byte aligned, private to this call; fault: a device word the kernel ORs 1 into when a bounded wait gave up
 *   (never in a correct launch: the library rejects chains whose workgroups cannot all be resident) — results are then invalid, the queue is not hung.
 * CONCURRENCY: the workgroups of a sample wait for one another inside the launch, so all of them must be resident together.  The library guarantees that for a
 *   launch that is not competing for CUs with ANOTHER launch of this kind (vs_conv_k3_chain, vs_conv_k3_bwd_data_applied): one process per GPU issuing its step on
 *   one stream — the deployment model.  Two such launches running at the same time on one device (two processes sharing a GPU, two streams) can each hold part of
 *   the chip and starve the other's waiters; the bounded waits then give up and raise `fault`.  A host that shares a device switches the two forms off first
 *   (vs_set_config: chain = 0, epilogue_apply = 0; Python: ops.device_is_shared()).
 * Shapes: (d+2)(h+2)(w+2) <= 512 (up to 6^3), channels multiples of 32 (c_in) / 8 (m_out) up to 256, at most 256 workgroups per sample (32 per XCD): vs_conv_k3_chain_supported(n, d, h, w,
 * largest channel count of the chain, dtype) says 1 / 0 (env VS_CHAIN=0: always 0).  All three storage types; results are bit-identical to the per-layer launches
 * in the deterministic build. */
typedef struct vs_chain_layer {
    const void* x;
    const double* x_stats;
    const void* w_packed;
    void* y;
    double* y_stats;
    const void* mask_x;
    const double* mask_stats;
    double* sums;
    int c_in, m_out;
    int apply;
    int reserved_;
} vs_chain_layer;
int vs_conv_k3_chain_supported(int n, int d, int h, int w, int c_max, int dtype);
long long vs_conv_k3_chain_sync_bytes(int n);
int vs_conv_k3_chain(const vs_chain_layer* layers, int n_layers, int backward, const void* add, unsigned int* sync, unsigned int* fault,
                     int n, int d, int h, int w, int dtype, float eps, void* stream);
/* fp32 parity mode: 1 when a 3x3x3 convolution of dtype VS_F32 on a (d, h, w) volume with c_in stored input channels runs on the bf16 matrix cores through exact three-limb operand splitting
 * (csrc/igemm_k3x.h: every fp32 operand = three bf16 limbs, six exact limb products per product, fp32 accumulation — 2.7x fewer matrix cycles
 * than the exact-f32 MFMA at the accuracy of one fp32 rounding).  Their packed weights must then be VS_F32X3 images: vs_pack_weight /
 * vs_packed_weight_bytes / vs_pack_weight_multi with dtype VS_F32X3 (a PACK-ONLY dtype: tensors stay VS_F32).  Env VS_F32_LIMBS=0 -> 0: the
 * exact-f32 MFMA kernels with plain VS_F32 images; so do the volumes up to 6^3 with c_in a multiple of 32 (k3s_kernel<float>). */
int vs_conv_k3_f32_limbs(int d, int h, int w, int c_in);

int vs_conv_k3_bwd_data_fused_apply(const void* g, const void* act_x, const double* act_stats, const double* act_sums,
                                    const void* w_packed, void* y, const void* mask_x, const double* mask_stats, double* sums,
                                    void* dx_out, int n, int d, int h, int w, int c_in, int m_out, int dtype, float eps, void* stream);

/* out_block + Softmax(dim=1) fused (joint_model.py:224-225,265-266,366-367,386-388):
 * prob[n][k][v] (planar fp32, k < 2) = softmax_k( bias[k] + conv3x3x3(act(x))[k] ). */
int vs_conv_k3_softmax2_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias,
                            float* prob, int n, int d, int h, int w, int c_in, int dtype, float eps, void* stream);
/* same with F.dropout applied to the two logits before the softmax (Segmentation.forward's last dropout site,
 * joint_model.py:386-388); drop_p == 0 is the call above. */
int vs_conv_k3_softmax2_dropout_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias,
                                    float* prob, int n, int d, int h, int w, int c_in, int dtype, float eps, float drop_p,
                                    unsigned long long drop_seed, void* stream);
/* same, additionally writing the probabilities as a channels-last bf16 tensor prob_cl[n][v][8] (2 real channels) — the input layout of the
 * network that consumes them next (Joint.forward feeds Segmentation's prediction to the VAE, joint_model.py:447-450): saves the
 * vs_pack_planar launch and its re-read.  prob_cl may be NULL (then this is the call above); bf16 only. */
int vs_conv_k3_softmax2_cl_fwd(const void* x, const double* x_stats, const void* w_packed, const float* bias,
                               float* prob, void* prob_cl, int n, int d, int h, int w, int c_in, int dtype, float eps, float drop_p,
                               unsigned long long drop_seed, void* stream);

/* weight gradient of all three conv kinds:
 *   dW[m][c][tap] = sum_{n,v} actP(P)[n,v,m] * actQ(Q)[n, v*s + off(tap) - p, c]        (fp32, reference layout)
 * Conv3d (K3/K2S2): P = dL/dy on the OUTPUT grid (dp,hp,wp), Q = the conv input  -> dW[co][ci][tap].
 * ConvTranspose3d : P = the (coarse) input on (dp,hp,wp), Q = dL/dy (fine grid), kind = VS_CONV_K2S2 -> dW[ci][co][tap].
 * m_real / c_real: how many leading channels of P / Q are real (dW has exactly m_real*c_real*ntaps floats).
 * workspace: vs_conv_wgrad_workspace_bytes() bytes, contents undefined on entry. */
size_t vs_conv_wgrad_workspace_bytes(int n, int dp, int hp, int wp, int m_ch, int c_ch, int kind);
int vs_conv_wgrad(const void* p, const double* p_stats, const void* q, const double* q_stats, float* dw,
                  void* workspace, size_t workspace_bytes, int n, int dp, int hp, int wp, int m_ch, int c_ch,
                  int m_real, int c_real, int kind, int dtype, float eps, void* stream);
/* The weight (and bias) gradients of MANY conv layers in a handful of launches.  They are leaves of backward — nothing in
 * the pass reads them (the optimiser step of main_source.py:660-661 does, after backward) — so the host side collects one
 * descriptor per layer while autograd walks the graph and issues them together when the pass ends: layers of the same
 * kernel instantiation share one grid, all slab reductions share one.  Per layer the arguments mean what they mean in
 * vs_conv_wgrad; bias_g != NULL additionally requests db[c] = sum over bias_rows of bias_g[bias_rows][bias_c_ch],
 * c < bias_c_real (fixed summation order: bitwise reproducible, unlike vs_bias_grad's float atomics).
 * Descriptors that share `dw` (and `db`) are the uses of ONE weight in this backward pass (a network applied several times, e.g. the VAE
 * inside Embed, joint_model.py:469-500): their contributions are summed — the slabs of all uses feed one reduction — as autograd's
 * accumulation would, without an add launch per use.
 * workspace: vs_conv_wgrad_multi_workspace_bytes() bytes for the same (descs, count, dtype), contents undefined. */
typedef struct vs_wgrad_desc {
    const void* p; const double* p_stats;
    const void* q; const double* q_stats;
    float* dw;
    const void* bias_g; float* db;
    long long bias_rows;
    int bias_c_ch, bias_c_real;
    int n, dp, hp, wp, m_ch, c_ch, m_real, c_real, kind;
    int reserved_;      /* VS_CONV_UP: Co, the channels of the fine tensor p points to; 0 otherwise */
} vs_wgrad_desc;
size_t vs_conv_wgrad_multi_workspace_bytes(const vs_wgrad_desc* descs, int count, int dtype);
int vs_conv_wgrad_multi(const vs_wgrad_desc* descs, int count, void* workspace, size_t workspace_bytes, int dtype,
                        float eps, void* stream);
/* db[c] = sum over rows of g[rows][c_ch], c < c_real (bias gradient of a conv whose bias is live). */
int vs_bias_grad(const void* g, float* db, long long rows, int c_ch, int c_real, int dtype, void* stream);
/* same; accumulate != 0 adds to db instead of overwriting it (a bias used several times in one backward pass) */
int vs_bias_grad_acc(const void* g, float* db, long long rows, int c_ch, int c_real, int dtype, int accumulate, void* stream);

/* ---- InstanceNorm3d + ReLU ---------------------------------------------------------------------- */
/* (sum,sumsq) per (n,c) of x, accumulated into stats (caller zeroes) — only needed when the producer
 * of x was not one of the convs above. */
int vs_instnorm_stats(const void* x, double* stats, int n, long long voxels, int c, int dtype, void* stream);
/* a = relu((x-mean)*rstd) [+ relu((x2-mean2)*rstd2)]  — materialises a lazy activation; with the second
 * operand it is the U-Net skip `up(x)+x3` (joint_model.py:380,382). */
int vs_instnorm_relu_fwd(const void* x, const double* x_stats, const void* x2, const double* x2_stats,
                         void* out, int n, long long voxels, int c, int dtype, float eps, void* stream);
/* backward of a = relu(instnorm(x)) given g = dL/da:
 *   reduce: sums[n][c] = (sum g*[xhat>0], sum g*[xhat>0]*xhat)   (ACCUMULATED, caller zeroes)
 *   apply : gx = rstd * (g*[xhat>0] - mean_v(.) - xhat * mean_v(. * xhat))                                      */
int vs_instnorm_relu_bwd_reduce(const void* g, const void* x, const double* x_stats, double* sums,
                                int n, long long voxels, int c, int dtype, float eps, void* stream);
int vs_instnorm_relu_bwd_apply(const void* g, const void* x, const double* x_stats, const double* sums,
                               void* gx, int n, long long voxels, int c, int dtype, float eps, void* stream);
/* apply with a second gradient of the same raw tensor summed in: gx = round(apply(g)) + add — an activation that feeds both the next
 * encoder level and a U-Net skip (joint_model.py:380,382) receives two gradients; autograd would add them with a kernel of its own. */
int vs_instnorm_relu_bwd_apply_add(const void* g, const void* x, const double* x_stats, const double* sums, const void* add,
                                   void* gx, int n, long long voxels, int c, int dtype, float eps, void* stream);
/* p[0 .. bytes) = 0 (16-byte aligned, bytes a multiple of 16): the per-forward statistics arena (every (sum, sumsq) / IN-backward-sums
 * buffer of a pass is carved from ONE zeroed allocation). */
int vs_zero_fill(void* p, long long bytes, void* stream);
/* The backward of the additive skip a = relu(instnorm(x1)) + relu(instnorm(x2)) (joint_model.py:380,382): one gradient g, both
 * operands' reduce in one launch and both applies in one (sums1 / sums2 ACCUMULATED: caller zeroes; gx1 / gx2 distinct from g). */
int vs_instnorm_relu_bwd_pair(const void* g, const void* x1, const double* x1_stats, double* sums1, void* gx1,
                              const void* x2, const double* x2_stats, double* sums2, void* gx2, int n, long long voxels,
                              int c, int dtype, float eps, void* stream);

/* ---- general normalisation + activation ------------------------------------------------------------------------------------------
 * The settings of joint_model.py's blocks that no entry point of the reference passes: norm_type=2 = nn.BatchNorm3d(C, momentum=0.1)
 * (joint_model.py:12-13, the constructors' default) with its affine pair and running statistics, and soft=True = torch.nn.Softplus()
 * (joint_model.py:38,58,93,104).  Not fused into the convs: the conv writes its raw output and (sum, sumsq) statistics as always and
 * these streaming passes follow; the activation that leaves is a stored tensor.  u = xhat * gamma + beta, xhat = (x - mean) * rstd. */
enum { VS_NORM_INSTANCE = 0, VS_NORM_BATCH = 1, VS_NORM_BATCH_EVAL = 2, VS_NORM_NONE = 3 };   /* per (n,c) | pooled over the batch (training) | running statistics | no normalisation: mean 0, rstd 1 (conv -> activation of the *_GS blocks, joint_model.py:58-63) */
enum { VS_ACT_RELU = 0, VS_ACT_SOFTPLUS = 1 };                               /* Softplus: beta 1, threshold 20 (torch defaults) */
/* mean / rstd tables float[n][c] from a conv epilogue's statistics (double[VS_STAT_SLOTS][n][c][2], `count` voxels per sample).
 * VS_NORM_BATCH: batch mean and biased variance; running_mean / running_var (nullable pair, fp32 [c_real]) take
 * (1-momentum) * old + momentum * (mean | unbiased variance) and *num_batches_tracked (nullable) is incremented — torch.nn.BatchNorm3d
 * in training mode.  VS_NORM_BATCH_EVAL: the tables are the running pair (stats unused). */
int vs_norm_tables(const double* stats, int n, int c, int c_real, double count, int mode, float eps, float momentum,
                   float* running_mean, float* running_var, long long* num_batches_tracked, float* mean, float* rstd, void* stream);
/* y = act(u); channels >= c_real (padding) are written as zeros.  gamma / beta: fp32 [c_real] or NULL (1 / 0). */
int vs_norm_act_fwd(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y, int n,
                    long long voxels, int c, int c_real, int act, int dtype, void* stream);
/* backward, given g = dL/dy:  da = g * act'(u)
 *   reduce: sums[n][c] = (sum da, sum da * xhat)          (double[VS_STAT_SLOTS][n][c][2], ACCUMULATED: caller zeroes)
 *   finish: coef[n][c] = (k, m1, m2) with k = gamma * rstd and (m1, m2) = the means of (da, da * xhat) over the sample (INSTANCE),
 *           over the batch (BATCH) or 0 (BATCH_EVAL);  dgamma[c] = sum_n sum da * xhat, dbeta[c] = sum_n sum da (nullable)
 *   apply : dx = k * (da - m1 - xhat * m2) */
int vs_norm_act_bwd_reduce(const void* g, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           double* sums, int n, long long voxels, int c, int c_real, int act, int dtype, void* stream);
int vs_norm_act_bwd_finish(const double* sums, int n, int c, int c_real, double count, int mode, const float* rstd, const float* gamma,
                           float* coef, float* dgamma, float* dbeta, void* stream);
int vs_norm_act_bwd_apply(const void* g, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                          const float* coef, void* dx, int n, long long voxels, int c, int c_real, int act, int dtype, void* stream);

/* ---- the `*_GS` model family (joint_model.py:17-33, 54-99, 307-346; instantiated nowhere in the reference) ------------------------------
 * GSNorm3d (joint_model.py:17-33): y[c] = x[c] / (sum of x over c's group of c / num_group consecutive channels + 1e-4), per voxel;
 * rows = n * voxels channels-last rows of c channels.  bwd: dx[c] = g[c] / S - (sum_j g[j] x[j]) / S^2. */
int vs_gsnorm_fwd(const void* x, void* y, long long rows, int c, int num_group, int dtype, void* stream);
int vs_gsnorm_bwd(const void* g, const void* x, void* dx, long long rows, int c, int num_group, int dtype, void* stream);
/* torch.nn.Upsample(scale_factor=scale, mode='trilinear') (joint_model.py:69,323-325; align_corners=False): x (n,d,h,w,c) -> y (n,d*s,h*s,w*s,c).
 * bwd: g (upsampled grid) -> dx; scratch = n*d*h*w*c floats (16-byte aligned; zeroed and used for fp32 atomic accumulation by the call). */
int vs_upsample_trilinear_fwd(const void* x, void* y, int n, int d, int h, int w, int c, int scale, int dtype, void* stream);
int vs_upsample_trilinear_bwd(const void* g, void* dx, float* scratch, int n, int d, int h, int w, int c, int scale, int dtype, void* stream);
/* nn.Softmax(dim=1) over two classes as its own pass (Segmentation_GS.final after the 1x1x1 out_block2, joint_model.py:326-327,343-344):
 * channels 0, 1 of channels-last logits -> planar fp32 [n][2][voxels]; its backward is vs_softmax2_bwd. */
int vs_softmax2_fwd(const void* logits, float* prob, int n, long long voxels, int c, int dtype, void* stream);

/* F.dropout(x, p, training=True) on a channels-last tensor (joint_model.py:256-264,379-385): out = x * keep / (1-p),
 * keep ~ Bernoulli(1-p) from a counter-based hash of (seed, element index) — the same call with the same seed applied to
 * the incoming gradient is the backward.  (The reference draws from torch's Philox stream; only the distribution matches.) */
int vs_dropout(const void* x, void* out, long long count, float p, unsigned long long seed, int dtype, void* stream);
/* The multiplier vs_dropout (and the fused logit dropout of vs_conv_k3_softmax2_dropout_fwd) applies to element i, i < count:
 * mask[i] = 0 or 1/(1-p).  Element order: the tensor's own memory order — channels-last [N][V][C] for vs_dropout, planar [N][2][V]
 * for the logits.  Lets a checker feed the SAME mask to the reference arithmetic (F.dropout replaced by a multiply). */
int vs_dropout_mask(float* mask, long long count, float p, unsigned long long seed, void* stream);

/* ---- training data pipeline on the device ---------------------------------------------------------------------------
 * Planar fp32 volumes [D][H][W].  What utils/utils.py's transform chain does per sample on CPU workers (main_source.py:191-211):
 * NumpyLoader_Multi_merge relabelling (utils.py:253-262), CropResize (utils.py:326-383), MySpatialTransform = batchgenerators
 * augment_spatial (utils.py:927-968; rotation, scale, random crop; cubic-spline image / nearest label), Clip + CenterIntensities
 * (utils.py:508-533, 575-618).  The interpolation arithmetic is scipy.ndimage's, which skimage.transform.resize and augment_spatial call. */
/* box6 = {min z, y, x, max z, y, x} of label > 0 (INT_MAX / -1 when there is none) */
int vs_data_bbox(const float* label, int d, int h, int w, int* box6, void* stream);
/* out = target of the last (source -> target) pair whose source equals the label, 0 otherwise; sources / targets: HOST arrays, n_pairs <= 16 */
int vs_data_relabel(const float* in, float* out, long long total, const float* sources, const float* targets, int n_pairs, void* stream);
/* dst[p] = src[p - off + lo] for p - off + lo inside [lo, hi) of the source, 0 elsewhere (crop + np.pad); lo3 / hi3 / off3: HOST arrays */
int vs_data_crop_pad(const float* src, float* dst, int sd, int sh, int sw, int dd, int dh, int dw, const int* lo3, const int* hi3,
                     const int* off3, void* stream);
/* scipy.ndimage.gaussian_filter1d(mode='mirror', truncate=4.0) along one axis (src != dst) */
int vs_data_gaussian_axis(const float* src, float* dst, int d, int h, int w, int axis, float sigma, void* stream);
int vs_data_minmax(const float* x, long long total, float* minmax2, void* stream);
/* scipy.ndimage.zoom(mode='mirror', grid_mode=True), order 0 or 1; order 1 results are clamped to [clip_lo, clip_hi] unless clip_lo > clip_hi.
 * Output index o of an axis reads the input at c = (o + 0.5) * (n_in / n_out) - 0.5, the division first as in scipy (it decides exact order-0 ties);
 * order 0 takes the voxel floor(c + 0.5), mirrored. */
int vs_data_zoom(const float* src, float* dst, int sd, int sh, int sw, int dd, int dh, int dw, int order, float clip_lo, float clip_hi, void* stream);
/* order-3 B-spline coefficients of x in fp64 (scipy.ndimage.spline_filter, mirror boundary) */
int vs_data_spline3_prefilter(const float* x, double* coef, int d, int h, int w, void* stream);
/* dst[o] = sample(src, A (o - (P-1)/2) + ctr), scipy map_coordinates(mode='constant', cval): order 3 (src = the fp64 coefficients) or 0 (src = fp32
 * volume); a9 (row-major 3x3) / ctr3: HOST arrays */
int vs_data_affine_sample(const void* src, float* dst, int sd, int sh, int sw, int pd, int ph, int pw, const double* a9, const double* ctr3, int order,
                          float cval, void* stream);
/* x = (clamp(x, lo, hi) - subtrahend) / divisor, in place */
int vs_data_clip_center(float* x, long long total, float lo, float hi, float subtrahend, float divisor, void* stream);

/* ---- elastic deformation of the spatial augmentation (csrc/elastic.hip) -------------------------------------------------------------------
 * augment_spatial's first stage: per sample a displacement off[k] = scipy.ndimage.gaussian_filter(noise[k], sigma, mode="constant", cval=0) * alpha,
 * k = 0, 1, 2 (z, y, x), noise uniform in [-1, 1), is added to the zero-centred output mesh BEFORE rotation and scale: the input coordinate of output
 * voxel o is A (o - (P - 1) / 2 + off[:, o]) + ctr.  noise / field / tmp: (3, d, h, w) fp64, contiguous, 8-byte aligned, three different buffers.
 *   vs_data_noise_philox   noise[k][v] = 2 u - 1 from Philox4x32-10 with key (seed low 32 bits, seed high 32 bits) and counter (v low 32, v high 32, k,
 *                          sample low 32), v the linear voxel index of one field; u = ((w0 >> 5) 2^26 + (w1 >> 6)) / 2^53 of the first two output
 *                          words, in [0, 1).  A pure function of (seed, sample, k, v): the same bits on every run and in every launch geometry.
 *   vs_data_elastic_field  three separable passes (z, y, x) over all three fields, fp64 throughout; weights exp(-0.5 k^2 / sigma^2) over their sum,
 *                          radius int(4 sigma + 0.5), made on the host and handed over in the kernel arguments; taps beyond the volume are zeros.
 *                          tmp is scratch.  sigma <= 0 or not finite, a radius above 128 (sigma > 32.1), alpha not finite, a null pointer or two
 *                          buffers being one: VS_EINVAL.  alpha == 0 gives zeros.
 *   vs_data_warp_sample    vs_data_affine_sample with field[(k, oz, oy, ox)] added to the zero-centred output coordinate before the matrix; field has
 *                          the patch's shape (3, pd, ph, pw).  The sampler is the same code: a zero field gives vs_data_affine_sample's bits.
 * An empty shape, or fields of 2^31 elements or more: VS_ESHAPE; a misaligned fp64 buffer: VS_EALIGN; all answered on the host before any launch.  No
 * atomics, no memset, nothing allocated, synchronised or read back; one thread writes each output in a fixed order of additions: the same bits on
 * every run, in both builds and under graph replay (1, 3 and 1 launches). */
int vs_data_noise_philox(double* noise, int d, int h, int w, unsigned long long seed, unsigned long long sample, void* stream);
int vs_data_elastic_field(const double* noise, double* field, double* tmp, int d, int h, int w, double sigma, double alpha, void* stream);
int vs_data_warp_sample(const void* src, float* dst, const double* field, int sd, int sh, int sw, int pd, int ph, int pw, const double* a9,
                        const double* ctr3, int order, float cval, void* stream);

/* ---- intensity augmentation (csrc/augment.hip) ---------------------------------------------------------------------------------------------
 * The batchgenerators / nnU-Net intensity set on fp32 planes (d, h, w): an op is computed in fp64 from the fp32 input and from fp64 plane statistics
 * and rounded to fp32 once (DESIGN "Intensity augmentation" states every rule).  A statistics RECORD is four doubles {min, max, mean, population std};
 * the sums are shifted by the plane's first voxel and added over a fixed chunking (8192 voxels) of the linear index in chunk order: a function of the
 * plane's bits alone, whichever entry point makes it.  workspace: vs_aug_stats_workspace_bytes(planes, d, h, w) bytes of scratch, 8-byte aligned.
 *   vs_aug_stats          rec[planes][4] of x[planes][d][h][w]
 *   vs_aug_normal_philox  n[v], v < d h w: pair j = v / 2 from Philox4x32-10 under key (seed low, seed high) and counter (j low, j high, 0x100 + channel,
 *                         sample low); u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53, u2 = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53, r = sqrt(-2 ln u1),
 *                         n[2j] = r cos(2 pi u2), n[2j + 1] = r sin(2 pi u2), fp64
 *   vs_aug_stage          one pass over one plane, in this order, with an fp32 rounding after each step that is present:
 *                           read x at the voxel mirrored by `flip` (z / y / x = 4 / 2 / 1)
 *                           + s n     noise_mode 1: n = noise[] (fp64), 2: n as vs_aug_normal_philox makes it; n is indexed by the OUTPUT voxel when
 *                                     flip_first != 0 (the mirror is the stage's first op) and by the voxel READ otherwise (the mirror is its last op)
 *                           * m       has_mult
 *                           op 1 contrast: (v - mean) p + mean, clamped to [min, max] when flag; op 2 power: v' = -v when flag, then
 *                                     ((v' - min) / (max - min + 1e-7))^p (max - min) + min, negated back; op 3 restat: (v' - mean) / (std + 1e-8) std0
 *                                     + mean0, same negation.  min / max / mean / std: the record `rec` of the plane the op applies to — which the
 *                                     caller has, so an op may share a stage only with steps that FOLLOW it or with the mirror — negated and swapped
 *                                     for v'.  (mean0, std0): the host values, or, when rec0 is given, the mean (negated when flag) and std of rec0.
 *                           store y; when rec_out is given, the record of y (one more small launch; workspace for one plane)
 *   vs_aug_blur           scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=4) of a float32 array: radius int(4 sigma + 0.5), passes along
 *                         z, y, x with fp64 accumulation, each rounded to fp32; weights: a HOST array, the half kernel w[0 .. radius] (w[k]: taps -k
 *                         and +k) as scipy's _gaussian_kernel1d makes it, copied into the kernel arguments.  0 < sigma <= 2, VS_EINVAL beyond.  One
 *                         launch; vs_aug_blur_tile writes the (z, y, x) output tile of a workgroup at that sigma to tile3 (host ints).
 *   vs_aug_flip           y = x mirrored by mask, per plane: a copy
 * x and y are different buffers.  A null pointer, flip / mask outside [0, 7], an unknown mode or op, a parameter that is not finite: VS_EINVAL; an empty
 * plane or one of 2^31 voxels or more: VS_ESHAPE; fp32 buffers not 4-byte, fp64 buffers not 8-byte aligned: VS_EALIGN; all answered on the host before
 * any launch.  No atomics, no memset, nothing allocated, synchronised or read back: the same bits on every run, in both builds and under graph replay. */
long long vs_aug_stats_workspace_bytes(int planes, int d, int h, int w);
int vs_aug_stats(const float* x, double* rec, double* workspace, int planes, int d, int h, int w, void* stream);
int vs_aug_normal_philox(double* n, int d, int h, int w, unsigned long long seed, unsigned long long sample, int channel, void* stream);
int vs_aug_stage(const float* x, float* y, int d, int h, int w, int flip, int flip_first, int noise_mode, const double* noise, double s,
                 unsigned long long seed, unsigned long long sample, int channel, int has_mult, double m, int op, double p, int flag,
                 const double* rec, const double* rec0, double mean0, double std0, double* rec_out, double* workspace, void* stream);
int vs_aug_blur_tile(double sigma, int* tile3);
int vs_aug_blur(const float* x, float* y, int d, int h, int w, double sigma, const double* weights, void* stream);
int vs_aug_flip(const float* x, float* y, int planes, int d, int h, int w, int mask, void* stream);

/* ---- zoom with edge boundaries: simulated low resolution (csrc/lowres.hip) ------------------------------------------------------------------
 * y (dd, dh, dw) = scipy.ndimage.zoom(x.astype(float64), out / in, order, mode="nearest", grid_mode=True) of one fp32 volume x (sd, sh, sw), clipped to
 * [min x, max x] when clip != 0 and order > 0, rounded to fp32 once (DESIGN 3.17 states every rule).  Output index o of an axis of input length m and
 * output length n reads c = (o + 0.5) zoom - 0.5 with zoom = m / n one fp64 division.  order 0: floor(c + 0.5); order 1: two taps per axis, clamped to
 * the axis; order 3: per axis (z, y, x) the line padded by 12 edge values in LDS, scipy's mirror-started order-3 recursion, four taps at c + 12, fp64
 * between the passes.  nnU-Net's simulated low resolution is two calls: down with order 0, up with order 3 and clip.
 * workspace: vs_zoom_edge_workspace_bytes(...) bytes, 8-byte aligned (0 for arguments vs_zoom_edge refuses); needed for order 3 and for a clip.
 * vs_zoom_edge_bundle(m, n): the lines one workgroup of an order-3 pass holds at input length m and output length n (64, 32, 16 or 8; 0 outside 1..512).
 * Launches: order 0 and 1: 1, order 3: 3; a clip adds vs_aug_stats' 2, whose record of x (in the workspace) supplies the bounds on the device.  x and y
 * are different buffers.  A null pointer, an order other than 0, 1, 3: VS_EINVAL; an empty volume, one of 2^31 voxels or more, or for order 3 an axis
 * longer than 512 on either side: VS_ESHAPE; buffers not 4-byte (fp32) / 8-byte (workspace) aligned: VS_EALIGN; all answered on the host before any
 * launch.  No atomics, no memset, nothing allocated, synchronised or read back: the same bits on every run, in both builds and under graph replay. */
long long vs_zoom_edge_workspace_bytes(int sd, int sh, int sw, int dd, int dh, int dw, int order);
int vs_zoom_edge_bundle(int m, int n);
int vs_zoom_edge(const float* x, float* y, int sd, int sh, int sw, int dd, int dh, int dw, int order, int clip, void* workspace, void* stream);

/* ---- layout glue at the NCDHW boundary ----------------------------------------------------------- */
/* planar fp32 [N][c_src][V] -> channels-last [N][V][c_pad] (zero-filled channels >= c_src) */
int vs_pack_planar(const float* src, void* dst, int n, long long voxels, int c_src, int c_pad, int dtype, void* stream);
/* channels-last [N][V][c_pad] -> planar fp32 [N][c_dst][V] */
int vs_unpack_planar(const void* src, float* dst, int n, long long voxels, int c_dst, int c_pad, int dtype, void* stream);
/* backward of the 2-class softmax: glogit[n,v,k] = p_k (g_k - sum_j p_j g_j), written channels-last with c_pad
 * channels (k >= 2 zero).  prob, gprob planar fp32 [N][2][V]. */
int vs_softmax2_bwd(const float* prob, const float* gprob, void* glogit, int n, long long voxels, int c_pad, int dtype, void* stream);
/* same, followed by the backward of the logit dropout of vs_conv_k3_softmax2_dropout_fwd (same p / seed) */
int vs_softmax2_dropout_bwd(const float* prob, const float* gprob, void* glogit, int n, long long voxels, int c_pad, int dtype,
                            float drop_p, unsigned long long drop_seed, void* stream);
/* same with the upstream gradient arriving in two parts: gprob (planar fp32, may be NULL) and gprob_cl (channels-last [n][v][c_pad] in
 * `dtype`, channels 0..1 used, may be NULL) — the gradients of prob and of its channels-last copy (vs_conv_k3_softmax2_cl_fwd). */
int vs_softmax2_cl_bwd(const float* prob, const float* gprob, const void* gprob_cl, void* glogit, int n, long long voxels,
                       int c_pad, int dtype, float drop_p, unsigned long long drop_seed, void* stream);
/* nn.Softmax(dim=1) over n_class = 1..8 classes as its own pass (joint_model.py:225,266 / 367,388 with a label set of more than one structure:
 * main_source.py:92-93 makes n_class = 1 + the number of --pan_index entries; the two-class case has the fused kernels above).
 * fwd: channels 0..n_class-1 of channels-last logits [n][v][c_pad] -> planar fp32 prob [n][n_class][v]; drop_p > 0 first applies
 * F.dropout to the logits (joint_model.py:386-387; element index = planar index into [n][n_class][v]).
 * bwd: glogit[n,v,k] = p_k (g_k - sum_j p_j g_j) (then the dropout's backward), written channels-last with c_pad channels, k >= n_class zero. */
int vs_softmax_cl_fwd(const void* logits, float* prob, int n, long long voxels, int c_pad, int n_class, int dtype, float drop_p,
                      unsigned long long drop_seed, void* stream);
int vs_softmax_cl_bwd(const float* prob, const float* gprob, void* glogit, int n, long long voxels, int c_pad, int n_class, int dtype,
                      float drop_p, unsigned long long drop_seed, void* stream);
/* label (float, values 0..n_class-1) [N][1][V] -> one-hot planar fp32 [N][n_class][V]   (main_source.py:449-451) */
int vs_onehot(const float* label, float* out, int n, long long voxels, int n_class, void* stream);
/* hard masks of the validation Dice (utils/evaluation.py:58-64: torch.argmax over channels -> scatter_ into zeros): x, out planar
 * (n, n_class, voxels) fp32; out[b][k][v] = (k == argmax_k' x[b][k'][v]), ties to the first maximal channel as torch.argmax; any n_class >= 1 */
int vs_hard_onehot(const float* x, float* out, int n, int n_class, long long voxels, void* stream);
/* mode 0: (a >= 0.5) ; mode 1: a>hi -> 1, a<lo -> 0, else a        (utils/evaluation.py:9-18) */
int vs_binarize(const float* a, float* out, long long count, int mode, float lo, float hi, void* stream);

/* ---- connected components of a prediction (csrc/cc.hip) ---------------------------------------------------------------------------------
 * mask: planar fp32 (n, c, d, h, w), contiguous; foreground is value >= 0.5 (the binarize rule, utils/evaluation.py:9-10); every (n, c)
 * plane is an independent problem; any d, h, w >= 1 with d*h*w < 2^31 (VS_ESHAPE beyond).  connectivity: 26 (what the reference uses:
 * utils/utils.py:20-57 Tag scans the 3x3x3 neighbourhood, utils/utils.py:776-796 predict_vol sets SetFullyConnected(True)) or 6; neighbours
 * never wrap from one row to the next and the volume border is background.
 * labels: int32 (n, c, d, h, w); 0 = background, components numbered 1..K per plane in the order of their first voxel in raster order
 * (z slowest, x fastest) — the numbering of scipy.ndimage.label and of the reference's check_connection(np.argwhere(mask), mask).
 * counts: int32 (n, c) = K.  The per-plane size table — int32 [n * c][maxk], sizes[label - 1] = voxels, zero beyond K — is written to the
 * START of the workspace; maxk = ceil(d/2) * ceil(h/2) * ceil(w/2) for connectivity 26, ceil(d*h*w / 2) for 6 (the most components a plane can hold).
 * Only 32-bit integer atomics are used and the result does not depend on their order: both builds of the library give the same bits.
 * No kernel waits for another workgroup (every phase is a launch, every loop is bounded by the data), nothing is read back: a call is a
 * straight line of launches that can be captured in a HIP graph.  workspace: vs_cc_workspace_bytes() bytes (negative: VS_E*), 16-byte aligned,
 * contents undefined on entry; mask / labels / out 16-byte aligned.  Bad arguments are answered on the host: connectivity not 6 / 26, k < 0,
 * lo_channel outside [0, c): VS_EINVAL; an empty or too large shape: VS_ESHAPE. */
long long vs_cc_workspace_bytes(int n, int c, int d, int h, int w, int connectivity);
/* utils/utils.py:20-57 (Tag / check_connection): the component labels of every plane */
int vs_cc_label(const float* mask, int* labels, int* counts, int n, int c, int d, int h, int w, int connectivity, void* workspace, void* stream);
/* utils/utils.py:776-796 (predict_vol step 2: ConnectedComponent -> RelabelComponent by size -> drop all but the largest -> re-binarise; it hard-codes
 * k = 2, min_size = 10000): out[v] = 1.0 where v's component is among the k largest of its plane AND holds at least min_size voxels, 0.0 elsewhere.
 * Components of equal size rank by label, the lower one (the earlier first voxel) first — a rule of this library: SimpleITK's tie order is unspecified.
 * Channels below lo_channel are not labelled: they are copied to out; with to_background != 0 and lo_channel >= 1 every removed voxel is added to
 * channel 0 (a one-hot tensor stays one-hot).  out must not alias mask.  Labels, counts and sizes of the call stay in the workspace. */
int vs_cc_keep_largest(const float* mask, float* out, int n, int c, int d, int h, int w, int connectivity, int k, int min_size, int lo_channel,
                       int to_background, void* workspace, void* stream);

/* ---- surface distances of two masks (csrc/surface.hip) ---------------------------------------------------------------------------------------
 * The validation metrics the segmentation literature reports next to Dice — ASSD, Hausdorff distance, HD95 — in medpy's convention
 * (medpy.metric.binary.assd / hd / hd95 over scipy.ndimage), and their building block, an exact Euclidean distance transform.  The reference has no
 * such metric.  Masks are planar fp32 (n, c, d, h, w), contiguous, foreground where the value is >= 0.5; every (n, c) plane is its own problem.
 *   surface   S(X) = X & ~binary_erosion(X, structure, border_value=0): a foreground voxel with a background or out-of-volume neighbour among its 6
 *             (connectivity 6, the default of medpy) or 26 neighbours.
 *   distance  dist_F(v)^2 = min over voxels u of F of (sz dz)^2 + (sy dy)^2 + (sx dx)^2; spacing = HOST array {sz, sy, sx}, or NULL for unit spacing.
 *             spacing == NULL: int32 squared distances, exact, INT32_MAX where the plane has no feature voxel; otherwise doubles, +inf there.
 *             A min over exact candidates (unit spacing) / over the same rounded candidates (doubles): both builds of the library and every run
 *             give the same bits; there are no atomics in this file.
 *   record    per plane, for A = pred, B = gt and the directed sets d(A->B) = { dist_S(B)(v) : v in S(A) }, d(B->A) likewise:
 *             count_ab, count_ba  their sizes                       sum_ab, sum_ba  the sums of the distances (a fixed summation tree)
 *             max_sq              the largest squared distance      lo_sq, hi_sq    the squared order statistics v[k]^2, v[k+1]^2 of the union,
 *                                                                                   k = floor(0.95 (count_ab + count_ba - 1)), 0-based, ascending
 *             assd = (sum_ab / count_ab + sum_ba / count_ba) / 2    hd = sqrt(max_sq)
 *             hd95 = numpy.percentile(union, 95), the default linear rule: v[k] + (0.95 (n - 1) - k) (v[k+1] - v[k])
 *             A plane in which S(A) or S(B) is empty has both counts 0 and every other field NaN (medpy raises; a device op cannot).
 * Limits: d, h <= 1024 (a line of the y / z passes is staged in LDS), d*h*w < 2^31, and d^2 + h^2 + w^2 < 2^31 - 1 for unit spacing: VS_ESHAPE beyond,
 * as for an empty shape.  connectivity not 6 / 26, a spacing that is not positive and finite, a null pointer, an output that is one of the inputs:
 * VS_EINVAL.  mask / out / workspace not 16-byte aligned: VS_EALIGN.  All of this is answered on the host before any launch.
 * A call is a straight line of launches — no kernel waits for another workgroup, every loop is bounded by the data, nothing is allocated,
 * synchronised or read back — and can be captured in a HIP graph. */
typedef struct vs_surface_record {
    long long count_ab, count_ba;
    double sum_ab, sum_ba;
    double max_sq, lo_sq, hi_sq;
    double assd, hd, hd95;
} vs_surface_record;
/* out (fp32, mask's shape) = 1.0 on S(mask), 0.0 elsewhere */
int vs_surface(const float* mask, float* out, int n, int c, int d, int h, int w, int connectivity, void* stream);
/* out[v] = dist_F(v)^2 for F = { feature >= 0.5 }: int32 (spacing == NULL) or double, feature's shape.  The transform works in `out`: no workspace. */
int vs_edt(const float* feature, void* out, int n, int c, int d, int h, int w, const double* spacing, void* stream);
/* bytes of the workspace of vs_surface_distances (negative: VS_E*); with_spacing != 0: the double path.  Both surfaces as bytes, both distance maps
 * and the list of surface distances: 18 bytes per voxel of one mask for unit spacing, 34 with a spacing, plus 32 / 40 bytes per 4096 voxels. */
long long vs_edt_workspace_bytes(int n, int c, int d, int h, int w, int with_spacing);
/* out: vs_surface_record[n * c].  workspace: 16-byte aligned, contents undefined on entry; the maps and surfaces of the call stay in it. */
int vs_surface_distances(const float* pred, const float* gt, vs_surface_record* out, int n, int c, int d, int h, int w, int connectivity,
                         const double* spacing, void* workspace, void* stream);

/* ---- binary morphology and hole filling of a prediction (csrc/morph.hip) ------------------------------------------------------------------
 * scipy.ndimage's binary_dilation / binary_erosion / binary_opening / binary_closing (structure = generate_binary_structure(3, 1) for connectivity
 * 6, (3, 3) for 26; iterations; border_value; origin 0, no mask) and binary_fill_holes(X, structure).  The reference dilates its bone mask with
 * binary_dilation(iterations=2) (utils/utils.py:647-655, get_synthesis_mask).  mask: planar fp32 (n, c, d, h, w), contiguous, foreground where the
 * value is >= 0.5; every (n, c) plane is its own problem; any d, h, w >= 1 with d*h*w < 2^31 (VS_ESHAPE beyond, as for an empty shape).  out: fp32
 * 0 / 1, mask's shape, must not alias mask.
 *   vs_morph       voxels outside the volume read as border_value (0 or 1) in BOTH halves of an opening (erode^n then dilate^n) or closing
 *                  (dilate^n then erode^n), as scipy passes it on.  The mask is packed to one bit per voxel (64-bit words along x); connectivity 26
 *                  with n iterations is the box of half-width n, done as three axis passes: 5 launches (8 for open / close) whatever n is.
 *                  Connectivity 6 is the L1 ball, one launch per step: n + 2 launches (2 n + 2), n capped at d + h + w where the result is fixed.
 *   vs_fill_holes  out = the complement of the background voxels that reach the outside of the volume through `connectivity`-neighbours
 *                  (scipy's default structure is connectivity 6).  The complement is labelled with the union-find of csrc/cc_core.h, the roots of
 *                  the background voxels on the six faces are marked, every voxel reads its root's mark: 4 launches.
 * connectivity not 6 / 26, op outside VS_MORPH_*, iterations < 1, border_value not 0 / 1, a null pointer, out or workspace aliasing mask:
 * VS_EINVAL; workspace not 16-byte aligned: VS_EALIGN; all answered on the host before any launch.  workspace: vs_*_workspace_bytes() bytes
 * (negative: VS_E*), contents undefined on entry.  A call is a straight line of launches — no kernel waits for another workgroup, every loop is
 * bounded by the data, nothing is allocated, synchronised or read back — and can be captured in a HIP graph.  The results are sets: both builds of
 * the library and every run give the same bits (vs_morph has no atomics; vs_fill_holes only the order-independent atomicMin of the union-find). */
enum { VS_MORPH_DILATE = 0, VS_MORPH_ERODE = 1, VS_MORPH_OPEN = 2, VS_MORPH_CLOSE = 3 };
long long vs_morph_workspace_bytes(int n, int c, int d, int h, int w);
int vs_morph(const float* mask, float* out, int n, int c, int d, int h, int w, int op, int connectivity, int iterations, int border_value,
             void* workspace, void* stream);
long long vs_fill_holes_workspace_bytes(int n, int c, int d, int h, int w, int connectivity);
int vs_fill_holes(const float* mask, float* out, int n, int c, int d, int h, int w, int connectivity, void* workspace, void* stream);

/* ---- per-component measurements and the contingency table of label volumes (csrc/regions.hip; no counterpart in the reference) -------------
 * What scipy.ndimage.find_objects / np.bincount give on the host, for int32 label volumes (n, c, d, h, w) as vs_cc_label writes them: 0 is
 * background, 1..K are components (or classes); every (n, c) plane is its own problem; any d, h, w >= 1 with d*h*w < 2^31.
 *   vs_region_props  table: int64 (n, c, max_rows, 10), row r for label r + 1, columns
 *                        count, zmin, ymin, xmin, zmax, ymax, xmax, sum_z, sum_y, sum_x      (box inclusive; sums of the voxel indices)
 *                    a label that does not occur has count 0, mins (d, h, w), maxes -1, sums 0.
 *   vs_contingency   table: int64 (n, c, rows_a + 1, rows_b + 1), table[i][j] = voxels with a == i and b == j; row / column 0 are background.
 *                    (rows_a + 1) * (rows_b + 1) <= 2^22 per plane (VS_ESHAPE beyond).  Tables of at most 4096 cells are summed per workgroup in LDS.
 *   overflow         int32 (n, c): the voxels whose label (on either side) is negative or above max_rows / rows_a / rows_b.  They are counted
 *                    there and in no row or cell.
 * The caller owns every buffer and need not clear them: the first launch of a call writes the initial state, the second accumulates — nothing
 * is allocated, synchronised or read back, no kernel waits for another workgroup, and a call can be captured in a HIP graph.  Every accumulator is
 * an integer updated with atomicAdd / atomicMin / atomicMax by vector lanes, one update per RUN of equal labels along x (per wave and chunk of
 * rows for the label a wave currently carries), so the tables do not depend on the order of arrival: both builds of the library and every run
 * give the same bits.  a and b may be the same buffer.  A null pointer, max_rows < 1, rows_a or rows_b < 0: VS_EINVAL; an empty or too large
 * shape or table: VS_ESHAPE; labels not 4-byte, table not 8-byte aligned: VS_EALIGN; all answered on the host before any launch. */
int vs_region_props(const int* labels, int n, int c, int d, int h, int w, int max_rows, long long* table, int* overflow, void* stream);
int vs_contingency(const int* a, const int* b, int n, int c, int d, int h, int w, int rows_a, int rows_b, long long* table, int* overflow,
                   void* stream);

/* ---- intensity histograms, joint histograms and mutual information (csrc/hist.hip) -------------------------------------------------------
 * np.histogram / np.histogram2d of volumes and the tail of the reference's mutual_information_3d (utils/utils.py:804-845) without the host.  x, y:
 * planar fp32 (n, c, d, h, w), contiguous; every (n, c) plane is its own problem; any d, h, w >= 1 with d*h*w < 2^31.  Counts are int64.
 * The binning rule (it does not follow numpy's dtype rules):
 *   edges     for bins = B >= 1 and bounds lo <= hi the B + 1 edges are the fp64 values with the bits of np.linspace(lo, hi, B + 1):
 *             step = (hi - lo) / B, e_i = i * step + lo with the product and the sum rounded separately (no fused multiply-add), e_B = hi.
 *             lo == hi becomes (lo - 0.5, hi + 0.5) first.  They are written to the caller's buffer, fp64 (n, c, B + 1).
 *   bin       a voxel x, promoted to fp64, is in bin i iff e_i <= x < e_{i+1}; x == e_B is in bin B - 1.  The kernels estimate the bin as
 *             (x - e_0) * B / (e_B - e_0) and then walk the edge table until that inequality holds.
 *   outside   int64 (n, c): NaN, +-inf and values outside [e_0, e_B] are counted there and in no bin.
 *   bounds    from_data == 0: the host doubles given, for all planes (not finite or lo > hi: VS_EINVAL).  from_data != 0: per plane, on the device
 *             and without a synchronisation, lo / hi = the minimum / maximum over the plane's FINITE voxels (a zero bound is +0.0); a plane
 *             without a finite voxel gets (0, 0), hence (-0.5, 0.5).  The running extrema live in the plane's own edge table until it is written.
 *   vs_histogram        table: int64 (n, c, rows + 1, bins).  labels == NULL: rows is 0, one row.  Otherwise labels is an int32 volume of x's shape
 *                       as vs_cc_label or an argmax writes it and row r is the histogram of the voxels labelled r; voxels whose label is negative or
 *                       above rows are counted in overflow, int32 (n, c), and nowhere else (vs_contingency's rule).  bins <= 4096 and
 *                       (rows + 1) * bins <= 2^22, VS_ESHAPE beyond.  lo, hi: the host bounds.
 *   vs_joint_histogram  table: int64 (n, c, bins_x, bins_y); a voxel counts in cell (bin of x, bin of y) iff both values are in range, otherwise in
 *                       outside.  range4: host doubles (lo_x, hi_x, lo_y, hi_y), not read with from_data.  bins_x * bins_y <= 2^22.
 * Three counting kernels, chosen by the cells of one plane's table: up to 8192 cells 32-bit counters in LDS; up to 65536 cells (256 x 256) two 16-bit
 * counters per LDS word, 128 KB, where a workgroup flushes to the int64 table after 16384 voxels — fewer than 2^16, so no half can carry; larger tables
 * one 64-bit global atomic per run, with the cell a wave currently sees most carried in registers.  In all of them a run of equal cells along x is one
 * update of the run's length.  vs_config.hist_form forces a form for measurements; the tables do not depend on it.
 *   vs_mutual_information  table: int64 (n, c, bins_x, bins_y) as vs_joint_histogram writes it -> mi: fp64 (n, c), all in fp64:
 *                       scipy.ndimage.gaussian_filter(jh, sigma, mode="constant") — the separable kernel of radius int(4 * sigma + 0.5), weights
 *                       exp(-k^2 / (2 sigma^2)) over their sum, along x then y, zeros beyond the table; sigma == 0 skips it — then + eps
 *                       (2^-52), division by the total, the two marginals s1, s2 and  normalized ? (sum s1 log s1 + sum s2 log s2) / sum jh log jh - 1
 *                       : sum jh log jh - sum s1 log s1 - sum s2 log s2.  sigma < 0, NaN or a radius above 64: VS_EINVAL; n * c <= 65535.
 *                       workspace: n * c * (2 * bins_x * bins_y + 2 * bins_x + bins_y) doubles, contents undefined on entry.  Every sum runs in a
 *                       fixed order (strided partials, then a tree per workgroup), there are no floating-point atomics: the same bits on every
 *                       run, in both builds and under graph replay.
 * The caller owns every buffer and need not clear them: the first launch of a call writes the initial state.  Nothing is allocated, synchronised or
 * read back, no kernel waits for another workgroup, every call can be captured in a HIP graph (3 launches with host bounds, 4 from the data; 4 or 5
 * for the mutual information).  Every count is an integer added with vector-lane atomics, so the tables do not depend on the order of arrival:
 * both builds of the library and every run give the same bits.  A null pointer, bins < 1, rows < 0 (or != 0 without labels), edges_x == edges_y:
 * VS_EINVAL; an empty or too large shape or table: VS_ESHAPE; x, y, labels, overflow not 4-byte, the other buffers not 8-byte aligned: VS_EALIGN;
 * all answered on the host before any launch. */
int vs_histogram(const float* x, const int* labels, int n, int c, int d, int h, int w, int bins, int rows, double lo, double hi, int from_data,
                 double* edges, long long* table, long long* outside, int* overflow, void* stream);
int vs_joint_histogram(const float* x, const float* y, int n, int c, int d, int h, int w, int bins_x, int bins_y, const double* range4, int from_data,
                       double* edges_x, double* edges_y, long long* table, long long* outside, void* stream);
int vs_mutual_information(const long long* table, int n, int c, int bins_x, int bins_y, double sigma, int normalized, double* workspace, double* mi,
                          void* stream);

/* ---- exact percentiles and the piecewise-linear intensity map (csrc/quantile.hip) -------------------------------------------
 * x: planar fp32 (planes, d, h, w), contiguous; every plane is its own problem; d*h*w < 2^31.
 *   vs_quantile  A voxel is SELECTED iff it is finite, use_above == 0 or x > above (strict fp32 comparison), and mask == NULL or its mask byte
 *                (uint8, x's shape) is not 0.  Non-finite voxels are never selected and are counted in rejected, whatever the selectors say.
 *                With v[0] <= ... <= v[n-1] the selected values in fp64 and p01[i] in [0, 1] (HOST doubles, Q of them, 1 <= Q <= 16):
 *                h = (double)(n - 1) * p01, k = floor(h), k1 = min(k + 1, n - 1), t = h - k, a = v[k], b = v[k1], d = b - a,
 *                q_out = t >= 0.5 ? b - d * (1 - t) : a + d * t, every product and sum rounded separately (no fused multiply-add): the bits of
 *                np.percentile(selected.astype(np.float64), 100 * p01).  lo_out = (float)a, hi_out = (float)b.  n == 0: the three are NaN.
 *                q_out: fp64 (planes, Q); lo_out, hi_out: fp32 (planes, Q); count = n and rejected: int64 (planes).
 *                A radix select over the order-preserving integer image of the fp32 bits, four passes of 8 bits for the 2 Q ranks at once; NINE
 *                launches whatever the data.  workspace: vs_quantile_workspace_bytes(planes, d*h*w, Q) bytes (0 for arguments vs_quantile refuses),
 *                16-byte aligned, contents undefined on entry: the first launch writes its initial state.
 *   vs_intensity_map  src: fp64 (planes, L) in DEVICE memory, ascending landmarks per plane (vs_quantile's q_out); dst: fp64 (L) in device memory,
 *                strictly ascending; 2 <= L <= 16.  For a finite voxel x, j = the largest index in [0, L - 2] with src[j] <= x (0 when x < src[0]),
 *                w = src[j+1] - src[j], slope = w > 0 ? (dst[j+1] - dst[j]) / w : 0, y = dst[j] + (x - src[j]) * slope in fp64, products and sums
 *                rounded separately, rounded to fp32 once.  clamp 0: the end segments run on; clamp 1: y is clamped to [dst[0], dst[L-1]].  A
 *                non-finite voxel is written unchanged; a plane with a NaN landmark (nothing was selected) is copied.  One launch; y may be x.
 * Nothing is allocated, synchronised or read back; no kernel waits for another workgroup; both calls can be captured in a HIP graph.  Every count is an
 * integer added with vector-lane atomics: the same bits on every run, under replay and in both builds.  A null pointer (mask may be NULL), Q outside
 * [1, 16], a p01 that is NaN or outside [0, 1], a NaN threshold, L outside [2, 16], clamp outside {0, 1}: VS_EINVAL; an empty plane or one of 2^31
 * voxels or more: VS_ESHAPE; x, y, lo_out, hi_out not 4-byte, q_out, count, rejected, src, dst not 8-byte, workspace not 16-byte aligned: VS_EALIGN;
 * all answered on the host before any launch. */
size_t vs_quantile_workspace_bytes(int planes, long long V, int Q);
int vs_quantile(const float* x, const unsigned char* mask, int use_above, float above, const double* p01, int Q, double* q_out, float* lo_out,
                float* hi_out, long long* count, long long* rejected, void* workspace, int planes, int d, int h, int w, void* stream);
int vs_intensity_map(const float* x, const double* src, const double* dst, int L, int clamp, float* y, int planes, int d, int h, int w, void* stream);

/* ---- training patches: foreground-oversampled windows of an unscaled volume, cut on the device (csrc/patch.hip) -------------------
 * A training batch is made of windows of (pd, ph, pw) voxels cut from a volume (d, h, w); a share of them is forced to contain a uniformly chosen
 * voxel of a uniformly chosen class that is present.  All arithmetic is integer; nothing here is inherited from another loader's random stream.
 *   classes   A voxel of the label belongs to class k iff its value is the integer k, 0 <= k < n_class <= 8; any other value (NaN, a fraction, a
 *             value >= n_class) belongs to no class.  label: fp32 (VS_PATCH_F32) or uint8 (VS_PATCH_U8), (d, h, w) contiguous, d*h*w < 2^31.
 *   bounds    per axis, volume side S and patch side P: need = max(P - S, 0), lb = -(need / 2), ub = S + need / 2 + need % 2 - P.  S >= P gives
 *             [0, S - P]; S < P gives lb == ub, the volume centred in the patch.
 *   request   five unsigned 32-bit words (wc, wv, wz, wy, wx) and a flag `forced`.  A word w maps to a range of m values as (w * m) >> 32 with a
 *             64-bit product: no rejection, no floating point.
 *   forced    present = the classes of the call's list whose voxel count n_k is > 0, ascending, mc of them.  mc > 0: k = present[(wc * mc) >> 32],
 *             rank r = (wv * n_k) >> 32, v = the r-th voxel of class k in ascending linear index (z * h + y) * w + x, and per axis
 *             o = min(max(lb, v - P / 2), ub): the patch contains v.  mc == 0: the request is treated as free.
 *   free      per axis o = lb + ((w_axis * (ub - lb + 1)) >> 32); wc and wv are not looked at.
 * vs_patch_index  table: int32 [n_chunks + 1][n_class], n_chunks = ceil(d*h*w / VS_PATCH_CHUNK): row j holds the number of voxels of each class in
 *             the chunks before chunk j (a chunk is VS_PATCH_CHUNK consecutive voxels of the linear index), the last row the totals.  Two launches:
 *             workgroups count whole chunks with wave ballots and store one word per (chunk, class); one workgroup per class scans its column.
 *             vs_patch_index_bytes: the table's size (0 for arguments vs_patch_index refuses); vs_patch_chunk: VS_PATCH_CHUNK.
 * vs_patch_pick   words: uint32 [r][5], forced: int32 [r], both in DEVICE memory; the class list by value: n_sel <= 8 strictly ascending classes, class
 *             i in bits [3 i, 3 i + 3) of `classes`.  picks: int32 [r][8] = (oz, oy, ox, k, vz, vy, vx, 0) for a forced request, (oz, oy, ox, -1, -1,
 *             -1, -1, 0) for a free one.  One wave per request: totals, binary search of the chunk in the class's column, a walk through the chunk 64
 *             voxels at a time (ballot, popcount) to the r-th match.  label and table are those of vs_patch_index; a table that does not belong to the
 *             label cannot send a read out of bounds (the request then falls to a free origin).
 * vs_patch_gather n_src <= 4 fp32 volumes (d, h, w), the pointers and a cval per source by value; out: fp32 (n_src, r, qd, qh, qw) with q = p + 2 margin
 *             per axis, out[s][i][z][y][x] = src_s[o_i - margin + (z, y, x)] where that lies inside the volume and cval_s elsewhere; o_i = picks[i][0..2]
 *             read from DEVICE memory — any integers, negative ones and ones past the volume included.  A thread owns four x of an output row.
 * No atomics, no memset, nothing allocated, synchronised or read back; every call can be captured in a HIP graph and gives the same bits eagerly, under
 * replay and in both builds.  A null pointer, n_class outside [1, 8], a class list that is not strictly ascending inside [0, n_class), r < 1, a patch
 * side < 1, margin < 0, n_src outside [1, 4], a NaN cval, out equal to a source: VS_EINVAL; an unknown label type: VS_EDTYPE; an empty volume, one of
 * 2^31 voxels or more, an output block of 2^31 voxels or more: VS_ESHAPE; an fp32 / int32 buffer not 4-byte, picks, sources or out not 16-byte aligned:
 * VS_EALIGN; all answered on the host before any launch. */
#define VS_PATCH_CHUNK 4096
enum { VS_PATCH_F32 = 0, VS_PATCH_U8 = 1 };
int vs_patch_chunk(void);
size_t vs_patch_index_bytes(int d, int h, int w, int n_class);
int vs_patch_index(const void* label, int dtype, int d, int h, int w, int n_class, int* table, void* stream);
int vs_patch_pick(const void* label, int dtype, const int* table, int n_class, int n_sel, int classes, const unsigned int* words, const int* forced,
                  int r, int d, int h, int w, int pd, int ph, int pw, int* picks, void* stream);
int vs_patch_gather(const float* src0, const float* src1, const float* src2, const float* src3, float cval0, float cval1, float cval2, float cval3,
                    int n_src, const int* picks, int r, int d, int h, int w, int pd, int ph, int pw, int margin, float* out, void* stream);

/* ---- sliding-window prediction of a whole volume (csrc/window.hip; no counterpart in the reference) -------------------------------
 * A volume (C, D, H, W) is tiled with overlapping cubic windows of side `patch`, a network maps batches (B, C, P, P, P) of them to planar
 * probabilities (B, K, P, P, P), and the windows are blended: prob[k][v] = sum_i w_i(v) p_i[k](v) / sum_i w_i(v) over the windows i that cover
 * v, with a separable importance map w = (wz[lz] * wy[ly]) * wx[lx] (fp32, rounded after each product) of the voxel's position in the window.
 * All tensors are planar fp32, 16-byte aligned.  No call synchronises; none uses atomics: the sums are bit-identical for every batch size,
 * from run to run and between the two builds of the library.
 *
 * vs_sw_plan (host only): per axis step = max(1, floor(patch * (1 - overlap))), n = 1 if S <= patch else ceil((S - patch) / step) + 1, the
 * origin of window i is min(i * step, max(S - patch, 0)).  -> the number of windows nw (negative: VS_E*); with origins != NULL also the table
 * int[nw][3] = (z, y, x) of every window, D-major, then H, then W (capacity: the entries origins has room for).  0 <= overlap < 1. */
int vs_sw_plan(int d, int h, int w, int patch, double overlap, int* origins, int capacity);
/* batch[s] = window first[0] + s of the plan (origins: the DEVICE copy of the table) for s < b; `first` is a DEVICE word, so a launch captured
 * into a HIP graph serves every batch.  Slots with first[0] + s >= nw are filled with cval, as are positions past the volume (S < patch). */
int vs_sw_gather(const float* volume, float* batch, const int* origins, const int* first, int nw, int b, int c, int d, int h, int w, int patch,
                 float cval, void* stream);
/* acc[k][v] = fmaf(w, prob[s][k][v - origin], acc[k][v]) and wsum[v] += w for every slot s < b with first[0] + s < nw and every voxel v of its
 * window inside the volume; a voxel's terms are added in ascending window index (batches must be accumulated in ascending order of `first`).
 * acc (k, d, h, w) and wsum (d, h, w) start as zeros; wz, wy, wx: `patch` floats each, on the device. */
int vs_sw_accumulate(const float* prob, float* acc, float* wsum, const int* origins, const int* first, int nw, int b, int k, int d, int h, int w,
                     int patch, const float* wz, const float* wy, const float* wx, void* stream);
/* Mirror test-time augmentation of the two calls above.  A flip is a 3-bit code: bit 0 mirrors W (x), bit 1 mirrors H (y), bit 2 mirrors D (z), a
 * mirrored axis reading f(i) = patch - 1 - i.  A pass has nf distinct codes, 1 <= nf <= 8, handed over by value: code i in bits [3 i, 3 i + 3) of
 * `codes`, nothing set above them (VS_EINVAL otherwise).  first[0] now counts ITEMS: item j is window j / nf under flip code j % nf, there are
 * nw * nf of them (VS_ESHAPE when nw * nf + b passes INT_MAX), and a batch may hold several flips of one window.
 * vs_sw_gather_tta: batch[s][c][z][y][x] = window(item first[0] + s)[c][fz(z)][fy(y)][fx(x)] — the whole padded window is mirrored, so positions
 * past the volume (S < patch) put their cval at the low end; slots with first[0] + s >= nw * nf are cval. */
int vs_sw_gather_tta(const float* volume, float* batch, const int* origins, const int* first, int nw, int b, int c, int d, int h, int w, int patch,
                     float cval, int nf, int codes, void* stream);
/* vs_sw_accumulate_tta: acc[k][v] = fmaf(w(l), prob[s][k][f(l)], acc[k][v]) and wsum[v] += w(l) with l = v - origin: the network's answer is read
 * mirrored back, the weight is taken at the un-mirrored position.  A voxel's terms are added in ascending item index, one writer per voxel and
 * no atomics, as vs_sw_accumulate: bit-identical for every b (it need divide neither nf nor nw * nf), from run to run and between the two
 * builds.  vs_sw_finalize follows unchanged (wsum is nf times larger).  With nf = 1 and code 0 both calls give the bits of the plain ones. */
int vs_sw_accumulate_tta(const float* prob, float* acc, float* wsum, const int* origins, const int* first, int nw, int b, int k, int d, int h, int w,
                         int patch, const float* wz, const float* wy, const float* wx, int nf, int codes, void* stream);
/* prob = acc / wsum (prob may be acc itself); label (may be NULL): the channel argmax as bytes (k <= 255; ties: the first maximal channel, a
 * NaN channel wins, as vs_hard_onehot); onehot (may be NULL): the label's planar fp32 one-hot (k, d, h, w). */
int vs_sw_finalize(const float* acc, const float* wsum, float* prob, unsigned char* label, float* onehot, int k, int d, int h, int w, void* stream);

/* ---- a crop-space prediction pasted back into scan geometry (csrc/uncrop.hip; no counterpart in the reference) ---------------------
 * data_gpu.CropResize cuts the scan rows [lo, hi) of every axis, places them at [off, off + hi - lo) of a zero cube of side `side` and resizes the
 * cube to patch^3 (data_gpu.crop_geometry gives lo, hi, off, side for a box).  vs_uncrop is the way back for the network's answer on that patch:
 * prob (k, patch, patch, patch), planar fp32, 1 <= k <= 8, is resampled onto the scan grid (d, h, w).
 *   A scan voxel v with lo <= v < hi on every axis has cube index u = v - lo + off and patch coordinate q = (u + 0.5) * patch / side - 0.5 per axis,
 *   the inverse of vs_data_zoom's grid (skimage / scipy.ndimage.zoom(grid_mode=True)), computed in fp64.
 *   interp 1 (linear): q is clamped to [0, patch - 1] (edge replicate) and each class is interpolated trilinearly, weights and the eight products
 *   in fp64, the sum rounded to fp32 once: scipy.ndimage.zoom(prob[c], side / patch, order=1, mode='nearest', grid_mode=True) on the cube rows that
 *   exist in the scan.  interp 0 (nearest): the sample at index floor(q + 0.5), clamped - the rounding of vs_data_zoom's order 0.
 *   Every other voxel lies outside the cube: probability 1 in channel 0 and 0 in the others.
 * label (d, h, w) bytes: the channel argmax of those fp32 probabilities, ties to the first maximal channel, a NaN channel wins (vs_hard_onehot,
 * vs_sw_finalize); 0 outside the cube.  prob_out (may be NULL): the resampled probabilities, planar fp32 (k, d, h, w).
 * One launch writes every element of label and prob_out exactly once: no memset before it, no atomics, bit-identical from run to run and between
 * the two builds.  It does not synchronise.  Pointers are 16-byte aligned (VS_EALIGN); a geometry with lo < 0, hi < lo, hi > the scan's size,
 * off < 0 or off + hi - lo > side, side <= 0, k outside [1, 8] or interp outside {0, 1}: VS_EINVAL, on the host before any launch.  The kernel
 * clamps every patch index itself and bounds its stores by (d, h, w) alone. */
int vs_uncrop(const float* prob, unsigned char* label, float* prob_out, int k, int patch, int d, int h, int w, int lo_z, int lo_y, int lo_x,
              int hi_z, int hi_y, int hi_x, int off_z, int off_y, int off_x, int side, int interp, void* stream);

/* ---- scan geometry: the array a scanner wrote <-> the re-oriented 1 mm grid every entry point works on (csrc/scan.hip) -------------------
 * The reference's data/data_process.py:24-33 makes, from raw (x, y, z) and the signed diagonal `spacing` of its affine,
 *   oriented = transpose(raw, [1, 0, 2])[::ind[1], ::ind[0], ::ind[2]],  ind[i] = +1 if spacing[i] < 0 else -1      shape (y, x, z)
 * and resizes it to the 1 mm grid (d1, h1, w1) = int((y, x, z) * |spacing|) — the TRANSPOSED shape times the UNTRANSPOSED spacing, as the reference
 * writes it (data_gpu.ScanGeometry does that arithmetic on the host).  The kernels take the raw shape and three flips in oriented axis order
 * (flip0 = ind[1] < 0, flip1 = ind[0] < 0, flip2 = ind[2] < 0):
 *   oriented[o0][o1][o2] = raw[g1(o1)][g0(o0)][g2(o2)],  g_a(o) = flip_a ? n_a - 1 - o : o,  (n_0, n_1, n_2) = (y, x, z).
 * vs_scan_orient: raw of VS_SCAN_I16 / U8 / I8 / F32 -> out, the contiguous fp32 oriented volume (y, x, z), exact values, one launch.  The contiguous
 * axis stays contiguous and is at most reversed; a lane moves four of its elements per load and store.
 * vs_scan_to_native: the way back for an answer on the 1 mm grid.  src: planar fp32 probabilities (k, d1, h1, w1), 1 <= k <= 8 (src_is_label 0), or a
 * uint8 label (d1, h1, w1) (src_is_label 1: k = 1, interp 0, prob_out NULL).  Raw voxel (i0, i1, i2) has the oriented index (g0(i1), g1(i0), g2(i2))
 * and per axis the 1 mm coordinate q = (o + 0.5) * n_1mm / n_oriented - 0.5 in fp64.
 *   interp 0 (nearest): the sample at floor(q + 0.5), clamped to [0, n_1mm - 1].
 *   interp 1 (linear): q mirrored at the borders (q < 0 -> -q, q > n_1mm - 1 -> 2 (n_1mm - 1) - q), trilinear, weights and products in fp64, the sum
 *   rounded to fp32 once: scipy.ndimage.zoom(src[c], (y, x, z) / (d1, h1, w1), order=1, mode='mirror', grid_mode=True) carried to the raw axes.
 * label (x, y, z) bytes: the channel argmax of those fp32 values, ties to the first maximal channel, a NaN channel wins (vs_hard_onehot, vs_uncrop);
 * for a label source the sample itself.  prob_out (may be NULL): the resampled probabilities, planar fp32 (k, x, y, z).
 * One launch writes every element of label and prob_out exactly once: no memset before it, no atomics, no synchronisation (capturable), bit-identical
 * from run to run and between the two builds.  Pointers are 16-byte aligned (VS_EALIGN); an empty shape or one of 2^31 voxels or more: VS_ESHAPE; k
 * outside [1, 8], interp outside {0, 1}, a label source with k != 1, interp 1 or prob_out: VS_EINVAL; an unknown dtype: VS_EDTYPE — all on the host
 * before any launch.  The kernels clamp every source index into its axis and bound their stores by (x, y, z) alone. */
enum { VS_SCAN_I16 = 0, VS_SCAN_U8 = 1, VS_SCAN_I8 = 2, VS_SCAN_F32 = 3 };
int vs_scan_orient(const void* raw, int dtype, float* out, int x, int y, int z, int flip0, int flip1, int flip2, void* stream);
int vs_scan_to_native(const void* src, int src_is_label, unsigned char* label, float* prob_out, int k, int d1, int h1, int w1, int x, int y, int z,
                      int flip0, int flip1, int flip2, int interp, void* stream);

/* ---- fully connected (VAE bottleneck, joint_model.py:216-218,242-243,248-253) -------------------- */
/* y[b][j] = act( bias[j] + sum_k W[j][k] * x[b][phys(k)] )  with phys(k) = (k % pv)*pc + k / pv when pc > 0:
 * x is a channels-last activation [B][pv voxels][pc channels] read in the reference's flatten order
 * (k = c*pv + v); pc == 0 means x is a plain float[B][K].  x_dtype applies to x; y, W, bias are fp32. */
int vs_linear_fwd(const void* x, int x_dtype, const float* wgt, const float* bias, float* y, int batch, int k_in,
                  int j_out, int pc, int pv, int relu, void* stream);
/* two layers on the same input (fc_mean and fc_std, joint_model.py:216-217,241-243) in one launch; arguments as vs_linear_fwd */
int vs_linear_fwd_pair(const void* x, int x_dtype, const float* w1, const float* b1, float* y1, int relu1, const float* w2,
                       const float* b2, float* y2, int relu2, int batch, int k_in, int j_out, int pc, int pv, void* stream);
/* y[b][phys(j)] = bias[j] + sum_k W[j][k] * z[b][k]   — fc2: fp32 latent in, channels-last activation out. */
int vs_linear_fwd_perm_out(const float* z, const float* wgt, const float* bias, void* y, int y_dtype, int batch,
                           int k_in, int j_out, int pc, int pv, void* stream);
/* backward of vs_linear_fwd: gy is float[B][J] (already masked by the caller's ReLU if any).
 * gx (may be NULL) gets dL/dx in x's layout/dtype; gw / gb (may be NULL) are fp32 [J][K] / [J]. */
int vs_linear_bwd(const void* x, int x_dtype, const float* wgt, const float* gy, const float* y_for_relu,
                  void* gx, float* gw, float* gb, int batch, int k_in, int j_out, int pc, int pv, void* stream);
/* backward of vs_linear_fwd_perm_out: gy channels-last; gz float[B][K] (may be NULL); gw,gb may be NULL. */
int vs_linear_perm_out_bwd(const float* z, const float* wgt, const void* gy, int y_dtype, float* gz, float* gw,
                           float* gb, int batch, int k_in, int j_out, int pc, int pv, void* stream);

/* ---- VAE latent ---------------------------------------------------------------------------------- */
/* z = mean + noise*std*scale  (joint_model.py:248) ; bwd: gmean = gz, gstd = gz*noise*scale */
int vs_reparam_fwd(const float* mean, const float* std_, const float* noise, float scale, float* z, long long count, void* stream);
int vs_reparam_bwd(const float* gz, const float* noise, float scale, float* gmean, float* gstd, long long count, void* stream);
/* The latent's noise drawn on the device.  A latent STREAM is (seed, draw), two unsigned 64-bit words.  Element i < count of draw t, pair q = i >> 1:
 * Philox4x32-10 (csrc/philox.h) under key (seed low 32, seed high 32) and counter (q, t low 32, 0x200, t high 32); u1, u2 and r = sqrt(-2 ln u1) as
 * vs_aug_normal_philox forms them, in fp64; even i takes r cos(2 pi u2), odd i takes r sin(2 pi u2), rounded to fp32 once; an odd count uses only the
 * cosine of its last pair.  Counter word 2 = 0x200 keeps the stream apart from the elastic one (0 .. 2) and the augmentation's (0x100 + channel).
 *   vs_latent_normal_philox  noise[count] of the stream (seed, draw), both host arguments
 *   vs_reparam_philox_fwd    reads state[0] = seed and state[1] = draw from DEVICE memory, writes the normals to noise_out and z = mean + noise*std*scale
 *                            with vs_reparam_fwd's arithmetic (the same bits for that noise_out); backward is vs_reparam_bwd on noise_out
 *   vs_latent_advance        state[1] += 1, one thread, a launch of its own: on the stream of the forward it runs after every read of state[1]
 * A captured vs_reparam_philox_fwd + vs_latent_advance pair therefore draws a fresh sample on every replay.  Null pointer: VS_EINVAL; count <= 0 or
 * count >= 2^31: VS_ESHAPE; state not 8-byte, an fp32 buffer not 4-byte aligned: VS_EALIGN; all answered on the host before any launch.  No atomics, no
 * memset, nothing allocated, synchronised or read back. */
int vs_latent_normal_philox(float* noise, long long count, unsigned long long seed, unsigned long long draw, void* stream);
int vs_reparam_philox_fwd(const float* mean, const float* std_, const unsigned long long* state, float scale, float* z, float* noise_out,
                          long long count, void* stream);
int vs_latent_advance(unsigned long long* state, void* stream);
/* out = mean_b 0.5*(sum std^2 + sum mean^2 - 2 sum log(std+1e-5))     (utils/evaluation.py:42-45) */
int vs_kl_fwd(const float* mean, const float* std_, float* out, int batch, int dim, void* stream);
int vs_kl_bwd(const float* mean, const float* std_, const float* gout, float* gmean, float* gstd, int batch, int dim, void* stream);

/* ---- losses ---------------------------------------------------------------------------------------- */
/* soft Dice (utils/evaluation.py:48-80; main_source.py:150-182):  s,t planar fp32 [B][C][V].
 *   sums[b][c] = (sum s*t, sum s, sum t) for bot <= c < top (double[B][C][3], fully overwritten)
 *   per_sample[b] = mean_{c in [bot,top)} 2*I/(S+T+eps) ;  mean_out[0] = mean_b per_sample[b]
 *   V is a multiple of 4 (the kernels read 16-byte quads; VS_EALIGN otherwise, here and in vs_dice_loss_multi_*): a caller with another
 *   plane size pads the planes with zeros — labels with -1 — as ops.Dice / ops.DiceLossSum do.            */
int vs_dice_fwd(const float* s, const float* t, double* sums, float* per_sample, float* mean_out,
                int batch, int channels, long long voxels, int bot, int top, float eps, void* stream);
/* gs/gt (either may be NULL) = d(sum_b w[b]*per_sample[b])/d(s|t); channels outside [bot,top) get 0.
 * gout_is_mean == 0: w[b] = gout[b] (float[B], upstream gradient of each per-sample score);
 * gout_is_mean == 1: w[b] = gout[0]/B (upstream gradient of mean_out). */
int vs_dice_bwd(const float* s, const float* t, const double* sums, const float* gout, int gout_is_mean, float* gs,
                float* gt, int batch, int channels, long long voxels, int bot, int top, float eps, void* stream);
/* A weighted sum of soft-Dice LOSSES of one source against k <= 4 targets in one pass over the source — the loss line of
 * every train method, e.g. main_source.py:469-471  final = lambda*(1-Dice(pred,recon)) + (1-Dice(pred,gt)):
 *   terms[j] = 1 - mean_b mean_{c in [bot,top)} 2*I_j/(S+T_j+eps);   final = ((w[0]*terms[0]) + w[1]*terms[1]) + ...   (fp32, that order)
 * t, w (and gt below) are HOST arrays of k entries.  scratch: vs_dice_loss_multi_scratch_doubles() doubles, contents undefined
 * on entry (per-block partials summed in a fixed order: no atomics, bitwise reproducible); the forward leaves the sums the
 * backward needs in its first 3*k*B*C entries.  The backward writes gs = d final/d s * gout[0] and,
 * for every non-NULL gt[j], d final/d t_j * gout[0]; channels outside [bot,top) get 0. */
size_t vs_dice_loss_multi_scratch_doubles(int k, int batch, int channels);
int vs_dice_loss_multi_fwd(const float* s, const float* const* t, const float* w, int k, double* scratch, float* terms,
                           float* final_out, int batch, int channels, long long voxels, int bot, int top, float eps, void* stream);
int vs_dice_loss_multi_bwd(const float* s, const float* const* t, const float* w, int k, const double* scratch,
                           const float* gout, float* gs, float* const* gt, int batch, int channels, long long voxels,
                           int bot, int top, float eps, void* stream);
/* The same with LABEL targets: labels[j] non-NULL (labels itself may be NULL) makes target j the one-hot of that label volume
 * ([batch][voxels] floats, truncated to int as vs_onehot does: main_source.py:449-451) evaluated on the fly — t[j] is then ignored,
 * gt[j] must be NULL, and the one-hot tensor (2 x the prediction's size, written once and read twice per step) never exists. */
int vs_dice_loss_multi_labels_fwd(const float* s, const float* const* t, const float* const* labels, const float* w, int k, double* scratch,
                                  float* terms, float* final_out, int batch, int channels, long long voxels, int bot, int top, float eps,
                                  void* stream);
int vs_dice_loss_multi_labels_bwd(const float* s, const float* const* t, const float* const* labels, const float* w, int k,
                                  const double* scratch, const float* gout, float* gs, float* const* gt, int batch, int channels,
                                  long long voxels, int bot, int top, float eps, void* stream);
/* Compound segmentation loss of planar fp32 probabilities p [B][C][V] (1 <= C <= 8) against a LABEL volume [B][V] (csrc/segloss.hip):
 * soft Dice over channels [bot, top) plus a class-weighted, optionally focal, voxel-wise cross-entropy.  The rule is this library's own; the reference has
 * no counterpart.
 *   A voxel is VALID iff label >= 0 and label < C (fp32 compares: NaN is not), its class is l = (int)label; every other voxel (-1 padding, 255, NaN) is
 *   IGNORED: it adds to no sum — S included — and its gradient is 0 in every channel.  vs_dice_loss_multi_labels_* differs on purpose: there an
 *   unmatched label still counts in S.
 *   Over the valid voxels of a plane, in fp64:  S[b][c] = sum p_c,  I[b][c] = sum_{l=c} p_c,  T[b][c] = #{l = c}.
 *   batch_dice == 0:  dice = mean_b mean_{c in [bot,top)} 2 I[b][c] / (S[b][c] + T[b][c] + eps)
 *   batch_dice != 0:  dice = mean_c 2 sum_b I / (sum_b S + sum_b T + eps)                      dice_term = 1 - dice
 *   f_v = -(1 - p_l)^gamma * max(ln p_l, -100)  (fp64 ln and pow; gamma == 0: plain cross-entropy);  ce_term = sum_v w[l_v] f_v / sum_v w[l_v], 0 when
 *   the denominator is 0.   terms = (dice_term, ce_term), each rounded to fp32 once;  final = (dice_w * dice_term) + ce_w * ce_term  (fp32, that order).
 * class_w: a HOST array of 8 floats >= 0 (entries >= C unused), copied into the kernel arguments.  scratch: vs_seg_loss_scratch_doubles() doubles, contents
 * undefined on entry; the forward (two launches: per-block partials, a one-workgroup finish that adds them in a fixed order) leaves S, I, T, sum w f, sum w
 * in its first batch * (3 * channels + 2) entries, which the backward (one launch) reads.  The backward writes every plane of
 *   gp[b][c][v] = gout[0] * (dice_w * d dice_term / d p + [c == l_v] * ce_w * d ce_term / d p_l)
 * — the exact derivative of the rule above (where the clamp is active the ln factor's derivative is 0), both parts formed in fp64 and rounded to fp32 once;
 * gout is read on the device.  No atomics, no memset, nothing allocated, synchronised or read back: the same bits eagerly, under graph replay and in both
 * builds.  V not a multiple of 4 or a pointer not 16-byte aligned: VS_EALIGN; a null pointer, C outside [1, 8], bot / top out of order, a negative
 * (or NaN) weight, gamma or eps: VS_EINVAL; batch > 64 or V >= 2^31: VS_ESHAPE; all answered on the host before any launch. */
size_t vs_seg_loss_scratch_doubles(int batch, int channels);
int vs_seg_loss_fwd(const float* p, const float* label, const float* class_w, double* scratch, float* terms, float* final_out, int batch, int channels,
                    long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma, void* stream);
int vs_seg_loss_bwd(const float* p, const float* label, const float* class_w, const double* scratch, const float* gout, float* gp, int batch, int channels,
                    long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma, void* stream);
/* The same loss with a TOP-K cross-entropy, K found on the device (csrc/topk.hip).  Validity, f_v, S / I / T and dice_term are those of
 * vs_seg_loss_fwd; the cross-entropy term is the mean of the K largest voxel losses of the POOL, the N valid voxels of the whole batch:
 *   key    g_v = (float)(w[l_v] f_v), the fp64 product rounded once; keys are ordered as real numbers (-0.0 equals 0.0)
 *   rank   K = max(1, floor(r * (double)N)), r a host double in (0, 1];  N == 0: ce_term = 0 and every gradient is 0
 *   tau    the K-th largest key;  n_gt = #{g > tau}, n_eq = #{g = tau}  (n_gt < K <= n_gt + n_eq)
 *   term   ce_term = (A + (K - n_gt) * (E / n_eq)) / K,  A = sum_{g > tau} w f,  E = sum_{g = tau} w f  in fp64: the K - n_gt places left at the
 *          threshold are shared equally by all voxels tied there — no tie-break by position.  NOT divided by sum w, unlike vs_seg_loss_fwd's term.
 *   final = (dice_w * dice_term) + ce_w * ce_term in fp32.
 * The backward is the exact derivative with tau, K and the membership held fixed: the cross-entropy part of gp[b][l_v][v] is
 * gout[0] * ce_w * (c_v / K) * w[l_v] * df/dp_l, c_v = 1 above tau, (K - n_gt) / n_eq at tau, 0 below; added to the Dice part in fp64, rounded once;
 * an ignored voxel gets exactly 0 in every channel.
 * A NaN key (a NaN probability with gamma > 0; with gamma == 0 fmax gives the clamp's 100) is ordered above +inf: the voxel counts among the hardest and
 * the term it enters is NaN.
 * workspace: vs_seg_topk_workspace_bytes() bytes, 16-byte aligned, contents undefined on entry (the first launch writes its initial state); the forward
 * leaves the keys, the totals and the selection there for the backward, which reads nothing else of the forward's.  record: NULL, or 4 doubles in
 * DEVICE memory the forward fills for the caller (it may be reused at once: the backward reads the workspace's own copy) —
 *   record[0] = N,  record[1] = K,  record[2] = tau (0 when N == 0),  record[3] = n_gt * 2^26 + n_eq   (n_gt = floor(record[3] / 2^26)).
 * Forward: seven launches whatever the data; backward: one.  No memset, nothing allocated, synchronised or read back; counts are integer atomics, no
 * floating-point sum uses one: the same bits eagerly, under graph replay and in both builds.  Errors are vs_seg_loss_fwd's, answered on the host before
 * any launch; in addition r NaN or outside (0, 1] or an infinite class weight: VS_EINVAL; batch * voxels >= 2^26: VS_ESHAPE (vs_seg_topk_workspace_bytes: 0);
 * workspace not 16-byte or record not 8-byte aligned: VS_EALIGN. */
size_t vs_seg_topk_workspace_bytes(int batch, long long voxels);
int vs_seg_loss_topk_fwd(const float* p, const float* label, const float* class_w, void* workspace, double* record, float* terms, float* final_out,
                         int batch, int channels, long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma,
                         double r, void* stream);
int vs_seg_loss_topk_bwd(const float* p, const float* label, const float* class_w, const void* workspace, const float* gout, float* gp,
                         int batch, int channels, long long voxels, int bot, int top, float eps, float dice_w, float ce_w, int batch_dice,
                         float gamma, double r, void* stream);
/* Deep-supervision head (csrc/dshead.hip): the 1x1x1 convolution of a coarse channels-last feature map, the softmax of its logits and the
 * loss of vs_seg_loss_* against the FULL-resolution label picked at stride s, fused: no logit or probability is stored.
 *   feat   [batch][d][h][w][channels], dtype VS_F32 / VS_BF16 / VS_F16, channels 8 / 16 / 32 / 64;   weight fp32 [classes][channels], bias fp32 [classes],
 *   1 <= classes <= 8;   label fp32 [batch][s d][s h][s w], s = stride in {2, 4, 8}: coarse voxel (z, y, x) takes the label at
 *   (s z + s/2, s y + s/2, s x + s/2), read in place (scipy.ndimage.zoom(label, 1/s, order=0, mode="nearest", grid_mode=True)).
 *   logit_k = bias_k + sum_c weight[k][c] feat_c in fp32 over the stored value of feat;  p = softmax(logit), max-subtracted, fp32;  dice_term and ce_term of
 *   p against that label by the rule of vs_seg_loss_fwd (class_w: a HOST array of 8 floats);  terms = (dice_term, ce_term);
 *   final = scale * ((dice_w * dice_term) + ce_w * ce_term) in fp32, scale >= 0 the level's weight.
 * scratch: vs_ds_head_scratch_doubles() doubles, contents undefined on entry.  The forward (two launches) leaves the per-sample totals in its first
 * batch * (3 * classes + 2) entries; the backward (two launches) reads them, recomputes p and writes
 *   dlogit_k = p_k (gp_k - sum_j gp_j p_j), gp = gout[0] * scale * (the gradient of vs_seg_loss_bwd), formed in fp64;
 *   dfeat_c = sum_k weight[k][c] dlogit_k (fp32, rounded once to dtype), exactly 0 in every channel of an ignored voxel;
 *   dweight[k][c] = sum_v dlogit_k feat_c and dbias[k] = sum_v dlogit_k in fp32: per-workgroup partials behind the forward's part of scratch, added in a
 *   fixed order.  gout is read on the device.
 * No atomics, no memset, nothing allocated, synchronised or read back: the same bits eagerly, under graph replay and in both builds.  A null pointer,
 * classes outside [1, 8], bot / top out of order, a negative (or NaN) weight, gamma, eps or scale, a stride outside {2, 4, 8}: VS_EINVAL; an unknown dtype:
 * VS_EDTYPE; channels outside {8, 16, 32, 64}, an empty volume, batch > 64 or batch * d * h * w >= 2^31: VS_ESHAPE; feat / dfeat not 16-byte, fp32 buffers
 * not 4-byte or scratch not 8-byte aligned: VS_EALIGN; all answered on the host, in that order, before any launch. */
size_t vs_ds_head_scratch_doubles(int batch, int classes, int channels);
int vs_ds_head_fwd(const void* feat, int dtype, const float* weight, const float* bias, const float* label, const float* class_w, double* scratch,
                   float* terms, float* final_out, int batch, int classes, int channels, int d, int h, int w, int stride, int bot, int top, float eps,
                   float dice_w, float ce_w, int batch_dice, float gamma, float scale, void* stream);
int vs_ds_head_bwd(const void* feat, int dtype, const float* weight, const float* bias, const float* label, const float* class_w, double* scratch,
                   const float* gout, void* dfeat, float* dweight, float* dbias, int batch, int classes, int channels, int d, int h, int w, int stride,
                   int bot, int top, float eps, float dice_w, float ce_w, int batch_dice, float gamma, float scale, void* stream);
/* Signed distance maps of a label volume and the boundary loss on them (csrc/sdm.hip; Kervadec et al., MIDL 2019).  The reference has
 * neither; the rule is this library's own.
 *   label  fp32 (n, 1, d, h, w).  The class of a voxel is (int)label where 0 <= label < n_class in fp32, none otherwise (-1, 255, NaN: the rule of
 *          vs_seg_loss_*).  P_c = the voxels of class c; every other voxel of the volume, the classless ones included, is outside P_c.
 *   phi    fp32 (n, top - bot, d, h, w), plane j for class c = bot + j.  With S = diag(spacing) (sz, sy, sx; NULL: the identity):
 *            v outside P_c:  phi_c(v) = +sqrt(min over u in P_c of |S (v - u)|^2)
 *            v in P_c:       phi_c(v) = 1 - sqrt(min over u outside P_c of |S (v - u)|^2)       (the "- 1" of one_hot2dist, under a spacing too)
 *            P_c empty, or the whole volume: the plane is 0.0 — decided per voxel by the "no such voxel" value (INT_MAX / +inf) its own minimum
 *            still holds: no reduction, nothing read back.
 *          Squared distances are exact int32 without a spacing and fp64 sums of (s r)^2 with one; square root and subtraction are fp64 and the
 *          result is rounded to fp32 once.
 * Three launches (two for h == 1): an x pass that reads the label once and writes both row maps (to P_c, to its complement) of every class into the
 * workspace, a y pass over both maps in place, a z pass that reads the label again and, per voxel, the map opposite to its membership, and stores
 * phi.  workspace: vs_signed_distance_workspace_bytes(n, top - bot, ...) bytes (2 maps of int32 / double per class; negative: VS_E*), contents undefined
 * on entry.  Limits as for vs_edt: d, h <= 1024, d*h*w < 2^31, d^2 + h^2 + w^2 < 2^31 - 1 without a spacing: VS_ESHAPE, as for an empty shape;
 * n_class < 1, bot / top out of order, a spacing that is not positive and finite, a null pointer, aliased buffers: VS_EINVAL; label / phi / workspace
 * not 16-byte aligned: VS_EALIGN — all on the host before any launch.  Rows need no alignment and w is arbitrary.  No atomics, no memset, nothing
 * allocated, synchronised or read back: capturable, the same bits eagerly, under graph replay and in both builds. */
long long vs_signed_distance_workspace_bytes(int n, int classes, int d, int h, int w, int with_spacing);
int vs_signed_distance(const float* label, float* phi, int n, int n_class, int bot, int top, int d, int h, int w, const double* spacing,
                       void* workspace, void* stream);
/* Boundary loss of planar fp32 probabilities p [b][c][voxels] against label [b][voxels] and phi [b][top - bot][voxels]:
 *   L_B = 1 / (b (top - bot)) sum_b 1 / N_b sum_{c in [bot, top)} sum_{v valid} p_c(v) phi_c(v),   N_b = the valid voxels of sample b (label in [0, c));
 * a sample with N_b = 0 contributes 0.  fp64 sums of exactly promoted fp32 products: per-workgroup partials by ordinary stores, then a one-workgroup
 * finish in a fixed order.  terms = (L_B, w L_B), each rounded once, w = weight_dev[0] read on the DEVICE (a weight schedule needs no re-capture).
 * scratch: vs_boundary_loss_scratch_doubles() doubles (0: b outside [1, 64] or c < 1), contents undefined on entry; the forward leaves (sum, N_b) per sample
 * at its head for the backward (one launch), which writes every plane of
 *   gp[b][c][v] = gout[0] w phi_c(v) / (b (top - bot) N_b)   formed in fp64, rounded once; exactly 0.0 at classless voxels and outside [bot, top).
 * 16-byte loads and stores when voxels is a multiple of 4 and the volumes are 16-byte aligned, dword accesses otherwise (any voxels >= 1).  A null pointer,
 * c < 1, bot / top out of order: VS_EINVAL; b > 64 or voxels >= 2^31: VS_ESHAPE; an fp32 buffer not 4-byte or scratch not 8-byte aligned: VS_EALIGN. */
long long vs_boundary_loss_scratch_doubles(int b, int c);
int vs_boundary_loss_fwd(const float* p, const float* label, const float* phi, const float* weight_dev, double* scratch, float* terms, int b, int c,
                         int bot, int top, long long voxels, void* stream);
int vs_boundary_loss_bwd(const float* label, const float* phi, const float* weight_dev, const double* scratch, const float* gout, float* gp, int b, int c,
                         int bot, int top, long long voxels, void* stream);
/* nn.BCELoss() mean reduction (utils/evaluation.py:29-39), log clamped at -100 like torch */
int vs_bce_fwd(const float* p, const float* t, float* out, double* scratch, long long count, void* stream);
int vs_bce_bwd(const float* p, const float* t, const float* gout, float* gp, long long count, void* stream);

/* ---- optimiser / teacher ---------------------------------------------------------------------------- */
/* multi-tensor updates: ptr tables are DEVICE arrays of n_tensors device pointers, sizes[] element counts,
 * block_map[] = (tensor index, first element) pairs, one per chunk of VS_MT_CHUNK elements (n_blocks of them); vs_mt_chunk: VS_MT_CHUNK. */
#define VS_MT_CHUNK 4096
int vs_mt_chunk(void);
/* SGD (torch.optim.SGD semantics, main_source.py:279-291): g += wd*p; buf = first ? g : mom*buf + g; p -= lr*buf */
int vs_sgd_momentum_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                          const int* block_map, int n_blocks, float lr, float momentum, float weight_decay,
                          int first_step, void* stream);
/* Adam (torch.optim.Adam, betas (b1,b2), eps 1e-8, L2 weight decay; main_source.py:292-294); step >= 1.  The betas are doubles
 * (python floats): 1 - beta and the bias corrections 1 - beta^step are formed in double, exactly as torch.optim.Adam forms them. */
int vs_adam_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  const long long* sizes, const int* block_map, int n_blocks, float lr, double beta1, double beta2,
                  float eps, float weight_decay, int step, void* stream);
/* ---- dynamic loss scaling: VS_F16 storage (BASELINE configs[4]; no counterpart in the reference, which trains in fp32) ------------
 * The soft-Dice gradients are O(1e-6): stored as fp16 they fall below the normal range.  The loss is therefore differentiated with
 * an upstream gradient of S = loss_scale[0] (a DEVICE scalar, so that a captured graph follows it), every gradient comes out S times
 * too large, and the optimiser divides by S.  Overflow protocol (torch.cuda.amp.GradScaler's, all on the device, no host sync):
 *   vs_grad_finite_multi      found_inf[0] = 1 if any gradient element is inf / nan (caller zero-initialises once)
 *   vs_*_scaled_multi         the update with g / S; the WHOLE step is skipped when found_inf[0] != 0  (NULL, NULL = the plain call)
 *   vs_loss_scale_update      found_inf ? S *= backoff, tracker = 0 : (++tracker == interval ? S *= growth, tracker = 0); found_inf = 0 */
int vs_sgd_momentum_scaled_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                                 const int* block_map, int n_blocks, float lr, float momentum, float weight_decay,
                                 int first_step, const float* loss_scale, const float* found_inf, void* stream);
/* the same update with the hyperparameters read from DEVICE memory, hyper[3] = {lr, momentum, weight_decay}: a launch captured into a HIP
 * graph (train.GraphedStep's captured tail) follows a learning-rate schedule without being re-captured — the host rewrites the three floats.
 * Momentum buffers must exist and hold zeros before the first step (buf = mom*0 + g = torch's clone(g)); loss_scale / found_inf may be NULL. */
int vs_sgd_momentum_dev_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                              const int* block_map, int n_blocks, const float* hyper, const float* loss_scale,
                              const float* found_inf, void* stream);
int vs_adam_scaled_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                         const long long* sizes, const int* block_map, int n_blocks, float lr, double beta1, double beta2,
                         float eps, float weight_decay, int step, const float* loss_scale, const float* found_inf, void* stream);
int vs_grad_finite_multi(const float* const* grads, const long long* sizes, const int* block_map, int n_blocks,
                         float* found_inf, void* stream);
int vs_loss_scale_update(float* scale, int* growth_tracker, float* found_inf, float growth_factor, float backoff_factor,
                         int growth_interval, void* stream);
/* ---- global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm type 2) and Nesterov momentum -------------------------------------
 * The norm spans every tensor of every param group, is taken AFTER the all-reduce and AFTER unscaling, and is summed in ONE order (no atomics),
 * so every data-parallel rank derives the same coefficient from the same all-reduced bits:
 *   vs_grad_sqnorm_multi   partials[b] = sum of squares (fp64 of exact fp32 x fp32 products) of chunk b of the tables vs_grad_finite_multi takes;
 *                          a function of the chunk's values alone (aligned vector loads and ragged / misaligned dword loads add in the same order).
 *                          The caller concatenates the partials of all its groups: partials + offset per group.
 *   vs_grad_clip_finish    one workgroup adds all n_partials in a fixed order.  clip is a DEVICE record float[4] = {max_norm, norm, coef, 0}:
 *                          max_norm is READ (a captured launch follows a change), norm = (float)(sqrt(sum) / S) with S = loss_scale[0] (NULL: 1),
 *                          coef = min(1, max_norm / (norm + 1e-6f)) in fp32 — a NaN norm gives 1, an infinite norm gives 0.
 * The steps take clip_coef = clip + 2 (NULL: no clipping) and multiply the unscaled gradient by it before weight decay is added:
 *   gi = (g / S) * coef + wd * p;  b = momentum * m + gi;  p -= lr * (nesterov ? gi + momentum * b : b)          (momentum == 0: p -= lr * gi)
 * Each of these multiply-adds is ONE fused multiply-add, as vs_sgd_momentum_*_multi has always been compiled, so a step with coef == 1 and
 * nesterov == 0 gives the bits of the plain step.  vs_sgd_step_multi with clip_coef NULL and nesterov 0 IS vs_sgd_momentum_scaled_multi.
 * vs_sgd_step_dev_multi reads hyper[4] = {lr, momentum, weight_decay, nesterov (0 / 1)} from DEVICE memory.  Momentum buffers must exist and
 * hold zeros before the first step. */
int vs_grad_sqnorm_multi(const float* const* grads, const long long* sizes, const int* block_map, int n_blocks, double* partials,
                         void* stream);
int vs_grad_clip_finish(const double* partials, int n_partials, float* clip, const float* loss_scale, void* stream);
int vs_sgd_step_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                      const int* block_map, int n_blocks, float lr, float momentum, float weight_decay, int nesterov,
                      const float* clip_coef, const float* loss_scale, const float* found_inf, void* stream);
int vs_sgd_step_dev_multi(float* const* params, const float* const* grads, float* const* bufs, const long long* sizes,
                          const int* block_map, int n_blocks, const float* hyper, const float* clip_coef, const float* loss_scale,
                          const float* found_inf, void* stream);
int vs_adam_clip_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                       const long long* sizes, const int* block_map, int n_blocks, float lr, double beta1, double beta2,
                       float eps, float weight_decay, int step, const float* clip_coef, const float* loss_scale, const float* found_inf,
                       void* stream);
/* EMA teacher: t = alpha*t + (1-alpha)*s       (main_target.py:512-516) */
int vs_ema_multi(float* const* teacher, const float* const* student, const long long* sizes, const int* block_map,
                 int n_blocks, float alpha, void* stream);
/* dst_k[i] = src_k[i]*scale for every tensor k: gathers the (scattered) gradient tensors into the slices of one flat
 * all-reduce bucket, with the 1/world_size factor folded in — replaces nn.DataParallel's ReduceAddCoalesced staging
 * (main_source.py:354). */
int vs_copy_scale_multi(const float* const* srcs, float* const* dsts, const long long* sizes, const int* block_map,
                        int n_blocks, float scale, void* stream);
/* flat helper: dst[i] = src[i]*scale (dst may equal src: the 1/world scale after a sum all-reduce when the collective has no average) */
int vs_scale_copy(const float* src, float* dst, long long count, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VAESEG_H */
