/*
 * mcquic_hip.h — C-ABI of libmcquic_hip.so, the MI355X (gfx950) replacement for the PyTorch ops
 * underneath McQuic's Compressor encode/decode hot path.
 *
 * The reference has no FFI for this path: it calls torch ops (nn.Conv2d / F.conv2d / torch.bmm /
 * argmin / advanced indexing).  Each entry point below cites the reference call site(s) it replaces
 * (paths relative to the reference tree).  The binding a reference maintainer would add (ctypes) is
 * shown in INTEGRATION.md and is what mcquic_amd/_lib.py does.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); work is only enqueued,
 *     no entry point synchronises;
 *   - return 0 on success, a negative MCQ_E* code on invalid arguments; nothing throws;
 *   - tensors are dense fp32 NCHW; code indices are int64 [N, m, h, w]  (reference:
 *     mcquic/modules/quantizer.py:144-150, argmin returns int64).
 *   - all entry points are re-entrant.
 */
#ifndef MCQUIC_HIP_H
#define MCQUIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a signature or struct in this header changes incompatibly (history in INTEGRATION.md section 2).  A binding
 * compares it with mcq_abi_version() of the library it loaded before calling anything else: a stale .so under new
 * prototypes (or the reverse) misaligns arguments silently otherwise.  3 = round 3 (mcq_rans_*_with_indexes take cdf_lens,
 * mcq_gate_f32 takes out_silu -- both changed in round 2 without a bump --, GroupNorm / logits-gradient entry points). */
#define MCQ_ABI_VERSION   18

#define MCQ_OK            0
#define MCQ_EINVAL       -1   /* NULL pointer / non-positive dimension / unsupported combination */
#define MCQ_ELAUNCH      -2   /* hipLaunchKernel failed (hipGetLastError() != hipSuccess)        */
#define MCQ_ETOOLARGE    -3   /* a per-image plane exceeds the 2 GiB buffer-addressing window    */

/* ---- conv flags (mcq_conv_desc.flags) ------------------------------------------------------- */
#define MCQ_CONV_SILU_IN    0x001u /* apply SiLU to the input on load   (mcquic/nn/blocks.py:70-78,179-200: act before conv) */
#define MCQ_CONV_SQUARE_IN  0x002u /* square the input on load          (mcquic/nn/gdn.py:75: F.conv2d(x ** 2, gamma, beta))  */
#define MCQ_CONV_SILU_OUT   0x004u /* apply SiLU to the result          (the act2 of _residulBlock, fused into conv1)        */
#define MCQ_CONV_RESIDUAL   0x008u /* y += res_scale * res              (blocks.py:77 `out += identity`; quantizer.py:318 `z - dequant`) */
#define MCQ_CONV_GDN        0x010u /* y = mul * (1/sqrt(acc))           (gdn.py:79  x * torch.rsqrt(std)) */
#define MCQ_CONV_IGDN       0x020u /* y = mul * sqrt(acc)               (gdn.py:91  x * torch.sqrt(std))  */
#define MCQ_CONV_GATE       0x040u /* y = mul * sigmoid(acc) + gate_id  (blocks.py:281-288 AttentionBlock.forward) */
#define MCQ_CONV_SHUFFLE2   0x080u /* store through nn.PixelShuffle(2)  (mcquic/nn/convs.py:221-255 pixelShuffle3x3) */
#define MCQ_CONV_MUL        0x200u /* y = mul * acc                     (GDN backward: 2 x * (gamma^T ds))                    */
#define MCQ_CONV_DSILU_MUL  0x400u /* y = acc * silu'(mul)              (backward of SiLU fused into the input-gradient conv:  */
                                   /*                                    mul = the SiLU's input; then + res as usual)           */
#define MCQ_CONV_GDN_BWD    0x4000u /* GDN backward in the epilogue of the recomputed s = beta + gamma x^2 launch (with SQUARE_IN): y = res / sqrt(s)
                                     * (the direct term dy f(s)), y_silu = res * mul * (-1/2 s^-3/2) (d s); res = dy, mul = x, RESIDUAL not set.
                                     * What torch.autograd derives for mcquic/nn/gdn.py:75-79; round 3 ran it as a launch of its own behind s. */
#define MCQ_CONV_IGDN_BWD   0x8000u /* the same for InvGenDivNorm (gdn.py:87-91): y = res * sqrt(s), y_silu = res * mul * (1/2 s^-1/2) */
#define MCQ_CONV_GATE_BWD   0x10000u /* (round 5) AttentionBlock gate backward in the epilogue of the recomputed s = conv1x1(b) launch (ksize 1, no other flag):
                                      * y = res * sigmoid(s) (d a), y_silu = res * mul * sigmoid(s) (1 - sigmoid(s)) (d s); res = d out, mul = a.
                                      * What torch.autograd derives for mcquic/nn/blocks.py:286-287; the forward keeps no s (the gate is the 1x1
                                      * launch's MCQ_CONV_GATE epilogue in training as in inference). */
#define MCQ_CONV_TAPS_LR    0x20000u /* (round 5) a PROMISE about w_packed, not an operation: the 3x3 stride-1 filter is zero outside its lower-right
                                      * 2 x 2 taps (dy, dx in {0, +1}) -- what mcq_pack_conv_dgrad_weight_f32 writes for a stride-2 layer
                                      * ([4 Cin, Cout, 3, 3] through MCQ_CONV_SHUFFLE2: torch.autograd's conv_transpose2d of mcquic/nn/convs.py:132-153
                                      * conv3x3(stride=2)).  The launch then walks 4 of the 9 taps; same sums.  No input prologue, no Winograd form. */
#define MCQ_CONV_POST_GDN   0x40000u  /* (round 6) the 1x1 layer that FOLLOWS this 3x3 convolution runs inside its launch, on the wave's fresh 128-channel
                                      * tile: v = conv(x) + bias, s = post_w @ v^2 + post_bias, y = v / sqrt(s)  (ResidualBlockWithStride: conv3x3 s2 -> GenDivNorm,
                                      * mcquic/nn/blocks.py:98-122, mcquic/nn/gdn.py:67-79).  Cout == 128, ksize 3; post_w from mcq_pack_post1x1_weight_f32. */
#define MCQ_CONV_POST_IGDN  0x80000u  /* the same with y = v * sqrt(s) (ResidualBlockShuffle: pixelShuffle3x3 -> InvGenDivNorm, blocks.py:141-159, gdn.py:81-91).
                                      * With MCQ_CONV_SHUFFLE2: Cout == 512 and w_packed / bias packed from the weight with its rows in SUB-PIXEL-MAJOR order
                                      * (row 128 T + c = conv channel 4 c + T: the 128 rows of tile T are the 128 shuffled channels of sub-pixel T = 2 dy + dx),
                                      * so that a wave holds all channels the normalisation mixes; the store goes to pixel (2 y + dy, 2 x + dx). */
#define MCQ_CONV_POST_GATE  0x100000u /* v = conv(x) + bias + res_scale * res, s = post_w @ v + post_bias, y = mul * sigmoid(s) + gate_id  (AttentionBlock:
                                      * the side stack's last convolution -> conv1x1 -> gate, blocks.py:281-288).  Cout == 128; DUAL_SILU allowed. */
#define MCQ_CONV_POST_MASK  (MCQ_CONV_POST_GDN | MCQ_CONV_POST_IGDN | MCQ_CONV_POST_GATE)
#define MCQ_CONV_DUAL_SILU  0x100u /* also store silu(y) to y_silu: the next block's act1(x), computed once per element */
#define MCQ_CONV_WINOGRAD2D 0x1000u /* OPT-IN like MCQ_CONV_WINOGRAD: F(2x2, 3x3), 4/9 of the multiplications; w_packed from   */
                                    /* mcq_pack_conv_weight_winograd2d_f32; Cout % 128 == 0, Cin % 8 == 0                                */
#define MCQ_CONV_WINOGRAD2D16 0x2000u /* OPT-IN: the same F(2x2, 3x3) arithmetic on v_mfma_f32_16x16x4_f32, two waves per SIMD (round 3);  */
                                     /* w_packed from mcq_pack_conv_weight_winograd16_f32; Cout % 128 == 0, Cin % 16 == 0; epilogues:    */
                                     /* SILU_OUT / RESIDUAL / DUAL_SILU combinations, or SHUFFLE2 alone                                   */
#define MCQ_CONV_WINOGRAD   0x800u /* OPT-IN, not the reference's arithmetic: 3x3 stride-1 layer in the Winograd F(2, 3) form along x */
                                   /* (2/3 of the multiplications, float32 throughout, results differ from the direct form in   */
                                   /* the last bits); w_packed then comes from mcq_pack_conv_weight_winograd_f32                 */

typedef struct mcq_conv_desc {
    const float* x;        /* [N, Cin, H, W]                                                      */
    const float* w_packed; /* from mcq_pack_conv_weight_f32                                        */
    const float* bias;     /* [Cout] or NULL                                                       */
    float*       y;        /* [N, Cout, Ho, Wo]; with SHUFFLE2: [N, Cout/4, 2Ho, 2Wo]              */
    float*       y_silu;   /* DUAL_SILU: same shape as y, receives silu(y)                         */
    const float* res;      /* RESIDUAL: same shape as y                                            */
    const float* mul;      /* GDN/IGDN/GATE: same shape as y                                       */
    const float* gate_id;  /* GATE: same shape as y                                                */
    int32_t N, Cin, H, W, Cout;
    int32_t ksize;         /* 1 or 3 (padding = ksize/2, zeros)                                    */
    int32_t stride;        /* 1 or 2                                                               */
    uint32_t flags;
    float   res_scale;     /* +1 or -1                                                             */
    int32_t tile;          /* 0 = auto; else (log2 split-K << 8) | (MB << 4) | NB forces the wave tile (testing / tuning);
                            * bit 0x400: the 128 x 64 tile of a 3x3 stride-1 layer over pixel PAIRS (same bits, wide epilogue accesses;
                            * even output width, flags within SiLU / twin / residual / silu' / PixelShuffle) */
    const float* post_w;    /* MCQ_CONV_POST_*: the following 1x1 layer's [128, 128] weight from mcq_pack_post1x1_weight_f32 (else NULL; ABI 9) */
    const float* post_bias; /* MCQ_CONV_POST_*: its bias [128] (GDN / IGDN: the folded beta) or NULL                                         */
} mcq_conv_desc;

/* (round 6) Operand stream of a [128, 128] 1x1 layer for the MCQ_CONV_POST_* epilogues: the contraction runs over the wave's OWN
 * accumulator registers, so its k-order is the accumulator order -- k-step t = 16 mb + r pairs channel 32 mb + (r & 3) + 8 (r >> 2)
 * (lanes 0..31) with that channel + 4 (lanes 32..63): out[(t * 64 + lane) * 4 + q] = w[32 q + (lane & 31)][that channel], followed by
 * a zero tail.  mcq_packed_post1x1_floats() floats. */
size_t mcq_packed_post1x1_floats(void);
int mcq_pack_post1x1_weight_f32(const float* w /* [128, 128] (1x1 OIHW) */, float* out, void* stream);
/* 0 if this geometry / flag set has no fused form (MCQ_CONV_POST_* in `flags`), else the number of 128 x 32 wave tiles the launch
 * would have: from 2048 (two per SIMD) mcq_conv2d_f32 takes it on its own; below that it refuses unless the caller forces the
 * unsplit tile (tile 0x41) -- small maps, whose 3x3 layer is otherwise split over waves, run the 1x1 layer as its own launch. */
int32_t mcq_conv2d_post_ok(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t ksize, int32_t stride, uint32_t flags);

/* Number of floats mcq_pack_conv_weight_f32 writes for a [Cout, Cin, ks, ks] weight. */
size_t mcq_packed_conv_weight_floats(int32_t Cout, int32_t Cin, int32_t ksize);

/* Re-lay a dense OIHW weight (nn.Conv2d.weight, mcquic/nn/convs.py:77-100,257-276) into the MFMA operand streams the
 * conv kernels read: [Cout/128][Cin/2 x taps][64 lanes][4] followed by dense copies for the 64- and 32-row wave tiles
 * ([Cout/64][..][64][2], [Cout/32][..][64][1]), for 3x3 layers with Cin 64 / 128 and Cout % 16 == 0 (>= 32) a fourth copy in
 * the order of the small-launch kernel ([Cout/16][Cin/4 x 9 / 4][64][4], csrc/conv_t16.h) and, for 3x3 layers with <= 16 output
 * channels, the operand order of the 16-row image-head kernel; every copy zero padded (one launch). */
int mcq_pack_conv_weight_f32(const float* w_oihw, int32_t Cout, int32_t Cin, int32_t ksize,
                             float* w_packed, void* stream);

/* OPT-IN fast path (never the default): the operand stream of a 3x3 stride-1 layer in the Winograd F(2, 3) form along x --
 * per filter row (g0, g1, g2) the four transformed taps (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2), formed in float64
 * and rounded once, in the same [Cout/128][Cin/2 x 12][64][4] (+ 64-row copy) order.  Used with MCQ_CONV_WINOGRAD, which
 * needs Cout % 64 == 0, ksize 3, stride 1 and no input prologue (SILU_IN / SQUARE_IN).  mcq_conv2d_winograd_ok tells
 * whether mcq_conv2d_f32 takes a geometry AND flag set (1) or refuses it with MCQ_EINVAL (0), by the launcher's own rules: exactly
 * one of MCQ_CONV_WINOGRAD / _WINOGRAD2D / _WINOGRAD2D16 (none = MCQ_CONV_WINOGRAD is meant), no MCQ_CONV_TAPS_LR, no POST_* or
 * backward-pair epilogue, the PixelShuffle store with no other epilogue, WINOGRAD2D: Cout % 128 == 0 and Cin % 8 == 0,
 * WINOGRAD2D16: Cout % 128 == 0, Cin % 16 == 0 and an epilogue within SiLU / residual / twin or the PixelShuffle store alone.
 * (Null side pointers and the 2 GiB addressing limit, MCQ_ETOOLARGE, are not its subject.) */
size_t mcq_packed_conv_winograd_floats(int32_t Cout, int32_t Cin);
/* The same in both directions, F(2x2, 3x3) (MCQ_CONV_WINOGRAD2D; Cout % 128 == 0 and Cin % 8 == 0): G g G^T, sixteen transformed taps per filter,
 * [Cout/32][Cin/2 x 16][64 lanes]; 4/9 of the multiplications. */
size_t mcq_packed_conv_winograd2d_floats(int32_t Cout, int32_t Cin);
int mcq_pack_conv_weight_winograd2d_f32(const float* w_oihw, int32_t Cout, int32_t Cin, float* w_packed, void* stream);
int mcq_pack_conv_weight_winograd_f32(const float* w_oihw, int32_t Cout, int32_t Cin, float* w_packed, void* stream);
/* ... and of the layer's stride-1 input-gradient convolution (torch.autograd's conv2d backward w.r.t. the input), straight from
 * the layer's own OIHW weight: w_packed holds mcq_packed_conv_winograd_floats(Cin, Cout) floats */
int mcq_pack_conv_dgrad_weight_winograd_f32(const float* w_oihw, int32_t Cout, int32_t Cin, float* w_packed, void* stream);
int32_t mcq_conv2d_winograd_ok(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t ksize, int32_t stride, uint32_t flags);
/* 1 if mcq_conv2d_f32 / mcq_conv2d_multi_f32 (nprob problems) run this geometry and flag set on the small-launch kernel (16 x 16
 * tiles on v_mfma_f32_16x16x4_f32, one per workgroup: launches that would leave most of the GPU idle with 32-row tiles -- the
 * 4x4 ... 16x16 maps of a training step, the 12x8 / 24x16 levels of a single image), 0 if on the general one.  Same arithmetic,
 * same epilogue order; the summation order over (channel, tap) differs as between any two tile shapes. */
int32_t mcq_conv2d_small_launch(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t ksize, int32_t stride, uint32_t flags,
                                int32_t nprob);

/* The operand stream of a layer's INPUT-GRADIENT convolution, packed straight from the layer's own OIHW weight
 * [Cout, Cin, k, k] in one launch (what torch.autograd derives for nn.Conv2d, mcquic/nn/convs.py:77-100):
 *   stride 1:          dX = conv(dY, W'),  W'[ci][co][tap] = W[co][ci][flipped tap]          -> a [Cin, Cout, k, k] conv
 *   stride 2 (3x3):    dX = PixelShuffle2(conv3x3(dY, W')), W' holding per input phase the taps that reach it
 *                                                                                            -> a [4 Cin, Cout, 3, 3] conv
 * mcq_dgrad_weight_shape gives that conv's (Cout_d, Cin_d); `out` holds mcq_packed_conv_weight_floats(Cout_d, Cin_d, k)
 * floats and is used with mcq_conv2d_f32 like any packed weight (MCQ_CONV_SHUFFLE2 for stride 2). */
int mcq_dgrad_weight_shape(int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, int32_t* Cout_d, int32_t* Cin_d);
int mcq_pack_conv_dgrad_weight_f32(const float* w, int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, float scale, float* out,
                                   void* stream);      /* every packed value times `scale` (GDN backward: 2 gamma^T; 1 otherwise) */

/* Dense 2-D convolution (zeros padding ksize/2) + fused prologue/epilogue.
 * Replaces nn.Conv2d.forward for conv3x3 / conv1x1 / pixelShuffle3x3 (mcquic/nn/convs.py:77-100,
 * 221-276), F.conv2d in GenDivNorm.forward (mcquic/nn/gdn.py:67-79), the SiLU / residual add of
 * _residulBlock.forward (mcquic/nn/blocks.py:70-78) and the gate of AttentionBlock.forward
 * (blocks.py:281-288). */
int mcq_conv2d_f32(const mcq_conv_desc* d, void* stream);

/* Up to mcq_conv2d_max_multi() independent convolutions of ONE geometry and flag set in one launch (descs[0..n): same N, Cin,
 * H, W, Cout, ksize, stride, flags, res_scale, tile; their own tensors and packed weights).  The two stacks of an
 * AttentionBlock (mcquic/nn/blocks.py:245-288) apply the same layer shapes to different tensors; on small maps, where a
 * launch is latency rather than work, they go out together. */
int32_t mcq_conv2d_max_multi(void);
int mcq_conv2d_multi_f32(const mcq_conv_desc* descs, int32_t n, void* stream);

/* GDN re-parametrisation folded once at load: out = max(p, bound)^2 - pedestal
 * (mcquic/nn/base.py:81-84 NonNegativeParametrizer.forward). */
int mcq_nonneg_reparam_f32(const float* p, float bound, float pedestal, float* out, int64_t n,
                           void* stream);
/* The same for up to mcq_nonneg_reparam_max_multi() parameters in ONE launch (host arrays of `count` entries): every GDN layer's
 * beta and gamma after an optimizer step (round 5; 20 launches per step of the qp = 2 model before). */
int32_t mcq_nonneg_reparam_max_multi(void);
int mcq_nonneg_reparam_multi_f32(const float* const* p, float* const* out, const int64_t* n, const float* bound, const float* pedestal,
                                 int32_t count, void* stream);

/* ---- multi-codebook quantizer ------------------------------------------------------------- */

/* Floats needed for the packed codebook of one level: the MFMA operand stream
 * m x [k/128][d/2][64][4] (+ prefetch tail) followed by the codeword norms c2 in operand layout. */
size_t mcq_packed_codebook_floats(int32_t m, int32_t k, int32_t d);

/* Pack codebook [m, k, d] into the operand stream and append c2[g, k] = sum_j c^2
 * (mcquic/modules/quantizer.py:163  c2 = (codebook ** 2).sum(-1)); padded codewords get +inf. */
int mcq_vq_pack_codebook_f32(const float* codebook, int32_t m, int32_t k, int32_t d,
                             float* cb_packed, void* stream);

/* The same pack with a rate penalty folded into the norm section (entropy-constrained assignment): cdf uint32 [m, k + 1] is one
 * level of mcq_pmf_to_quantized_cdf_dev's tables (device), lambda >= 0 a host float.  The operand stream is the one above; the norms are
 *   c2'[g, i] = fl32( c2[g, i] + fl32( lambda * fl32(16 - log2((double)(cdf[g, i + 1] - cdf[g, i]))) ) )
 * with c2 formed exactly as above, so mcq_vq_assign*_f32 on this buffer returns argmin_k (distance + lambda * bits_k) through the
 * unchanged kernel.  lambda == 0 gives the buffer of mcq_vq_pack_codebook_f32 bit for bit.  Padded codewords, and a slot of width 0
 * (no valid table has one), get +inf.  MCQ_EINVAL for lambda < 0, NaN or inf.  No allocation, no synchronisation. */
int mcq_vq_pack_codebook_rate_f32(const float* codebook, const uint32_t* cdf, float lambda, int32_t m, int32_t k, int32_t d,
                                  float* cb_packed, void* stream);

/* codes[n, g, y, x] = argmin_k ( (|x_v|^2 + |c_k|^2) - 2 <x_v, c_k> ), first index on ties.
 * x: [N, m*d, h, w] (channel = g*d + j).  Replaces _multiCodebookQuantization._distance + encode
 * (mcquic/modules/quantizer.py:144-179) without materialising [N, m, h, w, k]. */
int mcq_vq_assign_f32(const float* x, const float* cb_packed, int64_t* codes,
                      int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k,
                      void* stream);
/* The same with a scratch buffer of mcq_vq_assign_workspace_bytes(...) bytes (0 = none needed; workspace may then be NULL):
 * launches with too few latent vectors to fill the GPU -- a single 768x512 image is 48 workgroups at the first level -- range
 * the codewords of a vector over up to 16 workgroups and fold the per-range minima in range order (first index on ties, as
 * within one workgroup).  Identical codes. */
size_t mcq_vq_assign_workspace_bytes(int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k);
int mcq_vq_assign_ws_f32(const float* x, const float* cb_packed, int64_t* codes,
                         int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k,
                         void* workspace, void* stream);

/* Read-only: the launch plan of mcq_vq_assign_ws_f32 (rate = 0) and mcq_vq_assign_rate_map_f32 (rate = 1) for a shape.
 * out[6] = {instance, Sp, cs_log2, zs, bw_log2, vector_tiles}: the kernel instance (below), the k-steps per codeword tile, log2 of the
 * waves of a workgroup that slice the codeword tiles of one vector tile, the ranges they are dealt over when a workspace is given
 * (1 without one; mcq_vq_assign_workspace_bytes is zs * N * m * h * w * 8 for zs > 1, else 0; every (range, slice) takes
 * per = ceil(tiles / (zs << cs_log2)) tiles in order, and only the ceil(tiles / (per << cs_log2)) <= zs ranges that own a tile are
 * launched, one workgroup each), log2 of the pixel block's width (blocks
 * of 32 pixels, 32 >> bw_log2 rows high) and the tiles of two blocks = 64 latent vectors.  Host code only; the plan the entry points
 * themselves launch by -- today the same for both values of `rate`, which picks the kernel's form, not its instance.  Returns 1, or 0
 * (out untouched) for a shape the entry points refuse (MCQ_EINVAL / MCQ_ETOOLARGE), a `rate` other than 0 or 1 and a NULL out.
 * Additive: ABI 18 stays. */
#define MCQ_VQ_ASSIGN_LOOP       0   /* run-time k-loop: every vector length without an unrolled instance (d = 17..48, 65..240, > 256) */
#define MCQ_VQ_ASSIGN_SP8        1   /* 8 k-steps unrolled: d = 1..16 */
#define MCQ_VQ_ASSIGN_SP32       2   /* 32 k-steps unrolled: d = 49..64 */
#define MCQ_VQ_ASSIGN_SP128      3   /* 128 k-steps unrolled: d = 241..256 with fewer than four codeword tiles */
#define MCQ_VQ_ASSIGN_SP128_LDS  4   /* the same with the vector tile staged in LDS, always four slices */
int mcq_vq_assign_plan(int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, int32_t rate, int32_t* out);

/* ---- rate control per image and per region: lambda as an operand of the assignment (csrc/vq.hip, csrc/vq_rate_map.hip) ---- */
/* Floats of one level's `bits` section, and the section itself from that level's table cdf uint32 [m, k + 1] (device): the layout of
 * the packed codebook's norm section, [m][k/128 + 1][64][4], holding fl32(16 - log2((double)(cdf[g, i + 1] - cdf[g, i]))) for codeword
 * i < k, 0 for padded codewords and the upper half-wave, +inf for a slot of width 0.  It depends on the table alone. */
size_t mcq_packed_bits_floats(int32_t m, int32_t k);
int mcq_vq_pack_bits_f32(const uint32_t* cdf, int32_t m, int32_t k, float* bits_packed, void* stream);

/* mcq_vq_assign_ws_f32 with one lambda per latent vector: codes[n, g, y, x] = argmin_k fl32(fma(lambda_v, bits_k, dist_k)), dist_k
 * the plain entry's fma(-2, inter, x2 + c2) on the PLAIN pack `cb_packed`, bits_k from `bits_packed` (mcq_vq_pack_bits_f32), first index
 * on ties.  lambda of (n, y, x) is lam[n * stride_n + y * stride_y + x * stride_x] (device float32, element strides >= 0; (1, 0, 0) is
 * one lambda per image) and is shared by the m groups; the caller guarantees lambda finite and >= 0 (mcq_rate_map_levels_f32 does).
 * lambda_v = 0 returns the plain entry's code bit for bit; a slot of width 0 never wins.  Same workspace query and launch plan as
 * mcq_vq_assign_ws_f32.  MCQ_EINVAL before any launch for a NULL pointer (workspace may be NULL), a non-positive size or a negative
 * stride. */
int mcq_vq_assign_rate_map_f32(const float* x, const float* cb_packed, const float* bits_packed, const float* lam,
                               int64_t stride_n, int64_t stride_y, int64_t stride_x, int64_t* codes,
                               int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k,
                               void* workspace, void* stream);

/* Every level's lambda buffer from the caller's map in ONE launch.  h0 = w0 = 0: the per-image form, map[i * stride_n] -> out[l] [n] =
 * fl32(scale_l * map_i).  Else the grid form, map at [i * stride_n + y * stride_y + x * stride_x] on the level-0 code grid h0 x w0 ->
 * out[l] [n, h_l, w_l] with h_l = ceil(h_{l-1} / 2): level 0 is the map; level l, cell (y, x), is the mean of the level-(l - 1) cells
 * (2y .. 2y + 1, 2x .. 2x + 1) that exist, summed in row-major order in float32 and divided by their count, taken on the unscaled map;
 * every level is then multiplied by scale_l.  A map value that is negative, NaN or infinite counts as 0 and sets error[i] = 1 for its
 * image (error int32 [n], written 0 or 1 by every launch; no host read).  `scales`: host [levels], each finite and >= 0;
 * `scales_dev` (or NULL): the same on the device, read by the kernel instead, so that a captured launch takes new scales.  `out`:
 * host array of `levels` <= MCQ_VQ_MAX_LEVELS device pointers.  MCQ_EINVAL before any launch for a NULL pointer, a non-positive n or
 * levels, a negative size or stride, or one of h0, w0 zero alone. */
int mcq_rate_map_levels_f32(const float* map, int32_t n, int32_t h0, int32_t w0, int64_t stride_n, int64_t stride_y, int64_t stride_x,
                            const float* scales, const float* scales_dev /* or NULL */, int32_t levels, float* const* out,
                            int32_t* error, void* stream);

/* One step of the per-image target-rate search, one thread per image, after trial number `trial` of `trials` >= 2 ran the cascade at
 * lam[i]: bpp_i = (bits[i, 0] + ... + bits[i, levels - 1]) / pixels (double, in level order), met = bpp_i <= target[i].  Trial 0 ran
 * lambda = 0 (this call makes the state): met -> the image is finished with answer 0; else lam = lambda_max, bracket (0, lambda_max].
 * Trial 1: a miss finishes the image at lambda_max.  Later trials: met -> hi = lam, else lo = lam.  Then, unless finished, the next
 * lambda is mid = fl32(hi / 16) while lo == 0, else fl32(sqrt((double)lo * (double)hi)); when !(lo < mid < hi), or after trial
 * trials - 1, the image is finished with answer hi.  A finished image keeps lam = its answer.  trial == trials records the final run
 * and decides nothing.  State: lam float32 [n], bracket float32 [n, 2], done int32 [n]; trace_lam float32 / trace_bpp double
 * [trials + 1, n] (or NULL) receive row `trial`: the lambda that ran and its bpp.  All device pointers; no host read. */
int mcq_rate_search_step(const double* bits, const double* target, float* lam, float* bracket, int32_t* done,
                         float* trace_lam /* or NULL */, double* trace_bpp /* or NULL */, int32_t n, int32_t levels, double pixels,
                         float lambda_max, int32_t trial, int32_t trials, void* stream);

/* ---- adaptive quantisation: a rate map made from the image (csrc/rate_activity.hip) ---- */
/* x float32 [n, 3, H, W] (contiguous) -> a float32 [n, h0, w0], (h0, w0) = the image reflect-padded to multiples of `base` (a multiple
 * of 16; padTop = hPad / 2, padLeft = wPad / 2, read in place through the reflected index) in 16 x 16 cells.  Per pixel
 * Y = fmaf(0.114f, B, fmaf(0.587f, G, 0.299f * R)); per cell, in two passes, mu = sum Y / 256, v = sum (Y - mu)^2 / 256 (both sums
 * balanced trees of depth 8 in a fixed order), a = log2f(v + 0x1p-14f).  A cell with a non-finite luma (or an overflowing v) gets a = 0,
 * mask = 1 (mask int32 [n, h0, w0], written 0 or 1) and sets error[image] = 1 (error int32 [n], zeroed on the stream by every call).  No
 * atomics, no host read; equal images give equal bits wherever they stand in the batch.  MCQ_EINVAL before any launch for a NULL
 * pointer, a non-positive size, a base that is no multiple of 16, or padding that reflect cannot make (a side's padding must be smaller
 * than the image's side). */
int mcq_activity_cells_f32(const float* x, int32_t n, int32_t H, int32_t W, int32_t base, float* a, int32_t* mask, int32_t* error,
                           void* stream);

/* The map of one use from the cell activities, one workgroup per image: abar = the mean of `a` over the image's unmasked cells (double
 * sums of consecutive row-major runs added in run order, one division, one rounding to float32; 0 when every cell is masked),
 * e = clamp(strength * (a - abar), -clip, +clip), w = exp2f(e), 1 for a masked cell; out[i, y, x] = (w * roi) * lam[i].  `roi` (or NULL
 * = 1): the caller's own map at roi[i * stride_n + y * stride_y + x * stride_x], element strides >= 0 ((1, 0, 0): one value per image);
 * a negative, NaN or infinite value is written as NaN, which mcq_rate_map_levels_f32 counts as 0 and reports.  `lam` (or NULL = 1):
 * float32 [n] on the device.  MCQ_EINVAL before any launch for a NULL a / mask / out, a non-positive size, a strength that is not finite
 * and >= 0, a clip that is not finite and > 0, or a negative stride. */
int mcq_activity_weights_f32(const float* a, const int32_t* mask, int32_t n, int32_t h0, int32_t w0, float strength, float clip,
                             const float* roi /* or NULL */, int64_t stride_n, int64_t stride_y, int64_t stride_x,
                             const float* lam /* or NULL */, float* out, void* stream);

/* out[n, g*d + j, y, x] = codebook[g, codes[n, g, y, x], j]
 * (mcquic/modules/quantizer.py:249-259 _multiCodebookDeQuantization.decode).
 * Returns MCQ_OK; indices outside [0, k) are clamped (the reference would raise IndexError). */
int mcq_vq_gather_f32(const int64_t* codes, const float* codebook, float* out, float* out_silu /* or NULL */,
                      int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k,
                      void* stream);

/* ---- k-means on the device: the accumulate / update / reseed half of a Lloyd iteration (csrc/vq_kmeans.hip) ------------- */
/* Layouts are mcq_vq_assign_f32's: x [N, m*d, h, w] (channel = g*d + j), codes int64 [N, m, h, w], codebook the plain [m, k, d]
 * parameter (not the packed stream); V = N*h*w latent vectors per group.  Accumulators: sums double [m, k, d], sqsums double
 * [m, k], counts int64 [m, k].  Every entry returns MCQ_EINVAL before any launch for a NULL pointer or a non-positive size;
 * any d, k, m, V >= 1 is taken (V and m*k below 2^31). */

/* sums = 0, sqsums = 0, counts = 0 (a kernel: safe inside a captured graph, like every other zeroing here). */
int mcq_vq_kmeans_zero(double* sums, double* sqsums, int64_t* counts, int32_t m, int32_t k, int32_t d, void* stream);

/* Adds one batch: sums[g, c, :] += sum of the x_v with codes == c, sqsums[g, c] += sum of |x_v|^2, counts[g, c] += their number.
 * Each codeword is owned by one workgroup: no atomics, and every sum runs over ascending vector index (n, y, x) inside up to 16
 * contiguous segments that are folded in segment order; the segment count follows from (m, k, V) alone, so two calls on the
 * same inputs give identical bits.  A vector whose code lies outside [0, k) is skipped. */
int mcq_vq_kmeans_accumulate_f32(const float* x, const int64_t* codes, double* sums, double* sqsums, int64_t* counts,
                                 int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, void* stream);

/* In place on the codebook: where counts[g, c] > 0, codebook[g, c, :] = float32(sums / counts); other codewords stay as they are
 * and empty[g] (int64 [m]) counts them.  inertia[g] (double [m]) = sum over c ascending of
 * sqsums - 2 <c_old, sums> + counts |c_old|^2: the within-cluster sum of squares against the codewords the codes were made with. */
int mcq_vq_kmeans_update_f32(float* codebook, const double* sums, const double* sqsums, const int64_t* counts, double* inertia,
                             int64_t* empty, int32_t m, int32_t k, int32_t d, void* stream);

/* codebook[g, c, :] = latent vector number min(V - 1, floor(u V)) of group g, u = the generator's draw for stream 2, element
 * g*k + c under rng_state = {seed, offset} in device memory (what mcq_hash_uniform_f32(rng_state, 2, ...) returns there; the
 * product is taken in double, where it is exact) -- for every (g, c) when counts is NULL (Forgy seeding), otherwise for those
 * with counts[g, c] == 0 (reseeding empty clusters).  The caller advances the offset between calls, on the device. */
int mcq_vq_kmeans_seed_f32(const float* x, float* codebook, const int64_t* counts_or_null, const uint64_t* rng_state,
                           int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, void* stream);

/* ---- codebook cosine regulariser (ABI 13; csrc/codebook_cos.hip) ------------------------------------------------------------
 * The reference's BasicRate._cosineLoss (mcquic/loss/__init__.py:27-44) over one level's codebook [m, k, d] without the [k, k]
 * Gram matrix: with p = c c^T per group, n_i = sum_t c_it^2 and cos_ij = p_ij / sqrt(n_i n_j),
 *   mcq_codebook_cos_f32      loss[0] = sum over groups and pairs i < j of clamp(cos_ij, 0, 2)  (three launches);
 *   mcq_codebook_cos_bwd_f32  dcodebook[g, i, :] = gamma dout[0] sum_{j != i, 0 <= cos_ij <= 2} (c_j / s_ij - cos_ij c_i / n_i),
 *                             s_ij = sqrt(n_i n_j): the gradient of gamma * loss under clamp's inclusive mask, WRITTEN, not
 *                             accumulated (two launches); `dout` is a device scalar, `gamma` a host one.
 * A zero codeword makes the loss non-finite (0 / 0, as in the reference); the gradient's values for such a row are unspecified.
 * k == 1 gives loss 0 and gradient 0.  1 <= d <= 256 and m, k >= 1, else MCQ_EINVAL before any launch (as for a NULL pointer).
 * `workspace`: mcq_codebook_cos_workspace(m, k, d) bytes (0 for refused arguments), 8-byte aligned: per-workgroup double partials
 * and two floats per codeword, O(m k).  No atomics, no memset, every sum in a fixed order: equal inputs give equal bits, and both
 * calls are safe inside a captured hipGraph.  (The size query enqueues nothing and therefore takes no stream.) */
size_t mcq_codebook_cos_workspace(int32_t m, int32_t k, int32_t d);
int mcq_codebook_cos_f32(const float* codebook, float* loss, void* workspace, int32_t m, int32_t k, int32_t d, void* stream);
int mcq_codebook_cos_bwd_f32(const float* codebook, const float* dout, float gamma, float* dcodebook, void* workspace, int32_t m,
                             int32_t k, int32_t d, void* stream);

/* ---- training-mode quantizer forward (BASELINE config #5, forward half) ------------------------------ */

/* logits[n, g, y, x, k] = ((-1 * dist) / sqrt(k)) * max(temperature[g], bound), dist as in mcq_vq_assign_f32.
 * Replaces _logit (mcquic/modules/quantizer.py:181-183) and the temperature scaling of _sample (:204). */
int mcq_vq_logits_f32(const float* x, const float* cb_packed, const float* temperature /* [m] */, float bound,
                      float* logits, int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, void* stream);

/* Per latent vector, with the two uniform draws of the reference given as inputs u_drop, u_gumbel [N, m, h, w, k]:
 *   logits[c] += -1e9 where u_drop[c] ** drop_exponent[0] < freq_ema[g, c]      (_randomDrop, quantizer.py:194-200)
 *   codes        = argmax_c logits[c]                                            (forward, :232-239)
 *   sample_index = argmax_c softmax(logits + gumbel(u_gumbel))[c], sample_hot = (1 - s) + s with s the soft
 *   probability there: the value of y_hard - y_soft.detach() + y_soft, which is zero everywhere else
 *                                                                                (gumbelSoftmax, mcquic/nn/base.py:118-133) */
/* `rng_state` (round 4; NULL = both draws are given): {seed, offset} as two uint64 in DEVICE memory.  Where u_drop / u_gumbel is
 * NULL its draws are made inside the kernel from the state (stream 0 = the drop's, 1 = the Gumbel noise's): a counter-based
 * generator over (seed, offset, stream, element index), 24-bit uniforms in [0, 1) like torch.rand's -- the reference's
 * `torch.rand_like(logit)` tensors (2 x 134 MB at the first level of a training step) are never written or read.  The state is
 * read on the device, so a captured hipGraph sees the offset its host code advanced on the device before each replay. */
int mcq_vq_gumbel_sample_f32(float* logits, const float* u_drop /* or NULL */, const float* u_gumbel /* or NULL */,
                             const uint64_t* rng_state /* or NULL */, const float* freq_ema /* [m, k] */,
                             const float* drop_exponent /* device scalar */, int64_t* codes, int64_t* sample_index,
                             float* sample_hot, int64_t* code_counts /* [m, k] or NULL */, int32_t N, int32_t m, int32_t h, int32_t w,
                             int32_t k, void* stream);
/* `code_counts` (round 5): the level's code histogram -- what EntropyCoder.forward obtains by summing one-hot codes over images
 * and pixels (mcquic/modules/entropyCoder.py:33-35) -- is added to where each code is made (integer atomics: exact in any order);
 * the caller zeroes the buffer once per step (mcq_vq_step_prologue_f32). */
/* out[i] = the generator's draw for element i of `stream_id` under `rng_state` -- exactly what the two kernels around it use in
 * place of a NULL u_drop (stream 0) / u_gumbel (stream 1): for tests and for callers that want the tensors after all. */
int mcq_hash_uniform_f32(const uint64_t* rng_state, uint32_t stream_id, float* out, int64_t n, void* stream);

/* out[n, g*d + j, y, x] = sample_hot * codebook[g, sample_index, j]: bmm(sample, codebook) for the one-hot-valued
 * straight-through sample (_multiCodebookDeQuantization.forward, quantizer.py:262-274). */
int mcq_vq_dequant_soft_f32(const int64_t* sample_index, const float* sample_hot, const float* codebook, float* out,
                            float* out_silu /* or NULL: also silu(out), the consumer's first activation */,
                            int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, void* stream);

/* out[n, g, y, x, k] = <x_v, c_k>: the logits kernel's GEMM without the distance / temperature transform
 * (backward: dSample = dDeq . C^T, the adjoint of quantizer.py:262-274). */
int mcq_vq_inner_f32(const float* x, const float* cb_packed, float* out, int32_t N, int32_t m, int32_t d, int32_t h, int32_t w,
                     int32_t k, void* stream);

/* Backward of gumbelSoftmax(hard=True) + _logit per latent vector: ds_inout holds dSample on entry and d dist on
 * exit; rowsum[v] = sum_k d dist, dtrow[v] = the vector's contribution to d max(temperature, bound).
 * `dlogits` (NULL = none): a gradient on the logits the forward returned (quantizer.py:232-239 returns them with their
 * graph); it is added in front of `_logit`.  The random drop's `+= -1e9` (quantizer.py:194-200) passes gradients through,
 * so dropped entries take part and `raw_logits` = the logits WITHOUT the drop (mcq_vq_logits_f32 again) must come along. */
int mcq_vq_softmax_bwd_f32(const float* logits, const float* u_gumbel /* or NULL: remade from rng_state */, const uint64_t* rng_state /* or NULL */,
                           float* ds_inout, const float* temperature, float bound,
                           float* rowsum, float* dtrow, const float* dlogits, const float* raw_logits,
                           int32_t N, int32_t m, int32_t h, int32_t w, int32_t k, void* stream);

/* Latent and codebook gradients of dist = |x|^2 + |c|^2 - 2 <x, c> given d dist, plus the codebook gradient of
 * sample @ codebook (rows sample_index scaled by sample_hot).  Deterministic (no atomics). */
int mcq_vq_soft_bwd_f32(const float* ddist, const float* rowsum, const float* x, const float* x_nhwc, const float* ddeq_nhwc,
                        const int64_t* sample_index, const float* sample_hot, const float* codebook, float* dx,
                        float* dcodebook, int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, void* stream);

/* Read-only: which kernel forms mcq_vq_soft_bwd_f32 runs for a shape.  out[3] = {dx_form, dc_form, dx_split}: the form of the latent
 * and of the codebook contraction -- 0 lane-per-channel (any shape), 1 tiled, 2 MFMA -- and the workgroups per 32-row tile of the
 * MFMA dx form (2: the codewords are halved and the parts added onto a zeroed dx; 1 otherwise and for forms 0 / 1).  Host code
 * only; the routing the entry point itself launches by.  Returns 1, or 0 (out untouched) for a shape the entry point refuses
 * (MCQ_EINVAL / MCQ_ETOOLARGE) and for a NULL out. */
int mcq_vq_soft_bwd_plan(int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, int32_t* out);

/* ---- per-step bookkeeping of the training quantizer (round 5; csrc/step_ops.hip) ------------------------------ */
#define MCQ_VQ_MAX_LEVELS 32   /* (8 until ABI 9; the reference's generator configs run 17 levels) */
/* the cap a binding chunks by (returns MCQ_VQ_MAX_LEVELS of the library it loaded) */
int32_t mcq_vq_max_levels(void);
/* ONE launch in front of the level cascade of a training forward (host arrays of `levels` <= MCQ_VQ_MAX_LEVELS entries):
 *   exponents[l] = -(log2 k_l - 1) * usage_l^2 + log2 k_l,  usage_l = mean(freq_ema_l > eps) clamped to [0, 1]
 *                  -- the exponent of _randomDrop (mcquic/modules/quantizer.py:194-198), rounded op by op like torch;
 *   rng_snaps[l] = {seed, offset + l} and the generator state {seed, offset} advanced by `levels` (both NULL: no generator);
 *   counts[0 .. counts_n) = 0  (the buffer mcq_vq_gumbel_sample_f32 adds the levels' code histograms into; NULL / 0: none).
 * Replaces seven tensor ops per level and the generator's clone + add. */
int mcq_vq_step_prologue_f32(const float* const* freq_ema /* [levels] device pointers to [m_l, k_l] */, const int32_t* m, const int32_t* k,
                             int32_t levels, float eps, float* exponents /* device [levels] */, uint64_t* rng_state /* device, or NULL */,
                             uint64_t* rng_snaps /* device [levels][2], or NULL */, int64_t* counts /* device, or NULL */, int64_t counts_n,
                             void* stream);
/* dtemperature[g] = mask_g * sum_{n, y, x} dtrow[n, g, y, x] with mask_g = (temperature[g] >= bound) | (sum < 0): the soft-max
 * backward's per-row temperature terms reduced in a fixed order, then LowerBound's gradient rule (mcquic/nn/base.py:24-29). */
int mcq_vq_temperature_grad_f32(const float* dtrow /* [N, m, hw] */, const float* temperature /* [m] */, float bound,
                                float* dtemperature /* [m] */, int32_t N, int32_t m, int32_t hw, void* stream);
/* freq_ema_l = (1 - ema) * counts_l / sum_k counts_l + ema * freq_ema_l for every level in ONE launch, in place
 * (EntropyCoder.forward, mcquic/modules/entropyCoder.py:28-44, after its all-reduce); `counts` = the levels' [m_l, k_l]
 * histograms back to back (mcq_vq_gumbel_sample_f32's code_counts). */
int mcq_freq_ema_update_f32(float* const* freq_ema /* [levels] device pointers */, const int32_t* m, const int32_t* k, int32_t levels,
                            const int64_t* counts, double ema /* a Python float on the reference side */, void* stream);
/* mcq_nonneg_reparam_bwd_f32 (below) for two parameters -- a GDN layer's beta [C] and gamma [C, C] -- in one launch. */
int mcq_nonneg_reparam_bwd2_f32(const float* p0, const float* dfolded0, float bound0, float* dp0, int64_t n0, const float* p1,
                                const float* dfolded1, float bound1, float* dp1, int64_t n1, void* stream);

/* ---- backward pass of the training step (BASELINE config #5) ----------------------------------------- */
/* Input gradients of the convolutions reuse mcq_conv2d_f32 with transformed weights (see mcquic_amd/autograd.py);
 * the reference obtains all of these from torch.autograd over nn.Conv2d / SiLU / GDN / sigmoid
 * (mcquic/nn/convs.py, nn/gdn.py:67-91, nn/blocks.py:70-78,281-288). */

/* Backward of mcq_nonneg_reparam_f32 under LowerBound's gradient rule (mcquic/nn/base.py:17-29,81-84):
 * g = 2 max(p, bound) dfolded;  dp = g where p >= bound or g < 0, else 0. */
int mcq_nonneg_reparam_bwd_f32(const float* p, const float* dfolded, float bound, float* dp, int64_t n, void* stream);

/* out[n][p][c] = x[n][c][p] (squared if `square`): channel-major copies feeding the weight-gradient GEMM. */
int mcq_nchw_to_nhwc_f32(const float* x, float* out, int32_t N, int32_t C, int32_t HW, int32_t square, void* stream);
/* The same for the two operands of one weight-gradient GEMM (x [N,Cx,HWx], squared if `square_x`, and y [N,Cy,HWy]) in
 * a single launch. */
int mcq_nchw_to_nhwc_pair_f32(const float* x, float* x_out, int32_t Cx, int32_t HWx, int32_t square_x, const float* y,
                              float* y_out, int32_t Cy, int32_t HWy, int32_t N, void* stream);

/* dW[co][ci][ky][kx] = sum_{n,yo,xo} dY[n][co][yo][xo] * X[n][ci][yo*stride + ky - k/2][xo*stride + kx - k/2]
 * from NHWC copies of X [N,H,W,Cin] and dY [N,Ho,Wo,Cout]; `workspace` holds the per-range partial sums.  If `dbias` is
 * not NULL it also receives db[co] = sum_{n,yo,xo} dY[n][co][yo][xo] (the bias gradient of the same conv, summed by the
 * waves that stream dY anyway). */
size_t mcq_conv2d_wgrad_workspace_floats(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t ksize,
                                         int32_t stride);
int mcq_conv2d_wgrad_f32(const float* x_nhwc, const float* dy_nhwc, float* dw, float* dbias, float* workspace, int32_t N,
                         int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t ksize, int32_t stride, void* stream);

/* The same gradient for 3x3 stride-1 convolutions straight from the NCHW tensors X [N,Cin,H,W] and dY [N,Cout,H,W], W a
 * multiple of 8, each tensor below 1 GiB (mcq_conv2d_wgrad_nchw_workspace_floats returns 0 for any other shape: use the
 * NHWC entry point then).  No channel-major copies: a wave walks an 8-pixel strip down the rows with a three-row window of
 * X in registers, all nine taps per dY operand (csrc/wgrad_rows.hip).  Deterministic.
 * Shapes with N H W <= 512 pixels, H W a multiple of 4 (<= 256) and channel counts in sixteens -- the 4x4 / 8x8 maps of a training
 * step -- take a one-pass kernel on 16 x 16 tiles instead (csrc/wgrad_t16.h: whole images staged in LDS, no partial sums): the
 * workspace query returns 1 for them (as for the other small maps) and `workspace` is not touched.  The same holds for the 1x1
 * entry point below. */
size_t mcq_conv2d_wgrad_nchw_workspace_floats(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout);
int mcq_conv2d_wgrad_nchw_f32(const float* x, const float* dy, float* dw, float* dbias, float* workspace, int32_t N, int32_t Cin,
                              int32_t H, int32_t W, int32_t Cout, void* stream);
/* `nconv` (1 .. mcq_conv2d_wgrad_nchw_max_group()) convolutions of ONE shape in one launch pair: x[c], dy[c] -> dw[c], dbias[c]
 * (dbias NULL, or NULL entries, for none).  The pointer tables are host arrays read during the call; `workspace` holds
 * nconv * mcq_conv2d_wgrad_nchw_workspace_floats(...) floats.  The 16x16 ... 8x8 levels of a training step are
 * launch-bound: a block's weight gradients go out together (mcquic_amd/autograd.py). */
int32_t mcq_conv2d_wgrad_nchw_max_group(void);
int mcq_conv2d_wgrad_nchw_group_f32(const float* const* x, const float* const* dy, float* const* dw, float* const* dbias,
                                    int32_t nconv, float* workspace, int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                                    void* stream);

/* The 3x3 stride-2 case (ResidualBlockWithStride's convs, the 3-channel stem): X [N,Cin,H,W] with H, W even, dY
 * [N,Cout,H/2,W/2], W/2 a multiple of 8.  The walk runs over dY's rows with a ring of four input rows. */
size_t mcq_conv2d_wgrad_s2_nchw_workspace_floats(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout);
int mcq_conv2d_wgrad_s2_nchw_f32(const float* x, const float* dy, float* dw, float* dbias, float* workspace, int32_t N, int32_t Cin,
                                 int32_t H, int32_t W, int32_t Cout, void* stream);

/* The 1x1 case (the AttentionBlock gate conv; with square_x the gamma of GDN / IGDN, whose operand is x^2,
 * mcquic/nn/gdn.py:75): dW[co][ci] = sum dY[co] * X[ci] straight from NCHW, H even, W a multiple of 8.  The workspace query
 * returns 0 for shapes this kernel does not take. */
size_t mcq_conv2d_wgrad1x1_nchw_workspace_floats(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout);
int mcq_conv2d_wgrad1x1_nchw_f32(const float* x, const float* dy, float* dw, float* dbias, float* workspace, int32_t N, int32_t Cin,
                                 int32_t H, int32_t W, int32_t Cout, int32_t square_x, void* stream);

/* Read-only: the plan the strip walk of the three entry points above would run for X [N,Cin,H,W] -- `taps` 9 or 1, `stride2` the
 * 3x3 stride-2 form (H, W: the input map, as its entry point takes them), `nconv` the convolutions sharing the launch (only
 * mcq_conv2d_wgrad_nchw_group_f32 launches more than one; for the other forms the plan is what the planner would hand such a
 * launch).  out[9] = {F, strips, row_chunks, rpc, units, splits, ups, groups, gmax}: floats a lane reads per row, strips per row,
 * row ranges per (image, strip), rows per range, walks = N strips row_chunks, waves per tile, walks per wave, workgroups per tile
 * and convolution = ceil(splits / 4), and the groups the workspace query sizes by -- after the fall-back of a grouped plan that
 * would need more groups than that to the one-by-one plan.  The launch writes nconv * groups * (taps Cout Cin + 4 Cout) floats
 * of `workspace`.  Host code only; the planner the launchers call.  Returns 1, or 0 (out untouched) for a shape the strip walk
 * does not take: the one-pass 16 x 16-tile kernel's, the small-map kernel's, or one for the NHWC entry point. */
int32_t mcq_conv2d_wgrad_nchw_plan(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t taps, int32_t stride2,
                                   int32_t nconv, int32_t* out);

/* out[c] = sum_{n,p} x[n][c][p]   (bias / beta gradients); optional workspace of min(N, 16) * C floats. */
int mcq_channel_sum_f32(const float* x, float* out, float* workspace, int32_t N, int32_t C, int32_t HW, void* stream);

/* Stand-alone forms of ops that the inference path fuses into conv prologues / epilogues; the training graph keeps
 * them separate so that each has its own backward:  y = silu(x);  out = a * sigmoid(b) + x;  out = alpha a + beta b. */
int mcq_silu_f32(const float* x, float* y, int64_t n, void* stream);
int mcq_gate_f32(const float* a, const float* b, const float* x, float* out, float* out_silu /* or NULL */, int64_t n, void* stream);
int mcq_axpby_f32(const float* a, const float* b, float alpha, float beta, float* out, float* out_silu /* or NULL */, int64_t n,
                  void* stream);

/* dx = dy * d/dx silu(x) (+ other: the gradient reaching x along a second path, e.g. a strided block's skip convolution,
 * mcquic/nn/blocks.py:98-122 -- the sum torch.autograd's engine would make with a launch of its own). */
int mcq_silu_bwd_f32(const float* x, const float* dy, const float* other /* or NULL */, float* dx, int64_t n, void* stream);

/* AttentionBlock gate out = a * sigmoid(b) + x: da = dout * s, db = dout * a * s (1 - s). */
int mcq_gate_bwd_f32(const float* a, const float* b, const float* dout, float* da, float* db, int64_t n, void* stream);

/* GDN / IGDN y = x * f(s): dx_direct = dy * f(s), ds = dy * x * f'(s) (f = s^-1/2, or s^1/2 when `inverse`). */
int mcq_gdn_bwd_prep_f32(const float* x, const float* s, const float* dy, int32_t inverse, float* dx_direct, float* ds,
                         int64_t n, void* stream);

/* out[n][c*4 + i*2 + j][y][x] = in[n][c][2y + i][2x + j]: the adjoint of nn.PixelShuffle(2). */
int mcq_pixel_unshuffle2_f32(const float* in, float* out, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);

/* ---- small element-wise helpers on the path ------------------------------------------------ */

/* out = a + b  (quantizer.py:354  xHat = q + sideHead(formerLevel)). */
int mcq_add_f32(const float* a, const float* b, float* out, float* out_silu /* or NULL */, int64_t n, void* stream);
/* out = (a + b) + c: the three gradient paths that meet at the input of an AttentionBlock (main stack, side stack, the gate's
 * identity term; what torch.autograd accumulates with two additions for mcquic/nn/blocks.py:281-288) in one launch. */
int mcq_add3_f32(const float* a, const float* b, const float* c, float* out, int64_t n, void* stream);

/* mean((a - b)^2) over n floats -> out[0] (F.mse_loss, the distortion term of mcquic/loss/__init__.py:62), and its gradient
 * da = 2 (a - b) / n * dloss[0] (db = -da when non-NULL).  Two launches, a fixed summation order (double partials in
 * `workspace`, mcq_mse_workspace_bytes(n) bytes) and no memset: safe inside a captured hipGraph, which a library reduction that
 * zeroes semaphores with hipMemsetAsync is not on ROCm 7.2 ("graph replays"). */
size_t mcq_mse_workspace_bytes(int64_t n);
int mcq_mse_f32(const float* a, const float* b, float* out, void* workspace, int64_t n, void* stream);
int mcq_mse_bwd_f32(const float* a, const float* b, const float* dloss, float* da, float* db /* or NULL */, int64_t n, void* stream);
/* Gradient clipping by global norm over ONE flat buffer (mcquic/train/trainer.py:280 `self._optimizer.clip_grad_norm(4.0)`;
 * torch.nn.utils.clip_grad_norm_'s arithmetic): out[0] = sum(x^2) with the reduction above (workspace: mcq_mse_workspace_bytes(n)),
 * then x *= max_norm / (sqrt(sumsq) + eps) where that factor is < 1; the norm goes to norm_out[0] when non-NULL.  Everything
 * stays on the device: no host read between the two launches, so both are captured with the optimizer's update. */
int mcq_sumsq_f32(const float* x, float* out, void* workspace, int64_t n, void* stream);
int mcq_clip_by_norm_f32(float* x, const float* sumsq, float max_norm, float eps, float* norm_out /* or NULL */, int64_t n, void* stream);

/* Many tensors -> their slices of one flat buffer in ONE launch (the gradients of a captured training step into the buffer the
 * all-reduce and the optimizer read; torch.cat moves 666 tensors in six launches): device tables as for mcq_adam_step_f32 --
 * `src_ptrs` [ntensors] addresses, `dst_offsets` / `numel` [ntensors] in floats, and one (tensor, first element) entry per
 * mcq_adam_chunk()-element chunk in `blk_tensor` / `blk_first` [nblocks]. */
int mcq_gather_flat_f32(const void* src_ptrs, float* flat, const int64_t* dst_offsets, const int64_t* numel, const int32_t* blk_tensor,
                        const int64_t* blk_first, int32_t nblocks, void* stream);

/* Gradient accumulation over the k micro-steps of one update (parallel.GraphedTrainStep(accumulate=k)).  `phase` is ONE device
 * int32 the host sets between launches (0 .. k-1): the same captured launch serves every micro-step.
 *   mcq_gather_accum_flat_f32  mcq_gather_flat_f32's tables and walk; per element, in float32 and in this order:
 *                                phase 0            flat = src
 *                                0 < phase < k-1    flat = flat + src
 *                                phase = k-1        flat = (flat + src) * (1.0f / k)      (one add, then one multiply)
 *                              so that k launches leave (((g0 + g1) + ...) + g_{k-1}) * fl(1 / k).  The slices are only 4-byte
 *                              aligned: 128-bit accesses between a scalar head and tail.  k < 2 is MCQ_EINVAL (mcq_gather_flat_f32
 *                              is the copy).  A phase outside 0 .. k-1 is taken as the nearer end.
 *   mcq_accum_step_scalars     the step's scalars by the same phases in one launch: counts_acc[i] = counts[i] at phase 0 and
 *                              += counts[i] afterwards (n int64 code counts: exact), and loss_acc[0] from loss[0] by the rule above
 *                              (the mean of the k micro losses after the last phase).  Either pair may be NULL (with n = 0 for
 *                              the counts), not both. */
int mcq_gather_accum_flat_f32(const void* src_ptrs, float* flat, const int64_t* dst_offsets, const int64_t* numel, const int32_t* blk_tensor,
                              const int64_t* blk_first, int32_t nblocks, const int32_t* phase, int32_t k, void* stream);
int mcq_accum_step_scalars(const int64_t* counts, int64_t* counts_acc, int64_t n, const float* loss, float* loss_acc, const int32_t* phase,
                           int32_t k, void* stream);

/* Adam / AdamW over a whole model in ONE launch (the `self._optimizer.step()` of mcquic/train/trainer.py:283 with the reference's
 * `Adam`, configs/a800_8.yaml:20-25; arithmetic of torch.optim.Adam / AdamW: lerp of exp_avg, mul + addcmul of exp_avg_sq, bias
 * corrections from the step count, param -= lr / bc1 * exp_avg / (sqrt(exp_avg_sq) / sqrt(bc2) + eps); L2 or decoupled decay).
 * All lists are DEVICE arrays: ptr_tables = uint64[4][ntensors] (param, grad, exp_avg, exp_avg_sq addresses), numel[ntensors],
 * and one (blk_tensor, blk_first) entry per mcq_adam_chunk()-element chunk of every tensor (nblocks entries).  `step` is a device
 * float the call increments; `lr_dev` (device float) overrides `lr` when non-NULL, so a scheduled rate needs no re-capture;
 * `scalars` = 16 bytes of device scratch.  Two launches, nothing read by the host. */
int32_t mcq_adam_chunk(void);
int mcq_adam_step_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                      int32_t nblocks, float* step, const float* lr_dev /* or NULL */, double lr, double beta1, double beta2, double eps,
                      double weight_decay, int32_t decoupled, int32_t maximize, void* scalars, void* stream);

/* LAMB over many tensors with per-tensor trust ratios (the reference's `FusedLAMB` registry entry, mcquic/train/ddp.py:53-69; the
 * arithmetic is written out in mcquic_amd/optim.py `Lamb`).  Tables as for mcq_adam_step_f32, chunks of mcq_adam_chunk() elements,
 * plus tensor_first_blk[ntensors + 1]: tensor t owns chunks [tensor_first_blk[t], tensor_first_blk[t + 1]).
 *   mcq_lamb_grad_partials_f32  partials[b] = sum of g^2 over chunk b, b < nblocks (double; one launch).  Called once per parameter
 *                               group into consecutive slices of ONE array: the gradient norm spans all groups.
 *   mcq_lamb_step_f32           four launches: the n_grad_partials partials summed in a fixed order -> G (to grad_norm[0]), the clip
 *                               divisor G / max_grad_norm (1 unless G > max_grad_norm), `step` += 1, bias corrections; m and v
 *                               updated with (sum p^2, sum u^2) per chunk; per tensor ratios[t] = ||p|| / ||u|| and the rate lr * that
 *                               (lr alone unless use_nvlamb or weight_decay != 0, or where a norm is zero); p -= rate * u.
 *                               Gradients are only read.  `workspace`: mcq_lamb_workspace_bytes(ntensors, nblocks) bytes (0 for
 *                               non-positive arguments), 8-byte aligned; `scalars` = 16 bytes of device scratch; `lr_dev` as above.
 * All sums are doubles reduced in fixed trees (no atomics): equal inputs give equal bits.  Nothing is read by the host. */
size_t mcq_lamb_workspace_bytes(int32_t ntensors, int32_t nblocks);
int mcq_lamb_grad_partials_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                               const int64_t* blk_first, int32_t nblocks, double* partials, void* stream);
int mcq_lamb_step_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                      const int32_t* tensor_first_blk, int32_t nblocks, const double* grad_partials, int32_t n_grad_partials,
                      float* step, const float* lr_dev /* or NULL */, double lr, double beta1, double beta2, double eps, double weight_decay,
                      int32_t bias_correction, int32_t adam_w_mode, int32_t grad_averaging, int32_t use_nvlamb, double max_grad_norm,
                      float* grad_norm, float* ratios, void* workspace, void* scalars, void* stream);

/* SGD over a whole model in one launch (the `self._optimizer.step()` of mcquic/train/trainer.py:283 with the reference's `"SGD"`
 * registry entry, mcquic/train/ddp.py:53-69; torch.optim.SGD's arithmetic per element in float32: g = maximize ? -grad : grad;
 * g += weight_decay p; with momentum buf = g on the update where `step` was 0, else buf = momentum buf + (1 - dampening) g, and
 * g = nesterov ? g + momentum buf : buf; p -= lr g).  Tables, `step`, `lr_dev` / `lr` and `scalars` as for mcq_adam_step_f32; row 2 of
 * ptr_tables holds the momentum buffers (read only when momentum != 0), row 3 is not read.  Two launches: a scalar kernel and one pass
 * over 12 bytes per element (20 with momentum), 16 bytes per lane where all of a tensor's addresses are 16-byte aligned.
 * With `grad_partials` (n_grad_partials doubles from mcq_lamb_grad_partials_f32, every parameter group's in one array: a third
 * launch, in front) the scalar kernel sums them in a fixed order -> G, written to grad_norm[0], and
 *   max_grad_norm (device float, or NULL)  grad is multiplied by min(1, max_grad_norm / (G + 1e-6)) before everything else
 *                                          (torch.nn.utils.clip_grad_norm_'s arithmetic; the gradients themselves are only read);
 *   skip_nonfinite                         when G is not finite the call changes no parameter, no buffer and not `step`, and adds 1 to
 *                                          skipped[0] (device int64, or NULL: a caller with several parameter groups counts a call
 *                                          once); every workgroup reads the flag on the device.
 * Without grad_partials all three must be 0 / NULL.  No atomics: equal inputs give equal bits.  Nothing is read by the host. */
int mcq_sgd_step_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                     int32_t nblocks, float* step, const float* lr_dev /* or NULL */, double lr, double momentum, double dampening,
                     double weight_decay, int32_t nesterov, int32_t maximize, const double* grad_partials /* or NULL */,
                     int32_t n_grad_partials, const float* max_grad_norm /* or NULL */, float* grad_norm /* or NULL without grad_partials */,
                     int32_t skip_nonfinite, int64_t* skipped /* or NULL */, void* scalars, void* stream);

/* Exponential moving average of a whole model's weights in one launch, and the in-place exchange of the live and the averaged
 * weights (csrc/ema.hip; host mirror mcquic_amd.optim.EMA).  Tables as for mcq_adam_step_f32: row 0 of ptr_tables holds the live
 * parameters (only read by the update), row 1 the averages, rows 2 and 3 are not read.
 *   mcq_ema_update_f32  two launches.  A scalar kernel reads n = num_updates[0] (device int64), takes d = decay, or decay_dev[0]
 *                       (device float) when non-NULL, with `warmup` d = min(d, (1 + n) / (10 + n)) in double, writes the weight
 *                       w = float(1 - d) to `scalars` (16 bytes of device scratch) and stores n + 1; then one pass over 12 bytes
 *                       per element, avg = lerp(avg, p, w) in float32 with torch's lerp (what torch.optim.swa_utils'
 *                       get_ema_multi_avg_fn runs): avg + w (p - avg) where w < 0.5, p - (p - avg) (1 - w) otherwise, so decay 0
 *                       leaves avg == p bit for bit.  `decay` must lie in [0, 1] (pass 0 with decay_dev).
 *   mcq_ema_swap_f32    one launch, 16 bytes per element: rows 0 and 1 exchanged as raw 32-bit words (NaN payloads and the sign of
 *                       -0.0 survive; two swaps are the identity on bits).
 * 16 bytes per lane where both rows of a tensor are 16-byte aligned, dwords otherwise.  No atomics: equal inputs give equal bits.
 * Nothing is read by the host, so both are captured like the optimizers' updates. */
int mcq_ema_update_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                       int32_t nblocks, int64_t* num_updates, const float* decay_dev /* or NULL */, double decay, int32_t warmup,
                       void* scalars, void* stream);
int mcq_ema_swap_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                     int32_t nblocks, void* stream);

/* The non-finite guard of a training step (csrc/step_guard.hip; host mirror mcquic_amd.guard.StepGuard): ONE flag per step, decided on
 * the device from the global norm G of the gradient, and the `_skip` forms of every entry point of the update, which obey it.
 * `record` = 24 bytes of device memory, 8-byte aligned, zero-initialised by the owner:
 *     { int32 skip; float grad_norm; int64 skipped; int64 consecutive }
 * A guard call stores skip = !isfinite(G) and grad_norm = float(G); a skipped step adds 1 to `skipped` and to `consecutive`, a clean one
 * stores consecutive = 0.  G = sqrt(sum g^2) as csrc/sgd.hip forms it: one double partial per mcq_adam_chunk()-element chunk, every sum
 * a fixed tree (no atomics: equal inputs give equal bits; a finite gradient of 1e19 per element is NOT an overflow of its squares).
 *   mcq_step_guard_list_f32      the gradients of a tensor table (row 1; tables as for mcq_adam_step_f32): this table's nblocks partials into
 *                                `partials`; then, unless `record` is NULL (a further parameter group follows), the n_all_partials
 *                                doubles at `all_partials` are summed and the record written.  Two launches (one without record).
 *   mcq_step_guard_flat_f32      the same over one flat buffer of n floats; `partials`: mcq_step_guard_chunks(n) doubles.
 *   mcq_step_guard_partials_f32  the record from partials that exist already (LAMB's and SGD's own, mcq_lamb_grad_partials_f32): one
 *                                launch of one workgroup, no second pass over the gradients.
 *   mcq_step_guard_norm_f32      the record from a float32 norm (squared = 0) or sum of squares (squared != 0: sqrtf of it, as
 *                                mcq_clip_by_norm_f32 takes mcq_sumsq_f32's) that exists already: one launch of one lane.  The flag is then
 *                                the lender's arithmetic -- a float32 sum of squares that overflowed is skipped.
 * The `_skip` entry points take `const int32_t* skip` (= record, or NULL) in front of `stream` and are otherwise the entry points of the
 * same name: with NULL they ARE those (the same kernels, launch for launch); with a pointer every workgroup reads the word once,
 * branches uniformly, and when it is non-zero the launch writes nothing -- no parameter, moment, step count, average, update count,
 * schedule state, rate or frequency entry (mcq_clip_by_norm_skip_f32 still stores norm_out; mcq_sgd_step_skip_f32 stores the scratch
 * word its second launch obeys and leaves SGD's own `skipped` alone).  Nothing is read by the host. */
int64_t mcq_step_guard_chunks(int64_t n);
int mcq_step_guard_list_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                            int32_t nblocks, double* partials, const double* all_partials /* or NULL without record */, int32_t n_all_partials,
                            void* record /* or NULL */, void* stream);
int mcq_step_guard_flat_f32(const float* grad, int64_t n, double* partials, void* record, void* stream);
int mcq_step_guard_partials_f32(const double* partials, int32_t n_partials, void* record, void* stream);
int mcq_step_guard_norm_f32(const float* value, int32_t squared, void* record, void* stream);
int mcq_clip_by_norm_skip_f32(float* x, const float* sumsq, float max_norm, float eps, float* norm_out /* or NULL */, int64_t n,
                              const int32_t* skip /* or NULL */, void* stream);
int mcq_adam_step_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                           int32_t nblocks, float* step, const float* lr_dev /* or NULL */, double lr, double beta1, double beta2, double eps,
                           double weight_decay, int32_t decoupled, int32_t maximize, void* scalars, const int32_t* skip /* or NULL */, void* stream);
int mcq_lamb_grad_partials_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                    const int64_t* blk_first, int32_t nblocks, double* partials, const int32_t* skip /* or NULL */, void* stream);
int mcq_lamb_step_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                           const int32_t* tensor_first_blk, int32_t nblocks, const double* grad_partials, int32_t n_grad_partials,
                           float* step, const float* lr_dev /* or NULL */, double lr, double beta1, double beta2, double eps, double weight_decay,
                           int32_t bias_correction, int32_t adam_w_mode, int32_t grad_averaging, int32_t use_nvlamb, double max_grad_norm,
                           float* grad_norm, float* ratios, void* workspace, void* scalars, const int32_t* skip /* or NULL */, void* stream);
int mcq_sgd_step_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                          int32_t nblocks, float* step, const float* lr_dev /* or NULL */, double lr, double momentum, double dampening,
                          double weight_decay, int32_t nesterov, int32_t maximize, const double* grad_partials /* or NULL */,
                          int32_t n_grad_partials, const float* max_grad_norm /* or NULL */, float* grad_norm /* or NULL without grad_partials */,
                          int32_t skip_nonfinite, int64_t* skipped /* or NULL */, void* scalars, const int32_t* skip /* or NULL */, void* stream);
int mcq_ema_update_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                            int32_t nblocks, int64_t* num_updates, const float* decay_dev /* or NULL */, double decay, int32_t warmup,
                            void* scalars, const int32_t* skip /* or NULL */, void* stream);
int mcq_freq_ema_update_skip_f32(float* const* freq_ema /* [levels] device pointers */, const int32_t* m, const int32_t* k, int32_t levels,
                                 const int64_t* counts, double ema, const int32_t* skip /* or NULL */, void* stream);

/* Codebook reassignment inside the step (csrc/vq_reassign.hip; host mirror mcquic_amd.reassign.CodebookReassign): every `every` updates
 * the dead codewords (normalised frequency < 1e-6) of every level and group are overwritten by the most used ones, by the rule of
 * mcquic/modules/quantizer.py:111-136 -- TWO launches per step for all levels and groups, which on a step that does not fire read the
 * decision and return.  Level tables as for mcq_freq_ema_update_f32 (host arrays of `levels` <= MCQ_VQ_MAX_LEVELS entries; a binding
 * chunks beyond: every plan launch of a step first, then every apply launch).
 *   `state`   int64 [MCQ_REASSIGN_STATE_WORDS] on the device:
 *               0 count       completed updates; advanced by the plan launch with `advance` (the first table of a step)
 *               1 seen        the count the last apply launch with `last` committed (what the plan launch decides from)
 *               2 fired       steps that fired
 *               3 moved       codewords that moved by more than 1e-4 in squared distance on the last step that fired
 *               4 proportion  moved / step_codewords of that step, a float32 in the low word (the reference's return value)
 *               5 seed, 6 offset   the generator state of the drawn priorities; offset += step_levels on a step that fires
 *   decision  with *skip set (the step's guard flag, see mcq_step_guard_list_f32; NULL = never) nothing moves and nothing is written,
 *             the count included.  Otherwise s = seen + 1 is the completed count after this update and the step fires when
 *             s >= start and (s + 1) % every == 0 (the reference increments its step and then tests (step + 1) % freq).
 *   plan      one workgroup per (level, group): from the RAW frequency row f [k] and the priority row (priority[l], or with priority
 *             or priority[l] NULL the generator's draws for stream MCQ_RNG_STREAM_REASSIGN under {seed, offset + level0 + l}, element
 *             g k + i: what mcq_hash_uniform_f32 returns for it) `source` [m, k] (donor index per codeword, its own where nothing moves)
 *             and `refill` [m, k] (0 / 1).  The row sum is formed in double in a fixed order and rounded once to float32.  Ranks are
 *             counted over the row held in LDS (k^2 compares per ordering), stable with ties by index; k > mcq_vq_reassign_max_k()
 *             is MCQ_EINVAL.
 *   apply     ONE workgroup: per group the donor rows are gathered into `scratch` (max k_l d_l floats) before any row of the group is
 *             written (a donor can itself be refilled), `changed` [m, k] (0 / 1) = squared distance > 1e-4 in float32 summed over d
 *             in index order; `first` starts `moved` at 0, `last` forms proportion from step_codewords (the sum of m_l k_l over the
 *             step) and commits seen, fired and the generator's offset. */
#define MCQ_REASSIGN_MAX_K 8192
#define MCQ_REASSIGN_STATE_WORDS 7
#define MCQ_RNG_STREAM_REASSIGN 3u
int32_t mcq_vq_reassign_max_k(void);
int mcq_vq_reassign_plan(const float* const* freq_ema /* [levels] device pointers */, const float* const* priority /* or NULL; entries or NULL */,
                         const int32_t* m, const int32_t* k, int32_t levels, int32_t level0, int32_t advance, int32_t* const* source,
                         uint8_t* const* refill, int64_t* state, int64_t every, int64_t start, const int32_t* skip /* or NULL */, void* stream);
int mcq_vq_reassign_apply(float* const* codebook /* [levels] device pointers to [m_l, k_l, d_l] */, const int32_t* const* source,
                          const uint8_t* const* refill, uint8_t* const* changed, const int32_t* m, const int32_t* k, const int32_t* d,
                          int32_t levels, int32_t first, int32_t last, int32_t step_levels, int64_t step_codewords, float* scratch,
                          int64_t* state, int64_t every, int64_t start, const int32_t* skip /* or NULL */, void* stream);

/* The entropy coder's tables and code lengths on the device (csrc/vq_cdf.hip; callers: mcquic_amd.ops.pmf_to_quantized_cdf_dev /
 * code_bits, EntropyCoder.deviceCDFs / codeBits).  Level tables as for mcq_freq_ema_update_f32 (host arrays of `levels` <=
 * MCQ_VQ_MAX_LEVELS entries; a binding chunks beyond).  No atomics, no host read: equal inputs give equal bits, and both capture.
 *   mcq_pmf_to_quantized_cdf_dev   ONE launch, one workgroup per (level, group) row: pmf[l] float32 [m_l, k_l] -> cdf[l] uint32
 *             [m_l, k_l + 1], entry for entry what mcq_pmf_to_quantized_cdf (below) writes at precision 16 -- the same rounding, uint32
 *             total, 64-bit division, scan, cdf[k] = 65536 and steal loop (first index among the least widths > 1), the loop evaluated
 *             in closed form (the file's head has the argument).  `normalize`: each row is first divided by its sum, formed in double in
 *             a fixed order and rounded once to float32 (the rule of mcq_vq_reassign_plan's row sum); else the rows are taken as given.
 *             `status` int32 [sum m_l], (level, group) order: 0 valid; 1 a negative or non-finite element, or a scaled element or total
 *             beyond 32 bits; 2 a zero total (with `normalize`: a row sum of zero, tested before the division); 3 no donor left -- the
 *             host function's MCQ_EINVAL cases; that row's table is unspecified.
 *             k_l > mcq_cdf_max_k() is MCQ_EINVAL (the row is held in LDS).
 *   mcq_code_bits   ONE launch, one workgroup per (image, level): bits[i, level0 + l] = sum over groups g and positions of
 *             16 - log2(cdf_g[c + 1] - cdf_g[c]) for codes[l] int64 [n, m_l, h_l, w_l] (hw[l] = h_l w_l), accumulated in double in a
 *             fixed order; `bits` double and `error` int32 are [n, row_levels], both written by every launch: error = 1 where a code
 *             lay outside [0, k_l) or met a bin of width 0 (such a code adds nothing), else 0.  What the single-state rANS coder
 *             below spends beyond this sum is its 64-bit flush and its 32-bit renormalisation steps; bypass symbols are not modelled.
 *             n <= 65535 and m_l h_l w_l <= MCQ_CODE_BITS_MAX_SYMBOLS per image and level, else MCQ_ETOOLARGE. */
#define MCQ_CDF_MAX_K 8192
#define MCQ_CODE_BITS_MAX_SYMBOLS 0x40000000LL
int32_t mcq_cdf_max_k(void);
int mcq_pmf_to_quantized_cdf_dev(const float* const* pmf /* [levels] device pointers */, uint32_t* const* cdf /* [levels] device pointers */,
                                 const int32_t* m, const int32_t* k, int32_t levels, int32_t normalize, int32_t* status, void* stream);
int mcq_code_bits(const int64_t* const* codes /* [levels] device pointers */, const uint32_t* const* cdf /* [levels] device pointers */,
                  const int32_t* m, const int32_t* k, const int32_t* hw, int32_t levels, int32_t n, int32_t level0, int32_t row_levels,
                  double* bits, int32_t* error, void* stream);

/* The rANS coder itself on the device (csrc/rans_dev.hip; callers: mcquic_amd.ops.rans_encode_dev / rans_decode_dev,
 * EntropyCoder.compressDevice / decompressDevice): the byte streams of mcq_rans_encode_with_indexes (below), bit for bit -- 64-bit
 * state, L = 2^31, 16-bit precision, symbols in reverse, 32-bit words backwards, two flush words -- in integer arithmetic only.  Level
 * tables as for mcq_code_bits: codes[l] int64 [n, m_l, h_l, w_l] (hw[l] = h_l w_l), cdf[l] uint32 [m_l, k_l + 1] (the tables of
 * mcq_pmf_to_quantized_cdf_dev), host arrays of `levels` <= MCQ_VQ_MAX_LEVELS entries; a binding chunks beyond, naming its first
 * level among the `row_levels` levels of the batch as `level0`.  One stream per (image, level): the symbols are codes[l][i] flattened,
 * [m, h, w] order, the group index selecting the table.  Stream s = i * row_levels + level0 + l: image-major, the order of
 * `binaries[n][level]`.  No kernel reads back to the host, uses atomics or allocates: equal inputs give equal bytes, and all capture.
 *   mcq_rans_encode_dev   ONE launch, one workgroup per stream, into its slot of `scratch` [n row_levels, cap_bytes], filled from the
 *             slot's END: `sizes` int64 [n row_levels] = the stream's bytes (a multiple of 4), `status` int32 [n row_levels].  A code
 *             outside [0, k_l) or a bin of width 0 (as a uint16: the host's `Sym`) is MCQ_RANS_BAD_SYMBOL -- the host coder's
 *             MCQ_EINVAL -- found before anything is indexed with it; that stream's size is 0.  cap_bytes: a multiple of 4, at least
 *             4 (m_l h_l w_l + 2) for every level (a symbol emits at most one word, the flush two), else MCQ_EINVAL.
 *   mcq_rans_pack_dev     two launches: offsets int64 [streams + 1] = the exclusive scan of `sizes` (one workgroup), then every stream
 *             copied from its slot to blob + offsets[s] (one workgroup per stream).  `offsets` and `blob` are what leaves the device.
 *             A stream that would pass blob_bytes is not copied: give the blob the sum of the worst cases, 4 (m_l h_l w_l + 2) per stream.
 *   mcq_rans_decode_dev   ONE launch, one wave per stream: stream s is blob[offsets[s], offsets[s + 1]) and decodes straight into
 *             codes[l][i] as int64.  The stream is untrusted input: a size below 8 bytes or not a multiple of 4, offsets that decrease
 *             or reach beyond blob_bytes, running out of words, and a table whose bins do not increase are
 *             MCQ_RANS_BAD_STREAM for that stream only, which leaves its outputs ZEROED; every read of a stream word is bounded by
 *             the stream's own extent, itself checked against blob_bytes first.
 * NOT on the device: the 4-bit bypass digits (a value at or beyond the table's sentinel slot).  With cdf_sizes = k + 2 over k + 1
 * entries, as the product passes them, no code in [0, k) reaches the sentinel; such a code is the status word here.
 * k_l <= MCQ_CDF_MAX_K (the decoder holds a table in LDS; MCQ_EINVAL), n <= 65535 and m_l h_l w_l <= MCQ_RANS_DEV_MAX_SYMBOLS per
 * stream, else MCQ_ETOOLARGE.  MCQ_RANS_DEV_CHUNK: symbols (and words) the kernels hold in LDS at a time -- what tests place their
 * stream lengths around. */
#define MCQ_RANS_DEV_CHUNK 1024
#define MCQ_RANS_DEV_MAX_SYMBOLS 0x10000000LL
#define MCQ_RANS_OK 0
#define MCQ_RANS_BAD_SYMBOL 1
#define MCQ_RANS_BAD_STREAM 2
int mcq_rans_encode_dev(const int64_t* const* codes /* [levels] device pointers */, const uint32_t* const* cdf /* [levels] device pointers */,
                        const int32_t* m, const int32_t* k, const int32_t* hw, int32_t levels, int32_t n, int32_t level0, int32_t row_levels,
                        uint8_t* scratch, int64_t cap_bytes, int64_t* sizes, int32_t* status, void* stream);
int mcq_rans_pack_dev(const uint8_t* scratch, int64_t cap_bytes, const int64_t* sizes, int64_t streams, uint8_t* blob, int64_t blob_bytes,
                      int64_t* offsets, void* stream);
int mcq_rans_decode_dev(const uint8_t* blob, int64_t blob_bytes, const int64_t* offsets, const uint32_t* const* cdf /* [levels] device pointers */,
                        const int32_t* m, const int32_t* k, const int32_t* hw, int32_t levels, int32_t n, int32_t level0, int32_t row_levels,
                        int64_t* const* codes /* [levels] device pointers */, int32_t* status, void* stream);

/* Lane-interleaved streams (additive: ABI 18 stays; csrc/rans_lanes.hip on the device, csrc/rans.cpp on the host): a second, opt-in stream layout whose
 * unit of work is a wave, not a lane.  A stream still codes one (image, level), but carries W in {1, 2, 4, ..., 64} independent rANS
 * states over ONE sequence of 32-bit little-endian words.  Per-state arithmetic is the plain coder's, unchanged.  Within group g, round
 * r = 0 .. ceil(hw / W) - 1 holds positions p = r W + l; lane l is active iff p < hw; the states carry over from group to group and a
 * round never straddles two groups.  As the decoder reads it:
 *   word 0            the prefix 'M' 'Q' 'L' W, i.e. MCQ_RANS_LANES_MAGIC | W << 24
 *   words 1 .. 2 W    the initial states: lane l's x = word[1 + 2 l] | word[2 + 2 l] << 32
 *   then              round by round every active lane decodes its symbol; the active lanes whose new x < L take the next words in
 *                     increasing lane order
 * The encoder is the mirror: groups m - 1 .. 0, rounds last to first, lanes from the highest to the lowest, words written backwards, then
 * the state words, then the prefix; every lane starts at L, and a lane that never codes flushes L.  At W = 1 the stream is the prefix
 * followed by the plain stream, byte for byte.  A stream never exceeds 4 (1 + 2 W + m hw) bytes.
 * `lanes` (per level on the device, per call on the host): 0 = auto, mcq_rans_lanes_auto(m hw) = the largest power of two
 * <= m hw / MCQ_RANS_LANES_AUTO_SYMBOLS, clamped to [1, MCQ_RANS_LANES_MAX] -- the 2 W flush words then cost at most 1/8 bit per symbol --,
 * or one of the seven widths; anything else is MCQ_EINVAL.  The decoders take W from the prefix and from nothing else.
 *   mcq_rans_lanes_encode_dev   as mcq_rans_encode_dev, ONE launch, one wave per stream; the packed blob comes from mcq_rans_pack_dev
 *             unchanged.  cap_bytes: at least 4 (1 + 2 W_l + m_l hw_l) for every level, else MCQ_EINVAL.
 *   mcq_rans_lanes_decode_dev   as mcq_rans_decode_dev, ONE launch, one wave per stream.  Untrusted input: a wrong prefix, a W that is not
 *             one of the seven, fewer than 4 (1 + 2 W) bytes, a length that is not a multiple of 4, running out of words, a bin that does
 *             not contain the state's low 16 bits, offsets outside the blob or decreasing: MCQ_RANS_BAD_STREAM for that stream only, its
 *             outputs zeroed; no content of the blob, the offsets or the prefix leads to a load outside the stream. */
#define MCQ_RANS_LANES_MAX 64
#define MCQ_RANS_LANES_AUTO_SYMBOLS 512
#define MCQ_RANS_LANES_MAGIC 0x4C514D
int mcq_rans_lanes_encode_dev(const int64_t* const* codes /* [levels] device pointers */, const uint32_t* const* cdf /* [levels] device pointers */,
                              const int32_t* m, const int32_t* k, const int32_t* hw, const int32_t* lanes, int32_t levels, int32_t n,
                              int32_t level0, int32_t row_levels, uint8_t* scratch, int64_t cap_bytes, int64_t* sizes, int32_t* status,
                              void* stream);
int mcq_rans_lanes_decode_dev(const uint8_t* blob, int64_t blob_bytes, const int64_t* offsets, const uint32_t* const* cdf /* [levels] device pointers */,
                              const int32_t* m, const int32_t* k, const int32_t* hw, int32_t levels, int32_t n, int32_t level0,
                              int32_t row_levels, int64_t* const* codes /* [levels] device pointers */, int32_t* status, void* stream);

/* Per-step training telemetry kept on the device (csrc/step_meter.hip; host mirror mcquic_amd.monitor.StepMeter): what the
 * reference's trainer reports after an update (mcquic/train/trainer.py:423-441, 463-491) as one float32 row per step in a ring
 * buffer, written by two launches that read every per-step value through a device pointer.  Level tables as for
 * mcq_freq_ema_update_f32 (host arrays of `levels` <= MCQ_VQ_MAX_LEVELS entries); `counts` = this step's global [m_l, k_l] code
 * histograms back to back (int64).
 *   launch 1  one workgroup per (level, group) row; into `workspace` (mcq_step_meter_workspace_bytes(m, k, levels) bytes, 8-byte
 *             aligned: total int64 [rows], used int32 [rows], hit int32 [rows], ema_entropy float [rows], step_bits float [rows]):
 *               used         entries with f / sum f > 1e-6 (strict; the sum and the quotient in double)
 *               ema_entropy  -sum p log2 p of the normalised frequency row (a zero entry contributes 0)
 *               hit          entries with a non-zero count
 *               total        the sum of the row's counts, exact
 *               step_bits    total * (-sum q log2 q), q = count / total; 0 when total == 0, never NaN
 *   launch 2  one wave.  db = -10 log10(loss / upper_bound^2); the shadow (state[2], a float32 in the low word) is set to db while
 *             it is NaN and afterwards shadow -= (1 - momentum) (shadow - db), float32 op by op (validate/utils.py:6-28);
 *             state[1] (first_bad_step, -1 = none) is set to the step number the first time loss or grad_norm is inf / NaN, or the
 *             shadow is NaN or < `floor` (NaN: that test is off); the row goes to ring[count % capacity], count to
 *             steps[count % capacity], and state[0] (count) is advanced.  Row, mcq_step_meter_columns(levels) = 8 + 4 levels floats:
 *               0 loss  1 db  2 shadow  3 grad_norm (NaN if NULL)  4 lr (lr_dev[0], or `lr` by value if NULL: pass NaN for none)
 *               5 skipped (0 if NULL)  6 sum used / sum m_l k_l  7 sum step_bits / pixels
 *               8 + 4 l ..: used_l / (m_l k_l), mean_g ema_entropy, hit_l / (m_l k_l), sum_g step_bits / sum_g total (0 if that is 0)
 * No atomics: equal inputs give equal bits.  Nothing is read by the host. */
size_t mcq_step_meter_workspace_bytes(const int32_t* m, const int32_t* k, int32_t levels);      /* 0 for an invalid table */
int32_t mcq_step_meter_columns(int32_t levels);                                                 /* 0 for levels out of range */
int mcq_step_meter_update_f32(const float* const* freq_ema /* [levels] device pointers */, const int32_t* m, const int32_t* k,
                              int32_t levels, const int64_t* counts, void* workspace, const float* loss, const float* grad_norm /* or NULL */,
                              const float* lr_dev /* or NULL */, double lr, const int64_t* skipped /* or NULL */, double upper_bound,
                              double momentum, double floor, double pixels, int64_t* state /* device [4] */, int64_t* steps /* [capacity] */,
                              float* ring /* [capacity][columns] */, int64_t capacity, void* stream);

/* Per-parameter gradient / weight / update norms kept on the device (csrc/param_stats.hip; host mirror mcquic_amd.monitor.ParamStats).
 * Tables as for mcq_adam_step_f32, pointer rows: 0 param, 1 grad (a NULL entry: a gradient of zeros), 2 shadow (read and written only
 * with `updates`; a flat float32 copy of the weights the caller owns), plus tensor_first_blk[ntensors + 1] as mcq_lamb_step_f32 takes
 * it.  `state` (device int64 [4]): 0 count, advanced by every finish; 1 first_bad_step and 2 first_bad_tensor (-1 = none), set, and then
 * kept, by the first recorded row with a non-finite gradient (the lowest such tensor); 3 rows recorded so far.  A step is SAMPLED when
 * count % every == 0 and RECORDED when it is sampled or skip[0] (a step's guard flag, or NULL) is set; on any other step every workgroup
 * reads the decision and returns, apart from one lane latching it and one lane advancing count.
 *   mcq_param_stats_before_f32   sampled steps: the weights into the shadow (call it in front of the optimizer, only with `updates`)
 *   mcq_param_stats_after_f32    recorded steps: one partial record per chunk into `workspace` (mcq_param_stats_workspace_bytes(nblocks,
 *                                ntensors) bytes, 8-byte aligned; 0 for counts that are not positive), sums of products in double
 *   mcq_param_stats_finish_f32   one workgroup per tensor: row ring[(rows % capacity) * ntensors + t] of mcq_param_stats_columns() = 5 floats
 *                                  0 weight_norm ||w||   1 grad_norm ||g|| over the finite elements   2 grad_absmax over the finite elements
 *                                  3 grad_nonfinite (count of inf / NaN)   4 update_norm ||w - shadow|| (0 in a row recorded only because
 *                                  of `skip`; NaN without `updates`)
 *                                each a double sum's square root rounded to float32 once; steps[rows % capacity] = count; rows and count
 *                                advance.  A tensor without elements: zeros.
 * `every`, `capacity` and `updates` must be the same in the three calls of a step.  No atomics, fixed trees: equal inputs at equal
 * addresses give equal bits.  Nothing is read by the host. */
int32_t mcq_param_stats_columns(void);
size_t mcq_param_stats_workspace_bytes(int32_t nblocks, int32_t ntensors);
int mcq_param_stats_before_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                               int32_t nblocks, const int64_t* state /* device [4] */, int64_t every, void* stream);
int mcq_param_stats_after_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                              int32_t nblocks, const int64_t* state /* device [4] */, int64_t every, int64_t capacity, int32_t updates,
                              const int32_t* skip /* or NULL */, void* workspace, void* stream);
int mcq_param_stats_finish_f32(const int32_t* tensor_first_blk, const int32_t* blk_tensor, int32_t ntensors, int32_t nblocks,
                               const void* workspace, int32_t updates, int64_t* state /* device [4] */, int64_t* steps /* [capacity] */,
                               float* ring /* [capacity][ntensors][5] */, void* stream);

/* The trainer's periodic log payload made on the device (csrc/step_snapshot.hip; host mirror mcquic_amd.monitor.StepSnapshot): what
 * the reference's `MainTrainer.log` (mcquic/train/trainer.py:463-491) builds on the host from whole tensors of the step.  Additions:
 * the ABI number stays.
 *
 * mcq_histogram_f32: np.histogram(v, bins) of n float32 values, v = x (transform 0) or log10f(clamp(-x, min = eps)) (transform 1:
 * `neg`, `clamp(min)` -- a NaN passes through --, `log10`, each rounded to float32), evaluated in registers and never stored.
 * Three launches.  Pass 1: min and max of v over the FINITE entries, a fixed two-stage reduction (equal inputs give equal bits).
 * Pass 2: per-workgroup LDS integer counts, folded into `counts` with integer atomics (exact in any order).  Restated from
 * numpy/lib/_histograms_impl.py (`_get_outer_edges`, `_get_bin_edges`, the uniform-bin fast path of `histogram`), in float64
 * throughout -- what np.histogram returns for the same values widened to float64 (for a float32 ARRAY numpy >= 2 keeps the edges
 * in float32; widened values are the same numbers, the edges then carry float64):
 *   range   (min, max); (0, 1) without a finite value; if min == max: (min - 0.5, max + 0.5)
 *   edges   np.linspace(first, last, bins + 1): i * ((last - first) / bins) + first (i / bins * (last - first) + first if that step is
 *           0), two roundings; the last edge is `last` itself
 *   index   int(((v - first) / (last - first)) * bins), `bins` folded into bins - 1; then one down if v < edges[i], then one up if
 *           v >= edges[i + 1] unless i is the last bin (closed on the right)
 * A non-finite v is counted in stats[1] and left out, where numpy raises ("autodetected range ... is not finite"); stats[0] counts
 * the finite ones (= sum of `counts`).  Where numpy raises "Too many bins for data range" (all values equal and |v| >= 2^53, so
 * that a half does not widen the range) everything lands in bin 0.  1 <= bins <= 4096, n <= 2^40 (MCQ_ETOOLARGE beyond);
 * `workspace`: mcq_histogram_workspace_bytes(n, bins) bytes, 8-byte aligned (0 for arguments the call refuses).  A workgroup takes
 * mcq_histogram_chunk() elements per trip, as float4 loads when x is 16-byte aligned and the chunk is full. */
int32_t mcq_histogram_chunk(void);
size_t mcq_histogram_workspace_bytes(int64_t n, int32_t bins);
int mcq_histogram_f32(const float* x, int64_t n, int32_t transform, float eps, int32_t bins, int64_t* counts /* [bins] */,
                      double* edges /* [bins + 1] */, int64_t* stats /* [2]: finite, non-finite */, void* workspace, void* stream);
/* out[i] = log10f(clamp(-x[i], min = eps)): transform 1 of mcq_histogram_f32, written out. */
int mcq_log_distance_f32(const float* x, float* out, int64_t n, float eps, void* stream);

/* `Validator.visualizeIntermediate` (mcquic/validate/validator.py:30-38) of int64 codes [N, m, h, w] -> uint8 [N, 1, 4h, 4w]:
 * t = (float(c) / float(max) - 0.5f) * 2 with the maximum over the WHOLE tensor (all images, all groups; launch 1, one workgroup,
 * left in maxbuf[0]), DeTransform as mcq_detransform_u8, group 0 only, each value stored to the 4 x 4 block that
 * F.interpolate(scale_factor=4, mode="nearest") fills (launch 2).  A maximum of 0 is 0 / 0 in the reference, a NaN converted to
 * uint8, which is unspecified: 0 is written here.  `out` 4-byte aligned.  mcq_code_image_first_u8 writes the first `keep` <= N
 * images only ([keep, 1, 4h, 4w]); the maximum is still the whole tensor's. */
int mcq_code_image_u8(const int64_t* codes, uint8_t* out, int64_t* maxbuf /* device [1] */, int32_t N, int32_t m, int32_t h, int32_t w,
                      void* stream);
int mcq_code_image_first_u8(const int64_t* codes, uint8_t* out, int64_t* maxbuf /* device [1] */, int32_t N, int32_t m, int32_t h, int32_t w,
                            int32_t keep, void* stream);

/* Group 0 of every level's normalised frequency EMA, f / sum f (`NormalizedFreq[l][0]`, mcquic/modules/entropyCoder.py:46-52), back
 * to back in `out` (sum_l k_l floats), and `Compressor.CodeUsage` in usage[0]: entries of ALL groups with f / sum f > 1e-6 (float32
 * against float32(1e-6), strict) over all entries, divided in float32.  The row sum is formed in double in a fixed order and
 * rounded to float32 once; the quotient is float32.  Level tables as for mcq_step_meter_update_f32; `workspace`:
 * mcq_snapshot_freq_workspace_bytes(m, k, levels) bytes (0 for an invalid table), 4-byte aligned.  Two launches, no atomics. */
size_t mcq_snapshot_freq_workspace_bytes(const int32_t* m, const int32_t* k, int32_t levels);
int mcq_snapshot_freq_f32(const float* const* freq_ema /* [levels] device pointers */, const int32_t* m, const int32_t* k, int32_t levels,
                          float* out, float* usage /* device [1] */, void* workspace, void* stream);

/* Learning-rate schedules stepped on the device (csrc/schedule.hip, the rule itself: csrc/schedule_rule.h; host mirror
 * mcquic_amd.schedule): the reference's four schedulers (mcquic/train/lrSchedulers.py), stepped after every batch
 * (mcquic/train/trainer.py `_stepFinish`), as ONE launch of ONE workgroup with one lane per parameter group, so that a captured
 * training step follows its schedule without the host.  At most MCQ_LR_MAX_GROUPS parameter groups, MCQ_EINVAL beyond.
 * `state` holds MCQ_LR_STATE_WORDS doubles per group -- the float64 state is the truth, the float32 `lr` tensors the optimizers
 * read are only its rounding:
 *   0 rate  1 cycle  2 step_in_cycle  3 cur_cycle_steps  4 max_lr  5 min_lr  6 base_lr  7 min_base_lr
 * (Cosine uses all; Cyclic 0, 1, 4, 6; MultiStep 0, 6; Placeholder 0, 6.  The cycle counters are doubles because the reference's
 * resume path leaves a fractional cycle length behind, first_cycle_steps * cycle_mult^n.)  One step:
 *   e = last_epoch[0] + 1 is stored; per group the state is advanced and `rate` recomputed in the reference's order of operations;
 *   *lr[g] = float(rate).
 *   Placeholder  rate = base_lr
 *   MultiStep    e <= first_milestone: base_lr * (e + 1) / first_milestone (this overshoots at e == first_milestone, and the first
 *                milestone never decays); afterwards rate * gamma where e is one of `milestones` (distinct values), else rate
 *   Cyclic       cycle = floor(1 + e / total_size); x = 1 + e / total_size - cycle; s = x / step_ratio where x <= step_ratio, else
 *                (x - 1) / (step_ratio - 1); rate = base_lr + (max_lr - base_lr) s f, f = 1 (triangular), 1 / 2^(cycle - 1)
 *                (triangular2), gamma^e (exp_range)
 *   Cosine       step_in_cycle += 1; once it reaches cur_cycle_steps: cycle += 1, step_in_cycle -= cur_cycle_steps, cur_cycle_steps =
 *                trunc((cur_cycle_steps - warmup_steps) cycle_mult) + warmup_steps, max_lr = base_lr gamma^cycle, min_lr =
 *                min_base_lr gamma^cycle.  rate = (max_lr - min_lr) step_in_cycle / warmup_steps + min_lr during the warm-up, else
 *                min_lr + (max_lr - min_lr) (1 + cos(pi (step_in_cycle - warmup_steps) / (cur_cycle_steps - warmup_steps))) / 2
 * No atomics, plain vector stores, nothing read by the host: equal state gives equal bits, and the launch is captured like the
 * optimizers' updates.  mcq_lr_schedule_host runs the same rule on HOST memory (`milestones`, `last_epoch`, `state` are host
 * pointers, `lr` an array of ngroups floats or NULL): with `advance` one step as above; without, `rate` (and lr) re-evaluated from
 * the state as it stands and last_epoch left alone -- how a resumed Cosine schedule is set up (MultiStep is a recurrence on the
 * rate and has nothing to re-evaluate: MCQ_EINVAL). */
#define MCQ_LR_MAX_GROUPS   64
#define MCQ_LR_STATE_WORDS  8
#define MCQ_LR_PLACEHOLDER  0
#define MCQ_LR_MULTISTEP    1
#define MCQ_LR_CYCLIC       2
#define MCQ_LR_COSINE       3
#define MCQ_LR_TRIANGULAR   0   /* mcq_lr_schedule.mode (Cyclic) */
#define MCQ_LR_TRIANGULAR2  1
#define MCQ_LR_EXP_RANGE    2
typedef struct mcq_lr_schedule {
    int32_t kind, mode, ngroups, nmilestones;
    const int64_t* milestones;     /* MultiStep: nmilestones distinct values (device memory for the launch); else NULL / 0 */
    double gamma;                  /* MultiStep, Cyclic exp_range, Cosine */
    double first_milestone;        /* MultiStep: min(milestones), >= 1 */
    double total_size, step_ratio; /* Cyclic: step_size_up + step_size_down (> 0), step_size_up / total_size (in (0, 1]) */
    double warmup_steps, cycle_mult; /* Cosine: >= 0 and an integer; > 0 */
} mcq_lr_schedule;
int mcq_lr_schedule_step(const mcq_lr_schedule* rule, int64_t* last_epoch, double* state /* [ngroups][8] */,
                         float* const* lr /* device array of ngroups device pointers */, void* stream);
/* (`skip`: the step's guard flag, see mcq_step_guard_list_f32 -- NULL is mcq_lr_schedule_step; set, the schedule stays where it is) */
int mcq_lr_schedule_step_skip(const mcq_lr_schedule* rule, int64_t* last_epoch, double* state, float* const* lr, const int32_t* skip /* or NULL */,
                              void* stream);
int mcq_lr_schedule_host(const mcq_lr_schedule* rule, int32_t advance, int64_t* last_epoch, double* state, float* lr /* or NULL */);

/* u8 = trunc(clamp(((x + 1) / 2) * 255.999, 0, 255))   (mcquic/utils/vision.py:143-146 DeTransform). */
int mcq_detransform_u8(const float* x, uint8_t* out, int64_t n, void* stream);

/* ---- entropy coder beside the tensor path (host code, no GPU work) ------------------------------ */

/* Up to mcq_pack_conv_weight_max_multi() weights of ONE shape packed in one launch: w[i] -> out[i], forward streams
 * (`dgrad` = 0) or input-gradient streams (`dgrad` = 1, with `stride` and `scale` as in mcq_pack_conv_dgrad_weight_f32).  Layers
 * with <= 16 output channels (they carry a second copy) are refused: pack those one by one.  After an optimizer step every
 * convolution of the network re-packs both streams; this turns 660 launches into ~45. */
int32_t mcq_pack_conv_weight_max_multi(void);
int mcq_pack_conv_weight_multi_f32(const float* const* w, float* const* out, int32_t n, int32_t Cout, int32_t Cin, int32_t ksize,
                                   int32_t dgrad, int32_t stride, float scale, void* stream);
/* The same with a section mask per weight (NULL or 0 = all): bit 0 the 128-row copy of the 3x3 operand stream, bit 1 the 64-row
 * copy, bit 2 the 32-row copy, bit 3 the 16x16-tile order; copies not named are left as they are.  For a re-pack INSIDE a captured
 * training step, whose launches -- and therefore the copies they read -- never change: mcq_conv_section_trace(1) starts recording
 * which copy every conv launch reads per packed buffer (clearing earlier records), (0) stops; mcq_conv_sections_used(packed) =
 * the recorded mask of a buffer (0: not seen).  1x1 weights ignore the mask.  (A training loop's re-pack after optimizer.step():
 * train/trainer.py's step; nothing in the reference corresponds to the mask -- cuDNN keeps no re-laid copies.) */
int mcq_pack_conv_weight_multi_masked_f32(const float* const* w, float* const* out, const uint8_t* masks, int32_t n, int32_t Cout,
                                          int32_t Cin, int32_t ksize, int32_t dgrad, int32_t stride, float scale, void* stream);
void mcq_conv_section_trace(int32_t on);
uint32_t mcq_conv_sections_used(const float* packed);

/* cdf[0..k] (uint32, cdf[0] = 0, cdf[k] = 1 << precision, strictly increasing) from pmf[0..k-1].
 * Same arithmetic as pmfToQuantizedCDF (third_party/CompressAI/cpp_exts/ops.cpp:42-111). */
int mcq_pmf_to_quantized_cdf(const float* pmf, int32_t k, int32_t precision, uint32_t* cdf);

/* One rANS stream over symbols[0..n): symbol i is coded with CDF number indexes[i]; CDF c occupies
 * cdfs[cdf_starts[c] ...] with cdf_lens[c] entries actually present; cdf_sizes[c] follows the reference's convention
 * (sentinel slot = cdf_sizes[c] - 2; the reference's caller passes k + 2 over k + 1 entries,
 * mcquic/modules/entropyCoder.py:121), offsets[c] is subtracted from the symbol.  A symbol whose table slot would lie
 * beyond cdf_lens[c] is MCQ_EINVAL (the reference reads past the table there).  Returns the number of bytes written to
 * `out`, or a negative MCQ_E* (MCQ_ETOOLARGE if `capacity` is too small: 4 * n + 8 always suffices without bypass
 * symbols).  Bit-identical to RansEncoder.encodeWithIndexes (cpp_exts/buffered_rans_encoder.cpp:104-196 over
 * ryg_rans/rans64.h). */
int64_t mcq_rans_encode_with_indexes(const int32_t* symbols, const int32_t* indexes, int64_t n,
                                     const uint32_t* cdfs, const int32_t* cdf_starts, const int32_t* cdf_sizes,
                                     const int32_t* cdf_lens, const int32_t* offsets, int32_t n_cdfs, uint8_t* out, int64_t capacity);

/* Inverse of the above (cpp_exts/rans_decoder.cpp:104-167); MCQ_EINVAL on a truncated / malformed stream. */
int mcq_rans_decode_with_indexes(const uint8_t* in, int64_t nbytes, const int32_t* indexes, int64_t n,
                                 const uint32_t* cdfs, const int32_t* cdf_starts, const int32_t* cdf_sizes,
                                 const int32_t* cdf_lens, const int32_t* offsets, int32_t n_cdfs, int32_t* out_symbols);

/* All images of one level in ONE call (replaces the reference's Python loop `for code in codes: for codePerImage in
 * code: encoder.encodeWithIndexes(...)`, mcquic/modules/entropyCoder.py:108-126): n_streams independent streams of n
 * symbols each (symbols[n_streams][n], one shared `indexes[n]`), stream i written to out + i * stride (stride >= 4 n + 8
 * without bypass symbols) with its length in out_nbytes[i].  Streams are spread over `n_threads` host threads (<= 0: one
 * per hardware thread); the bytes of a stream do not depend on the thread count.  Returns MCQ_OK or the first failing
 * stream's error. */
int mcq_rans_encode_batch_with_indexes(const int32_t* symbols, int64_t n_streams, int64_t n, const int32_t* indexes,
                                       const uint32_t* cdfs, const int32_t* cdf_starts, const int32_t* cdf_sizes,
                                       const int32_t* cdf_lens, const int32_t* offsets, int32_t n_cdfs, uint8_t* out,
                                       int64_t stride, int64_t* out_nbytes, int32_t n_threads);

/* Inverse (entropyCoder.py:141-154): stream i = in[in_offsets[i] .. in_offsets[i + 1]), decoded into out_symbols[i][n]. */
int mcq_rans_decode_batch_with_indexes(const uint8_t* in, const int64_t* in_offsets, int64_t n_streams, const int32_t* indexes,
                                       int64_t n, const uint32_t* cdfs, const int32_t* cdf_starts, const int32_t* cdf_sizes,
                                       const int32_t* cdf_lens, const int32_t* offsets, int32_t n_cdfs, int32_t* out_symbols,
                                       int32_t n_threads);

/* The lanes layout (see mcq_rans_lanes_encode_dev) on the host: n_streams streams of m hw symbols each (symbols[n_streams][m hw], [m, hw]
 * order), coded under `cdfs` uint32 [m, k + 1] with `lanes` states (0 = auto), stream i written to out + i * stride (stride >=
 * 4 (1 + 2 W + m hw) always suffices) with its length in out_nbytes[i]; a symbol outside [0, k) or a bin of width 0 is MCQ_EINVAL.  The
 * inverse reads stream i = in[in_offsets[i] .. in_offsets[i + 1]) of a blob of in_bytes bytes into out_symbols[i][m hw]; a stream it
 * refuses (the list at mcq_rans_lanes_decode_dev) leaves zeros and makes the call return MCQ_EINVAL.  Same thread pool as above. */
int32_t mcq_rans_lanes_auto(int64_t symbols);
int mcq_rans_lanes_encode_batch(const int32_t* symbols, int64_t n_streams, int32_t m, int64_t hw, const uint32_t* cdfs, int32_t k,
                                int32_t lanes, uint8_t* out, int64_t stride, int64_t* out_nbytes, int32_t n_threads);
int mcq_rans_lanes_decode_batch(const uint8_t* in, int64_t in_bytes, const int64_t* in_offsets, int64_t n_streams, int32_t m, int64_t hw,
                                const uint32_t* cdfs, int32_t k, int32_t* out_symbols, int32_t n_threads);

/* ---- validation metrics (callers of the path: mcquic/validate/handlers.py:14-41) --------------------------------
 * MS-SSIM of two uint8 batches x, y [N, C, H, W] as the reference's MsSSIM handler computes it
 * (handlers.py:14-27 -> metrics.py:69-104 `_ssim`, :142-193 `ms_ssim`, module defaults metrics.py:222: 11-tap sigma-1.5
 * window, K = (0.01, 0.03), data range 255, five levels with weights metrics.py:19).  out[N] receives the MS-SSIM VALUE
 * in [0, 1] (the reference module returns 1 - value and the handler prints -10 log10 of that).  H and W must exceed 160
 * (metrics.py:163-166), else MCQ_EINVAL.  `workspace` holds the pooled pyramids and partial sums:
 * mcq_ms_ssim_workspace_bytes(N, C, H, W) bytes (0 for an invalid shape), 8-byte aligned.  Where a call leaves its
 * intermediate results in it is answered by mcq_ms_ssim_workspace_layout below and by nothing else: read no offset that
 * function did not return; anything it does not name is undefined after a call. */
size_t mcq_ms_ssim_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int mcq_ms_ssim_u8(const uint8_t* x, const uint8_t* y, float* out, void* workspace, int32_t N, int32_t C, int32_t H,
                   int32_t W, void* stream);
/* Host helper: the 11 float32 window taps the kernels use (metrics.py:22-37 for size 11, sigma 1.5). */
void mcq_ms_ssim_window(float* out11);

/* The stages of mcq_ms_ssim_u8 on their own, through the launch code mcq_ms_ssim_u8 itself runs (same kernels, same
 * grids): what tests/test_gpu_metrics_leaf.py holds to references stage by stage.  Additive: ABI 18 stays.
 *   mcq_ssim_tiles               host: the map of an H x W level ((H - 10) x (W - 10) positions) is cut into
 *                                tiles_y x tiles_x tiles of 16 x 118 positions; H, W >= 11, else MCQ_EINVAL.
 *   mcq_ssim_level_u8 / _f32     one level: X, Y [planes, H, W]; partial_out [planes][tiles_y * tiles_x][2] float64
 *                                receives per tile (row-major) the sum of the SSIM map and the sum of the
 *                                contrast-structure map over the tile's positions inside the map.  H, W >= 11;
 *                                planes and tiles_y at most 65535, else MCQ_ETOOLARGE.
 *   mcq_ms_ssim_halve_u8 / _f32  one pooling step of both images: Xo, Yo [planes, (H + 1) / 2, (W + 1) / 2] float32.
 *   mcq_ms_ssim_combine_f32      levels [5][N * C][2] float32 ({SSIM mean, CS mean} per level and plane) -> out[N]:
 *                                prod over levels of relu(CS)^w (relu(SSIM)^w on the last), mean over the C channels.
 *   mcq_ms_ssim_workspace_layout host: where a mcq_ms_ssim_u8 call of this shape leaves its intermediate results in
 *                                `workspace`.  out[MCQ_MS_SSIM_LAYOUT_WORDS] int64 (HOST memory): per level l six
 *                                words at out[6 l] -- H, W, tiles_y, tiles_x, and the FLOAT offsets of the pooled x
 *                                and y planes [N * C, H, W] (-1 at level 0, the caller's input) --, then out[30] the
 *                                BYTE offset of the tile partials (those of the last level after a call), out[31]
 *                                the BYTE offset of the float32 level table [5][N * C][2] that
 *                                mcq_ms_ssim_combine_f32 reads, out[32] = mcq_ms_ssim_workspace_bytes.  MCQ_EINVAL
 *                                where that is 0. */
#define MCQ_MS_SSIM_LAYOUT_WORDS 33
int mcq_ssim_tiles(int32_t H, int32_t W, int32_t* tiles_y, int32_t* tiles_x);
int mcq_ssim_level_u8(const uint8_t* X, const uint8_t* Y, int32_t planes, int32_t H, int32_t W, double* partial_out,
                      void* stream);
int mcq_ssim_level_f32(const float* X, const float* Y, int32_t planes, int32_t H, int32_t W, double* partial_out,
                       void* stream);
int mcq_ms_ssim_halve_u8(const uint8_t* X, const uint8_t* Y, float* Xo, float* Yo, int32_t planes, int32_t H, int32_t W,
                         void* stream);
int mcq_ms_ssim_halve_f32(const float* X, const float* Y, float* Xo, float* Yo, int32_t planes, int32_t H, int32_t W,
                          void* stream);
int mcq_ms_ssim_combine_f32(const float* levels, int32_t N, int32_t C, float* out, void* stream);
int mcq_ms_ssim_workspace_layout(int32_t N, int32_t C, int32_t H, int32_t W, int64_t* out);

/* MS-SSIM as a float32 TRAINING LOSS (the distortion of the reference's training configs, `target: MsSSIM`:
 * mcquic/loss/__init__.py:47-55 -> metrics.py:69-104, 142-193 with MsSSIM(data_range=2.0, sizeAverage=True) on restored + 1,
 * image + 1).  a, b [N, C, H, W] float32; X = a + offset, Y = b + offset; C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2;
 * the window, weights, pooling and relu of the metric above.  H and W must exceed 160, else MCQ_EINVAL; N * C <= 65535.
 *   mcq_ms_ssim_loss_f32      loss_out[0] = 1 - mean over (image, channel) of prod_l relu(v_l)^w_l; values_out[5][N][C] = v, the
 *                             per-level means of the cs map (levels 0..3) and of the SSIM map (level 4); `saved` receives the
 *                             pooled X / Y of levels 1..4 (mcq_ms_ssim_loss_saved_bytes bytes), which the backward reads.
 *   mcq_ms_ssim_loss_bwd_f32  da = dloss[0] * d loss / d a from the forward's `values` and `saved` (same a, b, offset, data range);
 *                             db the same for b when non-NULL.  dL/dv_l = -(1 / (N C)) w_l v_l^(w_l - 1) prod_{k != l} relu(v_k)^w_k
 *                             where v_l > 0, else 0 (torch's relu backward); then per level, coarse to fine, the maps' pointwise
 *                             gradients through the transposed blur plus the adjoint of the 2x2 pooling.
 * `workspace`: mcq_ms_ssim_loss_workspace_bytes(N, C, H, W, backward) bytes (backward = 0 for the forward, 1 for the backward;
 * 0 for an invalid shape), 8-byte aligned, contents undefined after.  Caller-owned memory only, no host synchronisation, no
 * memset, no atomics: safe inside a captured hipGraph and bitwise deterministic. */
size_t mcq_ms_ssim_loss_saved_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
size_t mcq_ms_ssim_loss_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t backward);
int mcq_ms_ssim_loss_f32(const float* a, const float* b, float offset, float data_range, float* loss_out, float* values_out,
                         void* saved, void* workspace, int32_t N, int32_t C, int32_t H, int32_t W, void* stream);
int mcq_ms_ssim_loss_bwd_f32(const float* a, const float* b, float offset, float data_range, const float* values,
                             const void* saved, const float* dloss, float* da, float* db /* or NULL */, void* workspace,
                             int32_t N, int32_t C, int32_t H, int32_t W, void* stream);

/* out[n] = sum over the per_image bytes of image n of (x - y)^2, exact (int64).  The reference's PSNR
 * (metrics.py:264-274) is 10 log10(255^2 / (out[n] / per_image + 1e-4)) in float64. */
int mcq_sqdiff_sum_u8(const uint8_t* x, const uint8_t* y, int64_t* out, int64_t per_image, int32_t N, void* stream);

/* F(2x2, 3x3) weights for MCQ_CONV_WINOGRAD2D16: U = G g G^T (float64, rounded once) in the operand order of the 16 x 16 x 4
 * instance, [Cout/32][Cin/4][16 positions][2 halves][64 lanes] + one group of zeros. */
size_t mcq_packed_conv_winograd16_floats(int32_t Cout, int32_t Cin);
int mcq_pack_conv_weight_winograd16_f32(const float* w, int32_t Cout, int32_t Cin, float* out, void* stream);

/* ---- the weight gradients' reduce passes, batched (round 5) ----------------------------------------------------------------------------
 * mcq_wgrad_defer(1): from now on the mcq_conv2d_wgrad*_nchw* entry points record their second pass (the fixed-order sum of the
 * partial tiles in `workspace` -> dW in OIHW order, db) instead of launching it; mcq_wgrad_flush(0, stream) launches everything
 * recorded, 80 convolutions per launch, and empties the record (discard != 0: empties it without launching, after an error).
 * Until the flush the caller keeps every workspace alive and reads no dW / db.  Same sums in the same order as the one-by-one pass.
 * mcq_wgrad_pending(): convolutions recorded and not yet flushed ON THE CALLING THREAD'S CURRENT DEVICE.  The switch is process-wide
 * (the autograd engine records from its own per-device thread): one backward pass at a time uses it; the record is kept per
 * device (ABI 9), a flush launches the current device's jobs on `stream` and a discard empties every device's.
 * The caller also keeps every dW / db alive until the flush (a dropped one would be written over whatever took its memory). */
void mcq_wgrad_defer(int32_t on);
int32_t mcq_wgrad_pending(void);
int mcq_wgrad_flush(int32_t discard, void* stream);

/* ---- GroupNorm (`denseNorm=True`) ------------------------------------------------------------------------------------
 * y = (x - mean) * rstd * gamma[c] + beta[c] over each (image, group) of C / groups adjacent channels, biased variance,
 * rstd = 1 / sqrt(var + eps): nn.GroupNorm(groups, C) as the reference's ResidualBlock inserts it in place of its second
 * activation when denseNorm is set (mcquic/nn/blocks.py:179-200).  gamma / beta may be NULL (1 / 0).  y_silu (NULL = none)
 * receives silu(y).  mean_out / rstd_out [N * groups] (both or neither): what the backward pass needs. */
/* `workspace` (round 5; mcq_group_norm_workspace_floats floats, 0 = none needed, NULL = take the one-workgroup-per-run kernel):
 * planes of 256 pixels and more are cut into 8192-float chunks, one workgroup each, whose three statistics -- the chunk's float32
 * mean m_c, the residue sum (x - m_c) its rounding left, and sum (x - m_c)^2: 3 floats per chunk -- are merged in (plane, chunk)
 * order about one point -- Neon's GroupNorm(32, 32) on 512 x 512 maps is 32 chunks per run instead of one workgroup. */
size_t mcq_group_norm_workspace_floats(int32_t N, int32_t C, int32_t HW, int32_t groups);
int mcq_group_norm_f32(const float* x, const float* gamma, const float* beta, float* y, float* y_silu, float* mean_out,
                       float* rstd_out, float* workspace /* or NULL */, int32_t N, int32_t C, int32_t HW, int32_t groups, float eps,
                       void* stream);
/* Backward of the above: dx [N, C, HW], dgamma / dbeta [C] (NULL = not wanted) from x, dy and the forward's mean / rstd.
 * workspace: mcq_group_norm_bwd_workspace_floats(N, C, HW, groups) floats.  Deterministic (no atomics). */
size_t mcq_group_norm_bwd_workspace_floats(int32_t N, int32_t C, int32_t HW, int32_t groups);
int mcq_group_norm_bwd_f32(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dx,
                           float* dgamma, float* dbeta, float* workspace, int32_t N, int32_t C, int32_t HW, int32_t groups,
                           void* stream);

/* ---- the training input transform (ABI 10) ---------------------------------------------------------------------------------
 * What the reference's loader and trainer run in front of every step (mcquic/data/transforms.py:14-21 getTrainingPreprocess:
 * RandomResizedCrop + RandomGamma; :37-43 getTrainingTransform: RandomPlanckianJitter, the two flips, Normalize(0.5, 0.5);
 * mcquic/train/trainer.py:266) as two launches.  The jitter and the flips are the INTENDED operations (the reference's in-place
 * forms act on copies, mcquic/utils/vision.py:99-104, 167-169, 192-194); with gain 1 and no flip the pass is the reference's
 * effective clamp(x, 0, 1) then (x - 0.5) / 0.5.
 * The decisions of image n are row n of a table [N, MCQ_AUG_COLUMNS] float32: */
#define MCQ_AUG_COLUMNS     16
#define MCQ_AUG_TOP          0   /* crop box inside the source, in pixels: top, left, height, width (clamped into it by the pass) */
#define MCQ_AUG_LEFT         1
#define MCQ_AUG_H            2
#define MCQ_AUG_W            3
#define MCQ_AUG_GAMMA_MODE   4   /* one of MCQ_AUG_GAMMA_* */
#define MCQ_AUG_GAMMA        5   /* the exponent g of MCQ_AUG_GAMMA_POWER */
#define MCQ_AUG_GAIN0        6   /* factor on channel 0 */
#define MCQ_AUG_GAIN2        7   /* factor on channel 2 */
#define MCQ_AUG_HFLIP        8   /* 0 / 1 */
#define MCQ_AUG_VFLIP        9   /* 0 / 1 */
#define MCQ_AUG_GAIN_ROW    10   /* informational: the row of `coeffs` the gains came from, -1 = none drawn */
#define MCQ_AUG_FALLBACK    11   /* informational: 1 = the ten attempts failed and the box is the central crop */
#define MCQ_AUG_OUTPUT      12   /* one of MCQ_AUG_OUT_*: what follows the gains */
                                 /* 13..15: zero */
#define MCQ_AUG_GAMMA_SRGB_TO_LINEAR 0  /* x < 0.0031308 ? 12.92 x : 1.055 |x|^(1/2.4) - 0.055   (vision.py:108-109, its naming) */
#define MCQ_AUG_GAMMA_LINEAR_TO_SRGB 1  /* x < 0.04045 ? x / 12.92 : (|x + 0.055| / 1.055)^2.4     (vision.py:111-112)            */
#define MCQ_AUG_GAMMA_POWER          2  /* clamp(clamp(x, 0)^g, 0, 1)                              (vision.py:114-116)            */
#define MCQ_AUG_GAMMA_IDENTITY       3
#define MCQ_AUG_OUT_NORMALIZED 0  /* clamp to [0, 1], then (v - 0.5) / 0.5: the whole pipeline, or its second half            */
#define MCQ_AUG_OUT_CLAMPED    1  /* clamp to [0, 1] only (RandomPlanckianJitter on its own, vision.py:104)                    */
#define MCQ_AUG_OUT_RAW        2  /* neither (the loader's half -- crop, gamma -- and a flip on its own: values pass unchanged) */
/* mcq_augment_draw: fills `params` for N images of a [Hs, Ws] source from rng_state = {seed, offset} (device memory) and advances
 * the offset by one, in stream order: a captured launch draws a fresh table on every replay.
 *   crop != 0   torchvision's RandomResizedCrop box rule: up to 10 attempts of area = Hs Ws U(scale), log r ~ U(log ratio),
 *               w = round(sqrt(area r)), h = round(sqrt(area / r)), accepted if it fits, then top / left uniform; after 10
 *               failures the central crop with the aspect clamped into `ratio`.  Otherwise the box is the whole source.
 *   gamma != 0  one of the four modes uniformly, g ~ U(0.05, 2.0) for MCQ_AUG_GAMMA_POWER.  Otherwise identity.
 *   coeffs      [T, 2] gains or NULL: with probability p_gain one row, uniformly.  Otherwise gains of 1.
 *   p_hflip / p_vflip   probability of each flip.
 *   output      MCQ_AUG_OUT_*, copied into every row.
 * mcq_augment_f32 / _u8: out[N, 3, H, W] float32 from src[N, 3, Hs, Ws] (float32 in [0, 1]; uint8 read as v / 255) under `params`:
 * the box resampled to [H, W] like F.interpolate(mode="bilinear", antialias=True, align_corners=False) on the crop, then gamma,
 * gains, clamp to [0, 1] and (v - 0.5) / 0.5 (as MCQ_AUG_OUTPUT says), with the flips as an index map on the output.  MCQ_ETOOLARGE: more than 65535 images, a
 * side above 2^24, or a source more than ~30x the output along an axis. */
int mcq_augment_draw(uint64_t* rng_state, float* params, int32_t N, int32_t Hs, int32_t Ws, int32_t crop, double scale_lo,
                     double scale_hi, double ratio_lo, double ratio_hi, int32_t gamma, const float* coeffs /* or NULL */, int32_t T,
                     float p_gain, float p_hflip, float p_vflip, int32_t output, void* stream);
int mcq_augment_f32(const float* src, const float* params, float* out, int32_t N, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                    void* stream);
int mcq_augment_u8(const uint8_t* src, const float* params, float* out, int32_t N, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                   void* stream);

/* Library / build identification: returns a static string "mcquic_hip <ver> gfx950". */
/* Launches a kernel with an invalid configuration on purpose and returns what every entry point returns when its launch is
 * refused: MCQ_ELAUNCH.  Test hook for the error path (tests/test_gpu_ops.py); harmless (launch errors are not sticky). */
int mcq_selftest_launch_failure(void* stream);

const char* mcq_version(void);
/* MCQ_ABI_VERSION the library was built from. */
int32_t mcq_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MCQUIC_HIP_H */
