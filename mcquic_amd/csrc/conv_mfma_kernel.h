// Dense 3x3 / 1x1 convolution for gfx950 as an implicit GEMM on exact-f32 MFMA.
//
// Replaces nn.Conv2d / F.conv2d under McQuic's conv3x3, conv1x1, pixelShuffle3x3 and GenDivNorm
// (reference: mcquic/nn/convs.py:77-100,221-276, mcquic/nn/gdn.py:67-91) plus the element-wise
// ops the reference runs around them (SiLU, `out += identity`, x*rsqrt(std), a*sigmoid(b)+x;
// mcquic/nn/blocks.py:70-78,281-288).
//
// GEMM view:  D[co][p] = sum_{tap, ci} Wt[co][tap, ci] * X[ci][p + tap]
//   rows  = output channels  (A operand = packed weights, one float4 per lane per k-step)
//   cols  = output pixels    (B operand = activations, NCHW so 32 pixels = 32 consecutive floats)
//   k     = (ci pair, tap) walked channel-major / tap-inner (two input channels per 32x32x2 MFMA): the nine taps
//           of a channel pair re-read the same rows back to back, so they hit L1 instead of being nine separate
//           sweeps over the whole activation (tap-major measured 2.4-4.8x the algorithmic bytes at the L2 fabric).
// A wave owns MB x NB accumulator tiles of 32 couts x 32 pixels and is a self-contained stream:
// per k-step it issues one weight load (MB floats per lane, from the copy packed for its tile height) and NB
// activation loads (buffer loads; out-of-image taps are turned into out-of-range offsets, for which the hardware
// returns 0 = the conv's zero padding), 9 resp. 18 k-steps ahead of the MFMAs that consume them.  Small layers split
// the k-steps of a tile over 2 / 4 / 8 waves of a workgroup (LDS reduction); the epilogue (bias, GDN / IGDN, gate,
// residual, SiLU, SiLU twin, PixelShuffle store) runs on buffer instructions without predication.
// Build switches below (all measured on MI355X): ring depths, XCD-aware tile order, tile rules.
#pragma once
#include <type_traits>

#include "mcq_common.h"
#include "../../include/mcquic_hip.h"

// (The ablation / stamp / packed-SiLU / peel build switches of rounds 1-2 are gone from this file: what they measured is in
//  DESIGN.md section 4, the code in the history up to commit 0aa82a9.)
// 3x3 ring depths in k-steps (weights / activations).  Activations 18 steps = two channel pairs ahead.
#ifndef MCQ_PF42A
#define MCQ_PF42A 9
#endif
#ifndef MCQ_PF42B
#define MCQ_PF42B 18
#endif
#ifndef MCQ_PFB
#define MCQ_PFB 18
#endif
// (measured and dropped, round 3: deeper rings -- 18 / 36 and 36 / 36 steps -- for the 32 x 32 tile of the smallest maps, where a
//  wave's share of a split 128-channel 3x3 layer is 72 steps: kernel durations unchanged in isolation (10.2-10.8 us), the training
//  step 24.1 -> 24.2 ms.  tools/probes/pf11_sweep.sh)
#ifndef MCQ_WINO_PERSIST
#define MCQ_WINO_PERSIST 1          // workgroups per CU of the persistent 128-row Winograd instance; 0 = one workgroup per four tiles
#endif
// SiLU of the band epilogue two values at a time on packed fp32 instructions (mcq_silu2: bit-identical results, 15 issue
// slots per pair instead of 24).  Measured on the direct kernel: 253.2 vs 256.2 images/s (same box, alternating runs) -- the
// packed forms cost the co-resident wave's MFMA stream MORE than the scalar ones they replace: off.
#ifndef MCQ_WINO_PFB2
#define MCQ_WINO_PFB2 48
#endif
#ifndef MCQ_CONV_MAX_MULTI
#define MCQ_CONV_MAX_MULTI 4
#endif
// (round 6, built and dropped: conv_c32_kernel, a persistent kernel for Neon's 32 -> 32 layers with the whole filter bank in registers
//  and the input patch double-buffered in LDS by DMA -- bit-identical to the 32 x 32 tile below, and no faster: 185 / 192 / 260 us on
//  4 x 32 x 512x512 plain / SiLU / residual + twin against 181 / 189 / 230 here.  Source and test last in tree at bca81ee; counters:
//  docs/experiments.md section 11.3)

// (ConvPtrs / ConvK are the argument of the launch functions of conv_instances.h, which are defined in one file and called
//  from another: they are the only names of this header outside the anonymous namespace)

// tensors of one convolution; a launch can carry up to MCQ_CONV_MAX_MULTI independent convolutions of ONE geometry and flag
// set (blockIdx.z picks the problem): the two stacks of an AttentionBlock run the same layer shapes side by side, and on the
// 16x16 ... 4x4 maps of a training crop (or at batch 1) a launch is latency, not work
struct ConvPtrs {
    const float* x; const float* wp; const float* wp64; const float* wp32; const float* bias; float* y; float* y2;
    const float* res; const float* mul; const float* gid;
};

struct ConvK {
    const float* x; const float* wp; const float* wp64; const float* wp32; const float* bias; float* y; float* y2;
    const float* res; const float* mul; const float* gid;
    ConvPtrs alt[MCQ_CONV_MAX_MULTI - 1];      // problems 1 .. nprob - 1
    int nprob;
    int N, Cin, H, W, Cout, Ho, Wo;
    int ks, stride;
    int S;             // input-channel pairs (padded to a multiple of 16 for 1x1 convs)
    int TP;            // k-steps per 128-cout tile = S * taps
    int bw_log2;       // a pixel block is (32 >> bw_log2) rows x (1 << bw_log2) cols
    int nbx, nby, total_blocks;
    int ks_log2;       // split-K: 1 << ks_log2 waves of a workgroup share one output tile, each a slice of the k-steps
    int slice_pairs;   // channel pairs per split-K slice
    int tiles_log2;    // (1 << tiles_log2) output tiles per workgroup
    int total_wgs;     // (persistent Winograd instance) workgroups' worth of tiles along x; the grid may be smaller
    unsigned flags; float res_scale;
    const float* post_w; const float* post_b;   // MCQ_CONV_POST_*: the following 1x1 layer (accumulator-order operand stream, bias)
    int post_sub;      // MCQ_CONV_POST_IGDN through the PixelShuffle store: the four waves of a workgroup are the four sub-pixel row tiles of ONE pixel tile
};

namespace {

constexpr int PRO_NONE = 0, PRO_SILU = 1, PRO_SQUARE = 2;
// 128-row Winograd instance: the epilogue flag set instance `id` (the kernel's PRO slot) is compiled for; 0 = any (run-time flags)
constexpr unsigned wino_epilogue_flags(int id) {
    return id == 1 ? 0u : id == 2 ? MCQ_CONV_SILU_OUT : id == 3 ? MCQ_CONV_RESIDUAL : id == 4 ? (MCQ_CONV_RESIDUAL | MCQ_CONV_DUAL_SILU)
         : id == 5 ? MCQ_CONV_DUAL_SILU : id == 6 ? (MCQ_CONV_RESIDUAL | MCQ_CONV_SILU_OUT) : 0xffffffffu;
}
constexpr unsigned RUNTIME_FLAGS = 0xffffffffu;    // epilogue instance that tests the flags at run time

template <int MB> struct AVec;
template <> struct AVec<4> { typedef f32x4v T; };
template <> struct AVec<2> { typedef f32x2v T; };
template <> struct AVec<1> { typedef float T; };

template <int MB> __device__ __forceinline__ float a_elem(const typename AVec<MB>::T& v, int i) { return v[i]; }
template <> __device__ __forceinline__ float a_elem<1>(const float& v, int) { return v; }

extern __shared__ __attribute__((aligned(16))) float mcq_lds[];

#define MCQ_CLOBBER_ALL_AGPRS() asm volatile("" ::: "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255")

// weight-ring load: 4 * MB bytes per lane from a buffer descriptor, per-lane byte offset + wave-uniform byte offset
template <int MB> __device__ __forceinline__ typename AVec<MB>::T mcq_wload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff);
template <> __device__ __forceinline__ f32x4v mcq_wload<4>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
template <> __device__ __forceinline__ f32x2v mcq_wload<2>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
}
template <> __device__ __forceinline__ float mcq_wload<1>(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}


constexpr int POST_STEPS = 64;          // k-steps of the fused 1x1 layer: 128 channels, two per step
constexpr int POST_TAIL = 8;            // zero steps behind them (the weight ring's over-read)
constexpr int POST_PF = 4;              // its weight ring, in k-steps (a step is four MFMAs = 256 cycles; the stream is L2-resident)

// POST (round 6): 0 = none; 1 = GDN / IGDN, 2 = AttentionBlock gate -- the 1x1 layer behind this 3x3 convolution inside the same launch
// (MCQ_CONV_POST_*), see the section behind the k-loop
template <int MB, int NB, int PRO, int PFA, int PFB, int TAPS, int OCC, bool PAIR = false, int POST = 0>
__global__ __launch_bounds__(TAPS >= 12 ? 256 : 512, OCC) void conv_mfma_kernel(ConvK p) {
    // (NB == 1: with two pixel blocks the 128 + 64 accumulators left the compiler 50-80 spilled registers -- outside the k-loop, but a
    //  kernel with scratch ran 0.4-0.6 % slower IN the 32-image step than the two-launch form it replaces, profiles/r06_post_ab.txt)
    static_assert(POST == 0 || (MB == 4 && TAPS == 9 && !PAIR && NB == 1), "the fused 1x1 layer needs all 128 channels of a pixel in one wave");
    static_assert(TAPS == 1 ? PFA == PFB : ((TAPS % PFA == 0 || PFA % TAPS == 0) && PFB % TAPS == 0 && PFB % PFA == 0),
                  "ring depths must tile the unrolled body");
    // TAPS == 12: the Winograd F(2, 3) form of a 3x3 stride-1 convolution along x (opt-in, MCQ_CONV_WINOGRAD).  A lane owns a
    // PAIR of horizontally adjacent output pixels; per channel pair and filter row it loads the four inputs d0..d3 under the
    // pair (x = 2 xp - 1 .. 2 xp + 2), forms (d0 - d2, d1 + d2, d2 - d1, d1 - d3) and feeds them to four k-steps whose weights
    // are the transformed filter row (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2): 12 k-steps per channel pair instead of
    // 18 for the two pixels, accumulated per transform position (4 x MB tiles) and folded back to the two pixels
    // (M0 + M1 + M2, M1 - M2 - M3) in front of the unchanged epilogue, which sees them as NB = 2 pixel blocks.
    // TAPS == 16: F(2x2, 3x3), the same idea in both directions.  A lane owns a 2 x 2 tile of output pixels; per channel pair it
    // loads the 4 x 4 inputs under the tile, forms B^T d B (32 additions, one group ahead) and feeds the sixteen results to sixteen
    // k-steps whose weights are G g G^T: 16 MFMA k-steps per channel pair for FOUR pixels (36 in the direct form, 24 in the 1-D
    // form).  Sixteen accumulator tiles per 32-row band: the instance takes ONE band per wave (MB = 1; the four waves of a
    // workgroup are the four bands of 128 output channels over the same tiles, so the input patches hit L1 three times out of
    // four), accumulators again in hand-numbered AGPRs; the epilogue sees NB = 4 pixel blocks (oy, ox).
    // PAIR (round 5; direct 3x3 stride 1, NB = 2): the two pixel blocks of a wave are the EVEN and the ODD pixels of 32 horizontally
    // adjacent pairs (the Winograd form's geometry without its arithmetic).  Per channel pair and filter row a lane loads the four
    // inputs under its pair once (x = 2 xp - 1 .. 2 xp + 2) and feeds them to the six (tap, pixel) MFMA groups that read them -- 12
    // activation loads per channel pair instead of 18 -- and every output-shaped access of the epilogue is one 64-bit access per row
    // for both pixels (even widths) instead of two 32-bit ones.
    static_assert(!PAIR || (TAPS == 9 && NB == 2 && PRO == 0 && PFB % 9 == 0), "PAIR: the direct 3x3 form with two pixel blocks");
    // TAPS == 4 (round 5): a 3x3 stride-1 layer whose filter is zero outside its lower-right 2 x 2 taps (MCQ_CONV_TAPS_LR: the
    // input-gradient convolution of a stride-2 layer, [4 Cin, Cout, 3, 3] through the PixelShuffle store -- output pixel 2 q + i
    // reads dY[q] and, for i = 1, dY[q + 1]: rows / columns -1 of the window never).  The operand stream stays the dense 9-tap one;
    // the k-loop walks taps 4, 5, 7, 8 of every channel pair only: 4 / 9 of the MFMAs and activation loads, the same sums.
    constexpr bool LR4 = TAPS == 4;
    constexpr int WT = LR4 ? 9 : TAPS;              // k-steps per channel pair in the packed weights
    constexpr bool W2D = TAPS == 16;
    constexpr bool WINO = TAPS == 12 || W2D;
    constexpr int PG = W2D ? 16 : 4;                // transform positions = k-steps per group of operand loads
    static_assert(!WINO || NB == (W2D ? 4 : 2), "the Winograd forms have two / four virtual pixel blocks");
    static_assert(!W2D || MB == 1, "the 2-D form takes one 32-row band per wave");
    // (the Winograd form has no input prologue; its 128-row instance reuses the PRO slot of the template for the flag set its
    //  epilogue is compiled for -- one set per kernel instance: dispatching on the flags inside the persistent tile loop left
    //  every instance's temporaries live around the loop and pushed the compiler into the AGPRs)
    constexpr unsigned WEF = wino_epilogue_flags(PRO);
    constexpr int NBG = (WINO || PAIR) ? 1 : NB;    // pixel blocks the operand stream walks (pair blocks for WINO / PAIR)
    constexpr int LT = PAIR ? 12 : TAPS;            // activation loads per channel pair and pixel block
    constexpr int NACC = WINO ? PG : NB;            // accumulator tiles per 32-row band
    // The 128-row Winograd instance has 4 x 4 accumulator tiles = 256 registers: the whole AGPR half of a one-wave-per-SIMD
    // register file.  hipcc's allocator cannot work with that (it parks other values in AGPRs that do not exist and splits
    // every tuple into VGPRs at the loop exit: 130-345 spilled dwords, scratch traffic inside the k-loop), so this instance
    // keeps its accumulators out of the compiler's sight: tile (band mb, position t) IS a[16 (4 mb + t) : +15], written only
    // by the inline-asm MFMAs below and read back element by element in the epilogue.  The compiler's own code stays within
    // the VGPR half (tests/test_host_abi.py checks the disassembly: no AGPR operand outside these instructions).
    constexpr bool WASM = WINO && MB * PG == 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // this workgroup's problem (scalar selects; one problem per launch is the common case)
    const float* P_x = p.x; const float* P_wp = p.wp; const float* P_wp64 = p.wp64; const float* P_wp32 = p.wp32;
    const float* P_bias = p.bias; float* P_y = p.y; float* P_y2 = p.y2;
    const float* P_res = p.res; const float* P_mul = p.mul; const float* P_gid = p.gid;
    if (p.nprob > 1) {
#pragma unroll
        for (int c = 1; c < MCQ_CONV_MAX_MULTI; ++c)
            if ((int)blockIdx.z == c) {
                const ConvPtrs& a = p.alt[c - 1];
                P_x = a.x; P_wp = a.wp; P_wp64 = a.wp64; P_wp32 = a.wp32; P_bias = a.bias; P_y = a.y; P_y2 = a.y2;
                P_res = a.res; P_mul = a.mul; P_gid = a.gid;
            }
    }
    const int KS = 1 << p.ks_log2;
    const bool post_sub = POST == 1 && p.post_sub;  // (wave-uniform) the workgroup's waves are the four sub-pixel row tiles of one pixel tile
    const int tile_in_wg = (W2D || post_sub) ? 0 : wave >> p.ks_log2;       // which output tile of this workgroup (W2D: all waves share it)
    const int kslice = wave & (KS - 1);             // which slice of the k-steps
    // XCD-aware tile order: the dispatcher deals workgroups round-robin to the 8 XCDs (linear id % 8), each with its own
    // L2.  Taking the id as is, vertically adjacent pixel rows -- which share two of their three input rows -- always sit
    // on different XCDs and every XCD pulls the halo rows through the fabric again (FETCH_SIZE 3.1x the input on the
    // 384x256 level).  Remapped, XCD k walks the contiguous k-th eighth of the tiles, so the halo of one workgroup is the
    // row its own XCD touched a moment ago.
    // The 128-row Winograd instance is PERSISTENT: one workgroup per CU (it fills the register file) walks the tiles
    // vwg, vwg + gridDim.x, ... -- no kernel-argument fetch, dispatch gap and first-wave ramp per tile (~3 us of a ~95 us tile).
    unsigned vwg = blockIdx.x;
next_tile:
    // (everything below is recomputed per tile on the scalar unit: hoisted out of the tile loop, the ~100 wave-uniform offsets of
    //  prologue and epilogue would not fit the SGPR file and come back as VGPR spills -- `tile_zero` keeps them loop-variant)
    int tile_zero = 0;
    if (WASM) asm volatile("" : "+s"(tile_zero));
    unsigned wg = vwg;
    {
        const unsigned nwg = WASM ? (unsigned)p.total_wgs : gridDim.x, xcd = wg & 7u, slot = wg >> 3;   // (WASM: gridDim.x % 8 == 0)
        const unsigned base = xcd * (nwg >> 3) + (xcd < (nwg & 7u) ? xcd : (nwg & 7u));      // workgroups of the XCDs before this one
        wg = base + slot;
    }
    const int gw = (int)(wg << p.tiles_log2) + tile_in_wg;       // tile index along the pixel-block axis
    const bool active = gw * NBG < p.total_blocks;  // wave-uniform
    if (KS == 1 && !active) return;                 // (split-K waves stay for the barriers)
    const int co_base = (W2D ? ((int)blockIdx.y * 4 + wave) * 32 : post_sub ? wave * 128 : (int)blockIdx.y * (32 * MB)) + tile_zero;     // first output channel of this wave
    const int hi = lane >> 5, j = lane & 31;
    const int BW = 1 << p.bw_log2;
    const int ly = j >> p.bw_log2, lx = j & (BW - 1);
    const int BH = 32 >> p.bw_log2;
    const int HW = p.H * p.W + tile_zero;
    const int pad = (TAPS == 1 || LR4) ? 0 : 1;
    const unsigned plane_bytes = (unsigned)p.Cin * (unsigned)HW * 4u;

    // ---- geometry of the NB pixel blocks this wave owns -------------------------------------
    int img[NB], yo[NB], xo[NB];
    bool valid[NB];
    __amdgpu_buffer_rsrc_t rsrc[NB];
    const char* xb[NB];                             // (wave-uniform) first byte of the block's image
    unsigned voff[NBG][LT];                       // per-tap byte offset of this lane's pixel, or the OOB marker
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        int pb = (WINO || PAIR) ? gw : gw * NB + nb;
        const bool pbv = pb < p.total_blocks;
        if (!pbv) pb = p.total_blocks - 1;
        const int per_img = p.nby * p.nbx;
        const int n = pb / per_img;
        const int rem = pb - n * per_img;
        const int by = rem / p.nbx;
        const int bx = rem - by * p.nbx;
        img[nb] = n;
        yo[nb] = W2D ? 2 * (by * BH + ly) + (nb >> 1) : by * BH + ly;
        xo[nb] = W2D ? 2 * (bx * BW + lx) + (nb & 1) : (WINO || PAIR) ? 2 * (bx * BW + lx) + nb : bx * BW + lx;
        valid[nb] = pbv && yo[nb] < p.Ho && xo[nb] < p.Wo;
        xb[nb] = reinterpret_cast<const char*>(mcq_uniform_ptr(P_x + (size_t)n * p.Cin * HW));
        rsrc[nb] = mcq_make_rsrc(xb[nb], plane_bytes);
        if ((WINO || PAIR) && nb > 0) continue;
#pragma unroll
        for (int tap = 0; tap < LT; ++tap) {
            // (WINO / PAIR: tap = 4 dy + position under the pair, x = 2 xp - 1 + position)
            const int dy = PAIR ? tap / 4 : TAPS == 9 ? tap / 3 : WINO ? tap / 4 : LR4 ? tap / 2 : 0,
                      dx = PAIR ? tap % 4 : TAPS == 9 ? tap % 3 : WINO ? tap % 4 : LR4 ? tap % 2 : 0;
            const int yi = yo[nb] * p.stride + dy - pad;
            const int xi = xo[nb] * p.stride + dx - pad;
            const bool inb = valid[nb] && yi >= 0 && yi < p.H && xi >= 0 && xi < p.W;
            voff[(WINO || PAIR) ? 0 : nb][tap] = inb ? (unsigned)(yi * p.W + xi + hi * HW) * 4u : MCQ_OOB;
        }
    }

    // ---- operand prefetch rings -------------------------------------------------------------
    // A k-step is (channel pair s, tap).  Weights (L2 resident, shared by every wave of the launch) run PFA steps
    // ahead of the MFMAs that consume them; activations, whose first touch of a row comes from HBM / MALL
    // (~2.5 us under load, i.e. more than the nine steps of one channel pair), run PFB steps ahead.  The loop body
    // covers U consecutive steps so that every ring slot, tap and look-ahead distance is a compile-time constant.
    constexpr int U = TAPS != 1 ? PFB : PFA;        // 3x3: one or two channel pairs; 1x1: PFA pairs
    constexpr int PAIRS_PER_ITER = TAPS != 1 ? U / TAPS : U;
    typedef typename AVec<MB>::T avec_t;
    avec_t A[PFA];
    constexpr int BSLOTS = PAIR ? PFB / 9 * 12 : PFB;     // (PAIR: the ring holds loads, 12 per channel pair, not k-steps)
    float B[BSLOTS][NBG];
    const int tile128 = co_base >> 7, q0 = (co_base & 127) >> 5;
    const int s0 = kslice * p.slice_pairs;          // first channel pair of this wave's slice
    // weights: the copy packed for this tile height, so that a wave-wide load is one dense run of 64 * MB floats
    // (reading the 32- / 64-row tiles out of the 128-row copy -- 4 / 8 bytes per lane at a 16-byte stride -- touched
    // four / two times the cache lines and made a 12x8-level launch 30 instead of 21 us)
    // -- as a wave-uniform base plus a constant per-lane offset, read through a buffer load whose running offset is
    // the scalar soffset (no per-lane pointer arithmetic in the k-loop)
    const float* wbu = MB == 4 ? P_wp + ((size_t)tile128 * p.TP + (size_t)s0 * WT) * 256 + q0
                     : MB == 2 ? P_wp64 + ((size_t)(co_base >> 6) * p.TP + (size_t)s0 * WT) * 128
                               : P_wp32 + ((size_t)(co_base >> 5) * p.TP + (size_t)s0 * WT) * 64;
    const __amdgpu_buffer_rsrc_t wr = mcq_make_rsrc(wbu, 0x7fffffffu);   // (the packed copies end in a zero tail: over-reads are in bounds)
    const unsigned wlane = (unsigned)lane * (unsigned)(4 * MB);
    // (LR4: the live taps of a channel pair are steps 4, 5, 7, 8 of its nine -- the distance to the next live step by position)
    auto winc = [](const int live_step) constexpr -> unsigned {
        return !LR4 ? 1u : (live_step & 3) == 0 ? 1u : (live_step & 3) == 1 ? 2u : (live_step & 3) == 2 ? 1u : 5u;
    };
    unsigned wso = LR4 ? 4u * 256u * MB : 0u;
    const unsigned step_bytes = 2u * (unsigned)HW * 4u;     // one channel pair further
    unsigned soff = (unsigned)s0 * step_bytes;

    f32x16 acc[MB][NACC];                           // (unused by the WASM instance)
    if (WASM) {
        MCQ_CLOBBER_ALL_AGPRS();                    // (tells hipcc the kernel uses a0 .. a255; nothing is emitted)
#pragma unroll
        for (int i = 0; i < 256; ++i) asm volatile("v_accvgpr_write_b32 a[%0], 0" :: "n"(i));
        asm volatile("s_nop 7");
    } else {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NACC; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.0f;
    }

    const int npairs = active ? p.slice_pairs : 0;
    if constexpr (W2D) {
        // ---- F(2x2, 3x3) k-loop ---------------------------------------------------------------------------------------------
        // The four waves of the workgroup are the four 32-row bands over the SAME 32 tiles, so they share the input transform
        // through LDS: wave w loads row w of every lane's 4 x 4 patch (4 loads per channel pair instead of 16 -- with each wave
        // loading whole patches the launch was bound by L1 throughput: 155 -> 246 "TFLOP/s" without those loads), transforms it
        // along x and parks the four values in LDS; after ONE workgroup barrier per channel pair (two buffers) every wave reads
        // the four rows back and transforms along y.  All of it one group ahead of the MFMAs that use it.
        constexpr int GA = 4;                               // channel pairs the row loads run ahead = groups per loop body
        unsigned vrow[4];
        {
            const int yi = yo[0] + wave - 1;
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const int xi = xo[0] - 1 + px;
                const bool inb = valid[0] && yi >= 0 && yi < p.H && xi >= 0 && xi < p.W;
                vrow[px] = inb ? (unsigned)(yi * p.W + xi + hi * HW) * 4u : MCQ_OOB;
            }
        }
        float Bw[GA][4];
        f32x4v* const tl = reinterpret_cast<f32x4v*>(mcq_lds);          // [2 buffers][4 patch rows][64 lanes]
        if (active) {
#pragma unroll
            for (int st = 0; st < PFA; ++st) { A[st] = mcq_wload<MB>(wr, wlane, wso); wso += 256 * MB; }
#pragma unroll
            for (int g = 0; g < GA; ++g)
#pragma unroll
                for (int px = 0; px < 4; ++px) Bw[g][px] = mcq_buffer_load(rsrc[0], vrow[px] + soff + (unsigned)g * step_bytes);
        }
        auto row_to_lds = [&](const int slot, const int buf) __attribute__((always_inline)) {
            const float d0 = Bw[slot][0], d1 = Bw[slot][1], d2 = Bw[slot][2], d3 = Bw[slot][3];
            tl[(buf * 4 + wave) * 64 + lane] = f32x4v{d0 - d2, d1 + d2, d2 - d1, d1 - d3};
        };
        auto lds_rows = [&](const int buf, f32x4v (&t)[4]) __attribute__((always_inline)) {
#pragma unroll
            for (int py = 0; py < 4; ++py) t[py] = tl[(buf * 4 + py) * 64 + lane];
        };
        auto rows_to_v = [&](const f32x4v (&t)[4], float (&out)[16]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                out[j] = t[0][j] - t[2][j]; out[4 + j] = t[1][j] + t[2][j]; out[8 + j] = t[2][j] - t[1][j]; out[12 + j] = t[1][j] - t[3][j];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(out[i]));      // (opaque: never re-formed in front of an MFMA)
        };
        // the workgroup barrier WITHOUT the fence of __syncthreads(): that one waits for every outstanding vector load,
        // i.e. it would drain the prefetch rings once per channel pair
        auto wg_barrier = [&]() __attribute__((always_inline)) { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
        float Vn[16];
        f32x4v tq[4];
        row_to_lds(0, 0);
        wg_barrier();
        lds_rows(0, tq);
        rows_to_v(tq, Vn);
        // The first body is peeled off the loop: hipcc's wait-count pass merges the loop-entry state (operands requested by the
        // preload above, back to back) with the back-edge state (requested one body ago, 80 loads apart) and would wait at every
        // use as if the loads had only just been issued -- draining the rings once per channel pair (55 instead of 155 "TFLOP/s").
        auto body = [&](const int sp) __attribute__((always_inline)) {
            __amdgpu_buffer_rsrc_t rB[GA];
#pragma unroll
            for (int j = 0; j < GA; ++j) {
                const unsigned off = soff + (unsigned)(GA + j) * step_bytes;
                const int left = (int)plane_bytes - (int)off;
                rB[j] = mcq_make_rsrc(xb[0] + off, (unsigned)(left > 0 ? left : 0));
            }
            float V[16];
#pragma unroll
            for (int u = 0; u < GA * 16; ++u) {
                const int k = u / 16, st = u % 16;
                // (no early exit: the launcher only takes layers whose channel pairs fill whole bodies, Cin % 8 == 0 -- a branch
                //  per step makes every step its own basic block, 86 instead of 155 "TFLOP/s", and a `break` around the barrier
                //  keeps the loop from unrolling at all)
                if (st == 0) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) V[i] = Vn[i];
                }
                // the next group's transform, spread over this group's steps so that neither the barrier (by step 6 every wave has
                // long written its row) nor the LDS round trip stalls the MFMA stream: in-order issue stops at a wait
                if (st == 1) row_to_lds((k + 1) % GA, (k + 1) & 1);
                if (st == 6) { wg_barrier(); lds_rows((k + 1) & 1, tq); }
                if (st == 11) rows_to_v(tq, Vn);
                asm volatile("v_mfma_f32_32x32x2_f32 a[%2:%3], %0, %1, a[%2:%3]"
                             :: "v"(a_elem<MB>(A[st], 0)), "v"(V[st]), "n"(16 * st), "n"(16 * st + 15));
                if (st < 4) Bw[k][st] = mcq_buffer_load(rB[k], vrow[st]);         // my row of the pair GA groups ahead
                A[st] = mcq_wload<MB>(wr, wlane, wso);
                wso += 256 * MB;
                __builtin_amdgcn_sched_barrier(0);
            }
            // (tried in round 3: weights as one 16-byte load per four k-steps + two statically alternating input buffers instead of
            //  the 16 copies -- 198 -> 150 non-MFMA instructions per 64 MFMAs in the ISA, and 4 % SLOWER on the GPU, 4381 -> 4560 us
            //  on the 384x256 layer: the wide loads hold the vector-memory path longer than four narrow ones spread over the steps)
            soff += (unsigned)GA * step_bytes;
        };
        if (npairs > 0) body(0);
        for (int sp = GA; sp < npairs; sp += GA) body(sp);
    } else {
    if (active) {
#pragma unroll
        for (int st = 0; st < PFA; ++st) {          // weights of steps 0 .. PFA-1 of the slice
            A[st] = mcq_wload<MB>(wr, wlane, wso);
            wso += 256 * MB * winc(st);
        }
#pragma unroll
        for (int st = 0; st < BSLOTS; ++st) {       // activations of steps 0 .. PFB-1
            const int tap = TAPS != 1 ? st % LT : 0;
            const unsigned so = soff + (unsigned)(TAPS != 1 ? st / LT : st) * step_bytes;
#pragma unroll
            for (int nb = 0; nb < NBG; ++nb) B[st][nb] = mcq_buffer_load(rsrc[nb], voff[nb][tap] + so);
        }
    }

    // (WINO) the transformed inputs of a group of PG k-steps from its PG loads, ring slots first .. first + PG - 1
    constexpr int PGV = WINO ? PG : 4;
    auto wino_transform = [&](const int first, float (&out)[PGV]) __attribute__((always_inline)) {
        if (W2D) {
            (void)first; (void)out;                      // (the 2-D form has its own loop above)
        } else {
            const float d0 = B[first % PFB][0], d1 = B[(first + 1) % PFB][0], d2 = B[(first + 2) % PFB][0], d3 = B[(first + 3) % PFB][0];
            out[0] = d0 - d2; out[1] = d1 + d2; out[2] = d2 - d1; out[3] = d1 - d3;
        }
    };
    float Vn[PGV];                                       // (WINO) transformed inputs of the group about to start
#pragma unroll
    for (int i = 0; i < PGV; ++i) Vn[i] = 0.0f;
    if (WINO && active) wino_transform(0, Vn);
    auto kbody = [&](const int sp) __attribute__((always_inline)) {
        // Every VALU instruction between two MFMAs costs the matrix pipe ~10 cycles (tools/probes/mfma_issue.hip), so
        // the k-loop has none: the channel-pair offset of an activation load lives in its buffer descriptor -- one per
        // pixel block and channel pair of the body, rebuilt by the scalar unit each iteration with num_records shrunk
        // accordingly (reads past the last channel stay out of range = 0) -- and the voffset is the bare tap offset.
        constexpr int PFBP = TAPS != 1 ? PFB / TAPS : PFB;   // look-ahead in channel pairs
        __amdgpu_buffer_rsrc_t rB[NBG][PAIRS_PER_ITER];
        float V[PGV];                                        // (WINO) the transformed inputs of the current group of PG steps
#pragma unroll
        for (int nb = 0; nb < NBG; ++nb)
#pragma unroll
            for (int j = 0; j < PAIRS_PER_ITER; ++j) {
                const unsigned off = soff + (unsigned)(PFBP + j) * step_bytes;
                const int left = (int)plane_bytes - (int)off;      // (signed max: the unsigned saturating form is VALU-only)
                rB[nb][j] = mcq_make_rsrc(xb[nb] + off, (unsigned)(left > 0 ? left : 0));
            }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (TAPS != 1 && u > 0 && u % TAPS == 0 && sp + u / TAPS >= npairs) break;   // the slice ends inside the body
            const int sa = u % PFA, sb = u % PFB;
            if constexpr (PAIR) {
                // k-step (channel pair q of the body, filter row dy, tap dx): the even pixel reads load `dx` of the row, the odd one
                // load `dx + 1`; load `dx` is dead after the even pixel's MFMAs (the odd pixel used it one step ago), load 3 after
                // the odd pixel's last tap -- each is refilled there with the same load two channel pairs on
                const int q = u / 9, t9 = u % 9, dy = t9 / 3, dx = t9 % 3, base = q * 12 + dy * 4;
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_elem<MB>(A[sa], mb), B[base + dx + nb][0], acc[mb][nb], 0, 0, 0);
                    if (nb == 0) B[base + dx][0] = mcq_buffer_load(rB[0][q], voff[0][dy * 4 + dx]);
                    else if (dx == 2) B[base + 3][0] = mcq_buffer_load(rB[0][q], voff[0][dy * 4 + 3]);
                }
                A[sa] = mcq_wload<MB>(wr, wlane, wso);
                wso += 256 * MB;
                __builtin_amdgcn_sched_barrier(0);
                continue;
            }
            float bv[NBG];
            if (WINO) {
                // four loads of one (channel pair, filter row) -> the B operands of four k-steps, formed one group AHEAD (during
                // the second step of the group before): a VALU result consumed by the very next MFMA is a hazard the inline-asm
                // MFMAs of the 128-row instance get no wait states for, and a stall for the others
                if (u % PG == 0) {
#pragma unroll
                    for (int i = 0; i < PGV; ++i) V[i] = Vn[i];
                }
                if (u % PG == 1) {
                    wino_transform(u + PG - 1, Vn);
                    if (WASM) {                              // (opaque: under register pressure the compiler re-forms a difference right in
                                                             //  front of its MFMA instead of keeping it -- seen once, caught by the hygiene test)
#pragma unroll
                        for (int i = 0; i < PGV; ++i) asm volatile("" : "+v"(Vn[i]));
                    }
                }
                bv[0] = V[(u % PG) % PGV];
            } else {
#pragma unroll
                for (int nb = 0; nb < NBG; ++nb) {
                    float v = B[sb][nb];
                    // (round 5, built and dropped: GDN / IGDN parking these x values in LDS for the epilogue, docs/experiments.md section 10.6)
                    if (PRO == PRO_SILU) v = mcq_silu(v);
                    if (PRO == PRO_SQUARE) v = v * v;
                    bv[nb] = v;
                }
            }
            // MFMAs pixel-block major, and each activation slot refilled right after its last use: the refill of block 0
            // issues while the MFMAs of block 1 run instead of queueing behind all MB x NB of them together with the
            // other loads (+1.6 % on the large layers); over-reads past the slice are harmless (the packed weights carry a
            // zero tail, activation offsets past the last channel are out of range = 0)
            const int tl = TAPS != 1 ? (u + PFB) % TAPS : 0;                    // tap of the step being loaded
            const int ds = TAPS != 1 ? (u + PFB) / TAPS : u + PFB;              // its channel-pair distance
#pragma unroll
            for (int nb = 0; nb < NBG; ++nb) {
                const int at = WINO ? u % PG : nb;           // accumulator tile: transform position / pixel block
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    if (WASM)
                        asm volatile("v_mfma_f32_32x32x2_f32 a[%2:%3], %0, %1, a[%2:%3]"
                                     :: "v"(a_elem<MB>(A[sa], mb)), "v"(bv[nb]), "n"(16 * (PG * mb + at)), "n"(16 * (PG * mb + at) + 15));
                    else
                        acc[mb][at % NACC] =
                            __builtin_amdgcn_mfma_f32_32x32x2f32(a_elem<MB>(A[sa], mb), bv[nb], acc[mb][at % NACC], 0, 0, 0);
                }
                B[sb][nb] = mcq_buffer_load(rB[nb][ds - PFBP], voff[nb][tl]);
            }
            A[sa] = mcq_wload<MB>(wr, wlane, wso);
            wso += 256 * MB * winc(u + PFA);
            // keep the software pipeline as written: without this fence the scheduler sinks the loads of all U
            // steps to the end of the (branch-free) body and waits for them one step later
            __builtin_amdgcn_sched_barrier(0);
        }
        soff += (unsigned)PAIRS_PER_ITER * step_bytes;
    };
    for (int sp = 0; sp < npairs; sp += PAIRS_PER_ITER) kbody(sp);
    }       // (!W2D)

    if (WASM) asm volatile("s_nop 15\n\ts_nop 15");       // (the last MFMAs' results must have landed before the first v_accvgpr_read)
    if constexpr (POST != 0) {
        // ---- the 1x1 layer that follows this convolution, on the fresh tile (MCQ_CONV_POST_*; round 6) ----------------------------------
        // The wave holds ALL 128 output channels of its NB x 32 pixels: lane (hi, j) owns channel 32 mb + (r & 3) + 8 (r >> 2) + 4 hi of
        // pixel j in acc[mb][nb][r] -- which is exactly the B operand of a 32x32x2 MFMA whose two k-slots are the channels (c, c + 4).  So the
        // 1x1 layer's contraction runs over the accumulator registers in THEIR order (k-step t = 16 mb + r; mcq_pack_post1x1_weight_f32
        // lays the weight out to match): no LDS, no exchange between lanes, no intermediate tensor.  Per pixel block: v = acc + bias
        // (+ res), 64 k-steps of four MFMAs into s[4], then the element-wise close of the layer from v and s -- the arithmetic of the
        // stand-alone 1x1 launch's epilogue (GDN: v * (1 / sqrt(s)), IGDN: v * sqrt(s), gate: mul * sigmoid(s) + id), whose k-order
        // over the 128 channels is the only thing that differs.
        const unsigned fl = p.flags;
        const unsigned HoWo = (unsigned)(p.Ho * p.Wo);
        const bool sub = post_sub;
        const int T = sub ? (co_base >> 7) : 0;                         // this wave's sub-pixel 2 dy + dx
        const unsigned OW = sub ? 2u * (unsigned)p.Wo : (unsigned)p.Wo, OHW = sub ? 4u * HoWo : HoWo;    // the output's row pitch / plane
        const unsigned oslab_bytes = 128u * OHW * 4u;                   // (the output has 128 channels either way)
        const __amdgpu_buffer_rsrc_t br = mcq_make_rsrc(mcq_uniform_ptr(P_bias ? P_bias : P_wp), P_bias ? (unsigned)p.Cout * 4u : 0u);
        const __amdgpu_buffer_rsrc_t pbr = mcq_make_rsrc(mcq_uniform_ptr(p.post_b ? p.post_b : P_wp), p.post_b ? 128u * 4u : 0u);
        const __amdgpu_buffer_rsrc_t pwr = mcq_make_rsrc(mcq_uniform_ptr(p.post_w), (unsigned)((POST_STEPS + POST_TAIL) * 1024));
        const unsigned pwlane = (unsigned)lane * 16u;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {                                // v = acc + bias: both pixel blocks of a band from one set of bias loads
            float b16[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) b16[r] = mcq_buffer_load_s(br, (unsigned)hi * 16u, (unsigned)(co_base + mb * 32 + mcq_drow(r, 0)) * 4u);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][nb][r] = acc[mb][nb][r] + b16[r];
            __builtin_amdgcn_sched_barrier(0);                          // (band by band: 64 bias values in flight at once would not fit)
        }
        // the closing phase runs band by band with the NEXT band's side values requested one band ahead (bias of the 1x1 layer; the gate's
        // multiplier and identity come from HBM), band 0's before the contraction starts; fences keep the compiler from pulling all four
        // bands' loads to the front, which the register file has no room for next to 128 + 64 accumulators
        auto band_so = [&](const int q, const int r) -> unsigned { return (unsigned)(q * 32 + mcq_drow(r, 0)) * OHW * 4u; };
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            __builtin_amdgcn_sched_barrier(0);
            const size_t oslab = (size_t)img[nb] * 128u * OHW;
            const __amdgpu_buffer_rsrc_t yr = mcq_make_rsrc(mcq_uniform_ptr(P_y + oslab), oslab_bytes);
            const unsigned opix = sub ? (unsigned)(2 * yo[nb] + (T >> 1)) * OW + (unsigned)(2 * xo[nb] + (T & 1)) : (unsigned)(yo[nb] * p.Wo + xo[nb]);
            const unsigned pvo = valid[nb] ? (opix + 4u * (unsigned)hi * OHW) * 4u : MCQ_OOB;
            if constexpr (POST == 2) {
                if (fl & MCQ_CONV_RESIDUAL) {                           // (the side stack's last ResidualBlock: + its input; conv-shaped = output-shaped here)
                    const __amdgpu_buffer_rsrc_t rr = mcq_make_rsrc(mcq_uniform_ptr(P_res + oslab), oslab_bytes);
                    float rv[2][16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) rv[0][r] = mcq_buffer_load_s(rr, pvo, band_so(0, r));
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb) {
                        if (mb < 3) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) rv[(mb + 1) & 1][r] = mcq_buffer_load_s(rr, pvo, band_so(mb + 1, r));
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[mb][nb][r] = acc[mb][nb][r] + p.res_scale * rv[mb & 1][r];
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            // s starts from the 1x1 layer's bias (beta for GDN / IGDN) instead of zero: no bias values to hold next to 128 + 64 accumulators
            f32x16 sacc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[q][r] = mcq_buffer_load_s(pbr, (unsigned)hi * 16u, (unsigned)(q * 32 + mcq_drow(r, 0)) * 4u);
            f32x4v AP[POST_PF];
#pragma unroll
            for (int st = 0; st < POST_PF; ++st) AP[st] = mcq_wload<4>(pwr, pwlane, (unsigned)st * 1024u);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < POST_STEPS; ++t) {
                float b = acc[t >> 4][nb][t & 15];
                if (POST == 1) b = b * b;
#pragma unroll
                for (int q = 0; q < 4; ++q) sacc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(AP[t % POST_PF][q], b, sacc[q], 0, 0, 0);
                AP[t % POST_PF] = mcq_wload<4>(pwr, pwlane, (unsigned)(t + POST_PF) * 1024u);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (POST == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (fl & MCQ_CONV_POST_IGDN) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) sacc[q][r] = acc[q][nb][r] * sqrtf(sacc[q][r]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) sacc[q][r] = acc[q][nb][r] * (1.0f / sqrtf(sacc[q][r]));
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) mcq_buffer_store_s(sacc[q][r], yr, pvo, band_so(q, r));
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                // the gate's multiplier and identity come from HBM: band q + 1's are requested before band q is closed (v is dead by now:
                // its registers hold them)
                const __amdgpu_buffer_rsrc_t mr = mcq_make_rsrc(mcq_uniform_ptr(P_mul + oslab), oslab_bytes);
                const __amdgpu_buffer_rsrc_t gr = mcq_make_rsrc(mcq_uniform_ptr(P_gid + oslab), oslab_bytes);
                const __amdgpu_buffer_rsrc_t y2r = mcq_make_rsrc(mcq_uniform_ptr(((fl & MCQ_CONV_DUAL_SILU) ? P_y2 : P_y) + oslab), oslab_bytes);
                float m[2][16], gi[2][16];
#pragma unroll
                for (int r = 0; r < 16; ++r) { m[0][r] = mcq_buffer_load_s(mr, pvo, band_so(0, r)); gi[0][r] = mcq_buffer_load_s(gr, pvo, band_so(0, r)); }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (q < 3) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            m[(q + 1) & 1][r] = mcq_buffer_load_s(mr, pvo, band_so(q + 1, r));
                            gi[(q + 1) & 1][r] = mcq_buffer_load_s(gr, pvo, band_so(q + 1, r));
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc[q][r] = m[q & 1][r] * mcq_sigmoid(sacc[q][r]) + gi[q & 1][r];
#pragma unroll
                    for (int r = 0; r < 16; ++r) mcq_buffer_store_s(sacc[q][r], yr, pvo, band_so(q, r));
                    if (fl & MCQ_CONV_DUAL_SILU) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) mcq_buffer_store_s(mcq_silu(sacc[q][r]), y2r, pvo, band_so(q, r));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        return;
    }
    // ---- epilogue ---------------------------------------------------------------------------
    // Lane (hi, j) owns pixel j of each of its NB blocks and, per 32-row tile, the 16 output channels
    // row(r) + 4 hi, row(r) = (r & 3) + 8 (r >> 2).  Element (co, pixel) of image n sits at byte (co HoWo + pixel) 4 of
    // that image's [Cout, Ho, Wo] slab, for the output and for every side input (all have the output's shape).  All
    // epilogue traffic goes through buffer instructions on a per-image descriptor: the per-lane part (pixel, the 4 hi
    // rows) is the voffset, the row of register r the wave-uniform soffset.  Rows >= Cout land beyond num_records and
    // lanes without a pixel carry the out-of-range marker, so loads return 0 and stores are dropped by the hardware:
    // no predication, no branches, and hipcc is free to overlap the side loads of one tile with the math of another.
    const unsigned fl = p.flags;
    const unsigned HoWo = (unsigned)(p.Ho * p.Wo + tile_zero);
    const unsigned slab_bytes = (unsigned)p.Cout * HoWo * 4u;

    auto epilogue = [&](auto tag, const bool tile_active, auto&& get_acc, const int mb_first, auto count_tag) {
        constexpr unsigned EF = decltype(tag)::value;                 // compile-time flag set, or RUNTIME_FLAGS
        constexpr int MC = decltype(count_tag)::value;                // 32-row bands this wave finishes
        const unsigned f = EF == RUNTIME_FLAGS ? fl : EF;
        if (!tile_active) return;
        unsigned pvo[NB];
        __amdgpu_buffer_rsrc_t yr[NB], y2r[NB], rr_[NB], mr[NB], gr[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const size_t slab = (size_t)img[nb] * p.Cout * HoWo;
            yr[nb] = mcq_make_rsrc(mcq_uniform_ptr(P_y + slab), slab_bytes);
            constexpr unsigned GBWD = MCQ_CONV_GDN_BWD | MCQ_CONV_IGDN_BWD | MCQ_CONV_GATE_BWD;
            if (f & (MCQ_CONV_DUAL_SILU | GBWD)) y2r[nb] = mcq_make_rsrc(mcq_uniform_ptr(P_y2 + slab), slab_bytes);
            if (f & (MCQ_CONV_RESIDUAL | GBWD)) rr_[nb] = mcq_make_rsrc(mcq_uniform_ptr(P_res + slab), slab_bytes);
            if (f & (MCQ_CONV_GDN | MCQ_CONV_IGDN | MCQ_CONV_GATE | MCQ_CONV_MUL | MCQ_CONV_DSILU_MUL | GBWD))
                mr[nb] = mcq_make_rsrc(mcq_uniform_ptr(P_mul + slab), slab_bytes);
            if (f & MCQ_CONV_GATE) gr[nb] = mcq_make_rsrc(mcq_uniform_ptr(P_gid + slab), slab_bytes);
            if (f & MCQ_CONV_SHUFFLE2)      // [Cout/4, 2 Ho, 2 Wo]: channel c = co / 4 -> rows of 2 Wo, this lane's 2x2 cell
                pvo[nb] = valid[nb] ? ((unsigned)hi * 4u * HoWo + (unsigned)(2 * yo[nb]) * (unsigned)(2 * p.Wo) + (unsigned)(2 * xo[nb])) * 4u
                                    : MCQ_OOB;
            else
                pvo[nb] = valid[nb] ? ((unsigned)(yo[nb] * p.Wo + xo[nb]) + 4u * (unsigned)hi * HoWo) * 4u : MCQ_OOB;
        }
        const __amdgpu_buffer_rsrc_t br = mcq_make_rsrc(mcq_uniform_ptr(P_bias ? P_bias : P_wp), P_bias ? (unsigned)p.Cout * 4u : 0u);

#pragma unroll
        for (int mi = 0; mi < MC; ++mi) {
            const int mb = mb_first + mi;
            const unsigned co_row0 = (unsigned)(co_base + mb * 32);   // wave-uniform
            float bias16[16];
#pragma unroll
            for (int r = 0; r < 16; ++r)
                bias16[r] = mcq_buffer_load_s(br, (unsigned)hi * 16u, (co_row0 + (unsigned)mcq_drow(r, 0)) * 4u);
            // The four flag sets that make up the network's 3x3 layers (plain, SiLU, residual, residual + SiLU twin) finish a
            // whole 32-row band in three phases -- side loads of all its pixel blocks, then all arithmetic, then all stores --
            // instead of block by block with loads, activation and stores alternating (measured: +1.8 % on a 384x256 layer
            // with the twin epilogue, +0.9 % images/s)
            // (the two flag sets of the training step's input-gradient launches -- * silu'(.) and * silu'(.) + dy -- as well: in
            //  the generic path their side loads sat in front of each block's arithmetic; 8 x 128 x 128 x 128 map 311 -> ~277 us)
            constexpr unsigned SIMPLE = MCQ_CONV_SILU_OUT | MCQ_CONV_RESIDUAL | MCQ_CONV_DUAL_SILU | MCQ_CONV_DSILU_MUL;
            if (EF != RUNTIME_FLAGS && (EF & ~SIMPLE) == 0u && NB <= 2) {     // (NB = 4: 192 temporaries, spills)
                unsigned sob[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) sob[r] = (co_row0 + (unsigned)mcq_drow(r, 0)) * HoWo * 4u;
                // pixel blocks finished together per three-phase pass: both at two waves per SIMD; ONE at three waves per SIMD (the
                // 64 x 64 tile's 168-register budget: the 96 temporaries of two blocks spilled 24 registers to scratch there)
                constexpr int EB = OCC >= 3 ? 1 : NB;
#pragma unroll
                for (int nb0 = 0; nb0 < NB; nb0 += EB) {
                    float vv[EB][16], rvv[EB][16], tw[EB][16];
                    // (PAIR: the two blocks are the even and the odd pixel of a lane's pair -- 8 adjacent, 8-byte aligned bytes of every
                    //  output-shaped tensor, the width being even: one 64-bit access per row for both)
                    if (EF & MCQ_CONV_DSILU_MUL) {              // (tw is free here: no SiLU twin in a gradient launch)
                        if constexpr (PAIR && EB == 2) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) { const f32x2v t2 = mcq_buffer_load2_s(mr[0], pvo[0], sob[r]); tw[0][r] = t2[0]; tw[1][r] = t2[1]; }
                        } else {
#pragma unroll
                        for (int e = 0; e < EB; ++e)
#pragma unroll
                            for (int r = 0; r < 16; ++r) tw[e][r] = mcq_buffer_load_s(mr[nb0 + e], pvo[nb0 + e], sob[r]);
                        }
                    }
                    if (EF & MCQ_CONV_RESIDUAL) {
                        if constexpr (PAIR && EB == 2) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) { const f32x2v t2 = mcq_buffer_load2_s(rr_[0], pvo[0], sob[r]); rvv[0][r] = t2[0]; rvv[1][r] = t2[1]; }
                        } else {
#pragma unroll
                        for (int e = 0; e < EB; ++e)
#pragma unroll
                            for (int r = 0; r < 16; ++r) rvv[e][r] = mcq_buffer_load_s(rr_[nb0 + e], pvo[nb0 + e], sob[r]);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < EB; ++e) {
                        get_acc(mi, nb0 + e, vv[e]);
#pragma unroll
                        for (int r = 0; r < 16; ++r) vv[e][r] = vv[e][r] + bias16[r];
                        if (EF & MCQ_CONV_DSILU_MUL) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) vv[e][r] = vv[e][r] * mcq_dsilu(tw[e][r]);
                        }
                        if (EF & MCQ_CONV_RESIDUAL) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) vv[e][r] = vv[e][r] + p.res_scale * rvv[e][r];
                        }
                        if (EF & MCQ_CONV_SILU_OUT) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) vv[e][r] = mcq_silu(vv[e][r]);
                        }
                        if (EF & MCQ_CONV_DUAL_SILU) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) tw[e][r] = mcq_silu(vv[e][r]);
                        }
                    }
                    if constexpr (PAIR && EB == 2) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) mcq_buffer_store2_s(f32x2v{vv[0][r], vv[1][r]}, yr[0], pvo[0], sob[r]);
                        if (EF & MCQ_CONV_DUAL_SILU) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) mcq_buffer_store2_s(f32x2v{tw[0][r], tw[1][r]}, y2r[0], pvo[0], sob[r]);
                        }
                    } else {
#pragma unroll
                    for (int e = 0; e < EB; ++e) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) mcq_buffer_store_s(vv[e][r], yr[nb0 + e], pvo[nb0 + e], sob[r]);
                        if (EF & MCQ_CONV_DUAL_SILU) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) mcq_buffer_store_s(tw[e][r], y2r[nb0 + e], pvo[nb0 + e], sob[r]);
                        }
                    }
                    }
                }
                continue;
            }
            if constexpr (PAIR) {
                // every other flag set the launcher sends here (subsets of SiLU / twin / residual / * silu'(.), PixelShuffle store): both
                // pixels of the pair together, 64-bit accesses (128-bit through the shuffle: a pair's cells are four adjacent floats)
                float v0[16], v1[16];
                get_acc(mi, 0, v0);
                get_acc(mi, 1, v1);
#pragma unroll
                for (int r = 0; r < 16; ++r) { v0[r] = v0[r] + bias16[r]; v1[r] = v1[r] + bias16[r]; }
                if (f & MCQ_CONV_SHUFFLE2) {
                    const unsigned W2b = 2u * (unsigned)p.Wo * 4u;
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) {
                        const unsigned so = ((co_row0 >> 2) + 2u * (unsigned)rq) * HoWo * 16u;
                        f32x4v top = f32x4v{v0[rq * 4 + 0], v0[rq * 4 + 1], v1[rq * 4 + 0], v1[rq * 4 + 1]};
                        f32x4v bot = f32x4v{v0[rq * 4 + 2], v0[rq * 4 + 3], v1[rq * 4 + 2], v1[rq * 4 + 3]};
                        if (f & MCQ_CONV_DSILU_MUL) {
                            const f32x4v mt = mcq_buffer_load4_s(mr[0], pvo[0], so), mb2 = mcq_buffer_load4_s(mr[0], pvo[0], so + W2b);
#pragma unroll
                            for (int e = 0; e < 4; ++e) { top[e] = top[e] * mcq_dsilu(mt[e]); bot[e] = bot[e] * mcq_dsilu(mb2[e]); }
                        }
                        if (f & MCQ_CONV_RESIDUAL) {
                            const f32x4v rt = mcq_buffer_load4_s(rr_[0], pvo[0], so), rb = mcq_buffer_load4_s(rr_[0], pvo[0], so + W2b);
#pragma unroll
                            for (int e = 0; e < 4; ++e) { top[e] = top[e] + p.res_scale * rt[e]; bot[e] = bot[e] + p.res_scale * rb[e]; }
                        }
                        mcq_buffer_store4_s(top, yr[0], pvo[0], so);
                        mcq_buffer_store4_s(bot, yr[0], pvo[0], so + W2b);
                    }
                    continue;
                }
                unsigned so[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) so[r] = (co_row0 + (unsigned)mcq_drow(r, 0)) * HoWo * 4u;
                if (f & MCQ_CONV_DSILU_MUL) {
                    f32x2v m2[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) m2[r] = mcq_buffer_load2_s(mr[0], pvo[0], so[r]);
#pragma unroll
                    for (int r = 0; r < 16; ++r) { v0[r] = v0[r] * mcq_dsilu(m2[r][0]); v1[r] = v1[r] * mcq_dsilu(m2[r][1]); }
                }
                if (f & MCQ_CONV_RESIDUAL) {
                    f32x2v r2[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) r2[r] = mcq_buffer_load2_s(rr_[0], pvo[0], so[r]);
#pragma unroll
                    for (int r = 0; r < 16; ++r) { v0[r] = v0[r] + p.res_scale * r2[r][0]; v1[r] = v1[r] + p.res_scale * r2[r][1]; }
                }
                if (f & MCQ_CONV_SILU_OUT) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) { v0[r] = mcq_silu(v0[r]); v1[r] = mcq_silu(v1[r]); }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) mcq_buffer_store2_s(f32x2v{v0[r], v1[r]}, yr[0], pvo[0], so[r]);
                if (f & MCQ_CONV_DUAL_SILU) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mcq_buffer_store2_s(f32x2v{mcq_silu(v0[r]), mcq_silu(v1[r])}, y2r[0], pvo[0], so[r]);
                }
                continue;
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                float v[16];
                get_acc(mi, nb, v);
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = v[r] + bias16[r];
                if (f & MCQ_CONV_SHUFFLE2) {
                    // registers 4q..4q+3 are the 2x2 sub-pixels of output channel co / 4: two float2 rows
                    const unsigned W2b = 2u * (unsigned)p.Wo * 4u;
#pragma unroll
                    for (int rq = 0; rq < 4; ++rq) {
                        const unsigned so = ((co_row0 >> 2) + 2u * (unsigned)rq) * HoWo * 16u;
                        f32x2v top = f32x2v{v[rq * 4 + 0], v[rq * 4 + 1]}, bot = f32x2v{v[rq * 4 + 2], v[rq * 4 + 3]};
                        // (round 5) the input-gradient launch of a stride-2 convolution stores through the shuffle; when that convolution
                        // sits behind a SiLU and beside a skip path (ResidualBlockWithStride) the two side operations of the plain
                        // input-gradient launches apply here too, at the shuffled addresses: * silu'(mul), + res
                        if (f & MCQ_CONV_DSILU_MUL) {
                            const f32x2v mt = mcq_buffer_load2_s(mr[nb], pvo[nb], so), mb2 = mcq_buffer_load2_s(mr[nb], pvo[nb], so + W2b);
                            top = f32x2v{top[0] * mcq_dsilu(mt[0]), top[1] * mcq_dsilu(mt[1])};
                            bot = f32x2v{bot[0] * mcq_dsilu(mb2[0]), bot[1] * mcq_dsilu(mb2[1])};
                        }
                        if (f & MCQ_CONV_RESIDUAL) {
                            const f32x2v rt = mcq_buffer_load2_s(rr_[nb], pvo[nb], so), rb = mcq_buffer_load2_s(rr_[nb], pvo[nb], so + W2b);
                            top = f32x2v{top[0] + p.res_scale * rt[0], top[1] + p.res_scale * rt[1]};
                            bot = f32x2v{bot[0] + p.res_scale * rb[0], bot[1] + p.res_scale * rb[1]};
                        }
                        mcq_buffer_store2_s(top, yr[nb], pvo[nb], so);
                        mcq_buffer_store2_s(bot, yr[nb], pvo[nb], so + W2b);
                    }
                    continue;
                }
                unsigned so[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) so[r] = (co_row0 + (unsigned)mcq_drow(r, 0)) * HoWo * 4u;
                // (compiled into the one-pixel-block 1x1 instances with the squaring prologue only -- the launcher routes these
                //  launches there: in every other instance the extra 32 side values pushed the run-time-flag path into scratch)
                if (TAPS == 1 && PRO == PRO_SQUARE && NB == 1 && (f & (MCQ_CONV_GDN_BWD | MCQ_CONV_IGDN_BWD))) {
                    // v = s = beta + gamma x^2 (recomputed); the two element-wise gradients of y = x f(s) leave from here instead of a
                    // launch of their own behind a stored s: dxd = dy f(s), ds = dy x f'(s) (train_ops.hip: gdn_bwd_prep_kernel's order)
                    float m[16], g[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) { m[r] = mcq_buffer_load_s(mr[nb], pvo[nb], so[r]); g[r] = mcq_buffer_load_s(rr_[nb], pvo[nb], so[r]); }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float rs = 1.0f / sqrtf(v[r]);
                        float dxd, ds;
                        if (f & MCQ_CONV_IGDN_BWD) { dxd = g[r] * sqrtf(v[r]); ds = g[r] * m[r] * (0.5f * rs); }
                        else { dxd = g[r] * rs; ds = g[r] * m[r] * (-0.5f * rs * rs * rs); }
                        mcq_buffer_store_s(dxd, yr[nb], pvo[nb], so[r]);
                        mcq_buffer_store_s(ds, y2r[nb], pvo[nb], so[r]);
                    }
                    continue;
                }
                // (the same for the AttentionBlock gate out = a sigmoid(s) + x, s = conv1x1(b) recomputed here: the training forward then
                //  runs the gate as the 1x1 launch's epilogue like inference does and keeps no s; compiled into the plain 1x1
                //  one-pixel-block instances only)
                if (TAPS == 1 && PRO == PRO_NONE && NB == 1 && (f & MCQ_CONV_GATE_BWD)) {
                    float m[16], g[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) { m[r] = mcq_buffer_load_s(mr[nb], pvo[nb], so[r]); g[r] = mcq_buffer_load_s(rr_[nb], pvo[nb], so[r]); }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float sg = mcq_sigmoid(v[r]);
                        mcq_buffer_store_s(g[r] * sg, yr[nb], pvo[nb], so[r]);                                    // d a
                        mcq_buffer_store_s(g[r] * m[r] * sg * (1.0f - sg), y2r[nb], pvo[nb], so[r]);              // d s
                    }
                    continue;
                }
                if (f & (MCQ_CONV_GDN | MCQ_CONV_IGDN | MCQ_CONV_GATE | MCQ_CONV_MUL | MCQ_CONV_DSILU_MUL)) {
                    float m[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) m[r] = mcq_buffer_load_s(mr[nb], pvo[nb], so[r]);
                    // (round 5, built and dropped: 1/sqrt(s) and sqrt(s) from v_rsq_f32 + one Newton step, docs/experiments.md section 10.6)
                    if (f & MCQ_CONV_GDN) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = m[r] * (1.0f / sqrtf(v[r]));
                    } else if (f & MCQ_CONV_IGDN) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = m[r] * sqrtf(v[r]);
                    } else if (f & MCQ_CONV_MUL) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = m[r] * v[r];
                    } else if (f & MCQ_CONV_DSILU_MUL) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = v[r] * mcq_dsilu(m[r]);
                    } else {
                        float gi[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) gi[r] = mcq_buffer_load_s(gr[nb], pvo[nb], so[r]);
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = m[r] * mcq_sigmoid(v[r]) + gi[r];
                    }
                }
                if (f & MCQ_CONV_RESIDUAL) {
                    float rv[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) rv[r] = mcq_buffer_load_s(rr_[nb], pvo[nb], so[r]);
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = v[r] + p.res_scale * rv[r];
                }
                if (f & MCQ_CONV_SILU_OUT) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = mcq_silu(v[r]);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) mcq_buffer_store_s(v[r], yr[nb], pvo[nb], so[r]);
                if (f & MCQ_CONV_DUAL_SILU) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mcq_buffer_store_s(mcq_silu(v[r]), y2r[nb], pvo[nb], so[r]);
                }
            }
        }
    };
    // the flag sets the network issues most get their own branch-free instance; anything else takes the generic one
    auto run_epilogue = [&](const bool tile_active, auto&& get_acc, const int mb_first, auto mb_count) {
        const unsigned ef = fl & ~(unsigned)(MCQ_CONV_SILU_IN | MCQ_CONV_SQUARE_IN);
        if (ef == (MCQ_CONV_RESIDUAL | MCQ_CONV_DUAL_SILU))
            epilogue(std::integral_constant<unsigned, MCQ_CONV_RESIDUAL | MCQ_CONV_DUAL_SILU>{}, tile_active, get_acc, mb_first, mb_count);
        else if (ef == MCQ_CONV_SILU_OUT)
            epilogue(std::integral_constant<unsigned, MCQ_CONV_SILU_OUT>{}, tile_active, get_acc, mb_first, mb_count);
        else if (ef == 0u)
            epilogue(std::integral_constant<unsigned, 0u>{}, tile_active, get_acc, mb_first, mb_count);
        else if (ef == MCQ_CONV_RESIDUAL)
            epilogue(std::integral_constant<unsigned, MCQ_CONV_RESIDUAL>{}, tile_active, get_acc, mb_first, mb_count);
        // (the input-gradient flag sets only where one pixel block per wave leaves the registers for it -- the 128 x 32 and
        //  32 x 32 tiles; in the 128 x 64 instance the extra 32 side values spilled, and that instance is the inference path's)
        else if (!WINO && TAPS == 9 && NB == 1 && ef == MCQ_CONV_DSILU_MUL)
            epilogue(std::integral_constant<unsigned, MCQ_CONV_DSILU_MUL>{}, tile_active, get_acc, mb_first, mb_count);
        else if (!WINO && TAPS == 9 && NB == 1 && ef == (MCQ_CONV_DSILU_MUL | MCQ_CONV_RESIDUAL))
            epilogue(std::integral_constant<unsigned, MCQ_CONV_DSILU_MUL | MCQ_CONV_RESIDUAL>{}, tile_active, get_acc, mb_first, mb_count);
        else
            epilogue(std::integral_constant<unsigned, RUNTIME_FLAGS>{}, tile_active, get_acc, mb_first, mb_count);
    };

    if constexpr (WASM) {
        // Epilogue of the 128-row Winograd instance for the flag sets of the network's 3x3 layers (plain, SiLU, residual,
        // residual + SiLU twin); anything else (PixelShuffle store, ...) takes the generic path below.  One wave per SIMD:
        // nothing else hides the latency of the side loads, so ALL of them (bias and residual of the four bands: 64 + 128
        // registers, the operand rings are dead by now) are issued before the first band is finished.  With an even width
        // the two pixels of a lane's pair are 8 adjacent, 8-byte aligned bytes of every output-shaped tensor: one 64-bit
        // access per row instead of two 32-bit ones at a stride of 8 bytes.
        const unsigned ef = fl & ~(unsigned)(MCQ_CONV_SILU_IN | MCQ_CONV_SQUARE_IN);
        constexpr unsigned SIMPLE_W = MCQ_CONV_SILU_OUT | MCQ_CONV_RESIDUAL | MCQ_CONV_DUAL_SILU;
        auto wasm_epilogue = [&](auto tag) __attribute__((always_inline)) {
            constexpr unsigned EF = decltype(tag)::value;
            const size_t slab = (size_t)img[0] * p.Cout * HoWo;
            const __amdgpu_buffer_rsrc_t yr = mcq_make_rsrc(mcq_uniform_ptr(P_y + slab), slab_bytes);
            const __amdgpu_buffer_rsrc_t y2r = mcq_make_rsrc(mcq_uniform_ptr((EF & MCQ_CONV_DUAL_SILU) ? P_y2 + slab : P_y + slab), slab_bytes);
            const __amdgpu_buffer_rsrc_t rr = mcq_make_rsrc(mcq_uniform_ptr((EF & MCQ_CONV_RESIDUAL) ? P_res + slab : P_y + slab), slab_bytes);
            const __amdgpu_buffer_rsrc_t br = mcq_make_rsrc(mcq_uniform_ptr(P_bias ? P_bias : P_wp), P_bias ? (unsigned)p.Cout * 4u : 0u);
            unsigned pvo[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                pvo[nb] = valid[nb] ? ((unsigned)(yo[nb] * p.Wo + xo[nb]) + 4u * (unsigned)hi * HoWo) * 4u : MCQ_OOB;
            const bool wide = (p.Wo & 1) == 0;                  // (wave-uniform)
            if constexpr (W2D) {
                // one 32-row band, a 2 x 2 pixel tile per lane: rows oy = 0 / 1 of the tile are two 64-bit accesses (even width)
                unsigned pv4[4];
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
                    pv4[nb] = valid[nb] ? ((unsigned)(yo[nb] * p.Wo + xo[nb]) + 4u * (unsigned)hi * HoWo) * 4u : MCQ_OOB;
                float bias16[16];
                f32x2v res2[2][16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned row = (unsigned)co_base + (unsigned)mcq_drow(r, 0);
                    bias16[r] = mcq_buffer_load_s(br, (unsigned)hi * 16u, row * 4u);
                    if (EF & MCQ_CONV_RESIDUAL) {
#pragma unroll
                        for (int oy = 0; oy < 2; ++oy) {
                            if (wide) res2[oy][r] = mcq_buffer_load2_s(rr, pv4[2 * oy], row * HoWo * 4u);
                            else res2[oy][r] = f32x2v{mcq_buffer_load_s(rr, pv4[2 * oy], row * HoWo * 4u), mcq_buffer_load_s(rr, pv4[2 * oy + 1], row * HoWo * 4u)};
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if ((r & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                    float m[16];
#pragma unroll
                    for (int pos = 0; pos < 16; ++pos) asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(m[pos]) : "n"(16 * pos + r));
                    float sx[4][2];                           // A^T M A: along x ...
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        sx[i][0] = (m[4 * i] + m[4 * i + 1]) + m[4 * i + 2];
                        sx[i][1] = (m[4 * i + 1] - m[4 * i + 2]) - m[4 * i + 3];
                    }
                    const unsigned so = ((unsigned)co_base + (unsigned)mcq_drow(r, 0)) * HoWo * 4u;
#pragma unroll
                    for (int oy = 0; oy < 2; ++oy) {          // ... then along y: the two pixels of output row oy
                        f32x2v y, tw = {0.0f, 0.0f};
#pragma unroll
                        for (int ox = 0; ox < 2; ++ox) {
                            y[ox] = (oy == 0 ? (sx[0][ox] + sx[1][ox]) + sx[2][ox] : (sx[1][ox] - sx[2][ox]) - sx[3][ox]) + bias16[r];
                            if (EF & MCQ_CONV_RESIDUAL) y[ox] = y[ox] + p.res_scale * res2[oy][r][ox];
                        }
                        if (EF & MCQ_CONV_SILU_OUT) y = f32x2v{mcq_silu(y[0]), mcq_silu(y[1])};
                        if (EF & MCQ_CONV_DUAL_SILU) tw = f32x2v{mcq_silu(y[0]), mcq_silu(y[1])};
                        if (wide) {
                            mcq_buffer_store2_s(y, yr, pv4[2 * oy], so);
                            if (EF & MCQ_CONV_DUAL_SILU) mcq_buffer_store2_s(tw, y2r, pv4[2 * oy], so);
                        } else {
                            mcq_buffer_store_s(y[0], yr, pv4[2 * oy], so);
                            mcq_buffer_store_s(y[1], yr, pv4[2 * oy + 1], so);
                            if (EF & MCQ_CONV_DUAL_SILU) {
                                mcq_buffer_store_s(tw[0], y2r, pv4[2 * oy], so);
                                mcq_buffer_store_s(tw[1], y2r, pv4[2 * oy + 1], so);
                            }
                        }
                    }
                }
                return;
            }
            float ball[MB][16];
            f32x2v rall[MB][16];
            // side loads run one band ahead of the band being finished (a band takes longer than their latency; more of them in
            // flight would leave the compiler short of VGPRs, and it must not touch an AGPR here)
            auto side_loads = [&](const int mb) __attribute__((always_inline)) {
                const unsigned co_row0 = (unsigned)(co_base + mb * 32);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    ball[mb][r] = mcq_buffer_load_s(br, (unsigned)hi * 16u, (co_row0 + (unsigned)mcq_drow(r, 0)) * 4u);
                if (EF & MCQ_CONV_RESIDUAL) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const unsigned so = (co_row0 + (unsigned)mcq_drow(r, 0)) * HoWo * 4u;
                        if (wide) rall[mb][r] = mcq_buffer_load2_s(rr, pvo[0], so);
                        else rall[mb][r] = f32x2v{mcq_buffer_load_s(rr, pvo[0], so), mcq_buffer_load_s(rr, pvo[1], so)};
                    }
                }
            };
            side_loads(0);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("" ::: "memory");              // (keeps the next bands' side loads from being hoisted up here)
                if (mb + 1 < MB) side_loads(mb + 1);
                const unsigned co_row0 = (unsigned)(co_base + mb * 32);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // a row is stored as soon as it is finished (whole bands of results held back for a store phase cost
                    // 64 registers, which this instance does not have to spare next to the side loads)
                    if ((r & 3) == 0) __builtin_amdgcn_sched_barrier(0);
                    f32x2v y, tw = {0.0f, 0.0f};
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        float a, b, c;                            // back from the four transform positions to the pixel
                        asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(a) : "n"(16 * (4 * mb + (nb == 0 ? 0 : 1)) + r));
                        asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(b) : "n"(16 * (4 * mb + (nb == 0 ? 1 : 2)) + r));
                        asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(c) : "n"(16 * (4 * mb + (nb == 0 ? 2 : 3)) + r));
                        y[nb] = (nb == 0 ? (a + b) + c : (a - b) - c) + ball[mb][r];
                        if (EF & MCQ_CONV_RESIDUAL) y[nb] = y[nb] + p.res_scale * rall[mb][r][nb];
                    }
                    if (EF & MCQ_CONV_SILU_OUT) y = f32x2v{mcq_silu(y[0]), mcq_silu(y[1])};
                    if (EF & MCQ_CONV_DUAL_SILU) tw = f32x2v{mcq_silu(y[0]), mcq_silu(y[1])};
                    const unsigned so = (co_row0 + (unsigned)mcq_drow(r, 0)) * HoWo * 4u;
                    if (wide) {
                        mcq_buffer_store2_s(y, yr, pvo[0], so);
                        if (EF & MCQ_CONV_DUAL_SILU) mcq_buffer_store2_s(tw, y2r, pvo[0], so);
                    } else {
                        mcq_buffer_store_s(y[0], yr, pvo[0], so);
                        mcq_buffer_store_s(y[1], yr, pvo[1], so);
                        if (EF & MCQ_CONV_DUAL_SILU) {
                            mcq_buffer_store_s(tw[0], y2r, pvo[0], so);
                            mcq_buffer_store_s(tw[1], y2r, pvo[1], so);
                        }
                    }
                }
            }
        };
        (void)ef; (void)SIMPLE_W;
        if constexpr (WEF != RUNTIME_FLAGS) {
            wasm_epilogue(std::integral_constant<unsigned, WEF>{});
            vwg += gridDim.x;
            if (vwg < (unsigned)p.total_wgs) goto next_tile;
            return;
        }
    }
    if (KS == 1) {
        run_epilogue(true, [&](int mi, int nb, float (&v)[16]) {           // (mi, nb are constants once unrolled)
            if (WINO) {
                // back from the transform positions to the pixels of the pair / tile, band by band (all accumulator tiles at
                // once would need every accumulator in a VALU-readable register at the same time)
                auto m_at = [&](const int pos, const int r) __attribute__((always_inline)) -> float {
                    if (WASM) {
                        float x;
                        asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(x) : "n"(16 * (PG * mi + pos) + r));
                        return x;
                    }
                    return acc[mi][pos % NACC][r];
                };
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (W2D) {                               // pixel (oy, ox) = nb: A^T M A, first along x, then along y
                        const int oy = nb >> 1, ox = nb & 1;
                        float sx[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            sx[i] = ox == 0 ? (m_at(4 * i, r) + m_at(4 * i + 1, r)) + m_at(4 * i + 2, r)
                                            : (m_at(4 * i + 1, r) - m_at(4 * i + 2, r)) - m_at(4 * i + 3, r);
                        v[r] = oy == 0 ? (sx[0] + sx[1]) + sx[2] : (sx[1] - sx[2]) - sx[3];
                    } else
                        v[r] = nb == 0 ? (m_at(0, r) + m_at(1, r)) + m_at(2, r) : (m_at(1, r) - m_at(2, r)) - m_at(3, r);
                }
                return;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = acc[mi][nb][r];
        }, 0, std::integral_constant<int, MB>{});
        if constexpr (WASM) {
            vwg += gridDim.x;
            if (vwg < (unsigned)p.total_wgs) goto next_tile;
        }
        return;
    }

    // split-K: the KS partial tiles of a 32-row band meet in LDS ([slice][nb][r][lane], conflict-free) and wave
    // (mb % KS) adds them in slice order (deterministic).  The owner only SUMS between the two barriers and keeps
    // the band in registers; the global-memory epilogues of all bands then run concurrently on their owner waves
    // after the last barrier (finishing inside the barrier pair serialised the bands: ~11 us each).
    float* slot0 = mcq_lds + (size_t)(tile_in_wg << p.ks_log2) * (NB * 1024);
    if constexpr (MB == 1 && NB <= 2 && !WINO) {
        // One band: slice 0's wave owns it.  The others park their partial tiles, ONE barrier, and the owner adds them (slice
        // order, two slices per LDS round trip) from inside the epilogue's accumulator hook -- i.e. after the epilogue has
        // requested its bias / residual, whose latency then runs beside the sum instead of after it.  Stamp probe of an 8-way
        // split 4x4 launch (round 3, tools/probes/tiny_stamps.py): 1.4 us from the slowest slice's last MFMA to the summed tile
        // with the general form below -- seven dependent LDS round trips between two barriers -- and 1.1 us of epilogue behind
        // it; 0.3 + 1.5 us with this one.  (Also tried there: requesting the weight ring ahead of the ~1 us of pixel geometry.
        // Nothing: the eight slices of a tile share one CU, and their k-loop is that CU's matrix pipe, not a latency.)
        if (active && kslice != 0) {
            float* mine = slot0 + (size_t)kslice * (NB * 1024) + lane;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mine[(nb * 16 + r) * 64] = acc[0][nb][r];
        }
        __syncthreads();
        run_epilogue(active && kslice == 0, [&](int, int nb, float (&v)[16]) {
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = acc[0][nb][r];
            const float* other = slot0 + (size_t)(nb * 16) * 64 + lane;
            int w = 1;
            for (; w + 1 < KS; w += 2) {
                float a[16], b[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) { a[r] = other[(size_t)w * (NB * 1024) + r * 64]; b[r] = other[(size_t)(w + 1) * (NB * 1024) + r * 64]; }
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = (v[r] + a[r]) + b[r];
            }
            if (w < KS) {
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = v[r] + other[(size_t)w * (NB * 1024) + r * 64];
            }
        }, 0, std::integral_constant<int, 1>{});
        return;
    }
    float own[NB][16];                         // band `kslice` (the launcher guarantees KS >= MB when it splits)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        if (active) {
            float* mine = slot0 + (size_t)kslice * (NB * 1024) + lane;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mine[(nb * 16 + r) * 64] = acc[mb][nb][r];
        }
        __syncthreads();
        if (active && kslice == mb) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) own[nb][r] = slot0[(nb * 16 + r) * 64 + lane];
            for (int w = 1; w < KS; ++w) {
                const float* other = slot0 + (size_t)w * (NB * 1024) + lane;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) own[nb][r] = own[nb][r] + other[(nb * 16 + r) * 64];
            }
        }
        __syncthreads();
    }
    run_epilogue(active && kslice < MB, [&](int, int nb, float (&v)[16]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = own[nb][r];
    }, kslice, std::integral_constant<int, 1>{});
}

}  // namespace
