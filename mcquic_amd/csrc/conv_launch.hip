// mcq_conv2d_f32 / mcq_conv2d_multi_f32: validation, the choice of kernel, tile and split for a layer, and the launch.  Host code plus
// the two small 16-row kernels; the conv_mfma_kernel instances are in conv_tiles_*.hip / conv_wino32.hip (conv_instances.h).
#include <mutex>
#include <unordered_map>

#include "conv_instances.h"
#include "conv_sizes.h"
#include "conv_wino16.h"
#include "conv_head16.h"
#include "conv_t16.h"

namespace {

// Which copy of its operand stream a launch reads, recorded per packed buffer while tracing is on (mcq_conv_section_trace): a
// training step captured as a hipGraph replays the same launches forever, so its in-graph re-pack after the optimizer's update
// only needs to refresh the copies those launches read (mcq_pack_conv_weight_multi_masked_f32) -- a quarter of the bytes.
std::mutex g_sec_mu;
bool g_sec_trace = false;
std::unordered_map<const float*, unsigned> g_sec_used;
inline void sec_note(const mcq_conv_desc* descs, int nprob, unsigned bit) {
    if (!g_sec_trace) return;
    std::lock_guard<std::mutex> lock(g_sec_mu);
    for (int c = 0; c < nprob; ++c) g_sec_used[descs[c].w_packed] |= bit;
}

bool wino_shape(int Cout, int ksize, int stride, unsigned fl) {
    return ksize == 3 && stride == 1 && Cout % 64 == 0 && !(fl & (MCQ_CONV_SILU_IN | MCQ_CONV_SQUARE_IN));
}

// Does mcq_conv2d_f32 take a Winograd launch of this geometry and flag set (pointers and the 2 GiB addressing limits aside)?  Every
// rule conv_validate, conv_launch and mcq_wino16_launch apply to one, in one place: mcq_conv2d_winograd_ok answers with it and
// conv_launch refuses by it, so the two cannot disagree.  Without a Winograd flag the question is about MCQ_CONV_WINOGRAD.
bool wino_taken(int Cin, int Cout, int ksize, int stride, unsigned flags) {
    const unsigned W3 = MCQ_CONV_WINOGRAD | MCQ_CONV_WINOGRAD2D | MCQ_CONV_WINOGRAD2D16;
    const unsigned wf = (flags & W3) ? (flags & W3) : (unsigned)MCQ_CONV_WINOGRAD;
    if (wf & (wf - 1)) return false;                                        // one form per launch
    if (flags & MCQ_CONV_TAPS_LR) return false;                             // (the four-tap walk is the direct kernel's)
    const unsigned fl = flags & ~(W3 | (unsigned)MCQ_CONV_TAPS_LR);         // the prologue / epilogue flags
    if (!wino_shape(Cout, ksize, stride, fl)) return false;
    if (fl & (MCQ_CONV_POST_MASK | MCQ_CONV_GDN_BWD | MCQ_CONV_IGDN_BWD | MCQ_CONV_GATE_BWD)) return false;      // epilogues of the direct form
    if ((fl & MCQ_CONV_DUAL_SILU) && (fl & MCQ_CONV_SILU_OUT)) return false;
    if ((fl & MCQ_CONV_SHUFFLE2) && fl != MCQ_CONV_SHUFFLE2) return false;  // the PixelShuffle store of a Winograd form carries nothing else
    if (wf == MCQ_CONV_WINOGRAD2D && (Cout % 128 != 0 || Cin % 8 != 0)) return false;
    if (wf == MCQ_CONV_WINOGRAD2D16) {
        if (Cout % 128 != 0 || Cin % 16 != 0) return false;
        if (fl != MCQ_CONV_SHUFFLE2 && (fl & ~(unsigned)(MCQ_CONV_SILU_OUT | MCQ_CONV_RESIDUAL | MCQ_CONV_DUAL_SILU))) return false;
    }
    return true;
}

// does mcq_conv2d_f32 take a MCQ_CONV_POST_* launch on its own (`row_tiles` 128-row tiles per pixel block)?  From two 128 x 32 wave tiles
// per SIMD; below that the map's 3x3 layer is normally split over waves and the 1x1 layer stays a launch (unless the caller forces tile 0x41)
inline bool post_fills_chip(long long tb, int row_tiles) { return tb * row_tiles >= 2048; }

// The 32 lanes of a block cover (32 >> lg) rows x (1 << lg) columns of a rows x cols map (of pixels, pixel pairs or 2 x 2 tiles):
// the lg in 5 .. min_lg that wastes the fewest lanes (wider wins ties)
int block_width_log2(int rows, int cols, int min_lg) {
    int best_log2 = 5; double best_util = -1.0;
    for (int lg = 5; lg >= min_lg; --lg) {
        const int bw = 1 << lg, bh = 32 >> lg;
        const double cover = (double)((rows + bh - 1) / bh * bh) * (double)((cols + bw - 1) / bw * bw);
        const double util = (double)rows * cols / cover;
        if (util > best_util + 1e-9) { best_util = util; best_log2 = lg; }
    }
    return best_log2;
}

// the tensors of problem `e` of a launch: P = ConvK (problem 0) or ConvPtrs (its `alt`), W16K or W16Ptrs, and T16Ptrs
template <class P> void conv_ptrs(P& a, const mcq_conv_desc* e, size_t sec4, size_t sec2) {
    a.x = e->x; a.wp = e->w_packed; a.wp64 = a.wp + sec4; a.wp32 = a.wp64 + sec2;
    a.bias = e->bias; a.y = e->y; a.y2 = e->y_silu; a.res = e->res; a.mul = e->mul; a.gid = e->gate_id;
}
template <class P> void w16_ptrs(P& a, const mcq_conv_desc* e) {
    a.x = e->x; a.wp = e->w_packed; a.bias = e->bias; a.y = e->y; a.y2 = e->y_silu; a.res = e->res;
}
void t16_ptrs(T16Ptrs& a, const mcq_conv_desc* e, size_t sec) {
    a.x = e->x; a.wp = e->w_packed + sec; a.bias = e->bias; a.y = e->y; a.y2 = e->y_silu; a.res = e->res; a.mul = e->mul;
}

int conv_validate(const mcq_conv_desc* d) {
    if (!d || !d->x || !d->w_packed || !d->y) return MCQ_EINVAL;
    if (d->N <= 0 || d->Cin <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0) return MCQ_EINVAL;
    if ((d->ksize != 1 && d->ksize != 3) || (d->stride != 1 && d->stride != 2)) return MCQ_EINVAL;
    if ((d->flags & MCQ_CONV_TAPS_LR) && (d->ksize != 3 || d->stride != 1 || (d->flags & (MCQ_CONV_WINOGRAD | MCQ_CONV_WINOGRAD2D | MCQ_CONV_WINOGRAD2D16 |
                                                                                    MCQ_CONV_SILU_IN | MCQ_CONV_SQUARE_IN)))) return MCQ_EINVAL;
    const unsigned fl = d->flags & ~(unsigned)MCQ_CONV_TAPS_LR;      // (a promise about the weights, not an operation)
    if (fl & MCQ_CONV_POST_MASK) {                           // the following 1x1 layer inside this launch
        const unsigned post = fl & MCQ_CONV_POST_MASK;
        if ((post & (post - 1)) || !d->post_w || d->ksize != 3 || (d->flags & MCQ_CONV_TAPS_LR)) return MCQ_EINVAL;
        unsigned allowed = MCQ_CONV_POST_MASK | MCQ_CONV_SILU_IN;
        if (post == MCQ_CONV_POST_IGDN) allowed |= MCQ_CONV_SHUFFLE2;
        if (post == MCQ_CONV_POST_GATE) allowed |= MCQ_CONV_RESIDUAL | MCQ_CONV_DUAL_SILU;
        if (fl & ~allowed) return MCQ_EINVAL;
        if (d->Cout != ((fl & MCQ_CONV_SHUFFLE2) ? 512 : 128)) return MCQ_EINVAL;
        if (post == MCQ_CONV_POST_GATE && (!d->mul || !d->gate_id || d->stride != 1)) return MCQ_EINVAL;
    }
    if ((fl & MCQ_CONV_RESIDUAL) && !d->res) return MCQ_EINVAL;
    if ((fl & (MCQ_CONV_GDN | MCQ_CONV_IGDN | MCQ_CONV_GATE | MCQ_CONV_MUL | MCQ_CONV_DSILU_MUL)) && !d->mul) return MCQ_EINVAL;
    if ((fl & MCQ_CONV_GATE) && !d->gate_id) return MCQ_EINVAL;
    if ((fl & MCQ_CONV_DUAL_SILU) && (!d->y_silu || (fl & MCQ_CONV_SILU_OUT))) return MCQ_EINVAL;
    if (fl & (MCQ_CONV_GDN_BWD | MCQ_CONV_IGDN_BWD)) {      // s-launch with the GDN backward's element-wise part as its epilogue
        if (!d->res || !d->mul || !d->y_silu || (fl & ~(unsigned)(MCQ_CONV_SQUARE_IN | MCQ_CONV_GDN_BWD | MCQ_CONV_IGDN_BWD)) ||
            (fl & MCQ_CONV_GDN_BWD && fl & MCQ_CONV_IGDN_BWD) || d->ksize != 1) return MCQ_EINVAL;
    }
    if (fl & MCQ_CONV_GATE_BWD) {                            // s-launch with the gate's backward as its epilogue
        if (!d->res || !d->mul || !d->y_silu || (fl & ~(unsigned)MCQ_CONV_GATE_BWD) || d->ksize != 1 || d->stride != 1) return MCQ_EINVAL;
    }
    if ((fl & MCQ_CONV_SILU_IN) && (fl & MCQ_CONV_SQUARE_IN)) return MCQ_EINVAL;
    if (fl & MCQ_CONV_SHUFFLE2) {
        if ((d->Cout & 3) || (fl & ~(unsigned)(MCQ_CONV_SHUFFLE2 | MCQ_CONV_SILU_IN | MCQ_CONV_SQUARE_IN | MCQ_CONV_WINOGRAD | MCQ_CONV_WINOGRAD2D | MCQ_CONV_WINOGRAD2D16 |
                                               MCQ_CONV_DSILU_MUL | MCQ_CONV_RESIDUAL | MCQ_CONV_POST_IGDN))) return MCQ_EINVAL;
        if ((fl & (MCQ_CONV_DSILU_MUL | MCQ_CONV_RESIDUAL)) && (fl & (MCQ_CONV_WINOGRAD | MCQ_CONV_WINOGRAD2D | MCQ_CONV_WINOGRAD2D16)))
            return MCQ_EINVAL;
    }
    // one image's input slab plus the prefetch rings' over-read (up to 8 channels) must stay below 2 GiB: byte offsets and
    // the descriptors' shrinking num_records are 32-bit (signed in the scalar arithmetic of the k-loop)
    if ((uint64_t)(d->Cin + 8) * d->H * d->W * 4ull >= 0x80000000ull) return MCQ_ETOOLARGE;
    return MCQ_OK;
}

bool t16_takes(int N, int Cin, int H, int W, int Cout, int ksize, int stride, unsigned fl, int nprob) {
    return N > 0 && H > 0 && W > 0 && nprob >= 1 && t16_shape(Cout, Cin, ksize) && stride == 1 && (fl & ~T16_FLAGS) == 0 &&
           t16_tiles((long long)N * H * W, Cout, nprob) <= T16_MAX_TILES &&
           (uint64_t)N * (Cin > Cout ? Cin : Cout) * H * W * 4ull < 0x80000000ull;
}

int conv_launch(const mcq_conv_desc* descs, int nprob, void* stream) {
    const mcq_conv_desc* d = descs;
    const unsigned fl = d->flags & ~(unsigned)MCQ_CONV_TAPS_LR;
    const bool lr4 = d->flags & MCQ_CONV_TAPS_LR;      // only the filter's lower-right 2 x 2 taps are non-zero
    ConvK k;
    const size_t sec4 = section_floats(d->Cout, d->Cin, d->ksize, 4), sec2 = section_floats(d->Cout, d->Cin, d->ksize, 2);
    conv_ptrs(k, d, sec4, sec2);
    k.N = d->N; k.Cin = d->Cin; k.H = d->H; k.W = d->W; k.Cout = d->Cout;
    k.ks = d->ksize; k.stride = d->stride;
    const int pad = d->ksize / 2;
    k.Ho = (d->H + 2 * pad - d->ksize) / d->stride + 1;
    k.Wo = (d->W + 2 * pad - d->ksize) / d->stride + 1;
    k.S = pairs_padded(d->Cin, d->ksize);
    k.TP = steps_padded(d->Cin, d->ksize);
    k.flags = fl; k.res_scale = d->res_scale;
    k.nprob = nprob;
    k.post_w = d->post_w; k.post_b = d->post_bias; k.post_sub = 0;
    for (int c = 1; c < MCQ_CONV_MAX_MULTI; ++c) conv_ptrs(k.alt[c - 1], descs + (c < nprob ? c : 0), sec4, sec2);

    if ((fl & (MCQ_CONV_WINOGRAD | MCQ_CONV_WINOGRAD2D | MCQ_CONV_WINOGRAD2D16)) && !wino_taken(d->Cin, d->Cout, d->ksize, d->stride, d->flags))
        return MCQ_EINVAL;
    if (fl & MCQ_CONV_WINOGRAD2D16) {
        // F(2x2, 3x3) on the 16 x 16 x 4 instruction, two waves per SIMD (conv_wino16.hip)
        if ((fl & (MCQ_CONV_WINOGRAD | MCQ_CONV_WINOGRAD2D)) || !wino_shape(d->Cout, d->ksize, d->stride, fl)) return MCQ_EINVAL;
        W16K w;
        w16_ptrs(w, d);
        for (int c = 1; c < W16_MAX_MULTI; ++c) w16_ptrs(w.alt[c - 1], descs + (c < nprob ? c : 0));
        w.nprob = nprob; w.N = d->N; w.Cin = d->Cin; w.H = d->H; w.W = d->W; w.Cout = d->Cout; w.Ho = k.Ho; w.Wo = k.Wo;
        w.flags = fl & ~(unsigned)MCQ_CONV_WINOGRAD2D16; w.res_scale = d->res_scale;
        return mcq_wino16_launch(w, stream);
    }
    if (fl & MCQ_CONV_WINOGRAD2D) {
        if ((fl & MCQ_CONV_WINOGRAD) || !wino_shape(d->Cout, d->ksize, d->stride, fl) || d->Cout % 128 != 0 || d->Cin % 8 != 0) return MCQ_EINVAL;
        if ((uint64_t)(d->Cin + 16) * d->H * d->W * 4ull >= 0x80000000ull) return MCQ_ETOOLARGE;
        k.TP = k.S * 16;
        k.wp32 = k.wp; k.wp64 = k.wp;
        for (int c = 1; c < MCQ_CONV_MAX_MULTI; ++c) { k.alt[c - 1].wp32 = k.alt[c - 1].wp; k.alt[c - 1].wp64 = k.alt[c - 1].wp; }
        // tile blocks: 32 tiles of 2 x 2 pixels shaped (32 >> b) rows x (1 << b) tiles, b by the fewest wasted lanes
        const int Wt = (k.Wo + 1) / 2, Ht = (k.Ho + 1) / 2;
        const int best_log2 = block_width_log2(Ht, Wt, 0);
        k.bw_log2 = best_log2;
        k.nbx = (Wt + (1 << best_log2) - 1) >> best_log2;
        k.nby = (Ht + (32 >> best_log2) - 1) / (32 >> best_log2);
        const long long tbw = (long long)k.N * k.nbx * k.nby;
        if (tbw > 0x7fffffffLL) return MCQ_ETOOLARGE;
        k.total_blocks = (int)tbw;
        if ((uint64_t)d->Cout * (uint64_t)k.Ho * k.Wo * 4ull >= 0x80000000ull) return MCQ_ETOOLARGE;
        k.flags = fl & ~(unsigned)MCQ_CONV_WINOGRAD2D;
        return launch_wino2d(k, tbw, d->Cout / 128, (hipStream_t)stream);
    }
    if (fl & MCQ_CONV_WINOGRAD) {
        if (!wino_shape(d->Cout, d->ksize, d->stride, fl)) return MCQ_EINVAL;
        if ((uint64_t)(d->Cin + 16) * d->H * d->W * 4ull >= 0x80000000ull) return MCQ_ETOOLARGE;     // (rings up to 8 channel pairs ahead)
        const int forced_mb = (d->tile & 0xff) >> 4;
        const int MBw = forced_mb == 2 || d->Cout % 128 != 0 ? 2 : 4;
        k.TP = k.S * 12;
        k.wp64 = k.wp + wino_section_floats(d->Cout, d->Cin, 4);
        k.wp32 = k.wp64;
        for (int c = 1; c < MCQ_CONV_MAX_MULTI; ++c) {
            k.alt[c - 1].wp64 = k.alt[c - 1].wp + wino_section_floats(d->Cout, d->Cin, 4);
            k.alt[c - 1].wp32 = k.alt[c - 1].wp64;
        }
        // pair blocks: 32 pairs shaped (32 >> b) rows x (1 << b) pairs, b by the fewest wasted lanes
        const int Wp = (k.Wo + 1) / 2;
        const int best_log2 = block_width_log2(k.Ho, Wp, 2);
        k.bw_log2 = best_log2;
        k.nbx = (Wp + (1 << best_log2) - 1) >> best_log2;
        k.nby = (k.Ho + (32 >> best_log2) - 1) / (32 >> best_log2);
        const long long tbw = (long long)k.N * k.nbx * k.nby;
        if (tbw > 0x7fffffffLL) return MCQ_ETOOLARGE;
        k.total_blocks = (int)tbw;
        const int co_tiles = (d->Cout + 32 * MBw - 1) / (32 * MBw);
        if ((uint64_t)co_tiles * 32u * (unsigned)MBw * (uint64_t)k.Ho * k.Wo * 4ull >= 0x80000000ull) return MCQ_ETOOLARGE;
        k.flags = fl & ~(unsigned)MCQ_CONV_WINOGRAD;
        return MBw == 4 ? launch_wino<4>(k, tbw, co_tiles, (hipStream_t)stream) : launch_wino<2>(k, tbw, co_tiles, (hipStream_t)stream);
    }

    // launches too small to fill the chip with 32 x 32 tiles: 16 x 16 tiles, one per workgroup (conv_t16.h)
    if (d->tile == 0 && t16_takes(d->N, d->Cin, d->H, d->W, d->Cout, d->ksize, d->stride, fl, nprob)) {
        sec_note(descs, nprob, 8u);
        T16K t;
        const size_t sec = section_floats(d->Cout, d->Cin, 3, 4) + section_floats(d->Cout, d->Cin, 3, 2) + section_floats(d->Cout, d->Cin, 3, 1);
        for (int c = 0; c < MCQ_CONV_MAX_MULTI; ++c) t16_ptrs(t.p[c], descs + (c < nprob ? c : 0), sec);
        t.N = d->N; t.Cin = d->Cin; t.H = d->H; t.W = d->W; t.Cout = d->Cout; t.flags = fl; t.res_scale = d->res_scale;
        const dim3 grid((unsigned)(((long long)d->N * d->H * d->W + 15) / 16), (unsigned)(d->Cout / 16), (unsigned)nprob);
        if (d->Cin == 128) hipLaunchKernelGGL(conv_t16_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, t);
        else hipLaunchKernelGGL(conv_t16_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, t);
        return mcq_check_launch();
    }

    // <= 16 output channels, 3x3, stride 1, nothing but bias / PixelShuffle in the epilogue: the 16-row MFMA kernel
    if (nprob == 1 && head16_shape(d->Cout, d->ksize) && d->stride == 1 && (d->tile & 0xff) == 0 &&
        (fl & ~(unsigned)(MCQ_CONV_SHUFFLE2 | MCQ_CONV_SILU_IN)) == 0) {
        if ((uint64_t)d->Cout * d->H * d->W * 4ull >= 0x80000000ull) return MCQ_ETOOLARGE;
        Head16K h;
        h.x = d->x; h.wp16 = d->w_packed + general_floats(d->Cout, d->Cin, d->ksize); h.bias = d->bias; h.y = d->y;
        h.N = d->N; h.Cin = d->Cin; h.H = d->H; h.W = d->W; h.Cout = d->Cout;
        h.S4 = (d->Cin + 3) / 4;
        h.gpr = (d->W + 15) / 16;
        h.total_groups = (long long)d->N * d->H * h.gpr;
        h.flags = fl;
        const long long waves = (h.total_groups + H16_NB - 1) / H16_NB;
        if ((waves + 3) / 4 > 0x7fffffffLL) return MCQ_ETOOLARGE;
        const dim3 grid((unsigned)((waves + 3) / 4));
        if (fl & MCQ_CONV_SILU_IN) hipLaunchKernelGGL(conv_head16_kernel<PRO_SILU>, grid, dim3(256), 0, (hipStream_t)stream, h);
        else hipLaunchKernelGGL(conv_head16_kernel<PRO_NONE>, grid, dim3(256), 0, (hipStream_t)stream, h);
        return mcq_check_launch();
    }

    // pixel-block shape: the power-of-two width that wastes the fewest lanes (wider wins ties)
    const int best_log2 = block_width_log2(k.Ho, k.Wo, 2);
    k.bw_log2 = best_log2;
    const int bw = 1 << best_log2, bh = 32 >> best_log2;
    k.nbx = (k.Wo + bw - 1) / bw;
    k.nby = (k.Ho + bh - 1) / bh;
    const long long tb = (long long)k.N * k.nbx * k.nby;
    if (tb > 0x7fffffffLL) return MCQ_ETOOLARGE;
    k.total_blocks = (int)tb;

    // Wave tile and split-K.  Weight traffic per wave is the whole filter bank whatever the tile, so the tile stays
    // as large as the layer allows (128 co x 64 px); when that leaves too few waves for the 1024 SIMDs the k-steps of
    // a tile are split over 2/4/8 waves of one workgroup and reduced through LDS.
    const int co32 = (d->Cout + 31) / 32;
    int MB, NB, ksl = 0;
    bool dsilu41 = false;                 // the 128 x 32 tile chosen over the 128 x 64 one for an input-gradient epilogue (see below)
    const int forced = d->tile & 0xff;
    if (forced) {
        MB = forced >> 4; NB = forced & 15; ksl = (d->tile >> 8) & 3;
        if ((MB != 1 && MB != 2 && MB != 4) || (NB != 1 && NB != 2 && NB != 4)) return MCQ_EINVAL;      // (no such tile: NB = 0 would divide by zero below)
    }
    else if (co32 == 1) {
        // <= 32 output channels (the 12-channel head, the tiny fixture models): one weight load feeds NB MFMAs, so the
        // widest pixel tile that still leaves >= 2048 waves amortises it best (head conv 2.34 -> 2.05 ms with NB = 4)
        MB = 1; NB = (tb * nprob >= 4 * 2048) ? 4 : 2;
        // Neon's 32-wide layers (channel 32, stride-1 stem: 256 x 256 ... 16 x 16 maps; round 5, tools/microbench_conv.py --neon,
        // profiles/r05_neon_tile_sweep.txt): with <= 32 input channels a k-loop is 144 steps and the epilogue weighs as much as the
        // weights' amortisation -- two pixel blocks per wave only where the launch has waves to spare (4 x 512x512: 218 us against
        // 237 / 221 for one / four), one below that (256x256 49.9 vs 53.8 us, 128x128 16.0 vs 26.9, 64x64 11.5 vs 14.8), split over
        // two waves when even that leaves SIMDs idle (4 x 64 -> 8 at 64x64: 11.6 us against 22.4)
        if (d->Cin <= 64) {
            NB = (tb * nprob >= 16384) ? 2 : 1;
            while (ksl < 3 && (((tb + NB - 1) / NB * nprob) << ksl) < 1024) ++ksl;
        }
    }
    else if (co32 == 2 && ((tb + 1) / 2) * nprob < 2048 && d->ksize == 3) {
        // 64 output channels on maps that leave the 64 x 64 tile short of waves (Neon's 64-wide layers live on 64 x 64 maps):
        // one wave per 32 x 32 tile, unsplit, instead of the larger tile split 4 / 8 ways through LDS (4 x 64 -> 64 at 64x64:
        // 14.7 us against 21.4; 32 -> 64: 11.6 against 17.0)
        MB = 1; NB = 1;
        while (ksl < 3 && ((tb * co32 * nprob) << ksl) < 1024) ++ksl;
    }
    else {
        // (the 128 x 32 tile <4, 1> is instantiated and reachable through `tile`; an automatic rule preferring it on
        //  the 24x16 / 12x8 levels gained 0.4 % at batch 32 and lost 8 % on the batch-8 training step: not used)
        static const int cand[3][2] = {{4, 2}, {2, 2}, {1, 1}};
        MB = 1; NB = 1;
        // Cout that is no multiple of 128 (model No. 12 of the reference: channel 192 = six 32-row bands): the 128-row tile would
        // run its last instance half empty -- 8 bands of MFMAs for 6 -- where 64-row tiles cover the rows exactly; the 64 x 64 tile
        // costs ~3 % more per MFMA than the 128 x 64 one (operand loads per MFMA), far less than a quarter of the work
        const bool rows64 = ((co32 + 3) / 4) * 4 > ((co32 + 1) / 2) * 2;
        for (int c = 0; c < 3; ++c) {
            const int mb = cand[c][0], nb = cand[c][1];
            if (mb > co32 || (mb == 4 && rows64)) continue;
            const long long tiles = ((tb + nb - 1) / nb) * ((co32 + mb - 1) / mb);      // (per problem: the tile a single launch takes)
            MB = mb; NB = nb;
            if (tiles * 8 >= 1024) break;          // even an 8-way split would leave SIMDs idle: try a smaller tile
        }
        const long long tiles1 = ((tb + NB - 1) / NB) * ((co32 + MB - 1) / MB);             // one problem
        const long long tiles = tiles1 * nprob;                                              // all problems of the launch
        while (ksl < 3 && (tiles << ksl) < 2048) ++ksl;
        int ksl1 = 0;                                                                        // what a single-problem launch would split
        while (ksl1 < 3 && (tiles1 << ksl1) < 2048) ++ksl1;
        // an 8-way split of the 128 x 64 tile runs as a 4-way split of the 128 x 32 tile instead: the same number of
        // waves, half the LDS reduction depth, 3 waves / SIMD resident (8 x 128 x 32 x 32 layer: 50 -> 28 us)
        // a 4-way split 128 x 64 tile that needs 1.5 rounds at 2 waves / SIMD -- the 48x32 level -- runs as
        // the 64 x 64 tile split 2 ways, all waves resident at 3 / SIMD (120 -> 111 us per launch, +0.4 % images/s; with
        // the earlier k-loop, whose address arithmetic weighed twice as much on the smaller tile, it cost 0.4 %)
        // (judged per problem: two such problems in one launch are 6144 waves = two full rounds at 3 / SIMD, 204 us per pair,
        //  where the 128 x 64 tile split 2 ways would be 1.5 rounds at 2 / SIMD, 224 us)
        // (round 3, forced-tile sweeps with 2 / 4 problems per launch: with the paired heads in lockstep the 48x32 level mostly
        //  runs as such launches, and then the 64 x 64 tile needs no split at all -- 4 problems: 449 -> 414 us, 2: 217 -> 215)
        if (MB == 4 && NB == 2 && ksl1 == 2 && tiles1 * 4 > 2048 && tiles1 * 4 <= 3072 && d->ksize == 3 &&
            k.S % 2 == 0 && (k.S >> 1) >= 8) { MB = 2; NB = 2; ksl = nprob >= 2 ? 0 : 1; }
        if (MB == 4 && NB == 2 && ksl == 3 && d->ksize == 3 && k.S % 4 == 0 && (k.S >> 2) >= 8) { NB = 1; ksl = 2; }
        // the same trade one step down: a 2-way split of the 128 x 64 tile runs as the UNSPLIT 128 x 32 tile -- as many waves, no
        // LDS reduction, every wave finishes its own half of the pixels instead of the owner waves finishing all of them
        // (two 8 x 128 x 64 x 64 problems in one launch, the AttentionBlock stacks of a training step: 153-156 -> 140-142 us)
        else if (MB == 4 && NB == 2 && ksl == 1 && d->ksize == 3) { NB = 1; ksl = 0; }
        // ... and a 4-way split of it in a multi-problem launch as the 64 x 64 tile split 2 ways (32 x 24x16 maps, 4 problems:
        // 120 -> 112 us; one 192x128 map, 2 problems: 117 -> 110 us)
        else if (MB == 4 && NB == 2 && ksl == 2 && nprob >= 2 && d->ksize == 3 && k.S % 2 == 0 && (k.S >> 1) >= 8) { MB = 2; ksl = 1; }
        // input-gradient launches of the training step (* silu'(.) [+ dy]): their epilogue carries one more output-shaped side
        // read and a sigmoid per element; the 128 x 32 tile has a band-wise instance of it (the 128 x 64 tile has no registers
        // left for one) and at three waves per SIMD hides it better (8 x 128 x 128 x 128: 300-311 -> 270-277 us)
        else if (MB == 4 && NB == 2 && ksl == 0 && (fl & MCQ_CONV_DSILU_MUL) && d->ksize == 3) { NB = 1; dsilu41 = true; }
        // 1x1 layers (GDN / IGDN, the AttentionBlock gate): 64 k-steps per tile against an epilogue that reads and writes an
        // output-shaped tensor each -- HBM time, not matrix time.  One pixel block per wave (half the epilogue per wave, three
        // waves per SIMD to hide it) wins wherever the launch still fills the chip without a split: 32 x 128 x 384x256 GDN
        // 1276 -> 1234 us, 192x128 323 -> 306, 96x64 87 -> 73, 48x32 (64 x 32 tile) 38.7 -> 26.3 (tools/microbench_conv.py --k1 --flags gdn)
        if (d->ksize == 1 && d->stride == 1 && co32 >= 4) {
            const long long t41 = tb * ((co32 + 3) / 4) * nprob, t21 = tb * ((co32 + 1) / 2) * nprob;
            if (t41 >= 2048 && !rows64) { MB = 4; NB = 1; ksl = 0; }
            else if (t21 >= 2048) { MB = 2; NB = 1; ksl = 0; }
        }
    }
    if (fl & (MCQ_CONV_GDN_BWD | MCQ_CONV_IGDN_BWD)) {      // the instances that carry this epilogue: one pixel block per wave, no split
        if (!(fl & MCQ_CONV_SQUARE_IN)) return MCQ_EINVAL;
        NB = 1; ksl = 0;
    }
    if (fl & MCQ_CONV_GATE_BWD) { NB = 1; ksl = 0; }        // (likewise)
    int post = 0;
    if (fl & MCQ_CONV_POST_MASK) {
        // unsplit 128-row tiles that fill the chip, or the caller runs the 1x1 layer as its own launch (mcq_conv2d_post_ok)
        if (nprob != 1 || lr4) return MCQ_EINVAL;
        if (!post_fills_chip(tb, (fl & MCQ_CONV_SHUFFLE2) ? 4 : 1) && forced != 0x41) return MCQ_EINVAL;     // (tile 0x41: on any map size)
        MB = 4; NB = 1; ksl = 0; dsilu41 = false;
        post = (fl & MCQ_CONV_POST_GATE) ? 2 : 1;
        k.post_sub = (fl & MCQ_CONV_SHUFFLE2) ? 1 : 0;
    }
    const int pro = (fl & MCQ_CONV_SILU_IN) ? PRO_SILU : (fl & MCQ_CONV_SQUARE_IN) ? PRO_SQUARE : PRO_NONE;
    long long ptiles = (tb + NB - 1) / NB;
    // (round 5) the 128 x 64 tile of a 3x3 stride-1 layer over 32 PAIRS of horizontally adjacent pixels, when tile bit 0x400 asks
    // for it: pair blocks shaped (32 >> b) rows x (1 << b) pairs, b by the fewest wasted lanes
    const bool pair_ok = !post && !lr4 && MB == 4 && (NB == 2 || dsilu41) && ksl == 0 && d->ksize == 3 && d->stride == 1 && pro == PRO_NONE && (k.Wo & 1) == 0 &&
                         !(fl & ~(unsigned)(MCQ_CONV_SILU_OUT | MCQ_CONV_RESIDUAL | MCQ_CONV_DUAL_SILU | MCQ_CONV_DSILU_MUL | MCQ_CONV_SHUFFLE2));
    // (round 5, built and dropped: the launcher choosing it on its own for one-round launches, docs/experiments.md section 10.8)
    const bool pair = pair_ok && (d->tile & 0x400);
    if (pair) {
        const int Wp = k.Wo / 2;
        const int bl = block_width_log2(k.Ho, Wp, 2);
        const int pnbx = (Wp + (1 << bl) - 1) >> bl, pnby = (k.Ho + (32 >> bl) - 1) / (32 >> bl);
        const long long pt = (long long)k.N * pnbx * pnby;
        NB = 2; k.bw_log2 = bl; k.nbx = pnbx; k.nby = pnby; ptiles = pt; k.total_blocks = (int)pt;
    }
    const int co_tiles = post ? 1 : (co32 + MB - 1) / MB;      // (POST through the shuffle: the four row tiles are the waves of a workgroup)
    // the epilogue addresses one image of the output (and of every side input) through a 32-bit buffer offset,
    // rows of the last cout tile included
    if ((uint64_t)(post && k.post_sub ? 4 : co_tiles) * 32u * (unsigned)MB * (uint64_t)k.Ho * k.Wo * 4ull >= 0x80000000ull) return MCQ_ETOOLARGE;
    hipStream_t s = (hipStream_t)stream;
    sec_note(descs, nprob, MB == 4 ? 1u : MB == 2 ? 2u : 4u);
    if (MB == 4 && NB == 2) return launch_tile<4, 2, MCQ_PF42A, MCQ_PF42B, 4>(k, pro, ptiles, co_tiles, ksl, s, pair, lr4);
    if (MB == 4 && NB == 1) return launch_tile<4, 1, 9, MCQ_PFB, 8>(k, pro, ptiles, co_tiles, ksl, s, false, lr4, post);
    if (MB == 2 && NB == 2) return launch_tile<2, 2, 9, MCQ_PFB, 8>(k, pro, ptiles, co_tiles, ksl, s, false, lr4);
    if (MB == 2 && NB == 1) return launch_tile<2, 1, 9, MCQ_PFB, 16>(k, pro, ptiles, co_tiles, ksl, s, false, lr4);
    if (MB == 1 && NB == 4) return launch_tile<1, 4, 9, MCQ_PFB, 8>(k, pro, ptiles, co_tiles, ksl, s, false, lr4);
    if (MB == 1 && NB == 2) return launch_tile<1, 2, 9, MCQ_PFB, 8>(k, pro, ptiles, co_tiles, ksl, s, false, lr4);
    if (MB == 1 && NB == 1) return launch_tile<1, 1, 9, MCQ_PFB, 16>(k, pro, ptiles, co_tiles, ksl, s, false, lr4);
    return MCQ_EINVAL;
}

}  // namespace

extern "C" int32_t mcq_conv2d_winograd_ok(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t ksize, int32_t stride,
                                          uint32_t flags) {
    return (N > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0 && wino_taken(Cin, Cout, ksize, stride, flags)) ? 1 : 0;
}

extern "C" void mcq_conv_section_trace(int32_t on) {
    std::lock_guard<std::mutex> lock(g_sec_mu);
    if (on) g_sec_used.clear();
    g_sec_trace = on != 0;
}

extern "C" uint32_t mcq_conv_sections_used(const float* packed) {
    std::lock_guard<std::mutex> lock(g_sec_mu);
    const auto it = g_sec_used.find(packed);
    return it == g_sec_used.end() ? 0u : it->second;
}

extern "C" int mcq_conv2d_f32(const mcq_conv_desc* d, void* stream) {
    const int rc = conv_validate(d);
    return rc != MCQ_OK ? rc : conv_launch(d, 1, stream);
}

extern "C" int32_t mcq_conv2d_max_multi(void) { return MCQ_CONV_MAX_MULTI; }

extern "C" int32_t mcq_conv2d_post_ok(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t ksize, int32_t stride, uint32_t flags) {
    const unsigned post = flags & MCQ_CONV_POST_MASK;
    if (N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || ksize != 3 || (stride != 1 && stride != 2) || !post || (post & (post - 1))) return 0;
    const bool sub = flags & MCQ_CONV_SHUFFLE2;
    if (sub && post != MCQ_CONV_POST_IGDN) return 0;
    if (Cout != (sub ? 512 : 128)) return 0;
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (W + 2 - 3) / stride + 1;
    const int best_log2 = block_width_log2(Ho, Wo, 2);      // (the pixel-block shape conv_launch picks)
    const long long tb = (long long)N * ((Wo + (1 << best_log2) - 1) >> best_log2) * ((Ho + (32 >> best_log2) - 1) / (32 >> best_log2));
    // (the number of 128 x 32 wave tiles, capped: >= 2048 is what mcq_conv2d_f32 takes on its own; below that a caller may still
    //  force the fused form with tile 0x41 where it has measured a gain -- one image's large maps)
    const long long waves = tb * (sub ? 4 : 1);
    return (int32_t)(waves > 0x7fffffffLL ? 0x7fffffffLL : waves);
}

extern "C" int32_t mcq_conv2d_small_launch(int32_t N, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t ksize, int32_t stride,
                                           uint32_t flags, int32_t nprob) {
    return t16_takes(N, Cin, H, W, Cout, ksize, stride, flags, nprob) ? 1 : 0;
}

extern "C" int mcq_conv2d_multi_f32(const mcq_conv_desc* descs, int32_t n, void* stream) {
    if (!descs || n < 1 || n > MCQ_CONV_MAX_MULTI) return MCQ_EINVAL;
    for (int c = 0; c < n; ++c) {
        const int rc = conv_validate(descs + c);
        if (rc != MCQ_OK) return rc;
        const mcq_conv_desc &a = descs[0], &b = descs[c];
        if (a.N != b.N || a.Cin != b.Cin || a.H != b.H || a.W != b.W || a.Cout != b.Cout || a.ksize != b.ksize || a.stride != b.stride ||
            a.flags != b.flags || a.res_scale != b.res_scale || a.tile != b.tile || (a.bias == nullptr) != (b.bias == nullptr))
            return MCQ_EINVAL;                       // one geometry, one flag set, bias on all or none
    }
    return conv_launch(descs, n, stream);
}
