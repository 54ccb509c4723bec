// launch_tile<MB, NB, ...>: every direct-form instance of one wave tile.  Included by the conv_tiles_*.hip, one explicit
// instantiation each.
#pragma once
#include "conv_instances.h"

template <int MB, int NB, int PF3A, int PF3B, int PF1>
int launch_tile(ConvK k, int pro, long long tiles, int co_tiles, int ksplit_log2, hipStream_t s, bool pair, bool lr4, int post) {
    // split-K: one 32-row band per owner wave (KS >= MB), whole channel pairs per slice, slices of >= 8 pairs of a
    // 3x3 conv (1x1 convs, 64 steps in all, are never split)
    if (ksplit_log2 > 0 && (1 << ksplit_log2) < MB) ksplit_log2 = MB == 4 ? 2 : 1;
    if (k.ks == 1) ksplit_log2 = 0;
    while (ksplit_log2 > 0 && (k.S % (1 << ksplit_log2) != 0 || (k.S >> ksplit_log2) < 8)) --ksplit_log2;
    if ((1 << ksplit_log2) < MB) ksplit_log2 = 0;
    constexpr int OCC = (MB == 2 && NB == 2) ? 3 : 2;      // waves per SIMD the register budget is sized for
    k.ks_log2 = ksplit_log2;
    k.slice_pairs = k.S >> ksplit_log2;
    k.tiles_log2 = ksplit_log2 >= 2 ? 0 : 2 - ksplit_log2;           // 4 waves per workgroup, 8 for 8-way split
    const int waves = 1 << (k.ks_log2 + k.tiles_log2);
    const size_t lds = ksplit_log2 ? (size_t)waves * NB * 1024 * sizeof(float) : 0;
    const dim3 grid((unsigned)((tiles + (1 << k.tiles_log2) - 1) >> k.tiles_log2), (unsigned)co_tiles, (unsigned)k.nprob);
    const dim3 block(64 * waves);
    // (round 4, measured and removed: `s_setprio 2` for the first-dispatched workgroup of every CU in single-round launches, so that
    //  one of the two waves of a SIMD finishes its k-loop early and its epilogue runs under the other's MFMAs -- the captured
    //  training step 22.32 vs 22.34 ms, the 32-image step 123.3 vs 123.4 ms: two epilogues side by side cost what one does)
    if (post) {             // the following 1x1 layer inside the launch (MCQ_CONV_POST_*): unsplit 128-row tiles only
        if constexpr (MB == 4 && NB == 1) {
            if (ksplit_log2 != 0 || k.ks != 3 || pair || lr4 || k.nprob != 1 || (pro != PRO_NONE && pro != PRO_SILU)) return MCQ_EINVAL;
            dim3 pgrid = grid, pblock = block;
            if (k.post_sub) { k.tiles_log2 = 0; pgrid = dim3((unsigned)tiles, 1u, 1u); pblock = dim3(256); }   // one pixel tile per workgroup, its four waves = the four row tiles
            if (post == 1 && pro == PRO_NONE) hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_NONE, PF3A, PF3B, 9, OCC, false, 1>), pgrid, pblock, 0, s, k);
            else if (post == 1) hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_SILU, PF3A, PF3B, 9, OCC, false, 1>), pgrid, pblock, 0, s, k);
            else if (pro == PRO_NONE) hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_NONE, PF3A, PF3B, 9, OCC, false, 2>), pgrid, pblock, 0, s, k);
            else hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_SILU, PF3A, PF3B, 9, OCC, false, 2>), pgrid, pblock, 0, s, k);
            return mcq_check_launch();
        }
        return MCQ_EINVAL;
    }
    if (pair) {
        if constexpr (MB == 4 && NB == 2) {
            if (ksplit_log2 != 0 || pro != PRO_NONE || k.ks != 3) return MCQ_EINVAL;
            hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_NONE, PF3A, PF3B, 9, OCC, true>), grid, block, lds, s, k);
            return mcq_check_launch();
        }
        return MCQ_EINVAL;
    }
    if (lr4) {              // (the rings in live steps: weights 8 ahead, activations 16 = four channel pairs)
        if (pro != PRO_NONE || k.ks != 3) return MCQ_EINVAL;
        hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_NONE, 8, 16, 4, OCC>), grid, block, lds, s, k);
        return mcq_check_launch();
    }
    if (k.ks == 3) {
        if (pro == PRO_SILU) hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_SILU, PF3A, PF3B, 9, OCC>), grid, block, lds, s, k);
        else if (pro == PRO_NONE) hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_NONE, PF3A, PF3B, 9, OCC>), grid, block, lds, s, k);
        else return MCQ_EINVAL;
    } else {
        if (pro == PRO_SQUARE) hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_SQUARE, PF1, PF1, 1, OCC>), grid, block, lds, s, k);
        else if (pro == PRO_NONE) hipLaunchKernelGGL((conv_mfma_kernel<MB, NB, PRO_NONE, PF1, PF1, 1, OCC>), grid, block, lds, s, k);
        else return MCQ_EINVAL;
    }
    return mcq_check_launch();
}
