// conv_mfma_kernel instances: the Winograd forms on the 32x32x2 instruction -- F(2, 3) along x (the seven hand-numbered 128-row
// instances and the 64-row one) and F(2x2, 3x3) (seven hand-numbered instances).
#include "conv_instances.h"

// Winograd F(2, 3) launches: one pair block (32 pairs of pixels) per wave, four waves per workgroup, no split-K
template <int MB>
int launch_wino(ConvK k, long long tiles, int co_tiles, hipStream_t s) {
    constexpr int OCC = MB == 4 ? 1 : 2;                   // 4 x MB accumulator tiles: 256 registers at MB = 4
    k.ks_log2 = 0;
    k.slice_pairs = k.S;
    k.tiles_log2 = 2;
    k.total_wgs = (int)((tiles + 3) >> 2);
    // MB = 4: one workgroup per CU is all that fits, so 256 * MCQ_WINO_PERSIST of them walk the tiles (a multiple of 8 keeps a
    // workgroup on one XCD's eighth of the image); MB = 2 launches a workgroup per four tiles as usual
    const unsigned gx = MB == 4 && MCQ_WINO_PERSIST > 0 && k.total_wgs > 256 * MCQ_WINO_PERSIST ? 256u * MCQ_WINO_PERSIST : (unsigned)k.total_wgs;
    const dim3 grid(gx, (unsigned)co_tiles, (unsigned)k.nprob);
    // activations run ~2.6 us ahead of their MFMAs (a step is MB MFMAs of 64 cycles): 24 steps at MB = 4, 48 at MB = 2
    if constexpr (MB == 4) {
        const unsigned ef = k.flags & ~(unsigned)(MCQ_CONV_SILU_IN | MCQ_CONV_SQUARE_IN);
        int id = 0;
        for (int c = 1; c <= 6; ++c) if (ef == wino_epilogue_flags(c)) id = c;
        switch (id) {
            case 1: hipLaunchKernelGGL((conv_mfma_kernel<4, 2, 1, 12, 24, 12, OCC>), grid, dim3(256), 0, s, k); break;
            case 2: hipLaunchKernelGGL((conv_mfma_kernel<4, 2, 2, 12, 24, 12, OCC>), grid, dim3(256), 0, s, k); break;
            case 3: hipLaunchKernelGGL((conv_mfma_kernel<4, 2, 3, 12, 24, 12, OCC>), grid, dim3(256), 0, s, k); break;
            case 4: hipLaunchKernelGGL((conv_mfma_kernel<4, 2, 4, 12, 24, 12, OCC>), grid, dim3(256), 0, s, k); break;
            case 5: hipLaunchKernelGGL((conv_mfma_kernel<4, 2, 5, 12, 24, 12, OCC>), grid, dim3(256), 0, s, k); break;
            case 6: hipLaunchKernelGGL((conv_mfma_kernel<4, 2, 6, 12, 24, 12, OCC>), grid, dim3(256), 0, s, k); break;
            default: hipLaunchKernelGGL((conv_mfma_kernel<4, 2, 0, 12, 24, 12, OCC>), grid, dim3(256), 0, s, k); break;
        }
    } else
        hipLaunchKernelGGL((conv_mfma_kernel<MB, 2, PRO_NONE, 12, MCQ_WINO_PFB2, 12, OCC>), grid, dim3(256), 0, s, k);
    return mcq_check_launch();
}
template int launch_wino<4>(ConvK, long long, int, hipStream_t);
template int launch_wino<2>(ConvK, long long, int, hipStream_t);

// F(2x2, 3x3) launches: one block of 32 tiles (2 x 2 pixels each) per workgroup, its four waves = four 32-row bands
int launch_wino2d(ConvK k, long long tiles, int co_groups, hipStream_t s) {
    k.ks_log2 = 0;
    k.slice_pairs = k.S;
    k.tiles_log2 = 0;
    k.total_wgs = (int)tiles;
    const unsigned gx = MCQ_WINO_PERSIST > 0 && k.total_wgs > 256 * MCQ_WINO_PERSIST ? 256u * MCQ_WINO_PERSIST : (unsigned)k.total_wgs;
    const dim3 grid(gx, (unsigned)co_groups, (unsigned)k.nprob);
    const unsigned ef = k.flags & ~(unsigned)(MCQ_CONV_SILU_IN | MCQ_CONV_SQUARE_IN);
    int id = 0;
    for (int c = 1; c <= 6; ++c) if (ef == wino_epilogue_flags(c)) id = c;
    switch (id) {
        case 1: hipLaunchKernelGGL((conv_mfma_kernel<1, 4, 1, 16, 32, 16, 1>), grid, dim3(256), 8192, s, k); break;
        case 2: hipLaunchKernelGGL((conv_mfma_kernel<1, 4, 2, 16, 32, 16, 1>), grid, dim3(256), 8192, s, k); break;
        case 3: hipLaunchKernelGGL((conv_mfma_kernel<1, 4, 3, 16, 32, 16, 1>), grid, dim3(256), 8192, s, k); break;
        case 4: hipLaunchKernelGGL((conv_mfma_kernel<1, 4, 4, 16, 32, 16, 1>), grid, dim3(256), 8192, s, k); break;
        case 5: hipLaunchKernelGGL((conv_mfma_kernel<1, 4, 5, 16, 32, 16, 1>), grid, dim3(256), 8192, s, k); break;
        case 6: hipLaunchKernelGGL((conv_mfma_kernel<1, 4, 6, 16, 32, 16, 1>), grid, dim3(256), 8192, s, k); break;
        default: hipLaunchKernelGGL((conv_mfma_kernel<1, 4, 0, 16, 32, 16, 1>), grid, dim3(256), 8192, s, k); break;
    }
    return mcq_check_launch();
}
