// The launch functions of the conv_mfma_kernel instances.  Each is defined and explicitly instantiated in exactly one
// conv_tiles_*.hip / conv_wino32.hip, so that the instances compile side by side and conv_launch.hip, which only calls them, holds none.
#pragma once
#include "conv_mfma_kernel.h"

// direct form, MB x NB tiles of 32 output channels x 32 pixels per wave (conv_tile_launch.h)
template <int MB, int NB, int PF3A, int PF3B, int PF1>
int launch_tile(ConvK k, int pro, long long tiles, int co_tiles, int ksplit_log2, hipStream_t s, bool pair = false, bool lr4 = false, int post = 0);
// Winograd F(2, 3) along x, MB = 4 / 2, and F(2x2, 3x3) (conv_wino32.hip)
template <int MB>
int launch_wino(ConvK k, long long tiles, int co_tiles, hipStream_t s);
int launch_wino2d(ConvK k, long long tiles, int co_groups, hipStream_t s);
