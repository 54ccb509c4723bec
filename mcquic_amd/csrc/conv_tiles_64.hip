// conv_mfma_kernel instances: the 64-row tiles.
#include "conv_tile_launch.h"

template int launch_tile<2, 2, 9, MCQ_PFB, 8>(ConvK, int, long long, int, int, hipStream_t, bool, bool, int);
template int launch_tile<2, 1, 9, MCQ_PFB, 16>(ConvK, int, long long, int, int, hipStream_t, bool, bool, int);
