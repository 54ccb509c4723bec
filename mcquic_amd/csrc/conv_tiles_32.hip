// conv_mfma_kernel instances: the 32-row tiles.
#include "conv_tile_launch.h"

template int launch_tile<1, 4, 9, MCQ_PFB, 8>(ConvK, int, long long, int, int, hipStream_t, bool, bool, int);
template int launch_tile<1, 2, 9, MCQ_PFB, 8>(ConvK, int, long long, int, int, hipStream_t, bool, bool, int);
template int launch_tile<1, 1, 9, MCQ_PFB, 16>(ConvK, int, long long, int, int, hipStream_t, bool, bool, int);
