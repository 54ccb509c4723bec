// conv_mfma_kernel instances: the 128 x 32 tile (with the fused 1x1 layer, POST).
#include "conv_tile_launch.h"

template int launch_tile<4, 1, 9, MCQ_PFB, 8>(ConvK, int, long long, int, int, hipStream_t, bool, bool, int);
