// conv_mfma_kernel instances: the 128 x 64 tile (with its pair and four-tap instances).
#include "conv_tile_launch.h"

template int launch_tile<4, 2, MCQ_PF42A, MCQ_PF42B, 4>(ConvK, int, long long, int, int, hipStream_t, bool, bool, int);
