// The small kernels around the per-vector-lambda assignment (vq_assign_kernel<.., RATE = true>, vq.hip), for gfx950: plain stores, no atomics, no
// host read.
//
//   vq_pack_bits_kernel    one level's 16-bit table uint32 [m, k + 1] -> the `bits` section [m][ntile + 1][64][4] in the layout of the
//                          packed codebook's norms (vq_norm_slot, vq_common.h): vq_table_bits for a codeword < k (+inf for a slot of
//                          width 0), 0 for padded codewords and the upper half-wave (the lanes whose MFMA operand is multiplied by 0).
//   rate_map_levels_kernel every level's lambda buffer from the caller's map in ONE launch, one workgroup per image.  Level 0 is the
//                          map with every negative, NaN or infinite value replaced by 0 (the image's error word says so); level l,
//                          cell (y, x), is the mean of the level-(l - 1) cells (2y .. 2y + 1, 2x .. 2x + 1) that exist -- summed in
//                          row-major order in float32, divided by their count -- on grids that halve with ceil, as the code grids do.
//                          The means are taken on the unscaled map; every level is multiplied by its scale at the end.  The per-image
//                          form (h0 = w0 = 0) only checks and scales.
//   rate_search_kernel     one thread per image: the bracket update of Compressor.encode_to_rate(per_image=True) after a trial, state
//                          and trace on the device (see mcq_rate_search_step in the header for the rule).
#include "mcq_common.h"
#include "vq_common.h"
#include "../../include/mcquic_hip.h"
#include <math.h>

namespace {

__global__ void vq_pack_bits_kernel(const uint32_t* __restrict__ cdf, int k, int ntile, float* __restrict__ out, size_t total) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const VqSlot s = vq_norm_slot(i, ntile);
    out[i] = !s.upper && s.tile < ntile && s.word < k ? vq_table_bits(cdf, s.g, k, s.word) : 0.0f;
}

struct RateMapK {
    const float* map;                         // [n] (h0 = 0) or the grid at map[i * sn + y * sy + x * sx]
    long long sn, sy, sx;
    int n, h0, w0, levels;
    float scale[MCQ_VQ_MAX_LEVELS];
    const float* scale_dev;                   // or NULL: [levels] on the device, taken instead of `scale`
    float* out[MCQ_VQ_MAX_LEVELS];            // level l: [n] or [n, h_l, w_l]
    int32_t* error;                           // [n]
};

constexpr int RM_T = 256;

__global__ __launch_bounds__(RM_T) void rate_map_levels_kernel(RateMapK p) {
    __shared__ int s_bad;
    const int img = blockIdx.x;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    if (p.h0 == 0) {
        if (threadIdx.x == 0) {
            float v = p.map[(long long)img * p.sn];
            if (!(v >= 0.0f) || isinf(v)) { v = 0.0f; bad = 1; }
            for (int l = 0; l < p.levels; ++l) p.out[l][img] = (p.scale_dev ? p.scale_dev[l] : p.scale[l]) * v;
            p.error[img] = bad;
        }
        return;
    }
    int h = p.h0, w = p.w0;
    {
        float* o = p.out[0] + (size_t)img * h * w;
        for (int c = threadIdx.x; c < h * w; c += RM_T) {
            const int y = c / w, x = c - y * w;
            float v = p.map[(long long)img * p.sn + (long long)y * p.sy + (long long)x * p.sx];
            if (!(v >= 0.0f) || isinf(v)) { v = 0.0f; bad = 1; }
            o[c] = v;
        }
    }
    if (bad) s_bad = 1;                        // (every writer stores the same value)
    for (int l = 1; l < p.levels; ++l) {
        __syncthreads();                       // level l - 1 of this image is written (by this workgroup alone)
        const int hp = h, wp = w;
        h = (h + 1) >> 1; w = (w + 1) >> 1;
        const float* prev = p.out[l - 1] + (size_t)img * hp * wp;
        float* o = p.out[l] + (size_t)img * h * w;
        for (int c = threadIdx.x; c < h * w; c += RM_T) {
            const int y = c / w, x = c - y * w;
            float s = 0.0f;
            int cnt = 0;
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) {
                    const int yy = 2 * y + dy, xx = 2 * x + dx;
                    if (yy < hp && xx < wp) { s = s + prev[yy * wp + xx]; ++cnt; }
                }
            o[c] = s / (float)cnt;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) p.error[img] = s_bad;
    h = p.h0; w = p.w0;
    for (int l = 0; l < p.levels; ++l) {
        const float sc = p.scale_dev ? p.scale_dev[l] : p.scale[l];
        float* o = p.out[l] + (size_t)img * h * w;
        for (int c = threadIdx.x; c < h * w; c += RM_T) o[c] = sc * o[c];
        h = (h + 1) >> 1; w = (w + 1) >> 1;
    }
}

struct RateSearchK {
    const double* bits;                       // [n, levels]: what the tables charge for the trial's codes (mcq_code_bits)
    const double* target;                     // [n] bits per pixel
    float* lam;                               // [n] in: the lambda the trial ran at; out: the next trial's (a finished image: its answer)
    float* bracket;                           // [n, 2] lo, hi
    int32_t* done;                            // [n]
    float* trace_lam;                         // or NULL: [trials + 1, n]
    double* trace_bpp;                        // or NULL: [trials + 1, n]
    double pixels;
    float lambda_max;
    int n, levels, trial, trials;
};

__global__ void rate_search_kernel(RateSearchK p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    double s = 0.0;
    for (int l = 0; l < p.levels; ++l) s = s + p.bits[(size_t)i * p.levels + l];
    const double bpp = s / p.pixels;
    const float tried = p.lam[i];
    if (p.trace_lam) p.trace_lam[(size_t)p.trial * p.n + i] = tried;
    if (p.trace_bpp) p.trace_bpp[(size_t)p.trial * p.n + i] = bpp;
    if (p.trial >= p.trials) return;          // the final run: recorded, nothing to decide
    const bool met = bpp <= p.target[i];
    float lo, hi;
    int done;
    if (p.trial == 0) {                       // lambda = 0 ran: this call also makes the state
        lo = 0.0f; hi = p.lambda_max;
        done = met ? 1 : 0;
        p.lam[i] = met ? 0.0f : hi;
        if (met) hi = 0.0f;                   // (the answer is `hi`)
    } else {
        lo = p.bracket[2 * i]; hi = p.bracket[2 * i + 1];
        done = p.done[i];
        if (!done) {
            if (p.trial == 1) {
                if (!met) done = 1;           // lambda_max misses: the image ends there and shows its bpp
            } else if (met) hi = tried;
            else lo = tried;
            if (!done) {
                float mid = hi;
                bool open = false;
                if (p.trial + 1 < p.trials) {
                    mid = lo == 0.0f ? (float)((double)hi / 16.0) : (float)sqrt((double)lo * (double)hi);
                    open = lo < mid && mid < hi;
                }
                if (open) p.lam[i] = mid;
                else { done = 1; p.lam[i] = hi; }
            }
        }
    }
    p.bracket[2 * i] = lo; p.bracket[2 * i + 1] = hi;
    p.done[i] = done;
}

}  // namespace

extern "C" size_t mcq_packed_bits_floats(int32_t m, int32_t k) {
    if (m <= 0 || k <= 0) return 0;
    return vq_pack_layout(m, k, 1).c2_total;
}

extern "C" int mcq_vq_pack_bits_f32(const uint32_t* cdf, int32_t m, int32_t k, float* bits_packed, void* stream) {
    if (!cdf || !bits_packed || m <= 0 || k <= 0) return MCQ_EINVAL;
    const VqPackLayout L = vq_pack_layout(m, k, 1);          // (the section is the norms': the same for every d)
    hipLaunchKernelGGL(vq_pack_bits_kernel, dim3((unsigned)((L.c2_total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cdf, k, L.ntile,
                       bits_packed, L.c2_total);
    return mcq_check_launch();
}

extern "C" int mcq_rate_map_levels_f32(const float* map, int32_t n, int32_t h0, int32_t w0, int64_t stride_n, int64_t stride_y,
                                       int64_t stride_x, const float* scales, const float* scales_dev, int32_t levels, float* const* out,
                                       int32_t* error, void* stream) {
    if (!map || !scales || !out || !error || n <= 0 || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return MCQ_EINVAL;
    if (h0 < 0 || w0 < 0 || (h0 == 0) != (w0 == 0) || stride_n < 0 || stride_y < 0 || stride_x < 0) return MCQ_EINVAL;
    if ((int64_t)h0 * w0 > 0x7fffffffLL) return MCQ_ETOOLARGE;
    RateMapK p;
    p.map = map; p.sn = stride_n; p.sy = stride_y; p.sx = stride_x;
    p.n = n; p.h0 = h0; p.w0 = w0; p.levels = levels;
    p.scale_dev = scales_dev; p.error = error;
    for (int l = 0; l < levels; ++l) {
        if (!out[l] || !(scales[l] >= 0.0f) || isinf(scales[l])) return MCQ_EINVAL;
        p.scale[l] = scales[l];
        p.out[l] = out[l];
    }
    hipLaunchKernelGGL(rate_map_levels_kernel, dim3((unsigned)n), dim3(RM_T), 0, (hipStream_t)stream, p);
    return mcq_check_launch();
}

extern "C" int mcq_rate_search_step(const double* bits, const double* target, float* lam, float* bracket, int32_t* done,
                                    float* trace_lam, double* trace_bpp, int32_t n, int32_t levels, double pixels, float lambda_max,
                                    int32_t trial, int32_t trials, void* stream) {
    if (!bits || !target || !lam || !bracket || !done || n <= 0 || levels <= 0) return MCQ_EINVAL;
    if (!(pixels > 0.0) || !(lambda_max > 0.0f) || isinf(lambda_max) || trials < 2 || trial < 0 || trial > trials) return MCQ_EINVAL;
    RateSearchK p;
    p.bits = bits; p.target = target; p.lam = lam; p.bracket = bracket; p.done = done;
    p.trace_lam = trace_lam; p.trace_bpp = trace_bpp;
    p.pixels = pixels; p.lambda_max = lambda_max;
    p.n = n; p.levels = levels; p.trial = trial; p.trials = trials;
    hipLaunchKernelGGL(rate_search_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p);
    return mcq_check_launch();
}
