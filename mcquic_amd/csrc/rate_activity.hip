// Adaptive quantisation: a content-driven rate map made on the device, for gfx950: plain stores, no atomics, no host read.  Equal inputs give
// equal bits, wherever the image stands in the batch.
//
//   activity_cells_kernel    x float32 [n, 3, H, W] -> a float32 [n, h0, w0], one value per level-0 code cell (16 x 16 pixels of the image
//                            reflect-padded to multiples of `base`, AlignedPadding's split: padTop = hPad / 2, padLeft = wPad / 2).  The
//                            kernel reads the unpadded image and reflects the index itself (i -> -i below 0, i -> 2 (H - 1) - i at or past
//                            H); no padded copy exists.  One wave per cell, four pixels of one row per lane (lane l: row l / 4, columns
//                            4 (l % 4) ..+3; one 128-bit load per channel where the four are inside the image and 16-byte aligned, four
//                            reflected loads else -- the same values either way).  Y = fmaf(0.114, B, fmaf(0.587, G, 0.299 R)); the lane's
//                            four are summed as (Y0 + Y1) + (Y2 + Y3), the 64 lanes by an xor butterfly (strides 1, 2, .. 32), so every sum
//                            is a balanced tree of depth 8 and a constant cell sums exactly.  Two passes, centred: mu = sum Y / 256,
//                            v = sum (Y - mu)^2 / 256, a = log2f(v + 2^-14).  A cell that holds a non-finite luma (or whose v overflows)
//                            gets a = 0, mask = 1 and sets error[image] = 1; `error` is zeroed by a memset node in front of the launch and
//                            every writer stores the same value.
//   activity_weights_kernel  one workgroup per image: abar = the mean of `a` over the unmasked cells -- thread t sums the t-th run of
//                            ceil(cells / 256) consecutive row-major cells in double, thread 0 adds the 256 partial sums in run order,
//                            divides in double and rounds once to float32 (0 when every cell is masked) -- then per cell
//                            e = clamp(strength (a - abar), -clip, +clip), w = exp2f(e) (1 for a masked cell) and
//                            out = (w * roi) * lam, roi absent (1), per image or per cell, lam absent (1) or per image.  A roi value that
//                            is negative, NaN or infinite is written as NaN: rate_map_levels_kernel counts that as 0 and reports it.
#include "mcq_common.h"
#include "../../include/mcquic_hip.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int AC_WAVES = 4;                   // cells per workgroup
constexpr int AW_T = 256;
typedef float act_f32x4 __attribute__((ext_vector_type(4)));      // (a vector type: the load stays one 128-bit instruction)

struct ActCellsK {
    const float* x;                           // [n, 3, H, W]
    float* a;                                 // [n, h0, w0]
    int32_t* mask;                            // [n, h0, w0]
    int32_t* error;                           // [n]
    int H, W, h0, w0, pad_top, pad_left;
    long long cells;                          // n h0 w0
};

__device__ __forceinline__ int act_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

__device__ __forceinline__ float act_wave_sum(float v) {
    for (int k = 1; k < 64; k <<= 1) v = v + __shfl_xor(v, k, 64);      // (both partners add the same two values: every lane holds the same bits)
    return v;
}

__global__ __launch_bounds__(AC_WAVES * 64) void activity_cells_kernel(ActCellsK p) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * AC_WAVES + (threadIdx.x >> 6);
    if (cell >= p.cells) return;              // (a whole wave)
    const int per = p.h0 * p.w0;
    const int img = (int)(cell / per);
    const int c = (int)(cell - (long long)img * per);
    const int cy = c / p.w0, cx = c - cy * p.w0;
    const int sy = act_reflect(16 * cy + (lane >> 2) - p.pad_top, p.H);
    const int x0 = 16 * cx + 4 * (lane & 3) - p.pad_left;
    const size_t plane = (size_t)p.H * p.W;
    const float* row = p.x + (size_t)img * 3 * plane + (size_t)sy * p.W;
    const bool inside = x0 >= 0 && x0 + 3 < p.W;
    float px[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* r = row + ch * plane;
        if (inside && ((uintptr_t)(r + x0) & 15) == 0) {
            const act_f32x4 v = *reinterpret_cast<const act_f32x4*>(r + x0);
            px[ch][0] = v[0]; px[ch][1] = v[1]; px[ch][2] = v[2]; px[ch][3] = v[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) px[ch][j] = r[act_reflect(x0 + j, p.W)];
        }
    }
    float y[4];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        y[j] = fmaf(0.114f, px[2][j], fmaf(0.587f, px[1][j], 0.299f * px[0][j]));
        bad = bad || !(fabsf(y[j]) <= FLT_MAX);
    }
    const float mu = act_wave_sum((y[0] + y[1]) + (y[2] + y[3])) * 0.00390625f;
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float d = y[j] - mu;
        q[j] = d * d;
    }
    const float v = act_wave_sum((q[0] + q[1]) + (q[2] + q[3])) * 0.00390625f;
    bad = bad || !(v <= FLT_MAX);
    const bool masked = __ballot(bad) != 0ull;
    if (lane == 0) {
        p.a[cell] = masked ? 0.0f : log2f(v + 0x1p-14f);
        p.mask[cell] = masked ? 1 : 0;
        if (masked) p.error[img] = 1;
    }
}

struct ActWeightsK {
    const float* a;                           // [n, h0, w0]
    const int32_t* mask;                      // [n, h0, w0]
    const float* roi;                         // or NULL: at roi[i * sn + y * sy + x * sx]
    long long sn, sy, sx;
    const float* lam;                         // or NULL: [n]
    float* out;                               // [n, h0, w0]
    int h0, w0;
    float strength, clip;
};

__global__ __launch_bounds__(AW_T) void activity_weights_kernel(ActWeightsK p) {
    __shared__ double s_sum[AW_T];
    __shared__ int s_cnt[AW_T];
    __shared__ float s_mean;
    const int img = blockIdx.x, t = threadIdx.x;
    const int cells = p.h0 * p.w0;
    const float* a = p.a + (size_t)img * cells;
    const int32_t* m = p.mask + (size_t)img * cells;
    {
        const int run = (cells + AW_T - 1) / AW_T;
        const long long lo = (long long)t * run;
        const int hi = (int)(lo + run < cells ? lo + run : cells);
        double s = 0.0;
        int cnt = 0;
        for (int c = (int)(lo < cells ? lo : cells); c < hi; ++c)
            if (!m[c]) { s = s + (double)a[c]; ++cnt; }
        s_sum[t] = s;
        s_cnt[t] = cnt;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        int cnt = 0;
        for (int i = 0; i < AW_T; ++i) { s = s + s_sum[i]; cnt += s_cnt[i]; }
        s_mean = cnt ? (float)(s / (double)cnt) : 0.0f;
    }
    __syncthreads();
    const float mean = s_mean;
    const float lam = p.lam ? p.lam[img] : 1.0f;
    float* out = p.out + (size_t)img * cells;
    for (int c = t; c < cells; c += AW_T) {
        float w = 1.0f;
        if (!m[c]) {
            const float e = p.strength * (a[c] - mean);
            w = exp2f(fminf(fmaxf(e, -p.clip), p.clip));
        }
        float r = 1.0f;
        if (p.roi) {
            const int y = c / p.w0, x = c - y * p.w0;
            r = p.roi[(long long)img * p.sn + (long long)y * p.sy + (long long)x * p.sx];
            if (!(r >= 0.0f) || isinf(r)) r = NAN;
        }
        out[c] = (w * r) * lam;
    }
}

}  // namespace

extern "C" int mcq_activity_cells_f32(const float* x, int32_t n, int32_t H, int32_t W, int32_t base, float* a, int32_t* mask,
                                      int32_t* error, void* stream) {
    if (!x || !a || !mask || !error || n <= 0 || H <= 0 || W <= 0 || base <= 0 || base % 16 != 0) return MCQ_EINVAL;
    const int64_t hpad = (base - H % base) % base, wpad = (base - W % base) % base;
    // reflect padding: each side's padding must be smaller than the image (the larger side is pad - pad / 2)
    if (hpad - hpad / 2 > (int64_t)H - 1 || wpad - wpad / 2 > (int64_t)W - 1) return MCQ_EINVAL;
    const int64_t h0 = ((int64_t)H + hpad) / 16, w0 = ((int64_t)W + wpad) / 16;
    if (h0 * w0 > 0x7fffffffLL || (int64_t)H + hpad > 0x7fffffffLL || (int64_t)W + wpad > 0x7fffffffLL) return MCQ_ETOOLARGE;
    const int64_t cells = (int64_t)n * h0 * w0, blocks = (cells + AC_WAVES - 1) / AC_WAVES;
    if (blocks > 0x7fffffffLL) return MCQ_ETOOLARGE;
    if (hipMemsetAsync(error, 0, (size_t)n * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return MCQ_ELAUNCH;
    ActCellsK p;
    p.x = x; p.a = a; p.mask = mask; p.error = error;
    p.H = H; p.W = W; p.h0 = (int)h0; p.w0 = (int)w0; p.pad_top = (int)(hpad / 2); p.pad_left = (int)(wpad / 2);
    p.cells = cells;
    hipLaunchKernelGGL(activity_cells_kernel, dim3((unsigned)blocks), dim3(AC_WAVES * 64), 0, (hipStream_t)stream, p);
    return mcq_check_launch();
}

extern "C" int mcq_activity_weights_f32(const float* a, const int32_t* mask, int32_t n, int32_t h0, int32_t w0, float strength, float clip,
                                        const float* roi, int64_t stride_n, int64_t stride_y, int64_t stride_x, const float* lam,
                                        float* out, void* stream) {
    if (!a || !mask || !out || n <= 0 || h0 <= 0 || w0 <= 0) return MCQ_EINVAL;
    if (!(strength >= 0.0f) || isinf(strength) || !(clip > 0.0f) || isinf(clip)) return MCQ_EINVAL;
    if (roi && (stride_n < 0 || stride_y < 0 || stride_x < 0)) return MCQ_EINVAL;
    if ((int64_t)h0 * w0 > 0x7fffffffLL) return MCQ_ETOOLARGE;
    ActWeightsK p;
    p.a = a; p.mask = mask; p.roi = roi; p.sn = stride_n; p.sy = stride_y; p.sx = stride_x; p.lam = lam; p.out = out;
    p.h0 = h0; p.w0 = w0; p.strength = strength; p.clip = clip;
    hipLaunchKernelGGL(activity_weights_kernel, dim3((unsigned)n), dim3(AW_T), 0, (hipStream_t)stream, p);
    return mcq_check_launch();
}
