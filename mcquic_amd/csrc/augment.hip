// The training input pipeline on the device (mcquic/data/transforms.py:14-21, 37-43; mcquic/utils/vision.py:85-129, 150-197;
// the reference runs the crop in its loader and the rest through in-place ops that land on copies) for gfx950, two launches:
//
//   mcq_augment_draw      ONE workgroup, a thread per image: every random decision of the pipeline into a table [N, 16] float32
//                         (MCQ_AUG_* columns of include/mcquic_hip.h) from {seed, offset} in device memory -- rng_uniform of
//                         mcq_rng.h, stream 16 + k for the k-th decision of image n -- and offset += 1, so a replayed hipGraph
//                         draws fresh parameters without the host.  The box rule (torchvision's RandomResizedCrop: ten attempts,
//                         then the central crop with the aspect clamped) runs in float64.
//   mcq_augment_f32/_u8   resample of the box to [H, W] (the separable triangle filter of F.interpolate(mode="bilinear",
//                         antialias=True, align_corners=False): support max(in / out, 1) per axis, weights normalised per output
//                         pixel, taps clipped to the box) -> gamma -> colour gain + clamp -> flips -> (v - 0.5) / 0.5
//                         (MCQ_AUG_OUTPUT of the row: a half of the pipeline leaves the clamp and / or the normalisation out).
//
// The pass moves the source box once and 4 N 3 H W bytes of output.  A workgroup owns a tile of 64 VEC output columns by TR rows
// of one image; VEC = 4 where W % 4 == 0 (a lane owns four adjacent pixels of a row and stores 16 bytes per channel), else 1.
// The taps of the tile's columns and rows -- first source index, count, normalised weights -- are computed ONCE per workgroup, in
// float64 (a float32 `center = scale (i + 0.5)` is off by 3e-5 of a pixel at 512 columns: more than the whole error budget),
// rounded to float32 and kept in LDS: tap-major for the columns, so lanes read consecutive words; the row taps are wave-uniform
// broadcasts.  The three channels of a pixel run through the same lanes with the same weights.  A flip is an index map on the
// OUTPUT coordinate: the tile's taps are those of column W - 1 - x (row H - 1 - y), so the loads run backwards and the stores
// stay forward runs.  Whatever the table holds, the box is clamped into the source before any address is formed.
#include "mcq_common.h"
#include "mcq_rng.h"
#include "../../include/mcquic_hip.h"
#include <math.h>

namespace {

constexpr int AUG_COLS = MCQ_AUG_COLUMNS;
constexpr int AUG_MAX_DIM = 1 << 24;                         // sizes and offsets travel as float32 in the table
constexpr unsigned AUG_MAX_LDS = 64u * 1024u;

struct AugDraw {
    int N, Hs, Ws, crop, gamma, T, output;
    double scale_lo, scale_hi, log_ratio_lo, log_ratio_hi, ratio_lo, ratio_hi;
    const float* coeffs;                                     // [T, 2] or null
    float p_gain, p_hflip, p_vflip;
};

__device__ __forceinline__ int aug_randint(float u, int n) {  // uniform over [0, n)
    const int v = (int)((double)u * (double)n);
    return v < n ? v : n - 1;
}

__global__ __launch_bounds__(256) void augment_draw_kernel(unsigned long long* st, float* __restrict__ tab, AugDraw q) {
    const RngState rng = rng_load(st);
    __syncthreads();                                         // every thread holds the state before the offset moves
    if (threadIdx.x == 0) st[1] = st[1] + 1ull;
    for (int n = threadIdx.x; n < q.N; n += blockDim.x) {
        auto u = [&](uint32_t k) { return rng_uniform(rng, 16u + k, (size_t)n); };
        int top = 0, left = 0, h = q.Hs, w = q.Ws, fallback = 0;
        if (q.crop) {
            bool found = false;
            for (uint32_t a = 0; a < 10u && !found; ++a) {
                const double area = (double)q.Hs * (double)q.Ws * (q.scale_lo + (double)u(2u * a) * (q.scale_hi - q.scale_lo));
                const double ar = exp(q.log_ratio_lo + (double)u(2u * a + 1u) * (q.log_ratio_hi - q.log_ratio_lo));
                const int cw = (int)rint(sqrt(area * ar)), ch = (int)rint(sqrt(area / ar));
                if (0 < cw && cw <= q.Ws && 0 < ch && ch <= q.Hs) {
                    w = cw; h = ch;
                    top = aug_randint(u(20u), q.Hs - h + 1);
                    left = aug_randint(u(21u), q.Ws - w + 1);
                    found = true;
                }
            }
            if (!found) {                                    // the central crop, aspect clamped into [ratio_lo, ratio_hi]
                fallback = 1;
                const double in_ratio = (double)q.Ws / (double)q.Hs;
                if (in_ratio < q.ratio_lo) { w = q.Ws; h = (int)rint((double)w / q.ratio_lo); }
                else if (in_ratio > q.ratio_hi) { h = q.Hs; w = (int)rint((double)h * q.ratio_hi); }
                h = h < 1 ? 1 : (h > q.Hs ? q.Hs : h);
                w = w < 1 ? 1 : (w > q.Ws ? q.Ws : w);
                top = (q.Hs - h) / 2;
                left = (q.Ws - w) / 2;
            }
        }
        int mode = MCQ_AUG_GAMMA_IDENTITY;
        float g = 1.0f;
        if (q.gamma) {
            mode = aug_randint(u(22u), 4);
            if (mode == MCQ_AUG_GAMMA_POWER) g = 0.05f + 1.95f * u(23u);
        }
        float gain0 = 1.0f, gain2 = 1.0f;
        int row = -1;
        if (q.coeffs && q.T > 0 && u(24u) < q.p_gain) {
            row = aug_randint(u(25u), q.T);
            gain0 = q.coeffs[2 * row];
            gain2 = q.coeffs[2 * row + 1];
        }
        float* p = tab + (size_t)n * AUG_COLS;
        p[MCQ_AUG_TOP] = (float)top; p[MCQ_AUG_LEFT] = (float)left; p[MCQ_AUG_H] = (float)h; p[MCQ_AUG_W] = (float)w;
        p[MCQ_AUG_GAMMA_MODE] = (float)mode; p[MCQ_AUG_GAMMA] = g;
        p[MCQ_AUG_GAIN0] = gain0; p[MCQ_AUG_GAIN2] = gain2;
        p[MCQ_AUG_HFLIP] = u(26u) < q.p_hflip ? 1.0f : 0.0f;
        p[MCQ_AUG_VFLIP] = u(27u) < q.p_vflip ? 1.0f : 0.0f;
        p[MCQ_AUG_GAIN_ROW] = (float)row;
        p[MCQ_AUG_FALLBACK] = (float)fallback;
        p[MCQ_AUG_OUTPUT] = (float)q.output;
        for (int k = MCQ_AUG_OUTPUT + 1; k < AUG_COLS; ++k) p[k] = 0.0f;
    }
}

// ---- the pass ------------------------------------------------------------------------------------------------------------
struct AugK {
    int N, Hs, Ws, H, W;
    int KX, KY;                  // tap slots per column / row in LDS (bounds for any box inside the source)
    int TR;                      // output rows per workgroup
};

// Taps of output index `o` of an axis that maps `in` source samples (the box) to `out`: ATen's antialiased linear filter.
// wts[k * stride], k < K: the normalised weights, zero past the count.  Returns the first source index; *count = the taps.
__device__ __forceinline__ int aug_taps(int o, int in, int out, int K, float* wts, int stride, int* count) {
    const double scale = (double)in / (double)out;
    const double support = scale >= 1.0 ? scale : 1.0;
    const double invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    const double center = scale * ((double)o + 0.5);
    int lo = (int)(center - support + 0.5);
    lo = lo < 0 ? 0 : lo;
    int hi = (int)(center + support + 0.5);
    hi = hi > in ? in : hi;
    int size = hi - lo;
    size = size > K ? K : size;
    double total = 0.0;
    for (int j = 0; j < size; ++j) {
        const double t = fabs(((double)(j + lo) - center + 0.5) * invscale);
        total += t < 1.0 ? 1.0 - t : 0.0;
    }
    for (int j = 0; j < K; ++j) {
        const double t = fabs(((double)(j + lo) - center + 0.5) * invscale);
        const double wv = t < 1.0 ? 1.0 - t : 0.0;
        wts[j * stride] = (j < size && total != 0.0) ? (float)(wv / total) : 0.0f;
    }
    *count = size;
    return lo;
}

__device__ __forceinline__ int aug_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float aug_gamma(float x, int mode, float g) {
    if (mode == MCQ_AUG_GAMMA_SRGB_TO_LINEAR)                // (the reference's naming, utils/vision.py:108-109)
        return x < 0.0031308f ? 12.92f * x : 1.055f * powf(fabsf(x), 1.0f / 2.4f) - 0.055f;
    if (mode == MCQ_AUG_GAMMA_LINEAR_TO_SRGB)
        return x < 0.04045f ? x / 12.92f : powf(fabsf(x + 0.055f) / 1.055f, 2.4f);
    if (mode == MCQ_AUG_GAMMA_POWER)
        return fminf(fmaxf(powf(fmaxf(x, 0.0f), g), 0.0f), 1.0f);
    return x;
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void augment_kernel(const T* __restrict__ src, const float* __restrict__ tab, float* __restrict__ out, AugK q) {
    constexpr int CT = 64 * VEC;                             // output columns of a tile
    extern __shared__ float smem[];
    float* wx = smem;                                        // [KX][CT]
    int* xfirst = reinterpret_cast<int*>(wx + q.KX * CT);    // [CT]
    float* wy = reinterpret_cast<float*>(xfirst + CT);       // [TR][KY]
    int* yfirst = reinterpret_cast<int*>(wy + q.TR * q.KY);  // [TR]
    int* ycount = yfirst + q.TR;                             // [TR]

    const int n = blockIdx.z, tid = threadIdx.x;
    const float* p = tab + (size_t)n * AUG_COLS;
    const int bh = aug_clampi((int)p[MCQ_AUG_H], 1, q.Hs), bw = aug_clampi((int)p[MCQ_AUG_W], 1, q.Ws);
    const int top = aug_clampi((int)p[MCQ_AUG_TOP], 0, q.Hs - bh), left = aug_clampi((int)p[MCQ_AUG_LEFT], 0, q.Ws - bw);
    const int mode = (int)p[MCQ_AUG_GAMMA_MODE];
    const float g = p[MCQ_AUG_GAMMA], gain0 = p[MCQ_AUG_GAIN0], gain2 = p[MCQ_AUG_GAIN2];
    const bool hflip = p[MCQ_AUG_HFLIP] != 0.0f, vflip = p[MCQ_AUG_VFLIP] != 0.0f;
    const int output = (int)p[MCQ_AUG_OUTPUT];
    const int x0 = blockIdx.x * CT, y0 = blockIdx.y * q.TR;

    if (tid < CT) {
        const int x = x0 + tid < q.W ? x0 + tid : q.W - 1;
        int cnt;
        xfirst[tid] = aug_taps(hflip ? q.W - 1 - x : x, bw, q.W, q.KX, wx + tid, CT, &cnt);
    }
    if (tid < q.TR) {
        const int y = y0 + tid < q.H ? y0 + tid : q.H - 1;
        int cnt;
        yfirst[tid] = aug_taps(vflip ? q.H - 1 - y : y, bh, q.H, q.KY, wy + tid * q.KY, 1, &cnt);
        ycount[tid] = cnt;
    }
    __syncthreads();

    // column taps any output column of this box can have (floor(2 support) + 1), inside the slots the host sized for the source
    const double sx = (double)bw / (double)q.W;
    int kx = (int)(2.0 * (sx >= 1.0 ? sx : 1.0)) + 1;
    kx = kx > q.KX ? q.KX : kx;

    const int wave = tid >> 6, col = (tid & 63) * VEC;
    if (x0 + col >= q.W) return;                             // (no barrier below)
    int xf[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) xf[v] = xfirst[col + v];
    const size_t plane = (size_t)q.Hs * q.Ws;
    const T* img = src + (size_t)n * 3 * plane;

    for (int r = wave; r < q.TR; r += 4) {
        const int y = y0 + r;
        if (y >= q.H) break;
        const int yf = yfirst[r], yc = ycount[r];
        float acc[3][VEC];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[c][v] = 0.0f;
        for (int j = 0; j < yc; ++j) {
            const int sy = top + (yf + j < bh ? yf + j : bh - 1);
            const T* row = img + (size_t)sy * q.Ws + left;
            float rr[3][VEC];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v) rr[c][v] = 0.0f;
            for (int i = 0; i < kx; ++i) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float w = wx[i * CT + col + v];
                    const int sxi = xf[v] + i < bw ? xf[v] + i : bw - 1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) rr[c][v] = __builtin_fmaf(w, (float)row[c * plane + sxi], rr[c][v]);
                }
            }
            const float wj = wy[r * q.KY + j];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[c][v] = __builtin_fmaf(wj, rr[c][v], acc[c][v]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gain = c == 0 ? gain0 : (c == 2 ? gain2 : 1.0f);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                float t = acc[c][v];
                if (sizeof(T) == 1) t = t / 255.0f;          // ToTensor's v / 255, once per pixel: the filter is linear
                t = aug_gamma(t, mode, g);
                t = t * gain;
                if (output != MCQ_AUG_OUT_RAW) t = fminf(fmaxf(t, 0.0f), 1.0f);
                acc[c][v] = output == MCQ_AUG_OUT_NORMALIZED ? (t - 0.5f) / 0.5f : t;
            }
            float* o = out + (((size_t)n * 3 + c) * q.H + y) * q.W + x0 + col;
            if (VEC == 4) *reinterpret_cast<f32x4v*>(o) = f32x4v{acc[c][0], acc[c][1], acc[c][2], acc[c][3]};
            else o[0] = acc[c][0];
        }
    }
}

template <typename T>
int augment_launch(const T* src, const float* params, float* out, int N, int Hs, int Ws, int H, int W, void* stream) {
    if (!src || !params || !out || N <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return MCQ_EINVAL;
    if (N > 65535 || Hs > AUG_MAX_DIM || Ws > AUG_MAX_DIM || H > AUG_MAX_DIM || W > AUG_MAX_DIM) return MCQ_ETOOLARGE;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const int CT = vec ? 256 : 64;
    AugK q;
    q.N = N; q.Hs = Hs; q.Ws = Ws; q.H = H; q.W = W;
    const double sx = (double)Ws / W, sy = (double)Hs / H;
    q.KX = (int)(2.0 * (sx >= 1.0 ? sx : 1.0)) + 2;
    q.KY = (int)(2.0 * (sy >= 1.0 ? sy : 1.0)) + 2;
    const long long col_tiles = (W + CT - 1) / CT;
    q.TR = 16;                                               // fewer rows per workgroup until the launch has ~4 workgroups per CU
    while (q.TR > 4 && col_tiles * ((H + q.TR - 1) / q.TR) * N < 1024) q.TR /= 2;
    const long long row_tiles = (H + q.TR - 1) / q.TR;
    const size_t lds = ((size_t)q.KX * CT + CT + (size_t)q.TR * q.KY + 2 * (size_t)q.TR) * 4;
    if (lds > AUG_MAX_LDS || row_tiles > 65535) return MCQ_ETOOLARGE;     // (a reduction by more than ~30x per axis)
    const dim3 grid((unsigned)col_tiles, (unsigned)row_tiles, (unsigned)N);
    if (vec) hipLaunchKernelGGL((augment_kernel<T, 4>), grid, dim3(256), lds, (hipStream_t)stream, src, params, out, q);
    else hipLaunchKernelGGL((augment_kernel<T, 1>), grid, dim3(256), lds, (hipStream_t)stream, src, params, out, q);
    return mcq_check_launch();
}

}  // namespace

extern "C" int mcq_augment_draw(uint64_t* rng_state, float* params, int32_t N, int32_t Hs, int32_t Ws, int32_t crop, double scale_lo,
                                double scale_hi, double ratio_lo, double ratio_hi, int32_t gamma, const float* coeffs, int32_t T,
                                float p_gain, float p_hflip, float p_vflip, int32_t output, void* stream) {
    if (!rng_state || !params || N <= 0 || Hs <= 0 || Ws <= 0 || Hs > AUG_MAX_DIM || Ws > AUG_MAX_DIM || T < 0) return MCQ_EINVAL;
    if (output < MCQ_AUG_OUT_NORMALIZED || output > MCQ_AUG_OUT_RAW) return MCQ_EINVAL;
    if (crop && !(0.0 < scale_lo && scale_lo <= scale_hi && 0.0 < ratio_lo && ratio_lo <= ratio_hi)) return MCQ_EINVAL;
    if (coeffs && T > AUG_MAX_DIM) return MCQ_EINVAL;
    AugDraw q;
    q.N = N; q.Hs = Hs; q.Ws = Ws; q.crop = crop; q.gamma = gamma; q.T = coeffs ? T : 0; q.output = output;
    q.scale_lo = scale_lo; q.scale_hi = scale_hi; q.ratio_lo = ratio_lo; q.ratio_hi = ratio_hi;
    q.log_ratio_lo = crop ? log(ratio_lo) : 0.0; q.log_ratio_hi = crop ? log(ratio_hi) : 0.0;
    q.coeffs = coeffs; q.p_gain = p_gain; q.p_hflip = p_hflip; q.p_vflip = p_vflip;
    hipLaunchKernelGGL(augment_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<unsigned long long*>(rng_state), params, q);
    return mcq_check_launch();
}

extern "C" int mcq_augment_f32(const float* src, const float* params, float* out, int32_t N, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                               void* stream) {
    return augment_launch<float>(src, params, out, N, Hs, Ws, H, W, stream);
}

extern "C" int mcq_augment_u8(const uint8_t* src, const float* params, float* out, int32_t N, int32_t Hs, int32_t Ws, int32_t H, int32_t W,
                              void* stream) {
    return augment_launch<uint8_t>(src, params, out, N, Hs, Ws, H, W, stream);
}
