// MS-SSIM as a differentiable float32 training loss (the distortion term of the reference's training configs: `target: MsSSIM`,
// mcquic/loss/__init__.py:47-55 -> mcquic/validate/metrics.py:69-104, 142-193 with data range 2.0 on restored + 1, image + 1), gfx950.
//
//   mcq_ms_ssim_loss_f32      loss = 1 - mean_{n,c} prod_l relu(v_l)^w_l of X = a + offset, Y = b + offset; the per-(level, image,
//                             channel) map means v[5][N][C] and the pooled pyramids of levels 1..4 ("saved") for the backward.
//   mcq_ms_ssim_loss_bwd_f32  da (and db) from v, the saved pyramids and dloss, levels coarse to fine.
//
// Forward: per level one tiled blur + map-mean launch (the tiling of ssim_level_kernel in metrics.hip: a 16 x 118 map tile from a
// 26 x 128 input patch in LDS, the vertical pass in registers, the horizontal pass from five moment planes in LDS), one finish
// launch (tile partials -> means, float64 in tile order) and, below the last level, one 2x2 pooling launch.  fp32 operations follow
// oracle/metrics_ref.py's order (taps in index order, -ffp-contract=off); the means are float64 in a fixed order.
//
// Backward: dL/dv from v and dloss (explicit product form, 0 where v <= 0), then per level, coarse to fine:
//   grad-maps   recompute the five blurred moments on the same tiles as the forward and write the pointwise gradients of the
//               level's map (cs below the last level, ssim on it), scaled by dL/dv / (Ho Wo), with respect to mu_x, E[x^2], E[xy]
//               (and mu_y, E[y^2] when db is wanted) to workspace planes;
//   grad-input  the transposed blur of those planes (the window is symmetric: a 'full' correlation with the same taps, i.e. a
//               valid one over the zero-extended map) and dx_l = B'g_mu + 2x B'g_xx + y B'g_xy + pool_adjoint(dx_{l+1}); once for
//               x and, when db is wanted, once more with the roles of x and y swapped.
// Nothing is allocated, nothing is read back by the host, no memset, no atomics: safe inside a captured hipGraph and bitwise
// deterministic.
#include "mcq_common.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int TH = 16, TW = 118, IH = TH + 10, IW = 128;

// the 11 float32 taps of metrics.py:22-37 (size 11, sigma 1.5) and the level weights of metrics.py:19 (same values as metrics.hip)
__constant__ float c_win[11] = {0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f};
__constant__ float c_level_w[5] = {0x1.6f0068p-5f, 0x1.247454p-2f, 0x1.334d6ap-2f, 0x1.e3f142p-3f, 0x1.10ff98p-3f};

// Blur of NQ planes over one tile.  The NQ source planes of the 26 x 128 patch are in smem[q][IH][IW] (q < NSRC; the moments
// x, y, x^2, y^2, xy are formed from the first two when MOMENTS); on return sv[k][TH][IW + 1] holds the vertical pass of each of
// the NQ quantities, over the same bytes.
template <int NQ, bool MOMENTS>
__device__ __forceinline__ void vertical_pass(float* smem) {
    constexpr int NSRC = MOMENTS ? 2 : NQ;
    const int tid = threadIdx.x;
    const int c = tid & (IW - 1), rg = tid >> 7;
    float a[NQ][8];
#pragma unroll
    for (int t = 0; t < 18; ++t) {
        float q[NQ];
        if constexpr (MOMENTS) {
            const float x = smem[(rg * 8 + t) * IW + c], y = smem[IH * IW + (rg * 8 + t) * IW + c];
            q[0] = x; q[1] = y; q[2] = x * x; q[3] = y * y; q[4] = x * y;
        } else {
#pragma unroll
            for (int k = 0; k < NSRC; ++k) q[k] = smem[k * IH * IW + (rg * 8 + t) * IW + c];
        }
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const int tap = t - o;
            if (tap >= 0 && tap < 11) {
#pragma unroll
                for (int k = 0; k < NQ; ++k) a[k][o] = tap == 0 ? c_win[0] * q[k] : a[k][o] + c_win[tap] * q[k];
            }
        }
    }
    __syncthreads();                     // every strip is in registers: the patches may be overwritten
#pragma unroll
    for (int k = 0; k < NQ; ++k)
#pragma unroll
        for (int o = 0; o < 8; ++o) smem[(k * TH + rg * 8 + o) * (IW + 1) + c] = a[k][o];
    __syncthreads();
}

template <int NQ>
__device__ __forceinline__ void horizontal(const float* smem, int r, int c, float* f) {
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const float* row = smem + (k * TH + r) * (IW + 1) + c;
        float acc = c_win[0] * row[0];
#pragma unroll
        for (int t = 1; t < 11; ++t) acc = acc + c_win[t] * row[t];
        f[k] = acc;
    }
}

// the 26 x 128 patch of X + off and Y + off at (r0, c0), zeros outside the image
__device__ __forceinline__ void load_pair(float* smem, const float* xp, const float* yp, float off, int H, int W, int r0, int c0) {
    for (int i = threadIdx.x; i < IH * IW; i += 256) {
        const int r = i >> 7, c = i & (IW - 1);
        const int gr = r0 + r, gc = c0 + c;
        const bool ok = gr < H && gc < W;
        const size_t o = (size_t)gr * W + gc;
        smem[i] = ok ? xp[o] + off : 0.0f;
        smem[IH * IW + i] = ok ? yp[o] + off : 0.0f;
    }
    __syncthreads();
}

constexpr int SMEM_FLOATS = 5 * TH * (IW + 1);
static_assert(2 * IH * IW <= SMEM_FLOATS && 3 * IH * IW <= SMEM_FLOATS, "patches fit under the moment planes");

// forward, one level: tile partial (float64) of the cs map (levels 0..3) or of the ssim map (last level)
__global__ __launch_bounds__(256) void msl_level_kernel(const float* __restrict__ X, const float* __restrict__ Y, float off, int H,
                                                        int W, int Ho, int Wo, float C1, float C2, int last,
                                                        double* __restrict__ partial) {
    __shared__ float smem[SMEM_FLOATS];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const size_t plane = blockIdx.z;
    const int r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
    load_pair(smem, X + plane * (size_t)H * W, Y + plane * (size_t)H * W, off, H, W, r0, c0);
    vertical_pass<5, true>(smem);

    double s = 0.0;
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int r = idx / TW, c = idx - r * TW;
        float f[5];
        horizontal<5>(smem, r, c, f);
        const float mu1_sq = f[0] * f[0], mu2_sq = f[1] * f[1], mu12 = f[0] * f[1];
        const float s1 = f[2] - mu1_sq, s2 = f[3] - mu2_sq, s12 = f[4] - mu12;
        const float cs = (2.0f * s12 + C2) / (s1 + s2 + C2);
        const float v = last ? ((2.0f * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs : cs;
        if (r0 + r < Ho && c0 + c < Wo) s += (double)v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const size_t ntile = (size_t)gridDim.x * gridDim.y;
        partial[plane * ntile + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// per plane: tile partials in tile order -> the level's map mean
__global__ void msl_finish_kernel(const double* __restrict__ partial, int planes, int ntile, double count, float* __restrict__ v) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= planes) return;
    double a = 0.0;
    const double* q = partial + (size_t)p * ntile;
    for (int t = 0; t < ntile; ++t) a += q[t];
    v[p] = (float)(a / count);
}

// metrics.py:177-179 on X + off: avg_pool2d(kernel 2, stride 2, padding = side % 2), padded zeros counted in the divisor
__global__ void msl_halve_kernel(const float* __restrict__ X, const float* __restrict__ Y, float off, float* __restrict__ Xo,
                                 float* __restrict__ Yo, int H, int W, int Ho, int Wo, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int xo = (int)(i % Wo);
    const size_t t = i / Wo;
    const int yo = (int)(t % Ho);
    const size_t plane = t / Ho;
    const int y0 = 2 * yo - (H & 1), x0 = 2 * xo - (W & 1);
    const float* xp = X + plane * (size_t)H * W;
    const float* yp = Y + plane * (size_t)H * W;
    float vx[4], vy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
        const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const size_t o = (size_t)yy * W + xx;
        vx[k] = ok ? xp[o] + off : 0.0f;
        vy[k] = ok ? yp[o] + off : 0.0f;
    }
    Xo[i] = (((vx[0] + vx[1]) + vx[2]) + vx[3]) / 4.0f;
    Yo[i] = (((vy[0] + vy[1]) + vy[2]) + vy[3]) / 4.0f;
}

// metrics.py:184-193 with sizeAverage: 1 - mean over (image, channel) of prod_l relu(v_l)^w_l (one workgroup: strided float64
// sums per thread, then a fixed tree -- the same order every run)
__global__ __launch_bounds__(256) void msl_combine_kernel(const float* __restrict__ v, int planes, float* __restrict__ loss) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double sum = 0.0;
    for (int p = tid; p < planes; p += 256) {
        float prod = 1.0f;
        for (int l = 0; l < 5; ++l) {
            const float pw = powf(fmaxf(v[(size_t)l * planes + p], 0.0f), c_level_w[l]);
            prod = l == 0 ? pw : prod * pw;
        }
        sum += (double)prod;
    }
    red[tid] = sum;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) loss[0] = 1.0f - (float)(red[0] / (double)planes);
}

// dL/dv_l / (Ho_l Wo_l) per plane: -(dloss / planes) w_l v_l^(w_l - 1) prod_{k != l} relu(v_k)^w_k where v_l > 0, else 0
struct LevelCounts { double c[5]; };
__global__ void msl_dv_kernel(const float* __restrict__ v, const float* __restrict__ dloss, int planes, LevelCounts counts,
                              float* __restrict__ scale) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= planes) return;
    double vl[5], f[5];
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        vl[l] = (double)v[(size_t)l * planes + p];
        f[l] = vl[l] > 0.0 ? pow(vl[l], (double)c_level_w[l]) : 0.0;
    }
    const double g = -(double)dloss[0] / (double)planes;
#pragma unroll
    for (int l = 0; l < 5; ++l) {
        double d = 0.0;
        if (vl[l] > 0.0) {
            double others = 1.0;
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if (k != l) others *= f[k];
            d = g * (double)c_level_w[l] * pow(vl[l], (double)c_level_w[l] - 1.0) * others;
        }
        scale[(size_t)l * planes + p] = (float)(d / counts.c[l]);
    }
}

// backward, one level: the map's gradients with respect to mu_x, E[x^2], E[xy] (, mu_y, E[y^2]) at every map position.
// g planes: g + k * gstride + plane * Ho * Wo, k = 0 mu_x, 1 E[x^2], 2 E[xy], 3 mu_y, 4 E[y^2].
__global__ __launch_bounds__(256) void msl_grad_maps_kernel(const float* __restrict__ X, const float* __restrict__ Y, float off,
                                                            int H, int W, int Ho, int Wo, float C1, float C2, int last,
                                                            const float* __restrict__ scale, int want_db, float* __restrict__ g,
                                                            size_t gstride) {
    __shared__ float smem[SMEM_FLOATS];
    const int tid = threadIdx.x;
    const size_t plane = blockIdx.z;
    const int r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
    load_pair(smem, X + plane * (size_t)H * W, Y + plane * (size_t)H * W, off, H, W, r0, c0);
    vertical_pass<5, true>(smem);

    const float s = scale[plane];
    float* gp = g + plane * (size_t)Ho * Wo;
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int r = idx / TW, c = idx - r * TW;
        if (r0 + r >= Ho || c0 + c >= Wo) continue;
        float f[5];
        horizontal<5>(smem, r, c, f);
        const float mx = f[0], my = f[1];
        const float s1 = f[2] - mx * mx, s2 = f[3] - my * my, s12 = f[4] - mx * my;
        const float bden = (s1 + s2) + C2;
        const float cs = (2.0f * s12 + C2) / bden;
        // d cs / d E[xy] = 2 / B, d cs / d E[x^2] = -cs / B, d cs / d mu_x = 2 (mu_x cs - mu_y) / B   (B = s1 + s2 + C2)
        float gxy = 2.0f / bden, gxx = -cs / bden, gmx = 2.0f * (mx * cs - my) / bden, gmy = 2.0f * (my * cs - mx) / bden;
        float gyy = gxx;
        if (last) {       // ssim = l * cs, l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1): d l / d mu_x = 2 (mu_y - mu_x l) / Q
            const float q = (mx * mx + my * my) + C1;
            const float lum = (2.0f * mx * my + C1) / q;
            gmx = cs * (2.0f * (my - mx * lum) / q) + lum * gmx;
            gmy = cs * (2.0f * (mx - my * lum) / q) + lum * gmy;
            gxy = lum * gxy;
            gxx = lum * gxx;
            gyy = gxx;
        }
        const size_t o = (size_t)(r0 + r) * Wo + (c0 + c);
        const bool zero = s == 0.0f;          // the relu'd level: an exact 0, whatever the map's partials are
        gp[o] = zero ? 0.0f : s * gmx;
        gp[gstride + o] = zero ? 0.0f : s * gxx;
        gp[2 * gstride + o] = zero ? 0.0f : s * gxy;
        if (want_db) {
            gp[3 * gstride + o] = zero ? 0.0f : s * gmy;
            gp[4 * gstride + o] = zero ? 0.0f : s * gyy;
        }
    }
}

// backward, one level: dx = B'g_mu + 2 x B'g_sq + y B'g_xy (+ pool_adjoint(dnext)) on a 16 x 118 tile of the level's image.  The
// transposed blur of a map at image pixel (r, c) is sum_t,s w_t w_s g(r - t, c - s) over the map, i.e. (w symmetric) the valid blur
// of the map zero-extended by 10 on the top and the left: the patch of the three planes starts at (r0 - 10, c0 - 10).
__global__ __launch_bounds__(256) void msl_grad_input_kernel(const float* __restrict__ gm, const float* __restrict__ gsq,
                                                             const float* __restrict__ gxy, const float* __restrict__ X,
                                                             const float* __restrict__ Y, float off, int H, int W, int Ho, int Wo,
                                                             const float* __restrict__ dnext, int Hn, int Wn,
                                                             float* __restrict__ dx) {
    __shared__ float smem[SMEM_FLOATS];
    const int tid = threadIdx.x;
    const size_t plane = blockIdx.z;
    const int r0 = blockIdx.y * TH, c0 = blockIdx.x * TW;
    const size_t mo = plane * (size_t)Ho * Wo;
    for (int i = tid; i < IH * IW; i += 256) {
        const int r = i >> 7, c = i & (IW - 1);
        const int gr = r0 - 10 + r, gc = c0 - 10 + c;
        const bool ok = gr >= 0 && gr < Ho && gc >= 0 && gc < Wo;
        const size_t o = mo + (size_t)gr * Wo + gc;
        smem[i] = ok ? gm[o] : 0.0f;
        smem[IH * IW + i] = ok ? gsq[o] : 0.0f;
        smem[2 * IH * IW + i] = ok ? gxy[o] : 0.0f;
    }
    __syncthreads();
    vertical_pass<3, false>(smem);

    const float* xp = X + plane * (size_t)H * W;
    const float* yp = Y + plane * (size_t)H * W;
    const float* np = dnext ? dnext + plane * (size_t)Hn * Wn : nullptr;
    float* dp = dx + plane * (size_t)H * W;
    const int ph = H & 1, pw = W & 1;
    for (int idx = tid; idx < TH * TW; idx += 256) {
        const int r = idx / TW, c = idx - r * TW;
        const int gr = r0 + r, gc = c0 + c;
        if (gr >= H || gc >= W) continue;
        float b[3];
        horizontal<3>(smem, r, c, b);
        const size_t o = (size_t)gr * W + gc;
        const float x = xp[o] + off, y = yp[o] + off;
        float d = (b[0] + (2.0f * x) * b[1]) + y * b[2];
        // pool_adjoint: level-(l+1) pixel ((gr + ph) / 2, (gc + pw) / 2) averaged this pixel with weight 1/4
        if (np) d = d + np[(size_t)((gr + ph) >> 1) * Wn + ((gc + pw) >> 1)] * 0.25f;
        dp[o] = d;
    }
}

struct Pyramid {
    int H[5], W[5];
    int tiles_x[5], tiles_y[5];        // map tiles (forward, grad-maps)
    int itiles_x[5], itiles_y[5];      // image tiles (grad-input)
};

inline bool make_pyramid(int H, int W, Pyramid& p) {
    if (H <= 160 || W <= 160) return false;        // metrics.py:163-166
    for (int l = 0; l < 5; ++l) {
        p.H[l] = H;
        p.W[l] = W;
        p.tiles_x[l] = (W - 10 + TW - 1) / TW;
        p.tiles_y[l] = (H - 10 + TH - 1) / TH;
        p.itiles_x[l] = (W + TW - 1) / TW;
        p.itiles_y[l] = (H + TH - 1) / TH;
        const int ph = H & 1, pw = W & 1;
        H = (H + 2 * ph - 2) / 2 + 1;
        W = (W + 2 * pw - 2) / 2 + 1;
    }
    return true;
}

struct Layout {
    size_t off[5];           // float offsets of level l (1..4) in a pyramid of X / Y pairs: x at off[l], y at off[l] + planes H_l W_l
    size_t pyr_floats;       // the whole pyramid pair
    size_t partial_bytes;    // forward workspace: float64 tile partials of one level
    size_t scale_floats;     // backward workspace: dL/dv / count [5][planes] (rounded up to 64 floats)
    size_t g_floats;         // backward workspace: one gradient-map plane set [planes][Ho0 Wo0]
    size_t bwd_bytes;
};

inline Layout layout(const Pyramid& p, size_t planes) {
    Layout L{};
    size_t fl = 0;
    for (int l = 1; l < 5; ++l) {
        L.off[l] = fl;
        fl += 2 * planes * (size_t)p.H[l] * p.W[l];
    }
    L.pyr_floats = fl;
    size_t max_tiles = 0;
    for (int l = 0; l < 5; ++l) {
        const size_t t = (size_t)p.tiles_x[l] * p.tiles_y[l];
        max_tiles = t > max_tiles ? t : max_tiles;
    }
    L.partial_bytes = planes * max_tiles * sizeof(double);
    L.scale_floats = (5 * planes + 63) & ~(size_t)63;
    L.g_floats = planes * (size_t)(p.H[0] - 10) * (p.W[0] - 10);
    // scale | 5 gradient-map planes | dx pyramid (levels 1..4, x half) | dy pyramid (y half)
    L.bwd_bytes = (L.scale_floats + 5 * L.g_floats + L.pyr_floats) * sizeof(float);
    return L;
}

inline float c_of(double k, float data_range) { return (float)((k * (double)data_range) * (k * (double)data_range)); }

}  // namespace

extern "C" size_t mcq_ms_ssim_loss_saved_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
    Pyramid p;
    if (N <= 0 || C <= 0 || !make_pyramid(H, W, p)) return 0;
    return layout(p, (size_t)N * C).pyr_floats * sizeof(float);
}

extern "C" size_t mcq_ms_ssim_loss_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W, int32_t backward) {
    Pyramid p;
    if (N <= 0 || C <= 0 || !make_pyramid(H, W, p)) return 0;
    const Layout L = layout(p, (size_t)N * C);
    return backward ? L.bwd_bytes : L.partial_bytes;
}

extern "C" int mcq_ms_ssim_loss_f32(const float* a, const float* b, float offset, float data_range, float* loss_out,
                                    float* values_out, void* saved, void* workspace, int32_t N, int32_t C, int32_t H, int32_t W,
                                    void* stream) {
    if (!a || !b || !loss_out || !values_out || !saved || !workspace || N <= 0 || C <= 0 || !(data_range > 0.0f))
        return MCQ_EINVAL;
    Pyramid p;
    if (!make_pyramid(H, W, p)) return MCQ_EINVAL;
    const size_t planes = (size_t)N * C;
    if (planes > 65535) return MCQ_ETOOLARGE;      // grid.z
    const Layout L = layout(p, planes);
    hipStream_t s = (hipStream_t)stream;
    float* pyr = (float*)saved;
    double* partial = (double*)workspace;
    const float C1 = c_of(0.01, data_range), C2 = c_of(0.03, data_range);
    for (int l = 0; l < 5; ++l) {
        const int Hl = p.H[l], Wl = p.W[l], Ho = Hl - 10, Wo = Wl - 10;
        const float* xl = l == 0 ? a : pyr + L.off[l];
        const float* yl = l == 0 ? b : pyr + L.off[l] + planes * (size_t)Hl * Wl;
        const float off = l == 0 ? offset : 0.0f;
        const dim3 grid((unsigned)p.tiles_x[l], (unsigned)p.tiles_y[l], (unsigned)planes);
        hipLaunchKernelGGL(msl_level_kernel, grid, dim3(256), 0, s, xl, yl, off, Hl, Wl, Ho, Wo, C1, C2, (int)(l == 4), partial);
        hipLaunchKernelGGL(msl_finish_kernel, dim3((unsigned)((planes + 63) / 64)), dim3(64), 0, s, (const double*)partial,
                           (int)planes, p.tiles_x[l] * p.tiles_y[l], (double)Ho * (double)Wo, values_out + (size_t)l * planes);
        if (l < 4) {
            const size_t n1 = planes * (size_t)p.H[l + 1] * p.W[l + 1];
            hipLaunchKernelGGL(msl_halve_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, xl, yl, off,
                               pyr + L.off[l + 1], pyr + L.off[l + 1] + n1, Hl, Wl, p.H[l + 1], p.W[l + 1], n1);
        }
    }
    hipLaunchKernelGGL(msl_combine_kernel, dim3(1), dim3(256), 0, s, (const float*)values_out, (int)planes, loss_out);
    return mcq_check_launch();
}

extern "C" int mcq_ms_ssim_loss_bwd_f32(const float* a, const float* b, float offset, float data_range, const float* values,
                                        const void* saved, const float* dloss, float* da, float* db, void* workspace, int32_t N,
                                        int32_t C, int32_t H, int32_t W, void* stream) {
    if (!a || !b || !values || !saved || !dloss || !da || !workspace || N <= 0 || C <= 0 || !(data_range > 0.0f))
        return MCQ_EINVAL;
    Pyramid p;
    if (!make_pyramid(H, W, p)) return MCQ_EINVAL;
    const size_t planes = (size_t)N * C;
    if (planes > 65535) return MCQ_ETOOLARGE;
    const Layout L = layout(p, planes);
    hipStream_t s = (hipStream_t)stream;
    const float* pyr = (const float*)saved;
    float* scale = (float*)workspace;
    float* g = scale + L.scale_floats;
    float* dpyr = g + 5 * L.g_floats;
    const float C1 = c_of(0.01, data_range), C2 = c_of(0.03, data_range);
    LevelCounts counts;
    for (int l = 0; l < 5; ++l) counts.c[l] = (double)(p.H[l] - 10) * (double)(p.W[l] - 10);
    hipLaunchKernelGGL(msl_dv_kernel, dim3((unsigned)((planes + 63) / 64)), dim3(64), 0, s, values, dloss, (int)planes, counts, scale);
    const int want_db = db != nullptr;
    for (int l = 4; l >= 0; --l) {
        const int Hl = p.H[l], Wl = p.W[l], Ho = Hl - 10, Wo = Wl - 10;
        const size_t n = planes * (size_t)Hl * Wl;
        const float* xl = l == 0 ? a : pyr + L.off[l];
        const float* yl = l == 0 ? b : pyr + L.off[l] + n;
        const float off = l == 0 ? offset : 0.0f;
        const size_t gstride = planes * (size_t)Ho * Wo;
        hipLaunchKernelGGL(msl_grad_maps_kernel, dim3((unsigned)p.tiles_x[l], (unsigned)p.tiles_y[l], (unsigned)planes), dim3(256), 0,
                           s, xl, yl, off, Hl, Wl, Ho, Wo, C1, C2, (int)(l == 4), (const float*)(scale + (size_t)l * planes), want_db,
                           g, gstride);
        const float* dxn = l < 4 ? dpyr + L.off[l + 1] : nullptr;
        const float* dyn = l < 4 ? dpyr + L.off[l + 1] + planes * (size_t)p.H[l + 1] * p.W[l + 1] : nullptr;
        const int Hn = l < 4 ? p.H[l + 1] : 0, Wn = l < 4 ? p.W[l + 1] : 0;
        float* dxl = l == 0 ? da : dpyr + L.off[l];
        float* dyl = l == 0 ? db : dpyr + L.off[l] + n;
        const dim3 igrid((unsigned)p.itiles_x[l], (unsigned)p.itiles_y[l], (unsigned)planes);
        hipLaunchKernelGGL(msl_grad_input_kernel, igrid, dim3(256), 0, s, (const float*)g, (const float*)(g + gstride),
                           (const float*)(g + 2 * gstride), xl, yl, off, Hl, Wl, Ho, Wo, dxn, Hn, Wn, dxl);
        if (want_db)
            hipLaunchKernelGGL(msl_grad_input_kernel, igrid, dim3(256), 0, s, (const float*)(g + 3 * gstride),
                               (const float*)(g + 4 * gstride), (const float*)(g + 2 * gstride), yl, xl, off, Hl, Wl, Ho, Wo, dyn,
                               Hn, Wn, dyl);
    }
    return mcq_check_launch();
}
