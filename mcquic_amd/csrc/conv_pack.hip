// Packing of convolution weights into the operand streams conv_mfma_kernel, conv_head16_kernel and conv_t16_kernel read
// (sizes: conv_sizes.h).
#include "conv_mfma_kernel.h"       // POST_STEPS / POST_TAIL
#include "conv_sizes.h"

namespace {

// `mode` selects which convolution the operand stream is for (w is always the layer's own OIHW weight [Co, Ci, ks, ks]):
//   0  the layer itself:                    W'[co][ci][tap] = w[co][ci][tap]                                  (Cout = Co, Cin = Ci)
//   1  its input gradient, stride 1:        W'[co][ci][tap] = w[ci][co][taps - 1 - tap]  (flip + transpose)    (Cout = Ci, Cin = Co)
//   2  its input gradient, stride 2 (3x3):  dX = PixelShuffle2(conv3x3(dY, W')), W'[4 c + 2 i + j][o][(ty+1, tx+1)] =
//      w[o][c][ky(i, ty)][kx(j, tx)] with (phase, offset) -> kernel index {(0,0): 1, (1,0): 2, (1,1): 0}, else 0   (Cout = 4 Ci, Cin = Co)
// so the backward pass packs straight from the parameter in one launch (no flip / transpose / scatter on the way).
__device__ __forceinline__ float pack_source(const float* __restrict__ w, int mode, int Co, int Ci, int ks, int co, int ci, int tap) {
    const int taps = ks * ks;
    if (mode == 0) return w[((size_t)co * Ci + ci) * taps + tap];
    if (mode == 1) return w[((size_t)ci * Ci + co) * taps + (taps - 1 - tap)];
    const int c = co >> 2, i = (co >> 1) & 1, j = co & 1;
    const int ty = tap / 3 - 1, tx = tap % 3 - 1;
    const int ky = i == 0 ? (ty == 0 ? 1 : -1) : (ty == 0 ? 2 : ty == 1 ? 0 : -1);
    const int kx = j == 0 ? (tx == 0 ? 1 : -1) : (tx == 0 ? 2 : tx == 1 ? 0 : -1);
    if (ky < 0 || kx < 0) return 0.0f;
    return w[((size_t)ci * Ci + c) * 9 + ky * 3 + kx];
}

// OIHW -> [S4 * 9 + tail][64 lanes]: lane l of k-step s * 9 + tap holds W'[co = l & 15][ci = 4 s + (l >> 4)][tap]
__global__ void pack_head16_kernel(const float* __restrict__ w, int Cout, int Cin, int S4, float* __restrict__ out, size_t total,
                                   int mode, int Co, int Ci, float scale) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int lane = (int)(i & 63);
    const size_t step = i >> 6;
    float v = 0.0f;
    if (step < (size_t)S4 * 9) {
        const int s = (int)(step / 9), tap = (int)(step - (size_t)s * 9);
        const int co = lane & 15, ci = 4 * s + (lane >> 4);
        if (co < Cout && ci < Cin) v = pack_source(w, mode, Co, Ci, 3, co, ci, tap) * scale;
    }
    out[i] = v;
}

// OIHW -> [Cout/(32 bands)][TP][64 lanes][bands]: lane l, slot q holds W[co = 32 bands T + 32 q + (l & 31)][ci = 2 s + (l >> 5)][tap]
// for k-step = s * taps + tap (channel-major, tap-inner); zero beyond Cout / Cin and in the tail (MCQ_TAIL_STEPS).
// up to MCQ_PACK_MAX_MULTI weights of one shape per launch (blockIdx.y picks the pair): after an optimizer step every conv of
// the network re-packs its forward and its input-gradient operand stream -- 660 launches of ~4 us each, one by one
constexpr int PACK_MAX_MULTI = 64;       // (round 5: 16 -> 64; the qp=2 model's ~150 convolutions of one shape re-pack in 3 launches instead of 10)
struct PackTable { const float* w[PACK_MAX_MULTI]; float* out[PACK_MAX_MULTI]; unsigned char mask[PACK_MAX_MULTI]; };
// (mask: sections to write -- bit 0 the 128-row copy, 1 the 64-row, 2 the 32-row, 3 the 16x16-tile order; mcq_pack_conv_weight_multi_masked_f32)

__device__ __forceinline__ void pack_conv_weight_body(const float* __restrict__ w, int Cout, int Cin, int ks, int S, int TP,
                                                      float* __restrict__ out, size_t sec4, size_t sec2, size_t total, int mode, int Co, int Ci,
                                                      float scale) {
    // three copies back to back, `bands` = 32-row bands per tile (4 / 2 / 1 for the 128- / 64- / 32-row copies), each
    // laid out [tile][step][lane][band] and followed by its zero tail
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t at = i;
    int bands = 4;
    if (i >= sec4) { i -= sec4; bands = 2; if (i >= sec2) { i -= sec2; bands = 1; } }
    const size_t sec1 = ((size_t)((Cout + 31) / 32) * TP + MCQ_TAIL_STEPS) * 64;
    if (bands == 1 && i >= sec1) {
        // fourth section (conv_t16.h): [Cout / 16][(Cin / 4) * 9 / 4][lane][4], k-step 4 g + u = 9 (channel quad) + tap
        i -= sec1;
        const int u = (int)(i & 3), lane = (int)((i >> 2) & 63);
        const size_t gg = i >> 8;
        const int G = (Cin / 4) * 9 / 4;
        const int tile = (int)(gg / G), step = 4 * (int)(gg - (size_t)tile * G) + u;
        const int co = 16 * tile + (lane & 15), ci = 4 * (step / 9) + (lane >> 4);
        out[at] = pack_source(w, mode, Co, Ci, ks, co, ci, step % 9) * scale;
        return;
    }
    const int ntile = (Cout + 32 * bands - 1) / (32 * bands);
    const int q = (int)(i % bands);
    const int lane = (int)((i / bands) & 63);
    const size_t stepg = i / ((size_t)bands * 64);
    const int tile = (int)(stepg / TP);
    const int step = (int)(stepg - (size_t)tile * TP);
    float v = 0.0f;
    const int taps = mode == 5 ? 16 : mode >= 3 ? 12 : ks * ks;
    if (tile < ntile && step < TP) {
        const int s = step / taps, tap = step - s * taps;
        const int co = tile * 32 * bands + 32 * q + (lane & 31);
        const int ci = 2 * s + (lane >> 5);
        if (co < Cout && ci < Cin) {
            if (mode == 5) {
                // F(2x2, 3x3): tap = 4 i + j, U = G g G^T in float64, rounded once
                const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
                const int pi = tap >> 2, pj = tap & 3;
                double u = 0.0;
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 3; ++b) u += G[pi][a] * (double)pack_source(w, 0, Co, Ci, 3, co, ci, 3 * a + b) * G[pj][b];
                v = (float)u;
            } else if (mode >= 3) {
                // Winograd F(2, 3) along x: tap = 4 dy + position; G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]];
                // mode 3 from the layer's own filter rows, mode 4 from those of its stride-1 input-gradient convolution
                const int row = 3 * (tap >> 2), src = mode == 3 ? 0 : 1;
                const double g0 = pack_source(w, src, Co, Ci, 3, co, ci, row), g1 = pack_source(w, src, Co, Ci, 3, co, ci, row + 1),
                             g2 = pack_source(w, src, Co, Ci, 3, co, ci, row + 2);
                const int pos = tap & 3;
                v = (float)(pos == 0 ? g0 : pos == 1 ? 0.5 * (g0 + g1 + g2) : pos == 2 ? 0.5 * (g0 - g1 + g2) : g2);
            } else
                v = pack_source(w, mode, Co, Ci, ks, co, ci, tap) * scale;
        }
    }
    out[at] = v;
}

__global__ void pack_conv_weight_kernel(const float* __restrict__ w, int Cout, int Cin, int ks, int S, int TP,
                                        float* __restrict__ out, size_t sec4, size_t sec2, size_t total, int mode, int Co, int Ci,
                                        float scale) {
    pack_conv_weight_body(w, Cout, Cin, ks, S, TP, out, sec4, sec2, total, mode, Co, Ci, scale);
}

__global__ void pack_conv_weight_multi_kernel(PackTable t, int Cout, int Cin, int ks, int S, int TP, size_t sec4, size_t sec2, size_t total,
                                              int mode, int Co, int Ci, float scale) {
    // (a uniform dynamic index into the by-value table: scalar loads from the kernel-argument segment -- a compare chain over 64
    //  entries cost every thread ~190 vector instructions)
    const int c = (int)blockIdx.y;
    const float* w = t.w[c];
    float* out = t.out[c];
    pack_conv_weight_body(w, Cout, Cin, ks, S, TP, out, sec4, sec2, total, mode, Co, Ci, scale);
}

// The same four sections for a 3x3 weight with one thread per (output channel, input channel) run: the nine taps of a pair are
// 36 consecutive bytes of the OIHW tensor in every mode (forward, flipped / transposed, sub-pixel), so a thread reads its run
// once and leaves nine values 64 x bands floats apart -- a wave's store is still 256 consecutive bytes.  The element-per-thread
// kernel above fetched a 128-byte line for every float it wrote (a wave's 64 lanes = 64 different rows of the weight): with an
// optimizer step inside the training step every conv re-packs both its operand streams, and those ~45 grouped launches were
// 1.6 ms of a 24 ms step; this form does the same in a quarter of the time.  Same bits in the same places.
__device__ __forceinline__ void pack_conv_weight_runs_body(const float* __restrict__ w, int Cout, int Cin, int S, int TP,
                                                           float* __restrict__ out, int mode, int Co, int Ci, float scale, unsigned n16,
                                                           unsigned mask) {
    // (32-bit index arithmetic throughout: a packed weight is far below 2^31 floats -- the element-per-thread kernel's 64-bit
    //  divisions were a good part of its time)
    unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned base = 0;
#pragma unroll
    for (int b = 4; b >= 1; b >>= 1) {
        const unsigned ntile = (unsigned)(Cout + 32 * b - 1) / (32u * b);
        const unsigned main = ntile * (unsigned)S * 64u * b, tail = (unsigned)MCQ_TAIL_STEPS * 64u * b;
        const bool wanted = (mask >> (b == 4 ? 0 : b == 2 ? 1 : 2)) & 1u;
        if (i < main) {
            if (!wanted) return;
            const unsigned q = i % b, lane = (i / b) & 63u;
            const unsigned sg = i / (64u * b);
            const unsigned tile = sg / (unsigned)S, s = sg - tile * (unsigned)S;
            const int co = (int)(tile * 32u * b + 32u * q + (lane & 31u)), ci = (int)(2u * s + (lane >> 5));
            float v[9];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) v[tap] = 0.0f;
            if (co < Cout && ci < Cin) {
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) v[tap] = pack_source(w, mode, Co, Ci, 3, co, ci, tap) * scale;
            }
            float* o = out + base + ((tile * (unsigned)TP + s * 9u) * 64u + lane) * b + q;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) o[(unsigned)tap * 64u * b] = v[tap];
            return;
        }
        i -= main;
        if (i < tail) { if (wanted) out[base + ntile * (unsigned)TP * 64u * b + i] = 0.0f; return; }
        i -= tail;
        base += (ntile * (unsigned)TP + MCQ_TAIL_STEPS) * 64u * b;
    }
    if (i < n16 && (mask & 8u)) {             // fourth section (conv_t16.h): one 16-byte store = four consecutive k-steps of a lane
        const unsigned lane = i & 63u, gg = i >> 6;
        const unsigned G = (unsigned)(Cin / 4) * 9u / 4u;
        const unsigned tile = gg / G, g = gg - tile * G;
        const int co = (int)(16u * tile + (lane & 15u));
        f32x4v v;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned step = 4u * g + (unsigned)u;
            v[u] = pack_source(w, mode, Co, Ci, 3, co, (int)(4u * (step / 9u) + (lane >> 4)), (int)(step % 9u)) * scale;
        }
        *reinterpret_cast<f32x4v*>(out + base + i * 4u) = v;
    }
}

__global__ void pack_conv_weight_runs_kernel(const float* __restrict__ w, int Cout, int Cin, int S, int TP, float* __restrict__ out,
                                             int mode, int Co, int Ci, float scale, unsigned n16) {
    pack_conv_weight_runs_body(w, Cout, Cin, S, TP, out, mode, Co, Ci, scale, n16, 15u);
}

__global__ void pack_conv_weight_runs_multi_kernel(PackTable t, int Cout, int Cin, int S, int TP, int mode, int Co, int Ci, float scale, unsigned n16) {
    const int c = (int)blockIdx.y;
    const float* w = t.w[c];
    float* out = t.out[c];
    const unsigned mask = t.mask[c];
    pack_conv_weight_runs_body(w, Cout, Cin, S, TP, out, mode, Co, Ci, scale, n16, mask);
}

// threads of pack_conv_weight_runs_kernel: one per (channel pair run, lane, band), per zero of a tail, per 16 bytes of the fourth section
inline size_t pack_runs_threads(int Cout, int Cin) {
    size_t t = 0;
    for (int b = 4; b >= 1; b >>= 1) t += ((size_t)(Cout + 32 * b - 1) / (32 * b) * (size_t)pairs_padded(Cin, 3) + MCQ_TAIL_STEPS) * 64 * b;
    return t + t16_floats(Cout, Cin, 3) / 4;
}

// [128, 128] 1x1 weight -> [POST_STEPS + POST_TAIL][64 lanes][4]: k-step t = 16 mb + r holds the channels 32 mb + drow(r) (+ 4 for the
// upper half-wave) -- the order in which a wave's own accumulator registers supply them
__global__ void pack_post1x1_kernel(const float* __restrict__ w, float* __restrict__ out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (unsigned)((POST_STEPS + POST_TAIL) * 256)) return;
    const unsigned q = i & 3u, lane = (i >> 2) & 63u, t = i >> 8;
    float v = 0.0f;
    if (t < (unsigned)POST_STEPS) {
        const unsigned r = t & 15u;
        const unsigned ci = 32u * (t >> 4) + (r & 3u) + 8u * (r >> 2) + 4u * (lane >> 5);
        v = w[(32u * q + (lane & 31u)) * 128u + ci];
    }
    out[i] = v;
}

}  // namespace

extern "C" size_t mcq_packed_conv_winograd_floats(int32_t Cout, int32_t Cin) {
    if (Cout <= 0 || Cin <= 0) return 0;
    return wino_section_floats(Cout, Cin, 4) + wino_section_floats(Cout, Cin, 2);
}

extern "C" int mcq_pack_conv_weight_winograd_f32(const float* w, int32_t Cout, int32_t Cin, float* out, void* stream) {
    if (!w || !out || Cout <= 0 || Cin <= 0) return MCQ_EINVAL;
    const size_t sec4 = wino_section_floats(Cout, Cin, 4), sec2 = wino_section_floats(Cout, Cin, 2), total = sec4 + sec2;
    const int S = (Cin + 1) / 2, TP = S * 12;
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin,
                       3, S, TP, out, sec4, sec2, total, 3, Cout, Cin, 1.0f);
    return mcq_check_launch();
}

// the same for the layer's stride-1 INPUT-GRADIENT convolution (a [Cin, Cout, 3, 3] conv on flipped / transposed taps): `out`
// holds mcq_packed_conv_winograd_floats(Cin, Cout) floats
extern "C" int mcq_pack_conv_dgrad_weight_winograd_f32(const float* w, int32_t Cout, int32_t Cin, float* out, void* stream) {
    if (!w || !out || Cout <= 0 || Cin <= 0) return MCQ_EINVAL;
    const int co_d = Cin, ci_d = Cout;
    const size_t sec4 = wino_section_floats(co_d, ci_d, 4), sec2 = wino_section_floats(co_d, ci_d, 2), total = sec4 + sec2;
    const int S = (ci_d + 1) / 2, TP = S * 12;
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, co_d, ci_d,
                       3, S, TP, out, sec4, sec2, total, 4, Cout, Cin, 1.0f);
    return mcq_check_launch();
}

extern "C" size_t mcq_packed_conv_winograd2d_floats(int32_t Cout, int32_t Cin) {
    return Cout <= 0 || Cin <= 0 ? 0 : wino2d_floats(Cout, Cin);
}

extern "C" int mcq_pack_conv_weight_winograd2d_f32(const float* w, int32_t Cout, int32_t Cin, float* out, void* stream) {
    if (!w || !out || Cout <= 0 || Cin <= 0) return MCQ_EINVAL;
    const size_t total = wino2d_floats(Cout, Cin);
    const int S = (Cin + 1) / 2, TP = S * 16;
    hipLaunchKernelGGL(pack_conv_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin,
                       3, S, TP, out, (size_t)0, (size_t)0, total, 5, Cout, Cin, 1.0f);
    return mcq_check_launch();
}

extern "C" size_t mcq_packed_conv_weight_floats(int32_t Cout, int32_t Cin, int32_t ksize) {
    if (Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3)) return 0;
    return general_floats(Cout, Cin, ksize) + (head16_shape(Cout, ksize) ? head16_floats(Cin) : 0);
}

extern "C" int mcq_pack_conv_weight_f32(const float* w, int32_t Cout, int32_t Cin, int32_t ksize, float* out,
                                        void* stream) {
    if (!w || !out || Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3)) return MCQ_EINVAL;
    const size_t total = general_floats(Cout, Cin, ksize);
    const int S = pairs_padded(Cin, ksize), TP = steps_padded(Cin, ksize);
    if (ksize == 3 && total < (1ull << 31))
        hipLaunchKernelGGL(pack_conv_weight_runs_kernel, dim3((unsigned)((pack_runs_threads(Cout, Cin) + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           w, Cout, Cin, S, TP, out, 0, Cout, Cin, 1.0f, (unsigned)(t16_floats(Cout, Cin, 3) / 4));
    else
        hipLaunchKernelGGL(pack_conv_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin,
                           ksize, S, TP, out, section_floats(Cout, Cin, ksize, 4), section_floats(Cout, Cin, ksize, 2), total, 0, Cout, Cin, 1.0f);
    if (head16_shape(Cout, ksize)) {      // second copy in the 16-row operand order of conv_head16_kernel
        const size_t t16 = head16_floats(Cin);
        hipLaunchKernelGGL(pack_head16_kernel, dim3((unsigned)((t16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin,
                           (Cin + 3) / 4, out + total, t16, 0, Cout, Cin, 1.0f);
    }
    return mcq_check_launch();
}

extern "C" int mcq_dgrad_weight_shape(int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, int32_t* Cout_d, int32_t* Cin_d) {
    if (Cout <= 0 || Cin <= 0 || !Cout_d || !Cin_d) return MCQ_EINVAL;
    if (stride == 1 && (ksize == 1 || ksize == 3)) { *Cout_d = Cin; *Cin_d = Cout; return MCQ_OK; }
    if (stride == 2 && ksize == 3) { *Cout_d = 4 * Cin; *Cin_d = Cout; return MCQ_OK; }
    return MCQ_EINVAL;
}

extern "C" int mcq_pack_conv_dgrad_weight_f32(const float* w, int32_t Cout, int32_t Cin, int32_t ksize, int32_t stride, float scale,
                                              float* out, void* stream) {
    int32_t co_d = 0, ci_d = 0;
    if (!w || !out || mcq_dgrad_weight_shape(Cout, Cin, ksize, stride, &co_d, &ci_d) != MCQ_OK) return MCQ_EINVAL;
    // same layout and size as a forward pack of a [co_d, ci_d, ks, ks] weight: mcq_packed_conv_weight_floats(co_d, ci_d, ks)
    const size_t total = general_floats(co_d, ci_d, ksize);
    const int S = pairs_padded(ci_d, ksize), TP = steps_padded(ci_d, ksize);
    if (ksize == 3 && total < (1ull << 31))
        hipLaunchKernelGGL(pack_conv_weight_runs_kernel, dim3((unsigned)((pack_runs_threads(co_d, ci_d) + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           w, co_d, ci_d, S, TP, out, stride == 1 ? 1 : 2, Cout, Cin, scale, (unsigned)(t16_floats(co_d, ci_d, 3) / 4));
    else
        hipLaunchKernelGGL(pack_conv_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, co_d, ci_d,
                           ksize, S, TP, out, section_floats(co_d, ci_d, ksize, 4), section_floats(co_d, ci_d, ksize, 2), total,
                           stride == 1 ? 1 : 2, Cout, Cin, scale);
    if (head16_shape(co_d, ksize)) {      // narrow input gradients (the 8-channel fixture models) take the 16-row kernel
        const size_t t16 = head16_floats(ci_d);
        hipLaunchKernelGGL(pack_head16_kernel, dim3((unsigned)((t16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, co_d, ci_d,
                           (ci_d + 3) / 4, out + total, t16, stride == 1 ? 1 : 2, Cout, Cin, scale);
    }
    return mcq_check_launch();
}

extern "C" int32_t mcq_pack_conv_weight_max_multi(void) { return PACK_MAX_MULTI; }

namespace {
int pack_multi(const float* const* w, float* const* out, const uint8_t* masks, int32_t n, int32_t Cout, int32_t Cin, int32_t ksize,
               int32_t dgrad, int32_t stride, float scale, void* stream);
}

extern "C" int mcq_pack_conv_weight_multi_f32(const float* const* w, float* const* out, int32_t n, int32_t Cout, int32_t Cin, int32_t ksize,
                                              int32_t dgrad, int32_t stride, float scale, void* stream) {
    return pack_multi(w, out, nullptr, n, Cout, Cin, ksize, dgrad, stride, scale, stream);
}

extern "C" int mcq_pack_conv_weight_multi_masked_f32(const float* const* w, float* const* out, const uint8_t* masks, int32_t n, int32_t Cout,
                                                     int32_t Cin, int32_t ksize, int32_t dgrad, int32_t stride, float scale, void* stream) {
    return pack_multi(w, out, masks, n, Cout, Cin, ksize, dgrad, stride, scale, stream);
}

namespace {
int pack_multi(const float* const* w, float* const* out, const uint8_t* masks, int32_t n, int32_t Cout, int32_t Cin, int32_t ksize,
               int32_t dgrad, int32_t stride, float scale, void* stream) {
    if (!w || !out || n < 1 || n > PACK_MAX_MULTI || Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3)) return MCQ_EINVAL;
    int32_t co = Cout, ci = Cin;
    int mode = 0;
    if (dgrad) {
        if (mcq_dgrad_weight_shape(Cout, Cin, ksize, stride, &co, &ci) != MCQ_OK) return MCQ_EINVAL;
        mode = stride == 1 ? 1 : 2;
    }
    if (head16_shape(co, ksize)) return MCQ_EINVAL;          // (narrow layers carry a second copy: one by one)
    PackTable t;
    for (int c = 0; c < PACK_MAX_MULTI; ++c) {
        const int k = c < n ? c : 0;
        if (!w[k] || !out[k]) return MCQ_EINVAL;
        t.w[c] = w[k]; t.out[c] = out[k];
        t.mask[c] = (masks && (masks[k] & 15u)) ? (unsigned char)(masks[k] & 15u) : (unsigned char)15u;      // (0 = unknown = everything)
    }
    const size_t total = general_floats(co, ci, ksize);
    const int S = pairs_padded(ci, ksize), TP = steps_padded(ci, ksize);
    if (ksize == 3 && total < (1ull << 31))
        hipLaunchKernelGGL(pack_conv_weight_runs_multi_kernel, dim3((unsigned)((pack_runs_threads(co, ci) + 255) / 256), (unsigned)n), dim3(256), 0,
                           (hipStream_t)stream, t, co, ci, S, TP, mode, Cout, Cin, dgrad ? scale : 1.0f, (unsigned)(t16_floats(co, ci, 3) / 4));
    else
        hipLaunchKernelGGL(pack_conv_weight_multi_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, t, co,
                           ci, ksize, S, TP, section_floats(co, ci, ksize, 4), section_floats(co, ci, ksize, 2), total, mode, Cout, Cin,
                           dgrad ? scale : 1.0f);
    return mcq_check_launch();
}
}  // namespace

extern "C" size_t mcq_packed_post1x1_floats(void) { return (size_t)(POST_STEPS + POST_TAIL) * 256; }

extern "C" int mcq_pack_post1x1_weight_f32(const float* w, float* out, void* stream) {
    if (!w || !out) return MCQ_EINVAL;
    hipLaunchKernelGGL(pack_post1x1_kernel, dim3((unsigned)(POST_STEPS + POST_TAIL)), dim3(256), 0, (hipStream_t)stream, w, out);
    return mcq_check_launch();
}
