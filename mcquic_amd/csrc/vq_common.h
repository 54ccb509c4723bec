// Shared host/device definitions of the vector-quantizer kernels (vq.hip, vq_train.hip).
#pragma once
#include <math.h>
#include <stdint.h>

namespace {

#ifndef MCQ_VQ_PF
#define MCQ_VQ_PF 8
#endif
constexpr int VQ_MB = 4, VQ_NB = 2, VQ_PF = MCQ_VQ_PF;     // wave tile 128 codewords x 64 vectors; prefetch ring depth in k-steps

struct VqK {
    const float* x; const float* cbp; const float* c2p; int64_t* codes;
    int N, m, d, h, w, k;
    int Sp;            // k-steps (channel pairs) per tile, padded to a multiple of VQ_PF
    int ntile;         // 128-codeword tiles
    int bw_log2, nbx, nby, total_blocks;
    int cs_log2;       // vq_assign: 1 << cs_log2 waves of a workgroup share one vector tile, each a slice of the codeword tiles
    int zs;            // vq_assign: workgroups (grid.z) that share one vector tile, each a range of the codeword tiles (1 = none)
    float* ws_best;    // zs > 1: [zs][N m h w] best distance / its codeword per range, folded by vq_fold_kernel
    int* ws_idx;
};

inline void block_shape(int Ho, int Wo, int& lg_out) {
    int best_log2 = 5; double best_util = -1.0;
    for (int lg = 5; lg >= 2; --lg) {
        const int bw = 1 << lg, bh = 32 >> lg;
        const double cover = (double)((Ho + bh - 1) / bh * bh) * (double)((Wo + bw - 1) / bw * bw);
        const double util = (double)Ho * Wo / cover;
        if (util > best_util + 1e-9) { best_util = util; best_log2 = lg; }
    }
    lg_out = best_log2;
}

inline int vq_sp(int d) { return (((d + 1) / 2) + VQ_PF - 1) / VQ_PF * VQ_PF; }

// The packed codebook of (m, k, d), in floats -- the one copy of its sizes: the operand stream [m][ntile][Sp][64][4] (cb_total) with its
// prefetch tail (cb_alloc), then the norm section [m][ntile + 1][64][4] (c2_total; one spare tile per group).  A bits section
// (vq_rate_map.hip) has the norm section's layout and size, whatever d is.
struct VqPackLayout { int ntile, Sp; size_t cb_total, cb_alloc, c2_total; };
inline VqPackLayout vq_pack_layout(int m, int k, int d) {
    VqPackLayout L;
    L.ntile = (k + 127) / 128;
    L.Sp = vq_sp(d);
    L.cb_total = (size_t)m * L.ntile * L.Sp * 256;
    L.cb_alloc = L.cb_total + (size_t)VQ_PF * 256;
    L.c2_total = (size_t)m * (L.ntile + 1) * 256;
    return L;
}

// Float i of a section [g][tiles][steps][64 lanes][4]: lane (l, q) of a tile holds codeword tile * 128 + 32 q + (l & 31); the upper
// half-wave (l >= 32) holds the odd channel of a k-step in the operand stream and nothing (0) in the norm and bits sections.
struct VqSlot { int g, tile, step, word, upper; };
__host__ __device__ inline VqSlot vq_slot(size_t i, int tiles, int steps) {
    const int q = (int)(i & 3), lane = (int)((i >> 2) & 63);
    size_t rest = i >> 8;
    VqSlot s;
    s.step = (int)(rest % steps); rest /= steps;
    s.tile = (int)(rest % tiles);
    s.g = (int)(rest / tiles);
    s.word = s.tile * 128 + 32 * q + (lane & 31);
    s.upper = lane >> 5;
    return s;
}
__host__ __device__ inline VqSlot vq_norm_slot(size_t i, int ntile) { return vq_slot(i, ntile + 1, 1); }
__host__ __device__ inline VqSlot vq_operand_slot(size_t i, int ntile, int Sp) { return vq_slot(i, ntile, Sp); }

// what group g's 16-bit table cdf [m, k + 1] charges for codeword `word`: fl32(16 - log2((double)width)), +inf for a slot of width 0
__device__ inline float vq_table_bits(const uint32_t* cdf, int g, int k, int word) {
    const uint32_t* t = cdf + (size_t)g * (k + 1) + word;
    const uint32_t lo = t[0], up = t[1];
    return up > lo ? (float)(16.0 - log2((double)(up - lo))) : INFINITY;
}

// the geometry fields common to every VQ launch; returns false when the shape is too large
inline bool vq_geometry(VqK& p, int N, int m, int d, int h, int w, int k) {
    p.N = N; p.m = m; p.d = d; p.h = h; p.w = w; p.k = k;
    const VqPackLayout L = vq_pack_layout(m, k, d);
    p.ntile = L.ntile; p.Sp = L.Sp;
    block_shape(h, w, p.bw_log2);
    const int bw = 1 << p.bw_log2, bh = 32 >> p.bw_log2;
    p.nbx = (w + bw - 1) / bw;
    p.nby = (h + bh - 1) / bh;
    const long long tb = (long long)N * p.nbx * p.nby;
    if (tb > 0x7fffffffLL) return false;
    p.total_blocks = (int)tb;
    return true;
}

// the operand-stream fields, for the shape vq_geometry stored
inline void vq_operands(VqK& p, const float* x, const float* cb_packed) {
    p.x = x;
    p.cbp = cb_packed;
    p.c2p = cb_packed + vq_pack_layout(p.m, p.k, p.d).cb_alloc;
}

// both; returns false when the shape is too large
inline bool vq_setup(VqK& p, const float* x, const float* cb_packed, int N, int m, int d, int h, int w, int k) {
    const bool ok = vq_geometry(p, N, m, d, h, w, k);
    vq_operands(p, x, cb_packed);
    return ok;
}

}  // namespace
