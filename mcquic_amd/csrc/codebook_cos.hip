// The codebook cosine regulariser (mcquic/loss/__init__.py:27-44 BasicRate._cosineLoss) and its gradient on the device (gfx950):
//
//   loss = sum over groups g and pairs i < j of clamp(cos_ij, 0, 2),   cos_ij = <c_i, c_j> / sqrt(n_i n_j),   n_i = |c_i|^2
//   dc_i = gamma dout sum_{j != i, 0 <= cos_ij <= 2} ( c_j / s_ij - cos_ij c_i / n_i ),   s_ij = sqrt(n_i n_j)
//
// The Gram matrix is never written: at k = 8192 one group's plane is 256 MiB, the arithmetic 4.3 GFLOP.  Both kernels form
// 32 x 32 tiles of it on v_mfma_f32_32x32x2_f32 and consume them in registers.
//
//   cc_norms_kernel   rn[g, i] = 1 / sqrt(n_i) and 1 / n_i, n_i summed in double (one thread per codeword)
//   cc_fwd_kernel     a workgroup owns the 32 rows of block I of one group and walks the blocks J >= I, its four waves taking
//                     every fourth; a tile's 16 values per lane are added in float, the tiles of a lane in double; lanes, waves
//                     and (cc_sum_kernel, one workgroup) the workgroups' partials meet in fixed orders: no atomics, equal inputs
//                     give equal bits
//   cc_bwd_kernel     the same owner walks ALL blocks J.  The tile is formed TRANSPOSED, P^T = C_J C_I^T: a lane then holds one
//                     codeword i of the owner's block (its column) and 16 codewords j (its registers).  After the epilogue
//                     W_ji = mask / s_ij those registers are, as they stand, the A operand of the second product
//                     G[i][t] += sum_j W_ji C_J[j][t] -- k-step r contracts codeword drow(r, hi) on lane half hi, and the B
//                     operand is read from that row -- so W never passes through LDS.  The row scalar sum_j mask cos_ij rides
//                     along on the VALU.  At the end the four waves' G and row scalars are folded through LDS in wave order and
//                     the owner writes dc_i = scale (G_i - (rowscalar_i / n_i) c_i): every output element has one writer.
//
// Operand order of the first product: the contraction index may be taken in any order as long as both operands agree, so lane
// (hi, i) reads 16 contiguous bytes of its row -- channels 8 q + 4 hi .. + 3 -- and step (q, t) contracts channel 8 q + 4 hi + t
// (as vq_dx_mfma_kernel does for ddist).  Rows past k and channels past d are read as zeros; what such a row or a pair i >= j
// (forward) / i == j (backward) yields is replaced by 0 with a select, never multiplied: a padded row's 0 / 0 stays out of the sums.
// A zero codeword inside [0, k) is NOT masked: its cosines are NaN and so is the loss, as in the reference.
#include "mcq_common.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int CC_WAVES = 4;
constexpr int CC_MAXD = 256;

struct CcK {
    const float* cb;                   // [m, k, d]
    const float* rn;                   // [m, k] 1 / sqrt(n)
    const float* invn;                 // [m, k] 1 / n
    int k, d, kb;                      // kb = ceil(k / 32)
    int vec;                           // rows are 16-byte aligned: 128-bit loads
};

__global__ __launch_bounds__(256) void cc_norms_kernel(const float* __restrict__ cb, float* __restrict__ rn, float* __restrict__ invn,
                                                       size_t rows, int d) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const float* row = cb + i * (size_t)d;
    double n = 0.0;
    for (int t = 0; t < d; ++t) {
        const double v = (double)row[t];
        n += v * v;
    }
    rn[i] = (float)(1.0 / sqrt(n));                                    // (n == 0: +inf, and 0 * inf = NaN in the epilogues)
    invn[i] = (float)(1.0 / n);
}

// channels ch .. ch + 3 of row `row` of one group (base = the group's [k, d]); zeros past k and past d
__device__ __forceinline__ f32x4v cc_load4(const float* __restrict__ base, int row, int ch, const CcK& p) {
    f32x4v v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row < p.k) {
        const float* src = base + (size_t)row * p.d + ch;
        if (p.vec) {
            if (ch < p.d) v = *reinterpret_cast<const f32x4v*>(src);    // (d % 4 == 0: ch < d means ch + 3 < d)
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (ch + t < p.d) v[t] = src[t];
        }
    }
    return v;
}

// rn of row j0 + drow(r, hi) from a register that holds rn[j0 + lane] on lanes 0..31
__device__ __forceinline__ float cc_row_value(float v, int r, int hi) {
    const float lo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (r & 3) + 8 * (r >> 2)));
    const float up = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (r & 3) + 8 * (r >> 2) + 4));
    return hi ? up : lo;
}

__device__ __forceinline__ double cc_wave_sum(double v) {              // a fixed butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// P^T tile: acc[r] of lane (hi, i) = <c[j0 + drow(r, hi)], c[i0 + i]>.  NB = 32-channel blocks; HOLD: the owner's rows stay in cI.
template <int NB, bool HOLD>
__device__ __forceinline__ f32x16 cc_tile(const float* __restrict__ base, const f32x4v (&cI)[HOLD ? NB * 4 : 1], const f32x4v (&cJ)[HOLD ? NB * 4 : 1],
                                          int irow, int jrow, int hi, const CcK& p) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    if constexpr (HOLD) {
#pragma unroll
        for (int q = 0; q < NB * 4; ++q)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cJ[q][t], cI[q][t], acc, 0, 0, 0);
    } else {
#pragma unroll 1
        for (int q0 = 0; q0 < NB * 4; q0 += 4) {
            f32x4v a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = cc_load4(base, jrow, 8 * (q0 + q) + 4 * hi, p);
                b[q] = cc_load4(base, irow, 8 * (q0 + q) + 4 * hi, p);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][t], b[q][t], acc, 0, 0, 0);
        }
    }
    return acc;
}

// workgroup b = g * kb + I
template <int NB>
__global__ __launch_bounds__(64 * CC_WAVES) void cc_fwd_kernel(CcK p, double* __restrict__ partials) {
    constexpr bool HOLD = NB <= 2;
    constexpr int NQ = HOLD ? NB * 4 : 1;
    __shared__ double sh[CC_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int hi = lane >> 5, i = lane & 31;
    const int g = (int)(blockIdx.x / (unsigned)p.kb), I = (int)(blockIdx.x - (unsigned)g * (unsigned)p.kb);
    const float* base = p.cb + (size_t)g * p.k * p.d;
    const float* rn = p.rn + (size_t)g * p.k;
    const int irow = I * 32 + i;
    const float rnI = irow < p.k ? rn[irow] : 0.0f;
    f32x4v cI[NQ], cJ[NQ];
    if constexpr (HOLD) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) cI[q] = cc_load4(base, irow, 8 * q + 4 * hi, p);
#pragma unroll
        for (int q = 0; q < NQ; ++q) cJ[q] = cc_load4(base, (I + wave) * 32 + i, 8 * q + 4 * hi, p);
    }
    double total = 0.0;
    for (int J = I + wave; J < p.kb; J += CC_WAVES) {
        const int j0 = J * 32;
        const f32x16 acc = cc_tile<NB, HOLD>(base, cI, cJ, irow, j0 + i, hi, p);
        if constexpr (HOLD) {                                           // the next tile's rows, in flight during the epilogue
#pragma unroll
            for (int q = 0; q < NQ; ++q) cJ[q] = cc_load4(base, j0 + CC_WAVES * 32 + i, 8 * q + 4 * hi, p);
        }
        const float rnJ_lane = j0 + i < p.k ? rn[j0 + i] : 0.0f;
        float ts = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + mcq_drow(r, hi);
            const float cosv = (acc[r] * cc_row_value(rnJ_lane, r, hi)) * rnI;
            const float cl = cosv < 0.0f ? 0.0f : (cosv > 2.0f ? 2.0f : cosv);      // clamp(0, 2); a NaN stays a NaN
            ts += (j > irow && j < p.k && irow < p.k) ? cl : 0.0f;
        }
        total += (double)ts;
    }
    total = cc_wave_sum(total);
    if (lane == 0) sh[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sh[0];
#pragma unroll
        for (int w = 1; w < CC_WAVES; ++w) t += sh[w];
        partials[blockIdx.x] = t;
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in ascending order, then a fixed tree
__global__ __launch_bounds__(256) void cc_sum_kernel(const double* __restrict__ partials, int n, float* __restrict__ out) {
    __shared__ double sh[256];
    const int tid = (int)threadIdx.x;
    double t = 0.0;
    for (int b = tid; b < n; b += 256) t += partials[b];
    sh[tid] = t;
    __syncthreads();
#pragma unroll
    for (int half = 128; half >= 1; half >>= 1) {
        if (tid < half) sh[tid] += sh[tid + half];
        __syncthreads();
    }
    if (tid == 0) out[0] = (float)sh[0];
}

// workgroup b = g * kb + I
template <int NB>
__global__ __launch_bounds__(64 * CC_WAVES) void cc_bwd_kernel(CcK p, const float* __restrict__ dout, float gamma, float* __restrict__ dcb) {
    constexpr bool HOLD = NB <= 2;
    constexpr int NQ = HOLD ? NB * 4 : 1;
    __shared__ float red[NB][16][64];
    __shared__ double sh_rs[CC_WAVES][32];
    __shared__ float sh_coef[32];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int hi = lane >> 5, i = lane & 31;
    const int g = (int)(blockIdx.x / (unsigned)p.kb), I = (int)(blockIdx.x - (unsigned)g * (unsigned)p.kb);
    const float* base = p.cb + (size_t)g * p.k * p.d;
    const float* rn = p.rn + (size_t)g * p.k;
    const int irow = I * 32 + i;
    const float rnI = irow < p.k ? rn[irow] : 0.0f;
    f32x4v cI[NQ], cJ[NQ];
    if constexpr (HOLD) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) cI[q] = cc_load4(base, irow, 8 * q + 4 * hi, p);
#pragma unroll
        for (int q = 0; q < NQ; ++q) cJ[q] = cc_load4(base, wave * 32 + i, 8 * q + 4 * hi, p);
    }
    f32x16 G[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) G[nb][r] = 0.0f;
    double rs = 0.0;
    for (int J = wave; J < p.kb; J += CC_WAVES) {
        const int j0 = J * 32;
        f32x16 acc = cc_tile<NB, HOLD>(base, cI, cJ, irow, j0 + i, hi, p);
        if constexpr (HOLD) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) cJ[q] = cc_load4(base, j0 + CC_WAVES * 32 + i, 8 * q + 4 * hi, p);
        }
        const float rnJ_lane = j0 + i < p.k ? rn[j0 + i] : 0.0f;
        float ts = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + mcq_drow(r, hi);
            const float rnJ = cc_row_value(rnJ_lane, r, hi);
            const float cosv = (acc[r] * rnJ) * rnI;
            const bool pass = j != irow && j < p.k && irow < p.k && cosv >= 0.0f && cosv <= 2.0f;     // clamp's inclusive mask
            ts += pass ? cosv : 0.0f;
            acc[r] = pass ? rnJ * rnI : 0.0f;                           // W_ji = mask / s_ij
        }
        rs += (double)ts;
        // G[i][32 nb + t] += sum_j W_ji C_J[j][32 nb + t]: step r contracts j = j0 + drow(r, hi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + mcq_drow(r, hi);
            const float* src = base + (size_t)j * p.d;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float b = (j < p.k && 32 * nb + i < p.d) ? src[32 * nb + i] : 0.0f;
                G[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[r], b, G[nb], 0, 0, 0);
            }
        }
    }
    rs += __shfl_xor(rs, 32);                                           // the two halves hold different j of the same row i
    if (hi == 0) sh_rs[wave][i] = rs;
    // the waves' G in wave order through one buffer
    for (int w = 1; w < CC_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[nb][r][lane] = G[nb][r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) G[nb][r] += red[nb][r][lane];
        }
        __syncthreads();
    }
    if (wave != 0) return;
    if (hi == 0) {
        double t = sh_rs[0][i];
#pragma unroll
        for (int w = 1; w < CC_WAVES; ++w) t += sh_rs[w][i];
        sh_coef[i] = irow < p.k ? (float)t * p.invn[(size_t)g * p.k + irow] : 0.0f;
    }
    __builtin_amdgcn_s_waitcnt(0);                                      // (one wave: its own LDS writes, then the reads below)
    __builtin_amdgcn_wave_barrier();
    const float scale = gamma * dout[0];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int lr = mcq_drow(r, hi), row = I * 32 + lr;
        const float coef = sh_coef[lr];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int t = 32 * nb + i;
            if (row < p.k && t < p.d) {
                const size_t idx = ((size_t)g * p.k + row) * p.d + t;
                dcb[idx] = scale * (G[nb][r] - coef * p.cb[idx]);
            }
        }
    }
}

struct CcWs {
    double* partials;
    float* rn;
    float* invn;
};

inline size_t cc_blocks(int m, int k) { return (size_t)m * (size_t)((k + 31) / 32); }

inline CcWs cc_carve(void* workspace, int m, int k) {
    CcWs w;
    w.partials = reinterpret_cast<double*>(workspace);
    w.rn = reinterpret_cast<float*>(w.partials + cc_blocks(m, k));
    w.invn = w.rn + (size_t)m * k;
    return w;
}

inline int cc_args_ok(int m, int k, int d) { return m >= 1 && k >= 1 && d >= 1 && d <= CC_MAXD; }
inline int cc_too_large(int m, int k) { return (size_t)m * k > 0x7fff0000ull; }      // (row indices, with a tile of slack, stay ints)

inline CcK cc_params(const float* codebook, const CcWs& w, int k, int d) {
    CcK p;
    p.cb = codebook; p.rn = w.rn; p.invn = w.invn; p.k = k; p.d = d; p.kb = (k + 31) / 32;
    p.vec = (d % 4 == 0 && (reinterpret_cast<uintptr_t>(codebook) & 15u) == 0) ? 1 : 0;
    return p;
}

inline void cc_launch_norms(const float* codebook, const CcWs& w, int m, int k, int d, hipStream_t s) {
    const size_t rows = (size_t)m * k;
    hipLaunchKernelGGL(cc_norms_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, codebook, w.rn, w.invn, rows, d);
}

}  // namespace

extern "C" size_t mcq_codebook_cos_workspace(int32_t m, int32_t k, int32_t d) {
    if (!cc_args_ok(m, k, d) || cc_too_large(m, k)) return 0;
    return cc_blocks(m, k) * sizeof(double) + 2 * (size_t)m * k * sizeof(float);
}

extern "C" int mcq_codebook_cos_f32(const float* codebook, float* loss, void* workspace, int32_t m, int32_t k, int32_t d, void* stream) {
    if (!codebook || !loss || !workspace || !cc_args_ok(m, k, d)) return MCQ_EINVAL;
    if (cc_too_large(m, k)) return MCQ_ETOOLARGE;
    const hipStream_t s = (hipStream_t)stream;
    const CcWs w = cc_carve(workspace, m, k);
    const CcK p = cc_params(codebook, w, k, d);
    const unsigned blocks = (unsigned)cc_blocks(m, k);
    cc_launch_norms(codebook, w, m, k, d, s);
    const dim3 grid(blocks), block(64 * CC_WAVES);
    if (d <= 32) hipLaunchKernelGGL(cc_fwd_kernel<1>, grid, block, 0, s, p, w.partials);
    else if (d <= 64) hipLaunchKernelGGL(cc_fwd_kernel<2>, grid, block, 0, s, p, w.partials);
    else if (d <= 128) hipLaunchKernelGGL(cc_fwd_kernel<4>, grid, block, 0, s, p, w.partials);
    else hipLaunchKernelGGL(cc_fwd_kernel<8>, grid, block, 0, s, p, w.partials);
    hipLaunchKernelGGL(cc_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)w.partials, (int)blocks, loss);
    return mcq_check_launch();
}

extern "C" int mcq_codebook_cos_bwd_f32(const float* codebook, const float* dout, float gamma, float* dcodebook, void* workspace, int32_t m,
                                        int32_t k, int32_t d, void* stream) {
    if (!codebook || !dout || !dcodebook || !workspace || !cc_args_ok(m, k, d)) return MCQ_EINVAL;
    if (cc_too_large(m, k)) return MCQ_ETOOLARGE;
    const hipStream_t s = (hipStream_t)stream;
    const CcWs w = cc_carve(workspace, m, k);
    const CcK p = cc_params(codebook, w, k, d);
    cc_launch_norms(codebook, w, m, k, d, s);
    const dim3 grid((unsigned)cc_blocks(m, k)), block(64 * CC_WAVES);
    if (d <= 32) hipLaunchKernelGGL(cc_bwd_kernel<1>, grid, block, 0, s, p, dout, gamma, dcodebook);
    else if (d <= 64) hipLaunchKernelGGL(cc_bwd_kernel<2>, grid, block, 0, s, p, dout, gamma, dcodebook);
    else if (d <= 128) hipLaunchKernelGGL(cc_bwd_kernel<4>, grid, block, 0, s, p, dout, gamma, dcodebook);
    else hipLaunchKernelGGL(cc_bwd_kernel<8>, grid, block, 0, s, p, dout, gamma, dcodebook);
    return mcq_check_launch();
}
