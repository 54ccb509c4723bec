// Multi-codebook vector quantizer kernels for gfx950.
//
// mcq_vq_assign_f32 replaces _multiCodebookQuantization._distance + encode
// (reference: mcquic/modules/quantizer.py:144-179): per group g and latent vector v
//     dist[v, k] = (|x_v|^2 + |c_k|^2) - 2 <x_v, c_k>,   code[v] = argmin_k dist[v, k] (first index on ties)
// The reference materialises inter = bmm(x, codebook^T) as [N, m, h, w, k]; here the inner products
// stay in MFMA accumulators (rows = 128 codewords, cols = 64 latent vectors per wave), the epilogue
// of every 128-codeword tile folds them into a per-lane running (min, argmin), and only the int64
// codes are written.  The epilogue keeps the reference's rounding sequence (x2 + c2) - 2*inter.
//
// |c_k|^2 is needed in the accumulator's row layout.  It is obtained bit-exactly with one extra
// MFMA per 32 rows: A[i][0] = c2[i], B[0][j] = 1, everything else 0  =>  D[i][j] = c2[i].
#include "mcq_common.h"
#include "vq_common.h"
#include "../../include/mcquic_hip.h"
#include <math.h>


namespace {

// SPC = compile-time k-steps per tile (p.Sp) for the common vector lengths, 0 = run-time loop.  With the k-steps of a
// tile fully unrolled the whole tile body is straight-line code and hipcc counts the prefetch ring exactly
// (`s_waitcnt vmcnt(N)` per step); around a run-time inner loop it merges the loop-entry and back-edge states
// conservatively and drains the ring at every loop head (112 -> 117 TFLOP/s on config #4).
// XLDS (d = 256): a wave re-reads its 64 vectors (64 KB) for each of its codeword tiles; that does not fit L1, and
// taking it from L2 every time cost 7 % (ablation: activation loads forced to one hot line 122 -> 130 TFLOP/s).  In this
// mode the four waves of a workgroup are the four codeword slices of ONE vector tile, which they stage in LDS once
// ([channel][64 vectors]: the B operand of a k-step is then two conflict-free ds_read_b32 per lane).
// RATE (mcq_vq_assign_rate_map_f32): cost = fma(lambda_v, bits_k, dist) with one lambda per latent vector, an operand of the launch
// (VqRate), where the scalar knob folds lambda * bits into the pack's norms.  `bits` is a second section in the norms' layout and
// reaches the accumulator rows the way c2 does; lambda_v = 0 leaves the distance bit for bit.  RATE = false is the plain kernel: every
// addition below sits behind `if (RATE)`, a compile-time constant.
struct VqRate {
    const float* bits;            // [m][ntile + 1][64][4]: fl32(16 - log2 width); 0 for padded codewords and the upper half-wave; +inf at width 0
    const float* lam;             // lambda of (image, row, column) at lam[image * sn + row * sy + column * sx], shared by the m groups
    long long sn, sy, sx;         // element strides >= 0 ((1, 0, 0): one lambda per image)
};

template <bool RATE> struct VqRateArg {};              // nothing travels with the plain kernel
template <> struct VqRateArg<true> : VqRate {};

template <int SPC, bool XLDS, bool RATE = false>
__global__ __launch_bounds__(256, 2) void vq_assign_kernel(VqK p, VqRateArg<RATE> rt) {
    __shared__ float xs[XLDS ? 2 * SPC * 64 : 1];
    constexpr int MB = VQ_MB, NB = VQ_NB, PF = VQ_PF;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // 4 waves per workgroup = (4 >> cs_log2) vector tiles x (1 << cs_log2) slices of the codeword tiles
    const int CS = 1 << p.cs_log2;
    const int slice = wave & (CS - 1);
    const int gw = blockIdx.x * (4 >> p.cs_log2) + (wave >> p.cs_log2);
    const bool active = gw * NB < p.total_blocks;            // wave-uniform
    if (CS == 1 && !active) return;                          // (sliced waves stay for the barrier)
    const int g = blockIdx.y;
    const int hi = lane >> 5, j = lane & 31;
    const int BW = 1 << p.bw_log2;
    const int ly = j >> p.bw_log2, lx = j & (BW - 1);
    const int BH = 32 >> p.bw_log2;
    const int HW = p.h * p.w;
    const unsigned group_bytes = (unsigned)p.d * (unsigned)HW * 4u;

    int img[NB], yo[NB], xo[NB];
    bool valid[NB];
    unsigned pixoff[NB];
    __amdgpu_buffer_rsrc_t rsrc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        int pb = gw * NB + nb;
        const bool pbv = pb < p.total_blocks;
        if (!pbv) pb = p.total_blocks - 1;
        const int per_img = p.nby * p.nbx;
        const int n = pb / per_img;
        const int rem = pb - n * per_img;
        const int by = rem / p.nbx;
        const int bx = rem - by * p.nbx;
        img[nb] = n;
        yo[nb] = by * BH + ly;
        xo[nb] = bx * BW + lx;
        valid[nb] = pbv && yo[nb] < p.h && xo[nb] < p.w;
        pixoff[nb] = valid[nb] ? (unsigned)(yo[nb] * p.w + xo[nb]) * 4u : MCQ_OOB;
        // the descriptor covers exactly this image's group-g channels, so padded k-steps read 0
        rsrc[nb] = mcq_make_rsrc(mcq_uniform_ptr(p.x + ((size_t)n * p.m + g) * (size_t)p.d * HW), group_bytes);
    }

    if (XLDS) {
        // wave w stages channels w, w + 4, ... of the tile (its own lanes' pixels: every slice has the same geometry)
        for (int c = wave; c < 2 * SPC; c += 4) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
                if (hi == 0) xs[c * 64 + nb * 32 + j] = mcq_buffer_load(rsrc[nb], pixoff[nb] + (unsigned)c * (unsigned)HW * 4u);
        }
        __syncthreads();
    }

    // |x_v|^2, sequential over the d channels of the group (both half-waves compute it redundantly)
    // (sixteen independent loads per batch, both blocks together; the additions keep the channel order)
    float x2[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) x2[nb] = 0.0f;
    for (int c0 = 0; c0 < p.d; c0 += 16) {
        float v[NB][16];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {    // channels past d are out of range = 0: they add +0
                // (XLDS, round 6: from the staged tile -- four waves reading their 64 KB again from global memory made the launch pull
                //  3.2x its algorithmic bytes through the fabric, profiles/r05_pmc_by_kernel_vq.txt; same values, same order)
                if (XLDS) v[nb][i] = c0 + i < 2 * SPC ? xs[(c0 + i) * 64 + nb * 32 + j] : 0.0f;
                else v[nb][i] = mcq_buffer_load(rsrc[nb], pixoff[nb] + (unsigned)(c0 + i) * (unsigned)HW * 4u);
            }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int i = 0; i < 16; ++i) x2[nb] = x2[nb] + v[nb][i] * v[nb][i];
    }

    // each lane's lambdas, once (both half-waves hold the same latent vectors)
    float lamv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        lamv[nb] = 0.0f;
        if constexpr (RATE) if (valid[nb]) lamv[nb] = rt.lam[(long long)img[nb] * rt.sn + (long long)yo[nb] * rt.sy + (long long)xo[nb] * rt.sx];
    }

    f32x4v A[PF];
    float B[PF][NB];
    // (grid.z workgroups x CS waves share the codeword tiles of a vector tile: small launches, see the launcher)
    const int per_slice = (p.ntile + CS * p.zs - 1) / (CS * p.zs);
    const int tile0r = ((int)blockIdx.z * CS + slice) * per_slice;
    const int tile0 = tile0r < p.ntile ? tile0r : p.ntile;             // this wave's codeword tiles: [tile0, tile1) (possibly none)
    const int tile1 = active ? (tile0 + per_slice < p.ntile ? tile0 + per_slice : p.ntile) : tile0;
    // operand addresses stay off the vector ALU inside the k-loop (a VALU instruction between two MFMAs costs the
    // matrix pipe ~10 cycles, tools/probes/mfma_issue.hip): per-lane offsets are loop constants, the running part is
    // a wave-uniform soffset advanced by the scalar unit
    const __amdgpu_buffer_rsrc_t wr = mcq_make_rsrc(p.cbp + ((size_t)g * p.ntile + tile0) * p.Sp * 256, 0x7fffffffu);
    const unsigned wlane = (unsigned)lane * 16u;
    unsigned wso = 0;
    const f32x4v* c2l = reinterpret_cast<const f32x4v*>(p.c2p) + ((size_t)g * (p.ntile + 1) + tile0) * 64 + lane;
    // (RATE) the bits section through a descriptor: the lane offset is the operand stream's, the tile a scalar offset -- no registers
    __amdgpu_buffer_rsrc_t br = wr;
    if constexpr (RATE) br = mcq_make_rsrc(rt.bits + ((size_t)g * (p.ntile + 1) + tile0) * 256, 0x7fffffffu);
    int ls = 0;
    unsigned soffL = 0;
    const unsigned step_bytes = 2u * (unsigned)HW * 4u;
    unsigned voffL[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) voffL[nb] = valid[nb] ? pixoff[nb] + (unsigned)(hi * HW) * 4u : MCQ_OOB;

    auto issue = [&](int st) {
        A[st] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(wr, (int)wlane, (int)wso, 0));
        wso += 1024;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
            B[st][nb] = XLDS ? xs[(2 * ls + hi) * 64 + nb * 32 + j] : mcq_buffer_load_s(rsrc[nb], voffL[nb], soffL);
        ++ls;
        soffL += step_bytes;
        if (ls == p.Sp) { ls = 0; soffL = 0; }
    };

    float best[NB];
    int bidx[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { best[nb] = INFINITY; bidx[nb] = 0; }
    const float bone = hi == 0 ? 1.0f : 0.0f;

    f32x4v c2a = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4v bta = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    if (tile0 < tile1) {
#pragma unroll
        for (int st = 0; st < PF; ++st) issue(st);
        c2a = c2l[0];
    }

    for (int tile = tile0; tile < tile1; ++tile) {
        const f32x4v c2n = c2l[(size_t)(tile - tile0 + 1) * 64];   // next tile's norms (one spare tile is allocated)
        // (RATE) this tile's bits arrive behind its last k-steps: held over PF steps only, where the unrolled forms can place the load
        const unsigned bso = (unsigned)(tile - tile0) * 1024u;
        if (RATE && !SPC) bta = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(br, (int)wlane, (int)bso, 0));
        f32x16 acc[MB][NB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.0f;

        auto step = [&](int st, int t) {
            // fully unrolled variants: the slot being refilled belongs to k-step (t + PF) % SPC of the tile -- a
            // compile-time number, so the LDS read takes an immediate offset and nothing is computed per lane
            const int lsn = SPC ? (t + PF) % (SPC ? SPC : 1) : ls;
            const unsigned son = SPC ? (unsigned)lsn * step_bytes : soffL;
            if (RATE && SPC && t == (SPC ? SPC : PF) - PF && st == 0)
                bta = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(br, (int)wlane, (int)bso, 0));
            // vector-block major, each activation slot refilled right after its last use (as in the convolution kernel)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
                    acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[st][mb], B[st][nb], acc[mb][nb], 0, 0, 0);
                B[st][nb] = XLDS ? xs[(2 * lsn + hi) * 64 + nb * 32 + j] : mcq_buffer_load_s(rsrc[nb], voffL[nb], son);
            }
            A[st] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(wr, (int)wlane, (int)wso, 0));
            wso += 1024;
            ++ls;
            soffL += step_bytes;
            if (ls == p.Sp) { ls = 0; soffL = 0; }
            // keep the software pipeline as written (without the fence hipcc regroups the loads of the body)
            __builtin_amdgcn_sched_barrier(0);
        };
        if (SPC) {
#pragma unroll
            for (int t = 0; t < SPC; t += PF) {
#pragma unroll
                for (int st = 0; st < PF; ++st) step(st, t + st);
            }
        } else {
            for (int t = 0; t < p.Sp; t += PF) {
#pragma unroll
                for (int st = 0; st < PF; ++st) step(st, 0);
            }
        }

        const int word0 = tile * 128;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = 0.0f;
            const f32x16 c2d = __builtin_amdgcn_mfma_f32_32x32x2f32(c2a[mb], bone, z, 0, 0, 0);
            if constexpr (RATE) {
                // the distances first, in place of the inner products (c2d is then dead), then bits_k in the rows' layout, exact, and
                // cost = fma(lambda_v, bits_k, dist): one more rounding (a width-0 slot gives +inf, or NaN at lambda 0: never < best)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const f32x2v s2 = f32x2v{x2[nb], x2[nb]} + f32x2v{c2d[r], c2d[r + 1]};
                        const f32x2v dv2 = __builtin_elementwise_fma(f32x2v{-2.0f, -2.0f}, f32x2v{acc[mb][nb][r], acc[mb][nb][r + 1]}, s2);
                        acc[mb][nb][r] = dv2[0]; acc[mb][nb][r + 1] = dv2[1];
                    }
                const f32x16 btd = __builtin_amdgcn_mfma_f32_32x32x2f32(bta[mb], bone, z, 0, 0, 0);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    float dv[16];
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const f32x2v dv2 = __builtin_elementwise_fma(f32x2v{lamv[nb], lamv[nb]}, f32x2v{btd[r], btd[r + 1]},
                                                                     f32x2v{acc[mb][nb][r], acc[mb][nb][r + 1]});
                        dv[r] = dv2[0]; dv[r + 1] = dv2[1];
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int word = word0 + mb * 32 + mcq_drow(r, hi);
                        if (dv[r] < best[nb]) { best[nb] = dv[r]; bidx[nb] = word; }
                    }
                }
                // one band at a time: hipcc otherwise issues the eight row-layout MFMAs of a tile together and their 128 results spill
                __builtin_amdgcn_sched_barrier(0);
                continue;
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                // (x2 + c2) - 2 * inter ; 2 * inter is exact, so the fused form rounds identically.  Two distances per
                // instruction (v_pk_add_f32 / v_pk_fma_f32: same IEEE operations, half the issue slots)
                float dv[16];
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const f32x2v s2 = f32x2v{x2[nb], x2[nb]} + f32x2v{c2d[r], c2d[r + 1]};
                    const f32x2v dv2 = __builtin_elementwise_fma(f32x2v{-2.0f, -2.0f}, f32x2v{acc[mb][nb][r], acc[mb][nb][r + 1]}, s2);
                    dv[r] = dv2[0]; dv[r + 1] = dv2[1];
                }
                // (round 6, built and dropped: a two-level epilogue that skips bands no lane improves, docs/experiments.md section 11.5)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int word = word0 + mb * 32 + mcq_drow(r, hi);
                    if (dv[r] < best[nb]) { best[nb] = dv[r]; bidx[nb] = word; }
                }
            }
        }
        c2a = c2n;
    }

    // the two half-waves hold interleaved codeword rows of the same latent vector
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const float ob = __shfl_xor(best[nb], 32);
        const int oi = __shfl_xor(bidx[nb], 32);
        if (ob < best[nb] || (ob == best[nb] && oi < bidx[nb])) { best[nb] = ob; bidx[nb] = oi; }
    }
    if (CS > 1) {
        // slices meet in LDS; slice 0 folds the others in slice order -- a later slice holds larger codeword indices,
        // so it only wins with a strictly smaller distance (first index on ties, like torch.argmin)
        __shared__ float s_best[4][NB][64];
        __shared__ int s_idx[4][NB][64];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            s_best[wave][nb][lane] = best[nb];
            s_idx[wave][nb][lane] = bidx[nb];
        }
        __syncthreads();
        if (slice != 0 || !active) return;
        for (int s = 1; s < CS; ++s) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float ob = s_best[wave + s][nb][lane];
                const int oi = s_idx[wave + s][nb][lane];
                if (ob < best[nb]) { best[nb] = ob; bidx[nb] = oi; }
            }
        }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
        if (hi == 0 && valid[nb]) {
            const size_t v = (((size_t)img[nb] * p.m + g) * p.h + yo[nb]) * p.w + xo[nb];
            if (p.zs == 1) p.codes[v] = (int64_t)bidx[nb];
            else {
                const size_t nvec = (size_t)p.N * p.m * p.h * p.w;
                p.ws_best[(size_t)blockIdx.z * nvec + v] = best[nb];
                p.ws_idx[(size_t)blockIdx.z * nvec + v] = bidx[nb];
            }
        }
}

// the ranges of a vector meet: range order = codeword order, so a later range only wins with a strictly smaller distance
// (first index on ties, like torch.argmin and like the slices inside a workgroup)
__global__ void vq_fold_kernel(const float* __restrict__ ws_best, const int* __restrict__ ws_idx, int zs, size_t nvec,
                               int64_t* __restrict__ codes) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nvec) return;
    float best = ws_best[v];
    int idx = ws_idx[v];
    for (int z = 1; z < zs; ++z) {
        const float ob = ws_best[(size_t)z * nvec + v];
        if (ob < best) { best = ob; idx = ws_idx[(size_t)z * nvec + v]; }
    }
    codes[v] = (int64_t)idx;
}

// codebook [m, k, d] -> cbp [m][ntile][Sp][64][4] (+ zero tail) and c2p [m][ntile + 1][64][4] (VqPackLayout, vq_common.h)
__global__ void vq_pack_kernel(const float* __restrict__ cb, int k, int d, VqPackLayout L, float* __restrict__ cbp) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.cb_alloc) return;
    float v = 0.0f;
    if (i < L.cb_total) {
        const VqSlot s = vq_operand_slot(i, L.ntile, L.Sp);
        const int c = 2 * s.step + s.upper;
        if (s.word < k && c < d) v = cb[((size_t)s.g * k + s.word) * d + c];
    }
    cbp[i] = v;
}

// The norm section.  cdf == nullptr: |c_k|^2.  Else (mcq_vq_pack_codebook_rate_f32) with a per-codeword rate penalty folded in: the same
// |c|^2 loop, then c2' = fl32(c2 + fl32(lambda * bits_k)), bits_k = vq_table_bits of the group's 16-bit table [k + 1].  vq_assign_kernel
// reads this section as |c_k|^2, so its (x2 + c2') - 2 inter is distance + lambda * bits.  lambda = 0 adds +0 to a non-negative sum: the
// bits of the plain section.  Padded codewords and slots of width 0 (no valid table has one) are +inf: they can never win the argmin.
__global__ void vq_c2_kernel(const float* __restrict__ cb, const uint32_t* __restrict__ cdf, float lambda, int k, int d, VqPackLayout L,
                             float* __restrict__ c2p) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.c2_total) return;
    const VqSlot sl = vq_norm_slot(i, L.ntile);
    float v = 0.0f;
    if (!sl.upper) {
        v = INFINITY;
        if (sl.tile < L.ntile && sl.word < k) {
            const float* row = cb + ((size_t)sl.g * k + sl.word) * d;
            float s = 0.0f;
            for (int c = 0; c < d; ++c) s = s + row[c] * row[c];
            v = s;
            if (cdf) {
                const float bits = vq_table_bits(cdf, sl.g, k, sl.word);
                const float pen = lambda * bits;
                v = bits < INFINITY ? s + pen : INFINITY;
            }
        }
    }
    c2p[i] = v;
}

__global__ void vq_gather_kernel(const int64_t* __restrict__ codes, const float* __restrict__ cb, float* __restrict__ out,
                                 float* __restrict__ out2, int N, int m, int d, int hw, int k) {
    // one thread per (n, g, pixel); writes d channel planes (coalesced across threads)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)N * m * hw;
    if (i >= total) return;
    const int pix = (int)(i % hw);
    const size_t ng = i / hw;
    const int g = (int)(ng % m);
    const size_t n = ng / m;
    int64_t code = codes[i];
    code = code < 0 ? 0 : (code >= k ? k - 1 : code);
    const float* row = cb + ((size_t)g * k + (size_t)code) * d;
    float* o = out + ((n * m + g) * (size_t)d) * hw + pix;
    for (int c = 0; c < d; ++c) o[(size_t)c * hw] = row[c];
    if (out2) {
        float* o2 = out2 + ((n * m + g) * (size_t)d) * hw + pix;
        for (int c = 0; c < d; ++c) o2[(size_t)c * hw] = mcq_silu(row[c]);
    }
}

__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out,
                           float* __restrict__ out2, int64_t n) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const f32x4v va = *reinterpret_cast<const f32x4v*>(a + i);
        const f32x4v vb = *reinterpret_cast<const f32x4v*>(b + i);
        const f32x4v vs = va + vb;
        *reinterpret_cast<f32x4v*>(out + i) = vs;
        if (out2) *reinterpret_cast<f32x4v*>(out2 + i) = f32x4v{mcq_silu(vs[0]), mcq_silu(vs[1]), mcq_silu(vs[2]), mcq_silu(vs[3])};
    } else {
        for (; i < n; ++i) {
            const float v = a[i] + b[i];
            out[i] = v;
            if (out2) out2[i] = mcq_silu(v);
        }
    }
}

// out = (a + b) + c, the rounding order of two chained additions (the three gradient paths that meet at an AttentionBlock's input)
__global__ void add3_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c, float* __restrict__ out,
                            int64_t n) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const f32x4v va = *reinterpret_cast<const f32x4v*>(a + i);
        const f32x4v vb = *reinterpret_cast<const f32x4v*>(b + i);
        const f32x4v vc = *reinterpret_cast<const f32x4v*>(c + i);
        *reinterpret_cast<f32x4v*>(out + i) = (va + vb) + vc;
    } else {
        for (; i < n; ++i) out[i] = (a[i] + b[i]) + c[i];
    }
}

__global__ void detransform_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        // (x - min) / (max - min) with min = -1, max = 1, then * (255 + 1.0 - 1e-3), clamp, truncate
        float v = (x[i] - (-1.0f)) / 2.0f;
        v = v * 255.999f;
        v = fminf(fmaxf(v, 0.0f), 255.0f);
        out[i] = (uint8_t)v;
    }
}

}  // namespace

extern "C" size_t mcq_packed_codebook_floats(int32_t m, int32_t k, int32_t d) {
    if (m <= 0 || k <= 0 || d <= 0) return 0;
    const VqPackLayout L = vq_pack_layout(m, k, d);
    return L.cb_alloc + L.c2_total;
}

// both pack entry points: the operand stream, then the norm section (cdf == nullptr: the plain one)
static int vq_pack_launch(const float* codebook, const uint32_t* cdf, float lambda, int m, int k, int d, float* cb_packed, void* stream) {
    const VqPackLayout L = vq_pack_layout(m, k, d);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vq_pack_kernel, dim3((unsigned)((L.cb_alloc + 255) / 256)), dim3(256), 0, s, codebook, k, d, L, cb_packed);
    hipLaunchKernelGGL(vq_c2_kernel, dim3((unsigned)((L.c2_total + 255) / 256)), dim3(256), 0, s, codebook, cdf, lambda, k, d, L,
                       cb_packed + L.cb_alloc);
    return mcq_check_launch();
}

extern "C" int mcq_vq_pack_codebook_f32(const float* codebook, int32_t m, int32_t k, int32_t d, float* cb_packed,
                                        void* stream) {
    if (!codebook || !cb_packed || m <= 0 || k <= 0 || d <= 0) return MCQ_EINVAL;
    return vq_pack_launch(codebook, nullptr, 0.0f, m, k, d, cb_packed, stream);
}

extern "C" int mcq_vq_pack_codebook_rate_f32(const float* codebook, const uint32_t* cdf, float lambda, int32_t m, int32_t k,
                                             int32_t d, float* cb_packed, void* stream) {
    if (!codebook || !cdf || !cb_packed || m <= 0 || k <= 0 || d <= 0) return MCQ_EINVAL;
    if (!(lambda >= 0.0f) || isinf(lambda)) return MCQ_EINVAL;      // (negative, NaN, inf)
    return vq_pack_launch(codebook, cdf, lambda, m, k, d, cb_packed, stream);
}

namespace {
// Workgroups per vector tile (grid.z) for launches that would leave most of the GPU idle -- one 768x512 image is 24 vector
// tiles x 2 codebooks at the first level: 48 workgroups walking 8192 codewords each, 139 us for 20 us of MFMA work.  The
// codeword tiles are then ranged over up to 16 workgroups (each at least one tile per wave) until ~1536 waves exist.
int vq_assign_ranges(long long vtiles, int m, int ntile, int cs_log2) {
    const long long waves = vtiles * m << cs_log2;
    int zs = 1;
    while (zs < 16 && waves * zs < 1536 && (ntile >> cs_log2) >= 2 * zs) zs *= 2;
    return zs;
}
// The kernel deals per_slice = ceil(ntile / (CS zs)) tiles to every (range, slice) in order, so the tiles run out at some slot: range z
// owns none iff z CS per_slice >= ntile.  That happens wherever CS zs per_slice overshoots ntile by a whole range -- 17..24 tiles over
// 4 x 4 slots of 2 leave range 3 empty, 33..40 tiles over 8 x 4 leave ranges 5..7, 65..72 over 16 x 4 leave ranges 9..15.  Those workgroups
// are not launched (as vq_logits_kernel's launcher trims its grid.z): grid.z = ceil(ntile / (CS per_slice)), every launched range's first
// slice owns a tile, and the fold reads the launched ranges only.  zs stays the divisor, so no wave's walk gets longer.
int vq_assign_launched_ranges(int ntile, int cs_log2, int zs) {
    const int cs = 1 << cs_log2;
    const int per_range = cs * ((ntile + cs * zs - 1) / (cs * zs));
    return (ntile + per_range - 1) / per_range;
}

// Everything the assignment launch decides from the shape alone: pure host code, the one copy.  vq_assign_launch launches by it,
// mcq_vq_assign_workspace_bytes sizes by it and mcq_vq_assign_plan shows it (tests/test_vq_assign_plan.py holds it to literals).
struct VqAssignPlan {
    int instance;                 // MCQ_VQ_ASSIGN_*: the <SPC, XLDS> pair of vq_assign_kernel
    VqK p;                        // the kernel's argument with its geometry (vq_geometry), cs_log2 and zs filled in; zs = the ranges the tiles
                                  // are dealt over, given a workspace: ceil(ntile / (CS zs)) tiles a slice, in order
    int gz;                       // grid.z: the ranges that own a tile (see vq_assign_launched_ranges), <= zs
    long long vtiles;             // vector tiles of VQ_NB blocks: one wave (or one group of slices) each
};
// MCQ_OK, or the status the entry points refuse the shape with
int vq_assign_plan(int N, int m, int d, int h, int w, int k, VqAssignPlan& pl) {
    if (N <= 0 || m <= 0 || d <= 0 || h <= 0 || w <= 0 || k <= 0) return MCQ_EINVAL;
    if ((uint64_t)d * h * w * 4ull >= 0x80000000ull) return MCQ_ETOOLARGE;
    VqK& p = pl.p;
    if (!vq_geometry(p, N, m, d, h, w, k)) return MCQ_ETOOLARGE;
    pl.vtiles = ((long long)p.total_blocks + VQ_NB - 1) / VQ_NB;
    // Every wave walks all codeword tiles of its 64 vectors, so the launch has (vector tiles x m) waves whatever k is:
    // too few for the 2048 wave slots (2 per SIMD) on the small levels, and 1.5 rounds for config #4.  Splitting the
    // codeword tiles over 2 or 4 waves of a workgroup multiplies the waves and divides their length; pick the split
    // with the fewest whole rounds of work.
    int cs_log2 = 0;
    double best_cost = 1e30;
    for (int lg = 0; lg <= 2 && (1 << lg) <= p.ntile; ++lg) {
        const long long waves = pl.vtiles * m << lg;
        const double cost = (double)((waves + 2047) / 2048) / (double)(1 << lg);
        if (cost < best_cost - 1e-12) { best_cost = cost; cs_log2 = lg; }
    }
    if (p.Sp == 128 && p.ntile >= 4) cs_log2 = 2;            // the LDS-staged mode: four slices share one vector tile
    p.cs_log2 = cs_log2;
    p.zs = vq_assign_ranges(pl.vtiles, m, p.ntile, cs_log2);
    pl.gz = vq_assign_launched_ranges(p.ntile, cs_log2, p.zs);
    pl.instance = p.Sp == 32 ? MCQ_VQ_ASSIGN_SP32                                    // d = 49 .. 64
                : p.Sp == 8 ? MCQ_VQ_ASSIGN_SP8                                      // d = 16 (model No. 12), d = 1 .. 15
                : p.Sp == 128 ? (cs_log2 == 2 ? MCQ_VQ_ASSIGN_SP128_LDS : MCQ_VQ_ASSIGN_SP128)      // d = 241 .. 256
                : MCQ_VQ_ASSIGN_LOOP;
    return MCQ_OK;
}
}  // namespace

extern "C" int mcq_vq_assign_plan(int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, int32_t rate, int32_t* out) {
    VqAssignPlan pl;
    if (!out || (rate != 0 && rate != 1) || vq_assign_plan(N, m, d, h, w, k, pl) != MCQ_OK) return 0;
    out[0] = pl.instance; out[1] = pl.p.Sp; out[2] = pl.p.cs_log2; out[3] = pl.p.zs; out[4] = pl.p.bw_log2; out[5] = (int32_t)pl.vtiles;
    return 1;
}

extern "C" size_t mcq_vq_assign_workspace_bytes(int32_t N, int32_t m, int32_t d, int32_t h, int32_t w, int32_t k) {
    VqAssignPlan pl;
    if (vq_assign_plan(N, m, d, h, w, k, pl) != MCQ_OK) return 0;
    return pl.p.zs > 1 ? (size_t)pl.p.zs * N * m * h * w * 8u : 0;
}

extern "C" int mcq_vq_assign_f32(const float* x, const float* cb_packed, int64_t* codes, int32_t N, int32_t m, int32_t d,
                                 int32_t h, int32_t w, int32_t k, void* stream) {
    return mcq_vq_assign_ws_f32(x, cb_packed, codes, N, m, d, h, w, k, nullptr, stream);
}

namespace {
// one instance of the plan's table, with or without the rate operand
template <bool RATE>
void vq_assign_run(int instance, dim3 grid, hipStream_t s, const VqK& p, const VqRateArg<RATE>& rt) {
    switch (instance) {
    case MCQ_VQ_ASSIGN_SP32: hipLaunchKernelGGL((vq_assign_kernel<32, false, RATE>), grid, dim3(256), 0, s, p, rt); break;
    case MCQ_VQ_ASSIGN_SP8: hipLaunchKernelGGL((vq_assign_kernel<8, false, RATE>), grid, dim3(256), 0, s, p, rt); break;
    case MCQ_VQ_ASSIGN_SP128_LDS: hipLaunchKernelGGL((vq_assign_kernel<128, true, RATE>), grid, dim3(256), 0, s, p, rt); break;
    case MCQ_VQ_ASSIGN_SP128: hipLaunchKernelGGL((vq_assign_kernel<128, false, RATE>), grid, dim3(256), 0, s, p, rt); break;
    default: hipLaunchKernelGGL((vq_assign_kernel<0, false, RATE>), grid, dim3(256), 0, s, p, rt); break;
    }
}

// the plain launch (rate == nullptr) and the per-vector-lambda one share the plan, the workspace and the fold
int vq_assign_launch(const float* x, const float* cb_packed, const VqRate* rate, int64_t* codes, int32_t N, int32_t m, int32_t d,
                     int32_t h, int32_t w, int32_t k, void* workspace, void* stream) {
    VqAssignPlan pl;
    const int status = vq_assign_plan(N, m, d, h, w, k, pl);
    if (status != MCQ_OK) return status;
    VqK& p = pl.p;
    vq_operands(p, x, cb_packed);
    p.codes = codes;
    if (!workspace) p.zs = 1;                                // (without a workspace: one workgroup per vector tile, as before)
    const size_t nvec = (size_t)N * m * h * w;
    p.ws_best = static_cast<float*>(workspace);
    p.ws_idx = reinterpret_cast<int*>(p.ws_best + (size_t)p.zs * nvec);
    const int per_wg = 4 >> p.cs_log2;
    const unsigned gx = (unsigned)((pl.vtiles + per_wg - 1) / per_wg);
    const int gz = workspace ? pl.gz : 1;                    // the ranges that own a tile; the kernel deals by p.zs, the fold reads gz
    const dim3 grid(gx, (unsigned)m, (unsigned)gz);
    if (rate) {
        VqRateArg<true> rt;
        static_cast<VqRate&>(rt) = *rate;
        vq_assign_run<true>(pl.instance, grid, (hipStream_t)stream, p, rt);
    } else {
        vq_assign_run<false>(pl.instance, grid, (hipStream_t)stream, p, VqRateArg<false>{});
    }
    if (p.zs > 1)
        hipLaunchKernelGGL(vq_fold_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p.ws_best, p.ws_idx, gz,
                           nvec, codes);
    return mcq_check_launch();
}
}  // namespace

extern "C" int mcq_vq_assign_ws_f32(const float* x, const float* cb_packed, int64_t* codes, int32_t N, int32_t m, int32_t d,
                                    int32_t h, int32_t w, int32_t k, void* workspace, void* stream) {
    if (!x || !cb_packed || !codes || N <= 0 || m <= 0 || d <= 0 || h <= 0 || w <= 0 || k <= 0) return MCQ_EINVAL;
    return vq_assign_launch(x, cb_packed, nullptr, codes, N, m, d, h, w, k, workspace, stream);
}

extern "C" int mcq_vq_assign_rate_map_f32(const float* x, const float* cb_packed, const float* bits_packed, const float* lam,
                                          int64_t stride_n, int64_t stride_y, int64_t stride_x, int64_t* codes, int32_t N, int32_t m,
                                          int32_t d, int32_t h, int32_t w, int32_t k, void* workspace, void* stream) {
    if (!x || !cb_packed || !bits_packed || !lam || !codes || N <= 0 || m <= 0 || d <= 0 || h <= 0 || w <= 0 || k <= 0) return MCQ_EINVAL;
    if (stride_n < 0 || stride_y < 0 || stride_x < 0) return MCQ_EINVAL;
    const VqRate rt{bits_packed, lam, (long long)stride_n, (long long)stride_y, (long long)stride_x};
    return vq_assign_launch(x, cb_packed, &rt, codes, N, m, d, h, w, k, workspace, stream);
}

extern "C" int mcq_vq_gather_f32(const int64_t* codes, const float* codebook, float* out, float* out_silu, int32_t N,
                                 int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, void* stream) {
    if (!codes || !codebook || !out || N <= 0 || m <= 0 || d <= 0 || h <= 0 || w <= 0 || k <= 0) return MCQ_EINVAL;
    const size_t total = (size_t)N * m * h * w;
    hipLaunchKernelGGL(vq_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes,
                       codebook, out, out_silu, N, m, d, h * w, k);
    return mcq_check_launch();
}

extern "C" int mcq_add_f32(const float* a, const float* b, float* out, float* out_silu, int64_t n, void* stream) {
    if (!a || !b || !out || n <= 0) return MCQ_EINVAL;
    const int64_t threads = (n + 3) / 4;
    hipLaunchKernelGGL(add_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, out_silu, n);
    return mcq_check_launch();
}

extern "C" int mcq_add3_f32(const float* a, const float* b, const float* c, float* out, int64_t n, void* stream) {
    if (!a || !b || !c || !out || n <= 0) return MCQ_EINVAL;
    const int64_t threads = (n + 3) / 4;
    hipLaunchKernelGGL(add3_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, c, out, n);
    return mcq_check_launch();
}

extern "C" int mcq_detransform_u8(const float* x, uint8_t* out, int64_t n, void* stream) {
    if (!x || !out || n <= 0) return MCQ_EINVAL;
    hipLaunchKernelGGL(detransform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, n);
    return mcq_check_launch();
}

extern "C" const char* mcq_version(void) { return "mcquic_hip 0.3.0 gfx950"; }
extern "C" int32_t mcq_abi_version(void) { return MCQ_ABI_VERSION; }
