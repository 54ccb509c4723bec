// The other half of a Lloyd iteration on the device (gfx950): mcq_vq_assign_f32 (csrc/vq.hip) makes the codes, these kernels
// turn them into new codewords.
//
//   km_accumulate_kernel   per codeword: the sum of its latent vectors, the sum of their squared norms and their number, added
//                          onto running accumulators (double / double / int64), so that several batches fold into one update
//   km_update_kernel       codeword = float32(sum / count) where count > 0, the inertia against the OLD codewords, the number
//                          of codewords left untouched
//   km_seed_kernel         codeword = a data vector picked by the counter-based generator (csrc/mcq_rng.h, stream 2): Forgy
//                          seeding of a whole codebook, or of the codewords whose count is zero
//   km_zero_kernel         the accumulators' zeroing (a kernel, not a memset: see vq_bwd_mfma.hip)
//
// Form of the accumulation (DESIGN.md, section "k-means"): every codeword is OWNED by one workgroup, so nothing is added with
// atomics and every sum has one fixed order.  A wave walks its segment of the code array 256 entries at a time (four loads in
// flight), compares them with its codeword, and takes the matching lanes out of the ballots in ascending order; lane j then adds
// channel j of each matching vector onto its double.  The codes (8 bytes per vector and group) are re-read once per codeword out
// of L2; the latent vectors are read exactly once over the whole launch.  Launches with few codewords range the vectors over up
// to 16 waves per codeword (contiguous segments, folded in segment order through LDS): the number of segments follows from the
// shapes alone, so two launches of the same shapes add in the same order and give the same bits.
// A code outside [0, k) matches no workgroup: such a vector is not counted and nothing is written for it.
#include "mcq_common.h"
#include "mcq_rng.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int KM_MAXW = 16;            // waves (vector segments) per codeword at most
constexpr int KM_WAVES_WANTED = 8192;  // 256 CUs x 32 waves: segments are added until the launch has about this many waves
constexpr int KM_UPD_T = 1024;

struct KmAccK {
    const float* x;                    // [N, m*d, h, w]
    const long long* codes;            // [N, m, h, w]
    double* sums;                      // [m, k, d]
    double* sqsums;                    // [m, k]
    long long* counts;                 // [m, k]
    int m, d, hw, k;
    long long V;                       // N * h * w
    long long seg;                     // vectors per wave, a multiple of 256
    int step_n, step_p;                // 256 / hw, 256 % hw: what 256 vectors further means for (image, pixel)
};

__device__ __forceinline__ long long km_readlane64(long long v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(unsigned long long)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ double km_wave_sum(double v) {              // a fixed butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// workgroup b = g * k + c: codeword c of group g; wave w of the workgroup: vectors [w * seg, (w + 1) * seg)
__global__ __launch_bounds__(64 * KM_MAXW) void km_accumulate_kernel(KmAccK q) {
    extern __shared__ double km_lds[];                                  // [nwaves][64] sums, [nwaves][64] squares, [nwaves] counts
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, nwaves = (int)blockDim.x >> 6;
    double* sh_s = km_lds;
    double* sh_q = km_lds + nwaves * 64;
    long long* sh_c = reinterpret_cast<long long*>(km_lds + nwaves * 128);
    const long long gc = (long long)blockIdx.x;
    const int g = (int)(gc / q.k);
    const long long c = gc - (long long)g * q.k;
    const long long v0 = (long long)wave * q.seg;
    const long long vend = v0 + q.seg < q.V ? v0 + q.seg : q.V;
    double sq_total = 0.0;
    long long cnt = 0;
    for (int jb = 0; jb < q.d; jb += 64) {                             // (d <= 64 in every model: one pass)
        const int j = jb + lane;
        const bool jok = j < q.d;
        const long long joff = (long long)j * q.hw;
        double s = 0.0, s2 = 0.0;
        // (image, pixel) of this lane's vector in each of the four 64-vector chunks of a step
        int n[4], p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long v = v0 + e * 64 + lane;
            n[e] = (int)(v / q.hw);
            p[e] = (int)(v - (long long)n[e] * q.hw);
        }
        for (long long base = v0; base < vend; base += 256) {
            long long code[4], xoff[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long v = base + e * 64 + lane;
                const long long plane = (long long)n[e] * q.m + g;
                code[e] = v < vend ? q.codes[plane * q.hw + p[e]] : -1;      // (-1 matches no codeword)
                xoff[e] = plane * q.d * q.hw + p[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned long long mask = __ballot(code[e] == c);
                if (jb == 0) cnt += __popcll(mask);
                while (mask) {                                          // matching vectors in ascending order, four loads in flight
                    long long off[4];
                    bool ok[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        ok[t] = mask != 0ull;
                        const int b = ok[t] ? __builtin_ctzll(mask) : 0;
                        off[t] = km_readlane64(xoff[e], b);
                        mask &= mask - 1ull;
                    }
                    float val[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) val[t] = (ok[t] && jok) ? q.x[off[t] + joff] : 0.0f;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {                       // (+ 0.0 for a slot without a vector leaves the sums as they are)
                        const double dv = (double)val[t];
                        s += dv;
                        s2 += dv * dv;
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                n[e] += q.step_n;
                p[e] += q.step_p;
                if (p[e] >= q.hw) { p[e] -= q.hw; n[e] += 1; }
            }
        }
        sh_s[wave * 64 + lane] = s;
        sh_q[wave * 64 + lane] = s2;
        if (jb == 0 && lane == 0) sh_c[wave] = cnt;
        __syncthreads();
        if (wave == 0) {                                                // segments in order
            double ts = 0.0, tq = 0.0;
            for (int w = 0; w < nwaves; ++w) { ts += sh_s[w * 64 + lane]; tq += sh_q[w * 64 + lane]; }
            if (jok) q.sums[gc * q.d + j] += ts;
            sq_total += km_wave_sum(tq);
            if (jb == 0) {
                long long tc = 0;
                for (int w = 0; w < nwaves; ++w) tc += sh_c[w];
                cnt = tc;
            }
        }
        __syncthreads();
    }
    if (wave == 0 && lane == 0) {
        q.sqsums[gc] += sq_total;
        q.counts[gc] += cnt;
    }
}

// one workgroup per group; thread t takes codewords t, t + 1024, ...; thread 0 adds the per-codeword terms in ascending order
__global__ __launch_bounds__(KM_UPD_T) void km_update_kernel(float* __restrict__ codebook, const double* __restrict__ sums,
                                                            const double* __restrict__ sqsums, const long long* __restrict__ counts,
                                                            double* __restrict__ inertia, long long* __restrict__ empty, int k, int d) {
    __shared__ double term[KM_UPD_T];
    __shared__ int sh_empty;
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (tid == 0) sh_empty = 0;
    double total = 0.0;
    int untouched = 0;
    for (int c0 = 0; c0 < k; c0 += KM_UPD_T) {
        const int c = c0 + tid;
        double t = 0.0;
        if (c < k) {
            const size_t idx = (size_t)g * k + c;
            const long long cnt = counts[idx];
            float* row = codebook + idx * d;
            const double* srow = sums + idx * d;
            double dot = 0.0, c2 = 0.0;
            for (int j = 0; j < d; ++j) {
                const double cj = (double)row[j];
                dot += cj * srow[j];
                c2 += cj * cj;
            }
            t = (sqsums[idx] - 2.0 * dot) + (double)cnt * c2;
            if (cnt > 0) {
                const double n = (double)cnt;
                for (int j = 0; j < d; ++j) row[j] = (float)(srow[j] / n);
            } else {
                ++untouched;
            }
        }
        term[tid] = t;
        __syncthreads();
        if (tid == 0) {
            const int lim = k - c0 < KM_UPD_T ? k - c0 : KM_UPD_T;
#pragma unroll 8
            for (int i = 0; i < lim; ++i) total += term[i];
        }
        __syncthreads();
    }
    if (untouched) atomicAdd(&sh_empty, untouched);
    __syncthreads();
    if (tid == 0) {
        inertia[g] = total;
        empty[g] = (long long)sh_empty;
    }
}

// one thread per (g, c, j)
__global__ __launch_bounds__(256) void km_seed_kernel(const float* __restrict__ x, float* __restrict__ codebook,
                                                      const long long* __restrict__ counts, const unsigned long long* __restrict__ rng_state,
                                                      int m, int d, int hw, int k, long long V, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t gc = i / (size_t)d;
    const int j = (int)(i - gc * (size_t)d);
    if (counts && counts[gc] != 0) return;
    const RngState rs = rng_load(rng_state);
    const float u = rng_uniform(rs, 2u, gc);
    long long pick = (long long)((double)u * (double)V);               // floor(u V), exact in double: u = i / 2^24, V < 2^31
    if (pick > V - 1) pick = V - 1;
    const long long n = pick / hw, p = pick - n * hw;
    const long long g = (long long)(gc / (size_t)k);
    codebook[i] = x[((n * m + g) * d + j) * hw + p];
}

__global__ __launch_bounds__(256) void km_zero_kernel(double* __restrict__ sums, double* __restrict__ sqsums, long long* __restrict__ counts,
                                                      size_t mk, size_t mkd) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < mkd; i += (size_t)gridDim.x * 256) {
        sums[i] = 0.0;
        if (i < mk) { sqsums[i] = 0.0; counts[i] = 0; }
    }
}

}  // namespace

extern "C" int mcq_vq_kmeans_zero(double* sums, double* sqsums, int64_t* counts, int32_t m, int32_t k, int32_t d, void* stream) {
    if (!sums || !sqsums || !counts || m <= 0 || k <= 0 || d <= 0) return MCQ_EINVAL;
    const size_t mk = (size_t)m * k, mkd = mk * d;
    const size_t blocks = (mkd + 255) / 256;
    hipLaunchKernelGGL(km_zero_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, sums, sqsums,
                       reinterpret_cast<long long*>(counts), mk, mkd);
    return mcq_check_launch();
}

extern "C" int mcq_vq_kmeans_accumulate_f32(const float* x, const int64_t* codes, double* sums, double* sqsums, int64_t* counts, int32_t N,
                                            int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, void* stream) {
    if (!x || !codes || !sums || !sqsums || !counts || N <= 0 || m <= 0 || d <= 0 || h <= 0 || w <= 0 || k <= 0) return MCQ_EINVAL;
    const long long hw = (long long)h * w, V = (long long)N * hw;
    if (V > 0x7fffffffLL || (long long)m * k > 0x7fffffffLL) return MCQ_ETOOLARGE;
    KmAccK q;
    q.x = x; q.codes = reinterpret_cast<const long long*>(codes); q.sums = sums; q.sqsums = sqsums;
    q.counts = reinterpret_cast<long long*>(counts);
    q.m = m; q.d = d; q.hw = (int)hw; q.k = k; q.V = V;
    int waves = 1;                     // (from the shapes alone: the order of every sum is a function of the shapes)
    while (waves < KM_MAXW && (long long)m * k * waves < KM_WAVES_WANTED && V > (long long)waves * 256) waves *= 2;
    q.seg = ((V + waves - 1) / waves + 255) / 256 * 256;
    q.step_n = (int)(256 / hw); q.step_p = (int)(256 % hw);
    hipLaunchKernelGGL(km_accumulate_kernel, dim3((unsigned)((long long)m * k)), dim3(64u * (unsigned)waves), (size_t)waves * (128 + 1) * sizeof(double),
                       (hipStream_t)stream, q);
    return mcq_check_launch();
}

extern "C" int mcq_vq_kmeans_update_f32(float* codebook, const double* sums, const double* sqsums, const int64_t* counts, double* inertia,
                                        int64_t* empty, int32_t m, int32_t k, int32_t d, void* stream) {
    if (!codebook || !sums || !sqsums || !counts || !inertia || !empty || m <= 0 || k <= 0 || d <= 0) return MCQ_EINVAL;
    hipLaunchKernelGGL(km_update_kernel, dim3((unsigned)m), dim3(KM_UPD_T), 0, (hipStream_t)stream, codebook, sums, sqsums,
                       reinterpret_cast<const long long*>(counts), inertia, reinterpret_cast<long long*>(empty), k, d);
    return mcq_check_launch();
}

extern "C" int mcq_vq_kmeans_seed_f32(const float* x, float* codebook, const int64_t* counts_or_null, const uint64_t* rng_state, int32_t N,
                                      int32_t m, int32_t d, int32_t h, int32_t w, int32_t k, void* stream) {
    if (!x || !codebook || !rng_state || N <= 0 || m <= 0 || d <= 0 || h <= 0 || w <= 0 || k <= 0) return MCQ_EINVAL;
    const long long hw = (long long)h * w, V = (long long)N * hw;
    if (V > 0x7fffffffLL || (long long)m * k > 0x7fffffffLL) return MCQ_ETOOLARGE;
    const size_t total = (size_t)m * k * d;
    if ((total + 255) / 256 > 0x7fffffffull) return MCQ_ETOOLARGE;
    hipLaunchKernelGGL(km_seed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, codebook,
                       reinterpret_cast<const long long*>(counts_or_null), reinterpret_cast<const unsigned long long*>(rng_state), m, d,
                       (int)hw, k, V, total);
    return mcq_check_launch();
}
