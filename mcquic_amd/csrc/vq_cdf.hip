// The rate side on the device, for gfx950: the entropy coder's 16-bit quantized CDF tables built from the frequency rows where they
// live, and the length in bits those tables charge for a batch of codes -- no host loop, no host read, plain stores, no atomics.
//
//   vq_cdf_kernel        one workgroup per (level, group) row, all levels in ONE launch: float32 pmf row [k] -> uint32 table [k + 1] and
//                        one int32 status word.  The arithmetic is that of mcq_pmf_to_quantized_cdf (rans.cpp) at precision 16:
//                          1. c_i = round(p_i * 65536.f), halves away from zero          (float32 product, exact: a power of two)
//                          2. total = sum c_i                                              (uint32)
//                          3. w_i = (65536 * c_i) / total                                  (64-bit integers)
//                          4. cdf_i = w_0 + ... + w_{i-1}                                  (the inclusive scan behind cdf[0] = 0)
//                          5. cdf[k] = 65536                                               (the last bin takes what the floors left over)
//                          6. the steal loop: for i ascending, an empty bin (cdf[i] == cdf[i + 1]) takes one count from the first
//                             bin among those of least width > 1, by +-1 over the table entries between the two.
//                        With `normalize` the row is first divided by its sum: per-lane double partials over i = lane, lane + 1024, ...,
//                        a fixed tree, rounded ONCE to float32, then an IEEE float32 division (the rule of vq_reassign.hip's row sum).
//   vq_code_bits_kernel  one workgroup per (image, level), all levels in ONE launch: sum over groups g and positions of
//                        16 - log2(cdf_g[c + 1] - cdf_g[c]) for the int64 codes [n, m, h, w], in double: per-lane partials over
//                        s = lane, lane + 1024, ..., then a fixed tree.  A code outside [0, k) (or a bin of width 0: not a table this
//                        file makes) adds nothing and sets the (image, level)'s error word, which every launch writes (0 or 1).
//
// The steal loop without its k steps.  In widths (w_i = cdf[i + 1] - cdf[i], after step 5 they sum to 65536) a steal for bin i from
// donor j is w_i: 0 -> 1 and w_j -= 1; the +-1 over the entries between them leaves every other width as it was.  So
//   * the empty bins are those of step 5, and each ends at width 1: no steal empties a bin (a donor had width > 1) or fills a later one;
//   * a donor of width f > 2 is, after giving, the ONLY bin of width f - 1 below every other width > 1: it gives again, until it is 1.
//     The donors therefore give in ascending order of (width, index) of step 5's widths, each all it can spare (f - 1), and the loop
//     is: Z = number of empty bins; F = the least width with  cap(F) = sum over {1 < w_j <= F} of (w_j - 1) >= Z;  every donor below F
//     ends at 1; of the R = Z - cap(F - 1) counts still owed, the donors of width F give in index order, R / (F - 1) of them all they
//     have and the next one the remainder.  cap(65536) < Z is the host's "no donor left" (it needs more bins than counts: never with
//     k <= 8192, kept as status 3 all the same).
// The table is then the scan of the final widths: entry for entry the host's, whose loop it replaces by 16 workgroup sums (the search for
// F) instead of up to k argmin passes.  tests/test_gpu_quantized_cdf.py holds it to the host function bit for bit.
//
// Status words (int32 per row, (level, group) order): 0 valid; 1 a negative or non-finite element, or one whose scaled value or the
// scaled total does not fit 32 bits (the host's conversion is undefined there); 2 a zero total (with `normalize`: a row sum of zero,
// tested before the division); 3 no donor left.  A row with a non-zero status leaves its table unspecified.
#include "mcq_common.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int CDF_T = 1024;                         // lanes per workgroup
constexpr int CDF_W = CDF_T / 64;                   // waves
constexpr int CDF_KMAX = MCQ_CDF_MAX_K;             // the longest row the LDS array below holds
constexpr int CDF_E = CDF_KMAX / CDF_T;             // row entries per lane
static_assert(CDF_KMAX % CDF_T == 0, "whole entries per lane");

struct CdfK {
    const float* pmf[MCQ_VQ_MAX_LEVELS];            // level l: [m_l, k_l]
    uint32_t* cdf[MCQ_VQ_MAX_LEVELS];               // level l: [m_l, k_l + 1]
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t row0[MCQ_VQ_MAX_LEVELS + 1];            // first (level, group) row of level l in blockIdx order
    int32_t levels;
    int32_t normalize;
    int32_t* status;                                // [rows]
};

// sum of one value per lane over the workgroup, the same in every lane; `sm` holds CDF_W values
template <typename T>
__device__ __forceinline__ T cdf_block_sum(T v, T* sm) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    T all = 0;
#pragma unroll
    for (int w = 0; w < CDF_W; ++w) all += sm[w];
    __syncthreads();
    return all;
}

// exclusive scan of one value per lane over the workgroup, lane order; *total = the sum
__device__ __forceinline__ uint32_t cdf_block_scan(uint32_t v, uint32_t* sm, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(s, off);
        if (lane >= off) s += u;
    }
    if (lane == 63) sm[wave] = s;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CDF_W; ++w) {
        const uint32_t t = sm[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    __syncthreads();
    *total = all;
    return s - v + before;
}

__global__ __launch_bounds__(CDF_T) void vq_cdf_kernel(CdfK q) {
    __shared__ uint32_t row[CDF_KMAX];              // the scaled counts, then the widths, then the table
    __shared__ double smd[CDF_W];
    __shared__ unsigned long long sml[CDF_W];
    __shared__ uint32_t smu[CDF_W];

    int lv = 0;
    while (lv + 1 < q.levels && (int)blockIdx.x >= q.row0[lv + 1]) ++lv;
    const int g = (int)blockIdx.x - q.row0[lv];
    const int k = q.k[lv];
    const float* p = q.pmf[lv] + (size_t)g * k;
    uint32_t* out = q.cdf[lv] + (size_t)g * (k + 1);
    const int tid = threadIdx.x;

    float pv[CDF_E];
    double part = 0.0;
#pragma unroll
    for (int e = 0; e < CDF_E; ++e) {
        const int i = tid + e * CDF_T;
        pv[e] = i < k ? p[i] : 0.0f;
        part += (double)pv[e];
    }
    if (q.normalize) {                              // the row sum: double, lane-strided partials in index order, a fixed tree, one rounding
        const float sum = (float)cdf_block_sum<double>(part, smd);
        if (sum == 0.0f) {                          // a zero total, as without `normalize` (0 / 0 would report a bad element); uniform
            if (tid == 0) q.status[blockIdx.x] = 2;
            return;
        }
#pragma unroll
        for (int e = 0; e < CDF_E; ++e) pv[e] = pv[e] / sum;
    }

    // steps 1 and 2
    uint32_t c[CDF_E];
    unsigned long long tot = 0;
    uint32_t bad = 0;
#pragma unroll
    for (int e = 0; e < CDF_E; ++e) {
        const int i = tid + e * CDF_T;
        const float x = pv[e] * 65536.0f;
        const bool ok = i >= k || (pv[e] >= 0.0f && x < 4294967296.0f);        // (false for a NaN, an infinity, a negative element)
        bad |= ok ? 0u : 1u;
        c[e] = ok && i < k ? (uint32_t)__builtin_roundf(x) : 0u;
        tot += c[e];
    }
    bad = cdf_block_sum<uint32_t>(bad, smu);
    tot = cdf_block_sum<unsigned long long>(tot, sml);
    int status = bad || tot > 0xffffffffull ? 1 : tot == 0 ? 2 : 0;
    if (status) {                                   // (the same in every lane)
        if (tid == 0) q.status[blockIdx.x] = status;
        return;
    }

    // step 3, the widths of steps 4 and 5
    const uint32_t total = (uint32_t)tot;
    uint32_t wsum = 0;
#pragma unroll
    for (int e = 0; e < CDF_E; ++e) {
        const int i = tid + e * CDF_T;
        if (i < k) {
            const uint32_t w = (uint32_t)((65536ull * c[e]) / total);
            row[i] = w;
            wsum += i < k - 1 ? w : 0u;
        }
    }
    wsum = cdf_block_sum<uint32_t>(wsum, smu);      // (<= 65536: the floors of shares of 65536)
    if (tid == 0) row[k - 1] = 65536u - wsum;       // cdf[k] = 65536
    __syncthreads();

    // from here on lane t owns the entries [t n, t n + n) of the row: index order is lane order
    const int n = (k + CDF_T - 1) / CDF_T;
    const int first = tid * n < k ? tid * n : k, last = first + n < k ? first + n : k;
    uint32_t w[CDF_E];
    uint32_t empty = 0;
#pragma unroll
    for (int e = 0; e < CDF_E; ++e) {
        w[e] = first + e < last ? row[first + e] : 1u;      // (1: neither empty nor a donor)
        empty += w[e] == 0u ? 1u : 0u;
    }
    const uint32_t Z = cdf_block_sum<uint32_t>(empty, smu);
    if (Z) {                                        // step 6 (uniform)
        uint32_t lo = 2, hi = 65536, cap_hi, cap_below = 0;
        {
            uint32_t s = 0;
#pragma unroll
            for (int e = 0; e < CDF_E; ++e) s += w[e] > 1u ? w[e] - 1u : 0u;
            cap_hi = cdf_block_sum<uint32_t>(s, smu);
        }
        if (cap_hi < Z) {
            if (tid == 0) q.status[blockIdx.x] = 3;
            return;
        }
        while (lo < hi) {                           // the least F with cap(F) >= Z; cap_below = cap(lo - 1)
            const uint32_t mid = (lo + hi) >> 1;
            uint32_t s = 0;
#pragma unroll
            for (int e = 0; e < CDF_E; ++e) s += w[e] > 1u && w[e] <= mid ? w[e] - 1u : 0u;
            s = cdf_block_sum<uint32_t>(s, smu);
            if (s >= Z) hi = mid;
            else { lo = mid + 1; cap_below = s; }
        }
        const uint32_t F = lo, owed = Z - cap_below;        // 1 <= owed <= (number of width-F donors) (F - 1)
        const uint32_t full = owed / (F - 1u), rem = owed % (F - 1u);
        uint32_t mine = 0;
#pragma unroll
        for (int e = 0; e < CDF_E; ++e) mine += w[e] == F ? 1u : 0u;
        uint32_t donors;
        uint32_t rank = cdf_block_scan(mine, smu, &donors);
#pragma unroll
        for (int e = 0; e < CDF_E; ++e) {
            const uint32_t v = w[e];
            if (v == F) {
                w[e] = rank < full ? 1u : (rank == full ? F - rem : F);
                ++rank;
            } else if (v == 0u || (v > 1u && v < F)) {
                w[e] = 1u;
            }
        }
    }

    // the table: the scan of the widths
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < CDF_E; ++e) mine += first + e < last ? w[e] : 0u;
    uint32_t all;
    uint32_t at = cdf_block_scan(mine, smu, &all);
#pragma unroll
    for (int e = 0; e < CDF_E; ++e) {
        if (first + e < last) {
            row[first + e] = at;
            at += w[e];
        }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < CDF_E; ++e) {
        const int i = tid + e * CDF_T;
        if (i < k) out[i] = row[i];
    }
    if (tid == 0) {
        out[k] = 65536u;
        q.status[blockIdx.x] = 0;
    }
}

struct CodeBitsK {
    const long long* codes[MCQ_VQ_MAX_LEVELS];      // level l: [n, m_l, h_l, w_l]
    const uint32_t* cdf[MCQ_VQ_MAX_LEVELS];         // level l: [m_l, k_l + 1]
    int32_t m[MCQ_VQ_MAX_LEVELS];
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t hw[MCQ_VQ_MAX_LEVELS];                  // h_l w_l
    int32_t levels;                                 // of this launch
    int32_t level0, row_levels;                     // this launch's first level among the `row_levels` columns of `bits` / `error`
    double* bits;                                   // [n, row_levels]
    int32_t* error;                                 // [n, row_levels]
};

__global__ __launch_bounds__(CDF_T) void vq_code_bits_kernel(CodeBitsK q) {
    __shared__ double smd[CDF_W];
    __shared__ uint32_t smu[CDF_W];
    const int lv = (int)blockIdx.x, img = (int)blockIdx.y;
    const int m = q.m[lv], k = q.k[lv], hw = q.hw[lv];
    const int count = m * hw;                       // (<= 2^30: checked on the host)
    const long long* code = q.codes[lv] + (size_t)img * count;
    const uint32_t* cdf = q.cdf[lv];
    double part = 0.0;
    uint32_t bad = 0;
    for (int s = threadIdx.x; s < count; s += CDF_T) {
        const long long c = code[s];
        const uint32_t* t = cdf + (size_t)(s / hw) * (k + 1);
        const bool in = c >= 0 && c < k;
        const uint32_t width = in ? t[c + 1] - t[c] : 0u;
        bad |= width == 0u ? 1u : 0u;
        part += width ? 16.0 - log2((double)width) : 0.0;
    }
    // a fixed tree: within the wave, then over the waves
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    if ((threadIdx.x & 63) == 0) smd[threadIdx.x >> 6] = part;
    bad = cdf_block_sum<uint32_t>(bad, smu);        // (its barriers also publish smd)
    if (threadIdx.x == 0) {
        double v[CDF_W];
#pragma unroll
        for (int w = 0; w < CDF_W; ++w) v[w] = smd[w];
#pragma unroll
        for (int off = CDF_W / 2; off >= 1; off >>= 1)
#pragma unroll
            for (int w = 0; w < off; ++w) v[w] += v[w + off];
        const size_t at = (size_t)img * q.row_levels + q.level0 + lv;
        q.bits[at] = v[0];
        q.error[at] = bad ? 1 : 0;
    }
}

}  // namespace

extern "C" int32_t mcq_cdf_max_k(void) { return CDF_KMAX; }

extern "C" int mcq_pmf_to_quantized_cdf_dev(const float* const* pmf, uint32_t* const* cdf, const int32_t* m, const int32_t* k, int32_t levels,
                                            int32_t normalize, int32_t* status, void* stream) {
    if (!pmf || !cdf || !m || !k || !status || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return MCQ_EINVAL;
    CdfK q;
    int rows = 0;
    for (int l = 0; l < levels; ++l) {
        if (!pmf[l] || !cdf[l] || m[l] <= 0 || k[l] <= 0) return MCQ_EINVAL;
        if (k[l] > CDF_KMAX) return MCQ_EINVAL;     // the row does not fit the LDS array
        q.pmf[l] = pmf[l]; q.cdf[l] = cdf[l]; q.k[l] = k[l]; q.row0[l] = rows;
        rows += m[l];
    }
    q.row0[levels] = rows;
    q.levels = levels; q.normalize = normalize ? 1 : 0; q.status = status;
    hipLaunchKernelGGL(vq_cdf_kernel, dim3((unsigned)rows), dim3(CDF_T), 0, (hipStream_t)stream, q);
    return mcq_check_launch();
}

extern "C" int mcq_code_bits(const int64_t* const* codes, const uint32_t* const* cdf, const int32_t* m, const int32_t* k, const int32_t* hw,
                             int32_t levels, int32_t n, int32_t level0, int32_t row_levels, double* bits, int32_t* error, void* stream) {
    if (!codes || !cdf || !m || !k || !hw || !bits || !error || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return MCQ_EINVAL;
    if (n <= 0 || level0 < 0 || row_levels < level0 + levels) return MCQ_EINVAL;
    if (n > 65535) return MCQ_ETOOLARGE;            // (grid y)
    CodeBitsK q;
    for (int l = 0; l < levels; ++l) {
        if (!codes[l] || !cdf[l] || m[l] <= 0 || k[l] <= 0 || hw[l] <= 0) return MCQ_EINVAL;
        if ((long long)m[l] * hw[l] > MCQ_CODE_BITS_MAX_SYMBOLS) return MCQ_ETOOLARGE;     // (the lanes' int index steps past the count by < 1024)
        q.codes[l] = reinterpret_cast<const long long*>(codes[l]); q.cdf[l] = cdf[l];
        q.m[l] = m[l]; q.k[l] = k[l]; q.hw[l] = hw[l];
    }
    q.levels = levels; q.level0 = level0; q.row_levels = row_levels; q.bits = bits; q.error = error;
    hipLaunchKernelGGL(vq_code_bits_kernel, dim3((unsigned)levels, (unsigned)n), dim3(CDF_T), 0, (hipStream_t)stream, q);
    return mcq_check_launch();
}
