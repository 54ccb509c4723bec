// The trainer's periodic log payload made on the device (gfx950): what the reference's `MainTrainer.log` (mcquic/train/trainer.py:463-491)
// builds on the host from whole tensors of the step, here as launches that leave a few KB for one copy (host mirror:
// mcquic_amd.monitor.StepSnapshot).
//   histogram        np.histogram(v, bins) of a float32 slab, v = x or log10(clamp(-x, eps)) evaluated in registers, never stored:
//     hist_minmax_kernel     pass 1, stage 1: per-workgroup min / max over the finite v, counts of finite and non-finite v
//     hist_range_kernel      pass 1, stage 2: ONE workgroup folds those in index order, fixes the range, writes np.linspace's edges
//                            (float64), the two totals, and zeroes `counts` (a kernel, not a memset node: DESIGN.md, "graph replays")
//     hist_bin_kernel        pass 2: numpy's uniform-bin index with its two edge corrections, in float64; per-workgroup LDS counts,
//                            folded into `counts` with integer atomics (exact in any order)
//   log_distance     the same transform, written out (pins the transform element by element)
//   code image       `Validator.visualizeIntermediate` (mcquic/validate/validator.py:30-38): code_max_kernel (ONE workgroup, the maximum
//                    over all groups stays on the device), code_image_kernel (group 0, DeTransform, the 4 x 4 block of nearest x4)
//   frequencies      group 0 of every level's normalised frequency EMA and `Compressor.CodeUsage`: snap_freq_kernel, snap_usage_kernel
// The launch boundary is the only synchronisation between the kernels of one call.  Every float reduction runs in a fixed order.
#include "mcq_common.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int HIST_T = 256;
constexpr int HIST_CHUNK = 4096;               // elements a workgroup takes per trip: four float4 per thread when the slab is 16-byte aligned
constexpr int HIST_MAX_GROUPS = 1024;          // workgroups of the two passes (a 33 MB slab: 2048 chunks, two trips each)
constexpr int HIST_MAX_BINS = 4096;
constexpr long long HIST_MAX_N = 1LL << 40;    // (a workgroup's LDS counts are int32: at most n / HIST_MAX_GROUPS + HIST_CHUNK per bin)

struct HistRange {                             // the head of the workspace, written by hist_range_kernel
    double first, last, denom, step;           // np.histogram's (first_edge, last_edge), last - first, and linspace's step (last - first) / bins
};

__host__ __device__ inline long long hist_chunks(long long n) { return (n + HIST_CHUNK - 1) / HIST_CHUNK; }
inline int hist_groups(long long n) {
    const long long c = hist_chunks(n);
    return (int)(c < HIST_MAX_GROUPS ? c : HIST_MAX_GROUPS);
}

// neg, clamp(min), log10: one float32 rounding per op, as torch evaluates `(-x).clamp(eps).log10()`; clamp hands a NaN through
template <int TR>
__device__ __forceinline__ float hist_value(float x, float eps) {
    if (TR == 0) return x;
    const float nx = -x;
    const float c = nx != nx ? nx : (nx < eps ? eps : nx);
    return log10f(c);
}

// every element of this workgroup's chunks, once: f(v).  Full chunks of a 16-byte aligned slab go as float4 loads.
template <int TR, typename F>
__device__ __forceinline__ void hist_walk(const float* __restrict__ x, long long n, float eps, bool aligned, F f) {
    const long long chunks = hist_chunks(n);
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long base = c * HIST_CHUNK;
        if (aligned && base + HIST_CHUNK <= n) {
            const f32x4v* p = reinterpret_cast<const f32x4v*>(x + base);
#pragma unroll
            for (int j = 0; j < HIST_CHUNK / (4 * HIST_T); ++j) {
                const f32x4v q = p[j * HIST_T + threadIdx.x];
                f(hist_value<TR>(q[0], eps)); f(hist_value<TR>(q[1], eps)); f(hist_value<TR>(q[2], eps)); f(hist_value<TR>(q[3], eps));
            }
        } else {
            const long long end = base + HIST_CHUNK < n ? base + HIST_CHUNK : n;
            for (long long i = base + threadIdx.x; i < end; i += HIST_T) f(hist_value<TR>(x[i], eps));
        }
    }
}

template <int TR>
__global__ __launch_bounds__(HIST_T) void hist_minmax_kernel(const float* __restrict__ x, long long n, float eps, int aligned,
                                                             float* __restrict__ pmin, float* __restrict__ pmax,
                                                             long long* __restrict__ pfin, long long* __restrict__ pbad) {
    __shared__ float smn[HIST_T / 64], smx[HIST_T / 64];
    __shared__ long long sfin[HIST_T / 64], sbad[HIST_T / 64];
    float mn = __builtin_inff(), mx = -__builtin_inff();
    long long fin = 0, bad = 0;
    hist_walk<TR>(x, n, eps, aligned != 0, [&](float v) {
        if (__builtin_isfinite(v)) {
            mn = fminf(mn, v); mx = fmaxf(mx, v); ++fin;
        } else {
            ++bad;
        }
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off)); mx = fmaxf(mx, __shfl_xor(mx, off));
        fin += __shfl_xor(fin, off); bad += __shfl_xor(bad, off);
    }
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; sfin[threadIdx.x >> 6] = fin; sbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < HIST_T / 64; ++w) {
            mn = fminf(mn, smn[w]); mx = fmaxf(mx, smx[w]); fin += sfin[w]; bad += sbad[w];
        }
        pmin[blockIdx.x] = mn; pmax[blockIdx.x] = mx; pfin[blockIdx.x] = fin; pbad[blockIdx.x] = bad;
    }
}

// np.linspace(first, last, bins + 1)[i] in float64 (numpy/_core/function_base.py): y = arange * step (or arange / bins * delta when
// the step underflows to 0), y += first, and the last one is `last` itself.  -ffp-contract=off: two roundings, as numpy's two passes.
__device__ __forceinline__ double hist_edge(const HistRange& r, int i, int bins) {
    if (i == bins) return r.last;
    const double y = r.step == 0.0 ? ((double)i / (double)bins) * r.denom : (double)i * r.step;
    return y + r.first;
}

__global__ __launch_bounds__(HIST_T) void hist_range_kernel(const float* __restrict__ pmin, const float* __restrict__ pmax,
                                                            const long long* __restrict__ pfin, const long long* __restrict__ pbad, int groups,
                                                            int bins, HistRange* __restrict__ range, long long* __restrict__ counts,
                                                            double* __restrict__ edges, long long* __restrict__ stats) {
    __shared__ float smn[HIST_T / 64], smx[HIST_T / 64];
    __shared__ long long sfin[HIST_T / 64], sbad[HIST_T / 64];
    __shared__ HistRange sr;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    long long fin = 0, bad = 0;
    for (int g = threadIdx.x; g < groups; g += HIST_T) {
        mn = fminf(mn, pmin[g]); mx = fmaxf(mx, pmax[g]); fin += pfin[g]; bad += pbad[g];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off)); mx = fmaxf(mx, __shfl_xor(mx, off));
        fin += __shfl_xor(fin, off); bad += __shfl_xor(bad, off);
    }
    if ((threadIdx.x & 63) == 0) {
        smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; sfin[threadIdx.x >> 6] = fin; sbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < HIST_T / 64; ++w) {
            mn = fminf(mn, smn[w]); mx = fmaxf(mx, smx[w]); fin += sfin[w]; bad += sbad[w];
        }
        // _get_outer_edges: (min, max) of the data, (0, 1) without data, and an empty range widened by a half to either side
        double first = fin > 0 ? (double)mn : 0.0, last = fin > 0 ? (double)mx : 1.0;
        if (first == last) {
            first = first - 0.5;
            last = last + 0.5;
        }
        sr.first = first; sr.last = last;
        sr.denom = last - first;
        sr.step = sr.denom / (double)bins;
        *range = sr;
        stats[0] = fin; stats[1] = bad;
    }
    __syncthreads();
    const HistRange r = sr;
    for (int i = threadIdx.x; i <= bins; i += HIST_T) {
        edges[i] = hist_edge(r, i, bins);
        if (i < bins) counts[i] = 0;
    }
}

template <int TR>
__global__ __launch_bounds__(HIST_T) void hist_bin_kernel(const float* __restrict__ x, long long n, float eps, int aligned, int bins,
                                                          const HistRange* __restrict__ range, long long* __restrict__ counts) {
    __shared__ int sc[HIST_MAX_BINS];
    for (int b = threadIdx.x; b < bins; b += HIST_T) sc[b] = 0;
    __syncthreads();
    const HistRange r = *range;
    const double nb = (double)bins;
    hist_walk<TR>(x, n, eps, aligned != 0, [&](float v) {
        if (!__builtin_isfinite(v)) return;
        const double a = (double)v;
        int idx = 0;
        if (r.denom > 0.0) {                                   // (an empty range that a half does not widen, |v| >= 2^53: numpy raises; bin 0 here)
            // the uniform-bin fast path of np.histogram: truncate ((a - first) / (last - first)) * bins, fold `bins` into the last bin,
            const double f = ((a - r.first) / r.denom) * nb;
            idx = f >= nb ? bins - 1 : (f > 0.0 ? (int)f : 0);
            // then one step down if a < edges[idx], and one step up if a >= edges[idx + 1] unless idx is the (closed) last bin
            if (idx > 0 && a < hist_edge(r, idx, bins)) --idx;
            if (idx != bins - 1 && a >= hist_edge(r, idx + 1, bins)) ++idx;
        }
        atomicAdd(&sc[idx], 1);
    });
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += HIST_T) {
        const int c = sc[b];
        if (c != 0) atomicAdd(reinterpret_cast<unsigned long long*>(counts) + b, (unsigned long long)c);
    }
}

__global__ __launch_bounds__(HIST_T) void log_distance_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, float eps) {
    const long long i = (long long)blockIdx.x * HIST_T + threadIdx.x;
    if (i < n) out[i] = hist_value<1>(x[i], eps);
}

// ---- the code maps as images ---------------------------------------------------------------------------------------------------------
constexpr int CODE_MAX_T = 1024;

__global__ __launch_bounds__(CODE_MAX_T) void code_max_kernel(const long long* __restrict__ codes, long long total, long long* __restrict__ maxbuf) {
    __shared__ long long sm[CODE_MAX_T / 64];
    long long mx = codes[0];
    for (long long i = threadIdx.x; i < total; i += CODE_MAX_T) {
        const long long c = codes[i];
        mx = c > mx ? c : mx;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CODE_MAX_T / 64; ++w) mx = sm[w] > mx ? sm[w] : mx;
        maxbuf[0] = mx;
    }
}

// one thread per pixel of group 0 of the first `keep` images: its 4 x 4 block of the [keep, 1, 4h, 4w] image, four 32-bit stores
__global__ __launch_bounds__(256) void code_image_kernel(const long long* __restrict__ codes, const long long* __restrict__ maxbuf,
                                                         uint8_t* __restrict__ out, int keep, int m, int h, int w) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long hw = (long long)h * w;
    if (i >= (long long)keep * hw) return;
    const long long img = i / hw, pix = i - img * hw;
    const int y = (int)(pix / w), xq = (int)(pix - (long long)y * w);
    const long long mx = maxbuf[0];
    uint32_t u = 0;                                            // (a maximum of 0: the reference's 0 / 0 cast to uint8 is unspecified; 0 here)
    if (mx != 0) {
        // (code.float() / code.max() - 0.5) * 2, then DeTransform as detransform_kernel (csrc/vq.hip) has it
        float t = (float)codes[img * m * hw + pix] / (float)mx;
        t = t - 0.5f;
        t = t * 2.0f;
        float v = (t - (-1.0f)) / 2.0f;
        v = v * 255.999f;
        v = fminf(fmaxf(v, 0.0f), 255.0f);
        u = (uint32_t)(uint8_t)v;
    }
    const uint32_t word = u * 0x01010101u;
    uint32_t* o = reinterpret_cast<uint32_t*>(out + (img * 4 * h + 4 * y) * (4LL * w) + 4 * xq);
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) o[(long long)dy * w] = word;    // (a row of the image is 4w bytes = w words)
}

// ---- group 0 of the normalised frequencies, and CodeUsage -----------------------------------------------------------------------------
constexpr int FREQ_T = 256;

struct SnapFreqK {
    const float* freq[MCQ_VQ_MAX_LEVELS];     // level l: [m_l, k_l] frequency EMA
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t row0[MCQ_VQ_MAX_LEVELS + 1];      // first (level, group) row of level l in blockIdx order
    long long out0[MCQ_VQ_MAX_LEVELS];        // level l's first entry in `out`
    int32_t levels;
    float* out;                               // group 0 of every level, f / sum f, back to back
    int32_t* used;                            // [rows]: entries of the row with f / sum f > 1e-6
};

__global__ __launch_bounds__(FREQ_T) void snap_freq_kernel(SnapFreqK q) {
    __shared__ double smd[FREQ_T / 64];
    __shared__ int smi[FREQ_T / 64];
    int lv = 0;
    while (lv + 1 < q.levels && (int)blockIdx.x >= q.row0[lv + 1]) ++lv;
    const int g = (int)blockIdx.x - q.row0[lv];
    const int k = q.k[lv];
    const float* f = q.freq[lv] + (size_t)g * k;
    // `f / f.sum(-1, keepdim=True)` (entropyCoder.py:52): the row sum formed in double in a fixed order and rounded to float32 once
    // (torch's float32 sum is within a few ulp of it), the quotient in float32
    double s = 0.0;
    for (int i = threadIdx.x; i < k; i += FREQ_T) s += (double)f[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) smd[threadIdx.x >> 6] = s;
    __syncthreads();
    s = smd[0];
    for (int w = 1; w < FREQ_T / 64; ++w) s += smd[w];
    const float sum = (float)s;
    int used = 0;
    for (int i = threadIdx.x; i < k; i += FREQ_T) {
        const float p = f[i] / sum;
        used += p > 1e-6f ? 1 : 0;                             // strict, float32 against float32(1e-6), as `freq > 1e-6` compares (compressor.py:211-212)
        if (g == 0) q.out[q.out0[lv] + i] = p;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) used += __shfl_xor(used, off);
    if ((threadIdx.x & 63) == 0) smi[threadIdx.x >> 6] = used;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < FREQ_T / 64; ++w) used += smi[w];
        q.used[blockIdx.x] = used;
    }
}

// ONE wave: `.float().mean()` of the comparison, used / entries in float32
__global__ __launch_bounds__(64) void snap_usage_kernel(const int32_t* __restrict__ used, int rows, long long entries, float* __restrict__ usage) {
    long long u = 0;
    for (int r = threadIdx.x; r < rows; r += 64) u += used[r];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) u += __shfl_xor(u, off);
    if (threadIdx.x == 0) usage[0] = (float)u / (float)entries;
}

bool snap_rows(const int32_t* m, const int32_t* k, int32_t levels, int32_t* row0, long long* out0, long long* entries) {
    if (!m || !k || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return false;
    long long rows = 0, off = 0, all = 0;
    for (int l = 0; l < levels; ++l) {
        if (m[l] <= 0 || k[l] <= 0) return false;
        row0[l] = (int32_t)rows;
        if (out0) out0[l] = off;
        off += k[l];
        all += (long long)m[l] * k[l];
        rows += m[l];
        if (rows > 0x7fffffLL) return false;
    }
    row0[levels] = (int32_t)rows;
    if (entries) *entries = all;
    return true;
}

bool hist_args_ok(long long n, int32_t bins) { return n > 0 && n <= HIST_MAX_N && bins >= 1 && bins <= HIST_MAX_BINS; }

}  // namespace

extern "C" int32_t mcq_histogram_chunk(void) { return HIST_CHUNK; }

extern "C" size_t mcq_histogram_workspace_bytes(int64_t n, int32_t bins) {
    if (!hist_args_ok(n, bins)) return 0;
    return sizeof(HistRange) + (size_t)hist_groups(n) * (2 * sizeof(float) + 2 * sizeof(long long));
}

extern "C" int mcq_histogram_f32(const float* x, int64_t n, int32_t transform, float eps, int32_t bins, int64_t* counts, double* edges,
                                 int64_t* stats, void* workspace, void* stream) {
    if (!x || !counts || !edges || !stats || !workspace || n <= 0 || bins < 1 || bins > HIST_MAX_BINS) return MCQ_EINVAL;
    if (transform != 0 && transform != 1) return MCQ_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return MCQ_EINVAL;
    if (n > HIST_MAX_N) return MCQ_ETOOLARGE;
    const int groups = hist_groups(n);
    char* ws = static_cast<char*>(workspace);                  // [HistRange] [groups] min, [groups] max (float), [groups] finite, [groups] non-finite (int64)
    HistRange* range = reinterpret_cast<HistRange*>(ws);
    float* pmin = reinterpret_cast<float*>(ws + sizeof(HistRange));
    float* pmax = pmin + groups;
    long long* pfin = reinterpret_cast<long long*>(pmax + groups);
    long long* pbad = pfin + groups;
    long long* cnt = reinterpret_cast<long long*>(counts);
    long long* st = reinterpret_cast<long long*>(stats);
    const int aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    if (transform == 0)
        hipLaunchKernelGGL(hist_minmax_kernel<0>, dim3((unsigned)groups), dim3(HIST_T), 0, s, x, (long long)n, eps, aligned, pmin, pmax, pfin, pbad);
    else
        hipLaunchKernelGGL(hist_minmax_kernel<1>, dim3((unsigned)groups), dim3(HIST_T), 0, s, x, (long long)n, eps, aligned, pmin, pmax, pfin, pbad);
    if (mcq_check_launch() != 0) return MCQ_ELAUNCH;
    hipLaunchKernelGGL(hist_range_kernel, dim3(1), dim3(HIST_T), 0, s, pmin, pmax, pfin, pbad, groups, (int)bins, range, cnt, edges, st);
    if (mcq_check_launch() != 0) return MCQ_ELAUNCH;
    if (transform == 0)
        hipLaunchKernelGGL(hist_bin_kernel<0>, dim3((unsigned)groups), dim3(HIST_T), 0, s, x, (long long)n, eps, aligned, (int)bins, range, cnt);
    else
        hipLaunchKernelGGL(hist_bin_kernel<1>, dim3((unsigned)groups), dim3(HIST_T), 0, s, x, (long long)n, eps, aligned, (int)bins, range, cnt);
    return mcq_check_launch();
}

extern "C" int mcq_log_distance_f32(const float* x, float* out, int64_t n, float eps, void* stream) {
    if (!x || !out || n <= 0) return MCQ_EINVAL;
    if ((n + HIST_T - 1) / HIST_T > 0x7fffffffLL) return MCQ_ETOOLARGE;
    hipLaunchKernelGGL(log_distance_kernel, dim3((unsigned)((n + HIST_T - 1) / HIST_T)), dim3(HIST_T), 0, (hipStream_t)stream, x, out, (long long)n, eps);
    return mcq_check_launch();
}

extern "C" int mcq_code_image_first_u8(const int64_t* codes, uint8_t* out, int64_t* maxbuf, int32_t N, int32_t m, int32_t h, int32_t w,
                                       int32_t keep, void* stream) {
    if (!codes || !out || !maxbuf || N <= 0 || m <= 0 || h <= 0 || w <= 0 || keep <= 0 || keep > N) return MCQ_EINVAL;
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0) return MCQ_EINVAL;
    const long long total = (long long)N * m * h * w, pixels = (long long)keep * h * w;
    if ((pixels + 255) / 256 > 0x7fffffffLL) return MCQ_ETOOLARGE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(code_max_kernel, dim3(1), dim3(CODE_MAX_T), 0, s, reinterpret_cast<const long long*>(codes), total,
                       reinterpret_cast<long long*>(maxbuf));
    if (mcq_check_launch() != 0) return MCQ_ELAUNCH;
    hipLaunchKernelGGL(code_image_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const long long*>(codes),
                       reinterpret_cast<const long long*>(maxbuf), out, (int)keep, (int)m, (int)h, (int)w);
    return mcq_check_launch();
}

extern "C" int mcq_code_image_u8(const int64_t* codes, uint8_t* out, int64_t* maxbuf, int32_t N, int32_t m, int32_t h, int32_t w, void* stream) {
    return mcq_code_image_first_u8(codes, out, maxbuf, N, m, h, w, N, stream);
}

extern "C" size_t mcq_snapshot_freq_workspace_bytes(const int32_t* m, const int32_t* k, int32_t levels) {
    int32_t row0[MCQ_VQ_MAX_LEVELS + 1];
    if (!snap_rows(m, k, levels, row0, nullptr, nullptr)) return 0;
    return (size_t)row0[levels] * sizeof(int32_t);
}

extern "C" int mcq_snapshot_freq_f32(const float* const* freq_ema, const int32_t* m, const int32_t* k, int32_t levels, float* out, float* usage,
                                     void* workspace, void* stream) {
    SnapFreqK q;
    long long entries = 0;
    if (!freq_ema || !out || !usage || !workspace) return MCQ_EINVAL;
    if (!snap_rows(m, k, levels, q.row0, q.out0, &entries)) return MCQ_EINVAL;
    for (int l = 0; l < levels; ++l) {
        if (!freq_ema[l]) return MCQ_EINVAL;
        q.freq[l] = freq_ema[l]; q.k[l] = k[l];
    }
    q.levels = levels;
    q.out = out;
    q.used = static_cast<int32_t*>(workspace);
    const int rows = q.row0[levels];
    hipLaunchKernelGGL(snap_freq_kernel, dim3((unsigned)rows), dim3(FREQ_T), 0, (hipStream_t)stream, q);
    if (mcq_check_launch() != 0) return MCQ_ELAUNCH;
    hipLaunchKernelGGL(snap_usage_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, q.used, rows, entries, usage);
    return mcq_check_launch();
}
