// Per-step training telemetry kept on the device (gfx950): what the reference's trainer reports after an update
// (mcquic/train/trainer.py:423-441 `_stepFinishHook`: the loss in dB, its EMATracker((), 0.99) shadow, gradient norm, learning
// rate, the `Loss becomes NAN` guard; trainer.py:463-491 `log`: CodeUsage and the per-level code statistics) as ONE float32 row per
// step in a ring buffer the host copies back when it likes.  Two launches per update, nothing read by the host, so both sit in the
// captured post graph of parallel.GraphedTrainStep behind the frequency-EMA update:
//   meter_level_stats_kernel   one workgroup per (level, group) row of k_l entries: five partials from the level's frequency EMA
//                              [m_l, k_l] (float32) and this step's global code counts (int64)
//   meter_commit_kernel        ONE wave: folds the partials per level, reads loss / gradient norm / learning rate / skip count
//                              through device pointers, advances the shadow, the watchdog and the step counter, writes the row
// The launch boundary is the only synchronisation between them.  No atomics; every reduction runs in a fixed
// order (thread-strided partial sums, a butterfly over the wave, the waves in index order): equal inputs give equal bits.
#include "mcq_common.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int METER_T = 256;                   // (a row of 8192 entries is 32 per thread; the kernel is a few KB and latency-bound)
constexpr int METER_HEAD = 8;                  // columns in front of the per-level ones
constexpr int METER_PER_LEVEL = 4;

struct MeterStatsK {
    const float* freq[MCQ_VQ_MAX_LEVELS];     // level l: [m_l, k_l] frequency EMA
    int32_t k[MCQ_VQ_MAX_LEVELS];
    long long offset[MCQ_VQ_MAX_LEVELS];      // level l's first entry in `counts`
    int32_t row0[MCQ_VQ_MAX_LEVELS + 1];      // first (level, group) row of level l in blockIdx order
    int32_t levels;
    const long long* counts;
    long long* total;                          // the five partials, [rows] each
    int32_t* used;
    int32_t* hit;
    float* ema_entropy;
    float* step_bits;
};

// sum over the workgroup, the same value in every thread: butterfly inside each wave, then the waves in index order
template <typename T>
__device__ __forceinline__ T meter_block_sum(T v, T* sm) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = sm[0];
#pragma unroll
    for (int w = 1; w < METER_T / 64; ++w) t += sm[w];
    __syncthreads();
    return t;
}

// x log2 x with the limit 0 at x = 0 (and 0 for anything that is not positive: a zero entry contributes nothing, never a NaN).
// In double: next to x = 1 the term is as ill-conditioned as 1 / |ln x| (a row with one dominant entry, p = 1 - 2e-6, loses 3e-3
// of its entropy to the rounding of p alone in float32), and at a few KB per workgroup the kernel waits for its loads, not its VALU.
__device__ __forceinline__ double meter_xlog2x(double x) { return x > 0.0 ? x * log2(x) : 0.0; }

__global__ __launch_bounds__(METER_T) void meter_level_stats_kernel(MeterStatsK q) {
    __shared__ double smd[METER_T / 64];
    __shared__ long long sml[METER_T / 64];
    __shared__ int smi[METER_T / 64];
    int lv = 0;
    while (lv + 1 < q.levels && (int)blockIdx.x >= q.row0[lv + 1]) ++lv;
    const int g = (int)blockIdx.x - q.row0[lv];
    const int k = q.k[lv];
    const float* f = q.freq[lv] + (size_t)g * k;
    const long long* c = q.counts + q.offset[lv] + (long long)g * k;
    // pass 1: the two normalisers.  The frequency sum is kept in double: `used` compares entries against 1e-6 of it, and entries
    // within 2^-20 of that threshold must fall on the side a float64 evaluation puts them; the counts are integers, summed exactly
    // (a count above 2^24 is not a float32).
    double fsum = 0.0;
    long long tot = 0;
    for (int i = threadIdx.x; i < k; i += METER_T) {
        fsum += (double)f[i];
        tot += c[i];
    }
    fsum = meter_block_sum(fsum, smd);
    tot = meter_block_sum(tot, sml);
    // pass 2 (the row is a few KB: it comes back from the cache)
    const double ts = (double)tot;
    int used = 0, hit = 0;
    double plogp = 0.0, qlogq = 0.0;
    for (int i = threadIdx.x; i < k; i += METER_T) {
        const long long ci = c[i];
        if (fsum > 0.0) {
            const double p = (double)f[i] / fsum;
            used += p > 1e-6 ? 1 : 0;                         // strict, as Compressor.CodeUsage compares (compressor.py:211-212)
            plogp += meter_xlog2x(p);
        }
        hit += ci != 0 ? 1 : 0;
        if (ci > 0) qlogq += meter_xlog2x((double)ci / ts);   // (ci > 0 implies tot > 0: counts are not negative)
    }
    used = meter_block_sum(used, smi);
    hit = meter_block_sum(hit, smi);
    plogp = meter_block_sum(plogp, smd);
    qlogq = meter_block_sum(qlogq, smd);
    if (threadIdx.x == 0) {
        const int row = (int)blockIdx.x;
        q.total[row] = tot;
        q.used[row] = used;
        q.hit[row] = hit;
        q.ema_entropy[row] = (float)(0.0 - plogp);            // (0 - x: an empty sum is +0, not -0)
        q.step_bits[row] = tot > 0 ? (float)(ts * (0.0 - qlogq)) : 0.0f;
    }
}

struct MeterCommitK {
    int32_t m[MCQ_VQ_MAX_LEVELS];
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t row0[MCQ_VQ_MAX_LEVELS + 1];
    int32_t levels;
    const long long* total;
    const int32_t* used;
    const int32_t* hit;
    const float* ema_entropy;
    const float* step_bits;
    const float* loss;
    const float* grad_norm;                    // or null
    const float* lr_dev;                       // or null: `lr` by value
    const long long* skipped;                  // or null
    float lr;
    float upper_sq, decay, floor;              // float(upper_bound ** 2), float(1 - momentum), the watchdog's floor (NaN: off)
    double pixels;
    long long* state;                          // [0] count, [1] first_bad_step, [2] low word: the float32 shadow
    long long* steps;                          // [capacity]
    float* ring;                               // [capacity][METER_HEAD + METER_PER_LEVEL * levels]
    long long capacity;
};

template <typename T>
__device__ __forceinline__ T meter_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(64) void meter_commit_kernel(MeterCommitK q) {
    const int lane = threadIdx.x;
    const long long count = q.state[0];
    const int ncols = METER_HEAD + METER_PER_LEVEL * q.levels;
    const long long slot = count % q.capacity;
    float* row = q.ring + slot * ncols;
    long long used_all = 0, entries_all = 0;
    double bits_all = 0.0;
    for (int l = 0; l < q.levels; ++l) {
        const int m = q.m[l], r0 = q.row0[l];
        long long used = 0, hit = 0, tot = 0;
        double ent = 0.0, bits = 0.0;
        for (int g = lane; g < m; g += 64) {
            used += q.used[r0 + g];
            hit += q.hit[r0 + g];
            tot += q.total[r0 + g];
            ent += (double)q.ema_entropy[r0 + g];
            bits += (double)q.step_bits[r0 + g];
        }
        used = meter_wave_sum(used); hit = meter_wave_sum(hit); tot = meter_wave_sum(tot);
        ent = meter_wave_sum(ent); bits = meter_wave_sum(bits);
        const double entries = (double)m * (double)q.k[l];
        used_all += used; entries_all += (long long)m * q.k[l]; bits_all += bits;
        if (lane == 0) {
            float* o = row + METER_HEAD + METER_PER_LEVEL * l;
            o[0] = (float)((double)used / entries);
            o[1] = (float)(ent / (double)m);
            o[2] = (float)((double)hit / entries);
            o[3] = tot > 0 ? (float)(bits / (double)tot) : 0.0f;
        }
    }
    if (lane != 0) return;
    const float nan = __builtin_nanf("");
    const float loss = q.loss[0];
    const float gn = q.grad_norm ? q.grad_norm[0] : nan;
    const float lr = q.lr_dev ? q.lr_dev[0] : q.lr;
    // Decibel (validate/utils.py:6-12) then EMATracker.forward (validate/utils.py:22-28), float32 op by op (-ffp-contract=off)
    const float db = -10.0f * log10f(loss / q.upper_sq);
    float* shadowp = reinterpret_cast<float*>(q.state + 2);
    float shadow = *shadowp;
    if (shadow != shadow) {
        shadow = db;
    } else {
        const float d = shadow - db;
        const float t = q.decay * d;
        shadow = shadow - t;
    }
    *shadowp = shadow;
    // trainer.py:435-437: `torch.isnan(moment) or moment < 0.1`; here also a loss or a gradient norm that is inf or NaN.  Sticky.
    const bool bad = !__builtin_isfinite(loss) || (q.grad_norm && !__builtin_isfinite(gn)) || shadow != shadow || shadow < q.floor;
    if (bad && q.state[1] < 0) q.state[1] = count;
    row[0] = loss;
    row[1] = db;
    row[2] = shadow;
    row[3] = gn;
    row[4] = lr;
    row[5] = q.skipped ? (float)q.skipped[0] : 0.0f;
    row[6] = (float)((double)used_all / (double)entries_all);
    row[7] = (float)(bits_all / q.pixels);
    q.steps[slot] = count;
    q.state[0] = count + 1;
}

// the (level, group) rows in launch order; false for a table either kernel cannot hold
bool meter_rows(const int32_t* m, const int32_t* k, int32_t levels, int32_t* row0, long long* offset) {
    if (!m || !k || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return false;
    long long off = 0, rows = 0;
    for (int l = 0; l < levels; ++l) {
        if (m[l] <= 0 || k[l] <= 0) return false;
        row0[l] = (int32_t)rows;
        if (offset) offset[l] = off;
        off += (long long)m[l] * k[l];
        rows += m[l];
        if (rows > 0x7fffffLL) return false;
    }
    row0[levels] = (int32_t)rows;
    return true;
}

}  // namespace

extern "C" size_t mcq_step_meter_workspace_bytes(const int32_t* m, const int32_t* k, int32_t levels) {
    int32_t row0[MCQ_VQ_MAX_LEVELS + 1];
    if (!meter_rows(m, k, levels, row0, nullptr)) return 0;
    return (size_t)row0[levels] * (sizeof(long long) + 2 * sizeof(int32_t) + 2 * sizeof(float));
}

extern "C" int32_t mcq_step_meter_columns(int32_t levels) {
    return levels > 0 && levels <= MCQ_VQ_MAX_LEVELS ? METER_HEAD + METER_PER_LEVEL * levels : 0;
}

extern "C" int mcq_step_meter_update_f32(const float* const* freq_ema, const int32_t* m, const int32_t* k, int32_t levels, const int64_t* counts,
                                         void* workspace, const float* loss, const float* grad_norm, const float* lr_dev, double lr,
                                         const int64_t* skipped, double upper_bound, double momentum, double floor, double pixels,
                                         int64_t* state, int64_t* steps, float* ring, int64_t capacity, void* stream) {
    MeterStatsK s;
    MeterCommitK c;
    if (!freq_ema || !counts || !workspace || !loss || !state || !steps || !ring || capacity <= 0) return MCQ_EINVAL;
    if (!(upper_bound > 0.0) || !(pixels > 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return MCQ_EINVAL;
    if (!meter_rows(m, k, levels, s.row0, s.offset)) return MCQ_EINVAL;
    const int rows = s.row0[levels];
    for (int l = 0; l < levels; ++l) {
        if (!freq_ema[l]) return MCQ_EINVAL;
        s.freq[l] = freq_ema[l]; s.k[l] = k[l];
        c.m[l] = m[l]; c.k[l] = k[l]; c.row0[l] = s.row0[l];
    }
    c.row0[levels] = rows;
    s.levels = c.levels = levels;
    s.counts = reinterpret_cast<const long long*>(counts);
    char* ws = static_cast<char*>(workspace);                  // [rows] int64, then four [rows] 32-bit arrays
    s.total = reinterpret_cast<long long*>(ws);
    s.used = reinterpret_cast<int32_t*>(ws + (size_t)rows * 8);
    s.hit = s.used + rows;
    s.ema_entropy = reinterpret_cast<float*>(s.hit + rows);
    s.step_bits = s.ema_entropy + rows;
    c.total = s.total; c.used = s.used; c.hit = s.hit; c.ema_entropy = s.ema_entropy; c.step_bits = s.step_bits;
    c.loss = loss; c.grad_norm = grad_norm; c.lr_dev = lr_dev; c.lr = (float)lr;
    c.skipped = reinterpret_cast<const long long*>(skipped);
    // Decibel squares its bound in Python (a double) and divides a float32 tensor by it; EMATracker keeps 1 - momentum as a double
    // and multiplies a float32 tensor by it: both reach torch's kernels cast to float32
    c.upper_sq = (float)(upper_bound * upper_bound);
    c.decay = (float)(1.0 - momentum);
    c.floor = (float)floor;
    c.pixels = pixels;
    c.state = reinterpret_cast<long long*>(state);
    c.steps = reinterpret_cast<long long*>(steps);
    c.ring = ring;
    c.capacity = capacity;
    hipLaunchKernelGGL(meter_level_stats_kernel, dim3((unsigned)rows), dim3(METER_T), 0, (hipStream_t)stream, s);
    if (mcq_check_launch() != 0) return MCQ_ELAUNCH;
    hipLaunchKernelGGL(meter_commit_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, c);
    return mcq_check_launch();
}
