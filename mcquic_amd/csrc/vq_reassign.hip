// Codebook reassignment inside the training step, for gfx950: dead codewords refilled from the most used ones in TWO launches for
// all levels and groups (the reference's one training hook, mcquic/train/hooks.py:100-121 -> Compound.refresh ->
// _multiCodebookQuantization.reAssignCodebook, mcquic/modules/quantizer.py:111-136; the rule is the one of this project's eager
// `reAssignCodebook`, mcquic_amd/modules/quantizer.py, which stays as it is).
//
//   vq_reassign_plan_kernel    one workgroup per (level, group): from the level's RAW `_freqEMA` row [k] and a priority row [k] (the
//                              caller's, or drawn with the generator of mcq_rng.h, stream MCQ_RNG_STREAM_REASSIGN) the donor index per
//                              codeword `source` [m, k] (its own index where nothing moves) and the mask `refill` [m, k]
//   vq_reassign_apply_kernel   ONE workgroup: the moves, `changed` [m, k], and the scalars (moved, proportion, fired, generator offset)
//
// The rule, per group (f = raw frequencies, p = priorities, half = k / 2):
//   s      = the row sum: per-lane double partials over i = lane, lane + 1024, ..., then a fixed tree; rounded ONCE to float32.  ATen's
//            float32 sum (`NormalizedFreq`) can differ from it in the last place of s; the eager method keeps its own arithmetic.
//   fn     = f / s (float32, IEEE division);  dead = fn < 1e-6f
//   place  = stable ascending rank of (dead ? p : +inf): the dead codewords lined up by priority, the live ones behind them
//   refill = dead & (place < half);  crowded = #dead > half
//   score  = crowded & dead ? (refill ? 0 : -1) : fn
//   donors = stable DESCENDING order of score; the i-th refilled codeword in index order takes donors[i]
// Both ranks are counted, not sorted: rank(i) = #{j : key_j before key_i, or equal and j < i} over the row held in LDS -- k^2 compares
// per group per ordering (k = 8192: 67 M, ~65 k per lane), only on a step that fires.  Stable, ties by index, no atomics, the same bits
// on every run.  A rank is a permutation, so every `source` entry is written exactly once: entry i by its own lane when i is not
// refilled, else by the lane that holds the donor whose rank is i's slot.  NaN frequencies or priorities are not ordered by either side.
//
// Decision words.  `state` (int64 [MCQ_REASSIGN_STATE_WORDS], include/mcquic_hip.h) holds `count` (completed updates) and `seen` (the
// count the last apply launch committed).  Within a launch nothing that a workgroup reads is written: the plan launch reads `seen` and
// (its workgroup 0) writes count = seen + 1; the apply launch reads `count` and writes `seen` and everything else.  The step fires when
// the completed count s AFTER this update satisfies s >= start and (s + 1) % every == 0 -- the reference increments `_step` and then
// tests (step + 1) % freq (trainer.py:211-213, hooks.py:107); that off-by-one is kept.  On any other step both launches read the
// decision and return; no codebook byte is written.  With the guard's flag set (step_guard.hip) nothing moves and the count stays.
#include "mcq_common.h"
#include "mcq_rng.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int RE_T = 1024;                          // lanes per workgroup
constexpr int RE_KMAX = MCQ_REASSIGN_MAX_K;         // the longest row whose key set fits the LDS arrays below
constexpr int RE_E = RE_KMAX / RE_T;                // row entries per lane
enum { ST_COUNT = 0, ST_SEEN = 1, ST_FIRED = 2, ST_MOVED = 3, ST_PROPORTION = 4, ST_SEED = 5, ST_OFFSET = 6 };
static_assert(MCQ_REASSIGN_STATE_WORDS == 7, "count, seen, fired, moved, proportion, seed, offset");
static_assert(RE_KMAX % RE_T == 0 && RE_KMAX / 2 <= 65535, "whole entries per lane; donor slots held as uint16");

__device__ __forceinline__ bool reassign_fires(long long s, long long every, long long start) { return s >= start && (s + 1) % every == 0; }

struct ReassignPlanK {
    const float* freq[MCQ_VQ_MAX_LEVELS];     // level l: raw `_freqEMA` [m_l, k_l]
    const float* prio[MCQ_VQ_MAX_LEVELS];     // level l: priorities [m_l, k_l], or null: drawn
    int32_t* source[MCQ_VQ_MAX_LEVELS];       // level l: [m_l, k_l]
    unsigned char* refill[MCQ_VQ_MAX_LEVELS]; // level l: [m_l, k_l]
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t row0[MCQ_VQ_MAX_LEVELS + 1];      // first (level, group) row of level l in blockIdx order
    int32_t levels;
    int32_t level0;                           // number of this table's first level among all levels of the step (its generator offset)
    int32_t advance;                          // this launch writes the count (the first table of a step)
    long long every, start;
    long long* state;
    const int* skip;                          // or null
};

// inclusive scan of one int per lane over the workgroup, lane order; `sm` holds RE_T / 64 ints; *total = the sum
__device__ __forceinline__ int block_scan_int(int v, int* sm, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off);
        if (lane >= off) v += u;
    }
    if (lane == 63) sm[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RE_T / 64; ++w) {
        const int t = sm[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(RE_T) void vq_reassign_plan_kernel(ReassignPlanK q) {
    __shared__ float key[RE_KMAX];                  // the row's sort key: first the lined-up priorities, then the scores
    __shared__ unsigned short slot_index[RE_KMAX / 2];   // the t-th refilled codeword in index order
    __shared__ unsigned char mark[RE_KMAX];         // refill
    __shared__ double smd[RE_T / 64];
    __shared__ int smi[RE_T / 64];
    if (q.skip && q.skip[0]) return;
    const long long s = q.state[ST_SEEN] + 1;       // (`seen` is not written by this launch: every workgroup decides alike)
    if (q.advance && blockIdx.x == 0 && threadIdx.x == 0) q.state[ST_COUNT] = s;
    if (!reassign_fires(s, q.every, q.start)) return;

    int lv = 0;
    while (lv + 1 < q.levels && (int)blockIdx.x >= q.row0[lv + 1]) ++lv;
    const int g = (int)blockIdx.x - q.row0[lv];
    const int k = q.k[lv], half = k / 2;
    const size_t row = (size_t)g * k;
    const float* f = q.freq[lv] + row;
    const float* p = q.prio[lv] ? q.prio[lv] + row : nullptr;
    RngState r = {0u, 0u, 0u, 0u};
    if (!p) {                                       // level l of the step draws under {seed, offset + l}
        const unsigned long long seed = (unsigned long long)q.state[ST_SEED];
        const unsigned long long off = (unsigned long long)q.state[ST_OFFSET] + (unsigned long long)(q.level0 + lv);
        r.s0 = (uint32_t)seed; r.s1 = (uint32_t)(seed >> 32); r.o0 = (uint32_t)off; r.o1 = (uint32_t)(off >> 32);
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // the row sum: double, lane-strided partials in index order, a fixed tree, one rounding
    float fv[RE_E];
    double part = 0.0;
#pragma unroll
    for (int e = 0; e < RE_E; ++e) {
        const int i = tid + e * RE_T;
        fv[e] = i < k ? f[i] : 0.0f;
        part += (double)fv[e];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) smd[wave] = part;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < RE_T / 64; ++w) total += smd[w];
    const float sum = (float)total;

    float fn[RE_E], mine[RE_E];
    bool dead[RE_E];
    int ndead = 0;
#pragma unroll
    for (int e = 0; e < RE_E; ++e) {
        const int i = tid + e * RE_T;
        fn[e] = fv[e] / sum;
        dead[e] = i < k && fn[e] < 1e-6f;
        ndead += dead[e] ? 1 : 0;
        const float pr = i < k ? (p ? p[i] : rng_uniform(r, MCQ_RNG_STREAM_REASSIGN, row + (size_t)i)) : 0.0f;
        mine[e] = dead[e] ? pr : __builtin_inff();
        if (i < k) key[i] = mine[e];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ndead += __shfl_xor(ndead, off);
    if (lane == 0) smi[wave] = ndead;
    __syncthreads();                                // (also: `key` is whole)
    ndead = 0;
#pragma unroll
    for (int w = 0; w < RE_T / 64; ++w) ndead += smi[w];
    const bool crowded = ndead > half;

    // place: ascending, stable
    int rank[RE_E];
#pragma unroll
    for (int e = 0; e < RE_E; ++e) rank[e] = 0;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
        const float kj = key[j];
#pragma unroll
        for (int e = 0; e < RE_E; ++e) rank[e] += (kj < mine[e] || (kj == mine[e] && j < tid + e * RE_T)) ? 1 : 0;
    }
    bool refill[RE_E];
#pragma unroll
    for (int e = 0; e < RE_E; ++e) {
        refill[e] = dead[e] && rank[e] < half;
        mine[e] = crowded && dead[e] ? (refill[e] ? 0.0f : -1.0f) : fn[e];
    }
    __syncthreads();                                // every lane has read the priorities: `key` takes the scores
#pragma unroll
    for (int e = 0; e < RE_E; ++e) {
        const int i = tid + e * RE_T;
        if (i < k) {
            key[i] = mine[e];
            mark[i] = refill[e] ? 1 : 0;
            q.refill[lv][row + i] = refill[e] ? 1 : 0;
        }
    }
    __syncthreads();

    // slot_index: the refilled codewords in index order (lane t scans entries [t c, t c + c))
    const int c = (k + RE_T - 1) / RE_T;
    const int first = tid * c, last = first + c < k ? first + c : k;
    int cnt = 0;
    for (int i = first; i < last; ++i) cnt += mark[i];
    int nrefill;
    int at = block_scan_int(cnt, smi, &nrefill) - cnt;
    for (int i = first; i < last; ++i)
        if (mark[i]) slot_index[at++] = (unsigned short)i;     // (at < nrefill <= half <= RE_KMAX / 2)
    __syncthreads();

    // donors: descending, stable; donor number t goes to the t-th refilled codeword
#pragma unroll
    for (int e = 0; e < RE_E; ++e) rank[e] = 0;
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
        const float kj = key[j];
#pragma unroll
        for (int e = 0; e < RE_E; ++e) rank[e] += (kj > mine[e] || (kj == mine[e] && j < tid + e * RE_T)) ? 1 : 0;
    }
    int32_t* src = q.source[lv] + row;
#pragma unroll
    for (int e = 0; e < RE_E; ++e) {
        const int i = tid + e * RE_T;
        if (i >= k) continue;
        if (!refill[e]) src[i] = i;
        if (rank[e] < nrefill) src[slot_index[rank[e]]] = i;
    }
}

struct ReassignApplyK {
    float* codebook[MCQ_VQ_MAX_LEVELS];             // level l: [m_l, k_l, d_l], moved in place
    const int32_t* source[MCQ_VQ_MAX_LEVELS];
    const unsigned char* refill[MCQ_VQ_MAX_LEVELS];
    unsigned char* changed[MCQ_VQ_MAX_LEVELS];      // level l: [m_l, k_l]
    int32_t m[MCQ_VQ_MAX_LEVELS];
    int32_t k[MCQ_VQ_MAX_LEVELS];
    int32_t d[MCQ_VQ_MAX_LEVELS];
    int32_t levels;
    int32_t first, last;                            // the first / last table of a step: `moved` starts at 0 / the step is committed
    int32_t step_levels;                            // levels of the whole step: what the generator's offset advances by
    long long step_codewords;                       // sum of m_l k_l over the whole step: proportion's denominator
    long long every, start;
    float* scratch;                                 // max over this table's levels of k_l d_l floats
    long long* state;
    const int* skip;
};

// ONE workgroup walks the (level, group) rows in order.  A donor can itself be a refilled codeword (a group with fewer live codewords
// than refills, e.g. an all-dead group), so a move must read the codebook as it was: per group the donor rows are first gathered into
// `scratch` (and compared with the rows they replace), a barrier, then copied over the refilled rows.  Donors are of the same group
// and one workgroup owns it, so the barrier is all the ordering there is to keep.  The scalars are this workgroup's own sums: a fixed
// order, no atomics.
__global__ __launch_bounds__(RE_T) void vq_reassign_apply_kernel(ReassignApplyK q) {
    __shared__ int smi[RE_T / 64];
    if (q.skip && q.skip[0]) return;
    const long long s = q.state[ST_COUNT];
    if (s == q.state[ST_SEEN]) return;              // (no plan launch went before: nothing to commit)
    const bool fires = reassign_fires(s, q.every, q.start);
    const int tid = threadIdx.x;
    int moved = 0;
    if (fires) {
        for (int lv = 0; lv < q.levels; ++lv) {
            const int k = q.k[lv], d = q.d[lv];
            const int n = k * d;                    // (< 2^31: checked on the host)
            for (int g = 0; g < q.m[lv]; ++g) {
                float* cb = q.codebook[lv] + (size_t)g * n;
                const int32_t* src = q.source[lv] + (size_t)g * k;
                const unsigned char* rf = q.refill[lv] + (size_t)g * k;
                unsigned char* ch = q.changed[lv] + (size_t)g * k;
                for (int idx = tid; idx < n; idx += RE_T) {
                    const int i = idx / d;
                    if (!rf[i]) continue;
                    const unsigned from = (unsigned)src[i];
                    q.scratch[idx] = cb[(size_t)(from < (unsigned)k ? from : (unsigned)i) * d + (idx - i * d)];
                }
                for (int i = tid; i < k; i += RE_T) {
                    bool far = false;
                    if (rf[i]) {
                        const unsigned from = (unsigned)src[i];
                        const float* a = cb + (size_t)(from < (unsigned)k ? from : (unsigned)i) * d;
                        const float* b = cb + (size_t)i * d;
                        float dist = 0.0f;
                        for (int j = 0; j < d; ++j) {       // ((fresh - old) ** 2).sum(-1), in index order
                            const float t = a[j] - b[j];
                            dist += t * t;
                        }
                        far = dist > 1e-4f;
                    }
                    ch[i] = far ? 1 : 0;
                    moved += far ? 1 : 0;
                }
                __syncthreads();                    // every read of the group's old rows is done, the scratch rows are visible
                for (int idx = tid; idx < n; idx += RE_T)
                    if (rf[idx / d]) cb[idx] = q.scratch[idx];
                __syncthreads();                    // (the next group reuses the scratch)
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) moved += __shfl_xor(moved, off);
        if ((tid & 63) == 0) smi[tid >> 6] = moved;
        __syncthreads();
    }
    if (tid) return;
    if (fires) {
        long long total = q.first ? 0ll : q.state[ST_MOVED];
        for (int w = 0; w < RE_T / 64; ++w) total += smi[w];
        q.state[ST_MOVED] = total;
        if (q.last) {
            // the reference's return value: torch.cat(reassigned).float().mean()
            const float share = (float)total / (float)q.step_codewords;
            q.state[ST_PROPORTION] = (long long)__builtin_bit_cast(uint32_t, share);
            q.state[ST_FIRED] += 1;
            q.state[ST_OFFSET] += (long long)q.step_levels;
        }
    }
    if (q.last) q.state[ST_SEEN] = s;
}

bool reassign_decision_ok(const int64_t* state, int64_t every, int64_t start) { return state && every >= 1 && start >= 0; }

}  // namespace

extern "C" int32_t mcq_vq_reassign_max_k(void) { return RE_KMAX; }

extern "C" int mcq_vq_reassign_plan(const float* const* freq_ema, const float* const* priority, const int32_t* m, const int32_t* k, int32_t levels,
                                    int32_t level0, int32_t advance, int32_t* const* source, uint8_t* const* refill, int64_t* state,
                                    int64_t every, int64_t start, const int32_t* skip, void* stream) {
    if (!freq_ema || !m || !k || !source || !refill || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS || level0 < 0) return MCQ_EINVAL;
    if (!reassign_decision_ok(state, every, start)) return MCQ_EINVAL;
    ReassignPlanK q;
    int rows = 0;
    for (int l = 0; l < levels; ++l) {
        if (!freq_ema[l] || !source[l] || !refill[l] || m[l] <= 0 || k[l] <= 0) return MCQ_EINVAL;
        if (k[l] > RE_KMAX) return MCQ_EINVAL;      // the row's key set does not fit the LDS arrays
        q.freq[l] = freq_ema[l]; q.prio[l] = priority ? priority[l] : nullptr; q.source[l] = source[l]; q.refill[l] = refill[l];
        q.k[l] = k[l]; q.row0[l] = rows;
        rows += m[l];
    }
    q.row0[levels] = rows;
    q.levels = levels; q.level0 = level0; q.advance = advance ? 1 : 0; q.every = every; q.start = start;
    q.state = reinterpret_cast<long long*>(state); q.skip = (const int*)skip;
    hipLaunchKernelGGL(vq_reassign_plan_kernel, dim3((unsigned)rows), dim3(RE_T), 0, (hipStream_t)stream, q);
    return mcq_check_launch();
}

extern "C" int mcq_vq_reassign_apply(float* const* codebook, const int32_t* const* source, const uint8_t* const* refill, uint8_t* const* changed,
                                     const int32_t* m, const int32_t* k, const int32_t* d, int32_t levels, int32_t first, int32_t last,
                                     int32_t step_levels, int64_t step_codewords, float* scratch, int64_t* state, int64_t every, int64_t start,
                                     const int32_t* skip, void* stream) {
    if (!codebook || !source || !refill || !changed || !m || !k || !d || !scratch || levels <= 0 || levels > MCQ_VQ_MAX_LEVELS) return MCQ_EINVAL;
    if (!reassign_decision_ok(state, every, start) || step_levels < levels || step_codewords <= 0) return MCQ_EINVAL;
    ReassignApplyK q;
    for (int l = 0; l < levels; ++l) {
        if (!codebook[l] || !source[l] || !refill[l] || !changed[l] || m[l] <= 0 || k[l] <= 0 || d[l] <= 0) return MCQ_EINVAL;
        if (k[l] > RE_KMAX) return MCQ_EINVAL;
        if ((long long)k[l] * d[l] > 0x7fffffffLL) return MCQ_ETOOLARGE;
        q.codebook[l] = codebook[l]; q.source[l] = source[l]; q.refill[l] = refill[l]; q.changed[l] = changed[l];
        q.m[l] = m[l]; q.k[l] = k[l]; q.d[l] = d[l];
    }
    q.levels = levels; q.first = first ? 1 : 0; q.last = last ? 1 : 0; q.step_levels = step_levels; q.step_codewords = step_codewords;
    q.every = every; q.start = start; q.scratch = scratch; q.state = reinterpret_cast<long long*>(state); q.skip = (const int*)skip;
    hipLaunchKernelGGL(vq_reassign_apply_kernel, dim3(1), dim3(RE_T), 0, (hipStream_t)stream, q);
    return mcq_check_launch();
}
