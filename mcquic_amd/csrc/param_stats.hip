// Per-parameter gradient / weight / update norms of MANY tensors, kept on the device (gfx950; host mirror mcquic_amd.monitor.ParamStats):
// which tensor went non-finite, how large a layer's update is against its weights -- one float32 row of five columns per tensor and
// recorded step, in a ring the host copies back when it likes.  Nothing is read by the host, so the launches sit in the captured
// post graph of parallel.GraphedTrainStep around the optimizer's update.
//
// The tensor lists are the device tables of tensor_list.h (pointer rows: param, grad, shadow) plus tensor_first_blk[ntensors + 1].
// `state` is {count, first_bad_step, first_bad_tensor, rows}: count advances on every step, rows on every RECORDED one.  A step is
// sampled when count % every == 0 and recorded when it is sampled or the step's guard flag (step_guard.hip) is set.  Three launches:
//   (a) param_stats_before_kernel   sampled steps: each chunk's weights into the shadow                       8 B / element
//   (b) param_stats_after_kernel    recorded steps: per chunk (sum w^2, sum g^2 and max |g| over the finite g, the number of
//                                   non-finite g, sum (w - shadow)^2) into the chunk's own slot               12 B / element
//                                   Workgroup 0 also latches {count, recorded, ring slot} into the workspace's head: the
//                                   workgroups of (c) read the decision there, never a word that workgroup 0 of their own launch
//                                   is writing.
//   (c) param_stats_finish_kernel   one 64-lane workgroup per tensor: its chunks' partials in chunk order, the square roots, one
//                                   rounding to float32, the row.  Workgroup 0 owns `state`: the blame words (the lowest tensor
//                                   with a non-finite gradient, by a fixed-order minimum over the chunks), steps[], rows, count.
// On a step that is not recorded every workgroup reads the words of the decision and returns (a uniform branch); workgroup 0 of (b)
// still latches the head and workgroup 0 of (c) still advances count.  The launch boundary is the only synchronisation.  Products and
// differences are formed in double, every sum is a fixed tree, no atomics: equal inputs at equal addresses give equal bits.  The
// kernels are bound by HBM; all they do about speed is 16 bytes per lane where every row of a tensor is 16-byte aligned (a chunk
// starts a multiple of 4096 elements into its tensor); a gradient that is a view of a flat buffer may start at any 4-byte address and
// takes the dword loop, as do a tensor's last 1..3 elements.
#include "mcq_common.h"
#include "tensor_list.h"
#include "../../include/mcquic_hip.h"

namespace {

constexpr int STATS_COLUMNS = 5;                             // weight_norm, grad_norm, grad_absmax, grad_nonfinite, update_norm
constexpr int STATS_PART = 5;                                // doubles per chunk: sum w^2, sum g^2, max |g|, non-finite, sum d^2
constexpr int STATS_HEAD = 4;                                // int64 words in front of the partials: count, recorded, slot, reserved

__global__ __launch_bounds__(256) void param_stats_before_kernel(McqTensorList list, const long long* __restrict__ state, long long every) {
    if (state[0] % every != 0) return;
    const McqChunk c = list.chunk();
    const long long first = c.first, end = c.end;
    const float* __restrict__ w = list.row(0, c.t);
    float* __restrict__ s = list.row(2, c.t);
    long long done = first;
    if ((((uintptr_t)w | (uintptr_t)s) & 15) == 0) {
        const long long nvec = (end - first) >> 2;           // <= 1024 float4: at most four per lane
        const float4* __restrict__ w4 = (const float4*)(w + first);
        float4* __restrict__ s4 = (float4*)(s + first);
#pragma unroll 4
        for (long long i = threadIdx.x; i < nvec; i += 256) s4[i] = w4[i];
        done = first + (nvec << 2);
    }
    for (long long i = done + threadIdx.x; i < end; i += 256) s[i] = w[i];
}

struct StatsAcc {
    double w2 = 0.0, g2 = 0.0, d2 = 0.0;
    float gmax = 0.0f;
    int bad = 0;
    __device__ __forceinline__ void take(float w, float g, float s, bool diff) {
        w2 += (double)w * (double)w;
        if (__builtin_isfinite(g)) {
            g2 += (double)g * (double)g;
            gmax = fmaxf(gmax, fabsf(g));
        } else {
            ++bad;
        }
        if (diff) {
            const double d = (double)w - (double)s;
            d2 += d * d;
        }
    }
};

// max over the workgroup's 256 lanes in mcq_block_sum256's tree; the result is valid in lane 0
__device__ __forceinline__ float stats_block_max256(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void param_stats_after_kernel(McqTensorList list, const long long* __restrict__ state, long long every,
                                                                long long capacity, int updates, const int* __restrict__ skip,
                                                                long long* __restrict__ head, double* __restrict__ part) {
    __shared__ double red[4][256];
    __shared__ float redm[256];
    const long long count = state[0];
    const bool sampled = count % every == 0;
    const bool recorded = sampled || (skip && skip[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        head[0] = count;
        head[1] = recorded ? 1 : 0;
        head[2] = state[3] % capacity;
    }
    if (!recorded) return;
    const McqChunk c = list.chunk();
    const long long first = c.first, end = c.end;
    const float* __restrict__ w = list.row(0, c.t);
    const float* __restrict__ g = list.row(1, c.t);          // null: a parameter without a gradient counts as a gradient of zeros
    const float* __restrict__ s = list.row(2, c.t);
    // a row made only because the step was skipped does not read the shadow (stale: no `before` copied it): a skipped update moves no weight
    const bool diff = updates && sampled;
    StatsAcc a;
    long long done = first;
    if ((((uintptr_t)w | (uintptr_t)g | (diff ? (uintptr_t)s : 0)) & 15) == 0) {
        const long long nvec = (end - first) >> 2;
        const float4* __restrict__ w4 = (const float4*)(w + first);
        const float4* __restrict__ g4 = g ? (const float4*)(g + first) : nullptr;
        const float4* __restrict__ s4 = diff ? (const float4*)(s + first) : nullptr;
        const float4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (long long i = threadIdx.x; i < nvec; i += 256) {
            const float4 wv = w4[i];
            const float4 gv = g4 ? g4[i] : zero;
            const float4 sv = s4 ? s4[i] : zero;
            a.take(wv.x, gv.x, sv.x, diff);
            a.take(wv.y, gv.y, sv.y, diff);
            a.take(wv.z, gv.z, sv.z, diff);
            a.take(wv.w, gv.w, sv.w, diff);
        }
        done = first + (nvec << 2);
    }
    for (long long i = done + threadIdx.x; i < end; i += 256) a.take(w[i], g ? g[i] : 0.0f, diff ? s[i] : 0.0f, diff);
    // (one array per sum: no lane-0 read of red[0] has to be waited for before the next sum overwrites it)
    const double w2 = mcq_block_sum256(a.w2, red[0]);
    const double g2 = mcq_block_sum256(a.g2, red[1]);
    const double bad = mcq_block_sum256((double)a.bad, red[2]);  // (<= 4096: exact)
    const double d2 = mcq_block_sum256(a.d2, red[3]);
    const float gmax = stats_block_max256(a.gmax, redm);
    if (threadIdx.x == 0) {
        double* o = part + (size_t)blockIdx.x * STATS_PART;
        o[0] = w2;
        o[1] = g2;
        o[2] = (double)gmax;
        o[3] = bad;
        o[4] = d2;
    }
}

// lane l takes chunks l, l + 64, ... in order, then a fixed tree over the lanes (lamb_ratio_kernel's fold)
__global__ __launch_bounds__(64) void param_stats_finish_kernel(const double* __restrict__ part, const long long* __restrict__ head,
                                                                const int* __restrict__ tensor_first_blk, const int* __restrict__ blk_tensor,
                                                                int nblocks, int ntensors, int updates, long long* __restrict__ state,
                                                                long long* __restrict__ steps, float* __restrict__ ring) {
    __shared__ double rs[4][64];
    __shared__ double rm[64];
    __shared__ int rt[64];
    const int lane = threadIdx.x;
    const long long count = head[0];
    if (!head[1]) {
        if (blockIdx.x == 0 && lane == 0) state[0] = count + 1;
        return;
    }
    const long long slot = head[2];
    const int t = blockIdx.x;
    const int b0 = tensor_first_blk[t], b1 = tensor_first_blk[t + 1];
    double w2 = 0.0, g2 = 0.0, bad = 0.0, d2 = 0.0, gmax = 0.0;
    for (int b = b0 + lane; b < b1; b += 64) {
        const double* p = part + (size_t)b * STATS_PART;
        w2 += p[0];
        g2 += p[1];
        gmax = p[2] > gmax ? p[2] : gmax;
        bad += p[3];
        d2 += p[4];
    }
    rs[0][lane] = w2; rs[1][lane] = g2; rs[2][lane] = bad; rs[3][lane] = d2; rm[lane] = gmax;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (lane < off) {
#pragma unroll
            for (int k = 0; k < 4; ++k) rs[k][lane] += rs[k][lane + off];
            rm[lane] = rm[lane + off] > rm[lane] ? rm[lane + off] : rm[lane];
        }
        __syncthreads();
    }
    if (lane == 0) {
        float* row = ring + ((size_t)slot * ntensors + t) * STATS_COLUMNS;
        row[0] = (float)sqrt(rs[0][0]);
        row[1] = (float)sqrt(rs[1][0]);
        row[2] = (float)rm[0];
        row[3] = (float)rs[2][0];
        row[4] = updates ? (float)sqrt(rs[3][0]) : __builtin_nanf("");
    }
    if (blockIdx.x != 0) return;
    // workgroup 0 owns `state`: the lowest tensor with a non-finite gradient, over ALL chunks (lane l: chunks l, l + 64, ...; the chunk
    // table is in tensor order, so a lane's first hit is its lowest)
    int low = ntensors;
    for (int b = lane; b < nblocks; b += 64) {
        if (part[(size_t)b * STATS_PART + 3] > 0.0) {
            low = blk_tensor[b];
            break;
        }
    }
    rt[lane] = low;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if (lane < off) rt[lane] = rt[lane + off] < rt[lane] ? rt[lane + off] : rt[lane];
        __syncthreads();
    }
    if (lane) return;
    if (rt[0] < ntensors && state[1] < 0) {                  // sticky: the FIRST recorded row with a non-finite gradient
        state[1] = count;
        state[2] = rt[0];
    }
    steps[slot] = count;
    state[3] = state[3] + 1;
    state[0] = count + 1;
}

}  // namespace

extern "C" int32_t mcq_param_stats_columns(void) { return STATS_COLUMNS; }

extern "C" size_t mcq_param_stats_workspace_bytes(int32_t nblocks, int32_t ntensors) {
    return nblocks > 0 && ntensors > 0 ? STATS_HEAD * sizeof(long long) + (size_t)nblocks * STATS_PART * sizeof(double) : 0;
}

extern "C" int mcq_param_stats_before_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                          const int64_t* blk_first, int32_t nblocks, const int64_t* state, int64_t every, void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks) || !state || every <= 0) return MCQ_EINVAL;
    hipLaunchKernelGGL(param_stats_before_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, list, (const long long*)state,
                       (long long)every);
    return mcq_check_launch();
}

extern "C" int mcq_param_stats_after_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                         const int64_t* blk_first, int32_t nblocks, const int64_t* state, int64_t every, int64_t capacity,
                                         int32_t updates, const int32_t* skip, void* workspace, void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks) || !state || !workspace || every <= 0 || capacity <= 0)
        return MCQ_EINVAL;
    long long* head = (long long*)workspace;
    hipLaunchKernelGGL(param_stats_after_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, list, (const long long*)state,
                       (long long)every, (long long)capacity, updates ? 1 : 0, (const int*)skip, head, (double*)(head + STATS_HEAD));
    return mcq_check_launch();
}

extern "C" int mcq_param_stats_finish_f32(const int32_t* tensor_first_blk, const int32_t* blk_tensor, int32_t ntensors, int32_t nblocks,
                                          const void* workspace, int32_t updates, int64_t* state, int64_t* steps, float* ring, void* stream) {
    if (!tensor_first_blk || !blk_tensor || ntensors <= 0 || nblocks <= 0 || !workspace || !state || !steps || !ring) return MCQ_EINVAL;
    const long long* head = (const long long*)workspace;
    hipLaunchKernelGGL(param_stats_finish_kernel, dim3((unsigned)ntensors), dim3(64), 0, (hipStream_t)stream, (const double*)(head + STATS_HEAD),
                       head, (const int*)tensor_first_blk, (const int*)blk_tensor, (int)nblocks, (int)ntensors, updates ? 1 : 0,
                       (long long*)state, (long long*)steps, ring);
    return mcq_check_launch();
}
