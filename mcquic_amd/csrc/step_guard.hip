// The non-finite guard of a training step, for gfx950: ONE flag per step, decided on the device, that every kernel of the update obeys.
//
// A captured step has no host between replays, so nobody can look at a gradient before the optimizer, the weight average, the frequency
// EMA and the schedule have consumed it; one inf in one gradient poisons all of them for good.  The guard decides from the global norm
// G of the (all-reduced) gradient and writes a 24-byte record, include/mcquic_hip.h:
//     { int32 skip = !isfinite(G);  float grad_norm = G;  int64 skipped (+1 on a skipped step);  int64 consecutive (0 on a clean one) }
// The update kernels take `&record.skip` (adam.hip, lamb.hip, sgd.hip, ema.hip, schedule.hip, step_ops.hip, train_ops.hip: their `_skip`
// entry points): every workgroup reads the word once, branches uniformly and, when it is set, writes nothing.
//
// G is formed the way sgd.hip forms it: one double partial of sum g^2 per MCQ_LIST_CHUNK-element chunk, each a fixed tree over 256 lanes
// (guard_gradsq_*_kernel), then ONE workgroup sums the partials, lane-strided and through the same tree (guard_finish_kernel).  No
// atomics: equal inputs give equal bits.  The squares and their sums are doubles, so a gradient of 1e19 per element (whose float32 square
// is inf) has the finite norm it has; only a gradient that holds an inf or a NaN, or whose norm leaves double range, is skipped.
// Where a norm of the same gradient exists already, no second reduction is launched: guard_finish_kernel takes the partials LAMB and SGD
// computed for themselves (mcq_lamb_grad_partials_f32), and guard_borrow_kernel takes a float32 norm, or sum of squares, by pointer
// (the step's clipping, mcq_sumsq_f32) -- then the flag is the lender's arithmetic: a float32 sum of squares that overflowed is skipped.
// Plain C++ stores from lane 0; nothing is read by the host.
#include "mcq_common.h"
#include "tensor_list.h"
#include "../../include/mcquic_hip.h"

namespace {

struct GuardRecord { int32_t skip; float grad_norm; long long skipped; long long consecutive; };
static_assert(sizeof(GuardRecord) == 24, "the record is 24 bytes: int32, float, int64, int64");

__device__ __forceinline__ double guard_chunk_sumsq(const float* __restrict__ g, long long first, long long end, double* red) {
    double s = 0.0;
#pragma unroll 4
    for (long long i = first + threadIdx.x; i < end; i += 256) {
        const double gi = (double)g[i];
        s += gi * gi;
    }
    return mcq_block_sum256(s, red);
}

__global__ __launch_bounds__(256) void guard_gradsq_list_kernel(McqTensorList list, double* __restrict__ part) {
    __shared__ double red[256];
    const McqChunk c = list.chunk();
    const double s = guard_chunk_sumsq(list.row(1, c.t), c.first, c.end, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void guard_gradsq_flat_kernel(const float* __restrict__ g, long long n, double* __restrict__ part) {
    __shared__ double red[256];
    const long long first = (long long)blockIdx.x * MCQ_LIST_CHUNK;
    const double s = guard_chunk_sumsq(g, first, first + MCQ_LIST_CHUNK < n ? first + MCQ_LIST_CHUNK : n, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// (one lane) the record of this step from its norm
__device__ __forceinline__ void guard_commit(GuardRecord* __restrict__ rec, bool finite, float G) {
    rec->skip = finite ? 0 : 1;
    rec->grad_norm = G;
    if (finite) {
        rec->consecutive = 0;
    } else {
        rec->skipped += 1;
        rec->consecutive += 1;
    }
}

__global__ __launch_bounds__(256) void guard_finish_kernel(const double* __restrict__ part, int nparts, GuardRecord* __restrict__ rec) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = mcq_block_sum256(s, red);
    if (threadIdx.x) return;
    const double G = sqrt(s);                                // (sgd_prepare_kernel's G: inf or NaN when one element anywhere is)
    guard_commit(rec, isfinite(G), (float)G);
}

__global__ __launch_bounds__(64) void guard_borrow_kernel(const float* __restrict__ value, int squared, GuardRecord* __restrict__ rec) {
    if (threadIdx.x) return;
    const float G = squared ? sqrtf(value[0]) : value[0];    // (clip_by_norm_kernel's norm from mcq_sumsq_f32's sum)
    guard_commit(rec, isfinite(G), G);
}

}  // namespace

extern "C" int64_t mcq_step_guard_chunks(int64_t n) { return n > 0 ? (n + MCQ_LIST_CHUNK - 1) / MCQ_LIST_CHUNK : 0; }

extern "C" int mcq_step_guard_partials_f32(const double* partials, int32_t n_partials, void* record, void* stream) {
    if (!partials || n_partials <= 0 || !record) return MCQ_EINVAL;
    hipLaunchKernelGGL(guard_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (int)n_partials, (GuardRecord*)record);
    return mcq_check_launch();
}

extern "C" int mcq_step_guard_list_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                       const int64_t* blk_first, int32_t nblocks, double* partials, const double* all_partials,
                                       int32_t n_all_partials, void* record, void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks) || !partials) return MCQ_EINVAL;
    if (record && (!all_partials || n_all_partials <= 0)) return MCQ_EINVAL;
    hipLaunchKernelGGL(guard_gradsq_list_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, list, partials);
    if (!record) return mcq_check_launch();                  // (a further parameter group follows: the last one's call decides)
    return mcq_step_guard_partials_f32(all_partials, n_all_partials, record, stream);
}

extern "C" int mcq_step_guard_flat_f32(const float* grad, int64_t n, double* partials, void* record, void* stream) {
    if (!grad || n <= 0 || !partials || !record) return MCQ_EINVAL;
    const int64_t chunks = mcq_step_guard_chunks(n);
    if (chunks > 0x7fffffffLL) return MCQ_ETOOLARGE;
    hipLaunchKernelGGL(guard_gradsq_flat_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, grad, (long long)n, partials);
    return mcq_step_guard_partials_f32(partials, (int32_t)chunks, record, stream);
}

extern "C" int mcq_step_guard_norm_f32(const float* value, int32_t squared, void* record, void* stream) {
    if (!value || !record) return MCQ_EINVAL;
    hipLaunchKernelGGL(guard_borrow_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, value, squared ? 1 : 0, (GuardRecord*)record);
    return mcq_check_launch();
}
