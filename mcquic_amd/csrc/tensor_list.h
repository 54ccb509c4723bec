// MANY tensors in one launch: the device tables that Adam (adam.hip), LAMB (lamb.hip), SGD (sgd.hip), the weight average (ema.hip) and
// the gradient gather (train_ops.hip: gather_flat_kernel) walk, and the workgroup sum the optimizers share.  Not for the convolution
// sources.  The host builds the tables in mcquic_amd/tensor_list.py, class for struct (ChunkTable, TensorList).
//
// torch's fused Adam passes its tensor lists through kernel arguments (4 KB): 19 launches of ~91 us for this model's 666 tensors =
// 1.7 ms per step at 0.8 TB/s.  Here the lists live in device memory -- pointer tables [rows][ntensors] (row k of tensor t at
// ptrs[k * ntensors + t]; Adam, LAMB: param, grad, exp_avg, exp_avg_sq; SGD: param, grad, momentum buffer; EMA: param, average), numel[ntensors],
// and a block table (tensor, first element) with one entry per MCQ_LIST_CHUNK-element chunk, workgroup b taking entry b -- so the
// whole model is ONE launch of ~13 k workgroups.  A tensor without elements owns no chunk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int MCQ_LIST_CHUNK = 4096;                         // mcq_adam_chunk(): the host builds the block tables with it

struct McqChunk { int t; long long first, end; };            // elements [first, end) of tensor t

// the tables as ONE kernel argument, by value: the chunks (all the gather needs), then with the pointer rows
struct McqChunkTable {
    const long long* numel;
    const int* blk_tensor;
    const long long* blk_first;
    __device__ __forceinline__ McqChunk chunk() const {      // this workgroup's
        const int t = blk_tensor[blockIdx.x];
        const long long first = blk_first[blockIdx.x], n = numel[t];
        return {t, first, first + MCQ_LIST_CHUNK < n ? first + MCQ_LIST_CHUNK : n};
    }
};
struct McqTensorList : McqChunkTable {
    const unsigned long long* ptrs;
    int ntensors;
    __device__ __forceinline__ float* row(int k, int t) const { return (float*)ptrs[k * (size_t)ntensors + t]; }
};

// the list of an entry point's table arguments; false where one is missing or a count is not positive (MCQ_EINVAL)
inline bool mcq_tensor_list(McqTensorList* list, const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                            const int64_t* blk_first, int32_t nblocks) {
    if (!ptr_tables || !numel || !blk_tensor || !blk_first || ntensors <= 0 || nblocks <= 0) return false;
    *list = {{(const long long*)numel, (const int*)blk_tensor, (const long long*)blk_first}, (const unsigned long long*)ptr_tables, (int)ntensors};
    return true;
}

// sum over the workgroup's 256 lanes in a fixed tree (128, 64, ..., 1); the result is valid in lane 0.  A second sum through the same
// `red` needs a __syncthreads() in front: lane 0 must have read red[0] before it is overwritten.
__device__ __forceinline__ double mcq_block_sum256(double s, double* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}
