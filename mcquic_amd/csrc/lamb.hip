// LAMB over MANY tensors with per-tensor trust ratios (the reference's `FusedLAMB` registry entry, mcquic/train/ddp.py:53-69; the
// arithmetic is apex FusedLAMB's published algorithm, written out in mcquic_amd/optim.py) for gfx950.
//
// The tensor lists are the device tables of tensor_list.h (pointer rows: param, grad, exp_avg, exp_avg_sq) plus
// tensor_first_blk[ntensors + 1], so a tensor's chunks are a contiguous range.  A step is five launches whatever the number of tensors:
//   (a) lamb_gradsq_kernel    one double partial of sum g^2 per chunk                                   4 B / element
//   (b) lamb_prepare_kernel   ONE workgroup: the partials of every group in a fixed order -> G, the clip divisor, the step count
//                             and the bias corrections (double, rounded once), the learning rate
//   (c) lamb_stage1_kernel    m, v updated; (sum p^2, sum u^2) of the chunk into the chunk's own slot   24 B / element
//   (d) lamb_ratio_kernel     per tensor: its chunks' partials in chunk order -> ||p|| / ||u|| and r
//   (e) lamb_stage2_kernel    u recomputed from the new m, v and the old p by the SAME expression, p -= r u   16 B / element
// Every partial is a double, every sum a fixed tree, no atomics: the same state and gradients give the same bits.  The gradients
// are only read (apex overwrites them with u).  Loads are one dword per lane, consecutive lanes consecutive elements, as in
// adam_update_kernel: the slices of a flat gradient buffer are 4-byte aligned only.
#include "mcq_common.h"
#include "tensor_list.h"
#include "../../include/mcquic_hip.h"

namespace {

struct LambScalars { float clip; float bc1; float bc2; float lr; };

// the update direction; stage 1 (norm) and stage 2 (apply) both call this on the same floats, so they see the same bits
__device__ __forceinline__ float lamb_direction(float m, float v, float p, const LambScalars& sc, float eps, float weight_decay, int adam_w) {
    const float u = (m / sc.bc1) / (sqrtf(v / sc.bc2) + eps);
    return adam_w ? u + weight_decay * p : u;
}

__device__ __forceinline__ void lamb_gradsq(const McqTensorList& list, double* __restrict__ part, double* red) {
    const McqChunk c = list.chunk();
    const float* __restrict__ g = list.row(1, c.t);
    double s = 0.0;
#pragma unroll 4
    for (long long i = c.first + threadIdx.x; i < c.end; i += 256) {
        const double gi = (double)g[i];
        s += gi * gi;
    }
    s = mcq_block_sum256(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void lamb_gradsq_kernel(McqTensorList list, double* __restrict__ part) {
    __shared__ double red[256];
    lamb_gradsq(list, part, red);
}

// The `_skip` twins of all five launches (mcq_lamb_grad_partials_skip_f32, mcq_lamb_step_skip_f32): the step's guard flag (step_guard.hip)
// is read once per workgroup, the branch is uniform, and a set flag leaves partials, step count, scalars, moments, ratios, rates and
// parameters untouched.  The kernels without the suffix are what runs without a flag.
__global__ __launch_bounds__(256) void lamb_gradsq_skip_kernel(McqTensorList list, double* __restrict__ part, const int* __restrict__ skip) {
    __shared__ double red[256];
    if (skip[0]) return;
    lamb_gradsq(list, part, red);
}

__device__ __forceinline__ void lamb_prepare(const double* __restrict__ part, int nparts, float* __restrict__ step,
                                             const float* __restrict__ lr_dev, double lr_host, double beta1, double beta2,
                                             int bias_correction, float max_grad_norm, float* __restrict__ grad_norm,
                                             LambScalars* __restrict__ sc, double* red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = mcq_block_sum256(s, red);
    if (threadIdx.x) return;
    const float G = (float)sqrt(s);
    grad_norm[0] = G;
    sc->clip = G > max_grad_norm ? G / max_grad_norm : 1.0f;          // (a NaN norm compares false: no clipping)
    const float t = step[0] + 1.0f;
    step[0] = t;
    sc->bc1 = bias_correction ? (float)(1.0 - pow(beta1, (double)t)) : 1.0f;
    sc->bc2 = bias_correction ? (float)(1.0 - pow(beta2, (double)t)) : 1.0f;
    sc->lr = lr_dev ? lr_dev[0] : (float)lr_host;
}

__global__ __launch_bounds__(256) void lamb_prepare_kernel(const double* __restrict__ part, int nparts, float* __restrict__ step,
                                                           const float* __restrict__ lr_dev, double lr_host, double beta1, double beta2,
                                                           int bias_correction, float max_grad_norm, float* __restrict__ grad_norm,
                                                           LambScalars* __restrict__ sc) {
    __shared__ double red[256];
    lamb_prepare(part, nparts, step, lr_dev, lr_host, beta1, beta2, bias_correction, max_grad_norm, grad_norm, sc, red);
}

__global__ __launch_bounds__(256) void lamb_prepare_skip_kernel(const double* __restrict__ part, int nparts, float* __restrict__ step,
                                                                const float* __restrict__ lr_dev, double lr_host, double beta1, double beta2,
                                                                int bias_correction, float max_grad_norm, float* __restrict__ grad_norm,
                                                                LambScalars* __restrict__ sc, const int* __restrict__ skip) {
    __shared__ double red[256];
    if (skip[0]) return;
    lamb_prepare(part, nparts, step, lr_dev, lr_host, beta1, beta2, bias_correction, max_grad_norm, grad_norm, sc, red);
}

__device__ __forceinline__ void lamb_stage1(const McqTensorList& list, const LambScalars* __restrict__ scp, float beta1, float beta3, float beta2,
                                            float omb2, float eps, float weight_decay, int adam_w, double* __restrict__ part_pu, double* red) {
    const McqChunk c = list.chunk();
    const float* __restrict__ p = list.row(0, c.t);
    const float* __restrict__ g = list.row(1, c.t);
    float* __restrict__ m = list.row(2, c.t);
    float* __restrict__ v = list.row(3, c.t);
    const LambScalars sc = *scp;
    double sp = 0.0, su = 0.0;
#pragma unroll 4
    for (long long i = c.first + threadIdx.x; i < c.end; i += 256) {
        const float pi = p[i];
        float gi = g[i] / sc.clip;
        if (!adam_w) gi = gi + weight_decay * pi;                    // L2: the decay joins the gradient
        const float mi = beta1 * m[i] + beta3 * gi;
        const float vi = beta2 * v[i] + omb2 * (gi * gi);
        m[i] = mi;
        v[i] = vi;
        const double ui = (double)lamb_direction(mi, vi, pi, sc, eps, weight_decay, adam_w);
        sp += (double)pi * (double)pi;
        su += ui * ui;
    }
    sp = mcq_block_sum256(sp, red);
    __syncthreads();                                                 // (lane 0 has read red[0] before it is overwritten)
    su = mcq_block_sum256(su, red);
    if (threadIdx.x == 0) {
        part_pu[2 * (size_t)blockIdx.x] = sp;
        part_pu[2 * (size_t)blockIdx.x + 1] = su;
    }
}

__global__ __launch_bounds__(256) void lamb_stage1_kernel(McqTensorList list, const LambScalars* __restrict__ scp, float beta1, float beta3, float beta2,
                                                          float omb2, float eps, float weight_decay, int adam_w, double* __restrict__ part_pu) {
    __shared__ double red[256];
    lamb_stage1(list, scp, beta1, beta3, beta2, omb2, eps, weight_decay, adam_w, part_pu, red);
}

__global__ __launch_bounds__(256) void lamb_stage1_skip_kernel(McqTensorList list, const LambScalars* __restrict__ scp, float beta1, float beta3,
                                                               float beta2, float omb2, float eps, float weight_decay, int adam_w,
                                                               double* __restrict__ part_pu, const int* __restrict__ skip) {
    __shared__ double red[256];
    if (skip[0]) return;
    lamb_stage1(list, scp, beta1, beta3, beta2, omb2, eps, weight_decay, adam_w, part_pu, red);
}

// one 64-lane workgroup per tensor: lane l takes chunks l, l + 64, ... in order, then a fixed tree over the lanes
__device__ __forceinline__ void lamb_ratio(const double* __restrict__ part_pu, const int* __restrict__ tensor_first_blk,
                                           const LambScalars* __restrict__ scp, int scaled, float* __restrict__ rate, float* __restrict__ ratio,
                                           double* rp, double* ru) {
    const int t = blockIdx.x;
    const int b0 = tensor_first_blk[t], b1 = tensor_first_blk[t + 1];
    double sp = 0.0, su = 0.0;
    for (int b = b0 + threadIdx.x; b < b1; b += 64) {
        sp += part_pu[2 * (size_t)b];
        su += part_pu[2 * (size_t)b + 1];
    }
    rp[threadIdx.x] = sp;
    ru[threadIdx.x] = su;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            rp[threadIdx.x] += rp[threadIdx.x + off];
            ru[threadIdx.x] += ru[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x) return;
    const double pn = sqrt(rp[0]), un = sqrt(ru[0]);
    const float q = (float)(pn / un);                                // (inf / 0 / NaN where a norm is zero: a diagnostic, not used then)
    const float lr = scp->lr;
    ratio[t] = q;
    rate[t] = (scaled && pn != 0.0 && un != 0.0) ? lr * q : lr;
}

__global__ __launch_bounds__(64) void lamb_ratio_kernel(const double* __restrict__ part_pu, const int* __restrict__ tensor_first_blk,
                                                        const LambScalars* __restrict__ scp, int scaled, float* __restrict__ rate,
                                                        float* __restrict__ ratio) {
    __shared__ double rp[64], ru[64];
    lamb_ratio(part_pu, tensor_first_blk, scp, scaled, rate, ratio, rp, ru);
}

__global__ __launch_bounds__(64) void lamb_ratio_skip_kernel(const double* __restrict__ part_pu, const int* __restrict__ tensor_first_blk,
                                                             const LambScalars* __restrict__ scp, int scaled, float* __restrict__ rate,
                                                             float* __restrict__ ratio, const int* __restrict__ skip) {
    __shared__ double rp[64], ru[64];
    if (skip[0]) return;
    lamb_ratio(part_pu, tensor_first_blk, scp, scaled, rate, ratio, rp, ru);
}

__device__ __forceinline__ void lamb_stage2(const McqTensorList& list, const LambScalars* __restrict__ scp, const float* __restrict__ rate, float eps,
                                            float weight_decay, int adam_w) {
    const McqChunk c = list.chunk();
    float* __restrict__ p = list.row(0, c.t);
    const float* __restrict__ m = list.row(2, c.t);
    const float* __restrict__ v = list.row(3, c.t);
    const LambScalars sc = *scp;
    const float r = rate[c.t];
#pragma unroll 4
    for (long long i = c.first + threadIdx.x; i < c.end; i += 256) {
        const float pi = p[i];
        p[i] = pi - r * lamb_direction(m[i], v[i], pi, sc, eps, weight_decay, adam_w);
    }
}

__global__ __launch_bounds__(256) void lamb_stage2_kernel(McqTensorList list, const LambScalars* __restrict__ scp, const float* __restrict__ rate, float eps,
                                                          float weight_decay, int adam_w) {
    lamb_stage2(list, scp, rate, eps, weight_decay, adam_w);
}

__global__ __launch_bounds__(256) void lamb_stage2_skip_kernel(McqTensorList list, const LambScalars* __restrict__ scp, const float* __restrict__ rate,
                                                               float eps, float weight_decay, int adam_w, const int* __restrict__ skip) {
    if (skip[0]) return;
    lamb_stage2(list, scp, rate, eps, weight_decay, adam_w);
}

// double part_pu[2 * nblocks] | float rate[ntensors]
size_t lamb_rate_offset(int32_t nblocks) { return (size_t)nblocks * 2 * sizeof(double); }

}  // namespace

extern "C" size_t mcq_lamb_workspace_bytes(int32_t ntensors, int32_t nblocks) {
    return ntensors > 0 && nblocks > 0 ? lamb_rate_offset(nblocks) + (size_t)ntensors * sizeof(float) : 0;
}

extern "C" int mcq_lamb_grad_partials_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                               const int64_t* blk_first, int32_t nblocks, double* partials, const int32_t* skip, void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks) || !partials) return MCQ_EINVAL;
    if (skip) hipLaunchKernelGGL(lamb_gradsq_skip_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, list, partials, (const int*)skip);
    else hipLaunchKernelGGL(lamb_gradsq_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, list, partials);
    return mcq_check_launch();
}

extern "C" int mcq_lamb_grad_partials_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                          const int64_t* blk_first, int32_t nblocks, double* partials, void* stream) {
    return mcq_lamb_grad_partials_skip_f32(ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks, partials, nullptr, stream);
}

extern "C" int mcq_lamb_step_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                      const int64_t* blk_first, const int32_t* tensor_first_blk, int32_t nblocks, const double* grad_partials,
                                      int32_t n_grad_partials, float* step, const float* lr_dev, double lr, double beta1, double beta2, double eps,
                                      double weight_decay, int32_t bias_correction, int32_t adam_w_mode, int32_t grad_averaging, int32_t use_nvlamb,
                                      double max_grad_norm, float* grad_norm, float* ratios, void* workspace, void* scalars, const int32_t* skip,
                                      void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks) || !tensor_first_blk || !grad_partials || !step ||
        !grad_norm || !ratios || !workspace || !scalars || n_grad_partials <= 0)
        return MCQ_EINVAL;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0) || !(max_grad_norm >= 0.0))
        return MCQ_EINVAL;
    if (!lr_dev && !(lr >= 0.0)) return MCQ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const LambScalars* sc = (const LambScalars*)scalars;
    double* part_pu = (double*)workspace;
    float* rate = (float*)((char*)workspace + lamb_rate_offset(nblocks));
    const float wd = (float)weight_decay, epsf = (float)eps;
    const int adam_w = adam_w_mode ? 1 : 0;
    if (skip) {
        const int* sk = (const int*)skip;
        hipLaunchKernelGGL(lamb_prepare_skip_kernel, dim3(1), dim3(256), 0, s, grad_partials, (int)n_grad_partials, step, lr_dev, lr, beta1, beta2,
                           (int)bias_correction, (float)max_grad_norm, grad_norm, (LambScalars*)scalars, sk);
        hipLaunchKernelGGL(lamb_stage1_skip_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, list, sc, (float)beta1,
                           grad_averaging ? (float)(1.0 - beta1) : 1.0f, (float)beta2, (float)(1.0 - beta2), epsf, wd, adam_w, part_pu, sk);
        hipLaunchKernelGGL(lamb_ratio_skip_kernel, dim3((unsigned)ntensors), dim3(64), 0, s, (const double*)part_pu, (const int*)tensor_first_blk, sc,
                           (use_nvlamb || weight_decay != 0.0) ? 1 : 0, rate, ratios, sk);
        hipLaunchKernelGGL(lamb_stage2_skip_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, list, sc, (const float*)rate, epsf, wd, adam_w, sk);
        return mcq_check_launch();
    }
    hipLaunchKernelGGL(lamb_prepare_kernel, dim3(1), dim3(256), 0, s, grad_partials, (int)n_grad_partials, step, lr_dev, lr, beta1, beta2,
                       (int)bias_correction, (float)max_grad_norm, grad_norm, (LambScalars*)scalars);
    // (1 - beta rounded from double, as in mcq_adam_step_f32)
    hipLaunchKernelGGL(lamb_stage1_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, list, sc, (float)beta1, grad_averaging ? (float)(1.0 - beta1) : 1.0f,
                       (float)beta2, (float)(1.0 - beta2), epsf, wd, adam_w, part_pu);
    hipLaunchKernelGGL(lamb_ratio_kernel, dim3((unsigned)ntensors), dim3(64), 0, s, (const double*)part_pu, (const int*)tensor_first_blk, sc,
                       (use_nvlamb || weight_decay != 0.0) ? 1 : 0, rate, ratios);
    hipLaunchKernelGGL(lamb_stage2_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, list, sc, (const float*)rate, epsf, wd, adam_w);
    return mcq_check_launch();
}

extern "C" int mcq_lamb_step_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                                 const int32_t* tensor_first_blk, int32_t nblocks, const double* grad_partials, int32_t n_grad_partials,
                                 float* step, const float* lr_dev, double lr, double beta1, double beta2, double eps, double weight_decay,
                                 int32_t bias_correction, int32_t adam_w_mode, int32_t grad_averaging, int32_t use_nvlamb, double max_grad_norm,
                                 float* grad_norm, float* ratios, void* workspace, void* scalars, void* stream) {
    return mcq_lamb_step_skip_f32(ptr_tables, ntensors, numel, blk_tensor, blk_first, tensor_first_blk, nblocks, grad_partials, n_grad_partials, step,
                                  lr_dev, lr, beta1, beta2, eps, weight_decay, bias_correction, adam_w_mode, grad_averaging, use_nvlamb, max_grad_norm,
                                  grad_norm, ratios, workspace, scalars, nullptr, stream);
}
