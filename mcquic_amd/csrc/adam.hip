// Adam / AdamW over MANY tensors in one launch (the update of mcquic/train/trainer.py:283; torch.optim.Adam's arithmetic) for gfx950.
//
// The tensor lists are the device tables of tensor_list.h (pointer rows: param, grad, exp_avg, exp_avg_sq), so the whole model is ONE
// launch that moves 28 bytes per element once.  A one-thread kernel in front advances the step counter and derives the bias corrections
// on the device (double precision), so learning rate and step may be device scalars a captured graph re-reads on every replay.
#include "mcq_common.h"
#include "tensor_list.h"
#include "../../include/mcquic_hip.h"

namespace {

struct AdamScalars { float step_size; float inv_sqrt_bc2; float lr; float pad; };

__device__ __forceinline__ void adam_prepare(float* __restrict__ step, const float* __restrict__ lr_dev, double lr_host, double beta1, double beta2,
                                             AdamScalars* __restrict__ sc) {
    if (blockIdx.x || threadIdx.x) return;
    const float t = step[0] + 1.0f;
    step[0] = t;
    const double lr = lr_dev ? (double)lr_dev[0] : lr_host;
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    sc->step_size = (float)(lr / bc1);
    sc->inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    sc->lr = (float)lr;
    sc->pad = 0.0f;
}

__global__ void adam_prepare_kernel(float* __restrict__ step, const float* __restrict__ lr_dev, double lr_host, double beta1, double beta2,
                                    AdamScalars* __restrict__ sc) {
    adam_prepare(step, lr_dev, lr_host, beta1, beta2, sc);
}

// the `_skip` twins (mcq_adam_step_skip_f32): the step's guard flag (step_guard.hip) is read once per workgroup, the branch is uniform,
// and a set flag leaves step count, scalars, moments and parameters untouched.  The kernels above are what runs without a flag.
__global__ void adam_prepare_skip_kernel(float* __restrict__ step, const float* __restrict__ lr_dev, double lr_host, double beta1, double beta2,
                                         AdamScalars* __restrict__ sc, const int* __restrict__ skip) {
    if (skip[0]) return;
    adam_prepare(step, lr_dev, lr_host, beta1, beta2, sc);
}

__device__ __forceinline__ void adam_update(const McqTensorList& list, const AdamScalars* __restrict__ sc, float omb1, float beta2, float omb2,
                                            float eps, float weight_decay, int decoupled, int maximize) {
    const McqChunk c = list.chunk();
    float* __restrict__ p = list.row(0, c.t);
    const float* __restrict__ g = list.row(1, c.t);
    float* __restrict__ m = list.row(2, c.t);
    float* __restrict__ v = list.row(3, c.t);
    const float step_size = sc->step_size, inv_sqrt_bc2 = sc->inv_sqrt_bc2, lr = sc->lr;
    for (long long i = c.first + threadIdx.x; i < c.end; i += 256) {
        float gi = g[i], pi = p[i];
        if (maximize) gi = -gi;
        if (weight_decay != 0.0f) {
            if (decoupled) pi = pi * (1.0f - lr * weight_decay);     // AdamW: param.mul_(1 - lr * wd)
            else gi = gi + weight_decay * pi;                        // Adam: grad.add(param, alpha = wd)
        }
        float mi = m[i], vi = v[i];
        mi = mi + (gi - mi) * omb1;                                  // exp_avg.lerp_(grad, 1 - beta1)
        vi = vi * beta2 + omb2 * gi * gi;                            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        m[i] = mi;
        v[i] = vi;
        p[i] = pi - step_size * (mi / denom);
    }
}

__global__ __launch_bounds__(256) void adam_update_kernel(McqTensorList list, const AdamScalars* __restrict__ sc, float omb1, float beta2, float omb2,
                                                          float eps, float weight_decay, int decoupled, int maximize) {
    adam_update(list, sc, omb1, beta2, omb2, eps, weight_decay, decoupled, maximize);
}

__global__ __launch_bounds__(256) void adam_update_skip_kernel(McqTensorList list, const AdamScalars* __restrict__ sc, float omb1, float beta2,
                                                               float omb2, float eps, float weight_decay, int decoupled, int maximize,
                                                               const int* __restrict__ skip) {
    if (skip[0]) return;
    adam_update(list, sc, omb1, beta2, omb2, eps, weight_decay, decoupled, maximize);
}

}  // namespace

extern "C" int32_t mcq_adam_chunk(void) { return MCQ_LIST_CHUNK; }

extern "C" int mcq_adam_step_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                      const int64_t* blk_first, int32_t nblocks, float* step, const float* lr_dev, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, int32_t decoupled, int32_t maximize, void* scalars,
                                      const int32_t* skip, void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks) || !step || !scalars) return MCQ_EINVAL;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return MCQ_EINVAL;
    if (!lr_dev && !(lr >= 0.0)) return MCQ_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (skip) {
        hipLaunchKernelGGL(adam_prepare_skip_kernel, dim3(1), dim3(64), 0, s, step, lr_dev, lr, beta1, beta2, (AdamScalars*)scalars, (const int*)skip);
        hipLaunchKernelGGL(adam_update_skip_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, list, (const AdamScalars*)scalars, (float)(1.0 - beta1),
                           (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (int)decoupled, (int)maximize, (const int*)skip);
        return mcq_check_launch();
    }
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(64), 0, s, step, lr_dev, lr, beta1, beta2, (AdamScalars*)scalars);
    // (1 - beta rounded from double, as torch passes `1 - beta2` to addcmul_: 1 - 0.999f would be 1.3e-5 off)
    hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, list, (const AdamScalars*)scalars, (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, (int)decoupled, (int)maximize);
    return mcq_check_launch();
}

extern "C" int mcq_adam_step_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                                 int32_t nblocks, float* step, const float* lr_dev, double lr, double beta1, double beta2, double eps,
                                 double weight_decay, int32_t decoupled, int32_t maximize, void* scalars, void* stream) {
    return mcq_adam_step_skip_f32(ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks, step, lr_dev, lr, beta1, beta2, eps, weight_decay,
                                  decoupled, maximize, scalars, nullptr, stream);
}
