// SGD over MANY tensors in one launch (torch.optim.SGD's arithmetic: momentum, dampening, Nesterov, L2 decay, maximize) for gfx950,
// with two things torch's update does not have: clipping by the global gradient norm and a guard against a non-finite gradient.
//
// The tensor lists are the device tables of tensor_list.h (pointer rows: param, grad, momentum buffer, unused).  A call is
//   (a) sgd_prepare_kernel   ONE workgroup: the step count, the learning rate; with gradient partials (mcq_lamb_grad_partials_f32, one
//                            double per chunk) their sum in a fixed tree -> G, the clip factor and the skip flag
//   (b) sgd_update_kernel    one workgroup per chunk: 12 B / element without momentum, 20 B with it
// The kernel is bound by HBM: all it does about speed is 16 bytes per lane where a tensor's streams allow it -- a chunk starts a multiple
// of 4096 elements into its tensor, so a tensor's chunks are 16-byte aligned exactly when its base addresses are; a parameter that is a
// view, or a slice of a flat gradient buffer, may start at any 4-byte address and takes the dword loop.  No atomics, no sums in (b):
// equal inputs give equal bits.  Gradients are only read.  A skipped call writes nothing but the `skipped` counter: every workgroup of
// (b) reads the flag (a) wrote and leaves.
#include "mcq_common.h"
#include "tensor_list.h"
#include "../../include/mcquic_hip.h"

namespace {

struct SgdScalars { float lr; float clip; int first; int skip; };
static_assert(sizeof(SgdScalars) == 16, "`scalars` is 16 bytes");
struct SgdCoef { float momentum; float omd; float weight_decay; int nesterov; int maximize; };

__device__ __forceinline__ void sgd_prepare(const double* __restrict__ part, int nparts, float* __restrict__ step,
                                            const float* __restrict__ lr_dev, double lr_host,
                                            const float* __restrict__ max_grad_norm, float* __restrict__ grad_norm,
                                            int skip_nonfinite, long long* __restrict__ skipped, SgdScalars* __restrict__ sc, double* red) {
    double s = 0.0;
    if (part) {                                              // (the same for every lane: launched with 256 lanes then, with 64 otherwise)
        for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
        s = mcq_block_sum256(s, red);
    }
    if (threadIdx.x) return;
    float clip = 1.0f;
    int skip = 0;
    if (part) {
        const double G = sqrt(s);
        const float Gf = (float)G;
        grad_norm[0] = Gf;
        if (max_grad_norm) {                                 // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
            const float c = max_grad_norm[0] / (Gf + 1e-6f);
            clip = c > 1.0f ? 1.0f : c;                      // (a NaN factor stays NaN, as clamp leaves it)
        }
        if (skip_nonfinite && !isfinite(G)) {                // inf or NaN: one bad element anywhere poisons the sum
            skip = 1;
            if (skipped) skipped[0] += 1;
        }
    }
    const float t = step[0];
    if (!skip) step[0] = t + 1.0f;
    sc->lr = lr_dev ? lr_dev[0] : (float)lr_host;
    sc->clip = clip;
    sc->first = t == 0.0f ? 1 : 0;
    sc->skip = skip;
}

__global__ __launch_bounds__(256) void sgd_prepare_kernel(const double* __restrict__ part, int nparts, float* __restrict__ step,
                                                          const float* __restrict__ lr_dev, double lr_host,
                                                          const float* __restrict__ max_grad_norm, float* __restrict__ grad_norm,
                                                          int skip_nonfinite, long long* __restrict__ skipped, SgdScalars* __restrict__ sc) {
    __shared__ double red[256];
    sgd_prepare(part, nparts, step, lr_dev, lr_host, max_grad_norm, grad_norm, skip_nonfinite, skipped, sc, red);
}

// mcq_sgd_step_skip_f32: the step's guard flag (step_guard.hip) in front of SGD's own.  When it is set this kernel writes the scratch
// word (b) obeys and nothing else -- no step count, no norm, and not `skipped`: the step's guard has counted the step already.
__global__ __launch_bounds__(256) void sgd_prepare_skip_kernel(const double* __restrict__ part, int nparts, float* __restrict__ step,
                                                               const float* __restrict__ lr_dev, double lr_host,
                                                               const float* __restrict__ max_grad_norm, float* __restrict__ grad_norm,
                                                               int skip_nonfinite, long long* __restrict__ skipped, SgdScalars* __restrict__ sc,
                                                               const int* __restrict__ ext_skip) {
    __shared__ double red[256];
    if (ext_skip[0]) {
        if (threadIdx.x == 0) sc->skip = 1;
        return;
    }
    sgd_prepare(part, nparts, step, lr_dev, lr_host, max_grad_norm, grad_norm, skip_nonfinite, skipped, sc, red);
}

template <bool MOMENTUM>
__device__ __forceinline__ void sgd_element(float& p, float g, float& buf, const SgdScalars& sc, const SgdCoef& k) {
    if (sc.clip != 1.0f) g = g * sc.clip;                    // (a factor of exactly 1 changes nothing: not clipping is the same bits)
    if (k.maximize) g = -g;
    if (k.weight_decay != 0.0f) g = g + k.weight_decay * p;
    if (MOMENTUM) {
        buf = sc.first ? g : k.momentum * buf + k.omd * g;
        g = k.nesterov ? g + k.momentum * buf : buf;
    }
    p = p - sc.lr * g;
}

template <bool MOMENTUM>
__global__ __launch_bounds__(256) void sgd_update_kernel(McqTensorList list, const SgdScalars* __restrict__ scp, SgdCoef k) {
    const SgdScalars sc = *scp;
    if (sc.skip) return;
    const McqChunk c = list.chunk();
    const long long first = c.first, end = c.end;
    float* __restrict__ p = list.row(0, c.t);
    const float* __restrict__ g = list.row(1, c.t);
    float* __restrict__ m = MOMENTUM ? list.row(2, c.t) : nullptr;
    long long done = first;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0) {   // every stream of this tensor is 16-byte aligned (first % 4 == 0)
        const long long nvec = (end - first) >> 2;           // <= 1024 float4: at most four per lane
        float4* __restrict__ p4 = (float4*)(p + first);
        const float4* __restrict__ g4 = (const float4*)(g + first);
        float4* __restrict__ m4 = MOMENTUM ? (float4*)(m + first) : nullptr;
#pragma unroll 4
        for (long long i = threadIdx.x; i < nvec; i += 256) {
            float4 pv = p4[i];
            const float4 gv = g4[i];
            float4 mv = MOMENTUM ? m4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            sgd_element<MOMENTUM>(pv.x, gv.x, mv.x, sc, k);
            sgd_element<MOMENTUM>(pv.y, gv.y, mv.y, sc, k);
            sgd_element<MOMENTUM>(pv.z, gv.z, mv.z, sc, k);
            sgd_element<MOMENTUM>(pv.w, gv.w, mv.w, sc, k);
            if (MOMENTUM) m4[i] = mv;
            p4[i] = pv;
        }
        done = first + (nvec << 2);                          // the tensor's last 1..3 elements go through the dword loop below
    }
    for (long long i = done + threadIdx.x; i < end; i += 256) {
        float pi = p[i], mi = MOMENTUM ? m[i] : 0.0f;
        sgd_element<MOMENTUM>(pi, g[i], mi, sc, k);
        if (MOMENTUM) m[i] = mi;
        p[i] = pi;
    }
}

}  // namespace

extern "C" int mcq_sgd_step_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                     const int64_t* blk_first, int32_t nblocks, float* step, const float* lr_dev, double lr, double momentum,
                                     double dampening, double weight_decay, int32_t nesterov, int32_t maximize, const double* grad_partials,
                                     int32_t n_grad_partials, const float* max_grad_norm, float* grad_norm, int32_t skip_nonfinite, int64_t* skipped,
                                     void* scalars, const int32_t* skip, void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks) || !step || !scalars) return MCQ_EINVAL;
    if (!(momentum >= 0.0) || !(weight_decay >= 0.0) || !(dampening == dampening)) return MCQ_EINVAL;
    if (nesterov && (!(momentum > 0.0) || dampening != 0.0)) return MCQ_EINVAL;
    if (!lr_dev && !(lr >= 0.0)) return MCQ_EINVAL;
    if (grad_partials ? (n_grad_partials <= 0 || !grad_norm) : (max_grad_norm || skip_nonfinite || skipped)) return MCQ_EINVAL;   // clip and guard need the partials
    hipStream_t s = (hipStream_t)stream;
    if (skip)
        hipLaunchKernelGGL(sgd_prepare_skip_kernel, dim3(1), dim3(grad_partials ? 256 : 64), 0, s, grad_partials, (int)n_grad_partials, step, lr_dev, lr,
                           max_grad_norm, grad_norm, skip_nonfinite ? 1 : 0, (long long*)skipped, (SgdScalars*)scalars, (const int*)skip);
    else
        hipLaunchKernelGGL(sgd_prepare_kernel, dim3(1), dim3(grad_partials ? 256 : 64), 0, s, grad_partials, (int)n_grad_partials, step, lr_dev, lr,
                           max_grad_norm, grad_norm, skip_nonfinite ? 1 : 0, (long long*)skipped, (SgdScalars*)scalars);
    // (1 - dampening rounded from double, as torch passes `alpha = 1 - dampening` to _foreach_add_)
    const SgdCoef k = {(float)momentum, (float)(1.0 - dampening), (float)weight_decay, nesterov ? 1 : 0, maximize ? 1 : 0};
    hipLaunchKernelGGL(momentum != 0.0 ? sgd_update_kernel<true> : sgd_update_kernel<false>, dim3((unsigned)nblocks), dim3(256), 0, s, list,
                       (const SgdScalars*)scalars, k);
    return mcq_check_launch();
}

extern "C" int mcq_sgd_step_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                                int32_t nblocks, float* step, const float* lr_dev, double lr, double momentum, double dampening,
                                double weight_decay, int32_t nesterov, int32_t maximize, const double* grad_partials, int32_t n_grad_partials,
                                const float* max_grad_norm, float* grad_norm, int32_t skip_nonfinite, int64_t* skipped, void* scalars,
                                void* stream) {
    return mcq_sgd_step_skip_f32(ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks, step, lr_dev, lr, momentum, dampening, weight_decay,
                                 nesterov, maximize, grad_partials, n_grad_partials, max_grad_norm, grad_norm, skip_nonfinite, skipped, scalars,
                                 nullptr, stream);
}
