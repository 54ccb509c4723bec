// Exponential moving average of MANY tensors in one launch, and the exchange of the live and the averaged weights in place, for gfx950.
//
// The tensor lists are the device tables of tensor_list.h (pointer rows: live parameter, average, unused, unused).  An update is
//   (a) ema_prepare_kernel   ONE workgroup: n = num_updates[0]; d_t = decay (decay_dev[0] when given), with warm-up
//                            min(decay, (1 + n) / (10 + n)) in double; the weight w = float(1 - d_t) -> `scalars`; num_updates[0] = n + 1
//   (b) ema_update_kernel    one workgroup per chunk: avg = lerp(avg, p, w), 12 B / element
// lerp is torch's (ATen/native/Lerp.h, what torch.optim.swa_utils.get_ema_multi_avg_fn runs through _foreach_lerp_), in float32:
//   d = p - avg;  avg + w d  where w < 0.5,  p - d (1 - w)  otherwise -- at w = 1 (decay 0) the second form is p itself, bit for bit.
// The swap exchanges rows 0 and 1 as raw 32-bit words (16 B / element): no arithmetic touches a value, so NaN payloads and the sign
// of -0.0 survive and two swaps are the identity.  Both kernels are bound by HBM; as in sgd.hip, all they do about speed is 16 bytes
// per lane where both rows of a tensor are 16-byte aligned (a chunk starts a multiple of 4096 elements into its tensor), four such
// accesses per lane in flight; a parameter that is a view may start at any 4-byte address and takes the dword loop, as do a tensor's
// last 1..3 elements.  No atomics, no sums: equal inputs give equal bits.  The host reads nothing.
#include "mcq_common.h"
#include "tensor_list.h"
#include "../../include/mcquic_hip.h"

namespace {

struct EmaScalars { float w; float omw; float decay; int pad; };   // the weight of the live value, 1 - w (both float32), d_t (for inspection)
static_assert(sizeof(EmaScalars) == 16, "`scalars` is 16 bytes");

__device__ __forceinline__ void ema_prepare(long long* __restrict__ num_updates, const float* __restrict__ decay_dev, double decay_host,
                                            int warmup, EmaScalars* __restrict__ sc) {
    if (threadIdx.x) return;
    const long long n = num_updates[0];
    double d = decay_dev ? (double)decay_dev[0] : decay_host;
    if (warmup) {
        const double ramp = (1.0 + (double)n) / (10.0 + (double)n);
        d = ramp < d ? ramp : d;                             // (a NaN decay stays NaN, as torch's min leaves it)
    }
    const float w = (float)(1.0 - d);                        // torch hands `1 - decay`, a double, to the float32 lerp
    sc->w = w;
    sc->omw = 1.0f - w;
    sc->decay = (float)d;
    sc->pad = 0;
    num_updates[0] = n + 1;
}

__global__ __launch_bounds__(64) void ema_prepare_kernel(long long* __restrict__ num_updates, const float* __restrict__ decay_dev, double decay_host,
                                                         int warmup, EmaScalars* __restrict__ sc) {
    ema_prepare(num_updates, decay_dev, decay_host, warmup, sc);
}

// the `_skip` twins (mcq_ema_update_skip_f32): with the step's guard flag set (step_guard.hip) neither the count nor an average moves
__global__ __launch_bounds__(64) void ema_prepare_skip_kernel(long long* __restrict__ num_updates, const float* __restrict__ decay_dev, double decay_host,
                                                              int warmup, EmaScalars* __restrict__ sc, const int* __restrict__ skip) {
    if (skip[0]) return;
    ema_prepare(num_updates, decay_dev, decay_host, warmup, sc);
}

__device__ __forceinline__ float ema_lerp(float a, float p, float w, float omw, bool low) {
    const float d = p - a;
    return low ? a + w * d : p - d * omw;
}

__device__ __forceinline__ void ema_update(const McqTensorList& list, const EmaScalars* __restrict__ scp) {
    const float w = scp->w, omw = scp->omw;
    const bool low = fabsf(w) < 0.5f;
    const McqChunk c = list.chunk();
    const long long first = c.first, end = c.end;
    const float* __restrict__ p = list.row(0, c.t);
    float* __restrict__ a = list.row(1, c.t);
    long long done = first;
    if ((((uintptr_t)p | (uintptr_t)a) & 15) == 0) {         // both streams of this tensor are 16-byte aligned (first % 4 == 0)
        const long long nvec = (end - first) >> 2;           // <= 1024 float4: at most four per lane
        const float4* __restrict__ p4 = (const float4*)(p + first);
        float4* __restrict__ a4 = (float4*)(a + first);
#pragma unroll 4
        for (long long i = threadIdx.x; i < nvec; i += 256) {
            const float4 pv = p4[i];
            float4 av = a4[i];
            av.x = ema_lerp(av.x, pv.x, w, omw, low);
            av.y = ema_lerp(av.y, pv.y, w, omw, low);
            av.z = ema_lerp(av.z, pv.z, w, omw, low);
            av.w = ema_lerp(av.w, pv.w, w, omw, low);
            a4[i] = av;
        }
        done = first + (nvec << 2);                          // the tensor's last 1..3 elements go through the dword loop below
    }
    for (long long i = done + threadIdx.x; i < end; i += 256) a[i] = ema_lerp(a[i], p[i], w, omw, low);
}

__global__ __launch_bounds__(256) void ema_update_kernel(McqTensorList list, const EmaScalars* __restrict__ scp) { ema_update(list, scp); }

__global__ __launch_bounds__(256) void ema_update_skip_kernel(McqTensorList list, const EmaScalars* __restrict__ scp, const int* __restrict__ skip) {
    if (skip[0]) return;
    ema_update(list, scp);
}

__global__ __launch_bounds__(256) void ema_swap_kernel(McqTensorList list) {
    const McqChunk c = list.chunk();
    const long long first = c.first, end = c.end;
    uint32_t* __restrict__ p = (uint32_t*)list.row(0, c.t);
    uint32_t* __restrict__ a = (uint32_t*)list.row(1, c.t);
    long long done = first;
    if ((((uintptr_t)p | (uintptr_t)a) & 15) == 0) {
        const long long nvec = (end - first) >> 2;
        uint4* __restrict__ p4 = (uint4*)(p + first);
        uint4* __restrict__ a4 = (uint4*)(a + first);
#pragma unroll 4
        for (long long i = threadIdx.x; i < nvec; i += 256) {
            const uint4 pv = p4[i], av = a4[i];
            p4[i] = av;
            a4[i] = pv;
        }
        done = first + (nvec << 2);
    }
    for (long long i = done + threadIdx.x; i < end; i += 256) {
        const uint32_t pi = p[i], ai = a[i];
        p[i] = ai;
        a[i] = pi;
    }
}

}  // namespace

extern "C" int mcq_ema_update_skip_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor,
                                       const int64_t* blk_first, int32_t nblocks, int64_t* num_updates, const float* decay_dev, double decay,
                                       int32_t warmup, void* scalars, const int32_t* skip, void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks) || !num_updates || !scalars) return MCQ_EINVAL;
    if (!(decay >= 0.0 && decay <= 1.0)) return MCQ_EINVAL;  // (NaN too; with decay_dev the host value is not used: pass 0)
    hipStream_t s = (hipStream_t)stream;
    if (skip) {
        hipLaunchKernelGGL(ema_prepare_skip_kernel, dim3(1), dim3(64), 0, s, (long long*)num_updates, decay_dev, decay, warmup ? 1 : 0,
                           (EmaScalars*)scalars, (const int*)skip);
        hipLaunchKernelGGL(ema_update_skip_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, list, (const EmaScalars*)scalars, (const int*)skip);
        return mcq_check_launch();
    }
    hipLaunchKernelGGL(ema_prepare_kernel, dim3(1), dim3(64), 0, s, (long long*)num_updates, decay_dev, decay, warmup ? 1 : 0, (EmaScalars*)scalars);
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, list, (const EmaScalars*)scalars);
    return mcq_check_launch();
}

extern "C" int mcq_ema_update_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                                  int32_t nblocks, int64_t* num_updates, const float* decay_dev, double decay, int32_t warmup, void* scalars,
                                  void* stream) {
    return mcq_ema_update_skip_f32(ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks, num_updates, decay_dev, decay, warmup, scalars,
                                   nullptr, stream);
}

extern "C" int mcq_ema_swap_f32(const void* ptr_tables, int32_t ntensors, const int64_t* numel, const int32_t* blk_tensor, const int64_t* blk_first,
                                int32_t nblocks, void* stream) {
    McqTensorList list;
    if (!mcq_tensor_list(&list, ptr_tables, ntensors, numel, blk_tensor, blk_first, nblocks)) return MCQ_EINVAL;
    hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, list);
    return mcq_check_launch();
}
