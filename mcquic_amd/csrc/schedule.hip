// Learning-rate schedules stepped on the device, for gfx950: one launch of one workgroup, one lane per parameter group.
//
// The reference steps its scheduler on the host after every batch (mcquic/train/trainer.py `_stepFinish`); a captured training step
// has no host between replays, so the schedule's state lives on the device -- last_epoch (int64) and eight doubles per group,
// include/mcquic_hip.h -- and this kernel is what `scheduler.step()` is: it advances the state by the rule of schedule_rule.h and stores
// float(rate) into the 0-dim float32 tensor the optimizer's kernel reads.  The float64 state is the truth; the float32 store is only
// its rounding, so a recurrence on the rate (MultiStep's `rate * gamma`) never rounds through float32.  There is nothing to make
// fast here: a few dozen double operations per lane, one libm call at most.  Every lane reads last_epoch before lane 0 stores its
// successor (the barrier), each lane touches its own eight doubles and its own lr tensor: no atomics, equal state gives equal bits.
#include "mcq_common.h"
#include "schedule_rule.h"

namespace {

__device__ __forceinline__ void lr_schedule(const mcq_lr_schedule& r, long long* __restrict__ last_epoch, double* __restrict__ state,
                                            float* const* __restrict__ lr) {
    const int g = threadIdx.x;
    const long long e = last_epoch[0] + 1;
    __syncthreads();
    if (g == 0) last_epoch[0] = e;
    if (g >= r.ngroups) return;
    double* sg = state + (size_t)g * MCQ_LR_STATE_WORDS;
    double s[MCQ_LR_STATE_WORDS];
#pragma unroll
    for (int i = 0; i < MCQ_LR_STATE_WORDS; ++i) s[i] = sg[i];
    mcq_lr_step(r, e, s);
#pragma unroll
    for (int i = 0; i < MCQ_LR_STATE_WORDS; ++i) sg[i] = s[i];
    *lr[g] = (float)s[MCQ_LR_RATE];
}

__global__ __launch_bounds__(MCQ_LR_MAX_GROUPS) void lr_schedule_kernel(mcq_lr_schedule r, long long* __restrict__ last_epoch,
                                                                        double* __restrict__ state, float* const* __restrict__ lr) {
    lr_schedule(r, last_epoch, state, lr);
}

// mcq_lr_schedule_step_skip: with the step's guard flag set (step_guard.hip) the schedule stays where it is -- last_epoch, state and rates
__global__ __launch_bounds__(MCQ_LR_MAX_GROUPS) void lr_schedule_skip_kernel(mcq_lr_schedule r, long long* __restrict__ last_epoch,
                                                                             double* __restrict__ state, float* const* __restrict__ lr,
                                                                             const int* __restrict__ skip) {
    if (skip[0]) return;
    lr_schedule(r, last_epoch, state, lr);
}

}  // namespace

extern "C" int mcq_lr_schedule_step_skip(const mcq_lr_schedule* rule, int64_t* last_epoch, double* state, float* const* lr, const int32_t* skip,
                                         void* stream) {
    if (!rule || !last_epoch || !state || !lr || !mcq_lr_rule_ok(*rule)) return MCQ_EINVAL;
    if (skip) {
        hipLaunchKernelGGL(lr_schedule_skip_kernel, dim3(1), dim3(MCQ_LR_MAX_GROUPS), 0, (hipStream_t)stream, *rule, (long long*)last_epoch, state, lr,
                           (const int*)skip);
        return mcq_check_launch();
    }
    hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(MCQ_LR_MAX_GROUPS), 0, (hipStream_t)stream, *rule, (long long*)last_epoch, state, lr);
    return mcq_check_launch();
}

extern "C" int mcq_lr_schedule_step(const mcq_lr_schedule* rule, int64_t* last_epoch, double* state, float* const* lr, void* stream) {
    return mcq_lr_schedule_step_skip(rule, last_epoch, state, lr, nullptr, stream);
}

extern "C" int mcq_lr_schedule_host(const mcq_lr_schedule* rule, int32_t advance, int64_t* last_epoch, double* state, float* lr) {
    if (!rule || !last_epoch || !state || !mcq_lr_rule_ok(*rule)) return MCQ_EINVAL;
    if (!advance && rule->kind == MCQ_LR_MULTISTEP) return MCQ_EINVAL;
    const long long e = (long long)last_epoch[0] + (advance ? 1 : 0);
    last_epoch[0] = e;
    for (int g = 0; g < rule->ngroups; ++g) {
        double* s = state + (size_t)g * MCQ_LR_STATE_WORDS;
        if (advance) mcq_lr_step(*rule, e, s);
        else s[MCQ_LR_RATE] = mcq_lr_rate(*rule, e, s);
        if (lr) lr[g] = (float)s[MCQ_LR_RATE];
    }
    return MCQ_OK;
}
