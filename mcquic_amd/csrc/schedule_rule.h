// The learning-rate schedules of mcquic/train/lrSchedulers.py as ONE rule on eight doubles per parameter group, written once for
// the device (csrc/schedule.hip, one lane per group) and for the host (mcq_lr_schedule_host; a plain C++ compiler takes this file
// too: tests/test_schedule_host.py builds it with a main of its own).  Every expression keeps the reference's order of operations
// -- Python evaluates left to right in float64, and so does this with -ffp-contract=off -- so the branches without cos / pow are
// the reference's bits, and the others differ from it only by what the two libms differ by.  State layout: include/mcquic_hip.h.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/mcquic_hip.h"

#if defined(__HIPCC__)
#define MCQ_LR_HD __host__ __device__
#else
#define MCQ_LR_HD
#endif

enum { MCQ_LR_RATE = 0, MCQ_LR_CYCLE = 1, MCQ_LR_STEP_IN_CYCLE = 2, MCQ_LR_CYCLE_STEPS = 3, MCQ_LR_MAX = 4, MCQ_LR_MIN = 5, MCQ_LR_BASE = 6,
       MCQ_LR_MIN_BASE = 7 };

// x ** n as the reference computes it (CPython's float ** int is the host libm's pow, which returns an exactly representable result
// exactly: 0.5 ** 4 is 0.0625).  The device's pow does not (0.5 ** 4 came out one ulp low on gfx950), and `gamma ** cycle` scales a
// whole cycle's bounds, warm-up ramp included.  So for the exponents the schedules use -- non-negative integers -- the device squares and
// multiplies in double-double (error-free products through fma): exact where the result is representable, and correctly rounded but
// for ties beyond 2^-100 otherwise.  Anything else, and results outside the range where the products stay error-free, go to pow.
MCQ_LR_HD inline void mcq_lr_dd_mul(double& ah, double& al, double bh, double bl) {
    const double p = ah * bh;
    const double e = __builtin_fma(ah, bh, -p) + (ah * bl + al * bh);
    ah = p + e;
    al = e - (ah - p);
}
MCQ_LR_HD inline double mcq_lr_pow(double x, double n) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (n >= 0.0 && n == trunc(n) && n < 9007199254740992.0) {
        double rh = 1.0, rl = 0.0, bh = x, bl = 0.0;
        for (unsigned long long k = (unsigned long long)n; k;) {
            if (k & 1) mcq_lr_dd_mul(rh, rl, bh, bl);
            k >>= 1;
            if (k) mcq_lr_dd_mul(bh, bl, bh, bl);
        }
        const double r = rh + rl;
        if (fabs(r) >= 1e-290 && fabs(r) <= 1e290) return r;
    }
#endif
    return pow(x, n);
}

// What the entry points check before anything is read (pointers apart).
MCQ_LR_HD inline bool mcq_lr_rule_ok(const mcq_lr_schedule& r) {
    if (r.ngroups < 1 || r.ngroups > MCQ_LR_MAX_GROUPS) return false;
    switch (r.kind) {
        case MCQ_LR_PLACEHOLDER: return true;
        case MCQ_LR_MULTISTEP:   return r.nmilestones >= 1 && r.milestones && r.first_milestone >= 1.0 && r.gamma == r.gamma;
        case MCQ_LR_CYCLIC:      return r.mode >= MCQ_LR_TRIANGULAR && r.mode <= MCQ_LR_EXP_RANGE && r.total_size > 0.0 && r.step_ratio > 0.0 &&
                                        r.step_ratio <= 1.0 && r.gamma == r.gamma;
        case MCQ_LR_COSINE:      return r.warmup_steps >= 0.0 && r.warmup_steps == trunc(r.warmup_steps) && r.cycle_mult > 0.0 && r.gamma == r.gamma;
        default:                 return false;
    }
}

// Cosine, `step(None)` (lrSchedulers.py:455-464): the cycle counters move, and the bounds with them when a cycle ends.
MCQ_LR_HD inline void mcq_lr_advance(const mcq_lr_schedule& r, double* s) {
    if (r.kind != MCQ_LR_COSINE) return;
    s[MCQ_LR_STEP_IN_CYCLE] = s[MCQ_LR_STEP_IN_CYCLE] + 1.0;
    if (s[MCQ_LR_STEP_IN_CYCLE] >= s[MCQ_LR_CYCLE_STEPS]) {
        s[MCQ_LR_CYCLE] += 1.0;
        s[MCQ_LR_STEP_IN_CYCLE] = s[MCQ_LR_STEP_IN_CYCLE] - s[MCQ_LR_CYCLE_STEPS];
        s[MCQ_LR_CYCLE_STEPS] = trunc((s[MCQ_LR_CYCLE_STEPS] - r.warmup_steps) * r.cycle_mult) + r.warmup_steps;     // int(...) + warm
        const double g = mcq_lr_pow(r.gamma, s[MCQ_LR_CYCLE]);                                                              // gamma ** cycle
        s[MCQ_LR_MAX] = s[MCQ_LR_BASE] * g;
        s[MCQ_LR_MIN] = s[MCQ_LR_MIN_BASE] * g;
    }
}

// `get_lr()` at last_epoch == e, from the state as it stands; MultiStep reads the rate it is about to replace.
MCQ_LR_HD inline double mcq_lr_rate(const mcq_lr_schedule& r, long long e, double* s) {
    const double ed = (double)e;
    switch (r.kind) {
        case MCQ_LR_MULTISTEP: {
            if (ed <= r.first_milestone) return s[MCQ_LR_BASE] * (double)(e + 1) / r.first_milestone;    // (e == first: (first + 1) / first)
            for (int i = 0; i < r.nmilestones; ++i)
                if (r.milestones[i] == e) return s[MCQ_LR_RATE] * r.gamma;
            return s[MCQ_LR_RATE];
        }
        case MCQ_LR_CYCLIC: {
            const double cycle = floor(1.0 + ed / r.total_size);
            const double x = 1.0 + ed / r.total_size - cycle;
            const double scale = x <= r.step_ratio ? x / r.step_ratio : (x - 1.0) / (r.step_ratio - 1.0);
            const double height = (s[MCQ_LR_MAX] - s[MCQ_LR_BASE]) * scale;
            s[MCQ_LR_CYCLE] = cycle;
            double f = 1.0;
            if (r.mode == MCQ_LR_TRIANGULAR2) f = ldexp(1.0, -(int)(cycle - 1.0));      // 1 / 2. ** (cycle - 1): a power of two either way
            else if (r.mode == MCQ_LR_EXP_RANGE) f = mcq_lr_pow(r.gamma, ed);                   // gamma ** last_epoch
            return s[MCQ_LR_BASE] + height * f;
        }
        case MCQ_LR_COSINE: {
            const double sic = s[MCQ_LR_STEP_IN_CYCLE], lo = s[MCQ_LR_MIN], hi = s[MCQ_LR_MAX], warm = r.warmup_steps;
            if (sic == -1.0) return lo;
            if (sic < warm) return (hi - lo) * sic / warm + lo;
            return lo + (hi - lo) * (1.0 + cos(3.141592653589793 * (sic - warm) / (s[MCQ_LR_CYCLE_STEPS] - warm))) / 2.0;
        }
        default: return s[MCQ_LR_BASE];
    }
}

// One `scheduler.step()` of one group at the NEW last_epoch e.
MCQ_LR_HD inline void mcq_lr_step(const mcq_lr_schedule& r, long long e, double* s) {
    mcq_lr_advance(r, s);
    s[MCQ_LR_RATE] = mcq_lr_rate(r, e, s);
}
