// Stand-alone host build of the schedule rule (mcquic_amd/csrc/schedule_rule.h) for tests/test_schedule_host.py: no HIP, no library.
//   schedule_host_main kind mode ngroups gamma first_milestone total_size step_ratio warmup_steps cycle_mult last_epoch steps
//                      nmilestones [milestone ...] state[ngroups * 8]
// Numbers are parsed with strtod / strtoll (doubles may be hex floats); prints one line per step: last_epoch, then every group's
// rate as a hex float and its float32 rounding.  This is also the program to build with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../mcquic_amd/csrc/schedule_rule.h"

int main(int argc, char** argv) {
    if (argc < 13) return 2;
    int a = 1;
    mcq_lr_schedule r;
    r.kind = atoi(argv[a++]);
    r.mode = atoi(argv[a++]);
    r.ngroups = atoi(argv[a++]);
    r.gamma = strtod(argv[a++], nullptr);
    r.first_milestone = strtod(argv[a++], nullptr);
    r.total_size = strtod(argv[a++], nullptr);
    r.step_ratio = strtod(argv[a++], nullptr);
    r.warmup_steps = strtod(argv[a++], nullptr);
    r.cycle_mult = strtod(argv[a++], nullptr);
    long long e = strtoll(argv[a++], nullptr, 10);
    const int steps = atoi(argv[a++]);
    r.nmilestones = atoi(argv[a++]);
    if (r.nmilestones < 0 || r.ngroups < 1 || r.ngroups > MCQ_LR_MAX_GROUPS || argc != a + r.nmilestones + r.ngroups * MCQ_LR_STATE_WORDS) return 2;
    std::vector<int64_t> milestones((size_t)r.nmilestones);
    for (auto& m : milestones) m = strtoll(argv[a++], nullptr, 10);
    r.milestones = milestones.empty() ? nullptr : milestones.data();
    std::vector<double> state((size_t)r.ngroups * MCQ_LR_STATE_WORDS);
    for (auto& v : state) v = strtod(argv[a++], nullptr);
    if (!mcq_lr_rule_ok(r)) return 3;
    for (int i = 0; i < steps; ++i) {
        e += 1;
        printf("%lld", e);
        for (int g = 0; g < r.ngroups; ++g) {
            double* s = state.data() + (size_t)g * MCQ_LR_STATE_WORDS;
            mcq_lr_step(r, e, s);
            printf(" %a %a", s[MCQ_LR_RATE], (double)(float)s[MCQ_LR_RATE]);
        }
        printf("\n");
    }
    return 0;
}
