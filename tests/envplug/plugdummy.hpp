// Test plug-in: MO-Dummy-v0 (obs 6, 2 action dims, 2 objectives) as a plug-in, wrapping dummy_transition of
// pgm_dummy.hpp: bound 5, 500 steps, reset position 2 u - 1.  The fused plug-in kernels must equal pgm_rollout_dummy /
// pgm_eval_dummy in every stored field.
#pragma once
#include "pgm_envplug.h"
#include "../../pgmorl_amd/csrc/pgm_dummy.hpp"

struct pgm_user_env {
    static constexpr int O = 6, A = 2, K = 2, SD = 6, SI = 1, RW = 2, MAX_STEPS = 500;
    static constexpr bool DISCRETE = false;

    PGM_ENV_HD static void reset(double* sd, int32_t* si, const double* u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double t0 = 2.0 * u[0], t1 = 2.0 * u[1];
        sd[0] = t0 - 1.0;
        sd[1] = t1 - 1.0;
        sd[2] = sd[3] = sd[4] = sd[5] = 0.0;
        si[0] = 0;
    }
    PGM_ENV_HD static void observe(const double* sd, const int32_t*, double* obs) {
        for (int i = 0; i < 6; ++i) obs[i] = sd[i];
    }
    PGM_ENV_HD static void step(double* sd, int32_t* si, const float* action, double* obj, double* reward,
                                int32_t* done, int32_t* bad) {
        pgm::DummyEnv s{{sd[0], sd[1]}, {sd[2], sd[3]}, sd[4], sd[5], si[0], 0};
        const double none[2] = {0.0, 0.0};  // the caller resets: dummy_transition's own reset is overwritten
        const pgm::DummyOut o = pgm::dummy_transition(MAX_STEPS, 1, 5.0, K, none, 1, s, action[0], action[1]);
        if (!o.done) {
            pgm::dummy_observe(s, sd);
            si[0] = s.step;
        }
        obj[0] = o.obj[0];
        obj[1] = o.obj[1];
        *reward = o.reward;
        *done = o.done;
        *bad = o.bad;
    }
};
