// Measurement plug-in: tests/envplug/plugdummy.hpp (MO-Dummy-v0 as a plug-in) under contract 2 with 2 runtime
// parameters and 1 uniform per step.  The word scales a small disturbance of the action before dummy_transition:
//   a0' = a0 + gust (w0 - 0.5); a1' = a1 + lift
// With gust = lift = 0 (the defaults) the rule is plugdummy.hpp's.  scripts/envplug2_rollout.py times it against the
// contract-1 form in one session: what the parameters, the hash and the ctx cost in the fused rollout.
#pragma once
#include "pgm_envplug.h"
#include "../../pgmorl_amd/csrc/pgm_dummy.hpp"

struct pgm_user_env {
    static constexpr int CONTRACT = 2, NP = 2, NW = 1;
    static constexpr double PAR_DEFAULT[NP] = {0.0, 0.0};
    static constexpr const char* PAR_NAMES = "gust,lift";
    static constexpr int O = 6, A = 2, K = 2, SD = 6, SI = 1, RW = 2, MAX_STEPS = 500;
    static constexpr bool DISCRETE = false;

    PGM_ENV_HD static void reset(double* sd, int32_t* si, const double* u, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double t0 = 2.0 * u[0], t1 = 2.0 * u[1];
        sd[0] = t0 - 1.0;
        sd[1] = t1 - 1.0;
        sd[2] = sd[3] = sd[4] = sd[5] = 0.0;
        si[0] = 0;
    }
    PGM_ENV_HD static void observe(const double* sd, const int32_t*, double* obs, const pgm_env_ctx&) {
        for (int i = 0; i < 6; ++i) obs[i] = sd[i];
    }
    PGM_ENV_HD static void step(double* sd, int32_t* si, const float* action, double* obj, double* reward,
                                int32_t* done, int32_t* bad, const pgm_env_ctx& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double h = c.w[0] - 0.5;
        const double g = c.par[0] * h;
        const float a0 = (float)((double)action[0] + g), a1 = (float)((double)action[1] + c.par[1]);
        pgm::DummyEnv s{{sd[0], sd[1]}, {sd[2], sd[3]}, sd[4], sd[5], si[0], 0};
        const double none[2] = {0.0, 0.0};  // the caller resets: dummy_transition's own reset is overwritten
        const pgm::DummyOut o = pgm::dummy_transition(MAX_STEPS, 1, 5.0, K, none, 1, s, a0, a1);
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
