// Test plug-in: tests/envplug/line.hpp restated under contract 2 with no parameter and no uniform (NP = NW = 0).  The
// same rule, so the same numbers as line.hpp through every entry point.
//   v' = 0.9 v + 0.2 clip(a, -1, 1); x' = x + v'; t += 1
//   obs = [x, v, x x, v v, t / 40]; obj = [1 + v', 1 - a_c a_c]; reward = obj0 + 0.5 obj1
//   a TRUE terminal when |x'| > 1.5; the time limit (40 steps) is the caller's forced limit
//   reset: x = u0 - 0.5, v = (u1 - 0.5) 0.2
#pragma once
#include "pgm_envplug.h"

struct pgm_user_env {
    static constexpr int CONTRACT = 2, NP = 0, NW = 0;
    static constexpr int O = 5, A = 1, K = 2, SD = 2, SI = 1, RW = 2, MAX_STEPS = 40;
    static constexpr bool DISCRETE = false;

    PGM_ENV_HD static void reset(double* sd, int32_t* si, const double* u, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        sd[0] = u[0] - 0.5;
        const double h = u[1] - 0.5;
        sd[1] = h * 0.2;
        si[0] = 0;
    }
    PGM_ENV_HD static void observe(const double* sd, const int32_t* si, double* obs, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        obs[0] = sd[0];
        obs[1] = sd[1];
        obs[2] = sd[0] * sd[0];
        obs[3] = sd[1] * sd[1];
        obs[4] = (double)si[0] / 40.0;
    }
    PGM_ENV_HD static void step(double* sd, int32_t* si, const float* action, double* obj, double* reward,
                                int32_t* done, int32_t* bad, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double a = (double)action[0];
        const double ac = a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a);
        const double dv = 0.9 * sd[1], da = 0.2 * ac;
        sd[1] = dv + da;
        sd[0] = sd[0] + sd[1];
        si[0] += 1;
        const double a2 = ac * ac;
        obj[0] = 1.0 + sd[1];
        obj[1] = 1.0 - a2;
        const double half = 0.5 * obj[1];
        *reward = obj[0] + half;
        const double ax = sd[0] < 0.0 ? -sd[0] : sd[0];
        *done = ax > 1.5;
        *bad = 0;
    }
};
