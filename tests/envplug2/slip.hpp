// Test plug-in under contract 2: a point on a line whose action slips.  obs 3, 1 action dim, 2 objectives, Gaussian
// head, 2 runtime parameters (slip, wind), 1 uniform per step.  No transcendental.
//   a_c = clip(a, -1, 1); the action is ignored (a_e = 0) when w0 < slip, else a_e = a_c
//   m = 0.3 a_e + wind; x' = x + m
//   obs = [x, m, x x]; obj = [1 + m, 1 - a_c a_c]; reward = obj0 + 0.5 obj1
//   a TRUE terminal when |x'| > 1; the time limit (12 steps) is the caller's forced limit
//   reset: x = (u0 - 0.5) 0.5, m = 0
#pragma once
#include "pgm_envplug.h"

struct pgm_user_env {
    static constexpr int CONTRACT = 2, NP = 2, NW = 1;
    static constexpr double PAR_DEFAULT[NP] = {0.2, 0.05};
    static constexpr const char* PAR_NAMES = "slip,wind";
    static constexpr int O = 3, A = 1, K = 2, SD = 2, SI = 0, RW = 1, MAX_STEPS = 12;
    static constexpr bool DISCRETE = false;

    PGM_ENV_HD static void reset(double* sd, int32_t*, const double* u, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double h = u[0] - 0.5;
        sd[0] = h * 0.5;
        sd[1] = 0.0;
    }
    PGM_ENV_HD static void observe(const double* sd, const int32_t*, double* obs, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        obs[0] = sd[0];
        obs[1] = sd[1];
        obs[2] = sd[0] * sd[0];
    }
    PGM_ENV_HD static void step(double* sd, int32_t*, const float* action, double* obj, double* reward, int32_t* done,
                                int32_t* bad, const pgm_env_ctx& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double a = (double)action[0];
        const double ac = a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a);
        const double ae = c.w[0] < c.par[0] ? 0.0 : ac;
        const double push = 0.3 * ae;
        const double m = push + c.par[1];
        sd[0] = sd[0] + m;
        sd[1] = m;
        const double a2 = ac * ac;
        obj[0] = 1.0 + m;
        obj[1] = 1.0 - a2;
        const double half = 0.5 * obj[1];
        *reward = obj[0] + half;
        const double ax = sd[0] < 0.0 ? -sd[0] : sd[0];
        *done = ax > 1.0;
        *bad = 0;
    }
};
