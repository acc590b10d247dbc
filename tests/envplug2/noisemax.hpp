// Test plug-in under contract 2: the most uniforms per step (NW = 4), no runtime parameter.  obs 2, 1 action dim, 2
// objectives, Gaussian head.  No transcendental.
//   a_c = clip(a, -1, 1); x' = (x + 0.2 a_c) + 0.3 (w0 - 0.5)
//   obj0 = 1 + w1 a_c; obj1 = w2 - w3; reward = obj0 + obj1
//   a TRUE terminal when |x'| > 0.6; the time limit is 8 steps
//   obs = [x, x x]; reset: x = (u0 - 0.5) 0.4
#pragma once
#include "pgm_envplug.h"

struct pgm_user_env {
    static constexpr int CONTRACT = 2, NP = 0, NW = 4;
    static constexpr int O = 2, A = 1, K = 2, SD = 1, SI = 0, RW = 1, MAX_STEPS = 8;
    static constexpr bool DISCRETE = false;

    PGM_ENV_HD static void reset(double* sd, int32_t*, const double* u, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double h = u[0] - 0.5;
        sd[0] = h * 0.4;
    }
    PGM_ENV_HD static void observe(const double* sd, const int32_t*, double* obs, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        obs[0] = sd[0];
        obs[1] = sd[0] * sd[0];
    }
    PGM_ENV_HD static void step(double* sd, int32_t*, const float* action, double* obj, double* reward, int32_t* done,
                                int32_t* bad, const pgm_env_ctx& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double a = (double)action[0];
        const double ac = a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a);
        const double push = 0.2 * ac;
        const double h = c.w[0] - 0.5;
        const double gust = 0.3 * h;
        sd[0] = (sd[0] + push) + gust;
        const double wa = c.w[1] * ac;
        obj[0] = 1.0 + wa;
        obj[1] = c.w[2] - c.w[3];
        *reward = obj[0] + obj[1];
        const double ax = sd[0] < 0.0 ? -sd[0] : sd[0];
        *done = ax > 0.6;
        *bad = 0;
    }
};
