// Test plug-in whose step never reports done: only the caller's forced limit (7 steps) ends its episodes.
#pragma once
#include "pgm_envplug.h"

struct pgm_user_env {
    static constexpr int O = 1, A = 1, K = 1, SD = 1, SI = 0, RW = 1, MAX_STEPS = 7;
    static constexpr bool DISCRETE = false;

    PGM_ENV_HD static void reset(double* sd, int32_t*, const double* u) { sd[0] = u[0]; }
    PGM_ENV_HD static void observe(const double* sd, const int32_t*, double* obs) { obs[0] = sd[0]; }
    PGM_ENV_HD static void step(double* sd, int32_t*, const float* action, double* obj, double* reward, int32_t*,
                                int32_t*) {
        sd[0] = sd[0] + 1.0;
        obj[0] = (double)action[0];
        *reward = sd[0];
    }
};
