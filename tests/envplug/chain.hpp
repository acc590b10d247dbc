// Test plug-in: a chain of 7 cells.  obs 2, 3 actions (left, stay, right), 3 objectives, Categorical head.  No fp64
// state word at all (SD = 0): the cell and the step count are int32.
//   i += a - 1; t += 1; obs = [i / 6, t / 20]; obj = [i / 6, (6 - i) / 6, 1 if stay else 0]
//   reward = (obj0 + obj1) + obj2; a TRUE terminal at either end; the time limit (20 steps) is the forced limit
//   reset: i = 2 + floor(3 u) (cells 2, 3, 4)
#pragma once
#include "pgm_envplug.h"

struct pgm_user_env {
    static constexpr int O = 2, A = 3, K = 3, SD = 0, SI = 2, RW = 1, MAX_STEPS = 20;
    static constexpr bool DISCRETE = true;

    PGM_ENV_HD static void reset(double*, int32_t* si, const double* u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double c = u[0] * 3.0;
        si[0] = 2 + (int32_t)c;
        si[1] = 0;
    }
    PGM_ENV_HD static void observe(const double*, const int32_t* si, double* obs) {
        obs[0] = (double)si[0] / 6.0;
        obs[1] = (double)si[1] / 20.0;
    }
    PGM_ENV_HD static void step(double*, int32_t* si, int action, double* obj, double* reward, int32_t* done,
                                int32_t* bad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        si[0] += action - 1;
        si[1] += 1;
        obj[0] = (double)si[0] / 6.0;
        obj[1] = (double)(6 - si[0]) / 6.0;
        obj[2] = action == 1 ? 1.0 : 0.0;
        const double s01 = obj[0] + obj[1];
        *reward = s01 + obj[2];
        *done = si[0] <= 0 || si[0] >= 6;
        *bad = 0;
    }
};
