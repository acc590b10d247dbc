// Test plug-in at every maximum: obs 32, 8 action dims, 3 objectives, 16 fp64 + 4 int32 state words, 8 uniforms per
// reset entry.  A bounded linear rule, no transcendental.
//   a_c = clip(a, -1, 1); s'[i] = 0.5 s[i] + 0.1 a_c[i mod 8]; t += 1; clipped += number of a outside [-1, 1]
//   obs = [s (16), s s (15), t / 16]... obs[16 + i] = s[i] s[i] for i < 15, obs[31] = t / 16
//   obj[k] = 1 + s'[k]; reward = obj0 + 0.25 clipped-this-step; a TRUE terminal when s'[0] + s'[1] > 0.3
//   reset: s[i] = (u[i mod 8] - 0.5) (i < 8 ? 1 : 0.5)
#pragma once
#include "pgm_envplug.h"

struct pgm_user_env {
    static constexpr int O = 32, A = 8, K = 3, SD = 16, SI = 4, RW = 8, MAX_STEPS = 16;
    static constexpr bool DISCRETE = false;

    PGM_ENV_HD static void reset(double* sd, int32_t* si, const double* u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma GCC unroll 16
        for (int i = 0; i < 16; ++i) {
            const double c = u[i % 8] - 0.5;
            sd[i] = i < 8 ? c : c * 0.5;
        }
        si[0] = si[1] = si[2] = si[3] = 0;
    }
    PGM_ENV_HD static void observe(const double* sd, const int32_t* si, double* obs) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma GCC unroll 16
        for (int i = 0; i < 16; ++i) obs[i] = sd[i];
#pragma GCC unroll 15
        for (int i = 0; i < 15; ++i) obs[16 + i] = sd[i] * sd[i];
        obs[31] = (double)si[0] / 16.0;
    }
    PGM_ENV_HD static void step(double* sd, int32_t* si, const float* action, double* obj, double* reward,
                                int32_t* done, int32_t* bad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        double ac[8];
        int32_t nclip = 0, mask = 0;
#pragma GCC unroll 8
        for (int j = 0; j < 8; ++j) {
            const double a = (double)action[j];
            ac[j] = a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a);
            const int32_t c = a < -1.0 || a > 1.0;
            nclip += c;
            mask |= c << j;
        }
#pragma GCC unroll 16
        for (int i = 0; i < 16; ++i) {
            const double h = 0.5 * sd[i], g = 0.1 * ac[i % 8];
            sd[i] = h + g;
        }
        si[0] += 1;
        si[1] += nclip;
        si[2] = mask;
        si[3] = si[0] * 2;
        obj[0] = 1.0 + sd[0];
        obj[1] = 1.0 + sd[1];
        obj[2] = 1.0 + sd[2];
        const double q = 0.25 * (double)nclip;
        *reward = obj[0] + q;
        const double s01 = sd[0] + sd[1];
        *done = s01 > 0.3;
        *bad = 0;
    }
};
