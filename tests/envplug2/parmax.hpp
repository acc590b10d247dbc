// Test plug-in under contract 2: the most runtime parameters (NP = 16), no uniforms.  obs 2, 1 action dim, 3
// objectives, Gaussian head.  Every parameter enters an objective of the step.  No transcendental.
//   a_c = clip(a, -1, 1); x' = (p0 x + p1 a_c) + p2
//   obj0 = ((p3 x' + p4 a_c) + p5) + p6 x' x'
//   obj1 = ((p7 x' + p8 a_c) + p9) + p10 a_c a_c
//   obj2 = (((p11 x' + p12 a_c) + p13) + p14 x' x') + p15
//   reward = obj0 + 0.5 obj1; a TRUE terminal when |x'| > 2; the time limit is 6 steps
//   obs = [x, x x]; reset: x = u0 - 0.5
#pragma once
#include "pgm_envplug.h"

struct pgm_user_env {
    static constexpr int CONTRACT = 2, NP = 16, NW = 0;
    static constexpr double PAR_DEFAULT[NP] = {0.9,  0.5, 0.1,  1.0, 0.25, 0.5,   -0.125, 0.75,
                                               -0.5, 1.0, -1.0, 0.5, 0.5,  0.125, 0.25,   -0.25};
    static constexpr const char* PAR_NAMES = "p0,p1,p2,p3,p4,p5,p6,p7,p8,p9,p10,p11,p12,p13,p14,p15";
    static constexpr int O = 2, A = 1, K = 3, SD = 1, SI = 0, RW = 1, MAX_STEPS = 6;
    static constexpr bool DISCRETE = false;

    PGM_ENV_HD static void reset(double* sd, int32_t*, const double* u, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        sd[0] = u[0] - 0.5;
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
        const double* p = c.par;
        const double a = (double)action[0];
        const double ac = a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a);
        const double t0 = p[0] * sd[0], t1 = p[1] * ac;
        const double x = (t0 + t1) + p[2];
        const double xx = x * x, aa = ac * ac;
        const double u0 = p[3] * x, u1 = p[4] * ac, u2 = p[6] * xx;
        obj[0] = ((u0 + u1) + p[5]) + u2;
        const double v0 = p[7] * x, v1 = p[8] * ac, v2 = p[10] * aa;
        obj[1] = ((v0 + v1) + p[9]) + v2;
        const double z0 = p[11] * x, z1 = p[12] * ac, z2 = p[14] * xx;
        obj[2] = (((z0 + z1) + p[13]) + z2) + p[15];
        const double half = 0.5 * obj[1];
        *reward = obj[0] + half;
        sd[0] = x;
        const double ax = x < 0.0 ? -x : x;
        *done = ax > 2.0;
        *bad = 0;
    }
};
