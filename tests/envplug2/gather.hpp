// Test plug-in under contract 2: a small Resource-Gathering-like grid.  obs 4, 4 actions (Categorical head), 3
// objectives, 1 runtime parameter (p_attack), 3 uniforms per step of which a step uses one, two or none.
//   a 3 x 3 grid, home (0, 0), gold at (2, 0), a gem at (2, 2), enemies at (1, 0) and (1, 1)
//   si = [x, y, carried: bit 0 gold, bit 1 gem]; actions 0 right, 1 left, 2 up, 3 down, clipped to the grid
//   entering an enemy cell: attacked when w0 < p_attack -- obj0 = -1, a TRUE terminal
//   entering the gold cell without gold: picked up when w1 < 0.9; the gem cell without the gem: when w2 < 0.8
//   entering home with anything carried: obj1 = gold, obj2 = gem, a TRUE terminal
//   obj0 = -0.05 on every step without an attack; reward = obj0 + obj1 + obj2
//   obs = [x / 2, y / 2, gold, gem]; the time limit (10 steps) is the caller's forced limit
//   reset: x = 0 or 1 (u0 < 0.5: 0), y = 0, nothing carried
#pragma once
#include "pgm_envplug.h"

struct pgm_user_env {
    static constexpr int CONTRACT = 2, NP = 1, NW = 3;
    static constexpr double PAR_DEFAULT[NP] = {0.1};
    static constexpr const char* PAR_NAMES = "p_attack";
    static constexpr int O = 4, A = 4, K = 3, SD = 0, SI = 3, RW = 1, MAX_STEPS = 10;
    static constexpr bool DISCRETE = true;

    PGM_ENV_HD static void reset(double*, int32_t* si, const double* u, const pgm_env_ctx&) {
        si[0] = u[0] < 0.5 ? 0 : 1;
        si[1] = 0;
        si[2] = 0;
    }
    PGM_ENV_HD static void observe(const double*, const int32_t* si, double* obs, const pgm_env_ctx&) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        obs[0] = (double)si[0] / 2.0;
        obs[1] = (double)si[1] / 2.0;
        obs[2] = (double)(si[2] & 1);
        obs[3] = (double)((si[2] >> 1) & 1);
    }
    PGM_ENV_HD static void step(double*, int32_t* si, int action, double* obj, double* reward, int32_t* done,
                                int32_t* bad, const pgm_env_ctx& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        int x = si[0] + (action == 0) - (action == 1), y = si[1] + (action == 2) - (action == 3);
        x = x < 0 ? 0 : (x > 2 ? 2 : x);
        y = y < 0 ? 0 : (y > 2 ? 2 : y);
        const bool moved = x != si[0] || y != si[1];
        int carried = si[2];
        obj[0] = -0.05;
        obj[1] = 0.0;
        obj[2] = 0.0;
        *done = 0;
        if (moved && x == 1 && y <= 1) {
            if (c.w[0] < c.par[0]) {
                obj[0] = -1.0;
                *done = 1;
            }
        } else if (moved && x == 2 && y == 0) {
            if (!(carried & 1) && c.w[1] < 0.9) carried |= 1;
        } else if (moved && x == 2 && y == 2) {
            if (!(carried & 2) && c.w[2] < 0.8) carried |= 2;
        } else if (moved && x == 0 && y == 0 && carried != 0) {
            obj[1] = (double)(carried & 1);
            obj[2] = (double)((carried >> 1) & 1);
            *done = 1;
        }
        si[0] = x;
        si[1] = y;
        si[2] = carried;
        const double s01 = obj[0] + obj[1];
        *reward = s01 + obj[2];
        *bad = 0;
    }
};
