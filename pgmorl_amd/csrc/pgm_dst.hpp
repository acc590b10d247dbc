// Deep Sea Treasure: the transition of one env, written once for the host (pgm_dst_transition, a sanitizer harness,
// any caller that wants to check the rule) and for the device kernels of pgm_dst.hip.  It restates
// pgmorl_amd/hostenv.py DeepSeaTreasureHostVecEnv, the project's statement of the reference's
// environments/deep_sea_treasure.py:111-183.  Plain C++: no HIP header is needed to include it.
//
//   grid     11 x 11; cell (r, c) is open if r == 0 or r <= c, or if it is a treasure cell: (1,0) = 1, (2,1) = 3,
//            (4,3) = 8, (7,6) = 20
//   moves    0 up, 1 down, 2 left, 3 right (any other index acts as 0); off the grid or into a wall: stay
//   reward   step += 1; on a treasure cell reward = obj0 = its value and obj1 = 10 / (step + 1), else all 0
//   end      done = found || step >= max_steps; bad = time_limit_is_bad && limit && !found
//   reset    a done env returns to (0, 0, 0): row / col / step and the observation are the next episode's first
//   obs      [r / 10, c / 10, step / max_steps], each rounded to fp32 (the env's dtype) and widened
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PGM_DST_HD __host__ __device__
#else
#define PGM_DST_HD
#endif

namespace pgm {

constexpr int DST_SIZE = 11;

struct DstStep {
    int32_t row, col, step;  // after the auto-reset
    double obs[3];           // raw observation of (row, col, step)
    double obj[2];
    double reward;
    int32_t done, bad;
};

PGM_DST_HD inline double dst_value(int r, int c) {
    return (r == 1 && c == 0) ? 1.0 : (r == 2 && c == 1) ? 3.0 : (r == 4 && c == 3) ? 8.0 : (r == 7 && c == 6) ? 20.0 : 0.0;
}
PGM_DST_HD inline bool dst_open(int r, int c) { return r == 0 || r <= c || dst_value(r, c) > 0.0; }

PGM_DST_HD inline void dst_observe(int r, int c, int step, int max_steps, double* obs) {
    obs[0] = (double)(float)((double)r / (double)(DST_SIZE - 1));
    obs[1] = (double)(float)((double)c / (double)(DST_SIZE - 1));
    obs[2] = (double)(float)((double)step / (double)max_steps);
}

PGM_DST_HD inline DstStep dst_transition(int max_steps, int time_limit_is_bad, int r, int c, int step, int action) {
    const int a = (action >= 0 && action < 4) ? action : 0;
    const int nr = r + (a == 1) - (a == 0), nc = c + (a == 3) - (a == 2);
    if (nr >= 0 && nr < DST_SIZE && nc >= 0 && nc < DST_SIZE && dst_open(nr, nc)) {
        r = nr;
        c = nc;
    }
    step += 1;
    const double v = dst_value(r, c);
    const bool found = v > 0.0, limit = step >= max_steps;
    DstStep o;
    o.reward = v;
    o.obj[0] = v;
    o.obj[1] = found ? 10.0 / (double)(step + 1) : 0.0;
    o.done = found || limit;
    o.bad = time_limit_is_bad && limit && !found;
    o.row = o.done ? 0 : r;
    o.col = o.done ? 0 : c;
    o.step = o.done ? 0 : step;
    dst_observe(o.row, o.col, o.step, max_steps, o.obs);
    return o;
}

}  // namespace pgm
