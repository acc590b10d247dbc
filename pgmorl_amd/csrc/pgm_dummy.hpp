// MO-Dummy-v0 / MO-Dummy3-v0: the transition of one env, written once for the host (pgm_dummy_transition, a sanitizer
// harness, any caller that wants to check the rule) and for the device kernels of pgm_dummy.hip.  Plain C++: no HIP
// header is needed to include it.  Reference (paths relative to the reference tree):
//   the env                         environments/dummy_mo_env.py:57-148
//   registration (max_steps 500)    environments/__init__.py:4-16
//   TimeLimitMask bad_transition    a2c_ppo_acktr/envs.py (TimeLimitMask)
//
//   state    pos[2], vel[2], total_distance, total_energy (fp64) and the integer step; the raw observation is those
//            six fp64 values in that order (the env's dtype is float64: nothing is rounded through fp32)
//   step     ac = clip((double)a, -1, 1); last = pos; vel = (vel + ac * 0.1) * 0.95; pos = pos + vel; step += 1
//            step_distance = sqrt(dx*dx + dy*dy), d = pos - last; step_energy = sqrt(ac0*ac0 + ac1*ac1); both
//            totals accumulate
//   obj      obj0 = step_distance, obj1 = 1 / (step_energy + 0.1), obj2 = bound - |pos| (K = 3 only)
//   reward   obj0 + 0.1 * obj1
//   end      done = step >= max_steps || |pos| > bound; bad = time_limit_is_bad && done && step == max_steps (the
//            limit step reports a time-limit end even when the env leaves the disc on that same step)
//   reset    a done env: vel, totals, step = 0, episode += 1, pos = resets[episode mod R] (the env's row of
//            envspec.dummy_reset_table: a restatement of the reference's unseeded np.random.uniform(-1, 1, 2))
//
// The same bits on the host and on gfx950: every operation below is one correctly rounded fp64 add, multiply, divide
// or sqrt, and the compiler may not contract a*b + c into an fma (the pragma for clang, which compiles both sides of
// the library; a GCC build of a harness passes -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PGM_DUMMY_HD __host__ __device__
#else
#define PGM_DUMMY_HD
#endif

namespace pgm {

constexpr int DUMMY_OBS = 6, DUMMY_ACT = 2, DUMMY_KMAX = 3;

struct DummyEnv {
    double pos[2], vel[2], dist, energy;
    int32_t step, episode;  // episode: this env's resets since env_reset()
};

struct DummyOut {  // the terminal step's on a done env (the state is then already the next episode's first)
    double obj[DUMMY_KMAX];
    double reward;
    int32_t done, bad;
};

PGM_DUMMY_HD inline void dummy_observe(const DummyEnv& s, double* obs) {
    obs[0] = s.pos[0];
    obs[1] = s.pos[1];
    obs[2] = s.vel[0];
    obs[3] = s.vel[1];
    obs[4] = s.dist;
    obs[5] = s.energy;
}

PGM_DUMMY_HD inline double dummy_clip1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

// resets: this env's row [R][2] of the reset table
PGM_DUMMY_HD inline DummyOut dummy_transition(int max_steps, int time_limit_is_bad, double bound, int K,
                                              const double* resets, int R, DummyEnv& s, float a0, float a1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ac0 = dummy_clip1((double)a0), ac1 = dummy_clip1((double)a1);
    const double lx = s.pos[0], ly = s.pos[1];
    const double t0 = ac0 * 0.1, t1 = ac1 * 0.1;
    const double v0 = s.vel[0] + t0, v1 = s.vel[1] + t1;
    s.vel[0] = v0 * 0.95;
    s.vel[1] = v1 * 0.95;
    s.pos[0] = lx + s.vel[0];
    s.pos[1] = ly + s.vel[1];
    s.step += 1;
    const double dx = s.pos[0] - lx, dy = s.pos[1] - ly;
    const double dxx = dx * dx, dyy = dy * dy;
    const double step_distance = sqrt(dxx + dyy);
    const double e0 = ac0 * ac0, e1 = ac1 * ac1;
    const double step_energy = sqrt(e0 + e1);
    s.dist = s.dist + step_distance;
    s.energy = s.energy + step_energy;
    const double pxx = s.pos[0] * s.pos[0], pyy = s.pos[1] * s.pos[1];
    const double r = sqrt(pxx + pyy);
    DummyOut o;
    o.obj[0] = step_distance;
    o.obj[1] = 1.0 / (step_energy + 0.1);
    o.obj[2] = K >= 3 ? bound - r : 0.0;
    const double tenth = 0.1 * o.obj[1];
    o.reward = o.obj[0] + tenth;
    o.done = s.step >= max_steps || r > bound;
    o.bad = time_limit_is_bad && o.done && s.step == max_steps;
    if (o.done) {
        s.episode += 1;
        const double* rp = resets + 2 * (size_t)(s.episode % R);
        s.pos[0] = rp[0];
        s.pos[1] = rp[1];
        s.vel[0] = s.vel[1] = s.dist = s.energy = 0.0;
        s.step = 0;
    }
    return o;
}

}  // namespace pgm
