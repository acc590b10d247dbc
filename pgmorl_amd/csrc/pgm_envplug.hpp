// Device env plug-ins (include/pgm_envplug.h): the checks of a user env header and the transition around its three
// functions -- the forced step limit and the auto-reset -- written once for the host (pgm_envplug_transition, a
// sanitizer harness) and for the kernels of pgm_envplug.hip.  Plain C++: no HIP header is needed to include it.  The
// env header (which defines pgm_user_env) is included before this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/pgm_envplug.h"

namespace pgm {
namespace envplug {

// ---- a header that misses a member fails with a message naming it
#define PGM_ENVPLUG_HAS(member)                                                    \
    template <class E, class = void>                                               \
    struct has_##member : std::false_type {};                                      \
    template <class E>                                                             \
    struct has_##member<E, std::void_t<decltype(&E::member)>> : std::true_type {}; \
    static_assert(has_##member<pgm_user_env>::value, "env plug-in: pgm_user_env::" #member " is missing");
PGM_ENVPLUG_HAS(O)
PGM_ENVPLUG_HAS(A)
PGM_ENVPLUG_HAS(K)
PGM_ENVPLUG_HAS(DISCRETE)
PGM_ENVPLUG_HAS(SD)
PGM_ENVPLUG_HAS(SI)
PGM_ENVPLUG_HAS(RW)
PGM_ENVPLUG_HAS(MAX_STEPS)
PGM_ENVPLUG_HAS(reset)
PGM_ENVPLUG_HAS(observe)
PGM_ENVPLUG_HAS(step)
#undef PGM_ENVPLUG_HAS

// ---- ... and one that breaks a range with a message naming the limit (the compiler adds the value)
template <class E>
struct Checked {
    static_assert(E::O >= 1 && E::O <= PGM_ENVPLUG_MAX_OBS, "env plug-in: pgm_user_env::O outside 1 <= O <= 32");
    static_assert(E::A <= PGM_ENVPLUG_MAX_ACT, "env plug-in: pgm_user_env::A above the limit A <= 8");
    static_assert(E::A >= (E::DISCRETE ? 2 : 1),
                  "env plug-in: pgm_user_env::A below the limit A >= 1 (DISCRETE, a Categorical head: A >= 2 actions)");
    static_assert(E::K >= 1 && E::K <= PGM_ENVPLUG_MAX_OBJ, "env plug-in: pgm_user_env::K outside 1 <= K <= 3");
    static_assert(E::SD >= 0 && E::SD <= PGM_ENVPLUG_MAX_SD, "env plug-in: pgm_user_env::SD outside 0 <= SD <= 16");
    static_assert(E::SI >= 0 && E::SI <= PGM_ENVPLUG_MAX_SI, "env plug-in: pgm_user_env::SI outside 0 <= SI <= 4");
    static_assert(E::RW >= 0 && E::RW <= PGM_ENVPLUG_MAX_RW, "env plug-in: pgm_user_env::RW outside 0 <= RW <= 8");
    static_assert(E::MAX_STEPS >= 1, "env plug-in: pgm_user_env::MAX_STEPS must be positive");
    using type = E;
};
using Env = Checked<pgm_user_env>::type;

constexpr int SDN = Env::SD > 0 ? Env::SD : 1, SIN = Env::SI > 0 ? Env::SI : 1;  // register array lengths

// the action of one step: the raw policy sample (A floats) or, for a DISCRETE env, the action index
struct Action {
    const float* v;
    int i;
};
using act_arg = Action;
template <class E>
PGM_ENV_HD inline void call_step(double* sd, int32_t* si, const Action& a, double* obj, double* reward, int32_t* done,
                                 int32_t* bad) {
    if constexpr (E::DISCRETE) {
        E::step(sd, si, a.i, obj, reward, done, bad);
    } else {
        E::step(sd, si, a.v, obj, reward, done, bad);
    }
}

struct State {
    double sd[SDN];
    int32_t si[SIN];
    int32_t elapsed, episode;  // steps of the running episode; resets since pgm_envplug_reset
};

struct StepOut {  // the terminal step's on a done env
    double obj[Env::K];
    double reward;
    int32_t done, bad;
};

// the start state of one reset-table entry (RW uniforms)
PGM_ENV_HD inline void start(State& s, const double* u) {
    for (int i = 0; i < SDN; ++i) s.sd[i] = 0.0;
    for (int i = 0; i < SIN; ++i) s.si[i] = 0;
    s.elapsed = 0;
    Env::reset(s.sd, s.si, u);
}

// one step and the forced limit; no reset (the evaluation's step: an ended episode stands still)
PGM_ENV_HD inline StepOut step_limit(State& s, act_arg action) {
    StepOut o;
    int32_t done = 0, bad = 0;
    o.reward = 0.0;
    for (int k = 0; k < Env::K; ++k) o.obj[k] = 0.0;
    call_step<Env>(s.sd, s.si, action, o.obj, &o.reward, &done, &bad);
    s.elapsed += 1;
    o.done = done != 0;
    o.bad = bad != 0;
    if (s.elapsed >= Env::MAX_STEPS) {  // whatever step reported
        o.done = 1;
        o.bad = 1;
    }
    return o;
}

// ... and the auto-reset: row = this env's [R][RW] uniforms of the reset table
PGM_ENV_HD inline StepOut transition(State& s, act_arg action, const double* row, int R) {
    const StepOut o = step_limit(s, action);
    if (o.done) {
        s.episode += 1;
        start(s, row + (size_t)(s.episode % R) * Env::RW);
    }
    return o;
}

}  // namespace envplug
}  // namespace pgm
