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
#define PGM_ENVPLUG_DETECT(member)                \
    template <class E, class = void>              \
    struct has_##member : std::false_type {};     \
    template <class E>                            \
    struct has_##member<E, std::void_t<decltype(&E::member)>> : std::true_type {};
#define PGM_ENVPLUG_HAS(member) \
    PGM_ENVPLUG_DETECT(member)  \
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
// the optional members of contract 2
PGM_ENVPLUG_DETECT(CONTRACT)
PGM_ENVPLUG_DETECT(NP)
PGM_ENVPLUG_DETECT(NW)
PGM_ENVPLUG_DETECT(PAR_DEFAULT)
PGM_ENVPLUG_DETECT(PAR_NAMES)
#undef PGM_ENVPLUG_DETECT

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

// ---- contract 2 (runtime parameters, per-step uniforms): CONTRACT absent or 1 is the contract above, NP = NW = 0
template <class E, bool = has_CONTRACT<E>::value>
struct contract_of {
    static constexpr int value = 1;
};
template <class E>
struct contract_of<E, true> {
    static constexpr int value = E::CONTRACT;
};
template <class E, bool = has_NP<E>::value>
struct np_of {
    static constexpr int value = 0;
};
template <class E>
struct np_of<E, true> {
    static constexpr int value = E::NP;
};
template <class E, bool = has_NW<E>::value>
struct nw_of {
    static constexpr int value = 0;
};
template <class E>
struct nw_of<E, true> {
    static constexpr int value = E::NW;
};
// the identifiers of a comma-separated list, or -1 for an empty one / a character no identifier has
constexpr int count_names(const char* s) {
    int n = 0;
    bool in = false;
    for (; *s; ++s) {
        const char ch = *s;
        const bool alpha = (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || ch == '_';
        if (ch == ',') {
            if (!in) return -1;
            in = false;
        } else if (alpha || (in && ch >= '0' && ch <= '9')) {
            if (!in) ++n;
            in = true;
        } else {
            return -1;
        }
    }
    return in ? n : -1;
}
template <class E, bool = has_PAR_NAMES<E>::value>
struct names_of {
    static constexpr int count = 0;
    static constexpr const char* text = "";
};
template <class E>
struct names_of<E, true> {
    static constexpr int count = count_names(E::PAR_NAMES);
    static constexpr const char* text = E::PAR_NAMES;
};
template <class E, bool = has_PAR_DEFAULT<E>::value>
struct defaults_of {
    static constexpr int count = 0;
    static double at(int) { return 0.0; }
};
template <class E>
struct defaults_of<E, true> {
    static constexpr int count = (int)(sizeof(E::PAR_DEFAULT) / sizeof(double));
    static double at(int i) { return E::PAR_DEFAULT[i]; }
};

template <class E, int C = contract_of<E>::value>
struct CheckedCtx {  // contract 1
    static_assert(C == 1 || C == 2, "env plug-in: pgm_user_env::CONTRACT must be 1 or 2");
    static constexpr int NP = 0, NW = 0;
};
template <class E>
struct CheckedCtx<E, 2> {
    static_assert(has_NP<E>::value, "env plug-in: pgm_user_env::NP is missing (CONTRACT = 2 needs 0 <= NP <= 16)");
    static_assert(has_NW<E>::value, "env plug-in: pgm_user_env::NW is missing (CONTRACT = 2 needs 0 <= NW <= 4)");
    static constexpr int NP = np_of<E>::value, NW = nw_of<E>::value;
    static_assert(NP >= 0 && NP <= PGM_ENVPLUG_MAX_NP, "env plug-in: pgm_user_env::NP outside 0 <= NP <= 16");
    static_assert(NW >= 0 && NW <= PGM_ENVPLUG_MAX_NW, "env plug-in: pgm_user_env::NW outside 0 <= NW <= 4");
    static_assert(NP <= 0 || has_PAR_DEFAULT<E>::value,
                  "env plug-in: pgm_user_env::PAR_DEFAULT is missing (NP > 0 needs double PAR_DEFAULT[NP])");
    static_assert(NP <= 0 || has_PAR_NAMES<E>::value,
                  "env plug-in: pgm_user_env::PAR_NAMES is missing (NP > 0 needs NP comma-separated identifiers)");
    static_assert(NP <= 0 || !has_PAR_DEFAULT<E>::value || defaults_of<E>::count == NP,
                  "env plug-in: pgm_user_env::PAR_DEFAULT must hold NP values");
    static_assert(NP <= 0 || !has_PAR_NAMES<E>::value || names_of<E>::count == NP,
                  "env plug-in: pgm_user_env::PAR_NAMES must hold NP comma-separated identifiers");
};
constexpr int CONTRACT = contract_of<Env>::value;
constexpr bool C2 = CONTRACT == 2;
constexpr int NP = CheckedCtx<Env>::NP, NW = CheckedCtx<Env>::NW;
constexpr int NPN = NP > 0 ? NP : 1, NWN = NW > 0 ? NW : 1;  // register array lengths

// the action of one step: the raw policy sample (A floats) or, for a DISCRETE env, the action index
struct Action {
    const float* v;
    int i;
};
using act_arg = Action;
// the header's three functions; a contract-2 header's take the ctx, a contract-1 header's never see it
template <class E>
PGM_ENV_HD inline void call_step(double* sd, int32_t* si, const Action& a, double* obj, double* reward, int32_t* done,
                                 int32_t* bad, const pgm_env_ctx& c) {
    if constexpr (contract_of<E>::value == 2) {
        if constexpr (E::DISCRETE) {
            E::step(sd, si, a.i, obj, reward, done, bad, c);
        } else {
            E::step(sd, si, a.v, obj, reward, done, bad, c);
        }
    } else if constexpr (E::DISCRETE) {
        E::step(sd, si, a.i, obj, reward, done, bad);
    } else {
        E::step(sd, si, a.v, obj, reward, done, bad);
    }
}
template <class E>
PGM_ENV_HD inline void call_reset(double* sd, int32_t* si, const double* u, const double* par) {
    if constexpr (contract_of<E>::value == 2) {
        E::reset(sd, si, u, pgm_env_ctx{par, nullptr});
    } else {
        E::reset(sd, si, u);
    }
}
template <class E>
PGM_ENV_HD inline void call_observe(const double* sd, const int32_t* si, double* obs, const double* par) {
    if constexpr (contract_of<E>::value == 2) {
        E::observe(sd, si, obs, pgm_env_ctx{par, nullptr});
    } else {
        E::observe(sd, si, obs);
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

// the start state of one reset-table entry (RW uniforms); reset sees c.par alone
PGM_ENV_HD inline void start(State& s, const double* u, const pgm_env_ctx& c) {
    for (int i = 0; i < SDN; ++i) s.sd[i] = 0.0;
    for (int i = 0; i < SIN; ++i) s.si[i] = 0;
    s.elapsed = 0;
    call_reset<Env>(s.sd, s.si, u, c.par);
}

// one step and the forced limit; no reset (the evaluation's step: an ended episode stands still)
PGM_ENV_HD inline StepOut step_limit(State& s, act_arg action, const pgm_env_ctx& c) {
    StepOut o;
    int32_t done = 0, bad = 0;
    o.reward = 0.0;
    for (int k = 0; k < Env::K; ++k) o.obj[k] = 0.0;
    call_step<Env>(s.sd, s.si, action, o.obj, &o.reward, &done, &bad, c);
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
PGM_ENV_HD inline StepOut transition(State& s, act_arg action, const double* row, int R, const pgm_env_ctx& c) {
    const StepOut o = step_limit(s, action, c);
    if (o.done) {
        s.episode += 1;
        start(s, row + (size_t)(s.episode % R) * Env::RW, c);
    }
    return o;
}

// the forms without a ctx: a contract-1 header's (templates only so that the refusal waits for a call)
template <class E = Env>
PGM_ENV_HD inline void start(State& s, const double* u) {
    static_assert(contract_of<E>::value == 1, "env plug-in: a CONTRACT = 2 header needs the form taking pgm_env_ctx");
    start(s, u, pgm_env_ctx{nullptr, nullptr});
}
template <class E = Env>
PGM_ENV_HD inline StepOut step_limit(State& s, act_arg action) {
    static_assert(contract_of<E>::value == 1, "env plug-in: a CONTRACT = 2 header needs the form taking pgm_env_ctx");
    return step_limit(s, action, pgm_env_ctx{nullptr, nullptr});
}
template <class E = Env>
PGM_ENV_HD inline StepOut transition(State& s, act_arg action, const double* row, int R) {
    static_assert(contract_of<E>::value == 1, "env plug-in: a CONTRACT = 2 header needs the form taking pgm_env_ctx");
    return transition(s, action, row, R, pgm_env_ctx{nullptr, nullptr});
}

// ---- the env-noise stream of contract 2: integers only, so the host and the device agree bit for bit.  key is the
// stream key of counter_normal / counter_uniform (pgm_common.hpp; oracle/streams.py stream_key, hash_at).
PGM_ENV_HD inline uint64_t noise_mix(uint64_t x) {  // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
PGM_ENV_HD inline uint64_t noise_key(uint64_t seed) {
    return noise_mix(seed * 0xD1B54A32D192ED03ull + 0x632BE59BD9B4E019ull);
}
// the top 53 bits as a double in [0, 1): the conversion and the power-of-two scaling are exact
PGM_ENV_HD inline double u53_at(uint64_t key, uint64_t i) {
    return (double)(noise_mix(key ^ i) >> 11) * (1.0 / 9007199254740992.0);
}
PGM_ENV_HD inline double u53(uint64_t seed, uint64_t i) { return u53_at(noise_key(seed), i); }

}  // namespace envplug
}  // namespace pgm
