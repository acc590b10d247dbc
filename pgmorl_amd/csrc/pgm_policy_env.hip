// Policy forward, synthetic env + VecNormalize, the fused rollout and the deterministic
// evaluation.  One workgroup (256 threads) per task; everything a task touches per step lives
// in LDS (weights, env constants, env state, running statistics, the current obs rows), so a
// T-step rollout is one launch whose steps synchronise with LDS-only barriers: the per-step
// rollout-storage stores to HBM stay in flight across barriers instead of being drained.
// The device functions (LDS images, policy forward, env, VecNormalize) and launch helpers are in pgm_policy_dev.hpp,
// shared with the host-stepped environment kernels of pgm_hostenv.hip; this file keeps the kernels and entry points.
//
// Reference semantics (paths relative to the reference tree):
//   Policy.act / get_value                 a2c_ppo_acktr/model.py:57-73, 237-246
//   DiagGaussian sample + log_prob         a2c_ppo_acktr/distributions.py:29-40,71-90
//   DummyVecEnv auto-reset                 baselines/common/vec_env/dummy_vec_env.py:45-56
//   TimeLimitMask bad_transition           a2c_ppo_acktr/envs.py:122-131
//   VecNormalize.step_wait / reset         baselines/common/vec_env/vec_normalize.py:29-66
//   RunningMeanStd Chan merge              baselines/common/running_mean_std.py:3-31
//   masks / bad_masks / obj_tensor         morl/mopg.py:110-130
//   RolloutStorage.insert / after_update   a2c_ppo_acktr/storage.py:50-75
//   evaluation()                           morl/mopg.py:25-46
#include <stdlib.h>

#include "pgm_policy_dev.hpp"

PGM_STAMP_UNIT(rollout)

namespace pgm {

// ------------------------------------------------------------------------------------------
// kernels: each body once, for a Towers type and (where a discrete-action policy can run it) a Head type
//
// act: value, action and log-prob of N given rows per task (Policy.act, model.py:57-73)
template <class Hd>
struct ActArgs {
    int P, N;
    const float* params;
    const float* obs;  // [P][N][O]
    const float* rnd;  // [N][width], shared by the tasks; read unless deterministic
    int deterministic;
    float* value;                   // [P][N][K]
    typename Hd::action_t* action;  // [P][N][width]
    float* logp;                    // [P][N]
};

template <class Tw, class Hd, int O, int A, int K>
__global__ __launch_bounds__(RT) void act_kernel(ActArgs<Hd> a, typename Tw::Lay L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, N = a.N;
    constexpr int W = Hd::template width<A>;
    const float* prm = a.params + (size_t)p * L.total;
    typename Tw::template Reg<O, A, K> R;
    load_policy<Tw, Hd::has_logstd>(S, R, prm, L);
    load_rows(S, a.obs + (size_t)p * N * O, N);
    __syncthreads();
    policy_forward<Tw>(S, R, N, prm, L);
    store_values(S, a.value + (size_t)p * N * K, N);
    Hd::emit(S, N, a.deterministic ? nullptr : a.rnd, nullptr, a.action + (size_t)p * N * W, a.logp + (size_t)p * N);
}

struct EnvArgs {
    int P, N;
    pgm_env_spec spec;
    pgm_env_state st;
    pgm_norm_state ns;
    const float* action;
    float *obs_out, *rew_out, *mask_out, *bad_out;
    int reset;
};

struct EnvRunsArgs : EnvArgs {
    const int32_t* run_of_task;  // [P], device (pgm_env_reset_runs)
};
template <bool RUNS>
using EnvArgsT = std::conditional_t<RUNS, EnvRunsArgs, EnvArgs>;

// RUNS (here and in the two kernels below): the reset table is stacked per run, and the task's block is selected once,
// before Spec / load_spec take the pointer (pgm_rollout.hpp)
template <int O, int A, int K, bool RUNS>
__global__ __launch_bounds__(RT) void env_kernel(EnvArgsT<RUNS> a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N;
    if constexpr (RUNS) a.st.s0 += (size_t)a.run_of_task[p] * N * O;
    const NormCfg nc = norm_cfg(a.ns);
    const Spec<O, A, K> sp{E, a.spec, a.st.s0};
    load_spec(E, a.spec, a.st.s0, N);
    load_env(E, a.st, a.ns, p, N);
    __syncthreads();
    if (a.reset) {
        if (t < N) E.elapsed[t] = 0;
        for (int o = t; o < O; o += RT)
            for (int n = 0; n < N; ++n) {
                const double v = sp.s0(n, o);
                E.snew[n][o] = v;
                E.s[n][o] = v;
            }
        vecnorm_reset(E, N, nc, a.obs_out + (size_t)p * N * O);
    } else {
        for (int i = t; i < N * A; i += RT) {
            const int j = i % A;
            E.ac[i / A][j] = clipd((double)a.action[(size_t)p * N * A + i], sp.lo(j), sp.hi(j));
        }
        __syncthreads();
        env_dynamics(E, sp, N, a.spec.max_episode_steps);
        vecnorm_stats(E, sp, N, nc);
        vecnorm_emit<O, A, K, opad<O>()>(E, N, nc, S.pol.x, a.obs_out + (size_t)p * N * O,
                                         a.rew_out + (size_t)p * N * K, a.mask_out + (size_t)p * N,
                                         a.bad_out + (size_t)p * N);
    }
    __syncthreads();
    store_env(E, a.st, a.ns, p, N);
}

// fused rollout, block form (Gaussian head on the device envs).  L is the towers' layout (a.L for the plain ones).
template <class Tw, int O, int A, int K, bool RUNS>
__global__ __launch_bounds__(RT) void rollout_kernel(RolloutArgsT<RUNS> a, typename Tw::Lay L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& P = S.pol;
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T;
    if constexpr (RUNS) a.st.s0 += (size_t)a.run_of_task[p] * N * O;
    const NormCfg nc = norm_cfg(a.ns);
    const Spec<O, A, K> sp{E, a.spec, a.st.s0};
    const float* prm = a.params + (size_t)p * L.total;
    float* obs = a.rb.obs + (size_t)p * (T + 1) * N * O;
    float* act = a.rb.actions + (size_t)p * T * N * A;
    float* logp = a.rb.logp + (size_t)p * T * N;
    float* val = a.rb.values + (size_t)p * (T + 1) * N * K;
    float* rew = a.rb.rewards + (size_t)p * T * N * K;
    float* masks = a.rb.masks + (size_t)p * (T + 1) * N;
    float* bad = a.rb.bad_masks + (size_t)p * (T + 1) * N;

    typename Tw::template Reg<O, A, K> R;
    load_policy<Tw, true>(P, R, prm, L);
    load_spec(E, a.spec, a.st.s0, N);
    load_env(E, a.st, a.ns, p, N);
    if (a.carry) {  // after_update(): slot T -> slot 0 (storage.py:71-75); each thread re-reads its own writes
        for (int i = t; i < N * O; i += RT) obs[i] = obs[(size_t)T * N * O + i];
        if (t < N) {
            masks[t] = masks[(size_t)T * N + t];
            bad[t] = bad[(size_t)T * N + t];
        }
    }
    load_rows(P, obs, N);
    __syncthreads();

    // the lane drawing (n, a) of each step keeps its noise one step ahead in a register
    const bool drawer = t < N * A;
    float eps_next = 0.f;
    if (drawer) eps_next = a.noise ? a.noise[t] : counter_normal(a.seed, (uint64_t)t);
    PGM_STAMP_DECL
    for (int step = 0; step < T; ++step) {
        const float eps = eps_next;
        if (drawer && step + 1 < T) {
            const size_t idx = (size_t)(step + 1) * N * A + t;
            eps_next = a.noise ? a.noise[idx] : counter_normal(a.seed, idx);
        }
        PGM_STAMP(0);
        policy_forward<Tw>(P, R, N, prm, L);
        PGM_STAMP(1);
        store_values(P, val + (size_t)step * N * K, N);
        sample_actions(P, E, sp, N, eps, act + (size_t)step * N * A);
        PGM_STAMP(2);
        if (t < N) {
            float s = 0.f;
            for (int j = 0; j < A; ++j) s += P.lp[t][j];
            logp[(size_t)step * N + t] = s;
        }
        env_dynamics(E, sp, N, a.spec.max_episode_steps);
        PGM_STAMP(3);
        vecnorm_stats(E, sp, N, nc);
        PGM_STAMP(4);
        vecnorm_emit<O, A, K, opad<O>()>(E, N, nc, P.x, obs + (size_t)(step + 1) * N * O,
                                         rew + (size_t)step * N * K, masks + (size_t)(step + 1) * N,
                                         bad + (size_t)(step + 1) * N);
        PGM_STAMP(5);
    }
    // bootstrap value (mopg.py:132-135) -> value_preds[T] (storage.py:85)
    policy_forward<Tw>(P, R, N, prm, L);
    store_values(P, val + (size_t)T * N * K, N);
    __syncthreads();
    store_env(E, a.st, a.ns, p, N);
    PGM_STAMP_FLUSH;
}

// deterministic evaluation, block form (mopg.py:25-46)
template <class Tw, int O, int A, int K, bool RUNS>
__global__ __launch_bounds__(RT) void eval_kernel(EvalArgsT<RUNS> a, typename Tw::Lay L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& P = S.pol;
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x;
    if constexpr (RUNS) a.s0_eval += (size_t)a.run_of_task[p] * a.eval_num * O;
    const float* prm = a.params + (size_t)p * L.total;
    typename Tw::template Reg<O, A, K> R;
    load_policy<Tw, true>(P, R, prm, L);
    load_spec(E, a.spec, a.s0_eval, 1);
    for (int o = t; o < O; o += RT) {
        E.ob_mean[o] = a.use_ob ? a.ob_mean[(size_t)p * O + o] : 0.0;
        E.ob_inv[o] = a.use_ob ? eval_ob_inv(a.ob_var[(size_t)p * O + o]) : 1.0;
    }
    if (t < K) E.objsum[t] = 0.0;
    __syncthreads();
    for (int e = 0; e < a.eval_num; ++e) {
        const double* s0 = a.s0_eval + (size_t)e * O;
        const Spec<O, A, K> sp{E, a.spec, s0};
        for (int o = t; o < O; o += RT) E.s[0][o] = s0[o];
        if (t == 0) E.elapsed[0] = 0;
        double g = 1.0;
        __syncthreads();
        while (true) {
            for (int o = t; o < O; o += RT) P.x[0][o] = eval_normalise(E.s[0][o], a.use_ob, E.ob_mean[o], E.ob_inv[o]);
            lds_sync();
            policy_forward<Tw>(P, R, 1, prm, L);
            if (t < A) E.ac[0][t] = clipd((double)P.mu[0][t], sp.lo(t), sp.hi(t));
            lds_sync();
            env_dynamics(E, sp, 1, a.spec.max_episode_steps);
            if (t < K) E.objsum[t] += g * E.objraw[0][t];
            if (!a.raw) g *= a.gamma;
            const int done = E.done[0];
            for (int o = t; o < O; o += RT) E.s[0][o] = E.snew[0][o];
            lds_sync();
            if (done) break;
        }
    }
    if (t < K) a.objs[(size_t)p * K + t] = E.objsum[t] / (double)a.eval_num;
}

}  // namespace pgm

using namespace pgm;

extern "C" {

int pgm_act_forward(const pgm_dims* d, const float* params, const float* obs, const float* noise,
                    int32_t deterministic, float* value, float* action, float* logp, pgm_stream_t stream) {
    if (int rc = check_dims(d, "pgm_act_forward")) return rc;
    if (int rc = check_ln(d, "pgm_act_forward")) return rc;
    if (!params || !obs || !value || !action || !logp || (!deterministic && !noise)) {
        set_error("pgm_act_forward: null pointer (noise is required unless deterministic)");
        return PGM_E_INVALID_ARG;
    }
    ActArgs<GaussHead> a{d->P, d->N, params, obs, noise, deterministic, value, action, logp};
    return dispatch_towers(d, "pgm_act_forward", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(act_kernel<decltype(tw), GaussHead, O, A, K>, d->P, sizeof(PolSmem<O, A, K>),
                           (hipStream_t)stream, "pgm_act_forward", a, L);
    });
}

// Discrete-action policies.  Arguments are validated before any device work: NULL pointers, check_dims, the dim set,
// LN.
int pgm_act_forward_cat(const pgm_dims* d, const float* params, const float* obs, const float* uniforms,
                        int32_t deterministic, float* value, int32_t* action, float* logp, pgm_stream_t stream) {
    if (!d || !params || !obs || !value || !action || !logp || (!deterministic && !uniforms)) {
        set_error("pgm_act_forward_cat: null pointer (uniforms is required unless deterministic)");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, "pgm_act_forward_cat")) return rc;
    if (int rc = check_cat_dims(d, "pgm_act_forward_cat")) return rc;
    if (int rc = check_cat_ln(d, "pgm_act_forward_cat")) return rc;
    ActArgs<CatHead> a{d->P, d->N, params, obs, uniforms, deterministic, value, action, logp};
    return dispatch_towers_cat(d, "pgm_act_forward_cat", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(act_kernel<decltype(tw), CatHead, O, A, K>, d->P, sizeof(PolSmem<O, A, K>),
                           (hipStream_t)stream, "pgm_act_forward_cat", a, L);
    });
}

static int env_common(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st,
                      const pgm_norm_state* ns, const char* what) {
    if (int rc = check_dims(d, what)) return rc;
    if (!spec_ok(spec) || !state_ok(st) || !norm_ok(ns)) {
        set_error("%s: null pointer in spec/state/norm structs", what);
        return PGM_E_INVALID_ARG;
    }
    return PGM_OK;
}

static int launch_env(const pgm_dims* d, const EnvArgs& a, pgm_stream_t stream, const char* what,
                      const int32_t* runs = nullptr) {
    return dispatch_dims(d->O, d->A, d->K, what, [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        if (runs)
            return launch_smem(env_kernel<O, A, K, true>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream, what,
                               EnvRunsArgs{a, runs});
        return launch_smem(env_kernel<O, A, K, false>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream, what, a);
    });
}

// the *_runs entry points' own check, after every check of the entry point they extend
static int check_runs(const int32_t* run_of_task, int32_t num_runs, const char* what) {
    if (!run_of_task || num_runs < 1) {
        set_error("%s: run_of_task is NULL or num_runs < 1", what);
        return PGM_E_INVALID_ARG;
    }
    return PGM_OK;
}

// pgm_env_reset and pgm_env_reset_runs (runs: the second one's run_of_task / num_runs, checked last)
static int env_reset_impl(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st, const pgm_norm_state* ns,
                          float* obs_out, pgm_stream_t stream, const int32_t* const* runs, int32_t num_runs) {
    if (int rc = env_common(d, spec, st, ns, "pgm_env_reset")) return rc;
    if (!obs_out) {
        set_error("pgm_env_reset: null obs_out");
        return PGM_E_INVALID_ARG;
    }
    if (runs)
        if (int rc = check_runs(*runs, num_runs, "pgm_env_reset_runs")) return rc;
    return launch_env(d, EnvArgs{d->P, d->N, *spec, *st, *ns, nullptr, obs_out, nullptr, nullptr, nullptr, 1}, stream,
                      runs ? "pgm_env_reset_runs" : "pgm_env_reset", runs ? *runs : nullptr);
}

int pgm_env_reset(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st,
                  const pgm_norm_state* ns, float* obs_out, pgm_stream_t stream) {
    return env_reset_impl(d, spec, st, ns, obs_out, stream, nullptr, 0);
}

int pgm_env_reset_runs(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st, const pgm_norm_state* ns,
                       const int32_t* run_of_task, int32_t num_runs, float* obs_out, pgm_stream_t stream) {
    return env_reset_impl(d, spec, st, ns, obs_out, stream, &run_of_task, num_runs);
}

int pgm_env_step(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st,
                 const pgm_norm_state* ns, const float* action, float* obs_out, float* reward_out,
                 float* masks_out, float* bad_masks_out, pgm_stream_t stream) {
    if (int rc = env_common(d, spec, st, ns, "pgm_env_step")) return rc;
    if (!action || !obs_out || !reward_out || !masks_out || !bad_masks_out) {
        set_error("pgm_env_step: null pointer");
        return PGM_E_INVALID_ARG;
    }
    return launch_env(d, EnvArgs{d->P, d->N, *spec, *st, *ns, action, obs_out, reward_out, masks_out, bad_masks_out, 0},
                      stream, "pgm_env_step");
}

static int rollout_impl(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const pgm_env_state* st,
                        const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* noise, uint64_t seed,
                        int32_t carry, const pgm_launch_opts* opts, pgm_stream_t stream, const int32_t* const* runs_arg,
                        int32_t num_runs) {
    if (int rc = env_common(d, spec, st, ns, "pgm_rollout")) return rc;
    if (int rc = check_ln(d, "pgm_rollout")) return rc;
    pgm_launch_opts o;
    if (int rc = read_opts(opts, &o, "pgm_rollout")) return rc;
    if (!params || !rb || !rb->obs || !rb->actions || !rb->logp || !rb->values || !rb->rewards || !rb->masks ||
        !rb->bad_masks) {
        set_error("pgm_rollout: null pointer");
        return PGM_E_INVALID_ARG;
    }
    if (d->T <= 0) {
        set_error("pgm_rollout: T must be positive");
        return PGM_E_SHAPE;
    }
    const int32_t* runs = nullptr;
    if (runs_arg) {
        if (int rc = check_runs(*runs_arg, num_runs, "pgm_rollout_runs")) return rc;
        runs = *runs_arg;
    }
    RolloutArgs a{d->P, d->N, d->T, make_layout(d->O, d->A, d->K, d->H), params, *spec, *st, *ns, *rb,
                  noise, seed, carry};
    // LayerNorm towers: one kernel family, opts ignored; plain: the block kernel on request (A/B, tests) or last
    if (!d->LN && o.rollout_kernel != 1) {
        if (rollout_lanes_supported(d)) return launch_rollout_lanes(d, a, (hipStream_t)stream, runs);
        if (rollout_wide_supported(d)) return launch_rollout_wide(d, a, (hipStream_t)stream, runs);
    }
    return dispatch_towers(d, "pgm_rollout", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        if (runs)
            return launch_smem(rollout_kernel<decltype(tw), O, A, K, true>, d->P, sizeof(StepSmem<O, A, K>),
                               (hipStream_t)stream, "pgm_rollout_runs", RolloutRunsArgs{a, runs}, L);
        return launch_smem(rollout_kernel<decltype(tw), O, A, K, false>, d->P, sizeof(StepSmem<O, A, K>),
                           (hipStream_t)stream, "pgm_rollout", a, L);
    });
}

int pgm_rollout(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const pgm_env_state* st,
                const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* noise, uint64_t seed,
                int32_t carry, const pgm_launch_opts* opts, pgm_stream_t stream) {
    return rollout_impl(d, params, spec, st, ns, rb, noise, seed, carry, opts, stream, nullptr, 0);
}

int pgm_rollout_runs(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const pgm_env_state* st,
                     const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* noise, uint64_t seed,
                     int32_t carry, const int32_t* run_of_task, int32_t num_runs, const pgm_launch_opts* opts,
                     pgm_stream_t stream) {
    return rollout_impl(d, params, spec, st, ns, rb, noise, seed, carry, opts, stream, &run_of_task, num_runs);
}

static int eval_impl(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const double* ob_mean,
                     const double* ob_var, const double* s0_eval, int32_t eval_num, int32_t use_ob_rms, int32_t raw,
                     double gamma, double* objs_out, const pgm_launch_opts* opts, pgm_stream_t stream,
                     const int32_t* const* runs_arg, int32_t num_runs) {
    if (int rc = check_dims(d, "pgm_eval")) return rc;
    if (int rc = check_ln(d, "pgm_eval")) return rc;
    pgm_launch_opts o;
    if (int rc = read_opts(opts, &o, "pgm_eval")) return rc;
    if (!params || !spec_ok(spec) || !s0_eval || !objs_out || eval_num <= 0 || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("pgm_eval: bad arguments");
        return PGM_E_INVALID_ARG;
    }
    const int32_t* runs = nullptr;
    if (runs_arg) {
        if (int rc = check_runs(*runs_arg, num_runs, "pgm_eval_runs")) return rc;
        runs = *runs_arg;
    }
    EvalArgs a{d->P, make_layout(d->O, d->A, d->K, d->H), params, *spec, ob_mean, ob_var, s0_eval,
               eval_num, use_ob_rms, raw, gamma, objs_out};
    // LayerNorm towers: one kernel family, opts ignored; plain: the block kernel on request (A/B, tests) or last
    if (!d->LN && o.eval_kernel != 1) {
        if (eval_waves_supported(d, eval_num)) return launch_eval_waves(d, a, (hipStream_t)stream, runs);
        if (eval_wide_supported(d, eval_num)) return launch_eval_wide(d, a, (hipStream_t)stream, runs);
    }
    return dispatch_towers(d, "pgm_eval", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        if (runs)
            return launch_smem(eval_kernel<decltype(tw), O, A, K, true>, d->P, sizeof(StepSmem<O, A, K>),
                               (hipStream_t)stream, "pgm_eval_runs", EvalRunsArgs{a, runs}, L);
        return launch_smem(eval_kernel<decltype(tw), O, A, K, false>, d->P, sizeof(StepSmem<O, A, K>),
                           (hipStream_t)stream, "pgm_eval", a, L);
    });
}

int pgm_eval(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const double* ob_mean,
             const double* ob_var, const double* s0_eval, int32_t eval_num, int32_t use_ob_rms, int32_t raw,
             double gamma, double* objs_out, const pgm_launch_opts* opts, pgm_stream_t stream) {
    return eval_impl(d, params, spec, ob_mean, ob_var, s0_eval, eval_num, use_ob_rms, raw, gamma, objs_out, opts, stream,
                     nullptr, 0);
}

int pgm_eval_runs(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const double* ob_mean,
                  const double* ob_var, const double* s0_eval, int32_t eval_num, int32_t use_ob_rms, int32_t raw,
                  double gamma, double* objs_out, const int32_t* run_of_task, int32_t num_runs,
                  const pgm_launch_opts* opts, pgm_stream_t stream) {
    return eval_impl(d, params, spec, ob_mean, ob_var, s0_eval, eval_num, use_ob_rms, raw, gamma, objs_out, opts, stream,
                     &run_of_task, num_runs);
}
}  // extern "C"
