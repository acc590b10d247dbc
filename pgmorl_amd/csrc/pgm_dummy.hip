// MO-Dummy-v0 / MO-Dummy3-v0 on the device (pgm_abi_features() & PGM_FEATURE_DUMMY_DEVICE): the fused Gaussian rollout
// pgm_rollout_dummy, the deterministic evaluation pgm_eval_dummy and the host-only pgm_dummy_transition.  One
// 256-thread workgroup per task, the structure of rollout_kernel / rollout_dst_kernel: a T-step rollout is one launch
// whose steps synchronise with LDS-only barriers.  The towers (plain or LayerNorm), the Gaussian arithmetic and the
// VecNormalize arithmetic are the device functions of pgm_policy_dev.hpp (what pgm_rollout_act / pgm_env_ingest run per
// step of the host-stepped path); the env rule is dummy_transition of pgm_dummy.hpp, the same inline function
// pgm_dummy_transition evaluates on the host.
//
// Reference semantics (paths relative to the reference tree):
//   the env                                environments/dummy_mo_env.py:57-148, environments/__init__.py:4-16
//   TimeLimitMask bad_transition           a2c_ppo_acktr/envs.py (TimeLimitMask)
//   Policy.act / get_value, DiagGaussian   a2c_ppo_acktr/model.py:57-73; distributions.py:29-40,71-90
//   DummyVecEnv auto-reset                 baselines/common/vec_env/dummy_vec_env.py:45-56
//   VecNormalize.step_wait                 baselines/common/vec_env/vec_normalize.py:29-43
//   masks / bad_masks / obj_tensor, insert morl/mopg.py:103-135, a2c_ppo_acktr/storage.py:50-75
//   evaluation()                           morl/mopg.py:25-46
#include "pgm_dummy.hpp"
#include "pgm_policy_dev.hpp"

PGM_STAMP_UNIT(dummy)

namespace pgm {

// the step image of the block kernels plus the scalar env reward of the step (VecNormalize.ret's input)
template <int O, int A, int K>
struct DummySmem {
    StepSmem<O, A, K> st;
    double reward[NMAX];
};

struct DummyRolloutArgs {
    int P, N, T;
    const float* params;
    pgm_dummy_spec env;
    pgm_env_state st;  // s [P][N][6]: pos, vel, totals; elapsed [P][N]: step; s0 unused
    int32_t* episode;  // [P][N] resets since env_reset()
    pgm_norm_state ns;
    pgm_rollout_buf rb;
    const float* noise;  // [T][N][A] or NULL: counter_normal(seed, (t * N + n) * A + a)
    uint64_t seed;
    int carry;
};

template <int O>
__device__ __forceinline__ void dummy_load(DummyEnv& s, const double* sg, int step, int episode) {
    static_assert(O == DUMMY_OBS, "MO-Dummy: obs 6");
    s.pos[0] = sg[0];
    s.pos[1] = sg[1];
    s.vel[0] = sg[2];
    s.vel[1] = sg[3];
    s.dist = sg[4];
    s.energy = sg[5];
    s.step = step;
    s.episode = episode;
}

// fused rollout, block form (Gaussian head on the device MO-Dummy env).  Thread n < N owns env n: it keeps the env's
// state in registers, draws the env's A normals one step ahead, samples its action and runs its transition.  Four
// workgroup barriers per step (policy_forward, the transition hand-off, norm_stats, vecnorm_emit) against the six of
// rollout_kernel (sample_actions and the two of env_dynamics have no counterpart here).
template <class Tw, int O, int A, int K>
__global__ __launch_bounds__(RT) void rollout_dummy_kernel(DummyRolloutArgs a, typename Tw::Lay L) {
    static_assert(O == DUMMY_OBS && A == DUMMY_ACT && K <= DUMMY_KMAX, "MO-Dummy: obs 6, act 2, 2 or 3 objectives");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<DummySmem<O, A, K>*>(smem_raw);
    auto& P = S.st.pol;
    auto& E = S.st.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T;
    const NormCfg nc = norm_cfg(a.ns);
    const float* prm = a.params + (size_t)p * L.total;
    float* obs = a.rb.obs + (size_t)p * (T + 1) * N * O;
    float* act = a.rb.actions + (size_t)p * T * N * A;
    float* logp = a.rb.logp + (size_t)p * T * N;
    float* val = a.rb.values + (size_t)p * (T + 1) * N * K;
    float* rew = a.rb.rewards + (size_t)p * T * N * K;
    float* masks = a.rb.masks + (size_t)p * (T + 1) * N;
    float* bad = a.rb.bad_masks + (size_t)p * (T + 1) * N;
    double* sg = a.st.s + (size_t)p * N * O;
    const bool owner = t < N;

    typename Tw::template Reg<O, A, K> R;
    load_policy<Tw, true>(P, R, prm, L);
    load_env<false>(E, a.st, a.ns, p, N);
    DummyEnv env = {};
    if (owner) dummy_load<O>(env, sg + t * O, a.st.elapsed[p * N + t], a.episode[p * N + t]);
    const double* resets = a.env.reset_table + (size_t)(owner ? t : 0) * a.env.R * 2;
    if (a.carry) {  // after_update(): slot T -> slot 0 (storage.py:71-75); each thread re-reads its own writes
        for (int i = t; i < N * O; i += RT) obs[i] = obs[(size_t)T * N * O + i];
        if (owner) {
            masks[t] = masks[(size_t)T * N + t];
            bad[t] = bad[(size_t)T * N + t];
        }
    }
    load_rows(P, obs, N);
    __syncthreads();

    float ls[A], sd[A], eps_next[A] = {};
#pragma unroll
    for (int j = 0; j < A; ++j) {
        ls[j] = P.logstd[j];
        sd[j] = expf(ls[j]);
    }
    if (owner) {
#pragma unroll
        for (int j = 0; j < A; ++j)
            eps_next[j] = a.noise ? a.noise[t * A + j] : counter_normal(a.seed, (uint64_t)(t * A + j));
    }
    PGM_STAMP_DECL
    for (int step = 0; step < T; ++step) {
        float eps[A];
#pragma unroll
        for (int j = 0; j < A; ++j) eps[j] = eps_next[j];
        if (owner && step + 1 < T) {
#pragma unroll
            for (int j = 0; j < A; ++j) {
                const size_t idx = ((size_t)(step + 1) * N + t) * A + j;
                eps_next[j] = a.noise ? a.noise[idx] : counter_normal(a.seed, idx);
            }
        }
        PGM_STAMP(0);
        policy_forward<Tw>(P, R, N, prm, L);
        PGM_STAMP(1);
        store_values(P, val + (size_t)step * N * K, N);
        if (owner) {
            float av[A], lp = 0.f;
#pragma unroll
            for (int j = 0; j < A; ++j) {  // sample_actions' arithmetic; the log-prob summed over A in index order
                const float mu = P.mu[t][j];
                av[j] = fmaf(eps[j], sd[j], mu);
                lp += gauss_logp_term(av[j], mu, ls[j], sd[j]);
                act[((size_t)step * N + t) * A + j] = av[j];  // raw, unclipped: the env clips
            }
            logp[(size_t)step * N + t] = lp;
            const DummyOut o = dummy_transition(a.env.max_steps, a.env.time_limit_is_bad, a.env.bound, K, resets,
                                                a.env.R, env, av[0], av[1]);
            dummy_observe(env, E.snew[t]);
#pragma unroll
            for (int k = 0; k < K; ++k) E.objraw[t][k] = o.obj[k];
            E.done[t] = o.done;
            E.bad[t] = o.bad;
            S.reward[t] = o.reward;
        }
        lds_sync();
        PGM_STAMP(2);
        norm_stats(E, N, nc, S.reward);
        PGM_STAMP(3);
        vecnorm_emit<O, A, K, opad<O>()>(E, N, nc, P.x, obs + (size_t)(step + 1) * N * O, rew + (size_t)step * N * K,
                                         masks + (size_t)(step + 1) * N, bad + (size_t)(step + 1) * N);
        PGM_STAMP(4);
    }
    // bootstrap value (mopg.py:132-135) -> value_preds[T] (storage.py:85)
    policy_forward<Tw>(P, R, N, prm, L);
    store_values(P, val + (size_t)T * N * K, N);
    __syncthreads();
    store_env<false>(E, a.st, a.ns, p, N);
    if (owner) {
        dummy_observe(env, sg + t * O);
        a.st.elapsed[p * N + t] = env.step;
        a.episode[p * N + t] = env.episode;
    }
    PGM_STAMP_FLUSH;
}

struct DummyEvalArgs {
    int P;
    const float* params;
    pgm_dummy_spec env;  // reset_table: the evaluation table, episode e starts at entry (e, 0)
    const double *ob_mean, *ob_var;
    int eval_num, use_ob, raw;
    double gamma;
    double* objs;
};

// deterministic evaluation (mopg.py:25-46): eval_num episodes are the rows of one forward and step together; thread
// e < eval_num owns episode e.  An ended episode stands still and adds nothing more; the loop ends when every episode
// has (at most max_steps iterations: every live episode's step count grows by one).
template <class Tw, int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_dummy_kernel(DummyEvalArgs a, typename Tw::Lay L) {
    static_assert(O == DUMMY_OBS && A == DUMMY_ACT && K <= DUMMY_KMAX, "MO-Dummy: obs 6, act 2, 2 or 3 objectives");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<DummySmem<O, A, K>*>(smem_raw);
    auto& P = S.st.pol;
    auto& E = S.st.env;
    const int p = blockIdx.x, t = threadIdx.x, EN = a.eval_num;
    const float* prm = a.params + (size_t)p * L.total;
    typename Tw::template Reg<O, A, K> R;
    load_policy<Tw, true>(P, R, prm, L);
    for (int o = t; o < O; o += RT) {
        E.ob_mean[o] = a.use_ob ? a.ob_mean[(size_t)p * O + o] : 0.0;
        E.ob_inv[o] = a.use_ob ? eval_ob_inv(a.ob_var[(size_t)p * O + o]) : 1.0;
    }
    const bool owner = t < EN;
    const double* resets = a.env.reset_table + (size_t)(owner ? t : 0) * a.env.R * 2;
    DummyEnv env = {};
    int alive = 1;
    double acc[K] = {}, disc = 1.0;
    if (owner) {
        env.pos[0] = resets[0];
        env.pos[1] = resets[1];
        dummy_observe(env, E.snew[t]);
        E.done[t] = 0;
    }
    __syncthreads();
    while (true) {
        for (int i = t; i < EN * O; i += RT) {
            const int e = i / O, o = i % O;
            P.x[e][o] = eval_normalise(E.snew[e][o], a.use_ob, E.ob_mean[o], E.ob_inv[o]);
        }
        lds_sync();
        policy_forward<Tw>(P, R, EN, prm, L);
        if (owner && alive) {  // the mean action; the env clips it
            const DummyOut o = dummy_transition(a.env.max_steps, 0, a.env.bound, K, resets, a.env.R, env, P.mu[t][0],
                                                P.mu[t][1]);
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += disc * o.obj[k];
            if (o.done) {
                alive = 0;
                E.done[t] = 1;
            } else {
                dummy_observe(env, E.snew[t]);
            }
        }
        if (!a.raw) disc *= a.gamma;
        lds_sync();
        int live = 0;
        for (int e = 0; e < EN; ++e) live |= !E.done[e];
        if (!live) break;
    }
    if (owner) {
#pragma unroll
        for (int k = 0; k < K; ++k) E.objraw[t][k] = acc[k];
    }
    lds_sync();
    if (t < K) {  // the host path's order: per step inside an episode, then over the episodes
        double s = 0.0;
        for (int e = 0; e < EN; ++e) s += E.objraw[e][t];
        a.objs[(size_t)p * K + t] = s / (double)EN;
    }
}

static bool is_dummy_dims(const pgm_dims* d) { return d->O == DUMMY_OBS && d->A == DUMMY_ACT && (d->K == 2 || d->K == 3); }

static int check_dummy_dims(const pgm_dims* d, const char* what) {
    if (!is_dummy_dims(d)) {
        set_error("%s: unsupported dims O=%d A=%d K=%d for the MO-Dummy env (supported: 6/2/2, 6/2/3)", what, d->O, d->A,
                  d->K);
        return PGM_E_UNSUPPORTED;
    }
    return PGM_OK;
}

// need: the reset-table rows the call reads (N envs / eval_num episodes)
static int check_dummy_env(const pgm_dummy_spec* env, int need, const char* what) {
    if (env->max_steps <= 0) {
        set_error("%s: pgm_dummy_spec.max_steps = %d must be positive", what, env->max_steps);
        return PGM_E_INVALID_ARG;
    }
    if (!(env->bound > 0.0)) {
        set_error("%s: pgm_dummy_spec.bound = %g must be positive", what, env->bound);
        return PGM_E_INVALID_ARG;
    }
    if (env->R < 1) {
        set_error("%s: pgm_dummy_spec.R = %d reset positions per env must be at least 1", what, env->R);
        return PGM_E_INVALID_ARG;
    }
    if (env->reset_count < need) {
        set_error("%s: pgm_dummy_spec.reset_count = %d rows of the reset table, the call reads %d", what,
                  env->reset_count, need);
        return PGM_E_INVALID_ARG;
    }
    return PGM_OK;
}

// the instantiations are the two MO-Dummy dim sets only
template <class F>
static int dispatch_dummy(const pgm_dims* d, const char* what, F&& f) {
    return dispatch_towers(d, what, [&](auto tw, const auto& L, auto o, auto aa, auto k) -> int {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        if constexpr (O == DUMMY_OBS && A == DUMMY_ACT) {
            return f(tw, L, o, aa, k);
        } else {
            return check_dummy_dims(d, what);
        }
    });
}

}  // namespace pgm

using namespace pgm;

extern "C" {

// Arguments are validated before any device work: NULL pointers, check_dims, the dim set, LN, T / eval_num, the spec.
int pgm_rollout_dummy(const pgm_dims* d, const float* params, const pgm_dummy_spec* env, const pgm_env_state* st,
                      int32_t* episode, const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* noise,
                      uint64_t seed, int32_t carry, pgm_stream_t stream) {
    if (!d || !params || !env || !env->reset_table || !st || !st->s || !st->elapsed || !st->obj_acc ||
        !st->obj_acc_valid || !st->ret || !episode || !norm_ok(ns) || !rb || !rb->obs || !rb->actions || !rb->logp ||
        !rb->values || !rb->rewards || !rb->masks || !rb->bad_masks) {
        set_error("pgm_rollout_dummy: null pointer");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, "pgm_rollout_dummy")) return rc;
    if (int rc = check_dummy_dims(d, "pgm_rollout_dummy")) return rc;
    if (int rc = check_ln(d, "pgm_rollout_dummy")) return rc;
    if (d->T <= 0) {
        set_error("pgm_rollout_dummy: T must be positive");
        return PGM_E_SHAPE;
    }
    if (int rc = check_dummy_env(env, d->N, "pgm_rollout_dummy")) return rc;
    DummyRolloutArgs a{d->P, d->N, d->T, params, *env, *st, episode, *ns, *rb, noise, seed, carry};
    return dispatch_dummy(d, "pgm_rollout_dummy", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(rollout_dummy_kernel<decltype(tw), O, A, K>, d->P, sizeof(DummySmem<O, A, K>),
                           (hipStream_t)stream, "pgm_rollout_dummy", a, L);
    });
}

int pgm_eval_dummy(const pgm_dims* d, const float* params, const pgm_dummy_spec* env, const double* ob_mean,
                   const double* ob_var, int32_t eval_num, int32_t use_ob_rms, int32_t raw, double gamma,
                   double* objs_out, pgm_stream_t stream) {
    if (!d || !params || !env || !env->reset_table || !objs_out || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("pgm_eval_dummy: null pointer (ob_mean / ob_var are required with use_ob_rms)");
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: the rows are the evaluation episodes
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, "pgm_eval_dummy")) return rc;
    if (int rc = check_dummy_dims(&dd, "pgm_eval_dummy")) return rc;
    if (int rc = check_ln(&dd, "pgm_eval_dummy")) return rc;
    if (eval_num < 1 || eval_num > NMAX) {
        set_error("pgm_eval_dummy: eval_num=%d evaluation episodes outside [1, %d]", eval_num, NMAX);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dummy_env(env, eval_num, "pgm_eval_dummy")) return rc;
    DummyEvalArgs a{d->P, params, *env, ob_mean, ob_var, eval_num, use_ob_rms != 0, raw != 0, gamma, objs_out};
    return dispatch_dummy(d, "pgm_eval_dummy", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(eval_dummy_kernel<decltype(tw), O, A, K>, d->P, sizeof(DummySmem<O, A, K>),
                           (hipStream_t)stream, "pgm_eval_dummy", a, L);
    });
}

// Host only: launches nothing and needs no device.
int pgm_dummy_transition(const pgm_dummy_spec* spec, int32_t K, int32_t n, const double* state, const int32_t* step,
                         const int32_t* episode, const int32_t* env, const float* action, double* state_out,
                         int32_t* step_out, int32_t* episode_out, double* obj_out, double* reward_out,
                         int32_t* done_out, int32_t* bad_out) {
    if (!spec || !spec->reset_table || n < 0 || !state || !step || !episode || !env || !action || !state_out ||
        !step_out || !episode_out || !obj_out || !reward_out || !done_out || !bad_out) {
        set_error("pgm_dummy_transition: null pointer or negative n");
        return PGM_E_INVALID_ARG;
    }
    if (K != 2 && K != 3) {
        set_error("pgm_dummy_transition: K=%d objectives (supported: 2, 3)", K);
        return PGM_E_UNSUPPORTED;
    }
    if (int rc = check_dummy_env(spec, 1, "pgm_dummy_transition")) return rc;
    for (int32_t i = 0; i < n; ++i)
        if (env[i] < 0 || env[i] >= spec->reset_count || episode[i] < 0) {
            set_error("pgm_dummy_transition: pair %d has env %d (the reset table has %d rows) and episode %d", i, env[i],
                      spec->reset_count, episode[i]);
            return PGM_E_INVALID_ARG;
        }
    for (int32_t i = 0; i < n; ++i) {
        const double* sg = state + (size_t)i * DUMMY_OBS;
        DummyEnv s{{sg[0], sg[1]}, {sg[2], sg[3]}, sg[4], sg[5], step[i], episode[i]};
        const DummyOut o = dummy_transition(spec->max_steps, spec->time_limit_is_bad, spec->bound, K,
                                            spec->reset_table + (size_t)env[i] * spec->R * 2, spec->R, s,
                                            action[(size_t)i * 2], action[(size_t)i * 2 + 1]);
        dummy_observe(s, state_out + (size_t)i * DUMMY_OBS);
        step_out[i] = s.step;
        episode_out[i] = s.episode;
        for (int k = 0; k < K; ++k) obj_out[(size_t)i * K + k] = o.obj[k];
        reward_out[i] = o.reward;
        done_out[i] = o.done;
        bad_out[i] = o.bad;
    }
    return PGM_OK;
}

}  // extern "C"
