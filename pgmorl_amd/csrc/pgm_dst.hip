// Deep Sea Treasure on the device (pgm_abi_features() & PGM_FEATURE_DST_DEVICE): the fused Categorical rollout
// pgm_rollout_dst, the deterministic evaluation pgm_eval_dst and the host-only pgm_dst_transition.  One 256-thread
// workgroup per task, the structure of rollout_kernel / eval_kernel in pgm_policy_env.hip: a T-step rollout is one
// launch whose steps synchronise with LDS-only barriers.  The towers, the sampling rule and the VecNormalize arithmetic
// are the device functions of pgm_policy_dev.hpp (what pgm_rollout_act_cat / pgm_env_ingest run per step of the
// host-stepped path); the env rule is dst_transition of pgm_dst.hpp, the same inline function pgm_dst_transition
// evaluates on the host.
//
// Reference semantics (paths relative to the reference tree):
//   the env                                environments/deep_sea_treasure.py:111-183
//   Policy.act / get_value, Categorical    a2c_ppo_acktr/model.py:33-35,57-73; distributions.py:17-27,54-68
//   DummyVecEnv auto-reset                 baselines/common/vec_env/dummy_vec_env.py:45-56
//   VecNormalize.step_wait                 baselines/common/vec_env/vec_normalize.py:29-43
//   masks / bad_masks / obj_tensor, insert morl/mopg.py:103-135, a2c_ppo_acktr/storage.py:50-75
//   evaluation()                           morl/mopg.py:25-46
#include "pgm_dst.hpp"
#include "pgm_policy_dev.hpp"

PGM_STAMP_UNIT(dst)

namespace pgm {

// the step image of the block kernels plus the scalar env reward of the step (VecNormalize.ret's input)
template <int O, int A, int K>
struct DstSmem {
    StepSmem<O, A, K> st;
    double reward[NMAX];
};

struct DstRolloutArgs {
    int P, N, T;
    const float* params;
    pgm_dst_spec env;
    pgm_env_state st;  // s [P][N][3]: row, col, step as integer-valued fp64; elapsed / s0 unused
    pgm_norm_state ns;
    pgm_rollout_buf rb;
    const float* uniforms;  // [T][N] or NULL: counter_uniform(seed, t * N + n)
    uint64_t seed;
    int carry;
};

// fused rollout, block form (Categorical head on the device Deep Sea Treasure).  Thread n < N owns env n: it draws the
// env's uniform one step ahead, samples its action, runs its transition.
template <int O, int A, int K>
__global__ __launch_bounds__(RT) void rollout_dst_kernel(DstRolloutArgs a, Layout L) {
    static_assert(O == 3 && K == 2, "Deep Sea Treasure: obs 3, 2 objectives");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<DstSmem<O, A, K>*>(smem_raw);
    auto& P = S.st.pol;
    auto& E = S.st.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T;
    const NormCfg nc = norm_cfg(a.ns);
    const float* prm = a.params + (size_t)p * L.total;
    float* obs = a.rb.obs + (size_t)p * (T + 1) * N * O;
    float* act = a.rb.actions + (size_t)p * T * N;
    float* logp = a.rb.logp + (size_t)p * T * N;
    float* val = a.rb.values + (size_t)p * (T + 1) * N * K;
    float* rew = a.rb.rewards + (size_t)p * T * N * K;
    float* masks = a.rb.masks + (size_t)p * (T + 1) * N;
    float* bad = a.rb.bad_masks + (size_t)p * (T + 1) * N;
    double* sg = a.st.s + (size_t)p * N * O;

    PolReg<O, A, K> R;
    load_policy<PlainTowers, false>(P, R, prm, L);
    load_env<false>(E, a.st, a.ns, p, N);
    int row = 0, col = 0, cnt = 0;  // this thread's env (t < N): exact in fp64
    if (t < N) {
        row = (int)sg[t * O + 0];
        col = (int)sg[t * O + 1];
        cnt = (int)sg[t * O + 2];
    }
    if (a.carry) {  // after_update(): slot T -> slot 0 (storage.py:71-75); each thread re-reads its own writes
        for (int i = t; i < N * O; i += RT) obs[i] = obs[(size_t)T * N * O + i];
        if (t < N) {
            masks[t] = masks[(size_t)T * N + t];
            bad[t] = bad[(size_t)T * N + t];
        }
    }
    load_rows(P, obs, N);
    __syncthreads();

    const bool owner = t < N;
    float u_next = 0.f;
    if (owner) u_next = a.uniforms ? a.uniforms[t] : counter_uniform(a.seed, (uint64_t)t);
    PGM_STAMP_DECL
    for (int step = 0; step < T; ++step) {
        const float u = u_next;
        if (owner && step + 1 < T) {
            const size_t idx = (size_t)(step + 1) * N + t;
            u_next = a.uniforms ? a.uniforms[idx] : counter_uniform(a.seed, idx);
        }
        PGM_STAMP(0);
        policy_forward<PlainTowers>(P, R, N, prm, L);
        PGM_STAMP(1);
        store_values(P, val + (size_t)step * N * K, N);
        if (owner) {
            float lp;
            const int ai = cat_sample<A>(P.mu[t], false, u, lp);
            act[(size_t)step * N + t] = (float)ai;
            logp[(size_t)step * N + t] = lp;
            const DstStep o = dst_transition(a.env.max_steps, a.env.time_limit_is_bad, row, col, cnt, ai);
            row = o.row;
            col = o.col;
            cnt = o.step;
#pragma unroll
            for (int j = 0; j < O; ++j) E.snew[t][j] = o.obs[j];
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
    policy_forward<PlainTowers>(P, R, N, prm, L);
    store_values(P, val + (size_t)T * N * K, N);
    __syncthreads();
    store_env<false>(E, a.st, a.ns, p, N);
    if (owner) {
        sg[t * O + 0] = (double)row;
        sg[t * O + 1] = (double)col;
        sg[t * O + 2] = (double)cnt;
    }
    PGM_STAMP_FLUSH;
}

struct DstEvalArgs {
    int P;
    const float* params;
    pgm_dst_spec env;
    const double *ob_mean, *ob_var;
    int eval_num, use_ob, raw;
    double gamma;
    double* objs;
};

// deterministic evaluation (mopg.py:25-46): eval_num episodes are the rows of one forward and step together from
// (0, 0, 0); thread e < eval_num owns episode e.  An ended episode stands still and adds nothing more; the loop ends
// when every episode has (at most max_steps iterations: every live episode's step count grows by one).
template <int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_dst_kernel(DstEvalArgs a, Layout L) {
    static_assert(O == 3 && K == 2, "Deep Sea Treasure: obs 3, 2 objectives");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<DstSmem<O, A, K>*>(smem_raw);
    auto& P = S.st.pol;
    auto& E = S.st.env;
    const int p = blockIdx.x, t = threadIdx.x, EN = a.eval_num;
    const float* prm = a.params + (size_t)p * L.total;
    PolReg<O, A, K> R;
    load_policy<PlainTowers, false>(P, R, prm, L);
    for (int o = t; o < O; o += RT) {
        E.ob_mean[o] = a.use_ob ? a.ob_mean[(size_t)p * O + o] : 0.0;
        E.ob_inv[o] = a.use_ob ? eval_ob_inv(a.ob_var[(size_t)p * O + o]) : 1.0;
    }
    const bool owner = t < EN;
    int row = 0, col = 0, cnt = 0, alive = 1;
    double acc[K] = {}, disc = 1.0;
    if (owner) {
        dst_observe(0, 0, 0, a.env.max_steps, E.snew[t]);
        E.done[t] = 0;
    }
    __syncthreads();
    while (true) {
        for (int i = t; i < EN * O; i += RT) {
            const int e = i / O, o = i % O;
            P.x[e][o] = eval_normalise(E.snew[e][o], a.use_ob, E.ob_mean[o], E.ob_inv[o]);
        }
        lds_sync();
        policy_forward<PlainTowers>(P, R, EN, prm, L);
        if (owner && alive) {
            float lp;
            const int ai = cat_sample<A>(P.mu[t], true, 0.f, lp);  // the mode: the lowest index among the maxima
            const DstStep o = dst_transition(a.env.max_steps, 0, row, col, cnt, ai);
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += disc * o.obj[k];
            if (o.done) {
                alive = 0;
                E.done[t] = 1;
            } else {
                row = o.row;
                col = o.col;
                cnt = o.step;
#pragma unroll
                for (int j = 0; j < O; ++j) E.snew[t][j] = o.obs[j];
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

static int check_dst_env(const pgm_dst_spec* env, const char* what) {
    if (env->max_steps <= 0) {
        set_error("%s: pgm_dst_spec.max_steps = %d must be positive", what, env->max_steps);
        return PGM_E_INVALID_ARG;
    }
    return PGM_OK;
}

}  // namespace pgm

using namespace pgm;

extern "C" {

// Arguments are validated before any device work: NULL pointers, check_dims, the dim set, LN, T / eval_num, max_steps.
int pgm_rollout_dst(const pgm_dims* d, const float* params, const pgm_dst_spec* env, const pgm_env_state* st,
                    const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* uniforms, uint64_t seed,
                    int32_t carry, pgm_stream_t stream) {
    if (!d || !params || !env || !st || !st->s || !st->obj_acc || !st->obj_acc_valid || !st->ret || !norm_ok(ns) ||
        !rb || !rb->obs || !rb->actions || !rb->logp || !rb->values || !rb->rewards || !rb->masks || !rb->bad_masks) {
        set_error("pgm_rollout_dst: null pointer");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, "pgm_rollout_dst")) return rc;
    if (int rc = check_cat_dims(d, "pgm_rollout_dst")) return rc;
    if (int rc = check_cat_ln(d, "pgm_rollout_dst")) return rc;
    if (d->T <= 0) {
        set_error("pgm_rollout_dst: T must be positive");
        return PGM_E_SHAPE;
    }
    if (int rc = check_dst_env(env, "pgm_rollout_dst")) return rc;
    DstRolloutArgs a{d->P, d->N, d->T, params, *env, *st, *ns, *rb, uniforms, seed, carry};
    return dispatch_towers_cat(d, "pgm_rollout_dst", [&](auto, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(rollout_dst_kernel<O, A, K>, d->P, sizeof(DstSmem<O, A, K>), (hipStream_t)stream,
                           "pgm_rollout_dst", a, L);
    });
}

int pgm_eval_dst(const pgm_dims* d, const float* params, const pgm_dst_spec* env, const double* ob_mean,
                 const double* ob_var, int32_t eval_num, int32_t use_ob_rms, int32_t raw, double gamma,
                 double* objs_out, pgm_stream_t stream) {
    if (!d || !params || !env || !objs_out || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("pgm_eval_dst: null pointer (ob_mean / ob_var are required with use_ob_rms)");
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: the rows are the evaluation episodes
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, "pgm_eval_dst")) return rc;
    if (int rc = check_cat_dims(&dd, "pgm_eval_dst")) return rc;
    if (int rc = check_cat_ln(&dd, "pgm_eval_dst")) return rc;
    if (eval_num < 1 || eval_num > NMAX) {
        set_error("pgm_eval_dst: eval_num=%d evaluation episodes outside [1, %d]", eval_num, NMAX);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dst_env(env, "pgm_eval_dst")) return rc;
    DstEvalArgs a{d->P, params, *env, ob_mean, ob_var, eval_num, use_ob_rms != 0, raw != 0, gamma, objs_out};
    return dispatch_towers_cat(d, "pgm_eval_dst", [&](auto, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(eval_dst_kernel<O, A, K>, d->P, sizeof(DstSmem<O, A, K>), (hipStream_t)stream,
                           "pgm_eval_dst", a, L);
    });
}

// Host only: launches nothing and needs no device.
int pgm_dst_transition(const pgm_dst_spec* spec, int32_t n, const int32_t* row, const int32_t* col,
                       const int32_t* step, const int32_t* action, int32_t* row_out, int32_t* col_out,
                       int32_t* step_out, double* raw_obs_out, double* obj_out, double* reward_out, int32_t* done_out,
                       int32_t* bad_out) {
    if (!spec || n < 0 || !row || !col || !step || !action || !row_out || !col_out || !step_out || !raw_obs_out ||
        !obj_out || !reward_out || !done_out || !bad_out) {
        set_error("pgm_dst_transition: null pointer or negative n");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dst_env(spec, "pgm_dst_transition")) return rc;
    for (int32_t i = 0; i < n; ++i) {
        const DstStep o = dst_transition(spec->max_steps, spec->time_limit_is_bad, row[i], col[i], step[i], action[i]);
        row_out[i] = o.row;
        col_out[i] = o.col;
        step_out[i] = o.step;
        for (int j = 0; j < 3; ++j) raw_obs_out[(size_t)i * 3 + j] = o.obs[j];
        for (int k = 0; k < 2; ++k) obj_out[(size_t)i * 2 + k] = o.obj[k];
        reward_out[i] = o.reward;
        done_out[i] = o.done;
        bad_out[i] = o.bad;
    }
    return PGM_OK;
}

}  // extern "C"
