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
// kernels
struct ActArgs {
    int P, N;
    Layout L;
    const float* params;
    const float* obs;
    const float* noise;
    int deterministic;
    float *value, *action, *logp;
};

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void act_forward_kernel(ActArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x, N = a.N;
    const float* prm = a.params + (size_t)p * a.L.total;
    PolReg<O, A, K> R;
    load_policy(S, prm, a.L);
    load_polreg(R, prm, a.L);
    for (int i = t; i < N * O; i += RT) S.x[i / O][i % O] = a.obs[(size_t)p * N * O + i];
    __syncthreads();
    policy_forward(S, R, N, prm, a.L);
    for (int i = t; i < N * K; i += RT) a.value[(size_t)p * N * K + i] = S.val[i / K][i % K];
    for (int i = t; i < N * A; i += RT) {
        const int n = i / A, j = i % A;
        const float mu = S.mu[n][j], ls = S.logstd[j], sd = expf(ls);
        const float act = a.deterministic ? mu : fmaf(a.noise[i], sd, mu);
        const float dz = (act - mu) / sd;
        S.lp[n][j] = -0.5f * dz * dz - ls - LOG_SQRT_2PI;
        a.action[(size_t)p * N * A + i] = act;
    }
    __syncthreads();
    if (t < N) {
        float s = 0.f;
        for (int j = 0; j < A; ++j) s += S.lp[t][j];
        a.logp[(size_t)p * N + t] = s;
    }
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

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void env_kernel(EnvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N;
    const NormCfg nc = norm_cfg(a.ns);
    const Spec<O, A, K> sp{E, a.spec, a.st.s0};
    load_spec(E, a.spec, a.st.s0, N);
    load_env(E, a.st, a.ns, p, N);
    __syncthreads();
    if (a.reset) {  // fresh make_vec_envs + reset(): vec_normalize.py:10-27,63-66
        if (t < N) {
            E.elapsed[t] = 0;
            E.ret[t] = 0.0;
        }
        if (t == 0) E.obj_valid = 0;
        const double dn = (double)N;
        for (int o = t; o < O; o += RT) {
            double sum = 0.0;
            for (int n = 0; n < N; ++n) {
                const double v = sp.s0(n, o);
                E.snew[n][o] = v;
                E.s[n][o] = v;
                sum += v;
            }
            if (nc.use_ob) {
                const double bm = sum / dn;
                double sq = 0.0;
                for (int n = 0; n < N; ++n) sq += (E.snew[n][o] - bm) * (E.snew[n][o] - bm);
                chan_merge(E.ob_mean[o], E.ob_var[o], E.ob_count, bm, sq / dn, dn);
                E.ob_inv[o] = 1.0 / sqrt(E.ob_var[o] + nc.eps);
            }
        }
        __syncthreads();
        if (t == 0 && nc.use_ob) E.ob_count += dn;
        for (int i = t; i < N * O; i += RT) {
            const int o = i % O;
            double v = E.snew[i / O][o];
            if (nc.use_ob) v = clipd((v - E.ob_mean[o]) * E.ob_inv[o], -nc.clipob, nc.clipob);
            a.obs_out[(size_t)p * N * O + i] = (float)v;
        }
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


template <int O, int A, int K>
__global__ __launch_bounds__(RT) void rollout_kernel(RolloutArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& P = S.pol;
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T;
    const NormCfg nc = norm_cfg(a.ns);
    const Spec<O, A, K> sp{E, a.spec, a.st.s0};
    const float* prm = a.params + (size_t)p * a.L.total;
    float* obs = a.rb.obs + (size_t)p * (T + 1) * N * O;
    float* act = a.rb.actions + (size_t)p * T * N * A;
    float* logp = a.rb.logp + (size_t)p * T * N;
    float* val = a.rb.values + (size_t)p * (T + 1) * N * K;
    float* rew = a.rb.rewards + (size_t)p * T * N * K;
    float* masks = a.rb.masks + (size_t)p * (T + 1) * N;
    float* bad = a.rb.bad_masks + (size_t)p * (T + 1) * N;

    PolReg<O, A, K> R;
    load_policy(P, prm, a.L);
    load_polreg(R, prm, a.L);
    load_spec(E, a.spec, a.st.s0, N);
    load_env(E, a.st, a.ns, p, N);
    if (a.carry) {  // after_update(): slot T -> slot 0 (storage.py:71-75); each thread re-reads its own writes
        for (int i = t; i < N * O; i += RT) obs[i] = obs[(size_t)T * N * O + i];
        if (t < N) {
            masks[t] = masks[(size_t)T * N + t];
            bad[t] = bad[(size_t)T * N + t];
        }
    }
    for (int i = t; i < N * O; i += RT) P.x[i / O][i % O] = obs[i];
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
        policy_forward(P, R, N, prm, a.L);
        PGM_STAMP(1);
        for (int i = t; i < N * K; i += RT) val[(size_t)step * N * K + i] = P.val[i / K][i % K];
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
    policy_forward(P, R, N, prm, a.L);
    for (int i = t; i < N * K; i += RT) val[(size_t)T * N * K + i] = P.val[i / K][i % K];
    __syncthreads();
    store_env(E, a.st, a.ns, p, N);
    PGM_STAMP_FLUSH;
}

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_kernel(EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& P = S.pol;
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x;
    const float* prm = a.params + (size_t)p * a.L.total;
    PolReg<O, A, K> R;
    load_policy(P, prm, a.L);
    load_polreg(R, prm, a.L);
    load_spec(E, a.spec, a.s0_eval, 1);
    for (int o = t; o < O; o += RT) {  // mopg.py:37-38: fp64 normalisation with fixed eps/clip
        E.ob_mean[o] = a.use_ob ? a.ob_mean[(size_t)p * O + o] : 0.0;
        E.ob_inv[o] = a.use_ob ? 1.0 / sqrt(a.ob_var[(size_t)p * O + o] + 1e-8) : 1.0;
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
            for (int o = t; o < O; o += RT) {  // obs is NOT rounded through fp32 before normalising
                double v = E.s[0][o];
                if (a.use_ob) v = clipd((v - E.ob_mean[o]) * E.ob_inv[o], -10.0, 10.0);
                P.x[0][o] = (float)v;
            }
            lds_sync();
            policy_forward(P, R, 1, prm, a.L);
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

// ------------------------------------------------------------------------------------------
// LayerNorm towers (pgm_dims.LN = 1): the kernels above with policy_forward_ln (pgm_policy_dev.hpp)
template <int O, int A, int K>
__global__ __launch_bounds__(RT) void act_forward_ln_kernel(ActArgs a, LayoutLN L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x, N = a.N;
    const float* prm = a.params + (size_t)p * L.total;
    PolRegLN<O, A, K> R;
    load_policy_ln(S, prm, L);
    load_polreg_ln(R, prm, L);
    for (int i = t; i < N * opad<O>(); i += RT) {  // rows zero-padded to the float4 reads of layer 1
        const int n = i / opad<O>(), o = i % opad<O>();
        S.x[n][o] = o < O ? a.obs[((size_t)p * N + n) * O + o] : 0.f;
    }
    __syncthreads();
    policy_forward_ln(S, R, N);
    for (int i = t; i < N * K; i += RT) a.value[(size_t)p * N * K + i] = S.val[i / K][i % K];
    for (int i = t; i < N * A; i += RT) {
        const int n = i / A, j = i % A;
        const float mu = S.mu[n][j], ls = S.logstd[j], sd = expf(ls);
        const float act = a.deterministic ? mu : fmaf(a.noise[i], sd, mu);
        const float dz = (act - mu) / sd;
        S.lp[n][j] = -0.5f * dz * dz - ls - LOG_SQRT_2PI;
        a.action[(size_t)p * N * A + i] = act;
    }
    __syncthreads();
    if (t < N) {
        float s = 0.f;
        for (int j = 0; j < A; ++j) s += S.lp[t][j];
        a.logp[(size_t)p * N + t] = s;
    }
}

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void rollout_ln_kernel(RolloutArgs a, LayoutLN L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& P = S.pol;
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T;
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

    PolRegLN<O, A, K> R;
    load_policy_ln(P, prm, L);
    load_polreg_ln(R, prm, L);
    load_spec(E, a.spec, a.st.s0, N);
    load_env(E, a.st, a.ns, p, N);
    if (a.carry) {  // after_update(): slot T -> slot 0 (storage.py:71-75); each thread re-reads its own writes
        for (int i = t; i < N * O; i += RT) obs[i] = obs[(size_t)T * N * O + i];
        if (t < N) {
            masks[t] = masks[(size_t)T * N + t];
            bad[t] = bad[(size_t)T * N + t];
        }
    }
    for (int i = t; i < NMAX * opad<O>(); i += RT) (&P.x[0][0])[i] = 0.f;  // the float4 pad columns stay zero
    __syncthreads();
    for (int i = t; i < N * O; i += RT) P.x[i / O][i % O] = obs[i];
    __syncthreads();

    // the lane drawing (n, a) of each step keeps its noise one step ahead in a register
    const bool drawer = t < N * A;
    float eps_next = 0.f;
    if (drawer) eps_next = a.noise ? a.noise[t] : counter_normal(a.seed, (uint64_t)t);
    for (int step = 0; step < T; ++step) {
        const float eps = eps_next;
        if (drawer && step + 1 < T) {
            const size_t idx = (size_t)(step + 1) * N * A + t;
            eps_next = a.noise ? a.noise[idx] : counter_normal(a.seed, idx);
        }
        policy_forward_ln(P, R, N);
        for (int i = t; i < N * K; i += RT) val[(size_t)step * N * K + i] = P.val[i / K][i % K];
        sample_actions(P, E, sp, N, eps, act + (size_t)step * N * A);
        if (t < N) {
            float s = 0.f;
            for (int j = 0; j < A; ++j) s += P.lp[t][j];
            logp[(size_t)step * N + t] = s;
        }
        env_dynamics(E, sp, N, a.spec.max_episode_steps);
        vecnorm_stats(E, sp, N, nc);
        vecnorm_emit<O, A, K, opad<O>()>(E, N, nc, P.x, obs + (size_t)(step + 1) * N * O,
                                         rew + (size_t)step * N * K, masks + (size_t)(step + 1) * N,
                                         bad + (size_t)(step + 1) * N);
    }
    // bootstrap value (mopg.py:132-135) -> value_preds[T] (storage.py:85)
    policy_forward_ln(P, R, N);
    for (int i = t; i < N * K; i += RT) val[(size_t)T * N * K + i] = P.val[i / K][i % K];
    __syncthreads();
    store_env(E, a.st, a.ns, p, N);
}

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_ln_kernel(EvalArgs a, LayoutLN L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& P = S.pol;
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x;
    const float* prm = a.params + (size_t)p * L.total;
    PolRegLN<O, A, K> R;
    load_policy_ln(P, prm, L);
    load_polreg_ln(R, prm, L);
    load_spec(E, a.spec, a.s0_eval, 1);
    for (int o = t; o < O; o += RT) {  // mopg.py:37-38: fp64 normalisation with fixed eps/clip
        E.ob_mean[o] = a.use_ob ? a.ob_mean[(size_t)p * O + o] : 0.0;
        E.ob_inv[o] = a.use_ob ? 1.0 / sqrt(a.ob_var[(size_t)p * O + o] + 1e-8) : 1.0;
    }
    if (t < opad<O>()) P.x[0][t] = 0.f;
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
            for (int o = t; o < O; o += RT) {  // obs is NOT rounded through fp32 before normalising
                double v = E.s[0][o];
                if (a.use_ob) v = clipd((v - E.ob_mean[o]) * E.ob_inv[o], -10.0, 10.0);
                P.x[0][o] = (float)v;
            }
            lds_sync();
            policy_forward_ln(P, R, 1);
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
    ActArgs a{d->P, d->N, make_layout(d->O, d->A, d->K, d->H), params, obs, noise, deterministic, value, action, logp};
    if (d->LN) {
        const LayoutLN LL = make_layout_ln(d->O, d->A, d->K, d->H);
        return dispatch_dims_ln(d, "pgm_act_forward", [&](auto o, auto aa, auto k) {
            constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
            return launch_smem_ln(act_forward_ln_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream,
                                  "pgm_act_forward", a, LL);
        });
    }
    return dispatch_dims(d->O, d->A, d->K, "pgm_act_forward", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(act_forward_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_act_forward");
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

int pgm_env_reset(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st,
                  const pgm_norm_state* ns, float* obs_out, pgm_stream_t stream) {
    if (int rc = env_common(d, spec, st, ns, "pgm_env_reset")) return rc;
    if (!obs_out) {
        set_error("pgm_env_reset: null obs_out");
        return PGM_E_INVALID_ARG;
    }
    EnvArgs a{d->P, d->N, *spec, *st, *ns, nullptr, obs_out, nullptr, nullptr, nullptr, 1};
    return dispatch_dims(d->O, d->A, d->K, "pgm_env_reset", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(env_kernel<O, A, K>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_env_reset");
    });
}

int pgm_env_step(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st,
                 const pgm_norm_state* ns, const float* action, float* obs_out, float* reward_out,
                 float* masks_out, float* bad_masks_out, pgm_stream_t stream) {
    if (int rc = env_common(d, spec, st, ns, "pgm_env_step")) return rc;
    if (!action || !obs_out || !reward_out || !masks_out || !bad_masks_out) {
        set_error("pgm_env_step: null pointer");
        return PGM_E_INVALID_ARG;
    }
    EnvArgs a{d->P, d->N, *spec, *st, *ns, action, obs_out, reward_out, masks_out, bad_masks_out, 0};
    return dispatch_dims(d->O, d->A, d->K, "pgm_env_step", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(env_kernel<O, A, K>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_env_step");
    });
}

int pgm_rollout(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const pgm_env_state* st,
                const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* noise, uint64_t seed,
                int32_t carry, const pgm_launch_opts* opts, pgm_stream_t stream) {
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
    RolloutArgs a{d->P, d->N, d->T, make_layout(d->O, d->A, d->K, d->H), params, *spec, *st, *ns, *rb,
                  noise, seed, carry};
    if (d->LN) {  // LayerNorm towers: one kernel family, opts ignored
        const LayoutLN LL = make_layout_ln(d->O, d->A, d->K, d->H);
        return dispatch_dims_ln(d, "pgm_rollout", [&](auto o, auto aa, auto k) {
            constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
            return launch_smem_ln(rollout_ln_kernel<O, A, K>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream,
                                  "pgm_rollout", a, LL);
        });
    }
    const bool block = o.rollout_kernel == 1;  // the workgroup-per-step kernel (A/B, tests)
    if (!block && rollout_lanes_supported(d)) return launch_rollout_lanes(d, a, (hipStream_t)stream);
    if (!block && rollout_wide_supported(d)) return launch_rollout_wide(d, a, (hipStream_t)stream);
    return dispatch_dims(d->O, d->A, d->K, "pgm_rollout", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(rollout_kernel<O, A, K>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_rollout");
    });
}

int pgm_eval(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const double* ob_mean,
             const double* ob_var, const double* s0_eval, int32_t eval_num, int32_t use_ob_rms, int32_t raw,
             double gamma, double* objs_out, const pgm_launch_opts* opts, pgm_stream_t stream) {
    if (int rc = check_dims(d, "pgm_eval")) return rc;
    if (int rc = check_ln(d, "pgm_eval")) return rc;
    pgm_launch_opts o;
    if (int rc = read_opts(opts, &o, "pgm_eval")) return rc;
    if (!params || !spec_ok(spec) || !s0_eval || !objs_out || eval_num <= 0 || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("pgm_eval: bad arguments");
        return PGM_E_INVALID_ARG;
    }
    EvalArgs a{d->P, make_layout(d->O, d->A, d->K, d->H), params, *spec, ob_mean, ob_var, s0_eval,
               eval_num, use_ob_rms, raw, gamma, objs_out};
    if (d->LN) {  // LayerNorm towers: one kernel family, opts ignored
        const LayoutLN LL = make_layout_ln(d->O, d->A, d->K, d->H);
        return dispatch_dims_ln(d, "pgm_eval", [&](auto o, auto aa, auto k) {
            constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
            return launch_smem_ln(eval_ln_kernel<O, A, K>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream,
                                  "pgm_eval", a, LL);
        });
    }
    const bool block = o.eval_kernel == 1;  // the workgroup-per-step kernel (A/B, tests)
    if (!block && eval_waves_supported(d, eval_num)) return launch_eval_waves(d, a, (hipStream_t)stream);
    if (!block && eval_wide_supported(d, eval_num)) return launch_eval_wide(d, a, (hipStream_t)stream);
    return dispatch_dims(d->O, d->A, d->K, "pgm_eval", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(eval_kernel<O, A, K>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_eval");
    });
}
}  // extern "C"
