// Host-stepped environments (ABI minor 1): pgm_rollout_act, pgm_env_ingest, pgm_eval_act.  The environments run on the
// host; these kernels are the device side of the seam between a host envs.step() and the rollout storage.  The forwards
// and the VecNormalize arithmetic are the device functions of pgm_policy_dev.hpp, shared with the fused kernels of
// pgm_policy_env.hip; a translation unit of its own keeps that unit's code object as it was.
//
// Reference semantics (paths relative to the reference tree):
//   Policy.act / get_value of one step     morl/mopg.py:105-108, 132-135
//   VecNormalize.step_wait / reset         baselines/common/vec_env/vec_normalize.py:29-66
//   masks / bad_masks / obj_tensor, insert morl/mopg.py:110-130, a2c_ppo_acktr/storage.py:50-62
//   evaluation() normalise + act           morl/mopg.py:36-39
#include "pgm_policy_dev.hpp"

namespace pgm {

// One rollout step is
//   pgm_rollout_act(t) -> host envs.step(action_out) -> pgm_env_ingest(t)
// on the strided slots of the rollout storage: only the seams differ from the fused kernels (one slot per launch,
// transitions supplied instead of computed).
struct RolloutActArgs {
    int P, N, T, t;
    Layout L;
    const float* params;
    pgm_rollout_buf rb;
    const float* noise;  // base of [T][N][A]
    float* action_out;   // [P][N][A]
};

// values[p][t] always; for t < T the sampled action (storage + action_out) and its log-prob.  S.val / S.mu filled.
template <int O, int A, int K>
__device__ void rollout_act_emit(PolSmem<O, A, K>& S, const RolloutActArgs& a, int p) {
    const int t = threadIdx.x, N = a.N, T = a.T, st = a.t;
    float* val = a.rb.values + ((size_t)p * (T + 1) + st) * N * K;
    for (int i = t; i < N * K; i += RT) val[i] = S.val[i / K][i % K];
    if (st >= T) return;  // t == T: the bootstrap get_value only (uniform over the grid)
    const float* nz = a.noise + (size_t)st * N * A;
    float* act = a.rb.actions + ((size_t)p * T + st) * N * A;
    for (int i = t; i < N * A; i += RT) {
        const int n = i / A, j = i % A;
        const float mu = S.mu[n][j], ls = S.logstd[j], sd = expf(ls);
        const float av = fmaf(nz[i], sd, mu);
        const float dz = (av - mu) / sd;
        S.lp[n][j] = -0.5f * dz * dz - ls - LOG_SQRT_2PI;
        act[i] = av;
        a.action_out[(size_t)p * N * A + i] = av;  // raw, unclipped: the env clips (as the reference's does)
    }
    __syncthreads();
    if (t < N) {
        float s = 0.f;
        for (int j = 0; j < A; ++j) s += S.lp[t][j];
        a.rb.logp[((size_t)p * T + st) * N + t] = s;
    }
}

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void rollout_act_kernel(RolloutActArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x, N = a.N;
    const float* prm = a.params + (size_t)p * a.L.total;
    const float* obs = a.rb.obs + ((size_t)p * (a.T + 1) + a.t) * N * O;
    PolReg<O, A, K> R;
    load_policy(S, prm, a.L);
    load_polreg(R, prm, a.L);
    for (int i = t; i < N * O; i += RT) S.x[i / O][i % O] = obs[i];
    __syncthreads();
    policy_forward(S, R, N, prm, a.L);
    rollout_act_emit(S, a, p);
}

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void rollout_act_ln_kernel(RolloutActArgs a, LayoutLN L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x, N = a.N;
    const float* prm = a.params + (size_t)p * L.total;
    const float* obs = a.rb.obs + ((size_t)p * (a.T + 1) + a.t) * N * O;
    PolRegLN<O, A, K> R;
    load_policy_ln(S, prm, L);
    load_polreg_ln(R, prm, L);
    for (int i = t; i < N * opad<O>(); i += RT) {  // rows zero-padded to the float4 reads of layer 1
        const int n = i / opad<O>(), o = i % opad<O>();
        S.x[n][o] = o < O ? obs[n * O + o] : 0.f;
    }
    __syncthreads();
    policy_forward_ln(S, R, N);
    rollout_act_emit(S, a, p);
}

struct EvalActArgs {
    int P, E;
    Layout L;
    const float* params;
    const double *ob_mean, *ob_var, *raw_obs;  // [P][O], [P][O], [P][E][O]
    int use_ob;
    float* action_out;  // [P][E][A]
};

// mopg.py:36-38: fp64 normalisation of the raw observation with the frozen statistics, fixed eps / clip, then the
// fp32 cast (the observation is never rounded to fp32 first, as in eval_kernel).  PAD: zero the float4 pad columns.
template <int O, int A, int K, bool PAD>
__device__ void eval_act_load(PolSmem<O, A, K>& S, const EvalActArgs& a, int p) {
    constexpr int OW = PAD ? opad<O>() : O;
    for (int i = threadIdx.x; i < a.E * OW; i += RT) {
        const int e = i / OW, o = i % OW;
        float f = 0.f;
        if (o < O) {
            double v = a.raw_obs[((size_t)p * a.E + e) * O + o];
            if (a.use_ob) {
                const double inv = 1.0 / sqrt(a.ob_var[(size_t)p * O + o] + 1e-8);
                v = clipd((v - a.ob_mean[(size_t)p * O + o]) * inv, -10.0, 10.0);
            }
            f = (float)v;
        }
        S.x[e][o] = f;
    }
}

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_act_kernel(EvalActArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x;
    const float* prm = a.params + (size_t)p * a.L.total;
    PolReg<O, A, K> R;
    load_policy(S, prm, a.L);
    load_polreg(R, prm, a.L);
    eval_act_load<O, A, K, false>(S, a, p);
    __syncthreads();
    policy_forward(S, R, a.E, prm, a.L);
    for (int i = t; i < a.E * A; i += RT) a.action_out[(size_t)p * a.E * A + i] = S.mu[i / A][i % A];  // dist.mean
}

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_act_ln_kernel(EvalActArgs a, LayoutLN L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x;
    const float* prm = a.params + (size_t)p * L.total;
    PolRegLN<O, A, K> R;
    load_policy_ln(S, prm, L);
    load_polreg_ln(R, prm, L);
    eval_act_load<O, A, K, true>(S, a, p);
    __syncthreads();
    policy_forward_ln(S, R, a.E);
    for (int i = t; i < a.E * A; i += RT) a.action_out[(size_t)p * a.E * A + i] = S.mu[i / A][i % A];
}

struct IngestArgs {
    int P, N, T, t;  // t = -1: reset
    pgm_env_state st;
    pgm_norm_state ns;
    pgm_rollout_buf rb;
    const double *raw_obs, *raw_obj, *reward;  // [P][N][O], [P][N][K], [P][N]
    const int32_t *done, *bad;                 // [P][N]
};

// load_env / store_env without the synthetic env's own state (st.s, st.elapsed, st.s0 may be NULL here)
template <int O, int A, int K>
__device__ void load_ingest(EnvSmem<O, A, K>& E, const pgm_env_state& st, const pgm_norm_state& ns, int p, int N) {
    const int t = threadIdx.x;
    for (int i = t; i < N * K; i += RT) E.obj_acc[i / K][i % K] = st.obj_acc[(size_t)p * N * K + i];
    if (t < N) E.ret[t] = st.ret[p * N + t];
    for (int o = t; o < O; o += RT) {
        E.ob_mean[o] = ns.ob_mean[(size_t)p * O + o];
        E.ob_var[o] = ns.ob_var[(size_t)p * O + o];
    }
    if (t < K) {
        E.obj_mean[t] = ns.obj_mean[p * K + t];
        E.obj_var[t] = ns.obj_var[p * K + t];
    }
    if (t == 0) {
        E.ob_count = ns.ob_count[p];
        E.obj_count = ns.obj_count[p];
        E.ret_mean = ns.ret_mean[p];
        E.ret_var = ns.ret_var[p];
        E.ret_count = ns.ret_count[p];
        E.obj_valid = st.obj_acc_valid[p];
    }
}

template <int O, int A, int K>
__device__ void store_ingest(const EnvSmem<O, A, K>& E, const pgm_env_state& st, const pgm_norm_state& ns, int p,
                             int N) {
    const int t = threadIdx.x;
    for (int i = t; i < N * K; i += RT) st.obj_acc[(size_t)p * N * K + i] = E.obj_acc[i / K][i % K];
    if (t < N) st.ret[p * N + t] = E.ret[t];
    for (int o = t; o < O; o += RT) {
        ns.ob_mean[(size_t)p * O + o] = E.ob_mean[o];
        ns.ob_var[(size_t)p * O + o] = E.ob_var[o];
    }
    if (t < K) {
        ns.obj_mean[p * K + t] = E.obj_mean[t];
        ns.obj_var[p * K + t] = E.obj_var[t];
    }
    if (t == 0) {
        ns.ob_count[p] = E.ob_count;
        ns.obj_count[p] = E.obj_count;
        ns.ret_mean[p] = E.ret_mean;
        ns.ret_var[p] = E.ret_var;
        ns.ret_count[p] = E.ret_count;
        st.obj_acc_valid[p] = E.obj_valid;
    }
}

// ob_rms over the N rows of E.snew (the vec env's returned observations: already the reset observation of a done
// env), with the count from before this step.  use_ob only.
template <int O, int A, int K>
__device__ void ingest_ob_stats(EnvSmem<O, A, K>& E, int N, const NormCfg& nc) {
    const double dn = (double)N;
    const bool pow2 = (N & (N - 1)) == 0;  // the divide rule of vecnorm_stats
    const double rn = 1.0 / dn;
    auto divn = [&](double x) { return pow2 ? x * rn : x / dn; };
    for (int o = threadIdx.x; o < O; o += RT) {
        double sum = 0.0;
        for (int n = 0; n < N; ++n) sum += E.snew[n][o];
        const double bm = divn(sum);
        double sq = 0.0;
        for (int n = 0; n < N; ++n) {
            const double dd = E.snew[n][o] - bm;
            sq += dd * dd;
        }
        chan_merge(E.ob_mean[o], E.ob_var[o], E.ob_count, bm, divn(sq), dn);
        E.ob_inv[o] = 1.0 / sqrt(E.ob_var[o] + nc.eps);
    }
}

// vecnorm_stats for supplied transitions: no auto-reset (the host's vec env has done it) and the env's scalar reward
// in VecNormalize.ret (vec_normalize.py:32,41-43).  Same thread roles, same arithmetic, one barrier.
template <int O, int A, int K>
__device__ void ingest_stats(EnvSmem<O, A, K>& E, int N, const NormCfg& nc, const double* __restrict__ reward) {
    const int t = threadIdx.x;
    const double dn = (double)N;
    const bool pow2 = (N & (N - 1)) == 0;
    const double rn = 1.0 / dn;
    auto divn = [&](double x) { return pow2 ? x * rn : x / dn; };
    if (nc.use_ob) ingest_ob_stats(E, N, nc);
    const int k = RT - 1 - t;
    if (k < K) {
        for (int n = 0; n < N; ++n)
            E.obj_acc[n][k] = E.obj_valid ? E.obj_acc[n][k] * nc.gamma + E.objraw[n][k] : E.objraw[n][k];
        if (nc.use_obj) {
            double sum = 0.0;
            for (int n = 0; n < N; ++n) sum += E.obj_acc[n][k];
            const double bm = divn(sum);
            double sq = 0.0;
            for (int n = 0; n < N; ++n) {
                const double dd = E.obj_acc[n][k] - bm;
                sq += dd * dd;
            }
            chan_merge(E.obj_mean[k], E.obj_var[k], E.obj_count, bm, divn(sq), dn);
            E.obj_inv[k] = 1.0 / sqrt(E.obj_var[k] + nc.eps);
        }
    }
    if (t == RT - 1 - K) {
        double sum = 0.0;
        for (int n = 0; n < N; ++n) {
            E.ret[n] = E.ret[n] * nc.gamma + reward[n];
            sum += E.ret[n];
        }
        const double bm = divn(sum);
        double sq = 0.0;
        for (int n = 0; n < N; ++n) sq += (E.ret[n] - bm) * (E.ret[n] - bm);
        chan_merge(E.ret_mean, E.ret_var, E.ret_count, bm, divn(sq), dn);
        E.ret_count += dn;
    }
    lds_sync();
}

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void env_ingest_kernel(IngestArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& E = S.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T;
    const NormCfg nc = norm_cfg(a.ns);
    float* obs = a.rb.obs + (size_t)p * (T + 1) * N * O;
    float* masks = a.rb.masks + (size_t)p * (T + 1) * N;
    float* bad = a.rb.bad_masks + (size_t)p * (T + 1) * N;
    load_ingest(E, a.st, a.ns, p, N);
    for (int i = t; i < N * O; i += RT) E.snew[i / O][i % O] = a.raw_obs[(size_t)p * N * O + i];
    if (a.t >= 0) {
        for (int i = t; i < N * K; i += RT) E.objraw[i / K][i % K] = a.raw_obj[(size_t)p * N * K + i];
        if (t < N) {
            E.done[t] = a.done[p * N + t] != 0;
            E.bad[t] = a.bad[p * N + t] != 0;
        }
    }
    __syncthreads();
    if (a.t < 0) {  // fresh make_vec_envs + reset(): vec_normalize.py:10-27,63-66
        if (t < N) E.ret[t] = 0.0;
        if (t == 0) E.obj_valid = 0;
        if (nc.use_ob) ingest_ob_stats(E, N, nc);
        __syncthreads();
        if (t == 0 && nc.use_ob) E.ob_count += (double)N;
        for (int i = t; i < N * O; i += RT) {
            const int o = i % O;
            double v = E.snew[i / O][o];
            if (nc.use_ob) v = clipd((v - E.ob_mean[o]) * E.ob_inv[o], -nc.clipob, nc.clipob);
            obs[i] = (float)v;
        }
        if (t < N) {
            masks[t] = 1.f;
            bad[t] = 1.f;
        }
    } else {
        ingest_stats(E, N, nc, a.reward + (size_t)p * N);
        vecnorm_emit<O, A, K, opad<O>()>(E, N, nc, S.pol.x, obs + (size_t)(a.t + 1) * N * O,
                                         a.rb.rewards + ((size_t)p * T + a.t) * N * K,
                                         masks + (size_t)(a.t + 1) * N, bad + (size_t)(a.t + 1) * N);
    }
    __syncthreads();
    store_ingest(E, a.st, a.ns, p, N);
}


}  // namespace pgm

using namespace pgm;

extern "C" {

// ---- host-stepped environments (ABI minor 1).  Arguments are validated before any device work: NULL pointers,
// then check_dims, then check_ln, then the step index.
int pgm_rollout_act(const pgm_dims* d, const float* params, const pgm_rollout_buf* rb, int32_t t, const float* noise,
                    float* action_out, pgm_stream_t stream) {
    if (!d || !params || !rb || !rb->obs || !rb->actions || !rb->logp || !rb->values) {
        set_error("pgm_rollout_act: null pointer");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, "pgm_rollout_act")) return rc;
    if (int rc = check_ln(d, "pgm_rollout_act")) return rc;
    if (t < 0 || t > d->T) {
        set_error("pgm_rollout_act: step t=%d outside [0, T=%d]", t, d->T);
        return PGM_E_SHAPE;
    }
    if (t < d->T && (!noise || !action_out)) {
        set_error("pgm_rollout_act: noise and action_out are required for t < T");
        return PGM_E_INVALID_ARG;
    }
    RolloutActArgs a{d->P, d->N, d->T, t, make_layout(d->O, d->A, d->K, d->H), params, *rb, noise, action_out};
    if (d->LN) {
        const LayoutLN LL = make_layout_ln(d->O, d->A, d->K, d->H);
        return dispatch_dims_ln(d, "pgm_rollout_act", [&](auto o, auto aa, auto k) {
            constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
            return launch_smem_ln(rollout_act_ln_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream,
                                  "pgm_rollout_act", a, LL);
        });
    }
    return dispatch_dims(d->O, d->A, d->K, "pgm_rollout_act", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(rollout_act_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_rollout_act");
    });
}

int pgm_env_ingest(const pgm_dims* d, const pgm_env_state* st, const pgm_norm_state* ns, const pgm_rollout_buf* rb,
                   int32_t t, const double* raw_obs, const double* raw_obj, const double* reward, const int32_t* done,
                   const int32_t* bad_transition, pgm_stream_t stream) {
    if (!d || !st || !st->obj_acc || !st->obj_acc_valid || !st->ret || !norm_ok(ns) || !rb || !rb->obs ||
        !rb->rewards || !rb->masks || !rb->bad_masks || !raw_obs) {
        set_error("pgm_env_ingest: null pointer");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, "pgm_env_ingest")) return rc;
    if (int rc = check_ln(d, "pgm_env_ingest")) return rc;
    if (t < -1 || t >= d->T) {
        set_error("pgm_env_ingest: step t=%d outside [-1, T=%d)", t, d->T);
        return PGM_E_SHAPE;
    }
    if (t >= 0 && (!raw_obj || !reward || !done || !bad_transition)) {
        set_error("pgm_env_ingest: raw_obj, reward, done and bad_transition are required for t >= 0");
        return PGM_E_INVALID_ARG;
    }
    IngestArgs a{d->P, d->N, d->T, t, *st, *ns, *rb, raw_obs, raw_obj, reward, done, bad_transition};
    auto launch = [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(env_ingest_kernel<O, A, K>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_env_ingest");
    };
    // the ingest never reads the action: the discrete-action dim sets (A = number of actions) share the kernel
    if (is_cat_dims(d->O, d->A, d->K)) return dispatch_dims_cat(d->O, d->A, d->K, "pgm_env_ingest", launch);
    return dispatch_dims(d->O, d->A, d->K, "pgm_env_ingest", launch);
}

int pgm_eval_act(const pgm_dims* d, const float* params, const double* ob_mean, const double* ob_var,
                 int32_t use_ob_rms, const double* raw_obs, int32_t E, float* action_out, pgm_stream_t stream) {
    if (!d || !params || !raw_obs || !action_out || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("pgm_eval_act: null pointer (ob_mean / ob_var are required with use_ob_rms)");
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: the rows are the E evaluation episodes
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, "pgm_eval_act")) return rc;
    if (int rc = check_ln(&dd, "pgm_eval_act")) return rc;
    if (E < 1 || E > NMAX) {
        set_error("pgm_eval_act: E=%d evaluation episodes outside [1, %d]", E, NMAX);
        return PGM_E_SHAPE;
    }
    EvalActArgs a{d->P, E, make_layout(d->O, d->A, d->K, d->H), params, ob_mean, ob_var, raw_obs, use_ob_rms != 0,
                  action_out};
    if (d->LN) {
        const LayoutLN LL = make_layout_ln(d->O, d->A, d->K, d->H);
        return dispatch_dims_ln(d, "pgm_eval_act", [&](auto o, auto aa, auto k) {
            constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
            return launch_smem_ln(eval_act_ln_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream,
                                  "pgm_eval_act", a, LL);
        });
    }
    return dispatch_dims(d->O, d->A, d->K, "pgm_eval_act", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(eval_act_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_eval_act");
    });
}


}  // extern "C"
