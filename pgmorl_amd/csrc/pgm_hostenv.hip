// Host-stepped environments (ABI minor 1): pgm_rollout_act, pgm_env_ingest, pgm_eval_act, their discrete-action forms
// pgm_rollout_act_cat / pgm_eval_act_cat and the perf-mode uniform stream pgm_uniform_noise.  The environments run on
// the host; these kernels are the device side of the seam between a host envs.step() and the rollout storage.  The
// towers, the heads and the VecNormalize arithmetic are the device functions of pgm_policy_dev.hpp, shared with the
// fused kernels of pgm_policy_env.hip: each body below is written once for a Towers and a Head type.
//
// Reference semantics (paths relative to the reference tree):
//   Policy.act / get_value of one step     morl/mopg.py:105-108, 132-135; a2c_ppo_acktr/model.py:33-35,57-73
//   DiagGaussian / Categorical             a2c_ppo_acktr/distributions.py:17-40,54-90
//   VecNormalize.step_wait / reset         baselines/common/vec_env/vec_normalize.py:29-66
//   masks / bad_masks / obj_tensor, insert morl/mopg.py:110-130, a2c_ppo_acktr/storage.py:50-62
//   evaluation() normalise + act           morl/mopg.py:36-39
#include "pgm_policy_dev.hpp"

namespace pgm {

// One rollout step is
//   pgm_rollout_act(t) -> host envs.step(action_out) -> pgm_env_ingest(t)
// on the strided slots of the rollout storage: only the seams differ from the fused kernels (one slot per launch,
// transitions supplied instead of computed).
template <class Hd>
struct RolloutActArgs {
    int P, N, T, t;
    const float* params;
    pgm_rollout_buf rb;                 // actions [P][T][N][width]
    const float* rnd;                   // base of [T][N][width]
    typename Hd::action_t* action_out;  // [P][N][width]
};

// values[p][t] always; for t < T the sampled action (storage + action_out) and its log-prob
template <class Tw, class Hd, int O, int A, int K>
__global__ __launch_bounds__(RT) void rollout_act_kernel(RolloutActArgs<Hd> a, typename Tw::Lay L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, N = a.N, T = a.T, st = a.t;
    constexpr int W = Hd::template width<A>;
    const float* prm = a.params + (size_t)p * L.total;
    typename Tw::template Reg<O, A, K> R;
    load_policy<Tw, Hd::has_logstd>(S, R, prm, L);
    load_rows(S, a.rb.obs + ((size_t)p * (T + 1) + st) * N * O, N);
    __syncthreads();
    policy_forward<Tw>(S, R, N, prm, L);
    store_values(S, a.rb.values + ((size_t)p * (T + 1) + st) * N * K, N);
    if (st >= T) return;  // t == T: the bootstrap get_value only (uniform over the grid)
    Hd::emit(S, N, a.rnd + (size_t)st * N * W, a.rb.actions + ((size_t)p * T + st) * N * W,
             a.action_out + (size_t)p * N * W, a.rb.logp + ((size_t)p * T + st) * N);
}

template <class Hd>
struct EvalActArgs {
    int P, E;
    const float* params;
    const double *ob_mean, *ob_var, *raw_obs;  // [P][O], [P][O], [P][E][O]
    int use_ob;
    typename Hd::action_t* action_out;  // [P][E][width]
};

// mopg.py:36-39: the frozen-statistics normalisation of E raw observations per task, then the mode of the head
template <class Tw, class Hd, int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_act_kernel(EvalActArgs<Hd> a, typename Tw::Lay L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x;
    const float* prm = a.params + (size_t)p * L.total;
    typename Tw::template Reg<O, A, K> R;
    load_policy<Tw, Hd::has_logstd>(S, R, prm, L);
    for (int i = threadIdx.x; i < a.E * O; i += RT) {
        const int e = i / O, o = i % O;
        const size_t q = (size_t)p * O + o;
        S.x[e][o] = eval_normalise(a.raw_obs[((size_t)p * a.E + e) * O + o], a.use_ob, a.use_ob ? a.ob_mean[q] : 0.0,
                                   a.use_ob ? eval_ob_inv(a.ob_var[q]) : 1.0);
    }
    __syncthreads();
    policy_forward<Tw>(S, R, a.E, prm, L);
    Hd::emit(S, a.E, nullptr, nullptr, a.action_out + (size_t)p * a.E * Hd::template width<A>, nullptr);
}

struct IngestArgs {
    int P, N, T, t;  // t = -1: reset
    pgm_env_state st;
    pgm_norm_state ns;
    pgm_rollout_buf rb;
    const double *raw_obs, *raw_obj, *reward;  // [P][N][O], [P][N][K], [P][N]
    const int32_t *done, *bad;                 // [P][N]
};

// The VecNormalize step of supplied transitions: no auto-reset (the host's vec env has done it) and the env's scalar
// reward in VecNormalize.ret (vec_normalize.py:32,41-43); the thread roles and arithmetic of the fused step.
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
    load_env<false>(E, a.st, a.ns, p, N);
    for (int i = t; i < N * O; i += RT) E.snew[i / O][i % O] = a.raw_obs[(size_t)p * N * O + i];
    if (a.t >= 0) {
        for (int i = t; i < N * K; i += RT) E.objraw[i / K][i % K] = a.raw_obj[(size_t)p * N * K + i];
        if (t < N) {
            E.done[t] = a.done[p * N + t] != 0;
            E.bad[t] = a.bad[p * N + t] != 0;
        }
    }
    __syncthreads();
    if (a.t < 0) {
        vecnorm_reset(E, N, nc, obs);
        if (t < N) {
            masks[t] = 1.f;
            bad[t] = 1.f;
        }
    } else {
        norm_stats(E, N, nc, a.reward + (size_t)p * N);
        vecnorm_emit<O, A, K, opad<O>()>(E, N, nc, S.pol.x, obs + (size_t)(a.t + 1) * N * O,
                                         a.rb.rewards + ((size_t)p * T + a.t) * N * K,
                                         masks + (size_t)(a.t + 1) * N, bad + (size_t)(a.t + 1) * N);
    }
    __syncthreads();
    store_env<false>(E, a.st, a.ns, p, N);
}

// element i of the perf-mode uniform stream (counter_uniform, pgm_common.hpp: shared with the fused DST rollout)
__global__ void uniform_kernel(int64_t n, uint64_t seed, float* out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = counter_uniform(seed, (uint64_t)i);
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
    RolloutActArgs<GaussHead> a{d->P, d->N, d->T, t, params, *rb, noise, action_out};
    return dispatch_towers(d, "pgm_rollout_act", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(rollout_act_kernel<decltype(tw), GaussHead, O, A, K>, d->P, sizeof(PolSmem<O, A, K>),
                           (hipStream_t)stream, "pgm_rollout_act", a, L);
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
        return launch_smem(env_ingest_kernel<O, A, K>, d->P, sizeof(StepSmem<O, A, K>), (hipStream_t)stream,
                           "pgm_env_ingest", a);
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
    EvalActArgs<GaussHead> a{d->P, E, params, ob_mean, ob_var, raw_obs, use_ob_rms != 0, action_out};
    return dispatch_towers(d, "pgm_eval_act", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(eval_act_kernel<decltype(tw), GaussHead, O, A, K>, d->P, sizeof(PolSmem<O, A, K>),
                           (hipStream_t)stream, "pgm_eval_act", a, L);
    });
}

// ---- discrete-action policies.  NULL pointers, check_dims, the dim set, the step index or E, LN.
int pgm_rollout_act_cat(const pgm_dims* d, const float* params, const pgm_rollout_buf* rb, int32_t t,
                        const float* uniforms, int32_t* action_out, pgm_stream_t stream) {
    if (!d || !params || !rb || !rb->obs || !rb->actions || !rb->logp || !rb->values) {
        set_error("pgm_rollout_act_cat: null pointer");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, "pgm_rollout_act_cat")) return rc;
    if (int rc = check_cat_dims(d, "pgm_rollout_act_cat")) return rc;
    if (t < 0 || t > d->T) {
        set_error("pgm_rollout_act_cat: step t=%d outside [0, T=%d]", t, d->T);
        return PGM_E_SHAPE;
    }
    if (t < d->T && (!uniforms || !action_out)) {
        set_error("pgm_rollout_act_cat: uniforms and action_out are required for t < T");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_cat_ln(d, "pgm_rollout_act_cat")) return rc;
    RolloutActArgs<CatHead> a{d->P, d->N, d->T, t, params, *rb, uniforms, action_out};
    return dispatch_towers_cat(d, "pgm_rollout_act_cat", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(rollout_act_kernel<decltype(tw), CatHead, O, A, K>, d->P, sizeof(PolSmem<O, A, K>),
                           (hipStream_t)stream, "pgm_rollout_act_cat", a, L);
    });
}

int pgm_eval_act_cat(const pgm_dims* d, const float* params, const double* ob_mean, const double* ob_var,
                     int32_t use_ob_rms, const double* raw_obs, int32_t E, int32_t* action_out, pgm_stream_t stream) {
    if (!d || !params || !raw_obs || !action_out || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("pgm_eval_act_cat: null pointer (ob_mean / ob_var are required with use_ob_rms)");
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: the rows are the E evaluation episodes
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, "pgm_eval_act_cat")) return rc;
    if (int rc = check_cat_dims(&dd, "pgm_eval_act_cat")) return rc;
    if (E < 1 || E > NMAX) {
        set_error("pgm_eval_act_cat: E=%d evaluation episodes outside [1, %d]", E, NMAX);
        return PGM_E_SHAPE;
    }
    if (int rc = check_cat_ln(&dd, "pgm_eval_act_cat")) return rc;
    EvalActArgs<CatHead> a{d->P, E, params, ob_mean, ob_var, raw_obs, use_ob_rms != 0, action_out};
    return dispatch_towers_cat(d, "pgm_eval_act_cat", [&](auto tw, const auto& L, auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(eval_act_kernel<decltype(tw), CatHead, O, A, K>, d->P, sizeof(PolSmem<O, A, K>),
                           (hipStream_t)stream, "pgm_eval_act_cat", a, L);
    });
}

int pgm_uniform_noise(int64_t n, uint64_t seed, float* out, pgm_stream_t stream) {
    if (!out || n < 0) {
        set_error("pgm_uniform_noise: bad arguments");
        return PGM_E_INVALID_ARG;
    }
    if (n == 0) return PGM_OK;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(uniform_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n, seed, out);
    return launch_status("pgm_uniform_noise");
}

}  // extern "C"
