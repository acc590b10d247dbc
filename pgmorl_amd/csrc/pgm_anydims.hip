// Host-stepped environments of any dims (pgm_abi_feature_mask() & PGM_FEATURE_ANY_DIMS): pgm_rollout_act_any,
// pgm_eval_act_any, pgm_env_ingest_any.  The kernels of pgm_hostenv.hip compiled once for the maximum dims
// (OM, AM, KM) = (32, 8, 3) and launched with the true dims (o, a, k): the LDS and register images are zero-padded past
// the true dims, every stride into global memory is a true dim, and a padding slot is never stored.  Plain towers,
// Gaussian (head 0) or Categorical (head 1) head.
//
// The policy forward is policy_forward<PlainTowers, OM, AM, KM> itself on zero-padded images: the layer-1 chain ends
// with fma(0, 0, acc) = acc, so its results are those of the kernels compiled for (o, a, k); the head sums of the
// padding outputs are computed and never read.  The heads and the VecNormalize step are restated below with runtime
// loop bounds, operation for operation those of GaussHead / CatHead::emit and norm_stats / vecnorm_emit /
// vecnorm_reset (pgm_policy_dev.hpp), which they must keep matching.
#include "pgm_anydims.hpp"
#include "pgm_policy_dev.hpp"

namespace pgm {

using PolAny = PolSmem<OM, AM, KM>;
using EnvAny = EnvSmem<OM, AM, KM>;
using RegAny = PolReg<OM, AM, KM>;

struct AnyDims {
    int o, a, k;
};

// the task's weights -> zero-padded registers / LDS (PlainTowers::load_reg / load_smem with the true strides)
template <bool LOGSTD>
__device__ void load_policy_any(PolAny& S, RegAny& R, const float* __restrict__ prm, const Layout& L, AnyDims d) {
    const int t = threadIdx.x, lane = t & 63, m = (t >> 6) & 1;
    const int offW1 = m == 0 ? L.off[PGM_P_CRITIC_W1] : L.off[PGM_P_ACTOR_W1];
    const int offW2 = m == 0 ? L.off[PGM_P_CRITIC_W2] : L.off[PGM_P_ACTOR_W2];
#pragma unroll
    for (int i = 0; i < OM; ++i) R.w1[i] = i < d.o ? prm[offW1 + i * H + lane] : 0.f;
#pragma unroll
    for (int i = 0; i < H; ++i) R.w2[i] = prm[offW2 + i * H + lane];
#pragma unroll
    for (int q = 0; q < AM; ++q)
        R.wh[q] = m == 0 ? (q < d.k ? prm[L.off[PGM_P_VALUE_W] + lane * d.k + q] : 0.f)
                         : (q < d.a ? prm[L.off[PGM_P_MEAN_W] + lane * d.a + q] : 0.f);
    R.b1 = prm[(m == 0 ? L.off[PGM_P_CRITIC_B1] : L.off[PGM_P_ACTOR_B1]) + lane];
    R.b2 = prm[(m == 0 ? L.off[PGM_P_CRITIC_B2] : L.off[PGM_P_ACTOR_B2]) + lane];
    if (t < KM) S.bv[t] = t < d.k ? prm[L.off[PGM_P_VALUE_B] + t] : 0.f;
    if (t < AM) {
        S.bm[t] = t < d.a ? prm[L.off[PGM_P_MEAN_B] + t] : 0.f;
        S.logstd[t] = LOGSTD && t < d.a ? prm[L.off[PGM_P_LOGSTD] + t] : 0.f;
    }
}

// DiagGaussian: GaussHead::emit over the true action dims
struct GaussHeadAny {
    using action_t = float;
    static constexpr bool has_logstd = true;
    static __device__ int width(int a) { return a; }
    static __device__ void emit(PolAny& S, int n, int a, const float* rnd, float* storage, float* out, float* logp) {
        const int t = threadIdx.x;
        for (int i = t; i < n * a; i += RT) {
            const int r = i / a, j = i % a;
            const float mu = S.mu[r][j], ls = S.logstd[j], sd = expf(ls);
            const float av = rnd ? fmaf(rnd[i], sd, mu) : mu;
            if (logp) S.lp[r][j] = gauss_logp_term(av, mu, ls, sd);
            if (storage) storage[i] = av;
            out[i] = av;
        }
        if (!logp) return;  // uniform over the grid
        __syncthreads();
        if (t < n) {
            float s = 0.f;
            for (int j = 0; j < a; ++j) s += S.lp[t][j];
            logp[t] = s;
        }
    }
};

// cat_sample on the first a logits of a row
__device__ __forceinline__ int cat_sample_any(const float* z, int a, bool deterministic, float u, float& logp) {
    float m = z[0];
    int am = 0;
#pragma unroll
    for (int j = 1; j < AM; ++j)
        if (j < a && z[j] > m) {  // strict: the lowest index among the maxima
            m = z[j];
            am = j;
        }
    float e[AM], s = 0.f;
#pragma unroll
    for (int j = 0; j < AM; ++j) {
        e[j] = 0.f;
        if (j < a) {
            e[j] = expf(z[j] - m);
            s += e[j];
        }
    }
    int act = am;
    if (!deterministic) {
        float c = 0.f;
        act = 0;
#pragma unroll
        for (int j = 0; j < AM - 1; ++j)
            if (j < a - 1) {
                c += e[j] / s;
                act += c <= u ? 1 : 0;
            }
    }
    float za = z[0];
#pragma unroll
    for (int j = 1; j < AM; ++j) za = act == j ? z[j] : za;
    logp = za - (m + logf(s));
    return act;
}

struct CatHeadAny {
    using action_t = int32_t;
    static constexpr bool has_logstd = false;
    static __device__ int width(int) { return 1; }
    static __device__ void emit(PolAny& S, int n, int a, const float* rnd, float* storage, int32_t* out, float* logp) {
        const int t = threadIdx.x;
        if (t < n) {
            float lp;
            const int act = cat_sample_any(S.mu[t], a, rnd == nullptr, rnd ? rnd[t] : 0.f, lp);
            if (storage) storage[t] = (float)act;
            out[t] = act;
            if (logp) logp[t] = lp;
        }
    }
};

template <class Hd>
struct RolloutActAnyArgs {
    int P, N, T, t;
    AnyDims d;
    const float* params;
    pgm_rollout_buf rb;
    const float* rnd;
    typename Hd::action_t* action_out;
};

// rollout_act_kernel (pgm_hostenv.hip) at runtime dims
template <class Hd>
__global__ __launch_bounds__(RT) void rollout_act_any_kernel(RolloutActAnyArgs<Hd> a, Layout L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolAny*>(smem_raw);
    const int p = blockIdx.x, N = a.N, T = a.T, st = a.t, o = a.d.o, k = a.d.k, W = Hd::width(a.d.a);
    const float* prm = a.params + (size_t)p * L.total;
    RegAny R;
    load_policy_any<Hd::has_logstd>(S, R, prm, L, a.d);
    const float* rows = a.rb.obs + ((size_t)p * (T + 1) + st) * N * o;
    for (int i = threadIdx.x; i < N * OM; i += RT) {
        const int r = i / OM, c = i % OM;
        S.x[r][c] = c < o ? rows[r * o + c] : 0.f;
    }
    __syncthreads();
    policy_forward<PlainTowers>(S, R, N, prm, L);
    float* val = a.rb.values + ((size_t)p * (T + 1) + st) * N * k;
    for (int i = threadIdx.x; i < N * k; i += RT) val[i] = S.val[i / k][i % k];
    if (st >= T) return;  // t == T: the bootstrap get_value only (uniform over the grid)
    Hd::emit(S, N, a.d.a, a.rnd + (size_t)st * N * W, a.rb.actions + ((size_t)p * T + st) * N * W,
             a.action_out + (size_t)p * N * W, a.rb.logp + ((size_t)p * T + st) * N);
}

template <class Hd>
struct EvalActAnyArgs {
    int P, E;
    AnyDims d;
    const float* params;
    const double *ob_mean, *ob_var, *raw_obs;
    int use_ob;
    typename Hd::action_t* action_out;
};

// eval_act_kernel (pgm_hostenv.hip) at runtime dims
template <class Hd>
__global__ __launch_bounds__(RT) void eval_act_any_kernel(EvalActAnyArgs<Hd> a, Layout L) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolAny*>(smem_raw);
    const int p = blockIdx.x, o = a.d.o;
    const float* prm = a.params + (size_t)p * L.total;
    RegAny R;
    load_policy_any<Hd::has_logstd>(S, R, prm, L, a.d);
    for (int i = threadIdx.x; i < a.E * OM; i += RT) {
        const int e = i / OM, c = i % OM;
        float v = 0.f;
        if (c < o) {
            const size_t q = (size_t)p * o + c;
            v = eval_normalise(a.raw_obs[((size_t)p * a.E + e) * o + c], a.use_ob, a.use_ob ? a.ob_mean[q] : 0.0,
                               a.use_ob ? eval_ob_inv(a.ob_var[q]) : 1.0);
        }
        S.x[e][c] = v;
    }
    __syncthreads();
    policy_forward<PlainTowers>(S, R, a.E, prm, L);
    Hd::emit(S, a.E, a.d.a, nullptr, nullptr, a.action_out + (size_t)p * a.E * Hd::width(a.d.a), nullptr);
}

// ---- the VecNormalize step at runtime dims: the thread roles and fp64 arithmetic of pgm_policy_dev.hpp
__device__ void load_env_any(EnvAny& E, const pgm_env_state& st, const pgm_norm_state& ns, int p, int N, int o, int k) {
    const int t = threadIdx.x;
    for (int i = t; i < N * k; i += RT) E.obj_acc[i / k][i % k] = st.obj_acc[(size_t)p * N * k + i];
    if (t < N) E.ret[t] = st.ret[p * N + t];
    for (int c = t; c < o; c += RT) {
        E.ob_mean[c] = ns.ob_mean[(size_t)p * o + c];
        E.ob_var[c] = ns.ob_var[(size_t)p * o + c];
    }
    if (t < k) {
        E.obj_mean[t] = ns.obj_mean[p * k + t];
        E.obj_var[t] = ns.obj_var[p * k + t];
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

__device__ void store_env_any(const EnvAny& E, const pgm_env_state& st, const pgm_norm_state& ns, int p, int N, int o,
                              int k) {
    const int t = threadIdx.x;
    for (int i = t; i < N * k; i += RT) st.obj_acc[(size_t)p * N * k + i] = E.obj_acc[i / k][i % k];
    if (t < N) st.ret[p * N + t] = E.ret[t];
    for (int c = t; c < o; c += RT) {
        ns.ob_mean[(size_t)p * o + c] = E.ob_mean[c];
        ns.ob_var[(size_t)p * o + c] = E.ob_var[c];
    }
    if (t < k) {
        ns.obj_mean[p * k + t] = E.obj_mean[t];
        ns.obj_var[p * k + t] = E.obj_var[t];
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

__device__ void ob_stats_any(EnvAny& E, int N, int o, const NormCfg& nc, const DivN& divn) {
    for (int c = threadIdx.x; c < o; c += RT) {
        double sum = 0.0;
        for (int n = 0; n < N; ++n) sum += E.snew[n][c];
        ob_merge(E, c, N, nc, divn, sum);
    }
}

// norm_stats: ob_rms on feature threads, objective accumulators + obj_rms and ret_rms at the top of the block
__device__ void norm_stats_any(EnvAny& E, int N, int o, int K, const NormCfg& nc, const double* __restrict__ reward) {
    const DivN divn(N);
    if (nc.use_ob) ob_stats_any(E, N, o, nc, divn);
    const int t = threadIdx.x, k = RT - 1 - t;
    if (k < K) {
        for (int n = 0; n < N; ++n)
            E.obj_acc[n][k] = E.obj_valid ? E.obj_acc[n][k] * nc.gamma + E.objraw[n][k] : E.objraw[n][k];
        if (nc.use_obj) {
            double sum = 0.0;
            for (int n = 0; n < N; ++n) sum += E.obj_acc[n][k];
            batch_merge(E.obj_mean[k], E.obj_var[k], E.obj_count, N, divn, sum, [&](int n) { return E.obj_acc[n][k]; });
            E.obj_inv[k] = 1.0 / sqrt(E.obj_var[k] + nc.eps);
        }
    }
    if (t == RT - 1 - K) {
        double sum = 0.0;
        for (int n = 0; n < N; ++n) {
            E.ret[n] = E.ret[n] * nc.gamma + reward[n];
            sum += E.ret[n];
        }
        batch_merge(E.ret_mean, E.ret_var, E.ret_count, N, divn, sum, [&](int n) { return E.ret[n]; });
        E.ret_count += divn.dn;
    }
    lds_sync();
}

__device__ void vecnorm_reset_any(EnvAny& E, int N, int o, const NormCfg& nc, float* obs_out) {
    const int t = threadIdx.x;
    if (t < N) E.ret[t] = 0.0;
    if (t == 0) E.obj_valid = 0;
    if (nc.use_ob) ob_stats_any(E, N, o, nc, DivN(N));
    __syncthreads();
    if (t == 0 && nc.use_ob) E.ob_count += (double)N;
    for (int i = t; i < N * o; i += RT) {
        const int c = i % o;
        double v = E.snew[i / o][c];
        if (nc.use_ob) v = clipd((v - E.ob_mean[c]) * E.ob_inv[c], -nc.clipob, nc.clipob);
        obs_out[i] = (float)v;
    }
}

__device__ void vecnorm_emit_any(EnvAny& E, int N, int o, int K, const NormCfg& nc, float* obs_out, float* rew_out,
                                 float* mask_out, float* bad_out) {
    const int t = threadIdx.x;
    for (int i = t; i < N * o; i += RT) {
        const int n = i / o, c = i % o;
        double v = E.snew[n][c];
        if (nc.use_ob) v = clipd((v - E.ob_mean[c]) * E.ob_inv[c], -nc.clipob, nc.clipob);
        obs_out[i] = (float)v;  // VecPyTorch .float() (envs.py:192)
    }
    const int i = RT - 1 - t;
    if (i < N * K) {
        const int n = i / K, k = i % K;
        double r = E.objraw[n][k];
        if (nc.use_obj) r = clipd(r * E.obj_inv[k], -nc.cliprew, nc.cliprew);
        rew_out[i] = (float)r;
        if (E.done[n]) E.obj_acc[n][k] = 0.0;
    }
    const int n = RT - 1 - N * K - t;
    if (n >= 0 && n < N) {
        mask_out[n] = E.done[n] ? 0.f : 1.f;
        bad_out[n] = E.bad[n] ? 0.f : 1.f;
        if (E.done[n]) E.ret[n] = 0.0;
    }
    if (t == 0) {
        if (nc.use_ob) E.ob_count += (double)N;
        if (nc.use_obj) E.obj_count += (double)N;
        E.obj_valid = 1;
    }
    lds_sync();
}

struct IngestAnyArgs {
    int P, N, T, t;  // t = -1: reset
    AnyDims d;
    pgm_env_state st;
    pgm_norm_state ns;
    pgm_rollout_buf rb;
    const double *raw_obs, *raw_obj, *reward;  // [P][N][o], [P][N][k], [P][N]
    const int32_t *done, *bad;                 // [P][N]
};

// env_ingest_kernel (pgm_hostenv.hip) at runtime dims: no auto-reset, the scalar reward in VecNormalize.ret
__global__ __launch_bounds__(RT) void env_ingest_any_kernel(IngestAnyArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& E = *reinterpret_cast<EnvAny*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T, o = a.d.o, k = a.d.k;
    const NormCfg nc = norm_cfg(a.ns);
    float* obs = a.rb.obs + (size_t)p * (T + 1) * N * o;
    float* masks = a.rb.masks + (size_t)p * (T + 1) * N;
    float* bad = a.rb.bad_masks + (size_t)p * (T + 1) * N;
    load_env_any(E, a.st, a.ns, p, N, o, k);
    for (int i = t; i < N * o; i += RT) E.snew[i / o][i % o] = a.raw_obs[(size_t)p * N * o + i];
    if (a.t >= 0) {
        for (int i = t; i < N * k; i += RT) E.objraw[i / k][i % k] = a.raw_obj[(size_t)p * N * k + i];
        if (t < N) {
            E.done[t] = a.done[p * N + t] != 0;
            E.bad[t] = a.bad[p * N + t] != 0;
        }
    }
    __syncthreads();
    if (a.t < 0) {
        vecnorm_reset_any(E, N, o, nc, obs);
        if (t < N) {
            masks[t] = 1.f;
            bad[t] = 1.f;
        }
    } else {
        norm_stats_any(E, N, o, k, nc, a.reward + (size_t)p * N);
        vecnorm_emit_any(E, N, o, k, nc, obs + (size_t)(a.t + 1) * N * o, a.rb.rewards + ((size_t)p * T + a.t) * N * k,
                         masks + (size_t)(a.t + 1) * N, bad + (size_t)(a.t + 1) * N);
    }
    __syncthreads();
    store_env_any(E, a.st, a.ns, p, N, o, k);
}

static Layout any_layout(const pgm_dims* d, int head) {
    return head ? cat_as_plain(make_layout_cat(d->O, d->A, d->K, d->H)) : make_layout(d->O, d->A, d->K, d->H);
}

}  // namespace pgm

using namespace pgm;

extern "C" {

// Arguments are validated before any device work: NULL pointers, check_dims, the range of the family, LN, then the
// step index or E.
int pgm_rollout_act_any(const pgm_dims* d, int32_t head, const float* params, const pgm_rollout_buf* rb, int32_t t,
                        const float* rnd, void* action_out, pgm_stream_t stream) {
    const char* what = "pgm_rollout_act_any";
    if (!d || !params || !rb || !rb->obs || !rb->actions || !rb->logp || !rb->values) {
        set_error("%s: null pointer", what);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, what)) return rc;
    if (int rc = check_any_dims(d, head, what)) return rc;
    if (t < 0 || t > d->T) {
        set_error("%s: step t=%d outside [0, T=%d]", what, t, d->T);
        return PGM_E_SHAPE;
    }
    if (t < d->T && (!rnd || !action_out)) {
        set_error("%s: rnd and action_out are required for t < T", what);
        return PGM_E_INVALID_ARG;
    }
    const AnyDims ad{d->O, d->A, d->K};
    const Layout L = any_layout(d, head);
    if (head) {
        RolloutActAnyArgs<CatHeadAny> a{d->P, d->N, d->T, t, ad, params, *rb, rnd, (int32_t*)action_out};
        return launch_smem(rollout_act_any_kernel<CatHeadAny>, d->P, sizeof(PolAny), (hipStream_t)stream, what, a, L);
    }
    RolloutActAnyArgs<GaussHeadAny> a{d->P, d->N, d->T, t, ad, params, *rb, rnd, (float*)action_out};
    return launch_smem(rollout_act_any_kernel<GaussHeadAny>, d->P, sizeof(PolAny), (hipStream_t)stream, what, a, L);
}

int pgm_eval_act_any(const pgm_dims* d, int32_t head, const float* params, const double* ob_mean,
                     const double* ob_var, int32_t use_ob_rms, const double* raw_obs, int32_t E, void* action_out,
                     pgm_stream_t stream) {
    const char* what = "pgm_eval_act_any";
    if (!d || !params || !raw_obs || !action_out || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("%s: null pointer (ob_mean / ob_var are required with use_ob_rms)", what);
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: the rows are the E evaluation episodes
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, what)) return rc;
    if (int rc = check_any_dims(&dd, head, what)) return rc;
    if (E < 1 || E > NMAX) {
        set_error("%s: E=%d evaluation episodes outside [1, %d]", what, E, NMAX);
        return PGM_E_SHAPE;
    }
    const AnyDims ad{d->O, d->A, d->K};
    const Layout L = any_layout(d, head);
    if (head) {
        EvalActAnyArgs<CatHeadAny> a{d->P, E, ad, params, ob_mean, ob_var, raw_obs, use_ob_rms != 0,
                                     (int32_t*)action_out};
        return launch_smem(eval_act_any_kernel<CatHeadAny>, d->P, sizeof(PolAny), (hipStream_t)stream, what, a, L);
    }
    EvalActAnyArgs<GaussHeadAny> a{d->P, E, ad, params, ob_mean, ob_var, raw_obs, use_ob_rms != 0, (float*)action_out};
    return launch_smem(eval_act_any_kernel<GaussHeadAny>, d->P, sizeof(PolAny), (hipStream_t)stream, what, a, L);
}

// the ingest never reads the action: d->A is range-checked as a Gaussian head's (1..8), which covers both heads
int pgm_env_ingest_any(const pgm_dims* d, const pgm_env_state* st, const pgm_norm_state* ns,
                       const pgm_rollout_buf* rb, int32_t t, const double* raw_obs, const double* raw_obj,
                       const double* reward, const int32_t* done, const int32_t* bad_transition, pgm_stream_t stream) {
    const char* what = "pgm_env_ingest_any";
    if (!d || !st || !st->obj_acc || !st->obj_acc_valid || !st->ret || !norm_ok(ns) || !rb || !rb->obs ||
        !rb->rewards || !rb->masks || !rb->bad_masks || !raw_obs) {
        set_error("%s: null pointer", what);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, what)) return rc;
    if (int rc = check_any_dims(d, 0, what)) return rc;
    if (t < -1 || t >= d->T) {
        set_error("%s: step t=%d outside [-1, T=%d)", what, t, d->T);
        return PGM_E_SHAPE;
    }
    if (t >= 0 && (!raw_obj || !reward || !done || !bad_transition)) {
        set_error("%s: raw_obj, reward, done and bad_transition are required for t >= 0", what);
        return PGM_E_INVALID_ARG;
    }
    IngestAnyArgs a{d->P, d->N, d->T, t, {d->O, d->A, d->K}, *st, *ns, *rb, raw_obs, raw_obj, reward, done,
                    bad_transition};
    return launch_smem(env_ingest_any_kernel, d->P, sizeof(EnvAny), (hipStream_t)stream, what, a);
}

}  // extern "C"
