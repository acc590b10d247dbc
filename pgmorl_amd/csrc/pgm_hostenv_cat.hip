// Discrete-action policies at the host-env seam: pgm_act_forward_cat, pgm_rollout_act_cat, pgm_eval_act_cat and the
// perf-mode uniform stream pgm_uniform_noise.  The towers and the head's Linear run through policy_forward of
// pgm_policy_dev.hpp (the head weights have the shape of fc_mean, so S.mu receives the logits); only the emit differs:
// one integer action per row, drawn by the sampling rule of include/pgm_abi.h, and its log-prob.  One workgroup per
// task, as rollout_act_kernel.  A translation unit of its own keeps every existing code object as it was.
//
// Reference semantics (paths relative to the reference tree):
//   Policy.act / get_value, dist = Categorical   a2c_ppo_acktr/model.py:33-35,57-73
//   Categorical / FixedCategorical               a2c_ppo_acktr/distributions.py:17-27,54-68
//   one rollout step, bootstrap value            morl/mopg.py:105-108, 132-135
//   evaluation() normalise + act                 morl/mopg.py:36-39
#include "pgm_policy_dev.hpp"

namespace pgm {

// policy_forward / load_polreg address the towers, the value head and the head's Linear through a plain Layout: the
// categorical layout has the same first twelve tensors (no logstd; its offset is never read on this path, O <= 32)
inline Layout cat_as_plain(const LayoutCat& C) {
    Layout L;
    for (int i = 0; i < PGM_NUM_PARAM_TENSORS_CAT; ++i) L.off[i] = C.off[i];
    L.off[PGM_P_LOGSTD] = 0;
    L.total = C.total;
    return L;
}

// load_policy without the logstd slot
template <int O, int A, int K>
__device__ void load_policy_cat(PolSmem<O, A, K>& S, const float* __restrict__ prm, const Layout& L) {
    const int t = threadIdx.x;
    if (t < K) S.bv[t] = prm[L.off[PGM_P_VALUE_B] + t];
    if (t < A) S.bm[t] = prm[L.off[PGM_PC_LINEAR_B] + t];
}

// The sampling rule (include/pgm_abi.h) on the logits of one row: the action and its log-prob.  u is read only when
// !deterministic.
template <int A>
__device__ __forceinline__ int cat_sample(const float* z, bool deterministic, float u, float& logp) {
    float m = z[0];
    int am = 0;
#pragma unroll
    for (int j = 1; j < A; ++j)
        if (z[j] > m) {  // strict: the lowest index among the maxima
            m = z[j];
            am = j;
        }
    float e[A], s = 0.f;
#pragma unroll
    for (int j = 0; j < A; ++j) {
        e[j] = expf(z[j] - m);
        s += e[j];
    }
    int act = am;
    if (!deterministic) {
        float c = 0.f;
        act = 0;
#pragma unroll
        for (int j = 0; j < A - 1; ++j) {
            c += e[j] / s;
            act += c <= u ? 1 : 0;
        }
    }
    float za = z[0];
#pragma unroll
    for (int j = 1; j < A; ++j) za = act == j ? z[j] : za;
    logp = za - (m + logf(s));
    return act;
}

struct ActCatArgs {
    int P, N;
    Layout L;
    const float* params;
    const float* obs;       // [P][N][O]
    const float* uniforms;  // [N]
    int deterministic;
    float* value;           // [P][N][K]
    int32_t* action;        // [P][N]
    float* logp;            // [P][N]
};

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void act_forward_cat_kernel(ActCatArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x, N = a.N;
    const float* prm = a.params + (size_t)p * a.L.total;
    PolReg<O, A, K> R;
    load_policy_cat(S, prm, a.L);
    load_polreg(R, prm, a.L);
    for (int i = t; i < N * O; i += RT) S.x[i / O][i % O] = a.obs[(size_t)p * N * O + i];
    __syncthreads();
    policy_forward(S, R, N, prm, a.L);
    for (int i = t; i < N * K; i += RT) a.value[(size_t)p * N * K + i] = S.val[i / K][i % K];
    if (t < N) {
        float lp;
        const int act = cat_sample<A>(S.mu[t], a.deterministic != 0, a.deterministic ? 0.f : a.uniforms[t], lp);
        a.action[(size_t)p * N + t] = act;
        a.logp[(size_t)p * N + t] = lp;
    }
}

struct RolloutActCatArgs {
    int P, N, T, t;
    Layout L;
    const float* params;
    pgm_rollout_buf rb;     // actions [P][T][N][1]
    const float* uniforms;  // base of [T][N]
    int32_t* action_out;    // [P][N]
};

template <int O, int A, int K>
__global__ __launch_bounds__(RT) void rollout_act_cat_kernel(RolloutActCatArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T, st = a.t;
    const float* prm = a.params + (size_t)p * a.L.total;
    const float* obs = a.rb.obs + ((size_t)p * (T + 1) + st) * N * O;
    PolReg<O, A, K> R;
    load_policy_cat(S, prm, a.L);
    load_polreg(R, prm, a.L);
    for (int i = t; i < N * O; i += RT) S.x[i / O][i % O] = obs[i];
    __syncthreads();
    policy_forward(S, R, N, prm, a.L);
    float* val = a.rb.values + ((size_t)p * (T + 1) + st) * N * K;
    for (int i = t; i < N * K; i += RT) val[i] = S.val[i / K][i % K];
    if (st >= T) return;  // t == T: the bootstrap get_value only (uniform over the grid)
    if (t < N) {
        float lp;
        const int act = cat_sample<A>(S.mu[t], false, a.uniforms[(size_t)st * N + t], lp);
        const size_t slot = ((size_t)p * T + st) * N + t;
        a.rb.actions[slot] = (float)act;  // the index, exact in fp32
        a.rb.logp[slot] = lp;
        a.action_out[(size_t)p * N + t] = act;
    }
}

struct EvalActCatArgs {
    int P, E;
    Layout L;
    const float* params;
    const double *ob_mean, *ob_var, *raw_obs;  // [P][O], [P][O], [P][E][O]
    int use_ob;
    int32_t* action_out;  // [P][E]
};

// mopg.py:36-38 as eval_act_kernel (pgm_hostenv.hip): fp64 normalisation with the frozen statistics, fixed eps / clip,
// then the fp32 cast; the action is the mode
template <int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_act_cat_kernel(EvalActCatArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PolSmem<O, A, K>*>(smem_raw);
    const int p = blockIdx.x, t = threadIdx.x;
    const float* prm = a.params + (size_t)p * a.L.total;
    PolReg<O, A, K> R;
    load_policy_cat(S, prm, a.L);
    load_polreg(R, prm, a.L);
    for (int i = t; i < a.E * O; i += RT) {
        const int e = i / O, o = i % O;
        double v = a.raw_obs[((size_t)p * a.E + e) * O + o];
        if (a.use_ob) {
            const double inv = 1.0 / sqrt(a.ob_var[(size_t)p * O + o] + 1e-8);
            v = clipd((v - a.ob_mean[(size_t)p * O + o]) * inv, -10.0, 10.0);
        }
        S.x[e][o] = (float)v;
    }
    __syncthreads();
    policy_forward(S, R, a.E, prm, a.L);
    if (t < a.E) {
        float lp;
        a.action_out[(size_t)p * a.E + t] = cat_sample<A>(S.mu[t], true, 0.f, lp);
    }
}

// fp32 uniform in [0, 1) with 24 random bits for element i of stream `seed`: the hash of counter_normal
__device__ __forceinline__ float counter_uniform(uint64_t seed, uint64_t i) {
    const uint64_t h = splitmix64(splitmix64(seed * 0xD1B54A32D192ED03ull + 0x632BE59BD9B4E019ull) ^ i);
    return (float)(uint32_t)(h >> 40) * (1.0f / 16777216.0f);
}

__global__ void uniform_kernel(int64_t n, uint64_t seed, float* out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = counter_uniform(seed, (uint64_t)i);
}

}  // namespace pgm

using namespace pgm;

extern "C" {

// Arguments are validated before any device work: NULL pointers, check_dims, the dim set, the step index or E, LN.
int pgm_act_forward_cat(const pgm_dims* d, const float* params, const float* obs, const float* uniforms,
                        int32_t deterministic, float* value, int32_t* action, float* logp, pgm_stream_t stream) {
    if (!d || !params || !obs || !value || !action || !logp || (!deterministic && !uniforms)) {
        set_error("pgm_act_forward_cat: null pointer (uniforms is required unless deterministic)");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, "pgm_act_forward_cat")) return rc;
    if (int rc = check_cat_dims(d, "pgm_act_forward_cat")) return rc;
    if (int rc = check_cat_ln(d, "pgm_act_forward_cat")) return rc;
    ActCatArgs a{d->P, d->N, cat_as_plain(make_layout_cat(d->O, d->A, d->K, d->H)), params, obs, uniforms,
                 deterministic, value, action, logp};
    return dispatch_dims_cat(d->O, d->A, d->K, "pgm_act_forward_cat", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(act_forward_cat_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_act_forward_cat");
    });
}

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
    RolloutActCatArgs a{d->P, d->N, d->T, t, cat_as_plain(make_layout_cat(d->O, d->A, d->K, d->H)), params, *rb,
                        uniforms, action_out};
    return dispatch_dims_cat(d->O, d->A, d->K, "pgm_rollout_act_cat", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(rollout_act_cat_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_rollout_act_cat");
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
    EvalActCatArgs a{d->P, E, cat_as_plain(make_layout_cat(d->O, d->A, d->K, d->H)), params, ob_mean, ob_var, raw_obs,
                     use_ob_rms != 0, action_out};
    return dispatch_dims_cat(d->O, d->A, d->K, "pgm_eval_act_cat", [&](auto o, auto aa, auto k) {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        return launch_smem(eval_act_cat_kernel<O, A, K>, d->P, sizeof(PolSmem<O, A, K>), (hipStream_t)stream, a,
                           "pgm_eval_act_cat");
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
