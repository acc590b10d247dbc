// A device env plug-in library (include/pgm_envplug.h): this file compiled with a user env header force-included, into
// a libpgm_env.so of its own (pgmorl_amd.build.build_env).  It links nothing from libpgm.so: the error plumbing and the
// parameter layouts that pgm_common.hpp declares are defined here.
//
// rollout_env_kernel / eval_env_kernel are the block form of rollout_dummy_kernel / rollout_dst_kernel (pgm_dummy.hip,
// pgm_dst.hip) with the env rule taken from the header: one 256-thread workgroup per task, plain towers, the policy
// instantiated at the header's own (O, A, K), the Gaussian or the Categorical head by pgm_user_env::DISCRETE.  The
// towers, the head arithmetic and the VecNormalize arithmetic are the device functions of pgm_policy_dev.hpp, what
// the host-stepped runtime-dim path (pgm_rollout_act_any / pgm_env_ingest_any) runs per step on zero-padded images, so
// the stored fields of the two paths are equal.
//
// Reference semantics (paths relative to the reference tree):
//   Policy.act / get_value, the heads      a2c_ppo_acktr/model.py:57-73; distributions.py
//   DummyVecEnv auto-reset                 baselines/common/vec_env/dummy_vec_env.py:45-56
//   VecNormalize.step_wait                 baselines/common/vec_env/vec_normalize.py:29-43
//   masks / bad_masks / obj_tensor, insert morl/mopg.py:103-135, a2c_ppo_acktr/storage.py:50-75
//   evaluation()                           morl/mopg.py:25-46
#define PGM_ENVPLUG_DECLARE_API
#include "pgm_envplug.hpp"
#include "pgm_policy_dev.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#define PGM_ENVPLUG_EXPORT extern "C"

PGM_STAMP_UNIT(envplug)

namespace pgm {

// ---- what pgm_common.hpp declares and libpgm.so defines in pgm_abi.cpp, for this library alone
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int hip_fail(hipError_t e, const char* what) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return PGM_E_HIP;
}
int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what);
    return PGM_OK;
}
// pgm_param_layout / pgm_param_layout_cat: tensors 16-byte aligned, the total a multiple of 64 floats
template <int NT>
static void layout_offsets(const int32_t (&sizes)[NT], int32_t* off, int32_t& total) {
    int32_t p = 0;
    for (int i = 0; i < NT; ++i) {
        off[i] = p;
        p = (p + sizes[i] + 3) / 4 * 4;
    }
    total = (p + 63) / 64 * 64;
}
Layout make_layout(int O, int A, int K, int Hd) {
    const int32_t sizes[PGM_NUM_PARAM_TENSORS] = {O * Hd, Hd, Hd * Hd, Hd, O * Hd, Hd, Hd * Hd, Hd,
                                                  Hd * K, K,  Hd * A,  A,  A};
    Layout L;
    layout_offsets(sizes, L.off, L.total);
    return L;
}
LayoutCat make_layout_cat(int O, int A, int K, int Hd) {
    const int32_t sizes[PGM_NUM_PARAM_TENSORS_CAT] = {O * Hd, Hd, Hd * Hd, Hd, O * Hd, Hd, Hd * Hd, Hd,
                                                      Hd * K, K,  Hd * A,  A};
    LayoutCat L;
    layout_offsets(sizes, L.off, L.total);
    return L;
}

using envplug::Env;
using envplug::SDN;
using envplug::SIN;
constexpr int EO = Env::O, EA = Env::A, EK = Env::K;
constexpr bool CAT = Env::DISCRETE;
constexpr int AW = CAT ? 1 : EA;  // stored action width, random inputs per (step, env)
// contract 2 (runtime parameters, per-step uniforms); for a contract-1 header every use below is compiled out
using envplug::C2;
using envplug::NP;
using envplug::NPN;
using envplug::NW;
using envplug::NWN;

// the step image of the block kernels plus the scalar env reward of the step (VecNormalize.ret's input)
struct PlugSmem {
    StepSmem<EO, EA, EK> st;
    double reward[NMAX];
};

struct PlugRolloutArgs {
    int P, N, T;
    const float* params;
    double* sd;        // [P][N][SD]
    int32_t* si;       // [P][N][SI]
    int32_t* episode;  // [P][N]
    const double* table;  // [>= N][R][RW]
    int R;
    pgm_env_state st;  // elapsed [P][N]: steps of the running episode; s, s0 unused
    pgm_norm_state ns;
    pgm_rollout_buf rb;
    const float* rnd;  // normals [T][N][A] / uniforms [T][N], or NULL: the counter stream of seed
    uint64_t seed;
    int carry;
    // contract 2
    const double* env_par;  // [NP]
    const double* env_rnd;  // [T][N][NW], or NULL: u53 of env_seed
    uint64_t env_seed;
};

__device__ __forceinline__ float plug_draw(const PlugRolloutArgs& a, size_t idx) {
    if constexpr (CAT) {
        return a.rnd ? a.rnd[idx] : counter_uniform(a.seed, idx);
    } else {
        return a.rnd ? a.rnd[idx] : counter_normal(a.seed, idx);
    }
}

// word j of (step, env) of the rollout's env noise: element (step N + n) NW + j
__device__ __forceinline__ double plug_draw_env(const PlugRolloutArgs& a, uint64_t key, size_t idx) {
    return a.env_rnd ? a.env_rnd[idx] : envplug::u53_at(key, idx);
}

__device__ __forceinline__ void plug_load(envplug::State& s, const PlugRolloutArgs& a, int g) {
#pragma unroll
    for (int i = 0; i < Env::SD; ++i) s.sd[i] = a.sd[(size_t)g * Env::SD + i];
#pragma unroll
    for (int i = 0; i < Env::SI; ++i) s.si[i] = a.si[(size_t)g * Env::SI + i];
    s.elapsed = a.st.elapsed[g];
    s.episode = a.episode[g];
}
__device__ __forceinline__ void plug_store(const envplug::State& s, const PlugRolloutArgs& a, int g) {
#pragma unroll
    for (int i = 0; i < Env::SD; ++i) a.sd[(size_t)g * Env::SD + i] = s.sd[i];
#pragma unroll
    for (int i = 0; i < Env::SI; ++i) a.si[(size_t)g * Env::SI + i] = s.si[i];
    a.st.elapsed[g] = s.elapsed;
    a.episode[g] = s.episode;
}

// fused rollout.  Thread n < N owns env n: it keeps the env's state words in registers, draws the env's random inputs
// one step ahead, samples its action (sample_actions' / CatHead's arithmetic) and runs its transition.  Four
// workgroup barriers per step: policy_forward, the transition hand-off, norm_stats, vecnorm_emit.  Every loop is
// bounded by T + 1, N or a compile-time constant.  Contract 2: every thread holds the NP parameters (one address, a
// scalar load) and the owner draws the step's NW uniforms where it draws the action noise, one step ahead.
__global__ __launch_bounds__(RT) void rollout_env_kernel(PlugRolloutArgs a, Layout L) {
    constexpr int O = EO, A = EA, K = EK;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PlugSmem*>(smem_raw);
    auto& P = S.st.pol;
    auto& E = S.st.env;
    const int p = blockIdx.x, t = threadIdx.x, N = a.N, T = a.T;
    const NormCfg nc = norm_cfg(a.ns);
    const float* prm = a.params + (size_t)p * L.total;
    float* obs = a.rb.obs + (size_t)p * (T + 1) * N * O;
    float* act = a.rb.actions + (size_t)p * T * N * AW;
    float* logp = a.rb.logp + (size_t)p * T * N;
    float* val = a.rb.values + (size_t)p * (T + 1) * N * K;
    float* rew = a.rb.rewards + (size_t)p * T * N * K;
    float* masks = a.rb.masks + (size_t)p * (T + 1) * N;
    float* bad = a.rb.bad_masks + (size_t)p * (T + 1) * N;
    const bool owner = t < N;

    PolReg<O, A, K> R;
    load_policy<PlainTowers, !CAT>(P, R, prm, L);
    load_env<false>(E, a.st, a.ns, p, N);
    envplug::State env = {};
    if (owner) plug_load(env, a, p * N + t);
    double par[NPN] = {}, w[NWN] = {}, w_next[NWN] = {};
    uint64_t env_key = 0;
    if constexpr (C2) {
#pragma unroll
        for (int i = 0; i < NP; ++i) par[i] = a.env_par[i];
        if constexpr (NW > 0) env_key = envplug::noise_key(a.env_seed);
    }
    const double* row = a.table + (size_t)(owner ? t : 0) * a.R * Env::RW;
    if (a.carry) {  // after_update(): slot T -> slot 0 (storage.py:71-75); each thread re-reads its own writes
        for (int i = t; i < N * O; i += RT) obs[i] = obs[(size_t)T * N * O + i];
        if (owner) {
            masks[t] = masks[(size_t)T * N + t];
            bad[t] = bad[(size_t)T * N + t];
        }
    }
    load_rows(P, obs, N);
    __syncthreads();

    float ls[EA], sdv[EA], rnd_next[EA] = {};  // (AW of them used)
    if constexpr (!CAT) {
#pragma unroll
        for (int j = 0; j < A; ++j) {
            ls[j] = P.logstd[j];
            sdv[j] = expf(ls[j]);
        }
    }
    if (owner) {
#pragma unroll
        for (int j = 0; j < AW; ++j) rnd_next[j] = plug_draw(a, (size_t)(t * AW + j));
        if constexpr (C2) {
#pragma unroll
            for (int j = 0; j < NW; ++j) w_next[j] = plug_draw_env(a, env_key, (size_t)(t * NW + j));
        }
    }
    PGM_STAMP_DECL
    // T + 1 passes: the last one is the bootstrap value alone (mopg.py:132-135 -> value_preds[T], storage.py:85).  It
    // runs the loop's own copy of policy_forward on purpose: a second inlined copy, whose action head is dead, is
    // compiled with other fma contractions and its values differ from the step kernels' in the last bit.
    for (int step = 0; step <= T; ++step) {
        float rnd[EA];
#pragma unroll
        for (int j = 0; j < AW; ++j) rnd[j] = rnd_next[j];
        if constexpr (C2) {
#pragma unroll
            for (int j = 0; j < NW; ++j) w[j] = w_next[j];
        }
        if (owner && step + 1 < T) {
#pragma unroll
            for (int j = 0; j < AW; ++j) rnd_next[j] = plug_draw(a, ((size_t)(step + 1) * N + t) * AW + j);
            if constexpr (C2) {
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    w_next[j] = plug_draw_env(a, env_key, ((size_t)(step + 1) * N + t) * NW + j);
            }
        }
        PGM_STAMP(0);
        policy_forward<PlainTowers>(P, R, N, prm, L);
        PGM_STAMP(1);
        store_values(P, val + (size_t)step * N * K, N);
        if (step == T) break;  // uniform over the workgroup
        if (owner) {
            envplug::StepOut o;
            const pgm_env_ctx ctx{par, w};
            if constexpr (CAT) {
                float lp;
                const int ai = cat_sample<A>(P.mu[t], false, rnd[0], lp);
                act[(size_t)step * N + t] = (float)ai;
                logp[(size_t)step * N + t] = lp;
                o = envplug::transition(env, envplug::Action{nullptr, ai}, row, a.R, ctx);
            } else {
                float av[A], lp = 0.f;
#pragma unroll
                for (int j = 0; j < A; ++j) {  // sample_actions' arithmetic; the log-prob summed over A in index order
                    const float mu = P.mu[t][j];
                    av[j] = fmaf(rnd[j], sdv[j], mu);
                    lp += gauss_logp_term(av[j], mu, ls[j], sdv[j]);
                    act[((size_t)step * N + t) * A + j] = av[j];  // raw, unclipped: the env clips
                }
                logp[(size_t)step * N + t] = lp;
                o = envplug::transition(env, envplug::Action{av, 0}, row, a.R, ctx);
            }
            envplug::call_observe<Env>(env.sd, env.si, E.snew[t], par);
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
    __syncthreads();
    store_env<false>(E, a.st, a.ns, p, N);
    if (owner) plug_store(env, a, p * N + t);
    PGM_STAMP_FLUSH;
}

struct PlugEvalArgs {
    int P;
    const float* params;
    const double* table;  // [>= eval_num][R][RW]: episode e starts at entry (e, 0)
    int R;
    const double *ob_mean, *ob_var;
    int eval_num, use_ob, raw;
    double gamma;
    double* objs;
    // contract 2
    const double* env_par;  // [NP]
    uint64_t env_seed;      // word j of (episode e, step it): element (e MAX_STEPS + it) NW + j
};

// deterministic evaluation (mopg.py:25-46): eval_num episodes are the rows of one forward and step together; thread
// e < eval_num owns episode e.  An ended episode stands still and adds nothing more.  At most MAX_STEPS iterations:
// step_limit ends every live episode on its MAX_STEPS-th step.
__global__ __launch_bounds__(RT) void eval_env_kernel(PlugEvalArgs a, Layout L) {
    constexpr int O = EO, A = EA, K = EK;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<PlugSmem*>(smem_raw);
    auto& P = S.st.pol;
    auto& E = S.st.env;
    const int p = blockIdx.x, t = threadIdx.x, EN = a.eval_num;
    const float* prm = a.params + (size_t)p * L.total;
    PolReg<O, A, K> R;
    load_policy<PlainTowers, !CAT>(P, R, prm, L);
    for (int o = t; o < O; o += RT) {
        E.ob_mean[o] = a.use_ob ? a.ob_mean[(size_t)p * O + o] : 0.0;
        E.ob_inv[o] = a.use_ob ? eval_ob_inv(a.ob_var[(size_t)p * O + o]) : 1.0;
    }
    const bool owner = t < EN;
    envplug::State env = {};
    int alive = 1;
    double acc[K] = {}, disc = 1.0;
    double par[NPN] = {}, w[NWN] = {}, w_next[NWN] = {};
    uint64_t env_key = 0;
    if constexpr (C2) {
#pragma unroll
        for (int i = 0; i < NP; ++i) par[i] = a.env_par[i];
        if constexpr (NW > 0) {
            env_key = envplug::noise_key(a.env_seed);
            if (owner) {
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    w_next[j] = envplug::u53_at(env_key, (size_t)t * Env::MAX_STEPS * NW + j);
            }
        }
    }
    if (owner) {
        envplug::start(env, a.table + (size_t)t * a.R * Env::RW, pgm_env_ctx{par, nullptr});
        envplug::call_observe<Env>(env.sd, env.si, E.snew[t], par);
        E.done[t] = 0;
    }
    __syncthreads();
    for (int it = 0; it < Env::MAX_STEPS; ++it) {
        if constexpr (C2 && NW > 0) {  // this step's uniforms; the next step's are drawn beside the forward
#pragma unroll
            for (int j = 0; j < NW; ++j) w[j] = w_next[j];
            if (owner && alive && it + 1 < Env::MAX_STEPS) {
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    w_next[j] = envplug::u53_at(env_key, ((size_t)t * Env::MAX_STEPS + it + 1) * NW + j);
            }
        }
        for (int i = t; i < EN * O; i += RT) {
            const int e = i / O, o = i % O;
            P.x[e][o] = eval_normalise(E.snew[e][o], a.use_ob, E.ob_mean[o], E.ob_inv[o]);
        }
        lds_sync();
        policy_forward<PlainTowers>(P, R, EN, prm, L);
        if (owner && alive) {  // the mean action (the env clips it) / the lowest-index argmax
            envplug::StepOut o;
            const pgm_env_ctx ctx{par, w};
            if constexpr (CAT) {
                float lp;
                o = envplug::step_limit(env, envplug::Action{nullptr, cat_sample<A>(P.mu[t], true, 0.f, lp)}, ctx);
            } else {
                float av[A];
#pragma unroll
                for (int j = 0; j < A; ++j) av[j] = P.mu[t][j];
                o = envplug::step_limit(env, envplug::Action{av, 0}, ctx);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += disc * o.obj[k];
            if (o.done) {
                alive = 0;
                E.done[t] = 1;
            } else {
                envplug::call_observe<Env>(env.sd, env.si, E.snew[t], par);
            }
        }
        if (!a.raw) disc *= a.gamma;
        lds_sync();
        int live = 0;
        for (int e = 0; e < EN; ++e) live |= !E.done[e];
        if (!live) break;  // uniform over the workgroup
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

static Layout plug_layout() { return CAT ? cat_as_plain(make_layout_cat(EO, EA, EK, H)) : make_layout(EO, EA, EK, H); }

// after NULL pointers and check_dims: the compiled header's dims, then pgm_dims.LN
static int check_plug_dims(const pgm_dims* d, const char* what) {
    if (d->O != EO || d->A != EA || d->K != EK) {
        set_error("%s: dims O=%d A=%d K=%d, this plug-in library is compiled for %d/%d/%d (%s head)", what, d->O, d->A,
                  d->K, EO, EA, EK, CAT ? "Categorical" : "Gaussian");
        return PGM_E_UNSUPPORTED;
    }
    if (d->LN != 0) {
        set_error("%s: pgm_dims.LN = %d: env plug-ins are built for plain towers only (LN must be 0)", what, d->LN);
        return PGM_E_UNSUPPORTED;
    }
    return PGM_OK;
}

// need: the reset-table rows the call reads (N envs / eval_num episodes / 1)
static int check_plug_table(int R, int reset_count, int need, const char* what) {
    if (R < 1) {
        set_error("%s: R = %d reset-table entries per row must be at least 1", what, R);
        return PGM_E_INVALID_ARG;
    }
    if (reset_count < need) {
        set_error("%s: reset_count = %d rows of the reset table, the call reads %d", what, reset_count, need);
        return PGM_E_INVALID_ARG;
    }
    return PGM_OK;
}

// a library built from a CONTRACT = 2 header answers the calls without env_par / env noise with this
static int refuse_contract2(const char* what) {
    set_error("%s: this library is built from a CONTRACT = 2 header (NP = %d runtime parameters, NW = %d uniforms per "
              "step): call %s_ex", what, NP, NW, what);
    return PGM_E_UNSUPPORTED;
}
// after every check of the contract-1 call
static int check_env_par(const double* env_par, const char* what) {
    if (NP > 0 && !env_par) {
        set_error("%s: env_par is a null pointer, the header has NP = %d runtime parameters", what, NP);
        return PGM_E_INVALID_ARG;
    }
    return PGM_OK;
}

}  // namespace pgm

using namespace pgm;

PGM_ENVPLUG_EXPORT int pgm_envplug_abi(void) { return PGM_ENVPLUG_ABI; }
PGM_ENVPLUG_EXPORT const char* pgm_envplug_last_error(void) { return pgm::g_err; }

PGM_ENVPLUG_EXPORT int pgm_envplug_info(int32_t* out) {
    if (!out) {
        set_error("pgm_envplug_info: null pointer");
        return PGM_E_INVALID_ARG;
    }
    const int32_t v[8] = {EO, EA, EK, CAT ? 1 : 0, Env::SD, Env::SI, Env::RW, Env::MAX_STEPS};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return PGM_OK;
}

static int plug_rollout(const char* what, const pgm_dims* d, const float* params, double* sd, int32_t* si,
                        int32_t* episode, const double* table, int32_t R, int32_t reset_count,
                        const pgm_env_state* st, const pgm_norm_state* ns, const pgm_rollout_buf* rb,
                        const float* stream_in, uint64_t seed, int32_t carry, const double* env_par,
                        const double* env_rnd, uint64_t env_seed, pgm_stream_t stream) {
    if (!d || !params || (Env::SD > 0 && !sd) || (Env::SI > 0 && !si) || !episode || (Env::RW > 0 && !table) || !st ||
        !st->elapsed || !st->obj_acc || !st->obj_acc_valid || !st->ret || !norm_ok(ns) || !rb || !rb->obs ||
        !rb->actions || !rb->logp || !rb->values || !rb->rewards || !rb->masks || !rb->bad_masks) {
        set_error("%s: null pointer", what);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_dims(d, what)) return rc;
    if (int rc = check_plug_dims(d, what)) return rc;
    if (d->T <= 0) {
        set_error("%s: T must be positive", what);
        return PGM_E_SHAPE;
    }
    if (int rc = check_plug_table(R, reset_count, d->N, what)) return rc;
    if (int rc = check_env_par(env_par, what)) return rc;
    PlugRolloutArgs a{d->P, d->N, d->T, params, sd, si, episode, table, R, *st, *ns, *rb, stream_in, seed, carry,
                      C2 ? env_par : nullptr, C2 && NW > 0 ? env_rnd : nullptr, env_seed};
    return launch_smem(rollout_env_kernel, d->P, sizeof(PlugSmem), (hipStream_t)stream, what, a, plug_layout());
}

PGM_ENVPLUG_EXPORT int pgm_envplug_rollout(const pgm_dims* d, const float* params, double* sd, int32_t* si,
                                           int32_t* episode, const double* table, int32_t R, int32_t reset_count,
                                           const pgm_env_state* st, const pgm_norm_state* ns,
                                           const pgm_rollout_buf* rb, const float* stream_in, uint64_t seed,
                                           int32_t carry, pgm_stream_t stream) {
    if (C2) return refuse_contract2("pgm_envplug_rollout");
    return plug_rollout("pgm_envplug_rollout", d, params, sd, si, episode, table, R, reset_count, st, ns, rb, stream_in,
                        seed, carry, nullptr, nullptr, 0, stream);
}

PGM_ENVPLUG_EXPORT int pgm_envplug_rollout_ex(const pgm_dims* d, const float* params, double* sd, int32_t* si,
                                              int32_t* episode, const double* table, int32_t R, int32_t reset_count,
                                              const pgm_env_state* st, const pgm_norm_state* ns,
                                              const pgm_rollout_buf* rb, const float* stream_in, uint64_t seed,
                                              int32_t carry, const double* env_par, const double* env_rnd,
                                              uint64_t env_seed, pgm_stream_t stream) {
    return plug_rollout("pgm_envplug_rollout_ex", d, params, sd, si, episode, table, R, reset_count, st, ns, rb,
                        stream_in, seed, carry, env_par, env_rnd, env_seed, stream);
}

static int plug_eval(const char* what, const pgm_dims* d, const float* params, const double* table, int32_t R,
                     int32_t reset_count, const double* ob_mean, const double* ob_var, int32_t eval_num,
                     int32_t use_ob_rms, int32_t raw, double gamma, double* objs_out, const double* env_par,
                     uint64_t env_seed, pgm_stream_t stream) {
    if (!d || !params || (Env::RW > 0 && !table) || !objs_out || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("%s: null pointer (ob_mean / ob_var are required with use_ob_rms)", what);
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: the rows are the evaluation episodes
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, what)) return rc;
    if (int rc = check_plug_dims(&dd, what)) return rc;
    if (eval_num < 1 || eval_num > NMAX) {
        set_error("%s: eval_num=%d evaluation episodes outside [1, %d]", what, eval_num, NMAX);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_plug_table(R, reset_count, eval_num, what)) return rc;
    if (int rc = check_env_par(env_par, what)) return rc;
    PlugEvalArgs a{d->P,   params, table, R, ob_mean, ob_var, eval_num, use_ob_rms != 0, raw != 0, gamma, objs_out,
                   C2 ? env_par : nullptr, env_seed};
    return launch_smem(eval_env_kernel, d->P, sizeof(PlugSmem), (hipStream_t)stream, what, a, plug_layout());
}

PGM_ENVPLUG_EXPORT int pgm_envplug_eval(const pgm_dims* d, const float* params, const double* table, int32_t R,
                                        int32_t reset_count, const double* ob_mean, const double* ob_var,
                                        int32_t eval_num, int32_t use_ob_rms, int32_t raw, double gamma,
                                        double* objs_out, pgm_stream_t stream) {
    if (C2) return refuse_contract2("pgm_envplug_eval");
    return plug_eval("pgm_envplug_eval", d, params, table, R, reset_count, ob_mean, ob_var, eval_num, use_ob_rms, raw,
                     gamma, objs_out, nullptr, 0, stream);
}

PGM_ENVPLUG_EXPORT int pgm_envplug_eval_ex(const pgm_dims* d, const float* params, const double* table, int32_t R,
                                           int32_t reset_count, const double* ob_mean, const double* ob_var,
                                           int32_t eval_num, int32_t use_ob_rms, int32_t raw, double gamma,
                                           double* objs_out, const double* env_par, uint64_t env_seed,
                                           pgm_stream_t stream) {
    return plug_eval("pgm_envplug_eval_ex", d, params, table, R, reset_count, ob_mean, ob_var, eval_num, use_ob_rms,
                     raw, gamma, objs_out, env_par, env_seed, stream);
}

// Host only: launches nothing and needs no device.
static int plug_transition(const char* what, int32_t n, const double* sd, const int32_t* si, const int32_t* elapsed,
                           const int32_t* episode, const int32_t* row, const void* action, const double* table,
                           int32_t R, int32_t reset_count, const double* env_par, const double* w, double* sd_out,
                           int32_t* si_out, int32_t* elapsed_out, int32_t* episode_out, double* obs_out,
                           double* obj_out, double* reward_out, int32_t* done_out, int32_t* bad_out) {
    if (n < 0 || (Env::SD > 0 && (!sd || !sd_out)) || (Env::SI > 0 && (!si || !si_out)) || !elapsed || !episode ||
        !row || !action || (Env::RW > 0 && !table) || !elapsed_out || !episode_out || !obs_out || !obj_out ||
        !reward_out || !done_out || !bad_out) {
        set_error("%s: null pointer or negative n", what);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_plug_table(R, reset_count, 1, what)) return rc;
    for (int32_t i = 0; i < n; ++i) {
        if (row[i] < 0 || row[i] >= reset_count || episode[i] < 0 || elapsed[i] < 0) {
            set_error("%s: item %d has row %d (the reset table has %d rows), episode %d and elapsed %d", what, i,
                      row[i], reset_count, episode[i], elapsed[i]);
            return PGM_E_INVALID_ARG;
        }
        if (CAT && (((const int32_t*)action)[i] < 0 || ((const int32_t*)action)[i] >= EA)) {
            set_error("%s: item %d has action index %d outside [0, %d)", what, i, ((const int32_t*)action)[i], EA);
            return PGM_E_INVALID_ARG;
        }
    }
    if (int rc = check_env_par(env_par, what)) return rc;
    if (NW > 0 && !w) {
        set_error("%s: w is a null pointer, the header takes NW = %d uniforms per step", what, NW);
        return PGM_E_INVALID_ARG;
    }
    for (int32_t i = 0; i < n; ++i) {
        const pgm_env_ctx ctx{C2 ? env_par : nullptr, C2 && NW > 0 ? w + (size_t)i * NW : nullptr};
        envplug::State s = {};
        for (int j = 0; j < Env::SD; ++j) s.sd[j] = sd[(size_t)i * Env::SD + j];
        for (int j = 0; j < Env::SI; ++j) s.si[j] = si[(size_t)i * Env::SI + j];
        s.elapsed = elapsed[i];
        s.episode = episode[i];
        const double* rp = table + (size_t)row[i] * R * Env::RW;
        envplug::StepOut o;
        if (CAT) {
            o = envplug::transition(s, envplug::Action{nullptr, (int)((const int32_t*)action)[i]}, rp, R, ctx);
        } else {
            o = envplug::transition(s, envplug::Action{(const float*)action + (size_t)i * EA, 0}, rp, R, ctx);
        }
        for (int j = 0; j < Env::SD; ++j) sd_out[(size_t)i * Env::SD + j] = s.sd[j];
        for (int j = 0; j < Env::SI; ++j) si_out[(size_t)i * Env::SI + j] = s.si[j];
        elapsed_out[i] = s.elapsed;
        episode_out[i] = s.episode;
        envplug::call_observe<Env>(s.sd, s.si, obs_out + (size_t)i * EO, ctx.par);
        for (int k = 0; k < EK; ++k) obj_out[(size_t)i * EK + k] = o.obj[k];
        reward_out[i] = o.reward;
        done_out[i] = o.done;
        bad_out[i] = o.bad;
    }
    return PGM_OK;
}

PGM_ENVPLUG_EXPORT int pgm_envplug_transition(int32_t n, const double* sd, const int32_t* si, const int32_t* elapsed,
                                              const int32_t* episode, const int32_t* row, const void* action,
                                              const double* table, int32_t R, int32_t reset_count, double* sd_out,
                                              int32_t* si_out, int32_t* elapsed_out, int32_t* episode_out,
                                              double* obs_out, double* obj_out, double* reward_out, int32_t* done_out,
                                              int32_t* bad_out) {
    if (C2) return refuse_contract2("pgm_envplug_transition");
    return plug_transition("pgm_envplug_transition", n, sd, si, elapsed, episode, row, action, table, R, reset_count,
                           nullptr, nullptr, sd_out, si_out, elapsed_out, episode_out, obs_out, obj_out, reward_out,
                           done_out, bad_out);
}

PGM_ENVPLUG_EXPORT int pgm_envplug_transition_ex(int32_t n, const double* sd, const int32_t* si,
                                                 const int32_t* elapsed, const int32_t* episode, const int32_t* row,
                                                 const void* action, const double* table, int32_t R,
                                                 int32_t reset_count, const double* env_par, const double* w,
                                                 double* sd_out, int32_t* si_out, int32_t* elapsed_out,
                                                 int32_t* episode_out, double* obs_out, double* obj_out,
                                                 double* reward_out, int32_t* done_out, int32_t* bad_out) {
    return plug_transition("pgm_envplug_transition_ex", n, sd, si, elapsed, episode, row, action, table, R,
                           reset_count, env_par, w, sd_out, si_out, elapsed_out, episode_out, obs_out, obj_out,
                           reward_out, done_out, bad_out);
}

static int plug_reset(const char* what, int32_t n, const int32_t* row, const int32_t* episode, const double* table,
                      int32_t R, int32_t reset_count, const double* env_par, double* sd_out, int32_t* si_out,
                      double* obs_out) {
    if (n < 0 || !row || !episode || (Env::RW > 0 && !table) || (Env::SD > 0 && !sd_out) || (Env::SI > 0 && !si_out) ||
        !obs_out) {
        set_error("%s: null pointer or negative n", what);
        return PGM_E_INVALID_ARG;
    }
    if (int rc = check_plug_table(R, reset_count, 1, what)) return rc;
    for (int32_t i = 0; i < n; ++i)
        if (row[i] < 0 || row[i] >= reset_count || episode[i] < 0) {
            set_error("%s: item %d has row %d (the reset table has %d rows) and episode %d", what, i, row[i],
                      reset_count, episode[i]);
            return PGM_E_INVALID_ARG;
        }
    if (int rc = check_env_par(env_par, what)) return rc;
    const pgm_env_ctx ctx{C2 ? env_par : nullptr, nullptr};
    for (int32_t i = 0; i < n; ++i) {
        envplug::State s = {};
        envplug::start(s, table + ((size_t)row[i] * R + episode[i] % R) * Env::RW, ctx);
        for (int j = 0; j < Env::SD; ++j) sd_out[(size_t)i * Env::SD + j] = s.sd[j];
        for (int j = 0; j < Env::SI; ++j) si_out[(size_t)i * Env::SI + j] = s.si[j];
        envplug::call_observe<Env>(s.sd, s.si, obs_out + (size_t)i * EO, ctx.par);
    }
    return PGM_OK;
}

PGM_ENVPLUG_EXPORT int pgm_envplug_reset(int32_t n, const int32_t* row, const int32_t* episode, const double* table,
                                         int32_t R, int32_t reset_count, double* sd_out, int32_t* si_out,
                                         double* obs_out) {
    if (C2) return refuse_contract2("pgm_envplug_reset");
    return plug_reset("pgm_envplug_reset", n, row, episode, table, R, reset_count, nullptr, sd_out, si_out, obs_out);
}

PGM_ENVPLUG_EXPORT int pgm_envplug_reset_ex(int32_t n, const int32_t* row, const int32_t* episode, const double* table,
                                            int32_t R, int32_t reset_count, const double* env_par, double* sd_out,
                                            int32_t* si_out, double* obs_out) {
    return plug_reset("pgm_envplug_reset_ex", n, row, episode, table, R, reset_count, env_par, sd_out, si_out, obs_out);
}

// ---- contract 2: what the header declares, and the env-noise stream on the host
PGM_ENVPLUG_EXPORT int pgm_envplug_contract(void) { return envplug::CONTRACT; }

PGM_ENVPLUG_EXPORT int pgm_envplug_info_ex(int32_t* out) {
    if (!out) {
        set_error("pgm_envplug_info_ex: null pointer");
        return PGM_E_INVALID_ARG;
    }
    if (int rc = pgm_envplug_info(out)) return rc;
    out[8] = envplug::CONTRACT;
    out[9] = NP;
    out[10] = NW;
    return PGM_OK;
}

PGM_ENVPLUG_EXPORT int pgm_envplug_params(char* names, int32_t cap, double* defaults) {
    const char* text = NP > 0 ? envplug::names_of<Env>::text : "";
    if (names) {
        const size_t len = strlen(text);
        if (cap < 0 || (size_t)cap < len + 1) {
            set_error("pgm_envplug_params: cap = %d bytes, the names need %d", cap, (int)len + 1);
            return PGM_E_INVALID_ARG;
        }
        memcpy(names, text, len + 1);
    }
    if (defaults)
        for (int i = 0; i < NP; ++i) defaults[i] = envplug::defaults_of<Env>::at(i);
    return PGM_OK;
}

PGM_ENVPLUG_EXPORT int pgm_envplug_uniforms(uint64_t seed, uint64_t start, int64_t n, double* out) {
    if (n < 0 || (n > 0 && !out)) {
        set_error("pgm_envplug_uniforms: null pointer or negative n");
        return PGM_E_INVALID_ARG;
    }
    const uint64_t key = envplug::noise_key(seed);
    for (int64_t k = 0; k < n; ++k) out[k] = envplug::u53_at(key, start + (uint64_t)k);
    return PGM_OK;
}
