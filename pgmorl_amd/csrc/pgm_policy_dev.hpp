// Device functions shared by the policy / env kernels (pgm_policy_env.hip) and the host-stepped environment kernels
// (pgm_hostenv.hip): the LDS images of a task, the tower and head descriptions (plain / LayerNorm towers, Gaussian /
// Categorical head) with the policy forward written once for them, the synthetic env and the VecNormalize arithmetic,
// and the launch helpers of the workgroup-per-task kernels.  One workgroup (256 threads)
// per task; see pgm_policy_env.hip for the reference seams.
#pragma once
#include "pgm_dispatch.hpp"
#include "pgm_rollout.hpp"

namespace pgm {

template <int O>
constexpr bool w1_in_lds() { return O <= 128; }
template <int O>
constexpr bool spec_in_lds() { return O <= 128; }


// ------------------------------------------------------------------------------------------
// LDS images
template <int O, int A, int K>
struct PolSmem {
    float bv[K];
    float bm[A];
    float logstd[A];
    alignas(16) float x[NMAX][opad<O>()];   // fp32 policy input rows
    alignas(16) float h1[NMAX][H2];
    float val[NMAX][K];
    float mu[NMAX][A];
    float lp[NMAX][A];
};

template <int O, int A, int K>
struct SpecSmem {  // fp64 env constants (only for O <= 128; Humanoid reads them from HBM/L2)
    static constexpr int OL = spec_in_lds<O>() ? O : 1;
    double U[OL][A], V[K][OL], d[OL], c[OL], s0[NMAX][OL];
    double ebase[K], ecoef[K], lo[A], hi[A];
};

template <int O, int A, int K>
struct EnvSmem {
    SpecSmem<O, A, K> sp;
    double s[NMAX][O];        // env state
    double snew[NMAX][O];     // observation returned by step (post auto-reset)
    double ac[NMAX][A];       // clipped action
    double objraw[NMAX][K];   // info['obj'] before obj_rms scaling
    double obj_acc[NMAX][K];  // VecNormalize.obj
    double ret[NMAX];         // VecNormalize.ret
    double ob_mean[O], ob_var[O], ob_inv[O];
    double obj_mean[K], obj_var[K], obj_inv[K];
    double ob_count, obj_count, ret_mean, ret_var, ret_count;
    double objsum[K];         // evaluation accumulator
    int elapsed[NMAX], done[NMAX], bad[NMAX];
    int obj_valid;
};


// env-constant accessors: LDS copy when it fits, HBM otherwise
template <int O, int A, int K>
struct Spec {
    const EnvSmem<O, A, K>& E;
    const pgm_env_spec& g;
    const double* s0g;
    __device__ double U(int o, int a) const { if constexpr (spec_in_lds<O>()) return E.sp.U[o][a]; else return g.U[o * A + a]; }
    __device__ double V(int k, int o) const { if constexpr (spec_in_lds<O>()) return E.sp.V[k][o]; else return g.V[k * O + o]; }
    __device__ double d(int o) const { if constexpr (spec_in_lds<O>()) return E.sp.d[o]; else return g.d[o]; }
    __device__ double c(int o) const { if constexpr (spec_in_lds<O>()) return E.sp.c[o]; else return g.c[o]; }
    __device__ double s0(int n, int o) const { if constexpr (spec_in_lds<O>()) return E.sp.s0[n][o]; else return s0g[n * O + o]; }
    __device__ double ebase(int k) const { return E.sp.ebase[k]; }
    __device__ double ecoef(int k) const { return E.sp.ecoef[k]; }
    __device__ double lo(int a) const { return E.sp.lo[a]; }
    __device__ double hi(int a) const { return E.sp.hi[a]; }
};

template <int O, int A, int K>
__device__ void load_spec(EnvSmem<O, A, K>& E, const pgm_env_spec& g, const double* s0, int N) {
    const int t = threadIdx.x;
    if constexpr (spec_in_lds<O>()) {
        for (int i = t; i < O * A; i += RT) E.sp.U[i / A][i % A] = g.U[i];
        for (int i = t; i < K * O; i += RT) E.sp.V[i / O][i % O] = g.V[i];
        for (int i = t; i < O; i += RT) {
            E.sp.d[i] = g.d[i];
            E.sp.c[i] = g.c[i];
        }
        for (int i = t; i < N * O; i += RT) E.sp.s0[i / O][i % O] = s0[i];
    }
    if (t < K) {
        E.sp.ebase[t] = g.ebase[t];
        E.sp.ecoef[t] = g.ecoef[t];
    }
    if (t < A) {
        E.sp.lo[t] = g.act_lo[t];
        E.sp.hi[t] = g.act_hi[t];
    }
}

// ------------------------------------------------------------------------------------------
// policy: a kernel body is written once for a Towers type (which hidden layers run) and a Head type (what the action
// distribution emits); the kernels are its instantiations.
//
// Per-thread register image of the weights one lane needs: column c = (tower m, unit j) of both
// tower layers and unit j's head row.  Loaded once per launch (weights are constant inside a rollout).
template <int O>
constexpr bool w1_in_regs() { return O <= 32; }

template <int O, int A, int K>
struct TowerW {
    float w1[w1_in_regs<O>() ? O : 1];
    float w2[H];
    float wh[A > K ? A : K];
};
template <int O, int A, int K>
struct PolReg : TowerW<O, A, K> {
    float b1, b2;
};
template <int O, int A, int K>
struct PolRegLN : TowerW<O, A, K> {
    float g1, be1, g2, be2;
};

// the lane's layer-1 / layer-2 columns and head row, from the offsets of this lane's tower (m: 0 critic, 1 actor)
template <int O, int A, int K>
__device__ void load_tower_w(TowerW<O, A, K>& R, const float* __restrict__ prm, int lane, int m, int offW1, int offW2,
                             int offVW, int offMW) {
    if constexpr (w1_in_regs<O>()) {
#pragma unroll
        for (int k = 0; k < O; ++k) R.w1[k] = prm[offW1 + k * H + lane];
    }
#pragma unroll
    for (int k = 0; k < H; ++k) R.w2[k] = prm[offW2 + k * H + lane];
    constexpr int NQ = A > K ? A : K;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        R.wh[q] = m == 0 ? (q < K ? prm[offVW + lane * K + q] : 0.f) : (q < A ? prm[offMW + lane * A + q] : 0.f);
}

// value bias, head bias and (Gaussian head) logstd -> LDS
template <bool LOGSTD, int O, int A, int K>
__device__ void load_head_scalars(PolSmem<O, A, K>& S, const float* __restrict__ prm, int offVB, int offMB, int offLS) {
    const int t = threadIdx.x;
    if (t < K) S.bv[t] = prm[offVB + t];
    if (t < A) {
        S.bm[t] = prm[offMB + t];
        if constexpr (LOGSTD) S.logstd[t] = prm[offLS + t];
    }
}

// 1 / sqrt(x) in fp32: hardware estimate + one Newton step (<= 1 ulp)
__device__ __forceinline__ float rsqrt_nr(float x) {
    const float r = __builtin_amdgcn_rsqf(x);
    return r * fmaf(-0.5f * x * r, r, 1.5f);
}
// LayerNorm over the wave's 64 lanes + affine + tanh: the variance is the mean of the mean-subtracted squares
// (E[z^2] - mean^2 cancels in fp32)
__device__ __forceinline__ float ln_tanh64(float z, float g, float be) {
    const float mu = wave_sum64(z) * (1.f / 64.f);
    const float dz = z - mu;
    const float var = wave_sum64(dz * dz) * (1.f / 64.f);
    return tanh_f(fmaf(dz * rsqrt_nr(var + 1e-5f), g, be));
}

// Plain towers (model.py:201-256): Linear -> tanh, twice per tower.  Layer 1 streams from global memory for O > 32.
struct PlainTowers {
    using Lay = Layout;
    template <int O, int A, int K>
    using Reg = PolReg<O, A, K>;
    template <int O>
    static constexpr bool w1_global = !w1_in_regs<O>();
    template <int O, int A, int K>
    static __device__ void load_reg(Reg<O, A, K>& R, const float* __restrict__ prm, const Lay& L) {
        const int lane = threadIdx.x & 63, m = (threadIdx.x >> 6) & 1;
        load_tower_w(R, prm, lane, m, m == 0 ? L.off[PGM_P_CRITIC_W1] : L.off[PGM_P_ACTOR_W1],
                     m == 0 ? L.off[PGM_P_CRITIC_W2] : L.off[PGM_P_ACTOR_W2], L.off[PGM_P_VALUE_W],
                     L.off[PGM_P_MEAN_W]);
        R.b1 = prm[(m == 0 ? L.off[PGM_P_CRITIC_B1] : L.off[PGM_P_ACTOR_B1]) + lane];
        R.b2 = prm[(m == 0 ? L.off[PGM_P_CRITIC_B2] : L.off[PGM_P_ACTOR_B2]) + lane];
    }
    template <bool LOGSTD, int O, int A, int K>
    static __device__ void load_smem(PolSmem<O, A, K>& S, const float* __restrict__ prm, const Lay& L) {
        load_head_scalars<LOGSTD>(S, prm, L.off[PGM_P_VALUE_B], L.off[PGM_P_MEAN_B], L.off[PGM_P_LOGSTD]);
    }
    static __device__ const float* w1_column(const float* prm, const Lay& L, int m) {
        return prm + (m == 0 ? L.off[PGM_P_CRITIC_W1] : L.off[PGM_P_ACTOR_W1]);
    }
    template <class R>
    static __device__ float acc1(const R& r) { return r.b1; }
    template <class R>
    static __device__ float acc2(const R& r) { return r.b2; }
    template <class R>
    static __device__ float act1(float z, const R&) { return tanh_f(z); }
    template <class R>
    static __device__ float act2(float z, const R&) { return tanh_f(z); }
};

// LayerNorm towers (pgm_dims.LN = 1; model.py:201-256 with layernorm=True): Linear(bias=False) -> LayerNorm(64) ->
// tanh, twice per tower.  The 64 pre-activations of a row sit in one wave, so the LayerNorm mean and the variance of
// the mean-subtracted values are 64-lane DPP sums (wave_sum64, no LDS round trip).  obs_dim <= 32 only (check_ln).
struct LNTowers {
    using Lay = LayoutLN;
    template <int O, int A, int K>
    using Reg = PolRegLN<O, A, K>;
    template <int O>
    static constexpr bool w1_global = false;
    template <int O, int A, int K>
    static __device__ void load_reg(Reg<O, A, K>& R, const float* __restrict__ prm, const Lay& L) {
        const int lane = threadIdx.x & 63, m = (threadIdx.x >> 6) & 1;
        const int b = m == 0 ? PGM_PL_CRITIC_W1 : PGM_PL_ACTOR_W1;  // the tower's six tensors are consecutive
        load_tower_w(R, prm, lane, m, L.off[b], L.off[b + 3], L.off[PGM_PL_VALUE_W], L.off[PGM_PL_MEAN_W]);
        R.g1 = prm[L.off[b + 1] + lane];
        R.be1 = prm[L.off[b + 2] + lane];
        R.g2 = prm[L.off[b + 4] + lane];
        R.be2 = prm[L.off[b + 5] + lane];
    }
    template <bool LOGSTD, int O, int A, int K>
    static __device__ void load_smem(PolSmem<O, A, K>& S, const float* __restrict__ prm, const Lay& L) {
        load_head_scalars<LOGSTD>(S, prm, L.off[PGM_PL_VALUE_B], L.off[PGM_PL_MEAN_B], L.off[PGM_PL_LOGSTD]);
    }
    template <class R>
    static __device__ float acc1(const R&) { return 0.f; }
    template <class R>
    static __device__ float acc2(const R&) { return 0.f; }
    template <class R>
    static __device__ float act1(float z, const R& r) { return ln_tanh64(z, r.g1, r.be1); }
    template <class R>
    static __device__ float act2(float z, const R& r) { return ln_tanh64(z, r.g2, r.be2); }
};

// value [N][K] -> S.val, head outputs [N][A] (action mean / logits) -> S.mu, from S.x.  Wave-local: wave w computes
// tower m = w & 1 for rows r = (w >> 1) + 2i; layer 1 -> layer 2 exchanges h1 inside the wave through LDS
// (no workgroup barrier), the heads are 64-lane butterfly sums of h2 * W_head over the tower's units.
// The float4 pad columns of S.x are read and never used.  Ends with one barrier (val/mu visible to every wave).
template <class Tw, int O, int A, int K>
__device__ void policy_forward(PolSmem<O, A, K>& S, const typename Tw::template Reg<O, A, K>& R, int N,
                               const float* __restrict__ prm, const typename Tw::Lay& L) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, m = w & 1, rg = w >> 1, c = m * H + lane;
    constexpr int RPT = NMAX / 2;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {  // tower layer 1
        const int r = rg + 2 * i;
        if (r < N) {
            float acc = Tw::acc1(R);
            if constexpr (!Tw::template w1_global<O>) {
#pragma unroll
                for (int k = 0; k < opad<O>(); k += 4) {
                    const float4 x = *reinterpret_cast<const float4*>(&S.x[r][k]);
                    acc = fmaf(x.x, R.w1[k], acc);
                    if (k + 1 < O) acc = fmaf(x.y, R.w1[k + 1], acc);
                    if (k + 2 < O) acc = fmaf(x.z, R.w1[k + 2], acc);
                    if (k + 3 < O) acc = fmaf(x.w, R.w1[k + 3], acc);
                }
            } else {
                const float* gw = Tw::w1_column(prm, L, m) + lane;
#pragma unroll 8
                for (int k = 0; k < O; ++k) acc = fmaf(S.x[r][k], gw[k * H], acc);
            }
            S.h1[r][c] = Tw::act1(acc, R);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // h1 row visible to this wave (lockstep)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < RPT; ++i) {  // tower layer 2 + heads
        const int r = rg + 2 * i;
        if (r < N) {
            float a0 = Tw::acc2(R), a1 = 0.f, a2 = 0.f, a3 = 0.f;  // four short chains instead of one of 64
#pragma unroll
            for (int k = 0; k < H; k += 4) {
                const float4 h = *reinterpret_cast<const float4*>(&S.h1[r][m * H + k]);
                a0 = fmaf(h.x, R.w2[k], a0);
                a1 = fmaf(h.y, R.w2[k + 1], a1);
                a2 = fmaf(h.z, R.w2[k + 2], a2);
                a3 = fmaf(h.w, R.w2[k + 3], a3);
            }
            const float h2 = Tw::act2((a0 + a1) + (a2 + a3), R);
            if (m == 0) {
#pragma unroll
                for (int q = 0; q < K; ++q) {
                    const float v = wave_sum64(h2 * R.wh[q]);
                    if (lane == 0) S.val[r][q] = v + S.bv[q];
                }
            } else {
#pragma unroll
                for (int q = 0; q < A; ++q) {
                    const float v = wave_sum64(h2 * R.wh[q]);
                    if (lane == 0) S.mu[r][q] = v + S.bm[q];
                }
            }
        }
    }
    lds_sync();
}

// The opening of every policy kernel body: the task's weights -> registers / LDS, n input rows [n][O] -> S.x
template <class Tw, bool LOGSTD, int O, int A, int K>
__device__ void load_policy(PolSmem<O, A, K>& S, typename Tw::template Reg<O, A, K>& R, const float* __restrict__ prm,
                            const typename Tw::Lay& L) {
    Tw::template load_smem<LOGSTD>(S, prm, L);
    Tw::load_reg(R, prm, L);
}
template <int O, int A, int K>
__device__ void load_rows(PolSmem<O, A, K>& S, const float* __restrict__ rows, int n) {
    for (int i = threadIdx.x; i < n * O; i += RT) S.x[i / O][i % O] = rows[i];
}
template <int O, int A, int K>
__device__ void store_values(const PolSmem<O, A, K>& S, float* __restrict__ val, int n) {
    for (int i = threadIdx.x; i < n * K; i += RT) val[i] = S.val[i / K][i % K];
}

// ---- heads.  emit(S, n, rnd, storage, out, logp), called by the whole workgroup once S.mu holds the head outputs of
// n rows: the action of every row (drawn from rnd, [n][width] random inputs; the mode when rnd is NULL) -> out
// ([n][width] action_t) and, as fp32, -> storage (rollout storage; NULL: none); its log-prob -> logp ([n]; NULL: none).
__device__ __forceinline__ float gauss_logp_term(float av, float mu, float ls, float sd) {
    const float dz = (av - mu) / sd;
    return -0.5f * dz * dz - ls - LOG_SQRT_2PI;
}

// DiagGaussian (distributions.py:29-40,71-90): torch.normal(mean, std) = z*std + mean; log-prob summed over A
struct GaussHead {
    using action_t = float;
    static constexpr bool has_logstd = true;
    template <int A>
    static constexpr int width = A;
    template <int O, int A, int K>
    static __device__ void emit(PolSmem<O, A, K>& S, int n, const float* rnd, float* storage, float* out, float* logp) {
        const int t = threadIdx.x;
        for (int i = t; i < n * A; i += RT) {
            const int r = i / A, j = i % A;
            const float mu = S.mu[r][j], ls = S.logstd[j], sd = expf(ls);
            const float av = rnd ? fmaf(rnd[i], sd, mu) : mu;
            if (logp) S.lp[r][j] = gauss_logp_term(av, mu, ls, sd);
            if (storage) storage[i] = av;
            out[i] = av;  // raw, unclipped: the env clips (as the reference's does)
        }
        if (!logp) return;  // uniform over the grid
        __syncthreads();
        if (t < n) {
            float s = 0.f;
            for (int j = 0; j < A; ++j) s += S.lp[t][j];
            logp[t] = s;
        }
    }
};

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

// Categorical (distributions.py:17-27,54-68): the head's Linear has the shape of fc_mean, so S.mu holds the logits;
// one integer action per row (its index, exact in fp32, in the rollout storage), one uniform per row
struct CatHead {
    using action_t = int32_t;
    static constexpr bool has_logstd = false;
    template <int A>
    static constexpr int width = 1;
    template <int O, int A, int K>
    static __device__ void emit(PolSmem<O, A, K>& S, int n, const float* rnd, float* storage, int32_t* out,
                                float* logp) {
        const int t = threadIdx.x;
        if (t < n) {
            float lp;
            const int act = cat_sample<A>(S.mu[t], rnd == nullptr, rnd ? rnd[t] : 0.f, lp);
            if (storage) storage[t] = (float)act;
            out[t] = act;
            if (logp) logp[t] = lp;
        }
    }
};

// policy_forward / PlainTowers address the towers, the value head and the head's Linear through a plain Layout: the
// categorical layout has the same first twelve tensors (no logstd; CatHead never loads it)
inline Layout cat_as_plain(const LayoutCat& C) {
    Layout L;
    for (int i = 0; i < PGM_NUM_PARAM_TENSORS_CAT; ++i) L.off[i] = C.off[i];
    L.off[PGM_P_LOGSTD] = 0;
    L.total = C.total;
    return L;
}

// mopg.py:37-38: fp64 normalisation of a raw observation with the frozen statistics, fixed eps / clip, then the fp32
// cast (the observation is NOT rounded through fp32 first).  inv = eval_ob_inv(var); without use_ob the cast alone.
__device__ __forceinline__ double eval_ob_inv(double var) { return 1.0 / sqrt(var + 1e-8); }
__device__ __forceinline__ float eval_normalise(double v, int use_ob, double mean, double inv) {
    if (use_ob) v = clipd((v - mean) * inv, -10.0, 10.0);
    return (float)v;
}

// ------------------------------------------------------------------------------------------
// env.  SYNTH = false leaves out the synthetic env's own state (st.s, st.elapsed: the host-stepped kernels, whose
// st.s / st.elapsed / st.s0 may be NULL)
template <bool SYNTH = true, int O, int A, int K>
__device__ void load_env(EnvSmem<O, A, K>& E, const pgm_env_state& st, const pgm_norm_state& ns, int p, int N) {
    const int t = threadIdx.x;
    if constexpr (SYNTH)
        for (int i = t; i < N * O; i += RT) E.s[i / O][i % O] = st.s[(size_t)p * N * O + i];
    for (int i = t; i < N * K; i += RT) E.obj_acc[i / K][i % K] = st.obj_acc[(size_t)p * N * K + i];
    if (t < N) {
        if constexpr (SYNTH) E.elapsed[t] = st.elapsed[p * N + t];
        E.ret[t] = st.ret[p * N + t];
    }
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

template <bool SYNTH = true, int O, int A, int K>
__device__ void store_env(const EnvSmem<O, A, K>& E, const pgm_env_state& st, const pgm_norm_state& ns, int p, int N) {
    const int t = threadIdx.x;
    if constexpr (SYNTH)
        for (int i = t; i < N * O; i += RT) st.s[(size_t)p * N * O + i] = E.s[i / O][i % O];
    for (int i = t; i < N * K; i += RT) st.obj_acc[(size_t)p * N * K + i] = E.obj_acc[i / K][i % K];
    if (t < N) {
        if constexpr (SYNTH) st.elapsed[p * N + t] = E.elapsed[t];
        st.ret[p * N + t] = E.ret[t];
    }
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

// s' = tanh(d*s + U a_c + c); objectives; time limit (E.ac filled, E.s current).  Two barriers.
template <int O, int A, int K>
__device__ void env_dynamics(EnvSmem<O, A, K>& E, const Spec<O, A, K>& sp, int N, int max_steps) {
    const int t = threadIdx.x;
    for (int i = t; i < N * O; i += RT) {
        const int n = i / O, o = i % O;
        double ua = 0.0;
#pragma unroll
        for (int a = 0; a < A; ++a) ua += sp.U(o, a) * E.ac[n][a];
        E.snew[n][o] = tanh_d(sp.d(o) * E.s[n][o] + ua + sp.c(o));
    }
    lds_sync();
    for (int i = t; i < N * K; i += RT) {
        const int n = i / K, k = i % K;
        double v = 0.0, e2 = 0.0;
        for (int o = 0; o < O; ++o) v += sp.V(k, o) * E.snew[n][o];
#pragma unroll
        for (int a = 0; a < A; ++a) e2 += E.ac[n][a] * E.ac[n][a];
        E.objraw[n][k] = v + sp.ebase(k) - sp.ecoef(k) * e2;
    }
    if (t >= RT - N) {
        const int n = t - (RT - N);
        const int el = E.elapsed[n] + 1;
        const int d = el >= max_steps;
        E.done[n] = d;
        E.bad[n] = d && (el == max_steps);
        E.elapsed[n] = d ? 0 : el;
    }
    lds_sync();
}

// numpy's x.mean(0) / x.var(0) divide by N; for N a power of two the reciprocal is exact
struct DivN {
    double dn, rn;
    bool pow2;
    __device__ explicit DivN(int N) : dn((double)N), rn(1.0 / (double)N), pow2((N & (N - 1)) == 0) {}
    __device__ double operator()(double x) const { return pow2 ? x * rn : x / dn; }
};

// Mean / variance of the batch x(0..N-1), whose sum is given, Chan-merged into (mean, var) at `count`
template <class X>
__device__ __forceinline__ void batch_merge(double& mean, double& var, double count, int N, const DivN& divn,
                                            double sum, X&& x) {
    const double bm = divn(sum);
    double sq = 0.0;
    for (int n = 0; n < N; ++n) {
        const double dd = x(n) - bm;
        sq += dd * dd;
    }
    chan_merge(mean, var, count, bm, divn(sq), divn.dn);
}

// ob_rms of feature o over the N rows of E.snew (the observations the vec env returns: already the reset observation
// of a done env), whose sum is given, with the count from before this step.  use_ob only.
template <int O, int A, int K>
__device__ __forceinline__ void ob_merge(EnvSmem<O, A, K>& E, int o, int N, const NormCfg& nc, const DivN& divn,
                                         double sum) {
    batch_merge(E.ob_mean[o], E.ob_var[o], E.ob_count, N, divn, sum, [&](int n) { return E.snew[n][o]; });
    E.ob_inv[o] = 1.0 / sqrt(E.ob_var[o] + nc.eps);
}
template <int O, int A, int K>
__device__ void ob_stats(EnvSmem<O, A, K>& E, int N, const NormCfg& nc, const DivN& divn) {
    for (int o = threadIdx.x; o < O; o += RT) {
        double sum = 0.0;
        for (int n = 0; n < N; ++n) sum += E.snew[n][o];
        ob_merge(E, o, N, nc, divn, sum);
    }
}

// obj accumulators + obj_rms on objective threads (top of the block), ret_rms on one thread, on the discounted return
// of `reward` ([N]; NULL: the synthetic env's, always zero; vec_normalize.py:32,41-43)
template <int O, int A, int K>
__device__ void obj_ret_stats(EnvSmem<O, A, K>& E, int N, const NormCfg& nc, const DivN& divn,
                              const double* __restrict__ reward) {
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
            E.ret[n] = E.ret[n] * nc.gamma + (reward ? reward[n] : 0.0);
            sum += E.ret[n];
        }
        batch_merge(E.ret_mean, E.ret_var, E.ret_count, N, divn, sum, [&](int n) { return E.ret[n]; });
        E.ret_count += divn.dn;
    }
}

// VecNormalize statistics of one step (vec_normalize.py:29-43): ob_rms on feature threads (bottom of the block), the
// objective and return statistics at the top; all with the counts from before this step (they advance in
// vecnorm_emit).  One barrier.  vecnorm_stats: the synthetic env's step, with the auto-reset of the done envs
// (dummy_vec_env.py:45-56) folded into the pass that sums a feature; norm_stats: supplied transitions (the host's vec
// env has reset them) and their scalar reward.
template <int O, int A, int K>
__device__ void vecnorm_stats(EnvSmem<O, A, K>& E, const Spec<O, A, K>& sp, int N, const NormCfg& nc) {
    const DivN divn(N);
    for (int o = threadIdx.x; o < O; o += RT) {
        double sum = 0.0;
        for (int n = 0; n < N; ++n) {
            const double v = E.done[n] ? sp.s0(n, o) : E.snew[n][o];
            E.snew[n][o] = v;
            E.s[n][o] = v;
            sum += v;
        }
        if (nc.use_ob) ob_merge(E, o, N, nc, divn, sum);
    }
    obj_ret_stats(E, N, nc, divn, nullptr);
    lds_sync();
}
template <int O, int A, int K>
__device__ void norm_stats(EnvSmem<O, A, K>& E, int N, const NormCfg& nc, const double* __restrict__ reward) {
    const DivN divn(N);
    if (nc.use_ob) ob_stats(E, N, nc, divn);
    obj_ret_stats(E, N, nc, divn, reward);
    lds_sync();
}

// Fresh make_vec_envs + reset() (vec_normalize.py:10-27,63-66) on the reset observations in E.snew (row o written by
// thread o mod RT, or behind a barrier): returns and accumulators cleared, ob_rms, the normalised obs -> obs_out.
template <int O, int A, int K>
__device__ void vecnorm_reset(EnvSmem<O, A, K>& E, int N, const NormCfg& nc, float* obs_out) {
    const int t = threadIdx.x;
    if (t < N) E.ret[t] = 0.0;
    if (t == 0) E.obj_valid = 0;
    if (nc.use_ob) ob_stats(E, N, nc, DivN(N));
    __syncthreads();
    if (t == 0 && nc.use_ob) E.ob_count += (double)N;
    for (int i = t; i < N * O; i += RT) {
        const int o = i % O;
        double v = E.snew[i / O][o];
        if (nc.use_ob) v = clipd((v - E.ob_mean[o]) * E.ob_inv[o], -nc.clipob, nc.clipob);
        obs_out[i] = (float)v;
    }
}

// Normalised fp32 obs (-> xs rows and obs_out), scaled objectives, masks; zero the accumulators of
// done envs; advance the counts.  One barrier.
template <int O, int A, int K, int XS>
__device__ void vecnorm_emit(EnvSmem<O, A, K>& E, int N, const NormCfg& nc, float (*xs)[XS], float* obs_out,
                             float* rew_out, float* mask_out, float* bad_out) {
    const int t = threadIdx.x;
    for (int i = t; i < N * O; i += RT) {
        const int n = i / O, o = i % O;
        double v = E.snew[n][o];
        if (nc.use_ob) v = clipd((v - E.ob_mean[o]) * E.ob_inv[o], -nc.clipob, nc.clipob);
        const float f = (float)v;  // VecPyTorch .float() (envs.py:192)
        xs[n][o] = f;
        if (obs_out) obs_out[i] = f;
    }
    const int i = RT - 1 - t;
    if (i < N * K) {
        const int n = i / K, k = i % K;
        double r = E.objraw[n][k];
        if (nc.use_obj) r = clipd(r * E.obj_inv[k], -nc.cliprew, nc.cliprew);
        if (rew_out) rew_out[i] = (float)r;
        if (E.done[n]) E.obj_acc[n][k] = 0.0;
    }
    const int n = RT - 1 - N * K - t;
    if (n >= 0 && n < N) {
        if (mask_out) mask_out[n] = E.done[n] ? 0.f : 1.f;
        if (bad_out) bad_out[n] = E.bad[n] ? 0.f : 1.f;
        if (E.done[n]) E.ret[n] = 0.0;
    }
    if (t == 0) {
        if (nc.use_ob) E.ob_count += (double)N;
        if (nc.use_obj) E.obj_count += (double)N;
        E.obj_valid = 1;
    }
    lds_sync();
}

// Draw actions (torch.normal(mean, std) = z*std + mean), log-prob terms, clipped env action.
template <int O, int A, int K>
__device__ void sample_actions(PolSmem<O, A, K>& P, EnvSmem<O, A, K>& E, const Spec<O, A, K>& sp, int N, float eps,
                               float* act_out) {
    const int t = threadIdx.x;
    if (t < N * A) {
        const int n = t / A, j = t % A;
        const float mu = P.mu[n][j], ls = P.logstd[j], sd = expf(ls);
        const float av = fmaf(eps, sd, mu);
        P.lp[n][j] = gauss_logp_term(av, mu, ls, sd);
        if (act_out) act_out[t] = av;
        E.ac[n][j] = clipd((double)av, sp.lo(j), sp.hi(j));
    }
    lds_sync();
}

template <int O, int A, int K>
struct StepSmem {
    PolSmem<O, A, K> pol;
    EnvSmem<O, A, K> env;
};

// ------------------------------------------------------------------------------------------
// host side
template <class Kern, class... Args>
static int launch_smem(Kern k, int grid, size_t smem, hipStream_t s, const char* what, const Args&... args) {
    if (smem > 160 * 1024) {
        set_error("%s: LDS image %zu bytes exceeds 160 KiB", what, smem);
        return PGM_E_UNSUPPORTED;
    }
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return hip_fail(e, what);
    hipLaunchKernelGGL(k, dim3(grid), dim3(RT), smem, s, args...);
    return launch_status(what);
}

// f(Towers{}, layout, ic<O>, ic<A>, ic<K>) for the towers d->LN names and the dims of d (after check_ln, which has
// refused LayerNorm towers on obs_dim > 32: no such kernel is instantiated)
template <class F>
static int dispatch_towers(const pgm_dims* d, const char* what, F&& f) {
    if (d->LN) {
        const LayoutLN L = make_layout_ln(d->O, d->A, d->K, d->H);
        return dispatch_dims(d->O, d->A, d->K, what, [&](auto o, auto aa, auto k) -> int {
            if constexpr (decltype(o)::value > 32) {
                set_error("%s: LayerNorm towers need obs_dim <= 32", what);
                return PGM_E_UNSUPPORTED;
            } else {
                return f(LNTowers{}, L, o, aa, k);
            }
        });
    }
    const Layout L = make_layout(d->O, d->A, d->K, d->H);
    return dispatch_dims(d->O, d->A, d->K, what,
                         [&](auto o, auto aa, auto k) -> int { return f(PlainTowers{}, L, o, aa, k); });
}
// f(PlainTowers{}, layout, ic<O>, ic<A>, ic<K>) for a Categorical-head policy (after check_cat_dims)
template <class F>
static int dispatch_towers_cat(const pgm_dims* d, const char* what, F&& f) {
    const Layout L = cat_as_plain(make_layout_cat(d->O, d->A, d->K, d->H));
    return dispatch_dims_cat(d->O, d->A, d->K, what,
                             [&](auto o, auto aa, auto k) -> int { return f(PlainTowers{}, L, o, aa, k); });
}

inline bool spec_ok(const pgm_env_spec* sp) {
    return sp && sp->d && sp->U && sp->c && sp->V && sp->ebase && sp->ecoef && sp->act_lo && sp->act_hi &&
           sp->max_episode_steps > 0;
}
inline bool state_ok(const pgm_env_state* st) {
    return st && st->s && st->elapsed && st->obj_acc && st->obj_acc_valid && st->ret && st->s0;
}
inline bool norm_ok(const pgm_norm_state* ns) {
    return ns && ns->ob_mean && ns->ob_var && ns->ob_count && ns->ret_mean && ns->ret_var && ns->ret_count &&
           ns->obj_mean && ns->obj_var && ns->obj_count;
}

}  // namespace pgm
