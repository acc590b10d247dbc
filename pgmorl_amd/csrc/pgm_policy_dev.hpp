// Device functions shared by the policy / env kernels (pgm_policy_env.hip) and the host-stepped environment kernels
// (pgm_hostenv.hip): the LDS images of a task, the policy forward (plain and LayerNorm towers), the synthetic env and
// the VecNormalize arithmetic, and the launch helpers of the workgroup-per-task kernels.  One workgroup (256 threads)
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
// policy
template <int O, int A, int K>
__device__ void load_policy(PolSmem<O, A, K>& S, const float* __restrict__ prm, const Layout& L) {
    const int t = threadIdx.x;
    if (t < K) S.bv[t] = prm[L.off[PGM_P_VALUE_B] + t];
    if (t < A) {
        S.bm[t] = prm[L.off[PGM_P_MEAN_B] + t];
        S.logstd[t] = prm[L.off[PGM_P_LOGSTD] + t];
    }
}

// Per-thread register image of the weights one lane needs: column c = (tower m, unit j) of both
// tower layers and unit j's head row.  Loaded once per launch (weights are constant inside a rollout).
template <int O>
constexpr bool w1_in_regs() { return O <= 32; }

template <int O, int A, int K>
struct PolReg {
    float w1[w1_in_regs<O>() ? O : 1];
    float w2[H];
    float wh[A > K ? A : K];
    float b1, b2;
};

template <int O, int A, int K>
__device__ void load_polreg(PolReg<O, A, K>& R, const float* __restrict__ prm, const Layout& L) {
    const int t = threadIdx.x, lane = t & 63, m = (t >> 6) & 1;  // m: 0 critic, 1 actor
    const int offW1 = m == 0 ? L.off[PGM_P_CRITIC_W1] : L.off[PGM_P_ACTOR_W1];
    const int offW2 = m == 0 ? L.off[PGM_P_CRITIC_W2] : L.off[PGM_P_ACTOR_W2];
    if constexpr (w1_in_regs<O>()) {
#pragma unroll
        for (int k = 0; k < O; ++k) R.w1[k] = prm[offW1 + k * H + lane];
    }
#pragma unroll
    for (int k = 0; k < H; ++k) R.w2[k] = prm[offW2 + k * H + lane];
    constexpr int NQ = A > K ? A : K;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        R.wh[q] = m == 0 ? (q < K ? prm[L.off[PGM_P_VALUE_W] + lane * K + q] : 0.f)
                         : (q < A ? prm[L.off[PGM_P_MEAN_W] + lane * A + q] : 0.f);
    R.b1 = prm[(m == 0 ? L.off[PGM_P_CRITIC_B1] : L.off[PGM_P_ACTOR_B1]) + lane];
    R.b2 = prm[(m == 0 ? L.off[PGM_P_CRITIC_B2] : L.off[PGM_P_ACTOR_B2]) + lane];
}

// value [N][K] -> S.val, action mean [N][A] -> S.mu, from S.x.  Wave-local: wave w computes tower
// m = w & 1 for rows r = (w >> 1) + 2i; layer 1 -> layer 2 exchanges h1 inside the wave through LDS
// (no workgroup barrier), the heads are 64-lane butterfly sums of h2 * W_head over the tower's units.
// Ends with one barrier (val/mu visible to every wave).
template <int O, int A, int K>
__device__ void policy_forward(PolSmem<O, A, K>& S, const PolReg<O, A, K>& R, int N, const float* __restrict__ prm,
                               const Layout& L) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, m = w & 1, rg = w >> 1, c = m * H + lane;
    constexpr int RPT = NMAX / 2;
    const float* gw = prm + (m == 0 ? L.off[PGM_P_CRITIC_W1] : L.off[PGM_P_ACTOR_W1]) + lane;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {  // tower layer 1
        const int r = rg + 2 * i;
        if (r < N) {
            float acc = R.b1;
            if constexpr (w1_in_regs<O>()) {
#pragma unroll
                for (int k = 0; k < opad<O>(); k += 4) {
                    const float4 x = *reinterpret_cast<const float4*>(&S.x[r][k]);
                    acc = fmaf(x.x, R.w1[k], acc);
                    if (k + 1 < O) acc = fmaf(x.y, R.w1[k + 1], acc);
                    if (k + 2 < O) acc = fmaf(x.z, R.w1[k + 2], acc);
                    if (k + 3 < O) acc = fmaf(x.w, R.w1[k + 3], acc);
                }
            } else {
#pragma unroll 8
                for (int k = 0; k < O; ++k) acc = fmaf(S.x[r][k], gw[k * H], acc);
            }
            S.h1[r][c] = tanh_f(acc);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // h1 row visible to this wave (lockstep)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < RPT; ++i) {  // tower layer 2 + heads
        const int r = rg + 2 * i;
        if (r < N) {
            float a0 = R.b2, a1 = 0.f, a2 = 0.f, a3 = 0.f;  // four short chains instead of one of 64
#pragma unroll
            for (int k = 0; k < H; k += 4) {
                const float4 h = *reinterpret_cast<const float4*>(&S.h1[r][m * H + k]);
                a0 = fmaf(h.x, R.w2[k], a0);
                a1 = fmaf(h.y, R.w2[k + 1], a1);
                a2 = fmaf(h.z, R.w2[k + 2], a2);
                a3 = fmaf(h.w, R.w2[k + 3], a3);
            }
            const float h2 = tanh_f((a0 + a1) + (a2 + a3));
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

// ------------------------------------------------------------------------------------------
// env
template <int O, int A, int K>
__device__ void load_env(EnvSmem<O, A, K>& E, const pgm_env_state& st, const pgm_norm_state& ns, int p, int N) {
    const int t = threadIdx.x;
    for (int i = t; i < N * O; i += RT) E.s[i / O][i % O] = st.s[(size_t)p * N * O + i];
    for (int i = t; i < N * K; i += RT) E.obj_acc[i / K][i % K] = st.obj_acc[(size_t)p * N * K + i];
    if (t < N) {
        E.elapsed[t] = st.elapsed[p * N + t];
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

template <int O, int A, int K>
__device__ void store_env(const EnvSmem<O, A, K>& E, const pgm_env_state& st, const pgm_norm_state& ns, int p, int N) {
    const int t = threadIdx.x;
    for (int i = t; i < N * O; i += RT) st.s[(size_t)p * N * O + i] = E.s[i / O][i % O];
    for (int i = t; i < N * K; i += RT) st.obj_acc[(size_t)p * N * K + i] = E.obj_acc[i / K][i % K];
    if (t < N) {
        st.elapsed[p * N + t] = E.elapsed[t];
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

// Auto-reset + VecNormalize statistics: ob_rms on feature threads (bottom of the block), obj
// accumulators + obj_rms on objective threads (top), ret_rms on one thread; all with the counts
// from before this step (they advance in vecnorm_emit).  One barrier.
template <int O, int A, int K>
__device__ void vecnorm_stats(EnvSmem<O, A, K>& E, const Spec<O, A, K>& sp, int N, const NormCfg& nc) {
    const int t = threadIdx.x;
    const double dn = (double)N;
    // numpy's x.mean(0) / x.var(0) divide by N; for N a power of two the reciprocal is exact
    const bool pow2 = (N & (N - 1)) == 0;
    const double rn = 1.0 / dn;
    auto divn = [&](double x) { return pow2 ? x * rn : x / dn; };
    for (int o = t; o < O; o += RT) {
        double sum = 0.0;
        for (int n = 0; n < N; ++n) {
            const double v = E.done[n] ? sp.s0(n, o) : E.snew[n][o];
            E.snew[n][o] = v;
            E.s[n][o] = v;
            sum += v;
        }
        if (nc.use_ob) {
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
    if (t == RT - 1 - K) {  // ret_rms on the (always zero-reward) discounted return, vec_normalize.py:32,41-43
        double sum = 0.0;
        for (int n = 0; n < N; ++n) {
            E.ret[n] = E.ret[n] * nc.gamma + 0.0;
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
        const float dz = (av - mu) / sd;
        P.lp[n][j] = -0.5f * dz * dz - ls - LOG_SQRT_2PI;
        if (act_out) act_out[t] = av;
        E.ac[n][j] = clipd((double)av, sp.lo(j), sp.hi(j));
    }
    lds_sync();
}

// ------------------------------------------------------------------------------------------
// kernels
template <int O, int A, int K>
struct StepSmem {
    PolSmem<O, A, K> pol;
    EnvSmem<O, A, K> env;
};

// ------------------------------------------------------------------------------------------
// LayerNorm towers (pgm_dims.LN = 1; model.py:201-256 with layernorm=True): Linear(bias=False) -> LayerNorm(64) ->
// tanh, twice per tower.  One wave per (env row, tower) with a lane per hidden unit, as policy_forward: the 64
// pre-activations of a row sit in one wave, so the LayerNorm mean and the variance of the mean-subtracted values are
// 64-lane DPP sums (wave_sum64, no LDS round trip).  Env step, VecNormalize, insert bookkeeping and the counter RNG
// are the device functions above, unchanged; the kernels below are the plain ones with this forward.
template <int O, int A, int K>
struct PolRegLN {
    float w1[O];
    float w2[H];
    float wh[A > K ? A : K];
    float g1, be1, g2, be2;
};

template <int O, int A, int K>
__device__ void load_policy_ln(PolSmem<O, A, K>& S, const float* __restrict__ prm, const LayoutLN& L) {
    const int t = threadIdx.x;
    if (t < K) S.bv[t] = prm[L.off[PGM_PL_VALUE_B] + t];
    if (t < A) {
        S.bm[t] = prm[L.off[PGM_PL_MEAN_B] + t];
        S.logstd[t] = prm[L.off[PGM_PL_LOGSTD] + t];
    }
}

template <int O, int A, int K>
__device__ void load_polreg_ln(PolRegLN<O, A, K>& R, const float* __restrict__ prm, const LayoutLN& L) {
    const int t = threadIdx.x, lane = t & 63, m = (t >> 6) & 1;  // m: 0 critic, 1 actor
    const int b = m == 0 ? PGM_PL_CRITIC_W1 : PGM_PL_ACTOR_W1;   // the tower's six tensors are consecutive
#pragma unroll
    for (int k = 0; k < O; ++k) R.w1[k] = prm[L.off[b] + k * H + lane];
#pragma unroll
    for (int k = 0; k < H; ++k) R.w2[k] = prm[L.off[b + 3] + k * H + lane];
    constexpr int NQ = A > K ? A : K;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        R.wh[q] = m == 0 ? (q < K ? prm[L.off[PGM_PL_VALUE_W] + lane * K + q] : 0.f)
                         : (q < A ? prm[L.off[PGM_PL_MEAN_W] + lane * A + q] : 0.f);
    R.g1 = prm[L.off[b + 1] + lane];
    R.be1 = prm[L.off[b + 2] + lane];
    R.g2 = prm[L.off[b + 4] + lane];
    R.be2 = prm[L.off[b + 5] + lane];
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

// policy_forward with LayerNorm towers: same wave / row split, same outputs (S.val, S.mu), one barrier at the end
template <int O, int A, int K>
__device__ void policy_forward_ln(PolSmem<O, A, K>& S, const PolRegLN<O, A, K>& R, int N) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, m = w & 1, rg = w >> 1, c = m * H + lane;
    constexpr int RPT = NMAX / 2;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {  // tower layer 1
        const int r = rg + 2 * i;
        if (r < N) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < opad<O>(); k += 4) {
                const float4 x = *reinterpret_cast<const float4*>(&S.x[r][k]);
                acc = fmaf(x.x, R.w1[k], acc);
                if (k + 1 < O) acc = fmaf(x.y, R.w1[k + 1], acc);
                if (k + 2 < O) acc = fmaf(x.z, R.w1[k + 2], acc);
                if (k + 3 < O) acc = fmaf(x.w, R.w1[k + 3], acc);
            }
            S.h1[r][c] = ln_tanh64(acc, R.g1, R.be1);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // h1 row visible to this wave (lockstep)
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < RPT; ++i) {  // tower layer 2 + heads
        const int r = rg + 2 * i;
        if (r < N) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int k = 0; k < H; k += 4) {
                const float4 h = *reinterpret_cast<const float4*>(&S.h1[r][m * H + k]);
                a0 = fmaf(h.x, R.w2[k], a0);
                a1 = fmaf(h.y, R.w2[k + 1], a1);
                a2 = fmaf(h.z, R.w2[k + 2], a2);
                a3 = fmaf(h.w, R.w2[k + 3], a3);
            }
            const float h2 = ln_tanh64((a0 + a1) + (a2 + a3), R.g2, R.be2);
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

// ------------------------------------------------------------------------------------------
template <class Kern, class... Args>
static int launch_smem_ln(Kern k, int grid, size_t smem, hipStream_t s, const char* what, const Args&... args) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return hip_fail(e, what);
    hipLaunchKernelGGL(k, dim3(grid), dim3(RT), smem, s, args...);
    return launch_status(what);
}
// f(ic<O>, ic<A>, ic<K>) for the obs_dim <= 32 dims (check_ln has refused wider observations)
template <class F>
static int dispatch_dims_ln(const pgm_dims* d, const char* what, F&& f) {
    return dispatch_dims(d->O, d->A, d->K, what, [&](auto o, auto aa, auto k) -> int {
        if constexpr (decltype(o)::value > 32) {
            set_error("%s: LayerNorm towers need obs_dim <= 32", what);
            return PGM_E_UNSUPPORTED;
        } else {
            return f(o, aa, k);
        }
    });
}

template <class Kern, class Args>
static int launch_smem(Kern k, int grid, size_t smem, hipStream_t s, const Args& args, const char* what) {
    if (smem > 160 * 1024) {
        set_error("%s: LDS image %zu bytes exceeds 160 KiB", what, smem);
        return PGM_E_UNSUPPORTED;
    }
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return hip_fail(e, what);
    hipLaunchKernelGGL(k, dim3(grid), dim3(RT), smem, s, args);
    return launch_status(what);
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
