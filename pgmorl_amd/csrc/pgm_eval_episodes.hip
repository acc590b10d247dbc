// Re-evaluation of a saved Pareto set (pgm_eval_episodes): E episodes of each of M policies from a table of start
// states, with the per-episode sums kept.  One workgroup (256 threads) per (policy, chunk of NMAX episodes): the
// episodes of a chunk are the rows of one policy_forward per step, so a policy's weights are loaded once per chunk and
// every step advances up to NMAX episodes.  The body is the block evaluation's (eval_kernel, pgm_policy_env.hip)
// row by row, from the same device functions of pgm_policy_dev.hpp; workgroups never talk to each other, so M may
// exceed the CU count many times over.
//
// Reference semantics: evaluation() morl/mopg.py:25-46 per (policy, start state); the stochastic arm draws
// torch.normal(mean, std) = z*std + mean (a2c_ppo_acktr/distributions.py:29-40) from a counter stream.
#include "pgm_policy_dev.hpp"

namespace pgm {

constexpr int EVAL_EPISODES_MAX = 65536;  // episodes per policy in one call (gridDim.y = ceil(E / NMAX) <= 65535)

struct EvalEpisodesArgs {
    int M, E;
    const float* params;  // [M][L]
    pgm_env_spec spec;
    const double *ob_mean, *ob_var;  // [M][O]; read with use_ob
    const double* starts;            // [E][O]
    int use_ob, raw, stochastic;
    double gamma;
    uint64_t noise_seed;
    double* episodes;  // [M][E][K]
};

template <class Tw, int O, int A, int K>
__global__ __launch_bounds__(RT) void eval_episodes_kernel(EvalEpisodesArgs a, typename Tw::Lay L) {
    static_assert(NMAX * A <= RT && NMAX * K <= RT, "one thread per (row, action dim) and per (row, objective)");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    auto& S = *reinterpret_cast<StepSmem<O, A, K>*>(smem_raw);
    auto& P = S.pol;
    auto& E = S.env;
    const int m = blockIdx.x, e0 = blockIdx.y * NMAX, t = threadIdx.x;
    const int rows = min(NMAX, a.E - e0);  // the last chunk is ragged: rows past E are neither computed nor stored
    const int max_steps = a.spec.max_episode_steps;
    const double* starts = a.starts + (size_t)e0 * O;
    const Spec<O, A, K> sp{E, a.spec, starts};
    const float* prm = a.params + (size_t)m * L.total;
    typename Tw::template Reg<O, A, K> R;
    load_policy<Tw, true>(P, R, prm, L);
    load_spec(E, a.spec, starts, rows);
    for (int o = t; o < O; o += RT) {
        E.ob_mean[o] = a.use_ob ? a.ob_mean[(size_t)m * O + o] : 0.0;
        E.ob_inv[o] = a.use_ob ? eval_ob_inv(a.ob_var[(size_t)m * O + o]) : 1.0;
    }
    for (int i = t; i < rows * O; i += RT) E.s[i / O][i % O] = starts[i];
    if (t < rows) E.elapsed[t] = 0;
    if (t < rows * K) E.obj_acc[t / K][t % K] = 0.0;  // the per-episode sums
    double g = 1.0;
    __syncthreads();
    for (int step = 0;; ++step) {
        for (int i = t; i < rows * O; i += RT) {
            const int o = i % O;
            P.x[i / O][o] = eval_normalise(E.s[i / O][o], a.use_ob, E.ob_mean[o], E.ob_inv[o]);
        }
        lds_sync();
        policy_forward<Tw>(P, R, rows, prm, L);
        if (t < rows * A) {
            const int n = t / A, j = t % A;
            float av = P.mu[n][j];
            if (a.stochastic) {  // the same z for every policy: element ((e, step), j) of the stream noise_seed
                const uint64_t idx = ((uint64_t)(e0 + n) * (uint64_t)max_steps + (uint64_t)step) * A + j;
                av = fmaf(counter_normal(a.noise_seed, idx), expf(P.logstd[j]), av);
            }
            E.ac[n][j] = clipd((double)av, sp.lo(j), sp.hi(j));
        }
        lds_sync();
        env_dynamics(E, sp, rows, max_steps);
        if (t < rows * K) E.obj_acc[t / K][t % K] += g * E.objraw[t / K][t % K];
        if (!a.raw) g *= a.gamma;
        const int done = E.done[0];  // SynthMO episodes end at the time limit: every row of the chunk with row 0
        for (int i = t; i < rows * O; i += RT) E.s[i / O][i % O] = E.snew[i / O][i % O];
        lds_sync();
        if (done) break;
    }
    if (t < rows * K) a.episodes[((size_t)m * a.E + e0) * K + t] = E.obj_acc[t / K][t % K];
}

// objs[m][k] = (episodes[m][0][k] + episodes[m][1][k] + ...) / E, summed in index order
__global__ __launch_bounds__(RT) void eval_episodes_mean_kernel(const double* __restrict__ episodes,
                                                                double* __restrict__ objs, int M, int E, int K) {
    const size_t i = (size_t)blockIdx.x * RT + threadIdx.x;
    if (i >= (size_t)M * K) return;
    const double* ep = episodes + (i / K) * (size_t)E * K + (i % K);
    double s = 0.0;
    for (int e = 0; e < E; ++e) s += ep[(size_t)e * K];
    objs[i] = s / (double)E;
}

}  // namespace pgm

using namespace pgm;

extern "C" {

// Validation order (include/pgm_abi.h): NULL pointers, check_dims (N = 1, T = 0), check_ln, spec_ok, E; then the
// dispatch refuses dims no kernel is compiled for.
int pgm_eval_episodes(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const double* ob_mean,
                      const double* ob_var, const double* starts, int32_t E, int32_t use_ob_rms, int32_t raw,
                      double gamma, int32_t stochastic, uint64_t noise_seed, double* episodes_out, double* objs_out,
                      pgm_stream_t stream) {
    const char* what = "pgm_eval_episodes";
    if (!d || !params || !spec || !starts || !episodes_out || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("%s: null pointer (ob_mean / ob_var are required with use_ob_rms; objs_out may be NULL)", what);
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: the rows of a workgroup are episodes
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, what)) return rc;
    if (int rc = check_ln(&dd, what)) return rc;
    if (!spec_ok(spec)) {
        set_error("%s: null pointer in the env spec, or max_episode_steps <= 0", what);
        return PGM_E_INVALID_ARG;
    }
    if (E < 1 || E > EVAL_EPISODES_MAX) {
        set_error("%s: E=%d episodes per policy outside [1, %d]", what, E, EVAL_EPISODES_MAX);
        return PGM_E_SHAPE;
    }
    const EvalEpisodesArgs a{d->P, E, params, *spec, ob_mean, ob_var, starts, use_ob_rms != 0, raw != 0,
                             stochastic != 0, gamma, noise_seed, episodes_out};
    const hipStream_t s = (hipStream_t)stream;
    const int rc = dispatch_towers(&dd, what, [&](auto tw, const auto& L, auto o, auto aa, auto k) -> int {
        constexpr int O = decltype(o)::value, A = decltype(aa)::value, K = decltype(k)::value;
        auto kern = eval_episodes_kernel<decltype(tw), O, A, K>;
        constexpr size_t smem = sizeof(StepSmem<O, A, K>);
        static_assert(smem <= 160 * 1024, "LDS image exceeds 160 KiB");
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return hip_fail(e, what);
        hipLaunchKernelGGL(kern, dim3(d->P, (E + NMAX - 1) / NMAX), dim3(RT), smem, s, a, L);
        return launch_status(what);
    });
    if (rc != PGM_OK || !objs_out) return rc;
    const size_t n = (size_t)d->P * d->K;
    hipLaunchKernelGGL(eval_episodes_mean_kernel, dim3((unsigned)((n + RT - 1) / RT)), dim3(RT), 0, s, episodes_out,
                       objs_out, d->P, E, d->K);
    return launch_status(what);
}

// Validation order (include/pgm_abi.h): NULL pointers, check_dims (N = 1, T = 0), check_ln and the LN = 1 refusal,
// spec_ok, M, E and Q * E; then the dispatch refuses dims outside the wave-per-episode kernel
// (eval_blend_kernel, pgm_rollout_lanes.hip).
int pgm_eval_blend(const pgm_dims* d, const float* params, int32_t M, const double* ob_mean, const double* ob_var,
                   const int32_t* src, const double* alpha, const pgm_env_spec* spec, const double* starts, int32_t E,
                   int32_t use_ob_rms, int32_t raw, double gamma, double* episodes_out, double* objs_out,
                   pgm_stream_t stream) {
    const char* what = "pgm_eval_blend";
    if (!d || !params || !src || !alpha || !spec || !starts || !episodes_out ||
        (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("%s: null pointer (ob_mean / ob_var are required with use_ob_rms; objs_out may be NULL)", what);
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: P = Q candidates, a wave per (candidate, episode)
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, what)) return rc;
    if (int rc = check_ln(&dd, what)) return rc;
    if (dd.LN == 1) {
        set_error("%s: LayerNorm towers (pgm_dims.LN = 1) have no wave-per-episode kernel; materialise the candidates "
                  "and use pgm_eval_episodes", what);
        return PGM_E_UNSUPPORTED;
    }
    if (!spec_ok(spec)) {
        set_error("%s: null pointer in the env spec, or max_episode_steps <= 0", what);
        return PGM_E_INVALID_ARG;
    }
    if (M < 1) {
        set_error("%s: M=%d members outside [1, 2^31)", what, M);
        return PGM_E_SHAPE;
    }
    if (E < 1 || E > EVAL_EPISODES_MAX) {
        set_error("%s: E=%d episodes per candidate outside [1, %d]", what, E, EVAL_EPISODES_MAX);
        return PGM_E_SHAPE;
    }
    if ((int64_t)d->P * E > EVAL_BLEND_WORK_MAX) {
        set_error("%s: Q * E = %d * %d exceeds the %d (candidate, episode) waves of one call; send the table in slices",
                  what, d->P, E, EVAL_BLEND_WORK_MAX);
        return PGM_E_SHAPE;
    }
    const EvalBlendArgs a{d->P, E, M, make_layout(d->O, d->A, d->K, d->H), params, *spec, ob_mean, ob_var, starts, src,
                          alpha, use_ob_rms != 0, raw != 0, gamma, episodes_out};
    const hipStream_t s = (hipStream_t)stream;
    const int rc = launch_eval_blend(&dd, a, s);
    if (rc != PGM_OK || !objs_out) return rc;
    const size_t n = (size_t)d->P * d->K;
    hipLaunchKernelGGL(eval_episodes_mean_kernel, dim3((unsigned)((n + RT - 1) / RT)), dim3(RT), 0, s, episodes_out,
                       objs_out, d->P, E, d->K);
    return launch_status(what);
}

// Validation order (include/pgm_abi.h): pgm_eval_blend's, item by item; then the dispatch refuses dims outside the
// wave-per-episode kernel (eval_blend3_kernel, pgm_rollout_lanes.hip).
int pgm_eval_blend3(const pgm_dims* d, const float* params, int32_t M, const double* ob_mean, const double* ob_var,
                    const int32_t* src, const double* w, const pgm_env_spec* spec, const double* starts, int32_t E,
                    int32_t use_ob_rms, int32_t raw, double gamma, double* episodes_out, double* objs_out,
                    pgm_stream_t stream) {
    const char* what = "pgm_eval_blend3";
    if (!d || !params || !src || !w || !spec || !starts || !episodes_out || (use_ob_rms && (!ob_mean || !ob_var))) {
        set_error("%s: null pointer (ob_mean / ob_var are required with use_ob_rms; objs_out may be NULL)", what);
        return PGM_E_INVALID_ARG;
    }
    pgm_dims dd = *d;  // N and T are not this call's: P = Q candidates, a wave per (candidate, episode)
    dd.N = 1;
    dd.T = 0;
    if (int rc = check_dims(&dd, what)) return rc;
    if (int rc = check_ln(&dd, what)) return rc;
    if (dd.LN == 1) {
        set_error("%s: LayerNorm towers (pgm_dims.LN = 1) have no wave-per-episode kernel; materialise the candidates "
                  "and use pgm_eval_episodes", what);
        return PGM_E_UNSUPPORTED;
    }
    if (!spec_ok(spec)) {
        set_error("%s: null pointer in the env spec, or max_episode_steps <= 0", what);
        return PGM_E_INVALID_ARG;
    }
    if (M < 1) {
        set_error("%s: M=%d members outside [1, 2^31)", what, M);
        return PGM_E_SHAPE;
    }
    if (E < 1 || E > EVAL_EPISODES_MAX) {
        set_error("%s: E=%d episodes per candidate outside [1, %d]", what, E, EVAL_EPISODES_MAX);
        return PGM_E_SHAPE;
    }
    if ((int64_t)d->P * E > EVAL_BLEND_WORK_MAX) {
        set_error("%s: Q * E = %d * %d exceeds the %d (candidate, episode) waves of one call; send the table in slices",
                  what, d->P, E, EVAL_BLEND_WORK_MAX);
        return PGM_E_SHAPE;
    }
    const EvalBlend3Args a{d->P, E, M, make_layout(d->O, d->A, d->K, d->H), params, *spec, ob_mean, ob_var, starts, src,
                           w, use_ob_rms != 0, raw != 0, gamma, episodes_out};
    const hipStream_t s = (hipStream_t)stream;
    const int rc = launch_eval_blend3(&dd, a, s);
    if (rc != PGM_OK || !objs_out) return rc;
    const size_t n = (size_t)d->P * d->K;
    hipLaunchKernelGGL(eval_episodes_mean_kernel, dim3((unsigned)((n + RT - 1) / RT)), dim3(RT), 0, s, episodes_out,
                       objs_out, d->P, E, d->K);
    return launch_status(what);
}
}  // extern "C"
