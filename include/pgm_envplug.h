/* Device env plug-ins: the contract of a user env header and the C interface of the library built from it.
 *
 * A plug-in is one header that states an environment as three inline functions of one struct, pgm_user_env.
 * pgmorl_amd.build.build_env(header) compiles pgmorl_amd/csrc/pgm_envplug.hip with that header force-included into a
 * library of its own, libpgm_env.so: a fused rollout kernel and a fused evaluation kernel for gfx950 around the env's
 * functions, and the same functions for the host.  libpgm.so is not touched, and the plug-in library links nothing
 * from it.
 *
 * ---- the env header
 *
 * It must compile as plain C++ (any host compiler, no HIP header) and as HIP device code.  Mark every function
 * PGM_ENV_HD (below).  The rules of pgmorl_amd/csrc/pgm_dummy.hpp apply:
 *   - the state is fp64 (and int32) words;
 *   - write `#pragma clang fp contract(off)` at the top of every function body that does arithmetic (a GCC build
 *     passes -ffp-contract=off), so that no a*b + c becomes an fma on one side only;
 *   - use only correctly rounded operations (+ - * / sqrt) if the host and the device are to agree bit for bit.  A
 *     transcendental (exp, sin, tanh, pow, ...) is allowed, but the device's and the host's libm differ in the last
 *     bits: a header that uses one forfeits that equality, and with it the bitwise host-stepped reference
 *     (hostenv.PluginHostVecEnv) of the fused path.
 *
 *   struct pgm_user_env {
 *       static constexpr int O, A, K;        obs dims, action dims (DISCRETE: number of actions), objectives
 *                                            1 <= O <= 32, 1 <= A <= 8 (DISCRETE: 2 <= A <= 8), 1 <= K <= 3
 *       static constexpr bool DISCRETE;      Categorical head: step receives the action index as an int
 *       static constexpr int SD, SI;         fp64 and int32 state words per env, 0 <= SD <= 16, 0 <= SI <= 4
 *       static constexpr int RW;             fp64 uniforms per reset-table entry, 0 <= RW <= 8
 *       static constexpr int MAX_STEPS;      an episode never lasts longer (positive)
 *
 *       PGM_ENV_HD static void reset(double* sd, int32_t* si, const double* u);
 *           a start state from the RW uniforms u in [0, 1).  sd / si arrive zeroed.
 *       PGM_ENV_HD static void observe(const double* sd, const int32_t* si, double* obs);
 *           the O fp64 values of the raw observation.
 *       PGM_ENV_HD static void step(double* sd, int32_t* si, const float* action, double* obj, double* reward,
 *                                   int32_t* done, int32_t* bad);            (DISCRETE: int action)
 *           one transition.  action: the RAW policy sample (A floats; the env clips it) or the action index in
 *           [0, A).  obj: K fp64 objectives.  reward: the scalar env reward (VecNormalize's ret input).  done: the
 *           episode ended.  bad: it ended at a time limit and not in a true terminal state (TimeLimitMask's
 *           bad_transition).  done and bad arrive as 0.
 *   };
 *
 * The dim ranges are those of the runtime-dim kernel family.  The state words live in the registers of the thread that
 * owns the env: index them with constants (unrolled loops), or they fall into scratch memory.  No loop of a header may
 * be unbounded.
 *
 * Auto-reset is the caller's job, not the env's: on done the caller increments the env's episode counter e, zeroes the
 * state and calls reset with entry (row, e mod R) of the reset table ([rows][R][RW] fp64 uniforms,
 * envspec.plugin_reset_table).  Training env n of every task uses row n; evaluation episode e starts at entry (e, 0)
 * of the eval_num-row table.
 *
 * The forced limit: the caller counts the steps of the running episode (`elapsed`).  On the step that brings the count
 * to MAX_STEPS it sets done = 1 and bad = 1, whatever step reported.  That bound makes every loop of the kernels and
 * of the host functions finite; it is not optional.
 *
 * ---- contract 2: runtime parameters and per-step uniforms (optional)
 *
 * A header that declares `static constexpr int CONTRACT = 2;` asks for two more inputs.  Absent, or 1, is the contract
 * above and nothing below applies.  With CONTRACT == 2 the header also declares
 *       static constexpr int NP;             fp64 runtime parameters of the env, 0 <= NP <= 16
 *       static constexpr int NW;             fp64 uniforms in [0, 1) handed to every step, 0 <= NW <= 4
 *   and, with NP > 0,
 *       static constexpr double PAR_DEFAULT[NP];      the value of a parameter the user does not set
 *       static constexpr const char* PAR_NAMES;       NP comma-separated identifiers, e.g. "slip,wind"
 * and its three functions take one trailing argument, `const pgm_env_ctx& c`:
 *       reset(sd, si, u, c)   observe(sd, si, obs, c)   step(sd, si, action, obj, reward, done, bad, c)
 * c.par points at the NP parameters in all three.  c.w points at the step's NW uniforms in step and is NULL in reset
 * and observe.  The parameters are the run's (TaskBatch(env_params={name: value}), --env-param NAME=VALUE): one set for
 * every task and env, uploaded per launch, so a changed value needs no new library.  They live in registers like the
 * state words: index c.par and c.w with constants.
 *
 * The uniforms are integer hashes, so the host and the device agree bit for bit:
 *       u53(seed, i) = (double)(splitmix64(key(seed) ^ i) >> 11) * 2^-53
 * with key the stream key of the action noise (pgm_normal_noise / pgm_uniform_noise).  They never depend on the task:
 *   training     word j of (step t, env n) of a rollout is element (t N + n) NW + j of the stream of env_seed;
 *   evaluation   word j of (episode e, step it) is element (e MAX_STEPS + it) NW + j of the stream of env_seed: every
 *                policy is evaluated under common random numbers.
 * pgm_envplug_uniforms is that stream on the host.
 */
#ifndef PGM_ENVPLUG_H
#define PGM_ENVPLUG_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PGM_ENV_HD __host__ __device__
#else
#define PGM_ENV_HD
#endif

#define PGM_ENVPLUG_ABI 1
#define PGM_ENVPLUG_MAX_OBS 32
#define PGM_ENVPLUG_MAX_ACT 8
#define PGM_ENVPLUG_MAX_OBJ 3
#define PGM_ENVPLUG_MAX_SD 16
#define PGM_ENVPLUG_MAX_SI 4
#define PGM_ENVPLUG_MAX_RW 8
#define PGM_ENVPLUG_MAX_NP 16
#define PGM_ENVPLUG_MAX_NW 4

/* contract 2: what reset, observe and step receive beside their own arguments */
typedef struct pgm_env_ctx {
    const double* par; /* NP runtime parameters */
    const double* w;   /* step: NW uniforms in [0, 1); reset, observe: NULL */
} pgm_env_ctx;

#endif /* PGM_ENVPLUG_H */

/* ---- the library (declared only where include/pgm_abi.h is wanted too, after #define PGM_ENVPLUG_DECLARE_API: an env
 * header needs none of it) */
#if defined(PGM_ENVPLUG_DECLARE_API) && !defined(PGM_ENVPLUG_API_DECLARED)
#define PGM_ENVPLUG_API_DECLARED
#include "pgm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

int pgm_envplug_abi(void);                /* PGM_ENVPLUG_ABI */
const char* pgm_envplug_last_error(void); /* the calling thread's last refusal */
/* out[8] = O, A, K, DISCRETE, SD, SI, RW, MAX_STEPS */
int pgm_envplug_info(int32_t* out);

/* The fused rollout: T steps of Policy.act, the env's step, VecNormalize and the storage insert, then the bootstrap
 * value, one launch.  sd [P][N][SD], si [P][N][SI], episode [P][N] (resets since pgm_envplug_reset) and st->elapsed
 * [P][N] (steps of the running episode) are the env state, read and written; of st only elapsed, obj_acc,
 * obj_acc_valid and ret are touched.  table [reset_count][R][RW], reset_count >= N.
 * stream_in, Gaussian head: standard normals [T][N][A], or NULL for counter_normal(seed, (t N + n) A + a);
 * Categorical head: uniforms [T][N], or NULL for counter_uniform(seed, t N + n) (pgm_normal_noise / pgm_uniform_noise).
 * Validated before any device work, in this order: NULL pointers; pgm_dims (positive, H, N <= 8); d->O/A/K against the
 * compiled header; d->LN == 0; T >= 1; R >= 1 and reset_count >= N. */
int pgm_envplug_rollout(const pgm_dims* d, const float* params, double* sd, int32_t* si, int32_t* episode,
                        const double* table, int32_t R, int32_t reset_count, const pgm_env_state* st,
                        const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* stream_in, uint64_t seed,
                        int32_t carry, pgm_stream_t stream);

/* The deterministic evaluation (semantics of pgm_eval_dummy): eval_num episodes per task (1..8) are the rows of one
 * forward; episode e starts at entry (e, 0) of table; the action is the mean / the lowest-index argmax; an ended
 * episode stands still; at most MAX_STEPS steps.  objs_out [P][K] fp64: the mean over the episodes of the (raw: not)
 * discounted objective sums.  Validation order as above, with 1 <= eval_num <= 8 and reset_count >= eval_num. */
int pgm_envplug_eval(const pgm_dims* d, const float* params, const double* table, int32_t R, int32_t reset_count,
                     const double* ob_mean, const double* ob_var, int32_t eval_num, int32_t use_ob_rms, int32_t raw,
                     double gamma, double* objs_out, pgm_stream_t stream);

/* Host only (no device needed): the header's functions on n items, with the forced limit and the auto-reset.  Item i
 * is an env at reset-table row row[i] with state sd [n][SD], si [n][SI], elapsed [n], episode [n]; action is float
 * [n][A] or (DISCRETE) int32 [n].  Outputs: the next state (already the next episode's first on done), its
 * observation [n][O], and the step's obj [n][K], reward, done, bad [n]. */
int pgm_envplug_transition(int32_t n, const double* sd, const int32_t* si, const int32_t* elapsed,
                           const int32_t* episode, const int32_t* row, const void* action, const double* table,
                           int32_t R, int32_t reset_count, double* sd_out, int32_t* si_out, int32_t* elapsed_out,
                           int32_t* episode_out, double* obs_out, double* obj_out, double* reward_out,
                           int32_t* done_out, int32_t* bad_out);
/* Host only: item i = the start state of entry (row[i], episode[i] mod R) and its observation */
int pgm_envplug_reset(int32_t n, const int32_t* row, const int32_t* episode, const double* table, int32_t R,
                      int32_t reset_count, double* sd_out, int32_t* si_out, double* obs_out);

/* ---- contract 2.  A library built from a CONTRACT = 2 header refuses the four calls above with PGM_E_UNSUPPORTED and
 * a message naming the _ex call.  A contract-1 library accepts the _ex calls with env_par = NULL, env_rnd = NULL (w =
 * NULL) and any seed: they are then the calls above. */
int pgm_envplug_contract(void); /* 1 or 2 */
/* out[11] = pgm_envplug_info's 8, then CONTRACT, NP, NW */
int pgm_envplug_info_ex(int32_t* out);
/* names: PAR_NAMES ("" with NP = 0) copied into cap bytes, NUL included; defaults: NP values.  Either may be NULL. */
int pgm_envplug_params(char* names, int32_t cap, double* defaults);
/* Host only: out[k] = u53(seed, start + k), k < n: the env-noise stream */
int pgm_envplug_uniforms(uint64_t seed, uint64_t start, int64_t n, double* out);

/* pgm_envplug_rollout with env_par [NP] (device) and the step uniforms env_rnd [T][N][NW] (device), or NULL for
 * u53(env_seed, (t N + n) NW + j).  Validation: pgm_envplug_rollout's, in its order; then env_par NULL with NP > 0 is
 * PGM_E_INVALID_ARG.  All of it before any device work. */
int pgm_envplug_rollout_ex(const pgm_dims* d, const float* params, double* sd, int32_t* si, int32_t* episode,
                           const double* table, int32_t R, int32_t reset_count, const pgm_env_state* st,
                           const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* stream_in, uint64_t seed,
                           int32_t carry, const double* env_par, const double* env_rnd, uint64_t env_seed,
                           pgm_stream_t stream);
/* pgm_envplug_eval with env_par [NP] (device); step `it` of episode e draws u53(env_seed, (e MAX_STEPS + it) NW + j) */
int pgm_envplug_eval_ex(const pgm_dims* d, const float* params, const double* table, int32_t R, int32_t reset_count,
                        const double* ob_mean, const double* ob_var, int32_t eval_num, int32_t use_ob_rms, int32_t raw,
                        double gamma, double* objs_out, const double* env_par, uint64_t env_seed, pgm_stream_t stream);
/* Host only: pgm_envplug_transition / pgm_envplug_reset with env_par [NP] and (transition) item i's uniforms w [n][NW];
 * after their own checks, env_par NULL with NP > 0 or w NULL with NW > 0 is PGM_E_INVALID_ARG */
int pgm_envplug_transition_ex(int32_t n, const double* sd, const int32_t* si, const int32_t* elapsed,
                              const int32_t* episode, const int32_t* row, const void* action, const double* table,
                              int32_t R, int32_t reset_count, const double* env_par, const double* w, double* sd_out,
                              int32_t* si_out, int32_t* elapsed_out, int32_t* episode_out, double* obs_out,
                              double* obj_out, double* reward_out, int32_t* done_out, int32_t* bad_out);
int pgm_envplug_reset_ex(int32_t n, const int32_t* row, const int32_t* episode, const double* table, int32_t R,
                         int32_t reset_count, const double* env_par, double* sd_out, int32_t* si_out, double* obs_out);

#ifdef __cplusplus
}
#endif
#endif /* PGM_ENVPLUG_DECLARE_API */
