/*
 * pgm_abi.h -- C ABI of libpgm.so, the MI355X (gfx950) kernels of the PG-MORL MOPG hot path.
 *
 * Every entry point is batched over P tasks (policies), takes CALLER-OWNED device buffers
 * (plain pointers; no allocation inside), is ordered on the passed hipStream_t and returns
 * an int status (PGM_OK or a negative PGM_E_*).  pgm_last_error() returns a thread-local
 * message for the last failure.  No global mutable state besides that string, the pre-zeroed-workspace
 * marks of pgm_ppo_update_reset (mutex-guarded) and a per-device CU count (an immutable device property):
 * no cached launch decisions, no allocation inside the library, and no environment variables read: every
 * launch choice is an argument (pgm_launch_opts).  Calls on distinct streams are independent.  One host
 * thread per device.
 *
 * Reference seams replaced (albo437/PGMORL; paths relative to the reference tree):
 *   pgm_act_forward       Policy.act / get_value            a2c_ppo_acktr/model.py:57-73
 *                          (+ DiagGaussian sample/log_prob   a2c_ppo_acktr/distributions.py:29-40,71-90)
 *   pgm_env_reset         envs.reset() through VecNormalize  baselines/.../vec_env/vec_normalize.py:63-66
 *   pgm_env_step          envs.step(): DummyVecEnv auto-reset + TimeLimitMask + VecNormalize
 *                          + VecPyTorch fp32 cast + mask/bad_mask bookkeeping
 *                                                           dummy_vec_env.py:45-56, a2c_ppo_acktr/envs.py:122-131,
 *                                                           171-217, vec_normalize.py:29-61, morl/mopg.py:110-130
 *   pgm_rollout           the T-step rollout loop + bootstrap value (morl/mopg.py:103-135 with
 *                          RolloutStorage.insert a2c_ppo_acktr/storage.py:50-62)
 *   pgm_gae               RolloutStorage.compute_returns    a2c_ppo_acktr/storage.py:77-116
 *   pgm_adv_normalize     PPO.update advantage prologue     a2c_ppo_acktr/algo/ppo.py:41-56
 *                          + WeightedSumScalarization        morl/scalarization_methods.py:28-29
 *   pgm_ppo_update        PPO.update epochs x minibatches   a2c_ppo_acktr/algo/ppo.py:58-115
 *                          (+ feed_forward_generator storage.py:118-154, clip_grad_norm_, Adam)
 *                          (pgm_ppo_update_reset: its workspace reset, issued ahead on another stream)
 *   pgm_eval              evaluation()                       morl/mopg.py:25-46
 *   pgm_rollout_act       Policy.act / get_value of one rollout step, into the strided storage slots
 *                                                           morl/mopg.py:105-108, 132-135
 *   pgm_env_ingest        VecNormalize.step_wait / reset + RolloutStorage.insert on a HOST env's transition
 *                                                           vec_normalize.py:29-66, morl/mopg.py:110-130,
 *                                                           storage.py:50-62
 *   pgm_eval_act          evaluation()'s normalise + deterministic act for a HOST env   morl/mopg.py:36-39
 *   pgm_act_forward_cat   Policy.act / get_value with a Categorical head   a2c_ppo_acktr/model.py:33-35,57-73
 *                          (+ Categorical / FixedCategorical sample, log_probs, mode
 *                                                           a2c_ppo_acktr/distributions.py:17-27,54-68)
 *   pgm_rollout_act_cat   the same for one rollout step, into the strided storage slots (one width-1 action per step,
 *                          a2c_ppo_acktr/storage.py:19-25)   morl/mopg.py:105-108, 132-135
 *   pgm_eval_act_cat      evaluation()'s normalise + dist.mode() for a HOST env   morl/mopg.py:36-39
 *   pgm_ppo_update_cat    PPO.update epochs x minibatches with FixedCategorical log_probs / entropy
 *                                                           a2c_ppo_acktr/algo/ppo.py:58-115, model.py:75-82
 *   pgm_uniform_noise     Categorical.sample's multinomial draw  (perf-mode RNG replacement)
 *   pgm_rollout_dst       the rollout loop on the device Deep Sea Treasure   morl/mopg.py:103-135,
 *                                                           environments/deep_sea_treasure.py:111-183
 *   pgm_eval_dst          evaluation() on the device Deep Sea Treasure       morl/mopg.py:25-46
 *   pgm_dst_transition    the Deep Sea Treasure step on the host   environments/deep_sea_treasure.py:111-183
 *   pgm_randperm         SubsetRandomSampler's randperm     (perf-mode RNG replacement)
 *   pgm_normal_noise      Normal.sample's torch.normal draw  (perf-mode RNG replacement)
 *
 * Layouts (row-major, fp32 unless noted; P = tasks, N = envs per task, T = rollout steps,
 * O/A/K = obs/action/objective dims, H = hidden width, fixed 64 in this build):
 *   params/adam_m/adam_v  [P][L]  L and tensor offsets from pgm_param_layout (weights stored
 *                                 TRANSPOSED, [in][out]; see DESIGN.md "Data layout in HBM")
 *   rollout buffers       obs [P][T+1][N][O], actions [P][T][N][A], logp [P][T][N],
 *                         values/returns [P][T+1][N][K], rewards [P][T][N][K],
 *                         masks/bad_masks [P][T+1][N], adv [P][T][N]
 *   env state (fp64)      s [P][N][O], elapsed int32 [P][N], obj_acc [P][N][K], obj_acc_valid int32 [P],
 *                         ret [P][N]
 *   running stats (fp64)  ob_mean/var [P][O], ob_count [P], ret_* [P], obj_mean/var [P][K], obj_count [P]
 *   shared RNG inputs     noise [T][N][A] fp32 and perms [E][T*N] int32 are shared by all tasks, as in the
 *                         reference where every task process reseeds torch with the iteration index
 *                         (morl/mopg.py:96).
 */
#ifndef PGM_ABI_H
#define PGM_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGM_ABI_VERSION 5
/* Additions that change no existing struct or entry point raise the minor only.
 * Minor 1: pgm_abi_minor, pgm_rollout_act, pgm_env_ingest, pgm_eval_act (host-stepped environments). */
#define PGM_ABI_MINOR 1

#define PGM_OK 0
#define PGM_E_INVALID_ARG (-1)
#define PGM_E_SHAPE (-2)
#define PGM_E_HIP (-3)
#define PGM_E_UNSUPPORTED (-4)

/* Parameter tensors in reference named_parameters() order (model.py:201-256, distributions.py:71-79). */
#define PGM_P_ACTOR_W1 0   /* base.actor.0.weight^T   [O][H] */
#define PGM_P_ACTOR_B1 1   /* base.actor.0.bias       [H]    */
#define PGM_P_ACTOR_W2 2   /* base.actor.2.weight^T   [H][H] */
#define PGM_P_ACTOR_B2 3   /* base.actor.2.bias       [H]    */
#define PGM_P_CRITIC_W1 4  /* base.critic.0.weight^T  [O][H] */
#define PGM_P_CRITIC_B1 5
#define PGM_P_CRITIC_W2 6  /* base.critic.2.weight^T  [H][H] */
#define PGM_P_CRITIC_B2 7
#define PGM_P_VALUE_W 8    /* base.critic_linear.weight^T [H][K] */
#define PGM_P_VALUE_B 9    /* base.critic_linear.bias [K] */
#define PGM_P_MEAN_W 10    /* dist.fc_mean.weight^T   [H][A] */
#define PGM_P_MEAN_B 11    /* dist.fc_mean.bias       [A] */
#define PGM_P_LOGSTD 12    /* dist.logstd._bias       [A] (reference shape [A][1]) */
#define PGM_NUM_PARAM_TENSORS 13

/* LayerNorm towers (pgm_dims.LN = 1; model.py:201-256 with layernorm=True): every tower layer is
 * Linear(bias=False) -> LayerNorm(H, elementwise_affine) -> tanh, so each layer carries a weight, the LayerNorm
 * scale (gamma) and the LayerNorm shift (beta).  named_parameters() order; offsets from pgm_param_layout_ln. */
#define PGM_PL_ACTOR_W1 0    /* base.actor.0.weight^T   [O][H] */
#define PGM_PL_ACTOR_G1 1    /* base.actor.1.weight     [H]    */
#define PGM_PL_ACTOR_BE1 2   /* base.actor.1.bias       [H]    */
#define PGM_PL_ACTOR_W2 3    /* base.actor.3.weight^T   [H][H] */
#define PGM_PL_ACTOR_G2 4    /* base.actor.4.weight     [H]    */
#define PGM_PL_ACTOR_BE2 5   /* base.actor.4.bias       [H]    */
#define PGM_PL_CRITIC_W1 6   /* base.critic.0.weight^T  [O][H] */
#define PGM_PL_CRITIC_G1 7
#define PGM_PL_CRITIC_BE1 8
#define PGM_PL_CRITIC_W2 9   /* base.critic.3.weight^T  [H][H] */
#define PGM_PL_CRITIC_G2 10
#define PGM_PL_CRITIC_BE2 11
#define PGM_PL_VALUE_W 12    /* base.critic_linear.weight^T [H][K] */
#define PGM_PL_VALUE_B 13
#define PGM_PL_MEAN_W 14     /* dist.fc_mean.weight^T   [H][A] */
#define PGM_PL_MEAN_B 15
#define PGM_PL_LOGSTD 16     /* dist.logstd._bias       [A] */
#define PGM_NUM_PARAM_TENSORS_LN 17

/* Discrete action spaces (Categorical head, distributions.py:54-68): the ten tower / value tensors in PGM_P_* order
 * (indices 0..9), then the head's Linear.  No logstd.  Offsets from pgm_param_layout_cat. */
#define PGM_PC_LINEAR_W 10   /* dist.linear.weight^T    [H][A]  (A = number of actions) */
#define PGM_PC_LINEAR_B 11   /* dist.linear.bias        [A] */
#define PGM_NUM_PARAM_TENSORS_CAT 12

/* Feature bits: additions that leave PGM_ABI_VERSION / PGM_ABI_MINOR alone are discovered here.  pgm_abi_features()
 * reports bits 1, 2 and 4 and its value (7) is frozen, since callers compare it for equality; pgm_abi_feature_mask()
 * reports every bit, PGM_FEATURE_ANY_DIMS and any later one included.  New callers read pgm_abi_feature_mask() and
 * fall back to pgm_abi_features() where a library lacks the symbol. */
#define PGM_FEATURE_CATEGORICAL 1 /* the *_cat entry points, pgm_param_layout_cat, pgm_uniform_noise */
#define PGM_FEATURE_DST_DEVICE 2  /* pgm_rollout_dst, pgm_eval_dst, pgm_dst_transition: Deep Sea Treasure on the device */
#define PGM_FEATURE_DUMMY_DEVICE 4 /* pgm_rollout_dummy, pgm_eval_dummy, pgm_dummy_transition; the dim sets 6/2/2, 6/2/3 */
#define PGM_FEATURE_ANY_DIMS 8    /* the *_any entry points (host envs of any dims); in pgm_abi_feature_mask() only */

typedef void* pgm_stream_t; /* a hipStream_t (0 = the null stream) */

/* LN (ABI 5): 0 = plain tanh towers, 1 = LayerNorm towers (params / Adam vectors in the pgm_param_layout_ln layout).
 * LN = 1 is built for obs_dim <= 32 (17/6/2, 11/3/2, 11/3/3, 27/8/2, 8/2/2, 6/2/2, 6/2/3); with 376/17/2 every entry
 * point that touches the policy returns PGM_E_UNSUPPORTED.  pgm_launch_opts is ignored for LN = 1 (one kernel family). */
typedef struct pgm_dims {
    int32_t P, N, T, O, A, K, H;
    int32_t LN;
} pgm_dims;

typedef struct pgm_env_spec { /* device pointers, fp64 */
    const double* d;      /* [O]    */
    const double* U;      /* [O][A] */
    const double* c;      /* [O]    */
    const double* V;      /* [K][O] */
    const double* ebase;  /* [K]    */
    const double* ecoef;  /* [K]    */
    const double* act_lo; /* [A]    */
    const double* act_hi; /* [A]    */
    int32_t max_episode_steps;
    int32_t _pad;
} pgm_env_spec;

typedef struct pgm_env_state { /* device pointers */
    double* s;              /* [P][N][O] */
    int32_t* elapsed;       /* [P][N]    */
    double* obj_acc;        /* [P][N][K] */
    int32_t* obj_acc_valid; /* [P]       */
    double* ret;            /* [P][N]    */
    const double* s0;       /* [N][O] reset state of env rank n (seed + n) */
} pgm_env_state;

typedef struct pgm_norm_state { /* device pointers (fp64) + flags */
    double *ob_mean, *ob_var, *ob_count;
    double *ret_mean, *ret_var, *ret_count;
    double *obj_mean, *obj_var, *obj_count;
    double gamma, clipob, cliprew, epsilon;
    int32_t use_ob_rms, use_obj_rms;
} pgm_norm_state;

typedef struct pgm_rollout_buf { /* device pointers */
    float* obs;
    float* actions;
    float* logp;
    float* values;
    float* rewards;
    float* masks;
    float* bad_masks;
    float* returns;
    float* adv;
} pgm_rollout_buf;

/* Launch options (ABI 4; no reference counterpart): which kernel family pgm_rollout / pgm_eval / pgm_ppo_update may
 * launch.  All zero, or a NULL pointer, = the automatic rule documented at each entry point.  The library reads no
 * environment variables; pgmorl_amd/_lib.py maps PGM_UPDATE_KERNEL / PGM_UPDATE_SPLIT / PGM_FS_DUAL /
 * PGM_ROLLOUT_KERNEL / PGM_EVAL_KERNEL onto this struct (A/B runs and tests). */
#define PGM_UPDATE_AUTO 0     /* feature-split while it gets >= 4 parts per tower, else the row split */
#define PGM_UPDATE_FS 1       /* the feature-split update wherever it fits */
#define PGM_UPDATE_ROWSPLIT 2 /* the row-split MFMA kernels (t16, MODE 2 / 1 / 0) */
#define PGM_UPDATE_VALU 3     /* the VALU reference update (obs_dim <= 64; A/B only) */
#define PGM_SPLIT_AUTO 0      /* row split: as many workgroups per tower as fit the device */
#define PGM_SPLIT_TASK 1      /* at most one workgroup per task (MODE 0; wide: one per tower) */
#define PGM_SPLIT_TOWER 2     /* at most one workgroup per tower (MODE 1; wide NS 1) */
#define PGM_SPLIT_HALVES 3    /* at most two per tower (MODE 2; wide NS 2) */
#define PGM_SPLIT_QUARTERS 4  /* at most four per tower (t16; wide NS 4) */
typedef struct pgm_launch_opts {
    int32_t update_kernel;   /* PGM_UPDATE_*; obs_dim <= 32 with update_split != AUTO means ROWSPLIT */
    int32_t update_split;    /* PGM_SPLIT_* (row-split and wide updates) */
    int32_t fs_one_per_cu;   /* 1: the feature-split update never places two workgroups on one CU */
    int32_t rollout_kernel;  /* 0 automatic (lane / wide kernels), 1 the workgroup-per-step kernel (A/B, tests) */
    int32_t eval_kernel;     /* 0 automatic (wave / wide kernels), 1 the workgroup-per-step kernel (A/B, tests) */
    int32_t _pad;
} pgm_launch_opts;

typedef struct pgm_ppo_hparams {
    float clip_param, value_loss_coef, entropy_coef, max_grad_norm;
    float adam_eps, beta1, beta2, _pad;
    int32_t ppo_epoch, num_mini_batch, use_clipped_value_loss, _pad2;
} pgm_ppo_hparams;

int pgm_abi_version(void);
int pgm_abi_minor(void); /* PGM_ABI_MINOR; a library without this symbol is minor 0 */
const char* pgm_last_error(void);

/* Flat per-task parameter layout: offsets[PGM_NUM_PARAM_TENSORS] (floats) and the padded
 * per-task length *total (a multiple of 64 floats). */
int pgm_param_layout(int32_t O, int32_t A, int32_t K, int32_t H, int32_t* offsets, int32_t* total);
/* The same for LayerNorm towers: offsets[PGM_NUM_PARAM_TENSORS_LN] in PGM_PL_* order, every tensor 16-byte aligned,
 * *total a multiple of 64 floats. */
int pgm_param_layout_ln(int32_t O, int32_t A, int32_t K, int32_t H, int32_t* offsets, int32_t* total);

/* Policy.act on obs [P][N][O] (model.py:57-69).  noise [N][A] (shared by tasks) gives
 * action = noise*exp(logstd) + mean; deterministic=1 gives action = mean (noise ignored).
 * Outputs value [P][N][K], action [P][N][A], logp [P][N]. */
int pgm_act_forward(const pgm_dims* d, const float* params, const float* obs, const float* noise,
                    int32_t deterministic, float* value, float* action, float* logp, pgm_stream_t stream);

/* envs.reset(): every env to its reset state, VecNormalize.ret = 0, ob_rms update + normalise.
 * Also clears elapsed and VecNormalize.obj (a fresh make_vec_envs, morl/mopg.py:67-81).
 * Writes obs_out [P][N][O]. */
int pgm_env_reset(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st,
                  const pgm_norm_state* ns, float* obs_out, pgm_stream_t stream);

/* One envs.step(action [P][N][A]) -> obs_out [P][N][O], reward_out [P][N][K] (info['obj'] after
 * obj_rms scaling), masks_out/bad_masks_out [P][N]. */
int pgm_env_step(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st,
                 const pgm_norm_state* ns, const float* action, float* obs_out, float* reward_out,
                 float* masks_out, float* bad_masks_out, pgm_stream_t stream);

/* The fused rollout: for t in [0,T): act on obs[t] -> env step -> insert (storage.py:50-62),
 * then values[T] = get_value(obs[T]).  carry=1 first applies after_update() (obs/masks/bad_masks
 * slot T -> 0, storage.py:71-75).  noise [T][N][A] or NULL: NULL draws the perf-mode counter RNG of
 * pgm_normal_noise keyed by seed (the iteration index). */
int pgm_rollout(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const pgm_env_state* st,
                const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* noise, uint64_t seed,
                int32_t carry, const pgm_launch_opts* opts, pgm_stream_t stream);

/* compute_returns(next_value already in values[T], use_gae, gamma, lam, use_proper_time_limits). */
int pgm_gae(const pgm_dims* d, const pgm_rollout_buf* rb, float gamma, float lam, int32_t use_gae,
            int32_t use_proper_time_limits, pgm_stream_t stream);

/* adv [P][T][N] = normalise(w . (R * s) - w . (V * s)), s = sqrt(obj_var + 1e-8) (or 1 if obj_var
 * is NULL); mean and UNBIASED std over T*N, (x - mean) / (std + 1e-5).  weights/obj_var [P][K] fp64. */
int pgm_adv_normalize(const pgm_dims* d, const pgm_rollout_buf* rb, const double* weights,
                      const double* obj_var, pgm_stream_t stream);

/* PPO.update minibatch loop: ppo_epoch x (T*N / (T*N/num_mini_batch)) Adam steps per task, rows
 * perms[e][b*mb:(b+1)*mb].  params/adam_m/adam_v [P][L] updated in place, adam_step [P] int32
 * incremented per step, lr [P].  stats [P][3] = mean (value_loss, action_loss, dist_entropy).
 * workspace: caller-owned device bytes (pgm_ppo_update_workspace_bytes), required (PGM_E_INVALID_ARG
 * when NULL), reset inside the call on `stream` unless pgm_ppo_update_reset did it since the last call.
 * The critic and actor towers of a task run on separate CUs that exchange the squared gradient norm per
 * minibatch step.  obs_dim <= 32 and small per-GPU populations (>= 4 parts per tower fit: 16 NS ceil(P/8) <= CUs,
 * or <= 2 x CUs with two workgroups per CU when each part takes two 16-row tiles; minibatch rows a multiple of 16 NS):
 * each tower on NS = 16 / 8 / 6 / 4 workgroups that split the minibatch rows, the four waves of a workgroup split the
 * hidden features, and the gradient is reduce-scattered over the parts before Adam (the feature-split update;
 * opts->fs_one_per_cu keeps one workgroup per CU).  Otherwise each tower is split over four CUs (a quarter of the minibatch rows each, gradient
 * images added through the workspace) while 64 * ceil(P/8) <= CU count, else over two CUs while
 * 32 * ceil(P/8) <= CU count (obs_dim > 32: 32 * ceil(P/4) / 16 * ceil(P/4)).  obs_dim <= 32: tower
 * images LDS-resident (falls back to 2 CUs per task, then 1, as P grows); obs_dim > 32 (Humanoid): layer
 * 1 streamed from L2, needs 2P <= CU count (PGM_E_UNSUPPORTED otherwise: shard the tasks over more
 * GPUs).  opts->update_split caps the row split; opts->update_kernel = PGM_UPDATE_FS forces the feature-split
 * update wherever it fits, PGM_UPDATE_ROWSPLIT the row-split kernels.
 * After the call, the 8-byte word at index 2P of the workspace is nonzero iff an exchange timed out
 * (the workgroups were not co-resident); the results of such a call are invalid.
 * d->LN = 1: ppo_update_ln_kernel, one workgroup per tower with the tower's parameters and Adam moments LDS-resident,
 * the same norm granules and timeout word; needs 2P <= CU count (PGM_E_UNSUPPORTED otherwise); opts ignored. */
int pgm_ppo_update(const pgm_dims* d, const pgm_ppo_hparams* hp, float* params, float* adam_m,
                   float* adam_v, int32_t* adam_step, const float* lr, const int32_t* perms,
                   const pgm_rollout_buf* rb, float* stats, void* workspace, const pgm_launch_opts* opts,
                   pgm_stream_t stream);
/* Workspace bytes for dims d; monotone in d->P, so a workspace sized for P serves every call with P' <= P tasks
 * (the same other dims). */
size_t pgm_ppo_update_workspace_bytes(const pgm_dims* d);
/* The update kernel pgm_ppo_update would launch for these dims, hyper-parameters and opts on the current device
 * (the same selection rule), as text into buf[n]
 * (e.g. "ppo_update_fs_kernel (NS=16, R=1)", "... (NS=8, R=2, 2 per CU)"): what benchmarks and profiles report.  No reference
 * counterpart (diagnostic). */
int pgm_ppo_update_variant(const pgm_dims* d, const pgm_ppo_hparams* hp, const pgm_launch_opts* opts, char* buf,
                           int n);
/* Zero, on `stream`, the part of the workspace the next pgm_ppo_update for dims d would reset inside the call,
 * and let that call skip its own reset (the caller orders this stream before the update's stream and after
 * every read of the previous update's timeout word).  Lets a caller take the reset off the update's stream. */
int pgm_ppo_update_reset(const pgm_dims* d, void* workspace, pgm_stream_t stream);
/* The feature-split update's fragment map (diagnostic, no reference counterpart): for tower m (0 critic, 1 actor)
 * of dims (O, A, K), O <= 32, out[(b * 64 + l) * 4 + r] = the tower-image index the kernel keeps in register r of
 * lane l of exchange block b (-1: padding), for every block b < NB; returns NB or a negative status (cap = out's
 * length in entries, >= 256 NB).  Host-only, no device work. */
int pgm_ppo_fs_fragment_map(int32_t O, int32_t A, int32_t K, int32_t m, int32_t* out, int32_t cap);

/* evaluation(): eval_num deterministic episodes per task from s0_eval [eval_num][O], obs normalised
 * with the snapshot ob_mean/ob_var [P][O] (use_ob_rms), objs_out [P][K] fp64 (discounted by gamma
 * unless raw). */
int pgm_eval(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const double* ob_mean,
             const double* ob_var, const double* s0_eval, int32_t eval_num, int32_t use_ob_rms, int32_t raw,
             double gamma, double* objs_out, const pgm_launch_opts* opts, pgm_stream_t stream);

/* ---- Several runs in one population (discovered by the presence of the symbol pgm_rollout_runs; no feature bit, no
 * version change).  The tasks of several runs of a sweep (one seed each, a2c_ppo_acktr/envs.py make_env(seed + rank)
 * per env process; the launchers scripts/<env>.py start --num-seeds of them per selection method) share one device
 * population.  Action noise, minibatch permutations and the learning-rate schedule depend on the iteration only
 * (morl/mopg.py:96), so the one thing a run owns on the device is its reset state.  run_of_task is a DEVICE int32 [P];
 * st->s0 is read as [num_runs][N][O] and s0_eval as [num_runs][eval_num][O]; task p uses block run_of_task[p] at its
 * initial reset, at every auto-reset and at every evaluation start.  Nothing else differs from pgm_env_reset /
 * pgm_rollout / pgm_eval: the arithmetic, the thread roles, the stored fields, the counter streams keyed by `seed`, the
 * kernel families and pgm_launch_opts; with num_runs = 1 and all-zero ids the outputs are theirs bit for bit.
 * Validation: every check of the entry point each extends, in its order and with its strings; then a NULL run_of_task
 * or num_runs < 1 is PGM_E_INVALID_ARG naming the _runs entry point.  The ids are device memory and are not read on
 * the host: the caller guarantees 0 <= run_of_task[p] < num_runs. */
int pgm_env_reset_runs(const pgm_dims* d, const pgm_env_spec* spec, const pgm_env_state* st, const pgm_norm_state* ns,
                       const int32_t* run_of_task, int32_t num_runs, float* obs_out, pgm_stream_t stream);
int pgm_rollout_runs(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const pgm_env_state* st,
                     const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* noise, uint64_t seed,
                     int32_t carry, const int32_t* run_of_task, int32_t num_runs, const pgm_launch_opts* opts,
                     pgm_stream_t stream);
int pgm_eval_runs(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const double* ob_mean,
                  const double* ob_var, const double* s0_eval, int32_t eval_num, int32_t use_ob_rms, int32_t raw,
                  double gamma, double* objs_out, const int32_t* run_of_task, int32_t num_runs,
                  const pgm_launch_opts* opts, pgm_stream_t stream);

/* ---- Per-task PPO settings (discovered by the presence of the symbol pgm_ppo_update_tasks; no feature bit, no version
 * change).  The runs of a sweep that differ in a hyper-parameter share one population: task p takes the four loss /
 * clip settings from hp_task[p] and its GAE lambda from lam_task[p]; lr is [P] already.  Everything else comes from
 * the shared arguments: the Adam constants, ppo_epoch, num_mini_batch, use_clipped_value_loss, gamma (which also
 * enters the rollout's return normalisation and the evaluation discount) and the shapes.  The kernel selection rule,
 * pgm_ppo_update_variant and pgm_ppo_update_workspace_bytes are pgm_ppo_update's: none of them reads the four fields.
 * The kernels are the TASKS instantiations of the ones pgm_ppo_update / pgm_gae launch: a workgroup serves one task
 * and replaces the launch's values by one wave-uniform 16-byte (4-byte) load before anything reads them; with every
 * entry equal to the shared value the outputs are pgm_ppo_update's / pgm_gae's bit for bit.
 * Validation: every check of the entry point each extends, in its order and with its strings; then a NULL table is
 * PGM_E_INVALID_ARG naming the _tasks entry point.  The tables are DEVICE memory ([P], the pgm_task_hparams array
 * 16-byte aligned) and are not read on the host: the caller guarantees finite values, clip_param > 0,
 * max_grad_norm > 0 and 0 <= lam <= 1. */
typedef struct pgm_task_hparams {
    float clip_param, value_loss_coef, entropy_coef, max_grad_norm;
} pgm_task_hparams;
int pgm_ppo_update_tasks(const pgm_dims* d, const pgm_ppo_hparams* hp, const pgm_task_hparams* hp_task, float* params,
                         float* adam_m, float* adam_v, int32_t* adam_step, const float* lr, const int32_t* perms,
                         const pgm_rollout_buf* rb, float* stats, void* workspace, const pgm_launch_opts* opts,
                         pgm_stream_t stream);
int pgm_gae_tasks(const pgm_dims* d, const pgm_rollout_buf* rb, float gamma, const float* lam_task, int32_t use_gae,
                  int32_t use_proper_time_limits, pgm_stream_t stream);

/* ---- Host-stepped environments (from minor 1). The environments run on the host; policy, VecNormalize
 * statistics, rollout storage and the PPO update stay on the device.  One rollout step t is
 *     pgm_rollout_act(t) -> copy action_out to the host -> envs.step(actions) -> copy the transition to the device
 *     -> pgm_env_ingest(t)
 * and pgm_rollout_act(T) after the last step writes the bootstrap value.  Neither touches a storage slot other than
 * the ones named below; pgm_env_spec and the synthetic dynamics play no part.
 *
 * Policy.act for rollout step t of every task (morl/mopg.py:105-108; t == T: get_value, :132-135).  Reads
 * rb->obs[p][t].  0 <= t < T: writes rb->values[p][t], rb->actions[p][t], rb->logp[p][t] and the raw (unclipped)
 * sampled action into action_out [P][N][A]; noise is the base of the [T][N][A] stream pgm_rollout takes (slice t is
 * read) and is required.  t == T: writes rb->values[p][T] only; noise and action_out may be NULL.  Other t:
 * PGM_E_SHAPE.  d->LN as pgm_act_forward. */
int pgm_rollout_act(const pgm_dims* d, const float* params, const pgm_rollout_buf* rb, int32_t t,
                    const float* noise, float* action_out, pgm_stream_t stream);

/* VecNormalize.step_wait + RolloutStorage.insert on one externally produced transition per env
 * (vec_normalize.py:29-66, morl/mopg.py:110-130, storage.py:50-62, the .float() of a2c_ppo_acktr/envs.py:192).
 * raw_obs fp64 [P][N][O] is what DummyVecEnv.step_wait returned (for a done env already its reset observation),
 * raw_obj fp64 [P][N][K] the step's info['obj'], reward fp64 [P][N] the scalar env reward (feeds ret / ret_rms),
 * done / bad_transition int32 [P][N]; all device pointers.
 * 0 <= t < T: ret = ret*gamma + reward; obj = obj*gamma + raw_obj (raw_obj while obj_acc_valid == 0); ob_rms update,
 * normalise, clip; ret_rms update; obj_rms update, scale and clip the objectives; zero ret / obj of done envs.
 * Writes rb->obs[p][t+1] (fp32), rb->rewards[p][t], rb->masks[p][t+1] = !done, rb->bad_masks[p][t+1] =
 * !bad_transition.
 * t == -1: a fresh make_vec_envs + reset(): ret = 0, obj_acc_valid = 0, ob_rms update + normalise; writes
 * rb->obs[p][0], masks[p][0] = bad_masks[p][0] = 1; raw_obj, reward, done, bad_transition may be NULL.
 * Other t: PGM_E_SHAPE.  Reads and writes st->obj_acc, st->obj_acc_valid, st->ret and all of ns; st->s,
 * st->elapsed, st->s0 are not read and may be NULL. */
int pgm_env_ingest(const pgm_dims* d, const pgm_env_state* st, const pgm_norm_state* ns,
                   const pgm_rollout_buf* rb, int32_t t, const double* raw_obs, const double* raw_obj,
                   const double* reward, const int32_t* done, const int32_t* bad_transition,
                   pgm_stream_t stream);

/* The evaluation forward with frozen statistics (morl/mopg.py:36-39): raw_obs fp64 [P][E][O], 1 <= E <= 8, is
 * normalised in fp64 as clip((ob - mean) / sqrt(var + 1e-8), -10, 10) when use_ob_rms (ob_mean / ob_var [P][O]), cast
 * to fp32 (never rounded to fp32 first) and action_out [P][E][A] receives the deterministic action dist.mean.
 * d->N and d->T are ignored.  d->LN as pgm_act_forward. */
int pgm_eval_act(const pgm_dims* d, const float* params, const double* ob_mean, const double* ob_var,
                 int32_t use_ob_rms, const double* raw_obs, int32_t E, float* action_out, pgm_stream_t stream);

/* count independent random permutations of [0, n) into out [count][n] (int32), keyed by seed. */
int pgm_randperm(int32_t n, int32_t count, uint64_t seed, int32_t* out, pgm_stream_t stream);

/* n standard-normal fp32 draws into out, element i keyed by (seed, i): the perf-mode noise stream. */
int pgm_normal_noise(int64_t n, uint64_t seed, float* out, pgm_stream_t stream);

/* ---- Discrete-action policies (pgm_abi_features() & PGM_FEATURE_CATEGORICAL).  The policy head is the reference's
 * Categorical (model.py:33-35, distributions.py:54-68): logits z = Linear(actor features), one integer action per
 * step.  In these entry points pgm_dims.A is the NUMBER OF ACTIONS; the stored action has width 1.  Environments are
 * host-stepped (pgm_env_ingest accepts the categorical dim sets; it never reads the action) or, for Deep Sea Treasure,
 * stepped on the device inside the fused rollout (pgm_rollout_dst / pgm_eval_dst below).  Built for
 * (O, A, K) = (3, 4, 2) (Deep Sea Treasure); pgm_dims.LN must be 0 (LayerNorm towers with a Categorical head are not
 * built: PGM_E_UNSUPPORTED).  Every entry point validates before any device work: NULL pointers, check of the dims,
 * the dim set, the step index or E, LN.
 *
 * SAMPLING RULE (device and test reference alike).  With fp32 logits z[0..A), m = max_j z_j, e_j = exp(z_j - m),
 * s = e_0 + ... + e_{A-1} (index order), p_j = e_j / s and one uniform u in [0, 1) per (step, env):
 *     action = #{ j < A-1 : p_0 + ... + p_j <= u }      (the partial sums in index order)
 * so the action is always in [0, A); logp = z_a - (m + log s).  Deterministic: the lowest index among the maxima of
 * z (FixedCategorical.mode = probs.argmax, distributions.py:27).  torch draws Categorical.sample through multinomial,
 * whose stream is not reproduced: the rule is equal in distribution, not in draws.
 *
 * Storage: rb->actions is [P][T][N][1] fp32 holding the action index (exact; the reference's width-1 action tensor,
 * storage.py:19-25); every other buffer as for the Gaussian head. */
int pgm_abi_features(void); /* bit mask of PGM_FEATURE_* up to 4 (frozen at 7); a library without this symbol has none */
int pgm_abi_feature_mask(void); /* bit mask of every PGM_FEATURE_*; a library without this symbol: pgm_abi_features() */

/* offsets[PGM_NUM_PARAM_TENSORS_CAT] (floats; indices 0..9 in PGM_P_* order, then PGM_PC_LINEAR_W / _B), every tensor
 * 16-byte aligned, *total a multiple of 64 floats. */
int pgm_param_layout_cat(int32_t O, int32_t A, int32_t K, int32_t H, int32_t* offsets, int32_t* total);

/* Policy.act on obs [P][N][O] (model.py:57-69 with dist = Categorical).  uniforms [N] (shared by tasks) draws by the
 * sampling rule; deterministic = 1 takes the mode (uniforms ignored, may be NULL).  Outputs value [P][N][K],
 * action int32 [P][N], logp [P][N]. */
int pgm_act_forward_cat(const pgm_dims* d, const float* params, const float* obs, const float* uniforms,
                        int32_t deterministic, float* value, int32_t* action, float* logp, pgm_stream_t stream);

/* pgm_rollout_act with a Categorical head (morl/mopg.py:105-108; t == T: get_value, :132-135).  Reads rb->obs[p][t].
 * 0 <= t < T: writes rb->values[p][t], rb->actions[p][t] (the index as fp32), rb->logp[p][t] and the index into
 * action_out int32 [P][N]; uniforms is the base of a [T][N] stream (slice t is read) and is required.  t == T: writes
 * rb->values[p][T] only; uniforms and action_out may be NULL.  Other t: PGM_E_SHAPE. */
int pgm_rollout_act_cat(const pgm_dims* d, const float* params, const pgm_rollout_buf* rb, int32_t t,
                        const float* uniforms, int32_t* action_out, pgm_stream_t stream);

/* pgm_eval_act with a Categorical head (morl/mopg.py:36-39): the same fp64 normalisation of raw_obs [P][E][O],
 * 1 <= E <= 8, then the deterministic action into action_out int32 [P][E]. */
int pgm_eval_act_cat(const pgm_dims* d, const float* params, const double* ob_mean, const double* ob_var,
                     int32_t use_ob_rms, const double* raw_obs, int32_t E, int32_t* action_out, pgm_stream_t stream);

/* PPO.update (a2c_ppo_acktr/algo/ppo.py:58-115) with FixedCategorical log_probs and entropy (model.py:75-82):
 * arguments as pgm_ppo_update, params / adam_m / adam_v [P][L] in the pgm_param_layout_cat layout, rb->actions
 * [P][T][N][1].  Per sample with taken action a: p = softmax(z), logp = log p_a, H = -sum_j p_j log p_j; the loss is
 * the clipped surrogate on exp(logp - old logp), the (clipped) value loss and -entropy_coef mean(H).
 * stats [P][3] = mean (value_loss, action_loss, entropy).  ppo_update_cat_kernel: one 256-thread workgroup per tower
 * with the tower's parameters and Adam moments LDS-resident, the norm granules and timeout word (8-byte word 2P of the
 * workspace) of pgm_ppo_update; needs 2 P <= CU count and all working workgroups co-resident (PGM_E_UNSUPPORTED
 * otherwise: shard the tasks over more GPUs).  workspace: pgm_ppo_update_cat_workspace_bytes(d) caller-owned device
 * bytes, reset inside the call on `stream`. */
int pgm_ppo_update_cat(const pgm_dims* d, const pgm_ppo_hparams* hp, float* params, float* adam_m, float* adam_v,
                       int32_t* adam_step, const float* lr, const int32_t* perms, const pgm_rollout_buf* rb,
                       float* stats, void* workspace, pgm_stream_t stream);
size_t pgm_ppo_update_cat_workspace_bytes(const pgm_dims* d); /* monotone in d->P */

/* n uniform fp32 draws in [0, 1) with 24 random bits into out, element i keyed by (seed, i) through the counter hash
 * of pgm_normal_noise: the perf-mode stream of the sampling rule. */
int pgm_uniform_noise(int64_t n, uint64_t seed, float* out, pgm_stream_t stream);

/* ---- Deep Sea Treasure on the device (pgm_abi_features() & PGM_FEATURE_DST_DEVICE).  The env of the reference's
 * environments/deep_sea_treasure.py:111-183 as pgmorl_amd/hostenv.py states it: an 11 x 11 grid, cell (r, c) open if
 * r == 0 or r <= c or a treasure ((1,0) = 1, (2,1) = 3, (4,3) = 8, (7,6) = 20); actions 0 up, 1 down, 2 left, 3 right
 * (a move off the grid or into a wall stays); step += 1 per transition; on a treasure reward = obj0 = its value and
 * obj1 = 10 / (step + 1), else 0; done = found || step >= max_steps; bad = time_limit_is_bad && limit && !found; a
 * done env resets to (0, 0, 0) and the returned observation is the reset one; raw observation
 * [r / 10, c / 10, step / max_steps], each rounded to fp32 and widened.  The rule is ONE inline function
 * (pgmorl_amd/csrc/pgm_dst.hpp) used by the two kernels and by pgm_dst_transition.  Dims (3, 4, 2), LN = 0.
 * Validation before any device work: NULL pointers (PGM_E_INVALID_ARG), the dims, the dim set (PGM_E_UNSUPPORTED), LN,
 * T <= 0 (PGM_E_SHAPE), eval_num outside 1..8 (PGM_E_INVALID_ARG), max_steps <= 0 (PGM_E_INVALID_ARG). */
typedef struct pgm_dst_spec {
    int32_t max_steps;         /* episode step limit (the env's default: 50) */
    int32_t time_limit_is_bad; /* 0: the limit ends an episode as a termination (the env's own report); 1: as a
                                  time-limit end (bad_transition, a2c_ppo_acktr/envs.py:122-131) */
} pgm_dst_spec;

/* T rollout steps of every task in one launch (morl/mopg.py:103-135 with the env, DummyVecEnv's auto-reset
 * dummy_vec_env.py:45-56 and VecNormalize.step_wait vec_normalize.py:29-43 on the device): per step Policy.act on
 * rb->obs[p][t] by the sampling rule, the transition of every env, the running statistics (the scalar treasure reward
 * feeds VecNormalize.ret / ret_rms), insert into slot t + 1; then the bootstrap value into rb->values[p][T].  Writes
 * what T pgm_rollout_act_cat / pgm_env_ingest pairs plus pgm_rollout_act_cat(T) write, bit for bit.  st->s [P][N][3]
 * holds (row, col, step) as integer-valued fp64; st->elapsed and st->s0 are not read and may be NULL.  uniforms
 * [T][N] shared by the tasks, or NULL: element (t, n) is then element t * N + n of pgm_uniform_noise's stream of
 * `seed`, drawn in the kernel.  carry != 0: slot T -> slot 0 first (storage.py:71-75).  rb->returns / adv are not
 * touched.  A fresh run starts from st->s = 0 and pgm_env_ingest(t = -1) on the all-zero reset observation. */
int pgm_rollout_dst(const pgm_dims* d, const float* params, const pgm_dst_spec* env, const pgm_env_state* st,
                    const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* uniforms, uint64_t seed,
                    int32_t carry, pgm_stream_t stream);

/* evaluation() (morl/mopg.py:25-46): eval_num (1..8) episodes per task from (0, 0, 0) with the deterministic action
 * (the lowest index among the maxima of the logits) on the raw fp64 observation normalised with the frozen ob_mean /
 * ob_var [P][3] (use_ob_rms; not rounded through fp32 first); per episode acc += disc * obj, disc *= gamma unless raw;
 * objs_out [P][2] fp64 = sum over episodes / eval_num.  pgm_dims.N and T are ignored. */
int pgm_eval_dst(const pgm_dims* d, const float* params, const pgm_dst_spec* env, const double* ob_mean,
                 const double* ob_var, int32_t eval_num, int32_t use_ob_rms, int32_t raw, double gamma,
                 double* objs_out, pgm_stream_t stream);

/* The env rule on n (state, action) pairs, on the HOST (environments/deep_sea_treasure.py:111-183): launches nothing,
 * needs no device, every pointer a host pointer.  Outputs: the state after the auto-reset, raw_obs_out [n][3] of that
 * state, obj_out [n][2], reward_out [n], done_out / bad_out [n]. */
int pgm_dst_transition(const pgm_dst_spec* spec, int32_t n, const int32_t* row, const int32_t* col,
                       const int32_t* step, const int32_t* action, int32_t* row_out, int32_t* col_out,
                       int32_t* step_out, double* raw_obs_out, double* obj_out, double* reward_out, int32_t* done_out,
                       int32_t* bad_out);

/* ---- MO-Dummy-v0 / MO-Dummy3-v0 on the device (pgm_abi_features() & PGM_FEATURE_DUMMY_DEVICE).  The reference's
 * environments/dummy_mo_env.py:57-148 (registered with max_steps 500, environments/__init__.py:4-16): continuous
 * actions, obs 6, act 2, 2 or 3 objectives, Gaussian head.  With that bit the dim sets (6, 2, 2) and (6, 2, 3) are
 * accepted by every Gaussian entry point (pgm_act_forward, pgm_rollout_act, pgm_env_ingest, pgm_eval_act, pgm_gae,
 * pgm_adv_normalize, pgm_ppo_update, plain and LayerNorm towers).
 * State of one env: pos[2], vel[2], total_distance, total_energy (fp64) and an integer step; the raw observation is
 * those six fp64 values (never rounded through fp32).  One step with the policy's raw fp32 action a:
 *   ac = clip((double)a, -1, 1); last = pos; vel = (vel + ac * 0.1) * 0.95; pos = pos + vel; step += 1
 *   step_distance = sqrt(dx*dx + dy*dy) with d = pos - last; step_energy = sqrt(ac0*ac0 + ac1*ac1); totals accumulate
 *   obj0 = step_distance; obj1 = 1 / (step_energy + 0.1); obj2 = bound - |pos| (K = 3); reward = obj0 + 0.1 * obj1
 *   done = step >= max_steps || |pos| > bound; bad = time_limit_is_bad && done && step == max_steps
 * A done env resets: vel, totals, step = 0, its episode counter e += 1 and pos = reset_table[env][e mod R]; the
 * returned observation is the reset state, the objectives, reward and flags are the terminal step's.  The reference
 * draws the reset position from numpy's unseeded global stream; the table (envspec.dummy_reset_table) restates it
 * reproducibly.  No product is contracted into an fma: the rule gives the same bits on the host and on the device.  It
 * is ONE inline function (pgmorl_amd/csrc/pgm_dummy.hpp) used by the two kernels and by pgm_dummy_transition.
 * Validation before any device work: NULL pointers (PGM_E_INVALID_ARG), the dims, the dim set (PGM_E_UNSUPPORTED),
 * LN (as pgm_act_forward), T <= 0 (PGM_E_SHAPE), eval_num outside 1..8, max_steps <= 0, bound <= 0, R < 1,
 * reset_count below the rows the call reads (PGM_E_INVALID_ARG). */
typedef struct pgm_dummy_spec {
    int32_t max_steps;         /* episode step limit (the registration's: 500) */
    int32_t time_limit_is_bad; /* 1 (the registration's TimeLimitMask): an end on the limit step is a time-limit end
                                  (bad_transition); 0: every end is a termination */
    double bound;              /* radius of the disc the env must stay in (the env's: 5.0) */
    const double* reset_table; /* [reset_count][R][2] fp64 reset positions; a device pointer for the kernels, a host
                                  pointer for pgm_dummy_transition */
    int32_t R;                 /* reset positions per env; episode e starts at entry e mod R */
    int32_t reset_count;       /* rows of the table: >= N (rollout), >= eval_num (evaluation) */
} pgm_dummy_spec;

/* T rollout steps of every task in one launch (morl/mopg.py:103-135 with the env, DummyVecEnv's auto-reset and
 * VecNormalize.step_wait on the device): per step Policy.act on rb->obs[p][t] (value, action = noise * exp(logstd) +
 * mean, log-prob summed over the 2 actions in index order, the raw action into rb->actions), the transition of every
 * env, the running statistics (the scalar reward feeds VecNormalize.ret / ret_rms), insert into slot t + 1; then the
 * bootstrap value into rb->values[p][T].  Writes what T pgm_rollout_act / pgm_env_ingest pairs plus
 * pgm_rollout_act(T) write, bit for bit.  st->s [P][N][6] holds the six state values, st->elapsed [P][N] the step,
 * episode [P][N] the episode counters (all read and written back); st->s0 is not read and may be NULL.  Env n of every
 * task uses row n of the reset table.  noise [T][N][2] shared by the tasks, or NULL: element (t, n, a) is then element
 * (t * N + n) * 2 + a of pgm_normal_noise's stream of `seed`, drawn in the kernel.  carry != 0: slot T -> slot 0 first
 * (storage.py:71-75).  rb->returns / adv are not touched.  A fresh run starts from pos = reset_table[n][0], everything
 * else 0, and pgm_env_ingest(t = -1) on that observation. */
int pgm_rollout_dummy(const pgm_dims* d, const float* params, const pgm_dummy_spec* env, const pgm_env_state* st,
                      int32_t* episode, const pgm_norm_state* ns, const pgm_rollout_buf* rb, const float* noise,
                      uint64_t seed, int32_t carry, pgm_stream_t stream);

/* evaluation() (morl/mopg.py:25-46): eval_num (1..8) episodes per task, episode e from pos = reset_table[e][0], with
 * the mean action on the raw fp64 observation normalised with the frozen ob_mean / ob_var [P][6] (use_ob_rms); per
 * episode acc += disc * obj, disc *= gamma unless raw; an ended episode stands still; objs_out [P][K] fp64 = sum over
 * the episodes in index order / eval_num.  pgm_dims.N and T are ignored. */
int pgm_eval_dummy(const pgm_dims* d, const float* params, const pgm_dummy_spec* env, const double* ob_mean,
                   const double* ob_var, int32_t eval_num, int32_t use_ob_rms, int32_t raw, double gamma,
                   double* objs_out, pgm_stream_t stream);

/* The env rule on n (state, action) pairs, on the HOST: launches nothing, needs no device, every pointer a host
 * pointer (spec->reset_table included).  K = 2 or 3.  Inputs: state [n][6], step / episode [n], env [n] (the pair's row
 * of the reset table, in [0, reset_count)), action fp32 [n][2].  Outputs: the state after the auto-reset (= the raw
 * observation) state_out [n][6], step_out / episode_out [n], obj_out [n][K], reward_out [n], done_out / bad_out [n]. */
int pgm_dummy_transition(const pgm_dummy_spec* spec, int32_t K, int32_t n, const double* state, const int32_t* step,
                         const int32_t* episode, const int32_t* env, const float* action, double* state_out,
                         int32_t* step_out, int32_t* episode_out, double* obj_out, double* reward_out,
                         int32_t* done_out, int32_t* bad_out);

/* ---- Host-stepped environments of any dims (pgm_abi_feature_mask() & PGM_FEATURE_ANY_DIMS).  One kernel family compiled
 * for dims up to (O, A, K) = (32, 8, 3) and launched with the true dims of pgm_dims: plain towers (LN = 0), H = 64,
 * 1 <= O <= 32, 1 <= K <= 3, N <= 8; head = 0: Gaussian, 1 <= A <= 8 action dims, params in the pgm_param_layout
 * layout; head = 1: Categorical, 2 <= A <= 8 actions, params in the pgm_param_layout_cat layout, the SAMPLING RULE
 * above.  Every buffer has the true dims as strides (rb->obs [P][T+1][N][O], ...).  On a dim set the compiled entry
 * points support, pgm_rollout_act_any / pgm_eval_act_any / pgm_env_ingest_any write what those write, bit for bit.
 * Every call validates before any device work: NULL pointers, the dims (H, N), the range above (PGM_E_UNSUPPORTED
 * naming the limit), LN != 0 (PGM_E_UNSUPPORTED), then the step index, E or the minibatch shape.
 * pgm_gae, pgm_adv_normalize, pgm_param_layout(_cat), pgm_normal_noise, pgm_uniform_noise and pgm_randperm take
 * runtime dims already. */

/* pgm_rollout_act / pgm_rollout_act_cat.  rnd: base of [T][N][A] normals (head 0) or [T][N] uniforms (head 1);
 * action_out: float [P][N][A] or int32_t [P][N].  t == T writes rb->values[p][T] only (rnd, action_out may be NULL). */
int pgm_rollout_act_any(const pgm_dims* d, int32_t head, const float* params, const pgm_rollout_buf* rb, int32_t t,
                        const float* rnd, void* action_out, pgm_stream_t stream);

/* pgm_eval_act / pgm_eval_act_cat: raw_obs [P][E][O] fp64, 1 <= E <= 8; action_out float [P][E][A] or int32_t [P][E]. */
int pgm_eval_act_any(const pgm_dims* d, int32_t head, const float* params, const double* ob_mean,
                     const double* ob_var, int32_t use_ob_rms, const double* raw_obs, int32_t E, void* action_out,
                     pgm_stream_t stream);

/* pgm_env_ingest: t = -1 is the reset; no auto-reset; the scalar reward feeds VecNormalize.ret.  d->A is not read
 * beyond its range check (1..8). */
int pgm_env_ingest_any(const pgm_dims* d, const pgm_env_state* st, const pgm_norm_state* ns,
                       const pgm_rollout_buf* rb, int32_t t, const double* raw_obs, const double* raw_obj,
                       const double* reward, const int32_t* done, const int32_t* bad_transition, pgm_stream_t stream);

/* PPO.update (arguments as pgm_ppo_update_cat) with the head's log-prob and entropy.  ppo_update_any_kernel: one
 * 256-thread workgroup per tower, parameters and Adam moments LDS-resident; needs 2 P <= CU count (PGM_E_UNSUPPORTED
 * otherwise).  workspace: pgm_ppo_update_any_workspace_bytes(d) caller-owned device bytes, reset inside the call. */
int pgm_ppo_update_any(const pgm_dims* d, int32_t head, const pgm_ppo_hparams* hp, float* params, float* adam_m,
                       float* adam_v, int32_t* adam_step, const float* lr, const int32_t* perms,
                       const pgm_rollout_buf* rb, float* stats, void* workspace, pgm_stream_t stream);
size_t pgm_ppo_update_any_workspace_bytes(const pgm_dims* d); /* monotone in d->P */

/* ---- Re-evaluation of a saved Pareto set (discovered by the presence of the symbol pgm_eval_episodes; no feature bit,
 * no version change).  evaluation() (morl/mopg.py:25-46) of each of d->P = M policies (d->N and d->T are not read) from
 * each of the E start states starts [E][O], on the SynthMO device envs; M is not a training population and may be in
 * the thousands.  Grid (M, ceil(E / 8)), 256 threads: workgroup (m, c) runs episodes 8c .. min(8c + 8, E) - 1 of
 * policy m as the rows of one policy forward per step, with the arithmetic of pgm_eval's block kernel row by row.
 * ob_mean / ob_var [M][O]: each policy's own frozen statistics (use_ob_rms).  stochastic != 0: the action is
 * fmaf(z, exp(logstd), mean) before the env's clip, z for (episode e, step t, action dim j) being element
 * (e * spec->max_episode_steps + t) * A + j of the counter stream pgm_normal_noise(noise_seed) -- the same for every
 * policy (common random numbers across the front); stochastic == 0 does not read noise_seed.
 * episodes_out [M][E][K] fp64: each episode's sum of g * obj, g = gamma^t unless raw.  objs_out [M][K] (may be NULL):
 * the episode sums added in index order, divided by E.
 * Validation, before any device work, in this order: NULL pointers (d, params, spec, starts, episodes_out; ob_mean /
 * ob_var with use_ob_rms) PGM_E_INVALID_ARG; the dims with N = 1, T = 0 as pgm_eval_act checks them; pgm_dims.LN;
 * a NULL field of spec or max_episode_steps <= 0 PGM_E_INVALID_ARG; 1 <= E <= 65536 else PGM_E_SHAPE; then a dim set
 * no kernel is compiled for PGM_E_UNSUPPORTED. */
int pgm_eval_episodes(const pgm_dims* d, const float* params, const pgm_env_spec* spec, const double* ob_mean,
                      const double* ob_var, const double* starts, int32_t E, int32_t use_ob_rms, int32_t raw,
                      double gamma, int32_t stochastic, uint64_t noise_seed, double* episodes_out, double* objs_out,
                      pgm_stream_t stream);

/* ---- Evaluation of policies blended between two members of a Pareto set (discovered by the presence of the symbol
 * pgm_eval_blend; no feature bit, no version change).  Candidate q of d->P = Q candidates (d->N and d->T are not read)
 * is (a, b) = src[q], alpha[q]: its parameter i is
 *     (float)((1.0 - alpha) * (double)params[a][i] + alpha * (double)params[b][i])
 * -- two fp64 products and one fp64 sum, each rounded on its own (no fma contraction), then one round to fp32 -- and its
 * ob_mean / ob_var (use_ob_rms) the same expression in fp64 without the last round, so alpha = 0 is member a and
 * alpha = 1 member b.  params [M][L], ob_mean / ob_var [M][O]: the M members, resident once; src int32 [Q][2] and alpha
 * fp64 [Q] are DEVICE memory and are not read on the host.  The blend is formed in the kernel's weight load: no
 * candidate is materialised.  evaluation() (morl/mopg.py:25-46) of each candidate, deterministic policy, from each of
 * the E start states starts [E][O], on the SynthMO device envs.  One wave per (candidate, episode) with pgm_eval's wave
 * kernel body: work item w = q * E + e, 4 waves per 256-thread workgroup, grid ceil(Q * E / 4); no LDS and no
 * workgroup barrier.  A candidate whose src entry lies outside [0, M) reads no parameters and gets NaN in its K sums
 * of every episode.
 * episodes_out [Q][E][K] fp64: each episode's sum of g * obj, g = gamma^t unless raw.  objs_out [Q][K] (may be NULL):
 * the episode sums added in index order, divided by E (the kernel pgm_eval_episodes uses).
 * Plain towers at the dims of the wave kernel only (obs_dim <= 48, K <= 4: every SynthMO dim set but 376/17/2): for
 * LayerNorm towers and MO-Humanoid the caller materialises the candidates and uses pgm_eval_episodes.
 * Validation, before any device work, in this order: NULL pointers (d, params, src, alpha, spec, starts, episodes_out;
 * ob_mean / ob_var with use_ob_rms) PGM_E_INVALID_ARG; the dims with N = 1, T = 0 as pgm_eval_act checks them;
 * pgm_dims.LN, then LN = 1 PGM_E_UNSUPPORTED; a NULL field of spec or max_episode_steps <= 0 PGM_E_INVALID_ARG; M >= 1,
 * 1 <= E <= 65536 and Q * E <= 2^24 else PGM_E_SHAPE; then a dim set outside the wave kernel PGM_E_UNSUPPORTED. */
int pgm_eval_blend(const pgm_dims* d, const float* params, int32_t M, const double* ob_mean, const double* ob_var,
                   const int32_t* src, const double* alpha, const pgm_env_spec* spec, const double* starts, int32_t E,
                   int32_t use_ob_rms, int32_t raw, double gamma, double* episodes_out, double* objs_out,
                   pgm_stream_t stream);

/* ---- Evaluation of policies blended among three members of a Pareto set: the simplex candidates of a three-objective
 * front (discovered by the presence of the symbol pgm_eval_blend3; no feature bit, no version change).  Candidate q of
 * d->P = Q candidates is (a, b, c) = src[q], (wa, wb, wc) = w[q]: its parameter i is
 *     (float)((wa * (double)params[a][i] + wb * (double)params[b][i]) + wc * (double)params[c][i])
 * -- three fp64 products and two fp64 sums, left to right, each rounded on its own (no fma contraction), then one round
 * to fp32 -- and its ob_mean / ob_var (use_ob_rms) the same expression in fp64 without the last round.  So
 * (i, i, i, 1, 0, 0) is member i, (a, b, b, 1 - alpha, alpha, 0) has the value of pgm_eval_blend's (a, b, alpha), and
 * swapping the first two (index, weight) slots changes no bit.  src int32 [Q][3] and w fp64 [Q][3] are DEVICE memory
 * and are not read on the host; the caller keeps the weights in [0, 1] with sum 1.  Everything else -- the members,
 * the start states, the kernel form (one wave per (candidate, episode), work item w = q * E + e, 4 waves per
 * 256-thread workgroup, no LDS, no workgroup barrier), the NaN of a candidate whose src names a member outside
 * [0, M), episodes_out [Q][E][K], objs_out [Q][K] (may be NULL), the dims covered and the validation order with its
 * limits -- is pgm_eval_blend's, with w in the place of alpha; every message starts with "pgm_eval_blend3:". */
int pgm_eval_blend3(const pgm_dims* d, const float* params, int32_t M, const double* ob_mean, const double* ob_var,
                    const int32_t* src, const double* w, const pgm_env_spec* spec, const double* starts, int32_t E,
                    int32_t use_ob_rms, int32_t raw, double gamma, double* episodes_out, double* objs_out,
                    pgm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
