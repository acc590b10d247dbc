"""MOPGPopulation: the drop-in replacement of the per-task process fan-out of one generation.

Reference: morl/morl.py:79-99 forks one ``MOPG_worker`` process per task (morl/mopg.py:60-182) and
gathers ``{'task_id', 'offspring_batch', 'done'}`` dicts from a multiprocessing Queue.  Here every
task of the generation lives in one ``TaskBatch`` on the GPU and each PPO iteration of all tasks
is a short sequence of libpgm kernels; ``run`` returns the same ``all_offspring_batch`` structure
(list over tasks of the per-iteration offspring Samples), so the rest of the generation loop is
unchanged.

RNG: ``rng='host'`` draws exactly what the reference draws for iteration j (torch.manual_seed(j),
then T Normal samples of shape [N, A] and ppo_epoch randperms of T*N, morl/mopg.py:96 and
storage.py:133) and uploads them -- bit-compatible with the CPU oracle; ``rng='device'`` uses the
counter-based device streams keyed by j (same distribution, no host work; the benchmark mode).
Like the reference, all tasks of an iteration share one noise stream.
"""
import os
import time

import numpy as np
import torch

from .runtime import TaskBatch
from .sample import DeviceSnapshot, RowStore, RunningMeanStd, Sample
from .shard import allgather_rows, move_rows, owner_of, task_block, world


def host_draws(j, T, N, A, E):
    torch.manual_seed(j)
    z = torch.stack([torch.normal(torch.zeros(N, A, dtype=torch.float64), torch.ones(N, A, dtype=torch.float64))
                     for _ in range(T)])
    perms = torch.stack([torch.randperm(T * N) for _ in range(E)])
    return z.float(), perms.to(torch.int32)


def host_draws_discrete(j, T, N, E):
    """The host stream of a Categorical head: after torch.manual_seed(j), one torch.rand(N) per step for the
    sampling rule of include/pgm_abi.h, then the randperms.  torch draws Categorical.sample through multinomial,
    whose stream is not reproduced: equal in distribution to the reference, not in draws."""
    torch.manual_seed(j)
    u = torch.stack([torch.rand(N, dtype=torch.float32) for _ in range(T)])
    perms = torch.stack([torch.randperm(T * N) for _ in range(E)])
    return u, perms.to(torch.int32)


def linear_lr(j, total_num_updates, lr, ratio=1.0):
    """update_linear_schedule (a2c_ppo_acktr/utils.py:46-50) as called at morl/mopg.py:97-101."""
    return lr - lr * (j * ratio / float(total_num_updates))


# the settings a run of a sweep may own (morl.GRID_FIELDS): the learning rate and its decay ratio feed the per-task lr,
# the others the per-task tables of TaskBatch.set_task_hparams
RUN_LR_FIELDS = ('lr', 'lr_decay_ratio')
RUN_TASK_FIELDS = ('gae_lambda', 'clip_param', 'value_loss_coef', 'entropy_coef', 'max_grad_norm')


class MOPGPopulation:
    def __init__(self, args, device='cuda', rng='device', host_env=None, device_env=None, env_plugin=None,
                 run_seeds=None, run_hparams=None):
        """run_hparams (with run_seeds): one dict per run with the settings that run owns (any of RUN_LR_FIELDS and
        RUN_TASK_FIELDS; a missing key is ``args``' value).  Each generation they are expanded through run_of_task
        into the per-task tables (TaskBatch.set_task_hparams) and the per-task lr of every iteration.
        run_seeds: the seeds of the runs of a sweep that share this runtime's population (TaskBatch(run_seeds=...));
        run() and evaluate_samples() then take the run index of every task.  One rank only.
        host_env (default ``args.host_env``, the --host-env flag; None = the device envs): 'synth',
        'module:callable' or a factory (env_name, P, N, seed) -> hostenv.HostVecEnv.  The environments then run on
        the host and every TaskBatch of this runtime is built over a HostVecEnv of its own task slots (a rank holds
        host envs for its block of the population only).  device_env (default ``args.device_env``, the --device-env
        flag): a discrete-action env runs on the device (TaskBatch(device_env=True)); a no-op on the SynthMO envs.
        env_plugin (default ``args.env_plugin``, the --env-plugin flag): an envplug.EnvPlugin or the path of its header;
        every TaskBatch of this runtime runs the plug-in's fused kernels (the library is loaded once and reused when the
        batch is re-allocated at a larger capacity), or, with host_env 'plugin', steps the same header on the host.
        ``args.env_params`` (the --env-param flags, a dict name -> float) are the runtime parameters of a contract-2
        plug-in on either path."""
        self.args = args
        self.device = torch.device(device)
        self.rng = rng
        self.tb = None
        host_env = getattr(args, 'host_env', None) if host_env is None else host_env
        env_plugin = getattr(args, 'env_plugin', None) if env_plugin is None else env_plugin
        self.env_plugin = None
        if env_plugin is not None:
            from .envplug import as_plugin
            self.env_plugin = as_plugin(env_plugin)
            self.env_plugin.register(args.env_name)
        if host_env == 'plugin':
            if self.env_plugin is None:
                raise ValueError('host_env "plugin" steps an env plug-in on the host: give env_plugin=...')
            from .hostenv import PluginHostVecEnv
            plugin, env_params = self.env_plugin, getattr(args, 'env_params', None)
            host_env = lambda env_name, P, N, seed=0: PluginHostVecEnv(plugin, P, N, seed,  # noqa: E731
                                                                       env_params=env_params)
        if isinstance(host_env, str):
            from .hostenv import resolve
            host_env = resolve(host_env)
        self.host_env_factory = host_env
        self.device_env = bool(getattr(args, 'device_env', False) if device_env is None else device_env)
        self.moved_bytes = 0  # snapshot bytes this rank contributed to move_rows (multi-GPU)
        # the process-global streams run() reseeds itself (host_draws: torch.manual_seed(j)); morl.run_many reads this
        self.reseeds_global_streams = ('torch',) if rng == 'host' else ()
        self.run_seeds = None if run_seeds is None else [int(x) for x in run_seeds]
        if self.run_seeds is not None and world()[1] > 1:
            from ._lib import PGMError
            raise PGMError(f'run_seeds=... on {world()[1]} ranks: a multi-run population lives on one GPU '
                           f'(multi-GPU sweeps are not built)')
        self.run_hparams = None
        if run_hparams is not None:
            from ._lib import PGMError
            from .runtime import check_task_hparam
            if self.run_seeds is None or len(run_hparams) != len(self.run_seeds):
                raise PGMError(f'run_hparams=... holds one dict per run of run_seeds=...: got '
                               f'{len(run_hparams)} for {0 if self.run_seeds is None else len(self.run_seeds)} runs')
            self.run_hparams = [dict(h) for h in run_hparams]
            for h in self.run_hparams:
                for k, v in h.items():
                    if k in RUN_TASK_FIELDS:
                        check_task_hparam(k, v, 'run_hparams')
                    elif k not in RUN_LR_FIELDS:
                        raise PGMError(f'run_hparams: {k!r} is not a per-run setting (one of '
                                       f'{", ".join(RUN_LR_FIELDS + RUN_TASK_FIELDS)})')
                    elif not np.isfinite(float(v)):
                        raise PGMError(f'run_hparams: {k}={v!r} must be finite')

    @property
    def layout(self):
        """The flat parameter layout of this run's env dims (pgm_param_layout)."""
        from .envspec import make_spec
        from .layout import ParamLayout
        if self.tb is not None:
            return self.tb.layout
        spec = make_spec(self.args.env_name)
        return ParamLayout(spec['obs_dim'], spec['act_dim'], spec['obj_num'],
                           layernorm=bool(getattr(self.args, 'layernorm', False)),
                           discrete=bool(spec.get('discrete', False)))

    def _batch(self, P):
        """The one TaskBatch of this runtime, P active task slots.  Allocated once (re-allocated only when a
        generation needs more slots than any before): populations of varying size reuse its buffers."""
        a = self.args
        if self.tb is None or self.tb.capacity < P:
            cap = max(P, getattr(a, 'num_tasks', 0) or 0) if self.tb is None else P
            rank, ws = world()
            cap = min(cap, max(P, -(-cap // ws)))  # a rank only ever holds its block of the population
            he = None
            if self.host_env_factory is not None:
                if self.tb is not None and self.tb.host_env is not None:
                    self.tb.host_env.close()
                he = self.host_env_factory(a.env_name, cap, a.num_processes, a.seed)
            self.tb = TaskBatch(a.env_name, P, num_processes=a.num_processes, num_steps=a.num_steps, seed=a.seed,
                                eval_num=a.eval_num, gamma=a.gamma, gae_lambda=a.gae_lambda, use_gae=a.use_gae,
                                use_proper_time_limits=a.use_proper_time_limits, ob_rms=a.ob_rms,
                                obj_rms=a.obj_rms, raw=a.raw, clip_param=a.clip_param, ppo_epoch=a.ppo_epoch,
                                num_mini_batch=a.num_mini_batch, value_loss_coef=a.value_loss_coef,
                                entropy_coef=a.entropy_coef, max_grad_norm=a.max_grad_norm, device=self.device,
                                capacity=cap, layernorm=bool(getattr(a, 'layernorm', False)), host_env=he,
                                device_env=self.device_env,
                                env_plugin=self.env_plugin if he is None else None, run_seeds=self.run_seeds,
                                env_params=getattr(a, 'env_params', None) if he is None else None)
        else:
            self.tb.set_active(P)
        return self.tb

    def load_tasks(self, tb, samples, weights):
        """Restore every active slot from its elite (mopg.py:67-82 per task, here batched): parameters + Adam
        moments by one gather of the snapshots' [3, L] blocks, the running statistics and task weights by one
        H2D copy of a host-built stats64 image, the Adam steps by one small copy."""
        P = len(samples)
        tb.set_active(P)
        blocks = [s.snapshot.block() for s in samples]
        tb.state.copy_(torch.stack(blocks, dim=1))
        flat = tb.new_stats64()
        v = tb.stat_views(flat, P)
        K = tb.K
        for p, (s, w) in enumerate(zip(samples, weights)):
            v['weights'][p] = np.asarray(w, dtype=np.float64)
            ep = s.env_params or {}
            ob, rt, oj = ep.get('ob_rms'), ep.get('ret_rms'), ep.get('obj_rms')
            if ob is not None:
                v['ob_mean'][p], v['ob_var'][p], v['ob_count'][p] = ob.mean, ob.var, float(ob.count)
            if rt is not None:
                v['ret_mean'][p] = float(np.asarray(rt.mean).reshape(-1)[0])
                v['ret_var'][p] = float(np.asarray(rt.var).reshape(-1)[0])
                v['ret_count'][p] = float(rt.count)
            if oj is not None:  # obj_rms may still be scalar-shaped (vec_normalize.py:21)
                v['obj_mean'][p] = np.broadcast_to(np.asarray(oj.mean, np.float64), (K,))
                v['obj_var'][p] = np.broadcast_to(np.asarray(oj.var, np.float64), (K,))
                v['obj_count'][p] = float(oj.count)
        tb.load_stats64(flat)
        tb.adam_step.copy_(torch.tensor([s.snapshot.adam_step for s in samples], dtype=torch.int32))

    def load_task(self, tb, p, sample, weights):
        """One slot (tests / tools); the generation loop uses load_tasks."""
        snap = sample.snapshot
        tb.params[p].copy_(snap.params)
        tb.adam_m[p].copy_(snap.adam_m)
        tb.adam_v[p].copy_(snap.adam_v)
        tb.adam_step[p] = snap.adam_step
        tb.weights[p].copy_(torch.as_tensor(np.asarray(weights, dtype=np.float64)))
        ep = sample.env_params or {}
        tb.set_env_params(p, {k: v for k, v in ep.items() if v is not None})

    def _env_params(self, st, p, O, K):
        """Slot p of a host stats64 record (TaskBatch.stat_views) -> env_params RunningMeanStd copies."""
        ep = {'ob_rms': None, 'ret_rms': None, 'obj_rms': None}
        if self.args.ob_rms:
            r = RunningMeanStd(shape=(O,))
            r.mean, r.var, r.count = st['ob_mean'][p].copy(), st['ob_var'][p].copy(), float(st['ob_count'][p])
            ep['ob_rms'] = r
        r = RunningMeanStd(shape=())
        r.mean, r.var, r.count = np.float64(st['ret_mean'][p]), np.float64(st['ret_var'][p]), float(st['ret_count'][p])
        ep['ret_rms'] = r
        if self.args.obj_rms:
            r = RunningMeanStd(shape=())
            r.mean, r.var, r.count = st['obj_mean'][p].copy(), st['obj_var'][p].copy(), float(st['obj_count'][p])
            ep['obj_rms'] = r
        return ep

    def place(self, samples, dsts):
        """Collective (every rank, same arguments): move each sample's snapshot to rank dsts[k] when it lives
        elsewhere (shard.move_rows).  A no-op in one process."""
        rank, ws = world()
        if ws == 1:
            return 0
        snaps = [s.snapshot for s in samples]
        moves = [(sn.owner if sn.owner is not None else -1, d) for sn, d in zip(snaps, dsts)]
        local = {k: snaps[k].stacked() for k, (src, _) in enumerate(moves) if src == rank}
        L = self.layout.total
        got, nbytes = move_rows(moves, local, (3, L), torch.float32, self.device)
        for k, rows in got.items():  # owner metadata stays as it is on every rank (identical move lists)
            snaps[k].adopt(rows)
        self.moved_bytes += nbytes
        return nbytes

    def materialize(self, samples, dst=0):
        """Collective: gather the snapshots of ``samples`` onto rank ``dst`` (final/EP_policy_*.pt)."""
        return self.place(samples, [dst] * len(samples))

    def check_generation(self, tb, step_mismatch=None):
        """Collective (every rank, also one without tasks): PGMError on EVERY rank when any rank's update timed
        out in a cross-workgroup exchange this generation, and RuntimeError on every rank when any rank's Adam
        step counts are not the expected ones (``step_mismatch``: that rank's message), before anyone enters the
        record all-gather (a rank raising alone would leave the others blocked in that collective)."""
        from ._lib import PGMError
        from .runtime import UPDATE_TIMEOUT_MSG
        from .shard import allreduce_max
        failed = bool(tb.take_update_failed()) if tb is not None else False
        rank, ws = world()
        any_failed, any_mismatch = (allreduce_max([float(failed), float(step_mismatch is not None)], self.device)
                                    if ws > 1 else (float(failed), float(step_mismatch is not None)))
        if any_failed:
            raise PGMError(UPDATE_TIMEOUT_MSG + ('' if failed else ' (on another rank)'))
        if any_mismatch:
            raise RuntimeError(step_mismatch or 'Adam step counts differ from the expected ones on another rank')

    @staticmethod
    def update_fits(args, P, device='cuda'):
        """Host-only probe: does pgm_ppo_update accept P tasks of these args' dims on this device
        (pgm_ppo_update_variant: the launcher's own rule; the LayerNorm and wide kernels need 2P <= CUs)."""
        import ctypes as C

        from ._lib import PGM_OK, Dims, PPOHParams, launch_opts, lib
        from .envspec import make_spec
        sp = make_spec(args.env_name)
        dev = torch.device(device)
        if dev.type == 'cuda':
            torch.cuda.set_device(dev if dev.index is not None else torch.cuda.current_device())
        d = Dims(P, args.num_processes, args.num_steps, sp['obs_dim'], sp['act_dim'], sp['obj_num'], 64,
                 int(bool(getattr(args, 'layernorm', False))))
        hp = PPOHParams(clip_param=args.clip_param, value_loss_coef=args.value_loss_coef,
                        entropy_coef=args.entropy_coef, max_grad_norm=args.max_grad_norm, adam_eps=1e-5, beta1=0.9,
                        beta2=0.999, ppo_epoch=args.ppo_epoch, num_mini_batch=args.num_mini_batch,
                        use_clipped_value_loss=1)
        buf = C.create_string_buffer(128)
        if lib().pgm_ppo_update_variant(C.byref(d), C.byref(hp), C.byref(launch_opts()), buf, 128) != PGM_OK:
            return False
        # pgm_ppo_update_variant names a kernel for any P; the launch itself refuses beyond the limit below
        cus = torch.cuda.get_device_properties(dev).multi_processor_count if dev.type == 'cuda' else 0
        return cus == 0 or P <= MOPGPopulation.update_task_limit(bool(d.LN), d.O, cus)

    # The launcher's limit on P, restated (tests/test_sweep.py ties it to the text of include/pgm_abi.h and to the
    # launchers' own refusals): the one-workgroup-per-tower updates need UPDATE_WORKGROUPS_PER_TASK * P <= CUs
    UPDATE_WORKGROUPS_PER_TASK = 2
    UPDATE_RESIDENT_MAX_OBS = 32  # obs_dim above it: layer 1 streamed from L2, the wide update

    @staticmethod
    def update_task_limit(layernorm, obs_dim, cus):
        """Most tasks pgm_ppo_update accepts on a device of `cus` CUs (inf: no limit, the LDS-resident plain-tower
        updates fall back to one workgroup per task as P grows)."""
        if layernorm or obs_dim > MOPGPopulation.UPDATE_RESIDENT_MAX_OBS:
            return cus // MOPGPopulation.UPDATE_WORKGROUPS_PER_TASK
        return float('inf')

    def _set_runs(self, tb, run_of_task, n):
        """run_of_task of the n tasks just loaded (a runtime built with run_seeds; refused otherwise)."""
        from ._lib import PGMError
        if self.run_seeds is None:
            if run_of_task is not None:
                raise PGMError('run_of_task=... needs a runtime built with run_seeds=...')
            return
        if run_of_task is None:
            raise PGMError(f'this runtime holds {len(self.run_seeds)} runs (run_seeds=...): run_of_task is required')
        if len(run_of_task) != n:
            raise PGMError(f'run_of_task has {len(run_of_task)} ids for {n} tasks')
        tb.set_runs(run_of_task)

    def run_lr(self, r, j, total):
        """Run r's learning rate of iteration j: the host expression of a solo run with that run's lr and
        lr_decay_ratio, in Python floats (the fp32 rounding happens once, at the upload)."""
        a, h = self.args, self.run_hparams[r]
        lr0, ratio = float(h.get('lr', a.lr)), float(h.get('lr_decay_ratio', a.lr_decay_ratio))
        return linear_lr(j, total, lr0, ratio) if a.use_linear_lr_decay else lr0

    def task_lr(self, run_of_task, j, total):
        """[P] fp32: every task's learning rate of iteration j (run_lr of its run, rounded to fp32)."""
        per_run = [self.run_lr(r, j, total) for r in range(len(self.run_hparams))]
        return np.asarray([per_run[r] for r in run_of_task], dtype=np.float64).astype(np.float32)

    def task_hparams(self, run_of_task):
        """{field: [P] list} of RUN_TASK_FIELDS: every task's settings, its run's dict over ``args``."""
        a = self.args
        return {k: [float(self.run_hparams[r].get(k, getattr(a, k))) for r in run_of_task] for k in RUN_TASK_FIELDS}

    def run(self, task_batch, iteration, num_updates, start_time=None, log=print, run_of_task=None):
        """Every task's MOPG iterations [iteration, iteration + num_updates) -> all_offspring_batch.
        run_of_task (with run_seeds): the run index of every task, whose reset tables it uses.

        Per iteration the device state of all local tasks is snapshotted by ONE copy into this generation's
        arena ([I][3][Pl][L]) and the running statistics by ONE copy of the stats64 region; the offspring
        Samples are index handles into the arena (no per-offspring copies) with env_params unpacked on demand.

        Multi-GPU (torch.distributed initialised, one process per GPU): this rank runs its contiguous
        block of tasks (shard.task_block).  Elites whose snapshot lives on another rank are moved first
        (place); at the end of the generation only the fp64 records (objectives + running statistics) are
        all-gathered, and each offspring's parameters / Adam state stay on the rank that produced them
        (remote handles elsewhere) until a later generation or the final writer needs them."""
        a = self.args
        P = len(task_batch)
        rank, ws = world()
        lo, hi = task_block(P, rank, ws)
        Pl = hi - lo
        if ws > 1:
            self.place([t.sample for t in task_batch], [owner_of(p, P, ws) for p in range(P)])
        total = int(a.num_env_steps) // a.num_steps // a.num_processes
        its = list(range(iteration, min(iteration + num_updates, total)))
        I = len(its)
        start_time = time.time() if start_time is None else start_time
        layout = self.layout
        L = layout.total
        tb = None
        if Pl > 0:
            tb = self._batch(Pl)
            self.load_tasks(tb, [t.sample for t in task_batch[lo:hi]],
                            [t.scalarization.weights.numpy() for t in task_batch[lo:hi]])
            step0 = [t.sample.snapshot.adam_step for t in task_batch[lo:hi]]
            self._set_runs(tb, run_of_task, Pl)
            if self.run_hparams is not None:
                tb.set_task_hparams(**self.task_hparams(run_of_task))
            tb.env_reset()  # envs are re-created and reset every generation (mopg.py:67-82)
            arena = torch.empty(I, 3, Pl, L, dtype=torch.float32, device=self.device)
            store = RowStore(arena, 'arena')
            rec = torch.empty(I, tb._stats64.numel(), dtype=torch.float64, device=self.device)
            objs_ar = torch.empty(I, Pl, tb.K, dtype=torch.float64, device=self.device)  # written by the evals
            for i, j in enumerate(its):
                lr = linear_lr(j, total, a.lr, a.lr_decay_ratio) if a.use_linear_lr_decay else a.lr
                if self.run_hparams is not None:
                    lr = self.task_lr(run_of_task, j, total)
                noise = perms = None
                if self.rng == 'host' and tb.discrete:
                    noise, perms = host_draws_discrete(j, a.num_steps, a.num_processes, a.ppo_epoch)
                elif self.rng == 'host':
                    noise, perms = host_draws(j, a.num_steps, a.num_processes, tb.A, a.ppo_epoch)
                tb.iteration(j, lr, noise=noise, perms=perms, carry=i > 0, overlap_eval=True, objs_out=objs_ar[i])
                arena[i].copy_(tb.state)
                tb.stats64_record(rec[i])
                if rank == 0 and a.rl_log_interval > 0 and (j + 1) % a.rl_log_interval == 0:
                    steps = (j + 1) * a.num_processes * a.num_steps
                    dt = time.time() - start_time
                    # (a sweep: one log per run, each with the line its solo run prints -- its own task count)
                    outs = ([(log, P)] if callable(log) else
                            [(lg, int(np.sum(np.asarray(run_of_task) == r))) for r, lg in enumerate(log)])
                    for lg, n in outs:
                        lg(f'[RL] Updates {j + 1}, num timesteps {steps}, FPS {int(steps / max(dt, 1e-9))}, '
                           f'time {dt:.2f} seconds (x{n} tasks on {ws} device(s))')
            tb.wait_eval()
            if os.environ.get('PGM_DEBUG_TASKS'):
                print(f'[debug] generation at iteration {iteration}: P={P} local={Pl} iters={I} '
                      f'failed={int(tb.update_failed.item())}', flush=True)
        mismatch = None
        B = a.num_steps * a.num_processes
        per_iter = a.ppo_epoch * (B // (B // a.num_mini_batch))  # Adam steps of one iteration
        if tb is not None:
            got = tb.adam_step.cpu().numpy()
            want = np.asarray(step0) + I * per_iter
            if not np.array_equal(got, want):
                mismatch = f'rank {rank}: Adam step counts {got} != expected {want}'
        # a timed-out exchange or a lost Adam step never becomes an offspring (raised on every rank together)
        self.check_generation(tb, mismatch)
        probe = tb if tb is not None else None
        O, K = (probe.O, probe.K) if probe is not None else (layout.O, layout.K)
        if tb is not None:
            host_rec = rec.cpu().numpy()
            host_objs = objs_ar.cpu().numpy()
            stv = [tb.stat_views(host_rec[i], Pl) for i in range(I)]
        if ws > 1:  # generation boundary: objective + statistics records only (a few KB)
            width = K + 2 * O + 3 + 2 * K + 1
            mine = np.zeros((Pl, I, width))
            for i in range(I if Pl else 0):
                st = stv[i]
                mine[:, i] = np.concatenate([host_objs[i], st['ob_mean'], st['ob_var'], st['ob_count'][:, None],
                                             st['ret_mean'][:, None], st['ret_var'][:, None], st['ret_count'][:, None],
                                             st['obj_mean'], st['obj_var'], st['obj_count'][:, None]], 1)
            allr = allgather_rows(torch.from_numpy(mine).to(self.device), P).cpu().numpy()
            steps_all = allgather_rows(torch.tensor(step0 if Pl else [], dtype=torch.float64,
                                                    device=self.device).reshape(Pl), P).cpu().numpy()
        offspring = [[] for _ in range(P)]
        for p in range(P):
            own = owner_of(p, P, ws)
            q = p - lo
            for i in range(I):
                if ws == 1 or own == rank:
                    step = step0[q] + (i + 1) * per_iter
                    snap = DeviceSnapshot.in_arena(layout, store, i, q, step, owner=rank if ws > 1 else None)
                    objs = host_objs[i, q].copy()
                    fn = (lambda st=stv[i], q=q: self._env_params(st, q, O, K))
                else:
                    step = int(steps_all[p]) + (i + 1) * per_iter
                    snap = DeviceSnapshot.remote(layout, step, own)
                    r = allr[p, i]
                    objs = r[:K].copy()
                    st = self._split_record(r, O, K)
                    fn = (lambda st=st: self._env_params(st, 0, O, K))
                offspring[p].append(Sample.lazy(snap, fn, objs))
        return offspring

    @staticmethod
    def _split_record(r, O, K):
        """One all-gathered record row (objs, ob_mean/var, ob_count, ret mean/var/count, obj mean/var/count) ->
        the stat_views shape with one slot."""
        o = K
        out = {}
        for name, w in (('ob_mean', O), ('ob_var', O), ('ob_count', 1), ('ret_mean', 1), ('ret_var', 1),
                        ('ret_count', 1), ('obj_mean', K), ('obj_var', K), ('obj_count', 1)):
            v = r[o:o + w]
            out[name] = v[None] if w > 1 or name.startswith(('ob_m', 'ob_v', 'obj_m', 'obj_v')) else v
            o += w
        return out

    def evaluate_samples(self, samples, weights_batch, run_of_task=None):
        """Objectives of fresh samples (warm-up evaluation, morl/warm_up.py:69); run_of_task as in run()."""
        tb = self._batch(len(samples))
        self.load_tasks(tb, samples, weights_batch)
        self._set_runs(tb, run_of_task, len(samples))
        return tb.evaluate().cpu().numpy().copy()
