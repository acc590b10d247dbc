"""Entry point with the reference's flags and defaults (morl/run.py:52-93, morl/arguments.py:3-173).

    python -m pgmorl_amd.run --env-name MO-Walker2d-v2 --num-env-steps 5000000 ... [--selection-method ra]

Adds ``--rng {device,host}`` (device counter streams, or the reference's own torch draws for
bit-compatible runs), ``--device``, ``--host-env SPEC`` (environments stepped on the host, hostenv.py) and
``--device-env`` (a discrete-action env, Deep Sea Treasure, stepped on the device instead) and ``--env-plugin HEADER``
(a user env stated as a C++ header, include/pgm_envplug.h, compiled into fused rollout and evaluation kernels), with
``--env-param NAME=VALUE`` for the runtime parameters of a header under contract 2.
"""
import argparse
import os
import sys

import torch

DEFAULTS = ['--lr', '3e-4', '--use-linear-lr-decay', '--gamma', '0.995', '--use-gae', '--gae-lambda', '0.95',
            '--entropy-coef', '0', '--value-loss-coef', '0.5', '--num-steps', '2048', '--num-processes', '4',
            '--ppo-epoch', '10', '--num-mini-batch', '32', '--use-proper-time-limits', '--ob-rms', '--obj-rms',
            '--raw']


def get_parser():
    ap = argparse.ArgumentParser(description='PG-MORL on MI355X')
    add = ap.add_argument
    add('--env-name', default='MO-HalfCheetah-v2')
    add('--obj-num', type=int, default=2)
    add('--num-env-steps', type=int, default=5e6)
    add('--num-tasks', type=int, default=6)
    add('--seed', type=int, default=0)
    add('--min-weight', type=float, default=0.0)
    add('--max-weight', type=float, default=1.0)
    add('--delta-weight', type=float, default=0.2)
    add('--warmup-iter', type=int, default=80)
    add('--update-iter', type=int, default=20)
    add('--eval-num', type=int, default=1)
    add('--selection-method', type=str, default='prediction-guided')
    add('--pbuffer-num', type=int, default=100)
    add('--pbuffer-size', type=int, default=2)
    add('--num-weight-candidates', type=int, default=7)
    add('--sparsity', type=float, default=1.0)
    add('--obj-rms', default=False, action='store_true')
    add('--ob-rms', default=False, action='store_true')
    add('--raw', default=False, action='store_true')
    add('--rl-log-interval', type=int, default=10)
    add('--save-dir', default='./trained_models/')
    add('--algo', default='ppo')
    add('--lr', type=float, default=3e-4)
    add('--use-linear-lr-decay', action='store_true', default=False)
    add('--lr-decay-ratio', type=float, default=1.0)
    add('--gamma', type=float, default=0.995)
    add('--use-gae', action='store_true', default=False)
    add('--gae-lambda', type=float, default=0.95)
    add('--entropy-coef', type=float, default=0.0)
    add('--value-loss-coef', type=float, default=0.5)
    add('--max-grad-norm', type=float, default=0.5)
    add('--num-steps', type=int, default=2048)
    add('--num-processes', type=int, default=4)
    add('--ppo-epoch', type=int, default=10)
    add('--num-mini-batch', type=int, default=32)
    add('--clip-param', type=float, default=0.2)
    add('--use-proper-time-limits', action='store_true', default=False)
    add('--layernorm', action='store_true', default=False)
    add('--rng', choices=['device', 'host'], default='device')
    add('--device', default='cuda')
    add('--host-env', default=None, metavar='SPEC',
        help='step the environments on the host (policy, VecNormalize, storage and PPO stay on the device): '
             '"synth" (SynthMO in numpy), "dummy" (the MO-Dummy envs, which otherwise run on the device) or '
             '"module:callable" with callable(env_name, seed, rank) -> a gym-style '
             'multi-objective env; default: the device envs')
    add('--device-env', action='store_true', default=False,
        help='run a discrete-action env on the device (MO-DeepSeaTreasure-v0: the fused Categorical rollout and '
             'evaluation) instead of --host-env; no effect on the SynthMO envs, which are device envs already')
    add('--env-plugin', default=None, metavar='HEADER',
        help='train on a user env stated as one C++ header (include/pgm_envplug.h): the header is compiled into a '
             'fused rollout and evaluation kernel of its own; --env-name is then any name envspec does not know.  '
             'With "--host-env plugin" the same compiled header is stepped on the host instead')
    add('--env-param', action='append', default=None, metavar='NAME=VALUE',
        help='set one runtime parameter of a CONTRACT = 2 --env-plugin header (one of its PAR_NAMES; the others keep '
             'the header\'s defaults); repeatable')
    return ap


def merge_argv(argv):
    """Command-line flags override the defaults (morl/run.py:29-50)."""
    defaults = list(DEFAULTS)
    for a in argv:
        if a.startswith('-') and a in defaults:
            i = defaults.index(a)
            j = i + 1
            while j < len(defaults) and not defaults[j].startswith('-'):
                j += 1
            del defaults[i:j]
    return defaults + list(argv)


class _Tee:
    def __init__(self, stream, f):
        self.stream, self.f = stream, f

    def write(self, d):
        self.stream.write(d)
        self.stream.flush()
        self.f.write(d)

    def flush(self):
        pass


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    torch.set_default_dtype(torch.float64)
    args = get_parser().parse_args(merge_argv(argv))
    if args.env_param and args.env_plugin is None:  # refused here, before the save dir or the device is touched
        from ._lib import PGMError
        raise PGMError('--env-param sets a runtime parameter of an env plug-in: it needs --env-plugin HEADER')
    if args.env_plugin is not None or args.host_env == 'plugin':
        # every refusal of a plug-in run, before the save dir or the device is touched; then the env name is registered
        # with the header's dims and the loaded library travels in args.env_plugin
        from ._lib import PGMError
        if args.env_plugin is None:
            raise PGMError('--host-env plugin steps the header of --env-plugin HEADER on the host: pass --env-plugin')
        if args.layernorm:
            raise PGMError('--layernorm with --env-plugin: env plug-ins are built for plain towers only')
        if args.device_env:
            raise PGMError('--device-env with --env-plugin: the plug-in\'s fused kernels already step the env on the '
                           'device; --device-env selects the built-in Deep Sea Treasure')
        if args.host_env not in (None, 'plugin'):
            raise PGMError(f'--host-env {args.host_env} with --env-plugin: the one host env of a plug-in run is '
                           f'"--host-env plugin" (the same header stepped on the host)')
        from .envplug import EnvPlugin
        plugin = EnvPlugin(args.env_plugin)  # PGMError with the compiler's message when the header does not build
        try:
            plugin.register(args.env_name)
        except ValueError as e:
            raise PGMError(f'--env-plugin with --env-name {args.env_name}: {e}') from e
        env_params = {}
        for item in args.env_param or ():
            name, sep, value = str(item).partition('=')
            if not sep or not name or not value:
                raise PGMError(f'--env-param {item!r}: expected NAME=VALUE')
            env_params[name] = value
        plugin.par_vector(env_params)  # PGMError for an unknown name, a value that is no number, a header without any
        args.env_params = {k: float(v) for k, v in env_params.items()}
        args.env_plugin = plugin
    elif args.host_env is not None and ':' in str(args.host_env):
        # an env name envspec does not know behind --host-env module:callable: a third-party env, registered with the
        # dims of one probe env (the runtime-dim kernels); dims out of their range and --layernorm are refused here
        from ._lib import PGMError
        from . import envspec
        from .hostenv import register_from_spec
        try:
            register_from_spec(args.host_env, args.env_name, args.seed)
        except ValueError as e:
            raise PGMError(str(e)) from e
        if args.env_name in envspec.user_env_names():
            if args.layernorm:
                raise PGMError(f'--layernorm with {args.env_name}: a third-party env runs on the runtime-dim kernels, '
                               f'which are built for plain towers only')
            if args.device_env:
                raise PGMError(f'--device-env with {args.env_name}: a third-party env is host-stepped only')
    if args.layernorm:  # refused here, before the save dir or the device is touched
        from ._lib import PGMError
        from .envspec import make_spec
        from .runtime import LN_MAX_OBS
        obs_dim = make_spec(args.env_name)['obs_dim']
        if obs_dim > LN_MAX_OBS:
            raise PGMError(f'--layernorm with {args.env_name}: the LayerNorm kernels keep layer 1 LDS-resident and '
                           f'are built for obs_dim <= {LN_MAX_OBS}; obs_dim {obs_dim} would need a streamed layer-1 '
                           f'LayerNorm kernel, which does not exist')
    from .envspec import discrete_env_names
    if args.device_env and args.host_env is not None:  # refused here too: two places to step the same env
        from ._lib import PGMError
        raise PGMError('--device-env together with --host-env: the environments run on the device or on the host, '
                       'pass one of the two')
    if args.env_name in discrete_env_names():  # refused here too: where the env runs is chosen, no LayerNorm kernel
        from ._lib import PGMError
        if args.host_env is None and not args.device_env:
            raise PGMError(f'{args.env_name} has discrete actions and no default environment: pass --host-env (dst: '
                           f'the built-in Deep Sea Treasure on the host, or module:callable) or --device-env (Deep '
                           f'Sea Treasure inside the fused rollout kernel)')
        if args.layernorm:
            raise PGMError(f'--layernorm with {args.env_name}: LayerNorm towers with a Categorical head are not built')
    if args.host_env is not None and args.host_env != 'plugin':  # refused here too: a spec that cannot be imported
        # or whose env dims differ
        from ._lib import PGMError
        from .hostenv import check_spec
        try:
            check_spec(args.host_env, args.env_name, args.seed)
        except ValueError as e:
            raise PGMError(str(e)) from e
    os.makedirs(args.save_dir, exist_ok=True)
    with open(os.path.join(args.save_dir, 'args.txt'), 'w') as fp:
        fp.write(str(merge_argv(argv)))
    from .morl import run
    with open(os.path.join(args.save_dir, 'log.txt'), 'w') as logf:
        tee = _Tee(sys.stdout, logf)
        run(args, device=args.device, rng=args.rng, log=lambda *m: tee.write(' '.join(str(x) for x in m) + '\n'))


if __name__ == '__main__':
    main()
