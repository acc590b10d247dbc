"""Register use of the plug-in kernels per env header, without a device: pgm_envplug.hip cross-compiled with build.py's
flags plus -Rpass-analysis=kernel-resource-usage, and the remarks of rollout_env_kernel / eval_env_kernel collected.

    python scripts/envplug2_resources.py [--parent-tree DIR] [--out FILE.json]

``--parent-tree``: a checkout of the parent commit (its include/ and pgmorl_amd/csrc/ are read).  The four contract-1
headers of tests/envplug are then compiled against both trees and the remarks must be equal: a header that does not
ask for contract 2 compiles into the kernels it compiled into before (asserted).  The contract-2 headers of
tests/envplug2 are compiled against this tree; none may use scratch memory (asserted).  DESIGN.md 28 tables the output.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pgmorl_amd import build  # noqa: E402

OLD = ['line', 'chain', 'plugdummy', 'wide']
NEW = ['slip', 'gather', 'parmax', 'noisemax', 'line2', 'plugdummy2']
KEYS = ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'SGPRs Spill',
        'VGPRs Spill')


def usage(tree, header):
    inc = os.path.join(ROOT, 'include')
    flags = [os.path.join(tree, 'include') if f == inc else f for f in build.FLAGS]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build._hipcc(), *flags, '-I', os.path.dirname(header), '-include', header, '-shared',
               '-Rpass-analysis=kernel-resource-usage', os.path.join(tree, 'pgmorl_amd', 'csrc', build.ENV_SOURCE),
               '-o', os.path.join(tmp, 'lib.so')]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-3000:])
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r'Function Name: (\S+)', ln)
        if m:
            cur = next((k for k in ('rollout_env_kernel', 'eval_env_kernel') if k in m.group(1)), None)
            if cur:
                out[cur] = {}
            continue
        m = re.search(r'remark:\s+(.+?): (\d+) \[', ln)
        if m and cur and m.group(1) in KEYS:
            out[cur][m.group(1)] = int(m.group(2))
    assert set(out) == {'rollout_env_kernel', 'eval_env_kernel'}, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {}
    for name in OLD:
        h = os.path.join(ROOT, 'tests', 'envplug', name + '.hpp')
        res[name] = {'branch': usage(ROOT, h)}
        if a.parent_tree:
            res[name]['parent'] = usage(a.parent_tree, h)
            assert res[name]['parent'] == res[name]['branch'], (name, res[name])
    for name in NEW:
        res[name] = {'branch': usage(ROOT, os.path.join(ROOT, 'tests', 'envplug2', name + '.hpp'))}
        for k, u in res[name]['branch'].items():
            assert u['ScratchSize [bytes/lane]'] == 0 and u['VGPRs Spill'] == 0, (name, k, u)
    print('header side kernel ' + ' '.join(KEYS))
    for name, r in res.items():
        for side, u in r.items():
            for k, v in u.items():
                print(name, side, k, *(v[x] for x in KEYS))
    if a.out:
        with open(a.out, 'w') as fp:
            json.dump(res, fp, indent=1)


if __name__ == '__main__':
    main()
