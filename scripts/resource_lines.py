"""Compare the -Rpass-analysis=kernel-resource-usage lines of two builds of the same sources.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include -Rpass-analysis=kernel-resource-usage --cuda-device-only \
        -c pgmorl_amd/csrc/pgm_rollout_lanes.hip -o /dev/null 2> lanes.remarks      (once per tree)
    python scripts/resource_lines.py PARENT_DIR BRANCH_DIR [--json OUT]

Each directory holds *.remarks files.  Kernels are matched by demangled name with the template arguments this change
adds (the trailing RUNS flag and the argument-block type) removed; the RUNS = true instantiations are listed apart.
§25: pgm_policy_env.hip, pgm_rollout_lanes.hip, pgm_rollout_wide.hip.  §26 (the trailing flag is TASKS):
pgm_ppo_fs.hip, pgm_ppo_mfma.hip, pgm_ppo_wide.hip, pgm_ppo_update.hip, pgm_ppo_ln.hip, pgm_misc.hip, and
pgm_ppo_cat.hip and pgm_ppo_any.hip, which share headers with them and gain no flag.  The parent's names are taken as they are (a parent
kernel whose own last template argument is a bool keeps it).
"""
import glob
import json
import os
import re
import subprocess
import sys

FIELDS = ['TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'SGPRs Spill',
          'VGPRs Spill', 'LDS Size [bytes/block]']


def parse(d):
    out, cur = {}, None
    for f in sorted(glob.glob(os.path.join(d, '*.remarks'))):
        for line in open(f):
            m = re.search(r'remark: Function Name: (\S+)', line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = re.search(r'remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass', line)
            if m and cur is not None:
                cur[m.group(1).strip()] = m.group(2)
    names = list(out)
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return {d_: out[n] for n, d_ in zip(names, dem)}


def key(name, strip=True):
    """(kernel<args> without the trailing RUNS / TASKS flag, the flag); strip=False: the name as it is, False"""
    name = name.replace('(anonymous namespace)::', '').replace('void ', '')  # (before the cut at the argument list)
    name = re.sub(r'\(.*$', '', name)
    m = re.match(r'(.*), (true|false)>$', name) if strip else None
    if m:
        return m.group(1) + '>', m.group(2) == 'true'
    m = re.match(r'(.*)<(true|false)>$', name) if strip else None  # (a kernel whose one template argument is the flag)
    if m:
        return m.group(1), m.group(2) == 'true'
    return name, False


def head_key(name, base_names):
    """key() of a branch kernel; a name the parent has as it stands is that kernel (its last bool is its own)"""
    plain = key(name, strip=False)
    return plain if plain[0] in base_names else key(name)


def main():
    base, head = parse(sys.argv[1]), parse(sys.argv[2])
    base_names = {key(n, strip=False)[0] for n in base}
    def keyed(fns, full):
        """{key: lines}; two functions under one key would hide each other: refused"""
        out = {}
        for n, v in fns.items():
            k = head_key(n, base_names) if full else key(n, strip=False)[0]
            if k in out:
                sys.exit(f'two kernels share the key {k!r} (last: {n})')
            out[k] = v
        return out
    b, h = keyed(base, False), keyed(head, True)
    rows, changed = [], 0
    for (k, runs), v in sorted(h.items()):
        if runs:
            continue
        if k not in b:
            rows.append({'kernel': k, 'status': 'new', 'branch': v})
            continue
        same = all(b[k].get(f) == v.get(f) for f in FIELDS)
        changed += not same
        rows.append({'kernel': k, 'status': 'same' if same else 'CHANGED', 'parent': b[k], 'branch': v,
                     'runs': h.get((k, True))})
    missing = sorted(set(b) - {k for k, _ in h})
    print(f'{len(rows)} kernels of the branch, {changed} changed lines, {len(missing)} parent kernels missing')
    for r in rows:
        if r['status'] != 'same':
            print(r['status'], r['kernel'], r.get('parent'), r['branch'])
    for r in rows:
        rr = r.get('runs')
        if rr and any(rr.get(f) != r['branch'].get(f) for f in FIELDS):
            print('runs differs', r['kernel'], {f: (r['branch'].get(f), rr.get(f)) for f in FIELDS
                                              if rr.get(f) != r['branch'].get(f)})
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as f:
            json.dump({'fields': FIELDS, 'changed': changed, 'missing': missing, 'kernels': rows}, f, indent=1)
    return 1 if changed or missing else 0


if __name__ == '__main__':
    sys.exit(main())
