"""Compare the device assembly of the kernels two trees have in common.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -I include --cuda-device-only -S pgmorl_amd/csrc/pgm_ppo_fs.hip \
        -o fs.s                                                                     (once per tree)
    python scripts/asm_twins.py PARENT_DIR BRANCH_DIR [--json OUT]

Each directory holds *.s files.  A kernel is its text from the entry label to its `.Lfunc_end` label plus its
`.amdhsa_kernel` descriptor block.  Kernels are matched by demangled name as scripts/resource_lines.py matches them:
the branch's trailing TASKS = false flag removed, the TASKS = true instantiations listed apart.  Two things are
normalised before the texts are compared, both consequences of the added template argument and of the added functions
and not of any instruction: the kernel's own mangled symbol (replaced by a placeholder), and the function ordinal inside
local labels (`.LBB12_3` -> `.LBB_3`), which counts the functions emitted before it; the assembler comments, which
repeat that ordinal (`Header=BB12_5`) and are padded to the label's length, are left out.  `.Lpost_getpc<n>` counts the
long branches of the file in the same way, and the directive that returns to the text section names a COMDAT section
for a template (gae_kernel became one).  The `__hip_cuid_` line is outside
every kernel's text.  Exit status 1 if a common kernel differs or a parent kernel is missing.
"""
import glob
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resource_lines import head_key, key  # noqa: E402


def kernels(d):
    """{mangled symbol: normalised text} of every kernel in the *.s files of d."""
    out = {}
    for f in sorted(glob.glob(os.path.join(d, '*.s'))):
        text = open(f).read()
        for m in re.finditer(r'^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel', text, re.M | re.S):
            sym, desc = m.group(1), m.group(2)
            b = re.search(r'^' + re.escape(sym) + r':.*?^\.Lfunc_end\d+:', text, re.M | re.S)
            if b is None:
                sys.exit(f'{f}: no body for {sym}')
            body = re.sub(r'\.L(BB|func_begin|func_end|tmp|post_getpc)\d+', r'.L\1', b.group(0))
            body = '\n'.join(ln.split(';')[0].rstrip() for ln in body.split('\n'))  # (comments name the ordinal too)
            text_k = (body + '\n' + desc).replace(sym, '<kernel>')
            # (gae_kernel became a template: its code moves from .text into a COMDAT section of its own)
            out[sym] = re.sub(r'^\t\.(text|section\t\.text\.<kernel>,.*)$', '\t<text section>', text_k, flags=re.M)
    return out


def demangled(syms):
    dem = subprocess.run(['c++filt'], input='\n'.join(syms), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(syms, dem))


def main():
    base, head = kernels(sys.argv[1]), kernels(sys.argv[2])
    bd, hd = demangled(list(base)), demangled(list(head))
    b = {key(bd[s], strip=False)[0]: t for s, t in base.items()}
    rows, changed, twins = [], 0, 0
    seen = set()
    for s, t in sorted(head.items(), key=lambda x: hd[x[0]]):
        k, tasks = head_key(hd[s], set(b))
        if tasks:
            twins += 1
            continue
        seen.add(k)
        if k not in b:
            rows.append({'kernel': k, 'status': 'new'})
            continue
        same = b[k] == t
        changed += not same
        rows.append({'kernel': k, 'status': 'same' if same else 'CHANGED', 'lines': t.count('\n')})
    missing = sorted(set(b) - seen)
    print(f'{len(rows)} kernels of the branch besides {twins} TASKS twins, {changed} with another text, '
          f'{len(missing)} parent kernels missing')
    for r in rows:
        if r['status'] != 'same':
            print(r['status'], r['kernel'])
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as f:
            json.dump({'changed': changed, 'missing': missing, 'twins': twins, 'kernels': rows}, f, indent=1)
    return 1 if changed or missing else 0


if __name__ == '__main__':
    sys.exit(main())
