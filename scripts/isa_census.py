#!/usr/bin/env python
"""Static instruction census of one kernel instantiation (CPU only: needs hipcc, no GPU).

Compiles one .hip of pgmorl_amd/csrc device-only to assembly with the flags of pgmorl_amd/build.py, finds the named
template instantiation, and prints (and writes as JSON) its resource usage -- SGPRs, VGPRs, AGPRs, scratch, occupancy
-- and a count of the instructions of its step loop by class.  The step loop is the outermost back-edge region (a
label and a later branch back to it) that contains MFMAs, overlapping regions (one loop with several back edges)
taken as one; a kernel that selects one of several loops up front (one per tower) has several, each counted on its
own.  Classes are decided by mnemonic prefix alone.  This is a counter: it asserts nothing about the code.

    python scripts/isa_census.py pgm_ppo_fs.hip ppo_update_fs_kernel 17,6,2,6,3 [more arg lists ...] --out FILE.json
    python scripts/isa_census.py --asm FILE.s pgm_ppo_fs.hip ppo_update_fs_kernel 17,6,2,6,3   (assembly made earlier)

A count is static: an instruction under a branch inside the loop counts once whether or not a step executes it.
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

CLASSES = ['mfma', 'lane_moves', 'f32_math', 'packed_f32', 'fp64', 'integer_address', 'compare_select', 'moves',
           'lds', 'buffer_global_memory', 'scalar_alu', 'branches', 'waits_barriers', 'other']
VALU_NON_MFMA = ['lane_moves', 'f32_math', 'packed_f32', 'fp64', 'integer_address', 'compare_select', 'moves']


def classify(mn):
    """Instruction class of a mnemonic, by prefix / suffix only."""
    if mn.startswith(('v_mfma', 'v_smfmac')):
        return 'mfma'
    if mn.startswith(('v_readlane', 'v_writelane', 'v_readfirstlane')):
        return 'lane_moves'
    if mn.startswith('v_'):
        if '_f64' in mn:
            return 'fp64'
        if mn.startswith(('v_cmp', 'v_cndmask')):
            return 'compare_select'
        if mn.startswith('v_pk_') and '_f32' in mn:
            return 'packed_f32'
        if mn.startswith(('v_mov', 'v_accvgpr', 'v_swap')):
            return 'moves'
        if '_f32' in mn or '_f16' in mn:
            return 'f32_math'
        return 'integer_address'
    if mn.startswith('ds_'):
        return 'lds'
    if mn.startswith(('buffer_', 'global_', 'flat_', 'scratch_', 's_load_', 's_buffer_load_')):
        return 'buffer_global_memory'
    if mn.startswith(('s_branch', 's_cbranch', 's_setpc', 's_swappc', 's_call', 's_endpgm')):
        return 'branches'
    if mn.startswith(('s_waitcnt', 's_barrier', 's_nop', 's_sleep')):
        return 'waits_barriers'
    if mn.startswith('s_'):
        return 'scalar_alu'
    return 'other'


def compile_flags():
    from pgmorl_amd import build as b
    return [f for f in b.FLAGS if f != '-fPIC'] + ['--cuda-device-only', '-S']


def shown_flags():
    return ' '.join(os.path.relpath(f, ROOT) if f.startswith(ROOT) else f for f in compile_flags())


def compile_asm(src, out):
    from pgmorl_amd import build as b
    path = src if os.path.isabs(src) or os.path.exists(src) else os.path.join(b.CSRC, src)
    r = subprocess.run([b._hipcc(), *compile_flags(), path, '-o', out], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f'hipcc failed:\n{r.stdout}\n{r.stderr}')


_LABEL = re.compile(r'^([A-Za-z_.$][\w.$]*):')
_INSN = re.compile(r'^\s+([a-z][a-z0-9_]*)\b(.*)$')
_TARGET = re.compile(r'(\.LBB[\w.]*)')


def kernel_body(lines, name, targs):
    """(symbol, lines of the function, trailing resource comments) of the instantiation name<targs...>."""
    key = f'{len(name)}{name}I' + ''.join(f'Li{a}E' for a in targs) + 'E'
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if m and key in m.group(1) and not m.group(1).endswith('.kd'):
            sym = m.group(1)
            for j in range(i + 1, len(lines)):
                if lines[j].startswith('.Lfunc_end'):
                    tail = []
                    for k in range(j, min(j + 80, len(lines))):
                        if k > j and _LABEL.match(lines[k]):
                            break
                        tail.append(lines[k])
                    return sym, lines[i + 1:j], tail
    raise SystemExit(f'no instantiation {name}<{",".join(map(str, targs))}> in the assembly')


def resources(tail):
    out = {}
    for key, pat in (('sgprs', r';\s*(?:Total)?NumSgprs:\s*(\d+)'), ('vgprs', r';\s*NumVgprs:\s*(\d+)'),
                     ('agprs', r';\s*NumAgprs:\s*(\d+)'), ('total_vgprs', r';\s*TotalNumVgprs:\s*(\d+)'),
                     ('scratch_bytes', r';\s*ScratchSize:\s*(\d+)'), ('occupancy', r';\s*Occupancy:\s*(\d+)'),
                     ('code_bytes', r';\s*codeLenInByte\s*=\s*(\d+)')):
        for ln in tail:
            m = re.search(pat, ln)
            if m:
                out[key] = int(m.group(1))
                break
    return out


def census(body):
    """Counts by class over the whole function and over each outermost MFMA-holding back-edge region."""
    insns, labels = [], {}
    for ln in body:
        m = _LABEL.match(ln)
        if m:
            labels[m.group(1)] = len(insns)
            continue
        m = _INSN.match(ln)
        if m and not ln.lstrip().startswith(('.', ';')):
            insns.append((m.group(1), m.group(2)))
    regions = []
    for i, (mn, rest) in enumerate(insns):
        if classify(mn) == 'branches':
            t = _TARGET.search(rest)
            if t and t.group(1) in labels and labels[t.group(1)] <= i:
                regions.append((labels[t.group(1)], i))
    holds = [r for r in regions if any(classify(insns[k][0]) == 'mfma' for k in range(r[0], r[1] + 1))]
    # a loop with several back edges (to different headers) gives overlapping regions: their union is one loop
    outer = []
    for lo, hi in sorted(holds):
        if outer and lo <= outer[-1][1]:
            outer[-1] = (outer[-1][0], max(outer[-1][1], hi))
        else:
            outer.append((lo, hi))

    def count(lo, hi):
        c = {k: 0 for k in CLASSES}
        for k in range(lo, hi + 1):
            c[classify(insns[k][0])] += 1
        c['total'] = hi - lo + 1
        c['valu_non_mfma'] = sum(c[k] for k in VALU_NON_MFMA)
        return c

    return {'function': dict(count(0, len(insns) - 1), labels=len(labels)),
            'step_loops': [count(lo, hi) for lo, hi in sorted(outer)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('source', help='a .hip of pgmorl_amd/csrc (or a path)')
    ap.add_argument('kernel', help='kernel template name, e.g. ppo_update_fs_kernel')
    ap.add_argument('targs', nargs='+', help='integer template arguments of an instantiation, e.g. 17,6,2,6,3')
    ap.add_argument('--asm', help='read this assembly file instead of compiling')
    ap.add_argument('--keep-asm', help='keep the compiled assembly here')
    ap.add_argument('--out', help='write the census as JSON here')
    a = ap.parse_args()
    if a.asm:
        asm = a.asm
    else:
        asm = a.keep_asm or os.path.join(tempfile.mkdtemp(prefix='isa_census_'), 'out.s')
        compile_asm(a.source, asm)
    with open(asm) as fp:
        lines = fp.read().splitlines()
    res = {'source': os.path.basename(a.source), 'kernel': a.kernel, 'flags': shown_flags(), 'instantiations': {}}
    for ta in a.targs:
        targs = [int(x) for x in ta.split(',')]
        sym, body, tail = kernel_body(lines, a.kernel, targs)
        ent = {'symbol': sym, 'resources': resources(tail), **census(body)}
        res['instantiations'][f'<{ta}>'] = ent
        print(f'{a.kernel}<{ta}>  {ent["resources"]}')
        cols = [('function', ent['function'])] + [(f'loop {i}', c) for i, c in enumerate(ent['step_loops'])]
        print(f'  {"class":<22}' + ''.join(f'{n:>10}' for n, _ in cols))
        for k in CLASSES + ['valu_non_mfma', 'total']:
            print(f'  {k:<22}' + ''.join(f'{c[k]:>10}' for _, c in cols))
    if a.out:
        with open(a.out, 'w') as fp:
            json.dump(res, fp, indent=1, sort_keys=True)
            fp.write('\n')


if __name__ == '__main__':
    main()
