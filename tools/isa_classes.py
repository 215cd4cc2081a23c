"""Instruction classes of one kernel instantiation, from hipcc's gfx950 assembly.  Needs no GPU.

    python tools/isa_classes.py [--kernel 'points_kernel<1,2,false,1,512,2,false,true,1>'] [-DNAME=VALUE ...] [-fFLAG ...]
                                [--json OUT.json] [--against PARENT.json] [--keep-asm FILE.s]

Compiles a translation unit that holds nothing but the named instantiation (a kernel template of neuray_amd/csrc/nr_kernels.h in
namespace nr) with the flags of neuray_amd/build.py plus `--cuda-device-only -S` and counts the STATIC instructions of the kernel
by class: the table of DESIGN.md section 4.12.  The default instantiation is the AR_X3 point kernel with the per-view record: it has no
slot skipping, so its one tile body is the two-slot (NA = 2) body of the product kernel plus the predicated debug stores.

Classes (each instruction is counted once, in the first class that claims it):
    MFMA             v_mfma_*, by mnemonic
    operand split    v_cvt_pk_bf16_f32, v_dot2*_f32_bf16
    ELU              v_med3_f32, the v_exp_f32 whose result reaches a v_med3_f32 through at most two arithmetic instructions
                     (exp -> multiply-add -> median), and the v_pk_fma_f32 on that path
    lane-group sums  v_permlane16_swap / v_permlane32_swap and the v_mov_b32 whose result is next touched by one of them (the swaps
                     overwrite both operands, so a value that has to survive, or to be swapped with itself, is copied first)
    SGPR spills      v_readlane_b32 / v_writelane_b32
    transcendentals  v_exp_f32 outside ELU, v_rcp_f32, v_log_f32, v_sqrt_f32, v_rsq_f32, v_div_scale_f32
    selects          v_cmp*, v_cndmask_b32
    arithmetic       v_mul / v_add / v_sub / v_fma(c) _f32 and the packed forms
    hazard padding   s_nop (and the wait states they stand for)
--against prints a second column from a table saved with --json (the parent's) and the three ratios the lane-group work is judged by."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuray_amd import build as nbuild  # noqa: E402

DEFAULT_KERNEL = 'points_kernel<1,2,false,1,512,2,false,true,1>'


def assembly(kernel, defines=()):
    """-> the assembly text of a device-only compile of `nr::<kernel>` alone"""
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, 'one_kernel.hip'), os.path.join(tmp, 'one_kernel.s')
        with open(src, 'w') as f:
            f.write('#include "nr_kernels.h"\nconst void* isa_classes_ref() { return (const void*)nr::%s; }\n' % kernel)
        flags = [f for f in nbuild.FLAGS if f not in ('-shared', '-fPIC')]
        subprocess.check_call([nbuild.HIPCC] + flags + list(defines) + ['-I', nbuild.CSRC, '--cuda-device-only', '-S', src, '-o', out])
        return open(out).read()


def kernel_body(asm, kernel):
    """-> the instruction lines [(mnemonic, operand string)] of nr::<kernel> (the header's plain kernels are in the file as well)"""
    lines = asm.splitlines()
    want = 'voidnr::' + kernel.replace(' ', '') + '('
    starts = []
    for i, ln in enumerate(lines):
        m = re.match(r'^(_Z\w+):', ln)
        if m and subprocess.run(['c++filt', m.group(1)], capture_output=True, text=True).stdout.replace(' ', '').startswith(want):
            starts.append(i)
    if len(starts) != 1:
        raise SystemExit('expected one nr::%s in the assembly, found %d' % (kernel, len(starts)))
    out = []
    for ln in lines[starts[0] + 1:]:
        if ln.startswith('.Lfunc_end'):
            break
        m = re.match(r'^\s+([a-z][a-z0-9_]+)\s*(.*?)\s*(?:;.*)?$', ln)
        if m and not m.group(1).startswith('.'):
            out.append((m.group(1), m.group(2)))
    return out


def vgprs(operand):
    """the VGPR numbers an operand names: v7 -> {7}, v[4:5] -> {4, 5}"""
    m = re.match(r'^[-|]?v(\d+)\b', operand)
    if m:
        return {int(m.group(1))}
    m = re.match(r'^[-|]?v\[(\d+):(\d+)\]', operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def split_ops(ops):
    return [o.strip() for o in re.split(r',\s*(?![^\[]*\])', ops) if o.strip()]


def classify(body):
    n = len(body)
    parsed = []
    for mn, ops in body:
        o = split_ops(ops)
        dst = vgprs(o[0]) if o and mn.startswith('v_') and not mn.startswith('v_cmp') else set()
        srcs = set().union(*[vgprs(x) for x in o[1:]]) if len(o) > 1 else set()
        parsed.append((mn, dst, srcs, o))
    is_swap = lambda mn: mn.startswith('v_permlane16_swap') or mn.startswith('v_permlane32_swap')   # noqa: E731

    def reaches_med3(i, regs, hops, via):
        """does a value in `regs`, defined at i, reach a v_med3 through <= hops arithmetic instructions?  Linear scan, ends where the
        registers are overwritten; `via` collects the instructions on the path"""
        regs = set(regs)
        for j in range(i + 1, min(n, i + 600)):
            mn, dst, srcs, _ = parsed[j]
            if srcs & regs:
                if mn.startswith('v_med3_f32'):
                    return True
                if hops > 0 and re.match(r'v_(pk_)?(fma|add|sub|mul|fmac|fmaak|fmamk)_f32', mn) and reaches_med3(j, dst, hops - 1, via):
                    via.add(j)
                    return True
            regs -= dst
            if not regs:
                return False
        return False

    cls = [None] * n
    elu_path = set()
    for i, (mn, dst, srcs, o) in enumerate(parsed):
        if mn.startswith('v_exp_f32') and reaches_med3(i, dst, 2, elu_path):
            cls[i] = 'ELU v_exp'
    for i, (mn, dst, srcs, o) in enumerate(parsed):
        if cls[i]:
            continue
        if mn.startswith('v_mfma'):
            cls[i] = 'MFMA ' + re.sub(r'^v_mfma_f32_', '', mn)
        elif mn.startswith('v_cvt_pk_bf16_f32'):
            cls[i] = 'split v_cvt_pk_bf16'
        elif re.match(r'v_dot2c?_f32_bf16', mn):
            cls[i] = 'split v_dot2'
        elif mn.startswith('v_med3_f32'):
            cls[i] = 'ELU v_med3'
        elif i in elu_path and mn.startswith('v_pk_fma_f32'):
            cls[i] = 'ELU v_pk_fma'
        elif is_swap(mn):
            cls[i] = 'group ' + mn.split('_swap')[0] + '_swap'
        elif mn.startswith('v_mov_b32') and dst:
            nxt = next((parsed[j][0] for j in range(i + 1, n) if (parsed[j][1] | parsed[j][2]) & dst), '')
            cls[i] = 'group v_mov (feeds a swap)' if is_swap(nxt) else 'v_mov (other)'
        elif mn.startswith('v_readlane_b32'):
            cls[i] = 'spill v_readlane'
        elif mn.startswith('v_writelane_b32'):
            cls[i] = 'spill v_writelane'
        elif re.match(r'v_(exp|rcp|log|sqrt|rsq)_f32', mn):
            cls[i] = 'transc ' + mn.split('_f32')[0]
        elif mn.startswith('v_div_scale_f32'):
            cls[i] = 'transc v_div_scale'
        elif mn.startswith('v_cmp'):
            cls[i] = 'select v_cmp'
        elif mn.startswith('v_cndmask'):
            cls[i] = 'select v_cndmask'
        elif re.match(r'v_(pk_)?(mul|add|sub|fma|fmac|fmaak|fmamk)_f32', mn):
            cls[i] = 'arith ' + re.match(r'v_(pk_)?(mul|add|sub|fma)', mn).group(0)
        elif mn == 's_nop':
            cls[i] = 'pad s_nop'
        elif mn.startswith('v_'):
            cls[i] = 'other VALU'
        elif mn.startswith('s_'):
            cls[i] = 'SALU / control'
        elif re.match(r'(buffer|global|flat|scratch)_', mn):
            cls[i] = 'memory ' + mn.split('_')[0]
        elif mn.startswith('ds_'):
            cls[i] = 'memory ds'
        else:
            cls[i] = 'other'
    table = {}
    for c in cls:
        table[c] = table.get(c, 0) + 1
    table['pad wait states'] = sum(int(o[0], 0) + 1 for (mn, _, _, o) in parsed if mn == 's_nop' and o)
    table['VALU total (without MFMA)'] = sum(1 for (mn, _, _, _) in parsed if mn.startswith('v_') and not mn.startswith('v_mfma'))
    table['scratch instructions'] = sum(1 for (mn, _, _, _) in parsed if mn.startswith('scratch_'))
    return table


def gates(t):
    g = lambda *keys: sum(v for k, v in t.items() if any(k.startswith(p) for p in keys))   # noqa: E731
    return {'lane-group swaps + copies': g('group '), 'v_readlane + v_writelane': g('spill '),
            'non-ELU v_exp + v_rcp + v_log': g('transc v_exp', 'transc v_rcp', 'transc v_log'),
            'MFMA': g('MFMA '), 'operand split': g('split '), 'ELU': g('ELU ')}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--kernel', default=DEFAULT_KERNEL)
    ap.add_argument('--json')
    ap.add_argument('--against')
    ap.add_argument('--keep-asm')
    a, rest = ap.parse_known_args()
    defines = [x for x in rest if x.startswith('-D') or x.startswith('-f') or x.startswith('-m')]   # (-f... / -m...: code-generation flags under trial)
    asm = assembly(a.kernel, defines)
    if a.keep_asm:
        open(a.keep_asm, 'w').write(asm)
    t = classify(kernel_body(asm, a.kernel))
    other = json.load(open(a.against)) if a.against else None
    print('nr::%s %s' % (a.kernel, ' '.join(defines)))
    keys = sorted(set(t) | set(other or {}))
    for k in keys:
        print('%-34s %6d' % (k, t.get(k, 0)) + ('  %6d' % other.get(k, 0) if other else ''))
    print()
    gt, go = gates(t), gates(other) if other else None
    for k, v in gt.items():
        print('%-34s %6d' % (k, v) + ('  %6d  (%.0f %%)' % (go[k], 100.0 * v / go[k] if go[k] else 0.0) if go else ''))
    if a.json:
        json.dump(t, open(a.json, 'w'), indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
