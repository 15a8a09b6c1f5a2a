"""Prices the phases of the persistent pass step by instruction issue (CPU tool, no GPU needed).

The 64-row step runs one wave per SIMD, so nothing hides an instruction's issue slot: a phase costs about the sum
of the issue costs of the instructions the wave executes in it.  This tool takes

  1. the device assembly of ONE instantiation of the pass kernel built with the phase clocks
     (-DOSA_PASS_CLOCKS): every PTICK of the step loop is one clock read (s_memtime) in program order, so the reads
     cut the loop into its phases;
  2. a phase-clock file as tools/phase_clocks.py prints it (the "PASS kernel: cycles per minibatch" block);
  3. a cost table: issue cycles per instruction class (the default below; --costs FILE.json replaces entries)

and prints, per phase, the instruction counts by class, the measured cycles, the modelled cycles and the gap.
Where model and clock agree the phase is issue bound and a removed instruction is worth its table entry; a large
positive gap means stalls (waits, LDS round trips) the table does not price.  What the flat table gets WRONG
(profiles/pass_trim_phase_clocks.txt): a packed f32 instruction replaced by two plain ones.  The table calls that a
wash (8 = 4 + 4); the clocks of a build without packed math say + 700 cycles in Adam and + 330 in bias + norms --
dependent plain instructions do not issue back to back at 4 cycles, and a packed one carries two elements per
dependency.  Trust the table for instructions that DISAPPEAR, not for ones that change form.

Opcodes are classified by PREFIX (first match wins); the tool looks for no particular instruction.

The assembly of the headline instantiation (obs 60 -> KB 4, act 2 -> OT 1, SO) comes from a stub next to the
sources, e.g. csrc/_one.hip:

    #include "ppo_pass_body.h"
    __global__ __launch_bounds__(256, 1) void one(OsaPassArgs a) {
      int net = blockIdx.x;
      if (a.one_xcc) { if (blockIdx.x & 7) return; net = blockIdx.x >> 3; }
      if (!((a.nets_mask >> net) & 1)) return;
      osa_ppo_pass_body<4, 1, false, false, false, false, false, true>(a, net, 0);
    }

(to price a target attribute, e.g. __attribute__((target("no-packed-fp32-ops"))), put it on `one`) compiled with

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -DOSA_PASS_CLOCKS \
          --cuda-device-only -S csrc/_one.hip -o one_clocks.s

(about 5 s), then

    python tools/pass_issue_model.py one_clocks.s profiles/pass_trim_phase_clocks.txt --block 1

--classes adds a second table that splits each phase's plain `valu` count into accumulator-register copies, lane moves
of spilled scalars, moves, address arithmetic and math (profiles/pass_regs_issue_classes.txt), with the opcodes behind
every cell.
"""
from __future__ import annotations

import argparse
import json
import re
import sys

# (prefix, class) in matching order; class -> issue cycles for one wave per SIMD
PREFIX_CLASS = [
    ('v_mfma', 'mfma'),
    ('v_pk_', 'packed'),
    ('v_exp', 'trans'), ('v_rcp', 'trans'), ('v_sqrt', 'trans'), ('v_rsq', 'trans'), ('v_log', 'trans'),
    ('v_', 'valu'),  # plain VALU: moves, accumulator moves, selects, lane operations, compares
    ('ds_read_b128', 'lds128'), ('ds_write_b128', 'lds128'),
    ('ds_', 'mem'), ('global_', 'mem'), ('flat_', 'mem'), ('scratch_', 'mem'), ('buffer_', 'mem'),
    ('s_nop', 'nop'),
    ('s_waitcnt', 'wait'), ('s_barrier', 'wait'),
    ('s_', 'salu'),
]
COSTS = {'mfma': 35, 'packed': 8, 'trans': 8, 'valu': 4, 'lds128': 8, 'mem': 4, 'salu': 1, 'wait': 0,
         'nop': 1}  # nop: cycles per (n + 1) of `s_nop n`
CLASSES = ['mfma', 'valu', 'packed', 'trans', 'lds128', 'mem', 'salu', 'nop', 'wait']
# phases of the step loop between consecutive clock reads, first PTICK of the loop onwards (ppo_pass_body.h), and
# the names tools/phase_clocks.py prints for them
PHASES = ['fwd', 'loss', 'bwd', 'transpose+barA', 'dW', 'bias+norms', 'barB', 'adam', 'stats+barC']
CLOCK_OPCODE = 's_memtime'

_INSTR = re.compile(r'^\s+([a-z][a-z0-9_]*)\b\s*([^;/]*)')


def classify(opcode: str) -> str | None:
    for prefix, cls in PREFIX_CLASS:
        if opcode.startswith(prefix):
            return cls
    return None


def instructions(asm_text: str):
    """(opcode, operands) of every instruction line: indented, not a directive, not a label, not a comment."""
    for line in asm_text.splitlines():
        if not line[:1].isspace():
            continue  # labels and directives at column 0
        m = _INSTR.match(line)
        if m and not line.lstrip().startswith(('.', ';', '/')):
            yield m.group(1), m.group(2).strip()


def split_phases(asm_text: str, phases=PHASES, skip: int = 1, clock_opcode: str = CLOCK_OPCODE):
    """Counts by class of the instructions between clock reads skip + k and skip + k + 1, for every phase k.
    skip = 1: the first read initialises the clock before the loop, the second is the loop's first PTICK."""
    segs, cur = [], None
    nreads = 0
    for op, args in instructions(asm_text):
        if op == clock_opcode:
            nreads += 1
            if nreads > skip:
                cur = {c: 0 for c in CLASSES}
                cur['n'] = 0
                segs.append(cur)
            continue
        if cur is None:
            continue
        cls = classify(op)
        if cls is None:
            continue
        cur['n'] += 1
        if cls == 'nop':
            first = args.split(',')[0].strip()
            cur['nop'] += (int(first, 0) if first else 0) + 1
        else:
            cur[cls] += 1
    if len(segs) < len(phases) + 1:
        raise SystemExit(f'{nreads} clock reads in the assembly: need at least {skip + len(phases) + 1} '
                         f'(a build with -DOSA_PASS_CLOCKS of one instantiation)')
    return dict(zip(phases, segs))


# ---- what the plain `valu` column is made of (--classes).  Every plain VALU instruction of a phase falls into one of
#   agpr   accumulator-register copies: a value the allocator parked in an AGPR, read back before a VALU use
#   lane   lane moves that serve SGPR spills: v_writelane, and v_readlane from a register some v_writelane of the kernel
#          fills (a v_readlane of lane 63 at the end of a DPP reduction is math: it delivers the sum)
#   mov    register-to-register and constant moves (DPP moves of a reduction are math: they carry the operand)
#   addr   integer arithmetic whose result reaches the address operand of an LDS or memory instruction, directly or
#          through further integer arithmetic, before its register is overwritten
#   math   everything else
VALU_CLASSES = ['agpr', 'lane', 'mov', 'addr', 'math']
_INT_PREFIXES = ('v_add_u32', 'v_sub_u32', 'v_subrev_u32', 'v_add_co', 'v_addc_co', 'v_sub_co', 'v_subb_co', 'v_lshl_add',
                 'v_add_lshl', 'v_lshl_or', 'v_lshlrev_b', 'v_lshrrev_b', 'v_ashrrev_i', 'v_mul_lo_u32', 'v_mul_u32_u24',
                 'v_mul_i32_i24', 'v_mad_u32_u24', 'v_mad_i32_i24', 'v_mad_u64_u32', 'v_and_b32', 'v_or_b32', 'v_and_or_b32',
                 'v_bfe_u32', 'v_add3_u32')
_MEM_PREFIXES = ('ds_', 'global_', 'flat_', 'scratch_', 'buffer_')
_VREG = re.compile(r'\bv(\d+)\b|\bv\[(\d+):(\d+)\]')


def _vregs(operand: str) -> set:
    regs = set()
    for m in _VREG.finditer(operand):
        if m.group(1) is not None:
            regs.add(int(m.group(1)))
        else:
            regs.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return regs


def _address_regs(op: str, operands: list) -> set:
    """VGPRs of the address operand of a memory instruction: operand 1 of a load / read, operand 0 otherwise."""
    load = 'read' in op or 'load' in op
    idx = 1 if load else 0
    return _vregs(operands[idx]) if idx < len(operands) else set()


def spill_registers(instrs: list) -> set:
    """VGPRs whose lanes hold spilled SGPRs: every destination of a v_writelane in the kernel."""
    regs = set()
    for op, args in instrs:
        if op.startswith('v_writelane'):
            regs |= _vregs(args.split(',')[0])
    return regs


def valu_class(op: str, args: str = '', spills: frozenset = frozenset()) -> str:
    """Class of a plain VALU instruction; integer arithmetic comes back as 'int' and is settled by feeds_address()."""
    if op.startswith('v_accvgpr'):
        return 'agpr'
    if op.startswith('v_writelane'):
        return 'lane'
    if op.startswith('v_readlane'):
        src = args.split(',')[1] if ',' in args else ''
        return 'lane' if _vregs(src) & spills else 'math'
    if op.startswith('v_mov') and 'dpp' not in op:
        return 'mov'
    if op.startswith(_INT_PREFIXES):
        return 'int'
    return 'math'


def feeds_address(instrs: list, i: int, window: int = 600, _memo=None) -> bool:
    """True if the destination of integer instruction i reaches an address operand further down the listing (straight
    scan, branches ignored: the step loop is one block between its clock reads apart from short uniform branches)."""
    memo = {} if _memo is None else _memo
    if i in memo:
        return memo[i]
    memo[i] = False
    op, args = instrs[i]
    operands = [s.strip() for s in args.split(',')]
    live = _vregs(operands[0]) if operands else set()
    for j in range(i + 1, min(len(instrs), i + 1 + window)):
        if not live:
            break
        opj, argsj = instrs[j]
        opsj = [s.strip() for s in argsj.split(',')]
        if opj.startswith(_MEM_PREFIXES):
            if live & _address_regs(opj, opsj):
                memo[i] = True
                break
            if 'read' in opj or 'load' in opj:
                live -= _vregs(opsj[0])
            continue
        if not opj.startswith('v_'):
            continue
        srcs = set().union(*[_vregs(s) for s in opsj[1:]]) if len(opsj) > 1 else set()
        if live & srcs and valu_class(opj) == 'int' and feeds_address(instrs, j, window, memo):
            memo[i] = True
            break
        live -= _vregs(opsj[0])
    return memo[i]


def split_valu(asm_text: str, phases=PHASES, skip: int = 1, clock_opcode: str = CLOCK_OPCODE) -> dict:
    """phase -> {class: count, 'opcodes': {class: {opcode: count}}} of the plain VALU instructions, cut at the clock
    reads like split_phases()."""
    instrs = list(instructions(asm_text))
    spills = frozenset(spill_registers(instrs))
    memo = {}
    segs, cur, nreads = [], None, 0
    for i, (op, args) in enumerate(instrs):
        if op == clock_opcode:
            nreads += 1
            if nreads > skip:
                cur = {c: 0 for c in VALU_CLASSES}
                cur['opcodes'] = {c: {} for c in VALU_CLASSES}
                segs.append(cur)
            continue
        if cur is None or classify(op) != 'valu':
            continue
        cls = valu_class(op, args, spills)
        if cls == 'int':
            cls = 'addr' if feeds_address(instrs, i, _memo=memo) else 'math'
        cur[cls] += 1
        cur['opcodes'][cls][op] = cur['opcodes'][cls].get(op, 0) + 1
    return dict(zip(phases, segs))


def render_valu(split: dict, phases=PHASES, cost: int = COSTS['valu']) -> str:
    cols = ['valu'] + VALU_CLASSES
    lines = ['  '.join([f'{"phase":>14s}'] + [f'{c:>6s}' for c in cols]) + '   non-math cycles']
    tot = {c: 0 for c in cols}
    for ph in phases:
        s = split[ph]
        row = {'valu': sum(s[c] for c in VALU_CLASSES), **{c: s[c] for c in VALU_CLASSES}}
        for c in cols:
            tot[c] += row[c]
        lines.append('  '.join([f'{ph:>14s}'] + [f'{row[c]:>6d}' for c in cols])
                     + f'   {cost * (row["valu"] - row["math"]):>6d}')
    lines.append('  '.join([f'{"sum":>14s}'] + [f'{tot[c]:>6d}' for c in cols]) + f'   {cost * (tot["valu"] - tot["math"]):>6d}')
    lines.append('')
    for ph in phases:
        for c in VALU_CLASSES:
            ops = split[ph]['opcodes'][c]
            if ops:
                body = ', '.join(f'{n} {o}' for o, n in sorted(ops.items(), key=lambda kv: -kv[1]))
                lines.append(f'{ph:>14s}  {c:>5s}: {body}')
    return '\n'.join(lines)


def modelled(counts: dict, costs: dict = COSTS) -> int:
    return sum(counts[c] * costs[c] for c in CLASSES)


def read_clocks(text: str, column: int = 0, phases=PHASES, block: int = 0) -> dict:
    """phase -> cycles from a pass-kernel block of tools/phase_clocks.py or tools/pass_phases.py: a header line
    `... cycles per minibatch / optimiser step   actor  V_r  V_c`, then one line `name  actor  V_r  V_c` per clock
    interval in loop order.  The first line is the loop top in front of the first phase; the rest are taken BY
    POSITION (the two tools name them differently).  block: which of the file's blocks (0 = the first)."""
    blocks, rows = [], None
    for line in text.splitlines():
        if re.search(r'cycles per (minibatch|optimiser step)', line):
            rows = []
            blocks.append(rows)
            continue
        if rows is None:
            continue
        parts = line.split()
        if len(parts) < 4 or parts[0] == 'total':
            rows = None if parts[:1] == ['total'] else rows
            continue
        try:
            rows.append([float(v) for v in parts[-3:]][column])
        except ValueError:
            continue
    if block >= len(blocks):
        raise SystemExit(f'{len(blocks)} pass-kernel blocks in the clock file, block {block} asked for')
    return dict(zip(phases, blocks[block][1:]))


def table(asm_text: str, clock_text: str, costs: dict = COSTS, column: int = 0, phases=PHASES, skip: int = 1,
          block: int = 0) -> list:
    counts = split_phases(asm_text, phases, skip)
    clocks = read_clocks(clock_text, column, phases, block)
    rows = []
    for ph in phases:
        c = counts[ph]
        mod = modelled(c, costs)
        meas = clocks.get(ph)
        rows.append({'phase': ph, 'instructions': c['n'], **{k: c[k] for k in CLASSES}, 'measured': meas,
                     'modelled': mod, 'gap': None if meas is None else round(meas - mod)})
    return rows


def render(rows: list) -> str:
    cols = ['phase', 'instructions'] + CLASSES + ['measured', 'modelled', 'gap']
    lines = ['  '.join(f'{c:>14s}' if c == 'phase' else f'{c:>9s}' for c in cols)]
    for r in rows:
        cells = []
        for c in cols:
            v = r[c]
            s = '-' if v is None else (f'{v:.0f}' if isinstance(v, float) else str(v))
            cells.append(f'{s:>14s}' if c == 'phase' else f'{s:>9s}')
        lines.append('  '.join(cells))
    tot = {c: sum(r[c] for r in rows if r[c] is not None) for c in cols[1:]}
    lines.append('  '.join([f'{"sum":>14s}'] + [f'{tot[c]:>9.0f}' for c in cols[1:]]))
    return '\n'.join(lines)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('assembly', help='device assembly of one -DOSA_PASS_CLOCKS instantiation')
    ap.add_argument('clocks', help="output of tools/phase_clocks.py (the 'PASS kernel' block is read)")
    ap.add_argument('--costs', help='JSON object that replaces entries of the cost table', default=None)
    ap.add_argument('--column', type=int, default=0, help='0 actor (default), 1 reward critic, 2 cost critic')
    ap.add_argument('--block', type=int, default=0, help='which pass-kernel block of the clock file (default 0)')
    ap.add_argument('--skip', type=int, default=1, help='clock reads in front of the loop (default 1)')
    ap.add_argument('--json', action='store_true', help='print the rows as JSON instead of a table')
    ap.add_argument('--classes', action='store_true',
                    help='also split the plain valu column: AGPR copies, lane moves, moves, address arithmetic, math')
    a = ap.parse_args(argv)
    costs = dict(COSTS)
    if a.costs:
        costs.update(json.load(open(a.costs)))
    rows = table(open(a.assembly).read(), open(a.clocks).read(), costs, a.column, PHASES, a.skip, a.block)
    print(json.dumps(rows) if a.json else render(rows))
    if a.classes:
        split = split_valu(open(a.assembly).read(), PHASES, a.skip)
        print(json.dumps(split) if a.json else '\n' + render_valu(split, cost=costs['valu']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
