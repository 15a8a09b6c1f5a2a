"""tools/pass_issue_model.py on a hand-written listing (tests/golden/pass_issue_model_snippet.s: one clock read in
front of the loop, ten in it) and a phase-clock file in the format of tools/pass_phases.py: per phase the instruction
counts by class, the modelled cycles (sum of issue costs) and the gap to the clock, worked out by hand below."""
import importlib.util
import json
import os

import pytest


@pytest.fixture(scope='module')
def tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'pass_issue_model.py')
    spec = importlib.util.spec_from_file_location('pass_issue_model', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def texts(golden_dir):
    return (open(os.path.join(golden_dir, 'pass_issue_model_snippet.s')).read(),
            open(os.path.join(golden_dir, 'pass_issue_model_clocks.txt')).read())


# phase: (instructions, {class: count}, measured actor cycles, modelled cycles)
#   fwd   2 MFMA x 35 + one 16-byte LDS read 8 + one exp 8 + `s_nop 3` = 4 cycles                = 90
#   loss  v_sub 4 + packed multiply 8 + select 4                                                 = 16
#   bwd   MFMA 35 + ds_bpermute 4 + wait 0 + packed fma 8                                        = 47
#   dW    MFMA 35 + 16-byte LDS read 8                                                           = 43
#   bias  add 4 + 4-byte LDS read 4 + readlane 4                                                 = 12
#   adam  sqrt 8 + rcp 8 + fma 4 + LDS store 4                                                   = 24
#   stats global store 4 + scalar add 1                                                          = 5
EXPECT = {
    'fwd': (5, {'mfma': 2, 'lds128': 1, 'trans': 1, 'nop': 4}, 100, 90),
    'loss': (3, {'valu': 2, 'packed': 1}, 16, 16),
    'bwd': (4, {'mfma': 1, 'mem': 1, 'wait': 1, 'packed': 1}, 60, 47),
    'transpose+barA': (1, {'wait': 1}, 30, 0),
    'dW': (2, {'mfma': 1, 'lds128': 1}, 43, 43),
    'bias+norms': (3, {'valu': 2, 'mem': 1}, 20, 12),
    'barB': (1, {'wait': 1}, 7, 0),
    'adam': (4, {'trans': 2, 'valu': 1, 'mem': 1}, 24, 24),
    'stats+barC': (2, {'mem': 1, 'salu': 1}, 9, 5),
}


def test_table_of_the_snippet(tool, texts):
    rows = tool.table(*texts)
    assert [r['phase'] for r in rows] == list(EXPECT) == tool.PHASES
    for r in rows:
        n, counts, meas, mod = EXPECT[r['phase']]
        assert r['instructions'] == n, r
        for cls in tool.CLASSES:
            assert r[cls] == counts.get(cls, 0), (r['phase'], cls)
        assert (r['measured'], r['modelled'], r['gap']) == (meas, mod, meas - mod), r


def test_what_is_not_an_instruction_is_not_counted(tool, texts):
    ops = [op for op, _ in tool.instructions(texts[0])]
    assert ops[0] == 's_load_dwordx2' and ops[-1] == 's_endpgm'
    assert ops.count(tool.CLOCK_OPCODE) == 11
    assert not any(op.startswith(('.', 'one', 'lbb')) for op in ops)  # directives, labels
    # the loop tail behind the last clock read and the prologue in front of the first belong to no phase
    assert sum(r['instructions'] for r in tool.table(*texts)) == len(ops) - 11 - 1 - 3


def test_other_column_and_cost_table(tool, texts):
    critic = tool.table(*texts, column=2)
    assert critic[0]['measured'] == 102 and critic[-1]['measured'] == 11
    costs = dict(tool.COSTS, packed=4, mfma=32)
    rows = {r['phase']: r for r in tool.table(*texts, costs=costs)}
    assert rows['loss']['modelled'] == 12 and rows['fwd']['modelled'] == 84


def test_second_block_of_a_clock_file(tool, texts):
    """A file with the blocks of two builds (tools/phase_clocks.py format after the pass_phases.py one)."""
    second = texts[1].replace('cycles per optimiser step', 'PASS kernel: cycles per minibatch').replace(' 100 ', ' 140 ')
    both = texts[1] + 'us per launch 44.6\n' + second
    assert tool.table(texts[0], both)[0]['gap'] == 10
    assert tool.table(texts[0], both, block=1)[0]['gap'] == 50
    with pytest.raises(SystemExit):
        tool.table(texts[0], both, block=2)


def test_too_few_clock_reads_is_an_error(tool, texts):
    asm = texts[0].replace('s_memtime', 's_mov_b64', 3)
    with pytest.raises(SystemExit):
        tool.table(asm, texts[1])


def test_command_line(tool, golden_dir, capsys):
    args = [os.path.join(golden_dir, 'pass_issue_model_snippet.s'), os.path.join(golden_dir, 'pass_issue_model_clocks.txt')]
    assert tool.main(args) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0].split()[:3] == ['phase', 'instructions', 'mfma'] and out[-1].split()[0] == 'sum'
    assert out[-1].split()[-3:] == ['309', '237', '72']
    assert tool.main(args + ['--json']) == 0
    rows = json.loads(capsys.readouterr().out)
    assert rows[0]['phase'] == 'fwd' and rows[0]['gap'] == 10
