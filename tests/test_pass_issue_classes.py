"""tools/pass_issue_model.py --classes on a hand-written listing: every plain VALU instruction of a phase is an
accumulator-register copy, a lane move of a spilled scalar, a move, address arithmetic or math."""
import importlib.util
import os

import pytest

# one clock read in front of the loop, then three phases (four reads); v254 is the register the kernel spills scalars into
LISTING = """
one:
	s_memtime s[0:1]
	v_writelane_b32 v254, s20, 3
.LBB0_1:
	s_memtime s[2:3]
	v_accvgpr_read_b32 v10, a4
	v_readlane_b32 s20, v254, 3
	v_add_u32_e32 v11, v12, v13
	ds_read_b128 v[20:23], v11 offset:64
	v_add_f32_e32 v30, v20, v21
	v_mov_b32_e32 v31, v30
	s_memtime s[4:5]
	v_ashrrev_i32_e32 v41, 31, v40
	v_lshl_add_u64 v[42:43], v[40:41], 2, s[8:9]
	global_load_dword v44, v[42:43], off
	v_add_u32_e32 v45, 1, v46
	v_cvt_f32_i32_e32 v47, v45
	v_add_f32_dpp v48, v48, v48 row_shr:1 row_mask:0xf bank_mask:0xf
	v_mov_b32_dpp v49, v48 row_bcast:15 row_mask:0xa bank_mask:0xf
	v_readlane_b32 s30, v48, 63
	s_memtime s[6:7]
	v_add_u32_e32 v50, v51, v52
	v_mov_b32_e32 v50, 0
	ds_write_b32 v50, v53
	v_accvgpr_write_b32 a7, v53
	v_xor_b32_e32 v54, 0x80000000, v53
	v_pk_fma_f32 v[56:57], v[54:55], v[58:59], v[60:61]
	s_memtime s[10:11]
	s_endpgm
"""
PHASES = ['a', 'b', 'c']
# a: one AGPR read, one spill reload, the add that forms the LDS address, a float add, a move
# b: sign extension + 64-bit address of a global load (2 addr); an integer add that only feeds a conversion is math, as
#    are the conversion, the DPP add, the DPP move and the lane-63 read of the reduction (v48 is no spill register)
# c: the add is overwritten before the store uses its register: math; move, AGPR write, xor (math); packed is not plain VALU
EXPECT = {
    'a': {'agpr': 1, 'lane': 1, 'mov': 1, 'addr': 1, 'math': 1},
    'b': {'agpr': 0, 'lane': 0, 'mov': 0, 'addr': 2, 'math': 5},
    'c': {'agpr': 1, 'lane': 0, 'mov': 1, 'addr': 0, 'math': 2},
}


@pytest.fixture(scope='module')
def tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'pass_issue_model.py')
    spec = importlib.util.spec_from_file_location('pass_issue_model', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_classes_of_the_listing(tool):
    split = tool.split_valu(LISTING, PHASES, skip=1)
    assert list(split) == PHASES
    for ph, want in EXPECT.items():
        assert {c: split[ph][c] for c in tool.VALU_CLASSES} == want, ph
    # the classes add up to the plain valu column of the issue table
    counts = tool.split_phases(LISTING, PHASES, skip=1)
    for ph in PHASES:
        assert sum(split[ph][c] for c in tool.VALU_CLASSES) == counts[ph]['valu'], ph
    assert split['b']['opcodes']['addr'] == {'v_ashrrev_i32_e32': 1, 'v_lshl_add_u64': 1}


def test_rendered_table_prices_the_non_math_instructions(tool):
    text = tool.render_valu(tool.split_valu(LISTING, PHASES, skip=1), PHASES)
    rows = {line.split()[0]: line.split() for line in text.splitlines()[1:5]}
    assert rows['a'][1:] == ['5', '1', '1', '1', '1', '1', '16']
    assert rows['sum'][1:] == ['16', '2', '1', '2', '3', '8', '32']
