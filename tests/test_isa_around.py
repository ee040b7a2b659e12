"""tools/isa_loop_count.py --around on a short synthetic assembly text: a pass kernel that holds the two programs of a sweep (the event
workgroups with a large loop of their own, whose code leads into the walk's entry as the compiler's structured control flow does), a
walk with prologue, loop (one inner loop), flush and rank loop."""
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("isa_loop_count", os.path.join(HERE, "..", "tools", "isa_loop_count.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _kernel(flat_flush):
    atomic = "flat_atomic_add_f32 v[8:9], v6" if flat_flush else "global_atomic_add_f32 v[8:9], v6, off"
    rank = "flat_atomic_add v2, v[6:7], v10 sc0" if flat_flush else "ds_add_rtn_u32 v2, v6, v10"
    t = """
_Z9fake_passILi0EEvi:                   ; @_Z9fake_passILi0EEvi
; %bb.0:
	s_load_dword s4, s[0:1], 0x0
	s_cbranch_scc1 .LBB0_3
; %bb.1:
	global_load_dwordx2 v[20:21], v0, s[2:3]
	s_waitcnt vmcnt(0)
.LBB0_2:                                ; =>This Inner Loop Header: Depth=1
""" + "	v_mov_b32_e32 v1, v2\n" * 401 + """	global_load_dword v30, v[20:21], off
	s_waitcnt vmcnt(0)
	s_cbranch_vccnz .LBB0_2
	s_cbranch_vccz .LBB0_12
.LBB0_3:
	global_load_dword v1, v0, s[0:1]
	global_load_dwordx4 v[2:5], v0, s[2:3]
	s_waitcnt vmcnt(0)
	v_cmp_lt_i32_e32 vcc, s2, v1
	s_cbranch_vccz .LBB0_12
; %bb.4:
	global_load_dword v6, v[2:3], off
	global_load_dword v7, v[2:3], off offset:4
	ds_write_b32 v9, v0
	s_waitcnt vmcnt(0)
	ds_write_b32 v8, v6
	s_waitcnt lgkmcnt(0)
	s_barrier
.LBB0_5:                                ; =>This Loop Header: Depth=1
                                        ;     Child Loop BB0_6 Depth 2
	global_load_dwordx4 v[40:43], v[2:3], off
	s_waitcnt vmcnt(0)
	v_fract_f32_e32 v1, v2
	ds_add_f32 v1, v2
.LBB0_6:                                ;   Parent Loop BB0_5 Depth=1
                                        ; =>  This Inner Loop Header: Depth=2
	ds_read_b32 v1, v2
	s_waitcnt lgkmcnt(0)
	s_cbranch_execnz .LBB0_6
; %bb.7:                                ;   in Loop: Header=BB0_5 Depth=1
	s_cbranch_vccnz .LBB0_5
; %bb.8:
	global_load_dword v10, v[2:3], off
	s_waitcnt lgkmcnt(0)
	s_barrier
	s_waitcnt vmcnt(0)
.LBB0_9:                                ; =>This Inner Loop Header: Depth=1
	ds_read_b32 v6, v1
	global_load_dword v11, v[2:3], off
	s_waitcnt lgkmcnt(0)
	ATOMIC
	ATOMIC
	s_waitcnt vmcnt(0)
	s_cbranch_execnz .LBB0_9
; %bb.10:
	s_nop 0
.LBB0_11:                               ; =>This Inner Loop Header: Depth=1
	global_load_dword v2, v[4:5], off
	s_waitcnt vmcnt(0)
	RANK
	s_waitcnt vmcnt(0) lgkmcnt(0)
	global_store_dword v[6:7], v2, off
	s_cbranch_execnz .LBB0_11
.LBB0_12:
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _Z9fake_passILi0EEvi
	.end_amdhsa_kernel
"""
    return t.replace("ATOMIC", atomic).replace("RANK", rank).split("\n")


@pytest.mark.parametrize("flat_flush", [True, False])
def test_prologue_and_flush_of_a_pass_kernel(tool, flat_flush):
    lines = []
    got = tool.around(tool.kernel_body(_kernel(flat_flush), "fake_passILi0EE"), out=lines.append)
    # the prologue: the walk's own two waits with the loads each waits for -- not the wait of the event workgroups' code, which leads
    # into the walk's entry, and not the loop's
    assert got["prologue"]["waits"] == [(0, ["global_load_dword", "global_load_dwordx4"]), (0, ["global_load_dword", "global_load_dword"])]
    assert got["prologue"]["order"] == ["global_load_dword", "global_load_dwordx4", "vmcnt(0)", "global_load_dword", "global_load_dword", "vmcnt(0)"]
    # the flush starts at the barrier behind the loop (the load ahead of it is not listed) and ends where the rank loop begins
    name = "flat_atomic_add_f32" if flat_flush else "global_atomic_add_f32"
    assert got["flush"]["atomics"] == [name, name]
    assert got["flush"]["waits"] == [(0, []), (0, ["global_load_dword"])]
    assert got["flush"]["order"] == ["vmcnt(0)", "global_load_dword", name, name, "vmcnt(0)"]
    assert got["ranks"]["atomics"] == ["flat_atomic_add" if flat_flush else "ds_add_rtn_u32"]
    text = "\n".join(lines)
    assert "2 %s" % name in text and "prologue" in text and "flush" in text


def test_the_loop_listing_still_finds_the_walk(tool, capsys, tmp_path, monkeypatch):
    """the instruction mix of the loop's arms, as before: the loop with the tally's LDS atomic, not the larger loop of the event code"""
    path = tmp_path / "fake.s"
    path.write_text("\n".join(_kernel(False)))
    monkeypatch.setattr("sys.argv", ["isa_loop_count.py", str(path), "fake_passILi0EE"])
    tool.main()
    out = capsys.readouterr().out
    assert "step  VALU    1  SALU    4  LDS   2  VMEM   1" in out      # (the 401 moves of the event code's loop are not counted)
