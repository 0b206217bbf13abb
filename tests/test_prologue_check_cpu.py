"""CPU: no GEMM-family kernel of the built libraries divides, or meets a barrier, in front of its first operand request.

tools/check_prologue.py walks the disassembly of every generic / producer-specialised, halo-conv and wide-GEGLU kernel of both builds
from entry to the first LDS-DMA request.  Every divisor of a prologue is a launch constant whose quotient or reciprocal the host
supplies (csrc/gemm.h GemmLaunch), and the first requests -- the weights' -- need neither the row arithmetic nor the halo-row table
with its barrier: zero division expansions and zero barriers.  Instruction counts are reported (profiles/prologue_static.txt), not
asserted."""
import importlib.util
import os

import pytest

from diff_foley_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    if not all(os.path.exists(p) for p in E.LIB_PATHS.values()):
        import __graft_entry__
        __graft_entry__.build()
    spec = importlib.util.spec_from_file_location("check_prologue", os.path.join(ROOT, "tools", "check_prologue.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.OBJDUMP):
        pytest.skip("llvm-objdump not found: the code objects cannot be read")
    return mod


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_no_division_and_no_barrier_in_front_of_the_first_request(tool, prec):
    rows = tool.scan(E.LIB_PATHS[prec])
    for fam in tool.FAMILIES:
        assert any(fam in k for k in rows), f"no {fam} kernel found in the {prec} build"
    assert len(rows) >= 250
    div = {k: v[2] for k, v in rows.items() if v[2]}
    bar = {k: v[3] for k, v in rows.items() if v[3]}
    assert not div, f"division expansions in front of the first operand request: {div}"
    assert not bar, f"barriers in front of the first operand request: {bar}"
    assert tool.violations(rows) == []


def test_walk_counts_what_it_says():
    """The walker on a hand-written listing: counts stop at the first LDS-DMA request; both division forms and the barrier are seen."""
    spec = importlib.util.spec_from_file_location("check_prologue", os.path.join(ROOT, "tools", "check_prologue.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ins = ["s_load_dwordx4 s[0:3], s[4:5], 0x0", "v_rcp_iflag_f32_e32 v1, v2", "v_div_scale_f32 v1, vcc, v2, v2, v3",
           "v_div_scale_f32 v4, vcc, v3, v2, v3", "v_div_fixup_f32 v1, v1, v2, v3", "s_barrier", "s_buffer_load_dword s6, s[0:3], 0x0",
           "buffer_load_dword v1, v2, s[0:3], 0 offen", "buffer_load_dwordx4 v2, s[72:75], 0 offen lds", "s_barrier", "v_rcp_iflag_f32_e32 v1, v2"]
    assert mod.walk(ins) == (8, 2, 2, 1)
    assert mod.walk(ins[:8]) is None
    assert mod.violations({"gemm_bf16_kernel<1>": (8, 2, 2, 1)}) != [] and mod.violations({"gemm_bf16_kernel<1>": (8, 2, 0, 0)}) == []
