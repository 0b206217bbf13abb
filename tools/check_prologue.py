#!/usr/bin/env python
"""Static view of what a GEMM-family block executes between kernel entry and its first operand request.

Nothing is in flight on a CU while a block works its way to the first `buffer_load ... lds`, so whatever stands in front of it is
paid once per launch of a chain of dependent launches.  Every divisor of the prologues is a constant of the
launch: gemm_launch_consts (csrc/gemm.hip) derives quotients and reciprocals on the host, the kernels only read them.  This tool
walks the disassembly of every GEMM-family kernel of a built library from its entry to the first LDS-DMA request, in text order, and
reports

  instructions      before the first request
  scalar loads      s_load_* / s_buffer_load_* among them
  divisions         expansions of a division: v_rcp_iflag_f32 (the integer form), v_div_scale_f32 + v_div_fixup_f32 (the float form;
                    one expansion has two scales and one fixup -- the fixups are counted)
  barriers          s_barrier

The families in scope are those of the shipped plans: the generic / producer-specialised body (gemm_bf16_kernel), the halo convs
(conv3x3_halo_kernel) and the wide GEGLU projection (geglu_wide_kernel).  The persistent GEGLU kernel and the split-K reduce kernels
are not walked.  The rule (exit code 1, tests/test_prologue_check_cpu.py): no division expansion in front of the first request of any
kernel walked, and no barrier in front of it.

usage: tools/check_prologue.py [--table] [lib ...]      (default: both in-tree libraries; --table prints one line per kernel)"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
FAMILIES = ("gemm_bf16_kernel", "conv3x3_halo_kernel", "geglu_wide_kernel")
NO_BARRIER = FAMILIES       # every walked family requests before it synchronises


def short(name):
    """`void (anonymous namespace)::gemm_bf16_kernel<128, 128, 2, 2, 3, 0, 0, 3, 0>(GemmParams)` -> `gemm_bf16_kernel<128,128,...>`"""
    m = re.search(r"(\w+_kernel)<([^>]*)>", name)
    return f"{m.group(1)}<{m.group(2).replace(' ', '')}>" if m else name


def walk(ins):
    """(instructions, scalar loads, division expansions, barriers) in front of the first LDS-DMA request; None: the kernel has none"""
    n = sl = dv = ba = 0
    for l in ins:
        op = l.split()[0]
        if op.startswith("buffer_load") and l.endswith("lds"):
            return n, sl, dv, ba
        n += 1
        if op.startswith(("s_load_", "s_buffer_load_")):
            sl += 1
        elif op.startswith(("v_rcp_iflag_f32", "v_div_fixup_f32")):
            dv += 1
        elif op == "s_barrier":
            ba += 1
    return None


def scan(lib):
    """{short kernel name: (instructions, scalar loads, divisions, barriers)} of the in-scope kernels of one library"""
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, dst)
        subprocess.run([OBJDUMP, "--offloading", dst], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        for co in sorted(f for f in glob.glob(dst + ".*") if "gfx950" in f):
            out = subprocess.run([OBJDUMP, "-d", "-C", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
            kern, kernels = None, {}
            for line in out.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
                if m:
                    kern = m.group(1)
                    kernels[kern] = []
                    continue
                line = line.split("//")[0].strip()
                if line and kern is not None:
                    kernels[kern].append(line)
            for k, ins in kernels.items():
                r = walk(ins) if any(f in k for f in FAMILIES) else None
                if r is not None:
                    rows[short(k)] = r
    return rows


def violations(rows):
    bad = []
    for k, (n, sl, dv, ba) in sorted(rows.items()):
        if dv:
            bad.append(f"{k}: {dv} division expansion(s) in front of the first operand request")
        if ba and any(f in k for f in NO_BARRIER):
            bad.append(f"{k}: {ba} barrier(s) in front of the first operand request")
    return bad


def main():
    args = [a for a in sys.argv[1:] if a != "--table"]
    table = "--table" in sys.argv[1:]
    libs = args or [os.path.join(ROOT, "diff_foley_amd", n) for n in ("libdfengine.so", "libdfengine_f16.so")]
    if not os.path.exists(OBJDUMP):
        print(f"check_prologue: {OBJDUMP} not found -- skipped (warning)")
        return 0
    bad, tot = [], 0
    for lib in libs:
        rows = scan(lib)
        tot += len(rows)
        if table:
            print(f"# {os.path.basename(lib)}: kernel, instructions, scalar loads, division expansions, barriers -- entry to first LDS-DMA request")
            for k, (n, sl, dv, ba) in sorted(rows.items()):
                print(f"{k:64s} {n:5d} {sl:3d} {dv:3d} {ba:2d}")
        for fam in FAMILIES:
            sel = [v for k, v in rows.items() if fam in k]
            if sel:
                print(f"{os.path.basename(lib)}: {fam}: {len(sel)} kernels, instructions {min(v[0] for v in sel)}..{max(v[0] for v in sel)}, "
                      f"scalar loads {min(v[1] for v in sel)}..{max(v[1] for v in sel)}, divisions {min(v[2] for v in sel)}..{max(v[2] for v in sel)}, "
                      f"barriers {min(v[3] for v in sel)}..{max(v[3] for v in sel)}")
        bad += [f"{os.path.basename(lib)}: {b}" for b in violations(rows)]
    for b in bad:
        print("VIOLATION:", b)
    print(f"check_prologue: {tot} kernels walked, {len(bad)} violation(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
