"""ISA guard of k_ssim<8, true> (the eight-column SSIM kernel of the pair pipeline's wide images), CPU-only: the gfx950 code object
inside the SHIPPED libssrhip.so is disassembled with the ROCm llvm-objdump, as tests/test_ssim_isa.py does for the four-column
kernel, and the steady-state row loop is checked for what the source asks for."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "k_ssim<8, true>"
STEPS_PER_TRIP = 14          # ring slot = step mod 7, prefetch set = step mod 2
LOADS_PER_ROW = 6            # one row request: 2 x 2 x buffer_load_dwordx4 + 2 x buffer_load_dword
MAX_VGPRS = 256              # two waves per SIMD


def _objdump():
    cands = [shutil.which("llvm-objdump")]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    cands += [os.path.join(r, sub, "llvm-objdump") for r in (rocm, os.environ.get("ROCM_PATH", "/opt/rocm"))
              for sub in ("lib/llvm/bin", "llvm/bin")]
    for c in cands:
        if c and os.path.exists(c):
            return c
    return None


def _disassemble(tmp_path):
    """[(offset in the kernel, mnemonic, operand text, branch-target offset or None)] of KERNEL, plus its descriptor."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    from ssr_eval_amd import _lib
    objdump = _objdump()
    if objdump is None:
        pytest.skip("no llvm-objdump on this machine")
    found = code_objects.kernel_elf(_lib.LIB_PATH, KERNEL)
    assert found is not None, "libssrhip.so holds no %s" % KERNEL
    mangled, elf = found
    desc = [k for k in code_objects.kernels(_lib.LIB_PATH) if k["name"] == mangled + ".kd" or k["name"] == mangled]
    assert len(desc) == 1, desc
    path = os.path.join(str(tmp_path), "k_ssim8.co")
    with open(path, "wb") as f:
        f.write(elf)
    text = subprocess.run([objdump, "-d", "--disassemble-symbols=" + mangled, path], capture_output=True, text=True, check=True).stdout
    base, insts = None, []
    for line in text.split("\n"):
        m = re.match(r"^([0-9a-fA-F]+) <%s>:" % re.escape(mangled), line)
        if m:
            base = int(m.group(1), 16)
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*[0-9A-Fa-f ]+?(?:<%s\+0x([0-9a-fA-F]+)>)?\s*$" % re.escape(mangled), line)
        if m and base is not None:
            insts.append((int(m.group(3), 16) - base, m.group(1), m.group(2), int(m.group(4), 16) if m.group(4) else None))
    assert len(insts) > 1000, "disassembly of %s not understood (%d instructions)" % (KERNEL, len(insts))
    return insts, desc[0]


def _steady_loop(insts):
    """The innermost loop (a backward branch and its target) that holds the fourteen row steps, as a list of instructions."""
    loops = []
    for off, mn, _ops, target in insts:
        if mn.startswith(("s_cbranch", "s_branch")) and target is not None and target <= off:
            body = [i for i in insts if target <= i[0] <= off]
            if sum(i[1].startswith("buffer_load") for i in body) >= STEPS_PER_TRIP * LOADS_PER_ROW:
                loops.append(body)
    assert loops, "no loop of %s holds fourteen row requests" % KERNEL
    return min(loops, key=len)


def test_wide_ssim_steady_loop_keeps_the_youngest_row_request_in_flight(tmp_path):
    """Inside the steady-state trip loop no s_waitcnt has a vmcnt operand below 6 (one row request is six loads, so the row requested
    last is never waited for in the step that requested it), the loop holds 14 x 6 = 84 buffer loads and no branch but its own back
    edge.  The kernel uses no scratch, spills no vector register and fits two waves per SIMD (VGPRs + AGPRs <= 256).  Printed, not
    asserted: the instruction mix of the trip (the constants of the four / eight column choice in ssim_geom come from it)."""
    insts, desc = _disassemble(tmp_path)
    loop = _steady_loop(insts)
    waits = [int(m.group(1)) for _o, mn, ops, _t in loop if mn == "s_waitcnt" for m in [re.search(r"vmcnt\((\d+)\)", ops)] if m]
    loads = sum(mn.startswith("buffer_load") for _o, mn, _ops, _t in loop)
    branches = sum(mn.startswith(("s_cbranch", "s_branch")) for _o, mn, _ops, _t in loop)
    mix = {p: sum(mn.startswith(p) for _o, mn, _ops, _t in loop) for p in ("v_", "ds_", "buffer_", "s_")}
    hist = {w: waits.count(w) for w in sorted(set(waits))}
    print("%s: %d VGPRs, %d B scratch; steady loop %d instructions (%s), %d bytes, %d buffer loads, vmcnt waits %s"
          % (KERNEL, desc["vgpr"] + desc["agpr"], desc["scratch"], len(loop), mix, loop[-1][0] - loop[0][0], loads, hist))
    assert waits, "the loop waits for no load at all"
    assert min(waits) >= LOADS_PER_ROW, "vmcnt waits in the steady loop (value: count): %s" % hist
    assert loads == STEPS_PER_TRIP * LOADS_PER_ROW, loads
    assert branches == 1, "%d branches inside the steady loop" % branches
    assert desc["scratch"] == 0 and desc["vgpr_spill"] == 0, desc
    assert desc["vgpr"] + desc["agpr"] <= MAX_VGPRS, desc
