"""ISA guard of the four float64 k_stft_wave instantiations, CPU-only: the gfx950 code object inside the SHIPPED libssrhip.so is
disassembled with the ROCm llvm-objdump (as tests/test_ssim_wide_isa.py does for k_ssim<8, true>) and the frame loop is checked for
what ssr_stft_wave.h asks for: both table requests (R.tw1: three 16-byte loads, R.tw2: twelve) a whole butterfly pass ahead of their
waits, exact waits, no vector-memory instruction under a lane condition, at most 256 VGPRs and no scratch.

"A whole butterfly pass" is counted in the same disassembly, not assumed.  The 64-bit DS writes of the transform belong to its two
exchanges; the float64 instructions between the last write of the first exchange and the first write of the second are pass 1 (281
to 290 in the shipped code, of the 292 of four ssr_bfly8_tw of 72 fused multiply-adds + 4 for t W8: the second exchange's first writes
are issued while the last butterfly finishes).
  tw2 is requested at the top of pass 1 and first needed by pass 2: at least that count lies between request and wait.
  tw1 is requested in pass 0 behind its first layer, which is where the 64 sample conversions (v_cvt_f64_f32) are: the request comes
  after the last conversion and at most one first-layer group (2 + 4 + 8 + 8 = 22 float64 instructions, ssr_dft32_win_layer1) behind
  it, its first wait comes after the first exchange's last write, and everything pass 0 still has to do - the float64 instructions
  up to the first exchange's first write, 262 in the shipped code - lies between the two.
(Requested inside the exchanges, as before, the distances are 0 float64 instructions.)"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["k_stft_wave<double, %s, true, %s>" % (s, m) for s in ("false", "true") for m in ("false", "true")]
MAX_VGPRS = 256              # two waves per SIMD
TW1_LOADS, TW2_LOADS = 3, 12
LAYER1_GROUP = 2 + 4 + 8 + 8                    # float64 instructions of one n2 group of ssr_dft32_win_layer1


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


def _disassemble(tmp_path, kernel):
    """[(offset in the kernel, mnemonic, operand text, branch-target offset or None)] of `kernel`, plus its descriptor."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    from ssr_eval_amd import _lib
    objdump = _objdump()
    if objdump is None:
        pytest.skip("no llvm-objdump on this machine")
    found = code_objects.kernel_elf(_lib.LIB_PATH, kernel)
    assert found is not None, "libssrhip.so holds no %s" % kernel
    mangled, elf = found
    desc = [k for k in code_objects.kernels(_lib.LIB_PATH) if k["name"] == mangled + ".kd" or k["name"] == mangled]
    assert len(desc) == 1, desc
    path = os.path.join(str(tmp_path), "k_stft_wave.co")
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
    assert len(insts) > 1000, "disassembly of %s not understood (%d instructions)" % (kernel, len(insts))
    return insts, desc[0]


def _is_vmem(mn):
    return mn.startswith(("buffer_", "global_", "flat_", "scratch_"))


def _is_fp64(mn):
    return mn.startswith("v_") and "_f64" in mn and "cvt" not in mn


def _frame_loop(insts, kernel):
    """The innermost loop (a backward branch and its target) that holds the fifteen 16-byte table loads."""
    loops = []
    for off, mn, _ops, target in insts:
        if mn.startswith(("s_cbranch", "s_branch")) and target is not None and target <= off:
            body = [i for i in insts if target <= i[0] <= off]
            if sum(i[1].startswith("buffer_load_dwordx4") for i in body) >= TW1_LOADS + TW2_LOADS:
                loops.append(body)
    assert loops, "no loop of %s holds the table loads" % kernel
    return min(loops, key=len)


def _covering_wait(loop, at):
    """(index of the first s_waitcnt behind loop[at] that guarantees the load loop[at] has returned, its vmcnt, the number of
    vector-memory instructions issued between the two): the memory counter returns in order, so vmcnt(n) covers the load once no more
    than n younger ones have been issued."""
    younger = 0
    for j in range(at + 1, len(loop)):
        _o, mn, ops, _t = loop[j]
        if _is_vmem(mn):
            younger += 1
        elif mn == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", ops)
            if m and int(m.group(1)) <= younger:
                return j, int(m.group(1)), younger
    raise AssertionError("a table load of the frame loop is never waited for")


@pytest.mark.parametrize("kernel", KERNELS)
def test_stft_wave_frame_loop_requests_its_tables_a_pass_ahead(tmp_path, kernel):
    insts, desc = _disassemble(tmp_path, kernel)
    loop = _frame_loop(insts, kernel)
    # registers
    assert desc["scratch"] == 0 and desc["vgpr_spill"] == 0, desc
    assert desc["vgpr"] + desc["agpr"] <= MAX_VGPRS, desc
    # the table requests: all of them in the straight-line transform, tw1's three first, tw2's twelve in one run
    x4 = [i for i, (_o, mn, _ops, _t) in enumerate(loop) if mn.startswith("buffer_load_dwordx4")]
    assert len(x4) == TW1_LOADS + TW2_LOADS, "%d 16-byte loads in the frame loop" % len(x4)
    groups = {"tw1": x4[:TW1_LOADS], "tw2": x4[TW1_LOADS:]}
    first_wait, vmcnts = {}, {}
    for name, group in groups.items():
        assert not any(loop[i][1].startswith(("s_cbranch", "s_branch")) for i in range(group[0], group[-1])), "%s is not one run" % name
        covers = [_covering_wait(loop, i) for i in group]
        # exact: a wait returns the youngest load it covers and nothing issued behind that one (one wait may cover several loads)
        for j in sorted(set(j for j, _v, _y in covers)):
            vmcnt, younger = min((v, y) for jj, v, y in covers if jj == j)
            assert vmcnt == younger, "%s: s_waitcnt vmcnt(%d) with %d younger requests in flight also waits for those" % (name, vmcnt, younger)
        first_wait[name], vmcnts[name] = min(j for j, _v, _y in covers), [v for _j, v, _y in covers]
        assert first_wait[name] > group[-1]
        assert not any(mn.startswith(("s_cbranch", "s_branch")) and t is not None and t <= o for o, mn, _ops, t in loop[group[-1] + 1:first_wait[name]])
    transform_end = max(j for j, _v, _y in [_covering_wait(loop, i) for i in groups["tw2"]])
    # float64 instructions in front of every instruction of the loop; the two exchanges from the transform's 64-bit DS writes
    before, n = [], 0
    for _o, mn, _ops, _t in loop:
        before.append(n)
        n += _is_fp64(mn)
    fp64 = lambda i, j: before[j] - before[i + 1]                    # float64 instructions strictly between loop[i] and loop[j]
    writes = [i for i in range(transform_end) if loop[i][1].startswith("ds_write") and "b64" in loop[i][1]]
    assert len(writes) >= 4
    k = max(range(len(writes) - 1), key=lambda k: fp64(writes[k], writes[k + 1]))
    e1_first, e1_last, e2_first = writes[0], writes[k], writes[k + 1]
    pass1 = fp64(e1_last, e2_first)
    assert pass1 > 0 and sum(fp64(writes[j], writes[j + 1]) for j in range(len(writes) - 1) if j != k) * 4 < pass1, "the exchanges are not two blocks"
    # tw2: a whole pass 1 between request and wait
    d2 = fp64(groups["tw2"][-1], first_wait["tw2"])
    assert e1_last < groups["tw2"][0] and first_wait["tw2"] > e2_first
    assert d2 >= pass1, "tw2 is requested %d float64 instructions before its first wait, pass 1 has %d" % (d2, pass1)
    # tw1: right behind the first layer of pass 0, awaited behind the first exchange
    cvts = [i for i in range(e1_first) if loop[i][1].startswith("v_cvt_f64_f32")]
    assert len(cvts) >= 64, len(cvts)
    slip = fp64(cvts[-1], groups["tw1"][0])
    assert cvts[-1] < groups["tw1"][0] and slip <= LAYER1_GROUP, "tw1 is requested %d float64 instructions behind the last sample conversion" % slip
    rest0 = fp64(groups["tw1"][-1], e1_first)
    d1 = fp64(groups["tw1"][-1], first_wait["tw1"])
    assert first_wait["tw1"] > e1_last and d1 >= rest0 > 0
    assert rest0 * 2 > pass1, "pass 0 has %d float64 instructions left behind the tw1 request, pass 1 has %d" % (rest0, pass1)
    report = ["pass 1 = %d float64 instructions; tw1 %d behind the last conversion, %d ahead of its wait (rest of pass 0: %d, vmcnt %s); "
              "tw2 %d ahead (vmcnt %s)" % (pass1, slip, d1, rest0, vmcnts["tw1"], d2, vmcnts["tw2"])]
    # no vector-memory instruction under a lane condition: none between an exec-mask save (s_and_saveexec / s_or_saveexec ...) and the
    # s_or_b64 exec that restores it, and no v_cmpx anywhere in the loop
    regions, inside = [], False
    for off, mn, ops, _t in loop:
        if "saveexec" in mn:
            inside = True
            regions.append([])
        elif mn in ("s_or_b64", "s_mov_b64", "s_xor_b64", "s_andn2_b64") and ops.startswith("exec,"):
            inside = mn == "s_xor_b64" or mn == "s_andn2_b64"
        elif inside and _is_vmem(mn):
            regions[-1].append((mn, ops))
        assert not mn.startswith("v_cmpx"), (hex(off), mn)
    masked = [r for r in regions if r]
    # the one exception, there all along: lane 0's own store of the Nyquist bin - one buffer_store_dword per magnitude row (the same
    # address register, the two rows' buffer resources), once in each of the epilogue's two copies
    assert len(masked) <= 2, masked
    for r in masked:
        assert [mn for mn, _ops in r] == ["buffer_store_dword"] * 2, r
        (va, ra), (vb, rb) = [re.match(r"v\d+, (v\d+), (s\[\d+:\d+\])", ops).groups() for _mn, ops in r]
        assert va == vb and ra != rb, r
    print("%s: %d VGPRs, %d B scratch; frame loop %d instructions; %s" % (kernel, desc["vgpr"] + desc["agpr"], desc["scratch"], len(loop), "; ".join(report)))
