"""ISA guard of k_stft_wave's stash-and-flush epilogue, CPU-only, on the gfx950 code object inside the SHIPPED libssrhip.so (in the manner
of tests/test_stft_wave_isa.py, whose disassembler it uses): in every instantiation that takes the new path (ssr_stft_wave.h:
ssr_stft_wave_stash - all but the two float64 ones with running sums) the frame loop holds

* no vector-memory instruction under a lane condition (lane 0's two stores of the Nyquist bin were the only ones), and
* no float64 reciprocal, reciprocal square root or square root (the close of the previous frame's LSD was the only user),

and the flush that took them over is outside the loop: the kernel still has its float64 division and square root (v_rcp_f64 and the
root's v_rsq_f64 seed), behind the loop's backward branch.
The two instantiations that keep the frame-by-frame code are asserted to still have both inside the loop - if they ever fit the stash,
this test says so."""
import pytest

from test_stft_wave_isa import _disassemble, _is_vmem

STASH = [("double", "false", "false"), ("double", "false", "true")] + [("float", s, m) for s in ("false", "true") for m in ("false", "true")]
KEPT = [("double", "true", "false"), ("double", "true", "true")]
TABLE_LOADS = 15                                  # tw1: three, tw2: twelve - one load each of 16 (float64) or 8 (float32) bytes
FP64_SLOW = ("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64")


def _name(v):
    return "k_stft_wave<%s, %s, true, %s>" % v


def _frame_loop(insts, kernel, t):
    load = "buffer_load_dwordx4" if t == "double" else "buffer_load_dwordx2"
    loops = []
    for off, mn, _ops, target in insts:
        if mn.startswith(("s_cbranch", "s_branch")) and target is not None and target <= off:
            body = [i for i in insts if target <= i[0] <= off]
            if sum(i[1].startswith(load) for i in body) >= TABLE_LOADS:
                loops.append(body)
    assert loops, "no loop of %s holds the table loads" % kernel
    return min(loops, key=len)


def _masked_vmem(loop):
    """vector-memory instructions between an exec-mask save and the instruction that restores exec (tests/test_stft_wave_isa.py)"""
    found, inside = [], False
    for off, mn, ops, _t in loop:
        if "saveexec" in mn:
            inside = True
        elif mn in ("s_or_b64", "s_mov_b64", "s_xor_b64", "s_andn2_b64") and ops.startswith("exec,"):
            inside = mn == "s_xor_b64" or mn == "s_andn2_b64"
        elif inside and _is_vmem(mn):
            found.append((hex(off), mn, ops))
        assert not mn.startswith("v_cmpx"), (hex(off), mn)
    return found


@pytest.mark.parametrize("variant", STASH, ids=_name)
def test_frame_loop_has_no_one_lane_store_and_no_float64_root(tmp_path, variant):
    kernel = _name(variant)
    insts, desc = _disassemble(tmp_path, kernel)
    assert desc["scratch"] == 0 and desc["vgpr_spill"] == 0 and desc["vgpr"] + desc["agpr"] <= 256, desc
    loop = _frame_loop(insts, kernel, variant[0])
    assert _masked_vmem(loop) == []
    slow = [(hex(o), mn) for o, mn, _ops, _t in loop if mn.startswith(FP64_SLOW)]
    assert slow == [], slow
    end = loop[-1][0]
    behind = [mn for o, mn, _ops, _t in insts if o > end and mn.startswith(FP64_SLOW)]
    assert any(mn.startswith("v_rcp_f64") for mn in behind) and any(mn.startswith(("v_rsq_f64", "v_sqrt_f64")) for mn in behind), \
        "%s: no float64 division and square root behind the frame loop - where is the flush?" % kernel
    valu = sum(mn.startswith("v_") for _o, mn, _ops, _t in loop)
    print("%s: %d VGPRs; frame loop %d instructions, %d of them VALU; %d float64 reciprocal / root seeds behind it"
          % (kernel, desc["vgpr"] + desc["agpr"], len(loop), valu, len(behind)))


@pytest.mark.parametrize("variant", KEPT, ids=_name)
def test_variants_without_the_stash_are_the_frame_by_frame_code(tmp_path, variant):
    kernel = _name(variant)
    insts, desc = _disassemble(tmp_path, kernel)
    assert desc["scratch"] == 0 and desc["vgpr_spill"] == 0, desc
    loop = _frame_loop(insts, kernel, variant[0])
    assert any(mn.startswith(FP64_SLOW) for _o, mn, _ops, _t in loop), "%s takes the stash now: move it to STASH" % kernel
