"""CPU test of the seven later per-pair families - bss, coherence, spectrum, auditory, modulation, csii, loudness - on the large batch
of tests/pairs_batch.py (2 NT + 3 pairs, four length classes per family, per-pair parameters from a cycle of period 7), through their
kernel bodies compiled for the host (tests/emu/*_emu.cpp, the build fixtures and runners of the families' own host tests): the
families' own count functions, per-pair parameter arrays and ssr_run_geometry_body at c = 3 pairs per thread.  The batch equals its
sub-batches of at most 64 pairs bit for bit, with and without the optional outputs; a repeated call repeats the bits; the pairs at
the seams of the geometry (0, NT - 1, NT, NT + 1, 2 NT + 2, the target two runs name) meet the family's float64 oracle at the bars of
its own tests.  tests/test_gpu_pairs_batch.py runs the same checks on the device: a failure there that this file does not show lies
in device-specific code."""
import pytest

import pairs_batch as PB
import test_auditory_host
import test_bss_host
import test_coherence_host
import test_csii_host
import test_loudness_host
import test_modulation_host
import test_spectrum_host
from test_auditory_host import emu as auditory_emu              # noqa: F401  (the families' module-scoped emulation builds)
from test_bss_host import emu as bss_emu                        # noqa: F401
from test_coherence_host import emu as coherence_emu            # noqa: F401
from test_csii_host import emu as csii_emu                      # noqa: F401
from test_loudness_host import emu as loudness_emu              # noqa: F401
from test_modulation_host import emu as modulation_emu          # noqa: F401
from test_spectrum_host import emu as spectrum_emu              # noqa: F401


def runner(name, lib):
    """run(batch, opt) of pairs_batch.check_family through the family's emulation library"""
    if name == "bss":
        return lambda b, opt: test_bss_host.run_emu(lib, b.tgts, b.ests, b.idx, b.cfg["taps"], filt=opt)
    if name == "coherence":
        return lambda b, opt: test_coherence_host.run_emu(lib, b.tgts, b.ests, b.idx, b.cfg["N"], b.cfg["H"], b.par["bands"], b.cfg["thr"],
                                                          spectrum=opt)
    if name == "spectrum":
        return lambda b, opt: test_spectrum_host.run(PB.case_spectrum(b), lib, ltas=opt, gap=2, debug=False)
    if name == "auditory":
        return lambda b, opt: test_auditory_host.run(PB.case_auditory(b), lib, bands=opt, images=opt)
    if name == "modulation":
        return lambda b, opt: test_modulation_host.run(PB.case_modulation(b), lib, spec=opt)
    if name == "csii":
        return lambda b, opt: test_csii_host.run_emu(lib, b.tgts, b.ests, b.idx, b.cfg["fs"], b.cfg["N"], b.cfg["H"], splits=b.par["splits"],
                                                     with_bands=opt)
    return lambda b, opt: test_loudness_host.run_emu(lib, b.ests, b.cfg["fs"], blocks=opt, gap=1)


@pytest.mark.parametrize("name", PB.NAMES)
def test_emulated_large_batch_equals_its_sub_batches_and_meets_the_oracle(request, name):
    lib = request.getfixturevalue(name + "_emu")
    check = (lambda b, o: PB.check_bss(b, o, test_bss_host.check_rows)) if name == "bss" else PB.CHECK[name]
    PB.check_family(name, runner(name, lib), check)
