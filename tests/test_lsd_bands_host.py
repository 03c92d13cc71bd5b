"""CPU tests of the band-split LSD (LSD-LF / LSD-HF): key -> cutoff parsing, the split bin, the C ABI's argument checks (they
return before anything touches a device, so they run without a GPU)."""
import ctypes as C

import numpy as np
import pytest

CUTOFFS_HZ = [1000, 2000, 4000, 6000, 8000, 12000, 16000]       # bench.py's cutoff sweep


def test_key_cutoffs_for_every_key_family():
    from ssr_eval_amd.eval import key_cutoff_hz
    assert key_cutoff_hz("proc_bw_8000_4_44100") == 4000
    assert key_cutoff_hz("proc_fft_24000_44100") == 12000
    assert key_cutoff_hz("proc_fft_44099_44100") == 22049             # sr - 1 quirk, floor-divided
    assert key_cutoff_hz("proc_subsampling_16000_44100") == 8000
    assert key_cutoff_hz("proc_ch_11025_8_44100") == 5512
    assert key_cutoff_hz("proc_el_4000_10_16000") == 2000
    assert key_cutoff_hz("proc_bessel_12000_2_44100") == 6000
    assert key_cutoff_hz("proc_mp3_64_44100") is None
    assert key_cutoff_hz("proc_mp3_320_48000") is None


def test_helper_split_setting():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    mk = lambda v: SSR_Eval_Helper(BasicTestee(), 44100, 44100, test_data_root=None, lsd_split=v)      # noqa: E731
    own, fixed = mk(True), mk(3000)
    assert own.split_cutoff_hz("proc_fft_16000_44100") == 8000 and own.split_cutoff_hz("proc_mp3_64_44100") is None
    assert fixed.split_cutoff_hz("proc_fft_16000_44100") == 3000.0 and fixed.split_cutoff_hz("proc_mp3_64_44100") == 3000.0
    assert mk(None).lsd_split is None
    for bad in (False, "8k", [4000]):
        with pytest.raises(ValueError):
            mk(bad)


def test_helper_metric_order_puts_the_split_after_the_reference_four():
    from ssr_eval_amd.eval import _METRIC_KEYS
    assert _METRIC_KEYS[:6] == ("lsd", "log_sispec", "sispec", "ssim", "lsd_lf", "lsd_hf")


@pytest.mark.parametrize("rate,F", [(44100, 1025), (48000, 1115), (16000, 372)])
def test_split_bin_from_the_formula(rate, F):
    from ssr_eval_amd import AudioMetrics
    am = AudioMetrics(rate)
    assert am.n_fft // 2 + 1 == F
    for c in CUTOFFS_HZ:
        assert am.split_bin(c) == int(F * (c / (rate / 2)))
    assert AudioMetrics(48000).split_bin(4000) == 185 and AudioMetrics(44100).split_bin(12000) == 557
    # the split's edges, and the empty sides that become NaN
    am = AudioMetrics(16000)
    assert am._split_edges(4000) == ((0, 186, 372), (0, 1))
    assert am._split_edges(8000) == ((0, 372), (0, None))           # cutoff at the evaluation Nyquist: no high band
    assert am._split_edges(12000) == ((0, 372), (0, None))
    assert am._split_edges(0) == ((0, 372), (None, 0))
    assert am._split_edges(None) == (None, (None, None))
    d = am._split_dict([0.5], (0, None))
    assert d["lsd_lf"] == 0.5 and np.isnan(d["lsd_hf"])


# ---- C ABI argument checks (no device call happens before any of these errors) ----------------------------------------------
def _lib():
    from ssr_eval_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.ssr_last_error().decode()


_DUMMY = C.c_void_p(0x1000)       # never dereferenced: every call below fails its host-side checks first


def _spec(lib, edges, n_images=2, n_bins=16, n_bands=None, ws=_DUMMY, ws_bytes=1 << 20, est=_DUMMY, out=_DUMMY):
    e = np.ascontiguousarray(edges, dtype=np.int32)
    nb = e.shape[-1] - 1 if n_bands is None else n_bands
    return lib.ssr_spectrogram_lsd_bands(est, _DUMMY, _DUMMY, _DUMMY, _DUMMY, n_images, 4, n_bins,
                                         e.ctypes.data_as(C.c_void_p), nb, out, ws, ws_bytes, None)


def test_spectrogram_lsd_bands_rejects_bad_edges():
    lib = _lib()
    from ssr_eval_amd._lib import ERR_INVALID_ARG
    assert _spec(lib, [[0, 8, 16], [0, 8, 8]]) == ERR_INVALID_ARG and "strictly ascending" in _err(lib)
    assert _spec(lib, [[0, 8, 16], [0, 9, 8]]) == ERR_INVALID_ARG and "strictly ascending" in _err(lib)
    assert _spec(lib, [[0, 8, 17], [0, 8, 16]]) == ERR_INVALID_ARG and "exceeds n_bins" in _err(lib)
    assert _spec(lib, [[-1, 8, 16], [0, 8, 16]]) == ERR_INVALID_ARG and ">= 0" in _err(lib)


def test_spectrogram_lsd_bands_rejects_band_counts_nulls_and_small_workspaces():
    lib = _lib()
    from ssr_eval_amd._lib import ERR_INVALID_ARG, ERR_WORKSPACE, MAX_BANDS
    ok = [[0, 8, 16], [0, 1, 16]]
    assert _spec(lib, ok, n_bands=0) == ERR_INVALID_ARG and "n_bands" in _err(lib)
    many = np.tile(np.arange(MAX_BANDS + 2, dtype=np.int32), (2, 1))
    assert _spec(lib, many, n_bins=64) == ERR_INVALID_ARG and "n_bands" in _err(lib)
    assert _spec(lib, ok, est=None) == ERR_INVALID_ARG and "null" in _err(lib)
    assert _spec(lib, ok, out=None) == ERR_INVALID_ARG and "null" in _err(lib)
    need = lib.ssr_spectrogram_lsd_bands_workspace_bytes(2, 4, 2)
    assert need > 0 and lib.ssr_spectrogram_lsd_bands_workspace_bytes(2, 4, MAX_BANDS + 1) == 0
    assert _spec(lib, ok, ws_bytes=need - 1) == ERR_WORKSPACE and "workspace" in _err(lib)
    assert _spec(lib, ok, ws=None) == ERR_WORKSPACE and "workspace" in _err(lib)
    assert lib.ssr_spectrogram_lsd_bands(_DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, 1, 4, 16, None, 1, _DUMMY, _DUMMY, 1 << 20,
                                         None) == ERR_INVALID_ARG and "null" in _err(lib)


@pytest.mark.parametrize("name", ["ssr_pair_lsd_bands", "ssr_pair_lsd_bands_est64"])
def test_pair_lsd_bands_rejects_null_plan_and_band_counts(name):
    lib = _lib()
    from ssr_eval_amd._lib import ERR_INVALID_ARG
    fn = getattr(lib, name)
    e = np.array([0, 8, 16], dtype=np.int32)
    args = lambda plan, nb: (plan, _DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, _DUMMY, 1, 1, 4096, 9,        # noqa: E731
                             e.ctypes.data_as(C.c_void_p), nb, _DUMMY, _DUMMY, 1 << 20, None)
    assert fn(*args(None, 2)) == ERR_INVALID_ARG and "null" in _err(lib)
    assert fn(*args(_DUMMY, 0)) == ERR_INVALID_ARG and "n_bands" in _err(lib)
    assert fn(*args(_DUMMY, 9)) == ERR_INVALID_ARG and "n_bands" in _err(lib)
    assert lib.ssr_pair_lsd_bands_workspace_bytes(None, 1, 1, 4096, 9, 2) == 0
