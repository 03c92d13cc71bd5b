"""GPU test (-m gpu) of the family registry of SSR_Eval_Helper (eval._FAMILIES): evaluate() on a small wav tree at 16 kHz with all
ten optional families on, through the multi path (two FFT cutoffs: K = 2 estimates per target) and through the flat batch path (one
cutoff: K = 1).  Every (speaker, file, key) lists its metrics in result_key_order(); every family's values are, bit for bit, those
of a run with that option alone, and the reference's four those of a run without any option.  There are no tolerances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 16000
REFERENCE = ("lsd", "log_sispec", "sispec", "ssim")
# option -> (a value that turns the family on, the keys it adds), in the order the families are queued
OPTIONS = {
    "lsd_split": (True, ("lsd_lf", "lsd_hf")),
    "stoi": ("both", ("stoi", "estoi")),
    "waveform": (True, ("snr", "si_sdr", "seg_snr")),
    "mel": (True, ("mel_lsd", "mel_l1", "mcd")),
    "mel_dtw": (True, ("mcd_dtw", "dtw_dev")),
    "quality": (True, ("llr", "cep_dist", "wss", "fwseg_snr")),
    "pitch": (True, ("f0_rmse", "f0_corr", "gpe", "vde", "ffe")),
    "phase": (True, ("phase_ip", "phase_gd", "phase_iaf")),
    "mrstft": (True, ("mrstft_sc", "mrstft_mag", "mrstft")),
    "bss_sdr": (True, ("sdr", "sdr_lag")),
}
LENGTHS = {"p360": (8000, 8411), "p361": (9001, 9600)}                    # 0.5 .. 0.6 s, no two alike


def bits(v):
    return np.float64(v).tobytes()                                        # NaN equals NaN


def write_tree(root):
    """Two speakers x two files: a 220 Hz tone with two harmonics (frames YIN calls voiced, bands STOI can score) plus noise."""
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(12)
    for spk, lens in LENGTHS.items():
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            t = np.arange(n) / FS
            x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 440 * t) + 0.05 * np.sin(2 * np.pi * 1760 * t)
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), (x + 0.02 * rng.standard_normal(n)).astype(np.float32), FS)


@pytest.mark.parametrize("cutoffs", [[2000, 3000], [2000]], ids=["K2-multi", "K1-batch"])
def test_all_families_together_are_each_family_alone(tmp_path, cutoffs):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.eval import _FAMILIES, result_key_order
    assert [f.option for f in _FAMILIES] == list(OPTIONS) and [f.keys for f in _FAMILIES] == [k for _, k in OPTIONS.values()]
    root = tmp_path / "vctk_test"
    write_tree(root)

    def run(**kw):
        h = SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(root),
                            setting_fft={"cutoff_freq": list(cutoffs)}, **kw)
        return h.evaluate(save_json=False)
    everything = run(**{o: v for o, (v, _) in OPTIONS.items()})
    none = run()
    alone = {o: run(**{o: v}) for o, (v, _) in OPTIONS.items()}
    keys = ["proc_fft_%d_%d" % (2 * c, FS) for c in cutoffs]
    order = result_key_order()
    seen = 0
    for spk in LENGTHS:
        assert len(everything[spk]) == 2
        for fn, by_key in everything[spk].items():
            assert list(by_key) == keys
            for key, d in by_key.items():
                assert list(d) == [k for k in order if k in d] and len(d) == len(order) == 33, (spk, fn, key, list(d))
                for m in REFERENCE:
                    assert bits(d[m]) == bits(none[spk][fn][key][m]), (spk, fn, key, m, d[m], none[spk][fn][key][m])
                assert list(none[spk][fn][key]) == list(REFERENCE)
                for option, (_, names) in OPTIONS.items():
                    one = alone[option][spk][fn][key]
                    assert list(one) == list(REFERENCE) + list(names), (option, list(one))
                    for m in names:
                        assert bits(d[m]) == bits(one[m]), (spk, fn, key, option, m, d[m], one[m])
                seen += 1
    assert seen == 4 * len(cutoffs)
    for key in keys:
        assert list(everything["averaged"][key]) == list(order)
        for spk in LENGTHS:
            assert list(everything["each_speaker"][spk][key]) == list(order)
