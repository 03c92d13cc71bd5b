"""GPU test (-m gpu) of every row of the family registry (eval._ALL_FAMILIES, 16 families, 56 keys in every_key_order()) in ONE
evaluate(): a 16 kHz tree of eight wav files over three speakers, 0.5 to 0.9 s long, no two lengths alike and written in ascending
order (every later batch of files needs larger buffers than the one before), with two key sets - "fft2+iir2": two FFT cutoffs and a
Butterworth and an elliptic low-pass, K = 4 keys per file with float32 and float64 estimates side by side (each dtype group takes its
own launch sequence), and "fft1": one FFT cutoff, K = 1, the flat batch path.

  1. with all 16 options on, every family's keys are those of a run with that option alone and the reference's four those of a run
     with no option, bit for bit; every (file, key), `averaged` and `each_speaker` list the 56 keys in every_key_order();
  2. evaluate(batch_files = 1, 3, 64) return identical results - with families on, batch N + 1 is queued before batch N's values
     are collected, through the descriptor ring, the cached device tables, the pinned result buffers and the per-call workspaces -
     and evaluate_single(file) is the file's entry;
  3. for every family and key, the IIR keys (float64 estimates) among them, the value is the family's AudioMetrics batch call on the
     arrays lowpass() returns for that key and the decoded file, bit for bit;
  4. every key name has a finite value somewhere in the tree.
The registry drives the test; the one table below holds the value that switches each option on (those of the families' own
evaluate() tests).  There are no tolerances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 16000
REFERENCE = ("lsd", "log_sispec", "sispec", "ssim")
ON = {"lsd_split": True, "stoi": "both", "waveform": True, "mel": True, "mel_dtw": True, "quality": True, "pitch": True, "phase": True,
      "mrstft": True, "bss_sdr": True, "coherence": True, "loudness": True, "bandwidth": True, "modulation": True, "auditory": True,
      "csii": True}
LENGTHS = {"p360": (8000, 8411, 9001), "p361": (9600, 10240, 11111), "p362": (12800, 14399)}      # ascending in evaluation order
# key set -> (the helper's settings, {key: (cutoff in Hz, lowpass() type, order)} in the order a file lists its keys)
KEY_SETS = {
    "fft2+iir2": (lambda: dict(setting_fft={"cutoff_freq": [2000, 3000]},
                               setting_lowpass_filtering={"cutoff_freq": [2000], "filter_order": [4], "filter": ["butter", "ellip"]}),
                  {"proc_bw_4000_4_16000": (2000, "butter", 4), "proc_el_4000_4_16000": (2000, "ellip", 4),
                   "proc_fft_4000_16000": (2000, "stft_hard", 1), "proc_fft_6000_16000": (3000, "stft_hard", 1)}),
    "fft1": (lambda: dict(setting_fft={"cutoff_freq": [2000]}), {"proc_fft_4000_16000": (2000, "stft_hard", 1)}),
}


def bits(v):
    """A result (nested dicts of floats) with every float as its bit pattern: NaN equals NaN, -0.0 is not 0.0; key order kept."""
    return [(k, bits(x)) for k, x in v.items()] if isinstance(v, dict) else np.float64(v).tobytes()


def write_tree(root):
    """The tone with two harmonics plus noise of tests/test_gpu_all_families.py under a stepped level (0, -6, 0, -20 dB in stretches
    of 0.1 s: the level classes of the csii family all hold segments) over a faint noise floor."""
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(16)
    gains = (1.0, 0.5, 1.0, 0.1)
    for spk, lens in LENGTHS.items():
        (root / spk).mkdir(parents=True)
        for i, n in enumerate(lens):
            t = np.arange(n) / FS
            x = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * np.sin(2 * np.pi * 440 * t) + 0.05 * np.sin(2 * np.pi * 1760 * t)
            env = np.array(gains)[(np.arange(n) // (FS // 10)) % len(gains)]
            write_wav(str(root / spk / ("%s_%03d_mic1.wav" % (spk, i))), (env * x + 0.005 * rng.standard_normal(n)).astype(np.float32), FS)


class Tree:
    """The wav tree of one key set and the evaluate() runs on it, each made once."""

    def __init__(self, root, name):
        self.root, (self.settings, self.keys) = root, KEY_SETS[name]
        self.runs = {}

    def helper(self, **options):
        from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
        # (the helper doubles the cutoff lists of its settings in place: fresh dicts for every helper)
        return SSR_Eval_Helper(BasicTestee(), test_name="t", input_sr=FS, output_sr=FS, evaluation_sr=FS, test_data_root=str(self.root),
                               **self.settings(), **options)

    def run(self, batch_files=None, **options):
        tag = (batch_files,) + tuple(sorted(options))
        if tag not in self.runs:
            self.runs[tag] = self.helper(**options).evaluate(save_json=False, batch_files=batch_files)
        return self.runs[tag]

    def everything(self):
        return self.run(**ON)


@pytest.fixture(scope="module", params=list(KEY_SETS))
def tree(request, tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    root = tmp_path_factory.mktemp("every_family") / "vctk_test"
    write_tree(root)
    lens = [n for spk in sorted(LENGTHS) for n in LENGTHS[spk]]
    assert len(lens) == 8 == len(set(lens)) and lens == sorted(lens) and 0.5 * FS <= lens[0] and lens[-1] <= 0.9 * FS
    return Tree(root, request.param)


def test_the_registry_is_the_one_this_file_switches_on():
    """A new row of the registry fails here until ON holds a value for its option."""
    from ssr_eval_amd.eval import _ALL_FAMILIES, every_key_order
    assert len(_ALL_FAMILIES) == 16 and [f.option for f in _ALL_FAMILIES] == list(ON)
    order = every_key_order()
    assert len(order) == 56 == len(set(order)) and order == REFERENCE + tuple(k for f in _ALL_FAMILIES for k in f.keys)


def test_every_family_together_is_each_family_alone(tree):
    from ssr_eval_amd.eval import _ALL_FAMILIES, every_key_order
    order = every_key_order()
    everything, none = tree.everything(), tree.run()
    alone = {f.option: tree.run(**{f.option: ON[f.option]}) for f in _ALL_FAMILIES}
    seen, finite = 0, set()
    for spk in LENGTHS:
        assert len(everything[spk]) == len(LENGTHS[spk])
        for fn, by_key in everything[spk].items():
            assert list(by_key) == list(tree.keys)
            for key, d in by_key.items():
                assert list(d) == list(order) and len(d) == 56, (spk, fn, key, list(d))
                assert list(none[spk][fn][key]) == list(REFERENCE)
                for m in REFERENCE:
                    assert bits(d[m]) == bits(none[spk][fn][key][m]), (spk, fn, key, m, d[m], none[spk][fn][key][m])
                for f in _ALL_FAMILIES:
                    one = alone[f.option][spk][fn][key]
                    assert list(one) == list(REFERENCE) + list(f.keys), (f.option, list(one))
                    for m in f.keys:
                        assert bits(d[m]) == bits(one[m]), (spk, fn, key, f.option, m, d[m], one[m])
                finite |= {m for m in order if np.isfinite(d[m])}
                seen += 1
    assert seen == 8 * len(tree.keys)
    assert finite == set(order), sorted(set(order) - finite)                  # no key is NaN against NaN throughout
    for key in tree.keys:
        assert list(everything["averaged"][key]) == list(order)
        for spk in LENGTHS:
            assert list(everything["each_speaker"][spk][key]) == list(order)


def test_every_family_on_does_not_depend_on_the_files_per_batch(tree):
    """batch_files = 1: eight batches, each queued before the one before it is collected; 3: the pipeline's fill (1, 1, 3, 3 files);
    64: one batch."""
    import os
    want = bits(tree.everything())
    for b in (1, 3, 64):
        got = tree.run(batch_files=b, **ON)
        assert list(got) == list(LENGTHS) + ["each_speaker", "averaged"]
        assert bits(got) == want, b
    # evaluate_single: the same keys in the same order, every metric the same bits (it lists a key's metrics as the families return
    # them; evaluate() sorts them into every_key_order())
    h = tree.helper(**ON)
    everything = tree.everything()
    for spk in LENGTHS:
        for fn in everything[spk]:
            got = h.evaluate_single(os.path.join(str(tree.root), spk, fn))
            assert list(got) == list(everything[spk][fn]), (spk, fn)
            for key, d in got.items():
                assert sorted(bits(d)) == sorted(bits(everything[spk][fn][key])) and len(d) == 56, (spk, fn, key)


def test_every_family_and_key_is_the_direct_call_on_the_same_arrays(tree):
    """getattr(AudioMetrics, family.batch)(estimates, targets, *family.arguments(helper, keys)) per key over the eight files: the
    estimates what lowpass() returns for the key (float64 for the IIR keys, float32 for the FFT keys), the targets the decoded files."""
    from ssr_eval_amd import AudioMetrics
    from ssr_eval_amd.eval import _ALL_FAMILIES
    from ssr_eval_amd.io import read_audio
    from ssr_eval_amd.lowpass import lowpass
    everything, h, am = tree.everything(), tree.helper(**ON), AudioMetrics(FS)
    files = [(spk, fn) for spk in LENGTHS for fn in everything[spk]]
    tgts = [np.asarray(read_audio(str(tree.root / spk / fn))[0], np.float32) for spk, fn in files]
    for key, (cut, kind, order) in tree.keys.items():
        ests = [lowpass(x, cut, FS, order=order, _type=kind) for x in tgts]
        ests = [np.asarray(e, np.float32 if kind == "stft_hard" else np.float64) for e in ests]
        assert all(e.dtype == (np.float32 if kind == "stft_hard" else np.float64) and len(e) == len(x) for e, x in zip(ests, tgts))
        for f in _ALL_FAMILIES:
            args, kw = f.arguments(h, [key] * len(files))
            want = getattr(am, f.batch)(ests, tgts, *args, **kw)
            for (spk, fn), w in zip(files, want):
                d = everything[spk][fn][key]
                for m in f.keys:
                    assert bits(d[m]) == bits(w[m]), (key, f.option, spk, fn, m, d[m], w[m])
