"""Developer tool: mel-spectrogram distances on the GPU.
  1. the image-level reduction (ssr_spectrogram_mel_metrics, all three metrics, NVSR-style 128-band HTK filterbank at 48 kHz:
     F = 1115) on 1024 resident image pairs of 4 s at 48 kHz (T = 401): HIP-event time, the bytes it must read (both images
     once) over that time, against bench.measured_hbm_peak() (the streaming-read ceiling of tools/ubench/hbm_probe.hip);
  2. the waveform-level call (backend.pair_mel_metrics: transforms + reduction) on 1024 pairs of 4 s at 48 kHz, against
     ssr_pair_metrics with the LSD mask alone (backend.pair_metrics) on the same pairs;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without mel=True, passes alternated.
Prints one JSON line (and writes it to OUT_DIR/exp_mel.json when OUT_DIR is set)."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ssr_eval_amd import AudioMetrics, backend as B  # noqa: E402
import bench  # noqa: E402


def events_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def image_level(read_gbs):
    dev = torch.device("cuda", 0)
    am = AudioMetrics(48000)
    fb, n_cep = am.mel_filterbank()
    N, T, F = 1024, 401, am.n_fft // 2 + 1
    g = torch.Generator(device=dev).manual_seed(3)
    tgt = torch.rand((N, T, F), generator=g, device=dev, dtype=torch.float32)
    est = (tgt * torch.exp(0.3 * torch.randn((N, T, F), generator=g, device=dev))).contiguous()
    res = {"N": N, "T": T, "F": F, "image_GB": N * T * F * 4 / 1e9}
    for which, name in ((7, "all"), (1, "mel_lsd"), (4, "mcd")):
        res["ms_" + name] = events_ms(lambda: B.spectrogram_mel_metrics(est, tgt, fb, n_cep, which), 10)
    res["ms_project"] = events_ms(lambda: B.spectrogram_mel(est, fb), 10)
    nbytes = 2 * N * T * F * 4
    res["read_TBs_all"] = nbytes / (res["ms_all"] * 1e-3) / 1e12
    res["read_TBs_project"] = nbytes / 2 / (res["ms_project"] * 1e-3) / 1e12
    if read_gbs:
        res["floor_ms"] = nbytes / (read_gbs * 1e9) * 1e3
        res["share_of_read_ceiling_all"] = res["read_TBs_all"] * 1e3 / read_gbs
    return res


def waveform_level():
    dev = torch.device("cuda", 0)
    am = AudioMetrics(48000)
    fb, n_cep = am.mel_filterbank()
    plan = am._plan()
    n, L = 1024, 4 * 48000
    g = torch.Generator(device=dev).manual_seed(2)
    tg = torch.randn((n, L), generator=g, device=dev, dtype=torch.float32)
    es = tg + 0.3 * torch.randn((n, L), generator=g, device=dev, dtype=torch.float32)
    tl, el = list(tg.unbind(0)), list(es.unbind(0))
    return {"n": n, "ms_mel_all": events_ms(lambda: B.pair_mel_metrics(plan, [el], tl, fb, n_cep, 7, deferred=True)(), 10),
            "ms_pair_metrics_lsd": events_ms(lambda: B.pair_metrics(plan, el, tl, B.M_LSD, deferred=True)(), 10)}


def evaluate_tree():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    root = tempfile.mkdtemp(prefix="ssr_mel_")
    try:
        n_files = 0
        for s, c in enumerate([53, 53, 15, 52, 38, 53, 53, 50]):           # bench.py's evaluate_end_to_end tree
            os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
            for i in range(c):
                n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
                write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
                n_files += 1
        hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                    setting_fft={"cutoff_freq": [12000]}, mel=v) for name, v in (("plain", None), ("mel", True))}
        for h in hs.values():
            h.evaluate(limit_test_nums=2, limit_test_speaker=1, save_json=False)
            h.evaluate(save_json=False)
        times = {k: [] for k in hs}
        for _ in range(5):
            for k, h in hs.items():
                t0 = time.perf_counter()
                h.evaluate(save_json=False)
                times[k].append(time.perf_counter() - t0)
        return {k: {"files_per_s": round(n_files / float(np.median(v)), 1), "pass_s": [round(x, 4) for x in v]} for k, v in times.items()} | \
            {"n_files": n_files}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    peak = bench.measured_hbm_peak()
    res = {"tool": "exp_mel", "hbm_measured": peak, "image_level": image_level(peak.get("read_GBs"))}
    torch.cuda.empty_cache()
    res["waveform_level"] = waveform_level()
    torch.cuda.empty_cache()
    if os.environ.get("SKIP_EVALUATE") != "1":
        res["evaluate"] = evaluate_tree()
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "exp_mel.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
