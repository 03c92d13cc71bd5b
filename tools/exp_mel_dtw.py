"""Developer tool: DTW-aligned mel-cepstral distortion on the GPU -> profiles/mel_dtw.json.
  1. the image-level call (ssr_spectrogram_mel_dtw: k_mel_schedule + k_mel_cepstra + k_mel_dtw) on 1024 resident image pairs of 4 s at
     48 kHz (AudioMetrics(48000): T = 401, F = 1115, NVSR's 128-band filterbank, n_cep = 13) for R in 0, 8, 16, 31: HIP-event time
     per call; next to it k_mel_metrics with mcd only on the same images (ssr_spectrogram_mel_metrics), the yardstick.  The split
     between k_mel_cepstra and k_mel_dtw comes from `rocprofv3 --kernel-trace --stats` runs of this tool, one per radius
     (DTW_RADII=<R> KERNELS_ONLY=1: the kernels of one radius only, so that the statistics of k_mel_dtw are that radius's), passed
     back in with KERNEL_STATS="R=path/to/kernel_stats.csv,...";
  2. the waveform-level call (backend.pair_mel_dtw: transforms + cepstra + warp, R = 16) on 1024 pairs of 4 s at 48 kHz, against
     backend.pair_mel_metrics with mcd only on the same pairs;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without mel_dtw=True, passes alternated.
Prints one JSON line (and writes it to OUT_DIR/mel_dtw.json when OUT_DIR is set)."""
import csv
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

RADII = tuple(int(r) for r in os.environ.get("DTW_RADII", "0,8,16,31").split(","))


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


def images():
    dev = torch.device("cuda", 0)
    am = AudioMetrics(48000)
    fb, n_cep = am.mel_filterbank()
    N, T, F = 1024, 401, am.n_fft // 2 + 1
    g = torch.Generator(device=dev).manual_seed(3)
    tgt = torch.rand((N, T, F), generator=g, device=dev, dtype=torch.float32)
    est = (tgt.roll(3, dims=1) * torch.exp(0.3 * torch.randn((N, T, F), generator=g, device=dev))).contiguous()      # three frames late
    return est, tgt, fb, n_cep


def image_level(kernels_only):
    est, tgt, fb, n_cep = images()
    N, T, F = (int(v) for v in est.shape)
    res = {"N": N, "T": T, "F": F, "n_cep": n_cep}
    reps = 3 if kernels_only else 10
    for R in RADII:
        res["ms_dtw_call_R%d" % R] = events_ms(lambda: B.spectrogram_mel_dtw(est, tgt, fb, n_cep, R), reps)
    res["ms_mel_metrics_mcd"] = events_ms(lambda: B.spectrogram_mel_metrics(est, tgt, fb, n_cep, 4), reps)
    return res


def kernel_stats(spec):
    """KERNEL_STATS="R=csv,..." -> {R: {kernel: average microseconds}} for the kernels of this family (rocprofv3 --stats columns
    Name, Calls, TotalDurationNs, AverageNs, ...)."""
    out = {}
    for item in filter(None, spec.split(",")):
        r, path = item.split("=", 1)
        rows = {}
        for row in csv.DictReader(open(path)):
            name = row.get("Name", "")
            if name.startswith(("k_mel_", "void k_mel_")):
                rows[name.split("(")[0]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
        out["R%s" % r] = rows
    return out


def waveform_level():
    dev = torch.device("cuda", 0)
    am = AudioMetrics(48000)
    fb, n_cep = am.mel_filterbank()
    plan = am._plan()
    n, L = 1024, 4 * 48000
    g = torch.Generator(device=dev).manual_seed(2)
    tg = torch.randn((n, L), generator=g, device=dev, dtype=torch.float32)
    es = tg.roll(1000, dims=1) + 0.3 * torch.randn((n, L), generator=g, device=dev, dtype=torch.float32)
    tl, el = list(tg.unbind(0)), list(es.unbind(0))
    return {"n": n, "ms_mel_dtw_R16": events_ms(lambda: B.pair_mel_dtw(plan, [el], tl, fb, n_cep, 16, deferred=True)(), 10),
            "ms_mel_metrics_mcd": events_ms(lambda: B.pair_mel_metrics(plan, [el], tl, fb, n_cep, 4, deferred=True)(), 10)}


def evaluate_tree():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    root = tempfile.mkdtemp(prefix="ssr_mel_dtw_")
    try:
        n_files = 0
        for s, c in enumerate([53, 53, 15, 52, 38, 53, 53, 50]):           # bench.py's evaluate_end_to_end tree
            os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
            for i in range(c):
                n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
                write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
                n_files += 1
        hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                    setting_fft={"cutoff_freq": [12000]}, mel_dtw=v) for name, v in (("plain", None), ("mel_dtw", True))}
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
    kernels_only = os.environ.get("KERNELS_ONLY") == "1"
    res = {"tool": "exp_mel_dtw", "radii": list(RADII), "image_level": image_level(kernels_only)}
    if os.environ.get("KERNEL_STATS"):
        res["kernels"] = kernel_stats(os.environ["KERNEL_STATS"])
    if not kernels_only:
        torch.cuda.empty_cache()
        res["waveform_level"] = waveform_level()
        torch.cuda.empty_cache()
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree()
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR") and not kernels_only:
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "mel_dtw.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
