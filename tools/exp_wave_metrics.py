"""Developer tool: SNR / SI-SDR / segmental SNR on the GPU.
  1. 1024 pairs of 4 s at 48 kHz in float32 (the cfg-2 shape), as K = 1 (1024 targets) and as 128 targets x 8 estimates: HIP-event
     time of ssr_wave_metrics per `which` (snr only; snr + seg_snr: pass 1 with its frames; all three: pass 1, pass 2) and of the
     public call (backend.wave_metrics) end to end; the split between kernels comes from a rocprofv3 --kernel-trace --stats run of
     this tool (k_wave_*);
  2. the bytes each pass must read ((n_tgt + n_est) x n samples) over its time, against bench.measured_hbm_peak() (the
     streaming-read ceiling of tools/ubench/hbm_probe.hip);
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without waveform=True, passes alternated.
Prints one JSON line (and writes it to OUT_DIR/exp_wave_metrics.json when OUT_DIR is set)."""
import ctypes as C
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
from ssr_eval_amd import _lib, backend as B  # noqa: E402
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


def run_case(n_tgt, k, n_samples, fs, read_gbs):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = torch.randn((n_tgt, n_samples), generator=g, device=dev, dtype=torch.float32)
    ests = tg.repeat_interleave(k, 0) + 0.3 * torch.randn((n_tgt * k, n_samples), generator=g, device=dev, dtype=torch.float32)
    tl, el = list(tg.unbind(0)), list(ests.unbind(0))
    idx = np.repeat(np.arange(n_tgt), k).astype(np.int32)
    n_est = len(el)
    lib = _lib.load()
    lens = np.full(n_tgt, n_samples, np.int32)
    toff = torch.arange(n_tgt, dtype=torch.int64, device=dev) * n_samples
    eoff = torch.arange(n_est, dtype=torch.int64, device=dev) * n_samples
    pinned = [torch.from_numpy(a).pin_memory() for a in (lens, idx)]
    res = {"n_tgt": n_tgt, "n_est": n_est}
    # bytes one pass must read: every target once, every estimate once (float32)
    pass_bytes = 4.0 * (n_tgt + n_est) * n_samples
    res["pass_bytes"] = pass_bytes
    for which, name in ((_lib.WAVE_SNR, "snr"), (_lib.WAVE_SNR | _lib.WAVE_SEG_SNR, "snr_seg"), (7, "all")):
        ws_bytes = int(lib.ssr_wave_metrics_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_tgt, idx.ctypes.data_as(C.c_void_p),
                                                            n_est, fs, which))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((n_est, 3), dtype=torch.float64, device=dev)

        def call():
            _lib.check(lib.ssr_wave_metrics(B._vp(tg), 0, B._vp(toff), C.c_void_p(pinned[0].data_ptr()), n_tgt, B._vp(ests), 0,
                                            B._vp(eoff), C.c_void_p(pinned[1].data_ptr()), n_est, fs, which, B._vp(out), B._vp(ws),
                                            ws_bytes, B._stream()))
        res["ms_" + name] = events_ms(call, 20)
    # the public path end to end (views of one buffer read where they lie, the copy of the values to the host)
    res["api_ms_all"] = events_ms(lambda: B.wave_metrics(tl, el, idx, fs, 7, dev, deferred=True)(), 10)
    # pass 1 alone (no moments, no frames) ~ ms_snr; pass 2 ~ ms_all - ms_snr_seg - the moments' share of pass 1 (kernel trace)
    res["pass1_snr_read_GBs"] = pass_bytes / (res["ms_snr"] * 1e-3) / 1e9
    if read_gbs:
        res["pass1_snr_share_of_read_ceiling"] = res["pass1_snr_read_GBs"] / read_gbs
        res["all_share_of_read_ceiling_2_passes"] = 2 * pass_bytes / (res["ms_all"] * 1e-3) / 1e9 / read_gbs
    return res


def evaluate_tree():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    root = tempfile.mkdtemp(prefix="ssr_wave_")
    try:
        n_files = 0
        for s, c in enumerate([53, 53, 15, 52, 38, 53, 53, 50]):           # bench.py's evaluate_end_to_end tree
            os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
            for i in range(c):
                n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
                write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
                n_files += 1
        hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                    setting_fft={"cutoff_freq": [12000]}, waveform=v) for name, v in (("plain", None), ("waveform", True))}
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
    fs, n_samples = 48000, 4 * 48000
    peak = bench.measured_hbm_peak()
    read_gbs = peak.get("read_GBs")
    res = {"tool": "exp_wave_metrics", "hbm_measured": peak, "k1": run_case(1024, 1, n_samples, fs, read_gbs)}
    torch.cuda.empty_cache()
    res["k8"] = run_case(128, 8, n_samples, fs, read_gbs)
    torch.cuda.empty_cache()
    if os.environ.get("SKIP_EVALUATE") != "1":
        res["evaluate"] = evaluate_tree()
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "exp_wave_metrics.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
