"""Developer tool: the band-split LSD (LSD-LF / LSD-HF) on the GPU.
  1. ssr_spectrogram_lsd_bands on resident magnitude images at the cfg-2 shape (1024 pairs x 4 s @ 48 kHz, 2048 / 512: 376 x 1025
     per image), split at 4 kHz (bin 170): HIP-event time per call;
  2. ssr_pair_lsd_bands (waveform level, K = 1) on the same pairs, next to ssr_pair_metrics with the LSD mask alone;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without lsd_split=True, passes alternated.
Prints one JSON line (and writes it to OUT_DIR/exp_lsd_bands.json when OUT_DIR is set)."""
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


def images(n, n_samples, cut):
    dev = torch.device("cuda", 0)
    T, F = 1 + n_samples // 512, 1025
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.rand((n, T, F), generator=g, device=dev)
    x = (y + 0.01 * torch.rand((n, T, F), generator=g, device=dev)).contiguous()
    lib = _lib.load()
    off = torch.arange(n, device=dev, dtype=torch.int64) * T
    rows = torch.full((n,), T, device=dev, dtype=torch.int32)
    edges = np.tile(np.array([0, cut, F], dtype=np.int32), (n, 1))
    pinned = torch.from_numpy(edges).pin_memory()
    out = torch.empty((n, 2), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_spectrogram_lsd_bands_workspace_bytes(n, T, 2))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.ssr_spectrogram_lsd_bands(B._vp(x), B._vp(off), B._vp(y), B._vp(off), B._vp(rows), n, T, F,
                                                 C.c_void_p(pinned.data_ptr()), 2, B._vp(out), B._vp(ws), ws_bytes, st))
    ms = events_ms(call, 20)
    return {"ms_per_call": round(ms, 4), "shape": [n, T, F], "image_GB_read": round(2 * x.numel() * 4 / 1e9, 3),
            "GB_per_s": round(2 * x.numel() * 4 / 1e9 / (ms / 1e3), 1)}


def waveform(n, n_samples, cut):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tgt = (0.1 * torch.randn((n, n_samples), generator=g, device=dev)).contiguous()
    est = (tgt + 0.01 * torch.randn((n, n_samples), generator=g, device=dev)).contiguous()
    plan = B.get_plan(2048, 512, "f64", dev)
    e, t = B.Ragged.from_uniform(est), B.Ragged.from_uniform(tgt)
    rows = B._Rows(plan, t.lens_host, dev)
    lib = plan.lib
    edges = np.tile(np.array([0, cut, plan.n_bins], dtype=np.int32), (n, 1))
    pinned = torch.from_numpy(edges).pin_memory()
    out = torch.empty((n, 1, 2), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_pair_lsd_bands_workspace_bytes(plan.handle, n, 1, t.max_len, rows.total, 2))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(lib.ssr_pair_lsd_bands(plan.handle, B._vp(e.data), B._vp(e.off), B._vp(t.data), B._vp(t.off), B._vp(t.len),
                                          B._vp(rows.off), n, 1, t.max_len, rows.total, C.c_void_p(pinned.data_ptr()), 2, B._vp(out),
                                          B._vp(ws), ws_bytes, st))
    ms = events_ms(call, 10)
    pb = B.PairBatch(plan, e, t)
    ms_lsd = events_ms(lambda: pb.run(B.M_LSD), 10)
    return {"ssr_pair_lsd_bands_ms": round(ms, 4), "ssr_pair_metrics_lsd_only_ms": round(ms_lsd, 4)}


def evaluate_tree():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    root = tempfile.mkdtemp(prefix="ssr_lsdb_")
    try:
        n_files = 0
        for s, c in enumerate([53, 53, 15, 52, 38, 53, 53, 50]):           # bench.py's evaluate_end_to_end tree
            os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
            for i in range(c):
                n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
                write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
                n_files += 1
        hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                    setting_fft={"cutoff_freq": [12000]}, lsd_split=v) for name, v in (("plain", None), ("lsd_split", True))}
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
    n, n_samples = int(os.environ.get("N_ITEMS", "1024")), 4 * 48000
    cut = int(1025 * (4000 / 24000))                                   # AudioMetrics.split_bin at the 2048-point plan: 170
    res = {"tool": "exp_lsd_bands", "split_bin": cut, "images": images(n, n_samples, cut)}
    torch.cuda.empty_cache()
    res["waveform"] = waveform(n, n_samples, cut)
    torch.cuda.empty_cache()
    res["evaluate"] = evaluate_tree()
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "exp_lsd_bands.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
