"""Developer tool: LLR, LPC cepstral distance, WSS and fwSNRseg on the GPU.
  1. 1024 pairs of 4 s at 48 kHz in float32 (the cfg-2 shape), as K = 1 (1024 targets) and as 128 targets x 8 estimates: HIP-event
     time of ssr_quality_metrics per leg (LPC only: llr + cep_dist; bands only: wss + fwseg_snr; all four) and of the public call
     (backend.quality_metrics) end to end;
  2. the all-four time against the FP64 floor of the arithmetic: per frame of each signal a packed N-point FFT (half of
     5 N log2 N) and the P + 1 lags (2 L (P + 1)), over the 78.6 TFLOP/s FP64 vector peak;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without quality=True, passes alternated.
Prints one JSON line (and writes it to OUT_DIR/exp_quality.json when OUT_DIR is set)."""
import ctypes as C
import json
import math
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

FP64_VECTOR_PEAK = 78.6e12


def events_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def floor_ms(n_signals_frames, fs, P):
    L = (3 * fs + 50) // 100
    N = 1 << math.ceil(math.log2(2 * L))
    flop = n_signals_frames * (0.5 * 5 * N * math.log2(N) + 2 * L * (P + 1))
    return flop, flop / FP64_VECTOR_PEAK * 1e3


def run_case(n_tgt, k, n_samples, fs):
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
    L = (3 * fs + 50) // 100
    M = (n_samples - L) // (L // 4)
    res = {"n_tgt": n_tgt, "n_est": n_est, "frames_per_pair": M}
    for which, name in ((3, "lpc"), (12, "bands"), (15, "all")):
        ws_bytes = int(lib.ssr_quality_metrics_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_tgt, idx.ctypes.data_as(C.c_void_p),
                                                               n_est, fs, 0, which))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty((n_est, 4), dtype=torch.float64, device=dev)

        def call():
            _lib.check(lib.ssr_quality_metrics(B._vp(tg), 0, B._vp(toff), C.c_void_p(pinned[0].data_ptr()), n_tgt, B._vp(ests), 0,
                                               B._vp(eoff), C.c_void_p(pinned[1].data_ptr()), n_est, fs, 0, which, B._vp(out),
                                               B._vp(ws), ws_bytes, B._stream()))
        res["ms_" + name] = events_ms(call, 5)
    res["api_ms_all"] = events_ms(lambda: B.quality_metrics(tl, el, idx, fs, 15, 0, dev, deferred=True)(), 3)
    flop, fl = floor_ms((n_tgt + n_est) * M, fs, 16)
    res["fp64_flop"] = flop
    res["fp64_floor_ms"] = fl
    res["all_over_floor"] = res["ms_all"] / fl
    return res


def evaluate_tree():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    root = tempfile.mkdtemp(prefix="ssr_quality_")
    try:
        n_files = 0
        for s, c in enumerate([53, 53, 15, 52, 38, 53, 53, 50]):           # bench.py's evaluate_end_to_end tree
            os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
            for i in range(c):
                n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
                write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
                n_files += 1
        hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                    setting_fft={"cutoff_freq": [12000]}, quality=v) for name, v in (("plain", None), ("quality", True))}
        for h in hs.values():
            h.evaluate(limit_test_nums=2, limit_test_speaker=1, save_json=False)
            h.evaluate(save_json=False)
        times = {k: [] for k in hs}
        for _ in range(3):
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
    res = {"tool": "exp_quality", "k1": run_case(1024, 1, n_samples, fs)}
    torch.cuda.empty_cache()
    res["k8"] = run_case(128, 8, n_samples, fs)
    torch.cuda.empty_cache()
    if os.environ.get("SKIP_EVALUATE") != "1":
        res["evaluate"] = evaluate_tree()
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "exp_quality.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
