"""Developer tool: YIN F0 tracking and the pitch pair metrics on the GPU.
  1. 1024 pairs of 4 s at 48 kHz in float32, as K = 1 (1024 targets) and as 128 targets x 8 estimates: HIP-event time of the
     resampling to 16 kHz (one ssr_resample_poly_f64 launch for targets and estimates), of the tracker alone (ssr_f0_track on every
     distinct signal), of ssr_f0_metrics (tracks + voicing + pair statistics; the pair statistics are the difference), and of the
     public call (backend.pitch_metrics) end to end;
  2. the tracker time against the FP64 floor of the direct-form difference function: signals x frames x tau_hi x W terms, each one
     float64 subtract and one FMA - two FP64 vector instructions, counted at the FMA rate of the 78.6 TFLOP/s vector peak;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without pitch=True, passes alternated.
Prints one JSON line (and writes it to OUT_DIR/exp_pitch.json when OUT_DIR is set).  SKIP_EVALUATE=1 skips part 3."""
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

FP64_VECTOR_PEAK = 78.6e12
W, TAU_HI = 400, 320          # the integration window and ceil(16000 / 50)


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


def run_case(n_tgt, k, n_samples, fs):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    t = torch.arange(n_samples, device=dev, dtype=torch.float64) / fs
    f0 = 100.0 + 150.0 * torch.rand((n_tgt, 1), generator=g, device=dev, dtype=torch.float64)
    tg = sum((0.6 ** h) * torch.sin(2 * torch.pi * (h + 1) * f0 * t) for h in range(6)).float()
    tg = tg + 0.01 * torch.randn((n_tgt, n_samples), generator=g, device=dev, dtype=torch.float32)
    ests = tg.repeat_interleave(k, 0) + 0.05 * torch.randn((n_tgt * k, n_samples), generator=g, device=dev, dtype=torch.float32)
    tl, el = list(tg.unbind(0)), list(ests.unbind(0))
    idx = np.repeat(np.arange(n_tgt), k).astype(np.int32)
    n_est = len(el)
    lib = _lib.load()
    r = B.resample_to_pitch_rate(tl + el, fs, dev)
    lens = r.lens_host.astype(np.int32)
    n16 = int(lens[0])
    T = B.pitch_frames(n16)
    res = {"n_tgt": n_tgt, "n_est": n_est, "n16": n16, "frames_per_signal": T}
    res["resample_ms"] = events_ms(lambda: B.resample_to_pitch_rate(tl + el, fs, dev), 5)
    n_sig = n_tgt + n_est
    pin = [torch.from_numpy(a).pin_memory() for a in (lens, idx)]
    foff = torch.arange(n_sig, dtype=torch.int64, device=dev) * T
    f0o, apo, eno = (torch.empty(n_sig * T, dtype=torch.float64, device=dev) for _ in range(3))
    vo = torch.empty(n_sig * T, dtype=torch.uint8, device=dev)
    ws_t = int(lib.ssr_f0_track_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_sig, 50.0, 500.0))
    wst = torch.empty(ws_t, dtype=torch.uint8, device=dev)

    def track():
        _lib.check(lib.ssr_f0_track(B._vp(r.data), B._vp(r.off), C.c_void_p(pin[0].data_ptr()), n_sig, 50.0, 500.0, B._vp(f0o),
                                    B._vp(apo), B._vp(eno), B._vp(vo), B._vp(foff), B._vp(wst), ws_t, B._stream()))
    res["track_ms"] = events_ms(track, 5)
    ws_m = int(lib.ssr_f0_metrics_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_tgt, idx.ctypes.data_as(C.c_void_p), n_est,
                                                  50.0, 500.0, 31))
    wsm = torch.empty(ws_m, dtype=torch.uint8, device=dev)
    out = torch.empty((n_est, 5), dtype=torch.float64, device=dev)

    def metrics():
        _lib.check(lib.ssr_f0_metrics(B._vp(r.data), B._vp(r.off), C.c_void_p(pin[0].data_ptr()), n_tgt, B._vp(r.data),
                                      B._vp(r.off[n_tgt:]), C.c_void_p(pin[1].data_ptr()), n_est, 50.0, 500.0, 31, B._vp(out), B._vp(wsm),
                                      ws_m, B._stream()))
    res["metrics_ms"] = events_ms(metrics, 5)
    res["pair_stats_ms"] = res["metrics_ms"] - res["track_ms"]
    res["api_ms"] = events_ms(lambda: B.pitch_metrics(tl, el, idx, fs, 31, 50.0, 500.0, dev, deferred=True)(), 3)
    terms = float(n_sig) * T * TAU_HI * W
    res["terms"] = terms
    res["fp64_floor_ms"] = terms * 2 * 2 / FP64_VECTOR_PEAK * 1e3
    res["track_over_floor"] = res["track_ms"] / res["fp64_floor_ms"]
    return res


def evaluate_tree():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    root = tempfile.mkdtemp(prefix="ssr_pitch_")
    try:
        n_files = 0
        for s, c in enumerate([53, 53, 15, 52, 38, 53, 53, 50]):           # bench.py's evaluate_end_to_end tree
            os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
            for i in range(c):
                n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
                write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
                n_files += 1
        hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                    setting_fft={"cutoff_freq": [12000]}, pitch=v) for name, v in (("plain", None), ("pitch", True))}
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
    res = {"tool": "exp_pitch", "k1": run_case(1024, 1, n_samples, fs)}
    torch.cuda.empty_cache()
    res["k8"] = run_case(128, 8, n_samples, fs)
    torch.cuda.empty_cache()
    if os.environ.get("SKIP_EVALUATE") != "1":
        res["evaluate"] = evaluate_tree()
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "exp_pitch.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
