"""Developer tool: STOI / ESTOI on the GPU.
  1. 1024 pairs of 4 s at 48 kHz (the cfg-2 shape), as K = 1 (1024 targets) and as 128 targets x 8 estimates: HIP-event time of
     the resampling leg (ssr_resample_poly_f64 with the Octave taps, targets and estimates in one launch) and of ssr_stoi
     (geometry, energy, vad, bands, segments, finalize) for STOI, ESTOI and both;
     the split of ssr_stoi between its kernels comes from a rocprofv3 --kernel-trace --stats run of this tool (k_stoi_*);
  2. FLOP and byte counts of each stage from the shapes, and the share of the FP64 vector peak (78.6 TFLOP/s, public spec);
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with
     and without stoi="both", passes alternated.
Prints one JSON line (and writes it to OUT_DIR/exp_stoi.json when OUT_DIR is set)."""
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

FP64_PEAK = 78.6e12


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


def shapes(n_tgt, n_est, n10k, taps_per_phase, n_in):
    """FLOP / byte counts per call from the shapes (all frames kept: the upper bound of the bands and segment stages)."""
    sig = n_tgt + n_est
    frames = (n10k - 256 + 127) // 128
    T = frames - 1
    J = max(T - 29, 0)
    return {
        "resample": {"flop": 2.0 * sig * n10k * taps_per_phase, "bytes": 8.0 * sig * (n_in + n10k)},
        "energy": {"flop": 3.0 * n_tgt * frames * 256, "bytes": 8.0 * n_tgt * frames * 256},
        "bands": {"flop": sig * T * (5.0 * 512 * 9 + 8 * 256 + 2 * 257), "bytes": 8.0 * sig * T * (512 + 15)},
        "segments": {"flop": n_est * J * (15 * 30 * 12.0 + 30 * 15 * 14.0), "bytes": 8.0 * n_est * (T + 29 * (J // 64 + 1)) * 30},
    }


def run_case(n_tgt, k, n_samples, fs):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = torch.randn((n_tgt, n_samples), generator=g, device=dev, dtype=torch.float32)
    ests = tg.repeat_interleave(k, 0) + 0.3 * torch.randn((n_tgt * k, n_samples), generator=g, device=dev, dtype=torch.float32)
    tl, el = list(tg.unbind(0)), list(ests.unbind(0))
    idx = np.repeat(np.arange(n_tgt), k)
    sp = B.StoiResamplePlan.get(fs, dev)
    r = B.Ragged.from_list(tl + el, dev, torch.float64)
    res = {"n_tgt": n_tgt, "n_est": n_tgt * k}
    res["resample_ms"] = events_ms(lambda: B.resample_to_stoi_rate(r, fs, dev), 10)
    r10 = B.resample_to_stoi_rate(r, fs, dev)
    n10k = int(r10.lens_host[0])
    lib = _lib.load()
    lens = r10.lens_host.astype(np.int32)
    i32 = idx.astype(np.int32)
    import ctypes as C
    ws_bytes = int(lib.ssr_stoi_workspace_bytes(lens[:n_tgt].ctypes.data_as(C.c_void_p), n_tgt, i32.ctypes.data_as(C.c_void_p), len(el)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    pinned = [torch.from_numpy(a).pin_memory() for a in (lens[:n_tgt].copy(), lens[n_tgt:].copy(), i32)]
    for which, name in ((_lib.STOI, "stoi"), (_lib.ESTOI, "estoi"), (_lib.STOI_BOTH, "both")):
        out = torch.empty((len(el), 2), dtype=torch.float64, device=dev)

        def call():
            _lib.check(lib.ssr_stoi(B._vp(r10.data), B._vp(r10.off), C.c_void_p(pinned[0].data_ptr()), n_tgt, B._vp(r10.data),
                                    B._vp(r10.off[n_tgt:]), C.c_void_p(pinned[1].data_ptr()), C.c_void_p(pinned[2].data_ptr()),
                                    len(el), which, B._vp(out), B._vp(ws), ws_bytes, B._stream()))
        res["ssr_stoi_ms_" + name] = events_ms(call, 10)
    # the public path end to end (resampling + ssr_stoi + the copy to the host), both measures
    res["stoi_api_ms_both"] = events_ms(lambda: B.stoi(tl, el, idx, fs, _lib.STOI_BOTH, dev, deferred=True), 5)
    hpp = -(-int(sp.taps64.numel()) // sp.up)
    sh = shapes(n_tgt, len(el), n10k, hpp, n_samples)
    sh["resample"]["ms"] = res["resample_ms"]
    for v in sh.values():
        if "ms" in v:
            v["share_fp64_peak"] = v["flop"] / (v["ms"] * 1e-3) / FP64_PEAK
            v["tb_per_s"] = v["bytes"] / (v["ms"] * 1e-3) / 1e12
    res["shapes"] = sh
    return res


def evaluate_tree():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    root = tempfile.mkdtemp(prefix="ssr_stoi_")
    try:
        n_files = 0
        for s, c in enumerate([53, 53, 15, 52, 38, 53, 53, 50]):           # bench.py's evaluate_end_to_end tree
            os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
            for i in range(c):
                n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
                write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
                n_files += 1
        hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                    setting_fft={"cutoff_freq": [12000]}, stoi=v) for name, v in (("plain", None), ("stoi_both", "both"))}
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
    res = {"tool": "exp_stoi", "k1": run_case(1024, 1, n_samples, fs)}
    torch.cuda.empty_cache()
    res["k8"] = run_case(128, 8, n_samples, fs)
    torch.cuda.empty_cache()
    if os.environ.get("SKIP_EVALUATE") != "1":
        res["evaluate"] = evaluate_tree()
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "exp_stoi.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
