"""Developer tool: the loudness family on the GPU.
  1. 1024 resident pairs (2048 signals) of 4 s at 48 kHz in float32: HIP-event time of ssr_loudness with and without blocks_out,
     median of five rounds, and of the public call (backend.loudness_metrics) end to end; next to them the streaming-read floor -
     both reads of the signals by the filter sweeps at bench.py's peak_measured - and the serial baseline: the library's
     one-lane-per-signal sosfiltfilt (exact=True) with the two K-weighting sections on the same signals.  That kernel runs the
     recurrence forwards AND backwards and writes y, so HALF its time stands for one serial pass;
  2. the split between the kernels: KERNEL_STATS=<csv> names the kernel-stats table of a `rocprofv3 --kernel-trace --stats
     --output-format csv` run of this tool with KERNELS_ONLY=1;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without loudness=True, passes alternated;
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, three timed passes each per round (exp_phase.py's comparison) - the one
     that has to hold.
Prints one JSON line (and writes it to OUT_DIR/loudness.json when OUT_DIR is set)."""
import csv
import ctypes as C
import json
import math
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exp_phase as P          # noqa: E402  (the tree, the event timer and the parent comparison)


def spread(torch, fn, reps, rounds=5):
    v = [P.events_ms(torch, fn, reps) for _ in range(rounds)]
    return {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)}


def k_weighting_sos(fs):
    """The two sections of DESIGN section 21 as scipy-style rows b0 b1 b2 1 a1 a2."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K, Vh = math.tan(math.pi * f0 / fs), 10.0 ** (G / 20.0)
    Vb, a0 = Vh ** 0.4996667741545416, 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 1.0, 2.0 * (K * K - 1.0) / a0,
          (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    d = 1.0 + K / Q + K * K
    return np.array([s1, [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d]])


def kernel_times(with_floor=True):
    import torch
    from ssr_eval_amd import _lib, backend as B
    n_pairs, fs = 1024, 48000
    n_sig, n_samples = 2 * n_pairs, 4 * fs
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    x = 0.1 * torch.randn((n_sig, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    lens = torch.from_numpy(np.full(n_sig, n_samples, np.int32)).pin_memory()
    S = n_samples // B.loudness_sub_len(fs)
    boff = torch.from_numpy(np.arange(n_sig, dtype=np.int64) * S).pin_memory()
    off = torch.arange(n_sig, dtype=torch.int64, device=dev) * n_samples
    out = torch.empty((n_sig, 6), dtype=torch.float64, device=dev)
    blocks = torch.empty(n_sig * S, dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_loudness_workspace_bytes(C.c_void_p(lens.data_ptr()), n_sig, fs))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    res = {"n_pairs": n_pairs, "n_signals": n_sig, "seconds_per_signal": 4, "rate": fs, "dtype": "float32", "sub_blocks_per_signal": S,
           "segments_per_signal": 8 * S, "workspace_mib": round(ws_bytes / 2 ** 20, 1), "input_bytes": 4 * n_sig * n_samples}

    def loud(bl):
        _lib.check(lib.ssr_loudness(B._vp(x), 0, B._vp(off), C.c_void_p(lens.data_ptr()), n_sig, fs, B._vp(out),
                                    C.c_void_p(boff.data_ptr()) if bl is not None else None, B._vp(bl), B._vp(ws), ws_bytes, B._stream()))
    res["loudness"] = spread(torch, lambda: loud(None), 5)
    res["loudness_with_blocks_out"] = spread(torch, lambda: loud(blocks), 5)
    res["median_lufs"], res["median_true_peak_db"] = float(out[:, 0].median().cpu()), float(out[:, 5].median().cpu())
    if with_floor:
        sigs = list(x.unbind(0))
        res["api"] = spread(torch, lambda: B.loudness_metrics(sigs, fs, False, dev, deferred=True)(), 2, 3)
        sos = k_weighting_sos(fs)
        r = B.Ragged.from_list(sigs, dev)
        res["serial_sosfiltfilt_two_passes"] = spread(torch, lambda: B.sosfiltfilt(sos, r, dev, exact=True), 1, 3)
        res["serial_one_pass_ms"] = res["serial_sosfiltfilt_two_passes"]["median_ms"] / 2
        res["serial_pass_over_loudness"] = res["serial_one_pass_ms"] / res["loudness"]["median_ms"]
        import bench
        peak = bench.measured_hbm_peak().get("read_GBs")
        res["peak_measured_GBs"] = peak
        if peak:
            res["two_reads_floor_ms"] = 2 * res["input_bytes"] / (peak * 1e9) * 1e3
            res["loudness_over_floor"] = res["loudness"]["median_ms"] / res["two_reads_floor_ms"]
    return res


def kernel_stats(path):
    """The kernel-stats table of rocprofv3 --stats (columns Name, Calls, TotalDurationNs, AverageNs, ...) -> {kernel: calls, average
    microseconds} for the kernels of this family."""
    rows = {}
    for row in csv.DictReader(open(path)):
        k = row.get("Name", "")
        if "k_loud_" in k:
            rows[k.split("(")[0].replace("void ", "")] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return rows


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, loudness=v) for name, v in (("plain", None), ("loudness", True))}
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


def main():
    sys.path.insert(0, ROOT)
    res = {"tool": "exp_loudness"}
    if os.environ.get("KERNELS_ONLY") == "1":
        res["kernel"] = kernel_times(with_floor=False)
        print(json.dumps(res), flush=True)
        return
    root = tempfile.mkdtemp(prefix="ssr_loud_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_loudness_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernel"] = kernel_times()
        if os.environ.get("KERNEL_STATS"):
            res["kernel_stats"] = kernel_stats(os.environ["KERNEL_STATS"])
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree(root, n_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "loudness.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
