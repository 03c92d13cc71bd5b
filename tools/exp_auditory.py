"""Developer tool: the auditory family on the GPU.
  1. 1024 resident pairs (2048 signals) of 4 s at 48 kHz in float32 at the defaults (32 bands, hop 480, range 60 dB, a split at
     12 kHz): HIP-event time of ssr_auditory with and without band_out / image_out, median of five rounds, and of the public call
     (backend.auditory_metrics) end to end; next to them the FP64 floor of the sweeps' own operation count (FLOP_PER_SAMPLE_BAND
     below, at bench.py's FP64_PEAK_TFLOPS) and the streaming-read floor, the two reads of the signals at bench.py's peak_measured;
  2. the split between the kernels: KERNEL_STATS=<csv> names the kernel-stats table of a `rocprofv3 --kernel-trace --stats
     --output-format csv` run of this tool with KERNELS_ONLY=1;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without auditory=True, nine passes each, alternated;
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, three timed passes each per round (exp_phase.py's comparison) - the one
     that has to hold.
Prints one JSON line (and writes it to OUT_DIR/auditory.json when OUT_DIR is set)."""
import csv
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exp_phase as P          # noqa: E402  (the tree, the event timer and the parent comparison)

# float64 operations of ssr_aud_step per sample and band (an FMA counts 2): g x, then 4 stages of 4 multiply-adds - 33 in sweep 1;
# sweep 2 adds |z|^2 (a multiply and an FMA) and the block sum's addition - 37
FLOP_PER_SAMPLE_BAND = 33 + 37


def spread(torch, fn, reps, rounds=5):
    v = [P.events_ms(torch, fn, reps) for _ in range(rounds)]
    return {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)}


def kernel_times(with_floor=True):
    import torch
    from ssr_eval_amd import _lib, backend as B
    n_pairs, fs, n_bands = 1024, 48000, 32
    n_samples, hop = 4 * fs, B.auditory_hop(fs)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = 0.1 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    es = 0.5 * tg + 0.03 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    fc, coef = B.gammatone_design(fs, n_bands)
    pin = lambda a: torch.from_numpy(a).pin_memory()      # noqa: E731
    lens, idx = pin(np.full(n_pairs, n_samples, np.int32)), pin(np.arange(n_pairs, dtype=np.int32))
    sb = 1 + int(np.searchsorted(fc[1:-1], 12000.0))
    split = pin(np.full(n_pairs, sb, np.int32))
    hp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n_samples
    rows = n_samples // hop - 1
    pair = torch.empty((n_pairs, 3), dtype=torch.float64, device=dev)
    bands = torch.empty((n_pairs, n_bands), dtype=torch.float64, device=dev)
    images = torch.empty((2 * n_pairs * rows, n_bands), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_auditory_workspace_bytes(hp(lens), n_pairs, hp(idx), n_pairs, hop, n_bands))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    flop = FLOP_PER_SAMPLE_BAND * 2 * n_pairs * (rows + 1) * hop * n_bands
    res = {"n_pairs": n_pairs, "n_signals": 2 * n_pairs, "seconds_per_signal": 4, "rate": fs, "dtype": "float32", "n_bands": n_bands, "hop": hop,
           "rows_per_signal": rows, "workspace_mib": round(ws_bytes / 2 ** 20, 1), "input_bytes": 4 * 2 * n_pairs * n_samples,
           "sweep_gflop": round(flop / 1e9, 1)}

    def aud(bd, im):
        _lib.check(lib.ssr_auditory(B._vp(tg), 0, B._vp(off), hp(lens), n_pairs, B._vp(es), 0, B._vp(off), hp(idx), n_pairs, hop, n_bands,
                                    coef.ctypes.data_as(C.c_void_p), 60.0, 1, hp(split), B._vp(pair), B._vp(bd), B._vp(im), B._vp(ws), ws_bytes,
                                    B._stream()))
    res["auditory"] = spread(torch, lambda: aud(None, None), 3)
    res["auditory_with_band_and_image_out"] = spread(torch, lambda: aud(bands, images), 3)
    res["median_nsim"], res["median_nsim_hf"] = float(pair[:, 0].median().cpu()), float(pair[:, 1].median().cpu())
    import bench
    res["fp64_peak_tflops"] = bench.FP64_PEAK_TFLOPS
    res["fp64_floor_ms"] = flop / (bench.FP64_PEAK_TFLOPS * 1e12) * 1e3
    res["auditory_over_fp64_floor"] = res["auditory"]["median_ms"] / res["fp64_floor_ms"]
    if with_floor:
        tl, el = list(tg.unbind(0)), list(es.unbind(0))
        res["api"] = spread(torch, lambda: B.auditory_metrics(tl, el, idx.numpy(), fs, n_bands, None, 60.0, True, split.numpy(), False, False, None,
                                                              dev, deferred=True)(), 2, 3)
        peak = bench.measured_hbm_peak().get("read_GBs")
        res["peak_measured_GBs"] = peak
        if peak:
            res["two_reads_floor_ms"] = 2 * res["input_bytes"] / (peak * 1e9) * 1e3
            res["auditory_over_read_floor"] = res["auditory"]["median_ms"] / res["two_reads_floor_ms"]
    return res


def kernel_stats(path):
    """The kernel-stats table of rocprofv3 --stats (columns Name, Calls, TotalDurationNs, AverageNs, ...) -> {kernel: calls, average
    microseconds} for the kernels of this family."""
    rows = {}
    for row in csv.DictReader(open(path)):
        k = row.get("Name", "")
        if "k_aud_" in k:
            rows[k.split("(")[0].replace("void ", "")] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return rows


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, auditory=v) for name, v in (("plain", None), ("auditory", True))}
    for h in hs.values():
        h.evaluate(limit_test_nums=2, limit_test_speaker=1, save_json=False)
        h.evaluate(save_json=False)
    times = {k: [] for k in hs}
    for _ in range(9):
        for k, h in hs.items():
            t0 = time.perf_counter()
            h.evaluate(save_json=False)
            times[k].append(time.perf_counter() - t0)
    return {k: {"files_per_s": round(n_files / float(np.median(v)), 1), "pass_s": [round(x, 4) for x in v]} for k, v in times.items()} | \
        {"n_files": n_files}


def main():
    sys.path.insert(0, ROOT)
    res = {"tool": "exp_auditory"}
    if os.environ.get("KERNELS_ONLY") == "1":
        res["kernel"] = kernel_times(with_floor=False)
        print(json.dumps(res), flush=True)
        return
    root = tempfile.mkdtemp(prefix="ssr_aud_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_auditory_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
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
        open(os.path.join(os.environ["OUT_DIR"], "auditory.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
