"""Developer tool: the spectrum family on the GPU.
  1. 1024 resident pairs (2048 signals) of 4 s at 48 kHz in float32 at the defaults (n_fft 2048, hop 1024, the third-octave table, a
     split at 12 kHz): HIP-event time of ssr_spectrum with and without ltas_out, median of five rounds, and of the public call
     (backend.spectrum_metrics) end to end; in the same run ssr_coherence at the same n_fft and hop on the same pairs - it does the
     same transforms for a pair (one complex transform per segment of the pair) and is the yardstick; the ratio is reported, not
     bounded; next to them the streaming-read floor, one read of the signals at bench.py's peak_measured;
  2. the split between the kernels: KERNEL_STATS=<csv> names the kernel-stats table of a `rocprofv3 --kernel-trace --stats
     --output-format csv` run of this tool with KERNELS_ONLY=1;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without bandwidth=True, passes alternated;
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, three timed passes each per round (exp_phase.py's comparison) - the one
     that has to hold.
Prints one JSON line (and writes it to OUT_DIR/spectrum.json when OUT_DIR is set)."""
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


def spread(torch, fn, reps, rounds=5):
    v = [P.events_ms(torch, fn, reps) for _ in range(rounds)]
    return {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)}


def kernel_times(with_floor=True):
    import torch
    from ssr_eval_amd import AudioMetrics, _lib, backend as B
    n_pairs, fs, n_fft, hop = 1024, 48000, 2048, 1024
    n_samples = 4 * fs
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = 0.1 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    es = 0.5 * tg + 0.03 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    bands = np.ascontiguousarray(AudioMetrics._ltas_bands(fs, n_fft, None), np.int32)
    n_bands, nb = len(bands), n_fft // 2 + 1
    pin = lambda a: torch.from_numpy(a).pin_memory()      # noqa: E731
    lens, idx = pin(np.full(n_pairs, n_samples, np.int32)), pin(np.arange(n_pairs, dtype=np.int32))
    split = pin(np.full(n_pairs, n_fft // 4, np.int32))
    hp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n_samples
    sig = torch.empty((2 * n_pairs, 3), dtype=torch.float64, device=dev)
    pair = torch.empty((n_pairs, 8), dtype=torch.float64, device=dev)
    ltas = torch.empty((2 * n_pairs, nb), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_spectrum_workspace_bytes(hp(lens), n_pairs, hp(idx), n_pairs, n_fft, hop, n_bands))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    K = 1 + (n_samples - n_fft) // hop
    res = {"n_pairs": n_pairs, "n_signals": 2 * n_pairs, "seconds_per_signal": 4, "rate": fs, "dtype": "float32", "n_fft": n_fft, "hop": hop,
           "segments_per_signal": K, "analysis_bands": n_bands, "workspace_mib": round(ws_bytes / 2 ** 20, 1), "input_bytes": 4 * 2 * n_pairs * n_samples}

    def spec(lt):
        _lib.check(lib.ssr_spectrum(B._vp(tg), 0, B._vp(off), hp(lens), n_pairs, B._vp(es), 0, B._vp(off), hp(idx), n_pairs, n_fft, hop, 0,
                                    n_fft // 2, B.SPECTRUM_ROLLOFF, B.SPECTRUM_DROP_DB, n_bands, bands.ctypes.data_as(C.c_void_p), hp(split),
                                    B._vp(sig), B._vp(pair), B._vp(lt), B._vp(ws), ws_bytes, B._stream()))
    res["spectrum"] = spread(torch, lambda: spec(None), 5)
    res["spectrum_with_ltas_out"] = spread(torch, lambda: spec(ltas), 5)
    hz = fs / n_fft
    res["median_bw_hz_of_the_estimates"] = float(sig[n_pairs:, 0].median().cpu()) * hz
    res["median_hf_diff_db"], res["median_ltas_dist_db"] = float(pair[:, 5].median().cpu()), float(pair[:, 6].median().cpu())
    # the yardstick: ssr_coherence on the same pairs at the same framing (one band: its band kernel is a small part)
    cband = pin(np.tile(np.array([[0, n_fft // 2]], np.int32), (n_pairs, 1)))
    cout = torch.empty((n_pairs, 3), dtype=torch.float64, device=dev)
    cws_bytes = int(lib.ssr_coherence_workspace_bytes(hp(lens), n_pairs, hp(idx), n_pairs, n_fft, hop, 1))
    cws = torch.empty(cws_bytes, dtype=torch.uint8, device=dev)

    def coh():
        _lib.check(lib.ssr_coherence(B._vp(tg), 0, B._vp(off), hp(lens), n_pairs, B._vp(es), 0, B._vp(off), hp(idx), n_pairs, n_fft, hop, 1,
                                     hp(cband), 0.5, B._vp(cout), None, B._vp(cws), cws_bytes, B._stream()))
    res["coherence_same_frames"] = spread(torch, coh, 5)
    res["spectrum_over_coherence"] = res["spectrum"]["median_ms"] / res["coherence_same_frames"]["median_ms"]
    if with_floor:
        tl, el = list(tg.unbind(0)), list(es.unbind(0))
        table = [tuple(int(v) for v in b) for b in bands]
        res["api"] = spread(torch, lambda: B.spectrum_metrics(tl, el, idx.numpy(), n_fft, hop, None, B.SPECTRUM_ROLLOFF, B.SPECTRUM_DROP_DB, table,
                                                              split.numpy(), False, dev, deferred=True)(), 2, 3)
        import bench
        peak = bench.measured_hbm_peak().get("read_GBs")
        res["peak_measured_GBs"] = peak
        if peak:
            res["one_read_floor_ms"] = res["input_bytes"] / (peak * 1e9) * 1e3
            res["spectrum_over_floor"] = res["spectrum"]["median_ms"] / res["one_read_floor_ms"]
    return res


def kernel_stats(path):
    """The kernel-stats table of rocprofv3 --stats (columns Name, Calls, TotalDurationNs, AverageNs, ...) -> {kernel: calls, average
    microseconds} for the kernels of this family and of the yardstick."""
    rows = {}
    for row in csv.DictReader(open(path)):
        k = row.get("Name", "")
        if "k_spec_" in k or "k_coh_" in k:
            rows[k.split("(")[0].replace("void ", "")] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return rows


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, bandwidth=v) for name, v in (("plain", None), ("bandwidth", True))}
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
    res = {"tool": "exp_spectrum"}
    if os.environ.get("KERNELS_ONLY") == "1":
        res["kernel"] = kernel_times(with_floor=False)
        print(json.dumps(res), flush=True)
        return
    root = tempfile.mkdtemp(prefix="ssr_spec_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_bandwidth_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
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
        open(os.path.join(os.environ["OUT_DIR"], "spectrum.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
