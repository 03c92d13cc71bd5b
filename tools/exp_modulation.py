"""Developer tool: the modulation family on the GPU.
  1. 1024 resident pairs (2048 signals) of 4 s at 48 kHz in float32 at the defaults (32 bands, env_rate 1600: hop_e 30, S 102, range
     60 dB, a split at 12 kHz): HIP-event time of ssr_modulation with and without spectrum_out, median of five rounds, of ssr_auditory
     on the same signals in the same run (the same sweeps at hop 480 instead of 30), and of the public call
     (backend.modulation_metrics, which splits the batch under its workspace cap) end to end; next to them the FP64 floor of the
     sweeps' operation count (exp_auditory's) and of k_mod_bank's own (FLOP_PER_SAMPLE_COUPLE below), at bench.py's FP64_PEAK_TFLOPS;
  2. the split between the kernels, k_mod_bank on its own among them: KERNEL_STATS=<csv> names the kernel-stats table of a
     `rocprofv3 --kernel-trace --stats --output-format csv` run of this tool with KERNELS_ONLY=1;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without modulation=True, nine passes each, alternated;
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, three timed passes each per round (exp_phase.py's comparison).
Prints one JSON line (and writes it to OUT_DIR/modulation.json when OUT_DIR is set).  Nothing here is a threshold."""
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
import exp_auditory as A       # noqa: E402  (the sweeps' operation count, the spread of five rounds)
import exp_phase as P          # noqa: E402  (the tree, the event timer and the parent comparison)

# float64 operations of ssr_mod_step per envelope sample and (band, modulation band) couple (an FMA counts 2): the biquad - y (2),
# z0 (a multiply, an FMA, an addition: 4), z1 (a multiply and an FMA: 3) - and four frames of a multiply and an FMA each (12)
FLOP_PER_SAMPLE_COUPLE = 9 + 12


def kernel_times(with_api=True):
    import torch
    from ssr_eval_amd import _lib, backend as B
    n_pairs, fs, n_bands = 1024, 48000, 32
    n_samples, hop_a, hop = 4 * fs, B.auditory_hop(fs), B.modulation_hop(fs)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = 0.1 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    es = 0.5 * tg + 0.03 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    fc, coef, mod, S, ktab = B.modulation_design(fs, hop, n_bands)
    pin = lambda a: torch.from_numpy(a).pin_memory()      # noqa: E731
    lens, idx, kst = pin(np.full(n_pairs, n_samples, np.int32)), pin(np.arange(n_pairs, dtype=np.int32)), pin(ktab)
    split = pin(np.full(n_pairs, int(np.searchsorted(fc, 12000.0)), np.int32))
    split_a = pin(np.full(n_pairs, 1 + int(np.searchsorted(fc[1:-1], 12000.0)), np.int32))
    hp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n_samples
    blocks = n_samples // hop
    frames = 1 + (blocks - 4 * S) // S
    sig = torch.empty((2 * n_pairs, 4), dtype=torch.float64, device=dev)
    pair = torch.empty((n_pairs, 4), dtype=torch.float64, device=dev)
    pair_a = torch.empty((n_pairs, 3), dtype=torch.float64, device=dev)
    spec = torch.empty((2 * n_pairs, n_bands, 8), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_modulation_workspace_bytes(hp(lens), n_pairs, hp(idx), n_pairs, hop, n_bands))
    ws_a = int(lib.ssr_auditory_workspace_bytes(hp(lens), n_pairs, hp(idx), n_pairs, hop_a, n_bands))
    ws = torch.empty(max(ws_bytes, ws_a), dtype=torch.uint8, device=dev)
    sweep_flop = A.FLOP_PER_SAMPLE_BAND * 2 * n_pairs * blocks * hop * n_bands
    bank_flop = FLOP_PER_SAMPLE_COUPLE * 2 * n_pairs * ((frames - 1) * S + 4 * S) * n_bands * 8
    res = {"n_pairs": n_pairs, "n_signals": 2 * n_pairs, "seconds_per_signal": 4, "rate": fs, "dtype": "float32", "n_bands": n_bands, "hop_e": hop,
           "S": S, "blocks_per_signal": blocks, "frames_per_signal": frames, "workspace_mib": round(ws_bytes / 2 ** 20, 1),
           "workspace_mb_per_signal": round(ws_bytes / (2 * n_pairs) / 1e6, 2), "input_bytes": 4 * 2 * n_pairs * n_samples,
           "sweep_gflop": round(sweep_flop / 1e9, 1), "bank_gflop": round(bank_flop / 1e9, 2)}

    def mod_call(sp):
        _lib.check(lib.ssr_modulation(B._vp(tg), 0, B._vp(off), hp(lens), n_pairs, B._vp(es), 0, B._vp(off), hp(idx), n_pairs, hop, n_bands,
                                      coef.ctypes.data_as(C.c_void_p), mod.ctypes.data_as(C.c_void_p), S, hp(kst), 60.0, hp(split), B._vp(sig),
                                      B._vp(pair), B._vp(sp), B._vp(ws), ws_bytes, B._stream()))

    def aud_call():
        _lib.check(lib.ssr_auditory(B._vp(tg), 0, B._vp(off), hp(lens), n_pairs, B._vp(es), 0, B._vp(off), hp(idx), n_pairs, hop_a, n_bands,
                                    coef.ctypes.data_as(C.c_void_p), 60.0, 1, hp(split_a), B._vp(pair_a), None, None, B._vp(ws), ws_a, B._stream()))
    res["modulation"] = A.spread(torch, lambda: mod_call(None), 3)
    res["modulation_with_spectrum_out"] = A.spread(torch, lambda: mod_call(spec), 3)
    res["auditory_same_run"] = A.spread(torch, aud_call, 3)
    res["median_srmr"], res["median_mod_dist"] = float(sig[:, 0].median().cpu()), float(pair[:, 1].median().cpu())
    import bench
    res["fp64_peak_tflops"] = bench.FP64_PEAK_TFLOPS
    res["sweeps_fp64_floor_ms"] = sweep_flop / (bench.FP64_PEAK_TFLOPS * 1e12) * 1e3
    res["bank_fp64_floor_ms"] = bank_flop / (bench.FP64_PEAK_TFLOPS * 1e12) * 1e3
    res["modulation_over_auditory"] = res["modulation"]["median_ms"] / res["auditory_same_run"]["median_ms"]
    if with_api:
        tl, el = list(tg.unbind(0)), list(es.unbind(0))
        res["api"] = A.spread(torch, lambda: B.modulation_metrics(tl, el, idx.numpy(), fs, n_bands, None, 1600, 60.0, None, split.numpy(), False,
                                                                  None, dev, deferred=True)(), 2, 3)
        res["api_workspace_cap_mib"] = B.MODULATION_WORKSPACE_CAP >> 20
    return res


def kernel_stats(path, bank_floor_ms):
    """The kernel-stats table of rocprofv3 --stats (columns Name, Calls, TotalDurationNs, AverageNs, ...) -> {kernel: calls, average
    microseconds} for the kernels of this family and the auditory family's, and k_mod_bank's time over its FP64 floor."""
    rows = {}
    for row in csv.DictReader(open(path)):
        k = row.get("Name", "")
        if "k_mod_" in k or "k_aud_" in k:
            rows[k.split("(")[0].replace("void ", "")] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    bank = [v["avg_us"] for k, v in rows.items() if k.startswith("k_mod_bank")]
    if bank:
        rows["k_mod_bank_over_fp64_floor"] = bank[0] / 1e3 / bank_floor_ms
    return rows


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, modulation=v) for name, v in (("plain", None), ("modulation", True))}
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
    res = {"tool": "exp_modulation", "tuned": False}
    if os.environ.get("KERNELS_ONLY") == "1":
        res["kernel"] = kernel_times(with_api=False)
        print(json.dumps(res), flush=True)
        return
    root = tempfile.mkdtemp(prefix="ssr_mod_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_modulation_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernel"] = kernel_times()
        if os.environ.get("KERNEL_STATS"):
            res["kernel_stats"] = kernel_stats(os.environ["KERNEL_STATS"], res["kernel"]["bank_fp64_floor_ms"])
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree(root, n_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "modulation.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
