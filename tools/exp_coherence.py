"""Developer tool: the magnitude-squared coherence family on the GPU.
  1. 1024 resident pairs of 4 s at 48 kHz in float32, n_fft 1024, hop 512, one full band: HIP-event time of ssr_coherence with and
     without the per-bin output, of the public call (backend.coherence_metrics) end to end, and - in the same run, on the same
     signals - of ssr_phase_metrics with IP alone at the same n_fft and hop: the same transform, so the ratio is reported, not
     assumed; next to them the streaming-read floor (both signals once at bench.py's peak_measured) and the partial buffer's size
     against the input bytes;
  2. the split between the kernels: KERNEL_STATS=<csv> names the kernel-stats table of a `rocprofv3 --kernel-trace --stats
     --output-format csv` run of this tool with KERNELS_ONLY=1;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without coherence=True, passes alternated;
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, 9 passes each (exp_phase.py's comparison) - the one that has to hold.
Prints one JSON line (and writes it to OUT_DIR/coherence.json when OUT_DIR is set)."""
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
    from ssr_eval_amd import _lib, backend as B
    n_pairs, n_samples, n_fft, hop = 1024, 4 * 48000, 1024, 512
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    es = tg + 0.3 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    lens, idx = np.full(n_pairs, n_samples, np.int32), np.arange(n_pairs, dtype=np.int32)
    bands = np.tile(np.array([[0, n_fft // 2]], np.int32), (n_pairs, 1, 1))
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n_samples
    pinned = [torch.from_numpy(a).pin_memory() for a in (lens, idx, bands)]
    ptr = [C.c_void_p(p.data_ptr()) for p in pinned]
    K = 1 + (n_samples - n_fft) // hop
    res = {"n_pairs": n_pairs, "seconds_per_pair": 4, "rate": 48000, "dtype": "float32", "n_fft": n_fft, "hop": hop,
           "segments_per_pair": K, "chunks_per_pair": -(-K // 32)}
    out = torch.empty((n_pairs, 1, 3), dtype=torch.float64, device=dev)
    spec = torch.empty((n_pairs, n_fft // 2 + 1), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_coherence_workspace_bytes(ptr[0], n_pairs, ptr[1], n_pairs, n_fft, hop, 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    res["workspace_mib"] = round(ws_bytes / 2 ** 20, 1)
    res["partial_bytes_per_pair"] = 32 * (n_fft // 2 + 1) * res["chunks_per_pair"]
    res["input_bytes_per_pair"] = 2 * 4 * n_samples

    def coh(sp):
        _lib.check(lib.ssr_coherence(B._vp(tg), 0, B._vp(off), ptr[0], n_pairs, B._vp(es), 0, B._vp(off), ptr[1], n_pairs, n_fft, hop, 1,
                                     ptr[2], 0.5, B._vp(out), sp, B._vp(ws), ws_bytes, B._stream()))
    res["coherence"] = spread(torch, lambda: coh(None), 5)
    res["coherence_with_msc_out"] = spread(torch, lambda: coh(B._vp(spec)), 5)
    res["median_msc"], res["median_coh_sdr_db"] = (float(v) for v in out[:, 0, :2].median(dim=0).values.cpu())
    pout = torch.empty((n_pairs, 1), dtype=torch.float64, device=dev)
    pws_bytes = int(lib.ssr_phase_metrics_workspace_bytes(ptr[0], n_pairs, ptr[1], n_pairs, n_fft, hop, 1))
    pws = torch.empty(pws_bytes, dtype=torch.uint8, device=dev)

    def phase():
        _lib.check(lib.ssr_phase_metrics(B._vp(tg), 0, B._vp(off), ptr[0], n_pairs, B._vp(es), 0, B._vp(off), ptr[1], n_pairs, n_fft, hop, 0,
                                         n_fft // 2, 1, B._vp(pout), B._vp(pws), pws_bytes, B._stream()))
    res["phase_ip_same_frames"] = spread(torch, phase, 5)
    res["phase_frames_per_pair"] = 1 + n_samples // hop
    res["coherence_over_phase_ip"] = res["coherence"]["median_ms"] / res["phase_ip_same_frames"]["median_ms"]
    if with_floor:
        tl, el = list(tg.unbind(0)), list(es.unbind(0))
        res["api"] = spread(torch, lambda: B.coherence_metrics(tl, el, idx, n_fft, hop, None, 0.5, False, dev, deferred=True)(), 2, 3)
        import bench
        peak = bench.measured_hbm_peak().get("read_GBs")
        res["peak_measured_GBs"] = peak
        if peak:
            res["read_floor_ms"] = n_pairs * res["input_bytes_per_pair"] / (peak * 1e9) * 1e3
    return res


def kernel_stats(path):
    """The kernel-stats table of rocprofv3 --stats (columns Name, Calls, TotalDurationNs, AverageNs, ...) -> {kernel: calls, average
    microseconds} for the kernels of this family and the phase kernel timed next to them."""
    rows = {}
    for row in csv.DictReader(open(path)):
        k = row.get("Name", "")
        if "k_coh_" in k or "k_phase_dist" in k:
            rows[k.split("(")[0].replace("void ", "")] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    return rows


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, coherence=v) for name, v in (("plain", None), ("coherence", True))}
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
    res = {"tool": "exp_coherence"}
    if os.environ.get("KERNELS_ONLY") == "1":
        res["kernel"] = kernel_times(with_floor=False)
        print(json.dumps(res), flush=True)
        return
    root = tempfile.mkdtemp(prefix="ssr_coh_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_coherence_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
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
        open(os.path.join(os.environ["OUT_DIR"], "coherence.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
