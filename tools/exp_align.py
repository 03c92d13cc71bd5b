"""Developer tool: the delay stage on the GPU.
  1. 1024 resident pairs of 4 s at 48 kHz in float32, the estimate 37 samples late, at max_lag 64, 1024 and 4096: HIP-event time of
     ssr_align with the shift (a copy) and without it, the workspace, and next to each time the two floors of its own work - the
     n (2 L + 1) float64 multiply-adds of a pair at the 78.6 TFLOP/s vector FP64 peak the other sections measure against, and one
     streaming read of both signals (plus, with the shift, one read and one write of the estimate) at the 8 TB/s data-sheet peak;
     and the time of the fractional shift (subsample) at max_lag 1024;
  2. the split between the kernels: KERNEL_STATS="L64=<csv>,L1024=<csv>,..." names the kernel-stats tables of
     `rocprofv3 --kernel-trace --stats` runs of this tool with CONFIG=<name> KERNELS_ONLY=1, one per configuration;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without align=True, 9 passes each, alternated (SKIP_EVALUATE=1 leaves it out);
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, 9 passes each (exp_phase.py's comparison).
Prints one JSON line (and writes it to OUT_DIR/align.json when OUT_DIR is set).  No speed bar is set: the times are recorded."""
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
from exp_coherence import spread          # noqa: E402

PEAK_FP64_FLOPS = 78.6e12
PEAK_HBM_BYTES = 8.0e12
CONFIGS = {"L64": 64, "L1024": 1024, "L4096": 4096}


def kernel_times(names, n_pairs=1024, rate=48000, seconds=4):
    import torch
    from ssr_eval_amd import _lib, backend as B
    n = seconds * rate
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = 0.1 * torch.randn((n_pairs, n), generator=g, device=dev, dtype=torch.float32)
    es = 0.8 * tg.roll(37, dims=1) + 0.03 * torch.randn((n_pairs, n), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    lens, idx = np.full(n_pairs, n, np.int32), np.arange(n_pairs, dtype=np.int32)
    pinned = [torch.from_numpy(a).pin_memory() for a in (lens, idx)]
    lp, ip = C.c_void_p(pinned[0].data_ptr()), C.c_void_p(pinned[1].data_ptr())
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n
    rows = torch.empty((n_pairs, B.ALIGN_COLUMNS), dtype=torch.float64, device=dev)
    out = torch.empty_like(es)
    res = {"n_pairs": n_pairs, "seconds_per_pair": seconds, "rate": rate, "dtype": "float32", "true_delay": 37,
           "peak_fp64_tflops": PEAK_FP64_FLOPS / 1e12, "peak_hbm_tb_s": PEAK_HBM_BYTES / 1e12}
    for name in names:
        L = CONFIGS[name]
        ws_bytes = int(lib.ssr_align_workspace_bytes(lp, n_pairs, lp, ip, n_pairs, L))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def call(shift=True, sub=0):
            _lib.check(lib.ssr_align(B._vp(tg), 0, B._vp(off), lp, n_pairs, B._vp(es), 0, B._vp(off), lp, ip, n_pairs, L, sub, B._vp(rows),
                                     B._vp(out) if shift else None, B._vp(off), None, B._vp(ws), ws_bytes, B._stream()))
        fma = n_pairs * n * (2 * L + 1)
        r = {"max_lag": L, "workspace_mib": round(ws_bytes / 2 ** 20, 1), "fma": fma,
             "fp64_floor_ms": 1e3 * 2 * fma / PEAK_FP64_FLOPS,
             "read_floor_ms": 1e3 * n_pairs * 2 * n * 4 / PEAK_HBM_BYTES,
             "read_floor_with_shift_ms": 1e3 * n_pairs * 4 * n * 4 / PEAK_HBM_BYTES}
        reps = 3 if L >= 1024 else 5
        r["search_and_shift"] = spread(torch, call, reps)
        r["search_only"] = spread(torch, lambda: call(False), reps)
        if L == 1024:
            r["search_and_fractional_shift"] = spread(torch, lambda: call(True, 1), reps)
        call()
        torch.cuda.synchronize()
        got = rows.cpu().numpy()
        r["delays_found"] = sorted({float(v) for v in got[:, 0]})
        r["median_corr"] = float(np.median(got[:, 2]))
        r["over_fp64_floor"] = r["search_only"]["median_ms"] / r["fp64_floor_ms"]
        res[name] = r
        del ws
    return res


def kernel_split(spec):
    """{config: {kernel: {calls, total_ms, share}}} of the k_align_* rows of rocprofv3's kernel-stats tables."""
    out = {}
    for item in spec.split(","):
        name, path = item.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if "k_align" in r["Name"]]
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        out[name] = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                                               "share": float(r["TotalDurationNs"]) / total} for r in rows}
    return out


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, align=v) for name, v in (("plain", None), ("align", True))}
    for h in hs.values():
        h.evaluate(limit_test_nums=2, limit_test_speaker=1, save_json=False)
        h.evaluate(save_json=False)
    times = {k: [] for k in hs}
    for _ in range(9):
        for k, h in hs.items():
            t0 = time.perf_counter()
            h.evaluate(save_json=False)
            times[k].append(time.perf_counter() - t0)
    fps = {k: [round(n_files / t, 1) for t in v] for k, v in times.items()}
    return {k: {"files_per_s": float(np.median(v)), "min": min(v), "max": max(v), "passes": v} for k, v in fps.items()} | {"n_files": n_files}


def main():
    sys.path.insert(0, ROOT)
    names = [os.environ["CONFIG"]] if os.environ.get("CONFIG") else list(CONFIGS)
    if os.environ.get("KERNELS_ONLY") == "1":
        print(json.dumps(kernel_times(names)), flush=True)
        return
    res = {"tool": "exp_align"}
    root = tempfile.mkdtemp(prefix="ssr_align_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_align_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernels"] = kernel_times(names)
        if os.environ.get("KERNEL_STATS"):
            res["kernel_split"] = kernel_split(os.environ["KERNEL_STATS"])
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree(root, n_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "align.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
