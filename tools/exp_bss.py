"""Developer tool: the filter-invariant SDR on the GPU.
  1. 1024 resident pairs of 4 s at 48 kHz in float32, at 512 and at 64 taps, as 1024 targets with one estimate each (K = 1) and as
     128 targets with eight estimates each next to each other (K = 8: the target's autocorrelation once per run): HIP-event time of
     ssr_bss_sdr, the float64 multiply-adds it needs - (K + 1) correlations and K residual filters per target, 2 L n flop each - and
     their time at the 78.6 TFLOP/s vector FP64 peak the other sections measure against (the floor);
  2. the split between the kernels: KERNEL_STATS="L512K1=<csv>,L64K1=<csv>,..." names the kernel-stats tables of
     `rocprofv3 --kernel-trace --stats` runs of this tool with CONFIG=<name> KERNELS_ONLY=1, one per configuration;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without bss_sdr=True, passes alternated;
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree (exp_phase.py's comparison) - the one that has to hold.
Prints one JSON line (and writes it to OUT_DIR/bss.json when OUT_DIR is set)."""
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

PEAK_FP64_FLOPS = 78.6e12
CONFIGS = {"L512K1": (512, 1), "L64K1": (64, 1), "L512K8": (512, 8), "L64K8": (64, 8)}


def spread(torch, fn, reps, rounds=5):
    v = [P.events_ms(torch, fn, reps) for _ in range(rounds)]
    return {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)}


def kernel_times(names):
    import torch
    from ssr_eval_amd import _lib, backend as B
    n_pairs, n_samples = 1024, 4 * 48000
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = 0.1 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    es = 0.8 * tg.roll(37, dims=1) + 0.03 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n_samples
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    res = {"n_pairs": n_pairs, "seconds_per_pair": 4, "rate": 48000, "dtype": "float32", "peak_fp64_tflops": PEAK_FP64_FLOPS / 1e12}
    for name in names:
        taps, K = CONFIGS[name]
        n_tgt = n_pairs // K
        lens, idx = np.full(n_tgt, n_samples, np.int32), np.repeat(np.arange(n_tgt, dtype=np.int32), K)
        pinned = [torch.from_numpy(a).pin_memory() for a in (lens, idx)]
        out = torch.empty((n_pairs, 2), dtype=torch.float64, device=dev)
        ws_bytes = int(lib.ssr_bss_sdr_workspace_bytes(vp(lens), n_tgt, vp(idx), n_pairs, taps))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.ssr_bss_sdr(B._vp(tg), 0, B._vp(off), C.c_void_p(pinned[0].data_ptr()), n_tgt, B._vp(es), 0, B._vp(off),
                                       C.c_void_p(pinned[1].data_ptr()), n_pairs, taps, B._vp(out), None, B._vp(ws), ws_bytes, B._stream()))
        flop = 2.0 * taps * n_samples * ((K + 1) + K) * n_tgt
        row = {"taps": taps, "estimates_per_target": K, "targets": n_tgt, "workspace_mib": round(ws_bytes / 2 ** 20, 1),
               "gflop": round(flop / 1e9, 1), "floor_ms": flop / PEAK_FP64_FLOPS * 1e3, "call": spread(torch, call, 3)}
        row["call_over_floor"] = row["call"]["median_ms"] / row["floor_ms"]
        row["median_sdr_db"], row["median_lag"] = (float(v) for v in out.median(dim=0).values.cpu())
        res[name] = row
        del ws, out
    if len(names) == len(CONFIGS):
        tl, el = list(tg.unbind(0)), list(es.unbind(0))
        idx = np.arange(n_pairs, dtype=np.int32)
        res["api_L512K1"] = spread(torch, lambda: B.bss_sdr(tl, el, idx, 512, False, dev, deferred=True)(), 2, 3)
    return res


def kernel_stats(spec):
    """KERNEL_STATS="config=csv,..." -> {config: {kernel: calls, average microseconds}} for the kernels of this family (rocprofv3
    --stats columns Name, Calls, TotalDurationNs, AverageNs, ...)."""
    out = {}
    for item in filter(None, spec.split(",")):
        name, path = item.split("=", 1)
        rows = {}
        for row in csv.DictReader(open(path)):
            k = row.get("Name", "")
            if "k_bss_" in k:
                rows[k.split("(")[0].replace("void ", "")] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
        out[name] = rows
    return out


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, bss_sdr=v) for name, v in (("plain", None), ("bss_sdr", True))}
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
    res = {"tool": "exp_bss"}
    names = [os.environ["CONFIG"]] if os.environ.get("CONFIG") else list(CONFIGS)
    if os.environ.get("KERNELS_ONLY") == "1":
        res["kernel"] = kernel_times(names)
        print(json.dumps(res), flush=True)
        return
    root = tempfile.mkdtemp(prefix="ssr_bss_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_bss_sdr_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernel"] = kernel_times(names)
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
        open(os.path.join(os.environ["OUT_DIR"], "bss.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
