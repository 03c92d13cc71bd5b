"""Developer tool: the noise-to-mask family on the GPU.
  1. 1024 resident pairs of 4 s in float32 at 48 kHz (n_fft 2048, hop 1024, 109 bands): HIP-event time of ssr_nmr, of ssr_nmr on all
     1024 targets with ONE estimate (geometry, excite and mask next to one pair's noise and score: the target side of the call) and -
     in the same run, on the same signals - of ssr_coherence at n_fft 2048, hop 1024 on one full band; the workspace of each; the
     FP64 floor of the kernels' own operation count (count below) at the vector peak;
  2. each kernel's time from a kernel trace of three such calls in a child process (`rocprofv3 --kernel-trace --stats`; left out where
     the profiler is absent or SKIP_TRACE=1);
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without nmr=True, 9 passes each, alternated (SKIP_EVALUATE=1 leaves it out);
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, 9 passes each (exp_phase.py's comparison).
Prints one JSON line (and writes it to OUT_DIR/nmr.json when OUT_DIR is set).  No speed bar is set: the times are recorded.

Operation count per frame (Nc bands, N-point frames; an exp2 / log2 / log10 counted as 26 flops, a sqrt as 10): one half of a packed
complex transform, 2.5 N log2 N; excite: the power and the band sums 5 (N / 2 + 1), per source band two logarithms, two exp2 and the
2 (Nc - l) column sum, per target band the (i + 1) exp2 terms at 29 and the 3 (Nc - 1 - i) lower-slope terms; noise: two such half
transforms, the magnitudes and the band sums 28 (N / 2 + 1), a division per band; the mask 5 per band."""
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exp_phase as P          # noqa: E402  (the tree, the event timer and the parent comparison)
from exp_coherence import spread          # noqa: E402

PEAK_FP64_FLOPS = 78.6e12      # MI355X vector FP64
FS, N_PAIRS, SECONDS = 48000, 1024, 4


def flops_per_frame(N, Nc):
    half = 2.5 * N * np.log2(N)
    src = Nc * (4 * 26 + 6) + sum(2 * (Nc - l) for l in range(Nc))
    dst = sum(29 * (i + 1) + 3 * (Nc - 1 - i) for i in range(Nc)) + 14 * Nc
    return {"excite": half + 5 * (N // 2 + 1) + src + dst, "mask": 5.0 * Nc, "noise": 2 * half + 28 * (N // 2 + 1) + 2 * Nc}


def setup(torch, B, lib):
    """The 1024 pairs and a function that queues one ssr_nmr call on the first n_est of them."""
    n_samples = SECONDS * FS
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = 0.1 * torch.randn((N_PAIRS, n_samples), generator=g, device=dev, dtype=torch.float32)
    es = tg + 0.003 * torch.randn((N_PAIRS, n_samples), generator=g, device=dev, dtype=torch.float32)
    d = B.nmr_design(FS)
    n_fft, J = d["n_fft"], len(d["fc"])
    lens, idx = np.full(N_PAIRS, n_samples, np.int32), np.arange(N_PAIRS, dtype=np.int32)
    split = np.full(N_PAIRS, J // 2, np.int32)
    bands = np.tile(np.array([[0, n_fft // 2]], np.int32), (N_PAIRS, 1, 1))
    off = torch.arange(N_PAIRS, dtype=torch.int64, device=dev) * n_samples
    pinned = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (lens, idx, split, d["bins"], d["table"], bands)]
    ptr = [C.c_void_p(p.data_ptr()) for p in pinned]
    w_dev = torch.from_numpy(d["weights"]).to(dev)
    out = torch.empty((N_PAIRS, B.NMR_COLUMNS), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_nmr_workspace_bytes(ptr[0], N_PAIRS, ptr[1], N_PAIRS, n_fft, J))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def nmr(n_est=N_PAIRS):
        from ssr_eval_amd import _lib
        _lib.check(lib.ssr_nmr(B._vp(tg), 0, B._vp(off), ptr[0], N_PAIRS, B._vp(es), 0, B._vp(off), ptr[1], n_est, n_fft, J, B._vp(w_dev), ptr[3],
                               ptr[4], ptr[2], B._vp(out), None, None, B._vp(ws), ws_bytes, B._stream()))
    return dict(tg=tg, es=es, off=off, ptr=ptr, pinned=pinned, out=out, ws=ws, ws_bytes=ws_bytes, n_fft=n_fft, J=J, nmr=nmr, dev=dev,
                n_samples=n_samples, w_dev=w_dev)


def kernel_times():
    import torch
    from ssr_eval_amd import _lib, backend as B
    lib = _lib.load()
    s = setup(torch, B, lib)
    n_fft, J, hop = s["n_fft"], s["J"], s["n_fft"] // 2
    K = 1 + (s["n_samples"] - n_fft) // hop
    res = {"n_pairs": N_PAIRS, "seconds_per_pair": SECONDS, "rate": FS, "dtype": "float32", "n_fft": n_fft, "hop": hop, "n_bands": J,
           "frames_per_pair": K, "chunks_per_pair": -(-K // 32), "workspace_mib": round(s["ws_bytes"] / 2 ** 20, 1)}
    res["nmr"] = spread(torch, s["nmr"], 5)
    res["nmr_all_targets_one_estimate"] = spread(torch, lambda: s["nmr"](1), 5)
    s["nmr"]()
    torch.cuda.synchronize()
    med = s["out"].nanmedian(dim=0).values.cpu()
    res["median_nmr_db"], res["median_rdf"] = float(med[0]), float(med[2])
    fl = flops_per_frame(n_fft, J)
    frames = N_PAIRS * K
    res["flops_per_frame"] = {k: float(v) for k, v in fl.items()}
    res["fp64_floor_ms"] = {k: float(v * frames / PEAK_FP64_FLOPS * 1e3) for k, v in fl.items()}
    res["fp64_floor_ms"]["call"] = float(sum(res["fp64_floor_ms"].values()))
    res["nmr_over_fp64_floor"] = res["nmr"]["median_ms"] / res["fp64_floor_ms"]["call"]
    ptr = s["ptr"]
    cout = torch.empty((N_PAIRS, 1, 3), dtype=torch.float64, device=s["dev"])
    cws_bytes = int(lib.ssr_coherence_workspace_bytes(ptr[0], N_PAIRS, ptr[1], N_PAIRS, n_fft, hop, 1))
    cws = torch.empty(cws_bytes, dtype=torch.uint8, device=s["dev"])
    res["coherence_workspace_mib"] = round(cws_bytes / 2 ** 20, 1)

    def coh():
        _lib.check(lib.ssr_coherence(B._vp(s["tg"]), 0, B._vp(s["off"]), ptr[0], N_PAIRS, B._vp(s["es"]), 0, B._vp(s["off"]), ptr[1], N_PAIRS, n_fft, hop,
                                     1, ptr[5], 0.5, B._vp(cout), None, B._vp(cws), cws_bytes, B._stream()))
    res["coherence_same_frames"] = spread(torch, coh, 5)
    res["nmr_over_coherence"] = res["nmr"]["median_ms"] / res["coherence_same_frames"]["median_ms"]
    return res


def trace_child():
    """Three full calls, for the kernel trace."""
    import torch
    from ssr_eval_amd import _lib, backend as B
    s = setup(torch, B, _lib.load())
    for _ in range(3):
        s["nmr"]()
    torch.cuda.synchronize()


def kernel_trace():
    """Mean time of each k_nmr_* kernel over the child's three calls, in ms, or None."""
    prof = shutil.which("rocprofv3")
    if prof is None or os.environ.get("SKIP_TRACE") == "1":
        return None
    out = tempfile.mkdtemp(prefix="ssr_nmr_trace_")
    try:
        subprocess.run([prof, "--kernel-trace", "--stats", "-d", out, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                        "--trace-child"], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600, check=True)
        rows = {}
        for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                name = r.get("Name", "")
                if "k_nmr_" in name:
                    short = name[name.index("k_nmr_"):].split("(")[0].split("<")[0]
                    rows[short] = {"calls": int(r["Calls"]), "mean_ms": float(r["AverageNs"]) / 1e6}
        return rows or None
    except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
        return {"error": repr(e)[:200]}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, nmr=v) for name, v in (("plain", None), ("nmr", True))}
    for h in hs.values():
        h.evaluate(limit_test_nums=2, limit_test_speaker=1, save_json=False)
        h.evaluate(save_json=False)
    times = {k: [] for k in hs}
    for _ in range(9):
        for k, h in hs.items():
            t0 = time.perf_counter()
            h.evaluate(save_json=False)
            times[k].append(time.perf_counter() - t0)
    return {k: {"files_per_s": round(n_files / float(np.median(v)), 1), "min": round(n_files / max(v), 1), "max": round(n_files / min(v), 1),
                "pass_s": [round(x, 4) for x in v]} for k, v in times.items()} | {"n_files": n_files}


def main():
    sys.path.insert(0, ROOT)
    if "--trace-child" in sys.argv:
        return trace_child()
    res = {"tool": "exp_nmr"}
    root = tempfile.mkdtemp(prefix="ssr_nmr_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_nmr_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernel_trace"] = kernel_trace()
        res["kernel_48k"] = kernel_times()
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree(root, n_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "nmr.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
