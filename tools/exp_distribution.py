"""Developer tool: the distribution family on the GPU.
  1. ssr_frechet and ssr_kernel_distance (one gamma) on resident float32 sets at (n = m = 4096, D = 128), (50,000, 128) and
     (4096, 512), K = 1 and 7, and at the dimension limit (4096, 1024), K = 1: HIP-event time of each call, median of three rounds, the Jacobi's sweep counts, and the FP64 floor of
     k_dstr_cov's and k_dstr_pairs' own operation counts at bench.py's FP64_PEAK_TFLOPS;
  2. the split between the kernels: KERNEL_STATS=<csv> names the kernel-stats table of a `rocprofv3 --kernel-trace --stats
     --output-format csv` run of this tool with KERNELS_ONLY=1 and SHAPE=<index of one (n, D, K) case> (KERNEL_STATS_SHAPE names
     that index to the later run; 3, the (50,000, 128, 7) case, by default);
  3. the worst differences to the float64 oracle (tests/distribution_oracle.py) at the test shapes, through the public functions;
  4. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without distribution=True, nine passes each, alternated;
  5. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, three timed passes each per round (exp_phase.py's comparison).
Prints one JSON line (and writes it to OUT_DIR/distribution.json when OUT_DIR is set).  Nothing here is a threshold."""
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
import exp_auditory as A       # noqa: E402  (the spread of rounds)
import exp_phase as P          # noqa: E402  (the tree, the event timer and the parent comparison)

SHAPES = [(4096, 128, 1), (4096, 128, 7), (50000, 128, 1), (50000, 128, 7), (4096, 512, 1), (4096, 512, 7), (4096, 1024, 1)]      # (n = m, D, K)


def cov_flop(n, D, K):
    """k_dstr_cov: an FMA (2) per row and column pair of the tiles tj >= ti (edge 64), 1 + K sets."""
    t = -(-D // 64)
    return 2.0 * n * (t * (t + 1) // 2) * 64 * 64 * (1 + K)


def pairs_flop(n, D, K):
    """k_dstr_pairs: a subtraction and an FMA (3) per row pair and dimension; a set's own combination takes the tiles tj >= ti."""
    t = -(-n // 64)
    own, cross = (t * (t + 1) // 2) * 64 * 64, t * t * 64 * 64
    return 3.0 * D * ((1 + K) * own + K * cross)


def kernel_times(shapes):
    import torch
    import bench
    from ssr_eval_amd import _lib, backend as B
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    out = []
    for n, D, K in shapes:
        g = torch.Generator(device=dev).manual_seed(2)
        data = torch.randn(((1 + K) * n, D), generator=g, device=dev, dtype=torch.float32) * torch.linspace(1.0, 0.05, D, device=dev)
        data[n:] = 1.1 * data[n:] + 0.05
        rows = np.full(1 + K, n, np.int64)
        off = np.arange(1 + K, dtype=np.int64) * n * D
        fd_out = torch.empty((K, 8), dtype=torch.float64, device=dev)
        kd_out = torch.empty((K, 1, 4), dtype=torch.float64, device=dev)
        gamma = np.array([1.0 / (2.0 * float(D) * 0.35)], np.float64)
        fd_bytes, kd_bytes = int(lib.ssr_frechet_workspace_bytes(hp(rows), K, D)), int(lib.ssr_kernel_distance_workspace_bytes(hp(rows), K, D, 1))
        ws = torch.empty(max(fd_bytes, kd_bytes), dtype=torch.uint8, device=dev)

        def fd():
            _lib.check(lib.ssr_frechet(B._vp(data), 0, hp(off), hp(rows), K, D, D, 60, B._vp(fd_out), None, B._vp(ws), fd_bytes, B._stream()))

        def kd():
            _lib.check(lib.ssr_kernel_distance(B._vp(data), 0, hp(off), hp(rows), K, D, D, hp(gamma), 1, 1000.0, B._vp(kd_out), B._vp(ws), kd_bytes,
                                               B._stream()))
        r = {"n": n, "m": n, "D": D, "K": K, "dtype": "float32", "frechet_workspace_mib": round(fd_bytes / 2 ** 20, 1),
             "kernel_distance_workspace_mib": round(kd_bytes / 2 ** 20, 1)}
        if os.environ.get("KERNELS_ONLY") == "1":
            fd(); kd()
            torch.cuda.synchronize()
        else:
            r["frechet"] = A.spread(torch, fd, 1, 3 if D < 1024 else 1)      # (seconds per call at the dimension limit)
            r["kernel_distance"] = A.spread(torch, kd, 1, 3)
        o = fd_out.cpu().numpy()
        r["sweeps_ref"], r["sweeps_est_max"], r["fd_median"], r["kd_median"] = int(o[0, 5]), int(o[:, 6].max()), float(np.median(o[:, 0])), \
            float(kd_out[:, 0, 0].median().cpu())
        r["cov_fp64_floor_ms"] = cov_flop(n, D, K) / (bench.FP64_PEAK_TFLOPS * 1e12) * 1e3
        r["pairs_fp64_floor_ms"] = pairs_flop(n, D, K) / (bench.FP64_PEAK_TFLOPS * 1e12) * 1e3
        out.append(r)
        del data, ws
    return out


def kernel_stats(path, case):
    """The kernel-stats table of rocprofv3 --stats -> {kernel: calls, average microseconds} for this family's kernels, and k_dstr_cov's
    and k_dstr_pairs' time over their FP64 floors."""
    rows = {}
    for row in csv.DictReader(open(path)):
        k = row.get("Name", "")
        if "k_dstr_" in k:
            rows[k.split("(")[0].replace("void ", "")] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3}
    for name, floor in (("k_dstr_cov", case["cov_fp64_floor_ms"]), ("k_dstr_pairs", case["pairs_fp64_floor_ms"])):
        t = [v["avg_us"] for k, v in rows.items() if k.startswith(name + "<")]
        if t:
            rows[name + "_over_fp64_floor"] = t[0] / 1e3 / floor
    return rows


def oracle_differences():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import distribution_oracle as O
    from ssr_eval_amd import backend as B
    worst = {"mean": 0.0, "cov": 0.0, "fd_full_rank": 0.0, "fd_rank_deficient": 0.0, "kernel_means": 0.0}
    for shapes, key in ((O.FRECHET_SHAPES, "fd_full_rank"), (O.DEFICIENT_SHAPES, "fd_rank_deficient")):
        for d, n, m in shapes:
            r, e = O.frechet_sets(d, n, m)
            out, mom = B.frechet_stats(r, [e], return_moments=True)
            w = O.check_frechet(out, mom, [r, e], deficient=key != "fd_full_rank")
            worst["mean"], worst["cov"], worst[key] = max(worst["mean"], w[0]), max(worst["cov"], w[1]), max(worst[key], w[2])
    for n, m, d in O.KERNEL_SHAPES:
        r, e = O.gaussian_set(n, d, 1, 10.0, scale=1.0 / np.sqrt(d)), O.gaussian_set(m, d, 2, 10.0, shift=0.1, scale=1.0 / np.sqrt(d))
        got = B.kernel_sums(r, [e], O.GAMMAS8)
        worst["kernel_means"] = max(worst["kernel_means"], float(np.max(np.abs(got[0, :, 1:] - O.kernel_means(r, e, O.GAMMAS8)[:, 1:]))))
    return worst


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, distribution=v) for name, v in (("plain", None), ("distribution", True))}
    last = {}
    for k, h in hs.items():
        h.evaluate(limit_test_nums=2, limit_test_speaker=1, save_json=False)
        last[k] = h.evaluate(save_json=False)
    times = {k: [] for k in hs}
    for _ in range(9):
        for k, h in hs.items():
            t0 = time.perf_counter()
            h.evaluate(save_json=False)
            times[k].append(time.perf_counter() - t0)
    return {k: {"files_per_s": round(n_files / float(np.median(v)), 1), "pass_s": [round(x, 4) for x in v]} for k, v in times.items()} | \
        {"n_files": n_files, "block": last["distribution"]["distribution"]}


def main():
    sys.path.insert(0, ROOT)
    res = {"tool": "exp_distribution", "tuned": False}
    shapes = SHAPES if os.environ.get("SHAPE") is None else [SHAPES[int(os.environ["SHAPE"])]]
    if os.environ.get("KERNELS_ONLY") == "1":
        res["kernel"] = kernel_times(shapes)
        print(json.dumps(res), flush=True)
        return
    root = tempfile.mkdtemp(prefix="ssr_dstr_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_distribution_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernel"] = kernel_times(shapes)
        if os.environ.get("KERNEL_STATS"):
            case = SHAPES[int(os.environ.get("KERNEL_STATS_SHAPE", "3"))]
            res["kernel_stats"] = {"n": case[0], "D": case[1], "K": case[2]} | \
                kernel_stats(os.environ["KERNEL_STATS"], next(k for k in res["kernel"] if (k["n"], k["D"], k["K"]) == case))
        res["oracle_differences"] = oracle_differences()
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree(root, n_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "distribution.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
