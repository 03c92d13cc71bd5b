"""Developer tool: the multi-resolution STFT distance on the GPU.
  1. 1024 resident pairs of 4 s at 48 kHz in float32: HIP-event time of ssr_mrstft_metrics with the three default resolutions in one
     call and with each of them alone, and of the public call (backend.mrstft_metrics) end to end;
  2. next to each resolution ssr_phase_metrics (SSR_PHASE_IP only) at the same (n_fft, hop): the same transform, geometry and chunking
     with an atan2 epilogue in place of the two square roots and the logarithm - the yardstick for the shared transform;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without mrstft=True, passes alternated;
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree (exp_phase.py's comparison) - the one that has to hold.
Prints one JSON line (and writes it to OUT_DIR/mrstft.json when OUT_DIR is set)."""
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


def kernel_times():
    import torch
    from ssr_eval_amd import _lib, backend as B
    n_pairs, n_samples = 1024, 4 * 48000
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = 0.1 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    es = tg + 0.03 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    lens, idx = np.full(n_pairs, n_samples, np.int32), np.arange(n_pairs, dtype=np.int32)
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n_samples
    pinned = [torch.from_numpy(a).pin_memory() for a in (lens, idx)]
    lp, ip = C.c_void_p(pinned[0].data_ptr()), C.c_void_p(pinned[1].data_ptr())
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    res = {"n_pairs": n_pairs, "seconds_per_pair": 4, "rate": 48000, "dtype": "float32"}

    def mrstft_call(resolutions):
        tab = np.ascontiguousarray(np.array([[n, h, w, 0, n // 2] for n, h, w in resolutions], np.int32).T)
        R = len(resolutions)
        out = torch.empty((n_pairs, R + 1, 2), dtype=torch.float64, device=dev)
        ws_bytes = int(lib.ssr_mrstft_workspace_bytes(vp(lens), n_pairs, vp(idx), n_pairs, R, vp(tab[0]), vp(tab[1]), vp(tab[2])))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.ssr_mrstft_metrics(B._vp(tg), 0, B._vp(off), lp, n_pairs, B._vp(es), 0, B._vp(off), ip, n_pairs, R,
                                              *[vp(tab[j]) for j in range(5)], B.MRSTFT_EPS, B._vp(out), B._vp(ws), ws_bytes, B._stream()))
        return call, (tab, out, ws)

    def phase_ip_call(n_fft, hop):
        out = torch.empty((n_pairs, 1), dtype=torch.float64, device=dev)
        ws_bytes = int(lib.ssr_phase_metrics_workspace_bytes(vp(lens), n_pairs, vp(idx), n_pairs, n_fft, hop, 1))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.ssr_phase_metrics(B._vp(tg), 0, B._vp(off), lp, n_pairs, B._vp(es), 0, B._vp(off), ip, n_pairs, n_fft, hop, 0,
                                             n_fft // 2, 1, B._vp(out), B._vp(ws), ws_bytes, B._stream()))
        return call, (out, ws)

    call, keep = mrstft_call(B.MRSTFT_RESOLUTIONS)
    res["default_resolutions"] = spread(torch, call, 3)
    res["per_resolution"] = []
    for n_fft, hop, win in B.MRSTFT_RESOLUTIONS:
        T = 1 + n_samples // hop
        call, keep = mrstft_call(((n_fft, hop, win),))
        row = {"n_fft": n_fft, "hop": hop, "win": win, "frames_per_pair": T, "chunks_per_pair": -(-T // 16),
               "mrstft": spread(torch, call, 3)}
        call, keep = phase_ip_call(n_fft, hop)
        row["phase_ip_same_n_fft_hop"] = spread(torch, call, 3)
        row["mrstft_over_phase_ip"] = row["mrstft"]["median_ms"] / row["phase_ip_same_n_fft_hop"]["median_ms"]
        res["per_resolution"].append(row)
    tl, el = list(tg.unbind(0)), list(es.unbind(0))
    res["api_default_resolutions"] = spread(torch, lambda: B.mrstft_metrics(tl, el, idx, None, None, B.MRSTFT_EPS, dev, deferred=True)(), 2, 3)
    return res


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, mrstft=v) for name, v in (("plain", None), ("mrstft", True))}
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
    res = {"tool": "exp_mrstft"}
    root = tempfile.mkdtemp(prefix="ssr_mrstft_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_mrstft_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernel"] = kernel_times()
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree(root, n_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "mrstft.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
