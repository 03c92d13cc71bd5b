"""Developer tool: the segment-parallel sosfiltfilt (exact=False) against the bit-exact kernel.
  1. 64 x 36 and 256 x 36 (files x designs; 4 filter types x 3 cutoffs x 3 orders) on 4 s float32 signals at 44.1 kHz: HIP-event
     time of ssr_sosfiltfilt_multi and of ssr_sosfiltfilt_fast (its seven kernels), 5 repeats each, every repeat timed by itself.
     The bar: on 256 x 36 the SLOWEST fast repeat is below the FASTEST exact repeat (`fast_below_exact`);
  2. the worst sample deviation max|y - scipy| / max|scipy| of exact=False over tools/stress_iir.py's random designs (those of
     <= 8 sections), float32 and float64 signals;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree with 36 IIR keys, iir_exact True and False,
     passes alternated.
Prints one JSON line (and writes it to OUT_DIR/iir_fast.json when OUT_DIR is set).  SKIP_EVALUATE=1 skips part 3."""
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ssr_eval_amd import _lib, backend as B  # noqa: E402
from ssr_eval_amd.lowpass import _design  # noqa: E402

FS = 44100
SPECS = [(c, o, f) for f in ("butter", "cheby1", "ellip", "bessel") for c in (2000, 4000, 8000) for o in (2, 5, 10)]


def each_ms(fn, reps):
    """HIP-event time of every one of `reps` calls (after two warm-up calls)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def kernel_case(n_files, reps=5):
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    rng = np.random.default_rng(n_files)
    sigs = [(0.1 * rng.standard_normal(4 * FS)).astype(np.float32) for _ in range(n_files)]
    r = B.Ragged.from_list_keep64(sigs, dev)
    designs = [_design(c, FS, o, f) for c, o, f in SPECS]
    D = len(designs)
    sos_h, zi_h = np.zeros((D, 8, 6)), np.zeros((D, 8, 2))
    for d, s_ in enumerate(designs):
        sos_h[d, :s_.shape[0]] = s_
        zi_h[d, :s_.shape[0]] = signal.sosfilt_zi(s_)
    ns = np.array([s_.shape[0] for s_ in designs], dtype=np.int32)
    eg = np.array([B._sos_edge(s_) for s_ in designs], dtype=np.int32)
    sos_d, zi_d = B._h2d(sos_h, dev), B._h2d(zi_h, dev)
    total = int(r.lens_host.sum())
    y = torch.empty((D, total), dtype=torch.float64, device=dev)
    res = {"files": n_files, "designs": D, "samples": total}
    outs = {}
    for name, ws_fn, fn in (("exact", lib.ssr_sosfiltfilt_multi_workspace_bytes, lib.ssr_sosfiltfilt_multi),
                            ("fast", lib.ssr_sosfiltfilt_fast_workspace_bytes, lib.ssr_sosfiltfilt_fast)):
        ws_bytes = int(ws_fn(total, r.n, eg.ctypes.data_as(C.c_void_p), D))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def run():
            _lib.check(fn(B._vp(r.data), B._vp(r.off), B._vp(r.len), r.n, total, B._vp(sos_d), B._vp(zi_d), ns.ctypes.data_as(C.c_void_p),
                          eg.ctypes.data_as(C.c_void_p), D, B._vp(y), total, B._vp(ws), ws_bytes, B._stream()))
        ms = each_ms(run, reps)
        res[name + "_ms"] = [round(v, 3) for v in ms]
        res[name + "_workspace_gb"] = round(ws_bytes / 1e9, 3)
        outs[name] = y[:, :4 * FS].clone()             # the first file under every design
        del ws
        torch.cuda.empty_cache()
    res["exact_over_fast"] = round(float(np.median(res["exact_ms"]) / np.median(res["fast_ms"])), 2)
    res["fast_below_exact"] = bool(max(res["fast_ms"]) < min(res["exact_ms"]))
    res["fast_gsamples_per_s"] = round(total * D / (np.median(res["fast_ms"]) * 1e-3) / 1e9, 2)
    dev_ = (outs["fast"] - outs["exact"]).abs().amax(1) / outs["exact"].abs().amax(1)
    res["worst_deviation_from_exact"] = float(dev_.max())
    return res


def stress_deviation(rounds=40):
    import stress_iir
    rng = np.random.default_rng(7)
    worst = {"float32": 0.0, "float64": 0.0}
    at = {}
    n_designs = 0
    for _ in range(rounds):
        sos = stress_iir.design(rng)
        if sos.shape[0] > 8:
            continue
        n_designs += 1
        edge = B._sos_edge(sos)
        for dt in (np.float32, np.float64):
            sigs = [(off + 0.1 * rng.standard_normal(n)).astype(dt) for n, off in ((edge + 1, 0.0), (1000, 0.5), (30000, 0.0), (4 * FS, 0.5))]
            for s_, g in zip(sigs, B.sosfiltfilt(sos, sigs, exact=False)):
                ref = signal.sosfiltfilt(sos, s_)
                e = float(np.abs(g.cpu().numpy() - ref).max() / np.abs(ref).max())
                if e > worst[np.dtype(dt).name]:
                    worst[np.dtype(dt).name] = e
                    at[np.dtype(dt).name] = {"sections": int(sos.shape[0]), "len": len(s_)}
    return {"designs": n_designs, "worst": worst, "at": at}


def evaluate_tree():
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    root = tempfile.mkdtemp(prefix="ssr_iir_fast_")
    try:
        n_files = 0
        for s, c in enumerate([53, 53, 15, 52, 38, 53, 53, 50]):           # bench.py's evaluate_end_to_end tree
            os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
            for i in range(c):
                n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
                write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
                n_files += 1
        hs = {}
        for name, v in (("iir_exact_true", True), ("iir_exact_false", False)):
            setting = {"filter": ["cheby", "butter", "bessel", "ellip"], "cutoff_freq": [1000, 2000, 4000], "filter_order": [2, 5, 10]}
            hs[name] = SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=44100, test_data_root=root,
                                       setting_lowpass_filtering=setting, iir_exact=v)
        for h in hs.values():
            h.evaluate(limit_test_nums=2, limit_test_speaker=1, save_json=False)
            h.evaluate(save_json=False)
        times = {k: [] for k in hs}
        for _ in range(3):
            for k, h in hs.items():
                t0 = time.perf_counter()
                h.evaluate(save_json=False)
                times[k].append(time.perf_counter() - t0)
        return {k: {"files_per_s": round(n_files / float(np.median(v)), 1), "pass_s": [round(x, 4) for x in v]} for k, v in times.items()} | \
            {"n_files": n_files, "keys": 36}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    res = {"tool": "exp_iir_fast", "segment": 128}
    for n in (64, 256):
        res["k%dx36" % n] = kernel_case(n)
        torch.cuda.empty_cache()
    res["stress"] = stress_deviation()
    if os.environ.get("SKIP_EVALUATE") != "1":
        res["evaluate"] = evaluate_tree()
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "iir_fast.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
