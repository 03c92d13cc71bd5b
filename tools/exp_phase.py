"""Developer tool: the anti-wrapping phase distances on the GPU.
  1. 1024 pairs of 4 s at 48 kHz in float32, n_fft 1024, hop 256: HIP-event time of ssr_phase_metrics for which = 1 (IP), 3 (IP + GD)
     and 7 (all three: one warm-up frame per chunk), and of the public call (backend.phase_metrics) end to end;
  2. next to them two floors: the FP64 floor - FP64_PER_FRAME vector instructions per thread and frame (the static count of
     k_phase_dist<float, float, 10> with every branch taken, from its ISA) over the 16 FP64 lanes a SIMD retires per clock at the
     engine clock read from sysfs while the kernel runs - and the streaming-read floor, both signals once at bench.py's
     peak_measured;
  3. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without phase=True, passes alternated;
  4. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT phase from that checkout and from this one, in
     child processes alternated ROUNDS times on the same tree - the one comparison that has to hold.
Prints one JSON line (and writes it to OUT_DIR/phase.json when OUT_DIR is set)."""
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = [53, 53, 15, 52, 38, 53, 53, 50]          # bench.py's evaluate_end_to_end tree: files per speaker
# Static counts from the compiler's assembly of tu_phase.hip; they move with the kernel, so count again after any change to
# ssr_phase.h: `python tools/isa_stats.py <the .s hipcc --save-temps writes for tu_phase.hip> k_phase_dist --blocks` gives the
# v_f64 count per block (1,129 in the whole of k_phase_dist<float, float, 10>, about 1,100 of them inside the frame loop; 14 atan2
# blocks of 45 - 49).
FP64_PER_FRAME = 1100                            # v_*_f64 in the frame loop of k_phase_dist<float, float, 10>
FP64_PER_FRAME_IP = 1100 - 9 * 53                # without the GD and IAF products and arguments (6 + 47 each, 4 + 5 per thread)
SIMDS, FP64_LANES_PER_CLOCK = 256 * 4, 16
ROUNDS = 3


def write_tree(root):
    from ssr_eval_amd.io import write_wav
    rng = np.random.default_rng(4)
    n_files = 0
    for s, c in enumerate(TREE):
        os.makedirs(os.path.join(root, "p%03d" % (360 + s)))
        for i in range(c):
            n = int(rng.integers(int(1.5 * 44100), 9 * 44100))
            write_wav(os.path.join(root, "p%03d" % (360 + s), "u%03d.wav" % i), 0.1 * rng.standard_normal(n), 44100)
            n_files += 1
    return n_files


def child(root, passes):
    """Timed evaluate() passes without phase by the ssr_eval_amd found first on sys.path (PYTHONPATH names the checkout)."""
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    h = SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                        setting_fft={"cutoff_freq": [12000]})
    h.evaluate(limit_test_nums=2, limit_test_speaker=1, save_json=False)
    h.evaluate(save_json=False)
    out = []
    for _ in range(passes):
        t0 = time.perf_counter()
        h.evaluate(save_json=False)
        out.append(time.perf_counter() - t0)
    print("PASSES " + json.dumps(out), flush=True)


def parent_ab(root, n_files, parent_root):
    res = {"parent": [], "new": []}
    for _ in range(ROUNDS):
        for name, pkg_root in (("parent", parent_root), ("new", ROOT)):
            env = dict(os.environ, PYTHONPATH=pkg_root)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "3"], env=env, cwd=pkg_root,
                                 capture_output=True, text=True, timeout=600, check=True).stdout
            res[name] += json.loads([l for l in out.splitlines() if l.startswith("PASSES ")][-1][7:])
    fps = {k: [round(n_files / t, 1) for t in v] for k, v in res.items()}
    return {k: {"files_per_s": v, "median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in fps.items()} | \
        {"new_median_inside_parent_spread": bool(min(fps["parent"]) <= float(np.median(fps["new"])))}


def sclk_mhz():
    for f in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input"):
        try:
            return int(open(f).read().strip()) / 1e6
        except (OSError, ValueError):
            pass
    return None


def events_ms(torch, fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def kernel_times():
    import torch
    from ssr_eval_amd import _lib, backend as B
    import bench
    n_pairs, n_samples, n_fft, hop = 1024, 4 * 48000, 1024, 256
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    es = tg + 0.3 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    lens, idx = np.full(n_pairs, n_samples, np.int32), np.arange(n_pairs, dtype=np.int32)
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n_samples
    pinned = [torch.from_numpy(a).pin_memory() for a in (lens, idx)]
    T = 1 + n_samples // hop
    chunks = -(-T // 16)
    res = {"n_pairs": n_pairs, "frames_per_pair": T, "chunks_per_pair": chunks, "n_fft": n_fft, "hop": hop}
    out = torch.empty((n_pairs, 3), dtype=torch.float64, device=dev)
    clocks, stop = [], threading.Event()

    def poll():
        while not stop.is_set():
            c = sclk_mhz()
            if c:
                clocks.append(c)
            time.sleep(0.02)
    for which in (1, 3, 7):
        ws_bytes = int(lib.ssr_phase_metrics_workspace_bytes(lens.ctypes.data_as(C.c_void_p), n_pairs, idx.ctypes.data_as(C.c_void_p),
                                                             n_pairs, n_fft, hop, which))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(lib.ssr_phase_metrics(B._vp(tg), 0, B._vp(off), C.c_void_p(pinned[0].data_ptr()), n_pairs, B._vp(es), 0, B._vp(off),
                                             C.c_void_p(pinned[1].data_ptr()), n_pairs, n_fft, hop, 0, n_fft // 2, which, B._vp(out),
                                             B._vp(ws), ws_bytes, B._stream()))
        th = None
        if which == 7:
            th = threading.Thread(target=poll)
            th.start()
        res["ms_which_%d" % which] = events_ms(torch, call, 10 if which == 7 else 5)
        if th is not None:
            stop.set()
            th.join()
    tl, el = list(tg.unbind(0)), list(es.unbind(0))
    res["api_ms_which_7"] = events_ms(torch, lambda: B.phase_metrics(tl, el, idx, n_fft, hop, None, 7, dev, deferred=True)(), 3)
    mhz = float(np.median(clocks)) if clocks else None
    res["sclk_MHz_while_running"] = mhz
    res["sclk_source"] = "hwmon freq1_input, median of %d samples" % len(clocks) if clocks else "not readable: 2400 MHz assumed"
    hz = (mhz or 2400.0) * 1e6
    waves = n_fft // 8 // 64
    for which, per_frame, frames in ((1, FP64_PER_FRAME_IP, n_pairs * T), (7, FP64_PER_FRAME, n_pairs * (T + chunks - 1))):
        cycles = frames * waves * per_frame * (64 // FP64_LANES_PER_CLOCK) / SIMDS
        res["fp64_floor_ms_which_%d" % which] = cycles / hz * 1e3
        res["over_fp64_floor_which_%d" % which] = res["ms_which_%d" % which] / res["fp64_floor_ms_which_%d" % which]
    peak = bench.measured_hbm_peak().get("read_GBs")
    res["peak_measured_GBs"] = peak
    if peak:
        res["read_floor_ms"] = 2 * n_pairs * n_samples * 4 / (peak * 1e9) * 1e3
    return res


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, phase=v) for name, v in (("plain", None), ("phase", True))}
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
        {"n_files": n_files}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]))
    sys.path.insert(0, ROOT)
    res = {"tool": "exp_phase"}
    root = tempfile.mkdtemp(prefix="ssr_phase_")
    try:
        n_files = write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_phase_parent_vs_new"] = parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernel"] = kernel_times()
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree(root, n_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "phase.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
