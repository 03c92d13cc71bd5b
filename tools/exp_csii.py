"""Developer tool: the coherence speech intelligibility index on the GPU.
  1. 1024 resident pairs of 4 s in float32 at 48 kHz (n_fft 1024, hop 512, 21 bands) and at 16 kHz (n_fft 256, hop 128, 20 bands):
     HIP-event time of ssr_csii and - in the same run, on the same signals, at the same n_fft and hop - of ssr_coherence on one full
     band, the ratio of the two and the workspace of each; and of ssr_csii on all 1024 targets with ONE estimate, which is
     k_csii_levels (one workgroup per target, a lane per segment) next to one pair's spectra and bands;
  2. SSR_Eval_Helper.evaluate() files/s on bench.py's generated 367-file 44.1 kHz tree (FFT key 12 kHz, evaluation 48 kHz), with and
     without csii=True, 9 passes each, alternated (SKIP_EVALUATE=1 leaves it out);
  3. with SSR_PARENT_ROOT=<a built checkout of the parent commit>: evaluate() WITHOUT the option from that checkout and from this
     one, in child processes alternated on the same tree, 9 passes each (exp_phase.py's comparison).
Prints one JSON line (and writes it to OUT_DIR/csii.json when OUT_DIR is set).  No speed bar is set: the times are recorded."""
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


def kernel_times(rate, n_pairs=1024, seconds=4):
    import torch
    from ssr_eval_amd import _lib, backend as B
    n_samples = seconds * rate
    n_fft = B.csii_default_nfft(rate)
    hop = n_fft // 2
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    tg = torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    tg *= (0.05 + torch.rand((n_pairs, n_samples // 480 + 1), generator=g, device=dev)).repeat_interleave(480, dim=1)[:, :n_samples]
    es = tg + 0.3 * torch.randn((n_pairs, n_samples), generator=g, device=dev, dtype=torch.float32)
    lib = _lib.load()
    _, imp, W = B.csii_design(rate, n_fft)
    J = len(imp)
    lens, idx = np.full(n_pairs, n_samples, np.int32), np.arange(n_pairs, dtype=np.int32)
    split, bands = np.full(n_pairs, J // 2, np.int32), np.tile(np.array([[0, n_fft // 2]], np.int32), (n_pairs, 1, 1))
    off = torch.arange(n_pairs, dtype=torch.int64, device=dev) * n_samples
    pinned = [torch.from_numpy(a).pin_memory() for a in (lens, idx, split, bands, imp)]
    ptr = [C.c_void_p(p.data_ptr()) for p in pinned]
    w_dev = torch.from_numpy(W).to(dev)
    K = 1 + (n_samples - n_fft) // hop
    res = {"n_pairs": n_pairs, "seconds_per_pair": seconds, "rate": rate, "dtype": "float32", "n_fft": n_fft, "hop": hop, "n_bands": J,
           "segments_per_pair": K, "chunks_per_pair": -(-K // 32)}
    out = torch.empty((n_pairs, B.CSII_COLUMNS), dtype=torch.float64, device=dev)
    ws_bytes = int(lib.ssr_csii_workspace_bytes(ptr[0], n_pairs, ptr[1], n_pairs, n_fft, hop, J))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    res["workspace_mib"] = round(ws_bytes / 2 ** 20, 1)

    def csii():
        _lib.check(lib.ssr_csii(B._vp(tg), 0, B._vp(off), ptr[0], n_pairs, B._vp(es), 0, B._vp(off), ptr[1], n_pairs, n_fft, hop, J, B._vp(w_dev),
                                ptr[4], ptr[2], B._vp(out), None, B._vp(ws), ws_bytes, B._stream()))
    res["csii"] = spread(torch, csii, 5)

    def levels_mostly():      # every target is classified, one pair is scored: k_csii_levels next to 12 spectra workgroups
        _lib.check(lib.ssr_csii(B._vp(tg), 0, B._vp(off), ptr[0], n_pairs, B._vp(es), 0, B._vp(off), ptr[1], 1, n_fft, hop, J, B._vp(w_dev),
                                ptr[4], ptr[2], B._vp(out), None, B._vp(ws), ws_bytes, B._stream()))
    res["csii_all_targets_one_estimate"] = spread(torch, levels_mostly, 5)
    csii()                    # (the medians below are of the full call)
    torch.cuda.synchronize()
    med = out.nanmedian(dim=0).values.cpu()
    res["median_csii"], res["median_i3"], res["median_segments_low_mid_high"] = float(med[0]), float(med[4]), [float(v) for v in med[10:13]]
    del ws
    cout = torch.empty((n_pairs, 1, 3), dtype=torch.float64, device=dev)
    cws_bytes = int(lib.ssr_coherence_workspace_bytes(ptr[0], n_pairs, ptr[1], n_pairs, n_fft, hop, 1))
    cws = torch.empty(cws_bytes, dtype=torch.uint8, device=dev)
    res["coherence_workspace_mib"] = round(cws_bytes / 2 ** 20, 1)

    def coh():
        _lib.check(lib.ssr_coherence(B._vp(tg), 0, B._vp(off), ptr[0], n_pairs, B._vp(es), 0, B._vp(off), ptr[1], n_pairs, n_fft, hop, 1,
                                     ptr[3], 0.5, B._vp(cout), None, B._vp(cws), cws_bytes, B._stream()))
    res["coherence_same_frames"] = spread(torch, coh, 5)
    res["csii_over_coherence"] = res["csii"]["median_ms"] / res["coherence_same_frames"]["median_ms"]
    return res


def evaluate_tree(root, n_files):
    from ssr_eval_amd import SSR_Eval_Helper, BasicTestee
    hs = {name: SSR_Eval_Helper(BasicTestee(), input_sr=44100, output_sr=44100, evaluation_sr=48000, test_data_root=root,
                                setting_fft={"cutoff_freq": [12000]}, csii=v) for name, v in (("plain", None), ("csii", True))}
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
    res = {"tool": "exp_csii"}
    root = tempfile.mkdtemp(prefix="ssr_csii_")
    try:
        n_files = P.write_tree(root)
        # the child processes first: one process with the GPU open at a time
        if os.environ.get("SSR_PARENT_ROOT"):
            res["evaluate_without_csii_parent_vs_new"] = P.parent_ab(root, n_files, os.path.abspath(os.environ["SSR_PARENT_ROOT"]))
        res["kernel_48k"] = kernel_times(48000)
        res["kernel_16k"] = kernel_times(16000)
        if os.environ.get("SKIP_EVALUATE") != "1":
            res["evaluate"] = evaluate_tree(root, n_files)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("OUT_DIR"):
        os.makedirs(os.environ["OUT_DIR"], exist_ok=True)
        open(os.path.join(os.environ["OUT_DIR"], "csii.json"), "w").write(line + "\n")


if __name__ == "__main__":
    main()
