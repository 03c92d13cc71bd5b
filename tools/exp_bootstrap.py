"""Developer tool: the bootstrap of the aggregate on the GPU on a table of the VCTK test set's shape
(8 speakers of 424 / 424 / 123 / 419 / 301 / 424 / 424 / 398 files = 2,937 rows).  For K = 148 (37 keys x 4 metrics) and K = 777
columns and B = 2,000 and 10,000 replicates, per configuration and resampling scheme:
  1. HIP-event time of ssr_bootstrap_means (k_boot_means + k_boot_mask) and of ssr_bootstrap_summary (k_boot_summary), table
     and replicates resident on the device;
  2. the achieved gather rate B N K 8 / t of the means call (bytes of table rows gathered per second; the table itself is
     N K 8 bytes and stays in L2 / MALL);
  3. the NumPy oracle (tests/bootstrap_oracle.py) on the same box: timed on ORACLE_REPS replicates (default 16) and scaled to B - its
     time is linear in B - and the largest deviation of the GPU's first ORACLE_REPS replicates from it.
Prints one JSON line and writes it to profiles/bootstrap.json (or OUT_DIR/bootstrap.json when OUT_DIR is set)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ssr_eval_amd import _lib, backend as B  # noqa: E402
import bootstrap_oracle as O  # noqa: E402

SPEAKERS = (424, 424, 123, 419, 301, 424, 424, 398)
QS = np.array([0.025, 0.975])


def events_ms(fn, reps):
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


def run_case(K, n_boot, scheme, oracle_reps):
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    off = np.concatenate(([0], np.cumsum(SPEAKERS))).astype(np.int32)
    N = int(off[-1])
    host = 1.0 + np.random.default_rng(K).standard_normal((N, K))
    table = torch.from_numpy(host).to(dev)
    reps = torch.empty((n_boot, K), dtype=torch.float64, device=dev)
    out = torch.empty((K, 2 + len(QS)), dtype=torch.float64, device=dev)
    counts = torch.empty((K, 2), dtype=torch.int32, device=dev)
    code = B.BOOTSTRAP_SCHEMES[scheme]

    def means():
        _lib.check(lib.ssr_bootstrap_means(B._vp(table), N, K, off.ctypes.data_as(C.c_void_p), len(SPEAKERS), n_boot, 7, code,
                                           B._vp(reps), B._stream()))

    def summary():
        _lib.check(lib.ssr_bootstrap_summary(B._vp(reps), n_boot, K, QS.ctypes.data_as(C.c_void_p), len(QS), B._vp(out), B._vp(counts),
                                             B._stream()))
    res = {"K": K, "n_boot": n_boot, "N": N, "scheme": scheme, "table_bytes": N * K * 8}
    res["means_ms"] = events_ms(means, 5)
    res["summary_ms"] = events_ms(summary, 5)
    res["gathered_bytes"] = float(n_boot) * N * K * 8
    res["gather_GBps"] = res["gathered_bytes"] / (res["means_ms"] * 1e-3) / 1e9
    t0 = time.perf_counter()
    want = O.replicates(host, off, oracle_reps, 7, scheme)
    dt = time.perf_counter() - t0
    res["oracle_reps_timed"] = oracle_reps
    res["oracle_s_per_replicate"] = dt / oracle_reps
    res["oracle_s_scaled_to_B"] = dt / oracle_reps * n_boot
    res["max_abs_dev_from_oracle"] = float(np.abs(reps[:oracle_reps].cpu().numpy() - want).max())
    return res


def main():
    oracle_reps = int(os.environ.get("ORACLE_REPS", "16"))
    res = {"tool": "exp_bootstrap", "device": torch.cuda.get_device_name(0), "cases": []}
    for K in (148, 777):
        for n_boot in (2000, 10000):
            for scheme in ("utterance", "speaker"):
                res["cases"].append(run_case(K, n_boot, scheme, oracle_reps))
                torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    out_dir = os.environ.get("OUT_DIR") or os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bootstrap.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
