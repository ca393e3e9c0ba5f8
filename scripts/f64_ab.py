#!/usr/bin/env python3
"""FP64 MFMA GEMM vs the vendor library (torch.matmul on float64) at the
same M = N = K.

mfma_gemm_f64_128 and torch.matmul INTERLEAVED in one process (both within
every round) so clock drift hits both alike; device-event timing around
each launch, median and p10-p90 over the rounds. Standard-normal data on
both sides; the two results are compared once per size before timing
(largest |difference| over the gamma_K bound of tests/test_gpu_fp64.py).
Prints one JSON line per size; pass sizes and rounds as argv:
f64_ab.py 2048,4096,8192 40
"""

import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from k8s_cc_manager_amd.ops import attest
from mxfp4_ab import timed


def bench(n: int, rounds: int) -> dict:
    g = torch.Generator(device="cuda").manual_seed(n)
    a = torch.randn(n, n, device="cuda", generator=g, dtype=torch.float64)
    bt = torch.randn(n, n, device="cuda", generator=g, dtype=torch.float64)
    b = bt.t()  # the library reads Bt through a transposed view: no copy
    c = torch.empty(n, n, device="cuda", dtype=torch.float64)
    c_lib = torch.empty(n, n, device="cuda", dtype=torch.float64)
    arms = {
        "f64": lambda: attest.mfma_gemm_f64(
            0, a.data_ptr(), bt.data_ptr(), c.data_ptr(), n, n, n),
        "lib": lambda: torch.matmul(a, b, out=c_lib),
    }
    for _ in range(3):  # warm both
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ku = n * 2.0**-53
    bound = 2 * ku / (1 - ku) * (a.abs() @ b.abs())
    ratio = float(((c - c_lib).abs() / bound).max())
    del bound
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    tf = {k: 2.0 * n**3 / (v * 1e-3) / 1e12 for k, v in med.items()}
    out = {"kind": "f64_ab", "n": n, "rounds": rounds,
           "max_diff_over_bound": round(ratio, 4)}
    for k in arms:
        q = statistics.quantiles(ms[k], n=10)
        out[f"{k}_ms_med"] = round(med[k], 4)
        out[f"{k}_ms_p10_p90"] = [round(q[0], 4), round(q[-1], 4)]
        out[f"{k}_tflops_med"] = round(tf[k], 2)
        # the arm against itself: the middle 80 % of its rounds over its median
        out[f"{k}_spread_p10_p90"] = [round(med[k] / q[-1], 3),
                                      round(med[k] / q[0], 3)]
    out["f64_over_lib"] = round(tf["f64"] / tf["lib"], 3)
    return out


def main():
    sizes = ([int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1
             else [2048, 4096, 8192])
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    for n in sizes:
        print(json.dumps(bench(n, rounds)), flush=True)


if __name__ == "__main__":
    main()
