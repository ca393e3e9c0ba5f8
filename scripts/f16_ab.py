#!/usr/bin/env python3
"""FP16 (both f16 MFMA shapes) vs bf16 at the same M = N = K.

mfma_gemm_f16_128<0> (32x32x16 op), <1> (16x16x32 op), the production
bf16 dispatch and the forced bf16 variant 3 (mfma_gemm_bf16_128u: the same
bytes, tile and single-buffered structure as the fp16 kernel), INTERLEAVED
in one process (all four within every round) so clock drift hits all
alike; device-event timing around each launch, median over the rounds.
Standard-normal data, the same values rounded to each type. Both fp16
results are compared with each other once before timing. Prints one JSON
line per size, with the bf16 128u arm's own round-to-round spread next to
the ratios and whether the fp16 32x32x16 median lies inside it; pass sizes
and rounds as argv: f16_ab.py 4096,8192 40
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
    a32 = torch.randn(n, n, device="cuda", generator=g)
    bt32 = torch.randn(n, n, device="cuda", generator=g)
    a16, bt16 = a32.half(), bt32.half()
    abf, btbf = a32.bfloat16(), bt32.bfloat16()
    del a32, bt32
    names = {"f16_32x32x16": 0, "f16_16x16x32": 1}
    arms = {}
    c = {k: torch.empty(n, n, device="cuda", dtype=torch.float32)
         for k in (*names, "bf16", "bf16_128u")}

    def f16(name):
        return lambda: attest.mfma_gemm_f16(
            0, a16.data_ptr(), bt16.data_ptr(), c[name].data_ptr(), n, n, n,
            names[name])

    for name in names:
        arms[name] = f16(name)
    arms["bf16"] = lambda: attest.mfma_gemm_bf16(
        0, abf.data_ptr(), btbf.data_ptr(), c["bf16"].data_ptr(), n, n, n)
    arms["bf16_128u"] = lambda: attest.mfma_gemm_bf16_variant(
        0, abf.data_ptr(), btbf.data_ptr(), c["bf16_128u"].data_ptr(), n, n, n,
        3)
    for _ in range(3):  # warm all
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    diff = (c["f16_32x32x16"] - c["f16_16x16x32"]).abs().max().item()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    tf = {k: 2.0 * n**3 / (v * 1e-3) / 1e12 for k, v in med.items()}
    out = {"kind": "f16_ab", "n": n, "rounds": rounds,
           "f16_shapes_max_abs_diff": diff}
    for k in arms:
        out[f"{k}_ms_med"] = round(med[k], 4)
        out[f"{k}_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out[f"{k}_tflops_med"] = round(tf[k], 1)
    for k in names:
        out[f"{k}_over_bf16"] = round(tf[k] / tf["bf16"], 3)
        out[f"{k}_over_bf16_128u"] = round(tf[k] / tf["bf16_128u"], 3)
    # the 128u arm against itself: the middle 80 % of its rounds
    q = statistics.quantiles(ms["bf16_128u"], n=10)
    out["bf16_128u_ms_p10_p90"] = [round(q[0], 4), round(q[-1], 4)]
    out["f16_32x32x16_inside_128u_p10_p90"] = q[0] <= med["f16_32x32x16"] <= q[-1]
    return out


def main():
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 8192]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    for n in sizes:
        print(json.dumps(bench(n, rounds)), flush=True)


if __name__ == "__main__":
    main()
