#!/usr/bin/env python3
"""MXFP8 (three format pairs) vs the production fp8 dispatch at the same
M = N = K.

mfma_gemm_mxfp8_128<0,0>, <1,1> and <0,1> and the production fp8
dispatch (mfma_gemm_fp8_128u at these grids), INTERLEAVED in one process
(all four within every round) so clock drift hits all alike; device-event
timing around each launch, median over the rounds. Random finite data:
random bytes with the non-finite codes of each format cleared, scale
bytes 126..128; the fp8 arm reads the same e4m3 bytes with its unit
scales. Prints one JSON line per size, with the fp8 arm's own
round-to-round spread next to the ratios; pass sizes and rounds as argv:
mxfp8_ab.py 4096,8192 40
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

    def rand_u8(cols, lo=0, hi=256):
        return torch.randint(lo, hi, (n, cols), device="cuda", generator=g,
                             dtype=torch.uint8)

    def e4m3(x):  # NaN at S.1111.111
        return torch.where((x & 0x7F) == 0x7F, torch.zeros_like(x), x)

    def e5m2(x):  # Inf and NaN at exponent 31
        return torch.where((x & 0x7C) == 0x7C, x & 0x83, x)

    ops = {0: (e4m3(rand_u8(n)), e4m3(rand_u8(n))),
           1: (e5m2(rand_u8(n)), e5m2(rand_u8(n)))}
    sa, sb = rand_u8(n // 32, 126, 129), rand_u8(n // 32, 126, 129)
    pairs = {"e4m3_e4m3": (0, 0), "e5m2_e5m2": (1, 1), "e4m3_e5m2": (0, 1)}
    c = {k: torch.empty(n, n, device="cuda", dtype=torch.float32)
         for k in list(pairs) + ["fp8"]}

    def mx8(name):
        fa, fb = pairs[name]
        a, bt = ops[fa][0], ops[fb][1]
        return lambda: attest.mfma_gemm_mxfp8(
            0, a.data_ptr(), sa.data_ptr(), bt.data_ptr(), sb.data_ptr(),
            c[name].data_ptr(), n, n, n, fa, fb)

    arms = {name: mx8(name) for name in pairs}
    arms["fp8"] = lambda: attest.mfma_gemm_fp8(
        0, ops[0][0].data_ptr(), ops[0][1].data_ptr(), c["fp8"].data_ptr(),
        n, n, n)
    for _ in range(3):  # warm all
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    tf = {k: 2.0 * n**3 / (v * 1e-3) / 1e12 for k, v in med.items()}
    out = {"kind": "mxfp8_ab", "n": n, "rounds": rounds}
    for k in arms:
        out[f"{k}_ms_med"] = round(med[k], 4)
        out[f"{k}_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out[f"{k}_tflops_med"] = round(tf[k], 1)
    for k in pairs:
        out[f"{k}_over_fp8"] = round(tf[k] / tf["fp8"], 3)
    # the fp8 arm against itself: the middle 80 % of its rounds over its median
    q = statistics.quantiles(ms["fp8"], n=10)
    out["fp8_spread_p10_p90"] = [round(med["fp8"] / q[-1], 3),
                                 round(med["fp8"] / q[0], 3)]
    return out


def main():
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 8192]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    for n in sizes:
        print(json.dumps(bench(n, rounds)), flush=True)


if __name__ == "__main__":
    main()
