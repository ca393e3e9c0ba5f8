#!/usr/bin/env python3
"""INT8 (both integer MFMA shapes) vs the production fp8 dispatch at the
same M = N = K.

mfma_gemm_i8_128<0> (32x32x32 op), <1> (16x16x64 op) and the production
fp8 dispatch (mfma_gemm_fp8_128u at these grids), INTERLEAVED in one
process (all three within every round) so clock drift hits all alike;
device-event timing around each launch, median over the rounds. Random
full-range bytes for int8; the fp8 arm reads random bytes with e4m3's NaN
codes cleared. Both int8 results are compared with each other once before
timing (bitwise). Prints one JSON line per size, with the fp8 arm's own
round-to-round spread next to the ratios; pass sizes and rounds as argv:
int8_ab.py 4096,8192 40
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

    def rand_i8():
        return torch.randint(-128, 128, (n, n), device="cuda", generator=g,
                             dtype=torch.int8)

    def e4m3(x):  # NaN at S.1111.111
        u = x.view(torch.uint8)
        return torch.where((u & 0x7F) == 0x7F, torch.zeros_like(u), u)

    a, bt = rand_i8(), rand_i8()
    a8, bt8 = e4m3(a), e4m3(bt)
    names = {"i8_32x32x32": 0, "i8_16x16x64": 1}
    c = {k: torch.empty(n, n, device="cuda", dtype=torch.int32) for k in names}
    c["fp8"] = torch.empty(n, n, device="cuda", dtype=torch.float32)

    def i8(name):
        return lambda: attest.mfma_gemm_i8(
            0, a.data_ptr(), bt.data_ptr(), c[name].data_ptr(), n, n, n,
            names[name])

    arms = {name: i8(name) for name in names}
    arms["fp8"] = lambda: attest.mfma_gemm_fp8(
        0, a8.data_ptr(), bt8.data_ptr(), c["fp8"].data_ptr(), n, n, n)
    for _ in range(3):  # warm all
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    same = torch.equal(c["i8_32x32x32"], c["i8_16x16x64"])
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    tops = {k: 2.0 * n**3 / (v * 1e-3) / 1e12 for k, v in med.items()}
    out = {"kind": "int8_ab", "n": n, "rounds": rounds,
           "i8_shapes_agree_bitwise": same}
    for k in arms:
        out[f"{k}_ms_med"] = round(med[k], 4)
        out[f"{k}_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out[f"{k}_tops_med"] = round(tops[k], 1)
    for k in names:
        out[f"{k}_over_fp8"] = round(tops[k] / tops["fp8"], 3)
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
