#!/usr/bin/env python3
"""MXFP6 (both formats) vs MXFP4 vs fp8 GEMM A/B at the same M = N = K.

mfma_gemm_mxfp6_128<2> and <3>, mfma_gemm_mxfp4_128u and the production
fp8 dispatch, INTERLEAVED in one process (e2m3, e3m2, fp4, fp8 within
every round) so clock drift hits all alike; device-event timing around
each launch, median over the rounds. Random data everywhere (random
bytes are all 64 fp6 and all 16 fp4 codes, scale bytes 126..128; fp8
from randn). Prints one JSON line per size; pass sizes and rounds as
argv: mxfp6_ab.py 4096,8192 25
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

    a6, b6 = rand_u8(n // 4 * 3), rand_u8(n // 4 * 3)
    a4, b4 = rand_u8(n // 2), rand_u8(n // 2)
    sa, sb = rand_u8(n // 32, 126, 129), rand_u8(n // 32, 126, 129)
    a8 = torch.randn(n, n, device="cuda", generator=g).to(torch.float8_e4m3fn)
    b8 = torch.randn(n, n, device="cuda", generator=g).to(torch.float8_e4m3fn)
    c = {k: torch.empty(n, n, device="cuda", dtype=torch.float32)
         for k in ("e2m3", "e3m2", "mxfp4", "fp8")}
    arms = {
        "e2m3": lambda: attest.mfma_gemm_mxfp6(
            0, a6.data_ptr(), sa.data_ptr(), b6.data_ptr(), sb.data_ptr(),
            c["e2m3"].data_ptr(), n, n, n, 2),
        "e3m2": lambda: attest.mfma_gemm_mxfp6(
            0, a6.data_ptr(), sa.data_ptr(), b6.data_ptr(), sb.data_ptr(),
            c["e3m2"].data_ptr(), n, n, n, 3),
        "mxfp4": lambda: attest.mfma_gemm_mxfp4(
            0, a4.data_ptr(), sa.data_ptr(), b4.data_ptr(), sb.data_ptr(),
            c["mxfp4"].data_ptr(), n, n, n),
        "fp8": lambda: attest.mfma_gemm_fp8(
            0, a8.data_ptr(), b8.data_ptr(), c["fp8"].data_ptr(), n, n, n),
    }
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
    out = {"kind": "mxfp6_ab", "n": n, "rounds": rounds}
    for k in arms:
        out[f"{k}_ms_med"] = round(med[k], 4)
        out[f"{k}_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out[f"{k}_tflops_med"] = round(tf[k], 1)
    for k in ("e2m3", "e3m2"):
        out[f"{k}_over_fp8"] = round(tf[k] / tf["fp8"], 3)
        out[f"{k}_over_mxfp4"] = round(tf[k] / tf["mxfp4"], 3)
    return out


def main():
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 8192]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    for n in sizes:
        print(json.dumps(bench(n, rounds)), flush=True)


if __name__ == "__main__":
    main()
