#!/usr/bin/env python3
"""MXFP4 vs fp8 GEMM A/B at the same M = N = K.

mfma_gemm_mxfp4_128u against the production fp8 dispatch, INTERLEAVED
in one process (fp4, fp8, fp4, fp8 ... within every round) so clock
drift hits both alike; device-event timing around each launch, median
over the rounds. Random data on both sides (all 16 e2m1 codes, scale
bytes 126..128; fp8 from randn). Prints one JSON line per size; pass
sizes and rounds as argv: mxfp4_ab.py 4096,8192 25
"""

import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from k8s_cc_manager_amd.ops import attest


def timed(fn) -> float:
    """One launch between two device events, in ms. The entry points
    launch on the null stream, which is torch's default stream."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench(n: int, rounds: int) -> dict:
    g = torch.Generator(device="cuda").manual_seed(n)
    a4 = torch.randint(0, 256, (n, n // 2), device="cuda", generator=g, dtype=torch.uint8)
    b4 = torch.randint(0, 256, (n, n // 2), device="cuda", generator=g, dtype=torch.uint8)
    sa = torch.randint(126, 129, (n, n // 32), device="cuda", generator=g, dtype=torch.uint8)
    sb = torch.randint(126, 129, (n, n // 32), device="cuda", generator=g, dtype=torch.uint8)
    a8 = torch.randn(n, n, device="cuda", generator=g).to(torch.float8_e4m3fn)
    b8 = torch.randn(n, n, device="cuda", generator=g).to(torch.float8_e4m3fn)
    c4 = torch.empty(n, n, device="cuda", dtype=torch.float32)
    c8 = torch.empty(n, n, device="cuda", dtype=torch.float32)

    def fp4():
        attest.mfma_gemm_mxfp4(0, a4.data_ptr(), sa.data_ptr(), b4.data_ptr(),
                               sb.data_ptr(), c4.data_ptr(), n, n, n)

    def fp8():
        attest.mfma_gemm_fp8(0, a8.data_ptr(), b8.data_ptr(), c8.data_ptr(), n, n, n)

    for _ in range(3):  # warm both
        fp4()
        fp8()
    torch.cuda.synchronize()
    ms4, ms8 = [], []
    for _ in range(rounds):
        ms4.append(timed(fp4))
        ms8.append(timed(fp8))
    flop = 2.0 * n**3
    t4 = flop / (statistics.median(ms4) * 1e-3) / 1e12
    t8 = flop / (statistics.median(ms8) * 1e-3) / 1e12
    return {
        "kind": "mxfp4_ab",
        "n": n,
        "rounds": rounds,
        "mxfp4_ms_med": round(statistics.median(ms4), 4),
        "fp8_ms_med": round(statistics.median(ms8), 4),
        "mxfp4_ms_min_max": [round(min(ms4), 4), round(max(ms4), 4)],
        "fp8_ms_min_max": [round(min(ms8), 4), round(max(ms8), 4)],
        "mxfp4_tflops_med": round(t4, 1),
        "fp8_tflops_med": round(t8, 1),
        "mxfp4_over_fp8": round(t4 / t8, 3),
    }


def main():
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 8192]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    for n in sizes:
        print(json.dumps(bench(n, rounds)), flush=True)


if __name__ == "__main__":
    main()
