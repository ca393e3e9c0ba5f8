#!/usr/bin/env python3
"""2:4 sparse bf16 GEMM (both SMFMAC shapes) vs the production dense bf16
dispatch on the decompressed operand, at the same M = N = K.

mfma_gemm_sp24_128<0> (32x32x32 op), <1> (16x16x64 op) and
mfma_gemm_bf16 on sp24_dense(ac, am), INTERLEAVED in one process (all
three within every round) so clock drift hits all alike; device-event
timing around each launch, median over the rounds. Standard-normal bf16
values, random legal index nibbles. Rates are dense-equivalent, 2 n^3
over the time, for all three arms. Each sparse result is compared with
the dense one once before timing (largest |difference| over the bound of
tests/test_gpu_sparse24.py). Prints one JSON line per size, with the
dense arm's own round-to-round spread next to the ratios; pass sizes and
rounds as argv: sparse_ab.py 4096,8192 40
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
    ac = torch.randn(n, n // 2, device="cuda", generator=g).bfloat16()
    bt = torch.randn(n, n, device="cuda", generator=g).bfloat16()
    nib = torch.tensor(attest.SP24_NIBBLES, device="cuda")[
        torch.randint(0, 6, (n, n // 4), device="cuda", generator=g)]
    am = (nib[:, 0::2] | nib[:, 1::2] << 4).to(torch.uint8)
    a = attest.sp24_dense(ac, am)
    names = {"sp_32x32x32": 0, "sp_16x16x64": 1}
    c = {k: torch.empty(n, n, device="cuda") for k in [*names, "dense"]}

    def sp(name):
        return lambda: attest.mfma_gemm_sp24(
            0, ac.data_ptr(), am.data_ptr(), bt.data_ptr(), c[name].data_ptr(),
            n, n, n, names[name])

    arms = {name: sp(name) for name in names}
    arms["dense"] = lambda: attest.mfma_gemm_bf16(
        0, a.data_ptr(), bt.data_ptr(), c["dense"].data_ptr(), n, n, n)
    for _ in range(3):  # warm all
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    bound = (n // 2) * 2.0**-23 * (a.float().abs() @ bt.float().abs().t())
    ratio = {k: float(((c[k] - c["dense"]).abs() / bound).max()) for k in names}
    del bound
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    tf = {k: 2.0 * n**3 / (v * 1e-3) / 1e12 for k, v in med.items()}
    out = {"kind": "sparse_ab", "n": n, "rounds": rounds}
    for k in arms:
        q = statistics.quantiles(ms[k], n=10)
        out[f"{k}_ms_med"] = round(med[k], 4)
        out[f"{k}_ms_p10_p90"] = [round(q[0], 4), round(q[-1], 4)]
        out[f"{k}_tflops_med"] = round(tf[k], 1)
    for k in names:
        out[f"{k}_diff_over_bound"] = round(ratio[k], 4)
        out[f"{k}_over_dense"] = round(tf[k] / tf["dense"], 3)
    # the dense arm against itself: the middle 80 % of its rounds over its median
    q = statistics.quantiles(ms["dense"], n=10)
    out["dense_spread_p10_p90"] = [round(med["dense"] / q[-1], 3),
                                   round(med["dense"] / q[0], 3)]
    return out


def main():
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4096, 8192]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    for n in sizes:
        print(json.dumps(bench(n, rounds)), flush=True)


if __name__ == "__main__":
    main()
