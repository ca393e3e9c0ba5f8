#!/usr/bin/env python3
"""HBM march step vs a plain copy of the same bytes.

march_step<check, write> (N bytes read and compared, N bytes written)
against torch's dst.copy_(src) of N bytes (N read, N written),
INTERLEAVED in one process (step, copy, fill, check within every round)
so clock drift hits all alike. Device-event time per launch: the
library's own events around the step's launches (HbmMarchReport), torch
events around the copy; medians over the rounds. Round r checks phase
r % 2 and writes the other one, so every step verifies what the
previous step wrote and must come back clean. Fill-only and check-only
rates come from the same rounds. Prints one JSON line per size; pass
sizes in MiB and rounds as argv: hbm_march_ab.py 2048,64 40
"""

import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from k8s_cc_manager_amd.ops import attest


def timed(fn) -> float:
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def bench(mib: int, rounds: int) -> dict:
    nbytes = mib << 20
    buf = torch.empty(nbytes // 4, device="cuda", dtype=torch.int32)
    scratch = torch.empty(nbytes // 4, device="cuda", dtype=torch.int32)
    src = torch.zeros(nbytes // 4, device="cuda", dtype=torch.int32)
    dst = torch.empty(nbytes // 4, device="cuda", dtype=torch.int32)

    def step(ptr, check=-1, write=-1):
        rep = attest.hbm_step(0, ptr, nbytes, 0, check, write)
        assert rep.ok, rep
        return rep

    step(buf.data_ptr(), write=0)
    for r in range(3):  # warm all four
        step(buf.data_ptr(), check=r % 2, write=1 - r % 2)
        dst.copy_(src)
        step(scratch.data_ptr(), write=0)
        step(scratch.data_ptr(), check=0)
    torch.cuda.synchronize()
    first = 3 % 2  # the phase buf holds now
    ms = {"step": [], "copy": [], "fill": [], "check": []}
    for r in range(rounds):
        held = (first + r) % 2
        ms["step"].append(step(buf.data_ptr(), check=held, write=1 - held).flip_ms)
        ms["copy"].append(timed(lambda: dst.copy_(src)))
        ms["fill"].append(step(scratch.data_ptr(), write=0).fill_ms)
        ms["check"].append(step(scratch.data_ptr(), check=0).zero_ms)
    med = {k: statistics.median(v) for k, v in ms.items()}
    moved = {"step": 2, "copy": 2, "fill": 1, "check": 1}
    out = {"kind": "hbm_march_ab", "mib": mib, "rounds": rounds}
    for k in ms:
        out[f"{k}_ms_med"] = round(med[k], 4)
        out[f"{k}_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out[f"{k}_gbps_med"] = round(moved[k] * nbytes / (med[k] * 1e-3) / 1e9)
    out["step_over_copy_time"] = round(med["step"] / med["copy"], 3)
    return out


def main():
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2048, 64]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    for mib in sizes:
        print(json.dumps(bench(mib, rounds)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
