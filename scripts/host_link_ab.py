#!/usr/bin/env python3
"""Host-link shader passes vs the runtime's copy of the same bytes.

Builds scripts/host_link_ab.hip (a stand-alone program around the
kernels of ops/host_link.hip) next to itself when it is missing or older
than its sources, and runs it: ONE process, 64 MiB by default, 40 rounds
that interleave link_pull, link_push, link_duplex and hipMemcpyAsync in
each direction, for every grid / vectors-in-flight setting given. Time
is device events around each launch or copy; the program prints one JSON
line per setting with medians and ranges, and verifies every setting's
results. The baseline is the copy path in the same process and the same
rounds, never the kernel itself. A pull rate above the link's spec rate
(63 GB/s for Gen5 x16) would mean a cache served it.

    host_link_ab.py [MIB] [ROUNDS] [BLOCKS:U ...]

Without settings it sweeps blocks in {64, 128, 256, 512, 1024} x U in
{1, 2, 4, 8}.
"""

import os
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
OPS = HERE.parent / "k8s_cc_manager_amd" / "ops"
SRC = HERE / "host_link_ab.hip"
EXE = HERE / "host_link_ab"
DEPS = [SRC] + [OPS / n for n in ("host_link.hip", "host_pattern.hip",
                                  "hbm_march.hip", "probe_kernels.hip",
                                  "gemm_common.hip")]


def build() -> Path:
    newest = max(p.stat().st_mtime for p in DEPS)
    if EXE.exists() and EXE.stat().st_mtime >= newest:
        return EXE
    cmd = [os.environ.get("HIPCC", "hipcc"),
           f"--offload-arch={os.environ.get('CC_GPU_ARCH', 'gfx950')}",
           "-O3", "-std=c++17", "-Wno-unused-value", str(SRC), "-o", str(EXE)]
    subprocess.run(cmd, check=True)
    return EXE


def main() -> int:
    args = sys.argv[1:]
    if args and args[0] == "--build-only":
        print(build())
        return 0
    mib = args[0] if args else "64"
    rounds = args[1] if len(args) > 1 else "40"
    settings = args[2:] or [f"{b}:{u}" for u in (1, 2, 4, 8)
                            for b in (64, 128, 256, 512, 1024)]
    return subprocess.run([str(build()), mib, rounds] + settings).returncode


if __name__ == "__main__":
    sys.exit(main())
