"""Node diagnostics: ``python -m k8s_cc_manager_amd.doctor``.

One JSON document answering the first questions an operator asks on a
misbehaving CC node: can the host do TEE at all, is KFD alive, what do
PCI and amdsmi each see, does the attestation library load, and (with
``--attest``) does a full probe pass (``--cu-sweep`` adds the
compute-unit sweep, per XCC; ``--hbm-march MIB`` a verified march and
zeroing scrub of that much VRAM; ``--host-link MIB`` five verified
passes of that much across PCIe). Every section degrades gracefully
— a CPU-only box reports absence, not a stack trace.
"""

from __future__ import annotations

import argparse
import json
import sys
from typing import Any, Dict

from .core.hostprobe import is_host_cc_enabled


def _cu_sweep_section(attest, device_index: int) -> Dict[str, Any]:
    """The compute-unit sweep of one GPU, with one line per XCC: CUs the
    sweep reached there and CUs with a failing SIMD."""
    rep = attest.cu_sweep_report(device_index)
    seen: Dict[int, set] = {}
    for key in attest.cu_sweep_units(device_index):
        seen.setdefault(key >> 10, set()).add(key >> 2)
    failed: Dict[int, set] = {}
    for unit in rep.failed_units:
        failed.setdefault(unit[0], set()).add(unit[:4])
    return {
        "device": device_index,
        "ok": rep.ok,
        "units": f"{rep.units_seen}/{rep.units_expected}",
        "launches": rep.launches,
        "sweep_ms": rep.sweep_ms,
        "error": rep.error,
        "failed_units": [attest.unit_name(u) for u in rep.failed_units],
        "per_xcc": [
            f"xcc{x}: {len(cus)} CUs seen, {len(failed.get(x, ()))} failed"
            for x, cus in sorted(seen.items())
        ],
    }


def _hbm_march_section(attest, device_index: int, mib: int) -> Dict[str, Any]:
    """The HBM march of one GPU over ``mib`` MiB of its VRAM."""
    rep = attest.hbm_march_report(device_index, mib)
    first = rep.first_bad_offset
    return {
        "device": device_index,
        "ok": rep.ok,
        "mib_tested": rep.bytes_tested >> 20,
        "gbps": round(rep.gbps, 1),
        "mismatch_words": rep.mismatch_words,
        "first_bad_offset": None if first is None else hex(first),
        "scrubbed": rep.scrubbed,
        "error": rep.error,
    }


def _host_link_section(attest, device_index: int, mib: int) -> Dict[str, Any]:
    """The host-link leg of one GPU over ``mib`` MiB of pinned memory."""
    rep = attest.host_link_report(device_index, mib)
    first = rep.first_bad_offset
    return {
        "device": device_index,
        "ok": rep.ok,
        "mib_tested": rep.bytes_tested >> 20,
        "passes": rep.passes,
        "gbps": {
            "pull": round(rep.pull_gbps, 1),
            "push": round(rep.push_gbps, 1),
            "h2d": round(rep.h2d_gbps, 1),
            "d2h": round(rep.d2h_gbps, 1),
            "duplex": [round(rep.duplex_pull_gbps, 1),
                       round(rep.duplex_push_gbps, 1)],
        },
        "host_ms": round(rep.host_ms, 3),
        "mismatch_words": rep.mismatch_words,
        "first_bad_offset": None if first is None else hex(first),
        "bad_pass": rep.bad[0][3] if rep.bad else None,
        "error": rep.error,
    }


def collect(run_attest: bool = False, gemm_dim: int = 512,
            cu_sweep: bool = False, hbm_march_mib: int = 0,
            host_link_mib: int = 0) -> Dict[str, Any]:
    report: Dict[str, Any] = {"schema": "cc-doctor/v1"}

    # host TEE capability
    report["host_cc_enabled"] = is_host_cc_enabled()

    # native library + KFD + PCI
    native_info: Dict[str, Any] = {"available": False}
    try:
        from .device import native

        native_info["available"] = native.available()
        if native_info["available"]:
            ver = native.kfd_version()
            native_info["kfd_version"] = list(ver) if ver else None
            topo = [e for e in native.kfd_topology() if e.get("is_gpu")]
            native_info["kfd_gpu_nodes"] = [
                {
                    "node": e.get("node"),
                    "gfx_target_version": e.get("gfx_target_version"),
                    "cu_count": e.get("cu_count"),
                    "io_links_count": e.get("io_links_count"),
                }
                for e in topo
            ]
            native_info["pci_amd_gpus"] = native.pci_scan()
    except Exception as e:
        native_info["error"] = str(e)
    report["native"] = native_info

    # amdsmi enumeration
    smi: Dict[str, Any] = {"available": False}
    try:
        from .device.amdsmi_backend import AmdSmiBackend

        be = AmdSmiBackend()
        devices, count = be.find_devices()
        smi["available"] = True
        smi["devices"] = []
        for d in devices:
            entry = {
                "bdf": d.bdf,
                "name": d.name,
                "cc_mode": d.query_cc_mode(),
                "fabric_mode": d.query_fabric_mode(),
            }
            # best-effort telemetry (fields vary by stack version)
            try:
                import amdsmi

                vram = amdsmi.amdsmi_get_gpu_vram_info(d._handle)
                if isinstance(vram, dict):
                    raw = int(vram.get("vram_total", 0))
                    # stacks disagree on units: treat small values as MB
                    entry["vram_total_mb"] = raw if raw < (1 << 24) else raw >> 20
            except Exception:
                pass
            try:
                import amdsmi

                entry["power_w"] = amdsmi.amdsmi_get_power_info(d._handle).get(
                    "average_socket_power"
                )
            except Exception:
                pass
            smi["devices"].append(entry)
        smi["count"] = count
    except Exception as e:
        smi["error"] = str(e)
    report["amdsmi"] = smi

    # attestation library
    att: Dict[str, Any] = {"library_loaded": False}
    try:
        from .ops import attest

        count = attest.device_count()  # raises when the library is missing
        att["library_loaded"] = True
        att["hip_device_count"] = count
        if run_attest and att["hip_device_count"] > 0:
            import dataclasses

            reports = []
            for i in range(att["hip_device_count"]):
                rep = attest.attest_device(i, gemm_dim=gemm_dim)
                reports.append(dataclasses.asdict(rep))
            att["probes"] = reports
            if cu_sweep:
                att["cu_sweep"] = [
                    _cu_sweep_section(attest, i)
                    for i in range(att["hip_device_count"])
                ]
            if hbm_march_mib > 0:
                att["hbm_march"] = [
                    _hbm_march_section(attest, i, hbm_march_mib)
                    for i in range(att["hip_device_count"])
                ]
            if host_link_mib > 0:
                att["host_link"] = [
                    _host_link_section(attest, i, host_link_mib)
                    for i in range(att["hip_device_count"])
                ]
    except Exception as e:
        att["error"] = str(e)
    report["attestation"] = att

    # reset-path boundary: would the FLR ladder work HERE? (read-only —
    # same evidence scripts/reset_probe.py collects; the pool that
    # motivated this mounts /sys read-only, profiles/reset_exercise_r02)
    reset: Dict[str, Any] = {}
    try:
        import os

        devs = smi.get("devices") or []
        probes = []
        for d in devs[:8]:
            node = f"/sys/bus/pci/devices/{d['bdf']}/reset"
            entry = {"bdf": d["bdf"], "reset_node": os.path.exists(node)}
            if entry["reset_node"]:
                entry["sys_writable"] = os.access(node, os.W_OK)
            probes.append(entry)
        reset["devices"] = probes
        reset["sys_readonly_mount"] = False
        try:
            with open("/proc/mounts") as f:
                for line in f:
                    parts = line.split()
                    if len(parts) >= 4 and parts[1] == "/sys":
                        reset["sys_readonly_mount"] = "ro" in parts[3].split(",")
        except OSError:
            pass
    except Exception as e:  # pragma: no cover - defensive
        reset["error"] = str(e)
    report["reset_path"] = reset

    # verdict
    ok_gpu = att.get("hip_device_count", 0) > 0 and att.get("library_loaded")
    reset_blocked = reset.get("sys_readonly_mount") is True
    report["verdict"] = {
        "cc_capable": bool(report["host_cc_enabled"] and ok_gpu),
        "notes": []
        + ([] if report["host_cc_enabled"] else ["host TEE (SEV-SNP/TDX) disabled"])
        + ([] if ok_gpu else ["no attestable GPU (library or device missing)"])
        + (
            ["/sys mounted read-only: the FLR tier of the reset ladder "
             "will fail EROFS (container must mount sysfs rw)"]
            if reset_blocked
            else []
        ),
    }
    return report


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="cc-doctor", description=__doc__)
    ap.add_argument("--attest", action="store_true",
                    help="run the full attestation probe on every GPU")
    ap.add_argument("--gemm-dim", type=int, default=512)
    ap.add_argument("--cu-sweep", action="store_true",
                    help="with --attest: also run the compute-unit sweep "
                    "(every SIMD of every CU) and list CUs seen and failed "
                    "per XCC")
    ap.add_argument("--hbm-march", type=int, default=0, metavar="MIB",
                    help="with --attest: also march MIB MiB of every GPU's "
                    "VRAM (verified fill, flip, scrub to zero, zero check) "
                    "and list MiB tested, GB/s, mismatches, first bad "
                    "offset and whether the window was left scrubbed")
    ap.add_argument("--host-link", type=int, default=0, metavar="MIB",
                    help="with --attest: also move MIB MiB (1..1024) across "
                    "every GPU's PCIe link in five verified passes (shader "
                    "pull and push, copy-path h2d and d2h, duplex) and list "
                    "GB/s per pass, mismatches and the first bad offset")
    ap.add_argument(
        "--verify-attest-log",
        metavar="PATH",
        help="verify the hash chain of a CC_ATTEST_LOG file and exit "
        "(tamper-evident audit of past readiness decisions)",
    )
    args = ap.parse_args(argv)

    if args.verify_attest_log:
        from .ops import attest

        try:
            n = attest.verify_attest_log(args.verify_attest_log)
        except attest.AttestationError as e:
            print(json.dumps({"verified": False, "error": str(e)}))
            return 1
        print(json.dumps({"verified": True, "records": n}))
        return 0
    report = collect(run_attest=args.attest, gemm_dim=args.gemm_dim,
                     cu_sweep=args.cu_sweep, hbm_march_mib=args.hbm_march,
                     host_link_mib=args.host_link)
    print(json.dumps(report, indent=2))
    return 0 if report["verdict"]["cc_capable"] or not args.attest else 1


if __name__ == "__main__":
    sys.exit(main())
