"""Python surface of the CDNA4 attestation probe.

Loads the in-tree ``libccattest.so`` via ctypes (the control-plane
daemon must not depend on torch). On a GPU box the library is REQUIRED:
if AMD GPUs are visible but the library is missing or fails to load,
attestation raises instead of silently passing — a reset GPU may never
be labeled ready on the strength of a Python fallback.
"""

from __future__ import annotations

import ctypes
import logging
import os
import re
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Optional

logger = logging.getLogger(__name__)

_LIB_PATH = Path(__file__).resolve().parent / "libccattest.so"
_lib: Optional[ctypes.CDLL] = None


class AttestationError(Exception):
    """The post-reset attestation probe failed — the device must NOT be
    labeled ready."""


def _from_c(cls, c, **special):
    """Build report dataclass ``cls`` from its C mirror: every same-named
    field is copied, ``error`` decoded and ``ok`` made a bool; ``special``
    holds the fields whose Python form differs."""
    special.update(error=c.error.decode(errors="replace"), ok=bool(c.ok))
    return cls(**{f.name: special[f.name] if f.name in special
                  else getattr(c, f.name) for f in fields(cls)})


class _CReport(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("cu_count", ctypes.c_int),
        ("xcc_count", ctypes.c_int),
        ("arch", ctypes.c_char * 64),
        ("error", ctypes.c_char * 256),
        ("vram_total_mb", ctypes.c_longlong),
        ("gemm_m", ctypes.c_int),
        ("gemm_n", ctypes.c_int),
        ("gemm_k", ctypes.c_int),
        ("gemm_ms", ctypes.c_double),
        ("gemm_tflops", ctypes.c_double),
        ("ref_ms", ctypes.c_double),
        ("max_abs_err", ctypes.c_float),
        ("checksum", ctypes.c_ulonglong),
        ("fp8_ms", ctypes.c_double),
        ("fp8_tflops", ctypes.c_double),
        ("fp8_max_abs_err", ctypes.c_float),
        ("lds_ms", ctypes.c_double),
        ("lds_failures", ctypes.c_uint),
        ("hbm_ms", ctypes.c_double),
        ("hbm_gbps", ctypes.c_double),
        ("peer_count", ctypes.c_int),
        ("peers_accessible", ctypes.c_int),
        ("peers_attempted", ctypes.c_int),
        ("peers_verified", ctypes.c_int),
        ("xgmi_ms", ctypes.c_double),
        ("xgmi_gbps_min", ctypes.c_double),
        ("xgmi_gbps_max", ctypes.c_double),
        ("ok", ctypes.c_int),
    ]


@dataclass
class AttestReport:
    device: int
    cu_count: int
    arch: str
    vram_total_mb: int
    gemm_dim: int
    gemm_ms: float
    gemm_tflops: float
    ref_ms: float
    max_abs_err: float
    checksum: int
    fp8_ms: float
    fp8_tflops: float
    fp8_max_abs_err: float
    lds_ms: float
    lds_failures: int
    hbm_ms: float
    hbm_gbps: float
    peer_count: int
    peers_accessible: int
    peers_attempted: int
    peers_verified: int
    xgmi_ms: float
    xgmi_gbps_min: float
    xgmi_gbps_max: float
    ok: bool
    error: str = ""

    @classmethod
    def from_c(cls, c: _CReport) -> "AttestReport":
        return _from_c(cls, c, arch=c.arch.decode(errors="replace"),
                       gemm_dim=c.gemm_m)


class _CMxReport(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("mx_m", ctypes.c_int),
        ("mx_n", ctypes.c_int),
        ("mx_k", ctypes.c_int),
        ("mx_ms", ctypes.c_double),
        ("mx_tflops", ctypes.c_double),
        ("mx_ref_ms", ctypes.c_double),
        ("mx_max_abs_err", ctypes.c_float),
        ("mx_checksum", ctypes.c_ulonglong),
        ("ok", ctypes.c_int),
        ("error", ctypes.c_char * 256),
    ]


@dataclass
class MxReport:
    """Result of the opt-in MXFP4 probe (``attest_mxfp4``)."""

    device: int
    mx_dim: int
    mx_ms: float
    mx_tflops: float
    mx_ref_ms: float
    mx_max_abs_err: float
    mx_checksum: int
    ok: bool
    error: str = ""

    @classmethod
    def from_c(cls, c: _CMxReport) -> "MxReport":
        return _from_c(cls, c, mx_dim=c.mx_m)


class _CSweepReport(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("cu_count", ctypes.c_int),
        ("units_expected", ctypes.c_int),
        ("units_seen", ctypes.c_int),
        ("cus_seen", ctypes.c_int),
        ("xccs_seen", ctypes.c_int),
        ("units_failed", ctypes.c_int),
        ("mfma_failures", ctypes.c_uint),
        ("lds_failures", ctypes.c_uint),
        ("launches", ctypes.c_int),
        ("rounds", ctypes.c_int),
        ("sweep_ms", ctypes.c_double),
        ("gold_ms", ctypes.c_double),
        ("failed_keys", ctypes.c_uint * 16),
        ("ok", ctypes.c_int),
        ("error", ctypes.c_char * 256),
    ]


SWEEP_GOLD_ELEMS = 3328  # floats in the sweep's four golden C images


# Unit key of the compute-unit sweep (ops/cu_sweep.hip):
# XCC_ID[3:0] << 10 | HW_ID[15:8] << 2 | SIMD_ID, with HW_ID's CU_ID in
# bits 11:8, SH_ID in bit 12, SE_ID in bits 14:13.

def encode_unit(xcc: int, se: int, sh: int, cu: int, simd: int) -> int:
    """(xcc, se, sh, cu, simd) -> the sweep's 14-bit unit key."""
    for name, value, limit in (("xcc", xcc, 16), ("se", se, 4), ("sh", sh, 2),
                               ("cu", cu, 16), ("simd", simd, 4)):
        if not 0 <= value < limit:
            raise ValueError(f"{name}={value} outside 0..{limit - 1}")
    return (xcc << 10) | (se << 7) | (sh << 6) | (cu << 2) | simd


def decode_unit(key: int) -> tuple:
    """Unit key -> (xcc, se, sh, cu, simd). Bit 9 of the key (HW_ID bit
    15, above the documented SE_ID field) is not part of the tuple."""
    return (
        (key >> 10) & 15,
        (key >> 7) & 3,
        (key >> 6) & 1,
        (key >> 2) & 15,
        key & 3,
    )


@dataclass
class CuSweepReport:
    """Result of the opt-in compute-unit sweep (``sweep_compute_units``).
    A unit is one SIMD of one CU; ``failed_units`` holds the first 16
    that miscompared, decoded to (xcc, se, sh, cu, simd)."""

    device: int
    cu_count: int
    units_expected: int
    units_seen: int
    cus_seen: int
    xccs_seen: int
    units_failed: int
    mfma_failures: int
    lds_failures: int
    launches: int
    rounds: int
    sweep_ms: float
    gold_ms: float
    failed_units: list
    ok: bool
    error: str = ""

    @classmethod
    def from_c(cls, c: _CSweepReport) -> "CuSweepReport":
        n = max(0, min(c.units_failed, len(c.failed_keys)))
        return _from_c(
            cls, c, failed_units=[decode_unit(k) for k in c.failed_keys[:n]])


class _CHbmReport(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("chunks", ctypes.c_int),
        ("passes", ctypes.c_int),
        ("n_bad", ctypes.c_int),
        ("bytes_requested", ctypes.c_longlong),
        ("bytes_tested", ctypes.c_longlong),
        ("chunk_bytes", ctypes.c_longlong),
        ("origin", ctypes.c_ulonglong),
        ("mismatch_words", ctypes.c_ulonglong),
        ("first_bad_offset", ctypes.c_ulonglong),
        ("bad_offset", ctypes.c_ulonglong * 16),
        ("bad_expected", ctypes.c_uint * 16),
        ("bad_got", ctypes.c_uint * 16),
        ("bad_pass", ctypes.c_int * 16),
        ("fill_ms", ctypes.c_double),
        ("flip_ms", ctypes.c_double),
        ("scrub_ms", ctypes.c_double),
        ("zero_ms", ctypes.c_double),
        ("alloc_ms", ctypes.c_double),
        ("gbps", ctypes.c_double),
        ("beyond_cache", ctypes.c_int),
        ("scrubbed", ctypes.c_int),
        ("ok", ctypes.c_int),
        ("error", ctypes.c_char * 256),
    ]


# Pattern of the HBM march (ops/hbm_march.hip), keyed by the 64-bit
# logical word index w = (origin + byte offset in window) / 4.
HBM_MUL_LO, HBM_MUL_HI, HBM_SALT = 2654435769, 2246822519, 0x5EED0001
_HBM_NO_OFFSET = (1 << 64) - 1


def hbm_pattern_word(w: int, phase: int) -> int:
    """The 32-bit word the march expects at logical word index ``w``:
    phase 0 is ``lo*2654435769 + hi*2246822519 + 0x5EED0001`` mod 2^32
    with lo, hi the halves of ``w``; phase 1 its complement; phase 2
    zero."""
    if phase == 2:
        return 0
    if phase not in (0, 1):
        raise ValueError(f"phase={phase} outside 0..2")
    p = ((w & 0xFFFFFFFF) * HBM_MUL_LO + (w >> 32) * HBM_MUL_HI
         + HBM_SALT) & 0xFFFFFFFF
    return p ^ 0xFFFFFFFF if phase else p


@dataclass
class HbmMarchReport:
    """Result of the opt-in HBM march (``march_hbm``) or of one step on a
    caller's buffer (``hbm_step``). Offsets are bytes from the start of
    the window; ``bad`` holds the first 16 wrong words as (offset,
    expected, got, pass), ``first_bad_offset`` is None when clean."""

    device: int
    bytes_requested: int
    bytes_tested: int
    chunk_bytes: int
    origin: int
    chunks: int
    passes: int
    mismatch_words: int
    first_bad_offset: Optional[int]
    bad: list
    fill_ms: float
    flip_ms: float
    scrub_ms: float
    zero_ms: float
    alloc_ms: float
    gbps: float
    beyond_cache: bool
    scrubbed: bool
    ok: bool
    error: str = ""

    @classmethod
    def from_c(cls, c: _CHbmReport) -> "HbmMarchReport":
        n = max(0, min(c.n_bad, len(c.bad_offset)))
        first = c.first_bad_offset
        return _from_c(
            cls, c,
            first_bad_offset=None if first == _HBM_NO_OFFSET else first,
            bad=[(c.bad_offset[i], c.bad_expected[i], c.bad_got[i],
                  c.bad_pass[i]) for i in range(n)],
            beyond_cache=bool(c.beyond_cache), scrubbed=bool(c.scrubbed))


class _CHostReport(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("engine", ctypes.c_int),
        ("passes", ctypes.c_int),
        ("n_bad", ctypes.c_int),
        ("bytes_requested", ctypes.c_longlong),
        ("bytes_tested", ctypes.c_longlong),
        ("origin", ctypes.c_ulonglong),
        ("mismatch_words", ctypes.c_ulonglong),
        ("first_bad_offset", ctypes.c_ulonglong),
        ("bad_offset", ctypes.c_ulonglong * 16),
        ("bad_expected", ctypes.c_uint * 16),
        ("bad_got", ctypes.c_uint * 16),
        ("bad_pass", ctypes.c_int * 16),
        ("pull_ms", ctypes.c_double),
        ("push_ms", ctypes.c_double),
        ("h2d_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
        ("duplex_ms", ctypes.c_double),
        ("pull_gbps", ctypes.c_double),
        ("push_gbps", ctypes.c_double),
        ("h2d_gbps", ctypes.c_double),
        ("d2h_gbps", ctypes.c_double),
        ("duplex_pull_gbps", ctypes.c_double),
        ("duplex_push_gbps", ctypes.c_double),
        ("host_ms", ctypes.c_double),
        ("alloc_ms", ctypes.c_double),
        ("ok", ctypes.c_int),
        ("error", ctypes.c_char * 256),
    ]


# The host-link leg (ops/host_link.hip) moves the march's pattern across
# PCIe in five passes; pass k uses logical origin origin + k * 2^40.
HOST_LINK_PASSES = ("pull", "push", "h2d", "d2h", "duplex")
_HOST_LINK_PASS_STRIDE = 1 << 40


def host_link_word(offset: int, pass_no: int, origin: int = 0) -> int:
    """The 32-bit word pass ``pass_no`` (1..5) of the host-link leg
    expects at window byte offset ``offset``: the march's pattern at
    logical byte address ``origin + pass_no * 2^40 + offset``, phase 0 in
    passes 1, 3 and 5 and its complement in passes 2 and 4."""
    if not 1 <= pass_no <= len(HOST_LINK_PASSES):
        raise ValueError(f"pass_no={pass_no} outside 1..5")
    return hbm_pattern_word(
        (origin + pass_no * _HOST_LINK_PASS_STRIDE + offset) // 4,
        (pass_no + 1) & 1)


@dataclass
class HostLinkReport:
    """Result of the opt-in host-link leg (``attest_host_link``), of one
    direction on a caller's host buffer (``host_step``) or of the CPU
    fill / compare alone (``host_pattern``). Offsets are bytes from the
    start of the window; ``bad`` holds the first 16 wrong words as
    (offset, expected, got, pass), ``first_bad_offset`` is None when
    clean. ``*_ms`` are device events around the launch or copy alone,
    ``host_ms`` is the CPU's fill and compare time."""

    device: int
    engine: int
    bytes_requested: int
    bytes_tested: int
    origin: int
    passes: int
    mismatch_words: int
    first_bad_offset: Optional[int]
    bad: list
    pull_ms: float
    push_ms: float
    h2d_ms: float
    d2h_ms: float
    duplex_ms: float
    pull_gbps: float
    push_gbps: float
    h2d_gbps: float
    d2h_gbps: float
    duplex_pull_gbps: float
    duplex_push_gbps: float
    host_ms: float
    alloc_ms: float
    ok: bool
    error: str = ""

    @classmethod
    def from_c(cls, c: _CHostReport) -> "HostLinkReport":
        n = max(0, min(c.n_bad, len(c.bad_offset)))
        first = c.first_bad_offset
        return _from_c(
            cls, c,
            first_bad_offset=None if first == _HBM_NO_OFFSET else first,
            bad=[(c.bad_offset[i], c.bad_expected[i], c.bad_got[i],
                  c.bad_pass[i]) for i in range(n)])


_INT, _PTR = ctypes.c_int, ctypes.c_void_p
_I64, _U64 = ctypes.c_longlong, ctypes.c_ulonglong
_GEMM =[_INT, _PTR, _PTR, _PTR, _INT, _INT, _INT]  # device, A, Bt, C, M, N, K
_MX_GEMM = [_INT] + [_PTR] * 5 + [_INT] * 3  # device, A, SA, Bt, SB, C, M, N, K
_UNIT_TABLE = [_INT, ctypes.POINTER(ctypes.c_uint), _INT]

# Every exported function of the library: name -> (restype, argtypes).
_BINDINGS = {
    "cc_device_alive": (_INT, [_INT]),
    "cc_device_count": (_INT, []),
    "cc_device_index_for_bdf": (_INT, [_INT] * 3),
    "cc_mfma_gemm_bf16": (_INT, _GEMM),
    "cc_mfma_gemm_bf16_variant": (_INT, _GEMM + [_INT]),
    "cc_mfma_gemm_fp8_variant": (_INT, _GEMM + [_INT]),
    "cc_mfma_gemm_fp8": (_INT, _GEMM),
    "cc_ref_gemm_f32": (_INT, _GEMM),
    "cc_attest_device": (_INT, [_INT, _INT, ctypes.POINTER(_CReport)]),
    "cc_report_sizeof": (_INT, []),
    "cc_mfma_gemm_mxfp4": (_INT, _MX_GEMM),
    "cc_ref_gemm_mxfp4_f32": (_INT, _MX_GEMM),
    "cc_attest_mxfp4": (_INT, [_INT, _INT, ctypes.POINTER(_CMxReport)]),
    "cc_mx_report_sizeof": (_INT, []),
    "cc_cu_sweep": (_INT, [_INT, _INT, _INT, ctypes.POINTER(_CSweepReport)]),
    "cc_cu_sweep_gold": (_INT, [_INT, _INT, ctypes.POINTER(ctypes.c_float)]),
    "cc_cu_sweep_units": (_INT, _UNIT_TABLE),
    "cc_cu_sweep_hits": (_INT, _UNIT_TABLE),
    "cc_sweep_report_sizeof": (_INT, []),
    "cc_hbm_march": (_INT, [_INT, _I64, _INT, _U64, _I64, _INT,
                            ctypes.POINTER(_CHbmReport)]),
    "cc_hbm_step": (_INT, [_INT, _PTR, _I64, _U64, _INT, _INT,
                           ctypes.POINTER(_CHbmReport)]),
    "cc_hbm_report_sizeof": (_INT, []),
    "cc_host_link": (_INT, [_INT, _I64, _U64, _I64, _INT,
                            ctypes.POINTER(_CHostReport)]),
    "cc_host_step": (_INT, [_INT, _PTR, _I64, _U64, _INT, _INT, _INT,
                            ctypes.POINTER(_CHostReport)]),
    "cc_host_pattern": (_INT, [_PTR, _I64, _U64, _INT, _INT,
                               ctypes.POINTER(_CHostReport)]),
    "cc_host_report_sizeof": (_INT, []),
    "cc_attest_shutdown": (None, []),
}


def _load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise AttestationError(
            f"attestation library missing: {_LIB_PATH} — run "
            "python -m k8s_cc_manager_amd.ops.build"
        )
    lib = ctypes.CDLL(str(_LIB_PATH))
    for name, (restype, argtypes) in _BINDINGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def probe_available() -> bool:
    """True when the library loads AND at least one GPU is visible."""
    try:
        return _load().cc_device_count() > 0
    except Exception:
        return False


def device_count() -> int:
    return _load().cc_device_count()


def device_alive(device_index: int) -> int:
    """Round-trip one kernel launch on the device: 0 when it answered,
    else the library's negative status."""
    return _load().cc_device_alive(device_index)


def shutdown() -> None:
    """Free everything the library caches on every device (buffers,
    references, the last sweep's unit table)."""
    _load().cc_attest_shutdown()


def attest_device(device_index: int, gemm_dim: int = 1024) -> AttestReport:
    """Run the full MFMA+LDS+HBM+xGMI probe on one GPU; raise on failure."""
    lib = _load()
    c = _CReport()
    rc = lib.cc_attest_device(device_index, gemm_dim, ctypes.byref(c))
    rep = AttestReport.from_c(c)
    if rc != 0:
        raise AttestationError(
            f"device {device_index}: probe runtime error rc={rc}: {rep.error}"
        )
    if not rep.ok:
        raise AttestationError(
            f"device {device_index}: attestation FAILED "
            f"(max_abs_err={rep.max_abs_err}, fp8_max_abs_err={rep.fp8_max_abs_err}, "
            f"lds_failures={rep.lds_failures}, "
            f"xgmi {rep.peers_verified}/{rep.peers_attempted} attempted links verified)"
        )
    logger.info(
        "attested device %d: %s %d CUs, bf16 GEMM %.1f TF/s, fp8 GEMM "
        "%.1f TF/s (%dx%dx%d), LDS ok, HBM %.0f GB/s, xGMI %d/%d peers "
        "(%d verified, %.0f-%.0f GB/s/link)",
        rep.device,
        rep.arch,
        rep.cu_count,
        rep.gemm_tflops,
        rep.fp8_tflops,
        rep.gemm_dim,
        rep.gemm_dim,
        rep.gemm_dim,
        rep.hbm_gbps,
        rep.peers_accessible,
        rep.peer_count,
        rep.peers_verified,
        rep.xgmi_gbps_min,
        rep.xgmi_gbps_max,
    )
    _append_attest_log(rep)
    return rep


def attest_mxfp4(device_index: int, gemm_dim: int = 1024) -> MxReport:
    """Run the MXFP4 probe on one GPU: the fp4 MFMA GEMM with real E8M0
    block scales against the VALU reference, bitwise. Raises on failure.
    gemm_dim below 256 rounds up to 256, otherwise down to a multiple."""
    lib = _load()
    c = _CMxReport()
    rc = lib.cc_attest_mxfp4(device_index, gemm_dim, ctypes.byref(c))
    rep = MxReport.from_c(c)
    if rc != 0:
        raise AttestationError(
            f"device {device_index}: mxfp4 probe runtime error rc={rc}: {rep.error}"
        )
    if not rep.ok:
        raise AttestationError(
            f"device {device_index}: mxfp4 attestation FAILED "
            f"(mx_max_abs_err={rep.mx_max_abs_err}, mx_tflops={rep.mx_tflops})"
        )
    logger.info(
        "attested device %d: mxfp4 GEMM %.1f TF/s (%dx%dx%d), bitwise ok",
        rep.device,
        rep.mx_tflops,
        rep.mx_dim,
        rep.mx_dim,
        rep.mx_dim,
    )
    return rep


CU_SWEEP_MAX_ROUNDS = 256  # exactness cap of the sweep's MFMA chains


def unit_name(unit: tuple) -> str:
    return "xcc%d/se%d/sh%d/cu%d/simd%d" % unit


def cu_sweep_report(device_index: int, rounds: int = 32,
                    _poison_key: int = -1) -> CuSweepReport:
    """Run the compute-unit sweep and return its report whatever it
    found; raises only when the sweep itself could not run (rc != 0,
    e.g. rc=-2 for ``rounds`` outside 1..CU_SWEEP_MAX_ROUNDS)."""
    lib = _load()
    c = _CSweepReport()
    rc = lib.cc_cu_sweep(device_index, rounds, _poison_key, ctypes.byref(c))
    rep = CuSweepReport.from_c(c)
    if rc != 0:
        raise AttestationError(
            f"device {device_index}: cu sweep runtime error: {rep.error} rc={rc}"
        )
    return rep


def sweep_compute_units(device_index: int, rounds: int = 32,
                        _poison_key: int = -1) -> CuSweepReport:
    """Run the matrix-core and whole-LDS self-test on every SIMD of every
    CU of one GPU: four MFMA chains of ``rounds`` accumulating
    instructions per wave (bf16 32x32x16 and 16x16x32, block-scaled e4m3
    and e2m1 32x32x64) compared bitwise with a VALU reference, an LDS
    march over all 160 KiB, and the unit each wave ran on read from the
    hardware ID registers. Raises when a unit miscompares or when a unit
    was never reached. ``_poison_key`` makes the waves of that unit
    produce one wrong number (for testing the detector)."""
    rep = cu_sweep_report(device_index, rounds, _poison_key)
    if not rep.ok:
        if rep.units_failed or rep.lds_failures:
            units = ", ".join(unit_name(u) for u in rep.failed_units)
            more = rep.units_failed - len(rep.failed_units)
            raise AttestationError(
                f"device {device_index}: cu sweep FAILED on {rep.units_failed} "
                f"unit(s): {units}{f' and {more} more' if more > 0 else ''} "
                f"(mfma_failures={rep.mfma_failures}, "
                f"lds_failures={rep.lds_failures})"
            )
        raise AttestationError(
            f"device {device_index}: cu sweep FAILED: {rep.error} "
            f"({rep.cus_seen}/{rep.cu_count} CUs)"
        )
    logger.info(
        "attested device %d: cu sweep %d/%d units on %d CUs of %d XCCs, "
        "%d launch(es), %.2f ms",
        rep.device,
        rep.units_seen,
        rep.units_expected,
        rep.cus_seen,
        rep.xccs_seen,
        rep.launches,
        rep.sweep_ms,
    )
    return rep


def cu_sweep_gold(device_index: int, rounds: int) -> list:
    """The sweep's golden C images for ``rounds`` from the VALU reference
    kernel: 3328 floats, row-major 32x32 (bf16 32x32x16), 16x16 (bf16
    16x16x32), 32x32 (e4m3) and 32x32 (e2m1)."""
    buf = (ctypes.c_float * SWEEP_GOLD_ELEMS)()
    rc = _load().cc_cu_sweep_gold(device_index, rounds, buf)
    if rc != 0:
        raise AttestationError(f"cu_sweep_gold rc={rc}")
    return list(buf)


def _cu_sweep_table(fn_name: str, device_index: int) -> list:
    fn = getattr(_load(), fn_name)
    n = fn(device_index, None, 0)
    if n < 0:
        raise AttestationError(f"{fn_name} rc={n}")
    buf = (ctypes.c_uint * max(n, 1))()
    n = min(n, fn(device_index, buf, n))
    return [int(buf[i]) for i in range(n)]


def cu_sweep_units(device_index: int) -> list:
    """Keys of the units the last sweep on this device reached,
    ascending (``decode_unit`` names them)."""
    return _cu_sweep_table("cc_cu_sweep_units", device_index)


def cu_sweep_hits(device_index: int) -> dict:
    """Unit key -> number of waves that reported from it in the last
    sweep on this device."""
    return dict(zip(cu_sweep_units(device_index),
                    _cu_sweep_table("cc_cu_sweep_hits", device_index)))


def hbm_step(device_index: int, ptr: int, nbytes: int, origin: int = 0,
             check: int = -1, write: int = -1) -> HbmMarchReport:
    """One march step on a caller-owned device buffer (a torch tensor via
    .data_ptr()): every 16-byte vector is compared with phase ``check``
    and then overwritten with phase ``write`` (0 pattern, 1 complement,
    2 zero, -1 none; not both none). ``origin`` is the logical byte
    address of the buffer's first byte, a multiple of 16. ``nbytes`` a
    positive multiple of 16, ``ptr`` 16-aligned; anything else raises
    with rc=-2. Mismatches are reported, not raised."""
    c = _CHbmReport()
    rc = _load().cc_hbm_step(device_index, ptr, nbytes, origin, check, write,
                             ctypes.byref(c))
    rep = HbmMarchReport.from_c(c)
    if rc != 0:
        raise AttestationError(
            f"device {device_index}: hbm step runtime error: {rep.error} rc={rc}"
        )
    return rep


def hbm_march_report(device_index: int, mib: int, chunk_mib: int = 1024,
                     _origin: int = 0, _poison_offset: int = -1,
                     _poison_after: int = 0) -> HbmMarchReport:
    """Run the HBM march and return its report whatever it found; raises
    only when the march itself could not run (rc != 0, e.g. rc=-2 for
    ``mib`` < 1 or ``chunk_mib`` outside 1..1024). A window that could
    not be allocated is a report with ``ok`` false, ``bytes_tested`` 0
    and the amounts in ``error``."""
    c = _CHbmReport()
    rc = _load().cc_hbm_march(device_index, mib, chunk_mib, _origin,
                              _poison_offset, _poison_after, ctypes.byref(c))
    rep = HbmMarchReport.from_c(c)
    if rc != 0:
        raise AttestationError(
            f"device {device_index}: hbm march runtime error: {rep.error} rc={rc}"
        )
    return rep


def march_hbm(device_index: int, mib: int, chunk_mib: int = 1024,
              _origin: int = 0, _poison_offset: int = -1,
              _poison_after: int = 0) -> HbmMarchReport:
    """March ``mib`` MiB of one GPU's VRAM, held as chunks of
    ``chunk_mib``: fill with an address-keyed pattern, verify it while
    writing its complement, verify that while writing zeros, verify the
    zeros. The window is real VRAM taken for the duration of the call
    and is left zeroed. Raises when a word was wrong or when the window
    could not be allocated. ``_poison_offset`` / ``_poison_after`` flip
    one bit between two passes (for testing the detector)."""
    rep = hbm_march_report(device_index, mib, chunk_mib, _origin,
                           _poison_offset, _poison_after)
    if not rep.ok:
        if rep.mismatch_words:
            where = f"first at offset {rep.first_bad_offset:#x}"
            if rep.bad:
                _, expected, got, bad_pass = rep.bad[0]
                where += (f" in pass {bad_pass}, expected^got="
                          f"{expected ^ got:#010x}")
            raise AttestationError(
                f"device {device_index}: hbm march FAILED: "
                f"{rep.mismatch_words} wrong word(s), {where}"
            )
        raise AttestationError(
            f"device {device_index}: hbm march FAILED: {rep.error} "
            f"({rep.passes}/4 passes)"
        )
    logger.info(
        "attested device %d: hbm march %d MiB in %d chunk(s), %.0f GB/s, "
        "scrubbed",
        rep.device,
        rep.bytes_tested >> 20,
        rep.chunks,
        rep.gbps,
    )
    return rep


def host_pattern(ptr: int, nbytes: int, origin: int = 0, check: int = -1,
                 write: int = -1) -> HostLinkReport:
    """The CPU side of the host-link leg on its own, on host memory
    (a numpy array via .ctypes.data): fill ``nbytes`` at ``ptr`` with
    phase ``write`` of the pattern, or compare them with phase ``check``
    (0 pattern, 1 complement, 2 zero; exactly one of the two, the other
    -1). Makes no GPU call. ``ptr`` 16-aligned, ``nbytes`` a positive
    multiple of 16 of at most 1 GiB; anything else raises with rc=-2.
    Mismatches are reported, not raised."""
    c = _CHostReport()
    rc = _load().cc_host_pattern(ptr, nbytes, origin, check, write,
                                 ctypes.byref(c))
    rep = HostLinkReport.from_c(c)
    if rc != 0:
        raise AttestationError(
            f"host pattern runtime error: {rep.error} rc={rc}")
    return rep


def host_step(device_index: int, ptr: int, nbytes: int, origin: int = 0,
              check: int = -1, write: int = -1,
              engine: int = 0) -> HostLinkReport:
    """One direction of the host link on caller-owned host memory (a
    numpy array via .ctypes.data). ``check`` (phase 0..2) sends the
    buffer host -> device and compares it there; ``write`` generates the
    pattern on the device and lands it in the buffer; exactly one of the
    two, the other -1. ``engine`` 0 is the shader on the mapped range
    (link_pull / link_push), 1 the runtime's copy path with a device
    staging buffer. The range is page-locked for the call unless it
    already is. ``ptr`` 16-aligned, ``nbytes`` a positive multiple of 16
    of at most 1 GiB; anything else raises with rc=-2. Mismatches are
    reported, not raised."""
    c = _CHostReport()
    rc = _load().cc_host_step(device_index, ptr, nbytes, origin, check, write,
                              engine, ctypes.byref(c))
    rep = HostLinkReport.from_c(c)
    if rc != 0:
        raise AttestationError(
            f"device {device_index}: host step runtime error: {rep.error} rc={rc}"
        )
    return rep


def host_link_report(device_index: int, mib: int, _origin: int = 0,
                     _poison_offset: int = -1,
                     _poison_pass: int = 0) -> HostLinkReport:
    """Run the host-link leg and return its report whatever it found;
    raises only when the leg itself could not run (rc != 0, e.g. rc=-2
    for ``mib`` outside 1..1024). Buffers that could not be allocated
    are a report with ``ok`` false, ``bytes_tested`` 0 and the amounts in
    ``error``."""
    c = _CHostReport()
    rc = _load().cc_host_link(device_index, mib, _origin, _poison_offset,
                              _poison_pass, ctypes.byref(c))
    rep = HostLinkReport.from_c(c)
    if rc != 0:
        raise AttestationError(
            f"device {device_index}: host link runtime error: {rep.error} rc={rc}"
        )
    return rep


def attest_host_link(device_index: int, mib: int, _origin: int = 0,
                     _poison_offset: int = -1,
                     _poison_pass: int = 0) -> HostLinkReport:
    """Move ``mib`` MiB across the PCIe link of one GPU five times, every
    word checked on the far side: the shader loads a CPU-filled pinned
    window (pull) and stores into it (push), the runtime's copy path
    carries it to the device (h2d) and back (d2h), and one launch does
    both directions at once (duplex). The pinned window and the device
    buffer live for the call. Raises when a word was wrong, when a pass
    did not run or when the buffers could not be allocated; there is no
    bandwidth floor here. ``_poison_offset`` / ``_poison_pass`` make the
    CPU flip one bit between a pass's write and its check (for testing
    the detector)."""
    rep = host_link_report(device_index, mib, _origin, _poison_offset,
                           _poison_pass)
    if not rep.ok:
        if rep.mismatch_words:
            where = f"first at offset {rep.first_bad_offset:#x}"
            if rep.bad:
                _, expected, got, bad_pass = rep.bad[0]
                name = (HOST_LINK_PASSES[bad_pass - 1]
                        if 1 <= bad_pass <= len(HOST_LINK_PASSES) else "?")
                where += (f" in pass {bad_pass} ({name}), expected^got="
                          f"{expected ^ got:#010x}")
            raise AttestationError(
                f"device {device_index}: host link FAILED: "
                f"{rep.mismatch_words} wrong word(s), {where}"
            )
        raise AttestationError(
            f"device {device_index}: host link FAILED: {rep.error} "
            f"({rep.passes}/5 passes)"
        )
    logger.info(
        "attested device %d: host link %d MiB, pull %.1f push %.1f h2d %.1f "
        "d2h %.1f GB/s, duplex %.1f + %.1f GB/s",
        rep.device,
        rep.bytes_tested >> 20,
        rep.pull_gbps,
        rep.push_gbps,
        rep.h2d_gbps,
        rep.d2h_gbps,
        rep.duplex_pull_gbps,
        rep.duplex_push_gbps,
    )
    return rep


_GENESIS = "cc-attest-log-v1"


def _chain_hash(prev: str, payload: str) -> str:
    import hashlib

    return hashlib.sha256((prev + payload).encode()).hexdigest()


def _append_attest_log(rep: AttestReport) -> None:
    """Append the report as HASH-CHAINED JSONL when CC_ATTEST_LOG is
    set: each record carries ``chain`` = sha256(prev_chain + record),
    so the audit trail of readiness decisions is tamper-evident —
    editing or deleting any record breaks every later link
    (:func:`verify_attest_log`)."""
    path = os.environ.get("CC_ATTEST_LOG")
    if not path:
        return
    import dataclasses
    import json
    import time

    try:
        prev = _GENESIS
        try:
            with open(path, "rb") as f:
                tail = f.read()[-4096:]
            for line in reversed(tail.splitlines()):
                if line.strip():
                    prev = json.loads(line).get("chain", _GENESIS)
                    break
        except (OSError, ValueError):
            pass
        entry = {"ts": time.time(), **dataclasses.asdict(rep)}
        payload = json.dumps(entry, sort_keys=True)
        entry["chain"] = _chain_hash(prev, payload)
        with open(path, "a") as f:
            f.write(json.dumps(entry, sort_keys=True) + "\n")
    except OSError as e:  # pragma: no cover
        logger.debug("attest log write failed: %s", e)


def verify_attest_log(path) -> int:
    """Walk the hash chain; return the number of verified records.
    Raises AttestationError at the first broken link (tampered, edited
    or truncated-in-the-middle log)."""
    import json

    prev = _GENESIS
    count = 0
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            if not line.strip():
                continue
            rec = json.loads(line)
            chain = rec.pop("chain", None)
            payload = json.dumps(rec, sort_keys=True)
            want = _chain_hash(prev, payload)
            if chain != want:
                raise AttestationError(
                    f"{path}:{lineno}: attestation log chain broken "
                    f"(record altered or log spliced)"
                )
            prev = chain
            count += 1
    return count


_BDF_RE = re.compile(
    r"^(?:(?P<domain>[0-9a-fA-F]{4}):)?(?P<bus>[0-9a-fA-F]{2}):(?P<dev>[0-9a-fA-F]{2})\.(?P<fn>[0-7])$"
)


def device_index_for_bdf(bdf: str) -> int:
    m = _BDF_RE.match(bdf.strip())
    if not m:
        raise AttestationError(f"unparseable bdf {bdf!r}")
    lib = _load()
    idx = lib.cc_device_index_for_bdf(
        int(m.group("domain") or "0", 16),
        int(m.group("bus"), 16),
        int(m.group("dev"), 16),
    )
    if idx < 0:
        raise AttestationError(f"no HIP device with bdf {bdf}")
    return idx


def attest_device_by_bdf(device) -> dict:
    """TransitionEngine attestor hook: CCDevice -> evidence summary
    (raises on failure).

    The probe gates cc.ready.state: a GPU that resets but cannot run
    MFMA/LDS work correctly must not be labeled ready (replaces the
    register-readback-only verify of the reference,
    /root/reference/main.py:523-529). The returned summary is published
    as the node's ``amd.com/gpu.cc.attest`` annotation — the evidence
    each readiness decision was based on.
    """
    gemm_dim = int(os.environ.get("CC_ATTEST_GEMM_DIM", "1024"))
    idx = device_index_for_bdf(device.bdf)
    rep = attest_device(idx, gemm_dim=gemm_dim)
    deep = False
    if os.environ.get("CC_ATTEST_DEEP", "0") == "1":
        from .deep_attest import deep_attest_device

        deep_attest_device(idx, gemm_dim=gemm_dim)
        deep = True
    mx = None
    if os.environ.get("CC_ATTEST_MXFP4", "0") == "1":
        mx = attest_mxfp4(idx, gemm_dim=gemm_dim)
    sweep = None
    if os.environ.get("CC_ATTEST_CU_SWEEP", "0") == "1":
        sweep = sweep_compute_units(idx)
    march = None
    hbm_mib = int(os.environ.get("CC_ATTEST_HBM_MIB") or "0")
    if hbm_mib > 0:
        march = march_hbm(
            idx, hbm_mib,
            chunk_mib=int(os.environ.get("CC_ATTEST_HBM_CHUNK_MIB") or "1024"))
    link = None
    host_mib = int(os.environ.get("CC_ATTEST_HOST_MIB") or "0")
    if host_mib > 0:
        link = attest_host_link(idx, host_mib)
        # an operator's own floor for the copy path; the project ships none
        floor = float(os.environ.get("CC_ATTEST_HOST_MIN_GBPS") or "0")
        if floor > 0 and min(link.h2d_gbps, link.d2h_gbps) < floor:
            raise AttestationError(
                f"device {idx}: host link below CC_ATTEST_HOST_MIN_GBPS="
                f"{floor:g}: h2d {link.h2d_gbps:.1f} GB/s, "
                f"d2h {link.d2h_gbps:.1f} GB/s"
            )
    summary = {
        "arch": rep.arch.split(":")[0],
        "cus": rep.cu_count,
        "gemm_tflops": round(rep.gemm_tflops, 1),
        "fp8_tflops": round(rep.fp8_tflops, 1),
        "hbm_gbps": round(rep.hbm_gbps),
        "bitwise_ok": rep.max_abs_err == 0.0 and rep.fp8_max_abs_err == 0.0,
        "xgmi": f"{rep.peers_verified}/{rep.peers_attempted} of {rep.peers_accessible}",
    }
    if rep.peers_accessible:
        summary["xgmi_gbps"] = [
            round(rep.xgmi_gbps_min), round(rep.xgmi_gbps_max)
        ]
    if deep:
        summary["deep_pmc"] = True
    if mx is not None:
        summary["mxfp4_tflops"] = round(mx.mx_tflops, 1)
        summary["mxfp4_bitwise_ok"] = mx.mx_max_abs_err == 0.0
    if sweep is not None:
        summary["cu_sweep"] = f"{sweep.units_seen}/{sweep.units_expected}"
        summary["cu_sweep_ok"] = sweep.ok
    if march is not None:
        summary["hbm_march_mib"] = march.bytes_tested >> 20
        summary["hbm_march_gbps"] = round(march.gbps)
        summary["hbm_march_ok"] = march.ok
        summary["hbm_scrubbed"] = march.scrubbed
    if link is not None:
        summary["host_link_mib"] = link.bytes_tested >> 20
        summary["host_link_gbps"] = [
            round(link.pull_gbps), round(link.push_gbps),
            round(link.h2d_gbps), round(link.d2h_gbps)
        ]
        summary["host_link_ok"] = link.ok
    return summary


def _gemm_call(fn_name: str, label: str, *args: int) -> None:
    """Call one of the library's GEMM entry points; raise on rc != 0."""
    rc = getattr(_load(), fn_name)(*args)
    if rc != 0:
        raise AttestationError(f"{label} rc={rc}")


def mfma_gemm_bf16(device_index: int, a_ptr: int, bt_ptr: int, c_ptr: int,
                   m: int, n: int, k: int) -> None:
    """Launch C[M,N] = A[M,K] @ Bt[N,K]^T on caller-owned device buffers
    (torch tensors via .data_ptr()). M,N multiples of 128, K of 64."""
    _gemm_call("cc_mfma_gemm_bf16", "mfma_gemm_bf16",
               device_index, a_ptr, bt_ptr, c_ptr, m, n, k)


def ref_gemm_f32(device_index: int, a_ptr: int, bt_ptr: int, c_ptr: int,
                 m: int, n: int, k: int) -> None:
    _gemm_call("cc_ref_gemm_f32", "ref_gemm_f32",
               device_index, a_ptr, bt_ptr, c_ptr, m, n, k)


def mfma_gemm_fp8(device_index: int, a_ptr: int, bt_ptr: int, c_ptr: int,
                  m: int, n: int, k: int) -> None:
    """MX-scaled fp8 e4m3 GEMM (unit scales): C = A @ Bt^T, fp32 out.
    M,N multiples of 128, K of 64."""
    _gemm_call("cc_mfma_gemm_fp8", "mfma_gemm_fp8",
               device_index, a_ptr, bt_ptr, c_ptr, m, n, k)


def mfma_gemm_fp8_variant(device_index: int, a_ptr: int, bt_ptr: int,
                          c_ptr: int, m: int, n: int, k: int,
                          which: int) -> None:
    """Force an fp8 variant: 3=BK64 4-blk (default dispatch for
    K%64-only shapes), 5=BK128 4-blk 1-buf (default dispatch past 1
    block/CU), 7=producer/consumer wave split (4 stage + 4 MFMA waves,
    LDS-flag handoff, barrier-free K loop; default dispatch up to 1
    block/CU), 8-12=instrumentation arms (8=5+XCD remap, 9=7+XCD remap,
    10=5+skew, 11=5+rotation, 12=5+skew+rotation), 13=256-tile 1-blk
    persistent. Any other number (0, 1, 2, 4, 6 and 14 were kernels that
    have been measured out and removed) raises with rc=-2 and launches
    nothing."""
    _gemm_call("cc_mfma_gemm_fp8_variant", f"mfma_gemm_fp8_variant({which})",
               device_index, a_ptr, bt_ptr, c_ptr, m, n, k, which)


def mfma_gemm_bf16_variant(device_index: int, a_ptr: int, bt_ptr: int,
                           c_ptr: int, m: int, n: int, k: int,
                           which: int) -> None:
    """Force a GEMM variant: 0 = 128x128 step-3, 1 = 256x256 8-phase,
    2 = 256x256 8-phase 32x32-op, 3 = 128x128 4-blocks/CU 1-buf. Any
    other number raises with rc=-2 and launches nothing."""
    _gemm_call("cc_mfma_gemm_bf16_variant", f"mfma_gemm_bf16_variant({which})",
               device_index, a_ptr, bt_ptr, c_ptr, m, n, k, which)


def mfma_gemm_mxfp4(device_index: int, a_ptr: int, sa_ptr: int, bt_ptr: int,
                    sb_ptr: int, c_ptr: int, m: int, n: int, k: int) -> None:
    """MXFP4 GEMM: C[m,n] = sum over 32-element K blocks kb of
    2^(SA[m,kb]+SB[n,kb]-254) * sum_k A[m,k]*Bt[n,k], fp32 out. A[M,K]
    and Bt[N,K] are e2m1 packed two per byte (low nibble = even k), SA
    and SB uint8 E8M0 [rows, K/32]. M,N multiples of 128, K of 256,
    16-byte aligned pointers; anything else raises with rc=-2."""
    _gemm_call("cc_mfma_gemm_mxfp4", "mfma_gemm_mxfp4",
               device_index, a_ptr, sa_ptr, bt_ptr, sb_ptr, c_ptr, m, n, k)


def ref_gemm_mxfp4_f32(device_index: int, a_ptr: int, sa_ptr: int, bt_ptr: int,
                       sb_ptr: int, c_ptr: int, m: int, n: int, k: int) -> None:
    """VALU reference of :func:`mfma_gemm_mxfp4` (integer nibble decode,
    ldexpf scales, no MFMA): any M and N, K a multiple of 32."""
    _gemm_call("cc_ref_gemm_mxfp4_f32", "ref_gemm_mxfp4_f32",
               device_index, a_ptr, sa_ptr, bt_ptr, sb_ptr, c_ptr, m, n, k)
