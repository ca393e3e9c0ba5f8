// CDNA4 (gfx950 / MI355X) post-reset attestation probe: the C API.
//
// The one hand-written kernel family of the AMD CC manager. After a CC
// transition resets a GPU, the reference merely re-reads the mode
// register. Here the device must additionally PROVE it executes
// correctly inside the TEE. This file is the one translation unit the
// build compiles. The device code lives next to it:
//
//   gemm_common.hip    types, LDS swizzles, shared staging / epilogue /
//                      remap helpers;
//   gemm_bf16.hip      bf16 MFMA GEMMs: mfma_gemm_bf16 (128x128 step-3),
//                      _256 / _256w (256x256 8-phase deep-pipelined,
//                      16x16x32 / 32x32x16 ops), _128u (4 blocks/CU);
//   gemm_fp8.hip       MX-scaled OCP e4m3 MFMA GEMMs (unit e8m0 scales):
//                      mfma_gemm_fp8_128s / _128u / _128pc / _256x;
//   gemm_fp4.hip       MXFP4 (e2m1, real e8m0 block scales) MFMA GEMM:
//                      mfma_gemm_mxfp4_128u;
//   probe_kernels.hip  fills, ref_gemm_f32 (plain VALU fp32 GEMM of the
//                      same inputs: the independent on-device ground
//                      truth), the MXFP4 fills and ref_gemm_mxfp4_f32,
//                      max-diff, checksum, LDS, HBM, liveness;
//   cu_sweep.hip       compute-unit sweep: cu_sweep (per-SIMD MFMA chains
//                      and a whole-LDS march, keyed by the hardware ID
//                      registers) and cu_sweep_gold (its VALU reference);
//   hbm_march.hip      HBM march: march_step<check, write> (address-keyed
//                      pattern, its complement, zero; every word verified)
//                      and march_poison;
//   host_link.hip      host link: link_pull / link_push / link_duplex, the
//                      same pattern loaded and stored by the shader across
//                      PCIe on mapped, page-locked host memory.
//
// and the host code, included after it:
//
//   probe_reports.hip  the five report structs (frozen layouts);
//   gemm_dispatch.hip  named variants, launchers, production dispatch;
//   probe_ctx.hip      CC_CHECK / CC_TRY, DevBuf, the per-leg contexts of
//                      a DeviceCtx, timed_ms, read_back, DeviceHop;
//   host_pattern.hip   the CPU fill and compare of the host-link leg
//                      (plain C++, no HIP call);
//   probe_legs.hip     the ten legs and the steps the GEMM legs share.
//
// cc_attest_device runs five legs in order:
//   1. probe_bf16  — production bf16 GEMM dispatch, timed, compared
//                    with ref_gemm_f32 (inputs are small integers, so
//                    the bf16 AND fp8 MFMA paths must both agree
//                    BITWISE — any mismatch is silicon/TEE trouble) and
//                    checksummed;
//   2. probe_fp8   — production fp8 GEMM dispatch, same reference;
//   3. probe_lds   — LDS cell sweep with rotating patterns;
//   4. probe_hbm   — vectorized streaming copy (HBM3E path, GB/s);
//   5. probe_xgmi  — for every sampled accessible peer: timed copies of
//                    the result buffer across the link and a checksum
//                    recomputed ON THE PEER.
// cc_attest_mxfp4 is a separate, opt-in probe with its own report:
// the MXFP4 GEMM against ref_gemm_mxfp4_f32, bitwise.
// cc_cu_sweep is another: cu_sweep.hip's matrix-core and whole-LDS
// self-test on every SIMD of every CU, with the units it reached read
// from the hardware ID registers.
// cc_hbm_march is the third: hbm_march.hip's four verified passes over
// an explicit window of VRAM, which is left zeroed and checked zero.
// cc_host_link is the fourth: five verified passes of that pattern across
// PCIe, both engines (shader and the runtime's copy path), both
// directions and both at once, on a pinned host window that lives for
// the call.

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "gemm_common.hip"
#include "gemm_bf16.hip"
#include "gemm_fp8.hip"
#include "gemm_fp4.hip"
#include "probe_kernels.hip"
#include "cu_sweep.hip"
#include "hbm_march.hip"
#include "host_link.hip"

#include "probe_reports.hip"
#include "gemm_dispatch.hip"
#include "probe_ctx.hip"
#include "host_pattern.hip"
#include "probe_legs.hip"

// What the report-returning entry points begin with: -1 for a
// null report; else the report zeroed and rep->device set, -5 for a
// device outside the context table, `refuse` (a nonzero status ends the
// call before the device is touched), hipSetDevice.
template <typename Report, typename Refuse = int (*)()>
static int report_begin(Report* rep, int device,
                        Refuse refuse = [] { return 0; }) {
  if (!rep) return -1;
  __builtin_memset(rep, 0, sizeof(*rep));
  rep->device = device;
  if (device < 0 || device >= kMaxDevices) return -5;
  CC_TRY(refuse());
  CC_CHECK(hipSetDevice(device));
  return 0;
}

// What the march and host-link entry points refuse about the logical
// address range: the kernels rely on 16-byte vectors that never straddle
// 2^32 words.
template <typename Report>
static int hbm_refuse_range(Report* rep, unsigned long long origin,
                            unsigned long long bytes) {
  if (origin % 16 == 0 && origin <= (1ull << 48) &&
      bytes <= (1ull << 48) - origin)
    return 0;
  snprintf(rep->error, sizeof(rep->error),
           "origin %llu not a multiple of 16, or origin + bytes above 2^48",
           origin);
  return -2;
}

extern "C" {

int cc_device_alive(int device) {
  if (device < 0 || device >= kMaxDevices) return -1;
  if (hipSetDevice(device) != hipSuccess) return -1;
  int* d = nullptr;
  {
    // the word outlives the lock: nothing but cc_attest_shutdown frees it
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    DeviceCtx& dev = device_ctx(device);
    if (dev.dLive.ensure(sizeof(int)) != hipSuccess) return -2;
    d = dev.dLive;
  }
  if (hipMemset(d, 0, sizeof(int)) != hipSuccess) return -2;
  hipLaunchKernelGGL(liveness_kernel, dim3(1), dim3(64), 0, 0, d);
  int h = 0;
  hipError_t e = hipMemcpy(&h, d, sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return -3;
  return h == 0x600D ? 0 : -4;
}

int cc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

int cc_device_index_for_bdf(int domain, int bus, int dev) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) != hipSuccess) continue;
    if (p.pciDomainID == domain && p.pciBusID == bus && p.pciDeviceID == dev)
      return i;
  }
  return -1;
}

// Run the bf16 MFMA GEMM on caller-provided device buffers (e.g. torch
// tensors): C[M,N] = A[M,K] @ Bt[N,K]^T. M,N multiples of 128, K of 64
// (the deep-pipelined 256x256 variants are selected automatically when
// M,N are multiples of 256, K of 128 and the 128-tile grid exceeds one
// block per CU).
int cc_mfma_gemm_bf16(int device, const void* A, const void* Bt, void* C,
                      int M, int N, int K) {
  if (hipSetDevice(device) != hipSuccess) return -3;
  int rc = launch_mfma_gemm(A, Bt, C, M, N, K);
  if (rc != 0) return rc;
  return (int)hipDeviceSynchronize();
}

// Force a specific bf16 variant (perf characterization / A-B); `which`
// is one of kBf16Forced (0-3), anything else returns -2 without launching.
int cc_mfma_gemm_bf16_variant(int device, const void* A, const void* Bt,
                              void* C, int M, int N, int K, int which) {
  return run_forced_variant(forced_variant(kBf16Forced, which), 2, device, A,
                            Bt, C, M, N, K);
}

// Force a specific fp8 variant (perf characterization / A-B); `which`
// is one of kFp8Forced (3, 5, 7-13), anything else returns -2 without
// launching.
int cc_mfma_gemm_fp8_variant(int device, const void* A, const void* Bt,
                             void* C, int M, int N, int K, int which) {
  return run_forced_variant(forced_variant(kFp8Forced, which), 1, device, A,
                            Bt, C, M, N, K);
}

// MX-scaled fp8 (e4m3) GEMM: C[M,N] = A[M,K] @ Bt[N,K]^T, fp8 inputs,
// fp32 out. M,N multiples of 128; K multiple of 64.
int cc_mfma_gemm_fp8(int device, const void* A, const void* Bt, void* C,
                     int M, int N, int K) {
  if (hipSetDevice(device) != hipSuccess) return -3;
  int rc = launch_fp8_best(A, Bt, C, M, N, K);
  if (rc != 0) return rc;
  return (int)hipDeviceSynchronize();
}

// Plain fp32 reference GEMM on the same operand convention.
int cc_ref_gemm_f32(int device, const void* A, const void* Bt, void* C,
                    int M, int N, int K) {
  if (hipSetDevice(device) != hipSuccess) return -3;
  dim3 block(16, 16);
  dim3 grid((N + 15) / 16, (M + 15) / 16);
  hipLaunchKernelGGL(ref_gemm_f32, grid, block, 0, 0, (const bf16*)A,
                     (const bf16*)Bt, (float*)C, M, N, K);
  return (int)hipDeviceSynchronize();
}

// The full self-contained attestation probe. gemm_dim: problem size
// (square); 1024 for the post-reset gate (fast), 4096+ for perf
// characterization. rep->ok = 1 iff every stage validated.
int cc_attest_device(int device, int gemm_dim, struct CcAttestReport* rep) {
  CC_TRY(report_begin(rep, device));

  hipDeviceProp_t prop;
  CC_CHECK(hipGetDeviceProperties(&prop, device));
  rep->cu_count = prop.multiProcessorCount;
  rep->vram_total_mb = (long long)(prop.totalGlobalMem >> 20);
  __builtin_strncpy(rep->arch, prop.gcnArchName, sizeof(rep->arch) - 1);

  const int D = (gemm_dim / BM) * BM > 0 ? (gemm_dim / BM) * BM : BM;
  rep->gemm_m = rep->gemm_n = rep->gemm_k = D;

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  DeviceCtx& dev = device_ctx(device);
  CC_CHECK(dev.main.acquire(D));
  CC_CHECK(dev.events());

  CC_TRY(probe_bf16(dev, rep));
  CC_TRY(probe_fp8(dev, rep));
  CC_TRY(probe_lds(dev, rep));
  CC_TRY(probe_hbm(dev, rep));
  CC_TRY(probe_xgmi(dev, rep));

  rep->ok = (rep->max_abs_err == 0.0f) && (rep->fp8_max_abs_err == 0.0f) &&
                    (rep->lds_failures == 0) && (rep->gemm_tflops > 0.0) &&
                    (rep->peers_verified == rep->peers_attempted)
                ? 1
                : 0;
  return 0;
}

// ABI guard: Python mirrors CcAttestReport with a ctypes.Structure —
// a size mismatch means the mirror drifted and fields would be read
// from wrong offsets (checked by a CPU test on every suite run).
int cc_report_sizeof(void) { return (int)sizeof(struct CcAttestReport); }

// MXFP4 GEMM on caller-provided device buffers (layout in
// gemm_fp4.hip): packed e2m1 A[M,K/2], Bt[N,K/2], e8m0 SA[M,K/32],
// SB[N,K/32], fp32 C[M,N]. M,N multiples of 128, K of 256; anything
// else returns -2 without launching.
int cc_mfma_gemm_mxfp4(int device, const void* A, const void* SA,
                       const void* Bt, const void* SB, void* C, int M, int N,
                       int K) {
  if (hipSetDevice(device) != hipSuccess) return -3;
  int rc = launch_mxfp4(A, SA, Bt, SB, C, M, N, K);
  if (rc != 0) return rc;
  return (int)hipDeviceSynchronize();
}

// VALU reference of the same convention: any M and N, K a multiple of 32.
int cc_ref_gemm_mxfp4_f32(int device, const void* A, const void* SA,
                          const void* Bt, const void* SB, void* C, int M,
                          int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32) return -2;
  if (hipSetDevice(device) != hipSuccess) return -3;
  launch_ref_mxfp4(A, SA, Bt, SB, C, M, N, K);
  return (int)hipDeviceSynchronize();
}

// The opt-in MXFP4 probe. gemm_dim below 256 rounds up to 256, otherwise
// down to a multiple of 256. rep->ok = 1 iff the MFMA result equals the
// VALU reference bitwise.
int cc_attest_mxfp4(int device, int gemm_dim, struct CcMxReport* rep) {
  CC_TRY(report_begin(rep, device));

  const int D = gemm_dim < BK4 ? BK4 : (gemm_dim / BK4) * BK4;
  rep->mx_m = rep->mx_n = rep->mx_k = D;

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  DeviceCtx& dev = device_ctx(device);
  CC_CHECK(dev.events());
  CC_CHECK(dev.mx.acquire(D));
  CC_TRY(probe_mxfp4(dev, rep));

  rep->ok = (rep->mx_max_abs_err == 0.0f) && (rep->mx_tflops > 0.0) ? 1 : 0;
  return 0;
}

// ABI guard for CcMxReport, as cc_report_sizeof for CcAttestReport.
int cc_mx_report_sizeof(void) { return (int)sizeof(struct CcMxReport); }

// The opt-in compute-unit sweep. rounds: accumulating MFMAs per chain,
// 1..CU_SWEEP_MAX_ROUNDS (anything else returns -2 without launching).
// poison_key: -1, or the key of a unit whose waves flip one accumulator
// bit before the compare (a wrong number, to test the detector).
// rep->ok = 1 iff no unit miscompared and every SIMD of every CU
// reported; short coverage is a failure with rep->error set.
int cc_cu_sweep(int device, int rounds, int poison_key,
                struct CcSweepReport* rep) {
  CC_TRY(report_begin(rep, device, [&] {
    rep->rounds = rounds;
    if (rounds >= 1 && rounds <= CU_SWEEP_MAX_ROUNDS) return 0;
    snprintf(rep->error, sizeof(rep->error), "rounds %d outside 1..%d", rounds,
             CU_SWEEP_MAX_ROUNDS);
    return -2;
  }));
  hipDeviceProp_t prop;
  CC_CHECK(hipGetDeviceProperties(&prop, device));
  rep->cu_count = prop.multiProcessorCount;
  rep->units_expected = 4 * rep->cu_count;

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  DeviceCtx& dev = device_ctx(device);
  CC_CHECK(dev.events());
  CC_CHECK(dev.sweep.acquire());
  CC_TRY(probe_cu_sweep(dev, rep, poison_key));

  const bool covered = rep->units_seen == rep->units_expected &&
                       rep->cus_seen == rep->cu_count;
  if (!covered)
    snprintf(rep->error, sizeof(rep->error),
             "coverage %d/%d after %d launches", rep->units_seen,
             rep->units_expected, rep->launches);
  rep->ok = covered && rep->units_failed == 0 && rep->lds_failures == 0 ? 1 : 0;
  return 0;
}

// The golden C images of the sweep for `rounds` (3328 floats: 32x32,
// 16x16, 32x32, 32x32, row-major), copied to the host.
int cc_cu_sweep_gold(int device, int rounds, float* host_out_3328) {
  if (!host_out_3328) return -1;
  if (device < 0 || device >= kMaxDevices) return -5;
  if (rounds < 1 || rounds > CU_SWEEP_MAX_ROUNDS) return -2;
  if (hipSetDevice(device) != hipSuccess) return -3;
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  DeviceCtx& dev = device_ctx(device);
  if (dev.events() != hipSuccess || dev.sweep.acquire() != hipSuccess)
    return -4;
  ErrorText err;
  double ms = 0.0;
  CC_TRY(sweep_gold(dev, &err, rounds, &ms));
  return (int)hipMemcpy(host_out_3328, dev.sweep.dSweepGold,
                        CU_SWEEP_GOLD_ELEMS * sizeof(float),
                        hipMemcpyDeviceToHost);
}

// The unit table of the last sweep on `device`: for every unit reached,
// ascending by key, its key (want_hits == 0) or the number of waves
// that reported from it; at most `cap` written, the count returned (0
// before the first sweep).
static int sweep_table(int device, unsigned* out, int cap, int want_hits) {
  if (device < 0 || device >= kMaxDevices) return -5;
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  const SweepCtx& c = g_ctx[device].sweep;
  if (!c.valid) return 0;
  int n = 0;
  for (int k = 0; k < CU_SWEEP_UNITS; ++k) {
    unsigned hits = c.hSweepTab[k * CU_SWEEP_REC];
    if (!hits) continue;
    if (out && n < cap) out[n] = want_hits ? hits : (unsigned)k;
    ++n;
  }
  return n;
}

// Keys of the units the last sweep on `device` reached.
int cc_cu_sweep_units(int device, unsigned* keys_out, int cap) {
  return sweep_table(device, keys_out, cap, 0);
}

// How many waves reported from each of those units, in the same order.
int cc_cu_sweep_hits(int device, unsigned* hits_out, int cap) {
  return sweep_table(device, hits_out, cap, 1);
}

// ABI guard for CcSweepReport, as cc_report_sizeof for CcAttestReport.
int cc_sweep_report_sizeof(void) { return (int)sizeof(struct CcSweepReport); }

// The opt-in HBM march: `mib` MiB of VRAM, held as chunks of `chunk_mib`
// (1..1024), filled, flipped, scrubbed to zero and checked zero, every
// word verified in between (hbm_march.hip). origin: logical byte address
// of the window's first byte (keys the pattern; 0 in production, a
// multiple of 16). poison_offset: -1, or the window byte offset of a
// word whose bit 0 is flipped after pass poison_after (1..3), to test
// the detector. Anything out of range returns -2 before the device is
// touched. rep->ok = 1 iff the whole window was allocated, all four
// passes ran and no word was wrong; a window that could not be
// allocated is ok = 0 with rc 0. Nothing stays allocated afterwards.
int cc_hbm_march(int device, long long mib, int chunk_mib,
                 unsigned long long origin, long long poison_offset,
                 int poison_after, struct CcHbmReport* rep) {
  hipDeviceProp_t prop;
  CC_TRY(report_begin(rep, device, [&] {
    rep->origin = origin;
    rep->first_bad_offset = ~0ull;
    auto refuse = [&](const char* what) {
      snprintf(rep->error, sizeof(rep->error), "%s", what);
      return -2;
    };
    if (mib < 1 || mib > (1ll << 28)) return refuse("mib outside 1..2^28");
    if (chunk_mib < 1 || chunk_mib > 1024)
      return refuse("chunk_mib outside 1..1024");
    const long long bytes = mib << 20;
    rep->bytes_requested = bytes;
    rep->chunk_bytes = (long long)chunk_mib << 20;
    CC_TRY(hbm_refuse_range(rep, origin, bytes));
    if (poison_offset != -1) {
      if (poison_offset < 0 || poison_offset >= bytes || poison_offset % 4)
        return refuse("poison offset outside the window or not 4-aligned");
      if (poison_after < 1 || poison_after > 3)
        return refuse("poison_after outside 1..3");
    }
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
      return refuse("no such device");
    if ((unsigned long long)bytes > prop.totalGlobalMem)
      return refuse("window larger than the device's memory");
    return 0;
  }));

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  DeviceCtx& dev = device_ctx(device);
  CC_CHECK(dev.events());
  CC_CHECK(dev.hbm.acquire());
  CC_TRY(probe_hbm_march(dev, rep, prop.multiProcessorCount, poison_offset,
                         poison_offset == -1 ? 0 : poison_after));

  rep->beyond_cache = rep->bytes_tested >= (512ll << 20);
  rep->scrubbed = rep->passes == 4 && rep->mismatch_words == 0;
  rep->ok = rep->bytes_tested == rep->bytes_requested && rep->scrubbed;
  return 0;
}

// One march_step on a caller-owned device buffer (e.g. a torch tensor):
// compare with phase `check`, overwrite with phase `write` (-1..2, -1 =
// none, not both). bytes a positive multiple of 16, ptr 16-aligned,
// origin as for cc_hbm_march; anything else returns -2 without
// launching. Offsets in the report are from ptr; bad_pass stays 0. The
// kernel time lands in fill_ms (write only), zero_ms (check only) or
// flip_ms (both), gbps counts the bytes read plus the bytes written.
int cc_hbm_step(int device, void* ptr, long long bytes,
                unsigned long long origin, int check, int write,
                struct CcHbmReport* rep) {
  CC_TRY(report_begin(rep, device, [&] {
    rep->origin = origin;
    rep->first_bad_offset = ~0ull;
    if (!ptr || (uintptr_t)ptr % 16 || bytes < 16 || bytes % 16 ||
        check < -1 || check > 2 || write < -1 || write > 2 ||
        (check == -1 && write == -1)) {
      snprintf(rep->error, sizeof(rep->error),
               "need a 16-aligned pointer, bytes a positive multiple of 16, "
               "check and write in -1..2 and not both -1");
      return -2;
    }
    return hbm_refuse_range(rep, origin, bytes);
  }));
  hipDeviceProp_t prop;
  CC_CHECK(hipGetDeviceProperties(&prop, device));
  rep->bytes_requested = bytes;
  rep->chunk_bytes = bytes < (long long)HBM_MARCH_MAX_CHUNK
                         ? bytes
                         : (long long)HBM_MARCH_MAX_CHUNK;
  rep->chunks = (int)((bytes + rep->chunk_bytes - 1) / rep->chunk_bytes);

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  DeviceCtx& dev = device_ctx(device);
  CC_CHECK(dev.events());
  CC_CHECK(dev.hbm.acquire());
  CC_TRY(march_reset(dev, rep));
  double* ms = check < 0 ? &rep->fill_ms
                         : write < 0 ? &rep->zero_ms : &rep->flip_ms;
  CC_TRY(timed_ms(dev, rep, ms, [&] {
    launch_march(check, write, ptr, bytes, origin, 0, dev.hbm.dRes, 0,
                 prop.multiProcessorCount);
    return 0;
  }));
  CC_CHECK(hipGetLastError());
  CC_TRY(march_collect(dev, rep));
  rep->passes = 1;
  rep->bytes_tested = bytes;
  rep->gbps = ((check >= 0) + (write >= 0)) * (double)bytes / (*ms * 1e-3) / 1e9;
  rep->beyond_cache = bytes >= (512ll << 20);
  rep->ok = rep->mismatch_words == 0;
  return 0;
}

// ABI guard for CcHbmReport, as cc_report_sizeof for CcAttestReport.
int cc_hbm_report_sizeof(void) { return (int)sizeof(struct CcHbmReport); }

// What cc_host_step and cc_host_pattern refuse about a caller's host
// range and direction, with the text in rep->error.
static int host_refuse_range(CcHostReport* rep, const void* host_ptr,
                             long long nbytes, unsigned long long origin,
                             int check, int write) {
  const bool one_way = (check >= 0 && check <= 2 && write == -1) ||
                       (write >= 0 && write <= 2 && check == -1);
  if (!host_ptr || (uintptr_t)host_ptr % 16 || nbytes < 16 || nbytes % 16 ||
      nbytes > (long long)HOST_LINK_MAX_BYTES || !one_way) {
    snprintf(rep->error, sizeof(rep->error),
             "need a 16-aligned pointer, nbytes a positive multiple of 16 of "
             "at most 1 GiB, and exactly one of check / write in 0..2 with "
             "the other -1");
    return -2;
  }
  return hbm_refuse_range(rep, origin, nbytes);
}

// The opt-in host-link leg: `mib` MiB (1..1024) of page-locked host
// memory H and as much device memory D, both allocated for the call.
// Five passes move the march's pattern across PCIe and check every word
// on the far side (probe_host_link): pull and push by the shader on the
// mapped window, h2d and d2h by the runtime's copy path, and a duplex
// launch that does both at once. Pass k (1..5) uses logical origin
// origin + k * 2^40; origin is a multiple of 16 with origin + 6 * 2^40
// at most 2^48. poison_offset: -1, or the window byte offset of a word
// of H whose bit 0 the CPU flips in pass poison_pass (1..5) between that
// pass's write and its check, to test the detector. Anything out of
// range returns -2 before anything is allocated or launched. rep->ok = 1
// iff all five passes ran, no word was wrong and every rate is above
// zero; there is no bandwidth floor. Buffers that could not be allocated
// are ok = 0 with rc 0. Nothing stays allocated or pinned afterwards.
int cc_host_link(int device, long long mib, unsigned long long origin,
                 long long poison_offset, int poison_pass,
                 struct CcHostReport* rep) {
  CC_TRY(report_begin(rep, device, [&] {
    rep->origin = origin;
    rep->first_bad_offset = ~0ull;
    auto refuse = [&](const char* what) {
      snprintf(rep->error, sizeof(rep->error), "%s", what);
      return -2;
    };
    if (mib < 1 || mib > 1024) return refuse("mib outside 1..1024");
    rep->bytes_requested = mib << 20;
    CC_TRY(hbm_refuse_range(rep, origin, 6 * HOST_LINK_PASS_STRIDE));
    if (poison_offset != -1) {
      if (poison_offset < 0 || poison_offset >= rep->bytes_requested ||
          poison_offset % 4)
        return refuse("poison offset outside the window or not 4-aligned");
      if (poison_pass < 1 || poison_pass > 5)
        return refuse("poison_pass outside 1..5");
    }
    return 0;
  }));
  hipDeviceProp_t prop;
  CC_CHECK(hipGetDeviceProperties(&prop, device));

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  DeviceCtx& dev = device_ctx(device);
  CC_CHECK(dev.events());
  CC_CHECK(dev.host.acquire());
  CC_TRY(probe_host_link(dev, rep, prop.multiProcessorCount, poison_offset,
                         poison_offset == -1 ? 0 : poison_pass));

  rep->ok = rep->passes == 5 && rep->mismatch_words == 0 &&
            rep->pull_gbps > 0.0 && rep->push_gbps > 0.0 &&
            rep->h2d_gbps > 0.0 && rep->d2h_gbps > 0.0 &&
            rep->duplex_pull_gbps > 0.0 && rep->duplex_push_gbps > 0.0;
  return 0;
}

// One direction of the host link on caller-owned host memory (e.g. a
// numpy array), the counterpart of cc_hbm_step. Exactly one of check /
// write is a phase 0..2, the other -1. check: the data flows host ->
// device and is compared on the device, by link_pull on the mapped range
// (engine 0) or by a copy into a staging buffer and march_step there
// (engine 1). write: the pattern is generated on the device and lands in
// the caller's memory, by link_push (engine 0) or by a march_step fill
// of the staging buffer and a copy (engine 1). The range is page-locked
// for the call with hipHostRegister unless it already is, and
// unregistered on every path out; device and managed memory are refused.
// host_ptr 16-aligned, nbytes a positive multiple of 16 of at most
// 1 GiB, origin as for cc_hbm_step; anything else returns -2 before the
// device is touched. Bytes outside the range are never written. Offsets
// in the report are from host_ptr; bad_pass stays 0. The time lands in
// pull_ms / push_ms (engine 0) or h2d_ms / d2h_ms (engine 1, the copy
// alone).
int cc_host_step(int device, void* host_ptr, long long nbytes,
                 unsigned long long origin, int check, int write, int engine,
                 struct CcHostReport* rep) {
  CC_TRY(report_begin(rep, device, [&] {
    rep->origin = origin;
    rep->engine = engine;
    rep->first_bad_offset = ~0ull;
    if (engine != 0 && engine != 1) {
      snprintf(rep->error, sizeof(rep->error), "engine %d outside 0..1",
               engine);
      return -2;
    }
    return host_refuse_range(rep, host_ptr, nbytes, origin, check, write);
  }));
  rep->bytes_requested = nbytes;
  hipDeviceProp_t prop;
  CC_CHECK(hipGetDeviceProperties(&prop, device));

  // already page-locked (hipHostMalloc or the caller's registration)?
  hipPointerAttribute_t attr = {};
  bool pinned = false;
  if (hipPointerGetAttributes(&attr, host_ptr) != hipSuccess) {
    (void)hipGetLastError();  // ordinary memory the runtime has not seen
  } else if (attr.type == hipMemoryTypeHost) {
    pinned = true;
  } else if (attr.type != hipMemoryTypeUnregistered) {
    snprintf(rep->error, sizeof(rep->error),
             "host_ptr is device or managed memory (type %d)", (int)attr.type);
    return -2;
  }

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  DeviceCtx& dev = device_ctx(device);
  CC_CHECK(dev.events());
  CC_CHECK(dev.host.acquire());
  HostWindow win;
  if (!pinned) {
    CC_CHECK(hipHostRegister(host_ptr, nbytes, hipHostRegisterMapped));
    win.registered = host_ptr;
  }
  void* dptr = nullptr;
  CC_CHECK(hipHostGetDevicePointer(&dptr, host_ptr, 0));
  CC_TRY(probe_host_step(dev, rep, win, host_ptr, dptr, check, write,
                         prop.multiProcessorCount));
  rep->ok = rep->passes == 1 && rep->mismatch_words == 0;
  return 0;
}

// The CPU fill (write) or compare (check) of the host-link leg on its
// own, on any host memory: no HIP call, so it runs without a GPU.
// Arguments and refusals as cc_host_step's; rep->device is -1 and the
// time lands in host_ms.
int cc_host_pattern(void* host_ptr, long long nbytes,
                    unsigned long long origin, int check, int write,
                    struct CcHostReport* rep) {
  if (!rep) return -1;
  __builtin_memset(rep, 0, sizeof(*rep));
  rep->device = -1;
  rep->origin = origin;
  rep->first_bad_offset = ~0ull;
  CC_TRY(host_refuse_range(rep, host_ptr, nbytes, origin, check, write));
  rep->bytes_requested = nbytes;
  HbmMarchResult res = {};
  res.first_bad_offset = ~0ull;
  const auto t0 = std::chrono::steady_clock::now();
  if (write >= 0)
    host_pattern_fill((uint32_t*)host_ptr, nbytes / 4, origin / 4, write);
  else
    host_pattern_compare((const uint32_t*)host_ptr, nbytes / 4, origin / 4, 0,
                         check, 0, &res);
  rep->host_ms = std::chrono::duration<double, std::milli>(
                     std::chrono::steady_clock::now() - t0)
                     .count();
  link_report(res, rep);
  rep->passes = 1;
  rep->bytes_tested = nbytes;
  rep->ok = rep->mismatch_words == 0;
  return 0;
}

// ABI guard for CcHostReport, as cc_report_sizeof for CcAttestReport.
int cc_host_report_sizeof(void) { return (int)sizeof(struct CcHostReport); }

// Free everything every device context holds (daemon shutdown / tests).
void cc_attest_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  for (int i = 0; i < kMaxDevices; ++i) {
    if (!g_ctx[i].used) continue;
    (void)hipSetDevice(i);
    g_ctx[i].release();
  }
}

}  // extern "C"
