// CDNA4 (gfx950 / MI355X) post-reset attestation probe: the C API.
//
// The one hand-written kernel family of the AMD CC manager. After a CC
// transition resets a GPU, the reference merely re-reads the mode
// register. Here the device must additionally PROVE it executes
// correctly inside the TEE. This file is the one translation unit the
// build compiles; the device code lives next to it:
//
//   gemm_common.hip    types, LDS swizzles, shared staging / epilogue /
//                      remap helpers;
//   gemm_bf16.hip      bf16 MFMA GEMMs: mfma_gemm_bf16 (128x128 step-3),
//                      _256 / _256w (256x256 8-phase deep-pipelined,
//                      16x16x32 / 32x32x16 ops), _128u (4 blocks/CU);
//   gemm_fp8.hip       MX-scaled OCP e4m3 MFMA GEMMs (unit e8m0 scales):
//                      mfma_gemm_fp8_128 / _256 / _128w / _128s / _128t /
//                      _128u / _256u / _128pc / _256x / _128sk;
//   gemm_fp4.hip       MXFP4 (e2m1, real e8m0 block scales) MFMA GEMM:
//                      mfma_gemm_mxfp4_128u;
//   probe_kernels.hip  fills, ref_gemm_f32 (plain VALU fp32 GEMM of the
//                      same inputs: the independent on-device ground
//                      truth), the MXFP4 fills and ref_gemm_mxfp4_f32,
//                      max-diff, checksum, LDS, HBM, liveness;
//   cu_sweep.hip       compute-unit sweep: cu_sweep (per-SIMD MFMA chains
//                      and a whole-LDS march, keyed by the hardware ID
//                      registers) and cu_sweep_gold (its VALU reference).
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

#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "gemm_common.hip"
#include "gemm_bf16.hip"
#include "gemm_fp8.hip"
#include "gemm_fp4.hip"
#include "probe_kernels.hip"
#include "cu_sweep.hip"

#define CC_CHECK(expr)                                                         \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      snprintf(rep->error, sizeof(rep->error), "%s: %s", #expr,                \
               hipGetErrorString(_e));                                         \
      return (int)_e;                                                          \
    }                                                                          \
  } while (0)

// propagate a nonzero int status
#define CC_TRY(expr)                                                           \
  do {                                                                         \
    int _rc = (expr);                                                          \
    if (_rc != 0) return _rc;                                                  \
  } while (0)

// ===========================================================================
// Variant tables and dispatch
// ===========================================================================
// A launcher starts one kernel on the null stream (no sync); `arg` is
// the kernel's extra opts / xcd_swizzle argument where it has one.
typedef int (*GemmLauncher)(dim3 grid, int threads, const void* A,
                            const void* Bt, void* C, int M, int N, int K,
                            int arg);

template <typename T, void (*KERNEL)(const T*, const T*, float*, int, int, int)>
static int launch_plain(dim3 grid, int threads, const void* A, const void* Bt,
                        void* C, int M, int N, int K, int) {
  hipLaunchKernelGGL(KERNEL, grid, dim3(threads), 0, 0, (const T*)A,
                     (const T*)Bt, (float*)C, M, N, K);
  return 0;
}

template <typename T,
          void (*KERNEL)(const T*, const T*, float*, int, int, int, int)>
static int launch_arg(dim3 grid, int threads, const void* A, const void* Bt,
                      void* C, int M, int N, int K, int arg) {
  hipLaunchKernelGGL(KERNEL, grid, dim3(threads), 0, 0, (const T*)A,
                     (const T*)Bt, (float*)C, M, N, K, arg);
  return 0;
}

// forced split-K (the tiny-grid shape at any size): slice K so the grid
// reaches ~1024 blocks, zero C, accumulate with atomics
static int launch_splitk(dim3 grid, int threads, const void* A, const void* Bt,
                         void* C, int M, int N, int K, int) {
  int nk = K / BK8;
  long blocks = (long)grid.x * grid.y;
  int S = (int)(1024 / (blocks ? blocks : 1));
  if (S > nk) S = nk;
  if (S < 2) S = 2;
  if (hipMemsetAsync(C, 0, (long)M * N * sizeof(float), 0) != hipSuccess)
    return -4;
  dim3 g(grid.x, grid.y, S);
  hipLaunchKernelGGL(mfma_gemm_fp8_128sk, g, dim3(threads), 0, 0,
                     (const char*)A, (const char*)Bt, (float*)C, M, N, K);
  return 0;
}

constexpr int kXcdAuto = -1;  // arg: XCD remap iff past_infinity_cache()

struct GemmVariant {
  int tile_m, tile_n;  // block tile; M and N must be multiples
  int k_mult;          // K must be a multiple
  int threads;
  GemmLauncher launch;
  int arg;
};

// bf16 variants, indexed by `which` of cc_mfma_gemm_bf16_variant:
// 0 = 128x128 step-3, 1 = 256x256 8-phase (16x16 op),
// 2 = 256x256 8-phase (32x32 op), 3 = 128x128 single-buffered
// 4-blocks/CU (measured slower than the deep pipeline — kept as the
// recorded negative arm of the occupancy series).
static const GemmVariant kBf16Variants[] = {
    {BM, BN, BK, 256, launch_plain<bf16, mfma_gemm_bf16>, 0},
    {BM2, BN2, 2 * BK2, 512, launch_arg<bf16, mfma_gemm_bf16_256>, kXcdAuto},
    {BM2, BN2, 2 * BK2, 512, launch_arg<bf16, mfma_gemm_bf16_256w>, kXcdAuto},
    {BM, BN, 64, 256, launch_plain<bf16, mfma_gemm_bf16_128u>, 0},
};
enum { kBf16_128 = 0, kBf16_256 = 1, kBf16_256w = 2 };

// fp8 variants, indexed by `which` of cc_mfma_gemm_fp8_variant
// (measured ladder in BASELINE.md):
//  0 = 128-tile BK=128 double-buffered (2 blocks/CU),
//  1 = 256-tile 8-phase deep pipeline,
//  2 = 128-tile BK=256 (1 block/CU),
//  3 = BK=64 32x32-op (4 blocks/CU; production's K%64-only fall-back),
//  4 = BK=128 1.5-buffered (3 blocks/CU),
//  5 = BK=128 SINGLE-buffered (4 blocks/CU; production past 1 block/CU),
//  6 = 256x128 tile, 512 threads (2 blocks/CU),
//  7 = producer/consumer wave split (4 stage waves + 4 MFMA waves,
//      LDS-flag handoff, no block barrier in the K loop; production at
//      <=1 block/CU),
//  8 = variant 5 + XCD remap, 9 = variant 7 + XCD remap,
//  10 = variant 5 + timing skew, 11 = + kt rotation, 12 = skew + rotation,
//  13 = 256x256 @ 1 block/CU, persistent fragments, full double buffer,
//  14 = split-K of variant 5 (hw fp32 atomics into a zeroed C).
static const GemmVariant kFp8Variants[] = {
    {BM, BN, BK8, 256, launch_plain<char, mfma_gemm_fp8_128>, 0},
    {BM2, BN2, 2 * BK8, 512, launch_arg<char, mfma_gemm_fp8_256>, kXcdAuto},
    {BM, BN, BK8L, 256, launch_plain<char, mfma_gemm_fp8_128w>, 0},
    {BM, BN, 64, 256, launch_plain<char, mfma_gemm_fp8_128s>, 0},
    {BM, BN, BK8, 256, launch_plain<char, mfma_gemm_fp8_128t>, 0},
    {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 0},
    {256, BN, BK8, 512, launch_plain<char, mfma_gemm_fp8_256u>, 0},
    {BM, BN, BK8, 512, launch_arg<char, mfma_gemm_fp8_128pc>, 0},
    {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 1},
    {BM, BN, BK8, 512, launch_arg<char, mfma_gemm_fp8_128pc>, 1},
    {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 2},
    {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 4},
    {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 6},
    {256, 256, BK8, 512, launch_plain<char, mfma_gemm_fp8_256x>, 0},
    {BM, BN, BK8, 256, launch_splitk, 0},
};
enum { kFp8_128s = 3, kFp8_128u = 5, kFp8_128pc = 7 };

// working set (both operands + fp32 C) past the 256 MiB Infinity Cache:
// the XCD remap is enabled only then
static int past_infinity_cache(int M, int N, int K, int elem_bytes) {
  long ws = (long)elem_bytes * K * (M + N) + 4L * M * N;
  return ws > (256L << 20) ? 1 : 0;
}

static bool variant_fits(const GemmVariant& v, int M, int N, int K) {
  return M % v.tile_m == 0 && N % v.tile_n == 0 && K % v.k_mult == 0;
}

static long variant_blocks(const GemmVariant& v, int M, int N) {
  return (long)(N / v.tile_n) * (M / v.tile_m);
}

// Launch one table entry (no sync); -2 for a shape that does not fit.
static int launch_variant(const GemmVariant& v, const void* A, const void* Bt,
                          void* C, int M, int N, int K, int arg) {
  if (!variant_fits(v, M, N, K)) return -2;
  dim3 grid(N / v.tile_n, M / v.tile_m);
  return v.launch(grid, v.threads, A, Bt, C, M, N, K, arg);
}

// Forced variant: table lookup (unknown `which` -> entry 0), launch, sync.
static int run_forced_variant(const GemmVariant* table, int count,
                              int elem_bytes, int device, const void* A,
                              const void* Bt, void* C, int M, int N, int K,
                              int which) {
  if (hipSetDevice(device) != hipSuccess) return -3;
  const GemmVariant& v = table[which > 0 && which < count ? which : 0];
  int arg =
      v.arg == kXcdAuto ? past_infinity_cache(M, N, K, elem_bytes) : v.arg;
  int rc = launch_variant(v, A, Bt, C, M, N, K, arg);
  if (rc != 0) return rc;
  return (int)hipDeviceSynchronize();
}

// Launch the best-fitting bf16 MFMA GEMM variant (no sync).
static int launch_mfma_gemm(const void* A, const void* Bt, void* C, int M,
                            int N, int K) {
  const GemmVariant& v128 = kBf16Variants[kBf16_128];
  const GemmVariant& v256 = kBf16Variants[kBf16_256];
  // SMALL/MID sizes: the 128-tile step-3 kernel wins decisively below
  // ~2048² output — 407 vs 252 TF @2048³, 64 vs 51 @1024³
  // (profiles/final_kernel_sweep_r02.json): the deep 256-tile pipeline
  // cannot fill its phase schedule on a 64-block grid. Rule: take the
  // 128-tile shape whenever ITS grid still fits <=1 block/CU.
  if (variant_fits(v128, M, N, K) && variant_blocks(v128, M, N) <= 256)
    return launch_variant(v128, A, Bt, C, M, N, K, 0);
  if (variant_fits(v256, M, N, K)) {
    // enable the XCD remap only past the 256 MiB Infinity Cache
    int swz_on = past_infinity_cache(M, N, K, 2);
    // measured across boxes: the 32x32x16 shape wins at <=1 block/CU
    // grids (935 vs 848 TF @4096^3), the 16x16x32 shape past that
    // (1129 vs 1096 @8192^3) — profiles/gemm_final_sweep_2026-09-13.json
    if (variant_blocks(v256, M, N) <= 256)
      return launch_variant(kBf16Variants[kBf16_256w], A, Bt, C, M, N, K,
                            swz_on);
    return launch_variant(v256, A, Bt, C, M, N, K, swz_on);
  }
  return launch_variant(v128, A, Bt, C, M, N, K, 0);
}

// Best-fitting fp8 launch (no sync). Measured dispatch policy:
// - <=256 blocks (<=1 block/CU): producer/consumer wave split (stage
//   windows fully exposed there; +16% measured, fp8_ab_1/boundary);
// - past 1 block/CU: the single-buffered 4-blocks/CU barrier shape
//   (occupancy wins; 2125 vs 1811 @8k).
// Split-K for tiny grids was built and MEASURED OUT (fp8_sk.json:
// 50.7 vs 111.5 TF @1024 — sub-2048 sizes are launch-latency bound,
// not occupancy bound; the C memset + atomic RMW are pure overhead).
// K%64-only shapes fall back to the BK=64 4-blocks/CU kernel.
static int launch_fp8_best(const void* A, const void* Bt, void* C, int M,
                           int N, int K) {
  const GemmVariant& pc = kFp8Variants[kFp8_128pc];
  if (variant_fits(pc, M, N, K)) {
    int swz_on = past_infinity_cache(M, N, K, 1);
    if (variant_blocks(pc, M, N) <= 256)
      return launch_variant(pc, A, Bt, C, M, N, K, swz_on);
    return launch_variant(kFp8Variants[kFp8_128u], A, Bt, C, M, N, K, swz_on);
  }
  return launch_variant(kFp8Variants[kFp8_128s], A, Bt, C, M, N, K, 0);
}

// ===========================================================================
// Persistent per-device probe context. The CC manager is a long-lived
// daemon that attests after every transition: allocations, events and
// the liveness scratch word are cached so steady-state probes pay only
// kernel time (first call measured ~225 ms of hipMalloc/teardown
// overhead at dim=1024; with the cached context AND the cached fp32
// reference below, the warm probe is ~0.4 ms).
// ===========================================================================
constexpr int kMaxDevices = 64;

struct ProbeCtx {
  int dim = 0;
  int ref_valid = 0;  // the fp32 reference of the deterministic fill
  bf16 *dA = nullptr, *dB = nullptr;
  unsigned char *dA8 = nullptr, *dB8 = nullptr;
  float *dC = nullptr, *dRef = nullptr, *dHbm = nullptr, *dErr = nullptr;
  unsigned long long* dSum = nullptr;
  uint32_t* dFail = nullptr;
  int* dLive = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // lazily allocated when THIS device is the target of another
  // device's xGMI peer-traffic leg (destination buffer + checksum word)
  float* dPeerDst = nullptr;
  long peer_cap = 0;  // bytes
  unsigned long long* dPeerSum = nullptr;
  // round-robin cursor when CC_ATTEST_XGMI_MAX_PEERS bounds the
  // per-probe link sample (full 7-link coverage amortized over
  // consecutive probes instead of per probe)
  int peer_cursor = 0;
  // MXFP4 leg (cc_attest_mxfp4): lazily allocated like the peer
  // buffers, so the default probe's context holds nothing of it
  int mx_dim = 0;
  int mx_ref_valid = 0;
  unsigned char *dMxA = nullptr, *dMxB = nullptr;    // packed fp4
  unsigned char *dMxSA = nullptr, *dMxSB = nullptr;  // e8m0
  float *dMxC = nullptr, *dMxRef = nullptr, *dMxErr = nullptr;
  unsigned long long* dMxSum = nullptr;
  // compute-unit sweep (cc_cu_sweep): lazily allocated too. hSweepTab
  // is the host copy of the unit table after the last sweep.
  unsigned* dSweepTab = nullptr;
  float* dSweepGold = nullptr;
  int sweep_gold_rounds = 0;  // rounds dSweepGold was computed for
  unsigned* hSweepTab = nullptr;
  int sweep_valid = 0;  // hSweepTab holds a finished sweep
};

static ProbeCtx g_ctx[kMaxDevices];
static std::mutex g_ctx_mu;

// The context's device buffers, in allocation order. bytes == 0: not
// allocated by ctx_acquire (the peer-leg and MXFP4 buffers are lazy).
struct CtxBuffer {
  void** ptr;
  size_t bytes;
};

static std::array<CtxBuffer, 23> ctx_buffers(ProbeCtx& c, long elems) {
  return {{
      {(void**)&c.dA, elems * sizeof(bf16)},
      {(void**)&c.dB, elems * sizeof(bf16)},
      {(void**)&c.dA8, (size_t)elems},
      {(void**)&c.dB8, (size_t)elems},
      {(void**)&c.dC, elems * sizeof(float)},
      {(void**)&c.dRef, elems * sizeof(float)},
      {(void**)&c.dHbm, elems * sizeof(float)},
      {(void**)&c.dErr, sizeof(float)},
      {(void**)&c.dSum, sizeof(unsigned long long)},
      {(void**)&c.dFail, sizeof(uint32_t)},
      {(void**)&c.dLive, sizeof(int)},
      {(void**)&c.dPeerDst, 0},
      {(void**)&c.dPeerSum, 0},
      {(void**)&c.dMxA, 0},
      {(void**)&c.dMxB, 0},
      {(void**)&c.dMxSA, 0},
      {(void**)&c.dMxSB, 0},
      {(void**)&c.dMxC, 0},
      {(void**)&c.dMxRef, 0},
      {(void**)&c.dMxErr, 0},
      {(void**)&c.dMxSum, 0},
      {(void**)&c.dSweepTab, 0},
      {(void**)&c.dSweepGold, 0},
  }};
}

static void ctx_release(ProbeCtx& c) {
  for (const CtxBuffer& b : ctx_buffers(c, 0))
    if (*b.ptr) (void)hipFree(*b.ptr);
  free(c.hSweepTab);
  if (c.ev0) (void)hipEventDestroy(c.ev0);
  if (c.ev1) (void)hipEventDestroy(c.ev1);
  c = ProbeCtx{};
}

static hipError_t ctx_acquire(int device, int dim, ProbeCtx** out) {
  ProbeCtx& c = g_ctx[device];
  if (c.dim == dim) {
    *out = &c;
    return hipSuccess;
  }
  ctx_release(c);
  hipError_t e;
  for (const CtxBuffer& b : ctx_buffers(c, (long)dim * dim))
    if (b.bytes && (e = hipMalloc(b.ptr, b.bytes)) != hipSuccess) return e;
  if ((e = hipEventCreate(&c.ev0)) != hipSuccess) return e;
  if ((e = hipEventCreate(&c.ev1)) != hipSuccess) return e;
  c.dim = dim;
  *out = &c;
  return hipSuccess;
}

extern "C" {

struct CcAttestReport {
  int device;
  int cu_count;
  int xcc_count;
  char arch[64];
  char error[256];
  long long vram_total_mb;
  // GEMM probe
  int gemm_m, gemm_n, gemm_k;
  double gemm_ms;
  double gemm_tflops;
  double ref_ms;
  float max_abs_err;       // MFMA vs VALU fp32 (must be 0.0: exact inputs)
  unsigned long long checksum;
  // fp8 (MX-scaled e4m3) MFMA path, same integer data
  double fp8_ms;
  double fp8_tflops;
  float fp8_max_abs_err;   // vs the same fp32 VALU reference (0.0)
  // LDS probe
  double lds_ms;
  unsigned int lds_failures;
  // HBM probe
  double hbm_ms;
  double hbm_gbps;
  // fabric
  int peer_count;          // devices visible
  int peers_accessible;    // peers with canAccessPeer==1
  int peers_attempted;     // links sampled THIS probe (env-bounded)
  // xGMI peer-traffic leg (runs only when peers_accessible > 0): a
  // timed SDMA copy of the result buffer across every accessible link
  // plus a checksum recomputed ON THE PEER — link integrity, not just
  // visibility (round-1 verdict, weak #6)
  int peers_verified;      // peers whose copied data checksummed equal
  double xgmi_ms;          // total copy time, all links
  double xgmi_gbps_min;    // slowest single link
  double xgmi_gbps_max;    // fastest single link
  int ok;
};

// Report of the opt-in MXFP4 probe (cc_attest_mxfp4); CcAttestReport
// stays as it is.
struct CcMxReport {
  int device;
  int mx_m, mx_n, mx_k;
  double mx_ms;
  double mx_tflops;
  double mx_ref_ms;       // 0.0 when the cached reference was used
  float mx_max_abs_err;   // MFMA vs VALU reference (must be 0.0)
  unsigned long long mx_checksum;
  int ok;
  char error[256];
};

// Report of the opt-in compute-unit sweep (cc_cu_sweep). A unit is one
// SIMD of one CU, named by the 14-bit key of cu_sweep.hip.
struct CcSweepReport {
  int device, cu_count, units_expected, units_seen, cus_seen, xccs_seen;
  int units_failed;
  unsigned mfma_failures, lds_failures;
  int launches, rounds;
  double sweep_ms;           // device events, all launches
  double gold_ms;            // 0.0 when cached
  unsigned failed_keys[16];  // first 16
  int ok;
  char error[256];
};

}  // extern "C"

// The MXFP4 leg's buffers for dimension D, on top of whatever context
// the device has (none is needed: the events are created here if the
// main probe has not run yet).
static hipError_t mx_acquire(int device, int D, ProbeCtx** out) {
  ProbeCtx& c = g_ctx[device];
  *out = &c;
  hipError_t e;
  if (!c.ev0 && (e = hipEventCreate(&c.ev0)) != hipSuccess) return e;
  if (!c.ev1 && (e = hipEventCreate(&c.ev1)) != hipSuccess) return e;
  if (c.mx_dim == D) return hipSuccess;
  const size_t elems = (size_t)D * D;
  const CtxBuffer bufs[] = {
      {(void**)&c.dMxA, elems / 2},
      {(void**)&c.dMxB, elems / 2},
      {(void**)&c.dMxSA, elems / 32},
      {(void**)&c.dMxSB, elems / 32},
      {(void**)&c.dMxC, elems * sizeof(float)},
      {(void**)&c.dMxRef, elems * sizeof(float)},
      {(void**)&c.dMxErr, sizeof(float)},
      {(void**)&c.dMxSum, sizeof(unsigned long long)},
  };
  c.mx_dim = 0;
  c.mx_ref_valid = 0;
  for (const CtxBuffer& b : bufs) {
    if (*b.ptr) (void)hipFree(*b.ptr);
    *b.ptr = nullptr;
    if ((e = hipMalloc(b.ptr, b.bytes)) != hipSuccess) return e;
  }
  c.mx_dim = D;
  return hipSuccess;
}

// Launch the MXFP4 MFMA GEMM (no sync); -2 for a shape that does not
// fit the 128x128x256 tile or operands that are not 16-byte aligned
// (the tile DMA moves 16 B per lane, the scale loads 8 B).
static int launch_mxfp4(const void* A, const void* SA, const void* Bt,
                        const void* SB, void* C, int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK4) return -2;
  if ((((uintptr_t)A | (uintptr_t)Bt | (uintptr_t)SA | (uintptr_t)SB |
        (uintptr_t)C) & 15) != 0)
    return -2;
  hipLaunchKernelGGL(mfma_gemm_mxfp4_128u, dim3(N / BN, M / BM), dim3(256), 0,
                     0, (const char*)A, (const unsigned char*)SA,
                     (const char*)Bt, (const unsigned char*)SB, (float*)C, M,
                     N, K);
  return 0;
}

static void launch_ref_mxfp4(const void* A, const void* SA, const void* Bt,
                             const void* SB, void* C, int M, int N, int K) {
  dim3 block(16, 16), grid((N + 15) / 16, (M + 15) / 16);
  hipLaunchKernelGGL(ref_gemm_mxfp4_f32, grid, block, 0, 0,
                     (const unsigned char*)A, (const unsigned char*)SA,
                     (const unsigned char*)Bt, (const unsigned char*)SB,
                     (float*)C, M, N, K);
}

// ===========================================================================
// Probe legs. Each takes the context and the report and returns 0, a
// HIP error (text in rep->error) or a negative probe status.
// ===========================================================================

// record, launch, record, sync: the launch's time on the null stream.
// `launch` returns 0 or a status that aborts the leg.
template <typename Report, typename Launch>
static int timed_ms(ProbeCtx* ctx, Report* rep, double* ms, Launch launch) {
  hipEvent_t ev0 = ctx->ev0, ev1 = ctx->ev1;
  CC_CHECK(hipEventRecord(ev0, 0));
  CC_TRY(launch());
  CC_CHECK(hipEventRecord(ev1, 0));
  CC_CHECK(hipEventSynchronize(ev1));
  float f = 0.f;
  (void)hipEventElapsedTime(&f, ev0, ev1);
  *ms = (double)f;
  return 0;
}

// copy one device word back, bit for bit
template <typename T>
static hipError_t read_back(const void* dptr, T* out) {
  return hipMemcpy(out, dptr, sizeof(T), hipMemcpyDeviceToHost);
}

static int probe_bf16(ProbeCtx* ctx, CcAttestReport* rep) {
  const int D = ctx->dim;
  const long elems = (long)D * D;
  bf16 *dA = ctx->dA, *dB = ctx->dB;
  float *dC = ctx->dC, *dRef = ctx->dRef, *dErr = ctx->dErr;
  unsigned long long* dSum = ctx->dSum;
  CC_CHECK(hipMemset(dErr, 0, sizeof(float)));
  CC_CHECK(hipMemset(dSum, 0, sizeof(unsigned long long)));

  // -- fill (asymmetric seeds: catches row/col-swapped layouts) --------
  hipLaunchKernelGGL(fill_bf16_lcg, dim3(2048), dim3(256), 0, 0, dA, elems, 1u);
  hipLaunchKernelGGL(fill_bf16_lcg, dim3(2048), dim3(256), 0, 0, dB, elems, 7u);

  // -- MFMA GEMM (timed; warm once; best-fitting variant) --------------
  launch_mfma_gemm(dA, dB, dC, D, D, D);
  CC_CHECK(hipDeviceSynchronize());
  CC_TRY(timed_ms(ctx, rep, &rep->gemm_ms, [&] {
    launch_mfma_gemm(dA, dB, dC, D, D, D);
    return 0;
  }));
  rep->gemm_tflops = 2.0 * D * (double)D * D / (rep->gemm_ms * 1e-3) / 1e12;

  // -- VALU reference + compare ---------------------------------------
  // The fill is deterministic per dim, so the fp32 reference is a
  // constant: computed once per context (the dominant probe cost —
  // ~1.9 ms of a 2.4 ms warm probe at dim 1024 — disappears from the
  // steady-state transition path).
  if (!ctx->ref_valid) {
    CC_TRY(timed_ms(ctx, rep, &rep->ref_ms, [&] {
      dim3 rblock(16, 16), rgrid((D + 15) / 16, (D + 15) / 16);
      hipLaunchKernelGGL(ref_gemm_f32, rgrid, rblock, 0, 0, dA, dB, dRef, D, D,
                         D);
      return 0;
    }));
    ctx->ref_valid = 1;
  } else {
    rep->ref_ms = 0.0;  // cached
  }

  hipLaunchKernelGGL(max_abs_diff, dim3(1024), dim3(256), 0, 0, dC, dRef,
                     elems, dErr);
  hipLaunchKernelGGL(checksum_f32, dim3(1024), dim3(256), 0, 0, dC, elems, dSum);
  CC_CHECK(hipDeviceSynchronize());
  CC_CHECK(read_back(dErr, &rep->max_abs_err));
  CC_CHECK(read_back(dSum, &rep->checksum));
  return 0;
}

// fp8 (MX-scaled) MFMA path: same integer values, same fp32 reference,
// bitwise requirement; the PRODUCTION fp8 dispatch
static int probe_fp8(ProbeCtx* ctx, CcAttestReport* rep) {
  const int D = ctx->dim;
  const long elems = (long)D * D;
  float *dC = ctx->dC, *dErr = ctx->dErr;
  hipLaunchKernelGGL(fill_fp8_lcg, dim3(2048), dim3(256), 0, 0, ctx->dA8,
                     elems, 1u);
  hipLaunchKernelGGL(fill_fp8_lcg, dim3(2048), dim3(256), 0, 0, ctx->dB8,
                     elems, 7u);
  if (launch_fp8_best(ctx->dA8, ctx->dB8, dC, D, D, D) != 0) return -6;
  CC_CHECK(hipDeviceSynchronize());
  CC_TRY(timed_ms(ctx, rep, &rep->fp8_ms, [&] {
    return launch_fp8_best(ctx->dA8, ctx->dB8, dC, D, D, D) != 0 ? -6 : 0;
  }));
  rep->fp8_tflops = 2.0 * D * (double)D * D / (rep->fp8_ms * 1e-3) / 1e12;
  CC_CHECK(hipMemset(dErr, 0, sizeof(float)));
  hipLaunchKernelGGL(max_abs_diff, dim3(1024), dim3(256), 0, 0, dC, ctx->dRef,
                     elems, dErr);
  CC_CHECK(hipDeviceSynchronize());
  CC_CHECK(read_back(dErr, &rep->fp8_max_abs_err));
  return 0;
}

static int probe_lds(ProbeCtx* ctx, CcAttestReport* rep) {
  uint32_t* dFail = ctx->dFail;
  CC_CHECK(hipMemset(dFail, 0, sizeof(uint32_t)));
  CC_TRY(timed_ms(ctx, rep, &rep->lds_ms, [&] {
    hipLaunchKernelGGL(lds_probe, dim3(512), dim3(256), 0, 0, dFail, 8);
    return 0;
  }));
  CC_CHECK(read_back(dFail, &rep->lds_failures));
  return 0;
}

// HBM probe (dedicated dst: dRef is a cached constant)
static int probe_hbm(ProbeCtx* ctx, CcAttestReport* rep) {
  long n4 = (long)ctx->dim * ctx->dim / 4;
  CC_TRY(timed_ms(ctx, rep, &rep->hbm_ms, [&] {
    hipLaunchKernelGGL(hbm_copy_f4, dim3(4096), dim3(256), 0, 0,
                       (const float4v*)ctx->dC, (float4v*)ctx->dHbm, n4);
    return 0;
  }));
  rep->hbm_gbps = 2.0 * n4 * 16.0 / (rep->hbm_ms * 1e-3) / 1e9;
  return 0;
}

// The xGMI leg hops to the peer device and back; any early return while
// away must leave the calling thread on its own device again.
struct DeviceHop {
  int home;
  bool away = false;
  explicit DeviceHop(int device) : home(device) {}
  hipError_t to(int peer) {
    away = true;
    return hipSetDevice(peer);
  }
  hipError_t back() {
    hipError_t e = hipSetDevice(home);
    away = e != hipSuccess;
    return e;
  }
  ~DeviceHop() {
    if (away) (void)hipSetDevice(home);
  }
};

// xGMI peer visibility + traffic. Visibility alone attests nothing
// about link integrity: for every accessible peer, move the live result
// buffer across the link (SDMA over xGMI) and recompute its checksum ON
// THE PEER. Per-link bandwidth is reported (xGMI is point-to-point,
// 7 links x ~153 GB/s per GPU — each link is individually bound).
static int probe_xgmi(ProbeCtx* ctx, CcAttestReport* rep) {
  const int device = rep->device;
  float* dC = ctx->dC;
  unsigned long long* dSum = ctx->dSum;
  int ndev = 0;
  CC_CHECK(hipGetDeviceCount(&ndev));
  rep->peer_count = ndev - 1;
  if (ndev > kMaxDevices) ndev = kMaxDevices;
  // Bounded per-link sample (2 MiB x 2 copies): on an 8-GPU hive the
  // probe runs per device per transition and touches 7 links — an
  // unbounded sample would dominate the transition step. 4 MiB per
  // link is still real SDMA traffic with an on-peer checksum.
  long bytes = (long)ctx->dim * ctx->dim * sizeof(float);
  if (bytes > (2L << 20)) bytes = 2L << 20;
  long sum_elems = bytes / sizeof(float);
  // fresh source checksum over the sampled slice: dC now holds the
  // fp8 result (the bf16-era rep->checksum no longer matches)
  CC_CHECK(hipMemset(dSum, 0, sizeof(unsigned long long)));
  hipLaunchKernelGGL(checksum_f32, dim3(1024), dim3(256), 0, 0, dC, sum_elems,
                     dSum);
  CC_CHECK(hipDeviceSynchronize());
  unsigned long long src_sum = 0;
  CC_CHECK(read_back(dSum, &src_sum));
  // accessible peer list first; CC_ATTEST_XGMI_MAX_PEERS (0 = all)
  // bounds how many links one probe samples — the scaling bench sets
  // it so per-transition cost stays O(1) while the round-robin cursor
  // still covers every link across consecutive probes
  int acc[kMaxDevices];
  int n_acc = 0;
  for (int p = 0; p < ndev; ++p) {
    if (p == device) continue;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, device, p) == hipSuccess && can)
      acc[n_acc++] = p;
  }
  rep->peers_accessible = n_acc;
  int max_peers = 0;
  if (const char* mp = getenv("CC_ATTEST_XGMI_MAX_PEERS")) max_peers = atoi(mp);
  int attempts = (max_peers > 0 && max_peers < n_acc) ? max_peers : n_acc;
  rep->peers_attempted = attempts;
  DeviceHop hop(device);
  for (int t = 0; t < attempts; ++t) {
    int p = acc[(ctx->peer_cursor + t) % (n_acc ? n_acc : 1)];
    hipError_t pe = hipDeviceEnablePeerAccess(p, 0);
    if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) {
      (void)hipGetLastError();  // clear; copy may still route via SDMA
    }
    // destination + checksum word live on the peer (cached there)
    ProbeCtx& pc = g_ctx[p];
    CC_CHECK(hop.to(p));
    if (pc.peer_cap < bytes) {
      if (pc.dPeerDst) (void)hipFree(pc.dPeerDst);
      pc.dPeerDst = nullptr;
      pc.peer_cap = 0;
      if (hipMalloc(&pc.dPeerDst, bytes) != hipSuccess) {
        CC_CHECK(hop.back());
        continue;  // peer VRAM exhausted: counted accessible, not verified
      }
      pc.peer_cap = bytes;
    }
    if (!pc.dPeerSum &&
        hipMalloc(&pc.dPeerSum, sizeof(unsigned long long)) != hipSuccess) {
      CC_CHECK(hop.back());
      continue;
    }
    CC_CHECK(hipMemset(pc.dPeerDst, 0, bytes));
    CC_CHECK(hop.back());
    // timed link traffic: kPeerIters copies of the result buffer
    const int kPeerIters = 4;
    double ms = 0.0;
    CC_TRY(timed_ms(ctx, rep, &ms, [&] {
      for (int it = 0; it < kPeerIters; ++it)
        CC_CHECK(hipMemcpyPeerAsync(pc.dPeerDst, p, dC, device, bytes, 0));
      return 0;
    }));
    rep->xgmi_ms += ms;
    double gbps = (double)bytes * kPeerIters / (ms * 1e-3) / 1e9;
    if (rep->xgmi_gbps_min == 0.0 || gbps < rep->xgmi_gbps_min)
      rep->xgmi_gbps_min = gbps;
    if (gbps > rep->xgmi_gbps_max) rep->xgmi_gbps_max = gbps;
    // verify ON the peer: its own CUs must read back what crossed
    CC_CHECK(hop.to(p));
    CC_CHECK(hipMemset(pc.dPeerSum, 0, sizeof(unsigned long long)));
    // checksum the SAMPLED slice only (sum_elems) — the peer buffer
    // holds exactly `bytes`; summing all of dC would read out of bounds
    hipLaunchKernelGGL(checksum_f32, dim3(1024), dim3(256), 0, 0, pc.dPeerDst,
                       sum_elems, pc.dPeerSum);
    CC_CHECK(hipDeviceSynchronize());
    unsigned long long peer_sum = 0;
    CC_CHECK(read_back(pc.dPeerSum, &peer_sum));
    CC_CHECK(hop.back());
    if (peer_sum == src_sum) ++rep->peers_verified;
  }
  if (n_acc) ctx->peer_cursor = (ctx->peer_cursor + attempts) % n_acc;
  return 0;
}

// MXFP4 leg: all 16 e2m1 codes and scale bytes {126,127,128} through
// the fp4 decoders and the block-scale hardware, bitwise against the
// VALU reference (exactness budget at fill_fp4_lcg).
static int probe_mxfp4(ProbeCtx* ctx, CcMxReport* rep) {
  const int D = ctx->mx_dim;
  const long elems = (long)D * D;
  float *dC = ctx->dMxC, *dErr = ctx->dMxErr;
  unsigned long long* dSum = ctx->dMxSum;
  CC_CHECK(hipMemset(dErr, 0, sizeof(float)));
  CC_CHECK(hipMemset(dSum, 0, sizeof(unsigned long long)));
  // prefill with 0x7f7f7f7f (3.4e38, finite: max_abs_diff's fmaxf would
  // drop a NaN): an output the kernel never wrote shows as a huge error
  CC_CHECK(hipMemset(dC, 0x7F, elems * sizeof(float)));

  hipLaunchKernelGGL(fill_fp4_lcg, dim3(2048), dim3(256), 0, 0, ctx->dMxA,
                     elems / 2, 1u);
  hipLaunchKernelGGL(fill_fp4_lcg, dim3(2048), dim3(256), 0, 0, ctx->dMxB,
                     elems / 2, 7u);
  hipLaunchKernelGGL(fill_e8m0_lcg, dim3(256), dim3(256), 0, 0, ctx->dMxSA,
                     elems / 32, 1u);
  hipLaunchKernelGGL(fill_e8m0_lcg, dim3(256), dim3(256), 0, 0, ctx->dMxSB,
                     elems / 32, 7u);

  auto launch = [&] {
    return launch_mxfp4(ctx->dMxA, ctx->dMxSA, ctx->dMxB, ctx->dMxSB, dC, D, D,
                        D) != 0
               ? -6
               : 0;
  };
  CC_TRY(launch());
  CC_CHECK(hipDeviceSynchronize());
  CC_TRY(timed_ms(ctx, rep, &rep->mx_ms, launch));
  rep->mx_tflops = 2.0 * D * (double)D * D / (rep->mx_ms * 1e-3) / 1e12;

  // deterministic fill: the reference is a constant per dim
  if (!ctx->mx_ref_valid) {
    CC_TRY(timed_ms(ctx, rep, &rep->mx_ref_ms, [&] {
      launch_ref_mxfp4(ctx->dMxA, ctx->dMxSA, ctx->dMxB, ctx->dMxSB,
                       ctx->dMxRef, D, D, D);
      return 0;
    }));
    ctx->mx_ref_valid = 1;
  } else {
    rep->mx_ref_ms = 0.0;  // cached
  }

  hipLaunchKernelGGL(max_abs_diff, dim3(1024), dim3(256), 0, 0, dC,
                     ctx->dMxRef, elems, dErr);
  hipLaunchKernelGGL(checksum_f32, dim3(1024), dim3(256), 0, 0, dC, elems,
                     dSum);
  CC_CHECK(hipDeviceSynchronize());
  CC_CHECK(read_back(dErr, &rep->mx_max_abs_err));
  CC_CHECK(read_back(dSum, &rep->mx_checksum));
  return 0;
}

// The sweep's buffers, on top of whatever context the device has (as
// mx_acquire).
static hipError_t sweep_acquire(int device, ProbeCtx** out) {
  ProbeCtx& c = g_ctx[device];
  *out = &c;
  hipError_t e;
  if (!c.ev0 && (e = hipEventCreate(&c.ev0)) != hipSuccess) return e;
  if (!c.ev1 && (e = hipEventCreate(&c.ev1)) != hipSuccess) return e;
  const size_t tab_b = (size_t)CU_SWEEP_UNITS * CU_SWEEP_REC * sizeof(unsigned);
  if (!c.dSweepTab && (e = hipMalloc(&c.dSweepTab, tab_b)) != hipSuccess)
    return e;
  if (!c.dSweepGold &&
      (e = hipMalloc(&c.dSweepGold, CU_SWEEP_GOLD_ELEMS * sizeof(float))) !=
          hipSuccess)
    return e;
  if (!c.hSweepTab && !(c.hSweepTab = (unsigned*)calloc(1, tab_b)))
    return hipErrorOutOfMemory;
  return hipSuccess;
}

// The golden C images for `rounds`, a constant: computed once per
// (device, rounds). *ms = 0.0 when the cached images were used.
static int sweep_gold(ProbeCtx* ctx, CcSweepReport* rep, int rounds,
                      double* ms) {
  *ms = 0.0;
  if (ctx->sweep_gold_rounds == rounds) return 0;
  ctx->sweep_gold_rounds = 0;
  CC_TRY(timed_ms(ctx, rep, ms, [&] {
    hipLaunchKernelGGL(cu_sweep_gold, dim3(1), dim3(1024), 0, 0,
                       ctx->dSweepGold, rounds);
    return 0;
  }));
  CC_CHECK(hipGetLastError());
  ctx->sweep_gold_rounds = rounds;
  return 0;
}

static int sweep_units_seen(const unsigned* tab) {
  int n = 0;
  for (int k = 0; k < CU_SWEEP_UNITS; ++k) n += tab[k * CU_SWEEP_REC] != 0;
  return n;
}

// Sweep leg: up to 4 launches of 4 blocks per CU into one unit table,
// until every SIMD of every CU has reported.
static int probe_cu_sweep(ProbeCtx* ctx, CcSweepReport* rep, int poison_key) {
  const size_t tab_b = (size_t)CU_SWEEP_UNITS * CU_SWEEP_REC * sizeof(unsigned);
  unsigned* tab = ctx->hSweepTab;
  CC_TRY(sweep_gold(ctx, rep, rep->rounds, &rep->gold_ms));
  ctx->sweep_valid = 0;
  CC_CHECK(hipMemset(ctx->dSweepTab, 0, tab_b));
  const int kMaxLaunches = 4;
  for (int l = 0; l < kMaxLaunches; ++l) {
    double ms = 0.0;
    CC_TRY(timed_ms(ctx, rep, &ms, [&] {
      hipLaunchKernelGGL(cu_sweep, dim3(4 * rep->cu_count), dim3(1024), 0, 0,
                         ctx->dSweepGold, ctx->dSweepTab, rep->rounds,
                         poison_key);
      return 0;
    }));
    CC_CHECK(hipGetLastError());
    rep->sweep_ms += ms;
    rep->launches = l + 1;
    CC_CHECK(hipMemcpy(tab, ctx->dSweepTab, tab_b, hipMemcpyDeviceToHost));
    if (sweep_units_seen(tab) >= rep->units_expected) break;
  }
  ctx->sweep_valid = 1;

  unsigned long long xccs = 0;
  int last_cu = -1;  // keys ascend, a CU's four SIMDs are adjacent
  for (int k = 0; k < CU_SWEEP_UNITS; ++k) {
    const unsigned* rec = tab + k * CU_SWEEP_REC;
    if (!rec[0]) continue;
    ++rep->units_seen;
    if ((k >> 2) != last_cu) ++rep->cus_seen;
    last_cu = k >> 2;
    xccs |= 1ull << (k >> 10);
    rep->mfma_failures += rec[1];
    rep->lds_failures += rec[2];
    if (rec[1] || rec[2]) {
      if (rep->units_failed < 16) rep->failed_keys[rep->units_failed] = k;
      ++rep->units_failed;
    }
  }
  rep->xccs_seen = __builtin_popcountll(xccs);
  return 0;
}

// ===========================================================================
// C API
// ===========================================================================
extern "C" {

int cc_device_alive(int device) {
  if (device < 0 || device >= kMaxDevices) return -1;
  if (hipSetDevice(device) != hipSuccess) return -1;
  int* d = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    ProbeCtx& c = g_ctx[device];
    if (!c.dLive && hipMalloc(&c.dLive, sizeof(int)) != hipSuccess) return -2;
    d = c.dLive;
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
// indexes kBf16Variants, anything else runs variant 0.
int cc_mfma_gemm_bf16_variant(int device, const void* A, const void* Bt,
                              void* C, int M, int N, int K, int which) {
  return run_forced_variant(kBf16Variants, 4, 2, device, A, Bt, C, M, N, K,
                            which);
}

// Force a specific fp8 variant (perf characterization / A-B); `which`
// indexes kFp8Variants (0-14), anything else runs variant 0.
int cc_mfma_gemm_fp8_variant(int device, const void* A, const void* Bt,
                             void* C, int M, int N, int K, int which) {
  return run_forced_variant(kFp8Variants, 15, 1, device, A, Bt, C, M, N, K,
                            which);
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
  if (!rep) return -1;
  __builtin_memset(rep, 0, sizeof(*rep));
  rep->device = device;
  CC_CHECK(hipSetDevice(device));

  hipDeviceProp_t prop;
  CC_CHECK(hipGetDeviceProperties(&prop, device));
  rep->cu_count = prop.multiProcessorCount;
  rep->vram_total_mb = (long long)(prop.totalGlobalMem >> 20);
  __builtin_strncpy(rep->arch, prop.gcnArchName, sizeof(rep->arch) - 1);

  const int D = (gemm_dim / BM) * BM > 0 ? (gemm_dim / BM) * BM : BM;
  rep->gemm_m = rep->gemm_n = rep->gemm_k = D;

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  if (device < 0 || device >= kMaxDevices) return -5;
  ProbeCtx* ctx = nullptr;
  CC_CHECK(ctx_acquire(device, D, &ctx));

  CC_TRY(probe_bf16(ctx, rep));
  CC_TRY(probe_fp8(ctx, rep));
  CC_TRY(probe_lds(ctx, rep));
  CC_TRY(probe_hbm(ctx, rep));
  CC_TRY(probe_xgmi(ctx, rep));

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
  if (!rep) return -1;
  __builtin_memset(rep, 0, sizeof(*rep));
  rep->device = device;
  if (device < 0 || device >= kMaxDevices) return -5;
  CC_CHECK(hipSetDevice(device));

  const int D = gemm_dim < BK4 ? BK4 : (gemm_dim / BK4) * BK4;
  rep->mx_m = rep->mx_n = rep->mx_k = D;

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  ProbeCtx* ctx = nullptr;
  CC_CHECK(mx_acquire(device, D, &ctx));
  CC_TRY(probe_mxfp4(ctx, rep));

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
  if (!rep) return -1;
  __builtin_memset(rep, 0, sizeof(*rep));
  rep->device = device;
  rep->rounds = rounds;
  if (device < 0 || device >= kMaxDevices) return -5;
  if (rounds < 1 || rounds > CU_SWEEP_MAX_ROUNDS) {
    snprintf(rep->error, sizeof(rep->error), "rounds %d outside 1..%d", rounds,
             CU_SWEEP_MAX_ROUNDS);
    return -2;
  }
  CC_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  CC_CHECK(hipGetDeviceProperties(&prop, device));
  rep->cu_count = prop.multiProcessorCount;
  rep->units_expected = 4 * rep->cu_count;

  std::lock_guard<std::mutex> lk(g_ctx_mu);
  ProbeCtx* ctx = nullptr;
  CC_CHECK(sweep_acquire(device, &ctx));
  CC_TRY(probe_cu_sweep(ctx, rep, poison_key));

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
  ProbeCtx* ctx = nullptr;
  if (sweep_acquire(device, &ctx) != hipSuccess) return -4;
  CcSweepReport scratch;
  double ms = 0.0;
  CC_TRY(sweep_gold(ctx, &scratch, rounds, &ms));
  return (int)hipMemcpy(host_out_3328, ctx->dSweepGold,
                        CU_SWEEP_GOLD_ELEMS * sizeof(float),
                        hipMemcpyDeviceToHost);
}

// Keys of the units the last sweep on `device` reached, ascending, at
// most `cap` of them written; returns how many there are (0 before the
// first sweep).
int cc_cu_sweep_units(int device, unsigned* keys_out, int cap) {
  if (device < 0 || device >= kMaxDevices) return -5;
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  const ProbeCtx& c = g_ctx[device];
  if (!c.sweep_valid) return 0;
  int n = 0;
  for (int k = 0; k < CU_SWEEP_UNITS; ++k) {
    if (!c.hSweepTab[k * CU_SWEEP_REC]) continue;
    if (keys_out && n < cap) keys_out[n] = (unsigned)k;
    ++n;
  }
  return n;
}

// How many waves reported from each of those units, in the same order.
int cc_cu_sweep_hits(int device, unsigned* hits_out, int cap) {
  if (device < 0 || device >= kMaxDevices) return -5;
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  const ProbeCtx& c = g_ctx[device];
  if (!c.sweep_valid) return 0;
  int n = 0;
  for (int k = 0; k < CU_SWEEP_UNITS; ++k) {
    unsigned hits = c.hSweepTab[k * CU_SWEEP_REC];
    if (!hits) continue;
    if (hits_out && n < cap) hits_out[n] = hits;
    ++n;
  }
  return n;
}

// ABI guard for CcSweepReport, as cc_report_sizeof for CcAttestReport.
int cc_sweep_report_sizeof(void) { return (int)sizeof(struct CcSweepReport); }

// Free every cached probe context (daemon shutdown / tests).
void cc_attest_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  for (int i = 0; i < kMaxDevices; ++i) {
    if (g_ctx[i].dim || g_ctx[i].dLive || g_ctx[i].mx_dim || g_ctx[i].ev0) {
      (void)hipSetDevice(i);
      ctx_release(g_ctx[i]);
    }
  }
}

}  // extern "C"
