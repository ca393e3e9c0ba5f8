// Host side of the GEMM kernels: the named variants, launchers and the
// production dispatch policies. Included by attest_kernels.hip after the
// device files.

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

constexpr int kXcdAuto = -1;  // arg: XCD remap iff past_infinity_cache()

struct GemmVariant {
  int tile_m, tile_n;  // block tile; M and N must be multiples
  int k_mult;          // K must be a multiple
  int threads;
  GemmLauncher launch;
  int arg;  // what a forced run passes; production dispatch passes its own
};

// The kernels production dispatch launches, by name.
// bf16: 128x128 step-3, 256x256 8-phase (16x16 op), 256x256 8-phase
// (32x32 op).
static const GemmVariant kBf16_128 = {
    BM, BN, BK, 256, launch_plain<bf16, mfma_gemm_bf16>, 0};
static const GemmVariant kBf16_256 = {
    BM2, BN2, 2 * BK2, 512, launch_arg<bf16, mfma_gemm_bf16_256>, kXcdAuto};
static const GemmVariant kBf16_256w = {
    BM2, BN2, 2 * BK2, 512, launch_arg<bf16, mfma_gemm_bf16_256w>, kXcdAuto};

// fp8 (measured ladder in BASELINE.md): BK=64 32x32-op (4 blocks/CU;
// production's K%64-only fall-back), BK=128 SINGLE-buffered (4
// blocks/CU; production past 1 block/CU), producer/consumer wave split
// (4 stage waves + 4 MFMA waves, LDS-flag handoff, no block barrier in
// the K loop; production at <=1 block/CU).
static const GemmVariant kFp8_128s = {
    BM, BN, 64, 256, launch_plain<char, mfma_gemm_fp8_128s>, 0};
static const GemmVariant kFp8_128u = {
    BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 0};
static const GemmVariant kFp8_128pc = {
    BM, BN, BK8, 512, launch_arg<char, mfma_gemm_fp8_128pc>, 0};

// The `which` numbers of the cc_*_variant entry points. BASELINE.md and
// profiles/ name kernels by them, so they keep their values; a number
// that is not listed (fp8 0, 1, 2, 4, 6 and 14 were kernels that have
// been measured out and removed) names nothing.
struct ForcedVariant {
  int which;
  GemmVariant v;
};

// 3 = 128x128 single-buffered 4-blocks/CU (measured slower than the deep
// pipeline — the recorded negative arm of the occupancy series,
// BASELINE.md).
static const ForcedVariant kBf16Forced[] = {
    {0, kBf16_128},
    {1, kBf16_256},
    {2, kBf16_256w},
    {3, {BM, BN, 64, 256, launch_plain<bf16, mfma_gemm_bf16_128u>, 0}},
};

//  8 = variant 5 + XCD remap, 9 = variant 7 + XCD remap (production takes
//      that branch only past a 256 MiB working set, so these are how a
//      small test reaches it),
//  10 = variant 5 + timing skew, 11 = + kt rotation, 12 = skew + rotation,
//  13 = 256x256 @ 1 block/CU, persistent fragments, full double buffer.
static const ForcedVariant kFp8Forced[] = {
    {3, kFp8_128s},
    {5, kFp8_128u},
    {7, kFp8_128pc},
    {8, {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 1}},
    {9, {BM, BN, BK8, 512, launch_arg<char, mfma_gemm_fp8_128pc>, 1}},
    {10, {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 2}},
    {11, {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 4}},
    {12, {BM, BN, BK8, 256, launch_arg<char, mfma_gemm_fp8_128u>, 6}},
    {13, {256, 256, BK8, 512, launch_plain<char, mfma_gemm_fp8_256x>, 0}},
};

// The variant `which` names, or null.
template <int N>
static const GemmVariant* forced_variant(const ForcedVariant (&list)[N],
                                         int which) {
  for (const ForcedVariant& f : list)
    if (f.which == which) return &f.v;
  return nullptr;
}

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

// Launch one variant (no sync); -2 for a shape that does not fit.
static int launch_variant(const GemmVariant& v, const void* A, const void* Bt,
                          void* C, int M, int N, int K, int arg) {
  if (!variant_fits(v, M, N, K)) return -2;
  dim3 grid(N / v.tile_n, M / v.tile_m);
  return v.launch(grid, v.threads, A, Bt, C, M, N, K, arg);
}

// Forced variant: launch, sync. A null `v` (a `which` that names no
// kernel) is -2 before the device is touched.
static int run_forced_variant(const GemmVariant* v, int elem_bytes, int device,
                              const void* A, const void* Bt, void* C, int M,
                              int N, int K) {
  if (!v) return -2;
  if (hipSetDevice(device) != hipSuccess) return -3;
  int arg =
      v->arg == kXcdAuto ? past_infinity_cache(M, N, K, elem_bytes) : v->arg;
  int rc = launch_variant(*v, A, Bt, C, M, N, K, arg);
  if (rc != 0) return rc;
  return (int)hipDeviceSynchronize();
}

// Launch the best-fitting bf16 MFMA GEMM variant (no sync).
static int launch_mfma_gemm(const void* A, const void* Bt, void* C, int M,
                            int N, int K) {
  const GemmVariant& v128 = kBf16_128;
  const GemmVariant& v256 = kBf16_256;
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
      return launch_variant(kBf16_256w, A, Bt, C, M, N, K, swz_on);
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
  const GemmVariant& pc = kFp8_128pc;
  if (variant_fits(pc, M, N, K)) {
    int swz_on = past_infinity_cache(M, N, K, 1);
    if (variant_blocks(pc, M, N) <= 256)
      return launch_variant(pc, A, Bt, C, M, N, K, swz_on);
    return launch_variant(kFp8_128u, A, Bt, C, M, N, K, swz_on);
  }
  return launch_variant(kFp8_128s, A, Bt, C, M, N, K, 0);
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
