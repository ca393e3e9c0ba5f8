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

// What the GEMM and reference entry points do on caller-provided buffers:
// set the device (-3), `launch` (no sync; nonzero: refused, returned as it
// is), then the synchronise's status.
template <typename Launch>
static int run_synced(int device, Launch launch) {
  if (hipSetDevice(device) != hipSuccess) return -3;
  int rc = launch();
  if (rc != 0) return rc;
  return (int)hipDeviceSynchronize();
}

// Forced variant: launch, sync. A null `v` (a `which` that names no
// kernel) is -2 before the device is touched.
static int run_forced_variant(const GemmVariant* v, int elem_bytes, int device,
                              const void* A, const void* Bt, void* C, int M,
                              int N, int K) {
  if (!v) return -2;
  int arg =
      v->arg == kXcdAuto ? past_infinity_cache(M, N, K, elem_bytes) : v->arg;
  return run_synced(
      device, [&] { return launch_variant(*v, A, Bt, C, M, N, K, arg); });
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

// Launch the MXFP6 MFMA GEMM (no sync); fmt 2 = e2m3, 3 = e3m2. -2 for
// any other fmt, a shape that does not fit the 128x128x128 tile or
// operands that are not 16-byte aligned.
static int launch_mxfp6(int fmt, const void* A, const void* SA, const void* Bt,
                        const void* SB, void* C, int M, int N, int K) {
  if (fmt != 2 && fmt != 3) return -2;
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK6) return -2;
  if ((((uintptr_t)A | (uintptr_t)Bt | (uintptr_t)SA | (uintptr_t)SB |
        (uintptr_t)C) & 15) != 0)
    return -2;
  auto kernel = fmt == 2 ? mfma_gemm_mxfp6_128<2> : mfma_gemm_mxfp6_128<3>;
  hipLaunchKernelGGL(kernel, dim3(N / BN, M / BM), dim3(256), 0, 0,
                     (const char*)A, (const unsigned char*)SA, (const char*)Bt,
                     (const unsigned char*)SB, (float*)C, M, N, K);
  return 0;
}

static void launch_ref_mxfp6(int fmt, const void* A, const void* SA,
                             const void* Bt, const void* SB, void* C, int M,
                             int N, int K) {
  dim3 block(16, 16), grid((N + 15) / 16, (M + 15) / 16);
  auto kernel = fmt == 2 ? ref_gemm_mxfp6_f32<2> : ref_gemm_mxfp6_f32<3>;
  hipLaunchKernelGGL(kernel, grid, block, 0, 0, (const uint32_t*)A,
                     (const unsigned char*)SA, (const uint32_t*)Bt,
                     (const unsigned char*)SB, (float*)C, M, N, K);
}

// Launch the MXFP8 MFMA GEMM (no sync); fa / fb 0 = e4m3, 1 = e5m2,
// chosen independently. -2 for any other format, a shape that does not
// fit the 128x128x128 tile or operands that are not 16-byte aligned.
static int launch_mxfp8(int fa, int fb, const void* A, const void* SA,
                        const void* Bt, const void* SB, void* C, int M, int N,
                        int K) {
  if ((fa != 0 && fa != 1) || (fb != 0 && fb != 1)) return -2;
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK8) return -2;
  if ((((uintptr_t)A | (uintptr_t)Bt | (uintptr_t)SA | (uintptr_t)SB |
        (uintptr_t)C) & 15) != 0)
    return -2;
  auto kernel = fa == 0 ? (fb == 0 ? mfma_gemm_mxfp8_128<0, 0>
                                   : mfma_gemm_mxfp8_128<0, 1>)
                        : (fb == 0 ? mfma_gemm_mxfp8_128<1, 0>
                                   : mfma_gemm_mxfp8_128<1, 1>);
  hipLaunchKernelGGL(kernel, dim3(N / BN, M / BM), dim3(256), 0, 0,
                     (const char*)A, (const unsigned char*)SA, (const char*)Bt,
                     (const unsigned char*)SB, (float*)C, M, N, K);
  return 0;
}

static void launch_ref_mxfp8(int fa, int fb, const void* A, const void* SA,
                             const void* Bt, const void* SB, void* C, int M,
                             int N, int K) {
  dim3 block(16, 16), grid((N + 15) / 16, (M + 15) / 16);
  auto kernel = fa == 0 ? (fb == 0 ? ref_gemm_mxfp8_f32<0, 0>
                                   : ref_gemm_mxfp8_f32<0, 1>)
                        : (fb == 0 ? ref_gemm_mxfp8_f32<1, 0>
                                   : ref_gemm_mxfp8_f32<1, 1>);
  hipLaunchKernelGGL(kernel, grid, block, 0, 0, (const unsigned char*)A,
                     (const unsigned char*)SA, (const unsigned char*)Bt,
                     (const unsigned char*)SB, (float*)C, M, N, K);
}

// Largest K of the INT8 GEMM: the largest multiple of 128 with
// K * 2^14 <= 2^31 - 1 (|a * b| <= 2^14), so no sum can leave 32 bits and
// the instruction's overflow behaviour never comes into play.
constexpr int kI8MaxK = 130944;

// Launch the INT8 MFMA GEMM (no sync); shape 0 = the 32x32x32 op, 1 = the
// 16x16x64 op. -2 for any other shape, M, N or K that does not fit the
// 128x128x128 tile, K above kI8MaxK or operands that are not 16-byte
// aligned.
static int launch_i8(int shape, const void* A, const void* Bt, void* C, int M,
                     int N, int K) {
  if (shape != 0 && shape != 1) return -2;
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK8) return -2;
  if (K > kI8MaxK) return -2;
  if ((((uintptr_t)A | (uintptr_t)Bt | (uintptr_t)C) & 15) != 0) return -2;
  auto kernel = shape == 0 ? mfma_gemm_i8_128<0> : mfma_gemm_i8_128<1>;
  hipLaunchKernelGGL(kernel, dim3(N / BN, M / BM), dim3(256), 0, 0,
                     (const char*)A, (const char*)Bt, (int*)C, M, N, K);
  return 0;
}

static void launch_ref_i8(const void* A, const void* Bt, void* C, int M, int N,
                          int K) {
  dim3 block(16, 16), grid((N + 15) / 16, (M + 15) / 16);
  hipLaunchKernelGGL(ref_gemm_i8_i32, grid, block, 0, 0, (const signed char*)A,
                     (const signed char*)Bt, (int*)C, M, N, K);
}

// Launch the FP64 MFMA GEMM (no sync). -2 for M or N that is no multiple
// of the 128 tile, K that is no multiple of the 16-double K-tile, or
// operands that are not 16-byte aligned. No K cap here: the GEMM rounds
// like any fp64 sum; the exactness cap belongs to the leg (kF64ExactDim).
static int launch_f64(const void* A, const void* Bt, void* C, int M, int N,
                      int K) {
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK64) return -2;
  if ((((uintptr_t)A | (uintptr_t)Bt | (uintptr_t)C) & 15) != 0) return -2;
  hipLaunchKernelGGL(mfma_gemm_f64_128, dim3(N / BN, M / BM), dim3(512), 0, 0,
                     (const double*)A, (const double*)Bt, (double*)C, M, N, K);
  return 0;
}

static void launch_ref_f64(const void* A, const void* Bt, void* C, int M,
                           int N, int K) {
  dim3 block(16, 16), grid((N + 15) / 16, (M + 15) / 16);
  hipLaunchKernelGGL(ref_gemm_f64, grid, block, 0, 0, (const double*)A,
                     (const double*)Bt, (double*)C, M, N, K);
}

// Largest dim of the FP64 leg: the fill's products are integers below 2^40,
// so while K * 2^40 <= 2^53 every partial sum is exact in any order.
constexpr int kF64ExactDim = 8192;

// Launch the 2:4 sparse bf16 GEMM (no sync); shape 0 = the 32x32x32
// SMFMAC, 1 = the 16x16x64 one, numbered as for launch_i8. -2 for any
// other shape, M, N or K (the dense K) that does not fit the 128x128x128
// tile, or operands that are not 16-byte aligned.
static int launch_sp24(int shape, const void* Ac, const void* Am,
                       const void* Bt, void* C, int M, int N, int K) {
  if (shape != 0 && shape != 1) return -2;
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BKS) return -2;
  if ((((uintptr_t)Ac | (uintptr_t)Am | (uintptr_t)Bt | (uintptr_t)C) & 15) != 0)
    return -2;
  auto kernel = shape == 0 ? mfma_gemm_sp24_128<0> : mfma_gemm_sp24_128<1>;
  hipLaunchKernelGGL(kernel, dim3(N / BN, M / BM), dim3(256), 0, 0,
                     (const char*)Ac, (const unsigned char*)Am,
                     (const char*)Bt, (float*)C, M, N, K);
  return 0;
}

static void launch_ref_sp24(const void* Ac, const void* Am, const void* Bt,
                            void* C, int M, int N, int K) {
  dim3 block(16, 16), grid((N + 15) / 16, (M + 15) / 16);
  hipLaunchKernelGGL(ref_gemm_sp24_f32, grid, block, 0, 0, (const bf16*)Ac,
                     (const unsigned char*)Am, (const bf16*)Bt, (float*)C, M,
                     N, K);
}

// Launch the FP16 MFMA GEMM (no sync); shape 0 = the 32x32x16 op, 1 = the
// 16x16x32 op. -2 for any other shape, M or N that is no multiple of the
// 128 tile, K that is no multiple of the 64-element K-tile, or operands
// that are not 16-byte aligned. No K cap here: the GEMM rounds like any
// fp32 accumulate; the exactness cap belongs to the leg (kF16ExactDim).
static int launch_mfma_gemm_f16(int shape, const void* A, const void* Bt,
                                void* C, int M, int N, int K) {
  if (shape != 0 && shape != 1) return -2;
  if (M <= 0 || N <= 0 || K <= 0 || M % BM || N % BN || K % BK) return -2;
  if ((((uintptr_t)A | (uintptr_t)Bt | (uintptr_t)C) & 15) != 0) return -2;
  auto kernel = shape == 0 ? mfma_gemm_f16_128<0> : mfma_gemm_f16_128<1>;
  hipLaunchKernelGGL(kernel, dim3(N / BN, M / BM), dim3(256), 0, 0,
                     (const _Float16*)A, (const _Float16*)Bt, (float*)C, M, N,
                     K);
  return 0;
}

static void launch_ref_gemm_f16_f32(const void* A, const void* Bt, void* C,
                                    int M, int N, int K) {
  dim3 block(16, 16), grid((N + 15) / 16, (M + 15) / 16);
  hipLaunchKernelGGL(ref_gemm_f16_f32, grid, block, 0, 0,
                     (const unsigned short*)A, (const unsigned short*)Bt,
                     (float*)C, M, N, K);
}

// Largest dim of the FP16 leg: before the row factors a term of the fill is
// a multiple of 2^-4 of at most 961/16, so while K * 961 < 2^24 every
// partial sum fits fp32's 24 bits in any order.
constexpr int kF16ExactDim = 16384;
