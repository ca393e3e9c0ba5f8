// FP16 MFMA GEMM: C[M,N] (fp32) = A[M,K] (IEEE binary16) . Bt[N,K]^T
// (binary16), row-major, two bytes per element. The only kernel of the
// project that issues an f16 MFMA, in both shapes:
//   SHAPE 0   v_mfma_f32_32x32x16_f16   (16 accumulator registers)
//   SHAPE 1   v_mfma_f32_16x16x32_f16   (4 accumulator registers)
// binary16 has its own operand decoder (5-bit exponent, 10-bit mantissa,
// subnormals) and an 11x11-bit significand multiplier that no bf16, fp8
// or MX kernel reaches. Inf and NaN codes are out of scope: nothing here
// or in the leg produces or compares them.
//
// Exactness (the leg's fill, fill_f16_exact in probe_kernels.hip): an
// element is (j/4) * 2^e(row), |j| <= 31, e in -22..13. Inside one C
// element all terms share the factor 2^(e(m)+f(n)); before it a term is a
// multiple of 2^-4 of at most 961/16, so every partial sum fits 24 bits in
// any order while K * 961 < 2^24 (K <= 16384), and e + f >= -44 keeps
// every term and sum normal in fp32: MFMA and VALU must agree bitwise.
// For other data the kernel rounds like any fp32 accumulate.
//
// Outer shape: mfma_gemm_i8_128's (gemm_i8.hip; docs/KERNELS.md, finding
// 4), byte for byte: 128x128 block, 256 threads, a wave owns 64x64, BK =
// 64 elements = 128-byte rows, one single-buffered 32 KiB LDS image pair,
// 4 blocks/CU, operands by global_load_lds through
// stage_lds<swz8, 4, 7, true>, a barrier on both sides of the compute.
//
// Between LDS and the matrix core: an f16 MFMA operand is 16 bytes per
// lane (8 halves), half of the 32-byte fragment the swz8 image keeps
// contiguous. Both shapes read whole fragments (load_frag32, one
// contiguous 8-register tuple) and feed the low and the high 16 bytes to
// two MFMAs on the same accumulator. A and B are split the same way, so
// which k lands in which instruction does not matter for the sum's terms.
//
// SHAPE 0: lane (row l&31, half h = l>>5) reads swz8(row*128 + ks*64 +
//   h*32). 2 k-steps x 2x2 accumulators x 2 MFMAs per K-tile; two A
//   fragments and one B fragment live at a time.
// SHAPE 1: the wave's 64x64 is 4x4 accumulators of 16x16. Lane (row l&15,
//   group g = l>>4) reads swz8(row*128 + g*32): the four groups cover the
//   128-byte K-tile of a 16-row set in one read. 4x4 accumulators x 2
//   MFMAs per K-tile, no k-step loop; four A fragments (32 registers) stay
//   for the tile, B fragments come one column set at a time.
// The addresses are mfma_gemm_i8_128's, so the 2-way swz8 bank behaviour
// enumerated in docs/KERNELS.md, "INT8 leg", carries over unchanged.
//
// The operand row maps (l&31 / l&15, 8 consecutive k per lane part: those
// of the bf16 ops of the same shape) and the C/D maps (the f32 ones,
// store_acc_32x32 / store_acc_16x16) are pinned on both operand sides by
// test_decode_all_codes in tests/test_gpu_fp16.py. The MFMAs are builtins,
// not inline asm: the compiler sees the accumulator dependency, no
// mfma_drain() is needed.
#pragma once

#include <type_traits>

#include "gemm_common.hip"

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) int f16_regs;  // 8 halves

// the 16-byte halves of a 32-byte fragment as MFMA operands
__device__ __forceinline__ f16x8 f16_lo(const v8i& f) {
  return __builtin_bit_cast(f16x8,
                            (f16_regs)__builtin_shufflevector(f, f, 0, 1, 2, 3));
}
__device__ __forceinline__ f16x8 f16_hi(const v8i& f) {
  return __builtin_bit_cast(f16x8,
                            (f16_regs)__builtin_shufflevector(f, f, 4, 5, 6, 7));
}

// One K-tile of a wave's 64x64 sub-tile, SHAPE 0: 2 k-steps x (2x2) x 2
// MFMAs. a_off / b_off: the lane's logical image offsets at ks = 0.
__device__ __forceinline__ void mma_64x64_f16_32(const char* As, const char* Bs,
                                                 const int (&a_off)[2],
                                                 const int (&b_off)[2],
                                                 f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    v8i afrag[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
      afrag[i] = load_frag32(As + swz8(a_off[i] + ks * 64));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const v8i bfrag = load_frag32(Bs + swz8(b_off[j] + ks * 64));
      // low halves of both row sets first: the two MFMAs of one
      // accumulator are two instructions apart
#pragma unroll
      for (int i = 0; i < 2; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
            f16_lo(afrag[i]), f16_lo(bfrag), acc[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(
            f16_hi(afrag[i]), f16_hi(bfrag), acc[i][j], 0, 0, 0);
    }
  }
}

// One K-tile of a wave's 64x64 sub-tile, SHAPE 1: (4x4) x 2 MFMAs, the
// four A fragments loaded first and kept, one B fragment at a time. The
// low halves of a column set go out before the high halves, so the two
// MFMAs of one accumulator are four instructions apart.
__device__ __forceinline__ void mma_64x64_f16_16(const char* As, const char* Bs,
                                                 const int (&a_off)[4],
                                                 const int (&b_off)[4],
                                                 f32x4 (&acc)[4][4]) {
  v8i afrag[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) afrag[i] = load_frag32(As + swz8(a_off[i]));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const v8i bfrag = load_frag32(Bs + swz8(b_off[j]));
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
          f16_lo(afrag[i]), f16_lo(bfrag), acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
          f16_hi(afrag[i]), f16_hi(bfrag), acc[i][j], 0, 0, 0);
  }
}

template <int SHAPE>
__global__ __launch_bounds__(256, 4) void mfma_gemm_f16_128(
    const _Float16* __restrict__ A, const _Float16* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K) {
  static_assert(SHAPE == 0 || SHAPE == 1, "32x32x16 or 16x16x32");
  __shared__ char lds[2 * 16384];  // [A][B], single-buffered

  const TileCoords t = tile_coords<BM, BN, 2>(A, Bt, K, blockIdx.y, blockIdx.x);
  const int lane = t.lane;

  // tiles per wave side and rows per tile: 2 of 32, or 4 of 16
  constexpr int T = SHAPE == 0 ? 2 : 4;
  constexpr int R = 64 / T;
  const int frow = lane & (R - 1);
  const int fcol = (lane / R) * 32;  // h*32 or g*32, bytes

  // this lane's fragments in the images (logical byte offsets)
  int a_off[T], b_off[T];
#pragma unroll
  for (int i = 0; i < T; ++i) {
    a_off[i] = (t.wave_m + i * R + frow) * 128 + fcol;
    b_off[i] = (t.wave_n + i * R + frow) * 128 + fcol;
  }

  typename std::conditional<SHAPE == 0, f32x16, f32x4>::type acc[T][T] = {};

  char* As = &lds[0];
  char* Bs = &lds[16384];
  const int nk = K / BK;
  for (int kt = 0; kt < nk; ++kt) {
    stage_lds<swz8, 4, 7, true>(t.gA, t.row_b, (long)kt * 128, 0, As, t.wave,
                                lane);
    stage_lds<swz8, 4, 7, true>(t.gB, t.row_b, (long)kt * 128, 0, Bs, t.wave,
                                lane);
    __syncthreads();
    if constexpr (SHAPE == 0)
      mma_64x64_f16_32(As, Bs, a_off, b_off, acc);
    else
      mma_64x64_f16_16(As, Bs, a_off, b_off, acc);
    __syncthreads();
  }

  // C/D lane terms: col = l & (R-1); 32x32: row += 4*(l>>5), 16x16: 4*(l>>4)
  const int c_col = frow;
  const int c_row = (lane / R) * 4;
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int row0 = t.block_m + t.wave_m + i * R;
      const int col0 = t.block_n + t.wave_n + j * R;
      if constexpr (SHAPE == 0)
        store_acc_32x32(C, N, row0, col0, acc[i][j], c_row, c_col);
      else
        store_acc_16x16(C, N, row0, col0, acc[i][j], c_row, c_col);
    }
}
