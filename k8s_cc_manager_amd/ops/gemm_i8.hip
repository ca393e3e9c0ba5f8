// INT8 MFMA GEMM: C[M,N] (int32) = A[M,K] (int8) . Bt[N,K]^T (int8),
// row-major, one signed byte per element, exact 32-bit integer sums. The
// only kernel of the project that issues an integer MFMA, in both shapes:
//   SHAPE 0   v_mfma_i32_32x32x32_i8   (16 accumulator registers)
//   SHAPE 1   v_mfma_i32_16x16x64_i8   (4 accumulator registers)
// Integer addition is exact in any order, so a k permutation that A and B
// share changes nothing, and the launcher caps K so that no sum can leave
// 32 bits (gemm_dispatch.hip): neither overflow nor saturation semantics
// of the instruction are ever relied on.
//
// Outer shape: mfma_gemm_fp8_128u's, for the same reason (docs/KERNELS.md,
// finding 4; same bytes per element): 128x128 block, 256 threads, a wave
// owns 64x64, BK = 128 bytes, one single-buffered 32 KiB LDS image pair,
// 4 blocks/CU, operands by global_load_lds through
// stage_lds<swz8, 4, 7, true>, a barrier on both sides of the compute.
//
// Between LDS and the matrix core: an i8 MFMA operand is 16 bytes per
// lane (4 registers), half of the 32-byte fragment the swz8 image keeps
// contiguous. Both shapes therefore read whole 32-byte fragments
// (load_frag32, one contiguous 8-register tuple) and feed the low and the
// high 16 bytes to two MFMAs on the same accumulator. A and B are split
// the same way, so which k lands in which instruction does not matter.
//
// SHAPE 0: lane (row l&31, half h = l>>5) reads swz8(row*128 + ks*64 +
//   h*32), exactly mfma_gemm_fp8_128u's addresses (its bank behaviour).
//   The instruction takes k = 16*h + byte from the lane, so MFMA q of
//   k-step ks covers the tile's bytes ks*64 + {q*16 .. q*16+15} and
//   ks*64 + 32 + {q*16 .. q*16+15}. 2 k-steps x 2x2 accumulators x 2
//   MFMAs per K-tile; two A fragments and one B fragment live at a time.
// SHAPE 1: the wave's 64x64 is 4x4 accumulators of 16x16. Lane (row l&15,
//   group g = l>>4) reads swz8(row*128 + g*32): the four groups together
//   cover the whole 128-byte K-tile of a 16-row set in ONE read, and MFMA
//   q (k = 16*g + byte from the lane) covers bytes g*32 + q*16 + byte for
//   all g: 64 k. 4x4 accumulators x 2 MFMAs per K-tile, no k-step loop;
//   four A fragments (32 registers) stay for the tile, B fragments come
//   one column set at a time. Bank behaviour under swz8: the same as
//   SHAPE 0's, enumerated in docs/KERNELS.md, "INT8 leg".
//
// The operand row maps (l&31 / l&15) and the C/D maps (those of the f32
// ops of the same shape) are pinned by the identity test in
// tests/test_gpu_int8.py. The MFMAs are builtins, not inline asm: the
// compiler sees the accumulator dependency, no mfma_drain() is needed.
#pragma once

#include "gemm_common.hip"

typedef __attribute__((ext_vector_type(4))) int v4i;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

__device__ __forceinline__ v4i frag_lo(const v8i& f) {
  return __builtin_shufflevector(f, f, 0, 1, 2, 3);
}
__device__ __forceinline__ v4i frag_hi(const v8i& f) {
  return __builtin_shufflevector(f, f, 4, 5, 6, 7);
}

// both 16-byte halves of a fragment pair into one accumulator
__device__ __forceinline__ void mfma_i8_pair(i32x16& acc, const v8i& a,
                                             const v8i& b) {
  acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(frag_lo(a), frag_lo(b), acc, 0,
                                              0, 0);
  acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(frag_hi(a), frag_hi(b), acc, 0,
                                              0, 0);
}

// int32 C/D store epilogues: the lane maps of store_acc_32x32 /
// store_acc_16x16 (gemm_common.hip), the lane terms the caller's as there.
__device__ __forceinline__ void store_acc_32x32_i32(
    int* C, int N, int row0, int col0, const i32x16& acc, int c_rowhi,
    int c_col32) {
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    int row = row0 + (reg & 3) + 8 * (reg >> 2) + c_rowhi;
    C[(long)row * N + col0 + c_col32] = acc[reg];
  }
}

__device__ __forceinline__ void store_acc_16x16_i32(
    int* C, int N, int row0, int col0, const i32x4& acc, int c_row0,
    int c_col) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    C[(long)(row0 + c_row0 + r) * N + col0 + c_col] = acc[r];
}

// One K-tile of a wave's 64x64 sub-tile, SHAPE 0: 2 k-steps x (2x2) x 2
// MFMAs. a_off / b_off: the lane's logical image offsets at ks = 0.
__device__ __forceinline__ void mma_64x64_i8_32(const char* As, const char* Bs,
                                                const int (&a_off)[2],
                                                const int (&b_off)[2],
                                                i32x16 (&acc)[2][2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    v8i afrag[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
      afrag[i] = load_frag32(As + swz8(a_off[i] + ks * 64));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const v8i bfrag = load_frag32(Bs + swz8(b_off[j] + ks * 64));
#pragma unroll
      for (int i = 0; i < 2; ++i) mfma_i8_pair(acc[i][j], afrag[i], bfrag);
    }
  }
}

// One K-tile of a wave's 64x64 sub-tile, SHAPE 1: (4x4) x 2 MFMAs, the
// four A fragments loaded first and kept, one B fragment at a time. The
// low halves of a column set go out before the high halves, so the two
// MFMAs of one accumulator are four instructions apart.
__device__ __forceinline__ void mma_64x64_i8_16(const char* As, const char* Bs,
                                                const int (&a_off)[4],
                                                const int (&b_off)[4],
                                                i32x4 (&acc)[4][4]) {
  v8i afrag[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) afrag[i] = load_frag32(As + swz8(a_off[i]));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const v8i bfrag = load_frag32(Bs + swz8(b_off[j]));
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
          frag_lo(afrag[i]), frag_lo(bfrag), acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
          frag_hi(afrag[i]), frag_hi(bfrag), acc[i][j], 0, 0, 0);
  }
}

template <int SHAPE>
__global__ __launch_bounds__(256, 4) void mfma_gemm_i8_128(
    const char* __restrict__ A, const char* __restrict__ Bt,
    int* __restrict__ C, int M, int N, int K) {
  static_assert(SHAPE == 0 || SHAPE == 1, "32x32x32 or 16x16x64");
  __shared__ char lds[2 * 16384];  // [A][B], single-buffered

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = (wave >> 1) * 64;
  const int wave_n = (wave & 1) * 64;
  const int block_m = blockIdx.y * BM;
  const int block_n = blockIdx.x * BN;

  const long row_b = (long)K;
  const char* gA = A + (long)block_m * K;
  const char* gB = Bt + (long)block_n * K;

  // tiles per wave side and rows per tile: 2 of 32, or 4 of 16
  constexpr int T = SHAPE == 0 ? 2 : 4;
  constexpr int R = 64 / T;
  const int frow = lane & (R - 1);
  const int fcol = (lane / R) * 32;  // h*32 or g*32

  // this lane's fragments in the images (logical offsets)
  int a_off[T], b_off[T];
#pragma unroll
  for (int i = 0; i < T; ++i) {
    a_off[i] = (wave_m + i * R + frow) * 128 + fcol;
    b_off[i] = (wave_n + i * R + frow) * 128 + fcol;
  }

  typename std::conditional<SHAPE == 0, i32x16, i32x4>::type acc[T][T] = {};

  char* As = &lds[0];
  char* Bs = &lds[16384];
  const int nk = K / BK8;
  for (int kt = 0; kt < nk; ++kt) {
    stage_lds<swz8, 4, 7, true>(gA, row_b, (long)kt * BK8, 0, As, wave, lane);
    stage_lds<swz8, 4, 7, true>(gB, row_b, (long)kt * BK8, 0, Bs, wave, lane);
    __syncthreads();
    if constexpr (SHAPE == 0)
      mma_64x64_i8_32(As, Bs, a_off, b_off, acc);
    else
      mma_64x64_i8_16(As, Bs, a_off, b_off, acc);
    __syncthreads();
  }

  // C/D lane terms: col = l & (R-1); 32x32: row += 4*(l>>5), 16x16: 4*(l>>4)
  const int c_col = frow;
  const int c_row = (lane / R) * 4;
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int row0 = block_m + wave_m + i * R;
      const int col0 = block_n + wave_n + j * R;
      if constexpr (SHAPE == 0)
        store_acc_32x32_i32(C, N, row0, col0, acc[i][j], c_row, c_col);
      else
        store_acc_16x16_i32(C, N, row0, col0, acc[i][j], c_row, c_col);
    }
}
