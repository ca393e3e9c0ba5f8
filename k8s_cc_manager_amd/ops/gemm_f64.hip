// FP64 MFMA GEMM: C[M,N] (fp64) = A[M,K] (fp64) . Bt[N,K]^T (fp64),
// row-major. The only kernel of the project that issues a double-precision
// matrix op, v_mfma_f64_16x16x4_f64 (through the compiler's builtin): the
// fp64 matrix core is a datapath of its own (53-bit multiplier, 11-bit
// exponents, accumulators in register pairs) that no other leg reaches.
// M and N multiples of 128, K a multiple of 16, 16-byte aligned pointers
// (launch_f64 in gemm_dispatch.hip refuses anything else).
//
// LDS image: a K-tile of 16 doubles is a 128-byte row, so a 128-row
// operand tile is the 16 KiB image of the fp8 and int8 kernels, staged by
// global_load_lds through stage_lds<swz8, 2, 7, true>, single-buffered,
// a barrier on both sides of the compute. A 128x128x16 tile is 16 FLOP per
// staged byte at a matrix rate more than ten times below bf16's, and with
// 2 blocks/CU one block's stage window lies under the other's MFMAs.
//
// Between LDS and the matrix core: the op takes ONE double of A and one
// of B per lane, lane l holding row l&15 at k = l>>4 (4 k per
// instruction). Lane (row l&15, group g = l>>4) reads the 32-byte
// fragment at swz8(row*128 + g*32) with load_frag32: doubles 4g..4g+3 of
// the K-tile, the addressing (and the bank behaviour) of the INT8 kernel's
// SHAPE 1. The four groups cover the whole K-tile of a 16-row set in one
// read, and MFMA q (0..3) takes double q of the A and of the B fragment:
// it sums k = {q, 4+q, 8+q, 12+q}. A and B are split alike, so every
// instruction sees a consistent k set.
//
// Wave tiling, this kernel's own: an accumulator is 4 doubles = 8 VGPRs,
// so the 64x64 per wave of the other 128-tile kernels would be 128 VGPRs
// of accumulator alone. Here 512 threads = eight waves in a 4x2 grid, each
// owning 32x64 of C: 2x4 accumulators in 64 VGPRs, both A fragments (16
// VGPRs) kept for the K-tile, B fragments one column set at a time. That
// fits 128 VGPRs: 4 waves/SIMD, 2 blocks/CU (docs/KERNELS.md, "FP64 leg",
// has the resource report). Per K-tile a wave reads 6 fragments and
// issues 32 MFMAs; the two accumulators of a column set alternate, so
// dependent MFMAs are never adjacent.
//
// C/D map: NOT the f32 16x16 one. Register r of lane l is column l&15,
// row 4*r + (l>>4) (the f32 op: row 4*(l>>4) + r). store_acc_16x16_f64
// below; the operand maps and this one are pinned by the identity test in
// tests/test_gpu_fp64.py.
#pragma once

#include "gemm_common.hip"

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int BK64 = 16;  // doubles per K-tile (128 B rows)

// fp64 C/D store epilogue of the 16x16x4 op: col = lane & 15,
// row = 4*r + (lane >> 4). The lane terms are the caller's, as for the
// epilogues of gemm_common.hip: c_rowlo = lane >> 4, c_col = lane & 15.
__device__ __forceinline__ void store_acc_16x16_f64(
    double* C, int N, int row0, int col0, const f64x4& acc, int c_rowlo,
    int c_col) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    C[(long)(row0 + 4 * r + c_rowlo) * N + col0 + c_col] = acc[r];
}

__device__ __forceinline__ f64x4 load_frag_f64(const char* p) {
  return __builtin_bit_cast(f64x4, load_frag32(p));
}

// One K-tile of a wave's 32x64 sub-tile: (2x4) accumulators x 4 MFMAs.
// a_off / b_off: the lane's logical image offsets.
__device__ __forceinline__ void mma_32x64_f64(const char* As, const char* Bs,
                                              const int (&a_off)[2],
                                              const int (&b_off)[4],
                                              f64x4 (&acc)[2][4]) {
  f64x4 afrag[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) afrag[i] = load_frag_f64(As + swz8(a_off[i]));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f64x4 bfrag = load_frag_f64(Bs + swz8(b_off[j]));
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(
            afrag[i][q], bfrag[q], acc[i][j], 0, 0, 0);
  }
}

// second launch-bound argument: waves per SIMD (2 blocks of 8 waves per CU)
__global__ __launch_bounds__(512, 4) void mfma_gemm_f64_128(
    const double* __restrict__ A, const double* __restrict__ Bt,
    double* __restrict__ C, int M, int N, int K) {
  __shared__ char lds[2 * 16384];  // [A][B], single-buffered

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = (wave >> 1) * 32;
  const int wave_n = (wave & 1) * 64;
  const int block_m = blockIdx.y * BM;
  const int block_n = blockIdx.x * BN;

  const long row_b = (long)K * sizeof(double);
  const char* gA = (const char*)A + (long)block_m * row_b;
  const char* gB = (const char*)Bt + (long)block_n * row_b;

  const int frow = lane & 15;
  const int fgrp = lane >> 4;

  // this lane's fragments in the images (logical offsets)
  int a_off[2], b_off[4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    a_off[i] = (wave_m + i * 16 + frow) * 128 + fgrp * 32;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    b_off[j] = (wave_n + j * 16 + frow) * 128 + fgrp * 32;

  f64x4 acc[2][4] = {};

  char* As = &lds[0];
  char* Bs = &lds[16384];
  const int nk = K / BK64;
  for (int kt = 0; kt < nk; ++kt) {
    stage_lds<swz8, 2, 7, true>(gA, row_b, (long)kt * 128, 0, As, wave, lane);
    stage_lds<swz8, 2, 7, true>(gB, row_b, (long)kt * 128, 0, Bs, wave, lane);
    __syncthreads();
    mma_32x64_f64(As, Bs, a_off, b_off, acc);
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      store_acc_16x16_f64(C, N, block_m + wave_m + i * 16,
                          block_n + wave_n + j * 16, acc[i][j], fgrp, frow);
}
