// MXFP6 (OCP e2m3 or e3m2 values, one E8M0 scale per 32 elements along
// K) MFMA GEMM: C[M,N] = sum over 32-element K blocks of
//   2^(SA[m,kb] + SB[n,kb] - 254) * sum_{k in kb} A[m,k] * Bt[n,k],
// fp32 out. A[M,K] and Bt[N,K] are row-major, 3K/4 bytes per row: every
// 32-element block is 24 bytes read as one little-endian 192-bit number,
// element j in bits 6j..6j+5. SA[M,K/32] and SB[N,K/32] are E8M0 bytes.
// FMT is the hardware's format selector for both operands: 2 = e2m3
// (cbsz:2 blgp:2), 3 = e3m2 (cbsz:3 blgp:3). These are the only kernels
// of the project that run the two 6-bit operand decoders.
//
// Skeleton: mfma_gemm_mxfp4_128u (128x128 block, 256 threads, a wave
// owns 64x64 as 2x2 accumulators of the 32x32x64 op, single-buffered,
// 4 blocks/CU). Everything between global memory and the operand
// registers is this file's own, because a 24-byte fragment fits none of
// the 128-byte-row images.
//
// Lane map, as the device confirmed (scripts/mx_layout_probe.hip, one
// wave, distinct scales on the two K blocks, a distinct random code at
// every k): lane l supplies 6 registers for row l&31; they hold the 32
// consecutive elements of K block l>>5 of the instruction's 64, i.e.
// that block's 24 bytes in memory order, and the scale byte the lane
// selects applies to those same 32 elements, for A and B alike. The
// e4m3 pattern (two runs of 16 elements, 12 bytes from each K block)
// was the other candidate and miscompared for both formats.
//
// K-tile: BK6 = 128 elements = 4 K blocks = 96 bytes per row, two
// k-steps. LDS image (per operand, 12416 bytes): row r starts at
// 96*r + 8*(r>>3): dense rows with one 8-byte pad after every 8 rows.
// In 8-byte units a fragment piece of row r sits at 12*r + (r>>3) + c;
// over the 32 rows of a half-wave 12*r mod 32 takes 8 values, each a
// multiple of 4, four times, and (r>>3) mod 4 tells those four apart: 32
// distinct bank pairs for every piece of every K block of both
// half-waves, so the three ds_read_b64 of a fragment are conflict-free
// (enumerated over all 4 row sets x 4 K blocks x 3 pieces). A dense
// image would put the 32 rows on 8 bank positions (4-way).
// Staging goes through registers, not the LDS DMA: thread t moves the
// 8-byte units t + 256*p, p = 0..5, of the tile (12 units per row, so a
// wave's global load is 512 contiguous bytes) and writes them with
// ds_write_b64. The pad changes every 96 units = three aligned groups of
// 32 lanes, so inside a group the 32 units are contiguous: the writes
// are conflict-free too. The 16-byte DMA cannot produce this image (a
// pad of 8 bytes splits chunks), and any DMA image leaves the 8-byte
// piece of a fragment 2-way conflicted: 32 lanes reading the same half
// of 32 different 16-byte chunks reach only half the banks.
//
// Measured (docs/KERNELS.md, "MXFP6 leg"): 0.92-1.04 PF/s at 4096^3 and
// 8192^3, about 0.6 of the production fp8 dispatch. This kernel attests
// the decoders; it is not yet a fast fp6 GEMM.
#pragma once

#include "gemm_common.hip"

typedef __attribute__((ext_vector_type(6))) int v6i;
typedef __attribute__((ext_vector_type(2))) int v2i;

constexpr int BK6 = 128;                      // fp6 elements per K-tile
constexpr int FP6_TILE_ROW_B = BK6 * 3 / 4;   // 96
constexpr int FP6_IMG_B = BM * FP6_TILE_ROW_B + (BM / 8) * 8;  // 12416

// where image row `row` starts
__device__ __forceinline__ int fp6_row_off(int row) {
  return row * FP6_TILE_ROW_B + (row >> 3) * 8;
}

// A fragment: 24 bytes at an 8-byte-aligned image offset.
__device__ __forceinline__ v6i load_frag24(const char* p) {
  v2i x = *(const v2i*)p;
  v2i y = *(const v2i*)(p + 8);
  v2i z = *(const v2i*)(p + 16);
  v6i f = {x[0], x[1], y[0], y[1], z[0], z[1]};
  return f;
}

// fp6 operands are 6-register tuples. HI picks byte 0 or byte 2 of both
// scale registers, as in MFMA_FP4W_ASM.
#define MFMA_FP6_ASM(FMTS, ACCX, AOP, BOP, SCA, SCB, HI)                      \
  asm volatile(                                                               \
      "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 "              \
      "op_sel:[0,0,0] op_sel_hi:[" HI "," HI ",0] cbsz:" FMTS " blgp:" FMTS   \
      : "+v"(ACCX)                                                            \
      : "v"(AOP), "v"(BOP), "v"(SCA), "v"(SCB))

// One k-step of a wave's 64x64 sub-tile: 2x2 32x32x64 MFMAs. K block
// 2*KS + (lane>>5) of the tile: 24 bytes at 48*KS + 24*(lane>>5) of the
// row (the lane term is in a_off/b_off).
#define MX6_KSTEP(KS, HI)                                                     \
  do {                                                                        \
    v6i afrag[2], bfrag[2];                                                   \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                           \
      afrag[i] = load_frag24(As + a_off[i] + (KS) * 48);                      \
      bfrag[i] = load_frag24(Bs + b_off[i] + (KS) * 48);                      \
    }                                                                         \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                             \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) {                       \
      if (FMT == 2)                                                           \
        MFMA_FP6_ASM("2", acc[i][j], afrag[i], bfrag[j], sa[i], sb[j], HI);   \
      else                                                                    \
        MFMA_FP6_ASM("3", acc[i][j], afrag[i], bfrag[j], sa[i], sb[j], HI);   \
    }                                                                         \
  } while (0)

template <int FMT>
__global__ __launch_bounds__(256, 4) void mfma_gemm_mxfp6_128(
    const char* __restrict__ A, const unsigned char* __restrict__ SA,
    const char* __restrict__ Bt, const unsigned char* __restrict__ SB,
    float* __restrict__ C, int M, int N, int K) {
  static_assert(FMT == 2 || FMT == 3, "e2m3 or e3m2");
  __shared__ __attribute__((aligned(16))) char lds[2 * FP6_IMG_B];  // [A][B]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = (wave >> 1) * 64;
  const int wave_n = (wave & 1) * 64;
  const int block_m = blockIdx.y * BM;
  const int block_n = blockIdx.x * BN;

  const unsigned row_b = (unsigned)(K >> 2) * 3u;  // operand row, bytes
  const char* gA = A + (long)block_m * row_b;
  const char* gB = Bt + (long)block_n * row_b;

  f32x16 acc[2][2] = {};
  const int lane31 = lane & 31;
  const int sc_shift = (lane >> 5) * 8;

  // this lane's fragment rows in the images, K-block term included
  int a_off[2], b_off[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a_off[i] = fp6_row_off(wave_m + i * 32 + lane31) + (lane >> 5) * 24;
    b_off[i] = fp6_row_off(wave_n + i * 32 + lane31) + (lane >> 5) * 24;
  }

  // scale rows as 32-bit offsets from the block's uniform base, as in
  // mfma_gemm_mxfp4_128u
  const unsigned srow_b = (unsigned)(K >> 5);
  const unsigned char* gSA = SA + (long)block_m * srow_b;
  const unsigned char* gSB = SB + (long)block_n * srow_b;
  const unsigned sa_off = (unsigned)(wave_m + lane31) * srow_b;
  const unsigned sb_off = (unsigned)(wave_n + lane31) * srow_b;

  char* As = &lds[0];
  char* Bs = &lds[FP6_IMG_B];
  const int nk = K / BK6;
  for (int kt = 0; kt < nk; ++kt) {
    // the 4 scale bytes of a row for this K-tile, shifted right by
    // 8*(lane>>5): K block 2*ks + (lane>>5) then sits at byte 2*ks for
    // every lane. They go out ahead of the tile loads.
    int sa[2], sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned step = (unsigned)i * 32u * srow_b + (unsigned)kt * 4u;
      sa[i] = (int)(*(const unsigned*)(gSA + (sa_off + step)) >> sc_shift);
      sb[i] = (int)(*(const unsigned*)(gSB + (sb_off + step)) >> sc_shift);
    }
    // stage both tiles through registers: 8-byte unit u of the tile is
    // bytes 8*(u%12).. of row u/12
    v2i ra[6], rb[6];
    const unsigned k0_b = (unsigned)kt * FP6_TILE_ROW_B;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int u = tid + 256 * p;
      const int row = u / 12;
      const unsigned g = (unsigned)row * row_b + k0_b + (unsigned)(u - row * 12) * 8u;
      ra[p] = *(const v2i*)(gA + g);
      rb[p] = *(const v2i*)(gB + g);
    }
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int u = tid + 256 * p;
      const int l = u * 8 + ((u / 12) >> 3) * 8;
      *(v2i*)(As + l) = ra[p];
      *(v2i*)(Bs + l) = rb[p];
    }
    __syncthreads();
    MX6_KSTEP(0, "0");
    MX6_KSTEP(1, "1");
    __syncthreads();
  }
  mfma_drain();

  const int c_col32 = lane & 31;
  const int c_rowhi = (lane >> 5) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      store_acc_32x32(C, N, block_m + wave_m + i * 32,
                      block_n + wave_n + j * 32, acc[i][j], c_rowhi, c_col32);
}

#undef MX6_KSTEP
