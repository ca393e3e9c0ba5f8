// MXFP4 (OCP e2m1 values, one E8M0 scale per 32 elements along K) MFMA
// GEMM: C[M,N] = sum over 32-element K blocks of
//   2^(SA[m,kb] + SB[n,kb] - 254) * sum_{k in kb} A[m,k] * Bt[n,k],
// fp32 out. A[M,K] and Bt[N,K] are packed two fp4 per byte (low nibble =
// even k), row-major, K/2 bytes per row; SA[M,K/32] and SB[N,K/32] are
// E8M0 bytes, row-major. This is the only kernel of the project that
// runs the fp4 operand decoder (cbsz:4 blgp:4) and the block-scale
// hardware with scales other than 1.0.
//
// Structure: mfma_gemm_fp8_128u with the operand format changed. A
// 128-B image row holds 256 fp4, so BK4 = 256 and the 16 KiB swz8
// images and their staging are the fp8 kernel's. 32x32x64 op: lane l
// carries 32 fp4 = 16 B (one ds_read_b128) of row l&31 at K block
// 2*ks + (l>>5) of the K-tile, image offset row*128 + ks*32 +
// (l>>5)*16. swz8 relocates 32-B units, so the 16-B fragment moves
// whole.
// Scale map: the scale VGPR byte that a lane selects applies to that
// lane's own 32 elements (row l&31, K block l>>5 of the instruction),
// for A and B alike; the byte index is op_sel (bit 0) and op_sel_hi
// (bit 1), element 0 of the list for A and element 1 for B.
#pragma once

#include "gemm_common.hip"

typedef __attribute__((ext_vector_type(4))) int v4i;

constexpr int BK4 = 256;  // fp4 elements per K-tile (128 B rows)

// fp4 operands are 4-register tuples (the assembler rejects 8-register
// tuples at cbsz/blgp 4). HI picks byte 0 or byte 2 of both scale
// registers.
#define MFMA_FP4W_ASM(ACCX, AOP, BOP, SCA, SCB, HI)                           \
  asm volatile(                                                               \
      "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 "              \
      "op_sel:[0,0,0] op_sel_hi:[" HI "," HI ",0] cbsz:4 blgp:4"              \
      : "+v"(ACCX)                                                            \
      : "v"(AOP), "v"(BOP), "v"(SCA), "v"(SCB))

// The 8 scale bytes of one row for one K-tile, shifted right by
// 8*(lane>>5) so that the byte of K block 2*ks + (lane>>5) sits at byte
// 2*(ks&1) of dword ks>>1 for every lane: the MFMA's immediate byte
// select then depends on ks alone.
struct MxScale {
  int d[2];
};

__device__ __forceinline__ MxScale load_mx_scale(const unsigned char* p,
                                                 int shift) {
  unsigned long long v = *(const unsigned long long*)p >> shift;
  MxScale s;
  s.d[0] = (int)(unsigned)v;
  s.d[1] = (int)(unsigned)(v >> 32);
  return s;
}

// One ks step of a wave's 64x64 sub-tile: 2x2 32x32x64 MFMAs.
#define MX_KSTEP(KS, HI)                                                      \
  do {                                                                        \
    v4i afrag[2], bfrag[2];                                                   \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                           \
      int la = (wave_m + i * 32 + lane31) * 128 + (KS) * 32 + kq_b;           \
      int lb = (wave_n + i * 32 + lane31) * 128 + (KS) * 32 + kq_b;           \
      afrag[i] = *(const v4i*)(As + swz8(la));                                \
      bfrag[i] = *(const v4i*)(Bs + swz8(lb));                                \
    }                                                                         \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                             \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                         \
            MFMA_FP4W_ASM(acc[i][j], afrag[i], bfrag[j], sa[i].d[(KS) >> 1],  \
                          sb[j].d[(KS) >> 1], HI);                            \
  } while (0)

__global__ __launch_bounds__(256, 4) void mfma_gemm_mxfp4_128u(
    const char* __restrict__ A, const unsigned char* __restrict__ SA,
    const char* __restrict__ Bt, const unsigned char* __restrict__ SB,
    float* __restrict__ C, int M, int N, int K) {
  __shared__ char lds[2 * 16384];  // [A][B], single-buffered

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = (wave >> 1) * 64;
  const int wave_n = (wave & 1) * 64;
  const int block_m = blockIdx.y * BM;
  const int block_n = blockIdx.x * BN;

  const long row_b = (long)(K >> 1);  // operand row, bytes
  const char* gA = A + (long)block_m * row_b;
  const char* gB = Bt + (long)block_n * row_b;

  f32x16 acc[2][2] = {};
  const int lane31 = lane & 31;
  const int kq_b = (lane >> 5) * 16;
  const int sc_shift = (lane >> 5) * 8;

  // this lane's scale rows (two A row-sets, two B column-sets, 32 rows
  // apart) as 32-bit offsets from the block's uniform base: 64-bit
  // per-lane pointers would cost 8 VGPRs this kernel does not have
  const unsigned srow_b = (unsigned)(K >> 5);
  const unsigned char* gSA = SA + (long)block_m * srow_b;
  const unsigned char* gSB = SB + (long)block_n * srow_b;
  const unsigned sa_off = (unsigned)(wave_m + lane31) * srow_b;
  const unsigned sb_off = (unsigned)(wave_n + lane31) * srow_b;

  char* As = &lds[0];
  char* Bs = &lds[16384];
  const int nk = K / BK4;
  for (int kt = 0; kt < nk; ++kt) {
    // scale loads go out ahead of the tile DMA; the barrier's vmcnt(0)
    // retires both
    MxScale sa[2], sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned step = (unsigned)i * 32u * srow_b + (unsigned)kt * 8u;
      sa[i] = load_mx_scale(gSA + (sa_off + step), sc_shift);
      sb[i] = load_mx_scale(gSB + (sb_off + step), sc_shift);
    }
    stage_lds<swz8, 4, 7, true>(gA, row_b, (long)kt * (BK4 / 2), 0, As, wave,
                                lane);
    stage_lds<swz8, 4, 7, true>(gB, row_b, (long)kt * (BK4 / 2), 0, Bs, wave,
                                lane);
    __syncthreads();
    MX_KSTEP(0, "0");
    MX_KSTEP(1, "1");
    MX_KSTEP(2, "0");
    MX_KSTEP(3, "1");
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

#undef MX_KSTEP
