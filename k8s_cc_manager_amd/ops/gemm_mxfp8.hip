// MXFP8 (OCP e4m3 or e5m2 values, one E8M0 scale per 32 elements along
// K) MFMA GEMM: C[M,N] = sum over 32-element K blocks of
//   2^(SA[m,kb] + SB[n,kb] - 254) * sum_{k in kb} A[m,k] * Bt[n,k],
// fp32 out. A[M,K] and Bt[N,K] are one byte per element, row-major;
// SA[M,K/32] and SB[N,K/32] are E8M0 bytes. FA and FB are the hardware's
// format selectors of the two operands, chosen independently: 0 = e4m3
// (cbsz:0 / blgp:0), 1 = e5m2 (cbsz:1 / blgp:1). This is the only kernel
// of the project that runs the e5m2 decoder, 8-bit operands with scales
// other than 1.0, and the opcode with cbsz != blgp.
//
// Outer shape: mfma_gemm_fp8_128u (128x128 block, 256 threads, a wave
// owns 64x64 as 2x2 accumulators of the 32x32x64 op, BK = 128, one
// single-buffered 32 KiB LDS image pair, 4 blocks/CU, operands by
// global_load_lds through stage_lds<..., 4, 7, true>).
//
// Operand image: this kernel's own. The 8-register operand of the
// 32x32x64 op does not hold 32 consecutive k (docs/KERNELS.md,
// compute-unit sweep): byte b of register v of lane (row, h) is
//   k = 32*(v>>2) + 16*h + 4*(v&3) + b,
// i.e. bytes 16h..16h+15 of K block 2ks followed by bytes 16h..16h+15 of
// K block 2ks+1, and the lane supplies the scale of K block h. In memory
// those are two 16-byte pieces 32 bytes apart. Reading two pieces would
// assemble the 8-tuple from scattered pairs (the swz8 comment in
// gemm_common.hip says what that costs), so the k permutation is folded
// into the DMA's global source address instead, where stage_lds already
// applies the swizzle:
//   - the fragment read is mma_64x64_fp8w's: one load_frag32 at
//     swz8(L), L = row*128 + ks*64 + h*32, which covers the logical
//     offsets L + q*16 + byte, q = 0/1 the half of the 32-byte read;
//   - the lane map wants register half q to hold source column
//     ks*64 + q*32 + h*16 + byte: that is L with bits 4 (q) and 5 (h)
//     exchanged;
//   - stage_lds asks SWZ(P) for the source of physical offset P. swz8 is
//     an involution, so swz8(P) is the logical offset L that a reader
//     finds at P, and the source is swap_bits_4_and_5(swz8(P)). The swap
//     comes after swz8 because swz8 XORs bits 5-6: swapping first would
//     move the XOR onto the wrong bit.
// Both steps keep bits 7 and up (the row) and bits 0-3, so every DMA pass
// still fetches whole 128-byte row segments (coalescing unchanged), and
// the LDS read addresses are exactly mfma_gemm_fp8_128u's (its bank
// behaviour, no new enumeration).
//
// Scales: MXFP6's scheme. Per K-tile a lane loads the 4 scale bytes of
// its row as one dword (two A row-sets, two B column-sets, 32-bit offsets
// from a uniform base) and shifts it right by 8*(lane>>5): K block
// 2*ks + (lane>>5) then sits at byte 2*ks for every lane and op_sel_hi
// depends on ks only. The loads go out ahead of the tile DMA; the
// barrier's vmcnt(0) retires both.
//
// Registers: two A fragments and ONE B fragment at a time (24 fragment
// VGPRs, j outer / i inner); resources in docs/KERNELS.md, "MXFP8 leg".
#pragma once

#include "gemm_common.hip"

// swz8, then exchange byte-offset bits 4 and 5 (derivation above)
__device__ __forceinline__ int swz8mx(int byte_off) {
  const int l = swz8(byte_off);
  const int d = ((l >> 4) ^ (l >> 5)) & 1;
  return l ^ (d * 0x30);
}

// cbsz is A's format and blgp is B's; HI picks byte 0 or byte 2 of both
// scale registers, as in MFMA_FP6_ASM. All three are immediates.
template <int FA, int FB, int HI>
__device__ __forceinline__ void mfma_mx8(f32x16& acc, const v8i& a,
                                         const v8i& b, int sca, int scb) {
  asm volatile(
      "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 "
      "op_sel:[0,0,0] op_sel_hi:[%5,%5,0] cbsz:%6 blgp:%7"
      : "+v"(acc)
      : "v"(a), "v"(b), "v"(sca), "v"(scb), "n"(HI), "n"(FA), "n"(FB));
}

// One k-step of a wave's 64x64 sub-tile: 2x2 32x32x64 MFMAs on K blocks
// 2*KS and 2*KS+1 of the tile; a_off / b_off are the lane's logical image
// offsets at ks = 0.
template <int FA, int FB, int KS>
__device__ __forceinline__ void mx8_kstep(const char* As, const char* Bs,
                                          const int (&a_off)[2],
                                          const int (&b_off)[2],
                                          f32x16 (&acc)[2][2],
                                          const int (&sa)[2],
                                          const int (&sb)[2]) {
  v8i afrag[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    afrag[i] = load_frag32(As + swz8(a_off[i] + KS * 64));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const v8i bfrag = load_frag32(Bs + swz8(b_off[j] + KS * 64));
#pragma unroll
    for (int i = 0; i < 2; ++i)
      mfma_mx8<FA, FB, KS>(acc[i][j], afrag[i], bfrag, sa[i], sb[j]);
  }
}

template <int FA, int FB>
__global__ __launch_bounds__(256, 4) void mfma_gemm_mxfp8_128(
    const char* __restrict__ A, const unsigned char* __restrict__ SA,
    const char* __restrict__ Bt, const unsigned char* __restrict__ SB,
    float* __restrict__ C, int M, int N, int K) {
  static_assert((FA == 0 || FA == 1) && (FB == 0 || FB == 1), "e4m3 or e5m2");
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

  f32x16 acc[2][2] = {};
  const int lane31 = lane & 31;
  const int sc_shift = (lane >> 5) * 8;

  // this lane's fragments in the images (logical offsets, ks = 0)
  int a_off[2], b_off[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a_off[i] = (wave_m + i * 32 + lane31) * 128 + (lane >> 5) * 32;
    b_off[i] = (wave_n + i * 32 + lane31) * 128 + (lane >> 5) * 32;
  }

  // scale rows as 32-bit offsets from the block's uniform base, as in
  // mfma_gemm_mxfp4_128u
  const unsigned srow_b = (unsigned)(K >> 5);
  const unsigned char* gSA = SA + (long)block_m * srow_b;
  const unsigned char* gSB = SB + (long)block_n * srow_b;
  const unsigned sa_off = (unsigned)(wave_m + lane31) * srow_b;
  const unsigned sb_off = (unsigned)(wave_n + lane31) * srow_b;

  char* As = &lds[0];
  char* Bs = &lds[16384];
  const int nk = K / BK8;
  for (int kt = 0; kt < nk; ++kt) {
    int sa[2], sb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const unsigned step = (unsigned)i * 32u * srow_b + (unsigned)kt * 4u;
      sa[i] = (int)*(const unsigned*)(gSA + (sa_off + step));
      sb[i] = (int)*(const unsigned*)(gSB + (sb_off + step));
    }
    stage_lds<swz8mx, 4, 7, true>(gA, row_b, (long)kt * BK8, 0, As, wave,
                                  lane);
    stage_lds<swz8mx, 4, 7, true>(gB, row_b, (long)kt * BK8, 0, Bs, wave,
                                  lane);
    __syncthreads();
    // The shift is held behind the barrier: written next to the load, each
    // of the four loads lands in one shared scratch register and is waited
    // for by itself (four serial memory round trips per K-tile) before the
    // DMA is issued.
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      asm volatile("" : "+v"(sa[i]), "+v"(sb[i]));
      sa[i] = (int)((unsigned)sa[i] >> sc_shift);
      sb[i] = (int)((unsigned)sb[i] >> sc_shift);
    }
    mx8_kstep<FA, FB, 0>(As, Bs, a_off, b_off, acc, sa, sb);
    mx8_kstep<FA, FB, 1>(As, Bs, a_off, b_off, acc, sa, sb);
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
