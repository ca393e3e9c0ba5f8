// MX-scaled fp8 (OCP e4m3, unit e8m0 scales) MFMA GEMM kernels:
// C[M,N] = A[M,K] @ Bt[N,K]^T, fp8 in, fp32 out. v_mfma_scale_*_f8f6f4
// is the only path to the ~5 PF fp8 rate on gfx950 (non-scaled fp8 MFMA
// runs at the bf16 rate). The kernels are the measured ladder behind
// BASELINE.md; the numbers are the forced-variant `which` of kFp8Forced
// in gemm_dispatch.hip:
//   mfma_gemm_fp8_128s   3   128-tile BK=64 32x32 op, 4 blocks/CU
//   mfma_gemm_fp8_128u   5   128-tile BK=128 single-buffered, 4 blocks/CU
//                            (8, 10, 11, 12: its option arms)
//   mfma_gemm_fp8_128pc  7   producer/consumer wave split (9: XCD remap)
//   mfma_gemm_fp8_256x   13  256-tile full double buffer, 1 block/CU
// Measured out and removed (BASELINE.md keeps the numbers):
//   0   128-tile step-3 kernel, 2 blocks/CU
//   1   8-phase deep pipeline
//   2   128-tile BK=256, 1 block/CU
//   4   128-tile BK=128 1.5-buffered, 3 blocks/CU
//   6   256x128 tile, 2 blocks/CU
//   14  split-K
// Production dispatch (launch_fp8_best) launches only 128pc (K%128 == 0,
// grid <= 256 blocks), 128u (K%128 == 0 past that) and 128s (K%64 only).
//
// All 128-B-row images (BK=128 fp8) use swz8 and the same 16 KiB tile /
// half-tile staging as the bf16 kernels.
// Fragment map (32x32x64 op): A row=l&31, k=(l>>5)*32+j (32 consecutive
// fp8 = one v8i read); Bt likewise by column; C/D layout is
// shape-determined (same as bf16).
#pragma once

#include "gemm_common.hip"

// The scaled MFMAs are issued via INLINE ASM in every kernel that is
// register-tight: the __builtin_amdgcn_mfma_scale_* intrinsic's
// register-class constraints interact pathologically with
// global_load_lds on ROCm 7.2 (the identical 8-phase structure compiles
// to 180 VGPR/no-spill with bf16 MFMA but 256 VGPR + ~1 KB/lane scratch
// with the intrinsic, and scratch ops share the vm counter, corrupting
// counted-vmcnt drains). Hazards: inputs are ds_read results (compiler
// inserts lgkm waits for asm data deps); MFMA->MFMA on one accumulator
// is pipe-ordered; the only uncovered RAW is accumulator->epilogue
// VALU, guarded by mfma_drain().
#define MFMA_FP8W_ASM(ACCX, AOP, BOP)                                         \
  asm volatile(                                                               \
      "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 "              \
      "op_sel_hi:[0,0,0]"                                                     \
      : "+v"(ACCX)                                                            \
      : "v"(AOP), "v"(BOP), "v"(sc_reg), "v"(sc_reg))

// One BK=128 K-tile of a wave's 64x64 sub-tile from the swz8 images
// As/Bs: 2 k-steps x (2x2) 32x32x64 MFMAs, fragments transient.
__device__ __forceinline__ void mma_64x64_fp8w(
    const char* As, const char* Bs, int wave_m, int wave_n, int lane31,
    int kq_b, f32x16 (&acc)[2][2], int sc_reg) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    v8i afrag[2], bfrag[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int la = (wave_m + i * 32 + lane31) * 128 + ks * 64 + kq_b;
      int lb = (wave_n + i * 32 + lane31) * 128 + ks * 64 + kq_b;
      afrag[i] = load_frag32(As + swz8(la));
      bfrag[i] = load_frag32(Bs + swz8(lb));
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        MFMA_FP8W_ASM(acc[i][j], afrag[i], bfrag[j]);
  }
}

// fp8 step-3 variant with BK=64 + the 32x32x64 op: 32 KiB LDS/block
// -> 4 blocks/CU (16 waves/CU) — tests the occupancy hypothesis (a
// BK=256 1-block/CU kernel, since removed, showed the limiter is latency
// hiding, not FLOP/byte: BASELINE.md, "fp8 structure A/B").
// Image rows are 64 B (swz64).
__global__ __launch_bounds__(256, 4) void mfma_gemm_fp8_128s(
    const char* __restrict__ A, const char* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K) {
  __shared__ char lds[2 * 2 * 8192];  // [buf][A|B][8 KiB]

  const TileCoords t = tile_coords<BM, BN, 1>(A, Bt, K, blockIdx.y, blockIdx.x);

  f32x16 acc[2][2] = {};  // 2x2 tiles of 32x32 per wave (64 VGPR)
  const int lane31 = t.lane & 31;
  const int kq_b = (t.lane >> 5) * 32;
  const int sc_reg = mx_unit_scale();

  const int nk = K / 64;
  stage_lds<swz64, 2, 6, true>(t.gA, t.row_b, 0, 0, &lds[0], t.wave, t.lane);
  stage_lds<swz64, 2, 6, true>(t.gB, t.row_b, 0, 0, &lds[8192], t.wave, t.lane);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    char* As = &lds[buf * 2 * 8192];
    char* Bs = As + 8192;
    if (kt + 1 < nk) {
      char* An = &lds[(buf ^ 1) * 2 * 8192];
      stage_lds<swz64, 2, 6, true>(t.gA, t.row_b, (long)(kt + 1) * 64, 0, An,
                                   t.wave, t.lane);
      stage_lds<swz64, 2, 6, true>(t.gB, t.row_b, (long)(kt + 1) * 64, 0,
                                   An + 8192, t.wave, t.lane);
    }
    {
      v8i afrag[2], bfrag[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int la = (t.wave_m + i * 32 + lane31) * 64 + kq_b;
        int lb = (t.wave_n + i * 32 + lane31) * 64 + kq_b;
        afrag[i] = load_frag32(As + swz64(la));
        bfrag[i] = load_frag32(Bs + swz64(lb));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          MFMA_FP8W_ASM(acc[i][j], afrag[i], bfrag[j]);
    }
    __syncthreads();
  }
  mfma_drain();

  const int c_col32 = t.lane & 31;
  const int c_rowhi = (t.lane >> 5) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      store_acc_32x32(C, N, t.block_m + t.wave_m + i * 32,
                      t.block_n + t.wave_n + j * 32, acc[i][j],
                      c_rowhi, c_col32);
}

// fp8 BK=128 single-buffered at 4 blocks/CU: the remaining untried
// corner of the (BK, blocks/CU) grid — same 32 KiB LDS as the BK=64
// double-buffered shape (128s) but spent on tile DEPTH instead of a
// second buffer: stage A+B serially, one sync, 2x the math per
// barrier pair; the serial stage window is covered by the other 3
// blocks on the CU. Uses the 32x32x64 asm op (acc 2x2xf32x16 = 64
// VGPR) to stay under the 128-VGPR budget of 4 waves/SIMD.
// opts bitfield: 1 = XCD remap (measured LOSS for this tile size,
// fp8_ab_2 — kept for the record); 2 = timing skew (stagger
// co-resident blocks' barrier cadence: PMC shows 43% of wave cycles
// parked at 8192, consistent with the four blocks of a CU aligning
// their stage windows so the MFMA pipe idles in lockstep); 4 = kt
// rotation (same de-phasing applied to the DATA index — spreads tile
// reads in time for L2). Bits 2 and 4 are measured losses that only the
// forced variants 10-12 reach; taking them out measured neutral
// (profiles/fp8_128u_trim_ab.log) and waits for those variants to go.
__global__ __launch_bounds__(256, 4) void mfma_gemm_fp8_128u(
    const char* __restrict__ A, const char* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K, int opts) {
  __shared__ char lds[2 * 16384];  // [A][B], single-buffered

  // open-coded prologue: tile_coords() moves an s_waitcnt in this
  // kernel, which sits exactly on 128 VGPRs
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_m = (wave >> 1) * 64;
  const int wave_n = (wave & 1) * 64;
  int wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (opts & 1) wg = xcd_remap(wg, gridDim.x * gridDim.y);
  const int block_m = (wg / gridDim.x) * BM;
  const int block_n = (wg % gridDim.x) * BN;
  if (opts & 2) {
    // de-phase the ~4 co-resident blocks of a CU: dispatch walks XCDs
    // round-robin (block b -> XCD b%8), so blocks with consecutive
    // (b>>3) land near each other — skew their start by quarters of
    // the ~2 us per-kt round so stage windows interleave with the
    // neighbors' MFMA windows instead of aligning.
    int slot = (wg >> 3) & 3;
    for (int s = 0; s < slot * 3; ++s) __builtin_amdgcn_s_sleep(8);
  }

  const char* gA = A + (long)block_m * K;
  const char* gB = Bt + (long)block_n * K;
  const long row_b = (long)K;

  f32x16 acc[2][2] = {};
  const int lane31 = lane & 31;
  const int kq_b = (lane >> 5) * 32;
  const int sc_reg = mx_unit_scale();

  char* As = &lds[0];
  char* Bs = &lds[16384];
  const int nk = K / BK8;
  // fp32 accumulation over kt is order-independent for the bitwise
  // integer screens; rotation only changes WHICH tile each block
  // touches at a given time
  const int kt0 = (opts & 4) ? ((wg >> 3) & 3) * (nk >> 2) : 0;
  for (int ki = 0; ki < nk; ++ki) {
    const int kt = kt0 ? (ki + kt0) % nk : ki;
    stage_lds<swz8, 4, 7, true>(gA, row_b, (long)kt * BK8, 0, As, wave,
                                lane);
    stage_lds<swz8, 4, 7, true>(gB, row_b, (long)kt * BK8, 0, Bs, wave,
                                lane);
    __syncthreads();
    mma_64x64_fp8w(As, Bs, wave_m, wave_n, lane31, kq_b, acc, sc_reg);
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

// ---------------------------------------------------------------------------
// fp8 producer/consumer wave split (the round-2 lever named by the
// measured ladder): 512 threads = 4 PRODUCER waves (glds staging only)
// + 4 CONSUMER waves (MFMA only), double-buffered 64 KiB LDS,
// 2 blocks/CU -> 16 waves/CU (the winner's occupancy). There is NO
// block barrier in the K loop: buffers hand off through LDS flag
// counters (monotonic, so no reset races), producers run up to one
// buffer ahead, and consumers never sit in a stage window — the
// decoupling the barrier-stepped shapes cannot express. Safety: the
// flag polls are iteration-bounded so a logic bug produces garbage
// (caught by the bitwise screens), never a wedged GPU.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool lds_wait_ge(volatile int* p, int target) {
  for (long spin = 0; *p < target; ++spin) {
    if (spin > (1L << 24)) return false;  // bail, don't hang the device
    __builtin_amdgcn_s_sleep(1);
  }
  return true;
}

__global__ __launch_bounds__(512, 2) void mfma_gemm_fp8_128pc(
    const char* __restrict__ A, const char* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K, int xcd_swizzle) {
  __shared__ char lds[2 * 2 * 16384];  // [buf][A|B]
  __shared__ int prod_ready[2];        // 4 per staged iteration on buf
  __shared__ int cons_done[2];         // 4 per consumed iteration on buf

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;  // 0..7
  int wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (xcd_swizzle) wg = xcd_remap(wg, gridDim.x * gridDim.y);
  const int block_m = (wg / gridDim.x) * BM;
  const int block_n = (wg % gridDim.x) * BN;
  const char* gA = A + (long)block_m * K;
  const char* gB = Bt + (long)block_n * K;
  const long row_b = (long)K;
  const int nk = K / BK8;

  if (tid < 2) {
    prod_ready[tid] = 0;
    cons_done[tid] = 0;
  }
  __syncthreads();  // the only block barrier

  if (wave < 4) {
    // ---- producer: stage iteration kt into buffer kt&1 --------------
    for (int kt = 0; kt < nk; ++kt) {
      const int b = kt & 1;
      if (kt >= 2 && !lds_wait_ge(&cons_done[b], 4 * (kt / 2))) return;
      char* As = &lds[b * 2 * 16384];
      stage_lds<swz8, 4, 7, true>(gA, row_b, (long)kt * BK8, 0, As, wave, lane);
      stage_lds<swz8, 4, 7, true>(gB, row_b, (long)kt * BK8, 0, As + 16384,
                                  wave, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) atomicAdd(&prod_ready[b], 1);
    }
    return;
  }

  // ---- consumer: 64x64 per wave (same fragment map as 128u) ---------
  const int cw = wave - 4;
  const int wave_m = (cw >> 1) * 64;
  const int wave_n = (cw & 1) * 64;
  f32x16 acc[2][2] = {};
  const int lane31 = lane & 31;
  const int kq_b = (lane >> 5) * 32;
  const int sc_reg = mx_unit_scale();

  for (int kt = 0; kt < nk; ++kt) {
    const int b = kt & 1;
    if (!lds_wait_ge(&prod_ready[b], 4 * (kt / 2 + 1))) return;
    char* As = &lds[b * 2 * 16384];
    char* Bs = As + 16384;
    mma_64x64_fp8w(As, Bs, wave_m, wave_n, lane31, kq_b, acc, sc_reg);
    // every LDS read of this buffer must retire before releasing it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) atomicAdd(&cons_done[b], 1);
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

// ---------------------------------------------------------------------------
// fp8 256x256 tile at ONE block/CU (round-2 design point the ladder
// never tried): 512 threads = 8 waves = 2 waves/SIMD -> 256-VGPR
// budget, so the 128-VGPR accumulator AND all six 32-B fragments per
// ks persist in registers with no spills — the constraint that broke
// the bf16-template fp8 256 kernel (transient frags, 1.46 PF). LDS is
// a full double buffer (2 x 64 KiB); each kt overlaps the next tile's
// DMA with 16 MFMAs/wave of math. FLOP/byte doubles vs the 128-tile
// winner (256 vs 128), halving the L2 staging traffic that kernel
// runs at (9.2 TB/s of 34.5). Risk: only 2 MFMA-issuing waves/SIMD —
// the BK=256 lesson says 1/SIMD loses; 2/SIMD with 8 independent
// accumulator chains per wave is the open question this measures.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(512, 1) void mfma_gemm_fp8_256x(
    const char* __restrict__ A, const char* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K) {
  __shared__ char lds[2 * 2 * 32768];  // [buf][A|B], 128 KiB

  // 8 waves: wave_m 0..192, wave_n 0/128
  const TileCoords t =
      tile_coords<256, 256, 1>(A, Bt, K, blockIdx.y, blockIdx.x);

  f32x16 acc[2][4] = {};  // 2 m-tiles x 4 n-tiles of 32x32 = 128 VGPR
  const int lane31 = t.lane & 31;
  const int kq_b = (t.lane >> 5) * 32;
  const int sc_reg = mx_unit_scale();

  const int nk = K / BK8;
  // prologue: tile 0 into buffer 0 (8 waves x 4 KiB per 32 KiB tile)
  stage_lds<swz8, 4, 7, true>(t.gA, t.row_b, 0, 0, &lds[0], t.wave, t.lane);
  stage_lds<swz8, 4, 7, true>(t.gB, t.row_b, 0, 0, &lds[32768], t.wave, t.lane);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    char* As = &lds[buf * 2 * 32768];
    char* Bs = As + 32768;
    if (kt + 1 < nk) {  // overlap next tile's DMA with this tile's math
      char* An = &lds[(buf ^ 1) * 2 * 32768];
      stage_lds<swz8, 4, 7, true>(t.gA, t.row_b, (long)(kt + 1) * BK8, 0, An,
                                  t.wave, t.lane);
      stage_lds<swz8, 4, 7, true>(t.gB, t.row_b, (long)(kt + 1) * BK8, 0,
                                  An + 32768, t.wave, t.lane);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      v8i afrag[2], bfrag[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int la = (t.wave_m + i * 32 + lane31) * 128 + ks * 64 + kq_b;
        afrag[i] = load_frag32(As + swz8(la));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int lb = (t.wave_n + j * 32 + lane31) * 128 + ks * 64 + kq_b;
        bfrag[j] = load_frag32(Bs + swz8(lb));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          MFMA_FP8W_ASM(acc[i][j], afrag[i], bfrag[j]);
    }
    // barrier drains the in-flight glds (vmcnt(0) inside) and fences
    // every wave's reads of this buffer before its refill
    __syncthreads();
  }
  mfma_drain();

  const int c_col32 = t.lane & 31;
  const int c_rowhi = (t.lane >> 5) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      store_acc_32x32(C, N, t.block_m + t.wave_m + i * 32,
                      t.block_n + t.wave_n + j * 32, acc[i][j],
                      c_rowhi, c_col32);
}
