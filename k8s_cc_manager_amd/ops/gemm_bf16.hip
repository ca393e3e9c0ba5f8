// bf16 MFMA GEMM kernels:  C[M,N] = A[M,K] @ Bt[N,K]^T  (all row-major).
//   mfma_gemm_bf16       128x128 step-3, double-buffered
//   mfma_gemm_bf16_256   256x256 8-phase deep pipeline, 16x16x32 op
//   mfma_gemm_bf16_256w  256x256 8-phase deep pipeline, 32x32x16 op
//   mfma_gemm_bf16_128u  128x128 single-buffered, 4 blocks/CU
#pragma once

#include "gemm_common.hip"

// ---------------------------------------------------------------------------
// Grid: (N/BN, M/BM); block: 256 threads (4 waves, 2x2 of 64x64 = 4x4
// MFMA tiles of 16x16 each).
//
// Structure: the "step-3" ladder shape of the CDNA4 guide — 128x128
// tile, BK=64, direct global->LDS DMA double-buffered, st_16x32 XOR
// swizzle applied on the pre-swizzled GLOBAL source address (glds lands
// lane-linear in LDS, so the swizzle must ride the source) and on the
// ds_read fragment address, which turns the 8-way ds_read_b128 bank
// conflict of a linear [128][64]-bf16 image into a conflict-free read.
// ---------------------------------------------------------------------------
constexpr int TILE_B = BM * BK * 2;  // 16 KiB per operand tile

__global__ __launch_bounds__(256, 2) void mfma_gemm_bf16(
    const bf16* __restrict__ A, const bf16* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K) {
  // [buf][A|B][16 KiB]: one __shared__ object (a second one makes the
  // compiler drain vmcnt before every ds_read of a glds pipeline).
  __shared__ char lds[2 * 2 * TILE_B];

  // open-coded prologue: tile_coords() costs this kernel an SGPR
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;            // 0..3
  const int wave_m = (wave >> 1) * 64;  // wave row offset in block tile
  const int wave_n = (wave & 1) * 64;   // wave col offset
  const int block_m = blockIdx.y * BM;
  const int block_n = blockIdx.x * BN;

  const char* gA = (const char*)(A + (long)block_m * K);
  const char* gB = (const char*)(Bt + (long)block_n * K);
  const long row_b = (long)K * 2;

  f32x4 acc[4][4] = {};  // 4x4 MFMA tiles of 16x16 per wave

  const int lane15 = lane & 15;
  const int khalf_b = (lane >> 4) * 16;  // fragment k byte offset

  const int nk = K / BK;
  // prologue: stage tile 0 into buffer 0
  stage_lds<swz, 4, 7, true>(gA, row_b, 0, 0, &lds[0], wave, lane);
  stage_lds<swz, 4, 7, true>(gB, row_b, 0, 0, &lds[TILE_B], wave, lane);
  __syncthreads();  // drains the glds (vmcnt0 inside the barrier)

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    char* As = &lds[buf * 2 * TILE_B];
    char* Bs = As + TILE_B;
    // issue DMA for the NEXT tile into the other buffer (no wait here)
    if (kt + 1 < nk) {
      char* An = &lds[(buf ^ 1) * 2 * TILE_B];
      const long k0_b = (long)(kt + 1) * BK * 2;
      stage_lds<swz, 4, 7, true>(gA, row_b, k0_b, 0, An, wave, lane);
      stage_lds<swz, 4, 7, true>(gB, row_b, k0_b, 0, An + TILE_B, wave, lane);
    }
    // ---- MFMA over the 64-deep chunk: 2 k-steps of 32 ---------------
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 afrag[4], bfrag[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        int a_log = (wave_m + t * 16 + lane15) * 128 + ks * 64 + khalf_b;
        int b_log = (wave_n + t * 16 + lane15) * 128 + ks * 64 + khalf_b;
        afrag[t] = *(const bf16x8*)(As + swz(a_log));
        bfrag[t] = *(const bf16x8*)(Bs + swz(b_log));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[i], bfrag[j], acc[i][j], 0, 0, 0);
    }
    // one barrier per K-tile: everyone done reading buf, and the
    // in-flight glds for buf^1 is drained (implicit vmcnt(0) — the
    // structural cost of the 2-barrier structure, accepted here).
    __syncthreads();
  }

  const int c_col = lane & 15;
  const int c_row0 = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      store_acc_16x16(C, N, block_m + wave_m + i * 16,
                      block_n + wave_n + j * 16, acc[i][j], c_row0, c_col);
}

// ---------------------------------------------------------------------------
// 256x256 8-phase deep-pipelined MFMA GEMM (the CDNA4 guide's 256²
// template class). 512 threads = 8 waves (2M x 4N), BK=64, 128 KiB LDS:
// per double-buffer slot one K-tile of A and B, each in two 16 KiB
// halves (A rows 0-127 / 128-255; Bt rows likewise). Each phase
// computes one 128x128 block-quadrant (mh,nh) x K=64 — per wave 16
// MFMA — touching ONLY A-half mh and B-half nh, so half-tile slots free
// progressively and one half-tile is prefetched per phase with raw
// s_barrier + counted s_waitcnt vmcnt (never vmcnt(0) mid-loop except
// the final two iterations, where prefetch guards would otherwise leave
// needed DMAs undrained).
//
// Phase schedule per iteration J (t = 2J; quadrant order A0B0, A0B1,
// A1B1, A1B0 for tile t in buf0 then tile t+1 in buf1; A fragments are
// register-reused by quadrant pairs and B1 by phases 2-3, so the LDS
// read phases per slot are: A0@p1, B0@p1+p4, B1@p2, A1@p3 — slots free
// progressively and each phase prefetches exactly the slot freed the
// phase before):
//   p1 t:A0B0, prefetch B0(t+1);  p2 t:A0B1, A0(t+2);
//   p3 t:A1B1, B1(t+2);           p4 t:A1B0, A1(t+2) + vmcnt(6);
//   p5 t+1:A0B0, B0(t+2);         p6 t+1:A0B1, A0(t+3);
//   p7 t+1:A1B1, B1(t+3);         p8 t+1:A1B0, A1(t+3) + vmcnt(6).
// At each vmcnt(6)+s_barrier the three newest half-tiles may still fly;
// everything a following phase reads is >= 3 phases old and therefore
// drained for EVERY wave (the barrier makes the per-wave vmcnt
// chip-wide). Race-screened bitwise on integer data and against torch
// fp32 (tests/test_gpu_attest.py).
//
// A half-tile is staged by 8 waves x 2 glds (1 KiB per wave per
// instruction), pass-major.
// ---------------------------------------------------------------------------

// one phase: ds-read only the fragments this quadrant does NOT already
// hold (adjacent phases share an A-half or a B-half of the same K-tile,
// so those fragments persist in VGPRs across the phase barrier: phases
// read 12/4/8/4 b128 instead of 12 each), issue one half-tile prefetch,
// raw barrier, lgkmcnt(0), 16 MFMA at prio 1, raw barrier.
#define PHASE(buf, mh, nh, LOAD_A, LOAD_B, ACC, PREFETCH_STMT, DRAIN)          \
  do {                                                                         \
    if (LOAD_A) {                                                              \
      char* Ah = slot_ptr(lds, 0, (buf), (mh));                                \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                         \
          _Pragma("unroll") for (int i = 0; i < 4; ++i) {                      \
        int lg = (wave_mq + i * 16 + lane15) * 128 + ks * 64 + khalf_b;        \
        af[i][ks] = *(const bf16x8*)(Ah + swz(lg));                            \
      }                                                                        \
    }                                                                          \
    if (LOAD_B) {                                                              \
      char* Bh = slot_ptr(lds, 1, (buf), (nh));                                \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                         \
          _Pragma("unroll") for (int j = 0; j < 2; ++j) {                      \
        int lg = (wave_nq + j * 16 + lane15) * 128 + ks * 64 + khalf_b;        \
        bf[j][ks] = *(const bf16x8*)(Bh + swz(lg));                            \
      }                                                                        \
    }                                                                          \
    PREFETCH_STMT;                                                             \
    DRAIN;                                                                     \
    __builtin_amdgcn_s_barrier();                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         \
    __builtin_amdgcn_s_setprio(1);                                             \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                           \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                          \
            ACC[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(               \
                af[i][ks], bf[j][ks], ACC[i][j], 0, 0, 0);                     \
    __builtin_amdgcn_s_setprio(0);                                             \
    __builtin_amdgcn_s_barrier();                                              \
  } while (0)

__global__ __launch_bounds__(512, 1) void mfma_gemm_bf16_256(
    const bf16* __restrict__ A, const bf16* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K, int xcd_swizzle) {
  __shared__ char lds[8 * HALF_B];  // 128 KiB, ONE shared object

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;               // 0..7
  const int wave_mq = (wave >> 2) * 64;    // row offset inside a quadrant
  const int wave_nq = (wave & 3) * 32;     // col offset inside a quadrant
  const int lane15 = lane & 15;
  const int khalf_b = (lane >> 4) * 16;
  int wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (xcd_swizzle) wg = xcd_remap(wg, gridDim.x * gridDim.y);
  const int block_m = (wg / gridDim.x) * BM2;
  const int block_n = (wg % gridDim.x) * BN2;

  const char* gA = (const char*)(A + (long)block_m * K);
  const char* gB = (const char*)(Bt + (long)block_n * K);
  const long row_b = (long)K * 2;
  const int nk = K / BK2;

  // acc[mh][nh][i][j]: 2x2 quadrants x (4 m-frag x 2 n-frag) = 128 VGPR
  f32x4 acc00[4][2] = {}, acc01[4][2] = {}, acc10[4][2] = {}, acc11[4][2] = {};
  // fragment registers persist across phases (A shared by quadrant
  // pairs (mh,0)/(mh,1); B1 shared by phases 2-3, same K-tile)
  bf16x8 af[4][2], bf[2][2];

#define STAGE(op, buf, half, tile)                                             \
  stage_lds<swz, 2, 7, false>((op) == 0 ? gA : gB, row_b,                      \
                              (long)(tile) * BK2 * 2, (half) * 128,            \
                              slot_ptr(lds, (op), (buf), (half)), wave, lane)

  // prologue: tile 0 complete + A0,B1,A1 of tile 1 (iteration 0 stages
  // only B0(1) itself, at p1); full drain once.
  STAGE(0, 0, 0, 0);
  STAGE(1, 0, 0, 0);
  STAGE(0, 0, 1, 0);
  STAGE(1, 0, 1, 0);
  STAGE(0, 1, 0, 1);
  STAGE(1, 1, 1, 1);
  STAGE(0, 1, 1, 1);
  __syncthreads();

#define VM_DRAIN                                                               \
  do {                                                                         \
    if (tp + 4 >= nk)                                                          \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         \
    else                                                                       \
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                         \
  } while (0)

  for (int tp = 0; tp < nk; tp += 2) {
    // tile tp from buf0 (reads: 12 / 4 / 8 / 4 ds_read_b128) -----------
    PHASE(0, 0, 0, 1, 1, acc00, if (tp + 1 < nk) STAGE(1, 1, 0, tp + 1), );
    PHASE(0, 0, 1, 0, 1, acc01, if (tp + 2 < nk) STAGE(0, 0, 0, tp + 2), );
    PHASE(0, 1, 1, 1, 0, acc11, if (tp + 2 < nk) STAGE(1, 0, 1, tp + 2), );
    PHASE(0, 1, 0, 0, 1, acc10, if (tp + 2 < nk) STAGE(0, 0, 1, tp + 2), VM_DRAIN);
    // tile tp+1 from buf1 ----------------------------------------------
    PHASE(1, 0, 0, 1, 1, acc00, if (tp + 2 < nk) STAGE(1, 0, 0, tp + 2), );
    PHASE(1, 0, 1, 0, 1, acc01, if (tp + 3 < nk) STAGE(0, 1, 0, tp + 3), );
    PHASE(1, 1, 1, 1, 0, acc11, if (tp + 3 < nk) STAGE(1, 1, 1, tp + 3), );
    PHASE(1, 1, 0, 0, 1, acc10, if (tp + 3 < nk) STAGE(0, 1, 1, tp + 3), VM_DRAIN);
  }
#undef VM_DRAIN
#undef STAGE

#pragma unroll
  for (int mh = 0; mh < 2; ++mh) {
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      f32x4(*acc)[2] = mh == 0 ? (nh == 0 ? acc00 : acc01)
                               : (nh == 0 ? acc10 : acc11);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          store_acc_16x16(C, N, block_m + mh * 128 + wave_mq + i * 16,
                          block_n + nh * 128 + wave_nq + j * 16, acc[i][j],
                          (lane >> 4) * 4, lane & 15);
    }
  }
}

// ---------------------------------------------------------------------------
// Same 8-phase 256x256 structure on v_mfma_f32_32x32x16_bf16 (the
// higher-ceiling MFMA shape: 2382 vs 2075 TF/s µbench). Per quadrant a
// wave computes 2 m-tiles of 32x32 over 4 k-steps of 16 (8 MFMA/phase).
// Fragment maps: A row=l&31, k=(l>>5)*8+j; Bt col=l&31 likewise.
// ---------------------------------------------------------------------------
#define PHASE32(buf, mh, nh, ACC, PREFETCH_STMT, DRAIN, LOAD_A, LOAD_B)        \
  do {                                                                         \
    if (LOAD_A) {                                                              \
      char* Ah = slot_ptr(lds, 0, (buf), (mh));                                \
      _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                         \
          _Pragma("unroll") for (int t = 0; t < 2; ++t) {                      \
        int lg = (wave_mq + t * 32 + lane31) * 128 + ks * 32 + khalf32_b;      \
        a2[t][ks] = *(const bf16x8*)(Ah + swz(lg));                            \
      }                                                                        \
    }                                                                          \
    if (LOAD_B) {                                                              \
      char* Bh = slot_ptr(lds, 1, (buf), (nh));                                \
      _Pragma("unroll") for (int ks = 0; ks < 4; ++ks) {                       \
        int lg = (wave_nq + lane31) * 128 + ks * 32 + khalf32_b;               \
        b2[ks] = *(const bf16x8*)(Bh + swz(lg));                               \
      }                                                                        \
    }                                                                          \
    PREFETCH_STMT;                                                             \
    DRAIN;                                                                     \
    __builtin_amdgcn_s_barrier();                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         \
    __builtin_amdgcn_s_setprio(1);                                             \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                           \
        _Pragma("unroll") for (int t = 0; t < 2; ++t)                          \
            ACC[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                  \
                a2[t][ks], b2[ks], ACC[t], 0, 0, 0);                           \
    __builtin_amdgcn_s_setprio(0);                                             \
    __builtin_amdgcn_s_barrier();                                              \
  } while (0)

__global__ __launch_bounds__(512, 1) void mfma_gemm_bf16_256w(
    const bf16* __restrict__ A, const bf16* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K, int xcd_swizzle) {
  __shared__ char lds[8 * HALF_B];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_mq = (wave >> 2) * 64;
  const int wave_nq = (wave & 3) * 32;
  const int lane31 = lane & 31;
  const int khalf32_b = (lane >> 5) * 16;
  int wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (xcd_swizzle) wg = xcd_remap(wg, gridDim.x * gridDim.y);
  const int block_m = (wg / gridDim.x) * BM2;
  const int block_n = (wg % gridDim.x) * BN2;

  const char* gA = (const char*)(A + (long)block_m * K);
  const char* gB = (const char*)(Bt + (long)block_n * K);
  const long row_b = (long)K * 2;
  const int nk = K / BK2;

  f32x16 acc00[2] = {}, acc01[2] = {}, acc10[2] = {}, acc11[2] = {};
  bf16x8 a2[2][4], b2[4];

#define STAGE(op, buf, half, tile)                                             \
  stage_lds<swz, 2, 7, false>((op) == 0 ? gA : gB, row_b,                      \
                              (long)(tile) * BK2 * 2, (half) * 128,            \
                              slot_ptr(lds, (op), (buf), (half)), wave, lane)

  STAGE(0, 0, 0, 0);
  STAGE(1, 0, 0, 0);
  STAGE(0, 0, 1, 0);
  STAGE(1, 0, 1, 0);
  STAGE(0, 1, 0, 1);
  STAGE(1, 1, 1, 1);
  STAGE(0, 1, 1, 1);
  __syncthreads();

#define VM_DRAIN                                                               \
  do {                                                                         \
    if (tp + 4 >= nk)                                                          \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         \
    else                                                                       \
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                         \
  } while (0)

  for (int tp = 0; tp < nk; tp += 2) {
    PHASE32(0, 0, 0, acc00, if (tp + 1 < nk) STAGE(1, 1, 0, tp + 1), , 1, 1);
    PHASE32(0, 0, 1, acc01, if (tp + 2 < nk) STAGE(0, 0, 0, tp + 2), , 0, 1);
    PHASE32(0, 1, 1, acc11, if (tp + 2 < nk) STAGE(1, 0, 1, tp + 2), , 1, 0);
    PHASE32(0, 1, 0, acc10, if (tp + 2 < nk) STAGE(0, 0, 1, tp + 2), VM_DRAIN, 0, 1);
    PHASE32(1, 0, 0, acc00, if (tp + 2 < nk) STAGE(1, 0, 0, tp + 2), , 1, 1);
    PHASE32(1, 0, 1, acc01, if (tp + 3 < nk) STAGE(0, 1, 0, tp + 3), , 0, 1);
    PHASE32(1, 1, 1, acc11, if (tp + 3 < nk) STAGE(1, 1, 1, tp + 3), , 1, 0);
    PHASE32(1, 1, 0, acc10, if (tp + 3 < nk) STAGE(0, 1, 1, tp + 3), VM_DRAIN, 0, 1);
  }
#undef VM_DRAIN
#undef STAGE

  const int c_col32 = lane & 31;
  const int c_rowhi = (lane >> 5) * 4;
#pragma unroll
  for (int mh = 0; mh < 2; ++mh) {
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      f32x16* accq = mh == 0 ? (nh == 0 ? acc00 : acc01)
                             : (nh == 0 ? acc10 : acc11);
#pragma unroll
      for (int t = 0; t < 2; ++t)
        store_acc_32x32(C, N, block_m + mh * 128 + wave_mq + t * 32,
                        block_n + nh * 128 + wave_nq, accq[t],
                        c_rowhi, c_col32);
    }
  }
}

// bf16 transplant of the fp8 4-blocks/CU winner (mfma_gemm_fp8_128u):
// 128x128 tile, BK=64 (128-B rows, so the same 16-KiB-tile staging and
// swz8 image apply byte-for-byte), single-buffered 32 KiB LDS ->
// 4 blocks/CU, 32x32x16 ops with 2x2 tiles/wave (acc 64 VGPR). Tests
// whether the occupancy lever that took fp8 from 1516 to 2052 TF also
// moves bf16.
__global__ __launch_bounds__(256, 4) void mfma_gemm_bf16_128u(
    const bf16* __restrict__ A, const bf16* __restrict__ Bt,
    float* __restrict__ C, int M, int N, int K) {
  __shared__ char lds[2 * 16384];  // [A][B], single-buffered

  const TileCoords t = tile_coords<BM, BN, 2>(A, Bt, K, blockIdx.y, blockIdx.x);

  f32x16 acc[2][2] = {};
  const int lane31 = t.lane & 31;
  const int khalf_b = (t.lane >> 5) * 16;  // (l>>5)*8 bf16 = 16 B

  char* As = &lds[0];
  char* Bs = &lds[16384];
  const int nk = K / 64;  // 64 bf16 = 128 B per K-tile
  for (int kt = 0; kt < nk; ++kt) {
    stage_lds<swz8, 4, 7, true>(t.gA, t.row_b, (long)kt * 128, 0, As, t.wave,
                                t.lane);
    stage_lds<swz8, 4, 7, true>(t.gB, t.row_b, (long)kt * 128, 0, Bs, t.wave,
                                t.lane);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int la = (t.wave_m + i * 32 + lane31) * 128 + ks * 32 + khalf_b;
        int lb = (t.wave_n + i * 32 + lane31) * 128 + ks * 32 + khalf_b;
        af[i] = *(const bf16x8*)(As + swz8(la));
        bf[i] = *(const bf16x8*)(Bs + swz8(lb));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

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
