// Compute-unit sweep: a bitwise-checked matrix-core and whole-LDS
// self-test that every SIMD of every CU of every XCD has to run, with
// the place each wave ran read from the hardware ID registers.
//
//   cu_sweep       1024 threads and all 160 KiB of LDS per block, so a CU
//                  holds one block. Every wave marches the LDS with its
//                  block, runs four MFMA chains on operands it builds in
//                  registers, compares its accumulators bitwise with the
//                  golden C images and adds {hits, mfma_fail, lds_fail}
//                  to the record of the unit it ran on.
//   cu_sweep_gold  the golden C images: one block of plain VALU code
//                  (integer decode, fp32 adds, ldexpf; no MFMA, no
//                  conversion instruction) over the same generator.
//
// Unit key (14 bits): XCC_ID[3:0] << 10 | HW_ID[15:8] << 2 | SIMD_ID.
// HW_ID (hardware register 4): SIMD_ID 5:4, CU_ID 11:8, SH_ID 12,
// SE_ID 14:13; XCC_ID is register 20, bits 3:0 (bit layout from ROCm's
// amd_device_functions.h). Bit 15 of HW_ID stays in the key.
//
// Generator, defined in matrix space (never by block, wave or unit):
//   op 0  v_mfma_f32_32x32x16_bf16             A[32][16], B[32][16]
//   op 1  v_mfma_f32_16x16x32_bf16             A[16][32], B[16][32]
//   op 2  v_mfma_scale_f32_32x32x64_f8f6f4     e4m3, A[32][64], B[32][64],
//                                              E8M0 SA[32][2], SB[32][2]
//   op 3  the same opcode, e2m1 (cbsz:4 blgp:4), same shapes
// `which` is 0 for A / SA and 1 for B / SB; B is held transposed
// (B[col][k]) like every Bt of this project. Element (op, which, round
// r, row, k) is the e2m1 code
//   idx = (b + k * s) % 11,  b = (3 row + 5 r + 2 op + 4 which) % 11,
//                            s = 1 + ((row >> 2) + r) % 10
//   idx 0 -> 0, 1..5 -> +{0.5, 1, 1.5, 2, 3}, 6..10 -> -{0.5, 1, 1.5, 2, 3}
// (values exact in bf16, e4m3 and e2m1; 32 rows give 32 distinct (b, s)),
// and scale byte (op, which, r, row, kb) is
//   126 + (x + (x >> 3)) % 3,  x = (row + 1)(2 r + 3) + 5 kb + 7 which + op.
//
// Exactness: products are multiples of 2^-2 up to 9, scale pairs
// multiply by 2^-2 .. 2^2, so every term is a multiple of 2^-4 of at most
// 36 and a round adds at most 64 * 36 = 2304 per element: up to
// CU_SWEEP_MAX_ROUNDS = 256 rounds every partial sum, in any order, is
// a multiple of 2^-4 below 2^20 and fits 24 bits. MFMA and VALU must
// agree bitwise.
#pragma once

#include "gemm_common.hip"
#include "gemm_fp4.hip"
#include "probe_kernels.hip"

constexpr int CU_SWEEP_LDS_WORDS = 40960;  // 160 KiB of uint32: a CU's LDS
constexpr int CU_SWEEP_LDS_ROUNDS = 2;     // pattern, then its complement
constexpr int CU_SWEEP_MAX_ROUNDS = 256;   // exactness cap (above)
constexpr int CU_SWEEP_UNITS = 16384;      // 14-bit unit key
constexpr int CU_SWEEP_REC = 3;            // hits, mfma_fail, lds_fail
// row-major golden C images: op 0 32x32, op 1 16x16, op 2 and 3 32x32
constexpr int CU_SWEEP_GOLD0 = 0, CU_SWEEP_GOLD1 = 1024;
constexpr int CU_SWEEP_GOLD2 = 1280, CU_SWEEP_GOLD3 = 2304;
constexpr int CU_SWEEP_GOLD_ELEMS = 3328;

// s_getreg immediate: hardware register id, bit offset, field size
constexpr int sweep_getreg(int size, int offset, int reg) {
  return ((size - 1) << 11) | (offset << 6) | reg;
}

// ---------------------------------------------------------------------------
// The generator
// ---------------------------------------------------------------------------
__device__ __forceinline__ int sweep_base(int op, int which, int r, int row) {
  return (3 * row + 5 * r + 2 * op + 4 * which) % 11;
}

__device__ __forceinline__ int sweep_stride(int r, int row) {
  return 1 + ((row >> 2) + r) % 10;
}

__device__ __forceinline__ int sweep_idx_code(int idx) {
  return idx <= 5 ? idx : (8 | (idx - 5));
}

// direct form (the golden kernel's)
__device__ __forceinline__ int sweep_code(int op, int which, int r, int row,
                                          int k) {
  return sweep_idx_code(
      (sweep_base(op, which, r, row) + k * sweep_stride(r, row)) % 11);
}

__device__ __forceinline__ int sweep_scale(int op, int which, int r, int row,
                                           int kb) {
  int x = (row + 1) * (2 * r + 3) + 5 * kb + 7 * which + op;
  return 126 + (x + (x >> 3)) % 3;
}

// incremental form along k (the MFMA kernel's): same sequence, one add
// and one conditional subtract per element
struct SweepGen {
  int idx, s;
  __device__ __forceinline__ SweepGen(int op, int which, int r, int row,
                                      int k0) {
    s = sweep_stride(r, row);
    idx = (sweep_base(op, which, r, row) + k0 * s) % 11;
  }
  __device__ __forceinline__ int next() {
    int code = sweep_idx_code(idx);
    idx += s;
    if (idx >= 11) idx -= 11;
    return code;
  }
};

// 8 consecutive k of one row as a bf16 fragment
__device__ __forceinline__ bf16x8 sweep_frag_bf16(int op, int which, int r,
                                                  int row, int k0) {
  SweepGen g(op, which, r, row, k0);
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    f[j] = (bf16)(0.5f * (float)e2m1_times2(g.next()));
  return f;
}

// OCP e4m3 byte of an e2m1 code with magnitude index 0..5:
// 0, 0.5, 1, 1.5, 2, 3 = 0x00 0x30 0x38 0x3c 0x40 0x44
__device__ __forceinline__ unsigned sweep_e4m3(int code) {
  unsigned mag = (unsigned)(0x44403c383000ull >> (8 * (code & 7))) & 0xffu;
  return mag | ((unsigned)(code & 8) << 4);
}

// e4m3 operand of lane (row, half) for the 32x32x64 op: an 8-register
// operand holds two runs of 16 consecutive k, registers 0-3 from K block
// 0 and registers 4-7 from K block 1: byte b of register v is
// k = 32 (v >> 2) + 16 half + 4 (v & 3) + b. With unit scales any
// k order that A and B share gives the same sums (the GEMMs of
// gemm_fp8.hip load 32 consecutive bytes); with real scales the blocks
// are visible, and this is the map the device computes bitwise with
// (measured: docs/KERNELS.md, "Compute-unit sweep").
__device__ __forceinline__ v8i sweep_frag_fp8(int which, int r, int row,
                                              int half) {
  v8i f;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    SweepGen g(2, which, r, row, 32 * kb + 16 * half);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      unsigned w = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) w |= sweep_e4m3(g.next()) << (8 * j);
      f[4 * kb + d] = (int)w;
    }
  }
  return f;
}

// 32 consecutive k of one row: element j in bits 4j..4j+3 of 128
__device__ __forceinline__ v4i sweep_frag_fp4(int which, int r, int row,
                                              int k0) {
  SweepGen g(3, which, r, row, k0);
  v4i f;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) w |= (unsigned)g.next() << (4 * j);
    f[d] = (int)w;
  }
  return f;
}

// The scaled MFMAs in the form of MFMA_FP8W_ASM / MFMA_FP4W_ASM, scale
// byte 0 of both scale registers. Here the operands and scales come
// straight from VALU instructions, whose distance to an asm MFMA the
// compiler does not manage, hence the leading s_nop. FMT is "" for e4m3
// (8-register operands) or "cbsz:4 blgp:4" for e2m1 (4-register).
#define SWEEP_MFMA_SCALE_ASM(ACCX, AOP, BOP, SCA, SCB, FMT)                   \
  asm volatile(                                                               \
      "s_nop 3\n"                                                             \
      "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 "              \
      "op_sel:[0,0,0] op_sel_hi:[0,0,0] " FMT                                 \
      : "+v"(ACCX)                                                            \
      : "v"(AOP), "v"(BOP), "v"(SCA), "v"(SCB))

__device__ __forceinline__ unsigned sweep_wave_sum(unsigned v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // lane 0 holds the wave's sum
}

__device__ __forceinline__ unsigned sweep_differs(float got, float want) {
  return __float_as_uint(got) != __float_as_uint(want) ? 1u : 0u;
}

// ---------------------------------------------------------------------------
// cu_sweep. table: CU_SWEEP_UNITS records of CU_SWEEP_REC words, the
// only memory this kernel writes (atomic adds). No spins, no
// inter-block communication, fixed trip counts.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void cu_sweep(
    const float* __restrict__ gold, unsigned* __restrict__ table, int rounds,
    int poison_key) {
  __shared__ uint32_t slab[CU_SWEEP_LDS_WORDS];
  const int tid = threadIdx.x;
  const int lane = tid & 63;

  // -- identity: where this wave runs ----------------------------------
  const unsigned hw = __builtin_amdgcn_s_getreg(sweep_getreg(8, 8, 4));
  const unsigned simd = __builtin_amdgcn_s_getreg(sweep_getreg(2, 4, 4));
  const unsigned xcc = __builtin_amdgcn_s_getreg(sweep_getreg(4, 0, 20));
  const unsigned key = (xcc << 10) | (hw << 2) | simd;  // < CU_SWEEP_UNITS

  // -- LDS march over the CU's whole LDS (arithmetic of lds_probe) -----
  unsigned lds_fail = 0;
  for (int r = 0; r < CU_SWEEP_LDS_ROUNDS; ++r) {
    const uint32_t salt = 0x9e3779b9u * ((r >> 1) + 1) + blockIdx.x;
    const uint32_t inv = (r & 1) ? 0xffffffffu : 0u;
    for (int i = tid; i < CU_SWEEP_LDS_WORDS; i += 1024)
      slab[i] = ((uint32_t)i * 2654435769u + salt) ^ inv;
    __syncthreads();
    // read back through a bijective permutation (33 is coprime to 40960)
    for (int i = tid; i < CU_SWEEP_LDS_WORDS; i += 1024) {
      int j = (i * 33 + r) % CU_SWEEP_LDS_WORDS;
      uint32_t want = ((uint32_t)j * 2654435769u + salt) ^ inv;
      if (slab[j] != want) ++lds_fail;
    }
    // the count is final here: without this the compiler keeps the 40
    // words it read until after the MFMA chains (in scratch)
    asm volatile("" : "+v"(lds_fail));
    __syncthreads();
  }

  // -- four MFMA chains, operands built in registers -------------------
  const int row32 = lane & 31, half = lane >> 5;
  const int row16 = lane & 15, quad = lane >> 4;
  f32x16 c0 = {}, c2 = {}, c3 = {};
  f32x4 c1 = {};
#pragma unroll 1
  for (int r = 0; r < rounds; ++r) {
    {  // op 0: lane holds A[row32][8 half + j], B[row32][8 half + j]
      bf16x8 a = sweep_frag_bf16(0, 0, r, row32, 8 * half);
      bf16x8 b = sweep_frag_bf16(0, 1, r, row32, 8 * half);
      c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c0, 0, 0, 0);
    }
    {  // op 1: lane holds A[row16][8 quad + j], B[row16][8 quad + j]
      bf16x8 a = sweep_frag_bf16(1, 0, r, row16, 8 * quad);
      bf16x8 b = sweep_frag_bf16(1, 1, r, row16, 8 * quad);
      c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c1, 0, 0, 0);
    }
    {  // op 2: lane holds 16 k of each K block of row32 (sweep_frag_fp8)
       // and supplies the scale of K block `half`
      v8i a = sweep_frag_fp8(0, r, row32, half);
      v8i b = sweep_frag_fp8(1, r, row32, half);
      int sa = sweep_scale(2, 0, r, row32, half);
      int sb = sweep_scale(2, 1, r, row32, half);
      SWEEP_MFMA_SCALE_ASM(c2, a, b, sa, sb, "");
    }
    {  // op 3: the fp4 map of gemm_fp4.hip
      v4i a = sweep_frag_fp4(0, r, row32, 32 * half);
      v4i b = sweep_frag_fp4(1, r, row32, 32 * half);
      int sa = sweep_scale(3, 0, r, row32, half);
      int sb = sweep_scale(3, 1, r, row32, half);
      SWEEP_MFMA_SCALE_ASM(c3, a, b, sa, sb, "cbsz:4 blgp:4");
    }
  }
  mfma_drain();

  // a wrong number on request, so that detection can be tested
  if ((int)key == poison_key && lane == 0)
    c0[0] = __uint_as_float(__float_as_uint(c0[0]) ^ 1u);

  // -- bitwise compare through the C/D lane maps -----------------------
  // the golden loads stay below this point: hoisted above the chains
  // they would sit in 52 registers the accumulators need (and spill)
  asm volatile("" ::: "memory");
  unsigned mfma_fail = 0;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    // store_acc_32x32's map
    int at = ((reg & 3) + 8 * (reg >> 2) + 4 * half) * 32 + row32;
    mfma_fail += sweep_differs(c0[reg], gold[CU_SWEEP_GOLD0 + at]);
    mfma_fail += sweep_differs(c2[reg], gold[CU_SWEEP_GOLD2 + at]);
    mfma_fail += sweep_differs(c3[reg], gold[CU_SWEEP_GOLD3 + at]);
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)  // store_acc_16x16's map
    mfma_fail += sweep_differs(
        c1[reg], gold[CU_SWEEP_GOLD1 + (quad * 4 + reg) * 16 + row16]);

  mfma_fail = sweep_wave_sum(mfma_fail);
  lds_fail = sweep_wave_sum(lds_fail);
  if (lane == 0) {
    unsigned* rec = table + key * CU_SWEEP_REC;
    atomicAdd(rec + 0, 1u);
    if (mfma_fail) atomicAdd(rec + 1, mfma_fail);
    if (lds_fail) atomicAdd(rec + 2, lds_fail);
  }
}

// ---------------------------------------------------------------------------
// cu_sweep_gold: one block; thread e, e + blockDim.x, ... each own one
// element of the four row-major C images. Per 32-element K block (the
// whole K for the unscaled ops) the integer products, 4x their value,
// are summed in fp32 in k order and scaled with ldexpf.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void cu_sweep_gold(float* __restrict__ out,
                                                      int rounds) {
  for (int e = threadIdx.x; e < CU_SWEEP_GOLD_ELEMS; e += blockDim.x) {
    int op, at, dim, kblk, nblk;
    if (e < CU_SWEEP_GOLD1) {
      op = 0, at = e, dim = 32, kblk = 16, nblk = 1;
    } else if (e < CU_SWEEP_GOLD2) {
      op = 1, at = e - CU_SWEEP_GOLD1, dim = 16, kblk = 32, nblk = 1;
    } else if (e < CU_SWEEP_GOLD3) {
      op = 2, at = e - CU_SWEEP_GOLD2, dim = 32, kblk = 32, nblk = 2;
    } else {
      op = 3, at = e - CU_SWEEP_GOLD3, dim = 32, kblk = 32, nblk = 2;
    }
    const int i = at / dim, j = at % dim;
    float acc = 0.f;
    for (int r = 0; r < rounds; ++r) {
      for (int kb = 0; kb < nblk; ++kb) {
        float blk = 0.f;
        for (int kk = 0; kk < kblk; ++kk) {
          int k = kb * kblk + kk;
          blk += (float)(e2m1_times2(sweep_code(op, 0, r, i, k)) *
                         e2m1_times2(sweep_code(op, 1, r, j, k)));
        }
        int ex = -2;
        if (op >= 2)
          ex += sweep_scale(op, 0, r, i, kb) + sweep_scale(op, 1, r, j, kb) -
                254;
        acc += ldexpf(blk, ex);
      }
    }
    out[e] = acc;
  }
}
