// Shared device code of the MFMA GEMM families (included by
// attest_kernels.hip, the one translation unit): vector types, tile
// constants, the LDS swizzles, and the helpers every kernel used to
// paste — global->LDS staging, the C/D store epilogues, the XCD block
// remap, the fp8 unit-scale register and the asm-MFMA drain.
//
// Layout notes (from the CDNA4 guides): wave = 64 lanes; for
// v_mfma_f32_16x16x32_bf16 each lane carries 8 bf16 of A and B and 4
// fp32 of C/D; A lane mapping row=l&15, k=(l>>4)*8+j; B (we require the
// second operand TRANSPOSED, i.e. Bt[N][K], so its lane mapping is the
// same as A's with col=l&15); C/D mapping col=l&15, row=(l>>4)*4+r.
// LDS tile images carry an XOR bank swizzle (see swz()) so fragment
// reads are bank-conflict-free while the global->LDS DMA stays
// lane-linear (the swizzle rides the source address).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>

using bf16 = __bf16;
typedef __attribute__((ext_vector_type(8))) bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) int v8i;

// 128-tile kernels: 128x128 block tile, waves in a 2-column grid, each
// owning 64 rows; K staged through LDS in 128-B-row images.
constexpr int BM = 128;  // block tile rows
constexpr int BN = 128;  // block tile cols
constexpr int BK = 64;   // bf16 K chunk per LDS stage (128 B rows)
// 256-tile 8-phase kernels
constexpr int BM2 = 256, BN2 = 256, BK2 = 64;
constexpr int HALF_B = 16384;  // one half-tile (128 rows x 128 B)
constexpr int BK8 = 128;       // fp8 elements per K-tile (128 B rows)

// ---------------------------------------------------------------------------
// LDS swizzles
// ---------------------------------------------------------------------------
__device__ __forceinline__ int swz(int byte_off) {
  // 3-bit XOR swizzle: inject row bits 1-3 (byte bits 8-10 of the
  // 128-B-row image) into bank bits 2-4 (byte bits 4-6). With the
  // fragment pattern row=(lane&15|31), khalf=(lane>>4|5)*16B this puts
  // the 16 lanes of every ds_read_b128 lane group on 16 distinct
  // 4-bank quads (enumerated for all four groups) — the 1-bit st_16x32
  // form left rows 0-3 on two quads (2-way conflict, ~9% of cycles in
  // the PMC profile, profiles/v256_8192_pmc.txt).
  return byte_off ^ (((byte_off >> 8) & 7) << 4);
}

// fp8 swizzle: XOR only byte bits 5-6 so every 32-B fragment stays
// physically contiguous — the fragment can then be ONE v8i load into a
// contiguous 8-register tuple (assembling it from two 16-B halves
// leaves the allocator building 8-tuples out of scattered pairs, which
// fragments past 256 VGPRs and spills). Costs a few 2-way LDS bank
// conflicts; fp8's read count is half bf16's, so that is cheap.
__device__ __forceinline__ int swz8(int byte_off) {
  return byte_off ^ (((byte_off >> 8) & 3) << 5);
}

// 64-B-row image (fp8 BK=64): inject row bit 2 into bank bit 3 (byte 5
// — whole-fragment granularity, see docs/KERNELS.md item 5, "Swizzle
// bits must relocate whole fragments"); residual 4-way conflicts on
// rows mod 8 accepted for the experiment.
__device__ __forceinline__ int swz64(int off) {
  return off ^ (((off >> 8) & 1) << 5);
}

__device__ __forceinline__ v8i load_frag32(const char* p) {
  return *(const v8i*)(p);
}

// 8-phase kernels: LDS slot of operand op (0=A, 1=B), buffer, half
__device__ __forceinline__ char* slot_ptr(char* lds, int op, int buf, int half) {
  return lds + ((op * 2 + buf) * 2 + half) * HALF_B;
}

// ---------------------------------------------------------------------------
// Global->LDS staging (global_load_lds_dwordx4; the compiler never
// auto-emits it). Every wave moves PASSES x 1 KiB: the DMA lands
// lane-linear at a wave-uniform LDS base, so the swizzle SWZ is applied
// to the GLOBAL source address instead. Rows of the image are
// 1 << ROW_SHIFT bytes. WAVE_MAJOR picks which KiB a wave owns:
//   true  — (wave * PASSES + p): a wave stages PASSES consecutive KiB;
//   false — (p * 8 + wave): the 8 waves of a half-tile interleave.
// That mapping decides which wave's DMA lands where, so it is part of
// each kernel's synchronisation structure — call sites must keep theirs.
// ---------------------------------------------------------------------------
template <int (*SWZ)(int), int PASSES, int ROW_SHIFT, bool WAVE_MAJOR>
__device__ __forceinline__ void stage_lds(
    const char* gbase, long row_stride_b, long k0_b, int row0, char* lds,
    int wave, int lane) {
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    int base = (WAVE_MAJOR ? wave * PASSES + p : p * 8 + wave) * 1024;
    int logical = SWZ(base + lane * 16);  // where lane's 16 B lands
    int row = logical >> ROW_SHIFT;
    int colb = logical & ((1 << ROW_SHIFT) - 1);
    const char* g = gbase + (long)(row0 + row) * row_stride_b + k0_b + colb;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)g,
        (__attribute__((address_space(3))) void*)(lds + base), 16, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// C/D store epilogues; (row0, col0) is the MFMA tile's top-left in C.
// 32x32 map: col=lane&31, row=(reg&3)+8*(reg>>2)+4*(lane>>5); the
//   caller passes c_col32 = lane & 31 and c_rowhi = (lane >> 5) * 4.
// 16x16 map: col=lane&15, row=(lane>>4)*4+r; the caller passes
//   c_col = lane & 15 and c_row0 = (lane >> 4) * 4.
// The lane terms are the caller's on purpose: a helper that derives
// them from `lane` is simplified on its own before it is inlined, the
// shifts fold differently from the kernel's other lane arithmetic, and
// several kernels then allocate one or two registers differently.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void store_acc_32x32(
    float* C, int N, int row0, int col0, const f32x16& acc, int c_rowhi,
    int c_col32) {
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    int row = row0 + (reg & 3) + 8 * (reg >> 2) + c_rowhi;
    int col = col0 + c_col32;
    C[(long)row * N + col] = acc[reg];
  }
}

__device__ __forceinline__ void store_acc_16x16(
    float* C, int N, int row0, int col0, const f32x4& acc, int c_row0,
    int c_col) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int row = row0 + c_row0 + r;
    int col = col0 + c_col;
    C[(long)row * N + col] = acc[r];
  }
}

// XCD-aware bijective block remap (the dispatcher places block b on XCD
// b%8): consecutive remapped ids share an XCD's L2, so A/B row reuse
// stops crossing dies when HBM-bound; the host enables it only once the
// working set exceeds the Infinity Cache.
__device__ __forceinline__ int xcd_remap(int wg, int nwg) {
  int q = nwg >> 3, r = nwg & 7;
  int xcd = wg & 7, o = wg >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + o;
}

// e8m0 1.0 in all four bytes, pinned in a VGPR for the asm scaled MFMAs
__device__ __forceinline__ int mx_unit_scale() {
  int sc_reg;
  asm("v_mov_b32 %0, 0x7f7f7f7f" : "=v"(sc_reg));
  return sc_reg;
}

// accumulator -> VALU RAW guard after asm MFMAs (the compiler cannot
// see through them; ~34 cycles of nops once per kernel)
__device__ __forceinline__ void mfma_drain() {
  asm volatile("s_nop 15\ns_nop 15\ns_nop 2" :::);
}

// Common prologue of the kernels whose waves form an (n/2) x 2 grid:
// each wave owns 64 rows and half the tile's columns. ELEM_B = bytes
// per operand element; gA/gB point at the block's first operand rows.
struct TileCoords {
  int lane, wave, wave_m, wave_n, block_m, block_n;
  const char *gA, *gB;
  long row_b;
};

template <int TILE_M, int TILE_N, int ELEM_B>
__device__ __forceinline__ TileCoords tile_coords(
    const void* A, const void* Bt, int K, int tile_row, int tile_col) {
  TileCoords t;
  const int tid = threadIdx.x;
  t.lane = tid & 63;
  t.wave = tid >> 6;
  t.wave_m = (t.wave >> 1) * 64;
  t.wave_n = (t.wave & 1) * (TILE_N / 2);
  t.block_m = tile_row * TILE_M;
  t.block_n = tile_col * TILE_N;
  t.gA = (const char*)A + (long)t.block_m * K * ELEM_B;
  t.gB = (const char*)Bt + (long)t.block_n * K * ELEM_B;
  t.row_b = (long)K * ELEM_B;
  return t;
}
