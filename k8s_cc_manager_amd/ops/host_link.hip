// Host link: the shader side of the verified PCIe passes. The kernels
// run on a mapped, page-locked host buffer (hipHostMalloc or
// hipHostRegister memory, never managed or pageable), so every load and
// store below crosses the link.
//
//   link_pull<PHASE>   every 16-byte vector of the buffer is loaded over
//                      the link and compared with phase PHASE; nothing is
//                      written.
//   link_push<PHASE>   every vector is stored over the link with phase
//                      PHASE; nothing is read (no read-modify-write).
//   link_duplex        one launch, both directions: even blocks pull and
//                      check the lower half of the buffer, odd blocks push
//                      into the upper half, both in phase 0. The role is
//                      uniform per block and each half is strided by the
//                      blocks of its own role only.
//
// Pattern, phases, the mismatch record and its vector atomics are the
// HBM march's (hbm_march.hip); the caller moves the logical origin per
// pass so that no two passes expect the same word at the same offset.
//
// Shape. What counts over PCIe is the size of a request and how many are
// outstanding, not blocks per CU: the link is ~100x slower than HBM and
// march_step's 8 blocks per CU buy nothing here. Per stride a block owns
// U * 256 contiguous vectors (16 KiB at U = 4) and a lane's U vectors are
// 4 KiB apart, so every load or store instruction of a wave covers 1 KiB
// of contiguous, lane-ordered bytes (global_load_dwordx4 /
// global_store_dwordx4) and a block's stores form a run that write
// combining can pack into full payloads. U loads are issued before the
// first compare. The grid is HOST_LINK_MAX_BLOCKS blocks whatever the CU
// count (fewer for a small buffer), a stride of 1 MiB: grid and U were
// settled by measurement (docs/KERNELS.md, "Host link"). Every setting
// from 16 to 1024 blocks fills the link one way; the small grid is the
// one that also keeps both directions fed in link_duplex, and more
// blocks cost the pull 3 to 6 %.
//
// As in the march: one multiply per lane, the pattern advances by adds
// with the hi carry when lo wraps, in-buffer indices are 32-bit (a buffer
// is at most 1 GiB = 2^26 vectors), the last short group takes a tail
// path one vector at a time, the clean path does no atomics. Trip counts
// are fixed by nvec and the grid: no spins, no flags.
#pragma once

#include "hbm_march.hip"

constexpr int HOST_LINK_THREADS = 256;
constexpr int HOST_LINK_UNROLL = 4;         // vectors in flight per lane
constexpr int HOST_LINK_MAX_BLOCKS = 64;    // the grid, at most
constexpr unsigned long long HOST_LINK_MAX_BYTES = 1ull << 30;
constexpr unsigned long long HOST_LINK_PASS_STRIDE = 1ull << 40;  // origin per pass

// One role's walk over [base, base + nvec): `block` of `nblocks` blocks
// of that role. CHECK / WRITE: phase 0..2 or -1 (none), exactly one set.
// w0: logical word index of base[0]; byte0: its window byte offset.
template <int CHECK, int WRITE, int U>
__device__ __forceinline__ void link_span(u32x4* __restrict__ base,
                                          uint32_t nvec, unsigned long long w0,
                                          unsigned long long byte0,
                                          HbmMarchResult* __restrict__ res,
                                          int pass, uint32_t block,
                                          uint32_t nblocks) {
  static_assert((CHECK >= 0 && CHECK <= 2 && WRITE == -1) ||
                    (WRITE >= 0 && WRITE <= 2 && CHECK == -1),
                "one direction per role");
  constexpr uint32_t V = HOST_LINK_THREADS;  // vectors between a lane's U
  const uint32_t T = nblocks * (U * V);      // vectors per stride (<= 2^22)
  uint32_t i = block * (U * V) + threadIdx.x;
  const unsigned long long w = w0 + 4ull * i;
  uint32_t lo = (uint32_t)w;
  uint32_t p = hbm_march_pattern(w);  // the one multiply per lane
  const uint32_t dlo = 4u * T;
  const uint32_t dp = dlo * HBM_MARCH_MUL_LO;
  constexpr uint32_t ulo = 4u * V;
  constexpr uint32_t up = ulo * HBM_MARCH_MUL_LO;

  auto one = [&](uint32_t idx, uint32_t pv, u32x4 got) {
    if (CHECK >= 0) {
      const u32x4 want = hbm_march_vec<CHECK>(pv);
      const u32x4 d = got ^ want;
      if (d[0] | d[1] | d[2] | d[3])
        hbm_march_mismatch(res, byte0 + 16ull * idx, want, got, pass);
    } else {
      base[idx] = hbm_march_vec<WRITE>(pv);
    }
  };
  // pattern `words` further on: lo wrapped iff w crossed 2^32
  auto ahead = [&](uint32_t words, uint32_t step) {
    return p + step + (lo + words < lo ? HBM_MARCH_MUL_HI : 0u);
  };

  for (; i < nvec; i += T) {
    if (i + (U - 1) * V < nvec) {
      u32x4 got[U] = {};
      if (CHECK >= 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) got[u] = base[i + u * V];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        one(i + u * V, ahead(u * ulo, u * up), got[u]);
    } else {  // the buffer's last, short group: one vector at a time
#pragma unroll 1
      for (uint32_t u = 0; u < U && i + u * V < nvec; ++u)
        one(i + u * V, ahead(u * ulo, u * up),
            CHECK >= 0 ? base[i + u * V] : u32x4{});
    }
    p = ahead(dlo, dp);
    lo += dlo;
  }
}

template <int PHASE, int U = HOST_LINK_UNROLL>
__global__ __launch_bounds__(HOST_LINK_THREADS) void link_pull(
    u32x4* __restrict__ base, uint32_t nvec, unsigned long long w0,
    unsigned long long byte0, HbmMarchResult* __restrict__ res, int pass) {
  link_span<PHASE, -1, U>(base, nvec, w0, byte0, res, pass, blockIdx.x,
                          gridDim.x);
}

template <int PHASE, int U = HOST_LINK_UNROLL>
__global__ __launch_bounds__(HOST_LINK_THREADS) void link_push(
    u32x4* __restrict__ base, uint32_t nvec, unsigned long long w0,
    unsigned long long byte0, HbmMarchResult* __restrict__ res, int pass) {
  link_span<-1, PHASE, U>(base, nvec, w0, byte0, res, pass, blockIdx.x,
                          gridDim.x);
}

// base[0, nvec_lo) is pulled by the even blocks, base[nvec_lo, nvec_lo +
// nvec_hi) pushed by the odd ones. The grid is even and at least 2.
template <int U = HOST_LINK_UNROLL>
__global__ __launch_bounds__(HOST_LINK_THREADS) void link_duplex(
    u32x4* __restrict__ base, uint32_t nvec_lo, uint32_t nvec_hi,
    unsigned long long w0, unsigned long long byte0,
    HbmMarchResult* __restrict__ res, int pass) {
  const uint32_t idx = blockIdx.x >> 1, per_role = gridDim.x >> 1;
  if ((blockIdx.x & 1) == 0)
    link_span<0, -1, U>(base, nvec_lo, w0, byte0, res, pass, idx, per_role);
  else
    link_span<-1, 0, U>(base + nvec_lo, nvec_hi, w0 + 4ull * nvec_lo,
                        byte0 + 16ull * nvec_lo, res, pass, idx, per_role);
}

using LinkStepFn = void (*)(u32x4*, uint32_t, unsigned long long,
                            unsigned long long, HbmMarchResult*, int);
static const LinkStepFn kLinkPull[3] = {link_pull<0>, link_pull<1>,
                                        link_pull<2>};
static const LinkStepFn kLinkPush[3] = {link_push<0>, link_push<1>,
                                        link_push<2>};

// blocks for `nvec` (>= 1) vectors, at most `cap`
static inline uint32_t host_link_blocks(uint32_t nvec,
                                        uint32_t cap = HOST_LINK_MAX_BLOCKS) {
  const uint32_t per_block = HOST_LINK_THREADS * HOST_LINK_UNROLL;
  const uint32_t blocks = (nvec + per_block - 1) / per_block;
  return blocks > cap ? cap : blocks;
}
