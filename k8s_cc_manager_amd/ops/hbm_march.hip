// HBM march: a verified write / read-back march over an explicit window
// of VRAM that ends with the window zeroed, and the zeros checked.
//
//   march_step<CHECK, WRITE>  one pass over one chunk: every 16-byte vector
//                             is read and compared with phase CHECK, then
//                             overwritten with phase WRITE (either may be
//                             -1, "none"). The write happens whether or not
//                             the compare matched.
//   march_poison              one lane flips bit 0 of one word: a wrong
//                             number for the detector's tests, never a fault.
//
// Pattern. The window is addressed by a 64-bit logical word index
// w = (origin + byte offset in window) / 4; with lo = w mod 2^32 and
// hi = w >> 32,
//   p(w) = lo * 2654435769 + hi * 2246822519 + 0x5EED0001   (mod 2^32)
// (lds_probe's arithmetic with a high word). Both multipliers are odd, so
// flipping any single bit k of w moves p by an odd multiple of
// 2^(k mod 32): two addresses one decoder line apart never hold the same
// word. Phase 0 holds p, phase 1 holds ~p, phase 2 holds zero.
//
// Shape: grid-stride over 16-byte vectors, HBM_MARCH_UNROLL independent
// vectors in flight per lane, the grid sized by the caller from the CU
// count. Per stride a block owns 16 contiguous KiB (a lane's vectors are
// 4 KiB apart); with a lane's vectors a whole grid apart instead, the
// check-and-write step ran 22 % slower (docs/KERNELS.md, "HBM march").
// A chunk is at most 2^28 words (1 GiB), so every in-chunk index
// is 32-bit; only w0, the chunk's first logical word, is 64-bit. w is a
// multiple of 4 at every vector (origin is a multiple of 16), so the four
// words of a vector share hi. Along the stride the pattern advances by
// adds: lo is linear mod 2^32, and hi's multiplier is added once when lo
// wraps.
//
// The clean path does no atomics. A lane that sees a mismatch adds the
// number of wrong words to a 64-bit count, lowers a 64-bit "first bad
// byte offset" (atomicMin, all ones when clean) and, while the count it
// drew is below HBM_MARCH_RECORDS, writes {offset, expected, got, pass}
// into the slot of that number; past 16 it only counts.
#pragma once

#include "probe_kernels.hip"

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr uint32_t HBM_MARCH_MUL_LO = 2654435769u;
constexpr uint32_t HBM_MARCH_MUL_HI = 2246822519u;
constexpr uint32_t HBM_MARCH_SALT = 0x5EED0001u;
constexpr int HBM_MARCH_RECORDS = 16;
constexpr int HBM_MARCH_UNROLL = 4;    // vectors in flight per lane
constexpr int HBM_MARCH_THREADS = 256;
constexpr unsigned long long HBM_MARCH_MAX_CHUNK = 1ull << 30;  // bytes

// The device result block of one march (HbmCtx holds it).
struct HbmMarchResult {
  unsigned long long mismatch_words;
  unsigned long long first_bad_offset;  // byte offset in window; ~0 = none
  unsigned long long bad_offset[HBM_MARCH_RECORDS];
  uint32_t bad_expected[HBM_MARCH_RECORDS];
  uint32_t bad_got[HBM_MARCH_RECORDS];
  int bad_pass[HBM_MARCH_RECORDS];
};

__host__ __device__ inline uint32_t hbm_march_pattern(unsigned long long w) {
  return (uint32_t)w * HBM_MARCH_MUL_LO +
         (uint32_t)(w >> 32) * HBM_MARCH_MUL_HI + HBM_MARCH_SALT;
}

// the four words of the vector whose first word holds p, in phase PHASE
template <int PHASE>
__device__ __forceinline__ u32x4 hbm_march_vec(uint32_t p) {
  if (PHASE == 2) return u32x4{0u, 0u, 0u, 0u};
  u32x4 v = {p, p + HBM_MARCH_MUL_LO, p + 2u * HBM_MARCH_MUL_LO,
             p + 3u * HBM_MARCH_MUL_LO};
  return PHASE == 1 ? ~v : v;
}

// slow path: `off` is the window byte offset of the vector's first word
__device__ inline void hbm_march_mismatch(HbmMarchResult* res,
                                          unsigned long long off, u32x4 want,
                                          u32x4 got, int pass) {
  unsigned cnt = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) cnt += want[j] != got[j];
  unsigned long long slot =
      atomicAdd(&res->mismatch_words, (unsigned long long)cnt);
  bool first = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (want[j] == got[j]) continue;
    if (first) atomicMin(&res->first_bad_offset, off + 4ull * j);
    first = false;
    if (slot < (unsigned long long)HBM_MARCH_RECORDS) {
      res->bad_offset[slot] = off + 4ull * j;
      res->bad_expected[slot] = want[j];
      res->bad_got[slot] = got[j];
      res->bad_pass[slot] = pass;
    }
    ++slot;
  }
}

// base: the chunk, nvec 16-byte vectors (<= 2^26). w0: logical word index
// of its first word. byte0: window byte offset of its first word (what
// the records carry). `pass` is copied into the records.
template <int CHECK, int WRITE>
__global__ __launch_bounds__(HBM_MARCH_THREADS) void march_step(
    u32x4* __restrict__ base, uint32_t nvec, unsigned long long w0,
    unsigned long long byte0, HbmMarchResult* __restrict__ res, int pass) {
  static_assert(CHECK >= -1 && CHECK <= 2 && WRITE >= -1 && WRITE <= 2 &&
                    (CHECK >= 0 || WRITE >= 0),
                "phases are -1..2, not both none");
  constexpr int U = HBM_MARCH_UNROLL;
  constexpr uint32_t V = HBM_MARCH_THREADS;  // vectors between a lane's U
  // a block's U * V vectors of one stride are contiguous (16 KiB)
  const uint32_t T = gridDim.x * (U * V);  // vectors per stride
  uint32_t i = blockIdx.x * (U * V) + threadIdx.x;
  const unsigned long long w = w0 + 4ull * i;
  uint32_t lo = (uint32_t)w;
  uint32_t p = hbm_march_pattern(w);  // the one multiply per lane
  const uint32_t dlo = 4u * T;        // words per stride (< 2^32)
  const uint32_t dp = dlo * HBM_MARCH_MUL_LO;
  constexpr uint32_t ulo = 4u * V;
  constexpr uint32_t up = ulo * HBM_MARCH_MUL_LO;

  auto one = [&](uint32_t idx, uint32_t pv, u32x4 got) {
    if (CHECK >= 0) {
      const u32x4 want = hbm_march_vec<CHECK>(pv);
      const u32x4 d = got ^ want;
      if (d[0] | d[1] | d[2] | d[3])
        hbm_march_mismatch(res, byte0 + 16ull * idx, want, got, pass);
    }
    if (WRITE >= 0) base[idx] = hbm_march_vec<WRITE>(pv);
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
    } else {  // the chunk's last, short group: one vector at a time
#pragma unroll 1
      for (uint32_t u = 0; u < U && i + u * V < nvec; ++u)
        one(i + u * V, ahead(u * ulo, u * up),
            CHECK >= 0 ? base[i + u * V] : u32x4{});
    }
    p = ahead(dlo, dp);
    lo += dlo;
  }
}

__global__ void march_poison(uint32_t* word) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *word ^= 1u;
}

// [check + 1][write + 1]; cc_hbm_step reaches every combination, the leg
// uses <-1,0>, <0,1>, <1,2>, <2,-1>.
using MarchStepFn = void (*)(u32x4*, uint32_t, unsigned long long,
                             unsigned long long, HbmMarchResult*, int);
static const MarchStepFn kMarchStep[4][4] = {
    {nullptr, march_step<-1, 0>, march_step<-1, 1>, march_step<-1, 2>},
    {march_step<0, -1>, march_step<0, 0>, march_step<0, 1>, march_step<0, 2>},
    {march_step<1, -1>, march_step<1, 0>, march_step<1, 1>, march_step<1, 2>},
    {march_step<2, -1>, march_step<2, 0>, march_step<2, 1>, march_step<2, 2>},
};
