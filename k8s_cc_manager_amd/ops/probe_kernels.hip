// Probe kernels around the GEMMs: deterministic fills, the independent
// VALU fp32 reference GEMM, max-diff and checksum reductions, the LDS
// and HBM probes and the liveness kernel.
#pragma once

#include "gemm_common.hip"

typedef __attribute__((ext_vector_type(4))) float float4v;

// ---------------------------------------------------------------------------
// deterministic small-integer fill: values in {-2,-1,0,1}; products and
// K<=8192 partial sums stay exact in fp32 AND in the MFMA accumulator,
// so the MFMA and VALU paths must agree bitwise.
// ---------------------------------------------------------------------------
__global__ void fill_bf16_lcg(bf16* __restrict__ out, long n, uint32_t seed) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t x = (uint32_t)i * 1103515245u + seed * 747796405u + 12345u;
    x ^= x >> 16;
    x *= 2654435769u;
    int v = (int)((x >> 13) & 3u) - 2;  // {-2,-1,0,1}
    out[i] = (bf16)(float)v;
  }
}

// identical value sequence in OCP e4m3 (exact for {-2,-1,0,1}): lets
// the fp8 MFMA path be verified BITWISE against the same fp32 VALU
// reference the bf16 path uses.
__global__ void fill_fp8_lcg(unsigned char* __restrict__ out, long n,
                             uint32_t seed) {
  const unsigned char enc[4] = {0xC0, 0xB8, 0x00, 0x38};  // -2,-1,0,1
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t x = (uint32_t)i * 1103515245u + seed * 747796405u + 12345u;
    x ^= x >> 16;
    x *= 2654435769u;
    out[i] = enc[(x >> 13) & 3u];
  }
}

// ---------------------------------------------------------------------------
// VALU fp32 reference GEMM (independent ground truth; deliberately does
// NOT share tiling or fragment code with the MFMA path).
// One thread per C element, fp32 FMA chain over K.
// ---------------------------------------------------------------------------
__global__ void ref_gemm_f32(const bf16* __restrict__ A,
                             const bf16* __restrict__ Bt,
                             float* __restrict__ C, int M, int N, int K) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  int row = blockIdx.y * blockDim.y + threadIdx.y;
  if (row >= M || col >= N) return;
  float acc = 0.f;
  const bf16* a = A + (long)row * K;
  const bf16* b = Bt + (long)col * K;
  for (int k = 0; k < K; ++k) acc = fmaf((float)a[k], (float)b[k], acc);
  C[(long)row * N + col] = acc;
}

// ---------------------------------------------------------------------------
// MXFP4 leg: fills and the VALU reference (data convention in
// gemm_fp4.hip).
// ---------------------------------------------------------------------------
// n packed bytes, two e2m1 codes each, all 16 codes. Products are
// multiples of 2^-2 up to 36; with the scale fill below every term is a
// multiple of 2^-4 below 2^8, so partial sums up to K = 2048 fit 24
// bits in any order and the MFMA and VALU paths must agree bitwise.
__global__ void fill_fp4_lcg(unsigned char* __restrict__ out, long n,
                             uint32_t seed) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t x = (uint32_t)i * 1103515245u + seed * 747796405u + 12345u;
    x ^= x >> 16;
    x *= 2654435769u;
    out[i] = (unsigned char)(x >> 13);
  }
}

// E8M0 scale bytes in {126,127,128}: 2^-1, 2^0, 2^1
__global__ void fill_e8m0_lcg(unsigned char* __restrict__ out, long n,
                              uint32_t seed) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t x = (uint32_t)i * 1103515245u + seed * 747796405u + 12345u;
    x ^= x >> 16;
    x *= 2654435769u;
    out[i] = (unsigned char)(126u + ((x >> 13) % 3u));
  }
}

// twice the value of an e2m1 code, as an integer: 0,1,2,3,4,6,8,12
// with the sign of bit 3 (no hardware conversion instruction)
__device__ __forceinline__ int e2m1_times2(int code) {
  int e = (code >> 1) & 3, m = code & 1;
  int v = e ? (2 + m) << (e - 1) : m;
  return (code & 8) ? -v : v;
}

// VALU MXFP4 reference GEMM: one thread per C element; per 32-element
// block the products are summed in fp32 in k order, the block sum is
// scaled with ldexpf, and blocks are added in kb order.
__global__ void ref_gemm_mxfp4_f32(const unsigned char* __restrict__ A,
                                   const unsigned char* __restrict__ SA,
                                   const unsigned char* __restrict__ Bt,
                                   const unsigned char* __restrict__ SB,
                                   float* __restrict__ C, int M, int N,
                                   int K) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  int row = blockIdx.y * blockDim.y + threadIdx.y;
  if (row >= M || col >= N) return;
  const unsigned char* a = A + (long)row * (K >> 1);
  const unsigned char* b = Bt + (long)col * (K >> 1);
  const unsigned char* sa = SA + (long)row * (K >> 5);
  const unsigned char* sb = SB + (long)col * (K >> 5);
  float acc = 0.f;
  for (int kb = 0; kb < (K >> 5); ++kb) {
    float blk = 0.f;
    for (int j = 0; j < 16; ++j) {
      int ab = a[kb * 16 + j], bb = b[kb * 16 + j];
      blk += (float)(e2m1_times2(ab & 15) * e2m1_times2(bb & 15));
      blk += (float)(e2m1_times2(ab >> 4) * e2m1_times2(bb >> 4));
    }
    // blk holds 4x the block's dot product
    acc += ldexpf(blk, (int)sa[kb] + (int)sb[kb] - 254 - 2);
  }
  C[(long)row * N + col] = acc;
}

// ---------------------------------------------------------------------------
// MXFP6 leg: fill and the VALU reference (data convention in
// gemm_fp6.hip). fmt 2 = e2m3, 3 = e3m2.
// ---------------------------------------------------------------------------
// The codes of the magnitudes {0, 0.5, 1, 1.5, 2, 3} in each format
// (e2m3's 0.5 is a subnormal, e3m2's are all normals).
__device__ __forceinline__ unsigned fp6_exact_code(int fmt, unsigned idx) {
  return fmt == 2 ? 4u * idx : (0x12100E0C0800ull >> (8 * idx)) & 63u;
}

// nblocks 24-byte blocks of 32 codes drawn from those magnitudes with
// both signs (-0 included), one thread per block. With fill_e8m0_lcg's
// scale bytes every term is a multiple of 2^-4 of at most 36, so every
// partial sum fits 24 bits in any order while K * 576 < 2^24 (K up to
// 29,127) and the MFMA and VALU paths must agree bitwise. The other 52
// codes of each format are the tests' ground, not the gate's.
__global__ void fill_fp6_exact(uint32_t* __restrict__ out, long nblocks,
                               uint32_t seed, int fmt) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < nblocks; i += stride) {
    unsigned long long w[3] = {0, 0, 0};  // 64 bits hold 10 codes and 4 bits
    for (int j = 0; j < 32; ++j) {
      uint32_t x = (uint32_t)(i * 32 + j) * 1103515245u + seed * 747796405u +
                   12345u;
      x ^= x >> 16;
      x *= 2654435769u;
      unsigned r = (x >> 13) % 12u;
      unsigned long long code = fp6_exact_code(fmt, r % 6u) | (r / 6u) << 5;
      int bit = 6 * j;
      w[bit >> 6] |= code << (bit & 63);
      if ((bit & 63) > 58) w[(bit >> 6) + 1] |= code >> (64 - (bit & 63));
    }
    for (int q = 0; q < 3; ++q) {
      out[i * 6 + 2 * q] = (uint32_t)w[q];
      out[i * 6 + 2 * q + 1] = (uint32_t)(w[q] >> 32);
    }
  }
}

// the value of an fp6 code as a fixed-point integer: e2m3 times 8
// (0..60), e3m2 times 16 (0..448), with the sign of bit 5
template <int FMT>
__device__ __forceinline__ int fp6_fixed(unsigned code) {
  constexpr int MB = FMT == 2 ? 3 : 2;  // mantissa bits
  int e = (code >> MB) & (31 >> MB), m = code & ((1 << MB) - 1);
  int v = e ? ((1 << MB) + m) << (e - 1) : m;
  return (code & 32) ? -v : v;
}

// element j of a 24-byte block held as 6 dwords
__device__ __forceinline__ unsigned fp6_field(const uint32_t* blk, int j) {
  int bit = 6 * j, w = bit >> 5;
  unsigned long long two = blk[w];
  if (w < 5) two |= (unsigned long long)blk[w + 1] << 32;
  return (unsigned)(two >> (bit & 31)) & 63u;
}

// VALU MXFP6 reference GEMM: one thread per C element; per 32-element
// block the integer products are summed in fp32 in k order, the block
// sum is scaled with ldexpf, and blocks are added in kb order.
template <int FMT>
__global__ void ref_gemm_mxfp6_f32(const uint32_t* __restrict__ A,
                                   const unsigned char* __restrict__ SA,
                                   const uint32_t* __restrict__ Bt,
                                   const unsigned char* __restrict__ SB,
                                   float* __restrict__ C, int M, int N,
                                   int K) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  int row = blockIdx.y * blockDim.y + threadIdx.y;
  if (row >= M || col >= N) return;
  const int nkb = K >> 5;
  const uint32_t* a = A + (long)row * nkb * 6;
  const uint32_t* b = Bt + (long)col * nkb * 6;
  const unsigned char* sa = SA + (long)row * nkb;
  const unsigned char* sb = SB + (long)col * nkb;
  // the products carry the square of the fixed-point factor
  constexpr int kFixedLog2 = FMT == 2 ? 6 : 8;
  float acc = 0.f;
  for (int kb = 0; kb < nkb; ++kb) {
    float blk = 0.f;
    for (int j = 0; j < 32; ++j)
      blk += (float)(fp6_fixed<FMT>(fp6_field(a + kb * 6, j)) *
                     fp6_fixed<FMT>(fp6_field(b + kb * 6, j)));
    acc += ldexpf(blk, (int)sa[kb] + (int)sb[kb] - 254 - kFixedLog2);
  }
  C[(long)row * N + col] = acc;
}

// ---------------------------------------------------------------------------
// MXFP8 leg: fill and the VALU reference (data convention in
// gemm_mxfp8.hip). fmt 0 = e4m3, 1 = e5m2.
// ---------------------------------------------------------------------------
// n bytes drawn from the magnitudes {0, 0.5, 1, 1.5, 2, 3} with both
// signs (-0 included): e4m3 bytes 00 30 38 3c 40 44, e5m2 bytes 00 38 3c
// 3e 40 42. The exactness budget is fill_fp6_exact's: with
// fill_e8m0_lcg's scale bytes every term is a multiple of 2^-4 of at
// most 36, so every partial sum fits 24 bits in any order while
// K * 576 < 2^24 and the MFMA and VALU paths must agree bitwise. The
// other codes of each format are the tests' ground, not the gate's.
__global__ void fill_fp8_exact(unsigned char* __restrict__ out, long n,
                               uint32_t seed, int fmt) {
  const unsigned long long enc = fmt == 0 ? 0x44403C383000ull : 0x42403E3C3800ull;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t x = (uint32_t)i * 1103515245u + seed * 747796405u + 12345u;
    x ^= x >> 16;
    x *= 2654435769u;
    unsigned r = (x >> 13) % 12u;
    out[i] = (unsigned char)(((enc >> (8 * (r % 6u))) & 255u) | (r / 6u) << 7);
  }
}

// the value of an fp8 code: integer field extraction and ldexpf, no
// conversion instruction. e4m3: bias 7, NaN at S.1111.111, no Inf; e5m2:
// bias 15, Inf and NaN at exponent 31 (IEEE rules).
template <int FMT>
__device__ __forceinline__ float fp8_value(unsigned code) {
  constexpr int MB = FMT == 0 ? 3 : 2;  // mantissa bits
  constexpr int BIAS = FMT == 0 ? 7 : 15;
  const int e = (code >> MB) & (127 >> MB), m = code & ((1 << MB) - 1);
  float v;
  if (FMT == 0 && e == 15 && m == 7)
    v = __builtin_nanf("");
  else if (FMT == 1 && e == 31)
    v = m ? __builtin_nanf("") : __builtin_inff();
  else
    v = ldexpf((float)(e ? (1 << MB) + m : m), (e ? e : 1) - BIAS - MB);
  return (code & 128) ? -v : v;
}

// VALU MXFP8 reference GEMM: one thread per C element. Products are
// fp32 (two significands of at most 4 bits: exact); per 32-element block
// they are summed in k order, the block sum is scaled with ldexpf, and
// blocks are added in kb order. No fixed-point trick as for fp6: e5m2
// spans 2^-16 .. 57344.
template <int FA, int FB>
__global__ void ref_gemm_mxfp8_f32(const unsigned char* __restrict__ A,
                                   const unsigned char* __restrict__ SA,
                                   const unsigned char* __restrict__ Bt,
                                   const unsigned char* __restrict__ SB,
                                   float* __restrict__ C, int M, int N,
                                   int K) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  int row = blockIdx.y * blockDim.y + threadIdx.y;
  if (row >= M || col >= N) return;
  const int nkb = K >> 5;
  const unsigned char* a = A + (long)row * K;
  const unsigned char* b = Bt + (long)col * K;
  const unsigned char* sa = SA + (long)row * nkb;
  const unsigned char* sb = SB + (long)col * nkb;
  float acc = 0.f;
  for (int kb = 0; kb < nkb; ++kb) {
    float blk = 0.f;
    for (int j = 0; j < 32; ++j)
      blk += fp8_value<FA>(a[kb * 32 + j]) * fp8_value<FB>(b[kb * 32 + j]);
    acc += ldexpf(blk, (int)sa[kb] + (int)sb[kb] - 254);
  }
  C[(long)row * N + col] = acc;
}

// ---------------------------------------------------------------------------
// INT8 leg: fill, the VALU reference and the integer compare (data
// convention in gemm_i8.hip).
// ---------------------------------------------------------------------------
// n signed bytes over the full range -128..127: integer sums are exact
// for any data in any order, so there is no magnitude budget to keep.
// The LCG's byte is uniform: -128 occurs in both seeded fills at every
// gate dim (about n / 256 times).
__global__ void fill_i8_lcg(signed char* __restrict__ out, long n,
                            uint32_t seed) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t x = (uint32_t)i * 1103515245u + seed * 747796405u + 12345u;
    x ^= x >> 16;
    x *= 2654435769u;
    out[i] = (signed char)(unsigned char)(x >> 13);
  }
}

// VALU int8 reference GEMM: one thread per C element, sign-extended
// bytes, 32-bit multiply and add in k order. No MFMA, no dot instruction
// asked for. K * 2^14 <= 2^31 - 1 is the caller's to keep.
__global__ void ref_gemm_i8_i32(const signed char* __restrict__ A,
                                const signed char* __restrict__ Bt,
                                int* __restrict__ C, int M, int N, int K) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  int row = blockIdx.y * blockDim.y + threadIdx.y;
  if (row >= M || col >= N) return;
  const signed char* a = A + (long)row * K;
  const signed char* b = Bt + (long)col * K;
  int acc = 0;
  for (int k = 0; k < K; ++k) acc += (int)a[k] * (int)b[k];
  C[(long)row * N + col] = acc;
}

// max |x-y| over n int32 elements -> out[0] (pre-zeroed), the difference
// taken in 64 bits. max_abs_diff subtracts floats and cannot be used on
// reinterpreted integers.
__global__ void max_abs_diff_i32(const int* __restrict__ x,
                                 const int* __restrict__ y, long n,
                                 unsigned* out) {
  __shared__ unsigned smax[256];
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  unsigned m = 0;
  for (; i < n; i += stride) {
    long d = (long)x[i] - (long)y[i];
    unsigned a = (unsigned)(d < 0 ? -d : d);  // at most 2^32 - 1
    m = a > m ? a : m;
  }
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s && smax[threadIdx.x + s] > smax[threadIdx.x])
      smax[threadIdx.x] = smax[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(out, smax[0]);
}

// ---------------------------------------------------------------------------
// FP64 leg: fill, the VALU reference and the double compare (data
// convention in gemm_f64.hip).
// ---------------------------------------------------------------------------
// n integer-valued doubles with |v| <= 2^20 - 1: the hash's top 20 bits
// are the magnitude (the whole range, odd values included), bit 11 the
// sign. A product is an integer below 2^40 (beyond fp32's 24 bits), and
// while K * 2^40 <= 2^53 (K <= 8192) every partial sum in any order is an
// integer below 2^53: exact in fp64.
__global__ void fill_f64_exact(double* __restrict__ out, long n,
                               uint32_t seed) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t x = (uint32_t)i * 1103515245u + seed * 747796405u + 12345u;
    x ^= x >> 16;
    x *= 2654435769u;
    const double mag = (double)(x >> 12);
    out[i] = (x & 0x800u) ? -mag : mag;
  }
}

// VALU fp64 reference GEMM: one thread per C element, fma in double in k
// order (v_fmac_f64 in the shipped code). No MFMA: the VALU's fp64 FMA is
// a different datapath from the matrix core.
__global__ void ref_gemm_f64(const double* __restrict__ A,
                             const double* __restrict__ Bt,
                             double* __restrict__ C, int M, int N, int K) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  int row = blockIdx.y * blockDim.y + threadIdx.y;
  if (row >= M || col >= N) return;
  const double* a = A + (long)row * K;
  const double* b = Bt + (long)col * K;
  double acc = 0.0;
  for (int k = 0; k < K; ++k) acc = fma(a[k], b[k], acc);
  C[(long)row * N + col] = acc;
}

// max |x-y| over n doubles -> out[0] (pre-zeroed), for the report's float
// field. The difference and the reduction are in double and compare by
// value (+0 equals -0); a NaN on either side counts as infinity. The
// conversion to float clamps any nonzero difference up to the smallest
// normal float, so that it can neither round nor be flushed to 0.0f.
__global__ void max_abs_diff_f64(const double* __restrict__ x,
                                 const double* __restrict__ y, long n,
                                 float* out) {
  __shared__ double smax[256];
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  double m = 0.0;
  for (; i < n; i += stride) {
    double d = fabs(x[i] - y[i]);
    if (!(d == d)) d = __builtin_huge_val();
    m = d > m ? d : m;
  }
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s && smax[threadIdx.x + s] > smax[threadIdx.x])
      smax[threadIdx.x] = smax[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && smax[0] > 0.0) {
    float f = (float)smax[0];
    if (!(f >= 1.17549435e-38f)) f = 1.17549435e-38f;
    // fp32 max via atomicMax on the bit pattern (values are > 0)
    atomicMax((unsigned int*)out, __float_as_uint(f));
  }
}

// ---------------------------------------------------------------------------
// Sparse leg: fill and the VALU reference (data convention in
// gemm_sp24.hip and docs/KERNELS.md, "Sparse leg"). The compare is
// max_abs_diff.
// ---------------------------------------------------------------------------
// The six legal index nibbles (pos0 in bits 1:0 below pos1 in bits 3:2), one
// per 4 bits: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).
constexpr uint32_t kSp24Nibbles = 0xED9C84u;

// nbytes index bytes of Am and the 4 * nbytes kept values of Ac they
// govern. Values: the magnitudes {0, 0.5, 1, 1.5, 2, 3} with both signs
// (-0 included), bf16 bits 0000 3f00 3f80 3fc0 4000 4040; nibbles: drawn
// from the six legal ones. With am == nullptr it fills 4 * nbytes values
// alone: the leg's dense B, from the same set. A product is then a
// multiple of 2^-2 of at most 9 and a sum has K/2 terms, so every partial
// sum fits 24 bits in any order while (K/2) * 36 < 2^24, and the SMFMAC
// and VALU paths must agree bitwise.
__global__ void fill_sp24_exact(bf16* __restrict__ vals,
                                unsigned char* __restrict__ am, long nbytes,
                                uint32_t seed) {
  const unsigned long long mag = 0x404040003FC03F80ull;  // 1, 1.5, 2, 3
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < nbytes; i += stride) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t x = (uint32_t)(4 * i + j) * 1103515245u + seed * 747796405u +
                   12345u;
      x ^= x >> 16;
      x *= 2654435769u;
      const unsigned r = (x >> 13) % 12u, m = r % 6u;
      const unsigned bits = m == 0   ? 0u
                            : m == 1 ? 0x3F00u
                                     : (unsigned)(mag >> (16 * (m - 2))) & 0xFFFFu;
      const unsigned short h = (unsigned short)(bits | (r / 6u) << 15);
      vals[4 * i + j] = __builtin_bit_cast(bf16, h);
    }
    if (am) {
      uint32_t x =
          (uint32_t)i * 1103515245u + (seed + 64u) * 747796405u + 12345u;
      x ^= x >> 16;
      x *= 2654435769u;
      const unsigned r = (x >> 13) % 36u;
      am[i] = (unsigned char)(((kSp24Nibbles >> (4 * (r % 6u))) & 15u) |
                              ((kSp24Nibbles >> (4 * (r / 6u))) & 15u) << 4);
    }
  }
}

// VALU 2:4 reference GEMM: one thread per C element. The nibble of every
// group is decoded with integer shifts, literally (an illegal nibble reads
// the positions it names); fp32 fma in k order (a product of two bf16 is
// exact in fp32, so fusing changes nothing). No MFMA.
__global__ void ref_gemm_sp24_f32(const bf16* __restrict__ Ac,
                                  const unsigned char* __restrict__ Am,
                                  const bf16* __restrict__ Bt,
                                  float* __restrict__ C, int M, int N, int K) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  int row = blockIdx.y * blockDim.y + threadIdx.y;
  if (row >= M || col >= N) return;
  const bf16* a = Ac + (long)row * (K / 2);
  const unsigned char* am = Am + (long)row * (K / 8);
  const bf16* b = Bt + (long)col * K;
  float acc = 0.f;
  for (int g = 0; g < K / 4; ++g) {
    const unsigned nib = (am[g >> 1] >> (4 * (g & 1))) & 15u;
    acc = fmaf((float)a[2 * g], (float)b[4 * g + (nib & 3u)], acc);
    acc = fmaf((float)a[2 * g + 1], (float)b[4 * g + (nib >> 2)], acc);
  }
  C[(long)row * N + col] = acc;
}

// ---------------------------------------------------------------------------
// FP16 leg: fill and the VALU reference (data convention in gemm_f16.hip
// and docs/KERNELS.md, "FP16 leg"). The compare is max_abs_diff.
// ---------------------------------------------------------------------------
// The row exponent e(r) in -22..13 of fill_f16_exact: r times a unit of
// the integers mod 36, mod 36, so all 36 values occur inside any 36
// consecutive rows (and so inside any 128). The unit follows the seed:
// 5 for the leg's A (seed 1), 23 for its B (seed 7).
__device__ __forceinline__ int f16_row_exponent(long r, uint32_t seed) {
  const unsigned char units[12] = {1, 5, 7, 11, 13, 17, 19, 23, 25, 29, 31, 35};
  return (int)((r * units[seed % 12u]) % 36) - 22;
}

// rows x cols binary16 codes, element (r, k) = (j/4) * 2^e(r): j uniform
// in -31..31 from the LCG, whose 64th outcome is the code 0x8000 (-0).
// 31/4 * 2^13 = 63488 is finite and 1/4 * 2^-22 = 2^-24 is the smallest
// subnormal, so every element is representable: rows with e(r) < -12 hold
// subnormals (below -16 nothing else), and the exponent field runs from 0
// to 30 on both operands.
// Exactness budget at gemm_f16.hip: bitwise while K <= 16384.
__global__ void fill_f16_exact(unsigned short* __restrict__ out, int rows,
                               int cols, uint32_t seed) {
  const long n = (long)rows * cols;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    uint32_t x = (uint32_t)i * 1103515245u + seed * 747796405u + 12345u;
    x ^= x >> 16;
    x *= 2654435769u;
    const unsigned r = (x >> 13) & 63u;
    unsigned code = 0x8000u;  // r == 63: -0
    if (r != 63u) {
      const int j = (int)r - 31;
      const unsigned m = (unsigned)(j < 0 ? -j : j);  // value m * 2^xp
      const int xp = f16_row_exponent(i / cols, seed) - 2;
      code = 0;
      if (m) {
        const int p = 31 - __builtin_clz(m);  // m = 1.f * 2^p
        const int biased = xp + p + 15;
        code = biased >= 1 ? (unsigned)biased << 10 | ((m << (10 - p)) & 0x3FFu)
                           : m << (xp + 24);  // subnormal: units of 2^-24
      }
      if (j < 0) code |= 0x8000u;
    }
    out[i] = (unsigned short)code;
  }
}

// the value of a binary16 code: integer field extraction and ldexpf, no
// conversion instruction. Bias 15, subnormals at exponent 0, Inf and NaN
// at exponent 31 (IEEE rules).
__device__ __forceinline__ float f16_value(unsigned code) {
  const int e = (code >> 10) & 31, m = code & 1023;
  float v;
  if (e == 31)
    v = m ? __builtin_nanf("") : __builtin_inff();
  else
    v = ldexpf((float)(e ? 1024 + m : m), (e ? e : 1) - 25);
  return (code & 0x8000u) ? -v : v;
}

// VALU fp16 reference GEMM: one thread per C element, fp32 fma in k order
// (a product of two 11-bit significands is exact in fp32, so fusing
// changes nothing). No MFMA.
__global__ void ref_gemm_f16_f32(const unsigned short* __restrict__ A,
                                 const unsigned short* __restrict__ Bt,
                                 float* __restrict__ C, int M, int N, int K) {
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  int row = blockIdx.y * blockDim.y + threadIdx.y;
  if (row >= M || col >= N) return;
  const unsigned short* a = A + (long)row * K;
  const unsigned short* b = Bt + (long)col * K;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(f16_value(a[k]), f16_value(b[k]), acc);
  C[(long)row * N + col] = acc;
}

// max |x-y| reduction over n elements -> out[0] (pre-zeroed)
__global__ void max_abs_diff(const float* __restrict__ x,
                             const float* __restrict__ y, long n,
                             float* out) {
  __shared__ float smax[256];
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  float m = 0.f;
  for (; i < n; i += stride) {
    float d = fabsf(x[i] - y[i]);
    m = fmaxf(m, d);
  }
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // fp32 max via atomicMax on the bit pattern (values are >= 0)
    atomicMax((unsigned int*)out, __float_as_uint(smax[0]));
  }
}

// FNV-1a style checksum of a float buffer -> 64-bit xor-fold (order
// independent via per-element mix, so concurrent blocks are fine).
__global__ void checksum_f32(const float* __restrict__ x, long n,
                             unsigned long long* out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  unsigned long long h = 0;
  for (; i < n; i += stride) {
    unsigned long long v = (unsigned long long)__float_as_uint(x[i]) + 0x9e3779b97f4a7c15ull * (unsigned long long)(i + 1);
    v ^= v >> 33; v *= 0xff51afd7ed558ccdull; v ^= v >> 33;
    h ^= v;
  }
  // xor-reduce wave -> block (LDS) -> ONE atomic per block. The first
  // version did one atomic per wave: 4096 serialized atomicXors on a
  // single address cost ~40 us — more than the whole hash sweep
  // (bench kernel trace, profiles/bench_kernel_stats.csv).
  for (int off = 32; off > 0; off >>= 1)
    h ^= __shfl_down(h, off, 64);
  __shared__ unsigned long long partial[4];
  if ((threadIdx.x & 63) == 0) partial[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long b = partial[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) b ^= partial[w];
    atomicXor(out, b);
  }
}

// ---------------------------------------------------------------------------
// LDS probe: rotating write/read patterns across a 64 KiB LDS slab per
// workgroup; validates every cell and measures aggregate LDS traffic.
// ---------------------------------------------------------------------------
constexpr int LDS_PROBE_WORDS = 16384;  // 64 KiB of uint32 per workgroup

__global__ void lds_probe(uint32_t* __restrict__ fail_count, int rounds) {
  __shared__ uint32_t slab[LDS_PROBE_WORDS];
  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;
  uint32_t local_fail = 0;
  for (int r = 0; r < rounds; ++r) {
    uint32_t salt = 0x9e3779b9u * (r + 1) + blockIdx.x;
    for (int i = tid; i < LDS_PROBE_WORDS; i += nthreads)
      slab[i] = (uint32_t)i * 2654435769u + salt;
    __syncthreads();
    // read back with a different (conflict-heavy, bank-rotating) stride
    for (int i = tid; i < LDS_PROBE_WORDS; i += nthreads) {
      int j = (i * 33 + r) & (LDS_PROBE_WORDS - 1);
      uint32_t want = (uint32_t)j * 2654435769u + salt;
      if (slab[j] != want) ++local_fail;
    }
    __syncthreads();
  }
  if (local_fail) atomicAdd(fail_count, local_fail);
}

// ---------------------------------------------------------------------------
// HBM probe: float4 streaming copy (the measured-best pattern, ~79% of
// the 8 TB/s peak per MI355X_MICROARCH.md) + spot validation.
// ---------------------------------------------------------------------------
__global__ void hbm_copy_f4(const float4v* __restrict__ src,
                            float4v* __restrict__ dst, long n4) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

// Minimal liveness check: a real kernel launch must complete. Used as
// the post-reset boot-wait gate (a device can answer property queries
// from cached driver state while its command processor is wedged).
extern "C" __global__ void liveness_kernel(int* out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out = 0x600D;
}
