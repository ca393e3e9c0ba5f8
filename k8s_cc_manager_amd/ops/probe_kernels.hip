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
