// Layout probe for v_mfma_scale_f32_32x32x64_f8f6f4 operand fragments.
// Single wave computes one 32x32x64 tile with candidate byte->k maps;
// host compares against a CPU reference to identify the real layout.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>

typedef __attribute__((ext_vector_type(8))) int v8i;
typedef __attribute__((ext_vector_type(16))) float v16f;

// candidate L: byte j of lane l maps to k = kmap(l, j)
__device__ int kmap(int cand, int l, int j) {
  switch (cand) {
    case 0: return (l >> 5) * 32 + j;                        // 32 consecutive
    case 1: return 16 * (j >> 3) + (l >> 5) * 8 + (j & 7);   // 4 chained x16
    case 2: return (j >> 3) * 8 + (l >> 5) * 32 + (j & 7);   // blocks of 8? (=c0)
    case 3: return (l >> 5) * 8 + (j >> 3) * 16 + (j & 7);   // alt chain order
    default: return j;
  }
}

__global__ void probe(const char* A, const char* B, float* C, int cand) {
  int l = threadIdx.x;
  unsigned char abuf[32], bbuf[32];
  for (int j = 0; j < 32; ++j) {
    int k = kmap(cand, l, j);
    abuf[j] = A[(l & 31) * 64 + k];
    bbuf[j] = B[(l & 31) * 64 + k];
  }
  v8i a = *(v8i*)abuf;
  v8i b = *(v8i*)bbuf;
  v16f c = {};
  c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
      a, b, c, 0, 0, 0, 0x7F7F7F7Fu, 0, 0x7F7F7F7Fu);
  for (int r = 0; r < 16; ++r) {
    int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    int col = l & 31;
    C[row * 32 + col] = c[r];
  }
}

static float fp8_to_f(unsigned char v) {
  // e4m3fn decode
  int s = v >> 7, e = (v >> 3) & 0xF, m = v & 7;
  if (e == 0xF && m == 7) return nanf("");
  float val;
  if (e == 0) val = ldexpf((float)m / 8.0f, -6);
  else val = ldexpf(1.0f + (float)m / 8.0f, e - 7);
  return s ? -val : val;
}

// ---------------------------------------------------------------------------
// fp6 operands (cbsz/blgp 2 = e2m3, 3 = e3m2): 6-register tuples, 32
// elements of 6 bits per lane, one E8M0 scale byte per lane. The host
// builds the per-lane fragments; the kernel only issues the instruction.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(6))) int v6i;

template <int FMT>
__global__ void probe6(const int* fa, const int* fb, const int* sa,
                       const int* sb, float* C) {
  int l = threadIdx.x;
  v6i a, b;
  for (int r = 0; r < 6; ++r) {
    a[r] = fa[l * 6 + r];
    b[r] = fb[l * 6 + r];
  }
  int sca = sa[l], scb = sb[l];
  v16f c = {};
  if (FMT == 2)
    asm volatile(
        "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 "
        "op_sel:[0,0,0] op_sel_hi:[0,0,0] cbsz:2 blgp:2"
        : "+v"(c)
        : "v"(a), "v"(b), "v"(sca), "v"(scb));
  else
    asm volatile(
        "v_mfma_scale_f32_32x32x64_f8f6f4 %0, %1, %2, %0, %3, %4 "
        "op_sel:[0,0,0] op_sel_hi:[0,0,0] cbsz:3 blgp:3"
        : "+v"(c)
        : "v"(a), "v"(b), "v"(sca), "v"(scb));
  asm volatile("s_nop 15\ns_nop 15\ns_nop 2" :::);
  for (int r = 0; r < 16; ++r) {
    int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    C[row * 32 + (l & 31)] = c[r];
  }
}

static double fp6_to_d(int fmt, int code) {
  int s = code >> 5, e, m;
  double v;
  if (fmt == 2) {  // e2m3, bias 1
    e = (code >> 3) & 3, m = code & 7;
    v = e ? ldexp(1.0 + m / 8.0, e - 1) : m / 8.0;
  } else {  // e3m2, bias 3
    e = (code >> 2) & 7, m = code & 3;
    v = e ? ldexp(1.0 + m / 4.0, e - 3) : ldexp(m / 4.0, -2);
  }
  return s ? -v : v;
}

// slot j of a lane's 32: bits 6j..6j+5 of the 192-bit little-endian tuple
static void put6(int* frag, int j, int code) {
  int bit = 6 * j;
  unsigned long long v = (unsigned long long)(code & 63) << (bit & 31);
  frag[bit >> 5] |= (int)(unsigned)v;
  if ((bit & 31) > 26) frag[(bit >> 5) + 1] |= (int)(unsigned)(v >> 32);
}

// candidate maps: slot j of lane half h -> k of the instruction's 64
static int kmap6(int cand, int h, int j) {
  if (cand == 0) return 32 * h + j;              // the e2m1 pattern
  return 32 * (j >> 4) + 16 * h + (j & 15);      // the e4m3 pattern
}

struct Dev6 {
  int *fa, *fb, *sa, *sb;
  float* c;
};

static void run6(int fmt, const Dev6& d, const int* fa, const int* fb,
                 const int* sa, const int* sb, float* out) {
  (void)hipMemcpy(d.fa, fa, 64 * 6 * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(d.fb, fb, 64 * 6 * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(d.sa, sa, 64 * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(d.sb, sb, 64 * 4, hipMemcpyHostToDevice);
  (void)hipMemset(d.c, 0xFF, 32 * 32 * 4);
  if (fmt == 2)
    hipLaunchKernelGGL(probe6<2>, dim3(1), dim3(64), 0, 0, d.fa, d.fb, d.sa,
                       d.sb, d.c);
  else
    hipLaunchKernelGGL(probe6<3>, dim3(1), dim3(64), 0, 0, d.fa, d.fb, d.sa,
                       d.sb, d.c);
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    printf("fp6 probe: %s\n", hipGetErrorString(e));
    exit(1);
  }
  (void)hipMemcpy(out, d.c, 32 * 32 * 4, hipMemcpyDeviceToHost);
}

static void probe_fp6(int fmt) {
  Dev6 d;
  (void)hipMalloc(&d.fa, 64 * 6 * 4);
  (void)hipMalloc(&d.fb, 64 * 6 * 4);
  (void)hipMalloc(&d.sa, 64 * 4);
  (void)hipMalloc(&d.sb, 64 * 4);
  (void)hipMalloc(&d.c, 32 * 32 * 4);
  const int one = fmt == 2 ? 8 : 12;  // the code of 1.0
  float out[32 * 32];
  int fa[64 * 6], fb[64 * 6], sa[64], sb[64];

  // 1. candidates: every k a distinct-ish random code, the two K blocks
  // of every row distinct scales, against a double reference
  int A[32][64], B[32][64], SA[32][2], SB[32][2];
  for (int r = 0; r < 32; ++r) {
    for (int k = 0; k < 64; ++k) A[r][k] = rand() & 63, B[r][k] = rand() & 63;
    SA[r][0] = 126 + rand() % 3, SA[r][1] = 129 + rand() % 3;
    SB[r][0] = 125 + rand() % 3, SB[r][1] = 122 + rand() % 3;
  }
  for (int cand = 0; cand < 2; ++cand) {
    __builtin_memset(fa, 0, sizeof(fa));
    __builtin_memset(fb, 0, sizeof(fb));
    for (int l = 0; l < 64; ++l) {
      for (int j = 0; j < 32; ++j) {
        put6(fa + l * 6, j, A[l & 31][kmap6(cand, l >> 5, j)]);
        put6(fb + l * 6, j, B[l & 31][kmap6(cand, l >> 5, j)]);
      }
      sa[l] = SA[l & 31][l >> 5];
      sb[l] = SB[l & 31][l >> 5];
    }
    run6(fmt, d, fa, fb, sa, sb, out);
    double maxerr = 0, maxref = 0;
    for (int m = 0; m < 32; ++m)
      for (int n = 0; n < 32; ++n) {
        double ref = 0;
        for (int k = 0; k < 64; ++k)
          ref += ldexp(fp6_to_d(fmt, A[m][k]) * fp6_to_d(fmt, B[n][k]),
                       SA[m][k >> 5] + SB[n][k >> 5] - 254);
        maxerr = fmax(maxerr, fabs(out[m * 32 + n] - ref));
        maxref = fmax(maxref, fabs(ref));
      }
    printf("fmt %d cand %d (%s): max_abs_err = %g of max |ref| %g %s\n", fmt,
           cand, cand ? "2 x 16 per K block" : "32 consecutive", maxerr,
           maxref, maxerr <= maxref * 1e-6 ? "<-- MATCH" : "");
  }

  // 2. pairing: A lane (r, ha) holds 1.0 in slot r only, B lane (c, hb)
  // in slot c only, unit scales: C[r][c] = 1 where the two slots meet
  for (int ha = 0; ha < 2; ++ha)
    for (int hb = 0; hb < 2; ++hb) {
      __builtin_memset(fa, 0, sizeof(fa));
      __builtin_memset(fb, 0, sizeof(fb));
      for (int r = 0; r < 32; ++r) {
        put6(fa + (ha * 32 + r) * 6, r, one);
        put6(fb + (hb * 32 + r) * 6, r, one);
      }
      for (int l = 0; l < 64; ++l) sa[l] = sb[l] = 127;
      run6(fmt, d, fa, fb, sa, sb, out);
      int identity = 1, nz = 0;
      for (int r = 0; r < 32; ++r)
        for (int c = 0; c < 32; ++c) {
          float want = (r == c && ha == hb) ? 1.f : 0.f;
          if (out[r * 32 + c] != want) identity = 0;
          if (out[r * 32 + c] != 0.f) ++nz;
        }
      printf("fmt %d pairing ha=%d hb=%d: %s (%d nonzero)\n", fmt, ha, hb,
             identity ? "slot j of half h meets slot j of half h only"
                      : "NOT the identity",
             nz);
      if (!identity)
        for (int r = 0; r < 32; ++r)
          for (int c = 0; c < 32; ++c)
            if (out[r * 32 + c] != 0.f)
              printf("  A slot %d x B slot %d = %g\n", r, c, out[r * 32 + c]);
    }

  // 3. scale blocks: the side under test holds 1.0 in slot r of lane
  // (r, h) only and scales 2 (half 0) / 8 (half 1); the other side is
  // all ones with scales 1 (half 0) / 16 (half 1). The result for slot r
  // is own-scale x other-scale, which names both lanes that scaled it.
  for (int side = 0; side < 2; ++side)
    for (int h = 0; h < 2; ++h) {
      int* ft = side ? fb : fa;
      int* fo = side ? fa : fb;
      __builtin_memset(ft, 0, sizeof(fa));
      __builtin_memset(fo, 0, sizeof(fa));
      for (int r = 0; r < 32; ++r) put6(ft + (h * 32 + r) * 6, r, one);
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 32; ++j) put6(fo + l * 6, j, one);
      for (int l = 0; l < 64; ++l) {
        (side ? sb : sa)[l] = l < 32 ? 128 : 130;
        (side ? sa : sb)[l] = l < 32 ? 127 : 131;
      }
      run6(fmt, d, fa, fb, sa, sb, out);
      printf("fmt %d scales of %c half %d, slots 0..31:", fmt, side ? 'B' : 'A',
             h);
      for (int r = 0; r < 32; ++r)
        printf(" %g", side ? out[0 * 32 + r] : out[r * 32 + 0]);
      printf("\n");
    }
}

int main() {
  srand(42);
  unsigned char hA[32 * 64], hB[32 * 64];
  // small integers: bytes for {-2,-1,0,1}
  const unsigned char enc[4] = {0xC0, 0xB8, 0x00, 0x38};
  for (int i = 0; i < 32 * 64; ++i) {
    hA[i] = enc[rand() & 3];
    hB[i] = enc[rand() & 3];
  }
  float ref[32 * 32];
  for (int m = 0; m < 32; ++m)
    for (int n = 0; n < 32; ++n) {
      float acc = 0;
      for (int k = 0; k < 64; ++k)
        acc += fp8_to_f(hA[m * 64 + k]) * fp8_to_f(hB[n * 64 + k]);
      ref[m * 32 + n] = acc;
    }
  char *dA, *dB;
  float* dC;
  (void)hipMalloc(&dA, sizeof(hA));
  (void)hipMalloc(&dB, sizeof(hB));
  (void)hipMalloc(&dC, 32 * 32 * 4);
  (void)hipMemcpy(dA, hA, sizeof(hA), hipMemcpyHostToDevice);
  (void)hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
  for (int cand = 0; cand < 4; ++cand) {
    (void)hipMemset(dC, 0, 32 * 32 * 4);
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dC, cand);
    (void)hipDeviceSynchronize();
    float out[32 * 32];
    (void)hipMemcpy(out, dC, sizeof(out), hipMemcpyDeviceToHost);
    float maxerr = 0;
    for (int i = 0; i < 32 * 32; ++i)
      maxerr = fmaxf(maxerr, fabsf(out[i] - ref[i]));
    printf("cand %d: max_abs_err = %g %s\n", cand, maxerr,
           maxerr == 0 ? "<-- EXACT" : "");
  }
  // fp6: candidates, slot pairing and scale blocks, both formats
  probe_fp6(2);
  probe_fp6(3);
  return 0;
}
