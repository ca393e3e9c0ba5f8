// Layout probe for the gfx950 bf16 SMFMACs (v_smfmac_f32_32x32x32_bf16,
// v_smfmac_f32_16x16x64_bf16): which B element of which lane meets each
// compressed A slot, and which 2-bit field of the index register steers
// it, per abid. One wave, register operands built on the host: a wrong
// guess gives a wrong number, never a fault.
//   hipcc --offload-arch=gfx950 -O2 sp24_layout_probe.hip -o sp24_layout_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) __bf16 bf16x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// a: 64 x 8 bf16, b: 64 x 16 bf16, idx: 64 ints, C: 32x32 (SHAPE 0) or
// 16x16 (SHAPE 1) floats, row-major
template <int SHAPE, int ABID>
__global__ void probe(const bf16x8* a, const bf16x16* b, const int* idx,
                      float* C) {
  const int l = threadIdx.x;
  if constexpr (SHAPE == 0) {
    f32x16 c = {};
    c = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a[l], b[l], c, idx[l], 0, ABID);
    for (int r = 0; r < 16; ++r)
      C[((r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31)] = c[r];
  } else {
    f32x4 c = {};
    c = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a[l], b[l], c, idx[l], 0, ABID);
    for (int r = 0; r < 4; ++r) C[(4 * (l >> 4) + r) * 16 + (l & 15)] = c[r];
  }
}

static unsigned short bf16_bits(float v) {  // small integers: exact
  unsigned u;
  memcpy(&u, &v, 4);
  return (unsigned short)(u >> 16);
}

struct Dev {
  unsigned short *a, *b;
  int* idx;
  float* c;
};

// A = 1.0 in slot `slot` of every lane of k part `aq`, 0 elsewhere; B lane
// (col, q) element e = 1 + e + 16 q; every lane's index register = idx.
// Returns C[0][0] (-1 when C is not one value throughout).
static float run(const Dev& d, int shape, int abid, int aq, int slot, int idx) {
  const int R = shape == 0 ? 32 : 16;
  unsigned short ha[64 * 8] = {}, hb[64 * 16];
  int hi[64];
  for (int l = 0; l < 64; ++l) {
    if (l / R == aq) ha[l * 8 + slot] = bf16_bits(1.f);
    for (int e = 0; e < 16; ++e)
      hb[l * 16 + e] = bf16_bits((float)(1 + e + 16 * (l / R)));
    hi[l] = idx;
  }
  (void)hipMemcpy(d.a, ha, sizeof(ha), hipMemcpyHostToDevice);
  (void)hipMemcpy(d.b, hb, sizeof(hb), hipMemcpyHostToDevice);
  (void)hipMemcpy(d.idx, hi, sizeof(hi), hipMemcpyHostToDevice);
  (void)hipMemset(d.c, 0xFF, 32 * 32 * 4);
  auto k = shape == 0 ? (abid ? probe<0, 1> : probe<0, 0>)
                      : (abid ? probe<1, 1> : probe<1, 0>);
  hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, (const bf16x8*)d.a,
                     (const bf16x16*)d.b, d.idx, d.c);
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    printf("probe: %s\n", hipGetErrorString(e));
    exit(1);
  }
  float out[32 * 32];
  (void)hipMemcpy(out, d.c, R * R * 4, hipMemcpyDeviceToHost);
  for (int i = 1; i < R * R; ++i)
    if (out[i] != out[0]) return -1.f;
  return out[0];
}

int main() {
  Dev d;
  (void)hipMalloc(&d.a, 64 * 8 * 2);
  (void)hipMalloc(&d.b, 64 * 16 * 2);
  (void)hipMalloc(&d.idx, 64 * 4);
  (void)hipMalloc(&d.c, 32 * 32 * 4);
  for (int shape = 0; shape < 2; ++shape)
    for (int abid = 0; abid < 2; ++abid)
      for (int aq = 0; aq < (shape == 0 ? 2 : 4); ++aq)
        for (int slot = 0; slot < 8; ++slot) {
          // all fields 0: the element the slot meets at position 0
          const float v0 = run(d, shape, abid, aq, slot, 0);
          printf("shape %d abid %d A part %d slot %d: index 0 -> B part %d "
                 "element %d;",
                 shape, abid, aq, slot, ((int)v0 - 1) / 16, ((int)v0 - 1) % 16);
          // one 2-bit field = 3 at a time: the field that moves the slot
          for (int f = 0; f < 16; ++f) {
            const float v = run(d, shape, abid, aq, slot, 3 << (2 * f));
            if (v != v0)
              printf(" field %d=3 -> part %d element %d;", f,
                     ((int)v - 1) / 16, ((int)v - 1) % 16);
          }
          printf("\n");
        }
  return 0;
}
