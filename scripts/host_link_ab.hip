// Host-link shader passes against the runtime's copy path, for
// scripts/host_link_ab.py: one process, one pinned window per role, and
// for every (blocks, vectors in flight) setting ROUNDS rounds that
// interleave link_pull, link_push, link_duplex and hipMemcpyAsync in each
// direction over the same number of bytes. Device-event time per launch
// or copy; one JSON line per setting with medians and ranges. Every
// setting's results are verified (kernel record and CPU compare) so a
// fast wrong kernel cannot win.
//
//   host_link_ab MIB ROUNDS BLOCKS:U [BLOCKS:U ...]     U in 1, 2, 4, 8
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../k8s_cc_manager_amd/ops/host_link.hip"
#include "../k8s_cc_manager_amd/ops/host_pattern.hip"

#define HIP_OK(expr)                                                  \
  do {                                                                \
    hipError_t e_ = (expr);                                           \
    if (e_ != hipSuccess) {                                           \
      fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));      \
      return 2;                                                       \
    }                                                                 \
  } while (0)

template <int U>
static void launch(int what, unsigned blocks, u32x4* base, uint32_t nvec,
                   HbmMarchResult* res) {
  const dim3 block(HOST_LINK_THREADS);
  if (what == 0)
    hipLaunchKernelGGL((link_pull<0, U>), dim3(blocks), block, 0, 0, base,
                       nvec, 0ull, 0ull, res, 1);
  else if (what == 1)
    hipLaunchKernelGGL((link_push<1, U>), dim3(blocks), block, 0, 0, base,
                       nvec, 0ull, 0ull, res, 2);
  else
    hipLaunchKernelGGL((link_duplex<U>), dim3(blocks & ~1u), block, 0, 0, base,
                       nvec / 2, nvec - nvec / 2, 0ull, 0ull, res, 5);
}

static void launch_u(int u, int what, unsigned blocks, u32x4* base,
                     uint32_t nvec, HbmMarchResult* res) {
  switch (u) {
    case 1: return launch<1>(what, blocks, base, nvec, res);
    case 2: return launch<2>(what, blocks, base, nvec, res);
    case 4: return launch<4>(what, blocks, base, nvec, res);
    default: return launch<8>(what, blocks, base, nvec, res);
  }
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s MIB ROUNDS BLOCKS:U [BLOCKS:U ...]\n", argv[0]);
    return 1;
  }
  const long long mib = atoll(argv[1]);
  const int rounds = atoi(argv[2]);
  if (mib < 1 || mib > 1024 || rounds < 1 || rounds > 1000) return 1;
  const unsigned long long bytes = (unsigned long long)mib << 20;
  const uint32_t nvec = (uint32_t)(bytes / 16);
  const uint32_t per_vec_blocks = HOST_LINK_THREADS;

  HIP_OK(hipSetDevice(0));
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, 0));
  void *hPull, *hPush, *hDup, *hBack, *D;
  HIP_OK(hipHostMalloc(&hPull, bytes, hipHostMallocDefault));
  HIP_OK(hipHostMalloc(&hPush, bytes, hipHostMallocDefault));
  HIP_OK(hipHostMalloc(&hDup, bytes, hipHostMallocDefault));
  HIP_OK(hipHostMalloc(&hBack, bytes, hipHostMallocDefault));
  HIP_OK(hipMalloc(&D, bytes));
  HbmMarchResult* res;
  HIP_OK(hipMalloc(&res, sizeof(*res)));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));

  host_pattern_fill((uint32_t*)hPull, bytes / 4, 0, 0);
  host_pattern_fill((uint32_t*)hDup, bytes / 8, 0, 0);
  printf("{\"kind\": \"host_link_ab_device\", \"arch\": \"%s\", \"cus\": %d, "
         "\"mib\": %lld, \"rounds\": %d}\n",
         prop.gcnArchName, prop.multiProcessorCount, mib, rounds);

  for (int a = 3; a < argc; ++a) {
    unsigned blocks = 0;
    int u = 0;
    if (sscanf(argv[a], "%u:%d", &blocks, &u) != 2 || blocks < 2 ||
        blocks > 65536 || (u != 1 && u != 2 && u != 4 && u != 8)) {
      fprintf(stderr, "bad setting %s\n", argv[a]);
      return 1;
    }
    // never more blocks than the buffer has groups for
    const unsigned need = (nvec / 2 + per_vec_blocks * u - 1) / (per_vec_blocks * u);
    if (blocks > need) blocks = need < 2 ? 2 : need;

    HbmMarchResult h = {};
    h.first_bad_offset = ~0ull;
    HIP_OK(hipMemcpy(res, &h, sizeof(h), hipMemcpyHostToDevice));
    __builtin_memset(hPush, 0x5A, bytes);
    __builtin_memset((char*)hDup + bytes / 2, 0x5A, bytes - bytes / 2);
    __builtin_memset(hBack, 0x5A, bytes);

    const char* names[5] = {"pull", "push", "duplex", "h2d", "d2h"};
    std::vector<float> ms[5];
    for (int r = -3; r < rounds; ++r) {  // three warm rounds
      for (int what = 0; what < 5; ++what) {
        HIP_OK(hipEventRecord(e0, 0));
        if (what < 3) {
          void* base = what == 0 ? hPull : what == 1 ? hPush : hDup;
          void* dbase = nullptr;
          HIP_OK(hipHostGetDevicePointer(&dbase, base, 0));
          launch_u(u, what, blocks, (u32x4*)dbase, nvec, res);
          HIP_OK(hipGetLastError());
        } else if (what == 3) {
          HIP_OK(hipMemcpyAsync(D, hPull, bytes, hipMemcpyHostToDevice, 0));
        } else {
          HIP_OK(hipMemcpyAsync(hBack, D, bytes, hipMemcpyDeviceToHost, 0));
        }
        HIP_OK(hipEventRecord(e1, 0));
        HIP_OK(hipEventSynchronize(e1));
        float f = 0.f;
        HIP_OK(hipEventElapsedTime(&f, e0, e1));
        if (r >= 0) ms[what].push_back(f);
      }
    }
    // verify: the kernels' record, what push and duplex left in host
    // memory, and the round trip of the copy path
    HIP_OK(hipMemcpy(&h, res, sizeof(h), hipMemcpyDeviceToHost));
    HbmMarchResult cpu = {};
    cpu.first_bad_offset = ~0ull;
    host_pattern_compare((const uint32_t*)hPush, bytes / 4, 0, 0, 1, 2, &cpu);
    host_pattern_compare((const uint32_t*)hDup, bytes / 4, 0, 0, 0, 5, &cpu);
    host_pattern_compare((const uint32_t*)hBack, bytes / 4, 0, 0, 0, 4, &cpu);

    printf("{\"kind\": \"host_link_ab\", \"blocks\": %u, \"u\": %d, "
           "\"wrong_words\": %llu",
           blocks, u, h.mismatch_words + cpu.mismatch_words);
    for (int what = 0; what < 5; ++what) {
      std::vector<float>& v = ms[what];
      std::sort(v.begin(), v.end());
      const double med = (v[(v.size() - 1) / 2] + v[v.size() / 2]) / 2.0;
      // duplex moves half the window each way: its rate is per direction
      const double moved = what == 2 ? bytes / 2.0 : (double)bytes;
      printf(", \"%s_ms_med\": %.4f, \"%s_ms_min_max\": [%.4f, %.4f], "
             "\"%s_gbps_med\": %.2f",
             names[what], med, names[what], v.front(), v.back(), names[what],
             moved / (med * 1e-3) / 1e9);
    }
    printf("}\n");
    fflush(stdout);
    if (h.mismatch_words + cpu.mismatch_words) return 3;
  }
  (void)hipHostFree(hPull);
  (void)hipHostFree(hPush);
  (void)hipHostFree(hDup);
  (void)hipHostFree(hBack);
  (void)hipFree(D);
  (void)hipFree(res);
  return 0;
}
