// Persistent per-device probe state. The CC manager is a long-lived
// daemon that attests after every transition: allocations, events and
// the liveness scratch word are cached so steady-state probes pay only
// kernel time (first call measured ~225 ms of hipMalloc/teardown
// overhead at dim=1024; with the cached context AND the cached fp32
// reference, the warm probe is ~0.4 ms). Each leg owns its buffers and
// caches: resizing one leg leaves the others alone.

#define CC_CHECK(expr)                                                         \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      snprintf(rep->error, sizeof(rep->error), "%s: %s", #expr,                \
               hipGetErrorString(_e));                                         \
      return (int)_e;                                                          \
    }                                                                          \
  } while (0)

// propagate a nonzero int status
#define CC_TRY(expr)                                                           \
  do {                                                                         \
    int _rc = (expr);                                                          \
    if (_rc != 0) return _rc;                                                  \
  } while (0)

constexpr int kMaxDevices = 64;

// An owning device allocation: the pointer and the bytes it holds.
// Assigning over one frees what it held, so `ctx = Ctx{}` releases a
// whole context. No destructor: the context table is static and must
// not call into HIP at process exit.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf& operator=(DevBuf&& o) {
    release();
    p = o.p, bytes = o.bytes;
    o.p = nullptr, o.bytes = 0;
    return *this;
  }
  // hold exactly `n` bytes: frees and reallocates when the size differs
  hipError_t ensure(size_t n) {
    if (bytes == n) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) p = nullptr;
    bytes = p ? n : 0;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  operator T*() const { return p; }
};

// The main probe (cc_attest_device). A change of dim releases all ten
// buffers before allocating, so peak VRAM does not rise; a failed
// allocation leaves dim = 0 and the next acquire starts over.
struct MainCtx {
  int dim = 0;
  int ref_valid = 0;  // the fp32 reference of the deterministic fill
  // round-robin cursor when CC_ATTEST_XGMI_MAX_PEERS bounds the
  // per-probe link sample (full 7-link coverage amortized over
  // consecutive probes instead of per probe)
  int peer_cursor = 0;
  DevBuf<bf16> dA, dB;
  DevBuf<unsigned char> dA8, dB8;
  DevBuf<float> dC, dRef, dHbm, dErr;
  DevBuf<unsigned long long> dSum;
  DevBuf<uint32_t> dFail;

  hipError_t acquire(int D) {
    if (dim == D) return hipSuccess;
    *this = MainCtx{};
    const size_t n = (size_t)D * D;
    hipError_t e;
    if ((e = dA.ensure(n * sizeof(bf16))) || (e = dB.ensure(n * sizeof(bf16))) ||
        (e = dA8.ensure(n)) || (e = dB8.ensure(n)) ||
        (e = dC.ensure(n * sizeof(float))) ||
        (e = dRef.ensure(n * sizeof(float))) ||
        (e = dHbm.ensure(n * sizeof(float))) || (e = dErr.ensure(sizeof(float))) ||
        (e = dSum.ensure(sizeof(unsigned long long))) ||
        (e = dFail.ensure(sizeof(uint32_t))))
      return e;
    dim = D;
    return hipSuccess;
  }
};

// This device as the target of another device's xGMI leg: destination
// buffer (grow-only, probe_xgmi) and the checksum word computed here.
struct PeerCtx {
  DevBuf<float> dPeerDst;
  DevBuf<unsigned long long> dPeerSum;
};

// The MXFP4 leg (cc_attest_mxfp4), same rules as MainCtx.
struct MxCtx {
  int dim = 0;
  int ref_valid = 0;
  DevBuf<unsigned char> dMxA, dMxB;    // packed fp4
  DevBuf<unsigned char> dMxSA, dMxSB;  // e8m0
  DevBuf<float> dMxC, dMxRef, dMxErr;
  DevBuf<unsigned long long> dMxSum;

  hipError_t acquire(int D) {
    if (dim == D) return hipSuccess;
    *this = MxCtx{};
    const size_t n = (size_t)D * D;
    hipError_t e;
    if ((e = dMxA.ensure(n / 2)) || (e = dMxB.ensure(n / 2)) ||
        (e = dMxSA.ensure(n / 32)) || (e = dMxSB.ensure(n / 32)) ||
        (e = dMxC.ensure(n * sizeof(float))) ||
        (e = dMxRef.ensure(n * sizeof(float))) ||
        (e = dMxErr.ensure(sizeof(float))) ||
        (e = dMxSum.ensure(sizeof(unsigned long long))))
      return e;
    dim = D;
    return hipSuccess;
  }
};

// The compute-unit sweep (cc_cu_sweep): fixed sizes, allocated once.
struct SweepCtx {
  DevBuf<unsigned> dSweepTab;
  DevBuf<float> dSweepGold;
  int gold_rounds = 0;             // rounds dSweepGold was computed for
  std::vector<unsigned> hSweepTab;  // the unit table after the last sweep
  int valid = 0;                   // hSweepTab holds a finished sweep

  static constexpr size_t kTabWords = (size_t)CU_SWEEP_UNITS * CU_SWEEP_REC;
  hipError_t acquire() {
    hipError_t e;
    if ((e = dSweepTab.ensure(kTabWords * sizeof(unsigned))) ||
        (e = dSweepGold.ensure(CU_SWEEP_GOLD_ELEMS * sizeof(float))))
      return e;
    try {
      hSweepTab.resize(kTabWords);
    } catch (const std::bad_alloc&) {
      return hipErrorOutOfMemory;
    }
    return hipSuccess;
  }
};

// The HBM march (cc_hbm_march, cc_hbm_step): only the small result
// block. The window's chunks belong to the call and are gone when it
// returns.
struct HbmCtx {
  DevBuf<HbmMarchResult> dRes;
  hipError_t acquire() { return dRes.ensure(sizeof(HbmMarchResult)); }
};

// The host-link leg (cc_host_link, cc_host_step): only the device result
// block. The pinned window, a registration and the staging buffer belong
// to the call.
struct HostCtx {
  DevBuf<HbmMarchResult> dRes;
  hipError_t acquire() { return dRes.ensure(sizeof(HbmMarchResult)); }
};

struct DeviceCtx {
  bool used = false;  // set by device_ctx(): shutdown has something to free
  MainCtx main;
  PeerCtx peer;
  MxCtx mx;
  SweepCtx sweep;
  HbmCtx hbm;
  HostCtx host;
  DevBuf<int> dLive;  // cc_device_alive's word: freed by shutdown only
  hipEvent_t ev0 = nullptr, ev1 = nullptr;

  // the two timing events, created once per device on first use
  hipError_t events() {
    hipError_t e;
    if (!ev0 && (e = hipEventCreate(&ev0)) != hipSuccess) return e;
    if (!ev1 && (e = hipEventCreate(&ev1)) != hipSuccess) return e;
    return hipSuccess;
  }
  void release() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    *this = DeviceCtx{};
  }
};

static DeviceCtx g_ctx[kMaxDevices];
static std::mutex g_ctx_mu;

// Every path that may allocate takes its context here (g_ctx_mu held).
static DeviceCtx& device_ctx(int device) {
  g_ctx[device].used = true;
  return g_ctx[device];
}

// record, launch, record, sync: the launch's time on the null stream.
// `launch` returns 0 or a status that aborts the leg.
template <typename Report, typename Launch>
static int timed_ms(DeviceCtx& dev, Report* rep, double* ms, Launch launch) {
  hipEvent_t ev0 = dev.ev0, ev1 = dev.ev1;
  CC_CHECK(hipEventRecord(ev0, 0));
  CC_TRY(launch());
  CC_CHECK(hipEventRecord(ev1, 0));
  CC_CHECK(hipEventSynchronize(ev1));
  float f = 0.f;
  (void)hipEventElapsedTime(&f, ev0, ev1);
  *ms = (double)f;
  return 0;
}

// copy one device word back, bit for bit
template <typename T>
static hipError_t read_back(const void* dptr, T* out) {
  return hipMemcpy(out, dptr, sizeof(T), hipMemcpyDeviceToHost);
}

// The xGMI leg hops to the peer device and back; any early return while
// away must leave the calling thread on its own device again.
struct DeviceHop {
  int home;
  bool away = false;
  explicit DeviceHop(int device) : home(device) {}
  hipError_t to(int peer) {
    away = true;
    return hipSetDevice(peer);
  }
  hipError_t back() {
    hipError_t e = hipSetDevice(home);
    away = e != hipSuccess;
    return e;
  }
  ~DeviceHop() {
    if (away) (void)hipSetDevice(home);
  }
};
