// Probe legs. Each takes the device context and the report and returns
// 0, a HIP error (text in rep->error) or a negative probe status. The
// three GEMM legs share the steps that are identical (timed_gemm,
// cached_reference, compare_read_back); their clears and fills differ
// and stay in the leg.

// Warm launch, sync, timed launch, TF/s of the D^3 GEMM; -6 when
// `launch` refuses the shape (returns nonzero).
template <typename Report, typename Launch>
static int timed_gemm(DeviceCtx& dev, Report* rep, int D, double* ms,
                      double* tflops, Launch launch) {
  auto checked = [&] { return launch() != 0 ? -6 : 0; };
  CC_TRY(checked());
  CC_CHECK(hipDeviceSynchronize());
  CC_TRY(timed_ms(dev, rep, ms, checked));
  *tflops = 2.0 * D * (double)D * D / (*ms * 1e-3) / 1e12;
  return 0;
}

// The fills are deterministic per dim, so a leg's VALU reference is a
// constant: computed (and timed) once per context — ~1.9 ms of a 2.4 ms
// warm probe at dim 1024. *ms = 0.0 when cached.
template <typename Report, typename Launch>
static int cached_reference(DeviceCtx& dev, Report* rep, int* valid,
                            double* ms, Launch launch) {
  *ms = 0.0;
  if (*valid) return 0;
  CC_TRY(timed_ms(dev, rep, ms, [&] {
    launch();
    return 0;
  }));
  *valid = 1;
  return 0;
}

// max_abs_diff of dC against dRef, the checksum of dC where the leg has
// one, sync, read back.
template <typename Report>
static int compare_read_back(Report* rep, const float* dC, const float* dRef,
                             long elems, float* dErr, float* err,
                             unsigned long long* dSum = nullptr,
                             unsigned long long* sum = nullptr) {
  hipLaunchKernelGGL(max_abs_diff, dim3(1024), dim3(256), 0, 0, dC, dRef,
                     elems, dErr);
  if (dSum)
    hipLaunchKernelGGL(checksum_f32, dim3(1024), dim3(256), 0, 0, dC, elems,
                       dSum);
  CC_CHECK(hipDeviceSynchronize());
  CC_CHECK(read_back(dErr, err));
  if (dSum) CC_CHECK(read_back(dSum, sum));
  return 0;
}

static int probe_bf16(DeviceCtx& dev, CcAttestReport* rep) {
  MainCtx& ctx = dev.main;
  const int D = ctx.dim;
  const long elems = (long)D * D;
  bf16 *dA = ctx.dA, *dB = ctx.dB;
  float *dC = ctx.dC, *dRef = ctx.dRef, *dErr = ctx.dErr;
  unsigned long long* dSum = ctx.dSum;
  CC_CHECK(hipMemset(dErr, 0, sizeof(float)));
  CC_CHECK(hipMemset(dSum, 0, sizeof(unsigned long long)));

  // fill (asymmetric seeds: catches row/col-swapped layouts)
  hipLaunchKernelGGL(fill_bf16_lcg, dim3(2048), dim3(256), 0, 0, dA, elems, 1u);
  hipLaunchKernelGGL(fill_bf16_lcg, dim3(2048), dim3(256), 0, 0, dB, elems, 7u);

  // production bf16 dispatch (D is a multiple of its 128 tile)
  CC_TRY(timed_gemm(dev, rep, D, &rep->gemm_ms, &rep->gemm_tflops,
                    [&] { return launch_mfma_gemm(dA, dB, dC, D, D, D); }));
  CC_TRY(cached_reference(dev, rep, &ctx.ref_valid, &rep->ref_ms, [&] {
    dim3 rblock(16, 16), rgrid((D + 15) / 16, (D + 15) / 16);
    hipLaunchKernelGGL(ref_gemm_f32, rgrid, rblock, 0, 0, dA, dB, dRef, D, D,
                       D);
  }));
  return compare_read_back(rep, dC, dRef, elems, dErr, &rep->max_abs_err, dSum,
                           &rep->checksum);
}

// fp8 (MX-scaled) MFMA path: same integer values, same fp32 reference,
// bitwise requirement; the PRODUCTION fp8 dispatch
static int probe_fp8(DeviceCtx& dev, CcAttestReport* rep) {
  MainCtx& ctx = dev.main;
  const int D = ctx.dim;
  const long elems = (long)D * D;
  float *dC = ctx.dC, *dErr = ctx.dErr;
  hipLaunchKernelGGL(fill_fp8_lcg, dim3(2048), dim3(256), 0, 0, ctx.dA8.p,
                     elems, 1u);
  hipLaunchKernelGGL(fill_fp8_lcg, dim3(2048), dim3(256), 0, 0, ctx.dB8.p,
                     elems, 7u);
  CC_TRY(timed_gemm(dev, rep, D, &rep->fp8_ms, &rep->fp8_tflops, [&] {
    return launch_fp8_best(ctx.dA8, ctx.dB8, dC, D, D, D);
  }));
  CC_CHECK(hipMemset(dErr, 0, sizeof(float)));  // only now; no checksum
  return compare_read_back(rep, dC, ctx.dRef, elems, dErr,
                           &rep->fp8_max_abs_err);
}

static int probe_lds(DeviceCtx& dev, CcAttestReport* rep) {
  uint32_t* dFail = dev.main.dFail;
  CC_CHECK(hipMemset(dFail, 0, sizeof(uint32_t)));
  CC_TRY(timed_ms(dev, rep, &rep->lds_ms, [&] {
    hipLaunchKernelGGL(lds_probe, dim3(512), dim3(256), 0, 0, dFail, 8);
    return 0;
  }));
  CC_CHECK(read_back(dFail, &rep->lds_failures));
  return 0;
}

// HBM probe (dedicated dst: dRef is a cached constant)
static int probe_hbm(DeviceCtx& dev, CcAttestReport* rep) {
  MainCtx& ctx = dev.main;
  long n4 = (long)ctx.dim * ctx.dim / 4;
  CC_TRY(timed_ms(dev, rep, &rep->hbm_ms, [&] {
    hipLaunchKernelGGL(hbm_copy_f4, dim3(4096), dim3(256), 0, 0,
                       (const float4v*)ctx.dC.p, (float4v*)ctx.dHbm.p, n4);
    return 0;
  }));
  rep->hbm_gbps = 2.0 * n4 * 16.0 / (rep->hbm_ms * 1e-3) / 1e9;
  return 0;
}

// xGMI peer visibility + traffic. Visibility alone attests nothing
// about link integrity: for every accessible peer, move the live result
// buffer across the link (SDMA over xGMI) and recompute its checksum ON
// THE PEER. Per-link bandwidth is reported (xGMI is point-to-point,
// 7 links x ~153 GB/s per GPU — each link is individually bound).
static int probe_xgmi(DeviceCtx& dev, CcAttestReport* rep) {
  MainCtx& ctx = dev.main;
  const int device = rep->device;
  float* dC = ctx.dC;
  unsigned long long* dSum = ctx.dSum;
  int ndev = 0;
  CC_CHECK(hipGetDeviceCount(&ndev));
  rep->peer_count = ndev - 1;
  if (ndev > kMaxDevices) ndev = kMaxDevices;
  // Bounded per-link sample (2 MiB x 2 copies): on an 8-GPU hive the
  // probe runs per device per transition and touches 7 links — an
  // unbounded sample would dominate the transition step. 4 MiB per
  // link is still real SDMA traffic with an on-peer checksum.
  long bytes = (long)ctx.dim * ctx.dim * sizeof(float);
  if (bytes > (2L << 20)) bytes = 2L << 20;
  long sum_elems = bytes / sizeof(float);
  // fresh source checksum over the sampled slice: dC now holds the
  // fp8 result (the bf16-era rep->checksum no longer matches)
  CC_CHECK(hipMemset(dSum, 0, sizeof(unsigned long long)));
  hipLaunchKernelGGL(checksum_f32, dim3(1024), dim3(256), 0, 0, dC, sum_elems,
                     dSum);
  CC_CHECK(hipDeviceSynchronize());
  unsigned long long src_sum = 0;
  CC_CHECK(read_back(dSum, &src_sum));
  // accessible peer list first; CC_ATTEST_XGMI_MAX_PEERS (0 = all)
  // bounds how many links one probe samples — the scaling bench sets
  // it so per-transition cost stays O(1) while the round-robin cursor
  // still covers every link across consecutive probes
  int acc[kMaxDevices];
  int n_acc = 0;
  for (int p = 0; p < ndev; ++p) {
    if (p == device) continue;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, device, p) == hipSuccess && can)
      acc[n_acc++] = p;
  }
  rep->peers_accessible = n_acc;
  int max_peers = 0;
  if (const char* mp = getenv("CC_ATTEST_XGMI_MAX_PEERS")) max_peers = atoi(mp);
  int attempts = (max_peers > 0 && max_peers < n_acc) ? max_peers : n_acc;
  rep->peers_attempted = attempts;
  DeviceHop hop(device);
  for (int t = 0; t < attempts; ++t) {
    int p = acc[(ctx.peer_cursor + t) % (n_acc ? n_acc : 1)];
    hipError_t pe = hipDeviceEnablePeerAccess(p, 0);
    if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) {
      (void)hipGetLastError();  // clear; copy may still route via SDMA
    }
    // destination + checksum word live on the peer (cached there)
    PeerCtx& pc = device_ctx(p).peer;
    CC_CHECK(hop.to(p));
    // grow-only: ensure() frees the smaller buffer before allocating
    if ((long)pc.dPeerDst.bytes < bytes &&
        pc.dPeerDst.ensure(bytes) != hipSuccess) {
      CC_CHECK(hop.back());
      continue;  // peer VRAM exhausted: counted accessible, not verified
    }
    if (pc.dPeerSum.ensure(sizeof(unsigned long long)) != hipSuccess) {
      CC_CHECK(hop.back());
      continue;
    }
    CC_CHECK(hipMemset(pc.dPeerDst, 0, bytes));
    CC_CHECK(hop.back());
    // timed link traffic: kPeerIters copies of the result buffer
    const int kPeerIters = 4;
    double ms = 0.0;
    CC_TRY(timed_ms(dev, rep, &ms, [&] {
      for (int it = 0; it < kPeerIters; ++it)
        CC_CHECK(hipMemcpyPeerAsync(pc.dPeerDst, p, dC, device, bytes, 0));
      return 0;
    }));
    rep->xgmi_ms += ms;
    double gbps = (double)bytes * kPeerIters / (ms * 1e-3) / 1e9;
    if (rep->xgmi_gbps_min == 0.0 || gbps < rep->xgmi_gbps_min)
      rep->xgmi_gbps_min = gbps;
    if (gbps > rep->xgmi_gbps_max) rep->xgmi_gbps_max = gbps;
    // verify ON the peer: its own CUs must read back what crossed
    CC_CHECK(hop.to(p));
    CC_CHECK(hipMemset(pc.dPeerSum, 0, sizeof(unsigned long long)));
    // checksum the SAMPLED slice only (sum_elems) — the peer buffer
    // holds exactly `bytes`; summing all of dC would read out of bounds
    hipLaunchKernelGGL(checksum_f32, dim3(1024), dim3(256), 0, 0,
                       pc.dPeerDst.p, sum_elems, pc.dPeerSum.p);
    CC_CHECK(hipDeviceSynchronize());
    unsigned long long peer_sum = 0;
    CC_CHECK(read_back(pc.dPeerSum, &peer_sum));
    CC_CHECK(hop.back());
    if (peer_sum == src_sum) ++rep->peers_verified;
  }
  if (n_acc) ctx.peer_cursor = (ctx.peer_cursor + attempts) % n_acc;
  return 0;
}

// MXFP4 leg: all 16 e2m1 codes and scale bytes {126,127,128} through
// the fp4 decoders and the block-scale hardware, bitwise against the
// VALU reference (exactness budget at fill_fp4_lcg).
static int probe_mxfp4(DeviceCtx& dev, CcMxReport* rep) {
  MxCtx& ctx = dev.mx;
  const int D = ctx.dim;
  const long elems = (long)D * D;
  unsigned char *dA = ctx.dMxA, *dB = ctx.dMxB;
  unsigned char *dSA = ctx.dMxSA, *dSB = ctx.dMxSB;
  float *dC = ctx.dMxC, *dRef = ctx.dMxRef, *dErr = ctx.dMxErr;
  unsigned long long* dSum = ctx.dMxSum;
  CC_CHECK(hipMemset(dErr, 0, sizeof(float)));
  CC_CHECK(hipMemset(dSum, 0, sizeof(unsigned long long)));
  // prefill with 0x7f7f7f7f (3.4e38, finite: max_abs_diff's fmaxf would
  // drop a NaN): an output the kernel never wrote shows as a huge error
  CC_CHECK(hipMemset(dC, 0x7F, elems * sizeof(float)));

  hipLaunchKernelGGL(fill_fp4_lcg, dim3(2048), dim3(256), 0, 0, dA, elems / 2,
                     1u);
  hipLaunchKernelGGL(fill_fp4_lcg, dim3(2048), dim3(256), 0, 0, dB, elems / 2,
                     7u);
  hipLaunchKernelGGL(fill_e8m0_lcg, dim3(256), dim3(256), 0, 0, dSA,
                     elems / 32, 1u);
  hipLaunchKernelGGL(fill_e8m0_lcg, dim3(256), dim3(256), 0, 0, dSB,
                     elems / 32, 7u);

  CC_TRY(timed_gemm(dev, rep, D, &rep->mx_ms, &rep->mx_tflops, [&] {
    return launch_mxfp4(dA, dSA, dB, dSB, dC, D, D, D);
  }));
  CC_TRY(cached_reference(dev, rep, &ctx.ref_valid, &rep->mx_ref_ms, [&] {
    launch_ref_mxfp4(dA, dSA, dB, dSB, dRef, D, D, D);
  }));
  return compare_read_back(rep, dC, dRef, elems, dErr, &rep->mx_max_abs_err,
                           dSum, &rep->mx_checksum);
}

// The golden C images for `rounds`, a constant: computed once per
// (device, rounds). *ms = 0.0 when the cached images were used. `rep`
// is whatever holds the error text (a report, or ErrorText).
template <typename Report>
static int sweep_gold(DeviceCtx& dev, Report* rep, int rounds, double* ms) {
  SweepCtx& ctx = dev.sweep;
  *ms = 0.0;
  if (ctx.gold_rounds == rounds) return 0;
  ctx.gold_rounds = 0;
  CC_TRY(timed_ms(dev, rep, ms, [&] {
    hipLaunchKernelGGL(cu_sweep_gold, dim3(1), dim3(1024), 0, 0,
                       ctx.dSweepGold.p, rounds);
    return 0;
  }));
  CC_CHECK(hipGetLastError());
  ctx.gold_rounds = rounds;
  return 0;
}

static int sweep_units_seen(const unsigned* tab) {
  int n = 0;
  for (int k = 0; k < CU_SWEEP_UNITS; ++k) n += tab[k * CU_SWEEP_REC] != 0;
  return n;
}

// Sweep leg: up to 4 launches of 4 blocks per CU into one unit table,
// until every SIMD of every CU has reported.
static int probe_cu_sweep(DeviceCtx& dev, CcSweepReport* rep, int poison_key) {
  SweepCtx& ctx = dev.sweep;
  const size_t tab_b = SweepCtx::kTabWords * sizeof(unsigned);
  unsigned* tab = ctx.hSweepTab.data();
  CC_TRY(sweep_gold(dev, rep, rep->rounds, &rep->gold_ms));
  ctx.valid = 0;
  CC_CHECK(hipMemset(ctx.dSweepTab, 0, tab_b));
  const int kMaxLaunches = 4;
  for (int l = 0; l < kMaxLaunches; ++l) {
    double ms = 0.0;
    CC_TRY(timed_ms(dev, rep, &ms, [&] {
      hipLaunchKernelGGL(cu_sweep, dim3(4 * rep->cu_count), dim3(1024), 0, 0,
                         ctx.dSweepGold.p, ctx.dSweepTab.p, rep->rounds,
                         poison_key);
      return 0;
    }));
    CC_CHECK(hipGetLastError());
    rep->sweep_ms += ms;
    rep->launches = l + 1;
    CC_CHECK(hipMemcpy(tab, ctx.dSweepTab, tab_b, hipMemcpyDeviceToHost));
    if (sweep_units_seen(tab) >= rep->units_expected) break;
  }
  ctx.valid = 1;

  unsigned long long xccs = 0;
  int last_cu = -1;  // keys ascend, a CU's four SIMDs are adjacent
  for (int k = 0; k < CU_SWEEP_UNITS; ++k) {
    const unsigned* rec = tab + k * CU_SWEEP_REC;
    if (!rec[0]) continue;
    ++rep->units_seen;
    if ((k >> 2) != last_cu) ++rep->cus_seen;
    last_cu = k >> 2;
    xccs |= 1ull << (k >> 10);
    rep->mfma_failures += rec[1];
    rep->lds_failures += rec[2];
    if (rec[1] || rec[2]) {
      if (rep->units_failed < 16) rep->failed_keys[rep->units_failed] = k;
      ++rep->units_failed;
    }
  }
  rep->xccs_seen = __builtin_popcountll(xccs);
  return 0;
}

// The window of one march: chunks of VRAM that live for one call. A
// DevBuf frees nothing by itself, so this does, on every path out.
struct HbmWindow {
  std::vector<DevBuf<u32x4>> chunks;
  ~HbmWindow() {
    for (auto& c : chunks) c.release();
  }
};

// One march_step over [ptr, ptr + bytes) in launches of at most 1 GiB
// (32-bit in-chunk indices). addr: logical byte address of ptr (origin +
// window offset); byte0: its window offset. The grid follows the CU
// count, 8 blocks each, fewer when the range is smaller than that.
static void launch_march(int check, int write, void* ptr,
                         unsigned long long bytes, unsigned long long addr,
                         unsigned long long byte0, HbmMarchResult* res,
                         int pass, int cu_count) {
  for (unsigned long long at = 0; at < bytes; at += HBM_MARCH_MAX_CHUNK) {
    const unsigned long long n = bytes - at < HBM_MARCH_MAX_CHUNK
                                     ? bytes - at
                                     : HBM_MARCH_MAX_CHUNK;
    const uint32_t nvec = (uint32_t)(n / 16);
    const uint32_t per_block = HBM_MARCH_THREADS * HBM_MARCH_UNROLL;
    uint32_t blocks = (nvec + per_block - 1) / per_block;
    if (blocks > 8u * cu_count) blocks = 8u * cu_count;
    hipLaunchKernelGGL(kMarchStep[check + 1][write + 1], dim3(blocks),
                       dim3(HBM_MARCH_THREADS), 0, 0,
                       (u32x4*)((char*)ptr + at), nvec, (addr + at) / 4,
                       byte0 + at, res, pass);
  }
}

// the result block before a march: nothing counted, no first offset
static int march_reset(DeviceCtx& dev, CcHbmReport* rep) {
  HbmMarchResult h = {};
  h.first_bad_offset = ~0ull;
  CC_CHECK(hipMemcpy(dev.hbm.dRes, &h, sizeof(h), hipMemcpyHostToDevice));
  return 0;
}

// ... and after it, into the report
static int march_collect(DeviceCtx& dev, CcHbmReport* rep) {
  HbmMarchResult h;
  CC_CHECK(hipMemcpy(&h, dev.hbm.dRes, sizeof(h), hipMemcpyDeviceToHost));
  rep->mismatch_words = h.mismatch_words;
  rep->first_bad_offset = h.first_bad_offset;
  rep->n_bad = h.mismatch_words < HBM_MARCH_RECORDS ? (int)h.mismatch_words
                                                    : HBM_MARCH_RECORDS;
  for (int i = 0; i < rep->n_bad; ++i) {
    rep->bad_offset[i] = h.bad_offset[i];
    rep->bad_expected[i] = h.bad_expected[i];
    rep->bad_got[i] = h.bad_got[i];
    rep->bad_pass[i] = h.bad_pass[i];
  }
  return 0;
}

// HBM march leg: fill p, check p / write ~p, check ~p / write 0, check 0,
// each pass over the whole window before the next starts. rep carries
// bytes_requested, chunk_bytes and origin. poison_after: 0, or the pass
// (1..3) after which the word at poison_offset gets bit 0 flipped. A
// window that cannot be allocated is not a device failure: rc 0, ok 0,
// bytes_tested 0 and the amounts in rep->error.
static int probe_hbm_march(DeviceCtx& dev, CcHbmReport* rep, int cu_count,
                           long long poison_offset, int poison_after) {
  const unsigned long long bytes = rep->bytes_requested;
  const unsigned long long chunk = rep->chunk_bytes;
  HbmWindow win;
  try {
    win.chunks = std::vector<DevBuf<u32x4>>((bytes + chunk - 1) / chunk);
  } catch (const std::bad_alloc&) {
    CC_CHECK(hipErrorOutOfMemory);
  }
  rep->chunks = (int)win.chunks.size();
  auto chunk_len = [&](size_t c) {
    return bytes - c * chunk < chunk ? bytes - c * chunk : chunk;
  };

  const auto t0 = std::chrono::steady_clock::now();
  unsigned long long held = 0;
  for (size_t c = 0; c < win.chunks.size(); ++c) {
    if (win.chunks[c].ensure(chunk_len(c)) != hipSuccess) break;
    held += chunk_len(c);
  }
  rep->alloc_ms = std::chrono::duration<double, std::milli>(
                      std::chrono::steady_clock::now() - t0)
                      .count();
  if (held != bytes) {
    (void)hipGetLastError();  // the device is fine, the window was not there
    snprintf(rep->error, sizeof(rep->error), "allocated %llu of %llu MiB",
             held >> 20, bytes >> 20);
    return 0;
  }

  CC_TRY(march_reset(dev, rep));
  static const int kPhases[4][2] = {{-1, 0}, {0, 1}, {1, 2}, {2, -1}};
  double* const ms[4] = {&rep->fill_ms, &rep->flip_ms, &rep->scrub_ms,
                         &rep->zero_ms};
  for (int pass = 1; pass <= 4; ++pass) {
    CC_TRY(timed_ms(dev, rep, ms[pass - 1], [&] {
      for (size_t c = 0; c < win.chunks.size(); ++c)
        launch_march(kPhases[pass - 1][0], kPhases[pass - 1][1],
                     win.chunks[c].p, chunk_len(c), rep->origin + c * chunk,
                     c * chunk, dev.hbm.dRes, pass, cu_count);
      return 0;
    }));
    CC_CHECK(hipGetLastError());
    rep->passes = pass;
    if (pass == poison_after) {
      char* at = (char*)win.chunks[poison_offset / chunk].p +
                 poison_offset % chunk;
      hipLaunchKernelGGL(march_poison, dim3(1), dim3(64), 0, 0, (uint32_t*)at);
      CC_CHECK(hipGetLastError());
    }
  }
  CC_TRY(march_collect(dev, rep));
  rep->bytes_tested = (long long)bytes;
  rep->gbps = 6.0 * bytes /
              ((rep->fill_ms + rep->flip_ms + rep->scrub_ms + rep->zero_ms) *
               1e-3) /
              1e9;
  return 0;
}

// The buffers of one host-link call: a pinned, mapped host window, a
// device staging buffer, and a registration of caller-owned memory. All
// are released on every path out.
struct HostWindow {
  void* host = nullptr;        // hipHostMalloc
  void* registered = nullptr;  // hipHostRegister of the caller's range
  DevBuf<u32x4> staging;
  ~HostWindow() {
    if (host) (void)hipHostFree(host);
    if (registered) (void)hipHostUnregister(registered);
    staging.release();
  }
};

// link_pull (check >= 0) or link_push (write >= 0) over [dptr, dptr +
// bytes), bytes <= 1 GiB; arguments as launch_march's.
static void launch_link(int check, int write, void* dptr,
                        unsigned long long bytes, unsigned long long addr,
                        unsigned long long byte0, HbmMarchResult* res,
                        int pass) {
  const uint32_t nvec = (uint32_t)(bytes / 16);
  hipLaunchKernelGGL(check >= 0 ? kLinkPull[check] : kLinkPush[write],
                     dim3(host_link_blocks(nvec)),
                     dim3(HOST_LINK_THREADS), 0, 0, (u32x4*)dptr, nvec,
                     addr / 4, byte0, res, pass);
}

// the device result block before a host-link call
static int link_reset(DeviceCtx& dev, CcHostReport* rep) {
  HbmMarchResult h = {};
  h.first_bad_offset = ~0ull;
  CC_CHECK(hipMemcpy(dev.host.dRes, &h, sizeof(h), hipMemcpyHostToDevice));
  return 0;
}

// a result block into the report
static void link_report(const HbmMarchResult& h, CcHostReport* rep) {
  rep->mismatch_words = h.mismatch_words;
  rep->first_bad_offset = h.first_bad_offset;
  rep->n_bad = h.mismatch_words < HBM_MARCH_RECORDS ? (int)h.mismatch_words
                                                    : HBM_MARCH_RECORDS;
  for (int i = 0; i < rep->n_bad; ++i) {
    rep->bad_offset[i] = h.bad_offset[i];
    rep->bad_expected[i] = h.bad_expected[i];
    rep->bad_got[i] = h.bad_got[i];
    rep->bad_pass[i] = h.bad_pass[i];
  }
}

// ... and after it: what the kernels found, then what the CPU found
static int link_collect(DeviceCtx& dev, CcHostReport* rep,
                        const HbmMarchResult& cpu) {
  HbmMarchResult h;
  CC_CHECK(hipMemcpy(&h, dev.host.dRes, sizeof(h), hipMemcpyDeviceToHost));
  host_pattern_merge(&h, cpu);
  link_report(h, rep);
  return 0;
}

static double link_gbps(unsigned long long bytes, double ms) {
  return ms > 0.0 ? (double)bytes / (ms * 1e-3) / 1e9 : 0.0;
}

// Host-link leg: five verified passes over a pinned host window H and a
// device buffer D of the same size (pull, push, h2d, d2h, duplex), pass k
// at logical origin origin + k * 2^40, odd passes in phase 0 and even
// ones in phase 1. Every pass runs even after a mismatch. The CPU
// touches H only before a launch or after its synchronise (timed_ms
// ends in one). poison_pass: 0, or the pass (1..5) in which the CPU flips
// bit 0 of the word at poison_offset between that pass's write and its
// check. Buffers that cannot be allocated are not a device failure: rc
// 0, ok 0, bytes_tested 0 and the amounts in rep->error.
static int probe_host_link(DeviceCtx& dev, CcHostReport* rep, int cu_count,
                           long long poison_offset, int poison_pass) {
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(clock::now() - t0).count();
  };
  const unsigned long long bytes = rep->bytes_requested;
  const unsigned long long half = bytes / 2;  // a multiple of 16
  HostWindow win;

  auto t0 = clock::now();
  const hipError_t eh = hipHostMalloc(&win.host, bytes, hipHostMallocDefault);
  if (eh != hipSuccess) win.host = nullptr;
  const hipError_t ed =
      eh == hipSuccess ? win.staging.ensure(bytes) : hipErrorOutOfMemory;
  rep->alloc_ms = ms_since(t0);
  if (eh != hipSuccess || ed != hipSuccess) {
    (void)hipGetLastError();  // the device is fine, the buffers were not there
    snprintf(rep->error, sizeof(rep->error),
             "allocated %llu of %llu MiB pinned host, %llu of %llu MiB device",
             eh == hipSuccess ? bytes >> 20 : 0ull, bytes >> 20,
             ed == hipSuccess ? bytes >> 20 : 0ull, bytes >> 20);
    return 0;
  }
  uint32_t* const H = (uint32_t*)win.host;
  void* Hd = nullptr;  // H as the device addresses it
  CC_CHECK(hipHostGetDevicePointer(&Hd, win.host, 0));
  void* const D = win.staging.p;
  HbmMarchResult* const dRes = dev.host.dRes;

  CC_TRY(link_reset(dev, rep));
  HbmMarchResult cpu = {};
  cpu.first_bad_offset = ~0ull;

  auto addr = [&](int pass) {
    return rep->origin + (unsigned long long)pass * HOST_LINK_PASS_STRIDE;
  };
  // CPU work on H[at, at + n), timed into host_ms
  auto fill = [&](int pass, unsigned long long at, unsigned long long n) {
    const auto t = clock::now();
    host_pattern_fill(H + at / 4, n / 4, (addr(pass) + at) / 4, (pass + 1) & 1);
    rep->host_ms += ms_since(t);
  };
  auto compare = [&](int pass, unsigned long long at, unsigned long long n) {
    const auto t = clock::now();
    host_pattern_compare(H + at / 4, n / 4, (addr(pass) + at) / 4, at,
                         (pass + 1) & 1, pass, &cpu);
    rep->host_ms += ms_since(t);
  };
  // the detector's wrong number, when this pass and this range hold it
  auto poison = [&](int pass, unsigned long long at, unsigned long long n) {
    if (pass == poison_pass && (unsigned long long)poison_offset >= at &&
        (unsigned long long)poison_offset < at + n)
      H[poison_offset / 4] ^= 1u;
  };

  // 1 pull: CPU fill, the shader loads H over the link and checks it
  fill(1, 0, bytes);
  poison(1, 0, bytes);
  CC_TRY(timed_ms(dev, rep, &rep->pull_ms, [&] {
    launch_link(0, -1, Hd, bytes, addr(1), 0, dRes, 1);
    return 0;
  }));
  CC_CHECK(hipGetLastError());
  rep->passes = 1;

  // 2 push: the shader stores ~p into H over the link, the CPU checks it
  CC_TRY(timed_ms(dev, rep, &rep->push_ms, [&] {
    launch_link(-1, 1, Hd, bytes, addr(2), 0, dRes, 2);
    return 0;
  }));
  CC_CHECK(hipGetLastError());
  poison(2, 0, bytes);
  compare(2, 0, bytes);
  rep->passes = 2;

  // 3 h2d: CPU fill, the runtime copies H -> D, march_step checks D
  fill(3, 0, bytes);
  poison(3, 0, bytes);
  CC_TRY(timed_ms(dev, rep, &rep->h2d_ms, [&] {
    CC_CHECK(hipMemcpyAsync(D, H, bytes, hipMemcpyHostToDevice, 0));
    return 0;
  }));
  launch_march(0, -1, D, bytes, addr(3), 0, dRes, 3, cu_count);
  CC_CHECK(hipGetLastError());
  CC_CHECK(hipDeviceSynchronize());
  rep->passes = 3;

  // 4 d2h: march_step fills D with ~p, the runtime copies D -> H, the
  // CPU checks H
  launch_march(-1, 1, D, bytes, addr(4), 0, dRes, 4, cu_count);
  CC_CHECK(hipGetLastError());
  CC_TRY(timed_ms(dev, rep, &rep->d2h_ms, [&] {
    CC_CHECK(hipMemcpyAsync(H, D, bytes, hipMemcpyDeviceToHost, 0));
    return 0;
  }));
  poison(4, 0, bytes);
  compare(4, 0, bytes);
  rep->passes = 4;

  // 5 duplex: one launch pulls the lower half and pushes the upper one
  fill(5, 0, half);
  poison(5, 0, half);
  CC_TRY(timed_ms(dev, rep, &rep->duplex_ms, [&] {
    const uint32_t nlo = (uint32_t)(half / 16);
    const uint32_t nhi = (uint32_t)((bytes - half) / 16);
    // each role gets half of the grid a one-way pass would have
    const uint32_t per_role = host_link_blocks(nhi, HOST_LINK_MAX_BLOCKS / 2);
    hipLaunchKernelGGL(link_duplex<>, dim3(2 * per_role),
                       dim3(HOST_LINK_THREADS), 0, 0, (u32x4*)Hd, nlo, nhi,
                       addr(5) / 4, 0ull, dRes, 5);
    return 0;
  }));
  CC_CHECK(hipGetLastError());
  poison(5, half, bytes - half);
  compare(5, half, bytes - half);
  rep->passes = 5;

  CC_TRY(link_collect(dev, rep, cpu));
  rep->bytes_tested = (long long)bytes;
  rep->pull_gbps = link_gbps(bytes, rep->pull_ms);
  rep->push_gbps = link_gbps(bytes, rep->push_ms);
  rep->h2d_gbps = link_gbps(bytes, rep->h2d_ms);
  rep->d2h_gbps = link_gbps(bytes, rep->d2h_ms);
  rep->duplex_pull_gbps = link_gbps(half, rep->duplex_ms);
  rep->duplex_push_gbps = link_gbps(bytes - half, rep->duplex_ms);
  return 0;
}

// One direction over caller-owned host memory `ptr` (device address
// `dptr`), for cc_host_step. engine 0: link_pull / link_push on the
// mapped range. engine 1: the runtime's copy to or from a staging buffer
// that lives for the call, with march_step on the staging buffer; only
// the copy is timed.
static int probe_host_step(DeviceCtx& dev, CcHostReport* rep, HostWindow& win,
                           void* ptr, void* dptr, int check, int write,
                           int cu_count) {
  const unsigned long long bytes = rep->bytes_requested;
  HbmMarchResult* const dRes = dev.host.dRes;
  CC_TRY(link_reset(dev, rep));
  double* ms;
  double* gbps;
  if (rep->engine == 0) {
    ms = check >= 0 ? &rep->pull_ms : &rep->push_ms;
    gbps = check >= 0 ? &rep->pull_gbps : &rep->push_gbps;
    CC_TRY(timed_ms(dev, rep, ms, [&] {
      launch_link(check, write, dptr, bytes, rep->origin, 0, dRes, 0);
      return 0;
    }));
    CC_CHECK(hipGetLastError());
  } else {
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t e = win.staging.ensure(bytes);
    rep->alloc_ms = std::chrono::duration<double, std::milli>(
                        std::chrono::steady_clock::now() - t0)
                        .count();
    if (e != hipSuccess) {
      (void)hipGetLastError();
      snprintf(rep->error, sizeof(rep->error),
               "allocated 0 of %llu bytes of device staging", bytes);
      return 0;
    }
    void* const D = win.staging.p;
    if (check >= 0) {
      ms = &rep->h2d_ms, gbps = &rep->h2d_gbps;
      CC_TRY(timed_ms(dev, rep, ms, [&] {
        CC_CHECK(hipMemcpyAsync(D, ptr, bytes, hipMemcpyHostToDevice, 0));
        return 0;
      }));
      launch_march(check, -1, D, bytes, rep->origin, 0, dRes, 0, cu_count);
      CC_CHECK(hipGetLastError());
    } else {
      ms = &rep->d2h_ms, gbps = &rep->d2h_gbps;
      launch_march(-1, write, D, bytes, rep->origin, 0, dRes, 0, cu_count);
      CC_CHECK(hipGetLastError());
      CC_TRY(timed_ms(dev, rep, ms, [&] {
        CC_CHECK(hipMemcpyAsync(ptr, D, bytes, hipMemcpyDeviceToHost, 0));
        return 0;
      }));
    }
    CC_CHECK(hipDeviceSynchronize());
  }
  HbmMarchResult none = {};
  none.first_bad_offset = ~0ull;
  CC_TRY(link_collect(dev, rep, none));
  *gbps = link_gbps(bytes, *ms);
  rep->passes = 1;
  rep->bytes_tested = (long long)bytes;
  return 0;
}
