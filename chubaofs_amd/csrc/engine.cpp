// engine.cpp -- RSEngine / ECEncoder / LrcEncoder host logic (see engine.hpp).
#include <atomic>
#include <chrono>
#include <thread>

#include "engine.hpp"

#include <algorithm>
#include <cstring>
#include <map>
#include <optional>
#include <shared_mutex>
#include <unordered_map>
#include <utility>

namespace cfsec {

namespace {
thread_local std::string t_last_error;

size_t first_size(const cfsec_shard* shards, int n) {
  for (int i = 0; i < n; ++i)
    if (shards[i].len != 0) return shards[i].len;
  return 0;
}

}  // namespace

// KRS/reedsolomon.go:1314-1339 checkShards / shardSize.
Status check_shards(const cfsec_shard* shards, int n, bool nilok, size_t* size) {
  size_t s = 0;
  for (int i = 0; i < n; ++i)
    if (shards[i].len != 0) {
      s = shards[i].len;
      break;
    }
  if (s == 0) return CFSEC_ERR_SHARD_NO_DATA;
  for (int i = 0; i < n; ++i)
    if (shards[i].len != s && (shards[i].len != 0 || !nilok)) return CFSEC_ERR_SHARD_SIZE;
  *size = s;
  return CFSEC_OK;
}

// ec.fillFullShards (encoder.go:199-210).  Go allocates when cap is short; across the
// C ABI the caller must hand in buffers with enough capacity.
Status fill_full_shards(cfsec_shard* shards, int n) {
  const size_t s = first_size(shards, n);
  for (int i = 0; i < n; ++i)
    if (shards[i].len == 0) {
      if (s != 0 && (shards[i].cap < s || shards[i].data == nullptr)) {
        set_last_error("fillFullShards: shard " + std::to_string(i) + " has cap < shard size");
        return CFSEC_ERR_INVALID_ARG;
      }
      shards[i].len = s;
    }
  return CFSEC_OK;
}

// ec.initBadShards (encoder.go:182-188).
Status init_bad_shards(cfsec_shard* shards, int n, const std::vector<int>& bad) {
  for (int i : bad) {
    if (i < 0 || i >= n) {
      set_last_error("bad shard index out of range");
      return CFSEC_ERR_INVALID_ARG;
    }
    if (shards[i].data != nullptr && shards[i].len != 0 && shards[i].cap > 0) shards[i].len = 0;
  }
  return CFSEC_OK;
}

namespace {

// codemode.Tactic.IsValid (codemode.go:267-271).
bool tactic_valid(const cfsec_tactic& t) {
  return t.n > 0 && t.m > 0 && t.l >= 0 && t.az_count > 0 && t.put_quorum > 0 &&
         t.get_quorum >= 0 && t.min_shard_size >= 0 && t.n % t.az_count == 0 &&
         t.m % t.az_count == 0 && t.l % t.az_count == 0;
}

// codemode.Tactic.GetECLayoutByAZ (codemode.go:274-291).
std::vector<std::vector<int>> layout_by_az(const cfsec_tactic& t) {
  std::vector<std::vector<int>> az(t.az_count);
  const int n = t.n / t.az_count, m = t.m / t.az_count, l = t.l / t.az_count;
  for (int idx = 0; idx < t.az_count; ++idx) {
    for (int i = 0; i < n; ++i) az[idx].push_back(idx * n + i);
    for (int i = 0; i < m; ++i) az[idx].push_back(t.n + idx * m + i);
    for (int i = 0; i < l; ++i) az[idx].push_back(t.n + t.m + idx * l + i);
  }
  return az;
}
}  // namespace

void set_last_error(const std::string& msg) { t_last_error = msg; }
const char* last_error_cstr() { return t_last_error.c_str(); }

Status hip_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return CFSEC_OK;
  set_last_error(std::string(what) + ": " + hipGetErrorString(e));
  return CFSEC_ERR_DEVICE;
}

Status lane_wait(hipEvent_t ev, hipStream_t from, hipStream_t to) {
  const Status e = hip_status(hipEventRecord(ev, from), "hipEventRecord");
  return e != CFSEC_OK ? e : hip_status(hipStreamWaitEvent(to, ev, 0), "hipStreamWaitEvent");
}

// ---------------------------------------------------------------- devices

DeviceGuard::DeviceGuard(int device) {
  if (hipGetDevice(&prev_) != hipSuccess) return;
  if (prev_ != device && hipSetDevice(device) != hipSuccess) return;
  ok_ = true;
}
DeviceGuard::~DeviceGuard() {
  if (ok_) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != prev_) (void)hipSetDevice(prev_);
  }
}

DeviceContext* DeviceContext::get(int device, int slot) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, std::unique_ptr<DeviceContext>> ctxs;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count || slot < 0) return nullptr;
  std::lock_guard<std::mutex> l(mu);
  auto& p = ctxs[{device, slot}];
  if (!p) p.reset(new DeviceContext(device));
  return p.get();
}

Status DeviceContext::acquire(size_t bytes, size_t nflags, Workspace** out, size_t nbflags, size_t ncrc) {
  Workspace* ws = nullptr;
  bool wait = false;
  {
    std::lock_guard<std::mutex> l(mu_);
    // a workspace an asynchronous call returned is free once its stream has passed the call
    const auto ready = [](Workspace* w) {
      if (!w->pending) return true;
      const hipError_t q = hipEventQuery(w->done);
      if (q == hipErrorNotReady) return false;
      (void)hipGetLastError();
      w->pending = false;
      return true;
    };
    // best fit among the free workspaces
    auto best = free_.end();
    for (auto it = free_.begin(); it != free_.end(); ++it)
      if ((*it)->cap >= bytes && (*it)->nflags >= nflags && (*it)->nbflags >= nbflags && (*it)->ncrc >= ncrc &&
          (best == free_.end() || (*it)->cap < (*best)->cap) && ready(*it))
        best = it;
    if (best == free_.end())
      for (auto it = free_.begin(); it != free_.end() && best == free_.end(); ++it)
        if (ready(*it)) best = it;
    if (best != free_.end()) {
      ws = *best;
      free_.erase(best);
    } else if (all_.size() >= kMaxWorkspaces && !free_.empty()) {
      // every free workspace is still pending on an asynchronous call's stream: wait for the
      // oldest one instead of growing without bound (each holds streams, events, pinned words)
      ws = free_.front();
      free_.erase(free_.begin());
      wait = true;
    } else {
      all_.emplace_back(new Workspace());
      ws = all_.back().get();
    }
  }
  if (wait) {
    if (hipEventSynchronize(ws->done) != hipSuccess) {
      (void)hipGetLastError();
      DeviceGuard dg(device_);
      (void)hipDeviceSynchronize();
    }
    ws->pending = false;
  }
  DeviceGuard g(device_);
  if (!g.ok()) {
    release(ws);
    return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  }
  Status st = CFSEC_OK;
  // Non-blocking streams: work on them does not wait for (or hold up) the legacy default stream,
  // so concurrent callers overlap.  A device-memory call without a caller stream orders itself
  // after the default stream explicitly (order_after_default).
  if (!ws->stream) st = hip_status(hipStreamCreateWithFlags(&ws->stream, hipStreamNonBlocking), "hipStreamCreate");
  if (st == CFSEC_OK && !ws->stream2)
    st = hip_status(hipStreamCreateWithFlags(&ws->stream2, hipStreamNonBlocking), "hipStreamCreate");
  if (st == CFSEC_OK && !ws->ev)
    st = hip_status(hipEventCreateWithFlags(&ws->ev, hipEventDisableTiming), "hipEventCreate");
  if (st == CFSEC_OK && !ws->ev_in)
    st = hip_status(hipEventCreateWithFlags(&ws->ev_in, hipEventDisableTiming), "hipEventCreate");
  if (st == CFSEC_OK && ws->cap < bytes) {
    if (ws->dbuf) (void)hipFree(ws->dbuf);
    ws->dbuf = nullptr;
    ws->cap = 0;
    st = hip_status(hipMalloc(reinterpret_cast<void**>(&ws->dbuf), bytes), "hipMalloc(staging)");
    if (st == CFSEC_OK) ws->cap = bytes;
  }
  if (st == CFSEC_OK && ws->nflags < nflags) {
    const size_t nf = std::max<size_t>(nflags, 64);
    if (ws->dflags) (void)hipFree(ws->dflags);
    if (ws->hflags) (void)hipHostFree(ws->hflags);
    ws->dflags = nullptr;
    ws->hflags = nullptr;
    ws->hflags_dev = nullptr;
    ws->nflags = 0;
    st = hip_status(hipMalloc(reinterpret_cast<void**>(&ws->dflags), nf * 4), "hipMalloc(flags)");
    if (st == CFSEC_OK)
      st = hip_status(hipHostMalloc(reinterpret_cast<void**>(&ws->hflags), nf * 4,
                                    hipHostMallocMapped | hipHostMallocCoherent),
                      "hipHostMalloc(flags)");
    if (st == CFSEC_OK)
      st = hip_status(hipHostGetDevicePointer(reinterpret_cast<void**>(&ws->hflags_dev), ws->hflags, 0),
                      "hipHostGetDevicePointer(flags)");
    if (st == CFSEC_OK) ws->nflags = nf;
  }
  if (st == CFSEC_OK && ws->nbflags < nbflags) {
    const size_t nf = std::max<size_t>(nbflags, 256);
    if (ws->bflags) (void)hipFree(ws->bflags);
    ws->bflags = nullptr;
    ws->nbflags = 0;
    ws->bflags_clean = false;
    st = hip_status(hipMalloc(reinterpret_cast<void**>(&ws->bflags), nf * 4), "hipMalloc(batch flags)");
    if (st == CFSEC_OK) ws->nbflags = nf;
  }
  if (st == CFSEC_OK && ws->bflags && !ws->bflags_clean) {
    // once per allocation (or after a failed call): the gather kernel keeps them zero afterwards
    st = hip_status(hipMemset(ws->bflags, 0, ws->nbflags * 4), "hipMemset(batch flags)");
    if (st == CFSEC_OK) ws->bflags_clean = true;
  }
  if (st == CFSEC_OK && ws->ncrc < ncrc) {
    const size_t nc = std::max<size_t>(ncrc, 256);
    if (ws->dcrc) (void)hipFree(ws->dcrc);
    if (ws->hcrc) (void)hipHostFree(ws->hcrc);
    ws->dcrc = nullptr;
    ws->hcrc = nullptr;
    ws->ncrc = 0;
    st = hip_status(hipMalloc(reinterpret_cast<void**>(&ws->dcrc), nc * 4), "hipMalloc(crc words)");
    if (st == CFSEC_OK)
      st = hip_status(hipHostMalloc(reinterpret_cast<void**>(&ws->hcrc), nc * 4, hipHostMallocCoherent),
                      "hipHostMalloc(crc words)");
    if (st == CFSEC_OK) ws->ncrc = nc;
  }
  if (st == CFSEC_OK && !ws->done)
    st = hip_status(hipEventCreateWithFlags(&ws->done, hipEventDisableTiming), "hipEventCreate");
  if (st != CFSEC_OK) {
    release(ws);
    return st;
  }
  *out = ws;
  return CFSEC_OK;
}

Status DeviceContext::order_after_default(Workspace* ws) {
  // Nothing queued on the legacy null stream is still pending (the common case: a caller that does
  // not use it, e.g. the Go shim on HBM shards): no ordering to add.  Work another thread queues
  // there after this query is concurrent with this call, not before it.  Saves the event record +
  // cross-stream wait, ~6 us of host time and ~3 us of GPU-side dependency per synchronous call
  // (tools/seg_latency.hip: 24-25 -> 13-14 us per NULL-stream ReconstructData of a 64 KiB segment).
  const hipError_t q = hipStreamQuery(nullptr);
  if (q == hipSuccess) return CFSEC_OK;
  if (q != hipErrorNotReady) (void)hipGetLastError();
  // An event recorded on the legacy null stream completes after everything queued before it on
  // that stream and on every blocking stream of the device.
  Status st = hip_status(hipEventRecord(ws->ev_in, nullptr), "hipEventRecord(null stream)");
  if (st == CFSEC_OK) st = hip_status(hipStreamWaitEvent(ws->stream, ws->ev_in, 0), "hipStreamWaitEvent");
  return st;
}

void DeviceContext::release(Workspace* ws) {
  std::lock_guard<std::mutex> l(mu_);
  free_.push_back(ws);
}

Status DeviceContext::reserve_mix(Workspace* ws, int slot, size_t bytes, hipStream_t stream) {
  Status st = CFSEC_OK;
  if (!ws->mix_ev[slot])
    st = hip_status(hipEventCreateWithFlags(&ws->mix_ev[slot], hipEventDisableTiming), "hipEventCreate");
  if (st != CFSEC_OK || ws->mix_cap[slot] >= bytes) return st;
  if (ws->mix_busy[slot]) {  // the lane's earlier copy and launch still use the tables
    st = hip_status(hipStreamSynchronize(stream), "hipStreamSynchronize(mix table)");
    ws->mix_busy[slot] = false;
    if (st != CFSEC_OK) return st;
  }
  const size_t cap = std::max(align_up(bytes, 4096), size_t(64) << 10);
  if (ws->hmix[slot]) (void)hipHostFree(ws->hmix[slot]);
  if (ws->dmix[slot]) (void)hipFree(ws->dmix[slot]);
  ws->hmix[slot] = ws->dmix[slot] = nullptr;
  ws->mix_cap[slot] = 0;
  st = hip_status(hipHostMalloc(reinterpret_cast<void**>(&ws->hmix[slot]), cap, hipHostMallocDefault),
                  "hipHostMalloc(mix table)");
  if (st == CFSEC_OK) st = hip_status(hipMalloc(reinterpret_cast<void**>(&ws->dmix[slot]), cap), "hipMalloc(mix table)");
  if (st == CFSEC_OK) ws->mix_cap[slot] = cap;
  return st;
}

// CFSEC_SYNC_POLL=0 (or cfsec_set_sync_poll(0)): hipStreamSynchronize always (A/B, tests)
std::atomic<int>& sync_poll_mode() {
  static std::atomic<int> mode{[] {
    const char* v = std::getenv("CFSEC_SYNC_POLL");
    return (v && v[0] == '0') ? 0 : 1;
  }()};
  return mode;
}

Status DeviceContext::finish(Workspace* ws, hipStream_t stream) {
  const auto blocking = [&] { return hip_status(hipStreamSynchronize(stream), "hipStreamSynchronize"); };
  if (!sync_poll_mode().load(std::memory_order_relaxed)) return blocking();
  if (!ws->hmark) {
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
      (void)hipGetLastError();
      return blocking();
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipHostFree(h);
      return blocking();
    }
    ws->hmark = static_cast<uint32_t*>(h);
    ws->dmark = static_cast<uint32_t*>(d);
    __atomic_store_n(ws->hmark, 0u, __ATOMIC_RELEASE);
    ws->seq = 0;
  }
  const uint32_t seq = ++ws->seq;
  if (hipStreamWriteValue32(stream, ws->dmark, seq, 0) != hipSuccess) {
    (void)hipGetLastError();
    return blocking();
  }
  // The marker is written after the call's kernels and copies on this stream; the words the caller
  // reads next (hflags, hcrc) are coherent host memory, so they are visible once the marker is.
  // Busy-polling for the first kSpinBusyUs (a call's own latency), yielding the core after that.
  const auto t0 = std::chrono::steady_clock::now();
  bool busy = true;
  for (uint32_t spin = 0;; ++spin) {
    if (__atomic_load_n(ws->hmark, __ATOMIC_ACQUIRE) == seq) return CFSEC_OK;
    if (busy) __builtin_ia32_pause();
    else std::this_thread::yield();
    if ((spin & 255u) == 255u) {
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      if (us > kSpinLimitUs) return blocking();
      busy = us < kSpinBusyUs;
    }
  }
}

void DeviceContext::release_after(Workspace* ws, hipStream_t stream) {
  // if the record fails the stream's work is unknown: wait for the device before reuse
  if (hipEventRecord(ws->done, stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
    ws->pending = false;
  } else {
    ws->pending = true;
  }
  release(ws);
}

// ---------------------------------------------------------------- synchronous call scope

SyncCall::SyncCall(DeviceContext* ctx, size_t bytes, size_t nflags, hipStream_t caller, bool after_default)
    : guard_(ctx->device()), ctx_(ctx) {
  if (!guard_.ok()) {
    st_ = hip_status(hipErrorInvalidDevice, "hipSetDevice");
    return;
  }
  st_ = ctx_->acquire(bytes, nflags, &ws_);
  if (st_ != CFSEC_OK) return;
  stream_ = caller ? caller : ws_->stream;
  if (after_default) st_ = ctx_->order_after_default(ws_);
}

Status SyncCall::finish() {
  if (!ws_ || finished_) return st_;
  finished_ = true;
  const std::string first = st_ != CFSEC_OK ? last_error_cstr() : "";
  Status sync = ctx_->finish(ws_, stream_);
  if (two_lanes_) {
    const Status second = ctx_->finish(ws_, ws_->stream2);
    if (sync == CFSEC_OK) sync = second;
  }
  if (st_ == CFSEC_OK) st_ = sync;
  else set_last_error(first);  // a failed wait after a failed step: the step's text stays
  return st_;
}

SyncCall::~SyncCall() {
  if (!ws_) return;
  finish();
  ctx_->release(ws_);
}

// ---------------------------------------------------------------- inversion cache

bool InversionCache::get(const std::vector<int>& invalid, Matrix* out) const {
  std::shared_lock<std::shared_mutex> l(mu_);
  auto it = map_.find(invalid);
  if (it == map_.end()) return false;
  *out = it->second;
  return true;
}

void InversionCache::put(const std::vector<int>& invalid, const Matrix& m) {
  std::unique_lock<std::shared_mutex> l(mu_);
  map_.emplace(invalid, m);
}

// ---------------------------------------------------------------- RSEngine

Status RSEngine::create(int k, int m, int device, std::unique_ptr<RSEngine>* out) {
  // KRS/reedsolomon.go:413-447.  More than 256 shards switches the reference to its
  // leopard GF(2^16) codec, which CubeFS never reaches (max 38 shards).
  if (k + m > 256) return CFSEC_ERR_NOT_SUPPORTED;
  if (k <= 0 || m < 0) return CFSEC_ERR_INV_SHARD_NUM;
  std::unique_ptr<RSEngine> e(new RSEngine());
  e->k_ = k;
  e->m_ = m;
  if (m > 0) {
    if (!build_matrix(k, k + m, e->mat_)) return CFSEC_ERR_SINGULAR;
  } else {
    e->mat_ = Matrix(k, k);
    for (int i = 0; i < k; ++i) e->mat_.at(i, i) = 1;
  }
  e->parity_ = Matrix(m, k);
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < k; ++c) e->parity_.at(r, c) = e->mat_.at(k + r, c);
  if (device < 0) {
    int cur = 0;
    int count = 0;
    if (hipGetDeviceCount(&count) == hipSuccess && count > 0 && hipGetDevice(&cur) == hipSuccess)
      device = cur;
  }
  // A missing device is reported by the first call that needs it (CFSEC_ERR_DEVICE); the
  // host-only methods (matrix, Split, Join) work without one.
  e->ctx_ = device >= 0 ? DeviceContext::get(device) : nullptr;
  if (e->ctx_) e->devs_.push_back(e->ctx_);
  *out = std::move(e);
  return CFSEC_OK;
}

// crc32.ChecksumIEEE of n rows of S bytes as they stand into crcs[idx[i]] (idx null: crcs[i]), the
// nwords words zeroed first; S == 0: the words zeroed, nothing launched (ChecksumIEEE(nil) == 0).
static Status crc_rows_as_they_stand(const uint8_t* const* ptrs, int n, size_t S, uint32_t* crcs, size_t nwords,
                                     const uint32_t* idx, hipStream_t stream) {
  const Status st = hip_status(hipMemsetAsync(crcs, 0, sizeof(uint32_t) * nwords, stream), "hipMemsetAsync");
  if (st != CFSEC_OK || S == 0) return st;
  return hip_status(launch_crc32_to(ptrs, S, n, crcs, idx, crc32_shift_ones(S), stream), "launch_crc32_to");
}

// Product + checksums: the fused kernel where it takes the job, else the product then the
// standalone CRC kernel over the same shards (one more read of each).
static Status matvec_with_crc(const MatVecJob& job, uint8_t* const* ptrs, int total, const std::vector<int>& slot,
                              size_t S, uint32_t* crcs, hipStream_t stream) {
  if (matvec_crc_accepts(job, total, slot.data()))
    return hip_status(launch_matvec_crc(job, crcs, total, slot.data(), stream), "launch_matvec_crc");
  const Status st = hip_status(launch_matvec(job, stream), "launch_matvec");
  if (st != CFSEC_OK) return st;
  std::vector<const uint8_t*> p;
  std::vector<uint32_t> idx;
  const bool cin = slot[0] >= 0;
  for (int s = 0; s < job.nstripes; ++s)
    for (int i = 0; i < job.k + job.m; ++i) {
      if (i < job.k && !cin) continue;
      p.push_back(i < job.k ? job.in[(size_t)s * job.k + i] : job.out[(size_t)s * job.m + i - job.k]);
      idx.push_back((uint32_t)(s * total + slot[i]));
    }
  return crc_rows_as_they_stand(p.data(), (int)p.size(), S, crcs, (size_t)total * job.nstripes, idx.data(), stream);
}

// The device address of page-locked host memory (hipHostMalloc / cfsec_host_alloc); false for
// pageable memory.
namespace {
struct HostRange {
  size_t size;
  uint8_t* dev;  // device address of the base
};
struct HostRanges {
  std::shared_mutex mu;
  std::map<uintptr_t, HostRange> by_base;
};
HostRanges& host_ranges() {
  static HostRanges r;
  return r;
}
}  // namespace

void host_range_add(void* base, size_t size) {
  hipPointerAttribute_t attr;
  if (!base || hipPointerGetAttributes(&attr, base) != hipSuccess || !attr.devicePointer) {
    (void)hipGetLastError();
    return;
  }
  HostRanges& r = host_ranges();
  std::unique_lock<std::shared_mutex> lk(r.mu);
  r.by_base[(uintptr_t)base] = HostRange{size, static_cast<uint8_t*>(attr.devicePointer)};
}

void host_range_remove(void* base) {
  HostRanges& r = host_ranges();
  std::unique_lock<std::shared_mutex> lk(r.mu);
  r.by_base.erase((uintptr_t)base);
}

// Page-locked staging for small pageable host calls (RSEngine::run): a free list of cfsec-owned
// hipHostMalloc blocks (registered in the host-range registry, so the zero-copy path takes them),
// one per concurrent call, kept for reuse.
namespace {
struct PinnedStages {
  std::mutex mu;
  std::vector<std::pair<uint8_t*, size_t>> free;
};
PinnedStages& pinned_stages() {
  static PinnedStages p;
  return p;
}
}  // namespace

static std::pair<uint8_t*, size_t> pinned_stage_take(size_t bytes) {
  PinnedStages& p = pinned_stages();
  {
    std::lock_guard<std::mutex> lk(p.mu);
    for (size_t i = 0; i < p.free.size(); ++i)
      if (p.free[i].second >= bytes) {
        const auto b = p.free[i];
        p.free.erase(p.free.begin() + (long)i);
        return b;
      }
  }
  const size_t cap = std::max<size_t>(bytes, (size_t)256 << 10);
  void* h = nullptr;
  if (hipHostMalloc(&h, cap, hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    return {nullptr, 0};
  }
  host_range_add(h, cap);
  return {static_cast<uint8_t*>(h), cap};
}

static void pinned_stage_give(std::pair<uint8_t*, size_t> b) {
  if (!b.first) return;
  PinnedStages& p = pinned_stages();
  std::lock_guard<std::mutex> lk(p.mu);
  p.free.push_back(b);
}

bool device_alias(uint8_t* p, uint8_t** dptr) {
  {
    HostRanges& r = host_ranges();
    std::shared_lock<std::shared_mutex> lk(r.mu);
    if (!r.by_base.empty()) {
      auto it = r.by_base.upper_bound((uintptr_t)p);
      if (it != r.by_base.begin()) {
        --it;
        const uintptr_t off = (uintptr_t)p - it->first;
        if (off < it->second.size) {
          *dptr = it->second.dev + off;
          return true;
        }
      }
    }
  }
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (attr.type != hipMemoryTypeHost || !attr.devicePointer) return false;
  const uint8_t* hbase = static_cast<const uint8_t*>(attr.hostPointer);
  *dptr = static_cast<uint8_t*>(attr.devicePointer) + (hbase ? p - hbase : 0);
  return true;
}

// Verify with more inputs than one launch carries: computed into staging, then compared (wide_verify).
static bool two_step_verify(MatVecMode mode, int nin) { return mode == MatVecMode::kVerify && nin > 32; }

CallPath single_call_path(bool host, bool rows_aliasable, bool stage_usable, size_t moved_bytes, int nin,
                          MatVecMode mode) {
  if (!host) return CallPath::kInPlace;
  if (rows_aliasable) return CallPath::kPinnedInPlace;
  if (two_step_verify(mode, nin)) return CallPath::kStagedWhole;
  return moved_bytes <= RSEngine::kSmallPageable && stage_usable ? CallPath::kSmallStage : CallPath::kPipeline;
}

namespace {
std::vector<int> index_range(int a, int b) {
  std::vector<int> v;
  for (int i = a; i < b; ++i) v.push_back(i);
  return v;
}

// Device addresses of n rows: device memory as is, host memory through device_alias.  False at
// the first host row that is not page-locked (the rows from it on are left unresolved).
bool resolve_rows(cfsec_shard* const* rows, int n, bool host, uint8_t** dptr) {
  for (int i = 0; i < n; ++i)
    if (!host) dptr[i] = rows[i]->data;
    else if (!device_alias(rows[i]->data, &dptr[i])) return false;
  return true;
}

// The two-step Verify over d (device addresses: the rows.cols inputs, then the outputs): the product
// stored into tmp0 (a slot per output row), then compared with the outputs through an identity matrix.
void wide_verify(SyncCall& call, const Matrix& rows, uint8_t* const* d, size_t S, uint8_t* tmp0) {
  const int nout = rows.rows;
  std::vector<uint8_t*> tmp(nout);
  for (int r = 0; r < nout; ++r) tmp[r] = tmp0 + align_up(S, kSlotAlign) * r;
  MatVecJob job = matvec_job(rows.cols, nout, rows.v.data(), S, 1, d, tmp.data());
  job.flags = call.ws()->dflags;
  call.step("launch_matvec", [&] { return launch_matvec(job, call.stream()); });
  Matrix ident(nout, nout);
  for (int r = 0; r < nout; ++r) ident.at(r, r) = 1;
  MatVecJob cmp = matvec_job(nout, nout, ident.v.data(), S, 1, tmp.data(), d + rows.cols);
  cmp.flags = job.flags;
  cmp.mode = MatVecMode::kVerify;
  call.step("launch_matvec(verify)", [&] { return launch_matvec(cmp, call.stream()); });
}

// The product of a call over rows the GPU addresses (d as above; through tmp0 when given: the wide
// Verify), and Verify's word on its way back.
void issue_product(SyncCall& call, const Matrix& rows, uint8_t* const* d, size_t S, MatVecMode mode, uint8_t* tmp0) {
  const bool verify = mode == MatVecMode::kVerify;
  DeviceContext::Workspace* ws = call.ws();
  if (verify) call.memset(ws->dflags, 0, 4);
  if (tmp0) {
    wide_verify(call, rows, d, S, tmp0);
  } else {
    MatVecJob job = matvec_job(rows.cols, rows.rows, rows.v.data(), S, 1, d, d + rows.cols);
    job.flags = ws->dflags;
    job.mode = mode;
    call.step("launch_matvec", [&] { return launch_matvec(job, call.stream()); });
  }
  if (verify) call.fetch_words(1);
}

// The wait of a call whose product is issued, and what Verify's word says.
Status finish_product(SyncCall& call, MatVecMode mode, bool* ok) {
  std::optional<HostTimer> tm("  run: finish");
  const Status st = call.finish();
  tm.reset();
  if (st == CFSEC_OK && mode == MatVecMode::kVerify && ok) *ok = call.ws()->hflags[0] == 0;
  return st;
}
}  // namespace

Status RSEngine::run(const Matrix& rows, const std::vector<cfsec_shard*>& ins,
                     const std::vector<cfsec_shard*>& outs, size_t S, int mem, hipStream_t stream,
                     MatVecMode mode, bool* ok) {
  if (ok) *ok = true;
  if (outs.empty() || S == 0) return CFSEC_OK;
  if (!ctx_) {
    set_last_error("no HIP device available to the cfsec engine");
    return CFSEC_ERR_DEVICE;
  }
  if (mem != CFSEC_MEM_HOST && mem != CFSEC_MEM_DEVICE) return CFSEC_ERR_INVALID_ARG;
  std::vector<cfsec_shard*> all(ins);  // the call's rows: the inputs, then the outputs
  all.insert(all.end(), outs.begin(), outs.end());
  for (auto* s : all)
    if (!s->data) return CFSEC_ERR_INVALID_ARG;
  const int nin = (int)ins.size(), n = (int)all.size();
  if (rows.rows != n - nin || rows.cols != nin) return CFSEC_ERR_INVALID_ARG;

  // the facts: where the rows are, and for a small pageable call whether there is a stage for it
  const bool host = mem == CFSEC_MEM_HOST;
  const size_t moved = S * size_t(n);
  std::optional<DeviceGuard> g;  // a host call's facts ask the runtime; a device call's do not
  if (host) {
    g.emplace(ctx_->device());
    if (!g->ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  }
  std::vector<uint8_t*> d(n);
  const bool aliasable = resolve_rows(all.data(), n, host, d.data());
  CallPath path = single_call_path(host, aliasable, true, moved, nin, mode);
  std::pair<uint8_t*, size_t> stage{nullptr, 0};
  uint8_t* dstage = nullptr;
  if (path == CallPath::kSmallStage) {
    // the stage's device address, resolved once; a stage the GPU cannot address goes back at once
    stage = pinned_stage_take(moved);
    if (!stage.first || !device_alias(stage.first, &dstage)) {
      pinned_stage_give(std::exchange(stage, {}));
      path = single_call_path(host, aliasable, false, moved, nin, mode);
    }
  }
  Status st = CFSEC_OK;
  switch (path) {
    case CallPath::kInPlace: st = run_in_place(rows, d.data(), S, stream, mode, ok); break;
    case CallPath::kPinnedInPlace: st = run_in_place(rows, d.data(), S, nullptr, mode, ok); break;
    case CallPath::kSmallStage: st = run_small_stage(rows, all, S, mode, ok, stage.first, dstage); break;
    case CallPath::kPipeline: st = run_host(rows, ins, outs, S, mode, ok); break;
    case CallPath::kStagedWhole: st = run_staged_verify(rows, all, S, ok); break;
  }
  pinned_stage_give(stage);
  return st;
}

// Page-locked buffers (cfsec_host_alloc) are device-addressable: the kernel reads and writes them
// over PCIe with no staging copies (tools/bench_host.py: 50.7 GB/s of data for EC12P4 encode vs
// 32.4 through the staged pipeline and 26.7 from pageable memory).  A NULL stream: the call runs on
// the workspace's stream, ordered after the legacy default stream.
Status RSEngine::run_in_place(const Matrix& rows, uint8_t* const* d, size_t S, hipStream_t stream, MatVecMode mode,
                              bool* ok) {
  const bool wide = two_step_verify(mode, rows.cols);
  std::unique_ptr<HostTimer> tm(new HostTimer("  run: acquire"));
  SyncCall call(ctx_, wide ? align_up(S, kSlotAlign) * size_t(rows.rows) : 0, 1, stream, !stream);
  if (!call.begun()) return call.status();
  tm.reset(new HostTimer("  run: copies + launch"));
  issue_product(call, rows, d, S, mode, wide ? call.ws()->dbuf : nullptr);
  tm.reset();
  return finish_product(call, mode, ok);
}

// Small pageable calls (a degraded range read's segments): the rows copied on the CPU into
// page-locked staging and coded there in place, instead of HIP's staged copies of pageable memory
// (~130 us per call whatever the size up to 64 KiB, profiles/r06/bench_s1).
Status RSEngine::run_small_stage(const Matrix& rows, const std::vector<cfsec_shard*>& all, size_t S, MatVecMode mode,
                                 bool* ok, uint8_t* stage, uint8_t* dstage) {
  const int nin = rows.cols, n = (int)all.size();
  std::vector<uint8_t*> d(n);
  for (int i = 0; i < n; ++i) {
    if (i < nin || mode != MatVecMode::kStore) std::memcpy(stage + S * i, all[i]->data, S);
    d[i] = dstage + S * i;
  }
  const Status st = run_in_place(rows, d.data(), S, nullptr, mode, ok);
  if (st == CFSEC_OK && mode != MatVecMode::kVerify)
    for (int i = nin; i < n; ++i) std::memcpy(all[i]->data, stage + S * i, S);
  return st;
}

Status RSEngine::run_staged_verify(const Matrix& rows, const std::vector<cfsec_shard*>& all, size_t S, bool* ok) {
  const int n = (int)all.size();
  const size_t slot = align_up(S, kSlotAlign);
  std::unique_ptr<HostTimer> tm(new HostTimer("  run: acquire"));
  SyncCall call(ctx_, slot * size_t(n + rows.rows), 1, nullptr, false);
  if (!call.begun()) return call.status();
  tm.reset(new HostTimer("  run: copies + launch"));
  std::vector<uint8_t*> d(n);
  for (int i = 0; i < n; ++i) {
    d[i] = call.ws()->dbuf + slot * i;
    call.copy(d[i], all[i]->data, S, hipMemcpyHostToDevice);
  }
  issue_product(call, rows, d.data(), S, MatVecMode::kVerify, call.ws()->dbuf + slot * size_t(n));
  tm.reset();
  return finish_product(call, MatVecMode::kVerify, ok);
}

namespace {
// Rows of a host call that sit at one stride from each other (ec.Buffer carves its shards at
// stride S from one allocation, common/ec/buf.go:83-84): one 2-D copy moves all of them.
int64_t host_row_stride(const std::vector<cfsec_shard*>& rows) {
  if (rows.size() < 2) return 0;
  const int64_t st = (int64_t)(uintptr_t)rows[1]->data - (int64_t)(uintptr_t)rows[0]->data;
  if (st <= 0) return 0;
  for (size_t i = 2; i < rows.size(); ++i)
    if ((int64_t)(uintptr_t)rows[i]->data - (int64_t)(uintptr_t)rows[0]->data != st * (int64_t)i) return 0;
  return st;
}

hipError_t copy_rows(const std::vector<cfsec_shard*>& rows, int64_t hstride, size_t off, size_t len,
                     uint8_t* dev, size_t dpitch, bool h2d, hipStream_t s) {
  if (rows.empty()) return hipSuccess;
  if (hstride > 0 && (size_t)hstride >= len) {
    return h2d ? hipMemcpy2DAsync(dev, dpitch, rows[0]->data + off, (size_t)hstride, len, rows.size(),
                                  hipMemcpyHostToDevice, s)
               : hipMemcpy2DAsync(rows[0]->data + off, (size_t)hstride, dev, dpitch, len, rows.size(),
                                  hipMemcpyDeviceToHost, s);
  }
  for (size_t i = 0; i < rows.size(); ++i) {
    hipError_t e = h2d ? hipMemcpyAsync(dev + i * dpitch, rows[i]->data + off, len, hipMemcpyHostToDevice, s)
                       : hipMemcpyAsync(rows[i]->data + off, dev + i * dpitch, len, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
}  // namespace

// Host-memory call: the shard columns go through HBM in chunks of kHostChunk bytes per row,
// alternating over two streams, so chunk j+1's host->device copies, chunk j's kernel and chunk
// j-1's device->host copies overlap (the copy engines of each direction and the CUs run
// concurrently; PCIe Gen5 x16 is the bound).  Buffers from cfsec_host_alloc (pinned) DMA
// directly; pageable ones go through HIP's staging.  Chunks of one stream reuse its staging
// region, which that stream's order makes safe.
Status RSEngine::run_host(const Matrix& rows, const std::vector<cfsec_shard*>& ins,
                          const std::vector<cfsec_shard*>& outs, size_t S, MatVecMode mode, bool* ok) {
  const int nin = (int)ins.size(), nout = (int)outs.size();
  const bool verify = mode == MatVecMode::kVerify;
  const size_t chunk = std::min(align_up(S, kSlotAlign), kHostChunk);
  const size_t nchunks = (S + chunk - 1) / chunk;
  const int nlanes = nchunks > 1 ? 2 : 1;
  const size_t per_lane = chunk * size_t(nin + nout);
  SyncCall call(ctx_, per_lane * nlanes, 1, nullptr, false);
  if (!call.begun()) return call.status();
  DeviceContext::Workspace* ws = call.ws();
  hipStream_t lane[2] = {call.stream(), nlanes > 1 ? call.second_lane() : nullptr};
  const int64_t in_stride = host_row_stride(ins), out_stride = host_row_stride(outs);
  if (verify) {
    call.memset(ws->dflags, 0, 4);
    if (nlanes > 1) call.step("lane_wait", [&] { return lane_wait(ws->ev, lane[0], lane[1]); });
  }
  std::vector<uint8_t*> d(nin + nout);  // a chunk's rows in its lane: the inputs, then the outputs
  for (size_t j = 0; j < nchunks && call.ok(); ++j) {
    const int l = (int)(j % nlanes);
    hipStream_t s = lane[l];
    uint8_t* base = ws->dbuf + per_lane * l;
    const size_t off = j * chunk, len = std::min(chunk, S - off);
    for (int i = 0; i < nin + nout; ++i) d[i] = base + chunk * i;
    MatVecJob job = matvec_job(nin, nout, rows.v.data(), len, 1, d.data(), d.data() + nin);
    job.mode = mode;
    job.flags = ws->dflags;
    // the outputs: in before a Verify's launch, out after any other
    const auto out_rows = [&] { return copy_rows(outs, out_stride, off, len, base + chunk * nin, chunk, verify, s); };
    call.step("hipMemcpyAsync H2D", [&] { return copy_rows(ins, in_stride, off, len, base, chunk, true, s); });
    if (verify) call.step("hipMemcpyAsync H2D", out_rows);
    call.step("launch_matvec", [&] { return launch_matvec(job, s); });
    if (!verify) call.step("hipMemcpyAsync D2H", out_rows);
  }
  if (verify && nlanes > 1) call.step("lane_wait", [&] { return lane_wait(ws->ev, lane[1], lane[0]); });
  if (verify) call.fetch_words(1);
  const Status st = call.finish();
  if (st == CFSEC_OK && verify && ok) *ok = ws->hflags[0] == 0;
  return st;
}

// Encode (kStore) and Verify (kVerify): the parity rows over the whole stripe.
Status RSEngine::code_stripe(cfsec_shard* shards, int n, int mem, hipStream_t stream, MatVecMode mode, bool* ok) {
  if (!shards || n != total()) return CFSEC_ERR_TOO_FEW_SHARDS;
  size_t S = 0;
  Status st = check_shards(shards, n, false, &S);
  if (st != CFSEC_OK) return st;
  std::vector<cfsec_shard*> ins, outs;
  for (int i = 0; i < k_; ++i) ins.push_back(&shards[i]);
  for (int i = k_; i < n; ++i) outs.push_back(&shards[i]);
  return run(parity_, ins, outs, S, mem, stream, mode, ok);
}

Status RSEngine::encode(cfsec_shard* shards, int n, int mem, hipStream_t stream) {
  return code_stripe(shards, n, mem, stream, MatVecMode::kStore, nullptr);
}

Status RSEngine::encode_crc(cfsec_shard* shards, int n, int mem, hipStream_t stream, uint32_t* crcs) {
  if (!shards || n != total()) return CFSEC_ERR_TOO_FEW_SHARDS;
  if (!crcs) return CFSEC_ERR_INVALID_ARG;
  size_t S = 0;
  Status st = check_shards(shards, n, false, &S);
  if (st != CFSEC_OK) return st;
  if (!ctx_) {
    set_last_error("no HIP device available to the cfsec engine");
    return CFSEC_ERR_DEVICE;
  }
  if (mem != CFSEC_MEM_HOST && mem != CFSEC_MEM_DEVICE) return CFSEC_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i)
    if (!shards[i].data) return CFSEC_ERR_INVALID_ARG;
  // device addresses of the shards: device memory as is, pinned host pages aliased (zero-copy),
  // pageable host memory staged whole through the workspace
  const bool host = mem == CFSEC_MEM_HOST;
  std::optional<DeviceGuard> g;
  if (host) {
    g.emplace(ctx_->device());
    if (!g->ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  }
  std::vector<cfsec_shard*> all(n);
  for (int i = 0; i < n; ++i) all[i] = &shards[i];
  std::vector<uint8_t*> dptr(n);
  const bool staged = !resolve_rows(all.data(), n, host, dptr.data());
  const size_t slot = align_up(S, kSlotAlign);
  SyncCall call(ctx_, staged ? slot * n : 0, (size_t)n, host ? nullptr : stream, !staged && !stream);
  if (!call.begun()) return call.status();
  DeviceContext::Workspace* ws = call.ws();
  hipStream_t s = call.stream();
  for (int i = 0; i < n && staged; ++i) {
    dptr[i] = ws->dbuf + slot * i;
    if (i < k_) call.copy(dptr[i], shards[i].data, S, hipMemcpyHostToDevice);
  }
  if (m_ > 0) {
    const MatVecJob job = matvec_job(k_, m_, parity_.v.data(), S, 1, dptr.data(), dptr.data() + k_);
    const std::vector<int> every = index_range(0, n);
    call.step("matvec_with_crc", [&] { return matvec_with_crc(job, dptr.data(), n, every, S, ws->dflags, s); });
  } else {
    call.step("crc", [&] { return crc_rows_as_they_stand(dptr.data(), n, S, ws->dflags, (size_t)n, nullptr, s); });
  }
  for (int r = k_; r < n && staged; ++r) call.copy(shards[r].data, dptr[r], S, hipMemcpyDeviceToHost);
  call.fetch_words((size_t)n);
  st = call.finish();
  if (st == CFSEC_OK) std::memcpy(crcs, ws->hflags, 4 * (size_t)n);
  return st;
}

Status RSEngine::verify(cfsec_shard* shards, int n, int mem, hipStream_t stream, bool* ok) {
  *ok = false;
  return code_stripe(shards, n, mem, stream, MatVecMode::kVerify, ok);
}

Status RSEngine::plan_reconstruct(const std::vector<bool>& present, bool data_only, ReconPlan* plan) {
  // KRS/reedsolomon.go:1453-1501: first k present rows in index order; cache key is
  // the invalid rows met before the k-th valid one.
  std::vector<int> invalid;
  plan->valid.clear();
  for (int row = 0; row < total() && (int)plan->valid.size() < k_; ++row) {
    if (present[row]) plan->valid.push_back(row);
    else invalid.push_back(row);
  }
  if ((int)plan->valid.size() < k_) return CFSEC_ERR_TOO_FEW_SHARDS;
  Matrix dec;
  if (!tree_.get(invalid, &dec)) {
    Matrix sub(k_, k_);
    for (int r = 0; r < k_; ++r)
      for (int c = 0; c < k_; ++c) sub.at(r, c) = mat_.at(plan->valid[r], c);
    if (!mat_invert(sub, dec)) return CFSEC_ERR_SINGULAR;
    tree_.put(invalid, dec);
  }
  // Missing data rows: rows of inv(sub) (:1508-1524).  Missing parity rows: the
  // reference recomputes them from all data shards (:1537-1550); the same linear map
  // over the k survivors is parity_row x inv(sub), so one fused pass is bit-exact.
  plan->outputs.clear();
  std::vector<const uint8_t*> rowsrc;
  for (int i = 0; i < k_; ++i)
    if (!present[i]) plan->outputs.push_back(i);
  if (!data_only)
    for (int i = k_; i < total(); ++i)
      if (!present[i]) plan->outputs.push_back(i);
  plan->rows = Matrix((int)plan->outputs.size(), k_);
  const GF& gf = GF::get();
  for (size_t o = 0; o < plan->outputs.size(); ++o) {
    const int idx = plan->outputs[o];
    uint8_t* dst = plan->rows.row((int)o);
    if (idx < k_) {
      std::memcpy(dst, dec.row(idx), k_);
    } else {
      const uint8_t* p = parity_.row(idx - k_);
      for (int c = 0; c < k_; ++c) {
        uint8_t v = 0;
        for (int j = 0; j < k_; ++j) v ^= gf.mul(p[j], dec.at(j, c));
        dst[c] = v;
      }
    }
  }
  return CFSEC_OK;
}

Status RSEngine::reconstruct(cfsec_shard* shards, int n, bool data_only, int mem, hipStream_t stream) {
  if (!shards || n != total()) return CFSEC_ERR_TOO_FEW_SHARDS;
  size_t S = 0;
  Status st = check_shards(shards, n, true, &S);
  if (st != CFSEC_OK) return st;
  std::vector<bool> present(n);
  int npresent = 0, dpresent = 0;
  for (int i = 0; i < n; ++i) {
    present[i] = shards[i].len != 0;
    if (present[i]) {
      ++npresent;
      if (i < k_) ++dpresent;
    }
  }
  if (npresent == n || (data_only && dpresent == k_)) return CFSEC_OK;
  if (npresent < k_) return CFSEC_ERR_TOO_FEW_SHARDS;
  ReconPlan plan;
  {
    HostTimer tp("  reconstruct: plan");
    st = plan_reconstruct(present, data_only, &plan);
  }
  if (st != CFSEC_OK) return st;
  for (int idx : plan.outputs)
    if (!shards[idx].data || shards[idx].cap < S) {
      set_last_error("reconstruct: missing shard " + std::to_string(idx) + " has cap < shard size");
      return CFSEC_ERR_INVALID_ARG;
    }
  std::vector<cfsec_shard*> ins, outs;
  for (int v : plan.valid) ins.push_back(&shards[v]);
  for (int o : plan.outputs) outs.push_back(&shards[o]);
  for (auto* o : outs) o->len = S;  // KRS/reedsolomon.go:1514-1518: shards[i] = shards[i][0:S]
  return run(plan.rows, ins, outs, S, mem, stream, MatVecMode::kStore, nullptr);
}

Status RSEngine::reconstruct_some(cfsec_shard* shards, int n, const uint8_t* required, int nrequired, int mem,
                                  hipStream_t stream) {
  // KRS/reedsolomon.go:1407-1529 with dataOnly and a required mask
  if (!shards || n != total() || nrequired < k_) return CFSEC_ERR_TOO_FEW_SHARDS;
  if (!required) return CFSEC_ERR_INVALID_ARG;
  size_t S = 0;
  Status st = check_shards(shards, n, true, &S);
  if (st != CFSEC_OK) return st;
  const auto req = [&](int i) { return i < nrequired && required[i] != 0; };
  std::vector<bool> present(n);
  int npresent = 0, dpresent = 0, missing_required = 0;
  for (int i = 0; i < n; ++i) {
    present[i] = shards[i].len != 0;
    if (present[i]) {
      ++npresent;
      if (i < k_) ++dpresent;
    } else if (req(i)) {
      ++missing_required;  // (:1427-1429: a missing parity index counts too, though parity is never rebuilt)
    }
  }
  if (npresent == n || dpresent == k_ || missing_required == 0) return CFSEC_OK;
  if (npresent < k_) return CFSEC_ERR_TOO_FEW_SHARDS;
  ReconPlan plan;
  st = plan_reconstruct(present, true, &plan);
  if (st != CFSEC_OK) return st;
  // the rows of the data-only plan that the mask selects (:1508-1512)
  std::vector<int> picked;
  for (size_t o = 0; o < plan.outputs.size(); ++o)
    if (req(plan.outputs[o])) picked.push_back((int)o);
  Matrix rows((int)picked.size(), k_);
  std::vector<cfsec_shard*> ins, outs;
  for (size_t j = 0; j < picked.size(); ++j) {
    const int idx = plan.outputs[picked[j]];
    if (!shards[idx].data || shards[idx].cap < S) {
      set_last_error("reconstruct: missing shard " + std::to_string(idx) + " has cap < shard size");
      return CFSEC_ERR_INVALID_ARG;
    }
    std::memcpy(rows.row((int)j), plan.rows.row(picked[j]), k_);
    outs.push_back(&shards[idx]);
  }
  for (int v : plan.valid) ins.push_back(&shards[v]);
  for (auto* o : outs) o->len = S;
  return run(rows, ins, outs, S, mem, stream, MatVecMode::kStore, nullptr);
}

Status RSEngine::run_delta(const Matrix& coef, const std::vector<uint8_t*>& olds, const std::vector<uint8_t*>& news,
                           const std::vector<uint8_t*>& outs, size_t S, int mem, hipStream_t stream) {
  if (olds.empty() || outs.empty() || S == 0) return CFSEC_OK;
  if (!ctx_) {
    set_last_error("no HIP device available to the cfsec engine");
    return CFSEC_ERR_DEVICE;
  }
  if (mem != CFSEC_MEM_HOST && mem != CFSEC_MEM_DEVICE) return CFSEC_ERR_INVALID_ARG;
  std::vector<uint8_t*> all(olds);  // the call's rows: the columns, their new contents, the outputs
  all.insert(all.end(), news.begin(), news.end());
  all.insert(all.end(), outs.begin(), outs.end());
  for (uint8_t* p : all)
    if (!p) return CFSEC_ERR_INVALID_ARG;
  const int nc = (int)olds.size(), nn = (int)news.size(), n = (int)all.size();
  if (coef.rows != (int)outs.size() || coef.cols != nc || (nn != 0 && nn != nc)) return CFSEC_ERR_INVALID_ARG;
  const bool host = mem == CFSEC_MEM_HOST;
  std::optional<DeviceGuard> g;
  if (host) {
    g.emplace(ctx_->device());
    if (!g->ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  }
  // device memory as it is; host rows in place when every one of them is page-locked, else all staged
  std::vector<uint8_t*> d(all);
  bool staged = false;
  for (int i = 0; i < n && host && !staged; ++i) staged = !device_alias(all[i], &d[i]);
  const size_t slot = align_up(S, kSlotAlign);
  hipStream_t s = host ? nullptr : stream;
  SyncCall call(ctx_, staged ? slot * size_t(n) : 0, 1, s, !staged && !s);
  if (!call.begun()) return call.status();
  for (int i = 0; i < n && staged; ++i) {
    d[i] = call.ws()->dbuf + slot * size_t(i);
    call.copy(d[i], all[i], S, hipMemcpyHostToDevice);
  }
  DeltaJob job;
  job.nc = nc, job.m = coef.rows, job.coef = coef.v.data(), job.len = S, job.nstripes = 1;
  job.old = d.data();
  job.neu = nn ? d.data() + nc : nullptr;
  job.out = d.data() + nc + nn;
  call.step("launch_delta", [&] { return launch_delta(job, call.stream()); });
  for (int i = 0; i < n && staged; ++i)
    if (i >= nc + nn || (nn && i < nc)) call.copy(all[i], d[i], S, hipMemcpyDeviceToHost);
  return call.finish();
}

Status RSEngine::encode_idx(const cfsec_shard* data_shard, int idx, cfsec_shard* parity, int nparity, int mem,
                            hipStream_t stream) {
  if (nparity != m_) return CFSEC_ERR_TOO_FEW_SHARDS;
  if (m_ == 0) return CFSEC_OK;
  if (idx < 0 || idx >= k_) return CFSEC_ERR_INV_SHARD_NUM;
  if (!parity) return CFSEC_ERR_INVALID_ARG;
  size_t S = 0;
  const Status st = check_shards(parity, nparity, false, &S);
  if (st != CFSEC_OK) return st;
  if (!data_shard || data_shard->len != S) return CFSEC_ERR_SHARD_SIZE;
  Matrix coef(m_, 1);
  std::vector<uint8_t*> outs(m_);
  for (int r = 0; r < m_; ++r) {
    coef.at(r, 0) = parity_.at(r, idx);
    outs[r] = parity[r].data;
  }
  return run_delta(coef, {data_shard->data}, {}, outs, S, mem, stream);
}

Status RSEngine::update(cfsec_shard* shards, int n, const cfsec_shard* new_data, int nnew, int mem,
                        hipStream_t stream) {
  if (!shards || n != total() || nnew != k_) return CFSEC_ERR_TOO_FEW_SHARDS;
  if (!new_data) return CFSEC_ERR_INVALID_ARG;
  size_t S = 0, Sn = 0;
  Status st = check_shards(shards, n, true, &S);
  if (st == CFSEC_OK) st = check_shards(new_data, nnew, true, &Sn);
  if (st != CFSEC_OK) return st;
  for (int i = 0; i < k_; ++i)
    if (new_data[i].len != 0 && shards[i].len == 0) return CFSEC_ERR_INVALID_INPUT;
  for (int i = k_; i < n; ++i)
    if (shards[i].len == 0) return CFSEC_ERR_INVALID_INPUT;
  if (Sn != S) return CFSEC_ERR_SHARD_SIZE;  // (the reference never compares the two sizes: cfsec.h)
  if (m_ == 0) return CFSEC_OK;              // :713-715: no outputs, nothing is touched
  std::vector<int> cols;
  for (int i = 0; i < k_; ++i)
    if (new_data[i].len != 0) cols.push_back(i);
  const int nc = (int)cols.size();
  Matrix coef(m_, nc);
  std::vector<uint8_t*> olds(nc), news(nc), outs(m_);
  for (int j = 0; j < nc; ++j) {
    olds[j] = shards[cols[j]].data;
    news[j] = new_data[cols[j]].data;
    for (int r = 0; r < m_; ++r) coef.at(r, j) = parity_.at(r, cols[j]);
  }
  for (int r = 0; r < m_; ++r) outs[r] = shards[k_ + r].data;
  return run_delta(coef, olds, news, outs, S, mem, stream);
}

Status RSEngine::split(uint8_t* data, size_t len, size_t cap, cfsec_shard* out, uint8_t* pad,
                       size_t pad_len, size_t* pad_needed) {
  // KRS/reedsolomon.go:1574-1632
  if (pad_needed) *pad_needed = 0;
  if (len == 0) return CFSEC_ERR_SHORT_DATA;
  if (!data || !out) return CFSEC_ERR_INVALID_ARG;
  if (cap < len) cap = len;
  const int tot = total();
  if (tot == 1) {
    out[0] = cfsec_shard{data, len, cap};
    return CFSEC_OK;
  }
  const size_t per = (len + k_ - 1) / k_;
  const size_t need_total = per * tot;
  size_t eff = len;
  if (cap > len) {
    eff = std::min(cap, need_total);
    std::memset(data + len, 0, eff - len);
  }
  const size_t full = std::min<size_t>(eff / per, tot);
  const size_t npad = tot - full;
  // the padding shards as AllocAligned(npad, per) lays them out (KRS/unsafe.go:17-41): a 64-byte
  // aligned start, each shard at a 64-byte rounded stride with that stride as its capacity
  const size_t each = (per + 63) / 64 * 64;
  if (pad_needed) *pad_needed = npad ? npad * each + 63 : 0;
  if (npad > 0 && (!pad || pad_len < npad * each + 63)) return CFSEC_ERR_INVALID_ARG;
  uint8_t* base = pad;
  if (npad > 0) {
    base = pad + ((64 - (reinterpret_cast<uintptr_t>(pad) & 63)) & 63);
    std::memset(base, 0, npad * each);
    // the partial data after the full shards, copied shard by shard (copy(padding[i], copyFrom))
    size_t from = per * full;
    for (size_t j = 0; j < npad && from < len; ++j) {
      const size_t c = std::min(per, len - from);
      std::memcpy(base + j * each, data + from, c);
      from += c;
    }
  }
  for (size_t i = 0; i < full; ++i) out[i] = cfsec_shard{data + i * per, per, per};
  for (size_t j = 0; j < npad; ++j) out[full + j] = cfsec_shard{base + j * each, per, each};
  return CFSEC_OK;
}

Status RSEngine::join(uint8_t* dst, size_t dst_len, const cfsec_shard* shards, int n, size_t out_size) {
  // KRS/reedsolomon.go:1646-1684
  if (n < k_) return CFSEC_ERR_TOO_FEW_SHARDS;
  size_t size = 0;
  for (int i = 0; i < k_; ++i) {
    if (shards[i].data == nullptr) return CFSEC_ERR_RECONSTRUCT_REQUIRED;
    size += shards[i].len;
    if (size >= out_size) break;
  }
  if (size < out_size) return CFSEC_ERR_SHORT_DATA;
  if (!dst || dst_len < out_size) return CFSEC_ERR_INVALID_ARG;
  size_t write = out_size;
  for (int i = 0; i < k_ && write > 0; ++i) {
    const size_t c = std::min(write, shards[i].len);
    std::memcpy(dst + (out_size - write), shards[i].data, c);
    write -= c;
  }
  return CFSEC_OK;
}

namespace {
// The rows of a pointer batch: stripe s's row i is ptrs[s * width + i].
struct PtrTables {
  std::vector<const uint8_t*> in;
  std::vector<uint8_t*> out;
};

// The in / out tables of a launch: the rows in_idx, then out_idx, of every stripe.
PtrTables ptr_tables(uint8_t* const* ptrs, size_t width, int nstripes, const std::vector<int>& in_idx,
                     const std::vector<int>& out_idx) {
  const size_t k = in_idx.size(), m = out_idx.size();
  PtrTables t{std::vector<const uint8_t*>(size_t(nstripes) * k), std::vector<uint8_t*>(size_t(nstripes) * m)};
  for (int s = 0; s < nstripes; ++s) {
    for (size_t c = 0; c < k; ++c) t.in[size_t(s) * k + c] = ptrs[size_t(s) * width + in_idx[c]];
    for (size_t r = 0; r < m; ++r) t.out[size_t(s) * m + r] = ptrs[size_t(s) * width + out_idx[r]];
  }
  return t;
}

// The erasure set of a pointer batch: present[i] = shard i is not among erased[0 .. nerased), np of
// them present, dp of those data shards.
struct Erasures {
  std::vector<bool> present;
  int np = 0, dp = 0;
};

// False for an index outside [0, total).
bool parse_erased(const int* erased, int nerased, int total, int k, Erasures* e) {
  e->present.assign(total, true);
  for (int i = 0; i < nerased; ++i) {
    if (erased[i] < 0 || erased[i] >= total) return false;
    e->present[erased[i]] = false;
  }
  for (int i = 0; i < total; ++i)
    if (e->present[i]) {
      ++e->np;
      if (i < k) ++e->dp;
    }
  return true;
}
}  // namespace

Status RSEngine::encode_batch(uint8_t* const* ptrs, size_t S, int nstripes, hipStream_t stream) {
  if (!ctx_) return CFSEC_ERR_DEVICE;
  if (!ptrs || nstripes < 0) return CFSEC_ERR_INVALID_ARG;
  if (m_ == 0 || nstripes == 0 || S == 0) return CFSEC_OK;
  const PtrTables t = ptr_tables(ptrs, total(), nstripes, index_range(0, k_), index_range(k_, total()));
  DeviceGuard g(ctx_->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  const MatVecJob job = matvec_job(k_, m_, parity_.v.data(), S, nstripes, t.in.data(), t.out.data());
  return hip_status(launch_matvec(job, stream), "launch_matvec(encode_batch)");
}

Status RSEngine::matvec_batch(const uint8_t* coef, int rows, uint8_t* const* ptrs, size_t S, int nstripes,
                              hipStream_t stream) {
  if (!ctx_) return CFSEC_ERR_DEVICE;
  if (!coef || !ptrs || nstripes < 0 || rows < 0 || rows > 256) return CFSEC_ERR_INVALID_ARG;
  if (rows == 0 || nstripes == 0 || S == 0) return CFSEC_OK;
  const PtrTables t = ptr_tables(ptrs, (size_t)k_ + rows, nstripes, index_range(0, k_), index_range(k_, k_ + rows));
  DeviceGuard g(ctx_->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  const MatVecJob job = matvec_job(k_, rows, coef, S, nstripes, t.in.data(), t.out.data());
  return hip_status(launch_matvec(job, stream), "launch_matvec(matvec_batch)");
}

Status RSEngine::update_batch(uint8_t* const* ptrs, uint8_t* const* new_ptrs, const int* cols, int ncols, size_t S,
                              int nstripes, hipStream_t stream) {
  if (!ptrs || !new_ptrs || nstripes < 0 || ncols < 0 || (ncols > 0 && !cols)) return CFSEC_ERR_INVALID_ARG;
  for (int j = 0; j < ncols; ++j)
    if (cols[j] < 0 || cols[j] >= k_ || (j > 0 && cols[j] <= cols[j - 1])) return CFSEC_ERR_INVALID_ARG;
  if (!ctx_) return CFSEC_ERR_DEVICE;
  if (m_ == 0 || ncols == 0 || nstripes == 0 || S == 0) return CFSEC_OK;
  const PtrTables t = ptr_tables(ptrs, total(), nstripes, std::vector<int>(cols, cols + ncols), index_range(k_, total()));
  Matrix coef(m_, ncols);
  for (int r = 0; r < m_; ++r)
    for (int j = 0; j < ncols; ++j) coef.at(r, j) = parity_.at(r, cols[j]);
  DeviceGuard g(ctx_->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  DeltaJob job;
  job.nc = ncols, job.m = m_, job.coef = coef.v.data(), job.len = S, job.nstripes = nstripes;
  job.old = const_cast<uint8_t* const*>(t.in.data());  // (ptr_tables keeps its input rows as const)
  job.neu = new_ptrs;
  job.out = t.out.data();
  return hip_status(launch_delta(job, stream), "launch_delta(update_batch)");
}

Status RSEngine::verify_batch(uint8_t* const* ptrs, size_t S, int nstripes, uint32_t* flags,
                              hipStream_t stream) {
  if (!ctx_) return CFSEC_ERR_DEVICE;
  if (!ptrs || !flags || nstripes < 0) return CFSEC_ERR_INVALID_ARG;
  if (m_ == 0 || nstripes == 0 || S == 0) return CFSEC_OK;
  if (k_ > 32) return CFSEC_ERR_NOT_SUPPORTED;
  const PtrTables t = ptr_tables(ptrs, total(), nstripes, index_range(0, k_), index_range(k_, total()));
  DeviceGuard g(ctx_->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  MatVecJob job = matvec_job(k_, m_, parity_.v.data(), S, nstripes, t.in.data(), t.out.data());
  job.mode = MatVecMode::kVerify;
  job.flags = flags;
  return hip_status(launch_matvec(job, stream), "launch_matvec(verify_batch)");
}

Status RSEngine::reconstruct_batch(uint8_t* const* ptrs, size_t S, int nstripes, const int* erased,
                                   int nerased, bool data_only, hipStream_t stream) {
  if (!ctx_) return CFSEC_ERR_DEVICE;
  if (!ptrs || nstripes < 0 || nerased < 0 || (nerased > 0 && !erased)) return CFSEC_ERR_INVALID_ARG;
  Erasures e;
  if (!parse_erased(erased, nerased, total(), k_, &e)) return CFSEC_ERR_INVALID_ARG;
  if (e.np == total() || (data_only && e.dp == k_) || nstripes == 0 || S == 0) return CFSEC_OK;
  if (e.np < k_) return CFSEC_ERR_TOO_FEW_SHARDS;
  ReconPlan plan;
  Status st = plan_reconstruct(e.present, data_only, &plan);
  if (st != CFSEC_OK) return st;
  const PtrTables t = ptr_tables(ptrs, total(), nstripes, plan.valid, plan.outputs);
  DeviceGuard g(ctx_->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  const int nout = (int)plan.outputs.size();
  const MatVecJob job = matvec_job(k_, nout, plan.rows.v.data(), S, nstripes, t.in.data(), t.out.data());
  return hip_status(launch_matvec(job, stream), "launch_matvec(reconstruct_batch)");
}

Status RSEngine::encode_crc_batch(uint8_t* const* ptrs, size_t S, int nstripes, uint32_t* crcs,
                                  hipStream_t stream) {
  if (!ctx_) return CFSEC_ERR_DEVICE;
  if (!ptrs || !crcs || nstripes < 0) return CFSEC_ERR_INVALID_ARG;
  if (nstripes == 0) return CFSEC_OK;
  DeviceGuard g(ctx_->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  const size_t nwords = (size_t)total() * nstripes;
  if (m_ == 0 || S == 0) return crc_rows_as_they_stand(ptrs, (int)nwords, S, crcs, nwords, nullptr, stream);
  const PtrTables t = ptr_tables(ptrs, total(), nstripes, index_range(0, k_), index_range(k_, total()));
  const MatVecJob job = matvec_job(k_, m_, parity_.v.data(), S, nstripes, t.in.data(), t.out.data());
  return matvec_with_crc(job, ptrs, total(), index_range(0, total()), S, crcs, stream);
}

Status RSEngine::reconstruct_crc_batch(uint8_t* const* ptrs, size_t S, int nstripes, const int* erased,
                                       int nerased, bool data_only, uint32_t* crcs, hipStream_t stream) {
  if (!ctx_) return CFSEC_ERR_DEVICE;
  if (!ptrs || !crcs || nstripes < 0 || nerased < 0 || (nerased > 0 && !erased)) return CFSEC_ERR_INVALID_ARG;
  Erasures e;
  if (!parse_erased(erased, nerased, total(), k_, &e)) return CFSEC_ERR_INVALID_ARG;
  if (e.np < k_ && nstripes > 0) return CFSEC_ERR_TOO_FEW_SHARDS;
  DeviceGuard g(ctx_->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  if (nstripes == 0) return CFSEC_OK;
  ReconPlan plan;
  if (e.np < total()) {
    Status st = plan_reconstruct(e.present, data_only, &plan);
    if (st != CFSEC_OK) return st;
  }
  const int nout = (int)plan.outputs.size();
  if (nout == 0 || S == 0)
    return hip_status(hipMemsetAsync(crcs, 0, 4 * (size_t)total() * nstripes, stream), "hipMemsetAsync");
  const PtrTables t = ptr_tables(ptrs, total(), nstripes, plan.valid, plan.outputs);
  const MatVecJob job = matvec_job(k_, nout, plan.rows.v.data(), S, nstripes, t.in.data(), t.out.data());
  std::vector<int> slot(k_ + nout, -1);
  for (int r = 0; r < nout; ++r) slot[k_ + r] = plan.outputs[r];
  return matvec_with_crc(job, ptrs, total(), slot, S, crcs, stream);
}

Status RSEngine::repair_crc_batch(uint8_t* const* ptrs, size_t S, int nstripes, const int* erased, int nerased,
                                  uint32_t* flags, uint32_t* crcs, hipStream_t stream) {
  if (!ptrs || !crcs || !flags || nstripes < 0 || nerased < 0 || (nerased > 0 && !erased))
    return CFSEC_ERR_INVALID_ARG;
  Erasures e;
  if (!parse_erased(erased, nerased, total(), k_, &e)) return CFSEC_ERR_INVALID_ARG;
  if (!ctx_) return CFSEC_ERR_DEVICE;
  if (e.np < k_ && nstripes > 0) return CFSEC_ERR_TOO_FEW_SHARDS;
  if (k_ > kLaunchMaxRows) return CFSEC_ERR_NOT_SUPPORTED;  // compared rows over more inputs than a launch carries
  DeviceGuard g(ctx_->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  if (nstripes == 0) return CFSEC_OK;
  const size_t nwords = (size_t)total() * nstripes;
  if (S == 0) return crc_rows_as_they_stand(ptrs, (int)nwords, S, crcs, nwords, nullptr, stream);
  // the batch layer's plan of a bid: the first k present shards in, the missing ones stored, every
  // other present parity shard compared -- each shard exactly once
  StripePlan plan;
  const Status st = plan_stripe(e.present, true, &plan, nullptr);
  if (st != CFSEC_OK) return st;
  const int nout = (int)plan.out.size();
  if (nout > kLaunchMaxRows && plan.nstore > 0 && plan.nstore < nout) return CFSEC_ERR_NOT_SUPPORTED;
  // no parity shards: nothing to rebuild or compare
  if (nout == 0) return crc_rows_as_they_stand(ptrs, (int)nwords, S, crcs, nwords, nullptr, stream);
  const PtrTables t = ptr_tables(ptrs, total(), nstripes, plan.in, plan.out);
  MatVecJob job = matvec_job(k_, nout, plan.rows.v.data(), S, nstripes, t.in.data(), t.out.data());
  if (plan.nstore < nout) {
    job.mode = MatVecMode::kStoreVerify;
    job.nstore = plan.nstore;
    job.flags = flags;
  }
  std::vector<int> slot(plan.in);
  slot.insert(slot.end(), plan.out.begin(), plan.out.end());
  return matvec_with_crc(job, ptrs, total(), slot, S, crcs, stream);
}

// ---------------------------------------------------------------- ec.Encoder

Status ECEncoder::create(const cfsec_tactic& t, bool enable_verify, int concurrency, int device,
                         std::unique_ptr<ECEncoder>* out) {
  // ec.NewEncoder, encoder.go:78-112
  if (!tactic_valid(t)) return CFSEC_ERR_INVALID_CODE_MODE;
  if (concurrency <= 0) concurrency = 100;  // defaultConcurrency, encoder.go:29
  std::unique_ptr<RSEngine> engine;
  Status st = RSEngine::create(t.n, t.m, device, &engine);
  if (st != CFSEC_OK) return st;
  std::unique_ptr<ECEncoder> enc;
  if (t.l != 0) {
    std::unique_ptr<RSEngine> local;
    const int ln = (t.n + t.m) / t.az_count, lm = t.l / t.az_count;
    st = RSEngine::create(ln, lm, device, &local);
    if (st != CFSEC_OK) return st;
    auto* lrc = new LrcEncoder();
    // Fused LRC encode rows: global parity, then every AZ's local parity expressed over
    // the N data shards (local parity = localRow x [AZ data, AZ global parity], and the
    // global parity is itself parity_row x data).
    const Matrix& G = engine->matrix();
    const Matrix& Lm = local->matrix();
    lrc->fused_ = Matrix(t.m + t.l, t.n);
    for (int r = 0; r < t.m; ++r)
      for (int c = 0; c < t.n; ++c) lrc->fused_.at(r, c) = G.at(t.n + r, c);
    const GF& gf = GF::get();
    const auto az = layout_by_az(t);
    for (int a = 0; a < t.az_count; ++a)
      for (int j = 0; j < lm; ++j) {
        const int g = t.n + t.m + a * lm + j;
        uint8_t* dst = lrc->fused_.row(t.m + (g - t.n - t.m));
        for (int i = 0; i < ln; ++i) {
          const uint8_t coef = Lm.at(ln + j, i);
          const int member = az[a][i];
          for (int c = 0; c < t.n; ++c) {
            const uint8_t basis = member < t.n ? uint8_t(member == c) : G.at(member, c);
            dst[c] ^= gf.mul(coef, basis);
          }
        }
      }
    lrc->local_ = std::move(local);
    enc.reset(lrc);
  } else {
    enc.reset(new ECEncoder());
  }
  enc->t_ = t;
  enc->enable_verify_ = enable_verify;
  enc->pool_.reset(new BlockingCount(concurrency));
  enc->engine_ = std::move(engine);
  *out = std::move(enc);
  return CFSEC_OK;
}

// Encode, then with EnableVerify the Verify of what it wrote: CFSEC_ERR_VERIFY when that is false
// (encoder.go:114-131).
static Status encode_checked(RSEngine* e, cfsec_shard* shards, int n, int mem, hipStream_t s, bool verify) {
  Status st = e->encode(shards, n, mem, s);
  if (st != CFSEC_OK || !verify) return st;
  bool ok = false;
  st = e->verify(shards, n, mem, s, &ok);
  return st != CFSEC_OK ? st : ok ? CFSEC_OK : CFSEC_ERR_VERIFY;
}

Status ECEncoder::encode(cfsec_shard* shards, int n, int mem, hipStream_t s) {
  Slot slot(pool_.get());
  return encode_checked(engine_.get(), shards, n, mem, s, enable_verify_);
}

Status ECEncoder::verify(cfsec_shard* shards, int n, int mem, hipStream_t s, bool* ok) {
  Slot slot(pool_.get());  // encoder.go:133-137
  return engine_->verify(shards, n, mem, s, ok);
}

Status ECEncoder::reconstruct(cfsec_shard* shards, int n, const int* bad, int nbad, int mem,
                              hipStream_t s) {
  // encoder.go:139-144
  Status st = init_bad_shards(shards, n, std::vector<int>(bad, bad + nbad));
  if (st != CFSEC_OK) return st;
  Slot slot(pool_.get());
  return engine_->reconstruct(shards, n, false, mem, s);
}

Status ECEncoder::reconstruct_data(cfsec_shard* shards, int n, const int* bad, int nbad, int mem,
                                   hipStream_t s) {
  // encoder.go:146-151
  HostTimer whole("ec reconstruct_data");
  Status st = init_bad_shards(shards, n, std::vector<int>(bad, bad + nbad));
  if (st != CFSEC_OK) return st;
  Slot slot(pool_.get());
  return engine_->reconstruct(shards, n, true, mem, s);
}

bool ECEncoder::row_over_data(int g, uint8_t* dst) const {
  const int N = t_.n, M = t_.m;
  if (g < 0 || g >= N + M) return false;
  for (int c = 0; c < N; ++c) dst[c] = g < N ? uint8_t(g == c) : engine_->matrix().at(g, c);
  return true;
}

bool LrcEncoder::row_over_data(int g, uint8_t* dst) const {
  const int N = t_.n, M = t_.m, L = t_.l;
  if (g < N + M) return ECEncoder::row_over_data(g, dst);
  if (g >= N + M + L) return false;
  std::memcpy(dst, fused_.row(M + g - N - M), N);  // lrcencoder.go: the local parity over the data
  return true;
}

Status ECEncoder::repair_rows(const int* bad, int nbad, const int* want, int nwant, int* in, uint8_t* rows) {
  const int N = t_.n, M = t_.m, L = t_.l;
  if ((nbad && !bad) || nbad < 0 || nwant < 0 || (nwant && (!want || !rows)) || !in) return CFSEC_ERR_INVALID_ARG;
  std::vector<bool> present(N + M, true);
  for (int i = 0; i < nbad; ++i) {
    if (bad[i] < 0 || bad[i] >= N + M + L) return CFSEC_ERR_INVALID_ARG;
    if (bad[i] < N + M) present[bad[i]] = false;
  }
  ReconPlan rp;
  Status st = engine_->plan_reconstruct(present, false, &rp);
  if (st != CFSEC_OK) return st;
  // D: the data over the N inputs (unit rows for surviving data, decode rows for the missing)
  Matrix D(N, N);
  for (int i = 0; i < N; ++i) {
    const auto v = std::find(rp.valid.begin(), rp.valid.end(), i);
    const auto o = std::find(rp.outputs.begin(), rp.outputs.end(), i);
    if (v != rp.valid.end()) D.at(i, (int)(v - rp.valid.begin())) = 1;
    else if (o != rp.outputs.end()) std::memcpy(D.row(i), rp.rows.row((int)(o - rp.outputs.begin())), N);
    else return CFSEC_ERR_INVALID_ARG;
  }
  for (int c = 0; c < N; ++c) in[c] = rp.valid[c];
  const GF& gf = GF::get();
  std::vector<uint8_t> g(N);
  for (int w = 0; w < nwant; ++w) {
    if (!row_over_data(want[w], g.data())) return CFSEC_ERR_INVALID_ARG;
    uint8_t* dst = rows + (size_t)w * N;
    for (int c = 0; c < N; ++c) {
      uint8_t v = 0;
      for (int j = 0; j < N; ++j) v ^= gf.mul(g[j], D.at(j, c));
      dst[c] = v;
    }
  }
  return CFSEC_OK;
}

std::vector<int> ECEncoder::shards_in_idc(int idx) const {
  // encoder.go:169-176
  std::vector<int> v;
  const int ln = t_.n / t_.az_count, lm = t_.m / t_.az_count;
  for (int i = idx * ln; i < (idx + 1) * ln; ++i) v.push_back(i);
  for (int i = t_.n + lm * idx; i < t_.n + lm * (idx + 1); ++i) v.push_back(i);
  return v;
}

// ---------------------------------------------------------------- lrcEncoder

std::vector<int> LrcEncoder::shards_in_idc(int idx) const {
  // lrcencoder.go:236-243 via codemode.LocalStripeInAZ (codemode.go:334-345)
  if (idx < 0 || idx >= t_.az_count) return {};
  return layout_by_az(t_)[idx];
}

Status LrcEncoder::encode(cfsec_shard* shards, int n, int mem, hipStream_t s) {
  // lrcencoder.go:35-82
  const int N = t_.n, M = t_.m, L = t_.l;
  if (!shards || n != N + M + L) return CFSEC_ERR_INVALID_SHARDS;
  Slot slot(pool_.get());
  return encode_stripe(shards, n, mem, s);
}

Status LrcEncoder::encode_stripe(cfsec_shard* shards, int n, int mem, hipStream_t s) {
  const int N = t_.n, M = t_.m, L = t_.l;
  Status st = fill_full_shards(shards, n);
  if (st != CFSEC_OK) return st;
  size_t S = 0;
  st = check_shards(shards, N + M, false, &S);  // global engine.Encode's checkShards
  if (st != CFSEC_OK) return st;
  Status local_err = CFSEC_OK;
  for (int a = 0; a < t_.az_count && local_err == CFSEC_OK; ++a) {
    std::vector<cfsec_shard> ls;
    for (int g : shards_in_idc(a)) ls.push_back(shards[g]);
    size_t ignored;
    local_err = check_shards(ls.data(), (int)ls.size(), false, &ignored);
  }
  std::vector<cfsec_shard*> ins, outs;
  for (int i = 0; i < N; ++i) ins.push_back(&shards[i]);
  if (local_err != CFSEC_OK) {
    // The reference's sequence, step by step: global parity (+ Verify), then every AZ's local
    // task -- task.Run lets each goroutine finish, so the AZs that pass checkShards are encoded
    // -- and the first error in AZ order (oracle/ec_oracle.py: ECOracle.encode).
    st = encode_checked(engine_.get(), shards, N + M, mem, s, enable_verify_);
    if (st != CFSEC_OK) return st;
    Status first = CFSEC_OK;
    for (int a = 0; a < t_.az_count; ++a) {
      std::vector<cfsec_shard> ls;
      for (int g : shards_in_idc(a)) ls.push_back(shards[g]);
      const Status e = encode_checked(local_.get(), ls.data(), (int)ls.size(), mem, s, enable_verify_);
      if (first == CFSEC_OK) first = e;
    }
    return first;
  }
  for (int i = N; i < N + M + L; ++i) outs.push_back(&shards[i]);
  st = engine_->run(fused_, ins, outs, S, mem, s, MatVecMode::kStore, nullptr);
  if (st != CFSEC_OK) return st;
  if (enable_verify_) {
    bool ok = false;
    st = engine_->run(fused_, ins, outs, S, mem, s, MatVecMode::kVerify, &ok);
    if (st != CFSEC_OK) return st;
    if (!ok) return CFSEC_ERR_VERIFY;
  }
  return CFSEC_OK;
}

Status LrcEncoder::verify(cfsec_shard* shards, int n, int mem, hipStream_t s, bool* ok) {
  // lrcencoder.go:89-131
  *ok = false;
  Slot slot(pool_.get());
  const int N = t_.n, M = t_.m, L = t_.l;
  if (n == (N + M + L) / t_.az_count) return local_->verify(shards, n, mem, s, ok);
  if (!shards || n != N + M + L) return CFSEC_ERR_INVALID_SHARDS;
  Status st = engine_->verify(shards, N + M, mem, s, ok);
  if (st != CFSEC_OK || !*ok) return st;
  for (int a = 0; a < t_.az_count; ++a) {
    std::vector<cfsec_shard> ls;
    for (int g : shards_in_idc(a)) ls.push_back(shards[g]);
    st = local_->verify(ls.data(), (int)ls.size(), mem, s, ok);
    if (st != CFSEC_OK || !*ok) return st;
  }
  *ok = true;
  return CFSEC_OK;
}

Status LrcEncoder::reconstruct(cfsec_shard* shards, int n, const int* bad, int nbad, int mem,
                               hipStream_t s) {
  // lrcencoder.go:133-186
  const int N = t_.n, M = t_.m, L = t_.l, AZ = t_.az_count;
  if (!shards || n <= 0) return CFSEC_ERR_INVALID_SHARDS;
  Status st = fill_full_shards(shards, n);
  if (st != CFSEC_OK) return st;
  std::vector<int> global_bad;
  for (int i = 0; i < nbad; ++i)
    if (bad[i] < N + M) global_bad.push_back(bad[i]);
  st = init_bad_shards(shards, n, global_bad);
  if (st != CFSEC_OK) return st;
  Slot slot(pool_.get());
  if (n == (N + M + L) / AZ) return local_->reconstruct(shards, n, false, mem, s);
  if (n != N + M + L) return CFSEC_ERR_INVALID_SHARDS;
  st = engine_->reconstruct(shards, N + M, false, mem, s);
  if (st != CFSEC_OK) return st;
  std::map<int, std::vector<int>> local_bad;
  for (int i = 0; i < nbad; ++i) {
    const int b = bad[i];
    if (b >= N + M) {
      const int idc = (b - N - M) * AZ / L;
      local_bad[idc].push_back(b - N - M - L / AZ * idc + (N + M) / AZ);
    }
  }
  // task.Run (util/task/task.go:43-73) runs every AZ's local pass to the end and returns the first
  // error sent; the AZs are disjoint, so running them in AZ order and keeping the lowest AZ's error
  // gives the same bytes (the reference's pick among several failing AZs is scheduling-dependent,
  // oracle/ec_oracle.py takes the lowest AZ as well).
  Status first = CFSEC_OK;
  for (auto& kv : local_bad) {
    // Go copies the slice headers into a fresh [][]byte (lrcencoder.go:236-243); the
    // rebuilt bytes land in the shared buffers, the caller's headers keep their length.
    std::vector<cfsec_shard> ls;
    for (int g : shards_in_idc(kv.first)) ls.push_back(shards[g]);
    st = init_bad_shards(ls.data(), (int)ls.size(), kv.second);
    if (st == CFSEC_OK) st = local_->reconstruct(ls.data(), (int)ls.size(), false, mem, s);
    if (st == CFSEC_ERR_DEVICE) return st;  // the device failed: nothing further is meaningful
    if (first == CFSEC_OK) first = st;
  }
  return first;
}

Status LrcEncoder::reconstruct_data(cfsec_shard* shards, int n, const int* bad, int nbad, int mem,
                                    hipStream_t s) {
  // lrcencoder.go:188-201
  const int N = t_.n, M = t_.m;
  if (!shards || n < N + M) return CFSEC_ERR_INVALID_SHARDS;
  Status st = fill_full_shards(shards, N + M);
  if (st != CFSEC_OK) return st;
  std::vector<int> global_bad;
  for (int i = 0; i < nbad; ++i)
    if (bad[i] < N + M) global_bad.push_back(bad[i]);
  st = init_bad_shards(shards, n, global_bad);
  if (st != CFSEC_OK) return st;
  Slot slot(pool_.get());
  return engine_->reconstruct(shards, N + M, true, mem, s);
}

}  // namespace cfsec
