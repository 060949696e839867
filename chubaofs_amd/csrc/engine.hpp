// engine.hpp -- the MI355X erasure-coding engine behind the cfsec C ABI.
//
//   RSEngine   restates reedsolomon.Encoder (KRS/reedsolomon.go) for the default
//              Vandermonde code, with its arithmetic on the GPU.
//   ECEncoder  restates ec.Encoder (blobstore/common/ec/encoder.go) and
//   LrcEncoder the LRC variant (blobstore/common/ec/lrcencoder.go).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/cfsec.h"
#include "gf256.hpp"
#include "gf_delta.hpp"
#include "kernels.hpp"

namespace cfsec {

// synchronous calls poll a marker word (1) or hipStreamSynchronize (0): cfsec_set_sync_poll
std::atomic<int>& sync_poll_mode();

using Status = int;  // cfsec_status

void set_last_error(const std::string& msg);
const char* last_error_cstr();

// Host-side phase timing of the batch calls, printed to stderr when CFSEC_HOST_TIMING is set
// (development aid: where a synchronous batch call spends its time besides the kernels).
struct HostTimer {
  const char* name;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  static bool on() {
    static const bool v = std::getenv("CFSEC_HOST_TIMING") != nullptr;
    return v;
  }
  explicit HostTimer(const char* n) : name(n) {}
  ~HostTimer() {
    if (on())
      std::fprintf(stderr, "cfsec host %-28s %8.1f us\n", name,
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
};
// ec.initBadShards (encoder.go:182-188) / ec.fillFullShards (encoder.go:199-210), engine.cpp.
Status init_bad_shards(cfsec_shard* shards, int n, const std::vector<int>& bad);
Status fill_full_shards(cfsec_shard* shards, int n);
Status hip_status(hipError_t e, const char* what);
// Stream `to` waits for everything queued on stream `from` so far (the two lanes of a host call).
Status lane_wait(hipEvent_t ev, hipStream_t from, hipStream_t to);
constexpr size_t kSlotAlign = 256;  // staging rows start on 256-B boundaries
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// KRS/reedsolomon.go:1314-1339 checkShards / shardSize.
Status check_shards(const cfsec_shard* shards, int n, bool nilok, size_t* size);
// The plain store of coef (m x k) over nstripes stripes of S-byte rows; callers set what else they need.
inline MatVecJob matvec_job(int k, int m, const uint8_t* coef, size_t S, int nstripes, const uint8_t* const* in,
                            uint8_t* const* out) {
  return MatVecJob{k, m, coef, S, nstripes, in, out};
}
// The device address of page-locked host memory (hipHostMalloc / cfsec_host_alloc); false for
// pageable memory.
bool device_alias(uint8_t* p, uint8_t** dptr);
// The library's own page-locked allocations (cfsec_host_alloc / cfsec_host_free), looked up by
// device_alias before it asks the runtime: hipPointerGetAttributes costs microseconds per shard,
// which a small host-memory call (a degraded range read's segment) pays for every row.
void host_range_add(void* base, size_t size);
void host_range_remove(void* base);

// Per-device streams and staging workspaces, shared by every engine on the device.
class DeviceContext {
 public:
  // nullptr if the device does not exist.  slot > 0: another context on the same device (its own
  // streams and workspaces) -- the multi-device rehearsal of set_devices on a one-GPU machine.
  static DeviceContext* get(int device, int slot = 0);
  int device() const { return device_; }

  struct Workspace {
    uint8_t* dbuf = nullptr;   // device staging buffer
    size_t cap = 0;
    uint32_t* dflags = nullptr;  // device verify flags
    uint32_t* hflags = nullptr;  // pinned host mirror
    size_t nflags = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // second lane of the chunked host pipeline
    hipEvent_t ev = nullptr;        // orders stream2 after work enqueued on stream
    hipEvent_t ev_in = nullptr;     // orders stream after the legacy default stream (no caller stream)
    // batch calls (batch.cpp run_device): per-task verify words, kept zero between calls (the flag
    // gather kernel resets the words it reads), and the device address of hflags
    uint32_t* bflags = nullptr;
    size_t nbflags = 0;
    bool bflags_clean = false;
    uint32_t* hflags_dev = nullptr;
    // asynchronous calls: the workspace is reused only after `done` (recorded on the caller's
    // stream after the call's last kernel) has completed
    hipEvent_t done = nullptr;
    bool pending = false;
    // batch calls with shard checksums: device words (accumulated by the CRC kernel) + pinned mirror
    uint32_t* dcrc = nullptr;
    uint32_t* hcrc = nullptr;
    size_t ncrc = 0;
    // finish(): a pinned, coherent word the stream writes after its work, polled by the caller
    uint32_t* hmark = nullptr;
    uint32_t* dmark = nullptr;
    uint32_t seq = 0;
    // mixed-plan launches (batch.cpp launch_mixed): per lane an item table packed in page-locked host
    // memory and its device copy; mix_ev follows the copy to the device, so the host table is
    // repacked only once the previous copy has read it
    uint8_t* hmix[2] = {nullptr, nullptr};
    uint8_t* dmix[2] = {nullptr, nullptr};
    size_t mix_cap[2] = {0, 0};
    hipEvent_t mix_ev[2] = {nullptr, nullptr};
    bool mix_busy[2] = {false, false};
  };
  // Wait for everything queued on `stream` so far (a synchronous call's end): the stream writes a
  // sequence number into ws's pinned marker word after its work (hipStreamWriteValue32) and the
  // caller polls it, which returns as soon as the GPU gets there -- hipStreamSynchronize's
  // completion-signal wait returned ~15-20 us later (C4 / C5 calls, profiles/r04).  Falls back to
  // hipStreamSynchronize when the marker cannot be written, and after kSpinLimitUs of polling (a
  // long host batch, a fault: the runtime then reports the error).
  Status finish(Workspace* ws, hipStream_t stream);
  static constexpr double kSpinLimitUs = 20000.0;
  static constexpr double kSpinBusyUs = 200.0;
  // Order ws->stream after the work already queued on the legacy default stream (and, by that
  // stream's semantics, on every blocking stream of the device): a device-memory call made
  // without a caller stream must not read its input before the kernel that produced it ran.
  // The workspace streams themselves are non-blocking, so concurrent callers do not serialise
  // on each other's null-stream work.
  Status order_after_default(Workspace* ws);
  // Check out a workspace with at least `bytes` of staging, `nflags` flag words (device + pinned
  // host) and `nbflags` batch flag words (zero on return).
  Status acquire(size_t bytes, size_t nflags, Workspace** out, size_t nbflags = 0, size_t ncrc = 0);
  void release(Workspace* ws);
  // Item-table room of `bytes` (host and device) in lane `slot` of ws; waits for the lane's earlier
  // table to be done with before it reallocates.
  Status reserve_mix(Workspace* ws, int slot, size_t bytes, hipStream_t stream);
  // Return a workspace whose work is still queued on `stream`: it is handed out again only once
  // the stream has passed this point.
  void release_after(Workspace* ws, hipStream_t stream);

 private:
  explicit DeviceContext(int device) : device_(device) {}
  int device_;
  std::mutex mu_;
  std::vector<std::unique_ptr<Workspace>> all_;
  std::vector<Workspace*> free_;  // release order: the front was released first
  // beyond this many workspaces an acquire with every free one still pending (asynchronous calls
  // queued without a sync) waits for the oldest instead of allocating another
  static constexpr size_t kMaxWorkspaces = 64;
};

// Makes `device` current for the scope, restoring the caller's device after.
class DeviceGuard {
 public:
  explicit DeviceGuard(int device);
  ~DeviceGuard();
  bool ok() const { return ok_; }

 private:
  int prev_ = -1;
  bool ok_ = false;
};

// One synchronous call's round trip on a device: the DeviceGuard, a checked-out workspace, the
// call's stream (a second lane on request), a sticky status, the wait, the release.  Every
// single-stripe entry point runs on one (RSEngine::run's legs, run_host, encode_crc, the crc32block
// and CRC32 calls of capi.cpp); the batch calls have BatchRun (batch.cpp).  The rules:
//   * First error wins.  step() issues nothing once a step has failed; the call returns the first
//     failing step's status and its set_last_error text.  (step takes the work as a callable: an
//     argument of type hipError_t would have been issued before step could decline it.)
//   * Always finish before release.  finish() waits on every stream the call used, after a failed
//     step too, and the destructor finishes (if the caller has not) before the workspace goes back.
//     Only a call that never began -- the guard or acquire failed: begun() false, status() says
//     why -- returns early with nothing to wait for.
//   * Words only after a good finish.  ws()->hflags is read only after finish() gave CFSEC_OK.
//   * The stream is an argument.  `caller` non-null: the call runs on it; null: on the workspace's
//     own non-blocking stream.  after_default: that stream is first ordered after the legacy default
//     stream (order_after_default).  Which site passes what:
//       run's in-place leg   caller's stream (device memory) / null (host rows in place), after_default = null stream
//       run's staged Verify  null, never ordered;  run_host: null + second_lane(), never ordered
//       encode_crc           as run;  after_default = nothing staged and the caller's stream is null
//       crc32block call      caller's stream even for host memory;  after_default = null stream, nothing staged
//       CRC32 batch          caller's stream;  after_default = null stream
class SyncCall {
 public:
  SyncCall(DeviceContext* ctx, size_t bytes, size_t nflags, hipStream_t caller, bool after_default);
  ~SyncCall();
  SyncCall(const SyncCall&) = delete;
  SyncCall& operator=(const SyncCall&) = delete;
  bool begun() const { return ws_ != nullptr; }
  bool ok() const { return st_ == CFSEC_OK; }
  Status status() const { return st_; }
  DeviceContext::Workspace* ws() const { return ws_; }
  hipStream_t stream() const { return stream_; }
  // the workspace's second stream (run_host's other lane); finish() then waits on it too
  hipStream_t second_lane() {
    two_lanes_ = true;
    return ws_->stream2;
  }
  // issue() returns a hipError_t (reported as `what`) or a Status whose error text is already set
  template <class F>
  bool step(const char* what, F&& issue) {
    if (st_ == CFSEC_OK) st_ = as_status(issue(), what);
    return st_ == CFSEC_OK;
  }
  // the usual steps, on the call's stream; fetch_words: the first n flag words to their pinned mirror
  bool copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    return step(kind == hipMemcpyHostToDevice ? "hipMemcpyAsync H2D" : "hipMemcpyAsync D2H",
                [&] { return hipMemcpyAsync(dst, src, bytes, kind, stream_); });
  }
  bool memset(void* p, int value, size_t bytes) {
    return step("hipMemsetAsync", [&] { return hipMemsetAsync(p, value, bytes, stream_); });
  }
  bool fetch_words(size_t n) { return copy(ws_->hflags, ws_->dflags, 4 * n, hipMemcpyDeviceToHost); }
  Status finish();

 private:
  static Status as_status(hipError_t e, const char* what) { return hip_status(e, what); }
  static Status as_status(Status st, const char*) { return st; }
  DeviceGuard guard_;
  DeviceContext* ctx_;
  DeviceContext::Workspace* ws_ = nullptr;
  hipStream_t stream_ = nullptr;
  Status st_ = CFSEC_OK;
  bool two_lanes_ = false, finished_ = false;
};

// KRS/inversion_tree.go:16-164: decode matrices keyed by the invalid indices seen
// before k valid rows were found; RW-locked for concurrent readers.
class InversionCache {
 public:
  bool get(const std::vector<int>& invalid, Matrix* out) const;
  void put(const std::vector<int>& invalid, const Matrix& m);

 private:
  mutable std::shared_mutex mu_;
  std::map<std::vector<int>, Matrix> map_;
};

// Rows to compute for one reconstruct call (shared by the single and batch paths).
struct ReconPlan {
  std::vector<int> valid;    // k surviving shard indices, first-present order
  std::vector<int> outputs;  // shard indices to rebuild
  Matrix rows;               // outputs.size() x k, over the shards in `valid`
};

// The 16 + 20 code's reconstruct (+ verify) through its 16x16 dyadic parity block
// (Dy16RepairJob): missing data rows from decode rows, then all 20 parity rows from the data.
struct Dy16Plan {
  int nd = 0;             // missing data rows
  int e = 0;              // extra rows (ExtraRows) after the 20 parity rows
  std::vector<int> rows;  // output shard indices: the nd missing data rows, parity rows k .. k+19, extras
  uint8_t src[16] = {};
  uint32_t pstore = 0, pcmp = 0;
  Matrix coef;  // (20 + e + nd) x 16: parity matrix, extra rows, decode rows
  // the syndrome form of the bit-sliced repair (gf_bs16.hip): parity row prow[q] stands in for
  // missing data row rows[q]; the missing rows are ainv (nd x nd) times the stand-ins' syndromes
  bool syn = false;
  uint8_t prow[4] = {};
  uint8_t ainv[16] = {};
};

// Rows beyond a code's own that a Reconstruct + Verify pass can check on the way: row j over the
// k data columns, compared with shard idx[j] of the stripe's shard array.  The LRC local parities
// (LrcEncoder: the global pass also does the per-AZ local Verify, lrcencoder.go:89-131).
struct ExtraRows {
  Matrix rows;
  std::vector<int> idx;
};

// The product one stripe of a heterogeneous batch needs (batch.cpp): rows x shards[in]; rows
// [0, nstore) are written to shards[out[0 .. nstore)), the rest compared with shards[out[nstore ..)]
// (a mismatch raises the stripe's flag).  Shared by every stripe with the same erasure pattern.
struct StripePlan {
  std::vector<int> in;
  std::vector<int> out;
  int nstore = 0;
  int nextra = 0;  // the last nextra rows of out are ExtraRows, compared
  Matrix rows;  // out.size() x in.size()
  std::shared_ptr<const Dy16Plan> dy16;  // set where that product is the cheaper one
  bool compares() const { return out.size() > (size_t)nstore; }  // some row is compared (Verify)
};
// The plan over a whole stripe: rows (total - k x k) x shards [0, k) into shards [k, total), the first
// nstore of them stored (an Encode: all of them), the rest compared (a Verify: nstore = 0).
StripePlan whole_stripe_plan(int k, int total, const Matrix& rows, int nstore);

// The device (0 .. ndev-1) each of n stripes of a host-memory batch runs on: contiguous runs
// balanced by the bytes each stripe moves (cfsec_batch_partition).
void partition_stripes(const uint64_t* bytes, int n, int ndev, int* dev);

// An asynchronous batch call's destination: kernels on `stream`, per-item Verify mismatches OR-ed
// into the device words flags[owner] (the caller zeroes them).
struct AsyncOut {
  hipStream_t stream = nullptr;
  uint32_t* flags = nullptr;
};

// Shard checksums a batch call returns (crc32.ChecksumIEEE, access/stream_put.go:249-253,
// blobnode/work_shard_recover.go:335-342): words[w] for the rows the tasks name (StripeTask::crc);
// host memory for the synchronous calls (words the call does not compute are left alone), device
// memory on the call's stream for the asynchronous ones (zeroed by the call first).
struct CrcOut {
  uint32_t* words = nullptr;
  size_t n = 0;
  // reconstruct batches: false = the shards the call rebuilt (the _crc forms), true = every shard of
  // the bid as it stands after the call, survivors included (the repair form: StripeTask::crc = 3),
  // kept for a bid whose Verify is false
  bool every = false;
};

// One stripe of a batch call: its shard vector, the plan, its length, its result.
struct StripeTask {
  cfsec_shard* shards = nullptr;
  const StripePlan* plan = nullptr;
  size_t len = 0;
  int* status = nullptr;        // set to CFSEC_ERR_VERIFY when a compared row mismatches
  int dev = 0;                  // index into the engine's device list
  int phase = 0;                // tasks of phase p run after every task of phase p - 1 (same call)
  int owner = 0;                // batch item: a host batch keeps an item's tasks on one device; the
                                // item's Verify word (asynchronous calls: the caller's flags[owner])
  int crc = 0;                  // checksums: 0 none, 1 the stored rows, 2 inputs + stored rows, 3 every row
                                // (inputs, stored and compared rows, ExtraRows included), 4 the stored and
                                // compared rows (an AZ's local pass of a bid whose global pass is in mode 3:
                                // every word of an item is written by exactly one task)
  int64_t crc_word = 0;         // CrcOut word of shard index 0 of this task's item
  const int* crc_map = nullptr; // shard index -> index in the item (local views), or identity
  int split = 0;                // CFSEC_VERIFY_SPLIT: 1 the Verify pass over the whole stripe, 2 its store pass
};

// The stripe ranges [t0, t1) one launch group (stripes sharing a plan) is launched in, by the
// addresses of its rows: in[t * k + c], out[t * m + r] and (dy16 plans) hout[t * mo + r], lens[t].
// Maximal runs of stripes at one non-zero stride from each other on every row launch as affine
// batches; runs shorter than 4 stripes are gathered into pointer-table runs.  Groups of fewer than 3
// stripes or of several lengths are one run.  Host arithmetic only (batch.cpp).
std::vector<std::pair<size_t, size_t>> split_runs(const uint8_t* const* in, size_t k, const uint8_t* const* out,
                                                  size_t m, const uint8_t* const* hout, size_t mo,
                                                  const uint64_t* lens, size_t nt);
// The staged tasks [i0, i1) that share one staging lane of lane_bytes, i1 returned: whole stripes,
// every row of plan->in then plan->out (compared rows too) in a slot of align_up(len, kSlotAlign)
// bytes; offsets gets each row's offset from the lane's base, task after task.  A task larger than
// the lane still goes, alone.  Host arithmetic only (batch.cpp).
size_t pack_chunk(const StripeTask* const* tasks, size_t n, size_t i0, size_t lane_bytes,
                  std::vector<size_t>* offsets);

// The item table of a mixed-plan launch (gf_mix.hpp), packed from the tasks that qualify: a store-only
// plan without a dy16 product, 1 .. kLaunchMaxRows inputs, 0 < len <= max_len, no checksums, and room
// left below kMixMaxTiles tiles.  rows[i][p] = task i's row p of plan->in followed by plan->out, stored
// in that order; coefficient rows once per plan (by address).  dst == nullptr, or cap below the bytes
// needed: nothing is written (the sizing pass).  `left` lists the tasks not packed, in order.  Host
// arithmetic only (batch.cpp): no device calls, no address is dereferenced.
struct MixPack {
  size_t bytes = 0;  // the table's size
  uint32_t items = 0, tiles = 0, plans = 0;
  std::vector<size_t> left;
};
MixPack pack_mix(const StripeTask* const* tasks, uint8_t* const* const* rows, size_t n, size_t max_len, uint8_t* dst,
                 size_t cap);
// Segments up to this length go into a mixed launch (BatchRun::launch_part); CFSEC_MIX_MAX_LEN, read
// per call, overrides it (0: no mixed launch).  The value is the largest swept length at which the
// mixed launch was no slower than the launch groups on a one-pattern batch of 64 scattered EC12P4
// segments in HBM (tools/seg_batch_probe.py --sweep, us per segment, mixed / groups):
//                 16 KiB        64 KiB        256 KiB       1 MiB
//   one pattern   0.42 / 0.54   0.52 / 0.65   1.24 / 1.06   3.20 / 2.91
//   distinct      0.64 / 5.68   0.71 / 6.04   1.39 / 6.11   3.42 / 6.77
// EC6P6 (6 inputs: the fixed-K kernel's launches are short) does not fit the rule: its one-pattern
// batch is slower mixed at every swept length (0.38 / 0.32, 0.44 / 0.36, 0.92 / 0.60, 1.97 / 1.58),
// by 4-5 us per 64-segment call up to 64 KiB -- the table's copy to the device -- while its
// distinct-pattern batch is faster mixed up to 256 KiB (0.48 / 1.07, 0.52 / 1.12, 1.00 / 1.24,
// 2.04 / 2.15).  One limit serves both: a batch's patterns are not known to be one until it is planned.
constexpr size_t kMixMaxLen = size_t(64) << 10;
// The item table of a mixed-plan launch with checksums (gf_mix_crc.hpp), packed like pack_mix's from
// the tasks that qualify: a store-only plan without a dy16 product (no output rows at all is fine: the
// inputs are checksummed), 1 .. kLaunchMaxRows inputs, 0 < len <= max_len, every shard checksummed
// (crc == 2) without an index remap, the only checksummed task of its item -- tasks_per_owner counts
// the checksummed tasks per StripeTask::owner (NULL: counted over `tasks`), the rule and the reason
// of crc_word_stride -- every word inside [0, nwords), and room left below kMixMaxTiles tiles.  The
// table names each row's word (crc_word + shard index) and per item the two length-dependent CRC
// constants; tabs / crc: the device addresses of the CRC table block and of word 0, stored as numbers.
// Sizing pass, short buffer, `left` and one coefficient copy per plan as pack_mix.  Host arithmetic only.
MixPack pack_mix_crc(const StripeTask* const* tasks, uint8_t* const* const* rows, size_t n, size_t max_len,
                     size_t nwords, uint64_t tabs, uint64_t crc, const std::map<int, int>* tasks_per_owner,
                     uint8_t* dst, size_t cap);
// The route's length limit is kMixMaxLen: its rule, applied to this launch with one limit serving every
// mode, gives 64 KiB again (tools/put_blobs_probe.py --sweep, 64 scattered blobs of ONE shard size in
// HBM, us per blob, mixed / groups):
//                 16 KiB        64 KiB        256 KiB       1 MiB
//   EC12P4        1.07 / 3.72   1.49 / 3.75   3.15 / 4.01   9.56 / 6.72
//   EC6P10L2      1.21 / 4.75   1.73 / 4.72   3.87 / 5.21   12.28 / 9.62
//   EC6P6         0.79 / 2.38   1.41 / 2.40   3.02 / 2.89   9.00 / 6.29
// EC6P6 is slower mixed at 256 KiB, so the largest swept length at which no mode loses is 64 KiB; no
// point between 64 and 256 KiB was swept.
// The item table of a mixed-plan launch that stores, compares and checksums (gf_mix_sv.hpp): blobnode's
// repair step, Reconstruct + Verify + every shard's CRC32.  A task is taken when all of these hold: its
// plan has no dy16 product, 1 .. kLaunchMaxRows inputs and at least one output row (stored or compared:
// compares() may be true or false -- a bid with exactly N survivors compares nothing and still
// belongs); 0 < len <= max_len; not half of a split Verify (split == 0); every row checksummed
// (crc == 3) without an index remap; the only checksummed task of its item (tasks_per_owner, as
// pack_mix_crc); every word inside [0, nwords); room left below kMixMaxTiles tiles.  Each item carries
// the plan's nstore and flags[i], the address of task i's Verify word as a number (NULL: zeros).
// Sizing pass, short buffer, `left` and one coefficient copy per plan as pack_mix.  Host arithmetic only.
MixPack pack_mix_sv(const StripeTask* const* tasks, uint8_t* const* const* rows, const uint64_t* flags, size_t n,
                    size_t max_len, size_t nwords, uint64_t tabs, uint64_t crc,
                    const std::map<int, int>* tasks_per_owner, uint8_t* dst, size_t cap);
// This route's length limit is kMixMaxLen as well: the same rule (tools/repair_bids_probe.py --sweep, 64
// scattered bids of ONE shard size and one bad index in HBM, us per bid, mixed / groups):
//                 16 KiB        64 KiB        256 KiB       1 MiB
//   EC12P4        1.29 / 3.58   1.55 / 3.67   3.24 / 4.83   9.91 / 8.80
//   EC6P6         0.86 / 2.27   1.50 / 2.37   3.12 / 3.31   9.59 / 7.93
//   EC6P10L2      1.27 / 1.67   1.85 / 2.13   4.11 / 3.65   13.75 / 9.46
// EC6P10L2 is slower mixed at 256 KiB, so the largest swept length at which no mode loses is 64 KiB; no
// point between 64 and 256 KiB was swept.
// The item table of the mixed-plan repair launch of the 16 + 20 code (gf_mix_sv16.hpp): the tasks
// pack_mix_sv refuses for their dy16 product.  A task is taken when all of these hold: its plan carries
// a Dy16Plan (nd <= 4 missing data rows, 0 or 2 extra rows, src[] consistent with rows[]) and has 16
// inputs; 0 < len <= max_len; split == 0; crc == 3 without an index remap; the only checksummed task of
// its item (tasks_per_owner, as pack_mix_crc); every word inside [0, nwords); room left below
// kMixMaxTiles tiles.  Per item: len, tiles, the CRC constants, flags[i] (the address of task i's Verify
// word, NULL: zeros), the plan's nd, e, pstore, pcmp and src[j] = the data row of missing row j; the 16
// input addresses in data-row slot order (gf_dy16.hip to_slot_order), then the addresses of
// Dy16Plan::rows; parallel to them the word each row writes -- kMixNoWord for a parity row with neither
// mask bit (a stand-in already among the inputs, or a row nobody asked for), so every shard of the bid
// has exactly one writer.  One coefficient block per plan (by address): Dy16Plan::coef with the decode
// rows' columns permuted to slot order.  Sizing pass, short buffer and `left` as pack_mix.  Host
// arithmetic only.
MixPack pack_mix_sv16(const StripeTask* const* tasks, uint8_t* const* const* rows, const uint64_t* flags, size_t n,
                      size_t max_len, size_t nwords, uint64_t tabs, uint64_t crc,
                      const std::map<int, int>* tasks_per_owner, uint8_t* dst, size_t cap);

// Plans built for one batch call (stable addresses for the tasks that point at them).
struct PlanStore {
  std::vector<std::unique_ptr<StripePlan>> other;
  StripePlan* add(const StripePlan& p) {
    other.emplace_back(new StripePlan(p));
    return other.back().get();
  }
};

class RSEngine {
 public:
  static Status create(int k, int m, int device, std::unique_ptr<RSEngine>* out);
  int k() const { return k_; }
  int m() const { return m_; }
  int total() const { return k_ + m_; }
  int device() const { return ctx_ ? ctx_->device() : -1; }
  const Matrix& matrix() const { return mat_; }
  // rows [r0, r0 + nr) of the encoding matrix (the parity rows: matrix_rows(k, m))
  Matrix matrix_rows(int r0, int nr) const {
    Matrix out(nr, k_);
    for (int r = 0; r < nr; ++r)
      for (int c = 0; c < k_; ++c) out.at(r, c) = mat_.at(r0 + r, c);
    return out;
  }

  Status encode(cfsec_shard* shards, int n, int mem, hipStream_t stream);
  // Encode + crc32.ChecksumIEEE of every shard into host crcs[n], one fused pass.
  Status encode_crc(cfsec_shard* shards, int n, int mem, hipStream_t stream, uint32_t* crcs);
  Status verify(cfsec_shard* shards, int n, int mem, hipStream_t stream, bool* ok);
  Status reconstruct(cfsec_shard* shards, int n, bool data_only, int mem, hipStream_t stream);
  // EncodeIdx (KRS/reedsolomon.go:631-667): parity[r] ^= M[k + r][idx] * data_shard.
  Status encode_idx(const cfsec_shard* data_shard, int idx, cfsec_shard* parity, int nparity, int mem,
                    hipStream_t stream);
  // Update (KRS/reedsolomon.go:672-734): for every present new_data[c], shards[c] ^= new_data[c] (the
  // old shard is left holding the delta, as in the reference), then parity[r] ^= M[k + r][c] * shards[c].
  Status update(cfsec_shard* shards, int n, const cfsec_shard* new_data, int nnew, int mem, hipStream_t stream);
  // ReconstructSome (KRS/reedsolomon.go:1395-1397): the missing data shards i with required[i] only
  // (entries from nrequired on count as false).  The decode matrix is the inversion cache's; the
  // selected rows are copied out of it per call -- no plan is cached under the required mask.
  Status reconstruct_some(cfsec_shard* shards, int n, const uint8_t* required, int nrequired, int mem,
                          hipStream_t stream);
  Status split(uint8_t* data, size_t len, size_t cap, cfsec_shard* out, uint8_t* pad,
               size_t pad_len, size_t* pad_needed);
  Status join(uint8_t* dst, size_t dst_len, const cfsec_shard* shards, int n, size_t out_size);

  Status encode_batch(uint8_t* const* ptrs, size_t S, int nstripes, hipStream_t stream);
  Status verify_batch(uint8_t* const* ptrs, size_t S, int nstripes, uint32_t* flags,
                      hipStream_t stream);
  Status reconstruct_batch(uint8_t* const* ptrs, size_t S, int nstripes, const int* erased,
                           int nerased, bool data_only, hipStream_t stream);
  // outputs = coef (rows x k) x inputs for every stripe of a device batch: ptrs[s*(k+rows) ..] =
  // the k inputs, then the rows outputs (any rows, e.g. ECEncoder::repair_rows).
  Status matvec_batch(const uint8_t* coef, int rows, uint8_t* const* ptrs, size_t S, int nstripes,
                      hipStream_t stream);
  // Update of a device batch: columns cols[0 .. ncols) (strictly increasing) of every stripe change to
  // new_ptrs[s * ncols + j]; ptrs as encode_batch (unchanged data columns are never dereferenced).
  Status update_batch(uint8_t* const* ptrs, uint8_t* const* new_ptrs, const int* cols, int ncols, size_t S,
                      int nstripes, hipStream_t stream);
  // The same with crc32.ChecksumIEEE of the shards (fused into the kernel where supported):
  // crcs = device [nstripes * total()]; encode checksums every shard, reconstruct the rebuilt ones
  // (other words 0).
  Status encode_crc_batch(uint8_t* const* ptrs, size_t S, int nstripes, uint32_t* crcs, hipStream_t stream);
  Status reconstruct_crc_batch(uint8_t* const* ptrs, size_t S, int nstripes, const int* erased, int nerased,
                               bool data_only, uint32_t* crcs, hipStream_t stream);
  // Reconstruct, the Verify of the same pass (flags[s] |= 1 on a mismatch, as verify_batch) and every
  // shard's checksum as it stands afterwards: every word of crcs filled.
  Status repair_crc_batch(uint8_t* const* ptrs, size_t S, int nstripes, const int* erased, int nerased,
                          uint32_t* flags, uint32_t* crcs, hipStream_t stream);

  // Plan the rows of a reconstruct given which shards are present.
  Status plan_reconstruct(const std::vector<bool>& present, bool data_only, ReconPlan* plan);

  // ---- heterogeneous stripe batches (batch.cpp) ----
  // The devices batch entry points spread stripes over (the handle's own device first).
  Status set_devices(const int* devices, int n);
  int ndevices() const { return (int)devs_.size(); }
  // `stripes` holds nst pointers to shard vectors of total() entries; each stripe has its own
  // shard size and missing set.  Per-stripe results go to status[]; the return value reports only
  // failures of the call itself (device errors, bad arguments).
  //   encode:              Encode(shards)                         (KRS/reedsolomon.go:609-625)
  //   verify:              Verify(shards): OK, or CFSEC_ERR_VERIFY when it returns false
  //   reconstruct(verify): Reconstruct(shards) [then Verify(shards)], the blobnode repair step
  //                        (blobnode/work_shard_recover.go:751-760), in one fused pass
  Status encode_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status);
  //   encode_crc:          Encode(shards), then crc32.ChecksumIEEE of every shard into
  //                        crcs[s * total() + shard] (host words; all zero for a stripe that failed);
  //                        small stripes of any mix of lengths share one mixed launch with checksums
  Status encode_crc_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status, uint32_t* crcs);
  Status verify_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status);
  Status reconstruct_stripes(cfsec_shard* const* stripes, int nst, int mem, bool verify, int* status);
  //   repair_crc:          reconstruct(verify = true), and crc32.ChecksumIEEE of every shard as it stands
  //                        afterwards into crcs[s * total() + shard] (host words) for a stripe whose status
  //                        is OK or CFSEC_ERR_VERIFY, zeros for any other; small stripes of any mix of
  //                        lengths and erasure patterns share one mixed launch (run_stripes' mix_sv).
  //                        More than kLaunchMaxRows data shards: CFSEC_ERR_NOT_SUPPORTED.
  Status repair_crc_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status, uint32_t* crcs);
  //   reconstruct_data:    ReconstructData(shards) (KRS/reedsolomon.go:1377-1397): the missing data
  //                        shards only; small segments of any erasure patterns share one mixed launch
  Status reconstruct_data_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status);
  //   reconstruct_some:    ReconstructSome(shards, required + s * k) per stripe: of the missing data
  //                        shards only those its k-entry mask names; plans built per call (the rows of
  //                        the cached data-only plan that the mask selects), mixed launch as above
  Status reconstruct_some_stripes(cfsec_shard* const* stripes, int nst, const uint8_t* required, int mem,
                                  int* status);
  // The planning half of reconstruct_stripes: checks every stripe (errors to status[s]), sets the
  // rebuilt shards' lengths and appends the tasks (phase `phase`, and phase + 1 for a split Verify)
  // that run_stripes executes; owner of stripe s = owner0 + s.
  // extra / fuse (optional): stripe s also compares the ExtraRows when fuse[s] (and verify).
  // data_only (verify false): ReconstructData -- a stripe with every data shard present is a no-op, the
  // plans hold the missing data shards only, nothing compared, no dy16 product.
  void plan_reconstruct_tasks(cfsec_shard* const* stripes, int nst, bool verify, int* status, int phase,
                              int owner0, PlanStore* store, std::vector<StripeTask>* tasks,
                              const ExtraRows* extra = nullptr, const std::vector<bool>* fuse = nullptr,
                              bool data_only = false);
  // Run the tasks' products (device memory, pinned host memory in place, pageable host memory
  // through double-buffered staging), tasks partitioned over the devices.
  // async (device memory, the handle's first device): enqueue on async->stream and return; verify
  // mismatches OR 1 into async->flags[owner] instead of setting the tasks' status.
  // mix (synchronous calls): small store-only tasks of a part share one mixed-plan launch
  // (BatchRun::launch_part); false: every task goes through the launch groups.
  // mix_crc (synchronous calls): small store-only tasks that checksum every shard share one mixed-plan
  // launch with checksums per part (pack_mix_crc's rule); false: the launch groups and their checksum
  // routes, as every call before the put batches of mixed-size blobs.
  // mix_sv (synchronous calls): small tasks that store, compare and checksum every shard (a repair
  // tasklet's bids) share one mixed-plan launch per part (pack_mix_sv's rule), their Verify words routed
  // as the groups route theirs; false: the launch groups, as every call before the repair of mixed-size bids.
  Status run_stripes(std::vector<StripeTask>& tasks, int mem, const AsyncOut* async = nullptr,
                     const CrcOut* crc = nullptr, bool mix = false, bool mix_crc = false, bool mix_sv = false);
  // Plan of a Reconstruct (+ Verify) over the present shards; data_only: of a ReconstructData.
  Status plan_stripe(const std::vector<bool>& present, bool verify, StripePlan* plan,
                     const ExtraRows* extra = nullptr, bool data_only = false);
  // plan->dy16 where the code and the erasure pattern make that product cheaper (batch.cpp).
  void plan_dy16(const std::vector<bool>& present, const Matrix& dec, StripePlan* plan,
                 const ExtraRows* extra = nullptr) const;
  // The batch calls stripe by stripe through the single-stripe calls (k > kLaunchMaxRows Verify).
  Status stripes_one_by_one(cfsec_shard* const* stripes, int nst, int mem, bool reconstruct, bool verify,
                            int* status);
  // Run a plan's Verify as a separate encode-matrix pass instead of its compared rows.
  bool split_verify(const StripePlan& p) const;

  // Generic "outputs = rows x inputs" over caller shards (host or device memory).
  // mode kVerify: *ok set; outputs are read, not written.
  Status run(const Matrix& rows, const std::vector<cfsec_shard*>& ins,
             const std::vector<cfsec_shard*>& outs, size_t S, int mem, hipStream_t stream,
             MatVecMode mode, bool* ok);

  // Columns of a host-memory call per chunk (bytes per row) through the two-stream pipeline.
  static constexpr size_t kHostChunk = 1 << 20;
  // pageable host calls moving at most this many bytes take the page-locked staging path (run)
  static constexpr size_t kSmallPageable = 1 << 20;

 private:
  Status code_stripe(cfsec_shard* shards, int n, int mem, hipStream_t stream, MatVecMode mode, bool* ok);
  // The legs of run, one per CallPath (single_call_path below); a call's rows are its rows.cols
  // inputs, then its rows.rows outputs.  kInPlace / kPinnedInPlace: d holds the rows' device addresses
  // (device memory, aliases of page-locked host rows).
  Status run_in_place(const Matrix& rows, uint8_t* const* d, size_t S, hipStream_t stream, MatVecMode mode,
                      bool* ok);
  // kSmallStage: the rows copied on the CPU into the page-locked `stage` (device address dstage),
  // coded there in place, the outputs copied back
  Status run_small_stage(const Matrix& rows, const std::vector<cfsec_shard*>& all, size_t S, MatVecMode mode,
                         bool* ok, uint8_t* stage, uint8_t* dstage);
  // kPipeline
  Status run_host(const Matrix& rows, const std::vector<cfsec_shard*>& ins,
                  const std::vector<cfsec_shard*>& outs, size_t S, MatVecMode mode, bool* ok);
  // kStagedWhole: whole rows through the workspace, for the Verify of more inputs than one launch carries
  Status run_staged_verify(const Matrix& rows, const std::vector<cfsec_shard*>& all, size_t S, bool* ok);
  // EncodeIdx / Update on one SyncCall: out[r] ^= coef[r][c] * d[c] (gf_delta.hpp), d[c] = olds[c] ^
  // news[c] stored back to olds[c], or olds[c] itself when news is empty.  Device memory in place on the
  // caller's stream; host rows that are all page-locked in place on a workspace stream; any other host
  // call staged whole (every row copied in, olds -- when rewritten -- and outs copied back).
  Status run_delta(const Matrix& coef, const std::vector<uint8_t*>& olds, const std::vector<uint8_t*>& news,
                   const std::vector<uint8_t*>& outs, size_t S, int mem, hipStream_t stream);
  // encode_stripes (nstore = m) and verify_stripes (nstore = 0): the parity rows over whole stripes
  Status whole_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status, int nstore);
  RSEngine() = default;
  int k_ = 0, m_ = 0;
  Matrix mat_;     // total x k
  Matrix parity_;  // m x k (r.parity, KRS/reedsolomon.go:568-571)
  InversionCache tree_;
  // Reconstruct plans across calls (blobnode's tasklets repeat one erasure pattern call after call):
  // key = the present shards + [extra rows fused] + [verify] + [data only]; a cached plan is never changed or
  // freed, so concurrent callers share it.  Beyond kMaxCachedPlans patterns a call keeps its own.
  std::mutex plan_mu_;
  std::map<std::vector<bool>, std::unique_ptr<StripePlan>> plan_cache_;
  static constexpr size_t kMaxCachedPlans = 4096;
  const StripePlan* cached_plan(const std::vector<bool>& present, bool fx, bool verify, const ExtraRows* extra,
                                PlanStore* store, Status* st, bool data_only = false);
  DeviceContext* ctx_ = nullptr;
  std::vector<DeviceContext*> devs_;  // batch devices, ctx_ first
  Status run_device(std::vector<StripeTask*>& tasks, int mem, DeviceContext* ctx, const AsyncOut* async,
                    const CrcOut* crc, bool mix, bool mix_crc, bool mix_sv);
};

// The way a single-stripe call (RSEngine::run) takes, from facts gathered before anything is queued:
//   kInPlace        device memory: the rows as they are, on the caller's stream
//   kPinnedInPlace  host memory, every row page-locked (rows_aliasable: device_alias took every input
//                   and output row): the kernel reads and writes them over PCIe, no copies
//   kSmallStage     other host calls moving at most kSmallPageable bytes, with a page-locked stage
//                   the GPU addresses (stage_usable): copied there on the CPU and coded in place
//   kPipeline       other host calls: run_host's chunked two-stream pipeline
//   kStagedWhole    host Verify of more inputs than one launch carries (mode == kVerify && nin > 32)
//                   whose rows are not all page-locked: whole rows staged, two launches
// Host arithmetic only; tests/test_call_path.py pins the table.
enum class CallPath { kInPlace, kPinnedInPlace, kSmallStage, kPipeline, kStagedWhole };
CallPath single_call_path(bool host, bool rows_aliasable, bool stage_usable, size_t moved_bytes, int nin,
                          MatVecMode mode);

// Counting semaphore (util/limit/count.NewBlockingCount, encoder.go:90).
class BlockingCount {
 public:
  explicit BlockingCount(int n) : left_(n) {}
  void acquire() {
    std::unique_lock<std::mutex> l(mu_);
    cv_.wait(l, [&] { return left_ > 0; });
    --left_;
  }
  void release() {
    std::lock_guard<std::mutex> l(mu_);
    ++left_;
    cv_.notify_one();
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  int left_;
};

class ECEncoder {
 public:
  static Status create(const cfsec_tactic& t, bool enable_verify, int concurrency, int device,
                       std::unique_ptr<ECEncoder>* out);
  virtual ~ECEncoder() = default;
  virtual Status encode(cfsec_shard* shards, int n, int mem, hipStream_t s);
  virtual Status reconstruct(cfsec_shard* shards, int n, const int* bad, int nbad, int mem,
                             hipStream_t s);
  virtual Status reconstruct_data(cfsec_shard* shards, int n, const int* bad, int nbad, int mem,
                                  hipStream_t s);
  virtual Status verify(cfsec_shard* shards, int n, int mem, hipStream_t s, bool* ok);
  virtual std::vector<int> shards_in_idc(int idx) const;
  const cfsec_tactic& tactic() const { return t_; }
  // Repair over survivors held elsewhere (chubaofs_amd/repair.py ships only the first N present
  // global shards): in[0..N) = the first N global shards not in bad (KRS/reedsolomon.go:1453-1465),
  // rows[w * N ..] = shard want[w] (data, global parity, or an LRC local parity) over them.
  Status repair_rows(const int* bad, int nbad, const int* want, int nwant, int* in, uint8_t* rows);
  Status matvec_batch(const uint8_t* coef, int rows, uint8_t* const* ptrs, size_t S, int nstripes,
                      hipStream_t stream) {
    return engine_->matvec_batch(coef, rows, ptrs, S, nstripes, stream);
  }
  // Devices the batch entry points spread bids over (batch.cpp).
  virtual Status set_devices(const int* devices, int n);
  // blobnode's repair step over a batch of bids (work_shard_recover.go:708-771): for bid b, the
  // n shards at shards[b*n ..], Reconstruct(shards_b, bad_b) then Verify(shards_b), where bad_b =
  // bad[bad_off[b] .. bad_off[b+1]); status[b] = the Reconstruct error, CFSEC_ERR_VERIFY when Verify
  // returns false, or CFSEC_OK.  verify = false: Reconstruct only.
  // async (device memory, asynchronous on async->stream): status[b] gets the planning result at
  // return; a Verify mismatch ORs 1 into async->flags[b] when the stream gets there.
  // crc: the rebuilt shards' checksums into crc->words[b * n + shard] (other words untouched).
  // bids (with crc->every, synchronous): a tasklet of bids of mixed sizes -- the small bids share one
  // mixed launch that stores, compares and checksums (run_stripes' mix_sv); same results.
  virtual Status reconstruct_batch(cfsec_shard* shards, int n, int nbids, const int* bad, const int* bad_off,
                                   int mem, bool verify, int* status, const AsyncOut* async = nullptr,
                                   const CrcOut* crc = nullptr, bool bids = false);
  // Encode over a batch of stripes of n shards each (access puts, stream_put.go:104-143), with
  // the Config's EnableVerify; status[s] as Encode would return it.
  // crc: every shard's checksum after the Encode into crc->words[s * n + shard].
  // blobs (with crc, synchronous): a put batch of blobs of mixed sizes -- the small stripes share one
  // mixed launch with checksums (run_stripes' mix_crc); same results.
  virtual Status encode_batch(cfsec_shard* shards, int n, int nstripes, int mem, int* status,
                              const AsyncOut* async = nullptr, const CrcOut* crc = nullptr, bool blobs = false);
  // access's degraded reads as one call (stream_get.go:420-431): item i is the n shards at
  // shards[i*n ..] with bad indices bad[bad_off[i] .. bad_off[i+1]); status[i] = what
  // reconstruct_data returns for the item alone.  One concurrency slot for the call.
  virtual Status reconstruct_data_batch(cfsec_shard* shards, int n, int nitems, const int* bad, const int* bad_off,
                                        int mem, int* status);

 protected:
  // Shard index g (< N + M + L) as a row over the N data shards.
  virtual bool row_over_data(int g, uint8_t* dst) const;
  struct Slot {
    explicit Slot(BlockingCount* p) : p_(p) { p_->acquire(); }
    ~Slot() { p_->release(); }
    BlockingCount* p_;
  };
  cfsec_tactic t_{};
  bool enable_verify_ = false;
  std::unique_ptr<BlockingCount> pool_;
  std::unique_ptr<RSEngine> engine_;
};

class LrcEncoder : public ECEncoder {
 public:
  Status encode(cfsec_shard* shards, int n, int mem, hipStream_t s) override;
  Status reconstruct(cfsec_shard* shards, int n, const int* bad, int nbad, int mem,
                     hipStream_t s) override;
  Status reconstruct_data(cfsec_shard* shards, int n, const int* bad, int nbad, int mem,
                          hipStream_t s) override;
  Status verify(cfsec_shard* shards, int n, int mem, hipStream_t s, bool* ok) override;
  std::vector<int> shards_in_idc(int idx) const override;
  Status set_devices(const int* devices, int n) override;
  Status reconstruct_batch(cfsec_shard* shards, int n, int nbids, const int* bad, const int* bad_off, int mem,
                           bool verify, int* status, const AsyncOut* async = nullptr,
                           const CrcOut* crc = nullptr, bool bids = false) override;
  Status encode_batch(cfsec_shard* shards, int n, int nstripes, int mem, int* status,
                      const AsyncOut* async = nullptr, const CrcOut* crc = nullptr, bool blobs = false) override;
  Status reconstruct_data_batch(cfsec_shard* shards, int n, int nitems, const int* bad, const int* bad_off, int mem,
                                int* status) override;

 protected:
  bool row_over_data(int g, uint8_t* dst) const override;

 private:
  // Encode of one full stripe (n == N+M+L) without taking a concurrency slot (the caller holds one).
  Status encode_stripe(cfsec_shard* shards, int n, int mem, hipStream_t s);
  friend class ECEncoder;
  std::unique_ptr<RSEngine> local_;
  Matrix fused_;  // (M+L) x N: global parity rows then local parity rows, over data
};

}  // namespace cfsec
