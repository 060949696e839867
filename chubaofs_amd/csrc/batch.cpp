// batch.cpp -- heterogeneous stripe batches over one or more GPUs (see engine.hpp).
//
// The reference codes one stripe per call: access puts encode one blob at a time
// (access/stream_put.go:104-143, up to 4 in flight per request) and blobnode repairs a tasklet bid
// by bid, each bid with its own shard size and its own missing set, Reconstruct then Verify
// (blobnode/work_shard_recover.go:708-771).  Here a whole batch is one call: stripes with the same
// erasure pattern share one decode plan and run in the same launches (per-stripe lengths in the
// kernel arguments), Reconstruct + Verify is one pass (the stored rows and the compared rows come
// out of one product over the first k present shards), and the stripes are spread over the
// handle's devices, each with its own streams and staging.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <thread>

#include "engine.hpp"
#include "gf_mix.hpp"
#include "crc_pow.hpp"
#include "gf_mix_crc.hpp"
#include "gf_mix_sv.hpp"
#include "gf_mix_sv16.hpp"

namespace cfsec {
namespace {

constexpr size_t kLaneBudget = size_t(256) << 20;  // staging bytes per lane of a pageable batch

// The HIP device that owns device memory p, or -1.
int device_of(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  if (attr.type != hipMemoryTypeDevice) return -1;
  return attr.device;
}

// A whole stripe an Encode or a Verify takes: every shard of one size (checkShards), every one there.
Status whole_stripe_ok(const cfsec_shard* sh, int n, size_t* size) {
  Status st = check_shards(sh, n, false, size);
  for (int i = 0; i < n && st == CFSEC_OK; ++i)
    if (!sh[i].data) st = CFSEC_ERR_INVALID_ARG;
  return st;
}

// The tasks planned over the stripes a call kept (owner = index among those) belong to the items
// pos[owner] of the call: the item's verify word, its device, and -- with crc -- the checksums of its
// rebuilt shards (blobnode ShardCrc32) at words [item * n, item * n + n).
// crc->every: every shard of the item, each word written by exactly one task -- a task checksums all
// its rows (mode 3); where a Verify pass over the whole stripe follows a store pass (split), the
// Verify pass alone; a task from first_local on is an AZ's local pass behind a global one, which
// has checksummed the AZ's global shards: the local parities only (mode 4).
void stamp_items(std::vector<StripeTask>& tasks, const std::vector<int>& pos, const CrcOut* crc, int n,
                 size_t first_local = (size_t)-1) {
  for (size_t i = 0; i < tasks.size(); ++i) {
    StripeTask& t = tasks[i];
    t.owner = pos[t.owner];
    t.crc = !crc ? 0 : !crc->every ? 1 : t.split == 2 ? 0 : i >= first_local ? 4 : 3;
    t.crc_word = (int64_t)t.owner * n;
  }
}

// A set of tasks with resolved device addresses, launched on one stream: the in-place tasks of a
// phase, or one staged chunk.  rows[i][p] = task i's row p of plan->in followed by plan->out.
struct Part {
  std::vector<StripeTask*> tasks;
  std::vector<uint8_t* const*> rows;
};

// The rows a task checksums: f(position in plan->in followed by plan->out, CrcOut word) for every
// input row (crc == 2, 3), every stored row and every compared row (crc == 3, 4) whose word lies in
// [0, nwords).
template <class F>
void for_each_crc_row(const StripeTask& t, size_t nwords, F f) {
  if (!t.crc) return;
  const size_t k = t.plan->in.size();
  const auto visit = [&](size_t p, int row) {
    const int64_t w = t.crc_word + (t.crc_map ? t.crc_map[row] : row);
    if (w >= 0 && (size_t)w < nwords) f(p, (size_t)w);
  };
  if (t.crc == 2 || t.crc == 3)
    for (size_t c = 0; c < k; ++c) visit(c, t.plan->in[c]);
  const size_t nout = t.crc >= 3 ? t.plan->out.size() : (size_t)t.plan->nstore;
  for (size_t r = 0; r < nout; ++r) visit(k + r, t.plan->out[r]);
}

// Rows of one device launch group: stripes sharing a plan.
struct Group {
  const StripePlan* plan = nullptr;
  std::vector<StripeTask*> tasks;
  std::vector<size_t> at;          // tasks[i] is task at[i] of the part
  std::vector<const uint8_t*> in;  // [tasks * k]
  std::vector<uint8_t*> out;       // [tasks * m]
  std::vector<uint64_t> lens;
  std::vector<uint8_t*> hout;      // plan->dy16: [tasks * (nd + 20)] its output rows
  int flag0 = 0;                   // first flag word
  uint32_t* direct = nullptr;      // or: task i's Verify word is direct[i] (consecutive items' words)
  uint32_t* zero_words = nullptr;  // dy16: the call's checksum words, zeroed by the group's first launch
  uint32_t nzero = 0;
};

// Stripes [t0, t1) of a group: the mixed store/compare product, split into a store and a compare
// launch when the rows exceed one launch.
hipError_t launch_group_run(const Group& g, size_t t0, size_t t1, uint32_t* dflags, hipStream_t s) {
  // one length for the run: no per-stripe lengths, so stripes carved from one pitched buffer run
  // as a single affine launch (any number of stripes) instead of 8-32 per launch
  bool uniform = true;
  for (size_t t = t0; t < t1; ++t) uniform = uniform && g.lens[t] == g.lens[t0];
  const uint64_t* lens = uniform ? nullptr : g.lens.data() + t0;
  uint32_t* flags = g.direct ? g.direct + t0 : dflags + g.flag0 + t0;
  if (const Dy16Plan* d = g.plan->dy16.get()) {
    Dy16RepairJob job;
    job.nd = d->nd;
    job.coef = d->coef.v.data();
    std::memcpy(job.src, d->src, 16);
    job.pstore = d->pstore;
    job.pcmp = d->pcmp;
    if (d->syn) {
      job.syn = true;
      std::memcpy(job.prow, d->prow, 4);
      std::memcpy(job.ainv, d->ainv, 16);
    }
    job.nstripes = (int)(t1 - t0);
    job.in = g.in.data() + t0 * 16;
    job.e = d->e;
    job.out = g.hout.data() + t0 * d->rows.size();
    job.lens = lens;
    job.len = g.lens[t0];
    job.flags = flags;
    if (t0 == 0) {
      job.zero_words = g.zero_words;
      job.nzero = g.nzero;
    }
    return launch_dy16_repair(job, s);
  }
  const size_t nin = g.plan->in.size(), nout = g.plan->out.size();
  MatVecJob job = matvec_job((int)nin, (int)nout, g.plan->rows.v.data(), g.lens[t0], (int)(t1 - t0),
                             g.in.data() + t0 * nin, g.out.data() + t0 * nout);
  job.lens = lens;
  job.flags = flags;
  job.mode = MatVecMode::kStoreVerify;
  job.nstore = g.plan->nstore;
  if (job.m <= kLaunchMaxRows || job.nstore == 0 || job.nstore == job.m) return launch_matvec(job, s);
  // store rows [0, nstore) then compare rows [nstore, m): two jobs over row subsets
  const int k = job.k, m = job.m, ns = job.nstripes, nst = job.nstore;
  std::vector<uint8_t*> o1((size_t)ns * nst), o2((size_t)ns * (m - nst));
  for (int t = 0; t < ns; ++t) {
    for (int r = 0; r < nst; ++r) o1[(size_t)t * nst + r] = job.out[(size_t)t * m + r];
    for (int r = nst; r < m; ++r) o2[(size_t)t * (m - nst) + r - nst] = job.out[(size_t)t * m + r];
  }
  MatVecJob a = job, b = job;
  a.m = nst;
  a.out = o1.data();
  a.mode = MatVecMode::kStore;
  b.m = m - nst;
  b.coef = g.plan->rows.v.data() + (size_t)nst * k;
  b.out = o2.data();
  b.mode = MatVecMode::kVerify;
  hipError_t e = launch_matvec(a, s);
  return e != hipSuccess ? e : launch_matvec(b, s);
}

// Enqueue one group: maximal runs of stripes that sit at one stride from each other (every row)
// launch as affine batches of any size; the rest as pointer tables.
hipError_t launch_group(const Group& g, uint32_t* dflags, hipStream_t s) {
  const size_t mo = g.plan->dy16 ? g.plan->dy16->rows.size() : 0;
  for (const auto& run : split_runs(g.in.data(), g.plan->in.size(), g.out.data(), g.plan->out.size(), g.hout.data(), mo,
                                    g.lens.data(), g.tasks.size())) {
    const hipError_t e = launch_group_run(g, run.first, run.second, dflags, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The stride of a group's checksum words, for the launches that checksum in the product's own pass:
// every task checksums in `mode` and is the only checksummed task of its item (no other task writes
// that item's words), no index remap, one length, task i's words at word(task 0) + i * stride with
// the stride past maxrow (the largest shard index checksummed), all of them within [0, nwords).
// 0 when the group is not laid out so.
int64_t crc_word_stride(const Group& g, int mode, int maxrow, size_t nwords,
                        const std::map<int, int>& tasks_per_owner) {
  const size_t nt = g.tasks.size();
  const int64_t w0 = g.tasks[0]->crc_word;
  int64_t cs = maxrow + 1;  // a single task: any stride that clears its rows
  for (size_t i = 0; i < nt; ++i) {
    const StripeTask* t = g.tasks[i];
    if (t->crc != mode || t->crc_map || g.lens[i] != g.lens[0] || tasks_per_owner.at(t->owner) != 1) return 0;
    if (i == 1) cs = t->crc_word - w0;
    if (i >= 1 && t->crc_word - g.tasks[i - 1]->crc_word != cs) return 0;
  }
  if (cs <= maxrow || w0 < 0 || (size_t)(w0 + cs * (int64_t)nt) > nwords) return 0;
  return cs;
}

// A group whose product is a plain store the fused product + CRC kernels have a route for
// (matvec_crc_route, kernels.hpp, asked for the very job launched here; one length) and whose checksum
// words sit at one stride per task
// (no index remap, no other task of the same bid writing that bid's words) runs as one fused launch:
// the shards are checksummed from the registers the product already holds, instead of a second pass
// that reads every row again (EC12P4 8 x 64 MiB: 130 + 123 us -> ~180 us).  Returns false when the
// group does not qualify (then the product and the separate pass run as before).  The words are
// zeroed by run_device already (the launch skips its own memset).
// A group that compares rows too (nstore < m: Reconstruct + Verify) qualifies when its tasks checksum
// every row (mode 3) and the route takes the kStoreVerify job; its Verify words are routed as
// launch_group_run routes them.  Mode 3 with nothing compared is the mode-2 launch.
bool fused_crc_group(const Group& g, uint32_t* dcrc, size_t nwords, const std::map<int, int>& tasks_per_owner,
                     uint32_t* dflags, hipStream_t s, Status* st) {
  static const bool kOn = [] {  // CFSEC_BATCH_FUSED_CRC=0: the separate pass always (A/B)
    const char* v = std::getenv("CFSEC_BATCH_FUSED_CRC");
    return !(v && v[0] == '0');
  }();
  const StripePlan& p = *g.plan;
  const int k = (int)p.in.size(), m = (int)p.out.size();
  const size_t nt = g.tasks.size();
  const bool sv = p.nstore != m;
  if (!kOn || p.dy16 || m == 0 || nt == 0) return false;
  const uint64_t len = g.lens[0];
  if (len == 0) return false;
  const StripeTask* t0 = g.tasks[0];
  const int mode = t0->crc;  // 2: inputs and outputs, 1: the stored outputs only
  if (mode == 0 || mode == 4) return false;  // mode rule: any checksum mode, the one the tasks share
  if (sv && (mode != 3 || p.nstore == 0)) return false;
  int maxrow = 0;
  for (int c : p.in) maxrow = std::max(maxrow, c);
  for (int o : p.out) maxrow = std::max(maxrow, o);
  const int64_t cs = crc_word_stride(g, mode, maxrow, nwords, tasks_per_owner);
  if (cs == 0 || cs > 256) return false;  // no fused route takes a stride past 256 words (kernels.hpp)
  std::vector<int> slot(k + m);
  for (int c = 0; c < k; ++c) slot[c] = mode >= 2 ? p.in[c] : -1;
  for (int r = 0; r < m; ++r) slot[k + r] = p.out[r];
  MatVecJob job = matvec_job(k, m, p.rows.v.data(), len, (int)nt, g.in.data(), g.out.data());
  if (sv) {
    job.mode = MatVecMode::kStoreVerify;
    job.nstore = p.nstore;
    job.flags = g.direct ? g.direct : dflags + g.flag0;
  }
  // the route of exactly this job (its slots, length and stripe count): a shape only the bit-sliced
  // kernel covers has one with every shard checksummed (mode 2) and the tile counts in range only
  if (!matvec_crc_accepts(job, (int)cs, slot.data())) return false;
  *st = hip_status(launch_matvec_crc(job, dcrc + t0->crc_word, (int)cs, slot.data(), s, false),
                   "launch_matvec_crc(batch)");
  if (std::getenv("CFSEC_TRACE_BATCH"))  // which groups fused, for tests
    std::fprintf(stderr,"cfsec batch: fused crc group k=%d m=%d tasks=%zu len=%llu\n", k, m, nt, (unsigned long long)len);
  return true;
}

// Group tasks by plan (first appearance order) and give each group consecutive flag words from
// *next_flag; row pointers from the part's resolved addresses.
std::vector<Group> make_groups(const Part& part, int* next_flag) {
  std::vector<Group> groups;
  std::map<const StripePlan*, size_t> index;
  for (size_t i = 0; i < part.tasks.size(); ++i) {
    StripeTask* t = part.tasks[i];
    auto it = index.find(t->plan);
    if (it == index.end()) {
      it = index.emplace(t->plan, groups.size()).first;
      groups.emplace_back();
      groups.back().plan = t->plan;
    }
    groups[it->second].tasks.push_back(t);
    groups[it->second].at.push_back(i);
  }
  for (Group& g : groups) {
    const std::vector<int>&in = g.plan->in, &out = g.plan->out;
    const size_t k = in.size(), m = out.size();
    g.flag0 = *next_flag;
    g.in.reserve(g.tasks.size() * k);
    g.out.reserve(g.tasks.size() * m);
    g.lens.reserve(g.tasks.size());
    // dy16 output rows, as positions in the task's rows: rows the kernel neither stores nor compares
    // (inputs; parity not verified) get any pointer the task has (its first input's) -- decided once
    // per plan, not per task
    std::vector<size_t> hrow;
    if (g.plan->dy16)
      for (int idx : g.plan->dy16->rows) {
        const size_t c = std::find(in.begin(), in.end(), idx) - in.begin();
        const size_t o = std::find(out.begin(), out.end(), idx) - out.begin();
        hrow.push_back(c < k ? c : o < m ? k + o : 0);
      }
    g.hout.reserve(g.tasks.size() * hrow.size());
    for (size_t i : g.at) {
      uint8_t* const* rows = part.rows[i];
      g.in.insert(g.in.end(), rows, rows + k);
      g.out.insert(g.out.end(), rows + k, rows + k + m);
      g.lens.push_back(part.tasks[i]->len);
      for (size_t p : hrow) g.hout.push_back(rows[p]);
    }
    *next_flag += (int)g.tasks.size();
  }
  return groups;
}

}  // namespace

std::vector<std::pair<size_t, size_t>> split_runs(const uint8_t* const* in, size_t k, const uint8_t* const* out,
                                                  size_t m, const uint8_t* const* hout, size_t mo,
                                                  const uint64_t* lens, size_t nt) {
  std::vector<std::pair<size_t, size_t>> runs;
  bool uniform = true;
  for (size_t t = 0; t < nt; ++t) uniform = uniform && lens[t] == lens[0];
  if (!uniform || nt < 3) {
    runs.emplace_back(0, nt);
    return runs;
  }
  const auto addr = [](const void* p) { return (int64_t)(uintptr_t)p; };
  const auto stride_ok = [&](size_t t, int64_t d) {  // stripe t+1 = stripe t + d on every row
    for (size_t c = 0; c < k; ++c)
      if (addr(in[(t + 1) * k + c]) - addr(in[t * k + c]) != d) return false;
    for (size_t r = 0; r < m; ++r)
      if (addr(out[(t + 1) * m + r]) - addr(out[t * m + r]) != d) return false;
    for (size_t r = 0; r < mo; ++r)
      if (addr(hout[(t + 1) * mo + r]) - addr(hout[t * mo + r]) != d) return false;
    return true;
  };
  // Runs shorter than kMinRun stripes (separately allocated shards: blobnode's per-vuid buffers)
  // are not launched one by one -- a launch per stripe leaves most of the GPU idle (C5's tasklet
  // with every shard at its own address: 64 launches of 16 workgroups, 1.9 ms) -- but gathered into
  // pointer-table runs, which the launchers split into as many stripes per launch as their argument
  // block holds.
  constexpr size_t kMinRun = 4;
  const auto run_end = [&](size_t t0) {
    size_t t1 = t0 + 1;
    if (t1 < nt) {
      const int64_t d = addr(in[t1 * k]) - addr(in[t0 * k]);
      while (t1 < nt && d != 0 && stride_ok(t1 - 1, d)) ++t1;
    }
    return t1;
  };
  size_t t0 = 0;
  while (t0 < nt) {
    size_t t1 = run_end(t0);
    if (t1 - t0 < kMinRun) {  // extend over the following short runs
      while (t1 < nt) {
        const size_t t2 = run_end(t1);
        if (t2 - t1 >= kMinRun) break;
        t1 = t2;
      }
    }
    runs.emplace_back(t0, t1);
    t0 = t1;
  }
  return runs;
}

size_t pack_chunk(const StripeTask* const* tasks, size_t n, size_t i0, size_t lane_bytes,
                  std::vector<size_t>* offsets) {
  offsets->clear();
  size_t used = 0, i1 = i0;
  for (; i1 < n; ++i1) {
    const size_t sl = align_up(tasks[i1]->len, kSlotAlign);
    const size_t nrows = tasks[i1]->plan->in.size() + tasks[i1]->plan->out.size();
    if (i1 > i0 && used + sl * nrows > lane_bytes) break;
    for (size_t p = 0; p < nrows; ++p, used += sl) offsets->push_back(used);
  }
  return i1;
}

MixPack pack_mix(const StripeTask* const* tasks, uint8_t* const* const* rows, size_t n, size_t max_len, uint8_t* dst,
                 size_t cap) {
  MixPack pk;
  // the sizing pass: which tasks go in, their tiles and rows, one coefficient block per plan
  std::map<const StripePlan*, uint32_t> coef_at;  // plan -> byte offset within the coefficient area
  std::vector<size_t> take;
  size_t nrows = 0, ncoef = 0;
  for (size_t i = 0; i < n; ++i) {
    const StripeTask& t = *tasks[i];
    const StripePlan& p = *t.plan;
    const size_t k = p.in.size(), m = p.out.size();
    const uint64_t tiles = ((uint64_t)t.len + kMixTile - 1) / kMixTile;
    const bool ok = !p.compares() && !p.dy16 && m > 0 && k > 0 && k <= (size_t)kLaunchMaxRows && t.len > 0 &&
                    t.len <= max_len && !t.crc && tiles <= kMixMaxTiles - pk.tiles;
    if (!ok) {
      pk.left.push_back(i);
      continue;
    }
    take.push_back(i);
    pk.tiles += (uint32_t)tiles;
    nrows += k + m;
    if (coef_at.emplace(&p, (uint32_t)ncoef).second) ncoef += align_up(k * m, 16);
  }
  pk.items = (uint32_t)take.size();
  pk.plans = (uint32_t)coef_at.size();
  MixHead h{};
  h.nitems = pk.items;
  h.ntiles = pk.tiles;
  h.nplans = pk.plans;
  h.items_off = (uint32_t)sizeof(MixHead);
  h.rows_off = h.items_off + pk.items * (uint32_t)sizeof(MixItem);
  const size_t map_off = h.rows_off + nrows * 8;
  const size_t coef_off = align_up(map_off + (size_t)pk.tiles * 4, 16);
  pk.bytes = coef_off + ncoef;
  if (pk.bytes > 0xFFFFFFFFu) {  // 32-bit offsets: never with kMixMaxTiles tiles of rows a launch addresses
    pk = MixPack();
    for (size_t i = 0; i < n; ++i) pk.left.push_back(i);
    return pk;
  }
  h.map_off = (uint32_t)map_off;
  h.coef_off = (uint32_t)coef_off;
  h.bytes = (uint32_t)pk.bytes;
  if (!dst || cap < pk.bytes || pk.items == 0) return pk;
  std::memcpy(dst, &h, sizeof h);
  MixItem* item = reinterpret_cast<MixItem*>(dst + h.items_off);
  uint64_t* row = reinterpret_cast<uint64_t*>(dst + h.rows_off);
  uint32_t* tile_item = reinterpret_cast<uint32_t*>(dst + h.map_off);
  uint32_t tile = 0, at = 0;
  for (size_t j = 0; j < take.size(); ++j) {
    const StripeTask& t = *tasks[take[j]];
    const StripePlan& p = *t.plan;
    const uint32_t k = (uint32_t)p.in.size(), m = (uint32_t)p.out.size();
    MixItem& it = item[j];
    it.len = t.len;
    it.k = k;
    it.m = m;
    it.coef = h.coef_off + coef_at[&p];
    it.rows = at;
    it.tile0 = tile;
    it.ntiles = (uint32_t)((t.len + kMixTile - 1) / kMixTile);
    for (uint32_t r = 0; r < k + m; ++r) row[at++] = (uint64_t)(uintptr_t)rows[take[j]][r];
    for (uint32_t q = 0; q < it.ntiles; ++q) tile_item[tile++] = (uint32_t)j;
  }
  std::memset(dst + map_off + (size_t)pk.tiles * 4, 0, coef_off - (map_off + (size_t)pk.tiles * 4));
  for (const auto& kv : coef_at) {
    const size_t sz = kv.first->in.size() * kv.first->out.size();
    uint8_t* c = dst + h.coef_off + kv.second;
    std::memcpy(c, kv.first->rows.v.data(), sz);
    std::memset(c + sz, 0, align_up(sz, 16) - sz);
  }
  return pk;
}

namespace {
// x^(8 * 4096 * 2^q), q < kMixCrcPow: a tile's end to the row's end over whole tiles (MixCrcHead::xpow2)
struct MixCrcPow2 {
  uint32_t v[kMixCrcPow];
  MixCrcPow2() {
    v[0] = crc_xpow(int64_t(8) * kMixTile);
    for (int q = 1; q < kMixCrcPow; ++q) v[q] = crc_mulmod(v[q - 1], v[q - 1]);
  }
};
}  // namespace

MixPack pack_mix_crc(const StripeTask* const* tasks, uint8_t* const* const* rows, size_t n, size_t max_len,
                     size_t nwords, uint64_t tabs, uint64_t crc, const std::map<int, int>* tasks_per_owner,
                     uint8_t* dst, size_t cap) {
  MixPack pk;
  // an item's words have one writer: a task is taken when no other task of its item checksums
  std::map<int, int> counted;
  if (!tasks_per_owner) {
    for (size_t i = 0; i < n; ++i)
      if (tasks[i]->crc) ++counted[tasks[i]->owner];
    tasks_per_owner = &counted;
  }
  // the sizing pass: which tasks go in, their tiles and rows, one coefficient block per plan
  std::map<const StripePlan*, uint32_t> coef_at;  // plan -> byte offset within the coefficient area
  std::vector<size_t> take;
  size_t nrows = 0, ncoef = 0;
  for (size_t i = 0; i < n; ++i) {
    const StripeTask& t = *tasks[i];
    const StripePlan& p = *t.plan;
    const size_t k = p.in.size(), m = p.out.size();
    const uint64_t tiles = ((uint64_t)t.len + kMixTile - 1) / kMixTile;
    bool ok = !p.compares() && !p.dy16 && k > 0 && k <= (size_t)kLaunchMaxRows && t.len > 0 && t.len <= max_len &&
              t.crc == 2 && !t.crc_map && tiles <= kMixMaxTiles - pk.tiles;
    if (ok) {
      const auto owner = tasks_per_owner->find(t.owner);
      ok = owner != tasks_per_owner->end() && owner->second == 1;
    }
    for (size_t r = 0; ok && r < k + m; ++r) {  // every word inside the call's words
      const int64_t w = t.crc_word + (r < k ? p.in[r] : p.out[r - k]);
      ok = w >= 0 && (uint64_t)w < nwords && (uint64_t)w <= 0xFFFFFFFFu;
    }
    if (!ok) {
      pk.left.push_back(i);
      continue;
    }
    take.push_back(i);
    pk.tiles += (uint32_t)tiles;
    nrows += k + m;
    if (coef_at.emplace(&p, (uint32_t)ncoef).second) ncoef += align_up(k * m, 16);
  }
  pk.items = (uint32_t)take.size();
  pk.plans = (uint32_t)coef_at.size();
  MixCrcHead h{};
  h.nitems = pk.items;
  h.ntiles = pk.tiles;
  h.nplans = pk.plans;
  h.tabs = tabs;
  h.crc = crc;
  h.items_off = (uint32_t)sizeof(MixCrcHead);
  const size_t rows_off = h.items_off + (size_t)pk.items * sizeof(MixCrcItem);
  const size_t words_off = rows_off + nrows * 8;
  const size_t map_off = words_off + nrows * 4;
  const size_t coef_off = align_up(map_off + (size_t)pk.tiles * 4, 16);
  pk.bytes = coef_off + ncoef;
  if (pk.bytes > 0xFFFFFFFFu) {  // 32-bit offsets: never with kMixMaxTiles tiles of rows a launch addresses
    pk = MixPack();
    for (size_t i = 0; i < n; ++i) pk.left.push_back(i);
    return pk;
  }
  h.rows_off = (uint32_t)rows_off;
  h.words_off = (uint32_t)words_off;
  h.map_off = (uint32_t)map_off;
  h.coef_off = (uint32_t)coef_off;
  h.bytes = (uint32_t)pk.bytes;
  if (!dst || cap < pk.bytes || pk.items == 0) return pk;
  static const MixCrcPow2 pow2;
  static_assert(kMixTile <= 8192, "CrcPowTables::neg covers one tile of padding");
  const CrcPowTables& pw = crc_pow_tables();
  std::memcpy(h.xpow2, pow2.v, sizeof h.xpow2);
  std::memcpy(dst, &h, sizeof h);
  MixCrcItem* item = reinterpret_cast<MixCrcItem*>(dst + h.items_off);
  uint64_t* row = reinterpret_cast<uint64_t*>(dst + h.rows_off);
  uint32_t* word = reinterpret_cast<uint32_t*>(dst + h.words_off);
  uint32_t* tile_item = reinterpret_cast<uint32_t*>(dst + h.map_off);
  uint32_t tile = 0, at = 0;
  for (size_t j = 0; j < take.size(); ++j) {
    const StripeTask& t = *tasks[take[j]];
    const StripePlan& p = *t.plan;
    const uint32_t k = (uint32_t)p.in.size(), m = (uint32_t)p.out.size();
    MixCrcItem it{};
    it.len = t.len;
    it.k = k;
    it.m = m;
    it.coef = h.coef_off + coef_at[&p];
    it.rows = at;
    it.tile0 = tile;
    it.ntiles = (uint32_t)((t.len + kMixTile - 1) / kMixTile);
    it.fin = crc_shift_ones_of((uint64_t)t.len >> 40 ? crc_xpow((int64_t)(8 * (uint64_t)t.len)) : crc_xpow8((int64_t)t.len));
    it.gend = pw.neg[(uint64_t)it.ntiles * kMixTile - t.len];
    std::memcpy(&item[j], &it, sizeof it);
    for (uint32_t r = 0; r < k + m; ++r, ++at) {
      row[at] = (uint64_t)(uintptr_t)rows[take[j]][r];
      word[at] = (uint32_t)(t.crc_word + (r < k ? p.in[r] : p.out[r - k]));
    }
    for (uint32_t q = 0; q < it.ntiles; ++q) tile_item[tile++] = (uint32_t)j;
  }
  std::memset(dst + map_off + (size_t)pk.tiles * 4, 0, coef_off - (map_off + (size_t)pk.tiles * 4));
  for (const auto& kv : coef_at) {
    const size_t sz = kv.first->in.size() * kv.first->out.size();
    if (sz == 0) continue;  // no output rows: checksums only
    uint8_t* c = dst + h.coef_off + kv.second;
    std::memcpy(c, kv.first->rows.v.data(), sz);
    std::memset(c + sz, 0, align_up(sz, 16) - sz);
  }
  return pk;
}

MixPack pack_mix_sv(const StripeTask* const* tasks, uint8_t* const* const* rows, const uint64_t* flags, size_t n,
                    size_t max_len, size_t nwords, uint64_t tabs, uint64_t crc,
                    const std::map<int, int>* tasks_per_owner, uint8_t* dst, size_t cap) {
  MixPack pk;
  // an item's words have one writer: a task is taken when no other task of its item checksums
  std::map<int, int> counted;
  if (!tasks_per_owner) {
    for (size_t i = 0; i < n; ++i)
      if (tasks[i]->crc) ++counted[tasks[i]->owner];
    tasks_per_owner = &counted;
  }
  // the sizing pass: which tasks go in, their tiles and rows, one coefficient block per plan
  std::map<const StripePlan*, uint32_t> coef_at;  // plan -> byte offset within the coefficient area
  std::vector<size_t> take;
  size_t nrows = 0, ncoef = 0;
  for (size_t i = 0; i < n; ++i) {
    const StripeTask& t = *tasks[i];
    const StripePlan& p = *t.plan;
    const size_t k = p.in.size(), m = p.out.size();
    const uint64_t tiles = ((uint64_t)t.len + kMixTile - 1) / kMixTile;
    bool ok = !p.dy16 && k > 0 && k <= (size_t)kLaunchMaxRows && m > 0 && p.nstore >= 0 && (size_t)p.nstore <= m &&
              t.len > 0 && t.len <= max_len && t.split == 0 && t.crc == 3 && !t.crc_map &&
              tiles <= kMixMaxTiles - pk.tiles;
    if (ok) {
      const auto owner = tasks_per_owner->find(t.owner);
      ok = owner != tasks_per_owner->end() && owner->second == 1;
    }
    for (size_t r = 0; ok && r < k + m; ++r) {  // every word inside the call's words
      const int64_t w = t.crc_word + (r < k ? p.in[r] : p.out[r - k]);
      ok = w >= 0 && (uint64_t)w < nwords && (uint64_t)w <= 0xFFFFFFFFu;
    }
    if (!ok) {
      pk.left.push_back(i);
      continue;
    }
    take.push_back(i);
    pk.tiles += (uint32_t)tiles;
    nrows += k + m;
    if (coef_at.emplace(&p, (uint32_t)ncoef).second) ncoef += align_up(k * m, 16);
  }
  pk.items = (uint32_t)take.size();
  pk.plans = (uint32_t)coef_at.size();
  MixCrcHead h{};
  h.nitems = pk.items;
  h.ntiles = pk.tiles;
  h.nplans = pk.plans;
  h.tabs = tabs;
  h.crc = crc;
  h.items_off = (uint32_t)sizeof(MixCrcHead);
  const size_t rows_off = h.items_off + (size_t)pk.items * sizeof(MixSvItem);
  const size_t words_off = rows_off + nrows * 8;
  const size_t map_off = words_off + nrows * 4;
  const size_t coef_off = align_up(map_off + (size_t)pk.tiles * 4, 16);
  pk.bytes = coef_off + ncoef;
  if (pk.bytes > 0xFFFFFFFFu) {  // 32-bit offsets: never with kMixMaxTiles tiles of rows a launch addresses
    pk = MixPack();
    for (size_t i = 0; i < n; ++i) pk.left.push_back(i);
    return pk;
  }
  h.rows_off = (uint32_t)rows_off;
  h.words_off = (uint32_t)words_off;
  h.map_off = (uint32_t)map_off;
  h.coef_off = (uint32_t)coef_off;
  h.bytes = (uint32_t)pk.bytes;
  if (!dst || cap < pk.bytes || pk.items == 0) return pk;
  static const MixCrcPow2 pow2;
  const CrcPowTables& pw = crc_pow_tables();
  std::memcpy(h.xpow2, pow2.v, sizeof h.xpow2);
  std::memcpy(dst, &h, sizeof h);
  uint8_t* item = dst + h.items_off;
  uint64_t* row = reinterpret_cast<uint64_t*>(dst + h.rows_off);
  uint32_t* word = reinterpret_cast<uint32_t*>(dst + h.words_off);
  uint32_t* tile_item = reinterpret_cast<uint32_t*>(dst + h.map_off);
  uint32_t tile = 0, at = 0;
  for (size_t j = 0; j < take.size(); ++j) {
    const StripeTask& t = *tasks[take[j]];
    const StripePlan& p = *t.plan;
    const uint32_t k = (uint32_t)p.in.size(), m = (uint32_t)p.out.size();
    MixSvItem it{};
    it.len = t.len;
    it.k = k;
    it.m = m;
    it.coef = h.coef_off + coef_at[&p];
    it.rows = at;
    it.tile0 = tile;
    it.ntiles = (uint32_t)((t.len + kMixTile - 1) / kMixTile);
    it.fin = crc_shift_ones_of((uint64_t)t.len >> 40 ? crc_xpow((int64_t)(8 * (uint64_t)t.len)) : crc_xpow8((int64_t)t.len));
    it.gend = pw.neg[(uint64_t)it.ntiles * kMixTile - t.len];
    it.nstore = (uint32_t)p.nstore;
    it.flag = flags ? flags[take[j]] : 0;
    std::memcpy(item + j * sizeof it, &it, sizeof it);
    for (uint32_t r = 0; r < k + m; ++r, ++at) {
      row[at] = (uint64_t)(uintptr_t)rows[take[j]][r];
      word[at] = (uint32_t)(t.crc_word + (r < k ? p.in[r] : p.out[r - k]));
    }
    for (uint32_t q = 0; q < it.ntiles; ++q) tile_item[tile++] = (uint32_t)j;
  }
  std::memset(dst + map_off + (size_t)pk.tiles * 4, 0, coef_off - (map_off + (size_t)pk.tiles * 4));
  for (const auto& kv : coef_at) {
    const size_t sz = kv.first->in.size() * kv.first->out.size();
    uint8_t* c = dst + h.coef_off + kv.second;
    std::memcpy(c, kv.first->rows.v.data(), sz);
    std::memset(c + sz, 0, align_up(sz, 16) - sz);
  }
  return pk;
}

MixPack pack_mix_sv16(const StripeTask* const* tasks, uint8_t* const* const* rows, const uint64_t* flags, size_t n,
                      size_t max_len, size_t nwords, uint64_t tabs, uint64_t crc,
                      const std::map<int, int>* tasks_per_owner, uint8_t* dst, size_t cap) {
  MixPack pk;
  // an item's words have one writer: a task is taken when no other task of its item checksums
  std::map<int, int> counted;
  if (!tasks_per_owner) {
    for (size_t i = 0; i < n; ++i)
      if (tasks[i]->crc) ++counted[tasks[i]->owner];
    tasks_per_owner = &counted;
  }
  // A Dy16Plan output row as a position in the task's rows (plan->in then plan->out), and whether the
  // launch touches it: the missing data rows and the parity / extra rows with a mask bit.  A parity row
  // with neither bit is a stand-in among the inputs (checksummed there) or a row of no plan.
  const auto out_row = [](const StripePlan& p, const Dy16Plan& d, size_t r, size_t* pos) {
    const int idx = d.rows[r];
    const bool used = r < (size_t)d.nd || (((d.pstore | d.pcmp) >> (r - d.nd)) & 1u);
    const size_t o = std::find(p.out.begin(), p.out.end(), idx) - p.out.begin();
    *pos = p.in.size() + o;
    return used && o < p.out.size();
  };
  // the sizing pass: which tasks go in, their tiles and rows, one coefficient block per plan
  std::map<const StripePlan*, uint32_t> coef_at;  // plan -> byte offset within the coefficient area
  std::vector<size_t> take;
  size_t nrows = 0, ncoef = 0;
  for (size_t i = 0; i < n; ++i) {
    const StripeTask& t = *tasks[i];
    const StripePlan& p = *t.plan;
    const Dy16Plan* d = p.dy16.get();
    const uint64_t tiles = ((uint64_t)t.len + kMixTile - 1) / kMixTile;
    bool ok = d && p.in.size() == (size_t)kMixSv16In && d->nd >= 0 && d->nd <= 4 && (d->e == 0 || d->e == 2) &&
              d->rows.size() == (size_t)(d->nd + 20 + d->e) && d->coef.rows == 20 + d->e + d->nd && d->coef.cols == 16 &&
              t.len > 0 && t.len <= max_len && t.split == 0 && t.crc == 3 && !t.crc_map &&
              tiles <= kMixMaxTiles - pk.tiles;
    if (ok) {
      const auto owner = tasks_per_owner->find(t.owner);
      ok = owner != tasks_per_owner->end() && owner->second == 1;
    }
    int miss = 0;
    for (int c = 0; ok && c < 16; ++c) {  // src[] names every input once, the nd missing rows in order
      const int s = d->src[c];
      ok = s < 16 ? s == c - miss : (s - 16 == miss && miss < d->nd && d->rows[miss] == c);
      miss += s >= 16;
    }
    ok = ok && miss == d->nd;
    const auto word_ok = [&](int shard) {  // every word inside the call's words
      const int64_t w = t.crc_word + shard;
      return w >= 0 && (uint64_t)w < nwords && (uint64_t)w < kMixNoWord;
    };
    for (size_t c = 0; ok && c < p.in.size(); ++c) ok = word_ok(p.in[c]);
    for (size_t r = 0; ok && r < d->rows.size(); ++r) {
      size_t pos;
      const bool untouched = r >= (size_t)d->nd && !(((d->pstore | d->pcmp) >> (r - d->nd)) & 1u);
      ok = untouched || (out_row(p, *d, r, &pos) && word_ok(d->rows[r]));  // a touched row is one of plan->out
    }
    if (!ok) {
      pk.left.push_back(i);
      continue;
    }
    take.push_back(i);
    pk.tiles += (uint32_t)tiles;
    nrows += kMixSv16In + d->rows.size();
    if (coef_at.emplace(&p, (uint32_t)ncoef).second) ncoef += align_up(d->coef.v.size(), 16);
  }
  pk.items = (uint32_t)take.size();
  pk.plans = (uint32_t)coef_at.size();
  MixCrcHead h{};
  h.nitems = pk.items;
  h.ntiles = pk.tiles;
  h.nplans = pk.plans;
  h.tabs = tabs;
  h.crc = crc;
  h.items_off = (uint32_t)sizeof(MixCrcHead);
  const size_t rows_off = h.items_off + (size_t)pk.items * sizeof(MixSv16Item);
  const size_t words_off = rows_off + nrows * 8;
  const size_t map_off = words_off + nrows * 4;
  const size_t coef_off = align_up(map_off + (size_t)pk.tiles * 4, 16);
  pk.bytes = coef_off + ncoef;
  if (pk.bytes > 0xFFFFFFFFu) {  // 32-bit offsets: never with kMixMaxTiles tiles of rows a launch addresses
    pk = MixPack();
    for (size_t i = 0; i < n; ++i) pk.left.push_back(i);
    return pk;
  }
  h.rows_off = (uint32_t)rows_off;
  h.words_off = (uint32_t)words_off;
  h.map_off = (uint32_t)map_off;
  h.coef_off = (uint32_t)coef_off;
  h.bytes = (uint32_t)pk.bytes;
  if (!dst || cap < pk.bytes || pk.items == 0) return pk;
  static const MixCrcPow2 pow2;
  const CrcPowTables& pw = crc_pow_tables();
  std::memcpy(h.xpow2, pow2.v, sizeof h.xpow2);
  std::memcpy(dst, &h, sizeof h);
  uint8_t* item = dst + h.items_off;
  uint64_t* row = reinterpret_cast<uint64_t*>(dst + h.rows_off);
  uint32_t* word = reinterpret_cast<uint32_t*>(dst + h.words_off);
  uint32_t* tile_item = reinterpret_cast<uint32_t*>(dst + h.map_off);
  // Slot order (gf_dy16.hip to_slot_order): the plan's inputs come in first-present order -- the
  // present data rows, then the stand-in parities -- and Dy16Plan::src[i] is data row i's place there
  // (16 + j: missing row j); slot i takes input col[i], the j-th stand-in for missing row j.
  const auto slot_cols = [](const Dy16Plan& d, int (&col)[16]) {
    for (int i = 0; i < 16; ++i) col[i] = d.src[i] < 16 ? d.src[i] : (16 - d.nd) + (d.src[i] - 16);
  };
  uint32_t tile = 0, at = 0;
  for (size_t j = 0; j < take.size(); ++j) {
    const StripeTask& t = *tasks[take[j]];
    const StripePlan& p = *t.plan;
    const Dy16Plan& d = *p.dy16;
    MixSv16Item it{};
    it.len = t.len;
    it.flag = flags ? flags[take[j]] : 0;
    it.coef = h.coef_off + coef_at[&p];
    it.rows = at;
    it.tile0 = tile;
    it.ntiles = (uint32_t)((t.len + kMixTile - 1) / kMixTile);
    it.fin = crc_shift_ones_of((uint64_t)t.len >> 40 ? crc_xpow((int64_t)(8 * (uint64_t)t.len)) : crc_xpow8((int64_t)t.len));
    it.gend = pw.neg[(uint64_t)it.ntiles * kMixTile - t.len];
    it.pstore = d.pstore;
    it.pcmp = d.pcmp;
    it.nd = (uint8_t)d.nd;
    it.e = (uint8_t)d.e;
    for (int q = 0; q < d.nd; ++q) it.src[q] = (uint8_t)d.rows[q];
    std::memcpy(item + j * sizeof it, &it, sizeof it);
    int col[16];
    slot_cols(d, col);
    for (int s = 0; s < 16; ++s, ++at) {
      row[at] = (uint64_t)(uintptr_t)rows[take[j]][col[s]];
      word[at] = (uint32_t)(t.crc_word + p.in[col[s]]);
    }
    for (size_t r = 0; r < d.rows.size(); ++r, ++at) {
      size_t pos;
      const bool used = out_row(p, d, r, &pos);
      row[at] = used ? (uint64_t)(uintptr_t)rows[take[j]][pos] : 0;
      word[at] = used ? (uint32_t)(t.crc_word + d.rows[r]) : kMixNoWord;
    }
    for (uint32_t q = 0; q < it.ntiles; ++q) tile_item[tile++] = (uint32_t)j;
  }
  std::memset(dst + map_off + (size_t)pk.tiles * 4, 0, coef_off - (map_off + (size_t)pk.tiles * 4));
  for (const auto& kv : coef_at) {
    const Dy16Plan& d = *kv.first->dy16;
    const size_t sz = d.coef.v.size();
    uint8_t* c = dst + h.coef_off + kv.second;
    std::memcpy(c, d.coef.v.data(), sz);
    int col[16];
    slot_cols(d, col);
    for (int q = 0; q < d.nd; ++q)  // the decode rows' columns in slot order
      for (int s = 0; s < 16; ++s) c[(20 + d.e + q) * 16 + s] = d.coef.at(20 + d.e + q, col[s]);
    std::memset(c + sz, 0, align_up(sz, 16) - sz);
  }
  return pk;
}

void partition_stripes(const uint64_t* bytes, int n, int ndev, int* dev) {
  // Stripe i goes to the device whose share of the byte total holds the midpoint of stripe i's
  // bytes: contiguous, non-decreasing runs whose loads differ by at most one stripe's bytes.
  long double total = 0;
  for (int i = 0; i < n; ++i) total += bytes[i];
  long double acc = 0;
  for (int i = 0; i < n; ++i) {
    const long double mid = acc + (long double)bytes[i] / 2;
    int d = total > 0 ? (int)(mid * ndev / total) : (int)((long double)i * ndev / std::max(n, 1));
    dev[i] = std::max(0, std::min(ndev - 1, d));
    acc += bytes[i];
  }
}

Status RSEngine::set_devices(const int* devices, int n) {
  if (!devices || n <= 0) return CFSEC_ERR_INVALID_ARG;
  // CFSEC_DEVICE_REHEARSAL=1: a repeated ordinal is another context on that device (own thread,
  // streams and staging), so the multi-device split runs on a one-GPU machine
  const char* reh = std::getenv("CFSEC_DEVICE_REHEARSAL");
  const bool rehearsal = reh && *reh && *reh != '0';
  std::vector<DeviceContext*> v;
  for (int i = 0; i < n; ++i) {
    const int slot = rehearsal ? (int)std::count(devices, devices + i, devices[i]) : 0;
    DeviceContext* c = DeviceContext::get(devices[i], slot);
    if (!c) {
      set_last_error("set_devices: device " + std::to_string(devices[i]) + " does not exist");
      return CFSEC_ERR_DEVICE;
    }
    if (std::find(v.begin(), v.end(), c) != v.end()) return CFSEC_ERR_INVALID_ARG;
    v.push_back(c);
  }
  devs_ = std::move(v);
  return CFSEC_OK;
}

Status RSEngine::plan_stripe(const std::vector<bool>& present, bool verify, StripePlan* plan,
                             const ExtraRows* extra, bool data_only) {
  // KRS/reedsolomon.go:1453-1501: the first k present rows in index order, decode matrix from the
  // inversion cache (key: the invalid rows met before the k-th valid one).
  std::vector<int> invalid;
  plan->in.clear();
  for (int row = 0; row < total() && (int)plan->in.size() < k_; ++row) {
    if (present[row]) plan->in.push_back(row);
    else invalid.push_back(row);
  }
  if ((int)plan->in.size() < k_) return CFSEC_ERR_TOO_FEW_SHARDS;
  Matrix dec;
  if (!tree_.get(invalid, &dec)) {
    Matrix sub(k_, k_);
    for (int r = 0; r < k_; ++r)
      for (int c = 0; c < k_; ++c) sub.at(r, c) = mat_.at(plan->in[r], c);
    if (!mat_invert(sub, dec)) return CFSEC_ERR_SINGULAR;
    tree_.put(invalid, dec);
  }
  // Stored rows: missing data = dec rows (:1508-1524); missing parity = parity x data, the same
  // linear map over the k inputs as parity_row x dec (:1537-1550).  Compared rows (Verify,
  // :1287-1301, after the reconstruct): every present parity shard outside the k inputs against
  // parity_row x dec.  That is the whole of Verify: present data shards are always among the k
  // inputs (they come first), so the data after the reconstruct is exactly dec x inputs, and a
  // parity shard that is an input or was just rebuilt equals its row by construction.
  plan->out.clear();
  for (int i = 0; i < k_; ++i)
    if (!present[i]) plan->out.push_back(i);
  if (!data_only)  // ReconstructData leaves the missing parity missing (:1434, 1526-1528)
    for (int i = k_; i < total(); ++i)
      if (!present[i]) plan->out.push_back(i);
  plan->nstore = (int)plan->out.size();
  if (verify)
    for (int i = k_; i < total(); ++i)
      if (present[i] && std::find(plan->in.begin(), plan->in.end(), i) == plan->in.end()) plan->out.push_back(i);
  // extra rows over the data (LRC local parities): compared like the parity rows above
  plan->nextra = verify && extra ? (int)extra->idx.size() : 0;
  for (int j = 0; j < plan->nextra; ++j) plan->out.push_back(extra->idx[j]);
  plan->rows = Matrix((int)plan->out.size(), k_);
  const GF& gf = GF::get();
  for (size_t o = 0; o < plan->out.size(); ++o) {
    const int idx = plan->out[o];
    uint8_t* dst = plan->rows.row((int)o);
    if (idx < k_) {
      std::memcpy(dst, dec.row(idx), k_);
    } else {
      const int xo = (int)o - ((int)plan->out.size() - plan->nextra);  // extra row, or < 0
      const uint8_t* p = xo >= 0 ? extra->rows.row(xo) : parity_.row(idx - k_);
      for (int c = 0; c < k_; ++c) {
        uint8_t v = 0;
        for (int j = 0; j < k_; ++j) v ^= gf.mul(p[j], dec.at(j, c));
        dst[c] = v;
      }
    }
  }
  plan->dy16.reset();
  if (!data_only) plan_dy16(present, dec, plan, plan->nextra ? extra : nullptr);
  return CFSEC_OK;
}

namespace {
// The parity rows of a 16 + 20 code in the form repair_dy16 takes: rows 0..15 one 16x16 dyadic
// block, rows 16..19 4x4 dyadic blocks (KRS buildMatrix(16, 36): gf_dyadic16.hpp).
bool parity_dy16(const Matrix& p) {
  if (p.rows != 20 || p.cols != 16) return false;
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j)
      if (p.at(i, j) != p.at(0, i ^ j)) return false;
  for (int c0 = 0; c0 < 16; c0 += 4)
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j)
        if (p.at(16 + i, c0 + j) != p.at(16, c0 + (i ^ j))) return false;
  return true;
}
}  // namespace

void RSEngine::plan_dy16(const std::vector<bool>& present, const Matrix& dec, StripePlan* plan,
                         const ExtraRows* extra) const {
  plan->dy16.reset();
  static const bool off = std::getenv("CFSEC_NO_DY16_REPAIR") != nullptr;  // A/B switch
  if (off || k_ != 16 || m_ != 20 || !parity_dy16(parity_)) return;
  const int e = extra ? (int)extra->idx.size() : 0;
  if (e != 0 && e != 2) return;  // kernels: 0 or 2 extra rows (EC16P20L2's two local parities)
  auto d = std::make_shared<Dy16Plan>();
  for (int i = 0; i < k_; ++i)
    if (!present[i]) d->rows.push_back(i);
  d->nd = (int)d->rows.size();
  d->e = e;
  // products: 16 per decode row + 117 for the 20 parity rows + 16 per extra row, against 16 per
  // output row
  if (d->nd > 4 || 16 * d->nd + 117 + 16 * e >= 16 * (int)plan->out.size()) return;
  for (int r = 0; r < m_; ++r) d->rows.push_back(k_ + r);
  for (int j = 0; j < e; ++j) d->rows.push_back(extra->idx[j]);
  int slot = 0, j = 0;
  for (int i = 0; i < k_; ++i) d->src[i] = present[i] ? (uint8_t)slot++ : (uint8_t)(16 + j++);
  const int nx0 = (int)plan->out.size() - plan->nextra;
  for (size_t o = 0; o < plan->out.size(); ++o) {
    const int idx = plan->out[o];
    if (idx < k_) continue;
    const int bit = (int)o >= nx0 ? 20 + ((int)o - nx0) : idx - k_;
    (o < (size_t)plan->nstore ? d->pstore : d->pcmp) |= 1u << bit;
  }
  d->coef = Matrix(20 + e + d->nd, 16);
  std::memcpy(d->coef.v.data(), parity_.v.data(), 20 * 16);
  for (int q = 0; q < e; ++q) std::memcpy(d->coef.row(20 + q), extra->rows.row(q), 16);
  for (int q = 0; q < d->nd; ++q) std::memcpy(d->coef.row(20 + e + q), dec.row(d->rows[q]), 16);
  // syndrome form: the inputs past the present data rows are the stand-in parities (first-present
  // order); A[q][j] = parity row prow[q] at missing data column rows[j], invertible exactly when the
  // decode is (block elimination of the 16 x 16 input matrix)
  if (plan->in.size() == 16) {
    bool ok = true;
    Matrix A(d->nd, d->nd), Ai;
    for (int q = 0; q < d->nd && ok; ++q) {
      const int p = plan->in[16 - d->nd + q] - k_;
      ok = p >= 0 && p < 20;
      if (ok) {
        d->prow[q] = (uint8_t)p;
        for (int j = 0; j < d->nd; ++j) A.at(q, j) = parity_.at(p, d->rows[j]);
      }
    }
    if (ok && (d->nd == 0 || mat_invert(A, Ai))) {
      for (int j = 0; j < d->nd; ++j)
        for (int q = 0; q < d->nd; ++q) d->ainv[j * 4 + q] = Ai.at(j, q);
      d->syn = true;
    }
  }
  plan->dy16 = std::move(d);
}

StripePlan whole_stripe_plan(int k, int total, const Matrix& rows, int nstore) {
  StripePlan plan;
  for (int i = 0; i < k; ++i) plan.in.push_back(i);
  for (int i = k; i < total; ++i) plan.out.push_back(i);
  plan.nstore = nstore;
  plan.rows = rows;
  return plan;
}

Status RSEngine::whole_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status, int nstore) {
  if (!stripes || !status || nst < 0) return CFSEC_ERR_INVALID_ARG;
  const StripePlan plan = whole_stripe_plan(k_, total(), parity_, nstore);
  std::vector<StripeTask> tasks;
  for (int s = 0; s < nst; ++s) {
    size_t S = 0;
    status[s] = stripes[s] ? whole_stripe_ok(stripes[s], total(), &S) : CFSEC_ERR_INVALID_ARG;
    if (status[s] == CFSEC_OK && m_ > 0) tasks.push_back(StripeTask{stripes[s], &plan, S, &status[s], 0, 0, s});
  }
  return run_stripes(tasks, mem);
}

Status RSEngine::encode_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status) {
  return whole_stripes(stripes, nst, mem, status, m_);
}

Status RSEngine::encode_crc_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status, uint32_t* crcs) {
  // per stripe Encode, then crc32.ChecksumIEEE of every shard (access/stream_put.go:125-143, 249-253)
  if (nst < 0 || (nst > 0 && (!stripes || !status || !crcs))) return CFSEC_ERR_INVALID_ARG;
  const int n = total();
  std::memset(crcs, 0, sizeof(uint32_t) * (size_t)nst * n);
  CrcOut crc;
  crc.words = crcs;
  crc.n = (size_t)nst * n;
  const StripePlan plan = whole_stripe_plan(k_, n, parity_, m_);
  std::vector<StripeTask> tasks;
  for (int s = 0; s < nst; ++s) {
    size_t S = 0;
    status[s] = stripes[s] ? whole_stripe_ok(stripes[s], n, &S) : CFSEC_ERR_INVALID_ARG;
    if (status[s] != CFSEC_OK) continue;
    tasks.push_back(StripeTask{stripes[s], &plan, S, &status[s], 0, 0, s});
    tasks.back().crc = 2;
    tasks.back().crc_word = (int64_t)s * n;
  }
  // a stripe that failed has no task: its words stay zero
  return run_stripes(tasks, mem, nullptr, &crc, /*mix=*/false, /*mix_crc=*/true);
}

Status RSEngine::stripes_one_by_one(cfsec_shard* const* stripes, int nst, int mem, bool reconstruct, bool verify,
                                   int* status) {
  // More inputs than one compare launch carries (k > kLaunchMaxRows): the single-stripe calls,
  // whose Verify stores into staging and compares there (run(): two_step_verify), stripe by stripe.
  for (int s = 0; s < nst; ++s) {
    Status st = stripes[s] ? CFSEC_OK : CFSEC_ERR_INVALID_ARG;
    if (st == CFSEC_OK && reconstruct) st = this->reconstruct(stripes[s], total(), false, mem, nullptr);
    if (st == CFSEC_OK && verify) {
      bool ok = false;
      st = this->verify(stripes[s], total(), mem, nullptr, &ok);
      if (st == CFSEC_OK && !ok) st = CFSEC_ERR_VERIFY;
    }
    if (st == CFSEC_ERR_DEVICE) return st;
    status[s] = st;
  }
  return CFSEC_OK;
}

Status RSEngine::verify_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status) {
  if (!stripes || !status || nst < 0) return CFSEC_ERR_INVALID_ARG;
  if (k_ > kLaunchMaxRows && m_ > 0) return stripes_one_by_one(stripes, nst, mem, false, true, status);
  return whole_stripes(stripes, nst, mem, status, 0);
}

Status RSEngine::reconstruct_stripes(cfsec_shard* const* stripes, int nst, int mem, bool verify, int* status) {
  if (!stripes || !status || nst < 0) return CFSEC_ERR_INVALID_ARG;
  if (verify && k_ > kLaunchMaxRows && m_ > 0) return stripes_one_by_one(stripes, nst, mem, true, true, status);
  PlanStore store;
  std::vector<StripeTask> tasks;
  plan_reconstruct_tasks(stripes, nst, verify, status, 0, 0, &store, &tasks);
  return run_stripes(tasks, mem);
}

Status RSEngine::repair_crc_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status, uint32_t* crcs) {
  // per stripe Reconstruct, then Verify, and crc32.ChecksumIEEE of every shard as it stands
  // (blobnode/work_shard_recover.go:708-771, 335-342)
  if (nst < 0 || (nst > 0 && (!stripes || !status || !crcs))) return CFSEC_ERR_INVALID_ARG;
  if (k_ > kLaunchMaxRows && m_ > 0) return CFSEC_ERR_NOT_SUPPORTED;  // Verify there is the single-stripe path's
  const int n = total();
  std::memset(crcs, 0, sizeof(uint32_t) * (size_t)nst * n);
  CrcOut crc;
  crc.words = crcs;
  crc.n = (size_t)nst * n;
  crc.every = true;
  PlanStore store;
  std::vector<StripeTask> tasks;
  plan_reconstruct_tasks(stripes, nst, true, status, 0, 0, &store, &tasks);
  for (StripeTask& t : tasks) {  // every row, by the task that reads them all (a split Verify's second pass)
    t.crc = t.split == 2 ? 0 : 3;
    t.crc_word = (int64_t)t.owner * n;
  }
  const Status rc = run_stripes(tasks, mem, nullptr, &crc, /*mix=*/false, /*mix_crc=*/false, /*mix_sv=*/true);
  for (int s = 0; s < nst; ++s)  // a stripe that failed has no checksums
    if (status[s] != CFSEC_OK && status[s] != CFSEC_ERR_VERIFY) std::memset(crcs + (size_t)s * n, 0, sizeof(uint32_t) * n);
  return rc;
}

Status RSEngine::reconstruct_data_stripes(cfsec_shard* const* stripes, int nst, int mem, int* status) {
  if (nst < 0 || (nst > 0 && (!stripes || !status))) return CFSEC_ERR_INVALID_ARG;
  PlanStore store;
  std::vector<StripeTask> tasks;
  plan_reconstruct_tasks(stripes, nst, false, status, 0, 0, &store, &tasks, nullptr, nullptr, /*data_only=*/true);
  return run_stripes(tasks, mem, nullptr, nullptr, /*mix=*/true);
}

Status RSEngine::reconstruct_some_stripes(cfsec_shard* const* stripes, int nst, const uint8_t* required, int mem,
                                          int* status) {
  if (nst < 0 || (nst > 0 && (!stripes || !status || !required))) return CFSEC_ERR_INVALID_ARG;
  PlanStore store;
  std::vector<StripeTask> tasks;
  tasks.reserve((size_t)nst);
  // a stripe's plan: the rows of its pattern's (cached) data-only plan that its mask selects, built
  // once per (pattern, selection) of the call
  std::map<std::pair<const StripePlan*, std::vector<bool>>, const StripePlan*> cuts;
  std::vector<bool> present(total()), last_present, pick, last_pick;
  const StripePlan *base = nullptr, *plan = nullptr;  // of the previous stripe that was planned
  for (int s = 0; s < nst; ++s) {
    status[s] = CFSEC_OK;
    cfsec_shard* sh = stripes[s];
    const uint8_t* req = required + (size_t)s * k_;
    size_t S = 0;
    Status st = sh ? check_shards(sh, total(), true, &S) : CFSEC_ERR_INVALID_ARG;
    if (st != CFSEC_OK) {
      status[s] = st;
      continue;
    }
    int np = 0, dp = 0, missing_required = 0;
    for (int i = 0; i < total(); ++i) {
      present[i] = sh[i].len != 0;
      np += present[i] ? 1 : 0;
      dp += present[i] && i < k_ ? 1 : 0;
      missing_required += !present[i] && i < k_ && req[i] ? 1 : 0;
    }
    if (np == total() || dp == k_ || missing_required == 0) continue;  // KRS/reedsolomon.go:1438-1441
    if (np < k_) {
      status[s] = CFSEC_ERR_TOO_FEW_SHARDS;
      continue;
    }
    // batches mostly repeat one erasure pattern and one mask: the previous stripe's plans come first
    if (!base || present != last_present) {
      base = cached_plan(present, false, false, nullptr, &store, &st, /*data_only=*/true);
      last_present = present;
      plan = nullptr;
      if (!base) {
        status[s] = st;
        continue;
      }
    }
    pick.resize(base->out.size());
    for (size_t o = 0; o < base->out.size(); ++o) pick[o] = req[base->out[o]] != 0;
    if (!plan || pick != last_pick) {
      last_pick = pick;
      const StripePlan*& cut_plan = cuts[{base, pick}];
      if (!cut_plan) {
        StripePlan cut;
        cut.in = base->in;
        for (size_t o = 0; o < base->out.size(); ++o)
          if (pick[o]) cut.out.push_back(base->out[o]);
        cut.nstore = (int)cut.out.size();
        cut.rows = Matrix(cut.nstore, k_);
        for (size_t o = 0, j = 0; o < base->out.size(); ++o)
          if (pick[o]) std::memcpy(cut.rows.row((int)j++), base->rows.row((int)o), k_);
        cut_plan = store.add(cut);
      }
      plan = cut_plan;
    }
    for (int r = 0; r < plan->nstore && st == CFSEC_OK; ++r)
      if (!sh[plan->out[r]].data || sh[plan->out[r]].cap < S) st = CFSEC_ERR_INVALID_ARG;
    for (int c : plan->in)
      if (!sh[c].data) st = CFSEC_ERR_INVALID_ARG;
    if (st != CFSEC_OK) {
      set_last_error("reconstruct batch: stripe " + std::to_string(s) + " has a missing shard with cap < shard size");
      status[s] = st;
      continue;
    }
    for (int r = 0; r < plan->nstore; ++r) sh[plan->out[r]].len = S;
    tasks.push_back(StripeTask{sh, plan, S, &status[s], 0, 0, s});
  }
  return run_stripes(tasks, mem, nullptr, nullptr, /*mix=*/true);
}

void RSEngine::plan_reconstruct_tasks(cfsec_shard* const* stripes, int nst, bool verify, int* status, int phase,
                                      int owner0, PlanStore* store, std::vector<StripeTask>* tasks,
                                      const ExtraRows* extra, const std::vector<bool>* fuse, bool data_only) {
  if (verify) data_only = false;
  StripePlan* vplan = nullptr;  // Verify as an encode-matrix pass (split_verify)
  std::map<const StripePlan*, StripePlan*> store_only;
  tasks->reserve(tasks->size() + (size_t)nst);
  // batches mostly repeat one erasure pattern: the previous stripe's plan is checked first
  std::vector<bool> present(total()), last_present;
  const StripePlan* last_plan = nullptr;
  for (int s = 0; s < nst; ++s) {
    status[s] = CFSEC_OK;
    cfsec_shard* sh = stripes[s];
    size_t S = 0;
    Status st = sh ? check_shards(sh, total(), true, &S) : CFSEC_ERR_INVALID_ARG;
    if (st != CFSEC_OK) {
      status[s] = st;
      continue;
    }
    int np = 0, dp = 0;
    for (int i = 0; i < total(); ++i) {
      present[i] = sh[i].len != 0;
      np += present[i] ? 1 : 0;
      dp += present[i] && i < k_ ? 1 : 0;
    }
    if (np < k_) {
      status[s] = CFSEC_ERR_TOO_FEW_SHARDS;
      continue;
    }
    const bool fx = verify && extra && fuse && (*fuse)[s];
    if (np == total() && (!verify || (m_ == 0 && !fx))) continue;  // Reconstruct of a full stripe is a no-op
    if (data_only && dp == k_) continue;  // no data shard missing (KRS/reedsolomon.go:1434)
    // plans are keyed by the present shards, plus whether the extra rows ride along
    present.push_back(fx);
    if (!last_plan || present != last_present) {
      present.pop_back();
      last_plan = cached_plan(present, fx, verify, fx ? extra : nullptr, store, &st, data_only);
      present.push_back(fx);
      last_present = present;
      if (!last_plan) {
        present.pop_back();
        status[s] = st;
        continue;
      }
    }
    present.pop_back();
    const StripePlan* plan = last_plan;
    for (int r = 0; r < plan->nstore && st == CFSEC_OK; ++r)
      if (!sh[plan->out[r]].data || sh[plan->out[r]].cap < S) st = CFSEC_ERR_INVALID_ARG;
    for (int c : plan->in)
      if (!sh[c].data) st = CFSEC_ERR_INVALID_ARG;
    if (st != CFSEC_OK) {
      set_last_error("reconstruct batch: stripe " + std::to_string(s) + " has a missing shard with cap < shard size");
      status[s] = st;
      continue;
    }
    // KRS/reedsolomon.go:1514-1518: shards[i] = shards[i][0:S]
    for (int r = 0; r < plan->nstore; ++r) sh[plan->out[r]].len = S;
    const StripePlan* use = plan;
    if (split_verify(*plan)) {
      // Verify as a second pass over the whole stripe with the encoding matrix instead of compared
      // rows in the reconstruct pass: the compared rows (parity_row x dec over the k inputs) have
      // no structure, the parity rows over the data do (dyadic kernels)
      StripePlan*& so = store_only[plan];
      if (!so) {
        StripePlan cut = *plan;
        cut.dy16.reset();
        cut.out.resize(cut.nstore);
        cut.rows = Matrix(cut.nstore, k_);
        std::memcpy(cut.rows.v.data(), plan->rows.v.data(), (size_t)cut.nstore * k_);
        so = store->add(cut);
      }
      if (!vplan) vplan = store->add(whole_stripe_plan(k_, total(), parity_, 0));
      use = so;
      StripeTask vt{sh, vplan, S, &status[s], 0, phase + 1, owner0 + s};
      vt.split = 1;
      tasks->push_back(vt);
    }
    if (!use->out.empty()) {
      tasks->push_back(StripeTask{sh, use, S, &status[s], 0, phase, owner0 + s});
      tasks->back().split = use != plan ? 2 : 0;
    }
  }
}

const StripePlan* RSEngine::cached_plan(const std::vector<bool>& present, bool fx, bool verify,
                                        const ExtraRows* extra, PlanStore* store, Status* st, bool data_only) {
  std::vector<bool> key = present;
  key.push_back(fx);
  key.push_back(verify);
  key.push_back(data_only);
  {
    std::lock_guard<std::mutex> l(plan_mu_);
    auto it = plan_cache_.find(key);
    if (it != plan_cache_.end()) return it->second.get();
  }
  std::unique_ptr<StripePlan> p(new StripePlan());
  *st = plan_stripe(present, verify, p.get(), extra, data_only);
  if (*st != CFSEC_OK) return nullptr;
  std::lock_guard<std::mutex> l(plan_mu_);
  auto it = plan_cache_.find(key);  // another caller may have planned it meanwhile
  if (it != plan_cache_.end()) return it->second.get();
  if (plan_cache_.size() < kMaxCachedPlans) return plan_cache_.emplace(std::move(key), std::move(p)).first->second.get();
  return store->add(*p);
}

bool RSEngine::split_verify(const StripePlan& p) const {
  if (!p.compares() || p.nextra > 0) return false;
  static const int mode = [] {
    const char* e = getenv("CFSEC_VERIFY_SPLIT");
    return e ? atoi(e) : -1;
  }();
  if (mode >= 0) return mode != 0;
  return false;
}

Status RSEngine::run_stripes(std::vector<StripeTask>& tasks, int mem, const AsyncOut* async, const CrcOut* crc,
                             bool mix, bool mix_crc, bool mix_sv) {
  if (tasks.empty()) return CFSEC_OK;
  if (devs_.empty()) {
    set_last_error("no HIP device available to the cfsec engine");
    return CFSEC_ERR_DEVICE;
  }
  if (mem != CFSEC_MEM_HOST && mem != CFSEC_MEM_DEVICE) return CFSEC_ERR_INVALID_ARG;
  const int nd = async ? 1 : (int)devs_.size();
  if (mem == CFSEC_MEM_DEVICE && nd == 1) {
    // one device: the batch's memory must live on it (checked on the first stripe; per-stripe
    // pointer queries cost ~1 us each)
    const int d = device_of(tasks[0].shards[tasks[0].plan->in[0]].data);
    if (d != devs_[0]->device()) {
      set_last_error("stripe batch: device memory on device " + std::to_string(d) + ", the handle runs on device " +
                     std::to_string(devs_[0]->device()));
      return CFSEC_ERR_INVALID_ARG;
    }
  } else if (mem == CFSEC_MEM_DEVICE) {
    // device memory runs where it lives
    for (auto& t : tasks) {
      const int d = device_of(t.shards[t.plan->in[0]].data);
      int idx = -1;
      for (int i = 0; i < nd; ++i)
        if (devs_[i]->device() == d) idx = i;
      if (idx < 0) {
        set_last_error("stripe batch: device memory on device " + std::to_string(d) +
                       ", which is not one of the handle's devices");
        return CFSEC_ERR_INVALID_ARG;
      }
      t.dev = idx;
    }
  } else {
    // host memory: contiguous runs of batch items, balanced by the bytes each moves; every task of
    // an item (its phases) on one device, so a later phase reads what an earlier one wrote
    std::map<int, uint64_t> per_owner;
    for (auto& t : tasks) per_owner[t.owner] += uint64_t(t.len) * (t.plan->in.size() + t.plan->out.size());
    std::vector<uint64_t> bytes;
    std::map<int, int> slot;
    for (auto& kv : per_owner) {
      slot[kv.first] = (int)bytes.size();
      bytes.push_back(kv.second);
    }
    std::vector<int> dev(bytes.size());
    partition_stripes(bytes.data(), (int)bytes.size(), nd, dev.data());
    for (auto& t : tasks) t.dev = dev[slot[t.owner]];
  }
  std::vector<std::vector<StripeTask*>> per(nd);
  for (auto& t : tasks) per[t.dev].push_back(&t);
  const bool trace = std::getenv("CFSEC_TRACE_BATCH") != nullptr;  // the split, for tests
  if (trace)
    for (int d = 0; d < nd; ++d) {
      std::set<int> items;
      for (StripeTask* t : per[d]) items.insert(t->owner);
      std::fprintf(stderr, "cfsec batch: device index %d (ordinal %d): %zu tasks, items", d, devs_[d]->device(),
                   per[d].size());
      for (int it : items) std::fprintf(stderr, " %d", it);
      std::fprintf(stderr, "\n");
    }
  std::vector<Status> st(nd, CFSEC_OK);
  std::vector<std::string> err(nd);
  std::vector<std::thread> threads;
  for (int d = 1; d < nd; ++d)
    if (!per[d].empty())
      threads.emplace_back([&, d] {
        st[d] = run_device(per[d], mem, devs_[d], nullptr, crc, mix, mix_crc, mix_sv);
        if (st[d] != CFSEC_OK) err[d] = last_error_cstr();
      });
  if (!per[0].empty())
    st[0] = run_device(per[0], mem, devs_[0], async, crc, mix && !async, mix_crc && !async, mix_sv && !async);
  for (auto& th : threads) th.join();
  for (int d = 1; d < nd; ++d)
    if (st[d] != CFSEC_OK && st[0] == CFSEC_OK) {
      set_last_error(err[d]);
      return st[d];
    }
  return st[0];
}

namespace {

// The length limit of the mixed launch for this call: kMixMaxLen, or CFSEC_MIX_MAX_LEN (read per call,
// so tests force either route; 0 switches the mixed launch off).
size_t mix_max_len() {
  const char* v = std::getenv("CFSEC_MIX_MAX_LEN");
  return v && *v ? (size_t)std::strtoull(v, nullptr, 10) : kMixMaxLen;
}

// One run_device call: its workspace and lanes, what it found out about the tasks, and the flag and
// checksum bookkeeping of the parts launched so far.
struct BatchRun {
  const AsyncOut* async;
  const CrcOut* crc;
  DeviceContext::Workspace* ws = nullptr;
  // asynchronous calls run on the caller's stream (NULL: the legacy default stream); synchronous
  // ones on the workspace's streams, ordered after the legacy default stream for device memory
  hipStream_t lane[2] = {nullptr, nullptr};
  int nlanes = 1;
  size_t lane_bytes = 0, staged_total = 0;
  // which stripes the GPU addresses in place (device memory, or page-locked host memory on every
  // row the product touches) and which go through staging (pageable host memory)
  Part direct;
  std::vector<StripeTask*> staged;
  std::vector<uint8_t*> addr;  // the rows of `direct`
  int nphase = 1, nitems = 0;
  bool checks = false;  // some task compares rows (Verify)
  bool sums = false;    // some task checksums rows
  // checksum words: the caller's device array (asynchronous) or the workspace's, zeroed first (the
  // CRC kernel XOR-accumulates)
  uint32_t* dcrc = nullptr;
  bool zero_first = false;             // the first in-place launch zeroes the words (begin)
  std::map<int, int> tasks_per_owner;  // a bid with several checksummed tasks keeps the separate pass
                                       // (EnableVerify's compare task writes no words: not counted)
  uint32_t* fdirect = nullptr;  // the items' Verify words, where groups may write them directly (begin)
  int next_flag = 0;
  std::vector<std::pair<StripeTask*, int>> flags;  // (task, flag word; -1: written directly)
  int chunk = 0;                                   // staged chunks so far: chunk c runs on lane c % nlanes
  // the mixed-plan launch (ReconstructData batches): tasks of at most mix_len bytes share one launch
  // per part (launch_mixed); 0: every task goes through the launch groups
  DeviceContext* ctx = nullptr;
  size_t mix_len = 0;
  // the same with checksums (put batches of mixed-size blobs): tasks of at most mix_crc_len bytes that
  // checksum every shard share one launch per part (launch_mixed's crc form); 0: the groups
  size_t mix_crc_len = 0;
  // the same with Verify in it (repair tasklets of mixed-size bids): tasks of at most mix_sv_len bytes
  // that store, compare and checksum every shard share one launch per part (launch_mixed's sv form); 0:
  // the groups
  size_t mix_sv_len = 0;
  enum MixKind { kMix, kMixCrc, kMixSv, kMixSv16 };

  Status join(int from, int to) { return lane_wait(ws->ev, lane[from], lane[to]); }
  void classify(const std::vector<StripeTask*>& tasks, int mem);
  void size_lanes();
  Status acquire(DeviceContext* ctx, size_t ntasks);
  Status begin(DeviceContext* ctx, int mem, const std::vector<StripeTask*>& tasks);
  Status run_phase(int ph);
  Status run_staged(const std::vector<StripeTask*>& sph);
  Status launch_part(const Part& part, hipStream_t s, bool fuse_crc);
  Status launch_mixed(const Part& part, hipStream_t s, MixKind kind, Part* rest, bool* split);
  Status checksum(const Part& part, const std::vector<char>& taken, hipStream_t s);
  Status gather(Status st);
  void hand_back(const std::vector<StripeTask*>& tasks);
};

// Sort the tasks into in-place and staged ones, resolving every row's device address once.
void BatchRun::classify(const std::vector<StripeTask*>& tasks, int mem) {
  size_t nrows = 0;
  for (const StripeTask* t : tasks) nrows += t->plan->in.size() + t->plan->out.size();
  addr.resize(nrows);
  uint8_t** rows = addr.data();
  for (StripeTask* t : tasks) {
    sums = sums || (t->crc && crc && crc->words && crc->n);
    nphase = std::max(nphase, t->phase + 1);
    nitems = std::max(nitems, t->owner + 1);
    checks = checks || t->plan->compares();
    if (t->crc) ++tasks_per_owner[t->owner];
    const size_t k = t->plan->in.size(), n = k + t->plan->out.size();
    bool in_place = true;
    for (size_t p = 0; p < n; ++p) {
      uint8_t* data = t->shards[p < k ? t->plan->in[p] : t->plan->out[p - k]].data;
      rows[p] = mem == CFSEC_MEM_HOST ? nullptr : data;
      if (mem == CFSEC_MEM_HOST) in_place = in_place && device_alias(data, &rows[p]);
    }
    (in_place ? direct.tasks : staged).push_back(t);
    if (in_place) direct.rows.push_back(rows);
    rows += n;
  }
}

// Staging lanes: each holds whole stripes, at least the largest one.
void BatchRun::size_lanes() {
  for (const StripeTask* t : staged) {
    const size_t b = align_up(t->len, kSlotAlign) * (t->plan->in.size() + t->plan->out.size());
    lane_bytes = std::max(lane_bytes, b);
    staged_total += b;
  }
  if (!staged.empty()) lane_bytes = std::max(lane_bytes, std::min(kLaneBudget, staged_total));
  // two lanes only for staged chunks (a second phase of in-place stripes follows the first on one
  // stream)
  nlanes = !staged.empty() && (staged_total > lane_bytes || nphase > 1) ? 2 : 1;
}

Status BatchRun::acquire(DeviceContext* ctx, size_t ntasks) {
  const Status st = ctx->acquire(lane_bytes * nlanes, std::max(ntasks, (size_t)nitems), &ws, ntasks,
                                 sums && !async ? crc->n : 0);
  if (st != CFSEC_OK) return st;
  ws->mix_busy[0] = ws->mix_busy[1] = false;  // the workspace's previous call has finished its lanes
  dcrc = !sums ? nullptr : async ? crc->words : ws->dcrc;
  lane[0] = async ? async->stream : ws->stream;
  lane[1] = ws->stream2;
  return CFSEC_OK;
}

// Order the lanes, zero the checksum words and choose where the Verify flags go.
Status BatchRun::begin(DeviceContext* ctx, int mem, const std::vector<StripeTask*>& tasks) {
  Status st = CFSEC_OK;
  if (mem == CFSEC_MEM_DEVICE && !async) st = ctx->order_after_default(ws);
  // Zeroed inline on lane 0: a memset on lane 1 beside the first products, waited for by the first
  // checksum launch, measured slower (C5 +26 instead of +14 us, EC12P4 fused encode + CRC 246
  // instead of 224 us: the cross-stream wait costs more than the 10 KiB fill it hides).  When the
  // first launch is a 16x16-dyadic repair (C5's tasklet) its workgroup (0, 0) zeroes the words and
  // the memset launch goes (zero_first, handed to launch_part).
  // (not in a run that may send a mixed launch with checksums first: that launch XORs into the words
  // and zeroes nothing)
  if (sums && nlanes == 1 && nphase == 1 && !direct.tasks.empty() && !mix_crc_len && !mix_sv_len) {
    const StripeTask* t0 = direct.tasks.front();
    zero_first = t0->plan->dy16 && t0->phase == 0 && crc->n <= 0xFFFFFFFFu;
  }
  if (st == CFSEC_OK && sums && !zero_first)
    st = hip_status(hipMemsetAsync(dcrc, 0, crc->n * 4, lane[0]), "hipMemsetAsync(crc)");
  if (st == CFSEC_OK && nlanes > 1) st = join(0, 1);
  // Verify flags.  A group whose tasks belong to consecutive items writes each mismatch straight
  // into the items' words -- the caller's device array (asynchronous) or the pinned host words,
  // zeroed here first (synchronous) -- so no gather launch follows it (C4 / C5: one tasklet group,
  // -4 us of device time per call).  Other groups use per-task words and the gather.
  // CFSEC_BATCH_DIRECT_FLAGS=0: the gather always (A/B).
  static const bool kDirect = [] {
    const char* v = std::getenv("CFSEC_BATCH_DIRECT_FLAGS");
    return !(v && v[0] == '0');
  }();
  fdirect = checks && kDirect ? (async ? async->flags : ws->hflags_dev) : nullptr;
  if (fdirect && !async)
    for (const StripeTask* t : tasks) ws->hflags[t->owner] = 0;
  return st;
}

// One phase: its in-place tasks as one part on lane 0, then its staged tasks in chunks.  The in-place
// part alone tries the launches that checksum within the product's pass (launch_part's fuse_crc).
Status BatchRun::run_phase(int ph) {
  Status st = CFSEC_OK;
  if (ph > 0 && nlanes > 1) {  // a phase starts after everything of the previous one, on both lanes
    st = join(1, 0);
    if (st == CFSEC_OK) st = join(0, 1);
  }
  Part dph;
  std::vector<StripeTask*> sph;
  for (size_t i = 0; i < direct.tasks.size(); ++i)
    if (direct.tasks[i]->phase == ph) {
      dph.tasks.push_back(direct.tasks[i]);
      dph.rows.push_back(direct.rows[i]);
    }
  for (StripeTask* t : staged)
    if (t->phase == ph) sph.push_back(t);
  if (st == CFSEC_OK && !dph.tasks.empty()) st = launch_part(dph, lane[0], /*fuse_crc=*/true);
  if (st == CFSEC_OK) st = run_staged(sph);
  return st;
}

// Staged stripes: chunks of whole stripes alternating over the two lanes; each lane copies its
// chunk in, runs it and copies the stored rows back while the other lane's chunk moves.
Status BatchRun::run_staged(const std::vector<StripeTask*>& sph) {
  Status st = CFSEC_OK;
  std::vector<size_t> off;
  std::vector<uint8_t*> slot;
  const auto copy = [&](uint8_t* dst, const uint8_t* src, size_t len, hipMemcpyKind kind, hipStream_t s) {
    if (st == CFSEC_OK)
      st = hip_status(hipMemcpyAsync(dst, src, len, kind, s),
                      kind == hipMemcpyHostToDevice ? "hipMemcpyAsync H2D" : "hipMemcpyAsync D2H");
  };
  for (size_t i0 = 0; st == CFSEC_OK && i0 < sph.size(); ++chunk) {
    hipStream_t s = lane[chunk % nlanes];
    uint8_t* base = ws->dbuf + lane_bytes * (chunk % nlanes);
    const size_t i1 = pack_chunk(sph.data(), sph.size(), i0, lane_bytes, &off);
    slot.resize(off.size());
    for (size_t j = 0; j < off.size(); ++j) slot[j] = base + off[j];
    Part part;
    part.tasks.assign(sph.begin() + i0, sph.begin() + i1);
    uint8_t** rows = slot.data();
    for (const StripeTask* t : part.tasks) {  // the inputs and the compared rows go in
      const StripePlan& p = *t->plan;
      const size_t k = p.in.size();
      part.rows.push_back(rows);
      for (size_t c = 0; c < k; ++c) copy(rows[c], t->shards[p.in[c]].data, t->len, hipMemcpyHostToDevice, s);
      for (size_t r = p.nstore; r < p.out.size(); ++r)
        copy(rows[k + r], t->shards[p.out[r]].data, t->len, hipMemcpyHostToDevice, s);
      rows += k + p.out.size();
    }
    if (st == CFSEC_OK) st = launch_part(part, s, /*fuse_crc=*/false);
    for (size_t i = 0; i < part.tasks.size(); ++i) {  // the stored rows come back
      const StripeTask* t = part.tasks[i];
      for (int r = 0; r < t->plan->nstore; ++r)
        copy(t->shards[t->plan->out[r]].data, part.rows[i][t->plan->in.size() + r], t->len, hipMemcpyDeviceToHost, s);
    }
    i0 = i1;
  }
  return st;
}

// Launch one part on stream s: make its groups, route their Verify flags, launch them, record the
// flag words, then checksum the rows no launch checksummed (crc32.ChecksumIEEE, from the device
// addresses the product used; staged rows before their lane is reused).
// fuse_crc: try the launches that checksum within the product's own pass (fused_crc_group) and, for
// the call's first launch, the dy16 repair that zeroes the words itself (zero_first).  On for the in-place part, off for staged chunks, whose rows take the separate pass.
Status BatchRun::launch_part(const Part& whole, hipStream_t s, bool fuse_crc) {
  Status st = CFSEC_OK;
  // ReconstructData batches: the small store-only tasks, two or more, as one mixed launch whatever
  // their plans; the rest (a lone small task too: the fixed-K kernels do that better) in groups.
  // Put batches of mixed-size blobs: the same with the launch that also checksums every shard.
  // Repair tasklets of mixed-size bids: the same with the launch that also compares (Verify).
  Part rest;
  bool split = false;
  if (mix_len) st = launch_mixed(whole, s, kMix, &rest, &split);
  else if (mix_crc_len && sums) st = launch_mixed(whole, s, kMixCrc, &rest, &split);
  else if (mix_sv_len && sums) {
    st = launch_mixed(whole, s, kMixSv, &rest, &split);
    // the 16 + 20 code's bids, which that launch refuses for their dy16 product: a launch of their own
    // (gf_mix_sv16.hip), on the same terms -- two or more, the rest to the groups
    Part rest16;
    bool split16 = false;
    if (st == CFSEC_OK) st = launch_mixed(split ? rest : whole, s, kMixSv16, &rest16, &split16);
    if (split16) {
      rest = std::move(rest16);
      split = true;
    }
  }
  if (st != CFSEC_OK) return st;
  const Part& part = split ? rest : whole;
  std::vector<Group> groups;
  {
    HostTimer gt("      make_groups");
    groups = make_groups(part, &next_flag);
    if (fdirect)
      for (Group& gr : groups) {
        if (!gr.plan->compares()) continue;  // nothing compared
        bool consecutive = true;
        for (size_t i = 1; i < gr.tasks.size() && consecutive; ++i)
          consecutive = gr.tasks[i]->owner == gr.tasks[0]->owner + (int)i;
        if (consecutive) gr.direct = fdirect + gr.tasks[0]->owner;
      }
  }
  fuse_crc = fuse_crc && sums;
  if (fuse_crc && zero_first) {  // make_groups keeps first-appearance order: groups[0] holds direct.front()
    if (!groups.empty() && groups[0].plan->dy16) {
      groups[0].zero_words = dcrc;
      groups[0].nzero = (uint32_t)crc->n;
    } else {
      st = hip_status(hipMemsetAsync(dcrc, 0, crc->n * 4, s), "hipMemsetAsync(crc)");
    }
    zero_first = false;
  }
  std::vector<char> taken(part.tasks.size(), 0);  // tasks whose checksums a launch took
  for (const Group& gr : groups) {
    if (st != CFSEC_OK) break;
    if (fuse_crc && fused_crc_group(gr, dcrc, crc->n, tasks_per_owner, ws->bflags, s, &st)) {
      for (size_t i : gr.at) taken[i] = 1;
      continue;
    }
    if (gr.plan->out.empty()) continue;  // no output rows (an engine without parity shards): checksums only
    {
      HostTimer lt("      launch_group");
      st = hip_status(launch_group(gr, ws->bflags, s), "launch_matvec(batch)");
    }
  }
  for (const Group& gr : groups)
    for (size_t i = 0; i < gr.tasks.size(); ++i) flags.emplace_back(gr.tasks[i], gr.direct ? -1 : gr.flag0 + (int)i);
  if (st == CFSEC_OK) st = checksum(part, taken, s);
  return st;
}

// The tasks of a part the item table takes (pack_mix; kMixCrc: pack_mix_crc, whose launch also
// checksums every row of its items into the call's words; kMixSv: pack_mix_sv, whose launch compares
// rows too; kMixSv16: pack_mix_sv16, the same for the 16 + 20 code's dy16 plans), when there are at least two, as one mixed launch on stream s: the table packed into the
// lane's page-locked buffer, one copy to the device, the launch.  *rest gets the other tasks (*split
// true), which go through the groups and the separate checksum pass as before; with fewer than two
// takers nothing is launched and *split stays false.
// kMixSv, kMixSv16: a taker's Verify word is routed as the groups route theirs -- with fdirect the item's own word
// (recorded as written directly), otherwise a per-task word and the gather.
Status BatchRun::launch_mixed(const Part& part, hipStream_t s, MixKind kind, Part* rest, bool* split) {
  HostTimer mt("      launch_mixed");
  const size_t n = part.tasks.size();
  const uint32_t* tabs = nullptr;
  if (kind != kMix) {
    const Status e = hip_status(crc_device_tables(&tabs), "crc_device_tables");
    if (e != CFSEC_OK) return e;
  }
  const bool sv = kind == kMixSv || kind == kMixSv16;
  std::vector<uint64_t> fword;  // kMixSv, kMixSv16: the address of every taker's Verify word
  const auto pack = [&](uint8_t* dst, size_t cap) {
    if (sv)
      return (kind == kMixSv ? pack_mix_sv : pack_mix_sv16)(
          part.tasks.data(), part.rows.data(), fword.empty() ? nullptr : fword.data(), n, mix_sv_len, crc->n,
          (uint64_t)(uintptr_t)tabs, (uint64_t)(uintptr_t)dcrc, &tasks_per_owner, dst, cap);
    return kind == kMixCrc ? pack_mix_crc(part.tasks.data(), part.rows.data(), n, mix_crc_len, crc->n,
                                          (uint64_t)(uintptr_t)tabs, (uint64_t)(uintptr_t)dcrc, &tasks_per_owner, dst,
                                          cap)
                           : pack_mix(part.tasks.data(), part.rows.data(), n, mix_len, dst, cap);
  };
  const MixPack sz = pack(nullptr, 0);
  if (sz.items < 2) return CFSEC_OK;
  if (sv) {
    std::vector<char> is_left(n, 0);
    for (size_t i : sz.left) is_left[i] = 1;
    fword.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
      if (is_left[i]) continue;
      StripeTask* t = part.tasks[i];
      int w = -1;  // nothing compared: no word; fdirect: the item's own word
      if (t->plan->compares()) {
        if (!fdirect) w = next_flag++;
        fword[i] = (uint64_t)(uintptr_t)(fdirect ? fdirect + t->owner : ws->bflags + w);
      }
      flags.emplace_back(t, w);
    }
  }
  const int slot = nlanes > 1 && s == lane[1] ? 1 : 0;
  Status st = ctx->reserve_mix(ws, slot, sz.bytes, s);
  if (st != CFSEC_OK) return st;
  if (ws->mix_busy[slot]) {  // the lane's previous table is still being copied from
    st = hip_status(hipEventSynchronize(ws->mix_ev[slot]), "hipEventSynchronize(mix table)");
    ws->mix_busy[slot] = false;
    if (st != CFSEC_OK) return st;
  }
  const MixPack pk = pack(ws->hmix[slot], ws->mix_cap[slot]);
  st = hip_status(hipMemcpyAsync(ws->dmix[slot], ws->hmix[slot], pk.bytes, hipMemcpyHostToDevice, s),
                  "hipMemcpyAsync H2D(mix table)");
  if (st == CFSEC_OK) st = hip_status(hipEventRecord(ws->mix_ev[slot], s), "hipEventRecord(mix table)");
  ws->mix_busy[slot] = true;
  if (st == CFSEC_OK)
    st = kind == kMixSv16  ? hip_status(launch_mix_sv16(ws->dmix[slot], pk.tiles, s), "launch_mix_sv16")
         : kind == kMixSv  ? hip_status(launch_mix_sv(ws->dmix[slot], pk.tiles, s), "launch_mix_sv")
         : kind == kMixCrc ? hip_status(launch_mix_crc(ws->dmix[slot], pk.tiles, s), "launch_mix_crc")
                           : hip_status(launch_mix(ws->dmix[slot], pk.tiles, s), "launch_mix");
  const char* tr = std::getenv("CFSEC_TRACE_MATVEC");
  if (tr && tr[0] && tr[0] != '0')
    std::fprintf(stderr, "cfsec: %s items=%u tiles=%u plans=%u\n",
                 kind == kMixSv16 ? "mixsv16" : kind == kMixSv ? "mixsv" : kind == kMixCrc ? "mixcrc" : "mix", pk.items,
                 pk.tiles, pk.plans);
  for (size_t i : pk.left) {
    rest->tasks.push_back(part.tasks[i]);
    rest->rows.push_back(part.rows[i]);
  }
  *split = true;
  return st;
}

// The separate checksum pass over the tasks of a part no launch has taken: one launch per length.
Status BatchRun::checksum(const Part& part, const std::vector<char>& taken, hipStream_t s) {
  if (!sums) return CFSEC_OK;
  std::map<size_t, std::pair<std::vector<const uint8_t*>, std::vector<uint32_t>>> by_len;
  for (size_t i = 0; i < part.tasks.size(); ++i) {
    const StripeTask* t = part.tasks[i];
    if (taken[i] || !t->crc || t->len == 0) continue;
    auto& v = by_len[t->len];
    for_each_crc_row(*t, crc->n, [&](size_t p, size_t w) {
      v.first.push_back(part.rows[i][p]);
      v.second.push_back((uint32_t)w);
    });
  }
  for (auto& kv : by_len) {
    const Status e = hip_status(launch_crc32_to(kv.second.first.data(), kv.first, (int)kv.second.first.size(), dcrc,
                                                kv.second.second.data(), crc32_shift_ones(kv.first), s),
                                "launch_crc32_to(batch)");
    if (e != CFSEC_OK) return e;
  }
  return CFSEC_OK;
}

// After the last phase, on lane 0 behind both lanes: the checksum words to the pinned mirror, and
// the Verify flags per batch item, gathered from the per-task words (which the gather resets): into
// the caller's device array (asynchronous), or straight into the pinned host words (no D2H copy).
Status BatchRun::gather(Status st) {
  if (st == CFSEC_OK && nlanes > 1) st = join(1, 0);
  if (st == CFSEC_OK && sums && !async)
    st = hip_status(hipMemcpyAsync(ws->hcrc, ws->dcrc, crc->n * 4, hipMemcpyDeviceToHost, lane[0]),
                    "hipMemcpyAsync D2H(crc)");
  if (st == CFSEC_OK && checks) {
    std::vector<std::pair<int, int>> pairs;
    for (auto& f : flags)
      if (f.second >= 0 && f.first->plan->compares()) pairs.emplace_back(f.first->owner, f.second);
    std::sort(pairs.begin(), pairs.end());
    std::vector<int> item(pairs.size()), word(pairs.size());
    for (size_t i = 0; i < pairs.size(); ++i) item[i] = pairs[i].first, word[i] = pairs[i].second;
    st = hip_status(launch_flag_gather(ws->bflags, async ? async->flags : ws->hflags_dev, item.data(), word.data(),
                                       (int)pairs.size(), async != nullptr || fdirect != nullptr, lane[0]),
                    "launch_flag_gather");
  }
  if (st != CFSEC_OK) ws->bflags_clean = false;  // some task words may be left set: memset on reuse
  return st;
}

// A synchronous call's results, once its lanes are done: a false Verify into the tasks' statuses,
// the checksum words to the caller.
void BatchRun::hand_back(const std::vector<StripeTask*>& tasks) {
  if (checks)
    for (auto& f : flags)
      if (f.first->plan->compares() && ws->hflags[f.first->owner] != 0 && *f.first->status == CFSEC_OK)
        *f.first->status = CFSEC_ERR_VERIFY;
  if (sums)  // this device's words only (another device of the call fills the rest)
    for (const StripeTask* t : tasks)
      for_each_crc_row(*t, crc->n, [&](size_t, size_t w) { crc->words[w] = ws->hcrc[w]; });
}

}  // namespace

// A batch call on one device: classify the tasks, size the lanes, acquire and zero, run the phases
// (each: the in-place part, then the staged chunks), gather the flags, sync, hand back the results.
Status RSEngine::run_device(std::vector<StripeTask*>& tasks, int mem, DeviceContext* ctx, const AsyncOut* async,
                            const CrcOut* crc, bool mix, bool mix_crc, bool mix_sv) {
  HostTimer whole("  run_device");
  std::unique_ptr<HostTimer> tm(new HostTimer("    classify + acquire"));
  DeviceGuard g(ctx->device());
  if (!g.ok()) return hip_status(hipErrorInvalidDevice, "hipSetDevice");
  BatchRun run{async, crc};
  run.ctx = ctx;
  run.mix_len = mix ? mix_max_len() : 0;
  run.mix_crc_len = mix_crc ? mix_max_len() : 0;
  run.mix_sv_len = mix_sv ? mix_max_len() : 0;
  run.classify(tasks, mem);
  if (async && (!run.staged.empty() || (run.checks && !async->flags))) return CFSEC_ERR_INVALID_ARG;
  run.size_lanes();
  Status st = run.acquire(ctx, tasks.size());
  if (st != CFSEC_OK) return st;
  st = run.begin(ctx, mem, tasks);
  tm.reset(new HostTimer("    group + launch"));
  for (int ph = 0; ph < run.nphase && st == CFSEC_OK; ++ph) st = run.run_phase(ph);
  st = run.gather(st);
  if (async) {
    tm.reset();
    ctx->release_after(run.ws, run.lane[0]);
    return st;
  }
  tm.reset(new HostTimer("    sync"));
  for (int l = 0; l < run.nlanes; ++l) {
    const Status sync = ctx->finish(run.ws, run.lane[l]);
    if (st == CFSEC_OK) st = sync;
  }
  tm.reset();
  if (st == CFSEC_OK) run.hand_back(tasks);
  ctx->release(run.ws);
  return st;
}

}  // namespace cfsec

// ---------------------------------------------------------------- ec.Encoder batches

namespace cfsec {

namespace {
// Synchronous calls return checksums only for the items that succeeded (the reference checksums
// after a successful Encode / repair): the words of a failed item are zeroed.  (Asynchronous calls
// learn a false Verify on the stream; their caller skips the words of flagged items.)
// The repair form (crc->every) keeps the words of a bid whose Verify is false: they are the
// checksums of what is in memory, the survivors' check among them.
void clear_failed_crcs(const CrcOut* crc, const AsyncOut* async, const int* status, int nitems, int n) {
  if (!crc || async) return;
  for (int b = 0; b < nitems; ++b)
    if (status[b] != CFSEC_OK && !(crc->every && status[b] == CFSEC_ERR_VERIFY))
      for (int i = 0; i < n && (size_t)b * n + i < crc->n; ++i) crc->words[(size_t)b * n + i] = 0;
}
}  // namespace

Status ECEncoder::set_devices(const int* devices, int n) { return engine_->set_devices(devices, n); }

Status LrcEncoder::set_devices(const int* devices, int n) {
  Status st = engine_->set_devices(devices, n);
  return st != CFSEC_OK ? st : local_->set_devices(devices, n);
}

Status ECEncoder::reconstruct_batch(cfsec_shard* shards, int n, int nbids, const int* bad, const int* bad_off,
                                    int mem, bool verify, int* status, const AsyncOut* async, const CrcOut* crc,
                                    bool bids) {
  // encoder.go:139-144 per bid (initBadShards, engine Reconstruct), then encoder.go:133-137 (Verify)
  if (!shards || !status || !bad_off || nbids < 0) return CFSEC_ERR_INVALID_ARG;
  Slot slot(pool_.get());
  std::vector<cfsec_shard*> stripes;
  std::vector<int> pos;
  for (int b = 0; b < nbids; ++b) {
    status[b] = CFSEC_OK;
    cfsec_shard* sh = shards + (size_t)b * n;
    if (n != engine_->total()) {
      status[b] = CFSEC_ERR_TOO_FEW_SHARDS;  // reedsolomon.go:1408-1410
      continue;
    }
    const Status st = init_bad_shards(sh, n, std::vector<int>(bad + bad_off[b], bad + bad_off[b + 1]));
    if (st != CFSEC_OK) {
      status[b] = st;
      continue;
    }
    stripes.push_back(sh);
    pos.push_back(b);
  }
  std::vector<int> st(stripes.size());
  Status rc;
  if (verify && engine_->k() > kLaunchMaxRows) {
    // the single-stripe path is synchronous on its own streams: not for the checksummed or the
    // asynchronous forms (no code mode of SURVEY §8 has more than 16 inputs)
    if (crc || async) return CFSEC_ERR_NOT_SUPPORTED;
    rc = engine_->reconstruct_stripes(stripes.data(), (int)stripes.size(), mem, verify, st.data());
  } else {
    PlanStore store;
    std::vector<StripeTask> tasks;
    engine_->plan_reconstruct_tasks(stripes.data(), (int)stripes.size(), verify, st.data(), 0, 0, &store, &tasks);
    stamp_items(tasks, pos, crc, n);
    rc = engine_->run_stripes(tasks, mem, async, crc, /*mix=*/false, /*mix_crc=*/false,
                              /*mix_sv=*/bids && verify && crc && crc->every && !async);
  }
  for (size_t i = 0; i < pos.size(); ++i) status[pos[i]] = st[i];
  clear_failed_crcs(crc, async, status, nbids, n);
  return rc;
}

Status LrcEncoder::reconstruct_batch(cfsec_shard* shards, int n, int nbids, const int* bad, const int* bad_off,
                                     int mem, bool verify, int* status, const AsyncOut* async, const CrcOut* crc,
                                     bool bids) {
  const bool mix_sv = bids && verify && crc && crc->every && !async;
  // lrcencoder.go:133-186 per bid, then lrcencoder.go:89-131 (Verify): a local stripe (n = its size)
  // is the local engine alone; a whole stripe is the global engine over its first N+M shards, then
  // each AZ's local engine over that AZ's local stripe -- planned together and run as two phases of
  // one call (one sync), in that order, as the reference runs them.
  if (!shards || !status || !bad_off || nbids < 0) return CFSEC_ERR_INVALID_ARG;
  HostTimer whole("lrc reconstruct_batch");
  const int N = t_.n, M = t_.m, L = t_.l, AZ = t_.az_count;
  const int lsz = (N + M + L) / AZ;
  if (verify && std::max(N, local_->k()) > kLaunchMaxRows) {
    if (crc || async) return CFSEC_ERR_NOT_SUPPORTED;  // synchronous bid-by-bid path only
    // compared rows over more than one launch's inputs: the single calls, bid by bid (each takes
    // its own concurrency slot)
    for (int b = 0; b < nbids; ++b) {
      cfsec_shard* sh = shards + (size_t)b * n;
      Status st = reconstruct(sh, n, bad + bad_off[b], bad_off[b + 1] - bad_off[b], mem, nullptr);
      if (st == CFSEC_OK) {
        bool ok = false;
        st = this->verify(sh, n, mem, nullptr, &ok);
        if (st == CFSEC_OK && !ok) st = CFSEC_ERR_VERIFY;
      }
      if (st == CFSEC_ERR_DEVICE) return st;
      status[b] = st;
    }
    return CFSEC_OK;
  }
  Slot slot(pool_.get());
  std::unique_ptr<HostTimer> ph(new HostTimer("  init/fill"));
  std::vector<cfsec_shard*> stripes;
  std::vector<int> pos;
  for (int b = 0; b < nbids; ++b) {
    status[b] = CFSEC_OK;
    cfsec_shard* sh = shards + (size_t)b * n;
    if (n != lsz && n != N + M + L) {
      status[b] = CFSEC_ERR_INVALID_SHARDS;
      continue;
    }
    Status st = fill_full_shards(sh, n);
    std::vector<int> global_bad;
    for (int i = bad_off[b]; i < bad_off[b + 1]; ++i)
      if (bad[i] < N + M) global_bad.push_back(bad[i]);
    if (st == CFSEC_OK) st = init_bad_shards(sh, n, global_bad);
    if (st != CFSEC_OK) {
      status[b] = st;
      continue;
    }
    stripes.push_back(sh);
    pos.push_back(b);
  }
  if (n == lsz) {  // local stripes: local engine only (lrcencoder.go:93-99, 147-152)
    std::vector<int> st(stripes.size());
    PlanStore store;
    std::vector<StripeTask> tasks;
    local_->plan_reconstruct_tasks(stripes.data(), (int)stripes.size(), verify, st.data(), 0, 0, &store, &tasks);
    stamp_items(tasks, pos, crc, n);
    const Status rc = local_->run_stripes(tasks, mem, async, crc, /*mix=*/false, /*mix_crc=*/false, mix_sv);
    for (size_t i = 0; i < pos.size(); ++i) status[pos[i]] = st[i];
    clear_failed_crcs(crc, async, status, nbids, n);
    return rc;
  }
  // phase 0 (1): global Reconstruct (+ global Verify) over shards [0, N+M)
  ph.reset(new HostTimer("  global plan"));
  PlanStore gstore, lstore;
  std::vector<StripeTask> tasks;
  std::vector<int> st1(stripes.size());
  // A bid with no bad local shard has its local Verify done in the global pass: every local
  // parity is a fixed row over the data (fused_, as in the fused LRC encode), compared there --
  // the local pass would re-read the 2 x 19 shards of the AZs (C5: 74 -> 38 shard reads per bid).
  ExtraRows extra;
  std::vector<bool> fuse(stripes.size(), false);
  if (verify && L > 0) {
    extra.rows = Matrix(L, N);
    std::memcpy(extra.rows.v.data(), fused_.row(M), (size_t)L * N);
    for (int j = 0; j < L; ++j) extra.idx.push_back(N + M + j);
    for (size_t i = 0; i < stripes.size(); ++i) {
      const cfsec_shard* sh = stripes[i];
      const int b = pos[i];
      bool ok = true;
      for (int j = bad_off[b]; j < bad_off[b + 1]; ++j) ok = ok && bad[j] < N + M;
      size_t S = 0;
      for (int g = 0; g < N + M && !S; ++g) S = sh[g].len;
      for (int j = 0; j < L; ++j) ok = ok && sh[N + M + j].data && sh[N + M + j].len == S && S != 0;
      fuse[i] = ok;
    }
  }
  engine_->plan_reconstruct_tasks(stripes.data(), (int)stripes.size(), verify, st1.data(), 0, 0, &gstore, &tasks,
                                  verify && L > 0 ? &extra : nullptr, &fuse);
  int lphase = 1;
  for (auto& t : tasks) lphase = std::max(lphase, t.phase + 1);
  ph.reset(new HostTimer("  local views + plan"));
  // then every AZ's local stripe (copied headers, lrcencoder.go:236-243) with the rebuilt global
  // shards' lengths already set: local Reconstruct of its bad local shards (index remap
  // lrcencoder.go:161-171) (+ local Verify)
  // per AZ, in bid order: an AZ's views of bids carved from one pitched buffer sit at one stride
  // from each other, so each AZ runs as one affine launch
  // views[a]: AZ a's local stripes of the bids, lsz headers each, back to back
  std::vector<std::vector<cfsec_shard>> views(AZ);
  std::vector<std::vector<size_t>> vowner(AZ);
  std::vector<std::vector<int>> idc(AZ), local_bad(AZ);
  for (int a = 0; a < AZ; ++a) {
    idc[a] = shards_in_idc(a);
    views[a].reserve(stripes.size() * idc[a].size());
    vowner[a].reserve(stripes.size());
  }
  for (size_t i = 0; i < stripes.size(); ++i) {
    if (st1[i] != CFSEC_OK) continue;  // Reconstruct failed: no local pass
    cfsec_shard* sh = stripes[i];
    const int b = pos[i];
    for (auto& v : local_bad) v.clear();
    for (int j = bad_off[b]; j < bad_off[b + 1]; ++j)
      if (bad[j] >= N + M) {
        const int a = (bad[j] - N - M) * AZ / L;
        local_bad[a].push_back(bad[j] - N - M - L / AZ * a + (N + M) / AZ);
      }
    for (int a = 0; a < AZ; ++a) {
      const bool has_bad = !local_bad[a].empty();
      if (!has_bad && (!verify || fuse[i])) continue;  // nothing to rebuild; Verify done (or not asked)
      const size_t at = views[a].size();
      for (int g : idc[a]) views[a].push_back(sh[g]);
      cfsec_shard* ls = views[a].data() + at;
      if (has_bad) {
        const Status s = init_bad_shards(ls, (int)idc[a].size(), local_bad[a]);
        if (s != CFSEC_OK) {
          st1[i] = s;
          views[a].resize(at);
          break;
        }
      }
      vowner[a].push_back(i);
    }
  }
  std::vector<cfsec_shard*> lp;
  std::vector<size_t> owner;
  std::vector<int> vaz;  // the AZ of each local view
  for (int a = 0; a < AZ; ++a)
    for (size_t v = 0; v < vowner[a].size(); ++v) {
      lp.push_back(views[a].data() + v * idc[a].size());
      owner.push_back(vowner[a][v]);
      vaz.push_back(a);
    }
  std::vector<int> st2(lp.size());
  const size_t first_local = tasks.size();
  local_->plan_reconstruct_tasks(lp.data(), (int)lp.size(), verify, st2.data(), lphase, 0, &lstore, &tasks);
  for (size_t t = first_local; t < tasks.size(); ++t) {
    // owner: the bid (a host batch keeps a bid's passes on one device)
    const size_t v = (size_t)(tasks[t].status - st2.data());
    tasks[t].owner = (int)owner[v];
    tasks[t].crc_map = idc[vaz[v]].data();  // local index -> global shard index
  }
  ph.reset();
  // the bid: its device, its verify word; rebuilt shards, global or local
  stamp_items(tasks, pos, crc, n, first_local);
  const Status rc = engine_->run_stripes(tasks, mem, async, crc, /*mix=*/false, /*mix_crc=*/false, mix_sv);
  // per bid: a Reconstruct error (global, then local) wins over a failed Verify
  std::vector<int> local_err(stripes.size(), CFSEC_OK);
  for (size_t v = 0; v < lp.size(); ++v) {
    int& e = local_err[owner[v]];
    if (st2[v] != CFSEC_OK && (e == CFSEC_OK || (e == CFSEC_ERR_VERIFY && st2[v] != CFSEC_ERR_VERIFY))) e = st2[v];
  }
  for (size_t i = 0; i < stripes.size(); ++i) {
    int s = st1[i];
    if (s == CFSEC_OK || s == CFSEC_ERR_VERIFY) {
      if (local_err[i] != CFSEC_OK && local_err[i] != CFSEC_ERR_VERIFY) s = local_err[i];
      else if (s == CFSEC_OK) s = local_err[i];
    }
    status[pos[i]] = s;
  }
  clear_failed_crcs(crc, async, status, nbids, n);
  return rc;
}

Status ECEncoder::reconstruct_data_batch(cfsec_shard* shards, int n, int nitems, const int* bad, const int* bad_off,
                                         int mem, int* status) {
  // encoder.go:146-151 per item (initBadShards, engine ReconstructData), in reconstruct_data's order
  if (!shards || !status || !bad_off || nitems < 0) return CFSEC_ERR_INVALID_ARG;
  Slot slot(pool_.get());
  std::vector<cfsec_shard*> stripes;
  std::vector<int> pos;
  for (int b = 0; b < nitems; ++b) {
    cfsec_shard* sh = shards + (size_t)b * n;
    status[b] = init_bad_shards(sh, n, std::vector<int>(bad + bad_off[b], bad + bad_off[b + 1]));
    if (status[b] == CFSEC_OK && n != engine_->total()) status[b] = CFSEC_ERR_TOO_FEW_SHARDS;  // reedsolomon.go:1408-1410
    if (status[b] != CFSEC_OK) continue;
    stripes.push_back(sh);
    pos.push_back(b);
  }
  std::vector<int> st(stripes.size());
  const Status rc = engine_->reconstruct_data_stripes(stripes.data(), (int)stripes.size(), mem, st.data());
  for (size_t i = 0; i < pos.size(); ++i) status[pos[i]] = st[i];
  return rc;
}

Status LrcEncoder::reconstruct_data_batch(cfsec_shard* shards, int n, int nitems, const int* bad, const int* bad_off,
                                          int mem, int* status) {
  // lrcencoder.go:188-201 per item: fillFullShards over the global stripe, the global bad indices
  // only, the global engine's ReconstructData over shards [0, N+M)
  if (!shards || !status || !bad_off || nitems < 0) return CFSEC_ERR_INVALID_ARG;
  const int N = t_.n, M = t_.m;
  Slot slot(pool_.get());
  std::vector<cfsec_shard*> stripes;
  std::vector<int> pos;
  for (int b = 0; b < nitems; ++b) {
    cfsec_shard* sh = shards + (size_t)b * n;
    if (n < N + M) {
      status[b] = CFSEC_ERR_INVALID_SHARDS;
      continue;
    }
    status[b] = fill_full_shards(sh, N + M);
    std::vector<int> global_bad;
    for (int i = bad_off[b]; i < bad_off[b + 1]; ++i)
      if (bad[i] < N + M) global_bad.push_back(bad[i]);
    if (status[b] == CFSEC_OK) status[b] = init_bad_shards(sh, n, global_bad);
    if (status[b] != CFSEC_OK) continue;
    stripes.push_back(sh);
    pos.push_back(b);
  }
  std::vector<int> st(stripes.size());
  const Status rc = engine_->reconstruct_data_stripes(stripes.data(), (int)stripes.size(), mem, st.data());
  for (size_t i = 0; i < pos.size(); ++i) status[pos[i]] = st[i];
  return rc;
}

Status ECEncoder::encode_batch(cfsec_shard* shards, int n, int nstripes, int mem, int* status,
                               const AsyncOut* async, const CrcOut* crc, bool blobs) {
  // encoder.go:114-131 per stripe: engine Encode, then Verify when EnableVerify -- the Verify pass in
  // the same call (phase 1), after the encode
  if (!shards || !status || nstripes < 0) return CFSEC_ERR_INVALID_ARG;
  Slot slot(pool_.get());
  const int k = engine_->k(), m = engine_->m(), tot = k + m;
  if (enable_verify_ && k > kLaunchMaxRows) {  // compared rows over more inputs than one launch carries
    if (crc || async) return CFSEC_ERR_NOT_SUPPORTED;  // synchronous stripe-by-stripe path only
    std::vector<cfsec_shard*> stripes;
    std::vector<int> pos;
    for (int s = 0; s < nstripes; ++s) {
      status[s] = n != tot ? CFSEC_ERR_TOO_FEW_SHARDS : CFSEC_OK;
      if (n == tot) stripes.push_back(shards + (size_t)s * n), pos.push_back(s);
    }
    std::vector<int> st(stripes.size());
    Status rc = engine_->encode_stripes(stripes.data(), (int)stripes.size(), mem, st.data());
    std::vector<cfsec_shard*> ok;
    std::vector<size_t> okp;
    for (size_t i = 0; i < stripes.size(); ++i)
      if (st[i] == CFSEC_OK) ok.push_back(stripes[i]), okp.push_back(i);
    std::vector<int> vs(ok.size());
    if (rc == CFSEC_OK) rc = engine_->verify_stripes(ok.data(), (int)ok.size(), mem, vs.data());
    for (size_t i = 0; i < ok.size(); ++i) st[okp[i]] = vs[i];
    for (size_t i = 0; i < pos.size(); ++i) status[pos[i]] = st[i];
    return rc;
  }
  const StripePlan plan = whole_stripe_plan(k, tot, engine_->matrix_rows(k, m), m);
  const StripePlan vplan = whole_stripe_plan(k, tot, plan.rows, 0);
  std::vector<StripeTask> tasks;
  for (int s = 0; s < nstripes; ++s) {
    status[s] = CFSEC_OK;
    cfsec_shard* sh = shards + (size_t)s * n;
    if (n != tot) {
      status[s] = CFSEC_ERR_TOO_FEW_SHARDS;  // reedsolomon.go:610-612
      continue;
    }
    size_t S = 0;
    const Status st = whole_stripe_ok(sh, n, &S);
    if (st != CFSEC_OK) {
      status[s] = st;
      continue;
    }
    if (m == 0 && !crc) continue;
    tasks.push_back(StripeTask{sh, &plan, S, &status[s], 0, 0, s});
    tasks.back().crc = crc ? 2 : 0;  // every shard (access/stream_put.go:249-253)
    tasks.back().crc_word = (int64_t)s * n;
    if (enable_verify_ && m > 0) tasks.push_back(StripeTask{sh, &vplan, S, &status[s], 0, 1, s});
  }
  const Status rc = engine_->run_stripes(tasks, mem, async, crc, /*mix=*/false, /*mix_crc=*/blobs && crc && !async);
  clear_failed_crcs(crc, async, status, nstripes, n);
  return rc;
}

Status LrcEncoder::encode_batch(cfsec_shard* shards, int n, int nstripes, int mem, int* status,
                                const AsyncOut* async, const CrcOut* crc, bool blobs) {
  // lrcencoder.go:35-82 per stripe, fused: global parity and every AZ's local parity as one
  // (M+L) x N product over the data (the same rows LrcEncoder::encode launches); EnableVerify
  // compares all M+L rows in a second pass (the reference verifies the global and the local stripes)
  if (!shards || !status || nstripes < 0) return CFSEC_ERR_INVALID_ARG;
  const int N = t_.n, M = t_.m, L = t_.l;
  Slot slot(pool_.get());
  if (enable_verify_ && N > kLaunchMaxRows) {  // the fused Verify's rows exceed one compare launch
    if (crc || async) return CFSEC_ERR_NOT_SUPPORTED;  // synchronous stripe-by-stripe path only
    for (int s = 0; s < nstripes; ++s) {
      status[s] = n != N + M + L ? CFSEC_ERR_INVALID_SHARDS
                                 : encode_stripe(shards + (size_t)s * n, n, mem, async ? async->stream : nullptr);
      if (status[s] == CFSEC_ERR_DEVICE) return status[s];
    }
    return CFSEC_OK;
  }
  const StripePlan plan = whole_stripe_plan(N, N + M + L, fused_, M + L);
  const StripePlan vplan = whole_stripe_plan(N, N + M + L, fused_, 0);
  std::vector<StripeTask> tasks;
  for (int s = 0; s < nstripes; ++s) {
    status[s] = CFSEC_OK;
    cfsec_shard* sh = shards + (size_t)s * n;
    if (n != N + M + L) {
      status[s] = CFSEC_ERR_INVALID_SHARDS;
      continue;
    }
    Status st = fill_full_shards(sh, n);
    size_t S = 0;
    if (st == CFSEC_OK) st = whole_stripe_ok(sh, n, &S);
    if (st == CFSEC_ERR_SHARD_SIZE && check_shards(sh, N + M, false, &S) == CFSEC_OK) {
      // only a local shard has another length: the reference still writes the global parity and
      // the AZs that pass their check -- the single-stripe path restates that sequence
      status[s] = encode_stripe(sh, n, mem, async ? async->stream : nullptr);
      continue;
    }
    if (st != CFSEC_OK) {
      status[s] = st;
      continue;
    }
    tasks.push_back(StripeTask{sh, &plan, S, &status[s], 0, 0, s});
    tasks.back().crc = crc ? 2 : 0;  // every shard, global and local (access/stream_put.go:249-253)
    tasks.back().crc_word = (int64_t)s * n;
  }
  if (enable_verify_) {  // the Verify pass in the same call, after the encode (phase 1)
    const size_t ne = tasks.size();
    for (size_t i = 0; i < ne; ++i) {
      StripeTask v = tasks[i];
      v.plan = &vplan;
      v.phase = 1;
      v.crc = 0;
      tasks.push_back(v);
    }
  }
  const Status rc = engine_->run_stripes(tasks, mem, async, crc, /*mix=*/false, /*mix_crc=*/blobs && crc && !async);
  clear_failed_crcs(crc, async, status, nstripes, n);
  return rc;
}

}  // namespace cfsec
