// capi.cpp -- extern "C" boundary declared in include/cfsec.h.
#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include <cstring>

#include "crc32block_objects.hpp"
#include "engine.hpp"

namespace cfsec {
const char* last_error_cstr();
uint32_t crc_xpow(int64_t e);                   // gf_crc.hip: x^e mod P
uint32_t crc_mulmod(uint32_t a, uint32_t b);  // a * b mod P
}

using cfsec::ECEncoder;
using cfsec::RSEngine;

struct cfsec_rs {
  std::unique_ptr<RSEngine> e;
};
struct cfsec_ec {
  std::unique_ptr<ECEncoder> e;
};

namespace {

hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    cfsec::set_last_error("host allocation failed");
    return CFSEC_ERR_DEVICE;
  } catch (...) {
    cfsec::set_last_error("unexpected C++ exception");
    return CFSEC_ERR_DEVICE;
  }
}

// A bid batch's bad-shard lists: bad_idx[bad_off[b] .. bad_off[b + 1]), offsets from 0 and ascending.
// mismatch (when given): -1 for every bid whose offsets passed.
bool bad_off_valid(int nbids, const int* bad_off, const int* bad_idx, int* mismatch = nullptr) {
  if (nbids > 0 && bad_off[0] != 0) return false;
  for (int b = 0; b < nbids; ++b) {
    if (bad_off[b + 1] < bad_off[b] || (bad_off[b + 1] > bad_off[b] && !bad_idx)) return false;
    if (mismatch) mismatch[b] = -1;
  }
  return true;
}

// The checksum words of a batch call of `items` items of n shards each.
cfsec::CrcOut crc_out(uint32_t* words, int items, int n, bool every = false) {
  return cfsec::CrcOut{words, (size_t)items * n, every};
}

// codemode.go:56-79 (the constCodeModeTactic table), keyed by the CodeMode values of
// codemode.go:26-44.
struct ModeRow {
  int mode;
  cfsec_tactic t;
};
const ModeRow kModes[] = {
    {1, {15, 12, 0, 3, 24, 0, 2048}},   // EC15P12
    {2, {6, 6, 0, 3, 11, 0, 2048}},     // EC6P6
    {3, {16, 20, 2, 2, 34, 0, 2048}},   // EC16P20L2
    {4, {6, 10, 2, 2, 14, 0, 2048}},    // EC6P10L2
    {5, {6, 3, 3, 3, 9, 0, 2048}},      // EC6P3L3
    {6, {6, 6, 0, 3, 11, 0, 0}},        // EC6P6Align0
    {7, {6, 6, 0, 3, 11, 0, 512}},      // EC6P6Align512
    {8, {4, 4, 2, 2, 6, 0, 2048}},      // EC4P4L2
    {9, {12, 4, 0, 1, 15, 0, 2048}},    // EC12P4
    {10, {16, 4, 0, 1, 19, 0, 2048}},   // EC16P4
    {11, {3, 3, 0, 1, 5, 0, 2048}},     // EC3P3
    {12, {10, 4, 0, 1, 13, 0, 2048}},   // EC10P4
    {13, {6, 3, 0, 1, 8, 0, 2048}},     // EC6P3
    {14, {12, 9, 0, 3, 20, 0, 2048}},   // EC12P9
    {200, {6, 6, 9, 3, 11, 0, 2048}},   // EC6P6L9
    {201, {6, 8, 10, 2, 13, 0, 0}},     // EC6P8L10
};

// EncodeSize (common/crc32block/util.go:50-57) for a valid block length.
int64_t crc32block_framed(int64_t size, int64_t block_len) {
  const int64_t p = block_len - 4;
  return size + 4 * ((size + p - 1) / p);
}

// The blocks [b0, b0 + nb) a decode of the payload range [from, to) touches and f1, the framed end
// of the last of them (the whole object for an encode).  from == to touches the block `from` lies
// inside, and none when it sits on a block boundary (see crc32block.hip).
struct BlockRange {
  int64_t b0, nb, f1;
};
BlockRange blocks_touched(bool encode, int64_t size, int64_t block_len, int64_t from, int64_t to) {
  const int64_t P = block_len - 4;
  BlockRange r{0, (size + P - 1) / P, 0};
  if (!encode) {
    r.b0 = from / P;
    const int64_t b1 = from < to ? (to - 1) / P : (from % P ? r.b0 : r.b0 - 1);
    r.nb = b1 - r.b0 + 1;
  }
  r.f1 = std::min(crc32block_framed(size, block_len), (r.b0 + r.nb) * block_len);
  return r;
}

// Decoder.Reader reads the touched blocks through an io.SectionReader: a framed object that ends
// before them is io.ErrUnexpectedEOF there (decode.go:94-97, 126-130), ErrShortData here --
// checked before any copy or launch, so nothing reads past the caller's buffer.
bool decode_source_short(const BlockRange& r, int64_t src_len) {
  if (r.nb <= 0 || src_len >= r.f1) return false;
  cfsec::set_last_error("crc32block decode: framed source shorter than the blocks the range touches");
  return true;
}

// The context of `device` (< 0: the current one), or nullptr.
cfsec::DeviceContext* device_context(int device) {
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return nullptr;
  cfsec::DeviceContext* ctx = cfsec::DeviceContext::get(device);
  if (!ctx) cfsec::set_last_error("no HIP device available to the cfsec engine");
  return ctx;
}

// Encoder.Encode / Decoder.Reader through launch_crc32block: device pointers in place, page-locked
// host buffers in place (device aliases), other host memory staged through the workspace.
int crc32block_call(bool encode, const uint8_t* src, int64_t src_len, int64_t size, int64_t block_len, int64_t from,
                    int64_t to, uint8_t* dst, uint32_t* shard_crc, int64_t* bad_block, int mem, int device,
                    void* stream) {
  if (!cfsec::crc32block_valid_len(block_len)) return CFSEC_ERR_INVALID_BLOCK;
  if (size < 0 || (mem != CFSEC_MEM_HOST && mem != CFSEC_MEM_DEVICE)) return CFSEC_ERR_INVALID_ARG;
  if (!encode && (from < 0 || from > to || to > size)) return CFSEC_ERR_INVALID_ARG;
  if (bad_block) *bad_block = -1;
  if (shard_crc) *shard_crc = 0;  // crc32.ChecksumIEEE(nil)
  const BlockRange r = blocks_touched(encode, size, block_len, from, to);
  if (r.nb <= 0) return CFSEC_OK;
  const int64_t f0 = r.b0 * block_len;
  const int64_t in_bytes = encode ? size : r.f1 - f0;
  const int64_t out_bytes = encode ? r.f1 : to - from;
  if (!src || (!dst && out_bytes > 0)) return CFSEC_ERR_INVALID_ARG;
  if (!encode && decode_source_short(r, src_len)) return CFSEC_ERR_SHORT_DATA;
  return guarded([&] {
    cfsec::DeviceContext* ctx = device_context(device);
    if (!ctx) return (int)CFSEC_ERR_DEVICE;
    // the launch addresses the framed object from its start; what is aliased or staged begins at block b0
    const uint8_t* first = src + (encode ? 0 : f0);
    uint8_t *pi = nullptr, *po = dst;
    bool stage = false;
    if (mem == CFSEC_MEM_HOST) {
      cfsec::DeviceGuard g(ctx->device());
      if (!g.ok()) return cfsec::hip_status(hipErrorInvalidDevice, "hipSetDevice");
      stage = !cfsec::device_alias(const_cast<uint8_t*>(first), &pi) ||
              (out_bytes > 0 && !cfsec::device_alias(dst, &po));
    }
    cfsec::SyncCall call(ctx, stage ? (size_t)(in_bytes + out_bytes) : 0, 2, as_stream(stream), !stream && !stage);
    if (!call.begun()) return call.status();
    cfsec::DeviceContext::Workspace* ws = call.ws();
    hipStream_t s = call.stream();
    if (stage) {
      call.copy(ws->dbuf, first, (size_t)in_bytes, hipMemcpyHostToDevice);
      pi = ws->dbuf;
      po = ws->dbuf + in_bytes;
    }
    const uintptr_t base = reinterpret_cast<uintptr_t>(mem == CFSEC_MEM_HOST ? pi : first);
    const uint8_t* din = reinterpret_cast<const uint8_t*>(base - (uintptr_t)(encode ? 0 : f0));
    uint8_t* dout = po;
    call.memset(ws->dflags, 0xFF, 4);
    call.memset(ws->dflags + 1, 0, 4);
    cfsec::Crc32BlockJob j;
    j.encode = encode;
    j.n = 1;
    j.in = &din;
    j.out = &dout;
    j.size = size;
    j.block_len = block_len;
    j.from = from;
    j.to = to;
    j.bad = ws->dflags;
    j.whole = (encode && shard_crc) ? ws->dflags + 1 : nullptr;
    call.step("launch_crc32block", [&] { return cfsec::launch_crc32block(j, s); });
    if (stage && out_bytes > 0) call.copy(dst, dout, (size_t)out_bytes, hipMemcpyDeviceToHost);
    call.fetch_words(2);
    int st = call.finish();
    if (st == CFSEC_OK) {
      if (encode && shard_crc) *shard_crc = ws->hflags[1];
      if (!encode && ws->hflags[0] != 0xFFFFFFFFu) {
        if (bad_block) *bad_block = r.b0 + (int64_t)ws->hflags[0];
        st = CFSEC_ERR_MISMATCHED_CRC;
      }
    }
    return st;
  });
}

// ---- crc32block over mixed-size objects (crc32block_objects.hpp) ----

// One launch's worth of objects: the ones of a call (or of a staged run of it) that need the device.
struct BlkRun {
  std::vector<cfsec_blk_object> t;  // the objects as the kernel addresses them
  std::vector<size_t> who;          // the caller's index of each
  std::vector<cfsec::BlkSpan> span;
  std::vector<size_t> in_off, out_off;  // staged: offsets in the workspace buffer
  size_t stage_bytes = 0;
  void clear() {
    t.clear(), who.clear(), span.clear(), in_off.clear(), out_off.clear();
    stage_bytes = 0;
  }
};
// Staged host objects share one workspace buffer up to this many bytes per run (a larger object goes alone).
constexpr size_t kBlkStageRun = size_t(64) << 20;

// The round trip of one run on one SyncCall: (staged: the touched bytes in,) the table packed into the
// workspace's page-locked buffer and copied to its device twin, the launch, (staged: the results out,)
// the result words.  o: the caller's objects, read for the staged copies.
int blk_objects_run(cfsec::DeviceContext* ctx, int mode, BlkRun& run, const cfsec_blk_object* o, int64_t block_len,
                    bool stage, void* stream, int* status, int64_t* bad_block, uint32_t* shard_crc) {
  const size_t m = run.t.size();
  const bool encode = mode == cfsec::kBlkEncode;
  cfsec::SyncCall call(ctx, stage ? run.stage_bytes : 0, 2 * m, as_stream(stream), !stream && !stage);
  if (!call.begun()) return call.status();
  cfsec::DeviceContext::Workspace* ws = call.ws();
  hipStream_t s = call.stream();
  if (stage) {
    for (size_t j = 0; j < m; ++j) {
      const cfsec::BlkSpan& sp = run.span[j];
      const cfsec_blk_object& c = o[run.who[j]];
      uint8_t* in = ws->dbuf + run.in_off[j];
      call.copy(in, c.src + (encode ? 0 : sp.f0), (size_t)sp.in_bytes, hipMemcpyHostToDevice);
      // the kernel addresses a framed object from its byte 0; what is staged begins at block b0
      run.t[j].src = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(in) - (uintptr_t)(encode ? 0 : sp.f0));
      if (sp.out_bytes > 0) run.t[j].dst = ws->dbuf + run.out_off[j];
    }
  }
  const cfsec::BlkPack sz = cfsec::pack_blk_objects(mode, run.t.data(), m, block_len, nullptr, 0);
  if (sz.objects != m || sz.taken != m) {
    cfsec::set_last_error("crc32block objects: the plan of a run changed between its two passes");
    call.step("pack_blk_objects", [] { return (cfsec::Status)CFSEC_ERR_DEVICE; });
  }
  call.step("reserve_mix", [&] { return ctx->reserve_mix(ws, 0, sz.bytes, s); });
  if (call.ok() && ws->mix_busy[0]) {  // the previous table is still being copied from
    ws->mix_busy[0] = false;
    call.step("hipEventSynchronize(blk table)", [&] { return hipEventSynchronize(ws->mix_ev[0]); });
  }
  const uint32_t* tabs = nullptr;
  call.step("crc_device_tables", [&] { return cfsec::crc_device_tables(&tabs); });
  if (call.ok()) {
    cfsec::pack_blk_objects(mode, run.t.data(), m, block_len, ws->hmix[0], ws->mix_cap[0]);
    cfsec::BlkHead* head = reinterpret_cast<cfsec::BlkHead*>(ws->hmix[0]);
    head->tabs = (uint64_t)reinterpret_cast<uintptr_t>(tabs);
    head->words = (uint64_t)reinterpret_cast<uintptr_t>(ws->dflags);
  }
  call.memset(ws->dflags, 0xFF, 4 * m);
  call.memset(ws->dflags + m, 0, 4 * m);
  call.step("hipMemcpyAsync H2D(blk table)",
            [&] { return hipMemcpyAsync(ws->dmix[0], ws->hmix[0], sz.bytes, hipMemcpyHostToDevice, s); });
  if (call.step("hipEventRecord(blk table)", [&] { return hipEventRecord(ws->mix_ev[0], s); })) ws->mix_busy[0] = true;
  call.step("launch_crc32block_objects",
            [&] { return cfsec::launch_crc32block_objects(mode, ws->dmix[0], sz.objects, sz.items, s); });
  if (stage)
    for (size_t j = 0; j < m; ++j)
      if (run.span[j].out_bytes > 0)
        call.copy(o[run.who[j]].dst, run.t[j].dst, (size_t)run.span[j].out_bytes, hipMemcpyDeviceToHost);
  call.fetch_words(2 * m);
  const int st = call.finish();
  if (st != CFSEC_OK) return st;
  for (size_t j = 0; j < m; ++j) {
    const size_t i = run.who[j];
    if (ws->hflags[j] != 0xFFFFFFFFu) {
      status[i] = CFSEC_ERR_MISMATCHED_CRC;
      if (bad_block) bad_block[i] = run.span[j].b0 + (int64_t)ws->hflags[j];
    } else if (shard_crc && run.span[j].whole) {
      shard_crc[i] = ws->hflags[m + j];
    }
  }
  return CFSEC_OK;
}

// cfsec_crc32block_{check,decode,encode}_objects: the plan (pack_blk_objects' sizing pass: every object's
// status, the ones to launch), then device pointers and page-locked host objects in place in one run,
// other host memory staged through the workspace in runs of kBlkStageRun bytes.
int crc32block_objects_call(int mode, const cfsec_blk_object* o, int n, int64_t block_len, int* status,
                            int64_t* bad_block, uint32_t* shard_crc, int mem, int device, void* stream) {
  if (!cfsec::crc32block_valid_len(block_len) || block_len > (int64_t(1) << 30)) return CFSEC_ERR_INVALID_BLOCK;
  if (n < 0 || (n > 0 && (!o || !status)) || (mem != CFSEC_MEM_HOST && mem != CFSEC_MEM_DEVICE))
    return CFSEC_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i) {
    status[i] = CFSEC_OK;
    if (bad_block) bad_block[i] = -1;
    if (shard_crc) shard_crc[i] = 0;  // crc32.ChecksumIEEE(nil)
  }
  const bool encode = mode == cfsec::kBlkEncode;
  return guarded([&] {
    cfsec::DeviceContext* ctx = nullptr;
    BlkRun run;
    for (size_t i0 = 0; i0 < (size_t)n;) {
      const cfsec::BlkPack plan = cfsec::pack_blk_objects(mode, o + i0, (size_t)n - i0, block_len, nullptr, 0);
      for (size_t i = 0; i < plan.taken; ++i) status[i0 + i] = plan.status[i];
      if (plan.objects) {
        if (!ctx && !(ctx = device_context(device))) return (int)CFSEC_ERR_DEVICE;
        run.clear();
        for (uint32_t idx : plan.index) {
          run.who.push_back(i0 + idx);
          run.t.push_back(o[i0 + idx]);
          run.span.push_back(cfsec::blk_object_span(mode, o[i0 + idx], block_len));
        }
        bool stage = false;
        if (mem == CFSEC_MEM_HOST) {
          cfsec::DeviceGuard g(ctx->device());
          if (!g.ok()) return (int)cfsec::hip_status(hipErrorInvalidDevice, "hipSetDevice");
          for (size_t j = 0; j < run.t.size() && !stage; ++j) {
            const cfsec::BlkSpan& sp = run.span[j];
            const int64_t f0 = encode ? 0 : sp.f0;
            uint8_t *pi = nullptr, *po = run.t[j].dst;
            stage = !cfsec::device_alias(const_cast<uint8_t*>(run.t[j].src) + f0, &pi) ||
                    (sp.out_bytes > 0 && !cfsec::device_alias(run.t[j].dst, &po));
            run.t[j].src = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(pi) - (uintptr_t)f0);
            run.t[j].dst = po;
          }
        }
        if (!stage) {
          const int st = blk_objects_run(ctx, mode, run, o, block_len, false, stream, status, bad_block, shard_crc);
          if (st != CFSEC_OK) return st;
        } else {
          BlkRun part;
          const auto flush = [&] {
            const int st = part.t.empty() ? (int)CFSEC_OK
                                          : blk_objects_run(ctx, mode, part, o, block_len, true, stream, status,
                                                            bad_block, shard_crc);
            part.clear();
            return st;
          };
          for (size_t j = 0; j < run.t.size(); ++j) {
            const cfsec::BlkSpan& sp = run.span[j];
            const size_t need = cfsec::align_up((size_t)sp.in_bytes, cfsec::kSlotAlign) +
                                cfsec::align_up((size_t)sp.out_bytes, cfsec::kSlotAlign);
            if (!part.t.empty() && part.stage_bytes + need > kBlkStageRun) {
              const int st = flush();
              if (st != CFSEC_OK) return st;
            }
            part.who.push_back(run.who[j]);
            part.t.push_back(o[run.who[j]]);
            part.span.push_back(sp);
            part.in_off.push_back(part.stage_bytes);
            part.out_off.push_back(part.stage_bytes + cfsec::align_up((size_t)sp.in_bytes, cfsec::kSlotAlign));
            part.stage_bytes += need;
          }
          const int st = flush();
          if (st != CFSEC_OK) return st;
        }
      }
      i0 += plan.taken;
    }
    return (int)CFSEC_OK;
  });
}

}  // namespace

extern "C" {

const char* cfsec_version(void) { return "cfsec 0.5.1 (gfx950)"; }

const char* cfsec_last_error(void) { return cfsec::last_error_cstr(); }

const char* cfsec_status_name(int status) {
  switch (status) {
    case CFSEC_OK: return "OK";
    case CFSEC_ERR_TOO_FEW_SHARDS: return "ErrTooFewShards";
    case CFSEC_ERR_SHARD_NO_DATA: return "ErrShardNoData";
    case CFSEC_ERR_SHARD_SIZE: return "ErrShardSize";
    case CFSEC_ERR_INV_SHARD_NUM: return "ErrInvShardNum";
    case CFSEC_ERR_MAX_SHARD_NUM: return "ErrMaxShardNum";
    case CFSEC_ERR_SHORT_DATA: return "ErrShortData";
    case CFSEC_ERR_RECONSTRUCT_REQUIRED: return "ErrReconstructRequired";
    case CFSEC_ERR_SINGULAR: return "errSingular";
    case CFSEC_ERR_INVALID_CODE_MODE: return "ErrInvalidCodeMode";
    case CFSEC_ERR_VERIFY: return "ErrVerify";
    case CFSEC_ERR_INVALID_SHARDS: return "ErrInvalidShards";
    case CFSEC_ERR_INVALID_ARG: return "ErrInvalidArg";
    case CFSEC_ERR_DEVICE: return "ErrDevice";
    case CFSEC_ERR_NOT_SUPPORTED: return "ErrNotSupported";
    case CFSEC_ERR_INVALID_BLOCK: return "ErrInvalidBlock";
    case CFSEC_ERR_MISMATCHED_CRC: return "ErrMismatchedCrc";
    case CFSEC_ERR_INVALID_INPUT: return "ErrInvalidInput";
    default: return "ErrUnknown";
  }
}

int cfsec_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int cfsec_set_sync_poll(int on) { return cfsec::sync_poll_mode().exchange(on ? 1 : 0); }

// ---------------- reedsolomon.Encoder ----------------

int cfsec_rs_new(int data_shards, int parity_shards, int device, cfsec_rs** out) {
  if (!out) return CFSEC_ERR_INVALID_ARG;
  *out = nullptr;
  return guarded([&] {
    std::unique_ptr<RSEngine> e;
    int st = RSEngine::create(data_shards, parity_shards, device, &e);
    if (st != CFSEC_OK) return st;
    *out = new cfsec_rs{std::move(e)};
    return (int)CFSEC_OK;
  });
}

void cfsec_rs_free(cfsec_rs* h) { delete h; }

int cfsec_rs_data_shards(const cfsec_rs* h) { return h ? h->e->k() : -1; }
int cfsec_rs_parity_shards(const cfsec_rs* h) { return h ? h->e->m() : -1; }

int cfsec_rs_matrix(const cfsec_rs* h, uint8_t* out, size_t out_len) {
  if (!h || !out) return CFSEC_ERR_INVALID_ARG;
  const auto& m = h->e->matrix();
  if (out_len < m.v.size()) return CFSEC_ERR_INVALID_ARG;
  std::copy(m.v.begin(), m.v.end(), out);
  return CFSEC_OK;
}

int cfsec_rs_encode(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->encode(shards, n, mem, as_stream(stream)); });
}

int cfsec_rs_verify(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream, int* ok) {
  if (!h || !ok) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    bool b = false;
    int st = h->e->verify(shards, n, mem, as_stream(stream), &b);
    *ok = b ? 1 : 0;
    return st;
  });
}

int cfsec_rs_reconstruct(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->reconstruct(shards, n, false, mem, as_stream(stream)); });
}

int cfsec_rs_reconstruct_data(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->reconstruct(shards, n, true, mem, as_stream(stream)); });
}

int cfsec_rs_encode_idx(cfsec_rs* h, const cfsec_shard* data_shard, int idx, cfsec_shard* parity, int nparity,
                        int mem, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->encode_idx(data_shard, idx, parity, nparity, mem, as_stream(stream)); });
}

int cfsec_rs_update(cfsec_rs* h, cfsec_shard* shards, int n, const cfsec_shard* new_data, int nnew, int mem,
                    void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->update(shards, n, new_data, nnew, mem, as_stream(stream)); });
}

int cfsec_rs_reconstruct_some(cfsec_rs* h, cfsec_shard* shards, int n, const uint8_t* required, int nrequired,
                              int mem, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->reconstruct_some(shards, n, required, nrequired, mem, as_stream(stream)); });
}

int cfsec_rs_split(cfsec_rs* h, uint8_t* data, size_t len, size_t cap, cfsec_shard* out,
                   uint8_t* pad, size_t pad_len, size_t* pad_needed) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->split(data, len, cap, out, pad, pad_len, pad_needed); });
}

int cfsec_rs_join(cfsec_rs* h, uint8_t* dst, size_t dst_len, const cfsec_shard* shards, int n,
                  size_t out_size) {
  if (!h || (!shards && n > 0)) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->join(dst, dst_len, shards, n, out_size); });
}

int cfsec_rs_encode_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                          void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->encode_batch(ptrs, shard_size, nstripes, as_stream(stream)); });
}

int cfsec_rs_update_batch(cfsec_rs* h, uint8_t* const* ptrs, uint8_t* const* new_ptrs, const int* cols, int ncols,
                          size_t shard_size, int nstripes, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded(
      [&] { return h->e->update_batch(ptrs, new_ptrs, cols, ncols, shard_size, nstripes, as_stream(stream)); });
}

int cfsec_rs_verify_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                          uint32_t* flags, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded(
      [&] { return h->e->verify_batch(ptrs, shard_size, nstripes, flags, as_stream(stream)); });
}

int cfsec_rs_reconstruct_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                               const int* erased, int nerased, int data_only, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    return h->e->reconstruct_batch(ptrs, shard_size, nstripes, erased, nerased, data_only != 0,
                                   as_stream(stream));
  });
}

int cfsec_rs_encode_crc(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream, uint32_t* crcs) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->encode_crc(shards, n, mem, as_stream(stream), crcs); });
}

int cfsec_rs_encode_crc_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                              uint32_t* crcs, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->encode_crc_batch(ptrs, shard_size, nstripes, crcs, as_stream(stream)); });
}

int cfsec_rs_reconstruct_crc_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                                   const int* erased, int nerased, int data_only, uint32_t* crcs,
                                   void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    return h->e->reconstruct_crc_batch(ptrs, shard_size, nstripes, erased, nerased, data_only != 0, crcs,
                                       as_stream(stream));
  });
}

int cfsec_rs_repair_crc_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                              const int* erased, int nerased, uint32_t* flags, uint32_t* crcs, void* stream) {
  if (!h || nstripes < 0 || nerased < 0 || (nstripes > 0 && (!ptrs || !flags || !crcs)) || (nerased > 0 && !erased))
    return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    return h->e->repair_crc_batch(ptrs, shard_size, nstripes, erased, nerased, flags, crcs, as_stream(stream));
  });
}

// ---------------- stripe batches ----------------

int cfsec_rs_set_devices(cfsec_rs* h, const int* devices, int ndev) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->set_devices(devices, ndev); });
}

extern "C++" {
namespace {
std::vector<cfsec_shard*> stripe_views(cfsec_shard* shards, int nstripes, int total) {
  std::vector<cfsec_shard*> v((size_t)std::max(nstripes, 0));
  for (int s = 0; s < nstripes; ++s) v[s] = shards + (size_t)s * total;
  return v;
}
}  // namespace
}

int cfsec_batch_partition(const uint64_t* bytes, int n, int ndev, int* dev) {
  if (n < 0 || ndev <= 0 || (n > 0 && (!bytes || !dev))) return CFSEC_ERR_INVALID_ARG;
  cfsec::partition_stripes(bytes, n, ndev, dev);
  return CFSEC_OK;
}

int cfsec_rs_encode_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status) {
  if (!h || nstripes < 0 || (nstripes > 0 && (!shards || !status))) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    auto v = stripe_views(shards, nstripes, h->e->total());
    return h->e->encode_stripes(v.data(), nstripes, mem, status);
  });
}

int cfsec_rs_encode_crc_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status,
                                uint32_t* crcs) {
  if (!h || nstripes < 0 || (nstripes > 0 && (!shards || !status || !crcs))) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    auto v = stripe_views(shards, nstripes, h->e->total());
    return h->e->encode_crc_stripes(v.data(), nstripes, mem, status, crcs);
  });
}

int cfsec_rs_verify_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status) {
  if (!h || nstripes < 0 || (nstripes > 0 && (!shards || !status))) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    auto v = stripe_views(shards, nstripes, h->e->total());
    return h->e->verify_stripes(v.data(), nstripes, mem, status);
  });
}

int cfsec_rs_reconstruct_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int verify, int mem,
                                 int* status) {
  if (!h || nstripes < 0 || (nstripes > 0 && (!shards || !status))) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    auto v = stripe_views(shards, nstripes, h->e->total());
    return h->e->reconstruct_stripes(v.data(), nstripes, mem, verify != 0, status);
  });
}

int cfsec_rs_repair_crc_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status,
                                uint32_t* crcs) {
  if (!h || nstripes < 0 || (nstripes > 0 && (!shards || !status || !crcs))) return CFSEC_ERR_INVALID_ARG;
  if (nstripes == 0) return CFSEC_OK;
  return guarded([&] {
    auto v = stripe_views(shards, nstripes, h->e->total());
    return h->e->repair_crc_stripes(v.data(), nstripes, mem, status, crcs);
  });
}

int cfsec_rs_reconstruct_some_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, const uint8_t* required, int mem,
                                      int* status) {
  if (!h || nstripes < 0 || (nstripes > 0 && (!shards || !status || !required))) return CFSEC_ERR_INVALID_ARG;
  if (nstripes == 0) return CFSEC_OK;
  return guarded([&] {
    auto v = stripe_views(shards, nstripes, h->e->total());
    return h->e->reconstruct_some_stripes(v.data(), nstripes, required, mem, status);
  });
}

int cfsec_rs_reconstruct_data_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status) {
  if (!h || nstripes < 0 || (nstripes > 0 && (!shards || !status))) return CFSEC_ERR_INVALID_ARG;
  if (nstripes == 0) return CFSEC_OK;
  return guarded([&] {
    auto v = stripe_views(shards, nstripes, h->e->total());
    return h->e->reconstruct_data_stripes(v.data(), nstripes, mem, status);
  });
}

// ---------------- ec.Encoder ----------------

int cfsec_codemode_tactic(int codemode, cfsec_tactic* t) {
  if (!t) return CFSEC_ERR_INVALID_ARG;
  for (const auto& r : kModes)
    if (r.mode == codemode) {
      *t = r.t;
      return CFSEC_OK;
    }
  return CFSEC_ERR_INVALID_CODE_MODE;
}

int cfsec_ec_new(const cfsec_tactic* tactic, int enable_verify, int concurrency, int device,
                 cfsec_ec** out) {
  if (!out) return CFSEC_ERR_INVALID_ARG;
  *out = nullptr;
  if (!tactic) return CFSEC_ERR_INVALID_CODE_MODE;
  return guarded([&] {
    std::unique_ptr<ECEncoder> e;
    int st = ECEncoder::create(*tactic, enable_verify != 0, concurrency, device, &e);
    if (st != CFSEC_OK) return st;
    *out = new cfsec_ec{std::move(e)};
    return (int)CFSEC_OK;
  });
}

void cfsec_ec_free(cfsec_ec* h) { delete h; }

int cfsec_ec_encode(cfsec_ec* h, cfsec_shard* shards, int n, int mem, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->encode(shards, n, mem, as_stream(stream)); });
}

int cfsec_ec_reconstruct(cfsec_ec* h, cfsec_shard* shards, int n, const int* bad_idx, int nbad,
                         int mem, void* stream) {
  if (!h || (nbad > 0 && !bad_idx) || nbad < 0) return CFSEC_ERR_INVALID_ARG;
  return guarded(
      [&] { return h->e->reconstruct(shards, n, bad_idx, nbad, mem, as_stream(stream)); });
}

int cfsec_ec_reconstruct_data(cfsec_ec* h, cfsec_shard* shards, int n, const int* bad_idx,
                              int nbad, int mem, void* stream) {
  if (!h || (nbad > 0 && !bad_idx) || nbad < 0) return CFSEC_ERR_INVALID_ARG;
  return guarded(
      [&] { return h->e->reconstruct_data(shards, n, bad_idx, nbad, mem, as_stream(stream)); });
}

int cfsec_ec_verify(cfsec_ec* h, cfsec_shard* shards, int n, int mem, void* stream, int* ok) {
  if (!h || !ok) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    bool b = false;
    int st = h->e->verify(shards, n, mem, as_stream(stream), &b);
    *ok = b ? 1 : 0;
    return st;
  });
}

int cfsec_ec_set_devices(cfsec_ec* h, const int* devices, int ndev) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->set_devices(devices, ndev); });
}

int cfsec_ec_reconstruct_batch(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                               const int* bad_off, int verify, int mem, int* status) {
  if (!h || nbids < 0 || n <= 0 || (nbids > 0 && (!shards || !status || !bad_off))) return CFSEC_ERR_INVALID_ARG;
  if (!bad_off_valid(nbids, bad_off, bad_idx)) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->reconstruct_batch(shards, n, nbids, bad_idx, bad_off, mem, verify != 0, status); });
}

int cfsec_ec_reconstruct_data_batch(cfsec_ec* h, cfsec_shard* shards, int n, int nitems, const int* bad_idx,
                                    const int* bad_off, int mem, int* status) {
  if (!h || nitems < 0) return CFSEC_ERR_INVALID_ARG;
  if (nitems == 0) return CFSEC_OK;
  if (n <= 0 || !shards || !status || !bad_off || !bad_off_valid(nitems, bad_off, bad_idx)) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->reconstruct_data_batch(shards, n, nitems, bad_idx, bad_off, mem, status); });
}

int cfsec_ec_encode_batch(cfsec_ec* h, cfsec_shard* shards, int n, int nstripes, int mem, int* status) {
  if (!h || nstripes < 0 || n <= 0 || (nstripes > 0 && (!shards || !status))) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->encode_batch(shards, n, nstripes, mem, status); });
}

int cfsec_ec_reconstruct_batch_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                                   const int* bad_off, int verify, int mem, int* status, uint32_t* crcs) {
  if (!h || nbids < 0 || n <= 0 || (nbids > 0 && (!shards || !status || !bad_off || !crcs)))
    return CFSEC_ERR_INVALID_ARG;
  if (!bad_off_valid(nbids, bad_off, bad_idx)) return CFSEC_ERR_INVALID_ARG;
  std::memset(crcs, 0, sizeof(uint32_t) * (size_t)nbids * n);
  const cfsec::CrcOut c = crc_out(crcs, nbids, n);
  return guarded([&] {
    return h->e->reconstruct_batch(shards, n, nbids, bad_idx, bad_off, mem, verify != 0, status, nullptr, &c);
  });
}

extern "C++" {
namespace {
// cfsec_ec_repair_batch_crc and, with bids, cfsec_ec_repair_bids_crc: one contract, two sets of launches
int repair_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx, const int* bad_off, int mem,
               int* status, uint32_t* crcs, const uint32_t* expect, int* mismatch, bool bids) {
  if (!h || nbids < 0 || n <= 0 || (nbids > 0 && (!shards || !status || !bad_off || !crcs)) || (expect && !mismatch))
    return CFSEC_ERR_INVALID_ARG;
  if (!bad_off_valid(nbids, bad_off, bad_idx, mismatch)) return CFSEC_ERR_INVALID_ARG;
  std::memset(crcs, 0, sizeof(uint32_t) * (size_t)nbids * n);
  const cfsec::CrcOut c = crc_out(crcs, nbids, n, true);
  const int rc = guarded([&] {
    return h->e->reconstruct_batch(shards, n, nbids, bad_idx, bad_off, mem, true, status, nullptr, &c, bids);
  });
  if (rc != CFSEC_OK || !expect) return rc;
  // downloadShard's check (work_shard_recover.go:654-685) on the words that came back: host arithmetic
  for (int b = 0; b < nbids; ++b) {
    if (status[b] != CFSEC_OK && status[b] != CFSEC_ERR_VERIFY) continue;
    for (int i = 0; i < n && mismatch[b] < 0; ++i) {
      bool bad = false;
      for (int j = bad_off[b]; j < bad_off[b + 1]; ++j) bad = bad || bad_idx[j] == i;
      if (!bad && crcs[(size_t)b * n + i] != expect[(size_t)b * n + i]) mismatch[b] = i;
    }
  }
  return rc;
}
}  // namespace
}

int cfsec_ec_repair_batch_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                              const int* bad_off, int mem, int* status, uint32_t* crcs, const uint32_t* expect,
                              int* mismatch) {
  return repair_crc(h, shards, n, nbids, bad_idx, bad_off, mem, status, crcs, expect, mismatch, /*bids=*/false);
}

int cfsec_ec_repair_bids_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                             const int* bad_off, int mem, int* status, uint32_t* crcs, const uint32_t* expect,
                             int* mismatch) {
  return repair_crc(h, shards, n, nbids, bad_idx, bad_off, mem, status, crcs, expect, mismatch, /*bids=*/true);
}

int cfsec_ec_encode_batch_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nstripes, int mem, int* status,
                              uint32_t* crcs) {
  if (!h || nstripes < 0 || n <= 0 || (nstripes > 0 && (!shards || !status || !crcs))) return CFSEC_ERR_INVALID_ARG;
  std::memset(crcs, 0, sizeof(uint32_t) * (size_t)nstripes * n);
  const cfsec::CrcOut c = crc_out(crcs, nstripes, n);
  return guarded([&] { return h->e->encode_batch(shards, n, nstripes, mem, status, nullptr, &c); });
}

int cfsec_ec_encode_blobs_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nstripes, int mem, int* status,
                              uint32_t* crcs) {
  if (!h || nstripes < 0 || n <= 0 || (nstripes > 0 && (!shards || !status || !crcs))) return CFSEC_ERR_INVALID_ARG;
  std::memset(crcs, 0, sizeof(uint32_t) * (size_t)nstripes * n);
  const cfsec::CrcOut c = crc_out(crcs, nstripes, n);
  return guarded([&] { return h->e->encode_batch(shards, n, nstripes, mem, status, nullptr, &c, /*blobs=*/true); });
}

int cfsec_ec_reconstruct_batch_async(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                                     const int* bad_off, int verify, int* status, uint32_t* flags, uint32_t* crcs,
                                     void* stream) {
  if (!h || nbids < 0 || n <= 0 || (nbids > 0 && (!shards || !status || !bad_off))) return CFSEC_ERR_INVALID_ARG;
  if (!bad_off_valid(nbids, bad_off, bad_idx)) return CFSEC_ERR_INVALID_ARG;
  if (verify && nbids > 0 && !flags) return CFSEC_ERR_INVALID_ARG;
  cfsec::AsyncOut a;
  a.stream = as_stream(stream);
  a.flags = flags;
  const cfsec::CrcOut c = crc_out(crcs, nbids, n);
  return guarded([&] {
    return h->e->reconstruct_batch(shards, n, nbids, bad_idx, bad_off, CFSEC_MEM_DEVICE, verify != 0, status, &a,
                                   crcs ? &c : nullptr);
  });
}

int cfsec_ec_encode_batch_async(cfsec_ec* h, cfsec_shard* shards, int n, int nstripes, int* status, uint32_t* flags,
                                uint32_t* crcs, void* stream) {
  if (!h || nstripes < 0 || n <= 0 || (nstripes > 0 && (!shards || !status))) return CFSEC_ERR_INVALID_ARG;
  cfsec::AsyncOut a;
  a.stream = as_stream(stream);
  a.flags = flags;
  const cfsec::CrcOut c = crc_out(crcs, nstripes, n);
  return guarded([&] {
    return h->e->encode_batch(shards, n, nstripes, CFSEC_MEM_DEVICE, status, &a, crcs ? &c : nullptr);
  });
}

int cfsec_ec_repair_rows(cfsec_ec* h, const int* bad_idx, int nbad, const int* want, int nwant, int* in_idx,
                         uint8_t* rows) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->repair_rows(bad_idx, nbad, want, nwant, in_idx, rows); });
}

int cfsec_ec_matvec_batch(cfsec_ec* h, const uint8_t* coef, int rows, uint8_t* const* ptrs, size_t shard_size,
                          int nstripes, void* stream) {
  if (!h) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] { return h->e->matvec_batch(coef, rows, ptrs, shard_size, nstripes, as_stream(stream)); });
}

int cfsec_ec_shards_in_idc(const cfsec_ec* h, int idx, int* out, int out_cap, int* count) {
  if (!h || !count) return CFSEC_ERR_INVALID_ARG;
  const std::vector<int> v = h->e->shards_in_idc(idx);
  *count = (int)v.size();
  if (out_cap < (int)v.size() || (!out && !v.empty())) return CFSEC_ERR_INVALID_ARG;
  for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
  return CFSEC_OK;
}

// ---------------- pinned host memory ----------------

int cfsec_host_alloc(size_t size, void** out) {
  if (!out) return CFSEC_ERR_INVALID_ARG;
  *out = nullptr;
  if (size == 0) return CFSEC_OK;
  return guarded([&] {
    const int st = (int)cfsec::hip_status(hipHostMalloc(out, size, hipHostMallocPortable), "hipHostMalloc");
    if (st == CFSEC_OK) cfsec::host_range_add(*out, size);
    return st;
  });
}

int cfsec_host_free(void* p) {
  if (!p) return CFSEC_OK;
  return guarded([&] {
    cfsec::host_range_remove(p);
    return (int)cfsec::hip_status(hipHostFree(p), "hipHostFree");
  });
}

// ---------------- CRC32 ----------------

int cfsec_crc32_ieee_batch(uint8_t* const* ptrs, size_t shard_size, int n, uint32_t* out,
                           int device, void* stream) {
  if ((!ptrs && n > 0) || !out || n < 0) return CFSEC_ERR_INVALID_ARG;
  if (n > 0 && shard_size > 0xFFFFFFFFull - 4096) {  // launch_crc32_to's limit: boundary misuse, no device failure
    cfsec::set_last_error("cfsec_crc32_ieee_batch: shard_size above 2^32 - 1 - 4096");
    return CFSEC_ERR_INVALID_ARG;
  }
  return guarded([&] {
    cfsec::DeviceContext* ctx = device_context(device);
    if (!ctx) return (int)CFSEC_ERR_DEVICE;
    cfsec::SyncCall call(ctx, 0, (size_t)n, as_stream(stream), !stream);
    if (!call.begun()) return call.status();
    cfsec::DeviceContext::Workspace* ws = call.ws();
    hipStream_t s = call.stream();
    call.step("launch_crc32", [&] { return cfsec::launch_crc32(ptrs, shard_size, n, ws->dflags, s); });
    call.fetch_words((size_t)n);
    const int st = call.finish();
    if (st == CFSEC_OK)
      for (int i = 0; i < n; ++i) out[i] = cfsec::crc32_finalize(ws->hflags[i], shard_size);
    return st;
  });
}

// Checksums of concatenations (host arithmetic in GF(2)[x] mod P, gf_crc.hip's xpow / mulmod):
// ChecksumIEEE(A || B) = ChecksumIEEE(A) * x^(8|B|) ^ ChecksumIEEE(B) -- the init and final XORs of
// the two halves cancel (zlib's crc32_combine identity).
uint32_t cfsec_crc32_combine(uint32_t crc1, uint32_t crc2, int64_t len2) {
  if (len2 <= 0) return crc1 ^ crc2;
  return cfsec::crc_mulmod(cfsec::crc_xpow(8 * len2), crc1) ^ crc2;
}

int cfsec_crc32_shift(uint32_t* words, int n, int64_t nbytes) {
  if ((!words && n > 0) || n < 0 || nbytes < 0) return CFSEC_ERR_INVALID_ARG;
  if (nbytes == 0) return CFSEC_OK;
  const uint32_t xp = cfsec::crc_xpow(8 * nbytes);
  for (int i = 0; i < n; ++i) words[i] = cfsec::crc_mulmod(xp, words[i]);
  return CFSEC_OK;
}

int cfsec_stream_copy(void* dst, const void* src, size_t bytes, void* stream) {
  return guarded([&] {
    return (int)cfsec::hip_status(cfsec::launch_stream_copy(dst, src, bytes, static_cast<hipStream_t>(stream)),
                                  "launch_stream_copy");
  });
}

// ---------------- crc32block ----------------

int64_t cfsec_crc32block_encode_size(int64_t size, int64_t block_len) {
  if (!cfsec::crc32block_valid_len(block_len) || size < 0) return -1;
  return crc32block_framed(size, block_len);
}

int64_t cfsec_crc32block_decode_size(int64_t total, int64_t block_len) {
  if (!cfsec::crc32block_valid_len(block_len) || total < 0) return -1;
  return total - 4 * ((total + block_len - 1) / block_len);  // util.go:59-65
}

int cfsec_crc32block_encode(const uint8_t* src, int64_t size, int64_t block_len, uint8_t* dst,
                            uint32_t* shard_crc, int mem, int device, void* stream) {
  return crc32block_call(true, src, size, size, block_len, 0, size, dst, shard_crc, nullptr, mem, device, stream);
}

int cfsec_crc32block_decode(const uint8_t* src, int64_t src_len, int64_t size, int64_t block_len, int64_t from,
                            int64_t to, uint8_t* dst, int64_t* bad_block, int mem, int device, void* stream) {
  return crc32block_call(false, src, src_len, size, block_len, from, to, dst, nullptr, bad_block, mem, device,
                         stream);
}

int cfsec_crc32block_encode_batch(const uint8_t* const* srcs, uint8_t* const* dsts, int n, int64_t size,
                                  int64_t block_len, uint32_t* shard_crcs, void* stream) {
  if (!cfsec::crc32block_valid_len(block_len)) return CFSEC_ERR_INVALID_BLOCK;
  if (n < 0 || size < 0 || (n > 0 && (!srcs || !dsts))) return CFSEC_ERR_INVALID_ARG;
  return guarded([&] {
    hipStream_t s = as_stream(stream);
    int st = CFSEC_OK;
    if (shard_crcs && n > 0)
      st = cfsec::hip_status(hipMemsetAsync(shard_crcs, 0, 4 * (size_t)n, s), "hipMemsetAsync");
    cfsec::Crc32BlockJob j;
    j.encode = true;
    j.n = n;
    j.in = srcs;
    j.out = dsts;
    j.size = size;
    j.block_len = block_len;
    j.whole = shard_crcs;
    if (st == CFSEC_OK) st = cfsec::hip_status(cfsec::launch_crc32block(j, s), "launch_crc32block");
    return st;
  });
}

int cfsec_crc32block_decode_batch(const uint8_t* const* srcs, int64_t src_len, uint8_t* const* dsts, int n,
                                  int64_t size, int64_t block_len, int64_t from, int64_t to, uint32_t* bad,
                                  void* stream) {
  if (!cfsec::crc32block_valid_len(block_len)) return CFSEC_ERR_INVALID_BLOCK;
  if (n < 0 || size < 0 || from < 0 || from > to || to > size || (n > 0 && (!srcs || !bad)) ||
      (n > 0 && to > from && !dsts))
    return CFSEC_ERR_INVALID_ARG;
  // the framed end of the last block the range touches must lie inside every source object
  if (decode_source_short(blocks_touched(false, size, block_len, from, to), src_len)) return CFSEC_ERR_SHORT_DATA;
  return guarded([&] {
    hipStream_t s = as_stream(stream);
    int st = CFSEC_OK;
    if (n > 0) st = cfsec::hip_status(hipMemsetAsync(bad, 0xFF, 4 * (size_t)n, s), "hipMemsetAsync");
    cfsec::Crc32BlockJob j;
    j.encode = false;
    j.n = n;
    j.in = srcs;
    j.out = dsts;
    j.size = size;
    j.block_len = block_len;
    j.from = from;
    j.to = to;
    j.bad = bad;
    if (st == CFSEC_OK) st = cfsec::hip_status(cfsec::launch_crc32block(j, s), "launch_crc32block");
    return st;
  });
}

int cfsec_crc32block_check_objects(const cfsec_blk_object* o, int n, int64_t block_len, int* status,
                                   int64_t* bad_block, uint32_t* shard_crc, int mem, int device, void* stream) {
  return crc32block_objects_call(cfsec::kBlkCheck, o, n, block_len, status, bad_block, shard_crc, mem, device, stream);
}

int cfsec_crc32block_decode_objects(const cfsec_blk_object* o, int n, int64_t block_len, int* status,
                                    int64_t* bad_block, uint32_t* shard_crc, int mem, int device, void* stream) {
  return crc32block_objects_call(cfsec::kBlkDecode, o, n, block_len, status, bad_block, shard_crc, mem, device, stream);
}

int cfsec_crc32block_encode_objects(const cfsec_blk_object* o, int n, int64_t block_len, int* status,
                                    uint32_t* shard_crc, int mem, int device, void* stream) {
  return crc32block_objects_call(cfsec::kBlkEncode, o, n, block_len, status, nullptr, shard_crc, mem, device, stream);
}

}  // extern "C"

// ---------------- contiguous stripes (ec.Buffer layout) ----------------

namespace {
// Shard headers of a contiguous stripe: shard i at base + i * stride, `size` bytes, missing[] (when
// given) marked len 0 with their buffer kept as capacity.
int contig_shards(uint8_t* base, size_t size, size_t stride, int n, const int* missing, int nmissing,
                  std::vector<cfsec_shard>* out) {
  if (!base || n <= 0 || size == 0 || stride < size || nmissing < 0 || (nmissing > 0 && !missing))
    return CFSEC_ERR_INVALID_ARG;
  out->assign((size_t)n, cfsec_shard{nullptr, 0, 0});
  for (int i = 0; i < n; ++i) (*out)[i] = cfsec_shard{base + (size_t)i * stride, size, size};
  for (int j = 0; j < nmissing; ++j) {
    if (missing[j] < 0 || missing[j] >= n) return CFSEC_ERR_INVALID_ARG;
    (*out)[missing[j]].len = 0;
  }
  return CFSEC_OK;
}
}  // namespace

int cfsec_rs_encode_contig(cfsec_rs* h, uint8_t* base, size_t shard_size, size_t stride, int n, int mem,
                           void* stream) {
  std::vector<cfsec_shard> v;
  const int st = contig_shards(base, shard_size, stride, n, nullptr, 0, &v);
  if (!h || st != CFSEC_OK) return CFSEC_ERR_INVALID_ARG;
  return cfsec_rs_encode(h, v.data(), n, mem, stream);
}

int cfsec_rs_verify_contig(cfsec_rs* h, uint8_t* base, size_t shard_size, size_t stride, int n, int mem,
                           void* stream, int* ok) {
  std::vector<cfsec_shard> v;
  const int st = contig_shards(base, shard_size, stride, n, nullptr, 0, &v);
  if (!h || st != CFSEC_OK) return CFSEC_ERR_INVALID_ARG;
  return cfsec_rs_verify(h, v.data(), n, mem, stream, ok);
}

int cfsec_rs_reconstruct_contig(cfsec_rs* h, uint8_t* base, size_t shard_size, size_t stride, int n,
                                const int* missing, int nmissing, int data_only, int mem, void* stream) {
  std::vector<cfsec_shard> v;
  const int st = contig_shards(base, shard_size, stride, n, missing, nmissing, &v);
  if (!h || st != CFSEC_OK) return CFSEC_ERR_INVALID_ARG;
  return data_only ? cfsec_rs_reconstruct_data(h, v.data(), n, mem, stream)
                   : cfsec_rs_reconstruct(h, v.data(), n, mem, stream);
}

int cfsec_ec_encode_contig(cfsec_ec* h, uint8_t* base, size_t shard_size, size_t stride, int n, int mem,
                           void* stream) {
  std::vector<cfsec_shard> v;
  const int st = contig_shards(base, shard_size, stride, n, nullptr, 0, &v);
  if (!h || st != CFSEC_OK) return CFSEC_ERR_INVALID_ARG;
  return cfsec_ec_encode(h, v.data(), n, mem, stream);
}

int cfsec_ec_verify_contig(cfsec_ec* h, uint8_t* base, size_t shard_size, size_t stride, int n, int mem,
                           void* stream, int* ok) {
  std::vector<cfsec_shard> v;
  const int st = contig_shards(base, shard_size, stride, n, nullptr, 0, &v);
  if (!h || st != CFSEC_OK) return CFSEC_ERR_INVALID_ARG;
  return cfsec_ec_verify(h, v.data(), n, mem, stream, ok);
}

int cfsec_ec_reconstruct_contig(cfsec_ec* h, uint8_t* base, size_t shard_size, size_t stride, int n,
                                const int* bad_idx, int nbad, int data_only, int mem, void* stream) {
  std::vector<cfsec_shard> v;
  const int st = contig_shards(base, shard_size, stride, n, nullptr, 0, &v);
  if (!h || st != CFSEC_OK) return CFSEC_ERR_INVALID_ARG;
  return data_only ? cfsec_ec_reconstruct_data(h, v.data(), n, bad_idx, nbad, mem, stream)
                   : cfsec_ec_reconstruct(h, v.data(), n, bad_idx, nbad, mem, stream);
}

int cfsec_ec_encode_batch_contig(cfsec_ec* h, uint8_t* base, size_t shard_size, size_t stride, size_t stripe_stride,
                                 int n, int nstripes, int mem, int* status, uint32_t* crcs) {
  if (!h || nstripes < 0 || n <= 0 || (nstripes > 0 && (!base || !status))) return CFSEC_ERR_INVALID_ARG;
  if (nstripes > 1 && stripe_stride < stride * (size_t)n) return CFSEC_ERR_INVALID_ARG;  // stripes overlap
  std::vector<cfsec_shard> all((size_t)nstripes * n), one;
  for (int s = 0; s < nstripes; ++s) {
    if (contig_shards(base + (size_t)s * stripe_stride, shard_size, stride, n, nullptr, 0, &one) != CFSEC_OK)
      return CFSEC_ERR_INVALID_ARG;
    std::copy(one.begin(), one.end(), all.begin() + (size_t)s * n);
  }
  return crcs ? cfsec_ec_encode_batch_crc(h, all.data(), n, nstripes, mem, status, crcs)
              : cfsec_ec_encode_batch(h, all.data(), n, nstripes, mem, status);
}

int cfsec_ec_reconstruct_batch_contig(cfsec_ec* h, uint8_t* base, const uint64_t* bid_off,
                                      const uint64_t* bid_shard_size, int n, int nbids, const int* bad_idx,
                                      const int* bad_off, int verify, int mem, int* status, uint32_t* crcs) {
  if (!h || nbids < 0 || n <= 0 || (nbids > 0 && (!base || !bid_off || !bid_shard_size || !status)))
    return CFSEC_ERR_INVALID_ARG;
  std::vector<cfsec_shard> all((size_t)nbids * n), one;
  for (int b = 0; b < nbids; ++b) {
    const size_t S = (size_t)bid_shard_size[b];
    if (S == 0) {  // a zero-size bid: every shard empty (the reference loop skips those, :730-733)
      for (int i = 0; i < n; ++i) all[(size_t)b * n + i] = cfsec_shard{base + bid_off[b], 0, 0};
      continue;
    }
    if (contig_shards(base + bid_off[b], S, S, n, nullptr, 0, &one) != CFSEC_OK) return CFSEC_ERR_INVALID_ARG;
    std::copy(one.begin(), one.end(), all.begin() + (size_t)b * n);
  }
  return crcs ? cfsec_ec_reconstruct_batch_crc(h, all.data(), n, nbids, bad_idx, bad_off, verify, mem, status, crcs)
              : cfsec_ec_reconstruct_batch(h, all.data(), n, nbids, bad_idx, bad_off, verify, mem, status);
}
