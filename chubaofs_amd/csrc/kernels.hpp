// kernels.hpp -- host-side interface of the gfx950 GF(2^8) shard kernels.
//
// One kernel family does all the byte arithmetic of the path: a GF(2^8)
// matrix x shard-vector product over a batch of stripes,
//
//     out[s][r][b] = XOR_c coef[r][c] * in[s][c][b]      (b over the shard bytes)
//
// which is what KRS/reedsolomon.go:807-1134 (codeSomeShards / ...P / ...AVXP) and the
// generated AVX2/GFNI kernels (KRS/galois_gen_amd64.s) compute for Encode, for both
// passes of reconstruct, and (with a compare instead of a store) for Verify.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cfsec {

enum class MatVecMode : uint32_t {
  kStore = 0,        // out = M * in
  kAccum = 1,        // out ^= M * in     (input chunking when k > kMaxK)
  kVerify = 2,       // flags[s] |= (out != M * in)
  kStoreVerify = 3,  // rows [0, nstore): out = M * in; rows [nstore, m): flags[s] |= (out != M * in)
};

struct MatVecJob {
  int k = 0;                           // inputs per stripe
  int m = 0;                           // outputs per stripe
  const uint8_t* coef = nullptr;       // host, m x k row-major
  size_t len = 0;                      // bytes per shard
  int nstripes = 0;
  const uint8_t* const* in = nullptr;  // host array [nstripes * k] of device pointers
  uint8_t* const* out = nullptr;       // host array [nstripes * m] of device pointers
  MatVecMode mode = MatVecMode::kStore;
  uint32_t* flags = nullptr;           // device [nstripes], kVerify / kStoreVerify
  int nstore = 0;                      // kStoreVerify: stored rows (the first nstore of m)
  const uint64_t* lens = nullptr;      // host [nstripes] per-stripe lengths (len = 0 then); NULL: all `len`
};

// Reconstruct (+ Verify) of stripes of the 16 + 20 code through the 16x16 dyadic block
// (gf_dyadic16.hpp repair_dy16): the nd <= 4 missing data rows from decode rows, then every parity
// row from the 16 data rows, stored (pstore bit r) or compared (pcmp bit r, mismatch -> flags).
struct Dy16RepairJob {
  int nd = 0;                          // missing data rows
  int e = 0;                           // extra rows over the data after the parity rows (0 or 2)
  const uint8_t* coef = nullptr;       // host: parity matrix (20 x 16), the e extra rows, the nd decode rows
  uint8_t src[16] = {};                // data row i: input slot, or 16 + j for missing data row j
  uint32_t pstore = 0, pcmp = 0;       // parity (then extra) rows stored / compared
  size_t len = 0;
  const uint64_t* lens = nullptr;      // host [nstripes] per-stripe lengths, or NULL
  int nstripes = 0;
  const uint8_t* const* in = nullptr;  // host [nstripes * 16]: the first 16 present rows
  uint8_t* const* out = nullptr;       // host [nstripes * (nd + 20 + e)]: missing data rows, parity 0..19, extras
  uint32_t* flags = nullptr;           // device [nstripes]
  uint32_t* zero_words = nullptr;      // device: nzero words the first launch zeroes (a batch's checksum
  uint32_t nzero = 0;                  // words, XOR-accumulated by the checksum pass that follows)
  bool syn = false;                    // the syndrome form below is set: the bit-sliced kernel may run
  uint8_t prow[4] = {};                // input 16 - nd + q is parity row prow[q]
  uint8_t ainv[16] = {};               // missing row j = sum_q ainv[j * 4 + q] * syndrome of prow[q]
};
hipError_t launch_dy16_repair(const Dy16RepairJob& job, hipStream_t stream);

// Verify flags of a batch call gathered per batch item (batch.cpp run_device): for every item o,
// out[o] = OR of the per-task words tmp[word[j]] of the pairs (o, word[j]) -- `accumulate`: out[o] |=
// (v != 0), else out[o] = (v != 0) -- and those tmp words are reset to 0, so a workspace's flag words
// stay zero between calls (no memset per call).  pairs: n (item, word) entries sorted by item; out
// may be host-mapped pinned memory (the synchronous calls read it after the sync, no D2H copy).
// cfsec_stream_copy: dst[0, bytes) <- src, 16-byte non-temporal grid-stride copy (bytes % 16 == 0).
hipError_t launch_stream_copy(void* dst, const void* src, size_t bytes, hipStream_t stream);
hipError_t launch_flag_gather(uint32_t* tmp, uint32_t* out, const int* item, const int* word, int n,
                              bool accumulate, hipStream_t stream);

// Rows one launch carries (dev::kMaxK / dev::kMaxM); kStoreVerify needs m <= kLaunchMaxRows.
constexpr int kLaunchMaxRows = 32;

// Enqueue the product on `stream`.  Splits into as many launches as the kernel
// argument block needs (inputs > 32, outputs > 32, or too many pointers): plan_matvec decides them,
// launch_matvec fills one argument block per step and calls the launcher the step names.
hipError_t launch_matvec(const MatVecJob& job, hipStream_t stream);

// Which kernels run a job, decided in one place (gf_kernels.hip, whose header lists the families).
// A pure host function: no HIP calls; it reads the job's scalar fields, coef, lens, the pointer
// arrays (stride, alignment, span) and the A/B switches CFSEC_LUT, CFSEC_BS16, CFSEC_BS_TAB and
// CFSEC_BS_CRC.  It returns the error launch_matvec returns for the job, or visits its launches in
// order.  One step: rows [r0, r0 + mc) x inputs [c0, c0 + kc) of stripes [s0, s0 + ns), bytes
// [off, off + prefix) of each by the bit-sliced 16 + 20 kernel `bs` names, then `tail` bytes by the
// family kernel (either may be 0, not both).
enum class MatVecFamily : int { kRuntimeK = 0, kFixedK, kDyadic, kDyadic16, kLookup, kBsPlain };
enum class BsPrefix : int {
  kNone = 0,
  kEncode,  // launch_bs on the run (affine, or the run's stripes in the argument block)
  kVerify,  // the bit-sliced repair with nothing missing, every row compared (affine runs)
  kTable,   // launch_bs_tab: every stripe of a scattered job at once (s0 = 0, ns = nstripes, no tail);
            // the runs that follow carry off = prefix and only the rows' tails
};
struct MatVecStep {
  int r0, mc, c0, kc, s0, ns;
  MatVecMode mode;  // resolved: kStoreVerify with nstore 0 / m folded, kAccum for c0 > 0
  MatVecFamily family;
  BsPrefix bs;
  int M, OS, threads;          // runtime-k: rows per wave, waves per column chunk, workgroup size
  int B, E;                    // dyadic: block size, trailing plain rows
  uint64_t off, prefix, tail;  // off + prefix + tail = the run's (longest) length
  int64_t sstride;             // != 0: an affine run (one pointer set, any stripe count)
  uint32_t tile;               // bytes per workgroup of the family kernel
  uint32_t grid_x, grid_y;     // of the family launch (0 when tail == 0)
  const uint8_t* const* rows;  // kTable: every stripe's k inputs then m outputs (valid during the visit)
  // kTable only, set by the visitor: false when the device row-offset table could not be had -- the
  // one outcome the plan cannot know.  The plan then goes on as if it had not chosen the table.
  bool table_ok;
};
using MatVecVisitor = hipError_t (*)(MatVecStep& step, void* ctx);  // != hipSuccess ends the plan
hipError_t plan_matvec(const MatVecJob& job, MatVecVisitor visit, void* ctx);
const char* matvec_family_name(MatVecFamily f);  // "runtime-k", "fixed-k", "dyadic", "dyadic-16", "lookup", "bs-plain"
const char* bs_prefix_name(BsPrefix p);          // "none", "encode", "verify", "table"
// CFSEC_TRACE_MATVEC (read per call) prints one stderr line per step launch_matvec dispatches:
// "cfsec: matvec family=<name> bs=<none|encode|verify|table> mode=.. k=.. m=.. r0=.. c0=.. stripes=..
// prefix=.. tail=.. affine=..".

// The mixed-plan launch (gf_mix.hip): store-only products of many items, each with its own rows,
// length, input and output count and coefficient rows, read by the workgroups from the item table at
// device address `table` (gf_mix.hpp; packed by pack_mix, engine.hpp).  One workgroup per tile of
// 4 KiB of an item's rows; the argument block holds the table's address and the tile count only, so
// the item count is unbounded and one launch carries at most kMixMaxTiles tiles.
constexpr uint32_t kMixMaxTiles = 1u << 24;
hipError_t launch_mix(const uint8_t* table, uint32_t ntiles, hipStream_t stream);
// The same launch with crc32.ChecksumIEEE of every row of every item, inputs and outputs, out of the
// product's pass (gf_mix_crc.hip): `table` is the device copy of gf_mix_crc.hpp's table (packed by
// pack_mix_crc, engine.hpp), whose head names the CRC table block (crc_device_tables) and the checksum
// words; each row's word is XOR-accumulated, so the caller zeroes the words first.
hipError_t launch_mix_crc(const uint8_t* table, uint32_t ntiles, hipStream_t stream);
// The same again with Verify in it (gf_mix_sv.hip): of an item's output rows the first nstore are
// stored, the rest compared with the shards' own bytes -- a mismatch stores 1 into the item's Verify
// word, whose address the table holds (device memory or page-locked host memory the device addresses;
// the caller zeroes it) -- and a compared row's checksum is that of the shard as it stands.  `table` is
// the device copy of gf_mix_sv.hpp's table (packed by pack_mix_sv, engine.hpp).
hipError_t launch_mix_sv(const uint8_t* table, uint32_t ntiles, hipStream_t stream);
// The same for items of the 16 + 20 code whose plan carries a Dy16Plan (gf_mix_sv16.hip): the missing
// data rows from their decode rows, then every parity and extra row through the 16x16 dyadic block,
// stored, compared or dropped by the item's masks, from one read of the 16 inputs.  `table` is the
// device copy of gf_mix_sv16.hpp's table (packed by pack_mix_sv16, engine.hpp); words and Verify words
// as launch_mix_sv.
hipError_t launch_mix_sv16(const uint8_t* table, uint32_t ntiles, hipStream_t stream);

// launch_dy16_repair's decisions, the same way: per job the table launch, per run the affine
// bit-sliced prefix and the dyadic tail.
enum class RepairBs : int { kNone = 0, kAffine, kTable };
struct RepairStep {
  int s0, ns;
  RepairBs bs;  // kTable: every stripe at once (s0 = 0), the runs after it carry off = prefix
  uint64_t off, prefix, tail;
  int64_t sstride;
  const uint8_t* const* rows;  // kTable: as MatVecStep::rows (this table launch has no runtime fallback)
};
using RepairVisitor = hipError_t (*)(RepairStep& step, void* ctx);
hipError_t plan_dy16_repair(const Dy16RepairJob& job, RepairVisitor visit, void* ctx);

// crc32.ChecksumIEEE of n device shards of `len` bytes into device out[n].
// Leaves the raw (pre-conditioning) word per shard in out; crc32_finalize turns it
// into crc32.ChecksumIEEE.
hipError_t launch_crc32(const uint8_t* const* ptrs, size_t len, int n, uint32_t* out,
                        hipStream_t stream);
uint32_t crc32_finalize(uint32_t raw, size_t len);
// Standalone form with scattered outputs: shard i's word is out[idx[i]] (idx NULL: out[i]),
// accumulated with atomicXor into words the caller has zeroed, `fin` XOR-ed in once per shard
// (crc32_shift_ones(len) gives crc32.ChecksumIEEE directly).
hipError_t launch_crc32_to(const uint8_t* const* ptrs, size_t len, int n, uint32_t* out, const uint32_t* idx,
                           uint32_t fin, hipStream_t stream);
// The launches of that pass, decided the way plan_matvec_crc decides the fused kernels': a pure host
// function (no HIP calls) of the shard length (0 < len <= 2^32 - 1 - 4096), the list's shard count
// n > 0, whether the list is affine -- equally spaced pointers with consecutive words and at most
// 65535 shards, which launch_crc32_to finds out -- and `total`, the workgroups aimed at over the whole
// list (4096, or CFSEC_CRC32_GROUPS_PROBE, read per call).  A shard is `tiles` tiles of 4 KiB; every
// launch is `groups` workgroups of tpw consecutive tiles (at least 16 where the shard has them, at
// most 384 groups) by per_launch shards, workgroup g's tiles ending at byte end[g] (its constant is
// x^(8 (len - end[g]))).  The argument block's 800 flexible words hold the constants, padded to `pw`
// words, then the pointers and words of the shards: `slots` = (800 - pw) / 3 shards of a pointer-table
// launch, per_launch = min(n, slots); an affine list needs one pointer, per_launch = n.
// CFSEC_TRACE_CRC32 (read per call) prints one stderr line per kernel launch:
// "cfsec: crc32 len=.. shards=<of this launch> s0=<its first shard> tiles=.. groups=.. tpw=..
// affine=<0|1> idx=<0|1: scattered words> fin=<0|1: fin != 0>".
struct Crc32Plan {
  uint32_t tiles, groups, tpw, pw;
  int slots, per_launch;
  std::vector<int64_t> end;
};
Crc32Plan plan_crc32(size_t len, int n, bool affine, uint32_t total);

// Encode / reconstruct (kStore) and Reconstruct + Verify (kStoreVerify) with crc32.ChecksumIEEE of the rows the product touches, fused
// into the product kernel (gf_crc.hpp): row i of the product (inputs 0..k-1, then outputs) has its
// checksum in device word crc[s * crc_stride + slot[i]] of stripe s.  slot[0] < 0 skips the inputs
// (checksum the outputs only).  Every word of crc[0 .. nstripes*crc_stride) is zeroed first, so
// words no row maps to read 0 (zero = false: the caller zeroed them; the kernel XORs into them).
//
// Which fused kernel runs a job, decided in one place (gf_crc.hip).  A pure host function: no HIP
// calls, it reads the job's scalar fields, coef, slot and the A/B masks (CFSEC_BS_CRC,
// CFSEC_CRC_LDS, CFSEC_CRC_LDS12, CFSEC_SV_CRC):
//   kBitSliced  gf_bs_crc.hip: coef equals a code mode's network, the inputs checksummed too
//               (slot[0] >= 0), at most 64^3 tiles of 2 KiB per row and 2^32 - 1 over the stripes
//   kLookup     gf_crc_lds_kernel: k in {6, 8, 12, 16}, m <= 4; any 6 x 12 matrix with the inputs
//               checksummed
//   kVperm      the v_perm kernels: k in {6, 8, 12, 16, 18}, m <= 6; 6 x 12 of EC6P10L2's form (10
//               rows of 2x2 dyadic blocks + 2 plain rows) with the inputs checksummed.
//               kStoreVerify jobs (Reconstruct + Verify, gf_crc_sv_kernel: compared rows checksummed
//               from the bytes in memory) have this route alone: the same k, 2 <= m <= 6,
//               0 < nstore < m, every row checksummed (slot[0] >= 0), one length (lens == NULL),
//               flags set; CFSEC_SV_CRC=0 switches it off
//   kNone       no fused kernel (every other input count -- 3, 4, 10, 15 -- without its network's
//               conditions, m > 6, kAccum / kVerify, a kStoreVerify job outside the conditions above,
//               slots outside [0, crc_stride), crc_stride > 256, len > 2^32 - 1 - 4096): the product
//               and the separate pass
enum class CrcRoute : int { kNone = 0, kBitSliced = 1, kLookup = 2, kVperm = 3 };
CrcRoute matvec_crc_route(const MatVecJob& job, int crc_stride, const int* slot);
const char* crc_route_name(CrcRoute r);  // "none", "bit-sliced", "lookup", "v_perm"
// route != kNone.  launch_matvec_crc takes exactly the jobs this accepts, by construction: it
// dispatches on the same matvec_crc_route answer; callers send everything else to the product and
// the separate pass (launch_matvec + launch_crc32_to).  CFSEC_TRACE_CRC (read per call) prints
// "cfsec: crc route=<name> k=.. m=.. cin=.. stripes=.. len=.." to stderr per launch_matvec_crc of a
// kStore job, "cfsec: crc sv k=.. m=.. nstore=.. stripes=.. len=.. tpw=.. groups=.. per=.." per
// kStoreVerify job.
bool matvec_crc_accepts(const MatVecJob& job, int crc_stride, const int* slot);
hipError_t launch_matvec_crc(const MatVecJob& job, uint32_t* crc, int crc_stride, const int* slot,
                             hipStream_t stream, bool zero = true);

// The launches of the fused kernels, decided the way plan_matvec decides launch_matvec's: pure host
// functions (no HIP calls) of the job and of one device-dependent number, `resident` -- the workgroups
// of the chosen kernel the device holds at once, which the dispatchers get from an occupancy query
// (cached per device) and pass in.  resident <= 0 says the query failed: 768 for the bit-sliced
// kernels, 1024 for the lookup kernel (the v_perm kernels always take 1024).
//
// Bit-sliced (the fused kernel and the plain product of gf_bs_crc.hip): a row is tps tiles of 2 KiB.
// A launch takes stripes [s0, s0 + ns) -- all of an affine job (tab = 1), 96 / (k + m) of a
// pointer-table job (tab = ns) -- with W waves per stripe in `groups` wave groups: wave j of a group
// takes tiles j, j + W, ... below bend = W floor(tps / W) of the group's stripes, its registers
// jumping `jump` = 2048 W bytes between them, and the stripes' last tail = tps - bend tiles go one per
// wave to the workgroups from tblk on (4 waves per workgroup).  CFSEC_TRACE_CRC prints per launch
// "cfsec: bs launch stripes=<ns> tps=.. W=.. groups=.. resident=.. tail=..".
struct BsCrcStep {
  int s0, ns;
  uint32_t tab;
  int64_t sstride;
  uint32_t tps, W, groups, bend, tail, tblk, grid;
  uint64_t jump;
};
struct BsCrcPlan {
  int resident;       // as used (the fallback when none was given)
  int64_t pad;        // zero bytes after the row in its last tile
  int64_t pw[3];      // tile e's end to the row's end is x^(8 (e0 pw[0] + e1 pw[1] + e2 pw[2] - pad)),
                      // e = e0 + 64 e1 + 4096 e2 tiles after it: the bytes per entry of the three power tables
  std::vector<BsCrcStep> steps;
};
BsCrcPlan plan_bs_crc(const MatVecJob& job, int resident);
// Lookup / v_perm (gf_crc.hpp): a row is `tiles` tiles of 4 KiB; every launch is grid_x = groups
// workgroups of tpw consecutive tiles by grid_y stripes -- `per` stripes per launch (all of an affine
// job, else 96 / (k + m), at most 65535; grid_y is the first launch's) -- workgroup g's tiles ending
// at byte end[g] (its constant is x^(8 (len - end[g]))); dy: -1 the lookup kernel, 0 / 2 / 4 the
// v_perm kernel's plain / 2x2 / 4x4 dyadic product (a kStoreVerify job: always 0, its rows are decode
// rows).  CFSEC_CRC_GROUPS overrides the workgroup total.
struct CrcPlan {
  uint32_t tiles;
  int per, dy;
  int64_t sstride;
  uint32_t groups, tpw, grid_x, grid_y;
  std::vector<int64_t> end;
};
CrcPlan plan_matvec_crc(const MatVecJob& job, CrcRoute route, int resident);
// shift(~0, len) ^ ~0: XOR it into a raw (zero-preset) CRC of len bytes to get crc32.ChecksumIEEE.
uint32_t crc32_shift_ones(size_t len);

// blobstore/common/crc32block framing (crc32block.hip): blocks of block_len bytes, each the
// little-endian crc32.ChecksumIEEE of its payload (block_len - 4 bytes, less in the last block)
// followed by the payload.  Device pointers.  CFSEC_TRACE_BLK (read per call) prints one stderr line
// per kernel launch -- at most 128 objects each --
//   cfsec: blk launch encode=<0|1> objects=<n> blocks=<per object> items=<blocks x objects> grid=<workgroups>
//   resident=<workgroups of the strided kernel the device holds at once>
// (one line; grid = min(resident, items), or under CFSEC_BLK_GRID=0, read once per process, the fewest
// workgroups that give every one ceil(items / resident) blocks).
struct Crc32BlockJob {
  bool encode = true;
  int n = 1;                           // objects, all of the same payload size
  const uint8_t* const* in = nullptr;  // host array [n]: encode: payloads; decode: framed objects
  uint8_t* const* out = nullptr;       // host array [n]: encode: framed objects (EncodeSize bytes);
                                       // decode: to - from bytes each
  int64_t size = 0;                    // payload bytes of each object
  int64_t block_len = 0;               // positive multiple of 4096
  int64_t from = 0, to = 0;            // decode: payload range (Decoder.Reader(from, to))
  uint32_t* bad = nullptr;    // decode: device words [n] preset to ~0; receive the smallest mismatching
                              // block index relative to block from / (block_len - 4)
  uint32_t* whole = nullptr;  // encode, optional: device words [n] preset to 0; receive
                              // crc32.ChecksumIEEE of each whole payload
};
bool crc32block_valid_len(int64_t block_len);  // util.go:34-36
hipError_t launch_crc32block(const Crc32BlockJob& job, hipStream_t stream);
// Objects of mixed sizes, ranges and alignments in one launch (crc32block_objects.hip): `table` is the
// device copy of an object table (crc32block_objects.hpp; mode 0 check, 1 decode, 2 encode) whose head
// names the CRC table block (crc_device_tables) and the result words.  CFSEC_TRACE_BLK prints
//   cfsec: blk objects mode=<check|decode|encode> objects=<n> items=<blocks> grid=<workgroups> resident=<as above>
hipError_t crc_device_tables(const uint32_t** out);  // gf_crc.hip
hipError_t launch_crc32block_objects(int mode, const uint8_t* table, uint32_t objects, uint32_t items,
                                     hipStream_t stream);

}  // namespace cfsec
