/*
 * cfsec.h -- C ABI of the MI355X-native erasure-coding engine for CubeFS blobstore.
 *
 * This is the drop-in boundary.  Two layers are exported, each replacing one Go
 * interface of the reference (paths relative to the CubeFS tree):
 *
 *  1. cfsec_rs_*  replaces the reedsolomon.Encoder engine that blobstore/common/ec
 *     constructs at blobstore/common/ec/encoder.go:86 (global) and :95 (local),
 *     i.e. vendor/github.com/klauspost/reedsolomon/reedsolomon.go:25-131 with the
 *     default (Vandermonde) matrix of reedsolomon.go:220-244.  The six methods CubeFS
 *     uses are exported (Encode, Verify, Reconstruct, ReconstructData, Split, Join) and
 *     EncodeIdx, Update and ReconstructSome, plus GPU batch entry points.
 *
 *  2. cfsec_ec_*  replaces ec.Encoder (blobstore/common/ec/encoder.go:41-62) as
 *     returned by ec.NewEncoder (encoder.go:78-112), for both the plain RS encoder
 *     (encoder.go:71-180) and the LRC encoder (lrcencoder.go:28-247).
 *
 * Shard vectors.  A Go [][]byte is passed as an array of cfsec_shard {data,len,cap}.
 * len == 0 marks a missing shard (KRS/reedsolomon.go:1416-1428).  Reconstruct
 * writes into a missing shard's buffer and sets its len to the shard size; the
 * caller must have given it cap >= shard size (the cgo shim does what
 * KRS/reedsolomon.go:1514-1518 does: reuse cap, else allocate 64-B aligned).
 *
 * Memory.  mem = CFSEC_MEM_HOST: plain host memory; the engine stages through HBM
 * and returns after the results are back in host memory.  mem = CFSEC_MEM_DEVICE:
 * pointers are HBM device pointers on the engine's device; the call is enqueued on
 * `stream` (hipStream_t) and returns after it completes.  stream = NULL: the call runs on an
 * engine-owned non-blocking stream that first waits for an event recorded on the legacy default
 * stream, i.e. it is ordered after everything already queued on the default stream and on every
 * blocking stream of the device, but not after work on other non-blocking streams (PyTorch's
 * side streams are non-blocking: pass the producer's stream explicitly).
 * *_batch entry points never synchronise: they enqueue on `stream`.
 *
 * Threading.  Every handle is safe for concurrent calls from many threads (the
 * reference shares one encoder across goroutines, encoder.go:90,115-116).
 * The library never retains a caller pointer after a call returns (cgo rule).
 *
 * Errors.  Return codes map 1:1 onto the Go sentinel errors named in each value.
 */
#ifndef CFSEC_H_
#define CFSEC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  CFSEC_OK = 0,
  CFSEC_ERR_TOO_FEW_SHARDS = 1,        /* reedsolomon.ErrTooFewShards   KRS/reedsolomon.go:601  */
  CFSEC_ERR_SHARD_NO_DATA = 2,         /* reedsolomon.ErrShardNoData    KRS/reedsolomon.go:1305 */
  CFSEC_ERR_SHARD_SIZE = 3,            /* reedsolomon.ErrShardSize      KRS/reedsolomon.go:1309 */
  CFSEC_ERR_INV_SHARD_NUM = 4,         /* reedsolomon.ErrInvShardNum    KRS/reedsolomon.go:204  */
  CFSEC_ERR_MAX_SHARD_NUM = 5,         /* reedsolomon.ErrMaxShardNum    KRS/reedsolomon.go:209  */
  CFSEC_ERR_SHORT_DATA = 6,            /* reedsolomon.ErrShortData      KRS/reedsolomon.go:1556 (also ec.ErrShortData) */
  CFSEC_ERR_RECONSTRUCT_REQUIRED = 7,  /* reedsolomon.ErrReconstructRequired KRS/reedsolomon.go:1636 */
  CFSEC_ERR_SINGULAR = 8,              /* errSingular                   KRS/matrix.go:185       */
  CFSEC_ERR_INVALID_CODE_MODE = 9,     /* ec.ErrInvalidCodeMode         common/ec/encoder.go:35 */
  CFSEC_ERR_VERIFY = 10,               /* ec.ErrVerify                  common/ec/encoder.go:36 */
  CFSEC_ERR_INVALID_SHARDS = 11,       /* ec.ErrInvalidShards           common/ec/encoder.go:37 */
  CFSEC_ERR_INVALID_ARG = 12,          /* boundary misuse (NULL handle, cap < shard size, ...) */
  CFSEC_ERR_DEVICE = 13,               /* HIP runtime failure; see cfsec_last_error()         */
  CFSEC_ERR_NOT_SUPPORTED = 14,        /* reedsolomon.ErrNotSupported   KRS/reedsolomon.go:212  */
  CFSEC_ERR_INVALID_BLOCK = 15,        /* crc32block.ErrInvalidBlock    common/crc32block/util.go:29 */
  CFSEC_ERR_MISMATCHED_CRC = 16,       /* crc32block.ErrMismatchedCrc   common/crc32block/util.go:30 */
  CFSEC_ERR_INVALID_INPUT = 17         /* reedsolomon.ErrInvalidInput   KRS/reedsolomon.go:670  */
} cfsec_status;

typedef enum { CFSEC_MEM_HOST = 0, CFSEC_MEM_DEVICE = 1 } cfsec_mem;

/* One Go []byte: pointer, length, capacity. */
typedef struct {
  uint8_t* data;
  size_t len;
  size_t cap;
} cfsec_shard;

/* codemode.Tactic (blobstore/common/codemode/codemode.go:129-163). */
typedef struct {
  int n, m, l, az_count, put_quorum, get_quorum, min_shard_size;
} cfsec_tactic;

typedef struct cfsec_rs cfsec_rs;
typedef struct cfsec_ec cfsec_ec;

/* ---------------- library ---------------- */
/* "cfsec MAJOR.MINOR.PATCH (gfx950)".  ABI history: 0.2.0 inserted src_len into
 * cfsec_crc32block_decode / cfsec_crc32block_decode_batch (callers built against 0.1.0 must be
 * rebuilt); 0.3.0, 0.4.0 and 0.5.0 add entry points only; 0.5.1 adds cfsec_rs_encode_idx,
 * cfsec_rs_update, cfsec_rs_reconstruct_some, cfsec_rs_reconstruct_some_stripes, cfsec_rs_update_batch
 * and the status CFSEC_ERR_INVALID_INPUT. */
const char* cfsec_version(void);
/* Message for the last CFSEC_ERR_DEVICE on this thread ("" if none). */
const char* cfsec_last_error(void);
/* Name of a status code, e.g. "ErrTooFewShards". */
const char* cfsec_status_name(int status);
/* Number of visible HIP devices (0 if none; never an error). */
int cfsec_device_count(void);
/* How synchronous calls wait for their stream (no reference counterpart: a tuning knob):
 * 1 = poll a pinned marker word the stream writes after the call's work (default), 0 =
 * hipStreamSynchronize.  Process-wide; returns the previous mode.  Env: CFSEC_SYNC_POLL=0. */
int cfsec_set_sync_poll(int on);

/* ---------------- reedsolomon.Encoder seam ---------------- */
/* reedsolomon.New(dataShards, parityShards) -- KRS/reedsolomon.go:413-581.  The engine binds
 * to `device` (-1 = the calling thread's current HIP device). */
int cfsec_rs_new(int data_shards, int parity_shards, int device, cfsec_rs** out);
void cfsec_rs_free(cfsec_rs* h);
int cfsec_rs_data_shards(const cfsec_rs* h);
int cfsec_rs_parity_shards(const cfsec_rs* h);
/* Copy the (data+parity) x data encoding matrix (row-major) into out. */
int cfsec_rs_matrix(const cfsec_rs* h, uint8_t* out, size_t out_len);

/* Encode -- KRS/reedsolomon.go:609-625 */
int cfsec_rs_encode(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream);
/* Encode followed by crc32.ChecksumIEEE of every shard (access/stream_put.go:125-143 then
 * :249-253) in one fused pass: crcs is a host array of n words.  Host memory from
 * cfsec_host_alloc is coded in place over PCIe; other host memory is staged through HBM. */
int cfsec_rs_encode_crc(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream, uint32_t* crcs);
/* Verify -- KRS/reedsolomon.go:770-784; *ok = 1 when every parity shard matches. */
int cfsec_rs_verify(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream, int* ok);
/* Reconstruct / ReconstructData -- KRS/reedsolomon.go:1377-1552 */
int cfsec_rs_reconstruct(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream);
int cfsec_rs_reconstruct_data(cfsec_rs* h, cfsec_shard* shards, int n, int mem, void* stream);
/* EncodeIdx -- KRS/reedsolomon.go:631-667: parity[r] ^= M[k+r][idx] * data_shard for the nparity ==
 * parity_shards parity shards (all present, one size, equal to data_shard->len); the data shard is
 * read only.  Checks in the reference's order: nparity (ErrTooFewShards), no parity shards (OK), idx
 * (ErrInvShardNum), the parity shards (ErrShardNoData / ErrShardSize), the data shard's length
 * (ErrShardSize). */
int cfsec_rs_encode_idx(cfsec_rs* h, const cfsec_shard* data_shard, int idx,
                        cfsec_shard* parity, int nparity, int mem, void* stream);
/* Update -- KRS/reedsolomon.go:672-734: shards holds the n == data+parity shards of a stripe,
 * new_data the nnew == data_shards new data shards, absent (len == 0) where a column does not change.
 * For every changed column c: shards[c] ^= new_data[c], then parity[r] ^= M[k+r][c] * shards[c] for
 * every r -- after the call the old data shard holds the delta old ^ new, not the new contents, as in
 * the reference (:728-729); new_data is read only.  A present new_data[i] with an absent shards[i],
 * or any absent parity shard, returns CFSEC_ERR_INVALID_INPUT.  Where the C seam decides what Go
 * leaves to a panic: "absent" means len == 0 (Go's nil versus empty-non-nil distinction does not
 * cross the ABI), and a present new_data[i] whose length differs from the stripe's shard size
 * returns CFSEC_ERR_SHARD_SIZE (the reference never compares the two sizes).  Host memory that is
 * not all page-locked is staged whole through HBM. */
int cfsec_rs_update(cfsec_rs* h, cfsec_shard* shards, int n,
                    const cfsec_shard* new_data, int nnew, int mem, void* stream);
/* ReconstructSome -- KRS/reedsolomon.go:1395-1397 over :1407-1529: of the missing data shards only
 * those i with required[i] != 0 are rebuilt (cap >= shard size, len = shard size afterwards); every
 * other missing shard keeps len == 0 and no byte of its buffer is written; parity is never rebuilt.
 * nrequired < data_shards returns ErrTooFewShards; entries from nrequired on count as false (the
 * reference would index out of range).  required[i] at a missing parity index counts as a missing
 * required shard, so it defeats the "nothing required is missing" early OK, as in the reference. */
int cfsec_rs_reconstruct_some(cfsec_rs* h, cfsec_shard* shards, int n,
                              const uint8_t* required, int nrequired, int mem, void* stream);
/* Split -- KRS/reedsolomon.go:1574-1632 (host memory).  data has len/cap; the engine fills
 * out[0..total) with views into data and, when cap is short, into pad (caller-owned, at least
 * *pad_needed bytes; call once with pad == NULL to learn pad_needed), laid out as the reference's
 * AllocAligned (KRS/unsafe.go:17-41): from the first 64-byte aligned address of pad, shard j at
 * j * roundup(per, 64), len per, cap roundup(per, 64). */
int cfsec_rs_split(cfsec_rs* h, uint8_t* data, size_t len, size_t cap, cfsec_shard* out,
                   uint8_t* pad, size_t pad_len, size_t* pad_needed);
/* Join -- KRS/reedsolomon.go:1646-1684 (host memory): copies out_size bytes into dst. */
int cfsec_rs_join(cfsec_rs* h, uint8_t* dst, size_t dst_len, const cfsec_shard* shards, int n,
                  size_t out_size);

/* GPU batch entry points (device memory, asynchronous on `stream`).
 * ptrs holds nstripes * (data+parity) device pointers, stripe-major; every shard is
 * shard_size bytes. */
int cfsec_rs_encode_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                          void* stream);
/* flags: device array of nstripes uint32; flags[s] is OR-ed with 1 when stripe s mismatches
 * (caller zeroes it). */
int cfsec_rs_verify_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                          uint32_t* flags, void* stream);
/* Update of a device batch, asynchronous on stream (as cfsec_rs_encode_batch): one changed
 * column set cols[0..ncols) (strictly increasing, in [0, data_shards)) for every stripe;
 * ptrs as cfsec_rs_encode_batch (entries of unchanged data columns are never dereferenced and
 * may be NULL); new_ptrs[s * ncols + j] = the new contents of column cols[j] of stripe s.  As
 * cfsec_rs_update, the changed columns are left holding old ^ new. */
int cfsec_rs_update_batch(cfsec_rs* h, uint8_t* const* ptrs, uint8_t* const* new_ptrs,
                          const int* cols, int ncols, size_t shard_size, int nstripes, void* stream);
/* Rebuild the shards listed in erased[] (same pattern for every stripe) from the first
 * data_shards surviving shards, in one fused pass (missing data rows = inv(sub), missing
 * parity rows = parity * inv(sub)).  data_only = 1 rebuilds only erased data shards. */
int cfsec_rs_reconstruct_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                               const int* erased, int nerased, int data_only, void* stream);

/* Encode / reconstruct with the shard checksums CubeFS computes right after coding
 * (crc32.ChecksumIEEE, access/stream_put.go:249-253; blobnode/work_shard_recover.go:335-342),
 * fused into the coding kernel where the shape allows (k in {6,8,12,16,18}, <= 6 outputs): no
 * extra pass over the shards.  crcs: device array of nstripes * (data+parity) uint32, indexed
 * [stripe][shard].  Encode fills every word; reconstruct fills the words of the shards it rebuilt
 * and zeroes the rest.  Asynchronous on `stream`. */
int cfsec_rs_encode_crc_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                              uint32_t* crcs, void* stream);
int cfsec_rs_reconstruct_crc_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                                   const int* erased, int nerased, int data_only, uint32_t* crcs,
                                   void* stream);
/* blobnode's repair with the checksum work around it: cfsec_rs_reconstruct_crc_batch (every erased
 * shard rebuilt) with the Verify of the same pass (flags as cfsec_rs_verify_batch: flags[s] is OR-ed
 * with 1 when a surviving parity shard outside the first data_shards survivors does not match;
 * caller zeroes it) and every word of crcs filled: crcs[s * (data+parity) + i] = crc32.ChecksumIEEE
 * of shard i as it stands in memory after the call, survivors and rebuilt shards.  One fused pass
 * for k in {6,8,12,16,18} and 2..6 rebuilt + compared shards; other shapes take the product plus the
 * separate checksum pass, same words.  CFSEC_ERR_NOT_SUPPORTED for more than 32 data shards. */
int cfsec_rs_repair_crc_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes,
                              const int* erased, int nerased, uint32_t* flags, uint32_t* crcs, void* stream);

/* ---------------- stripe batches over one or more GPUs ----------------
 * The reference codes one stripe per call: access encodes blob by blob (access/stream_put.go:104-143,
 * up to 4 blobs in flight per request) and blobnode repairs a tasklet bid by bid, each bid with
 * its own shard size and missing set, Reconstruct then Verify (blobnode/work_shard_recover.go:
 * 708-771).  These entry points take a whole batch: `shards` holds nstripes consecutive shard
 * vectors of (data+parity) entries each (stripe-major), every stripe with its own shard size and
 * its own missing shards (len == 0); stripes with one erasure pattern share a decode plan and run
 * in the same launches.  mem = CFSEC_MEM_HOST: the stripes are split into contiguous runs over the
 * handle's devices (balanced by bytes), page-locked buffers (cfsec_host_alloc) are coded in place,
 * pageable ones through double-buffered staging, one host thread and stream pair per device.
 * mem = CFSEC_MEM_DEVICE: each stripe runs on the device its memory lives on (one of the handle's
 * devices), after the work queued on that device's legacy default stream; with a one-device handle
 * every stripe must live on that device (only the first stripe's memory is queried -- one pointer
 * query costs ~1 us -- so a stripe on another GPU is the caller's error, not detected).  Synchronous: returns
 * when every result is in place.  status[s] (nstripes words) receives stripe s's result as the
 * single-stripe call would return it; the return value reports failures of the call itself
 * (CFSEC_ERR_DEVICE, CFSEC_ERR_INVALID_ARG). */
/* Devices batches are spread over (default: the handle's own device).  Call before sharing the
 * handle between threads. */
int cfsec_rs_set_devices(cfsec_rs* h, const int* devices, int ndev);
/* The split a host-memory batch uses: stripe i (moving bytes[i] bytes) runs on device index dev[i]
 * of the handle's list -- contiguous runs, balanced by bytes.  Host only (no device needed); lets a
 * caller place its staging per device ahead of the call. */
int cfsec_batch_partition(const uint64_t* bytes, int n, int ndev, int* dev);
/* Encode each stripe (KRS/reedsolomon.go:609-625). */
int cfsec_rs_encode_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status);
/* Encode each stripe, then crc32.ChecksumIEEE of every shard, data and parity (access ends every put
 * so: access/stream_put.go:125-143, 249-253): crcs is a host array of nstripes * (data+parity) words,
 * indexed [stripe][shard]; a stripe whose status is not CFSEC_OK gets all-zero words and its buffers
 * are not touched.  The batch may mix shard sizes freely: stripes of up to 64 KiB per shard, two or
 * more, of any mix of lengths and byte alignments run as ONE kernel launch that codes and checksums
 * them (the mixed-plan launch with checksums); longer stripes and a lone small one
 * take the launches of cfsec_rs_encode_stripes and the checksum routes of cfsec_ec_encode_batch_crc.
 * CFSEC_MIX_MAX_LEN (bytes, read per call; 0: off) overrides the length limit; the results do not
 * depend on it.  An engine without parity shards checksums its data shards. */
int cfsec_rs_encode_crc_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status,
                                uint32_t* crcs);
/* Verify each stripe (KRS/reedsolomon.go:770-784): status CFSEC_OK when it holds, CFSEC_ERR_VERIFY
 * when Verify would return false (no error), another code for Verify's errors. */
int cfsec_rs_verify_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status);
/* Reconstruct each stripe (KRS/reedsolomon.go:1377-1552; missing shards need cap >= shard size and
 * get len = shard size) and, with verify != 0, Verify it afterwards, in one fused pass per stripe:
 * the kernel reads the first data_shards present shards and every other present parity shard once,
 * writes the missing ones and compares the rest (status CFSEC_ERR_VERIFY when Verify would return
 * false).  Bit-exact with the two calls on any input, consistent or not. */
int cfsec_rs_reconstruct_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int verify, int mem,
                                 int* status);
/* cfsec_rs_reconstruct_stripes(verify = 1) with every shard's checksum, the heterogeneous sibling of
 * cfsec_rs_repair_crc_batch (blobnode's repair step, work_shard_recover.go:708-771, 335-342): crcs is a
 * host array of nstripes * (data+parity) words; crcs[s * total + i] = crc32.ChecksumIEEE of shard i of
 * stripe s as it stands in memory after the call -- survivors and rebuilt shards -- for a stripe whose
 * status is CFSEC_OK or CFSEC_ERR_VERIFY, all-zero words for any other.  Stripes of up to 64 KiB per
 * shard, two or more, of any mix of lengths, byte alignments and missing sets run as ONE launch that
 * rebuilds, compares and checksums them -- RS(16, 20) stripes with at most 4 missing
 * data shards as one launch of their own, which drives the 16 x 16 dyadic product from the same kind
 * of item table; longer stripes and a lone small one (of either kind) take the launches of
 * cfsec_rs_reconstruct_stripes and a separate checksum pass.
 * CFSEC_MIX_MAX_LEN as below.  CFSEC_ERR_NOT_SUPPORTED with more than 32 data shards. */
int cfsec_rs_repair_crc_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status,
                                uint32_t* crcs);
/* reedsolomon.ReconstructData per stripe (KRS/reedsolomon.go:1377-1397, 1407-1552 with dataOnly):
 * the missing data shards only (cap >= shard size, len = shard size afterwards); missing parity
 * shards stay missing, a stripe with no data shard missing is a no-op.  status[s] is what
 * cfsec_rs_reconstruct_data returns for stripe s alone.  Segments of any mix of erasure patterns,
 * lengths and byte alignments run as one kernel launch where they are small (the mixed-plan
 * launch); CFSEC_MIX_MAX_LEN (bytes, read per call; 0: off) overrides the length limit. */
int cfsec_rs_reconstruct_data_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes, int mem, int* status);
/* ReconstructSome per stripe; required = nstripes * data_shards bytes, stripe s's mask at
 * required[s * data_shards ..].  status[s] is what cfsec_rs_reconstruct_some returns for stripe s
 * alone with that mask; small segments share the mixed-plan launch as above. */
int cfsec_rs_reconstruct_some_stripes(cfsec_rs* h, cfsec_shard* shards, int nstripes,
                                      const uint8_t* required, int mem, int* status);

/* ---------------- ec.Encoder ---------------- */
/* Code-mode table (codemode.go:26-79): fill *t for a CodeMode value; CFSEC_ERR_INVALID_CODE_MODE
 * when unknown. */
int cfsec_codemode_tactic(int codemode, cfsec_tactic* t);
/* ec.NewEncoder(Config{CodeMode, EnableVerify, Concurrency}) -- encoder.go:78-112 */
int cfsec_ec_new(const cfsec_tactic* tactic, int enable_verify, int concurrency, int device,
                 cfsec_ec** out);
void cfsec_ec_free(cfsec_ec* h);
int cfsec_ec_encode(cfsec_ec* h, cfsec_shard* shards, int n, int mem, void* stream);
int cfsec_ec_reconstruct(cfsec_ec* h, cfsec_shard* shards, int n, const int* bad_idx, int nbad,
                         int mem, void* stream);
int cfsec_ec_reconstruct_data(cfsec_ec* h, cfsec_shard* shards, int n, const int* bad_idx,
                              int nbad, int mem, void* stream);
int cfsec_ec_verify(cfsec_ec* h, cfsec_shard* shards, int n, int mem, void* stream, int* ok);
/* blobnode's repair loop over a tasklet (blobnode/work_shard_recover.go:708-771) in one call: bid b
 * is the n shards at shards[b*n ..] and its bad indices bad_idx[bad_off[b] .. bad_off[b+1]) (global
 * stripe indices, or local ones for a local stripe: n = its size); per bid exactly
 * encoder.Reconstruct(shards_b, bad_b) then, with verify != 0, encoder.Verify(shards_b).  status[b]:
 * the Reconstruct error, CFSEC_ERR_VERIFY when Verify returns false, or CFSEC_OK.  RS modes run one
 * fused Reconstruct+Verify pass; LRC modes (lrcencoder.go:133-186, 89-131) one pass too for a bid
 * with no bad local shard (its local parities compared in the global pass as rows over the data),
 * else the global pass then every AZ's local pass.  Memory and devices as for cfsec_rs_*_stripes. */
int cfsec_ec_reconstruct_batch(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                               const int* bad_off, int verify, int mem, int* status);
int cfsec_ec_set_devices(cfsec_ec* h, const int* devices, int ndev);
/* access's degraded reads as one call (stream_get.go:420-431): item i is the n shards at shards[i*n ..]
 * (each item its own segment length) with bad indices bad_idx[bad_off[i] .. bad_off[i+1]); per item
 * exactly encoder.ReconstructData(shards_i, bad_i) -- encoder.go:146-151, lrcencoder.go:188-201 (LRC
 * modes: n = N+M or N+M+L, the global bad indices only, fillFullShards over the first N+M shards).
 * status[i] is what cfsec_ec_reconstruct_data returns for item i alone; the buffers of a failed item
 * are not touched, an item with no bad data shard is a no-op, nothing but the bad data shards is
 * written (bad parity shards keep len 0).  One concurrency slot for the call; synchronous, no checksum
 * form.  Memory and devices as for cfsec_rs_*_stripes; launches as cfsec_rs_reconstruct_data_stripes. */
int cfsec_ec_reconstruct_data_batch(cfsec_ec* h, cfsec_shard* shards, int n, int nitems, const int* bad_idx,
                                    const int* bad_off, int mem, int* status);
/* access's Put over a batch of blobs (stream_put.go:104-143 encodes them one by one): for stripe s
 * (the n shards at shards[s*n ..]) exactly encoder.Encode(shards_s), EnableVerify included; LRC
 * modes as one fused (M+L) x N pass (lrcencoder.go:35-82).  status[s]: Encode's result (CFSEC_ERR_VERIFY
 * when the enabled Verify fails).  Memory and devices as for cfsec_rs_*_stripes. */
int cfsec_ec_encode_batch(cfsec_ec* h, cfsec_shard* shards, int n, int nstripes, int mem, int* status);
/* The two batch calls above returning the shard checksums CubeFS takes right after coding
 * (crc32.ChecksumIEEE): crcs is a host array of nstripes * n (nbids * n) words, indexed
 * [item][shard].  Encode: every shard of the stripe after the Encode (access/stream_put.go:249-253).
 * Reconstruct: the shards the call rebuilt -- global or local, data or parity -- (blobnode's
 * ShardCrc32 of each repaired shard, blobnode/work_shard_recover.go:335-342), 0 for the others.
 * Items whose status is not CFSEC_OK get all-zero words.  Computed on the GPU from the rows the
 * product wrote (device or staged copies), before they leave HBM.  CFSEC_ERR_NOT_SUPPORTED for
 * shapes with more than 32 inputs and Verify.  An encoder without parity shards (M == 0) has nothing to
 * encode: its data shards are checksummed (such a call used to fail: the empty product launch
 * was an invalid argument). */
int cfsec_ec_encode_batch_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nstripes, int mem, int* status,
                              uint32_t* crcs);
int cfsec_ec_reconstruct_batch_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                                   const int* bad_off, int verify, int mem, int* status, uint32_t* crcs);
/* cfsec_ec_encode_batch_crc for a put batch whose blobs differ in size (a blob smaller than the blob
 * size is one stripe of its own shard size, so a batch gathered across requests is mostly small
 * stripes of different lengths): the same contract word for word -- RS modes and LRC modes as one
 * fused (M+L) x N pass, status[s], all-zero words for a failed stripe, EnableVerify honoured (its
 * Verify pass runs as in cfsec_ec_encode_batch_crc) -- but the stripes of up to 64 KiB per shard, two
 * or more, share ONE launch that codes them and checksums every shard, whatever their lengths and
 * alignments, where cfsec_ec_encode_batch_crc takes a product launch per 18 EC12P4 stripes and a
 * checksum launch per distinct length.  Longer stripes and a lone small one keep that call's routes.
 * CFSEC_MIX_MAX_LEN as for cfsec_rs_reconstruct_data_stripes.  Call it for a put batch of 16 or more blobs that
 * differ in size; a batch of equal-size blobs, and a handful of blobs (two blobs cost 10-17 us more per
 * call here), are served best by cfsec_ec_encode_batch_crc. */
int cfsec_ec_encode_blobs_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nstripes, int mem, int* status,
                              uint32_t* crcs);
/* blobnode's repair of a tasklet with the checksum work around it (work_shard_recover.go:654-685,
 * 751-760, 335-342): per bid Reconstruct then Verify as cfsec_ec_reconstruct_batch(verify = 1), and
 * crcs[b*n + i] = crc32.ChecksumIEEE of shard i as it stands in the caller's memory after the call --
 * survivors and rebuilt shards, global and local -- for every bid whose status is CFSEC_OK or
 * CFSEC_ERR_VERIFY; all-zero words for a bid with any other status.  expect (host, nbids*n words, may
 * be NULL): the checksum each survivor came with; mismatch[b] (may be NULL when expect is) = the
 * lowest index of a survivor (a shard outside bad_b) whose word differs, or -1.  status[] keeps the
 * meaning it has in cfsec_ec_reconstruct_batch.  CFSEC_ERR_NOT_SUPPORTED as for the _crc form.
 * The survivors are read once: the pass that rebuilds and compares also checksums them, where a fused
 * kernel covers the shape (RS decode jobs of k in {6,8,12,16,18} with 2..6 rebuilt + compared rows,
 * device or page-locked memory, one shard size per bad set); elsewhere a separate checksum pass
 * gives the same words.  So the survivors' check runs after Reconstruct, not before it: a bid with
 * mismatch[b] >= 0 has been rebuilt from a corrupt survivor and must be discarded, as one that
 * failed its download check. */
int cfsec_ec_repair_batch_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                              const int* bad_off, int mem, int* status, uint32_t* crcs, const uint32_t* expect,
                              int* mismatch);
/* cfsec_ec_repair_batch_crc for a tasklet whose bids differ in size (the bids are whatever blobs lived
 * on the broken disk: most are smaller than the blob size, one stripe each of its own shard size): the
 * same contract word for word -- RS and LRC modes, status[], crcs kept for CFSEC_OK and
 * CFSEC_ERR_VERIFY, expect / mismatch -- but the bids of up to 64 KiB per shard, two or more, share ONE
 * launch that rebuilds, compares and checksums them (the mixed-plan launch with Verify, DESIGN.md
 * §4.5), whatever their sizes, byte alignments and bad sets, where cfsec_ec_repair_batch_crc takes a
 * product launch per bad set and a checksum launch per distinct length.  A compared survivor's word is
 * the checksum of the shard as it stands in memory, corrupt or not.  An LRC bid with no bad local
 * shard has its local parities compared and checksummed in that launch too.  Bids whose repair is the
 * 16 x 16 dyadic product (the 16 + 20 code with at most 4 missing data shards: most repairs of
 * EC16P20L2) share a second launch of the same kind, which computes that product from one read of the
 * bid's 16 inputs (DESIGN.md §4.5 "The 16 + 20 code"); two or more such bids make one, a lone one keeps
 * the old route.  These keep the routes of cfsec_ec_repair_batch_crc, with the same results: longer
 * bids and a lone small one; LRC bids with a bad local shard (two checksummed passes per bid).
 * Synchronous only.  CFSEC_MIX_MAX_LEN as for
 * cfsec_rs_reconstruct_data_stripes.  Call it for a tasklet of 16 or more bids that differ in size
 * (measured on one MI355X: 2.2-6.8 times faster per bid in HBM, 2.0-3.2 times on page-locked shards,
 * DESIGN.md §4.5); smaller tasklets were not measured, and a tasklet of equal-size bids is served by
 * cfsec_ec_repair_batch_crc. */
int cfsec_ec_repair_bids_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                             const int* bad_off, int mem, int* status, uint32_t* crcs, const uint32_t* expect,
                             int* mismatch);
/* Asynchronous forms of the two batch calls above, for device memory on the handle's (first) device:
 * the call plans the batch, enqueues its kernels on `stream` (hipStream_t; NULL = the legacy default
 * stream) and returns without waiting, so a caller overlaps the next tasklet's planning with this
 * one's kernels.  status[b] (host) receives at return what the synchronous call would report
 * except a false Verify: the shard checks and planning errors (the buffers of a failed bid are not
 * touched).  flags (device, one uint32 per bid, zeroed by the caller; may be NULL when no Verify is
 * asked for): once the stream has passed the call, flags[b] != 0 where Verify is false
 * (CFSEC_ERR_VERIFY of the synchronous call).  Missing shards' lengths are set at return, as in the
 * synchronous call; the bytes are there when the stream gets there.  The library keeps no caller
 * pointer after the call returns (the shard pointers are copied into the kernel arguments).  Shapes
 * the kernels cannot compare in one pass: more than 32 inputs with Verify (no code mode has them)
 * return CFSEC_ERR_NOT_SUPPORTED -- use the synchronous call; an LRC stripe whose local shard has
 * another length runs synchronously on `stream` and reports ErrVerify in status[b].
 * crcs (device, nbids * n / nstripes * n words, may be NULL): the checksums of the _crc forms,
 * written on the stream (zeroed by the call first); a flagged or failed item's words are
 * meaningless. */
int cfsec_ec_reconstruct_batch_async(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx,
                                     const int* bad_off, int verify, int* status, uint32_t* flags, uint32_t* crcs,
                                     void* stream);
int cfsec_ec_encode_batch_async(cfsec_ec* h, cfsec_shard* shards, int n, int nstripes, int* status, uint32_t* flags,
                                uint32_t* crcs, void* stream);
/* Repair over survivors held elsewhere (the multi-GPU repair of chubaofs_amd/repair.py ships only
 * the shards a decode reads): with the shards in bad_idx[0..nbad) lost (global or LRC local
 * indices), in_idx[0..N) = the first N present global shards in index order -- the ones
 * Reconstruct decodes from (KRS/reedsolomon.go:1453-1465) -- and rows[w*N .. w*N+N) = shard
 * want[w] (a data, global parity or local parity index) as a GF(2^8) row over them (the local
 * parity through lrcencoder.go's local engine over the AZ's shards).  No reference counterpart:
 * the reference repairs one bid at a time on one host. */
int cfsec_ec_repair_rows(cfsec_ec* h, const int* bad_idx, int nbad, const int* want, int nwant,
                         int* in_idx, uint8_t* rows);
/* outputs = coef (rows x N) x inputs over device memory, asynchronously on `stream` (NULL: the
 * legacy default stream): stripe s has N input pointers then `rows` output pointers at
 * ptrs[s*(N+rows) ..], shard_size bytes each (the product kernel of cfsec_rs_encode_batch with
 * caller rows, e.g. cfsec_ec_repair_rows'). */
int cfsec_ec_matvec_batch(cfsec_ec* h, const uint8_t* coef, int rows, uint8_t* const* ptrs, size_t shard_size,
                          int nstripes, void* stream);
/* GetShardsInIdc index map (encoder.go:169-176 / lrcencoder.go:236-243): writes the global
 * shard indices of AZ idx into out (capacity out_cap) and their count into *count. */
int cfsec_ec_shards_in_idc(const cfsec_ec* h, int idx, int* out, int out_cap, int* count);

/* ---------------- contiguous stripes (ec.Buffer's layout) ----------------
 * ec.Buffer carves a stripe's N+M+L shards at one stride from one allocation (common/ec/buf.go:
 * 83-84) and encoder.Split hands out exactly those slices (KRS/reedsolomon.go:1574-1632).  These
 * entry points take such a stripe as (base, shard_size, stride): shard i is shard_size bytes at
 * base + i * stride (stride >= shard_size), every shard present -- the broken ones are named by
 * bad_idx (ec) or missing (reedsolomon: what a len-0 shard marks in the vector forms) and rebuilt in
 * place.  One pointer per call: a Go caller passes Go memory under cgo's pointer rules as they stand
 * since Go 1.6 (no runtime.Pinner, no C array holding Go pointers), which is what CubeFS's Go 1.17
 * toolchain (go.mod:3, docker/Dockerfile:1) can build.  Semantics otherwise those of the vector
 * calls. */
int cfsec_rs_encode_contig(cfsec_rs* h, uint8_t* base, size_t shard_size, size_t stride, int n, int mem,
                           void* stream);
int cfsec_rs_verify_contig(cfsec_rs* h, uint8_t* base, size_t shard_size, size_t stride, int n, int mem,
                           void* stream, int* ok);
int cfsec_rs_reconstruct_contig(cfsec_rs* h, uint8_t* base, size_t shard_size, size_t stride, int n,
                                const int* missing, int nmissing, int data_only, int mem, void* stream);
int cfsec_ec_encode_contig(cfsec_ec* h, uint8_t* base, size_t shard_size, size_t stride, int n, int mem,
                           void* stream);
int cfsec_ec_verify_contig(cfsec_ec* h, uint8_t* base, size_t shard_size, size_t stride, int n, int mem,
                           void* stream, int* ok);
int cfsec_ec_reconstruct_contig(cfsec_ec* h, uint8_t* base, size_t shard_size, size_t stride, int n,
                                const int* bad_idx, int nbad, int data_only, int mem, void* stream);
/* Batches in one allocation: stripe s at base + s * stripe_stride (encode); bid b at
 * base + bid_off[b] with its shards packed at its own shard size bid_shard_size[b] (repair tasklet;
 * a zero-size bid is all empty shards).  crcs (host, may be NULL): the _crc forms' checksums. */
int cfsec_ec_encode_batch_contig(cfsec_ec* h, uint8_t* base, size_t shard_size, size_t stride, size_t stripe_stride,
                                 int n, int nstripes, int mem, int* status, uint32_t* crcs);
int cfsec_ec_reconstruct_batch_contig(cfsec_ec* h, uint8_t* base, const uint64_t* bid_off,
                                      const uint64_t* bid_shard_size, int n, int nbids, const int* bad_idx,
                                      const int* bad_off, int verify, int mem, int* status, uint32_t* crcs);

/* ---------------- pinned host memory ---------------- */
/* Page-locked host memory for shard buffers (the hook is resourcepool.NewMemPoolWith,
 * common/resourcepool/mempool.go:60, which ec.Buffer draws from, common/ec/buf.go:93-117).
 * CFSEC_MEM_HOST calls on such buffers DMA straight to HBM instead of through the runtime's
 * staging copies.  C memory: safe to hand to cgo. */
int cfsec_host_alloc(size_t size, void** out);
int cfsec_host_free(void* p);

/* ---------------- shard CRC32 (access/stream_put.go:249-253) ---------------- */
/* crc32.ChecksumIEEE of each device shard; out: host array of n uint32. Synchronous.
 * shard_size above 2^32 - 1 - 4096 is CFSEC_ERR_INVALID_ARG: nothing is launched or read. */
int cfsec_crc32_ieee_batch(uint8_t* const* ptrs, size_t shard_size, int n, uint32_t* out,
                           int device, void* stream);

/* Checksums of concatenations (host only, no device).  cfsec_crc32_combine: crc32.ChecksumIEEE(A || B)
 * from crc1 = ChecksumIEEE(A), crc2 = ChecksumIEEE(B) and len2 = |B| (zlib's crc32_combine).
 * cfsec_crc32_shift: words[i] <- words[i] * x^(8 nbytes) mod P, i.e. the term a byte range's checksum
 * contributes to the checksum of a longer run that continues for nbytes more bytes: the checksum of a
 * shard cut into column slices is the XOR of its slices' shifted checksums (the multi-GPU repair's
 * rebuilt shards, chubaofs_amd/repair.py; blobnode's ShardCrc32, blobnode/work_shard_recover.go:335-342). */
uint32_t cfsec_crc32_combine(uint32_t crc1, uint32_t crc2, int64_t len2);
int cfsec_crc32_shift(uint32_t* words, int n, int64_t nbytes);

/* Measurement helper (no reference counterpart): a flat grid-stride copy of `bytes` bytes (a
 * multiple of 16; both pointers device memory, 16-byte aligned) with non-temporal 16-byte loads and
 * stores, asynchronous on `stream` -- the device's streaming ceiling for a 1:1 read/write pattern,
 * which bench.py reports beside the HBM spec peak (tools/rot_probe.hip measured this form at 72-75 %
 * of 8 TB/s, above the HIP runtime's own copy). */
int cfsec_stream_copy(void* dst, const void* src, size_t bytes, void* stream);

/* ---------------- crc32block framing (blobstore/common/crc32block) ---------------- */
/* A framed object is a run of block_len-byte blocks (default 64 KiB; block_len a positive multiple
 * of 4096), each the little-endian crc32.ChecksumIEEE of its payload followed by the payload
 * (block_len - 4 bytes; fewer in the last block) -- block.go:34-49, encode.go:87-109.
 * Sizes: EncodeSize / DecodeSize (util.go:50-65); -1 when block_len is invalid (the Go functions
 * panic with ErrInvalidBlock) or the size is negative. */
int64_t cfsec_crc32block_encode_size(int64_t size, int64_t block_len);
int64_t cfsec_crc32block_decode_size(int64_t total, int64_t block_len);
/* Encoder.Encode (encode.go:48-58, blobnode core/storage/datafile.go:345-373): frame `size` payload
 * bytes of src into dst (cfsec_crc32block_encode_size bytes).  shard_crc (host, may be NULL)
 * receives crc32.ChecksumIEEE of the whole payload, which datafile.go:345-373 computes on the way
 * (shard.Crc).  One pass: every payload byte is read once and written once.  mem as for cfsec_rs_*:
 * CFSEC_MEM_DEVICE pointers run on `stream` (NULL = an internal stream) on `device` (-1 = current);
 * CFSEC_MEM_HOST buffers from cfsec_host_alloc are read and written in place, other host memory is
 * staged through HBM.  Returns after completion. */
int cfsec_crc32block_encode(const uint8_t* src, int64_t size, int64_t block_len, uint8_t* dst,
                            uint32_t* shard_crc, int mem, int device, void* stream);
/* Decoder.Reader(from, to) (decode.go:122-146; blobnode datafile.go:406-426): check the blocks of
 * the framed object src (src_len bytes readable; payload size `size`) that hold payload bytes
 * [from, to) -- and the block holding `from` when from == to is not block-aligned, as the
 * reference's skip does -- and copy those bytes to dst (to - from bytes; may be NULL when
 * from == to).  CFSEC_ERR_SHORT_DATA, before anything is read, when src_len ends before the last
 * touched block (the reference's SectionReader gives io.ErrUnexpectedEOF).
 * CFSEC_ERR_MISMATCHED_CRC when a checked block's checksum differs; *bad_block (may be NULL) =
 * index of the first such block, -1 otherwise. */
int cfsec_crc32block_decode(const uint8_t* src, int64_t src_len, int64_t size, int64_t block_len, int64_t from,
                            int64_t to, uint8_t* dst, int64_t* bad_block, int mem, int device, void* stream);
/* Batch forms on device memory, asynchronous on `stream` (NULL = the null stream): n objects of one
 * payload size -- the shards of a stripe batch (blobnode puts and repairs); decode: every source
 * object has at least src_len readable bytes (CFSEC_ERR_SHORT_DATA otherwise, as above).  encode: shard_crcs
 * (device, n words, may be NULL) receives each payload's crc32.ChecksumIEEE.  decode: checks and
 * unframes payload range [from, to) of each object; bad (device, n words) receives per object the
 * index of the first mismatching block counted from block from / (block_len - 4), or 0xFFFFFFFF. */
int cfsec_crc32block_encode_batch(const uint8_t* const* srcs, uint8_t* const* dsts, int n, int64_t size,
                                  int64_t block_len, uint32_t* shard_crcs, void* stream);
int cfsec_crc32block_decode_batch(const uint8_t* const* srcs, int64_t src_len, uint8_t* const* dsts, int n,
                                  int64_t size, int64_t block_len, int64_t from, int64_t to, uint32_t* bad,
                                  void* stream);

/* Many framed objects of different payload sizes, ranges and alignments in one launch (blobnode's data
 * inspect, datainspect.go:95-130; the rebuilt shards of a repair tasklet, datafile.go:345-373; concurrent
 * range Gets, datafile.go:393-427).  One block_len per call; n is not bounded. */
typedef struct cfsec_blk_object {
  const uint8_t* src; /* check/decode: framed object; encode: payload */
  int64_t src_len;    /* check/decode: readable framed bytes; encode: ignored */
  uint8_t* dst;       /* decode: to - from bytes; encode: EncodeSize(size) bytes; check: ignored */
  int64_t size;       /* payload bytes of this object */
  int64_t from, to;   /* check/decode: payload range, Decoder.Reader(from, to); encode: ignored */
} cfsec_blk_object;
/* The contract is the single call's, per object: status[i] (host, n entries) is what
 * cfsec_crc32block_decode / _encode returns for object i alone -- CFSEC_OK, CFSEC_ERR_MISMATCHED_CRC,
 * CFSEC_ERR_SHORT_DATA (src_len ends before the last touched block: decided on the host, nothing of
 * that object is read) or CFSEC_ERR_INVALID_ARG (a bad range, a negative size, a NULL pointer where one
 * is needed).  bad_block[i] (host, may be NULL) is the absolute index of the object's first mismatching
 * block, -1 otherwise.  A bad object never changes a neighbour's result and the call still returns
 * CFSEC_OK; the return value speaks for the whole call only: CFSEC_ERR_INVALID_BLOCK for an invalid
 * block_len, CFSEC_ERR_INVALID_ARG for n < 0, a NULL o (n > 0) or status, or an unknown mem,
 * CFSEC_ERR_DEVICE for a HIP error.  The checked blocks are exactly those Decoder.Reader(from, to)
 * touches (from == to inside a block: that block); a size-0 object is CFSEC_OK with nothing launched.
 *   check   verifies the blocks and writes no payload: no destination, every block read once
 *   decode  verifies and copies payload [from, to) to dst
 *   encode  frames `size` bytes of src into dst
 * shard_crc[i] (host, may be NULL) is crc32.ChecksumIEEE of the whole payload: always on encode; on
 * check and decode when [from, to) == [0, size) and the object is CFSEC_OK, else 0.
 * Synchronous.  CFSEC_MEM_DEVICE runs in place on `stream` (NULL = the engine's stream, ordered after
 * the null stream); CFSEC_MEM_HOST with every object in cfsec_host_alloc memory runs in place; any other
 * host memory is staged through HBM, runs of objects at a time (correct, not a fast path). */
int cfsec_crc32block_check_objects(const cfsec_blk_object* o, int n, int64_t block_len, int* status,
                                   int64_t* bad_block, uint32_t* shard_crc, int mem, int device, void* stream);
int cfsec_crc32block_decode_objects(const cfsec_blk_object* o, int n, int64_t block_len, int* status,
                                    int64_t* bad_block, uint32_t* shard_crc, int mem, int device, void* stream);
int cfsec_crc32block_encode_objects(const cfsec_blk_object* o, int n, int64_t block_len, int* status,
                                    uint32_t* shard_crc, int mem, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFSEC_H_ */
