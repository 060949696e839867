// Package cfsec is the cgo binding a CubeFS maintainer drops into
// blobstore/common/ec to run the EC engine on MI355X GPUs.
//
// It implements github.com/klauspost/reedsolomon.Encoder (the seam that
// blobstore/common/ec/encoder.go:86 and :95 construct) over the C ABI in
// include/cfsec.h.  The coding methods go to libcfsec.so -- Encode, Verify, Reconstruct,
// ReconstructData, and EncodeIdx, ReconstructSome and Update, which today's CubeFS does not call --
// while Split and Join (host bookkeeping, no coding) stay in Go as the reference writes them.
//
// Go releases.  CubeFS builds with Go 1.17 (go.mod:3, docker/Dockerfile:1), whose cgo rules forbid a
// C array holding Go pointers.  So every call first looks for the one-allocation layout that
// ec.Buffer and Split produce (stripeOf: shard i at base + i*stride, inside one buffer registered
// with RegisterBuffer or allocated by HostAlloc) and passes that stripe as a single pointer to the
// cfsec_*_contig entry points -- legal on every Go release.  Any other shard vector goes through
// callVec: shards in HostAlloc memory are C memory and go into the C array as they are; Go memory is
// pinned with Go >= 1.21 (runtime.Pinner, vec_pin.go) and staged through C memory before that
// (vec_copy.go).
//
// Source only: this container has no Go toolchain, so the package is not built or
// tested here (see INTEGRATION.md for the build line and the test plan).
package cfsec

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../chubaofs_amd -lcfsec -Wl,-rpath,${SRCDIR}/../../chubaofs_amd
#include <stdlib.h>
#include "cfsec.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"io"
	"runtime"
	"sync/atomic"
	"unsafe"

	"github.com/klauspost/reedsolomon"
)

// stripeOf reports whether every shard is size bytes at one stride from the first (ec.Buffer's
// layout, common/ec/buf.go:83-84, which encoder.Split carves) inside one registered allocation
// (regions.go: RegisterBuffer, HostAlloc): then the stripe crosses the C ABI as its base pointer
// alone (cfsec_*_contig).  Shards that only happen to sit at one stride are not enough -- cgo lets C
// reach the allocation a pointer points into, nothing beyond it.
func stripeOf(shards [][]byte) (base *C.uint8_t, size, stride int, ok bool) {
	if len(shards) == 0 || len(shards[0]) == 0 {
		return nil, 0, 0, false
	}
	size = len(shards[0])
	p0 := uintptr(unsafe.Pointer(&shards[0][0]))
	stride = size
	if len(shards) > 1 && len(shards[1]) == size {
		stride = int(uintptr(unsafe.Pointer(&shards[1][0])) - p0)
	}
	if stride < size {
		return nil, 0, 0, false
	}
	for i, s := range shards {
		if len(s) != size || uintptr(unsafe.Pointer(&s[0])) != p0+uintptr(i*stride) {
			return nil, 0, 0, false
		}
	}
	if _, one := regionOf(p0, (len(shards)-1)*stride+size); !one {
		// an equal-stride stripe outside every registered allocation (an ec.Buffer nobody passed
		// to RegisterBuffer): it still works, through callVec -- on Go < 1.21 that stages every
		// shard through C memory, two host copies per call.  Counted, so an integration that
		// forgot RegisterBuffer sees it (UnregisteredStripes).
		atomic.AddUint64(&unregisteredStripes, 1)
		return nil, 0, 0, false
	}
	return (*C.uint8_t)(unsafe.Pointer(&shards[0][0])), size, stride, true
}

var unregisteredStripes uint64

// UnregisteredStripes is the number of calls so far whose shards formed one equal-stride stripe
// (ec.Buffer's layout) that lay in no RegisterBuffer / HostAlloc region, so it missed the single-
// pointer zero-copy path.  Nonzero means some ec.Buffer allocation should be registered.
func UnregisteredStripes() uint64 { return atomic.LoadUint64(&unregisteredStripes) }

// stripeOfMissing is stripeOf for a Reconstruct input: a missing shard (len 0) counts when its
// capacity holds the shard at its place in the stripe; missing lists those indices.
func stripeOfMissing(shards [][]byte) (base *C.uint8_t, size, stride int, missing []C.int, ok bool) {
	first := -1
	for i, s := range shards {
		if len(s) != 0 {
			first, size = i, len(s)
			break
		}
	}
	if first < 0 {
		return nil, 0, 0, nil, false
	}
	addr := make([]uintptr, len(shards))
	for i, s := range shards {
		switch {
		case len(s) == size:
			addr[i] = uintptr(unsafe.Pointer(&s[0]))
		case len(s) == 0 && cap(s) >= size:
			addr[i] = uintptr(unsafe.Pointer(&s[:1][0]))
			missing = append(missing, C.int(i))
		default:
			return nil, 0, 0, nil, false
		}
	}
	stride = size
	if len(shards) > 1 {
		stride = int(addr[1] - addr[0])
	}
	if stride < size {
		return nil, 0, 0, nil, false
	}
	for i := range shards {
		if addr[i] != addr[0]+uintptr(i*stride) {
			return nil, 0, 0, nil, false
		}
	}
	if _, one := regionOf(addr[0], (len(shards)-1)*stride+size); !one {
		return nil, 0, 0, nil, false
	}
	return (*C.uint8_t)(unsafe.Pointer(addr[0])), size, stride, missing, true
}

func cints(v []int) ([]C.int, *C.int) {
	if len(v) == 0 {
		return nil, nil
	}
	c := make([]C.int, len(v))
	for i, x := range v {
		c[i] = C.int(x)
	}
	return c, &c[0]
}

// Engine is a reedsolomon.Encoder whose arithmetic runs on a GPU.
type Engine struct {
	h            *C.cfsec_rs
	dataShards   int
	parityShards int
}

var _ reedsolomon.Encoder = (*Engine)(nil)

// ErrDevice reports a HIP runtime failure (no device, out of memory, ...).
var ErrDevice = errors.New("cfsec: device error")

var errInvalidArg = errors.New("cfsec: invalid argument")

// toError maps cfsec_status codes back onto the Go sentinels (include/cfsec.h).
func toError(st C.int) error {
	switch st {
	case C.CFSEC_OK:
		return nil
	case C.CFSEC_ERR_TOO_FEW_SHARDS:
		return reedsolomon.ErrTooFewShards
	case C.CFSEC_ERR_SHARD_NO_DATA:
		return reedsolomon.ErrShardNoData
	case C.CFSEC_ERR_SHARD_SIZE:
		return reedsolomon.ErrShardSize
	case C.CFSEC_ERR_INV_SHARD_NUM:
		return reedsolomon.ErrInvShardNum
	case C.CFSEC_ERR_MAX_SHARD_NUM:
		return reedsolomon.ErrMaxShardNum
	case C.CFSEC_ERR_SHORT_DATA:
		return reedsolomon.ErrShortData
	case C.CFSEC_ERR_RECONSTRUCT_REQUIRED:
		return reedsolomon.ErrReconstructRequired
	case C.CFSEC_ERR_NOT_SUPPORTED:
		return reedsolomon.ErrNotSupported
	case C.CFSEC_ERR_INVALID_INPUT:
		return reedsolomon.ErrInvalidInput
	case C.CFSEC_ERR_DEVICE:
		return fmt.Errorf("%w: %s", ErrDevice, C.GoString(C.cfsec_last_error()))
	case C.CFSEC_ERR_SINGULAR:
		return errors.New("matrix is singular")
	default:
		return fmt.Errorf("%w: %s", errInvalidArg, C.GoString(C.cfsec_status_name(st)))
	}
}

// New mirrors reedsolomon.New(dataShards, parityShards) with default options.
func New(dataShards, parityShards int) (*Engine, error) {
	var h *C.cfsec_rs
	if err := toError(C.cfsec_rs_new(C.int(dataShards), C.int(parityShards), -1, &h)); err != nil {
		return nil, err
	}
	e := &Engine{h: h, dataShards: dataShards, parityShards: parityShards}
	runtime.SetFinalizer(e, func(e *Engine) { C.cfsec_rs_free(e.h) })
	return e, nil
}

func (e *Engine) Encode(shards [][]byte) error {
	if base, size, stride, ok := stripeOf(shards); ok {
		return toError(C.cfsec_rs_encode_contig(e.h, base, C.size_t(size), C.size_t(stride), C.int(len(shards)),
			C.CFSEC_MEM_HOST, nil))
	}
	return toError(callVec(shards, func(v *C.cfsec_shard, n C.int) C.int {
		return C.cfsec_rs_encode(e.h, v, n, C.CFSEC_MEM_HOST, nil)
	}))
}

// EncodeCRC is Encode followed by crc32.ChecksumIEEE of every shard -- what access computes
// right after encoding (blobstore/access/stream_put.go:249-253) -- in one fused GPU pass.
func (e *Engine) EncodeCRC(shards [][]byte) ([]uint32, error) {
	crcs := make([]uint32, len(shards)+1) // +1: a valid address even for an empty vector
	st := callVec(shards, func(v *C.cfsec_shard, n C.int) C.int {
		return C.cfsec_rs_encode_crc(e.h, v, n, C.CFSEC_MEM_HOST, nil, (*C.uint32_t)(unsafe.Pointer(&crcs[0])))
	})
	return crcs[:len(shards)], toError(st)
}

// HostAlloc returns size bytes of page-locked C memory (cfsec_host_alloc) as a byte slice: the
// allocation hook for resourcepool.NewMemPoolWith (common/resourcepool/mempool.go:60), so
// ec.Buffer shards are coded in place over PCIe, and for blobnode's shard buffers
// (blobnode/base/workutils/buf_pool.go:26-29).  The block is registered as one region (regions.go):
// its stripes take the one-pointer entry points and its shards sit in C arrays without staging or
// pinning on every Go release.  Release it with HostFree.
func HostAlloc(size int) ([]byte, error) {
	if size <= 0 {
		return nil, nil
	}
	var p unsafe.Pointer
	if err := toError(C.cfsec_host_alloc(C.size_t(size), &p)); err != nil {
		return nil, err
	}
	b := unsafe.Slice((*byte)(p), size)
	addRegion(b, true)
	return b, nil
}

// HostFree releases a slice from HostAlloc.
func HostFree(b []byte) error {
	if cap(b) == 0 {
		return nil
	}
	removeRegion(b)
	return toError(C.cfsec_host_free(unsafe.Pointer(&b[:1][0])))
}

func (e *Engine) Verify(shards [][]byte) (bool, error) {
	ok := make([]C.int, 1)
	if base, size, stride, contig := stripeOf(shards); contig {
		err := toError(C.cfsec_rs_verify_contig(e.h, base, C.size_t(size), C.size_t(stride), C.int(len(shards)),
			C.CFSEC_MEM_HOST, nil, &ok[0]))
		return ok[0] != 0, err
	}
	err := toError(callVec(shards, func(v *C.cfsec_shard, n C.int) C.int {
		return C.cfsec_rs_verify(e.h, v, n, C.CFSEC_MEM_HOST, nil, &ok[0])
	}))
	return ok[0] != 0, err
}

// prepareMissing gives the shards KRS's reconstruct rebuilds a buffer of the shard size when their
// capacity is short, as KRS/reedsolomon.go:1514-1518 and :1539-1543 do (reuse cap, else a 64-byte
// aligned allocation) -- and only those: nothing when the stripe is complete (or, for
// ReconstructData, its data is), nothing when too few shards are present (ErrTooFewShards comes
// first, :1418-1441), and no parity shard for ReconstructData.  The C side writes into cap only.
func prepareMissing(shards [][]byte, dataShards int, dataOnly bool) {
	size, present, dataPresent := 0, 0, 0
	for i, s := range shards {
		if len(s) != 0 {
			if size == 0 {
				size = len(s)
			}
			present++
			if i < dataShards {
				dataPresent++
			}
		}
	}
	if size == 0 || present == len(shards) || present < dataShards || (dataOnly && dataPresent == dataShards) {
		return
	}
	for i, s := range shards {
		if dataOnly && i >= dataShards {
			break
		}
		if len(s) == 0 && cap(s) < size {
			shards[i] = reedsolomon.AllocAligned(1, size)[0][:0]
		}
	}
}

func (e *Engine) reconstruct(shards [][]byte, dataOnly bool) error {
	donly := C.int(0)
	if dataOnly {
		donly = 1
	}
	// ec.Buffer's stripe with some shards marked missing: one pointer, rebuilt in place
	if base, size, stride, missing, ok := stripeOfMissing(shards); ok && len(shards) == e.dataShards+e.parityShards {
		var mp *C.int
		if len(missing) > 0 {
			mp = &missing[0]
		}
		err := toError(C.cfsec_rs_reconstruct_contig(e.h, base, C.size_t(size), C.size_t(stride), C.int(len(shards)),
			mp, C.int(len(missing)), donly, C.CFSEC_MEM_HOST, nil))
		if err == nil {
			// the rebuilt shards get their length, as KRS/reedsolomon.go:1514-1518 and :1539-1543 do
			present := len(shards) - len(missing)
			dataPresent := 0
			for i := 0; i < e.dataShards; i++ {
				if len(shards[i]) != 0 {
					dataPresent++
				}
			}
			if present < len(shards) && !(dataOnly && dataPresent == e.dataShards) {
				for _, i := range missing {
					if !dataOnly || int(i) < e.dataShards {
						shards[i] = shards[i][:size]
					}
				}
			}
		}
		return err
	}
	prepareMissing(shards, e.dataShards, dataOnly)
	return toError(callVec(shards, func(v *C.cfsec_shard, n C.int) C.int {
		if dataOnly {
			return C.cfsec_rs_reconstruct_data(e.h, v, n, C.CFSEC_MEM_HOST, nil)
		}
		return C.cfsec_rs_reconstruct(e.h, v, n, C.CFSEC_MEM_HOST, nil)
	}))
}

func (e *Engine) Reconstruct(shards [][]byte) error { return e.reconstruct(shards, false) }

func (e *Engine) ReconstructData(shards [][]byte) error { return e.reconstruct(shards, true) }

// Split and Join are host bookkeeping -- slice headers, a zero fill, one copy of the partial tail --
// with no coding arithmetic, so the shim keeps them in Go (KRS/reedsolomon.go:1574-1684) rather
// than sending Go memory through C: the C ABI's cfsec_rs_split / cfsec_rs_join run the same
// algorithm for C callers (pinned by tests/test_capi.py), but a C function that writes addresses of
// Go buffers into an array outlives the cgo call's pointer rules, and a Join through C costs two
// copies of the object where the reference writes the shard slices straight to dst.

// Split: the data shards are views of data itself (its spare capacity zeroed and used), the shards
// past the end of data come from AllocAligned (64-byte aligned, stride and capacity rounded up to
// 64), the bytes after the last full shard copied into them in order.
func (e *Engine) Split(data []byte) ([][]byte, error) {
	n := len(data)
	if n == 0 {
		return nil, reedsolomon.ErrShortData
	}
	tot := e.dataShards + e.parityShards
	if tot == 1 {
		return [][]byte{data}, nil
	}
	per := (n + e.dataShards - 1) / e.dataShards
	// usable bytes of data: its length, or its capacity up to tot*per (zeroed past the length)
	usable := n
	if c := cap(data); c > n {
		usable = tot * per
		if c < usable {
			usable = c
		}
		tail := data[n:usable]
		for i := range tail {
			tail[i] = 0
		}
	}
	buf := data[:usable]
	inPlace := usable / per
	if inPlace > tot {
		inPlace = tot
	}
	out := make([][]byte, tot)
	for i := 0; i < inPlace; i++ {
		out[i] = buf[i*per : (i+1)*per : (i+1)*per]
	}
	if inPlace < tot {
		pad := reedsolomon.AllocAligned(tot-inPlace, per)
		var rest []byte
		if inPlace*per < n {
			rest = data[inPlace*per : n]
		}
		for j := range pad {
			rest = rest[copy(pad[j], rest):]
			out[inPlace+j] = pad[j]
		}
	}
	return out, nil
}

// Join: ErrTooFewShards, ErrReconstructRequired (a nil data shard before outSize bytes are covered)
// and ErrShortData are decided before anything is written or allocated; then one Write per data
// shard, the last cut at outSize.
func (e *Engine) Join(dst io.Writer, shards [][]byte, outSize int) error {
	if len(shards) < e.dataShards {
		return reedsolomon.ErrTooFewShards
	}
	data := shards[:e.dataShards]
	have := 0
	for _, s := range data {
		if s == nil {
			return reedsolomon.ErrReconstructRequired
		}
		if have += len(s); have >= outSize {
			break
		}
	}
	if have < outSize {
		return reedsolomon.ErrShortData
	}
	left := outSize
	for _, s := range data {
		if left < len(s) {
			_, err := dst.Write(s[:left])
			return err
		}
		w, err := dst.Write(s)
		if err != nil {
			return err
		}
		left -= w
	}
	return nil
}

// vecAt is entry i of a C shard vector.
func vecAt(v *C.cfsec_shard, i int) *C.cfsec_shard {
	return (*C.cfsec_shard)(unsafe.Add(unsafe.Pointer(v), uintptr(i)*unsafe.Sizeof(*v)))
}

// EncodeIdx -- KRS/reedsolomon.go:631-667: parity[r] ^= M[k+r][idx] * dataShard.  The data shard and
// the parity shards cross the ABI as one vector (callVec pins or stages one vector per call); a nil
// and an empty slice both arrive as len == 0.
func (e *Engine) EncodeIdx(dataShard []byte, idx int, parity [][]byte) error {
	all := append([][]byte{dataShard}, parity...)
	return toError(callVec(all, func(v *C.cfsec_shard, n C.int) C.int {
		return C.cfsec_rs_encode_idx(e.h, v, C.int(idx), vecAt(v, 1), n-1, C.CFSEC_MEM_HOST, nil)
	}))
}

// ReconstructSome -- KRS/reedsolomon.go:1395-1397: the missing data shards with required[i] only.
// Those shards get a buffer of the shard size when their capacity is short (as prepareMissing does
// for ReconstructData), and only when the call will rebuild something.
func (e *Engine) ReconstructSome(shards [][]byte, required []bool) error {
	if required == nil {
		return e.reconstruct(shards, true)
	}
	if len(shards) != e.dataShards+e.parityShards || len(required) < e.dataShards {
		return reedsolomon.ErrTooFewShards
	}
	req := make([]byte, len(required))
	size, present, dataPresent, missingRequired := 0, 0, 0, 0
	for i, s := range shards {
		if i < len(required) && required[i] {
			req[i] = 1
		}
		if len(s) != 0 {
			if size == 0 {
				size = len(s)
			}
			present++
			if i < e.dataShards {
				dataPresent++
			}
		} else if i < len(req) && req[i] != 0 {
			missingRequired++
		}
	}
	if size != 0 && present < len(shards) && dataPresent < e.dataShards && missingRequired > 0 && present >= e.dataShards {
		for i := 0; i < e.dataShards; i++ {
			if len(shards[i]) == 0 && req[i] != 0 && cap(shards[i]) < size {
				shards[i] = reedsolomon.AllocAligned(1, size)[0][:0]
			}
		}
	}
	return toError(callVec(shards, func(v *C.cfsec_shard, n C.int) C.int {
		return C.cfsec_rs_reconstruct_some(e.h, v, n, (*C.uint8_t)(unsafe.Pointer(&req[0])), C.int(len(req)),
			C.CFSEC_MEM_HOST, nil)
	}))
}

// Update -- KRS/reedsolomon.go:672-734.  As in the reference, a changed entry of shards is left
// holding old ^ new.  The two vectors cross the ABI as one; a nil and an empty slice both arrive as
// len == 0 (include/cfsec.h).
func (e *Engine) Update(shards [][]byte, newDatashards [][]byte) error {
	all := append(append([][]byte{}, shards...), newDatashards...)
	ns := len(shards)
	return toError(callVec(all, func(v *C.cfsec_shard, n C.int) C.int {
		return C.cfsec_rs_update(e.h, v, C.int(ns), vecAt(v, ns), n-C.int(ns), C.CFSEC_MEM_HOST, nil)
	}))
}

// ---- crc32block framing (blobstore/common/crc32block) ----

// ErrMismatchedCrc / ErrInvalidBlock mirror crc32block's sentinels (common/crc32block/util.go:29-30);
// a shim dropped into crc32block returns that package's own values instead.
var (
	ErrMismatchedCrc = errors.New("crc32block: mismatched checksum")
	ErrInvalidBlock  = errors.New("crc32block: invalid block buffer")
)

// BlockEncode frames payload in blockLen-byte crc32block blocks (crc32block.Encoder.Encode,
// encode.go:48-58) on the GPU and returns the framed bytes together with crc32.ChecksumIEEE of the
// whole payload -- the shard checksum blobnode's datafile.Write takes on the way
// (core/storage/datafile.go:345-373) -- from the same single pass.
func BlockEncode(payload []byte, blockLen int64) ([]byte, uint32, error) {
	total := int64(C.cfsec_crc32block_encode_size(C.int64_t(len(payload)), C.int64_t(blockLen)))
	if total < 0 {
		return nil, 0, ErrInvalidBlock
	}
	out := make([]byte, total)
	if len(payload) == 0 {
		return out, 0, nil
	}
	crc := make([]C.uint32_t, 1)
	// Go pointers passed as arguments to memory holding no Go pointers: legal without pinning
	st := C.cfsec_crc32block_encode((*C.uint8_t)(unsafe.Pointer(&payload[0])), C.int64_t(len(payload)),
		C.int64_t(blockLen), (*C.uint8_t)(unsafe.Pointer(&out[0])), &crc[0], C.CFSEC_MEM_HOST, -1, nil)
	if st == C.CFSEC_ERR_INVALID_BLOCK {
		return nil, 0, ErrInvalidBlock
	}
	return out, uint32(crc[0]), toError(st)
}

// BlockDecode returns payload bytes [from, to) of a framed object whose payload is size bytes,
// checking every block the range touches (crc32block.Decoder.Reader, decode.go:122-146).
func BlockDecode(framed []byte, size, from, to, blockLen int64) ([]byte, error) {
	if from < 0 || from > to || to > size {
		return nil, errInvalidArg
	}
	out := make([]byte, to-from)
	var src, dst *C.uint8_t
	if len(framed) > 0 {
		src = (*C.uint8_t)(unsafe.Pointer(&framed[0]))
	}
	if len(out) > 0 {
		dst = (*C.uint8_t)(unsafe.Pointer(&out[0]))
	}
	bad := make([]C.int64_t, 1)
	switch st := C.cfsec_crc32block_decode(src, C.int64_t(len(framed)), C.int64_t(size), C.int64_t(blockLen),
		C.int64_t(from), C.int64_t(to), dst, &bad[0], C.CFSEC_MEM_HOST, -1, nil); st {
	case C.CFSEC_ERR_MISMATCHED_CRC:
		return nil, ErrMismatchedCrc
	case C.CFSEC_ERR_INVALID_BLOCK:
		return nil, ErrInvalidBlock
	case C.CFSEC_ERR_SHORT_DATA:
		// the framed object ends before the blocks the range touches: what the reference's
		// SectionReader reports (decode.go:94-97, 126-130)
		return nil, io.ErrUnexpectedEOF
	default:
		return out, toError(st)
	}
}

// ---- crc32block over many objects of different sizes (cfsec_crc32block_*_objects) ----

// BlockObject is one framed object of a BlockCheckObjects, BlockDecodeObjects or BlockEncodeObjects
// call.  Src is the framed object (check, decode) or the payload (encode); Size is the payload size of
// a framed object (encode takes len(Src)); [From, To) is the payload range Decoder.Reader(from, to)
// would read (check, decode).  Dst, when not nil, receives the result in place -- To-From bytes on
// decode, EncodeSize(len(Src)) bytes on encode -- and is allocated otherwise.
type BlockObject struct {
	Src      []byte
	Size     int64
	From, To int64
	Dst      []byte
}

// BlockResult is one object's outcome: Err is nil, ErrMismatchedCrc (BadBlock is then the first
// mismatching block, -1 otherwise), io.ErrUnexpectedEOF for a framed object that ends before the
// blocks the range touches (as BlockDecode), or an argument error.  Crc is crc32.ChecksumIEEE of the
// whole payload: always on encode; on check and decode when [From, To) is the whole payload and the
// object is good, else 0.  Out is the decoded range or the framed object (nil on check).
type BlockResult struct {
	Err      error
	BadBlock int64
	Crc      uint32
	Out      []byte
}

const (
	blkCheck = iota
	blkDecode
	blkEncode
)

// blockObjects runs one *_objects call.  The descriptor array holds pointers, so it is built in C
// memory from the vector callVec hands over (INTEGRATION.md §3a): buffers in HostAlloc memory go in as
// they are and run in place; Go memory is pinned with Go >= 1.21 and staged through C memory before
// that, copied back after the call.  The returned error speaks for the whole call only.
func blockObjects(mode int, objs []BlockObject, blockLen int64) ([]BlockResult, error) {
	if C.cfsec_crc32block_encode_size(0, C.int64_t(blockLen)) < 0 {
		return nil, ErrInvalidBlock
	}
	n := len(objs)
	res := make([]BlockResult, n)
	if n == 0 {
		return res, nil
	}
	vec := make([][]byte, 2*n) // object i: its source, then its destination
	for i, o := range objs {
		vec[2*i] = o.Src
		need := int64(0)
		switch mode {
		case blkDecode:
			if 0 <= o.From && o.From <= o.To && o.To <= o.Size {
				need = o.To - o.From
			}
		case blkEncode:
			need = int64(C.cfsec_crc32block_encode_size(C.int64_t(len(o.Src)), C.int64_t(blockLen)))
		}
		dst := o.Dst
		if mode != blkCheck && dst == nil {
			dst = make([]byte, need)
		}
		if mode != blkCheck && int64(len(dst)) < need {
			return nil, errInvalidArg
		}
		vec[2*i+1] = dst
	}
	status := make([]C.int, n)
	bad := make([]C.int64_t, n)
	crc := make([]C.uint32_t, n)
	st := callVec(vec, func(v *C.cfsec_shard, _ C.int) C.int {
		sh := unsafe.Slice(v, 2*n)
		arr := (*C.cfsec_blk_object)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(C.cfsec_blk_object{}))))
		defer C.free(unsafe.Pointer(arr))
		d := unsafe.Slice(arr, n)
		for i, o := range objs {
			d[i].src = sh[2*i].data
			d[i].src_len = C.int64_t(len(o.Src))
			d[i].dst = sh[2*i+1].data
			d[i].size = C.int64_t(o.Size)
			if mode == blkEncode {
				d[i].size = C.int64_t(len(o.Src))
			}
			d[i].from, d[i].to = C.int64_t(o.From), C.int64_t(o.To)
		}
		// Go pointers passed as arguments to memory holding no Go pointers: legal without pinning
		switch mode {
		case blkCheck:
			return C.cfsec_crc32block_check_objects(arr, C.int(n), C.int64_t(blockLen), &status[0], &bad[0], &crc[0],
				C.CFSEC_MEM_HOST, -1, nil)
		case blkDecode:
			return C.cfsec_crc32block_decode_objects(arr, C.int(n), C.int64_t(blockLen), &status[0], &bad[0], &crc[0],
				C.CFSEC_MEM_HOST, -1, nil)
		}
		for i := range bad {
			bad[i] = -1
		}
		return C.cfsec_crc32block_encode_objects(arr, C.int(n), C.int64_t(blockLen), &status[0], &crc[0],
			C.CFSEC_MEM_HOST, -1, nil)
	})
	if st == C.CFSEC_ERR_INVALID_BLOCK {
		return nil, ErrInvalidBlock
	}
	if err := toError(st); err != nil {
		return nil, err
	}
	for i := range res {
		res[i] = BlockResult{BadBlock: int64(bad[i]), Crc: uint32(crc[i])}
		switch status[i] {
		case C.CFSEC_OK:
			if mode != blkCheck {
				res[i].Out = vec[2*i+1]
			}
		case C.CFSEC_ERR_MISMATCHED_CRC:
			res[i].Err = ErrMismatchedCrc
		case C.CFSEC_ERR_SHORT_DATA:
			res[i].Err = io.ErrUnexpectedEOF
		default:
			res[i].Err = toError(status[i])
		}
	}
	return res, nil
}

// BlockCheckObjects verifies, for every object, the blocks Decoder.Reader(From, To) would read and
// copies nothing: blobnode's data inspect (datainspect.go:95-130) reads every shard of a chunk
// through cs.Read into io.Discard.  One launch for all objects, whatever their sizes.
func BlockCheckObjects(objs []BlockObject, blockLen int64) ([]BlockResult, error) {
	return blockObjects(blkCheck, objs, blockLen)
}

// BlockDecodeObjects is BlockDecode over many objects in one launch (concurrent range Gets,
// datafile.go:393-427); errors are per object.
func BlockDecodeObjects(objs []BlockObject, blockLen int64) ([]BlockResult, error) {
	return blockObjects(blkDecode, objs, blockLen)
}

// BlockEncodeObjects is BlockEncode over many payloads of different sizes in one launch: the rebuilt
// shards of a repair tasklet (work_shard_recover.go:751, then datafile.go:345-373), each with the
// shard checksum blobnode keeps in the footer.
func BlockEncodeObjects(objs []BlockObject, blockLen int64) ([]BlockResult, error) {
	return blockObjects(blkEncode, objs, blockLen)
}
