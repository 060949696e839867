"""reedsolomon -- the engine seam: mirror of reedsolomon.Encoder
(vendor/github.com/klauspost/reedsolomon/reedsolomon.go:25-131) backed by
libcfsec.so's cfsec_rs_* entry points (gfx950 kernels).

    enc = New(12, 4)
    enc.Encode(shards)            # shards: 16 equal-length uint8 buffers
    ok = enc.Verify(shards)
    shards[0] = shards[0][:0]     # mark missing
    enc.Reconstruct(shards)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._shards import BatchMarshal, Marshal, ptr_array, shard_size, stream_ptr


class ReedSolomon:
    def __init__(self, data_shards: int, parity_shards: int, device: int = -1):
        L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(L.cfsec_rs_new(data_shards, parity_shards, device, ctypes.byref(h)))
        self._h = h
        self._L = L
        self.data_shards = data_shards
        self.parity_shards = parity_shards
        self.total_shards = data_shards + parity_shards
        self.device = device if device >= 0 else _current_device()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.cfsec_rs_free(h)
            self._h = None

    # -- KRS Encoder methods used by CubeFS --
    def Encode(self, shards, stream=None) -> None:
        m = Marshal(shards)
        _lib.check(self._L.cfsec_rs_encode(self._h, m.ptr(), m.n, m.mem, stream_ptr(stream, m.like)))

    def EncodeCRC(self, shards, stream=None):
        """Encode + crc32.ChecksumIEEE of every shard, fused (cfsec_rs_encode_crc); returns the
        n checksums (what access computes per shard after Encode, stream_put.go:249-253)."""
        m = Marshal(shards)
        out = (ctypes.c_uint32 * max(m.n, 1))()
        _lib.check(self._L.cfsec_rs_encode_crc(self._h, m.ptr(), m.n, m.mem, stream_ptr(stream, m.like), out))
        return [int(out[i]) for i in range(m.n)]

    def Verify(self, shards, stream=None) -> bool:
        m = Marshal(shards)
        ok = ctypes.c_int(0)
        _lib.check(self._L.cfsec_rs_verify(self._h, m.ptr(), m.n, m.mem, stream_ptr(stream, m.like), ctypes.byref(ok)))
        return bool(ok.value)

    def _reconstruct(self, fn, shards, stream):
        m = Marshal(shards, fill_size=shard_size(shards))
        st = fn(self._h, m.ptr(), m.n, m.mem, stream_ptr(stream, m.like))
        m.writeback()
        _lib.check(st)

    def Reconstruct(self, shards, stream=None) -> None:
        self._reconstruct(self._L.cfsec_rs_reconstruct, shards, stream)

    def ReconstructData(self, shards, stream=None) -> None:
        self._reconstruct(self._L.cfsec_rs_reconstruct_data, shards, stream)

    def EncodeIdx(self, dataShard, idx: int, parity, stream=None) -> None:
        """parity[r] ^= M[k + r][idx] * dataShard (KRS/reedsolomon.go:631-667): parity accumulates as
        the data shards of a stripe arrive, each delivered once, into parity shards that start zeroed."""
        d, p = Marshal([dataShard]), Marshal(list(parity))
        if d.like is not None and p.like is not None and d.mem != p.mem:
            raise TypeError("mixing host and device shards in one call")
        like = p.like if p.like is not None else d.like
        _lib.check(self._L.cfsec_rs_encode_idx(self._h, d.ptr(), idx, p.ptr(), p.n, p.mem if p.like is not None else d.mem,
                                               stream_ptr(stream, like)))

    def Update(self, shards, newDatashards, stream=None) -> None:
        """Parity update for the data shards that change (KRS/reedsolomon.go:672-734): newDatashards
        has data_shards entries, None or empty where a column keeps its contents.  As in the
        reference, a changed entry of `shards` is left holding old ^ new, not the new contents."""
        m, nw = Marshal(shards), Marshal(list(newDatashards))
        if m.like is not None and nw.like is not None and m.mem != nw.mem:
            raise TypeError("mixing host and device shards in one call")
        _lib.check(self._L.cfsec_rs_update(self._h, m.ptr(), m.n, nw.ptr(), nw.n, m.mem, stream_ptr(stream, m.like)))

    def ReconstructSome(self, shards, required, stream=None) -> None:
        """Rebuild only the missing data shards i with required[i] (KRS/reedsolomon.go:1395-1397); every
        other missing entry of `shards` stays as it is."""
        m = Marshal(shards, fill_size=shard_size(shards))
        req = np.ascontiguousarray(np.asarray(required, dtype=bool).astype(np.uint8))
        st = self._L.cfsec_rs_reconstruct_some(self._h, m.ptr(), m.n, req.ctypes.data if req.size else None,
                                               int(req.size), m.mem, stream_ptr(stream, m.like))
        m.writeback()
        _lib.check(st)

    def Split(self, data: np.ndarray, length: int | None = None):
        """Split data[:length] (cap = data.size) into views, KRS/reedsolomon.go:1574-1632."""
        if length is None:
            length = int(data.size)
        out = (_lib.Shard * self.total_shards)()
        need = ctypes.c_size_t(0)
        ptr = data.ctypes.data if data.size else None
        st = self._L.cfsec_rs_split(self._h, ptr, length, int(data.size), out, None, 0, ctypes.byref(need))
        pad = None
        if st == _lib.ErrInvalidArg.status and need.value:
            pad = np.zeros(need.value, np.uint8)
            st = self._L.cfsec_rs_split(self._h, ptr, length, int(data.size), out, pad.ctypes.data,
                                        pad.size, ctypes.byref(need))
        _lib.check(st)
        views = []
        for i in range(self.total_shards):
            for src in (data, pad):
                if src is None or not src.size:
                    continue
                off = out[i].data - src.ctypes.data
                if 0 <= off < src.size:
                    views.append(src[off:off + out[i].len])
                    break
            else:
                raise RuntimeError("split returned a pointer outside its buffers")
        return views

    def Join(self, dst, shards, out_size: int) -> None:
        """Write out_size bytes of the data shards to dst (a writer or bytearray)."""
        m = Marshal(list(shards))
        for i, s in enumerate(shards):  # only a Go nil slice (None) is "missing" for Join
            if s is None:
                m.arr[i].data = None
            elif m.arr[i].data is None:
                m.arr[i].data = 1  # non-nil empty slice; never dereferenced
        buf = np.zeros(max(out_size, 1), np.uint8)
        _lib.check(self._L.cfsec_rs_join(self._h, buf.ctypes.data, buf.size, m.ptr(), m.n, out_size))
        data = buf[:out_size].tobytes()
        if hasattr(dst, "write"):
            dst.write(data)
        else:
            dst.extend(data)

    # -- stripe batches over the handle's devices (cfsec_rs_*_stripes) --
    def SetDevices(self, devices) -> None:
        """Spread stripe batches over these HIP devices (default: the handle's own)."""
        arr = (ctypes.c_int * len(devices))(*devices)
        _lib.check(self._L.cfsec_rs_set_devices(self._h, arr, len(devices)))

    def _stripes(self, fn, stripes, fill, *extra):
        bm = BatchMarshal(stripes, self.total_shards, fill=fill)
        status = (ctypes.c_int * max(len(stripes), 1))()
        st = fn(self._h, bm.arr, len(stripes), *extra, bm.mem, status)
        bm.writeback()
        _lib.check(st)
        return [int(status[i]) for i in range(len(stripes))]

    def EncodeStripes(self, stripes):
        """Encode every stripe (each a list of total_shards buffers, sizes may differ per stripe);
        returns one status code per stripe (0 = ok, else the code Encode would raise)."""
        return self._stripes(self._L.cfsec_rs_encode_stripes, stripes, False)

    def EncodeCRCStripes(self, stripes):
        """EncodeStripes, then crc32.ChecksumIEEE of every shard of every stripe, as access ends a put
        (cfsec_rs_encode_crc_stripes): small stripes of any mix of lengths share one kernel launch that
        codes and checksums them.  Returns (per-stripe status codes, per stripe its total_shards
        checksums; all zero for a stripe that failed)."""
        n = self.total_shards
        bm = BatchMarshal(stripes, n, fill=False)
        status = (ctypes.c_int * max(len(stripes), 1))()
        words = (ctypes.c_uint32 * max(len(stripes) * n, 1))()
        st = self._L.cfsec_rs_encode_crc_stripes(self._h, bm.arr, len(stripes), bm.mem, status, words)
        bm.writeback()
        _lib.check(st)
        return ([int(status[i]) for i in range(len(stripes))],
                [[int(words[s * n + i]) for i in range(n)] for s in range(len(stripes))])

    def VerifyStripes(self, stripes):
        """Per stripe: 0 when Verify holds, ErrVerify.status when it returns false, else the error."""
        return self._stripes(self._L.cfsec_rs_verify_stripes, stripes, False)

    def ReconstructStripes(self, stripes, verify: bool = True):
        """Reconstruct (+ Verify) every stripe in one fused pass per stripe; missing entries (None or
        empty) are replaced in the lists by the rebuilt shards.  Per-stripe status codes."""
        return self._stripes(self._L.cfsec_rs_reconstruct_stripes, stripes, True, int(verify))

    def RepairCRCStripes(self, stripes):
        """ReconstructStripes(verify=True), and crc32.ChecksumIEEE of every shard of every stripe as it
        stands afterwards, survivors and rebuilt shards (cfsec_rs_repair_crc_stripes): small stripes of any
        mix of lengths and missing sets share one kernel launch that rebuilds, compares and checksums
        them.  Returns (per-stripe status codes, per stripe its total_shards checksums; all zero for a
        stripe whose status is neither 0 nor ErrVerify)."""
        n = self.total_shards
        bm = BatchMarshal(stripes, n, fill=True)
        status = (ctypes.c_int * max(len(stripes), 1))()
        words = (ctypes.c_uint32 * max(len(stripes) * n, 1))()
        st = self._L.cfsec_rs_repair_crc_stripes(self._h, bm.arr, len(stripes), bm.mem, status, words)
        bm.writeback()
        _lib.check(st)
        return ([int(status[i]) for i in range(len(stripes))],
                [[int(words[s * n + i]) for i in range(n)] for s in range(len(stripes))])

    def ReconstructDataStripes(self, stripes):
        """ReconstructData of every stripe in one call: the missing data shards only (missing parity
        stays missing); small segments of any mix of erasure patterns and lengths share one kernel
        launch.  Per-stripe status codes, each what ReconstructData would raise for that stripe."""
        return self._stripes(self._L.cfsec_rs_reconstruct_data_stripes, stripes, True)

    def ReconstructSomeStripes(self, stripes, required):
        """ReconstructSome of every stripe in one call; required[s] is stripe s's mask of data_shards
        entries.  Per-stripe status codes, each what ReconstructSome would raise for that stripe."""
        req = np.zeros((max(len(stripes), 1), self.data_shards), np.uint8)
        for s, r in enumerate(required):
            r = np.asarray(r, dtype=bool)
            if r.size != self.data_shards:
                raise ValueError(f"every mask needs {self.data_shards} entries")
            req[s] = r
        return self._stripes(self._L.cfsec_rs_reconstruct_some_stripes, stripes, True, req.ctypes.data)

    # -- helpers / GPU batch API --
    def matrix(self) -> np.ndarray:
        out = np.zeros((self.total_shards, self.data_shards), np.uint8)
        _lib.check(self._L.cfsec_rs_matrix(self._h, out.ctypes.data, out.size))
        return out

    def encode_batch(self, ptrs, shard_len: int, nstripes: int, stream=None) -> None:
        _lib.check(self._L.cfsec_rs_encode_batch(self._h, ptr_array(ptrs), shard_len, nstripes,
                                                 stream_ptr(stream, device=self.device)))

    def update_batch(self, ptrs, new_ptrs, cols, shard_len: int, nstripes: int, stream=None) -> None:
        """Update of a device batch (cfsec_rs_update_batch): columns `cols` (strictly increasing) of
        every stripe change to new_ptrs[s * len(cols) + j]; ptrs as encode_batch.  The changed columns
        are left holding old ^ new."""
        ca = (ctypes.c_int * max(len(cols), 1))(*cols)
        _lib.check(self._L.cfsec_rs_update_batch(self._h, ptr_array(ptrs), ptr_array(new_ptrs), ca, len(cols), shard_len,
                                                 nstripes, stream_ptr(stream, device=self.device)))

    def verify_batch(self, ptrs, shard_len: int, nstripes: int, flags_ptr: int, stream=None) -> None:
        _lib.check(self._L.cfsec_rs_verify_batch(self._h, ptr_array(ptrs), shard_len, nstripes,
                                                 flags_ptr, stream_ptr(stream, device=self.device)))

    def reconstruct_batch(self, ptrs, shard_len: int, nstripes: int, erased, data_only=False,
                          stream=None) -> None:
        er = (ctypes.c_int * max(len(erased), 1))(*erased)
        _lib.check(self._L.cfsec_rs_reconstruct_batch(self._h, ptr_array(ptrs), shard_len, nstripes, er,
                                                      len(erased), int(data_only), stream_ptr(stream, device=self.device)))

    def encode_crc_batch(self, ptrs, shard_len: int, nstripes: int, crcs_ptr: int, stream=None) -> None:
        """encode_batch + crc32.ChecksumIEEE of every shard into the device uint32 array at
        crcs_ptr, [stripe][shard] (access/stream_put.go:249-253), fused where supported."""
        _lib.check(self._L.cfsec_rs_encode_crc_batch(self._h, ptr_array(ptrs), shard_len, nstripes, crcs_ptr,
                                                     stream_ptr(stream, device=self.device)))

    def reconstruct_crc_batch(self, ptrs, shard_len: int, nstripes: int, erased, crcs_ptr: int,
                              data_only=False, stream=None) -> None:
        """reconstruct_batch + crc32.ChecksumIEEE of each rebuilt shard ([stripe][shard]; other
        words 0)."""
        er = (ctypes.c_int * max(len(erased), 1))(*erased)
        _lib.check(self._L.cfsec_rs_reconstruct_crc_batch(self._h, ptr_array(ptrs), shard_len, nstripes, er,
                                                          len(erased), int(data_only), crcs_ptr,
                                                          stream_ptr(stream, device=self.device)))

    def repair_crc_batch(self, ptrs, shard_len: int, nstripes: int, erased, flags_ptr: int, crcs_ptr: int,
                         stream=None) -> None:
        """reconstruct_batch of every erased shard, the Verify of the same pass (flags_ptr as
        verify_batch) and crc32.ChecksumIEEE of every shard as it stands afterwards, survivors
        included ([stripe][shard], every word filled): blobnode's repair with its checksum work
        (work_shard_recover.go:654-685, 751-760, 335-342)."""
        er = (ctypes.c_int * max(len(erased), 1))(*erased)
        _lib.check(self._L.cfsec_rs_repair_crc_batch(self._h, ptr_array(ptrs), shard_len, nstripes, er,
                                                     len(erased), flags_ptr, crcs_ptr,
                                                     stream_ptr(stream, device=self.device)))


def _current_device() -> int:
    """The HIP device a handle created with device=-1 binds to (the calling thread's current one)."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return torch.cuda.current_device()
    return 0


def New(data_shards: int, parity_shards: int, device: int = -1) -> ReedSolomon:
    """reedsolomon.New with default options (KRS/reedsolomon.go:413)."""
    return ReedSolomon(data_shards, parity_shards, device)


def crc32_ieee_batch(ptrs, shard_len: int, device: int = -1, stream=None):
    """crc32.ChecksumIEEE of each device shard (list of device pointers)."""
    L = _lib.lib()
    out = (ctypes.c_uint32 * max(len(ptrs), 1))()
    dev = device if device >= 0 else _current_device()
    _lib.check(L.cfsec_crc32_ieee_batch(ptr_array(ptrs), shard_len, len(ptrs), out, device,
                                        stream_ptr(stream, device=dev)))
    return [int(out[i]) for i in range(len(ptrs))]
