// crc32block_objects.hip -- crc32block framing over objects of mixed sizes, ranges and alignments in
// one launch (the object table of crc32block_objects.hpp), gfx950.
//
// One work item is one block of one object; the kernel is crc32block.hip's shipped block kernel with
// everything that kernel reads from its argument block read from the table instead: 256 threads, the
// 5-bit Horner tables in LDS once per workgroup, a resident grid striding over consecutive items (the
// workgroups in flight sweep one region), RING tiles in flight per thread in registers named at compile
// time, the next item's first tiles loaded before the epilogue, per-wave epilogue multiplies and one
// barrier, atomicMin of the first bad block and one atomicXor per block into the object's whole-payload
// checksum.  The block body is a copy of crc32block_block_kernel's, not a function shared with it: the
// shipped kernel's code stays as it was measured.
//
//   decode, encode   pieces cut at 16-byte boundaries and tiles at 4 KiB boundaries of the destination,
//                    one writer per seam line on decode, stores through st16_out (as crc32block.hip)
//   check            no destination: pieces cut at 16-byte boundaries of the source, so every full load
//                    is an aligned 16-byte non-temporal load, and nothing is stored but the result words.
//                    With a 16-byte-aligned object the first piece of a block holds its 4 header bytes
//                    and 12 payload bytes: the header bytes are left out of it like any byte outside
//                    [0, plen), and the stored word is fetched on its own up front.
// No access leaves the framed bytes [b0 * block_len, f1) of an object (check, decode) or its payload and
// its framed destination (encode): full loads lie inside a block's payload, the ragged pieces at its two
// ends are read byte by byte inside it.
//
// Out of scope: packing several sub-tile objects into one workgroup.  A 100-byte object costs a
// workgroup pass here, as it costs a launch through the single call.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "crc32block_objects.hpp"
#include "gf_crc.hpp"
#include "kernels.hpp"

namespace cfsec {
namespace blkobj {

using crcdev::kTile;
using dev::u32x4;

constexpr int kRing = 8;  // tiles in flight per thread (the shipped block kernel's)

// The table holds addresses as numbers.  A plain pointer made from one is a generic pointer, and its
// accesses would be flat_ instructions, which count on the LDS counter too: every wait for a table lookup
// would wait for the ring's loads.  So data pointers are typed in the global address space; a store helper
// that takes a plain pointer gets the cast back at the call, which address-space inference undoes.
#define CFSEC_GLOBAL __attribute__((address_space(1)))
typedef CFSEC_GLOBAL uint8_t g8;
typedef CFSEC_GLOBAL uint32_t g32;
typedef CFSEC_GLOBAL dev::u32x4_ua gvec_ua;
typedef CFSEC_GLOBAL dev::u32x4 gvec;
template <class T>
__device__ __forceinline__ CFSEC_GLOBAL T* as_global(uint64_t addr) {
  return (CFSEC_GLOBAL T*)reinterpret_cast<T*>(addr);
}

// Bytes [lo, hi) of the 16 at p, zero elsewhere; no other byte is read.
__device__ __forceinline__ u32x4 ld_range(const g8* p, uint32_t lo, uint32_t hi) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i)
    if (i >= lo && i < hi) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
  return u32x4{w[0], w[1], w[2], w[3]};
}

// Piece p of a block: payload positions 16p - h .. 16p - h + 15; positions outside [0, plen) read as
// zero (leading zeros leave a zero-preset CRC unchanged, trailing ones are taken out by the tile-end
// factor).  ALIGNED: src - h is 16-byte aligned (check), so a full piece is an aligned load.
template <bool ALIGNED>
__device__ __forceinline__ void load_piece(const g8* src, uint32_t plen, uint32_t h, uint32_t p,
                                           uint32_t (&d)[4]) {
  const int64_t first = (int64_t)16 * p - h;
  u32x4 v{0u, 0u, 0u, 0u};
  if (first >= 0 && first + 16 <= plen) {
    if constexpr (ALIGNED) v = __builtin_nontemporal_load((const gvec*)(src + first));
    else v = __builtin_nontemporal_load((const gvec_ua*)(src + first));
  } else if (first < (int64_t)plen) {
    v = ld_range(src + first, first < 0 ? (uint32_t)-first : 0u, (uint32_t)min<int64_t>(16, plen - first));
  }
  d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
}

template <int MODE, int RING>
__global__ __launch_bounds__(256, 5) void crc32block_objects_kernel(const uint8_t* __restrict__ table, uint32_t nitems) {
  constexpr bool kCheck = MODE == kBlkCheck, kDecode = MODE == kBlkDecode, kEncode = MODE == kBlkEncode;
  __shared__ uint32_t ct[crcdev::kFiveTabWords];
  __shared__ uint32_t redb[2][8];  // per wave: its share of the block's raw CRC, and of the object's
  const BlkHead& hd = *reinterpret_cast<const BlkHead*>(table);
  const g32* const tabs = as_global<const uint32_t>(hd.tabs);
  for (int i = threadIdx.x; i < crcdev::kFiveTabWords; i += 256) ct[i] = tabs[crcdev::kFiveTabBase + i];
  const uint32_t tid = threadIdx.x;
  const uint32_t kj = tabs[crcdev::kShiftBase + tid];
  __syncthreads();
  uint32_t it = blockIdx.x;
  if (it >= nitems) return;  // whole workgroup: no barrier follows
  const BlkObject* const objs = reinterpret_cast<const BlkObject*>(table + hd.objs_off);
  const uint32_t* const map = reinterpret_cast<const uint32_t*>(table + hd.map_off);
  g32* const bad = as_global<uint32_t>(hd.words);
  g32* const whole = bad + hd.nobjects;
  const uint32_t P = hd.P;
  const uint64_t blen = (uint64_t)P + 4;

  // decode: each seam line (the 128-byte line of the destination holding the end of one block's payload
  // and the start of the next's) has one writer, as in crc32block.hip: a block stores from the first
  // line boundary of its payload [sbeg) on through the next block's first bytes up to the next line
  // boundary [send), those taken from the next block's frame
  struct Blk {
    const BlkObject* o;
    uint32_t y, w, b, plen, h, tiles, stored;
    int last;
    uint64_t q0;         // payload coordinate of the block's first byte
    const g8* src;  // the block's payload
    const g8* hdr;  // check, decode: the stored checksum word; encode: where it is written
    g8* dp;         // destination of payload byte 0 of the block
    uint32_t sbeg, send, lim;  // stored payload range [sbeg, send); main loop stores below lim
  };
  const auto make = [&](uint32_t item) {
    Blk k;
    k.y = map[item];
    k.o = objs + k.y;
    const BlkObject& o = *k.o;
    k.w = item - o.item0;
    k.b = o.b0 + k.w;
    k.q0 = (uint64_t)k.b * P;
    k.plen = (uint32_t)min<uint64_t>(P, o.size - k.q0);
    k.last = k.plen != P ? 1 : 0;
    if constexpr (kEncode) {
      k.src = as_global<const uint8_t>(o.src + k.q0);
      k.hdr = as_global<const uint8_t>(o.dst + (uint64_t)k.b * blen);
      k.dp = as_global<uint8_t>(o.dst + (uint64_t)k.b * blen + 4);
      k.h = o.h;
    } else {
      k.hdr = as_global<const uint8_t>(o.src + (uint64_t)k.b * blen);
      k.src = as_global<const uint8_t>(o.src + (uint64_t)k.b * blen + 4);
      k.dp = kDecode ? as_global<uint8_t>(o.dst + k.q0) : nullptr;
      k.h = kDecode ? (uint32_t)((o.dst + k.q0) & (kTile - 1)) : o.h;
    }
    k.tiles = (k.plen + k.h + kTile - 1) / kTile;
    k.sbeg = 0, k.send = k.plen, k.lim = k.plen;
    if constexpr (kDecode) {
      const uint64_t d0 = o.dst + k.q0;
      if (k.w > 0) k.sbeg = (uint32_t)((128u - (d0 & 127u)) & 127u);
      if (k.w + 1 < o.nb) {
        const uint64_t next = min<uint64_t>(P, o.size - k.q0 - k.plen);  // the next block's payload
        k.send = k.plen + (uint32_t)min<uint64_t>((128u - ((d0 + k.plen) & 127u)) & 127u, next);
        k.lim = k.plen - ((k.plen + k.h) & 15u);  // the piece across the seam goes with the tail
      }
    }
    // the stored checksum, fetched up front (read at the end it is one more dependent global load on
    // the workgroup's critical path)
    k.stored = 0;
    if (!kEncode && tid == 0)
      k.stored = k.hdr[0] | (uint32_t)k.hdr[1] << 8 | (uint32_t)k.hdr[2] << 16 | (uint32_t)k.hdr[3] << 24;
    return k;
  };
  uint32_t ring[RING][4];
  const auto prefetch = [&](const Blk& k) {
#pragma unroll
    for (int r = 0; r < RING; ++r)
      if (r < (int)k.tiles) load_piece<kCheck>(k.src, k.plen, k.h, tid + 256 * r, ring[r]);
  };
  Blk cur = make(it);
  prefetch(cur);
  for (uint32_t parity = 0;; parity ^= 1u) {
    const BlkObject& o = *cur.o;
    const uint64_t lo = o.lo, hi = o.hi;
    uint32_t R = 0;
    // piece t*256 + tid: Horner step, then (decode, encode) the copy to the destination
    const auto piece = [&](uint32_t t, uint32_t (&pc)[4]) {
      const uint32_t p = t * 256 + tid;
      R = crcdev::crc_step5(ct, R, pc);
      if constexpr (!kCheck) {
        const int64_t first = (int64_t)16 * p - cur.h;
        if (first + 16 > (int64_t)cur.sbeg && first < (int64_t)cur.lim) {  // sbeg > 0 is a piece boundary
          const int64_t q = (int64_t)cur.q0 + first;
          g8* dp = cur.dp + first;  // 16-byte aligned
          if (first >= 0 && first + 16 <= cur.lim && q >= (int64_t)lo && q + 16 <= (int64_t)hi) {
            dev::st16_out<true>((uint8_t*)dp, u32x4{pc[0], pc[1], pc[2], pc[3]});
          } else {
            for (int j = 0; j < 16; ++j)
              if (first + j >= 0 && first + j < cur.lim && q + j >= (int64_t)lo && q + j < (int64_t)hi)
                dp[j] = (uint8_t)(pc[j >> 2] >> (8 * (j & 3)));
          }
        }
      }
    };
    for (uint32_t t0 = 0; t0 < cur.tiles; t0 += RING) {
#pragma unroll
      for (int r = 0; r < RING; ++r) {
        const uint32_t t = t0 + r;
        if (t < cur.tiles) {
          piece(t, ring[r]);
          if (t + RING < cur.tiles) load_piece<kCheck>(cur.src, cur.plen, cur.h, t * 256 + tid + 256 * RING, ring[r]);
        }
      }
    }
    if constexpr (kDecode) {
      if (cur.send > cur.lim) {  // the pieces from lim to the seam line's end, one per thread
        const uint32_t nx = (cur.send - cur.lim + 15u) >> 4;
        if (tid < nx) {
          const int64_t first = (int64_t)cur.lim + 16 * tid;
          const uint32_t own = (uint32_t)max<int64_t>(0, min<int64_t>(16, (int64_t)cur.plen - first));
          const g8* nsrc = cur.src + blen;  // the next block's payload
          const u32x4 v = ld_range(cur.src + first, 0, own) |
                          ld_range(nsrc + (first - (int64_t)cur.plen), own, (uint32_t)min<int64_t>(16, (int64_t)cur.send - first));
          const int64_t q = (int64_t)cur.q0 + first;
          g8* dp = cur.dp + first;
          if (first + 16 <= cur.send && q >= (int64_t)lo && q + 16 <= (int64_t)hi) {
            dev::st16_out<true>((uint8_t*)dp, v);
          } else {
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 16; ++j)
              if (first + j < cur.send && q + j >= (int64_t)lo && q + j < (int64_t)hi)
                dp[j] = (uint8_t)(w4[j >> 2] >> (8 * (j & 3)));
          }
        }
      }
    }
    const uint32_t nit = it + gridDim.x;
    const bool more = nit < nitems;
    Blk nxt{};
    if (more) {
      nxt = make(nit);
      prefetch(nxt);
    }
    uint32_t* red = redb[parity];  // the other buffer may still be read by thread 0 of the last block
    uint32_t v = crcdev::mulmod(kj, R);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
    if ((tid & 63) == 0) {
      // this wave's share of the block's raw CRC: x^(8(plen + h - tiles*4096)) is one word of the object's
      // record (check, encode: one h per object); decode: the word for h mod 16 and the extra tile, times
      // x^(8*16*(h >> 4)), a word of the per-thread shift table
      uint32_t g;
      if constexpr (kDecode) {
        const uint32_t b16 = cur.h & 15u, dt = cur.tiles - ((cur.plen + b16 + kTile - 1) / kTile);
        g = crcdev::mulmod(o.g[cur.last][cur.w & 3u][dt], tabs[crcdev::kShiftBase + 255 - (cur.h >> 4)]);
      } else {
        g = o.g[cur.last][0][0];
      }
      const uint32_t raw = crcdev::mulmod(g, v);
      red[tid >> 6] = raw;
      if (o.whole) {
        uint32_t s = raw;  // the share moved to the object end: the last block's payload, then full blocks
        if (cur.b + 1 < o.nblk) {
          s = crcdev::mulmod(s, o.xlast);
          uint32_t e = o.nblk - 2 - cur.b;
          for (int q = 0; e; e >>= 1, ++q)
            if (e & 1) s = crcdev::mulmod(s, hd.xpow2[q]);
        }
        red[4 + (tid >> 6)] = s;
      }
    }
    __syncthreads();
    if (tid == 0) {
      const uint32_t crc = red[0] ^ red[1] ^ red[2] ^ red[3] ^ (cur.last ? o.fin_last : hd.fin_full);
      if constexpr (kEncode) {
        g8* hdr = cur.dp - 4;
        for (int j = 0; j < 4; ++j) hdr[j] = (uint8_t)(crc >> (8 * j));
      } else if (cur.stored != crc) {
        atomicMin((uint32_t*)(bad + cur.y), cur.w);
      }
      // one atomic per block (the four waves' shares XOR-ed here: many adders on one word are slow)
      if (o.whole) atomicXor((uint32_t*)(whole + cur.y), red[4] ^ red[5] ^ red[6] ^ red[7] ^ (cur.b + 1 == o.nblk ? o.whole_fin : 0u));
    }
    if (!more) break;
    cur = nxt;
    it = nit;
  }
}

// Workgroups of the kernel resident on the current device at once.
template <int MODE>
unsigned resident_groups() {
  int dev = 0, cus = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, crc32block_objects_kernel<MODE, kRing>, 256, 0) != hipSuccess)
    return 0;
  return (unsigned)std::max(cus * per, 1);
}

template <int MODE>
hipError_t launch(const uint8_t* table, uint32_t objects, uint32_t items, hipStream_t stream) {
  static thread_local int cached_dev = -1;
  static thread_local unsigned cap = 0;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess && dev != cached_dev) {
    cap = resident_groups<MODE>();
    cached_dev = dev;
  }
  // the whole resident grid, (items mod cap) workgroups taking one block more
  const unsigned g = cap ? std::min(cap, items) : items;
  const char* const tv = std::getenv("CFSEC_TRACE_BLK");  // read per call: tests turn it on mid-process
  if (tv && tv[0] && tv[0] != '0')
    std::fprintf(stderr, "cfsec: blk objects mode=%s objects=%u items=%u grid=%u resident=%u\n",
                 MODE == kBlkCheck ? "check" : MODE == kBlkDecode ? "decode" : "encode", objects, items, g, cap);
  hipLaunchKernelGGL((crc32block_objects_kernel<MODE, kRing>), dim3(g), dim3(256), 0, stream, table, items);
  return hipGetLastError();
}

}  // namespace blkobj

hipError_t launch_crc32block_objects(int mode, const uint8_t* table, uint32_t objects, uint32_t items,
                                     hipStream_t stream) {
  if (!table || !objects || !items || items > kBlkMaxItems) return hipErrorInvalidValue;
  switch (mode) {
    case kBlkCheck: return blkobj::launch<kBlkCheck>(table, objects, items, stream);
    case kBlkDecode: return blkobj::launch<kBlkDecode>(table, objects, items, stream);
    case kBlkEncode: return blkobj::launch<kBlkEncode>(table, objects, items, stream);
  }
  return hipErrorInvalidValue;
}

}  // namespace cfsec
