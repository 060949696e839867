// gf_mix.hip -- the mixed-plan launch: store-only GF(2^8) products of many items in one launch.
//
// access rebuilds the byte range of a degraded Get with ReconstructData over every shard's segment
// (access/stream_get.go:384-431), blob by blob, each with its own bad set and segment length.  The
// other product kernels take one coefficient matrix per launch from the kernel argument block, so a
// batch of such segments costs a launch per erasure pattern, and a pointer-table launch carries
// kPtrSlots rows.  Here a workgroup reads what it codes from a table in device memory (gf_mix.hpp):
// its tile's item, the item's rows, length and coefficient rows.  The whole batch is one launch,
// whatever its mix of patterns, lengths and addresses.
//
// One workgroup codes one tile: 256 lanes x 16 bytes of every row of one item.  It builds the v_perm_b32
// product tables of up to kMixPassRows of its item's coefficient rows in LDS (build_tables), one
// barrier, then the mac_row product of gf_device.hpp over the k inputs.  Items with more than
// kMixPassRows outputs (up to 16 missing data rows of the 16 + 20 code) take further passes over the
// tile, the inputs re-read from cache; a degraded read has 1 or 2 outputs and one pass.
//
// Rows start at any byte and have any length from 1: the lane holding a row's ragged end codes the
// row's last full 16-byte chunk instead (its leading bytes repeat the neighbour's, with the same
// values), rows shorter than 16 bytes take byte loads and stores in lane 0.  No access leaves
// [row, row + len); output rows are written with the compiler's own stores.
#include <hip/hip_runtime.h>

#include "gf_device.hpp"
#include "gf_mix.hpp"
#include "kernels.hpp"

namespace cfsec {
namespace {

using dev::u32x4;

// A row address of the table as a pointer into global memory (the table holds plain 64-bit numbers,
// which the compiler would otherwise access through the flat path).
typedef __attribute__((address_space(1))) uint8_t global_u8;
__device__ __forceinline__ uint8_t* row_ptr(uint64_t a) { return (uint8_t*)(global_u8*)a; }

// Rows [0, mc) of a pass (mc <= M; tables at stride kMixPassRows) over this lane's chunk.
template <int M, bool NTL>
__device__ __forceinline__ void mix_pass(int k, int mc, const uint64_t* in, const uint64_t* out, const u32x4* tab01,
                                         const uint32_t* tab2, uint64_t off, uint64_t len) {
  constexpr int MT = kMixPassRows, G = 4;
  u32x4 acc[M];
#pragma unroll
  for (int r = 0; r < M; ++r) acc[r] = u32x4{0u, 0u, 0u, 0u};
  if (len >= (uint64_t)dev::kLaneBytes) {
    const uint64_t loff = off + dev::kLaneBytes <= len ? off : len - dev::kLaneBytes;
    for (int c0 = 0; c0 < k; c0 += G) {
      u32x4 x[G];
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (c0 + g < k) x[g] = dev::ld16<NTL>(row_ptr(in[c0 + g]) + loff);
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (c0 + g < k) dev::mac_row<M>(acc, x[g], tab01 + (c0 + g) * MT, tab2 + (c0 + g) * MT);
    }
#pragma unroll
    for (int r = 0; r < M; ++r)
      if (r < mc) dev::st16_out<true>(row_ptr(out[r]) + loff, acc[r]);
  } else if (off == 0) {
    for (int c = 0; c < k; ++c)
      dev::mac_row<M>(acc, dev::ld_tail(row_ptr(in[c]), (size_t)len), tab01 + c * MT,
                      tab2 + c * MT);
#pragma unroll
    for (int r = 0; r < M; ++r)
      if (r < mc) dev::st_tail(row_ptr(out[r]), acc[r], (size_t)len);
  }
}

__global__ __launch_bounds__(256) void gf_mix_kernel(const uint8_t* __restrict__ table, uint32_t ntiles) {
  __shared__ u32x4 tab01[dev::kMaxK * kMixPassRows];
  __shared__ uint32_t tab2[dev::kMaxK * kMixPassRows];
  const uint32_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  const MixHead* h = reinterpret_cast<const MixHead*>(table);
  const uint32_t idx = reinterpret_cast<const uint32_t*>(table + h->map_off)[tile];
  const MixItem* it = reinterpret_cast<const MixItem*>(table + h->items_off) + idx;
  const int k = (int)it->k, m = (int)it->m;
  const uint64_t len = it->len;
  const uint64_t* in = reinterpret_cast<const uint64_t*>(table + h->rows_off) + it->rows;
  const uint64_t* out = in + k;
  const uint8_t* coef = table + it->coef;
  const uint64_t off = (uint64_t)(tile - it->tile0) * kMixTile + (uint64_t)threadIdx.x * dev::kLaneBytes;
  if (m <= kMixPassRows) {  // one pass: every input byte is read once
    dev::build_tables<kMixPassRows>(k, m, coef, tab01, tab2);
    __syncthreads();
    if (off < len) {
      if (m == 1) mix_pass<1, true>(k, m, in, out, tab01, tab2, off, len);
      else if (m == 2) mix_pass<2, true>(k, m, in, out, tab01, tab2, off, len);
      else mix_pass<kMixPassRows, true>(k, m, in, out, tab01, tab2, off, len);
    }
    return;
  }
  for (int r0 = 0; r0 < m; r0 += kMixPassRows) {
    const int mc = m - r0 < kMixPassRows ? m - r0 : kMixPassRows;
    if (r0) __syncthreads();  // the previous pass has read its tables
    dev::build_tables<kMixPassRows>(k, mc, coef + r0 * k, tab01, tab2);
    __syncthreads();
    if (off < len) mix_pass<kMixPassRows, false>(k, mc, in, out + r0, tab01, tab2, off, len);
  }
}

}  // namespace

hipError_t launch_mix(const uint8_t* table, uint32_t ntiles, hipStream_t stream) {
  if (!table || ntiles == 0 || ntiles > kMixMaxTiles) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gf_mix_kernel, dim3(ntiles), dim3(dev::kThreads), 0, stream, table, ntiles);
  return hipGetLastError();
}

}  // namespace cfsec
