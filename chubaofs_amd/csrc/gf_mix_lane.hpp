// gf_mix_lane.hpp -- what a lane of the mixed-plan launches with checksums (gf_mix_crc.hip,
// gf_mix_sv.hip) needs to checksum its 16-byte pieces of a tile: device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "gf_crc.hpp"
#include "gf_mix.hpp"
#include "kernels.hpp"

namespace cfsec {
namespace mixdev {

using dev::u32x4;

// Addresses held in the table are numbers.  Pointers made from them are typed in the global address
// space: a generic pointer's accesses are flat instructions, which count on the LDS counter too, and
// every wait for a table lookup would then wait for the row loads in flight.
#define CFSEC_GLOBAL __attribute__((address_space(1)))
typedef CFSEC_GLOBAL uint8_t global_u8;
typedef CFSEC_GLOBAL uint32_t global_u32;
__device__ __forceinline__ uint8_t* row_ptr(uint64_t a) { return (uint8_t*)(global_u8*)a; }

constexpr int kInSlots = kLaunchMaxRows;           // a pass's shares: inputs at [0, k), outputs from kInSlots
constexpr int kRedRows = kInSlots + kMixPassRows;  // per wave

// f(0, d): the raw CRC of one 16-byte piece -- crc_step5 without its register word, which is zero here
// (a tile's pieces are summed by position, not chained): 28 conflict-free lookups.
__device__ __forceinline__ uint32_t crc_piece(const uint32_t* ft, u32x4 d) {
  constexpr int F = crcdev::kFiveFields;
  uint32_t t[4 * F];
  crcdev::five_word<0>(ft, d.x, t);
  crcdev::five_word<1>(ft, d.y, t + F);
  crcdev::five_word<2>(ft, d.z, t + 2 * F);
  crcdev::five_word<3>(ft, d.w, t + 3 * F);
  uint32_t u[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) u[i] = __builtin_amdgcn_bitop3_b32(t[3 * i], t[3 * i + 1], t[3 * i + 2], 0x96);
  const uint32_t a0 = __builtin_amdgcn_bitop3_b32(u[0], u[1], u[2], 0x96);
  const uint32_t a1 = __builtin_amdgcn_bitop3_b32(u[3], u[4], u[5], 0x96);
  const uint32_t a2 = __builtin_amdgcn_bitop3_b32(u[6], u[7], u[8], 0x96);
  return __builtin_amdgcn_bitop3_b32(a0, a1, a2, 0x96) ^ t[27];
}

// What a lane needs to checksum its pieces: the tables, its shift columns col[i] = kj * x^i (kj moves a
// register from the lane's piece end to the tile's end: r * kj is the XOR of the columns r's bits pick),
// its wave's share words.
struct LaneCrc {
  const uint32_t* ct;
  uint32_t col[32];
  uint32_t* red;  // this wave's kRedRows words
  uint32_t lane;

  // This wave's share of a row's tile checksum from every lane's piece, into red[slot].
  __device__ __forceinline__ void share(int slot, u32x4 piece) const {
    const uint32_t r = crc_piece(ct, piece);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) v ^= (0u - ((r >> (31 - i)) & 1u)) & col[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
    if (lane == 0) red[slot] = v;
  }
};

}  // namespace mixdev
}  // namespace cfsec
