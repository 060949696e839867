// crc_pow.hpp -- powers of x modulo the CRC32 polynomial by table, for the host packers of the table
// launches (pack_blk_objects, blk_objects.cpp; pack_mix_crc, batch.cpp): a table of 1000 items wants a
// few thousand of them, and square-and-multiply (crc_xpow) is ~40 multiplies each.  Host arithmetic only.
#pragma once
#include <cstdint>

namespace cfsec {

uint32_t crc_xpow(int64_t e);                 // gf_crc.hip: x^e mod P, any integer e
uint32_t crc_mulmod(uint32_t a, uint32_t b);  // a * b mod P

struct CrcPowTables {
  uint32_t pos[5][256];  // [k][d]: x^(8 * d * 256^k)
  uint32_t neg[8192];    // [j]: x^(-8 j)
  CrcPowTables() {
    for (int k = 0; k < 5; ++k) {
      const uint32_t step = crc_xpow(int64_t(8) << (8 * k));
      pos[k][0] = 0x80000000u;  // x^0
      for (int d = 1; d < 256; ++d) pos[k][d] = crc_mulmod(pos[k][d - 1], step);
    }
    const uint32_t inv = crc_xpow(-8);
    neg[0] = 0x80000000u;
    for (int j = 1; j < 8192; ++j) neg[j] = crc_mulmod(neg[j - 1], inv);
  }
};
inline const CrcPowTables& crc_pow_tables() {
  static const CrcPowTables t;
  return t;
}
// x^(8 n), 0 <= n < 2^40
inline uint32_t crc_xpow8(int64_t n) {
  const CrcPowTables& t = crc_pow_tables();
  uint32_t v = t.pos[0][n & 255];
  for (int k = 1; k < 5; ++k)
    if (const int d = (int)((n >> (8 * k)) & 255)) v = crc_mulmod(v, t.pos[k][d]);
  return v;
}
// shift(~0, len) ^ ~0 from xlen = x^(8 len): turns a raw CRC of len bytes into crc32.ChecksumIEEE
inline uint32_t crc_shift_ones_of(uint32_t xlen) { return crc_mulmod(xlen, 0xFFFFFFFFu) ^ 0xFFFFFFFFu; }

}  // namespace cfsec
