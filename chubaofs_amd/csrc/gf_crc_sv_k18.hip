// gf_crc_sv_k18.hip -- Reconstruct + Verify with every row checksummed (gf_crc_sv_kernel), k = 18; see gf_crc.hpp.
#include "gf_crc.hpp"

CFSEC_CRC_SV_INSTANTIATE(18)
