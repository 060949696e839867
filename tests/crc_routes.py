"""Which fused product + checksum kernel a job takes, restated from the kernels that exist
(chubaofs_amd/csrc: gf_bs_crc.hip's networks, gf_crc.hpp's lookup and v_perm kernels) without calling
the library.  tests/test_crc_route.py pins the library's matvec_crc_route to this table on the CPU;
tests/test_gpu_crc_routes.py asserts the route each GPU case reports is the one the table names."""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NONE, BIT_SLICED, LOOKUP, V_PERM = "none", "bit-sliced", "lookup", "v_perm"
ROUTE_DIGIT = {"0": NONE, "1": BIT_SLICED, "2": LOOKUP, "3": V_PERM}

BS_CRC_DEFAULT = 119          # CFSEC_BS_CRC when unset
BS_TILE = 2048                # bytes of a row per bit-sliced tile
BS_MAX_TILES = 64 ** 3        # per row: three 64-entry tables of powers of x^(8 * 2048)
BS_MAX_TILES_ALL = 2 ** 32 - 1  # tiles x stripes: a 32-bit tile counter
FUSED_K = (6, 8, 12, 16, 18)  # input counts gf_crc_k<K>.hip instantiates
MAX_LEN = 0xFFFFFFFF - 4096   # 32-bit lane offsets over 4 KiB tiles

# (CFSEC_BS_CRC bits, k, output counts, generated network whose first m rows the matrix must equal)
NETWORKS = [
    (1, 6, (12,), "ec6p10l2"), (2 | 8, 12, (4,), "ec12p4"), (4, 16, (20, 22), "ec16p20l2"),
    (16, 6, (8, 10), "ec6p10l2"), (16, 12, (9,), "ec12p9"), (16, 15, (12,), "ec15p12"),
    (16, 10, (4,), "ec10p4"), (16, 4, (4,), "ec4p4"), (16, 3, (3,), "ec3p3"),
    (16, 6, (6,), "ec6p3l3"), (16, 4, (6,), "ec4p4l2"), (16, 6, (15,), "ec6p6l9"), (16, 6, (18,), "ec6p8l10"),
    (64, 6, (6,), "ec6p10l2"), (64, 16, (4,), "ec16p20l2"), (128, 6, (3,), "ec6p10l2"),
]
PLAIN_BIT = 32                # the product alone on the EC6P6L9 / EC6P8L10 networks


@functools.lru_cache(maxsize=None)
def network_rows(name):
    """The generated network's matrix (tools/gen_bs_net.py: KRS buildMatrix rows, then the AZ-local
    rows over the data), row-major bytes per row."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_bs_net as g
    finally:
        sys.path.pop(0)
    return tuple(bytes(r) for r in g.CODES[name][1]())


def match_bits(k, m, coef):
    """The CFSEC_BS_CRC bits under which a bit-sliced network equals the m x k matrix `coef`."""
    bits = 0
    for bit, nk, ms, name in NETWORKS:
        if nk == k and m in ms and b"".join(network_rows(name)[:m]) == bytes(coef):
            bits |= bit
    return bits


def dyadic_6x12(coef):
    """EC6P10L2's form: rows 0..9 of 2x2 blocks M[r0+i][c0+j] = M[r0][c0 + (i ^ j)], then 2 plain rows."""
    c = bytes(coef)
    return all(c[(r0 + i) * 6 + c0 + j] == c[r0 * 6 + c0 + (i ^ j)]
               for r0 in range(0, 10, 2) for c0 in range(0, 6, 2) for i in range(2) for j in range(2))


def bs_in_range(length, nstripes):
    tiles = (length + BS_TILE - 1) // BS_TILE
    return length > 0 and tiles <= BS_MAX_TILES and tiles * max(nstripes, 1) <= BS_MAX_TILES_ALL


def expect_route(k, m, cin, length, nstripes, bits=0, dyadic=False, bs_mask=BS_CRC_DEFAULT, lds=True):
    """The route of a kStore job with valid checksum slots: `bits` = match_bits of its matrix, `dyadic`
    = dyadic_6x12 of it (6 x 12 only), cin = the inputs are checksummed too."""
    if m < 1 or length > MAX_LEN:
        return NONE
    if cin and (bits & bs_mask) and bs_in_range(length, nstripes):
        return BIT_SLICED
    if k in FUSED_K and m <= 6:
        return LOOKUP if lds and m <= 4 and k <= 16 else V_PERM
    if k == 6 and m == 12 and cin:
        return LOOKUP if lds else V_PERM if dyadic else NONE
    return NONE


def expect_plain(k, m, coef, length, nstripes, lens=False, bs_mask=BS_CRC_DEFAULT):
    """launch_matvec's bit-sliced product for the wide LRC modes' fused encodes."""
    nets = {15: "ec6p6l9", 18: "ec6p8l10"}
    return (bool(bs_mask & PLAIN_BIT) and k == 6 and m in nets and not lens
            and b"".join(network_rows(nets[m])) == bytes(coef) and bs_in_range(length, nstripes))
