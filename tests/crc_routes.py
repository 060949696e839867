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


# ---- launch geometry (plan_bs_crc / plan_matvec_crc, kernels.hpp), restated from the kernels' indexing ----
BS_WAVES = 4                  # waves of a bit-sliced workgroup
BS_PTRS = 96                  # row pointers in its argument block
BS_RESIDENT_FALLBACK = 768    # resident workgroups assumed when the occupancy query fails
LK_TILE = 4096                # bytes of a row per tile of the lookup / v_perm kernels
LK_PTRS = 96
LK_MAX_GROUPS = 384           # group constants in their argument block
LK_GROUPS = 1024              # workgroups per launch of the v_perm kernels (and the lookup fallback)


def ceil_div(a, b):
    return -(-a // b)


def bs_plan(k, m, length, nstripes, affine, resident):
    """The bit-sliced launches of a job: gf_bs_crc_kernel's wave (g, j) = divmod(wave id, W) walks tiles
    j, j + W, ... < bend of stripes g, g + groups, ...; the workgroups from tblk on are tail waves, wave
    q of them taking tile bend + q % tail of stripe q // tail.  `affine`: the stripes keep one stride
    (a single stripe never does).  Returns (resident used, pad, power-table bytes, steps)."""
    resident = resident if resident > 0 else BS_RESIDENT_FALLBACK
    tps = ceil_div(length, BS_TILE)
    per = nstripes if affine and nstripes > 1 else BS_PTRS // (k + m)
    waves = resident * BS_WAVES
    steps = []
    for s0 in range(0, nstripes, per):
        ns = min(per, nstripes - s0)
        W = min(tps, max(1, waves // ns))      # waves per stripe: the resident waves over the stripes
        groups = min(ns, waves // W)
        tail = tps % W                         # the remainder tiles: one per extra wave
        tblk = ceil_div(groups * W, BS_WAVES)
        steps.append(dict(s0=s0, ns=ns, tab=1 if affine and nstripes > 1 else ns, affine=int(affine and nstripes > 1),
                          tps=tps, W=W, groups=groups, bend=tps - tail, tail=tail, tblk=tblk,
                          grid=tblk + ceil_div(tail * ns, BS_WAVES), jump=BS_TILE * W))
    return resident, tps * BS_TILE - length, (BS_TILE, BS_TILE * 64, BS_TILE * 64 * 64), steps


def dyadic_blocks(coef, k, m, B):
    c = bytes(coef)
    return all(c[(r0 + i) * k + c0 + j] == c[r0 * k + c0 + (i ^ j)]
               for r0 in range(0, m, B) for c0 in range(0, k, B) for i in range(B) for j in range(B))


def lk_plan(route, k, m, coef, length, nstripes, affine, resident):
    """The lookup / v_perm launches: a (groups, stripes) grid, workgroup g taking tiles [g tpw, (g + 1)
    tpw) of its stripe.  dy: -1 the lookup kernel; the v_perm kernel's product 4 for 4 outputs of 4x4
    dyadic blocks (k = 12, 16), 2 for 6 x 6 of 2x2 blocks and for the 6 x 12 fused encode, else 0."""
    affine = affine and nstripes > 1
    tiles = ceil_div(length, LK_TILE)
    per = min(nstripes if affine else LK_PTRS // (k + m), 65535)
    if route == LOOKUP:
        dy = -1
    elif m == 12:
        dy = 2
    elif m == 4 and k in (12, 16) and dyadic_blocks(coef, k, m, 4):
        dy = 4
    elif m == 6 and k == 6 and dyadic_blocks(coef, k, m, 2):
        dy = 2
    else:
        dy = 0
    total = resident if route == LOOKUP and resident > 0 else LK_GROUPS
    fit = min(tiles, max(1, total // min(nstripes, per)), LK_MAX_GROUPS)
    tpw = ceil_div(tiles, fit)
    groups = ceil_div(tiles, tpw)
    return dict(tiles=tiles, per=per, dy=dy, affine=int(affine), groups=groups, tpw=tpw, gx=groups, gy=min(nstripes, per),
                ends=[min((g + 1) * tpw, tiles) * LK_TILE for g in range(groups)])
