"""Which kernels run a plain product (launch_matvec), restated from the kernels that exist
(chubaofs_amd/csrc: gf_k<K>.hip, gf_dy_k<K>.hip, gf_dy16.hip, gf_lut_k<K>.hip, the runtime-k cases of
gf_kernels.hip, gf_bs16.hip, gf_bs_crc.hip) without calling the library.  tests/test_matvec_route.py
pins the library's plan_matvec to this table on the CPU; tests/test_gpu_matvec_routes.py asserts that
the launches each GPU case traces are the ones the table names."""
import crc_routes as R

STORE, ACCUM, VERIFY, STORE_VERIFY = 0, 1, 2, 3
MODE_NAMES = {STORE: "store", ACCUM: "accum", VERIFY: "verify", STORE_VERIFY: "store-verify"}
RUNTIME_K, FIXED_K, DYADIC, DYADIC16, LOOKUP, BS_PLAIN = "runtime-k", "fixed-k", "dyadic", "dyadic-16", "lookup", "bs-plain"
FAMILIES = {RUNTIME_K, FIXED_K, DYADIC, DYADIC16, LOOKUP, BS_PLAIN}
PREFIXES = {"none", "encode", "verify", "table"}

MAX_ROWS = 32        # inputs and outputs one argument block carries
PTR_SLOTS = 288      # row pointers one argument block carries
LEN_SLOTS = 32       # per-stripe lengths one argument block carries
BS_TILE = 2048       # bytes of a row per tile of the bit-sliced 16 + 20 network
MAX_LEN = 0xFFFFFFFF - 4096  # 32-bit lane offsets of the fixed-K kernels and their kin

# ---- the instantiation lists
# gf_k<K>.hip: launch_k<K, mode, fixed_max_m(K)> for kStore, kVerify, kStoreVerify, m = 1 .. max
FIXED_MAX_M = {3: 6, 4: 6, 6: 12, 7: 6, 8: 8, 10: 6, 12: 12, 15: 12, 16: 24, 18: 4}
# gf_dy_k<K>.hip: (k, block, plain rows after the blocks) -> output counts; kStore and kVerify
DYADIC_M = {(6, 2, 0): (6, 8, 10, 12), (6, 2, 2): (12,), (12, 4, 0): (4, 8, 12),
            (16, 4, 0): (4, 8, 12, 16, 20), (16, 4, 2): (22,)}
DYADIC16_M = (20, 22)  # gf_dy16.hip, k = 16; kStore and kVerify
# gf_lut_k<K>.hip: k -> output counts; kStore, kVerify, kStoreVerify
LOOKUP_M = {6: range(5, 13), 12: range(5, 10), 15: range(5, 13), 16: range(5, 17)}
# gf_kernels.hip launch_mode: (rows per wave, waves per column chunk); every mode
RUNTIME_SHAPES = {(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (4, 2), (5, 2), (6, 2), (4, 4), (5, 4), (6, 4), (8, 4)}
BS_PLAIN_SHAPES = {(6, 15), (6, 18)}  # gf_bs_crc.hip launch_bs_plain: EC6P6L9, EC6P8L10; kStore
BS16_M = (20, 22)                     # gf_bs16.hip: the EC16P20L2 network's first 20 / 22 rows, k = 16


def has_kernel(family, k, m, mode, M=0, OS=0, threads=0, B=0, E=0):
    """An instantiation of `family` exists for a launch of m rows over k inputs."""
    if family == RUNTIME_K:
        return (1 <= k <= MAX_ROWS and 1 <= m <= MAX_ROWS and (M, OS) in RUNTIME_SHAPES and M * OS >= m
                and threads in (128, 256) and threads % (64 * OS) == 0)
    if family == FIXED_K:
        return k in FIXED_MAX_M and 1 <= m <= FIXED_MAX_M[k] and mode in (STORE, VERIFY, STORE_VERIFY)
    if family == DYADIC:
        return m in DYADIC_M.get((k, B, E), ()) and mode in (STORE, VERIFY)
    if family == DYADIC16:
        return k == 16 and m in DYADIC16_M and mode in (STORE, VERIFY)
    if family == LOOKUP:
        return m in LOOKUP_M.get(k, ()) and mode in (STORE, VERIFY, STORE_VERIFY)
    if family == BS_PLAIN:
        return (k, m) in BS_PLAIN_SHAPES and mode == STORE
    return False


# ---- the matrix forms the reduced-product kernels need

def blocks_hold(coef, k, rows, B):
    """Rows [0, rows) are made of B x B blocks with M[r0 + i][c0 + j] = M[r0][c0 + (i ^ j)]."""
    return all(coef[(r0 + i) * k + c0 + j] == coef[r0 * k + c0 + (i ^ j)]
               for r0 in range(0, rows, B) for c0 in range(0, k, B) for i in range(B) for j in range(B))


def dyadic_form(coef, k, m):
    """(B, E) of the dyadic-block kernel the matrix can take (all rows, else all but 2 plain ones)."""
    for (dk, B, E), ms in sorted(DYADIC_M.items(), key=lambda kv: kv[0][2]):
        if dk == k and m in ms and blocks_hold(coef, k, m - E, B):
            return B, E
    return None


def dyadic16_form(coef, k, m):
    """One 16 x 16 dyadic block, one row of 4 x 4 blocks, then (m = 22) two plain rows."""
    return (k == 16 and m in DYADIC16_M and blocks_hold(coef, 16, 16, 16)
            and blocks_hold(coef[256:], 16, 4, 4))


def is_bs16_network(coef, k, m):
    return k == 16 and m in BS16_M and b"".join(R.network_rows("ec16p20l2")[:m]) == bytes(coef)


def runtime_shape(mc):
    """Rows per wave and waves per column chunk: at most 6 rows in one wave, else 2 or 4 waves."""
    if mc <= 6:
        return mc, 1
    if mc <= 8:
        return 4, 2
    if mc <= 12:
        return -(-mc // 2), 2
    if mc <= 24:
        return -(-mc // 4), 4
    return 8, 4


def expect_plan(k, m, coef, mode, nstore, length, nstripes, affine=True, aligned=True, far=False, lens=None,
                lut=True, bs16=True, bstab=True, bs_mask=R.BS_CRC_DEFAULT):
    """The launches of one job, in order, or "error".  `affine`: every stripe at one stride from the
    one before (a single run); `aligned`: every row 16-byte aligned; `far`: the rows span 4 GiB or
    more; lens: per-stripe lengths (length is ignored).  Each launch: dict(family, bs, mode, r0, mc,
    c0, kc, s0, ns, off, prefix, tail, B, E)."""
    coef = bytes(coef)
    if mode == STORE_VERIFY:
        if not 0 <= nstore <= m:
            return "error"
        if nstore == m:
            mode = STORE
        elif nstore == 0:
            mode = VERIFY
        elif m > MAX_ROWS:
            return "error"
    longest = max(lens) if lens is not None else length
    if lens is not None and longest > 0xFFFFFFFF:
        return "error"
    if m == 0 or nstripes == 0 or longest == 0:
        return []
    if mode == STORE and R.expect_plain(k, m, coef, length, nstripes, lens=lens is not None, bs_mask=bs_mask):
        return [dict(family=BS_PLAIN, bs="none", mode=STORE, r0=0, mc=m, c0=0, kc=k, s0=0, ns=nstripes, off=0,
                     prefix=0, tail=length, B=0, E=0)]
    if mode in (VERIFY, STORE_VERIFY) and k > MAX_ROWS:
        return "error"
    one_chunk = k <= MAX_ROWS and m <= MAX_ROWS
    # the reduced-product kernels read the whole matrix: single-chunk jobs only, no stored/compared split
    d16 = one_chunk and mode != STORE_VERIFY and dyadic16_form(coef, k, m)
    dy = one_chunk and mode != STORE_VERIFY and not d16 and dyadic_form(coef, k, m)
    network = bs16 and one_chunk and lens is None and aligned and length >= BS_TILE and is_bs16_network(coef, k, m)
    whole_tiles = length // BS_TILE * BS_TILE
    steps = []
    for r0 in range(0, m, MAX_ROWS):
        mc = min(MAX_ROWS, m - r0)
        for c0 in range(0, k, MAX_ROWS):
            kc = min(MAX_ROWS, k - c0)
            smode = ACCUM if mode == STORE and c0 else mode
            # a kernel compiled for the input count: the inputs in one chunk, the outputs within its list
            compiled = k in FIXED_MAX_M and mc <= FIXED_MAX_M[k] and smode != ACCUM and longest <= MAX_LEN
            B, E = dy if (compiled and dy) else (0, 0)
            if not compiled:
                family = RUNTIME_K
            elif lut and mc in LOOKUP_M.get(k, ()) and not (k == 6 and dy):
                family = LOOKUP  # (k = 6 keeps its 2x2-dyadic kernel where the matrix has the form)
            elif d16:
                family = DYADIC16
            elif dy:
                family = DYADIC
            else:
                family = FIXED_K
            cap = nstripes if affine else PTR_SLOTS // (kc + mc)
            if lens is not None:
                cap = min(cap, LEN_SLOTS)
            assert nstripes << 22 < 2 ** 31 and (family == RUNTIME_K or nstripes <= 65535), "grid limits: not modelled"
            common = dict(family=family, mode=smode, r0=r0, mc=mc, c0=c0, kc=kc, B=B, E=E)
            off = 0
            if network and smode == STORE and not affine and nstripes > cap and bstab and not far:
                steps.append(dict(common, bs="table", s0=0, ns=nstripes, off=0, prefix=whole_tiles, tail=0))
                off = whole_tiles
                if off == length:
                    continue
            for s0 in range(0, nstripes, cap):
                ns = min(cap, nstripes - s0)
                run = length if lens is None else max(lens[s0:s0 + ns])
                if run == 0:
                    continue
                bs = "none"
                if network and not off:
                    if smode == STORE:
                        bs = "encode"
                    elif smode == VERIFY and (affine or ns == 1):  # one pointer set for the run
                        bs = "verify"
                prefix = whole_tiles if bs != "none" else 0
                steps.append(dict(common, bs=bs, s0=s0, ns=ns, off=off, prefix=prefix, tail=run - off - prefix))
    return steps


def trace_line(step, affine):
    """The CFSEC_TRACE_MATVEC line of a launch of expect_plan."""
    return ("cfsec: matvec family=%s bs=%s mode=%s k=%d m=%d r0=%d c0=%d stripes=%d prefix=%d tail=%d affine=%d"
            % (step["family"], step["bs"], MODE_NAMES[step["mode"]], step["kc"], step["mc"], step["r0"], step["c0"],
               step["ns"], step["prefix"], step["tail"], 1 if affine and step["family"] != BS_PLAIN else 0))
