"""Batches of mixed stripe lengths, and batches split over launches, for every kernel body of the plain
product and of the 16 + 20 repair: the geometry restated from the kernels, the case table, and the
reference image of every case -- without calling the library.

A batch whose bids differ in size reaches the launchers as one job with per-stripe lengths (batch.cpp
launch_group_run: MatVecJob::lens, Dy16RepairJob::lens).  Such a job is never affine, is cut into
launches of min(288 / (k + m), 32) stripes (gf_device.hpp kPtrSlots, kLenSlots), and every launch carries
slen[s] = lens[s0 + s], flags + s0 and the run's longest stripe as its length.  Seven kernel bodies read
their stripe's length from that block, each with its own ragged-end clamp, byte path for rows shorter
than a lane chunk and exit for tiles past the stripe's end:

  runtime-k   gf_device.hpp matvec        16-byte chunks, tile = threads / OS * 16 * W; the accumulate form
                                          cannot re-code bytes and keeps the byte tail
  fixed-k     gf_device.hpp matvec_k      4 * fixed_lane_dwords bytes (8 from CFSEC_LANE8_MIN_M rows up), 256 lanes
  dyadic      gf_dyadic.hpp matvec_dy     16 bytes, DyShape: every row block in one wave, 4 column waves of 64 lanes
  dyadic-16   gf_dyadic16.hpp matvec_dy16 4 * CFSEC_DY16_W bytes, 256 lanes (gf_dy16.hip launches W = 2)
  repair      gf_dyadic16.hpp repair_dy16 the same W
  lookup      gf_lut.hpp gf_lut_kernel    4 * lut_lane_dwords(k) bytes, 256 lanes

tests/test_varlen_geometry.py pins the tiles to the library's plan, proves on the CPU that the table
reaches every class below and runs the reference alone; tests/test_gpu_varlen_edges.py runs every case on
the GPU in a pool of pitched slices with random slack, against the image and the statuses built here."""
import collections

import numpy as np

import matvec_routes as MR

PTR_SLOTS, LEN_SLOTS = MR.PTR_SLOTS, MR.LEN_SLOTS
LANE8_MIN_M = 10   # gf_device.hpp CFSEC_LANE8_MIN_M: fixed-K kernels of that many rows code 8 bytes per lane
LUT_K12_LW = 4     # gf_lut_launch.hpp CFSEC_LUT_K12_LW: dwords per lane of the k = 12 lookup kernels (else 2)
DY16_W = 2         # gf_dy16.hip CFSEC_DY16_W: dwords per lane of the dyadic-16 product and repair kernels
REPAIR = "repair"  # repair_dy16, beside matvec_routes' product families
MAX_LEN = 9 * 1024
ERR_VERIFY = 10    # ec.ErrVerify (oracle/ec_oracle.py ERR_VERIFY)
EXTRA = 3          # stripes past one launch's capacity

STORE, ACCUM, VERIFY, STORE_VERIFY = MR.STORE, MR.ACCUM, MR.VERIFY, MR.STORE_VERIFY


def geometry(family, mode, kc, mc):
    """(C, T): the bytes one lane codes and the bytes of a row one workgroup codes."""
    if family == MR.FIXED_K:
        C = 8 if mc >= LANE8_MIN_M else 16
        return C, 256 * C
    if family == MR.LOOKUP:
        C = 4 * (LUT_K12_LW if kc == 12 else 2)
        return C, 256 * C
    if family == MR.DYADIC:
        return 16, 64 * 16 * 4
    if family in (MR.DYADIC16, REPAIR):
        return 4 * DY16_W, 256 * 4 * DY16_W
    assert family == MR.RUNTIME_K
    _, OS = MR.runtime_shape(mc)
    verify = mode in (VERIFY, STORE_VERIFY)
    threads = 128 if verify and OS == 1 else 256  # (gf_kernels.hip plan_matvec: single-wave Verify)
    return 16, threads // OS * 16 * (2 if verify else 1)


def edge_lengths(C, T):
    return [1, C - 1, C, C + 1, 2 * C - 1, T - C - 1, T - 1, T, T + 1, T + C - 1, 2 * T, 2 * T + 17]


def stripe_lengths(C, T, n, cap):
    """n lengths for launches of `cap` stripes: the edge lengths in an order that puts the tile edges
    first (the short tables hold them), the first launch's last stripe shorter than a chunk, the
    second launch's first the longest of all -- so the longest stripe of the batch is not its first, and
    the two launches differ in the length they carry -- and stripe j of the second launch never of the
    length of stripe j of the first."""
    order = [T - 1, T, 2 * T, T + 1, C + 1, 1, 2 * C - 1, T + C - 1, C, T - C - 1, C - 1]
    assert sorted(order + [2 * T + 17]) == sorted(edge_lengths(C, T)) and n > cap >= 4
    first = [order[i % len(order)] for i in range(cap - 1)] + [C - 1]
    rest, i = [2 * T + 17], cap - 1
    while len(first) + len(rest) < n:
        j = (len(first) + len(rest)) % cap
        if order[i % len(order)] != first[j]:
            rest.append(order[i % len(order)])
        i += 1
    return first + rest


# ---------------------------------------------------------------------------------- the case table

# api: "encode" ReedSolomon(k, m).EncodeStripes | "lrc-encode" ec.EncodeBatch of the mode, EnableVerify off |
#      "verify" VerifyStripes | "repair" ec.ReconstructBatch(bids, bad, verify) on Tactic(k, m, 0, 1, k, 0, 0), or
#      on the LRC mode `lrc`
# family / mode / kc / mc: the launch the stripe count and the lengths are made for (a job of several
#      chunks: the chunk named in the comment); bad: the shards lost; uniform: one length, T + C - 1;
#      shift: row 1 of every stripe starts 1 byte late
Case = collections.namedtuple("Case", "name api k m family mode kc mc bad verify lrc uniform shift")


def _case(name, api, k, m, family, mode, kc=None, mc=None, bad=(), verify=False, lrc=None, uniform=False, shift=False):
    return Case(name, api, k, m, family, mode, k if kc is None else kc, m if mc is None else mc, tuple(bad), verify, lrc,
                uniform, shift)


EC6P10L2, EC16P20L2 = (6, 10, 2, 2), (16, 20, 2, 2)  # N, M, L, AZCount

CASES = [
    # -- Store
    _case("store-dyadic4-12x4", "encode", 12, 4, MR.DYADIC, STORE),
    _case("store-dyadic2-6x6", "encode", 6, 6, MR.DYADIC, STORE, shift=True),
    _case("store-dyadic2e2-ec6p10l2", "lrc-encode", 6, 12, MR.DYADIC, STORE, lrc=EC6P10L2),
    _case("store-dyadic16-16x20", "encode", 16, 20, MR.DYADIC16, STORE),
    _case("store-dyadic16-ec16p20l2", "lrc-encode", 16, 22, MR.DYADIC16, STORE, lrc=EC16P20L2),
    _case("store-lookup-12x9", "encode", 12, 9, MR.LOOKUP, STORE),
    _case("store-lookup-15x12", "encode", 15, 12, MR.LOOKUP, STORE),
    _case("store-lookup-6x5", "encode", 6, 5, MR.LOOKUP, STORE),
    _case("store-fixed-10x4", "encode", 10, 4, MR.FIXED_K, STORE),
    _case("store-fixed-16x17-lane8", "encode", 16, 17, MR.FIXED_K, STORE),
    _case("store-fixed-8x1", "encode", 8, 1, MR.FIXED_K, STORE),
    _case("store-fixed-18x1", "encode", 18, 1, MR.FIXED_K, STORE),
    _case("store-runtime-5x2-1wave", "encode", 5, 2, MR.RUNTIME_K, STORE),
    _case("store-runtime-5x7-2waves", "encode", 5, 7, MR.RUNTIME_K, STORE),
    _case("store-runtime-5x13-4waves", "encode", 5, 13, MR.RUNTIME_K, STORE),
    _case("store-runtime-4x33-row-chunks", "encode", 4, 33, MR.RUNTIME_K, STORE, mc=32),  # rows [0, 32); row 32: fixed-k
    # inputs [0, 32) stored in launches of 8, input 32 accumulated in launches of 32: made for the latter
    _case("accum-runtime-33x2", "encode", 33, 2, MR.RUNTIME_K, ACCUM, kc=1),
    # -- Verify
    _case("verify-dyadic4-12x4", "verify", 12, 4, MR.DYADIC, VERIFY),
    _case("verify-dyadic2-6x6", "verify", 6, 6, MR.DYADIC, VERIFY),
    _case("verify-dyadic16-16x20", "verify", 16, 20, MR.DYADIC16, VERIFY),
    _case("verify-lookup-12x9", "verify", 12, 9, MR.LOOKUP, VERIFY),
    _case("verify-fixed-10x4", "verify", 10, 4, MR.FIXED_K, VERIFY, shift=True),
    _case("verify-fixed-16x17-lane8", "verify", 16, 17, MR.FIXED_K, VERIFY),
    _case("verify-runtime-5x2-1wave", "verify", 5, 2, MR.RUNTIME_K, VERIFY),
    _case("verify-runtime-5x7-2waves", "verify", 5, 7, MR.RUNTIME_K, VERIFY),
    # -- kStoreVerify: Reconstruct + Verify in one launch
    _case("sv-fixed-12x4", "repair", 12, 4, MR.FIXED_K, STORE_VERIFY, bad=[3], verify=True),
    _case("sv-lookup-15x12", "repair", 15, 12, MR.LOOKUP, STORE_VERIFY, bad=[2, 20], verify=True),
    _case("sv-runtime-5x7", "repair", 5, 7, MR.RUNTIME_K, STORE_VERIFY, bad=[1, 6], verify=True),
    _case("sv-fixed-16x20-5-data-lost", "repair", 16, 20, MR.FIXED_K, STORE_VERIFY, bad=[0, 3, 7, 11, 15], verify=True),
    # -- the 16 + 20 repair kernel: nd missing data shards and one parity shard
    _case("repair-nd1", "repair", 16, 20, REPAIR, STORE_VERIFY, bad=[5, 18], verify=True),
    _case("repair-nd2", "repair", 16, 20, REPAIR, STORE_VERIFY, bad=[0, 9, 35], verify=True),
    _case("repair-nd3", "repair", 16, 20, REPAIR, STORE_VERIFY, bad=[2, 3, 14, 16], verify=True),
    _case("repair-nd4", "repair", 16, 20, REPAIR, STORE_VERIFY, bad=[1, 6, 10, 15, 27], verify=True),
    _case("repair-nd2-e2-ec16p20l2", "repair", 16, 20, REPAIR, STORE_VERIFY, bad=[0, 1, 16, 17], verify=True, lrc=EC16P20L2),
    _case("repair-nd0", "repair", 16, 20, REPAIR, STORE_VERIFY, bad=[21], verify=True),
    # -- a general matrix, stored: Reconstruct of m shards without Verify
    _case("rec-fixed-12x4", "repair", 12, 4, MR.FIXED_K, STORE, bad=[1, 7, 12, 15]),
    _case("rec-lookup-12x9", "repair", 12, 9, MR.LOOKUP, STORE, bad=[0, 2, 5, 11, 12, 14, 17, 19, 20]),
    _case("rec-runtime-5x2", "repair", 5, 2, MR.RUNTIME_K, STORE, bad=[2, 5]),
    # -- one length, scattered, more stripes than one argument block holds: lens == NULL, s0 > 0
    _case("uniform-verify-dyadic4-12x4", "verify", 12, 4, MR.DYADIC, VERIFY, uniform=True),
    _case("uniform-sv-fixed-12x4", "repair", 12, 4, MR.FIXED_K, STORE_VERIFY, bad=[3], verify=True, uniform=True),
    _case("uniform-verify-runtime-5x2", "verify", 5, 2, MR.RUNTIME_K, VERIFY, uniform=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def rows_of(c):
    """(inputs, outputs, stored): the shards a stripe's product reads, those it writes or compares --
    the first `stored` of them written -- as RSEngine::plan_stripe orders them (reedsolomon.go
    reconstruct, then Verify's compared rows: the present parity shards that are no inputs)."""
    total = c.k + c.m if c.lrc is None else c.lrc[0] + c.lrc[1]
    k = c.k
    if c.api in ("encode", "lrc-encode"):
        return list(range(k)), list(range(k, k + c.m)), c.m
    if c.api == "verify":
        return list(range(k)), list(range(k, k + c.m)), 0
    ins = [i for i in range(total) if i not in c.bad][:k]
    outs = [i for i in c.bad if i < k] + [i for i in c.bad if i >= k]
    stored = len(outs)
    if c.verify:
        outs += [i for i in range(k, total) if i not in c.bad and i not in ins]
        if c.lrc:
            outs += list(range(total, total + c.lrc[2]))  # the local parities, compared in the global pass
    return ins, outs, stored


def nshards(c):
    return c.k + c.m if c.lrc is None else sum(c.lrc[:3])


def repair_nd_e(c):
    return sum(i < 16 for i in c.bad), (c.lrc[2] if c.lrc else 0)


def capacity(c):
    """Stripes of one launch of the chunk the case is made for."""
    if c.family == REPAIR:
        nd, e = repair_nd_e(c)
        cap = PTR_SLOTS // (16 + nd + 20 + e)
    elif c.api in ("encode", "lrc-encode", "verify"):
        cap = PTR_SLOTS // (c.kc + c.mc)
    else:
        ins, outs, _ = rows_of(c)
        cap = PTR_SLOTS // (len(ins) + len(outs))
    return cap if c.uniform else min(cap, LEN_SLOTS)


def slot_bound(c):
    return not c.uniform and capacity(c) == LEN_SLOTS


def lengths(c):
    C, T = geometry(c.family, c.mode, c.kc, c.mc)
    cap = capacity(c)
    if c.uniform:
        return [T + C - 1] * (cap + EXTRA)
    return stripe_lengths(C, T, cap + EXTRA, cap)


def corruptions(c):
    """[(stripe, shard, byte)]: one flipped byte in each of the first two launches, in a compared row.
    First launch: the last byte of its last stripe (shorter than a chunk: the byte path; in a uniform
    case inside the clamped last chunk).  Second launch: its first stripe (the longest: C < len,
    len % C != 0), the first byte of the overlapped last chunk -- stripe 0 of the first launch is clean."""
    ins, outs, stored = rows_of(c)
    compared = outs[stored:]
    if not compared:
        return []
    C, _ = geometry(c.family, c.mode, c.kc, c.mc)
    lens, cap = lengths(c), capacity(c)
    assert lens[cap] > C and lens[cap] % C != 0 and (c.uniform or lens[cap - 1] < C)
    return [(cap - 1, compared[-1], lens[cap - 1] - 1), (cap, compared[0], lens[cap] - C)]


# ---------------------------------------------------------------------------------- the launches expected

def gf_tables():
    from oracle import oracle as O
    return O.tables()["mulTable"]


def gf_matmul(a, b):
    mul = gf_tables()
    out = np.zeros((a.shape[0], b.shape[1]), np.uint8)
    for j in range(a.shape[1]):
        out ^= mul[a[:, j][:, None], b[j][None, :]]
    return out


def generator(c):
    """Every shard as a row over the data, from the oracle's matrices alone: the Reed-Solomon matrix,
    then (LRC) each local parity as its AZ's local code over the AZ's rows (lrcencoder.go)."""
    from oracle import oracle as O
    from oracle.ec_oracle import layout_by_az
    if c.lrc is None:
        return O.build_matrix(c.k, c.k + c.m)
    N, M, L, AZ = c.lrc
    G = O.build_matrix(N, N + M)
    ln, lm = (N + M) // AZ, L // AZ
    local = O.build_matrix(ln, ln + lm)[ln:]
    rows = [gf_matmul(local, G[layout_by_az(N, M, L, AZ)[a][:ln]]) for a in range(AZ)]
    return np.concatenate([G] + rows)


def product_matrix(c):
    """The coefficient rows of the case's product, outputs over inputs."""
    from oracle import oracle as O
    ins, outs, _ = rows_of(c)
    G = generator(c)
    if ins == list(range(c.k)):
        return G[outs]
    err, dec = O.invert(G[ins])
    assert err == 0
    return gf_matmul(G[outs], dec)


def expected_steps(c):
    """The launches of the case's one batch call, in order: matvec_routes.expect_plan's steps, or for
    the repair kernel plan_dy16_repair's varlen branch restated (no bit-sliced prefix, no affine run)."""
    lens = lengths(c)
    n = len(lens)
    if c.family == REPAIR:
        nd, e = repair_nd_e(c)
        per = min(PTR_SLOTS // (16 + nd + 20 + e), LEN_SLOTS)
        return [dict(family=REPAIR, bs="none", mode=STORE_VERIFY, nd=nd, e=e, kc=16, mc=nd + 20 + e, s0=s0,
                     ns=min(per, n - s0), prefix=0, tail=max(lens[s0:s0 + per])) for s0 in range(0, n, per)]
    ins, outs, stored = rows_of(c)
    mode = STORE_VERIFY if c.api in ("verify", "repair") else STORE
    steps = MR.expect_plan(len(ins), len(outs), product_matrix(c).tobytes(), mode, stored, lens[0], n, affine=False,
                           aligned=not c.shift, lens=None if c.uniform else lens)
    assert steps != "error"
    return steps


def expected_trace(c):
    """The CFSEC_TRACE_MATVEC lines of those launches, as dicts of their fields."""
    out = []
    for s in expected_steps(c):
        if s["family"] == REPAIR:
            out.append(dict(kind="repair", bs="none", nd=str(s["nd"]), e=str(s["e"]), s0=str(s["s0"]), stripes=str(s["ns"]),
                            prefix="0", tail=str(s["tail"]), affine="0"))
        else:
            out.append(dict(fields(MR.trace_line(s, False)), kind="matvec"))
    return out


def primary_steps(c):
    """The launches of the chunk the case is made for."""
    return [s for s in expected_steps(c) if (s["family"], s["mode"], s["kc"], s["mc"]) == (c.family, c.mode, c.kc, c.mc)
            or c.family == REPAIR]


def fields(line):
    return dict(x.split("=") for x in line.split()[2:])


def parse_trace(err):
    out = []
    for ln in err.splitlines():
        for kind in ("matvec", "repair"):
            if ln.startswith("cfsec: %s " % kind):
                out.append(dict(fields(ln), kind=kind))
    return out


# ---------------------------------------------------------------------------------- pools and references

def round_up(a, b):
    return -(-a // b) * b


def bid_slots(c, n):
    """The pool slot of every bid: back to back, or (uniform) with gaps of 0, 1, 0, 1, ... slots."""
    return [b + b // 2 if c.uniform else b for b in range(n)]


class Pool:
    """One case as one pool: every shard a slice at pitch round_up(longest, 256) + 256 whatever its own
    length (a uniform case: the bids at uneven gaps, so that no three sit at one stride), seeded random
    bytes everywhere else.  before: the image handed to the library; want: the image the reference
    leaves; status: the reference's status per stripe; clean: no byte of the stripe flipped."""

    def __init__(self, c):
        from oracle.ec_oracle import ECOracle, Slice
        self.case, self.lens, self.total = c, lengths(c), nshards(c)
        n, total = len(self.lens), self.total
        self.pitch = round_up(max(self.lens), 256) + 256
        assert max(self.lens) < MAX_LEN
        self.slot = bid_slots(c, n)
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name))
        rng = np.random.default_rng(seed)
        self.before = rng.integers(0, 256, 256 + (self.slot[-1] + 1) * total * self.pitch, dtype=np.uint8)
        self.want = None
        ins, outs, stored = rows_of(c)
        flips = {}
        for s, shard, byte in corruptions(c):
            flips.setdefault(s, []).append((shard, byte))
        self.clean = [s not in flips for s in range(n)]
        lost = outs[:stored] if c.api != "verify" else []
        oracle = ECOracle(*c.lrc) if c.lrc else ECOracle(c.k, c.m)
        after, self.status = [], []
        for s, length in enumerate(self.lens):
            cw = [Slice.of(rng.integers(0, 256, length, dtype=np.uint8)) for _ in range(c.k)] + \
                 [Slice.of(np.zeros(length, np.uint8)) for _ in range(total - c.k)]
            assert oracle.encode(cw) == 0
            src = [x.view().copy() for x in cw]
            for shard, byte in flips.get(s, []):
                assert shard not in lost and shard >= c.k
                src[shard][byte] ^= 1 << ((s + byte) % 8)
            for i in lost:  # what the call is to write: junk of the pool's own
                src[i] = self.before[self.offset(s, i):self.offset(s, i) + length].copy()
            for i in range(total):
                self.before[self.offset(s, i):self.offset(s, i) + length] = src[i]
            work = [Slice.of(x) for x in src]
            if c.api in ("encode", "lrc-encode"):
                st = oracle.encode(work)
            elif c.api == "verify":
                ok, st = oracle.verify(work)
                st = st if st else 0 if ok else ERR_VERIFY
            else:
                st = oracle.repair(work, list(c.bad), verify=c.verify)
            self.status.append(st)
            after.append([w.view() for w in work])
            for i in range(total):  # the reference writes the lost shards and nothing else
                assert np.array_equal(after[s][i], cw[i].view() if i in lost else src[i]), (c.name, s, i)
        self.want = self.before.copy()
        for s, length in enumerate(self.lens):
            for i in range(total):
                self.want[self.offset(s, i):self.offset(s, i) + length] = after[s][i]

    def offset(self, s, i):
        return 256 + (self.slot[s] * self.total + i) * self.pitch + (1 if self.case.shift and i == 1 else 0)

    def check_reference(self):
        """The reference alone: status 0 for every clean stripe, ErrVerify for exactly the corrupted ones."""
        for s, st in enumerate(self.status):
            assert st == (0 if self.clean[s] else ERR_VERIFY), (self.case.name, s, self.lens[s], st)


_pools = {}


def pool(c):
    """The case's pool, built once per session; `before` and `want` stay as they are."""
    if c.name not in _pools:
        _pools[c.name] = Pool(c)
        _pools[c.name].before.setflags(write=False)
        _pools[c.name].want.setflags(write=False)
    return _pools[c.name]
