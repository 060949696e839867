"""The two repair kernels of the 16 + 20 code (EC16P20, EC16P20L2's global stripe) over the code they
select at run time by the erasure set: the host plan restated, the case table, the classes every case
belongs to and the oracle's image of every bid -- without calling the library.

  gf_bs16.hip       gf_bs16_repair_kernel<M, ND, TAB>  the bit-sliced syndrome form: whole 2 KiB tiles of
                                                       16-byte aligned rows, nd <= 2
  gf_dyadic16.hpp   repair_dy16<ND, E, ..., SLOTS>     row tails, nd = 3 and 4, rows shorter than a tile

What the erasure set selects: which of the 16 slots load from the zero tile (src[16]), whether a missing
slot comes through the LDS prefetch (slots 0..6) or a direct load, the branch body a solved row enters
the network through (one per slot, and the even slot of its pair in the paired basis), the row networks
of the stand-in parities (a 20-way switch), the host-inverted A^-1 tables at entry j * 4 + q, and the
store / compare / skip action of every parity row with the counted waits of the compared rows' ring.

tests/test_repair16_geometry.py proves on the CPU that the table reaches every class of REQUIRED and
runs the oracle alone on every bid; tests/test_gpu_repair16_sweep.py runs the table on the GPU against
the images and statuses built here and asserts the route of every launch."""
import collections
import re

import numpy as np

K, M = 16, 20
BS_TILE = 2048          # gf_launch.hpp kBs16Tile / gf_device.hpp kBsWaveBytes: a row's bytes per bit-sliced tile
BS_REPAIR_MAX_ND = 2    # gf_launch.hpp kBsRepairMaxNd (gf_kernels.hip plan_dy16_repair: `nd <= kBsRepairMaxNd`)
DY_MAX_ND = 4           # batch.cpp plan_dy16: `d->nd > 4` leaves the set to the product
REP_PREFETCH = 7        # gf_bs16.hip kRepPrefetch: slots 0..6 come through the LDS prefetch, 7..15 load direct
REP_RING = 3            # gf_bs16.hip kRepRing: LDS ring of compared rows per wave
REP_LOOKAHEAD = 2       # gf_bs16.hip: issue_ring() twice before the network, vmcnt(2) while two rows fly
PTR_SLOTS = 288         # gf_device.hpp kPtrSlots: row pointers one argument block carries
# gf_bs16.hip kBsTabWords: the words of GfArgs from coef to the end of ptr that a table launch keeps its row
# offsets in -- coef[32 * 32] at byte 84, slen[32], 4 bytes of padding, ptr[288] ending at byte 3544
BS_TAB_WORDS = (3544 - 84) // 4
ERR_VERIFY = 10         # ec.ErrVerify (oracle/ec_oracle.py ERR_VERIFY)

S = 4113                # two 2 KiB tiles and a 17-byte tail that the dyadic kernel codes as its last full 8-byte chunk
S_SHORT = 2047          # below the bit-sliced tile: the whole row on the dyadic kernel
S_BYTES = 5             # shorter than a lane's chunk: the dyadic kernel's byte path
S_TILES = 16 * BS_TILE + 17  # the several-tiles-per-wave test
CANARY, JUNK = 0xA5, 0xEE

Case = collections.namedtuple("Case", "name bad verify mode size")
Plan = collections.namedtuple("Plan", "nd e slot src prow pstore pcmp standin dropped nout takes bitsliced sym eqdiag")


def _matrix():
    from oracle import oracle as O
    global _G
    if _G is None:
        _G = O.build_matrix(K, K + M)
    return _G


_G = None


def restate(bad, verify, e, size=S):
    """batch.cpp plan_stripe + plan_dy16 for the shards `bad` of the global stripe lost, e extra compared
    rows (EC16P20L2's two local parities riding along, with verify only) and rows of `size` bytes."""
    bad = sorted(bad)
    assert all(0 <= i < K + M for i in bad) and len(set(bad)) == len(bad) and e in (0, 2) and (verify or e == 0)
    present = [i for i in range(K + M) if i not in bad]
    assert len(present) >= K
    inputs = present[:K]  # plan_stripe: the first k present rows in index order
    slot = [i for i in bad if i < K]
    nd = len(slot)
    nxt, src = 0, []
    for i in range(K):  # plan_dy16: `d->src[i] = present[i] ? slot++ : 16 + j++`
        src.append(K + slot.index(i) if i in slot else nxt)
        nxt += i not in slot
    prow = [i - K for i in inputs[K - nd:]] if nd else []  # `plan->in[16 - d->nd + q] - k_`: the first nd present parity rows
    assert all(p >= 0 for p in prow)
    pstore = sum(1 << (i - K) for i in bad if i >= K)
    spare = [i - K for i in present[K:]]
    pcmp = (sum(1 << p for p in spare) | (3 << M if e else 0)) if verify else 0
    dropped = 0 if verify else sum(1 << p for p in spare)
    standin = sum(1 << p for p in prow)
    assert pstore | pcmp | standin | dropped == (1 << (M + e)) - 1 and pstore + pcmp + standin + dropped == (1 << (M + e)) - 1
    nout = len(bad) + (len(spare) + e if verify else 0)  # plan->out: stored rows, then the compared ones
    # plan_dy16: `d->nd > 4 || 16 * d->nd + 117 + 16 * e >= 16 * (int)plan->out.size()`
    takes = nd <= DY_MAX_ND and 16 * nd + 117 + 16 * e < 16 * nout
    # plan_dy16_repair: `job.syn && kBs16 && nd <= kBsRepairMaxNd && !job.lens && job.len >= kBs16Tile`
    bitsliced = takes and nd <= BS_REPAIR_MAX_ND and size >= BS_TILE
    sym = eqdiag = None
    if nd == 2:  # A[q][j] = parity row prow[q] at missing data column slot[j]
        G = _matrix()
        A = [[int(G[K + prow[q]][slot[j]]) for j in range(2)] for q in range(2)]
        sym, eqdiag = A[0][1] == A[1][0], A[0][0] == A[1][1]
    return Plan(nd, e, slot, src, prow, pstore, pcmp, standin, dropped, nout, takes, bitsliced, sym, eqdiag)


def plan_of(c):
    """The global pass of the case: a bad local parity keeps the local rows out of it (batch.cpp
    LrcEncoder::reconstruct_batch `fuse`), the local pass follows."""
    glob = [i for i in c.bad if i < K + M]
    e = 2 if c.mode == "lrc" and c.verify and len(glob) == len(c.bad) else 0
    return restate(glob, c.verify, e, c.size)


def nshards(c):
    return K + M + (2 if c.mode == "lrc" else 0)


def bits(mask):
    return [i for i in range(32) if mask >> i & 1]


def compared_rows(c):
    """Shard indices of the rows the global pass compares, in row order."""
    return [K + p for p in bits(plan_of(c).pcmp)]


def tab_capacity(nd, e):
    """gf_bs16.hip bs_tab_stripes: stripes whose row offsets one argument block carries."""
    return BS_TAB_WORDS // (K + nd + M + e)


def expected_lines(c, nbids, affine):
    """The `cfsec: repair` lines of one group of nbids bids of the case (gf_kernels.hip plan_dy16_repair):
    bids at one 16-byte-multiple stride (affine), or every shard at its own 16-byte aligned address."""
    p = plan_of(c)
    if not p.takes:
        return []
    full = c.size // BS_TILE * BS_TILE if p.bitsliced else 0

    def line(bs, s0, ns, prefix, tail, aff):
        return dict(bs=bs, nd=str(p.nd), e=str(p.e), s0=str(s0), stripes=str(ns), prefix=str(prefix), tail=str(tail),
                    affine=str(int(aff)))
    if affine or nbids == 1:
        return [line("affine" if p.bitsliced else "none", 0, nbids, full, c.size - full, nbids > 1)]
    out = [line("table", 0, nbids, full, 0, False)] if p.bitsliced else []
    per = PTR_SLOTS // (K + p.nd + M + p.e)
    if c.size > full:
        out += [line("none", s0, min(per, nbids - s0), 0, c.size - full, False) for s0 in range(0, nbids, per)]
    return out


# ---------------------------------------------------------------------------------- the case table

def _case(name, data=(), par=(), local=(), verify=True, mode="rs", size=S):
    bad = sorted(data) + [K + p for p in sorted(par)] + [K + M + x for x in sorted(local)]
    return Case(name, tuple(bad), verify, mode, size)


def _below(p):
    return list(range(p))


# nd = 1: stand-in p (every parity row below it lost) for p = 0..19, every slot the missing one
ND1_SLOT = [(7 * p + 3) % 16 for p in range(16)] + [2, 9, 12, 15]
ND1_EXTRA = {0: [2, 3, 9], 3: [5, 6, 10, 11, 15], 6: [19], 9: [10, 12, 14, 16, 18], 12: [13, 14], 13: [17]}
# nd = 2: first stand-in p0 = 0..18, the second GAP rows further; slots: the 8 pairs, then mixed parities
ND2_GAP = [1, 2, 0, 1, 3, 0, 0, 1, 1, 1, 8, 0, 0, 0, 0, 0, 0, 0, 0]
ND2_SLOTS = [(2, 3), (4, 5), (0, 1), (6, 7), (8, 9), (10, 11), (4, 10), (14, 15), (12, 13), (7, 13), (2, 9), (5, 12),
             (0, 15), (6, 8), (3, 8), (1, 14), (10, 12), (11, 15), (0, 6)]
ND2_EXTRA = {0: [5, 7, 9], 3: [8, 9, 17], 5: [19], 8: [11, 13, 15, 16, 18]}

CASES = []
for _p in range(20):
    CASES.append(_case(f"nd1-standin{_p}-slot{ND1_SLOT[_p]}", [ND1_SLOT[_p]], _below(_p) + ND1_EXTRA.get(_p, [])))
for _p0 in range(19):
    _p1 = _p0 + 1 + ND2_GAP[_p0]
    _lost = [r for r in range(_p1) if r != _p0] + ND2_EXTRA.get(_p0, [])
    CASES.append(_case(f"nd2-standin{_p0}+{_p1}-slots{ND2_SLOTS[_p0][0]}+{ND2_SLOTS[_p0][1]}", ND2_SLOTS[_p0], _lost))
CASES += [
    _case("nd2-direct-odd-even", [9, 12], [0, 3]),           # odd then even, both loaded direct; stand-ins 1, 2
    _case("nd2-prefetch-even-even", [2, 6], [1, 2, 4]),      # stand-ins 0, 3
    # -- the compared rows' ring: 0..4 compared rows, and where they sit
    _case("cmp-0-nd0", [], range(20)),                       # the encode through the repair kernel
    _case("cmp-only-row19-nd0", [], range(19)),
    _case("cmp-only-row0-nd0", [], range(1, 20)),
    _case("cmp-2-nd0", [], [r for r in range(20) if r not in (0, 19)]),
    _case("cmp-3-nd0", [], [r for r in range(20) if r not in (3, 10, 17)]),
    _case("cmp-4-nd0", [], [r for r in range(20) if r not in (0, 7, 12, 18)]),
    _case("cmp-19-nd0", [], [5]),                            # varlen_cases' {21}
    _case("cmp-2-nd1-apart", [12], [r for r in range(20) if r not in (4, 9, 19)]),
    _case("cmp-3-nd2-apart", [3, 10], [r for r in range(20) if r not in (1, 2, 8, 13, 18)]),
    # -- stored (S) and compared (C) rows after the stand-ins
    _case("order-C-then-S-nd0", [], range(10, 20)),
    _case("order-C-then-S-nd2", [1, 4], range(12, 20)),
    _case("order-S-then-C-nd0", [], range(10)),
    _case("order-S-then-C-nd1", [15], [0, 1, 3, 4, 5, 6, 7]),
    _case("order-alternating-nd0", [], range(1, 20, 2)),
    _case("order-alternating-nd1", [2], range(2, 20, 2)),
    _case("order-alternating-nd2", [9, 10], range(3, 20, 2)),
    _case("order-SS-between-C-nd0", [], [1, 2, 5, 6, 7, 10, 11, 13, 14, 15, 16]),
    _case("order-SS-between-C-nd1", [12], [2, 3, 4, 7, 8, 12, 13, 14, 15, 18]),
    _case("order-SS-between-C-nd2", [0, 7], [3, 4, 5, 6, 9, 10, 17, 18]),
    _case("order-block-rows-nd0", [], [17, 19]),
    _case("order-block-rows-standin16-nd1", [10], list(range(16)) + [18]),
    _case("order-block-rows-standin16+17-nd2", [5, 9], list(range(16)) + [18]),
    # -- EC16P20L2: the two local parities compared in the global pass (e = 2), or a local pass after it
    _case("lrc-c5", [0, 1], [0, 1], mode="lrc"),
    _case("lrc-local-only-compared-nd0", [], range(20), mode="lrc"),
    _case("lrc-local-only-compared-nd1", [9], range(19), mode="lrc"),
    _case("lrc-local-only-compared-nd2", [5, 12], range(18), mode="lrc"),
    _case("lrc-local-with-global-nd0", [], [7], mode="lrc"),
    _case("lrc-local-with-global-nd1", [10], [4, 17], mode="lrc"),
    _case("lrc-local-with-global-nd2-standin-hi", [2, 15], list(range(15)) + [16], mode="lrc"),
    _case("lrc-bad-local-nd1", [3], [4], [0], mode="lrc"),
    _case("lrc-bad-local-nd2", [6, 11], [0], [1], mode="lrc"),
    # -- ReconstructStripes(verify=False): nd + 8 lost is the smallest count plan_dy16 takes
    _case("noverify-dropped-nd0", [], [1, 4, 5, 9, 12, 16, 17, 19], verify=False),
    _case("noverify-dropped-nd1", [12], [0, 1, 2, 6, 11, 16, 18, 19], verify=False),
    _case("noverify-dropped-nd2", [2, 15], [0, 3, 4, 8, 10, 15, 17, 18], verify=False),
    _case("noverify-below-nd0", [], [1, 4, 5, 9, 12, 16, 17], verify=False),
    _case("noverify-below-nd1", [12], [0, 1, 2, 6, 11, 16, 18], verify=False),
    _case("noverify-below-nd2", [2, 15], [0, 3, 4, 8, 10, 15, 17], verify=False),
    # -- the dyadic kernel alone: nd = 3 and 4 (every slot), short rows
    _case("dy-nd3-slots0+1+2", [0, 1, 2], [0]),              # varlen_cases' repair-nd3 set is {2, 3, 14, 16}
    _case("dy-nd3-slots3+4+5", [3, 4, 5], [1, 3, 8, 19]),
    _case("dy-nd3-slots6+7+8", [6, 7, 8], []),
    _case("dy-nd3-slots9+10+11-standin-hi-cmp2", [9, 10, 11], range(15)),
    _case("dy-nd3-slots12+13+14-standin-hi-cmp1", [12, 13, 14], range(16)),
    _case("dy-nd3-slots0+7+15-standin-hi-cmp0", [0, 7, 15], range(17)),
    _case("dy-nd4-slots0+5+10+15", [0, 5, 10, 15], [2]),
    _case("dy-nd4-slots1+4+11+14", [1, 4, 11, 14], [0, 2, 4, 6, 8, 10, 12]),
    _case("dy-nd4-slots2+7+8+13-standin-hi-cmp2", [2, 7, 8, 13], range(14)),
    _case("dy-nd4-slots3+6+9+12-standin-hi-cmp0", [3, 6, 9, 12], range(16)),
    _case("dy-short-nd1", [5], [2], size=S_SHORT),           # varlen_cases' {5, 18}
    _case("dy-short-nd2", [0, 9], [19], size=S_SHORT),       # varlen_cases' {0, 9, 35}
    _case("dy-bytes-nd1", [2], [7], size=S_BYTES),
    _case("dy-bytes-nd2", [9, 10], [0, 19], size=S_BYTES),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

FAMILIES = ["nd1", "nd2", "cmp-order", "lrc", "noverify", "dyadic"]


def family(c):
    head = c.name.split("-")[0]
    return {"nd1": "nd1", "nd2": "nd2", "cmp": "cmp-order", "order": "cmp-order", "lrc": "lrc", "noverify": "noverify",
            "dy": "dyadic"}[head]


def cases_of(fam):
    return [c for c in CASES if family(c) == fam]


# The scattered-layout test: a high stand-in, an asymmetric A, 0, 1 and 2 compared rows, alternating order,
# local-only-compared
SCATTERED = ["nd1-standin17-slot9", "nd1-standin19-slot15", "nd2-standin15+16-slots1+14", "nd2-standin16+17-slots10+12",
             "nd2-standin18+19-slots0+6", "nd2-standin4+8-slots8+9", "cmp-0-nd0", "cmp-only-row19-nd0", "cmp-2-nd0",
             "order-alternating-nd2", "lrc-local-only-compared-nd2", "lrc-c5"]
# The several-tiles-per-wave test: 1 compared row; alternating order; high stand-ins with an asymmetric A; and
# runs of consecutive compared rows (14 and 10), where nothing but the counted wait stands between a ring
# row's read and its DMA -- a stored row issued in between would be waited for with it
TILES = ["nd1-standin18-slot12", "order-alternating-nd1", "nd2-standin16+17-slots10+12", "cmp-19-nd0",
         "nd2-standin0+2-slots2+3"]


# ---------------------------------------------------------------------------------- classes

def _order(p):
    """S / C for the parity rows after the last stand-in (every row where nothing is missing)."""
    first = max(p.prow) + 1 if p.prow else 0
    return "".join("S" if p.pstore >> r & 1 else "C" for r in range(first, M) if (p.pstore | p.pcmp) >> r & 1)


def classes(c):
    p = plan_of(c)
    out = set()
    ncmp = len(bits(p.pcmp))
    if not c.verify:
        lost = len(c.bad)
        if p.takes and p.bitsliced and lost == p.nd + 8 and p.pcmp == 0 and p.dropped:
            out.add(f"noverify-dropped-nd{p.nd}")
        if not p.takes and lost == p.nd + 7:
            out.add(f"noverify-below-nd{p.nd}")
        return out
    if c.mode == "lrc":
        if not p.bitsliced:
            return out
        if p.e == 2:
            out.add(f"lrc-e2-nd{p.nd}")
            out.add("lrc-local-only-compared" if p.pcmp == 3 << M else "lrc-local-with-global")
        else:
            out.add("lrc-bad-local")
        return out
    if not p.takes:
        return out
    if not p.bitsliced:  # the dyadic kernel alone
        if c.size == S_SHORT:
            out.add(f"dy-short-nd{p.nd}")
        elif c.size == S_BYTES:
            out.add(f"dy-bytes-nd{p.nd}")
        elif p.nd in (3, 4):
            out |= {f"dy-nd{p.nd}-slot-{i}" for i in p.slot}
            if p.prow[-1] >= 16:
                out.add("dy-standin-hi")
            if ncmp <= 2:
                out.add(f"dy-cmp-{ncmp}")
        return out
    if c.size != S:
        return out
    # -- the bit-sliced route
    if p.nd == 1:
        out |= {f"nd1-slot-{p.slot[0]}", f"nd1-standin-{p.prow[0]}"}
    if p.nd == 2:
        s0, s1 = p.slot
        out |= {f"nd2-standin0-{p.prow[0]}", f"nd2-standin1-{p.prow[1]}"}
        if s0 // 2 == s1 // 2:
            out.add(f"nd2-pair-{s0 // 2}")
        else:
            out.add("nd2-%s-%s" % ("odd" if s0 & 1 else "even", "odd" if s1 & 1 else "even"))
        npf = sum(s < REP_PREFETCH for s in p.slot)
        out.add(["nd2-direct-both", "nd2-pf-split", "nd2-pf-both"][npf])
        if p.sym and p.eqdiag:
            out.add("nd2-sym")
        elif not p.sym:
            hi = sum(r >= 16 for r in p.prow)
            out.add(["nd2-asym-lo", "nd2-asym-mixed", "nd2-asym-hi"][hi])
    if ncmp <= 4:
        out.add(f"cmp-{ncmp}-nd{p.nd}")
    if p.pcmp == 1 << 19:
        out.add("cmp-only-row19")
    if p.nd == 0 and p.pcmp & 1:
        out.add("cmp-row0")
    seq = _order(p)
    if re.fullmatch("C+S+", seq):
        out.add("order-C-then-S")
    if re.fullmatch("S+C+", seq):
        out.add("order-S-then-C")
    if sum(a != b for a, b in zip(seq, seq[1:])) >= 4:
        out.add("order-alternating")
    if re.search("CS{2,}C", seq):
        out.add("order-SS-between-C")
    block = (p.pstore >> 16 & 15, p.pcmp >> 16 & 15, p.standin >> 16 & 15)
    if block[0] and block[1]:
        out.add("order-block-rows")
        if block[2]:
            out.add("order-block-rows-standin")
    return out


REQUIRED = (
    [f"nd1-slot-{i}" for i in range(16)] + [f"nd1-standin-{p}" for p in range(20)] +
    [f"nd2-standin0-{p}" for p in range(19)] + [f"nd2-standin1-{p}" for p in range(1, 20)] +
    [f"nd2-pair-{q}" for q in range(8)] +
    ["nd2-even-even", "nd2-odd-odd", "nd2-even-odd", "nd2-odd-even", "nd2-pf-both", "nd2-pf-split", "nd2-direct-both",
     "nd2-asym-lo", "nd2-asym-mixed", "nd2-asym-hi", "nd2-sym"] +
    [f"cmp-{n}-nd{x}" for n in range(5) for x in range(3)] + ["cmp-only-row19", "cmp-row0"] +
    ["order-C-then-S", "order-S-then-C", "order-alternating", "order-SS-between-C", "order-block-rows",
     "order-block-rows-standin"] +
    ["lrc-local-only-compared", "lrc-local-with-global", "lrc-bad-local"] + [f"lrc-e2-nd{x}" for x in range(3)] +
    [f"noverify-dropped-nd{x}" for x in range(3)] + [f"noverify-below-nd{x}" for x in range(3)] +
    [f"dy-nd3-slot-{i}" for i in range(16)] + [f"dy-nd4-slot-{i}" for i in range(16)] +
    ["dy-standin-hi"] + [f"dy-cmp-{n}" for n in range(3)] +
    [f"dy-short-nd{x}" for x in (1, 2)] + [f"dy-bytes-nd{x}" for x in (1, 2)])


def coverage(cases):
    """class name -> the names of the cases in it."""
    out = collections.defaultdict(list)
    for c in cases:
        for name in classes(c):
            out[name].append(c.name)
    return out


# ---------------------------------------------------------------------------------- bids and the oracle's images

FLIP_AT = [0, 2047, 2048, 4095, 4096, S - 1]  # clipped to the row: both kernels' compares, both sides of a tile edge

Bid = collections.namedtuple("Bid", "kind shard at bit")  # kind: clean / compared / input / blind


def bids_of(c, n0):
    """The bids of a case, the flips numbered from n0: one clean bid; one per compared row with one bit of
    that row flipped, for the first two and the last compared rows; one with a bit flipped in the last
    stand-in (nd > 0); one with a bit flipped in a present data row.  A flipped input is `blind` where
    nothing is compared: status 0 and rebuilt bytes that are not the codeword's."""
    p = plan_of(c)
    cmp_rows = compared_rows(c)
    if c.verify and not p.e and c.mode == "lrc":  # the local pass compares the local stripes
        cmp_rows = cmp_rows + [i for i in (K + M, K + M + 1) if i not in c.bad]
    picks = cmp_rows[:2] + cmp_rows[2:][-1:]
    present_data = [i for i in range(K) if i not in c.bad]
    flips = [("compared", r) for r in picks]
    kind = "input" if cmp_rows else "blind"
    if p.nd:
        flips.append((kind, K + p.prow[-1]))
    flips.append((kind, present_data[n0 % len(present_data)]))
    out = [Bid("clean", None, 0, 0)]
    for j, (k, shard) in enumerate(flips):
        n = n0 + j
        out.append(Bid(k, shard, min(FLIP_AT[n % len(FLIP_AT)], c.size - 1), (n + n // len(FLIP_AT)) % 8))
    return out


def table_bids():
    """case name -> its bids, the flip offsets rotating through the whole table."""
    out, n = {}, 0
    for c in CASES:
        out[c.name] = bids_of(c, n)
        n += len(out[c.name]) - 1
    return out


_codewords = {}


def codeword(mode, size, seed=0):
    """The codeword of (mode, size, seed), from the oracle's Encode: shared by every case, never written."""
    from oracle.ec_oracle import ECOracle, Slice
    key = (mode, size, seed)
    if key not in _codewords:
        rng = np.random.default_rng(1620 + 7 * size + (mode == "lrc") + 1000003 * seed)
        total = K + M + (2 if mode == "lrc" else 0)
        cw = [Slice.of(rng.integers(0, 256, size, dtype=np.uint8)) for _ in range(K)] + \
             [Slice.of(np.zeros(size, np.uint8)) for _ in range(total - K)]
        orc = ECOracle(K, M, 2, 2) if mode == "lrc" else ECOracle(K, M)
        assert orc.encode(cw) == 0
        _codewords[key] = [x.view().copy() for x in cw]
        for x in _codewords[key]:
            x.setflags(write=False)
    return _codewords[key]


def source(c, bid, cw=None):
    """The shards handed to the call: junk where lost, the codeword elsewhere, the bid's one bit flipped."""
    cw = codeword(c.mode, c.size) if cw is None else cw
    src = [np.full(len(cw[0]), JUNK, np.uint8) if i in c.bad else cw[i] for i in range(len(cw))]
    if bid.shard is not None:
        assert bid.shard not in c.bad
        src[bid.shard] = src[bid.shard].copy()
        src[bid.shard][bid.at] ^= 1 << bid.bit
    return src


def oracle_run(c, src):
    """(status, shards after) of the reference alone: Reconstruct then Verify (ECOracle.repair), or the C
    oracle's Reconstruct for verify=False."""
    from oracle import oracle as O
    from oracle.ec_oracle import ECOracle, Slice
    if not c.verify:
        work = [x.copy() for x in src]
        err, _ = O.reconstruct(K, M, work, [i not in c.bad for i in range(K + M)])
        return err, work
    orc = ECOracle(K, M, 2, 2) if c.mode == "lrc" else ECOracle(K, M)
    work = [Slice.of(x) for x in src]
    st = orc.repair(work, list(c.bad), verify=True)
    return st, [w.view().copy() for w in work]


def check_bid(c, bid, src, status, after, cw=None):
    """Each kind's expectation, on the oracle alone."""
    cw = codeword(c.mode, c.size) if cw is None else cw
    where = (c.name, bid)
    for i in range(len(cw)):
        if i not in c.bad:
            assert np.array_equal(after[i], src[i]), where  # the reference writes the lost shards and nothing else
    rebuilt_ok = all(np.array_equal(after[i], cw[i]) for i in c.bad)
    if bid.kind == "clean":
        assert status == 0 and rebuilt_ok, where
    elif bid.kind == "compared":  # (a local parity rebuilt by the local pass takes the flipped row's bytes in)
        assert status == ERR_VERIFY and all(np.array_equal(after[i], cw[i]) for i in c.bad if i < K + M), where
    elif bid.kind == "input":
        assert status == ERR_VERIFY, where
    else:
        assert bid.kind == "blind" and status == 0 and not rebuilt_ok, where


_results = {}


def results(c):
    """[(bid, source shards, status, shards after)] of the case, the oracle run once per session."""
    if c.name not in _results:
        out = []
        for bid in table_bids()[c.name]:
            src = source(c, bid)
            st, after = oracle_run(c, src)
            out.append((bid, src, st, after))
        _results[c.name] = out
    return _results[c.name]
