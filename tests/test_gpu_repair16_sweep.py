"""The two repair kernels of the 16 + 20 code over missing slots, stand-in parities and compare sets.

gf_bs16_repair_kernel (gf_bs16.hip) and repair_dy16 (gf_dyadic16.hpp) pick most of their code at run time
by the erasure set: the slots loaded from the zero tile, prefetched or direct; the branch body a solved
row enters the network through; the row networks of the stand-in parities (a 20-way switch); the A^-1
tables; the store / compare / skip action of every parity row and the counted waits of the compared
rows' ring.  tests/repair16_cases.py holds the table of erasure sets that reaches every such class
(tests/test_repair16_geometry.py proves it on the CPU) with, per case, a clean bid, bids with one bit of a
compared row flipped, one with a bit of the last stand-in flipped and one with a bit of a data row flipped.

Reference: the oracle's shards and statuses only (ECOracle.repair, the C oracle's Reconstruct for
verify=False), never another path of the library; everything is bit-exact.  The bids of one case sit at
one 256-byte-multiple pitch in one pool with at least 256 canary bytes after every shard and junk in the
lost shards; the whole pool image is compared after the call -- rebuilt shards, untouched survivors and
every canary byte -- and the per-bid statuses.  The `cfsec: repair` lines traced (CFSEC_TRACE_MATVEC) are
compared with the plan restated in repair16_cases: the route is asserted, not assumed.

Measured on the MI355X (pytest --durations): the nd = 1 table 0.42 s (it also builds the encoder and the
first codeword), the nd = 2 and the compare-count / order tables 0.16 s each, the LRC, no-verify and
dyadic-only tables 0.05 - 0.08 s, a scattered case 0.01 s for its two calls, a several-tiles case 0.14 -
0.27 s (150 MB of pool built, uploaded and compared); the whole module, 23 tests, 3.9 s.

Checked against scratch builds with one wrong value each (nothing committed): the A^-1 table read at
q * 4 + j fails every nd = 2 case but the symmetric one; row 11's network under `case 12` fails the nd =
1 and nd = 2 tables; the ring's vmcnt(2) as vmcnt(4) passes all but one bid of the small tables (their
copies presumably arrive from L2 in time) and fails every clean bid of the two several-tiles cases whose
compared rows follow each other -- where a stored row lies between two compared rows its store is waited
for together with the ring row, which hides a wait one row short."""
import random

import numpy as np
import pytest

import repair16_cases as R
from chubaofs_amd import codemode as cm
from chubaofs_amd.codemode import Tactic

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K, M = R.K, R.M
CANARY = R.CANARY


def pitch_of(size):
    return (size + 255) // 256 * 256 + 256  # at least 256 canary bytes after every shard


def encoder(mode):
    from chubaofs_amd import ec
    t = cm.GetTactic(cm.EC16P20L2) if mode == "lrc" else Tactic(K, M, 0, 1, K, 0, 0)
    return ec.NewEncoder(ec.Config(CodeMode=t, EnableVerify=False), device=0)


def fields(line):
    return dict(x.split("=") for x in line.split()[2:])


def repair_lines(err):
    return [fields(ln) for ln in err.splitlines() if ln.startswith("cfsec: repair ")]


def product_lines(err):
    return [ln for ln in err.splitlines() if ln.startswith("cfsec: matvec ")]


class Pool:
    """Bids, each (case, source shards, status, shards after), carved from one buffer: bid b's shard i at
    offset(b, i), canary bytes everywhere else.  before: the image handed to the library; want: the image
    the oracle leaves."""

    def __init__(self, bids, n, offsets, nbytes):
        self.bids, self.n, self.offsets = bids, n, offsets
        self.before = np.full(nbytes, CANARY, np.uint8)
        self.want = self.before.copy()
        self.status = [st for _, _, st, _ in bids]
        for b, (c, src, _, after) in enumerate(bids):
            assert len(src) == n
            for i in range(n):
                o = offsets[b][i]
                assert np.all(self.before[o:o + c.size + 16] == CANARY)  # no two shards overlap
                self.before[o:o + c.size] = src[i]
                self.want[o:o + c.size] = after[i]

    @classmethod
    def pitched(cls, bids, n):
        pitch = pitch_of(max(c.size for c, _, _, _ in bids))
        offsets = [[256 + (b * n + i) * pitch for i in range(n)] for b in range(len(bids))]
        return cls(bids, n, offsets, 256 + len(bids) * n * pitch)

    @classmethod
    def scattered(cls, bids, n, seed):
        """Every shard in a slot of its own, the slots shuffled over bids and shards, at a 16-byte aligned
        offset within the slot: no two bids at one stride on every row."""
        rnd = random.Random(seed)
        slot = pitch_of(max(c.size for c, _, _, _ in bids)) + 256
        perm = list(range(len(bids) * n))
        rnd.shuffle(perm)
        offsets = [[256 + perm[b * n + i] * slot + 16 * rnd.randrange(16) for i in range(n)] for b in range(len(bids))]
        return cls(bids, n, offsets, 256 + len(bids) * n * slot)

    def upload(self):
        pool = torch.from_numpy(self.before).cuda()
        assert pool.data_ptr() % 256 == 0
        views = [[pool[self.offsets[b][i]:self.offsets[b][i] + c.size] for i in range(self.n)]
                 for b, (c, _, _, _) in enumerate(self.bids)]
        return pool, views

    def check(self, pool, status):
        assert status == self.status, [(b, self.bids[b][0].name, status[b], self.status[b])
                                       for b in range(len(status)) if status[b] != self.status[b]][:8]
        image = pool.cpu().numpy()
        if not np.array_equal(image, self.want):  # rebuilt shards, survivors and every canary byte
            d = np.flatnonzero(image != self.want)
            at = int(d[0])
            o, b, i = max((o, b, i) for b, row in enumerate(self.offsets) for i, o in enumerate(row) if o <= at)
            pytest.fail(f"{d.size} bytes differ, first in bid {b} ({self.bids[b][0].name}, bad {self.bids[b][0].bad}) "
                        f"shard {i} at byte {at - o}")


def table_bids(cases):
    """Every bid of the cases, a case's bids consecutive; [(case, first bid, bids)]."""
    bids, groups = [], []
    for c in cases:
        res = R.results(c)
        for bid, src, st, after in res:
            R.check_bid(c, bid, src, st, after)  # each kind's expectation, on the oracle alone
        groups.append((c, len(bids), len(res)))
        bids += [(c, src, st, after) for _, src, st, after in res]
    return bids, groups


def check_standins(enc, c):
    """The library decodes from the stand-ins the plan restated names."""
    p = R.plan_of(c)
    glob = [i for i in c.bad if i < K + M]
    if p.nd:
        ins, _ = enc.repair_rows(glob, glob)
        assert ins[K - p.nd:] == [K + r for r in p.prow], (c.name, ins)
        assert ins[:K - p.nd] == [i for i in range(K) if i not in glob], (c.name, ins)


def run_family(fam, monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    cases = R.cases_of(fam)
    assert cases and len({c.mode for c in cases}) == 1 and all(c.verify for c in cases)
    bids, groups = table_bids(cases)
    pool = Pool.pitched(bids, R.nshards(cases[0]))
    enc = encoder(cases[0].mode)
    for c in cases:
        check_standins(enc, c)
    dev, views = pool.upload()
    capfd.readouterr()
    status = enc.ReconstructBatch(views, [list(c.bad) for c, _, _, _ in bids], verify=True)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    pool.check(dev, status)
    want = [ln for c, _, nb in groups for ln in R.expected_lines(c, nb, affine=True)]
    got = repair_lines(err)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:4] or (len(got), len(want))
    return cases, want


# ------------------------------------------------------------------ 1 - 4. the bit-sliced route

@pytest.mark.parametrize("fam", ["nd1", "nd2", "cmp-order", "lrc"])
def test_bitsliced_route(fam, monkeypatch, capfd):
    """One call per family, every case one affine group: the bit-sliced kernel on the two whole tiles,
    the dyadic kernel on the 17-byte tail."""
    cases, lines = run_family(fam, monkeypatch, capfd)
    assert len(lines) == len(cases)
    for c, ln in zip(cases, lines):
        assert (ln["bs"], ln["prefix"], ln["tail"], ln["affine"]) == ("affine", "4096", "17", "1"), c.name
        assert int(ln["nd"]) == R.plan_of(c).nd <= R.BS_REPAIR_MAX_ND and int(ln["e"]) == R.plan_of(c).e, c.name
    if fam == "lrc":
        assert {ln["e"] for ln in lines} == {"0", "2"}


# ------------------------------------------------------------------ 5. Reconstruct without Verify

def test_noverify(monkeypatch, capfd):
    """ReconstructStripes(verify=False): nd + 8 shards lost is the smallest count the repair kernel takes
    (nothing compared, the surviving spare parities neither stored nor compared), nd + 7 takes the
    product.  The call gives every lost shard a buffer of its own, so the bids sit at no common stride:
    the bit-sliced kernel over a table of row offsets, the tail on pointer-table launches."""
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    from chubaofs_amd import reedsolomon
    cases = R.cases_of("noverify")
    assert len(cases) == 6 and not any(c.verify for c in cases)
    bids, groups = table_bids(cases)
    pool = Pool.pitched(bids, K + M)
    dev, views = pool.upload()
    for b, (c, _, _, _) in enumerate(bids):
        for i in c.bad:
            views[b][i] = views[b][i][:0]  # missing: the call rebuilds it into a fresh buffer
    enc = reedsolomon.New(K, M, device=0)
    capfd.readouterr()
    status = enc.ReconstructStripes(views, verify=False)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert status == pool.status == [0] * len(bids)
    assert np.array_equal(dev.cpu().numpy(), pool.before)  # survivors, the lost shards' junk, every canary byte
    for b, (c, _, _, after) in enumerate(bids):
        for i in range(K + M):
            assert views[b][i].numel() == c.size and views[b][i].data_ptr() % 16 == 0, (c.name, b, i)
            if i in c.bad:
                assert np.array_equal(views[b][i].cpu().numpy(), after[i]), (c.name, b, i)
    want = [ln for c, _, nb in groups for ln in R.expected_lines(c, nb, affine=False)]
    assert repair_lines(err) == want, err
    assert [ln["bs"] for ln in want] == ["table", "none"] * 3
    assert len(product_lines(err)) == 3, err  # the three nd + 7 cases: the product, one launch each


# ------------------------------------------------------------------ 6. the dyadic kernel alone

def test_dyadic_only(monkeypatch, capfd):
    """nd = 3 and 4 over every slot, stand-ins among rows 16..19, 0 to 2 compared rows; rows of 2047
    bytes (below the bit-sliced tile) and of 5 bytes (the byte path)."""
    cases, lines = run_family("dyadic", monkeypatch, capfd)
    assert len(lines) == len(cases)
    for c, ln in zip(cases, lines):
        assert (ln["bs"], ln["prefix"], ln["tail"]) == ("none", "0", str(c.size)), c.name
    assert {ln["nd"] for ln in lines} == {"1", "2", "3", "4"}


# ------------------------------------------------------------------ 7. scattered layouts

@pytest.mark.parametrize("name", R.SCATTERED)
def test_scattered(name, monkeypatch, capfd):
    """Every shard at its own 16-byte aligned address, one bid count below and one above what the
    argument block's offset table holds (gf_bs16.hip bs_tab_stripes): the table in the argument block,
    then the table in device-visible memory; the tails on pointer-table launches."""
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    c = R.BY_NAME[name]
    p = R.plan_of(c)
    cap = R.tab_capacity(p.nd, p.e)
    assert cap == R.BS_TAB_WORDS // (K + p.nd + M + p.e) and 21 <= cap <= 24
    res = R.results(c)
    enc = encoder(c.mode)
    check_standins(enc, c)
    for nb in (cap - 1, cap + 1):
        bids = [(c,) + res[b % len(res)][1:] for b in range(nb)]
        pool = Pool.scattered(bids, R.nshards(c), seed=nb + len(name))
        dev, views = pool.upload()
        capfd.readouterr()
        status = enc.ReconstructBatch(views, [list(c.bad)] * nb, verify=True)
        torch.cuda.synchronize()
        err = capfd.readouterr().err
        pool.check(dev, status)
        want = R.expected_lines(c, nb, affine=False)
        assert repair_lines(err) == want, err
        assert (want[0]["bs"], want[0]["stripes"], want[0]["prefix"]) == ("table", str(nb), "4096")
        assert all(ln["bs"] == "none" and ln["tail"] == "17" for ln in want[1:]) and len(want) >= 4


# ------------------------------------------------------------------ 8. several tiles per wave

@pytest.mark.parametrize("name", R.TILES)
def test_several_tiles_per_wave(name, monkeypatch, capfd):
    """More tiles than the launch has waves, so that waves walk on to a next tile: its 7-row prefetch is
    issued between the ring's first two rows and the first compare, and the rows come from HBM, not from
    L2: the cases with runs of consecutive compared rows are the ones that need the ring's counted wait.
    Four distinct bids repeated: two clean codewords, a compared row flipped in a middle tile, and the last
    compared row flipped in its last tile."""
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    base = R.BY_NAME[name]
    c = base._replace(size=R.S_TILES)
    p = R.plan_of(c)
    assert p.bitsliced and p.pcmp
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = R.S_TILES // R.BS_TILE
    nb = 8 * cu // tiles + 1
    assert nb * tiles > 8 * cu  # 8 waves per CU, one workgroup per CU: some wave has a next tile
    rows = R.compared_rows(c)
    distinct = []
    for seed, bid in ((0, R.Bid("clean", None, 0, 0)), (1, R.Bid("clean", None, 0, 0)),
                      (0, R.Bid("compared", rows[0], 7 * R.BS_TILE + 1029, 5)),
                      (1, R.Bid("compared", rows[-1], tiles * R.BS_TILE - 1, 0))):
        cw = R.codeword(c.mode, c.size, seed)
        src = R.source(c, bid, cw)
        st, after = R.oracle_run(c, src)
        R.check_bid(c, bid, src, st, after, cw)
        distinct.append((c, src, st, after))
    assert [d[2] for d in distinct] == [0, 0, R.ERR_VERIFY, R.ERR_VERIFY]
    bids = [distinct[b % 4] for b in range(nb)]
    pool = Pool.pitched(bids, R.nshards(c))
    enc = encoder(c.mode)
    dev, views = pool.upload()
    capfd.readouterr()
    status = enc.ReconstructBatch(views, [list(c.bad)] * nb, verify=True)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    pool.check(dev, status)
    assert repair_lines(err) == R.expected_lines(c, nb, affine=True), err
    (ln,) = repair_lines(err)
    assert (ln["bs"], ln["stripes"], ln["prefix"], ln["tail"], ln["affine"]) == ("affine", str(nb), str(tiles * R.BS_TILE), "17", "1")
