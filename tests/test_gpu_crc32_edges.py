"""The standalone CRC32 pass (crc32.hip: crc32_horner_kernel, launch_crc32_to) at its group, tail and
launch-split edges, by design: tests/crc32_cases.py holds the case tables and tests/test_crc32_geometry.py
proves on the CPU that they reach every class of the launch geometry and of piece()'s loads.

Every word is compared bit-exact with zlib.crc32 and the C oracle's crc32_ieee (the two must agree
first), never with another path of the library.  Shards are carved from one device pool per test, filled
with 0xFF (so the zero padding past a shard's end sits next to 0xFF bytes), each in a slot of its own at
(256-aligned address) + offset; after every call the pool must equal its image before the call on the
device -- the pass writes no shard byte -- or, where a product runs first, the oracle's parity.  Every
call runs under CFSEC_TRACE_CRC32=1 and its lines must equal crc32_cases.launches: the launches, the
shards of each, groups, tpw, affine, idx and fin.

The data classes beside random bytes: all zero (the word depends on the length alone: `fin` and the host
finalize), one non-zero byte at position 0 and one at len - 1 (the group constant and the alignment
basis).

The idx + fin form runs through the public calls: encode_crc_batch on (5, 2), which no fused kernel
takes (crc_routes.expect_route: none), reconstruct_crc_batch on (10, 4), encode_crc_batch on a New(4, 0)
engine -- the ABI accepts m == 0, so that path is reachable and repair_crc_batch's no-parity path is the
same launch -- and a ReconstructBatch tasklet of three lengths (BatchRun::checksum).

Measured on the MI355X: the module's 56 tests 3.9 s of wall time inside pytest; the slowest are the three
25 MB shards of test_multi_group (0.28 s each: eight calls on a 200 MB pool) and the 92 MB list's setup
(0.28 s, shared by its two tests).  The 92 MB list fits, so pw = 6 is reached without the probe.
"""
import re
import zlib

import numpy as np
import pytest

import crc32_cases as G
import crc_routes as R
from chubaofs_amd import _lib, codemode as cm
from oracle import oracle as O
from oracle.ec_oracle import ECOracle, Slice

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CANARY = 0xFF
WORD_CANARY = 0xA5A5A5A5
GAP = 256  # untouched bytes at least after a shard
T = G.TILE
LINE = r"cfsec: crc32 len=(\d+) shards=(\d+) s0=(\d+) tiles=(\d+) groups=(\d+) tpw=(\d+) affine=(\d) idx=(\d) fin=(\d)"
FIELDS = ("len", "shards", "s0", "tiles", "groups", "tpw", "affine", "idx", "fin")


@pytest.fixture(scope="module")
def rs():
    from chubaofs_amd import reedsolomon
    return reedsolomon


@pytest.fixture(autouse=True)
def traced(monkeypatch):
    monkeypatch.setenv("CFSEC_TRACE_CRC32", "1")
    monkeypatch.delenv("CFSEC_CRC32_GROUPS_PROBE", raising=False)


def crc(a):
    """The reference word: zlib's, which the oracle's must equal."""
    a = np.ascontiguousarray(a)
    z = zlib.crc32(a.tobytes()) & 0xFFFFFFFF
    assert z == O.crc32_ieee(a)
    return z


def parse(err):
    return [dict(zip(FIELDS, map(int, g))) for g in re.findall(LINE, err)]


def trace(capfd):
    return parse(capfd.readouterr().err)


class Pool:
    """`nslots` slots for shards of up to `room` bytes at any offset below 256, from the first 256-aligned
    address of one device allocation filled with 0xFF."""

    def __init__(self, nslots, room):
        self.slot = G.ceil_div(room + 256 + GAP, 256) * 256
        total = nslots * self.slot + 256
        self.t = torch.empty(total, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()
        self.base = -self.ptr % 256
        self.img = np.full(total, CANARY, np.uint8)
        self.ref = None

    def at(self, k, off=0):
        return self.base + k * self.slot + off

    def put(self, k, off, data):
        """Bytes that belong at slot k + off; returns their device address."""
        assert 0 <= off and off + len(data) + GAP <= self.slot
        o = self.at(k, off)
        self.img[o:o + len(data)] = data
        return self.ptr + o

    def view(self, k, off, n):
        o = self.at(k, off)
        return self.t[o:o + n]

    def host(self, addr, n):
        o = addr - self.ptr
        assert 0 <= o and o + n <= self.img.size
        return self.img[o:o + n]

    def upload(self):
        self.t.copy_(torch.from_numpy(self.img))
        self.ref = self.t.clone()

    def expect(self):
        """The image changed on the host (rows a product is to write): the device must come to equal it."""
        self.ref.copy_(torch.from_numpy(self.img))

    def check(self):
        torch.cuda.synchronize()
        if not torch.equal(self.t, self.ref):
            got, want = self.t.cpu().numpy(), self.ref.cpu().numpy()
            i = int(np.flatnonzero(got != want)[0])
            k, off = divmod(i - self.base, self.slot)
            raise AssertionError(f"pool byte {i} (slot {k} + {off}) is {got[i]:#x}, expected {want[i]:#x}; "
                                 f"{int((got != want).sum())} bytes differ")


def data_classes(length, seed):
    """[(name, bytes)]: random, all zero, one non-zero byte at position 0, one at len - 1."""
    first, last = np.zeros(length, np.uint8), np.zeros(length, np.uint8)
    first[0], last[-1] = 0x80, 0x01
    return [("random", np.random.default_rng(seed).integers(0, 256, length, dtype=np.uint8)),
            ("zero", np.zeros(length, np.uint8)), ("first", first), ("last", last)]


def run(rs, capfd, pool, ptrs, length, total=G.TOTAL):
    """One cfsec_crc32_ieee_batch call: its words, with the trace and the pool checked."""
    capfd.readouterr()
    got = rs.crc32_ieee_batch(ptrs, length)
    assert trace(capfd) == G.launches(length, ptrs, total=total), (length, len(ptrs))
    pool.check()
    return got


def hexes(words):
    return [hex(w) for w in words]


# ------------------------------------------------------------------ length x pointer offset

@pytest.mark.parametrize("length", G.OFFSET_LENGTHS)
def test_length_by_offset(rs, capfd, length):
    """Per data class one call of 8 shards, each at its own pointer offset: every piece() path at every
    alignment, one group."""
    classes = data_classes(length, length)
    no = len(G.OFFSETS)
    pool = Pool(len(classes) * no, length)
    ptrs = [[pool.put(c * no + j, off, data) for j, off in enumerate(G.OFFSETS)] for c, (_, data) in enumerate(classes)]
    pool.upload()
    assert sorted(p % 256 for p in ptrs[0]) == sorted(G.OFFSETS)
    for c, (name, data) in enumerate(classes):
        want = crc(data)
        got = run(rs, capfd, pool, ptrs[c], length)
        assert got == [want] * no, (name, hexes(got), hex(want))
    assert G.plan(length, no, False).groups == 1


# ------------------------------------------------------------------ the group split

@pytest.mark.parametrize("length", G.MULTI_GROUP_LENGTHS)
def test_multi_group(rs, capfd, length):
    """One shard per call, every data class at pointer offsets 0 and 1: the group split, the last group's
    tiles, the clamp at 384 groups and the re-rounding past it, each group's constant and load-ahead."""
    classes = data_classes(length, length)
    cases = [(name, data, off) for name, data in classes for off in G.MULTI_GROUP_OFFSETS]
    pool = Pool(len(cases), length)
    ptrs = [pool.put(i, off, data) for i, (_, data, off) in enumerate(cases)]
    pool.upload()
    want = {name: crc(data) for name, data in classes}
    p = G.plan(length, 1, False)
    for (name, _, off), ptr in zip(cases, ptrs):
        capfd.readouterr()
        got = rs.crc32_ieee_batch([ptr], length)
        (line,) = trace(capfd)
        assert line == dict(len=length, shards=1, s0=0, tiles=p.tiles, groups=p.groups, tpw=p.tpw, affine=0, idx=0, fin=0)
        pool.check()
        assert got == [want[name]], (name, off, hexes(got), hex(want[name]))
    print(f"crc32 launch: len={length} tiles={p.tiles} groups={p.groups} tpw={p.tpw} last={p.ranges[-1][1] - p.ranges[-1][0]}")


# ------------------------------------------------------------------ lists: the launch split

class Shards:
    """n random shards of `length` bytes in a pool, shard i at pointer offset OFFSETS[i % 8]: no common
    stride.  The words are computed once."""

    def __init__(self, n, length, seed):
        data = np.random.default_rng(seed).integers(0, 256, (n, length), dtype=np.uint8)
        self.pool = Pool(n, length)
        self.ptrs = [self.pool.put(i, G.OFFSETS[i % len(G.OFFSETS)], data[i]) for i in range(n)]
        self.pool.upload()
        self.want = [crc(data[i]) for i in range(n)]


@pytest.fixture(scope="module")
def list_shards():
    return Shards(max(G.LIST_N), G.LIST_LEN, 1)


@pytest.fixture(scope="module")
def list5_shards():
    return Shards(max(G.LIST5_N), G.LIST5_LEN, 5)


@pytest.mark.parametrize("n", G.LIST_N)
def test_pointer_table_lists(rs, capfd, list_shards, n):
    """1, 2, slots, slots + 1 and 2 slots + 1 scattered shards at pw = 2: the launches of 266."""
    s = list_shards
    p = G.plan(G.LIST_LEN, n, False)
    assert (p.pw, p.slots) == (2, 266)
    got = run(rs, capfd, s.pool, s.ptrs[:n], G.LIST_LEN)
    assert got == s.want[:n], [i for i in range(n) if got[i] != s.want[i]][:8]


@pytest.mark.parametrize("n", G.LIST5_N)
def test_pointer_table_lists_five_groups(rs, capfd, list5_shards, n):
    """slots and slots + 1 shards of five groups each (pw = 6): 264 per launch, the 265th alone."""
    s = list5_shards
    p = G.plan(G.LIST5_LEN, n, False)
    assert (p.groups, p.pw, p.slots) == (5, 6, 264)
    assert len(G.launches(G.LIST5_LEN, s.ptrs[:n])) == (1 if n == 264 else 2)
    got = run(rs, capfd, s.pool, s.ptrs[:n], G.LIST5_LEN)
    assert got == s.want[:n], [i for i in range(n) if got[i] != s.want[i]][:8]


@pytest.mark.parametrize("name,stride", G.AFFINE_STRIDES)
def test_affine_strides(rs, capfd, name, stride):
    """Equally spaced lists -- pitched, contiguous at an odd length, descending -- run as one launch; the
    same list with a shard named twice, or with one pointer moved, falls back to the pointer table."""
    n, length = G.AFFINE_N, G.LIST_LEN
    pitch = abs(stride)
    pool = Pool(1, n * pitch + 256)
    data = np.random.default_rng(pitch).integers(0, 256, (n, length), dtype=np.uint8)
    up = [pool.put(0, 3 + i * pitch, data[i]) for i in range(n)]
    pool.upload()
    ptrs = up if stride > 0 else up[::-1]
    assert [b - a for a, b in zip(ptrs, ptrs[1:])] == [stride] * (n - 1)
    want = [crc(pool.host(p, length)) for p in ptrs]
    (line,) = G.launches(length, ptrs)
    assert (line["affine"], line["shards"]) == (1, n)
    assert run(rs, capfd, pool, ptrs, length) == want
    twice = [ptrs[0], ptrs[1], ptrs[0], ptrs[2]]
    assert G.launches(length, twice)[0]["affine"] == 0
    assert run(rs, capfd, pool, twice, length) == [want[0], want[1], want[0], want[2]]
    moved = list(ptrs)
    moved[3] += 1  # (still inside the pool: the shard's last byte is then the byte after shard 3)
    assert G.launches(length, moved)[0]["affine"] == 0
    assert run(rs, capfd, pool, moved, length) == [crc(pool.host(p, length)) for p in moved]


@pytest.mark.parametrize("n", G.CAP_N)
def test_affine_cap(rs, capfd, n):
    """65535 shards of 16 bytes 16 apart: one launch with grid.y = 65535; 65536: 247 pointer-table launches."""
    length = G.CAP_LEN
    pool = Pool(1, n * length)
    data = np.random.default_rng(n).integers(0, 256, n * length, dtype=np.uint8)
    p0 = pool.put(0, 0, data)
    pool.upload()
    ptrs = [p0 + length * i for i in range(n)]
    lines = G.launches(length, ptrs)
    assert len(lines) == G.CAP_LAUNCHES[n] and lines[0]["affine"] == int(n == 65535)
    assert [d["shards"] for d in lines] == ([65535] if n == 65535 else [266] * 246 + [100])
    got = run(rs, capfd, pool, ptrs, length)
    raw = data.tobytes()
    want = [zlib.crc32(raw[length * i:length * (i + 1)]) for i in range(n)]
    for i in list(range(0, n, 251)) + [n - 1]:
        assert want[i] == O.crc32_ieee(data[length * i:length * (i + 1)])
    assert got == want, [i for i in range(n) if got[i] != want[i]][:8]


# ------------------------------------------------------------------ CFSEC_CRC32_GROUPS_PROBE

def test_groups_probe(rs, capfd, monkeypatch):
    """The workgroup total read per launch: another split of the same shards, the same words."""
    n, length = G.PROBE_N, G.PROBE_LEN
    pool = Pool(n, length)
    classes = data_classes(length, 273)
    shards = [classes[0][1], classes[3][1], classes[1][1]]  # random, one byte at len - 1, all zero
    ptrs = [pool.put(i, off, shards[i]) for i, off in enumerate([0, 1, 17])]
    pool.upload()
    want = [crc(s) for s in shards]
    assert run(rs, capfd, pool, ptrs, length) == want
    for value, groups, tpw in G.PROBES:
        monkeypatch.setenv("CFSEC_CRC32_GROUPS_PROBE", str(value))
        (line,) = G.launches(length, ptrs, total=value)
        assert (line["groups"], line["tpw"], line["affine"]) == (groups, tpw, 0)
        got = run(rs, capfd, pool, ptrs, length, total=value)
        assert got == want, (value, hexes(got), hexes(want))


# ------------------------------------------------------------------ idx + fin through the public calls

def words_tensor(n):
    return torch.full((n + 8,), WORD_CANARY - (1 << 32), dtype=torch.int32, device="cuda")


def words_of(t, n):
    w = t.cpu().numpy().view(np.uint32)
    assert [int(x) for x in w[n:]] == [WORD_CANARY] * 8  # nothing written past the words
    return [int(x) for x in w[:n]]


def stripe_rows(k, S, seed):
    """k data rows: random, all zero, one byte at position 0, one at S - 1, then random ones."""
    classes = data_classes(S, seed)
    r = np.random.default_rng(seed + 1)
    return [classes[i][1] if i < 4 else r.integers(0, 256, S, dtype=np.uint8) for i in range(k)]


def no_fused_launch(err):
    assert "cfsec: crc route=" not in err and "cfsec: crc sv" not in err and "cfsec: bs launch" not in err, err
    assert "cfsec: matvec family=" in err, err  # the product alone, then the separate pass


@pytest.mark.parametrize("layout", ["pitched", "moved"])
@pytest.mark.parametrize("S,nst", G.IDX_LENGTHS)
def test_encode_crc_unfused(rs, capfd, monkeypatch, S, nst, layout):
    """encode_crc_batch on (5, 2): pitched stripes are one affine launch with consecutive words and fin
    set; with one row moved, a pointer table."""
    k, m = 5, 2
    total = k + m
    enc = rs.New(k, m)
    assert R.expect_route(k, m, True, S, nst, bits=R.match_bits(k, m, enc.matrix()[k:].tobytes())) == R.NONE
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    pool = Pool(nst * total, S)
    ptrs, rows = [], []
    for s in range(nst):
        data = stripe_rows(k, S, S + s)
        for i in range(total):
            off = 16 if layout == "moved" and (s, i) == (1, 3) else 0
            ptrs.append(pool.put(s * total + i, off, data[i]) if i < k else pool.ptr + pool.at(s * total + i, off))
        rows.append(data)
    pool.upload()
    for s in range(nst):
        full = [r.copy() for r in rows[s]] + [np.zeros(S, np.uint8) for _ in range(m)]
        assert O.encode(k, m, full) == 0
        for i in range(k, total):
            pool.put(s * total + i, 0, full[i])
        rows[s] = full
    pool.expect()
    words = words_tensor(nst * total)
    capfd.readouterr()
    enc.encode_crc_batch(ptrs, S, nst, words.data_ptr())
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    no_fused_launch(err)
    lines = parse(err)
    want_lines = G.launches(S, ptrs, idx=list(range(nst * total)), fin=True)
    assert lines == want_lines and [d["affine"] for d in lines] == [int(layout == "pitched")]
    pool.check()
    got = words_of(words, nst * total)
    want = [crc(rows[s][i]) for s in range(nst) for i in range(total)]
    assert got == want, [(j, hex(got[j]), hex(want[j])) for j in range(len(want)) if got[j] != want[j]][:8]


@pytest.mark.parametrize("S,nst,erased", [(S, nst, [2, 11]) for S, nst in G.IDX_LENGTHS] + [(4097, 1, [2, 3])])
def test_reconstruct_crc_scattered_words(rs, capfd, monkeypatch, S, nst, erased):
    """reconstruct_crc_batch on (10, 4) with shards 2 and 11 erased: words 2 and 11 of every stripe, so a
    pointer table with its own indices; the words of shards not rebuilt are 0.  One stripe with shards 2
    and 3 erased: two shards are always equally spaced, so the affine form from a first word that is not 0."""
    k, m = 10, 4
    total = k + m
    enc = rs.New(k, m)
    assert R.expect_route(k, len(erased), False, S, nst) == R.NONE
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    pool = Pool(nst * total, S)
    ptrs, rows = [], []
    for s in range(nst):
        full = stripe_rows(k, S, 3 * S + s) + [np.zeros(S, np.uint8) for _ in range(m)]
        assert O.encode(k, m, full) == 0
        for i in range(total):
            o = 1 if i in erased else 0  # the rebuilt rows off every alignment
            ptrs.append(pool.ptr + pool.at(s * total + i, o) if i in erased else pool.put(s * total + i, o, full[i]))
        rows.append(full)
    pool.upload()
    for s in range(nst):
        for i in erased:
            pool.put(s * total + i, 1, rows[s][i])
    pool.expect()
    words = words_tensor(nst * total)
    capfd.readouterr()
    enc.reconstruct_crc_batch(ptrs, S, nst, erased, words.data_ptr())
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    no_fused_launch(err)
    lines = parse(err)
    sub = [ptrs[s * total + i] for s in range(nst) for i in erased]
    idx = [s * total + i for s in range(nst) for i in erased]
    assert lines == G.launches(S, sub, idx=idx, fin=True) and lines[0]["idx"] == 1
    assert lines[0]["affine"] == int(erased == [2, 3])
    pool.check()
    got = words_of(words, nst * total)
    want = [crc(rows[s][i]) if i in erased else 0 for s in range(nst) for i in range(total)]
    assert got == want, [(j, hex(got[j]), hex(want[j])) for j in range(len(want)) if got[j] != want[j]][:8]


@pytest.mark.parametrize("S,nst", G.IDX_LENGTHS)
def test_encode_crc_no_parity(rs, capfd, S, nst):
    """A New(4, 0) engine: nothing to encode, every shard through the pass with fin set and the words in
    list order (idx = 0); rows 1 byte apart in alignment, so a pointer table -- and pitched, affine."""
    k = 4
    enc = rs.New(k, 0)
    for layout in ("pitched", "scattered"):
        pool = Pool(nst * k, S)
        rows = [stripe_rows(k, S, 7 * S + s) for s in range(nst)]
        ptrs = [pool.put(s * k + i, (s * k + i) % 5 if layout == "scattered" else 0, rows[s][i])
                for s in range(nst) for i in range(k)]
        pool.upload()
        words = words_tensor(nst * k)
        capfd.readouterr()
        enc.encode_crc_batch(ptrs, S, nst, words.data_ptr())
        torch.cuda.synchronize()
        lines = trace(capfd)
        assert lines == G.launches(S, ptrs, fin=True) and lines[0]["affine"] == int(layout == "pitched")
        pool.check()
        got = words_of(words, nst * k)
        want = [crc(rows[s][i]) for s in range(nst) for i in range(k)]
        assert got == want, (layout, hexes(got), hexes(want))


def test_mixed_length_tasklet(capfd, monkeypatch):
    """One ReconstructBatch with checksums on EC15P12 (k = 15: no fused kernel), three bids of three
    lengths, one multi-group: BatchRun::checksum's one launch per length into one words array."""
    from chubaofs_amd import ec
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    t = cm.GetTactic(cm.EC15P12)
    total = t.N + t.M + t.L
    enc = ec.NewEncoder(ec.Config(CodeMode=t, EnableVerify=False), device=0)
    orc = ECOracle.from_tactic(t)
    bad = [2, 11, 20]
    assert R.expect_route(t.N, len(bad), False, max(G.TASKLET_LENGTHS), 1) == R.NONE
    lengths = G.TASKLET_LENGTHS
    pool = Pool(len(lengths) * total, max(lengths))
    good, bids = [], []
    for b, S in enumerate(lengths):
        ref = [Slice.of(x) for x in stripe_rows(t.N, S, 11 * S) + [np.zeros(S, np.uint8) for _ in range(total - t.N)]]
        assert orc.encode(ref) == 0
        full = [x.view().copy() for x in ref]
        for i in range(total):
            if i not in bad:
                pool.put(b * total + i, i % 3, full[i])
        good.append(full)
        bids.append([pool.view(b * total + i, i % 3, S) for i in range(total)])
    pool.upload()
    for b in range(len(lengths)):
        for i in bad:
            pool.put(b * total + i, i % 3, good[b][i])
    pool.expect()
    capfd.readouterr()
    st, crcs = enc.ReconstructBatch(bids, [bad] * len(lengths), crcs=True)
    err = capfd.readouterr().err
    assert "cfsec: crc route=" not in err and "cfsec: crc sv" not in err, err
    lines = parse(err)
    want_lines = []
    for S in sorted(lengths):
        p = G.plan(S, len(bad), False)
        want_lines.append(dict(len=S, shards=len(bad), s0=0, tiles=p.tiles, groups=p.groups, tpw=p.tpw, affine=0, idx=1, fin=1))
    assert lines == want_lines
    assert st == [0] * len(lengths)
    pool.check()
    for b in range(len(lengths)):
        want = [crc(good[b][i]) if i in bad else 0 for i in range(total)]
        assert crcs[b] == want, (b, hexes(crcs[b]), hexes(want))


# ------------------------------------------------------------------ the length limit

def test_length_above_the_limit(rs, capfd):
    """A shard length above 2^32 - 1 - 4096 is an invalid argument: nothing is launched, and the pointer is
    never dereferenced (a 16-byte buffer serves)."""
    pool = Pool(1, 16)
    p = pool.put(0, 0, np.arange(16, dtype=np.uint8))
    pool.upload()
    capfd.readouterr()
    with pytest.raises(_lib.ErrInvalidArg):
        rs.crc32_ieee_batch([p], G.MAX_LEN + 1)
    assert trace(capfd) == []
    pool.check()
    assert run(rs, capfd, pool, [p], 16) == [crc(np.arange(16, dtype=np.uint8))]
