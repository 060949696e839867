"""Repair tasklets with every shard's checksum from the one repair pass: Encoder.RepairBatch
(cfsec_ec_repair_batch_crc) and cfsec_rs_repair_crc_batch against the oracle and zlib.

blobnode checks each downloaded survivor's CRC32, runs Reconstruct then Verify and checksums each rebuilt
shard (work_shard_recover.go:654-685, 751-760, 335-342).  The call does all three: where the shape has a
fused kernel (gf_crc_sv_kernel, gf_crc.hpp: k in {6, 8, 12, 16, 18}, 2..6 stored + compared rows) the
pass that rebuilds and compares also checksums every row it reads or writes; everywhere else the
product is followed by the separate checksum pass.  Either way every one of a bid's n words is the
checksum of the shard as it stands in memory after the call.

References: ECOracle.repair / the C oracle's Reconstruct + Verify for bytes and status, zlib.crc32 of the
oracle's shards after the repair for the words -- never another path of the library.  Everything is
bit-exact.  Before the GPU is touched each test asserts on the oracle alone that its clean bids give
status 0, its bids with a flipped compared survivor ErrVerify, and its exactly-N-survivor bids with a
flipped input status 0 (the case Verify cannot see and the survivors' checksums catch).

S = 8209: two whole 4 KiB tiles and a 17-byte ragged tail -- one thread with a full piece past the tile
edge, one with a 1-byte piece.  Canary bytes follow every shard carved from a pool."""
import os
import random
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

from chubaofs_amd import _lib, codemode as cm
from chubaofs_amd.codemode import Tactic
from oracle import oracle as O
from oracle.ec_oracle import ECOracle, Slice

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CHILD = os.environ.get("CFSEC_REPAIR_CRC_CHILD") == "1"
FUSED = os.environ.get("CFSEC_SV_CRC", "1")[:1] != "0"  # gf_crc.hip crc_sv_on (read once per process)

S = 8209
CANARY, JUNK = 0xA5, 0xEE
FLIP_AT = [0, 4095, 4096, 8191, 8192, S - 1]
ERR_VERIFY = _lib.ErrVerify.status
SV_K, SV_M = (6, 8, 12, 16, 18), (2, 3, 4, 5, 6)
SWEEP = [(6, 3), (6, 6), (8, 2), (12, 4), (16, 4), (18, 2), (18, 6)]


def pitch_of(size):
    return (size + 255) // 256 * 256 + 256  # at least 256 canary bytes after every shard


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def rs_encoder(k, m):
    from chubaofs_amd import ec
    return ec.NewEncoder(ec.Config(CodeMode=Tactic(k, m, 0, 1, k, 0, 0), EnableVerify=False), device=0)


def mode_encoder(mode):
    from chubaofs_amd import ec
    return ec.NewEncoder(ec.Config(CodeMode=cm.GetTactic(mode), EnableVerify=False), device=0)


def rs_codeword(k, m, size, seed):
    rng = np.random.default_rng(seed)
    cw = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(k)] + [np.zeros(size, np.uint8) for _ in range(m)]
    assert O.encode(k, m, cw) == 0
    return cw


def oracle_repair(orc, shards, bad):
    """(status, shards after) of the reference's Reconstruct(shards, bad) then Verify(shards)."""
    work = [Slice.of(s) for s in shards]
    st = orc.repair(work, list(bad), verify=True)
    return st, [w.view().copy() for w in work]


def want_words(status, after):
    return [crc(x) for x in after] if status in (0, ERR_VERIFY) else [0] * len(after)


def want_mismatch(status, src, bad, expect):
    """The lowest survivor whose bytes -- untouched by the repair -- no longer have the checksum given."""
    if status not in (0, ERR_VERIFY):
        return -1
    return next((i for i in range(len(src)) if i not in bad and crc(src[i]) != expect[i]), -1)


class Bid:
    def __init__(self, src, bad, expect, kind):
        self.src, self.bad, self.expect, self.kind = src, list(bad), expect, kind  # kind: clean / compared / input


class Pool:
    """Bids of n shards of `size` bytes carved from one buffer at one pitch, canary bytes between them."""

    def __init__(self, orc, bids, size):
        self.bids, self.size, self.n = bids, size, len(bids[0].src)
        self.pitch = pitch_of(size)
        self.before = np.full(256 + len(bids) * self.n * self.pitch, CANARY, np.uint8)
        self.want = self.before.copy()
        self.status, self.words, self.mismatch = [], [], []
        cache = {}
        for b, bid in enumerate(bids):
            key = (id(bid.src), tuple(bid.bad))  # repeated bids share one oracle run
            if key not in cache:
                st, after = oracle_repair(orc, bid.src, bid.bad)
                cache[key] = (st, after, want_words(st, after), want_mismatch(st, bid.src, bid.bad, bid.expect))
            st, after, words, mm = cache[key]
            self.status.append(st)
            self.words.append(words)
            self.mismatch.append(mm)
            for i in range(self.n):
                o = self.offset(b, i)
                self.before[o:o + size] = bid.src[i]
                self.want[o:o + size] = after[i]

    def offset(self, b, i):
        return 256 + (b * self.n + i) * self.pitch

    def check_oracle(self):
        """On the oracle alone, before the GPU is touched."""
        for b, bid in enumerate(self.bids):
            if bid.kind == "clean":
                assert self.status[b] == 0 and self.mismatch[b] == -1, (b, bid.bad)
            elif bid.kind == "compared":
                assert self.status[b] == ERR_VERIFY and self.mismatch[b] >= 0, (b, bid.bad)
            elif bid.kind == "blind":
                assert self.status[b] == 0 and self.mismatch[b] >= 0, (b, bid.bad)
            else:
                assert bid.kind == "input" and self.mismatch[b] >= 0, (b, bid.bad)

    def run(self, enc):
        pool = torch.from_numpy(self.before).cuda()
        assert pool.data_ptr() % 256 == 0
        views = [[pool[self.offset(b, i):self.offset(b, i) + self.size] for i in range(self.n)]
                 for b in range(len(self.bids))]
        out = enc.RepairBatch(views, [b.bad for b in self.bids], expect=[b.expect for b in self.bids])
        torch.cuda.synchronize()
        return out, pool.cpu().numpy()

    def check(self, out, image):
        status, words, mismatch = out
        assert status == self.status, [(b, self.bids[b].bad, status[b], self.status[b])
                                       for b in range(len(status)) if status[b] != self.status[b]][:8]
        if not np.array_equal(image, self.want):  # rebuilt shards, survivors and every canary byte
            d = np.flatnonzero(image != self.want)
            b, rest = divmod(int(d[0]) - 256, self.n * self.pitch)
            pytest.fail(f"{d.size} bytes differ, first in bid {b} (bad {self.bids[b].bad}) shard "
                        f"{rest // self.pitch} at byte {rest % self.pitch}")
        for b in range(len(self.bids)):
            assert words[b] == self.words[b], (b, self.bids[b].bad, self.bids[b].kind,
                                               [i for i in range(self.n) if words[b][i] != self.words[b][i]])
        assert mismatch == self.mismatch, [(b, mismatch[b], self.mismatch[b]) for b in range(len(mismatch))
                                           if mismatch[b] != self.mismatch[b]][:8]


def sv_lines(err):
    """The fused launches traced: dicts of the fields of 'cfsec: crc sv k=.. m=.. nstore=.. ...'."""
    return [dict((k, int(v)) for k, v in (x.split("=") for x in ln.split()[3:]))
            for ln in err.splitlines() if ln.startswith("cfsec: crc sv ")]


def flip(src, shard, n):
    src[shard] = src[shard].copy()
    at = FLIP_AT[n % len(FLIP_AT)]
    src[shard][min(at, src[shard].size - 1)] ^= 1 << ((n + n // len(FLIP_AT)) % 8)


def sweep_bids(k, m):
    """Per nstore = 1 .. m - 1 a bad set of nstore shards with a clean bid, one bid per compared row with
    one bit flipped in it and one bid with a bit flipped in a decode input."""
    total = k + m
    cw = rs_codeword(k, m, S, 1000003 * k + 1009 * m)
    expect = [crc(x) for x in cw]
    r = random.Random(7919 * k + m)
    bids, groups, n = [], [], k + m
    for nstore in range(1, m):
        nd = 1 if nstore == 1 else r.randint(1, min(k, nstore - 1))
        bad = sorted(r.sample(range(k), nd)) + sorted(r.sample(range(k, total), nstore - nd))
        present = [i for i in range(total) if i not in bad]
        inputs, compared = present[:k], present[k:]
        assert len(compared) == m - nstore
        base = [np.full(S, JUNK, np.uint8) if i in bad else cw[i] for i in range(total)]
        bids.append(Bid(list(base), bad, expect, "clean"))
        for c in compared:
            src = list(base)
            flip(src, c, n)
            n += 1
            bids.append(Bid(src, bad, expect, "compared"))
        src = list(base)
        flip(src, inputs[r.randrange(k)], n)
        n += 1
        bids.append(Bid(src, bad, expect, "input"))
        groups.append((nstore, bad, 2 + len(compared)))
    return bids, groups


# ------------------------------------------------------------------ 1. every instantiation

@pytest.mark.parametrize("k,m", SWEEP)
def test_kernel_sweep(k, m, monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    bids, groups = sweep_bids(k, m)
    pool = Pool(ECOracle(k, m), bids, S)
    pool.check_oracle()
    enc = rs_encoder(k, m)
    capfd.readouterr()
    out, image = pool.run(enc)
    err = capfd.readouterr().err
    pool.check(out, image)
    for b, bid in enumerate(bids):
        if bid.kind != "clean":  # the one flipped shard is the one named
            (f,) = [i for i in range(k + m) if i not in bid.bad and crc(bid.src[i]) != bid.expect[i]]
            assert out[2][b] == f, (b, bid.kind)
    got = [(g["k"], g["m"], g["nstore"], g["stripes"], g["len"]) for g in sv_lines(err)]
    want = [(k, m, nstore, nst, S) for nstore, _, nst in groups] if FUSED else []
    assert got == want, err  # the fused kernel, once per bad set


# ------------------------------------------------------------------ 2. sizes

@pytest.mark.parametrize("size", [1, 15, 16, 17, 4095, 4096, 4097, 8209])
def test_sizes(size, monkeypatch, capfd):
    """EC12P4, one lost data shard: a row shorter than a piece, the tile edge, a ragged second tile."""
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    k, m, bad = 12, 4, [5]
    cw = rs_codeword(k, m, size, 77 + size)
    expect = [crc(x) for x in cw]
    base = [np.full(size, JUNK, np.uint8) if i in bad else cw[i] for i in range(k + m)]
    bids = [Bid(list(base), bad, expect, "clean")]
    for shard, kind in ((13, "compared"), (15, "compared"), (0, "input")):
        src = list(base)
        src[shard] = src[shard].copy()
        src[shard][size - 1] ^= 0x80  # the row's last byte
        bids.append(Bid(src, bad, expect, kind))
    src = list(base)
    src[14] = src[14].copy()
    src[14][0] ^= 1
    bids.append(Bid(src, bad, expect, "compared"))
    pool = Pool(ECOracle(k, m), bids, size)
    pool.check_oracle()
    capfd.readouterr()
    out, image = pool.run(rs_encoder(k, m))
    err = capfd.readouterr().err
    pool.check(out, image)
    assert out[2] == [-1, 13, 15, 0, 14]
    if FUSED:
        (g,) = sv_lines(err)
        assert (g["nstore"], g["stripes"], g["len"], g["tpw"]) == (1, 5, size, 1), err


# ------------------------------------------------------------------ 3. several tiles per workgroup

def test_several_tiles_per_workgroup(monkeypatch, capfd):
    """1024 bids at one pitch, one bad set: one launch whose workgroups each walk a stripe's three tiles,
    the prefetched one and the ragged one.  8 distinct bids repeated (8 oracle runs)."""
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    k, m, bad = 12, 4, [2, 13]
    distinct = []
    for j in range(8):
        cw = rs_codeword(k, m, S, 4000 + j)
        expect = [crc(x) for x in cw]
        src = [np.full(S, JUNK, np.uint8) if i in bad else cw[i] for i in range(k + m)]
        kind = "clean"
        if j == 5:  # a flipped compared survivor, in the last (ragged) tile
            src[15] = src[15].copy()
            src[15][8200] ^= 0x04
            kind = "compared"
        distinct.append(Bid(src, bad, expect, kind))
    bids = [distinct[b % 8] for b in range(1024)]
    pool = Pool(ECOracle(k, m), bids, S)
    pool.check_oracle()
    capfd.readouterr()
    out, image = pool.run(rs_encoder(k, m))
    err = capfd.readouterr().err
    pool.check(out, image)
    assert [out[0][b] for b in range(8)] == [0, 0, 0, 0, 0, ERR_VERIFY, 0, 0] and out[2][5] == 15
    if FUSED:
        (g,) = sv_lines(err)
        assert (g["nstore"], g["stripes"], g["per"]) == (2, 1024, 1024), err
        assert g["tpw"] >= 2, err  # asserted, not assumed: one workgroup walks the full tiles and the ragged one


# ------------------------------------------------------------------ 4. layouts and memory

def place(shards, memory):
    if memory == "device":
        return [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in shards]
    if memory == "pinned":
        out = []
        for s in shards:
            p = _lib.pinned_empty(s.size)
            p[:] = s
            out.append(p)
        return out
    return [s.copy() for s in shards]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@pytest.mark.parametrize("memory", ["device", "pinned", "pageable"])
@pytest.mark.parametrize("k,m,bad", [(12, 4, [3]), (6, 6, [0, 7])])
def test_layouts_and_memory(k, m, bad, memory, monkeypatch, capfd):
    """20 bids, every shard its own allocation: pointer-table launches of 96 / (k + m) bids; page-locked
    host memory in place; pageable host memory staged, whose chunks take the separate pass."""
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    orc = ECOracle(k, m)
    total = k + m
    compared = [i for i in range(total) if i not in bad][k:]
    bids, want = [], []
    for b in range(20):
        cw = rs_codeword(k, m, S, 9000 + 20 * k + b)
        expect = [crc(x) for x in cw]
        src = [np.full(S, JUNK, np.uint8) if i in bad else cw[i] for i in range(total)]
        kind = "clean"
        if b in (7, 19):
            flip(src, compared[b % len(compared)], b)
            kind = "compared"
        st, after = oracle_repair(orc, src, bad)
        assert st == (0 if kind == "clean" else ERR_VERIFY)
        bids.append(Bid(src, bad, expect, kind))
        want.append((st, after, want_words(st, after), want_mismatch(st, src, bad, expect)))
    if memory == "device":  # allocations of varying sizes: no two bids at one stride on every row
        pad = random.Random(k)
        work = [[torch.empty(S + 512 * pad.randrange(4), dtype=torch.uint8, device="cuda")[:S] for _ in b.src] for b in bids]
        for b, bid in enumerate(bids):
            for i, x in enumerate(bid.src):
                work[b][i].copy_(torch.from_numpy(x))
    else:
        work = [place(b.src, memory) for b in bids]
    enc = rs_encoder(k, m)
    capfd.readouterr()
    status, words, mismatch = enc.RepairBatch(work, [b.bad for b in bids], expect=[b.expect for b in bids])
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    for b, (st, after, w, mm) in enumerate(want):
        assert status[b] == st and mismatch[b] == mm, (b, status[b], st, mismatch[b], mm)
        for i in range(total):
            assert np.array_equal(host(work[b][i]), after[i]), (b, i)
        assert words[b] == w, (b, [i for i in range(total) if words[b][i] != w[i]])
    lines = sv_lines(err)
    if memory == "pageable" or not FUSED:
        assert lines == [], err  # staged chunks: the product and the separate pass, the same words
    else:
        (g,) = lines
        assert (g["k"], g["m"], g["nstore"], g["stripes"]) == (k, m, len(bad), 20), err
        if memory == "device":  # a pointer table: 6 resp. 8 bids per launch, several launches
            assert g["per"] == 96 // total and -(-20 // g["per"]) >= 3, err


# ------------------------------------------------------------------ 5. the case Verify cannot see

@pytest.mark.parametrize("k,m", [(12, 4), (6, 6)])
def test_blind_case(k, m, monkeypatch, capfd):
    """Exactly N survivors and one flipped input: a self-consistent stripe, Verify is true, the rebuilt
    bytes are the oracle's (wrong) bytes, and the survivors' checksums name the flipped shard.  Nothing
    is compared, so this is the kStore kernel with every row checksummed: the plumbing of mode 3."""
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    total = k + m
    cw = rs_codeword(k, m, S, 31337 + k)
    expect = [crc(x) for x in cw]
    r = random.Random(k)
    bids = []
    for j in range(3):
        bad = sorted(r.sample(range(total), m))
        src = [np.full(S, JUNK, np.uint8) if i in bad else cw[i] for i in range(total)]
        bids.append(Bid(list(src), bad, expect, "clean"))
        survivor = [i for i in range(total) if i not in bad][r.randrange(k)]
        flip(src, survivor, j)
        bids.append(Bid(src, bad, expect, "blind"))
    pool = Pool(ECOracle(k, m), bids, S)
    pool.check_oracle()
    for b, bid in enumerate(bids):
        if bid.kind == "blind":  # the oracle's rebuilt bytes are not the codeword's
            o = pool.offset(b, bid.bad[0])
            assert not np.array_equal(pool.want[o:o + S], cw[bid.bad[0]])
    capfd.readouterr()
    out, image = pool.run(rs_encoder(k, m))
    err = capfd.readouterr().err
    pool.check(out, image)
    assert sv_lines(err) == []
    assert len([ln for ln in err.splitlines() if ln.startswith("cfsec: crc route=") and " cin=1 " in ln]) == 3, err


# ------------------------------------------------------------------ 6. every code mode

MOCK_SIZES = [1024, 2048, 512, 23, 65, 12]  # worker_for_test.go:79-83, without the empty bid


def gen_mock_bytes(letter, size):
    """worker_for_test.go:62-69"""
    return ((letter + np.arange(size)) & 0xFF).astype(np.uint8)


def mode_codeword(orc, t, size, bid):
    sh = [Slice.of(gen_mock_bytes(bid + i, size)) for i in range(t.N)] + \
         [Slice.of(np.zeros(size, np.uint8)) for _ in range(t.M + t.L)]
    assert orc.encode(sh) == 0
    return [x.view().copy() for x in sh]


@pytest.mark.parametrize("memory", ["device", "pageable"])
@pytest.mark.parametrize("mode", cm.GetAllCodeModes())
def test_every_code_mode(mode, memory):
    """One clean and one corrupted bid per mode, for LRC modes also a bad local parity and a corrupted
    one: the fallback routes (EC10P4, EC15P12, EC12P9, the 16 + 20 plans, EC6P10L2's 12 rows) and the
    LRC word ownership -- no word written twice, none missed.  Then local-stripe bids."""
    t = cm.GetTactic(mode)
    orc = ECOracle.from_tactic(t)
    enc = mode_encoder(mode)
    total, glob = t.N + t.M + t.L, t.N + t.M
    r = random.Random(mode * 31 + 5)
    plans = [("clean", None), ("corrupt", "global")]
    if t.L:
        plans += [("clean", "badlocal"), ("corrupt", "local"), ("corrupt", "badlocal")]
    bids = []
    for j, (kind, what) in enumerate(plans):
        size = MOCK_SIZES[(mode + j) % len(MOCK_SIZES)] + (4096 if j == 1 else 0)
        cw = mode_codeword(orc, t, size, 10 * j + 1)
        expect = [crc(x) for x in cw]
        bad = sorted(r.sample(range(glob), r.randint(1, min(t.M, 3))))
        if what == "badlocal":
            bad.append(glob + r.randrange(t.L))
        src = [np.full(size, JUNK, np.uint8) if i in bad else cw[i] for i in range(total)]
        if kind == "corrupt":
            pick = [i for i in range(glob if what != "local" else total) if i not in bad and (what != "local" or i >= glob)]
            src[pick[r.randrange(len(pick))]][size // 2] ^= 0x40
        bids.append(Bid(src, bad, expect, kind))
    run_mode_bids(enc, orc, bids, memory)
    if t.L:  # local stripes: n = the local stripe's size
        lsz = total // t.AZCount
        layout = [orc.shards_in_idc(list(range(total)), a) for a in range(t.AZCount)]
        local = []
        for j, az in enumerate(layout):
            size = MOCK_SIZES[(mode + j) % len(MOCK_SIZES)]
            cw = mode_codeword(orc, t, size, 50 + j)
            lcw = [cw[g] for g in az]
            expect = [crc(x) for x in lcw]
            bad = sorted(r.sample(range(lsz), r.randint(1, t.L // t.AZCount)))
            src = [np.full(size, JUNK, np.uint8) if i in bad else lcw[i] for i in range(lsz)]
            if j == 1:
                pick = [i for i in range(lsz) if i not in bad]
                src[pick[0]][size - 1] ^= 1
            local.append(Bid(src, bad, expect, "clean" if j != 1 else "corrupt"))
        run_mode_bids(enc, orc, local, memory)


def run_mode_bids(enc, orc, bids, memory):
    want = []
    for bid in bids:
        st, after = oracle_repair(orc, bid.src, bid.bad)
        if bid.kind == "clean":
            assert st == 0
        want.append((st, after, want_words(st, after), want_mismatch(st, bid.src, bid.bad, bid.expect)))
    assert any(w[0] == 0 for w in want)
    work = [place(b.src, memory) for b in bids]
    status, words, mismatch = enc.RepairBatch(work, [b.bad for b in bids], expect=[b.expect for b in bids])
    torch.cuda.synchronize()
    for b, (st, after, w, mm) in enumerate(want):
        assert status[b] == st, (b, bids[b].bad, status[b], st)
        for i in range(len(after)):
            assert np.array_equal(host(work[b][i]), after[i]), (b, i)
        assert words[b] == w, (b, bids[b].bad, [i for i in range(len(w)) if words[b][i] != w[i]])
        assert mismatch[b] == mm, (b, mismatch[b], mm)


# ------------------------------------------------------------------ 7. the switch, in a child

# Measured on the MI355X: the child (python start, `import torch`, the library's first use and the two
# cases) 4.0 s of wall time; it gets three times that.
CHILD_SECONDS = 4.0
CHILD_TIMEOUT = 3 * CHILD_SECONDS


@pytest.mark.skipif(CHILD, reason="the child process itself")
def test_switch_in_child():
    """CFSEC_SV_CRC=0: test 1's EC12P4 and EC6P6 cases on the product and the separate pass -- the same
    bytes, status and words.  One child; ended by a signal, an abort or its time limit it ends the
    session: nothing more starts on the GPU after a fault."""
    env = dict(os.environ, CFSEC_REPAIR_CRC_CHILD="1", CFSEC_SV_CRC="0")
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", __file__, "-k",
                            "test_kernel_sweep and (12-4 or 6-6)"],
                           env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.exit(f"CFSEC_SV_CRC=0: the child ran into its time limit ({CHILD_TIMEOUT:.0f} s)", returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        pytest.exit(f"CFSEC_SV_CRC=0: the child ended abnormally ({r.returncode})\n" + r.stdout[-2000:] + r.stderr[-2000:],
                    returncode=3)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert re.search(r"\b2 passed", r.stdout) and "failed" not in r.stdout, r.stdout[-2000:]


# ------------------------------------------------------------------ 8. the reedsolomon seam

@pytest.mark.parametrize("k,m,erased", [(12, 4, [1, 14]), (6, 6, [2])])
def test_rs_repair_crc_batch(k, m, erased, monkeypatch, capfd):
    """cfsec_rs_repair_crc_batch on a pitched device batch of 5 stripes: flags as verify_batch, bytes and
    every word; a second call on a non-default torch stream, ordered by that stream alone."""
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    from chubaofs_amd import reedsolomon
    total, nst = k + m, 5
    pitch = pitch_of(S)
    present = [i not in erased for i in range(total)]
    compared = [i for i in range(total) if present[i]][k:]
    before = np.full(256 + nst * total * pitch, CANARY, np.uint8)
    want = before.copy()
    flags_want, words_want = [], []
    for s in range(nst):
        cw = rs_codeword(k, m, S, 600 + 10 * k + s)
        src = [np.full(S, JUNK, np.uint8) if i in erased else cw[i] for i in range(total)]
        if s in (1, 4):
            flip(src, compared[s % len(compared)], s)
        work = [x.copy() for x in src]
        err, _ = O.reconstruct(k, m, work, present)
        assert err == 0
        err, ok = O.verify(k, m, work)
        assert err == 0 and ok == (s not in (1, 4))
        flags_want.append(0 if ok else 1)
        words_want += [crc(x) for x in work]
        for i in range(total):
            o = 256 + (s * total + i) * pitch
            before[o:o + S] = src[i]
            want[o:o + S] = work[i]
    enc = reedsolomon.New(k, m, device=0)
    for stream in (None, torch.cuda.Stream()):
        pool = torch.from_numpy(before).cuda()
        flags = torch.zeros(nst, dtype=torch.int32, device="cuda")
        crcs = torch.full((nst * total,), -1, dtype=torch.int32, device="cuda")
        ptrs = [pool.data_ptr() + 256 + j * pitch for j in range(nst * total)]
        torch.cuda.synchronize()
        capfd.readouterr()
        if stream is None:
            enc.repair_crc_batch(ptrs, S, nst, erased, flags.data_ptr(), crcs.data_ptr())
            torch.cuda.synchronize()
        else:
            with torch.cuda.stream(stream):
                enc.repair_crc_batch(ptrs, S, nst, erased, flags.data_ptr(), crcs.data_ptr(), stream=stream)
            stream.synchronize()  # that stream alone
        err = capfd.readouterr().err
        assert np.array_equal(pool.cpu().numpy(), want)
        assert flags.cpu().tolist() == flags_want
        assert crcs.cpu().numpy().astype(np.uint32).tolist() == words_want
        if FUSED:
            (g,) = sv_lines(err)
            assert (g["k"], g["m"], g["nstore"], g["stripes"], g["per"]) == (k, m, len(erased), nst, nst), err
