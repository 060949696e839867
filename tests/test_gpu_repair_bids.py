"""Repair tasklets of mixed-size bids on the GPU: cfsec_ec_repair_bids_crc and cfsec_rs_repair_crc_stripes
(the mixed-plan launch that stores, compares and checksums, gf_mix_sv.hip, and the launch groups behind it).

Every case lays its shards out in the arena of test_gpu_encode_blobs_crc.py: each row at its own byte offset
0..15 from a 16-byte boundary, at least 64 untouched bytes on either side.  The rows hold valid codewords
(ECOracle.encode), the bad shards' buffers junk, and the corruption cases one flipped byte.  The call runs
on one copy of the arena; ECOracle.reconstruct followed by verify runs on host copies of the rows.
Asserted for every bid of every case, none left out:

  * status for status: the call == the oracle == cfsec_ec_repair_batch_crc on a second copy of the arena;
  * byte for byte: the whole arena after the call equals the arena with the oracle's rebuilt shards put in
    -- so every guard byte, every survivor and every buffer of a failed bid is unchanged;
  * word for word: crcs[bid * n + shard] == zlib.crc32 of that shard as it stands (a corrupt survivor's
    word is the corrupt shard's), all-zero words for a bid that failed; mismatch[] as the old call's and as
    computed here from the words;
  * the launches the call traces (CFSEC_TRACE_MATVEC, CFSEC_TRACE_CRC32, CFSEC_TRACE_CRC).

Sizes are the smallest at which the kernel can go wrong: rows shorter than a 16-byte chunk (1, 15), a
whole chunk (16), the overlapped last chunk (17, 31, 4095, 8197), the 4 KiB tile seam (4095, 4096, 4097),
several tiles XOR-ed into one word (8197, 65536); 1, 2 and 3 passes, the store / compare seam inside a
pass, nothing stored, nothing compared, 16 inputs.  None is a workload size.
"""
import ctypes
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

from chubaofs_amd import _lib, ec, reedsolomon
from chubaofs_amd.codemode import Tactic
from oracle import ec_oracle as EO
from oracle.ec_oracle import ECOracle, Slice
from test_gpu_encode_blobs_crc import LENS, Case, Mem, lines, tactic, tiles_of, trace_on

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ERR_VERIFY = _lib.ErrVerify.status
CHILD = os.environ.get("CFSEC_REPAIR_BIDS_CHILD") == "1"


# ---------------------------------------------------------------- the calls

class EcCalls:
    """cfsec_ec_repair_bids_crc against cfsec_ec_repair_batch_crc and ECOracle.reconstruct + verify."""

    def __init__(self, name):
        self.t = tactic(name)
        self.n = self.t.N + self.t.M + self.t.L
        self.enc = ec.NewEncoder(ec.Config(CodeMode=self.t, EnableVerify=False))
        self.old_enc = self.enc
        self.orc = ECOracle.from_tactic(self.t)
        self.L = self.enc._L

    def new(self, arr, nbids, bads, mem, expect):
        return repair_call(self.L.cfsec_ec_repair_bids_crc, self.enc, arr, self.n, nbids, bads, mem, expect)


class RsCalls:
    """cfsec_rs_repair_crc_stripes (missing shards: len 0) against cfsec_ec_repair_batch_crc of the same code."""

    def __init__(self, k, m):
        self.n = k + m
        self.rs = reedsolomon.New(k, m, device=0)
        self.old_enc = ec.NewEncoder(ec.Config(CodeMode=Tactic(k, m, 0, 1, k, 0, 0), EnableVerify=False), device=0)
        self.orc = ECOracle(k, m)
        self.L = self.rs._L

    def new(self, arr, nbids, bads, mem, expect):
        for b, bad in enumerate(bads):
            for i in bad:
                arr[b * self.n + i].len = 0
        status = (ctypes.c_int * nbids)(*([-7] * nbids))
        words = (ctypes.c_uint32 * (nbids * self.n))(*([0xA5A5A5A5] * (nbids * self.n)))
        rc = self.L.cfsec_rs_repair_crc_stripes(self.rs._h, arr, nbids, mem, status, words)
        return rc, list(status), list(words), None


def repair_call(fn, enc, arr, n, nbids, bads, mem, expect):
    flat = [i for b in bads for i in b]
    offs = [0]
    for b in bads:
        offs.append(offs[-1] + len(b))
    bad = (ctypes.c_int * max(len(flat), 1))(*flat)
    off = (ctypes.c_int * len(offs))(*offs)
    status = (ctypes.c_int * nbids)(*([-7] * nbids))
    words = (ctypes.c_uint32 * (nbids * n))(*([0xA5A5A5A5] * (nbids * n)))
    mism = (ctypes.c_int * nbids)(*([-7] * nbids))
    exp = (ctypes.c_uint32 * (nbids * n))(*expect)
    rc = fn(enc._h, arr, n, nbids, bad, off, mem, status, words, exp, mism)
    return rc, list(status), list(words), list(mism)


def shard_array(case, mem):
    arr = (_lib.Shard * sum(len(rows) for rows in case.items))()
    at = 0
    for rows in case.items:
        for pos, size in rows:
            arr[at] = _lib.Shard(mem.ptr + pos, size, size)
            at += 1
    return arr


# ---------------------------------------------------------------- a tasklet and what the oracle makes of it

class Tasklet:
    """Bids of the given shard sizes and bad sets: valid codewords in the arena, junk in the bad shards'
    buffers, then `flips` = (bid, shard, byte) each XOR-ed with 0x40.  Computed once: the arena before, the
    oracle's statuses, arena, words and mismatch indices."""

    def __init__(self, calls, lens, bads, seed, flips=()):
        assert len(lens) == len(bads)
        self.calls, self.lens, self.bads, self.n = calls, lens, [list(b) for b in bads], calls.n
        n, orc = calls.n, calls.orc
        self.case = case = Case(n, seed)
        for S in lens:
            case.stripe(S)
        image = case.image()
        rng = np.random.default_rng(seed + 1)
        self.expect = []
        for rows, bad in zip(case.items, self.bads):
            sh = [Slice(image[pos:pos + size].copy(), size) for pos, size in rows]
            assert orc.encode(sh) == EO.OK
            for i, ((pos, size), s) in enumerate(zip(rows, sh)):
                self.expect.append(zlib.crc32(s.buf.tobytes()))  # the checksum every shard came with
                image[pos:pos + size] = rng.integers(0, 256, size, dtype=np.uint8) if i in bad else s.buf
        for b, i, at in flips:
            pos, size = case.items[b][i]
            assert at < size and i not in self.bads[b]
            image[pos + at] ^= 0x40
        self.image = image
        self.want = image.copy()
        self.status, self.words, self.mismatch = [], [], []
        for b, (rows, bad) in enumerate(zip(case.items, self.bads)):
            sh = [Slice(image[pos:pos + size].copy(), size) for pos, size in rows]
            st = orc.reconstruct(sh, bad)
            if st == EO.OK:
                ok, st = orc.verify(sh)
                st = st if st else (EO.OK if ok else EO.ERR_VERIFY)
            self.status.append(st)
            if st in (EO.OK, EO.ERR_VERIFY):
                for (pos, size), s in zip(rows, sh):
                    assert s.buf.size == size and s.len == size, "the oracle allocated"
                    self.want[pos:pos + size] = s.buf
                w = [zlib.crc32(s.buf.tobytes()) for s in sh]
                exp = self.expect[b * n:(b + 1) * n]
                self.mismatch.append(next((i for i in range(n) if i not in bad and w[i] != exp[i]), -1))
            else:
                w = [0] * n
                self.mismatch.append(-1)
            self.words += w

    def run(self, kind, capfd=None, old=True):
        """The new call on one copy of the arena against the oracle, the old call on a second copy against
        the new one; returns (trace of the new call, trace of the old call)."""
        calls, n, nb = self.calls, self.n, len(self.lens)
        a = Mem(kind, self.image)
        arr = shard_array(self.case, a)
        if capfd:
            capfd.readouterr()
        rc, status, words, mism = calls.new(arr, nb, self.bads, a.mem, self.expect)
        got = a.read()
        err = capfd.readouterr().err if capfd else ""
        assert rc == 0, _lib.lib().cfsec_last_error()
        assert status == self.status, "statuses differ from the oracle's"
        bad_at = np.flatnonzero(got != self.want)
        assert bad_at.size == 0, "arena differs from the oracle's at %d bytes, first at %d" % (bad_at.size, bad_at[0])
        wrong = [(i // n, i % n) for i, (g, w) in enumerate(zip(words, self.words)) if g != w]
        assert not wrong, "checksum words differ from zlib's at (bid, shard) %s" % wrong[:8]
        if mism is not None:
            assert mism == self.mismatch, "mismatch differs from the survivors' check computed here"
        err_old = ""
        if old:
            b = Mem(kind, self.image)
            rc, st_old, words_old, mism_old = repair_call(self.calls.L.cfsec_ec_repair_batch_crc, calls.old_enc,
                                                          shard_array(self.case, b), n, nb, self.bads, b.mem,
                                                          self.expect)
            got_old = b.read()
            err_old = capfd.readouterr().err if capfd else ""
            assert rc == 0 and st_old == status, "statuses differ from cfsec_ec_repair_batch_crc's"
            assert words_old == words and np.array_equal(got_old, got)
            assert mism is None or mism_old == mism
        return err, err_old


def mixsv_lines(err):
    return [dict(x.split("=") for x in ln.split()[2:]) for ln in lines(err, "cfsec: mixsv ")]


def other_launches(err):
    """Product launches, fused product + checksum launches, separate checksum launches, the other mixed ones."""
    return lines(err, "cfsec: matvec ", "cfsec: dy16", "cfsec: crc32 ", "cfsec: crc ", "cfsec: bs ", "cfsec: mix ",
                 "cfsec: mixcrc ")


def one_launch(err, items, tiles, plans):
    mx = mixsv_lines(err)
    assert len(mx) == 1, err
    assert (int(mx[0]["items"]), int(mx[0]["tiles"]), int(mx[0]["plans"])) == (items, tiles, plans)
    assert other_launches(err) == [], err


# ---------------------------------------------------------------- modes, bad sets, lengths, alignments

# name -> (the calls, the bad set of every bid)
ROWS = {
    "EC12P4-1bad": ("EC12P4", [3]),                   # 1 stored + 3 compared rows, one pass
    "EC6P6-2bad": ("EC6P6", [1, 7]),                  # 6 output rows: the seam inside pass 0, pass 1 all compared
    "EC6P6-6bad": ("EC6P6", [0, 1, 2, 6, 7, 8]),      # nothing compared
    "EC6P6-0bad": ("EC6P6", []),                      # nstore = 0
    "EC6P10L2-1global": ("EC6P10L2", [2]),            # 12 output rows, three passes, local parities compared
    "rs16+4": ("rs16+4", [0, 17]),                    # 16 inputs, cfsec_rs_repair_crc_stripes
}
_CALLS = {}


def calls_for(name):
    if name not in _CALLS:
        _CALLS[name] = RsCalls(16, 4) if name == "rs16+4" else EcCalls(name)
    return _CALLS[name]


@pytest.mark.parametrize("row", list(ROWS))
def test_every_length_in_one_launch_device(row, monkeypatch, capfd):
    name, bad = ROWS[row]
    calls = calls_for(name)
    assert {(5 * c + 3 * j) % 16 for c in range(len(LENS)) for j in range(calls.n)} == set(range(16))
    tk = Tasklet(calls, LENS, [bad] * len(LENS), seed=len(row) + calls.n)
    assert tk.status == [0] * len(LENS) and tk.mismatch == [-1] * len(LENS)
    trace_on(monkeypatch)
    err, err_old = tk.run("device", capfd)
    one_launch(err, len(LENS), tiles_of(LENS), 1)
    assert mixsv_lines(err_old) == [] and other_launches(err_old) != [], "cfsec_ec_repair_batch_crc keeps its launches"
    # switched off: the launch groups, the same results (run() compares them with the same oracle values)
    trace_on(monkeypatch, limit=0)
    err, _ = tk.run("device", capfd, old=False)
    assert mixsv_lines(err) == [] and other_launches(err) != []


@pytest.mark.parametrize("kind", ["pinned", "pageable"])
@pytest.mark.parametrize("row", ["EC12P4-1bad", "EC6P10L2-1global"])
def test_every_length_in_one_launch_host(row, kind, monkeypatch, capfd):
    name, bad = ROWS[row]
    calls = calls_for(name)
    tk = Tasklet(calls, LENS, [bad] * len(LENS), seed=3 + calls.n)
    trace_on(monkeypatch)
    err, _ = tk.run(kind, capfd)
    one_launch(err, len(LENS), tiles_of(LENS), 1)


def test_a_bad_local_shard_falls_to_the_groups(monkeypatch, capfd):
    calls = calls_for("EC6P10L2")
    tk = Tasklet(calls, LENS, [[16]] * len(LENS), seed=41)  # two checksummed passes per bid
    assert tk.status == [0] * len(LENS)
    trace_on(monkeypatch)
    err, _ = tk.run("device", capfd)
    assert mixsv_lines(err) == [] and other_launches(err) != []
    # bids with and without one in the same call: the launch takes the ones without
    bads = [[16] if c % 3 == 0 else [2, 17] if c % 3 == 1 else [5] for c in range(len(LENS))]
    tk = Tasklet(calls, LENS, bads, seed=42)
    assert tk.status == [0] * len(LENS)
    err, _ = tk.run("device", capfd)
    mx = mixsv_lines(err)
    mine = [S for c, S in enumerate(LENS) if c % 3 == 2]
    assert len(mx) == 1 and (int(mx[0]["items"]), int(mx[0]["tiles"])) == (len(mine), tiles_of(mine)), err
    assert other_launches(err) != []


def test_distinct_bad_sets_share_one_launch(monkeypatch, capfd):
    calls = calls_for("EC6P6")
    sets = [[0], [5, 11], [1, 2, 3], [6, 7, 8, 9], [0, 4, 6, 10, 11], [0, 1, 2, 3, 4, 5], [], [11], [2, 9], [3, 4, 5],
            [0, 1, 6, 7]]
    tk = Tasklet(calls, LENS, sets, seed=51)
    assert tk.status == [0] * len(LENS)
    trace_on(monkeypatch)
    err, _ = tk.run("device", capfd)
    one_launch(err, len(LENS), tiles_of(LENS), len(sets))
    calls = calls_for("rs16+4")
    sets = [[c % 20] + ([19 - c % 7] if c % 2 else []) for c in range(len(LENS))]
    tk = Tasklet(calls, LENS, sets, seed=52)
    assert tk.status == [0] * len(LENS)
    err, _ = tk.run("pinned", capfd)
    one_launch(err, len(LENS), tiles_of(LENS), len({tuple(sorted(set(s))) for s in sets}))


# ---------------------------------------------------------------- the length limit, a lone bid

def test_a_lone_small_bid_and_a_long_bid_go_to_the_groups(monkeypatch, capfd):
    calls = calls_for("EC12P4")
    trace_on(monkeypatch)
    tk = Tasklet(calls, [2048], [[3]], seed=61)
    err, _ = tk.run("device", capfd)
    assert tk.status == [0] and mixsv_lines(err) == [] and other_launches(err) != []
    # 65537 bytes is past the limit: that bid keeps the groups, the two small ones share the launch
    lens = [4097, 65537, 100]
    tk = Tasklet(calls, lens, [[3]] * 3, seed=62)
    err, _ = tk.run("device", capfd)
    assert tk.status == [0, 0, 0]
    mx = mixsv_lines(err)
    assert len(mx) == 1 and (int(mx[0]["items"]), int(mx[0]["tiles"])) == (2, 3), err
    assert other_launches(err) != [], "the long bid keeps the launch groups"
    # and with one small bid beside it nothing is left for the launch
    tk = Tasklet(calls, [65537, 100], [[3]] * 2, seed=63)
    err, _ = tk.run("device", capfd)
    assert tk.status == [0, 0] and mixsv_lines(err) == [] and other_launches(err) != []


# ---------------------------------------------------------------- corruption

@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_one_flipped_byte_per_bid_between_clean_neighbours(kind, monkeypatch, capfd):
    calls = calls_for("EC12P4")
    one, four = [3], [3, 13, 14, 15]  # compared survivors 13, 14, 15; or exactly N survivors
    #        len    bad   flip (shard, byte)
    bids = [(8197, one, None),
            (8197, one, (13, 5)),          # a compared survivor's tile 0
            (2048, one, None),
            (12388, one, (14, 12338)),     # its last tile only: the flag comes from a non-first tile
            (4097, one, None),
            (4097, one, (15, 4096)),       # the last byte of a ragged row
            (31, one, None),
            (8197, one, (13, 8185)),       # inside the overlapped last chunk: read by two tiles, checksummed once
            (31, one, (14, 15)),           # the same within one tile
            (15, one, None),
            (15, one, (15, 14)),           # a row shorter than 16 bytes
            (1, one, (13, 0)),
            (4096, four, None),
            (4097, four, (0, 4090)),       # an input survivor with exactly N survivors: only mismatch tells
            (17, four, (12, 16)),
            (65536, one, None)]
    flips = [(b, f[0], f[1]) for b, (_, _, f) in enumerate(bids) if f]
    tk = Tasklet(calls, [b[0] for b in bids], [b[1] for b in bids], seed=71, flips=flips)
    n = calls.n
    for b, (_, bad, f) in enumerate(bids):  # on the oracle alone, before the GPU is touched
        if f is None:
            assert tk.status[b] == 0 and tk.mismatch[b] == -1, b
        elif bad is one:
            assert tk.status[b] == ERR_VERIFY and tk.mismatch[b] == f[0], b
            assert tk.words[b * n + f[0]] != tk.expect[b * n + f[0]]  # the corrupt shard's own checksum
        else:
            assert tk.status[b] == 0 and tk.mismatch[b] == f[0], b
    trace_on(monkeypatch)
    err, _ = tk.run(kind, capfd)
    lens = [b[0] for b in bids]
    one_launch(err, len(bids), tiles_of(lens), 2)
    # the same with the bids on both sides of a limit: Verify words from the launch and from the groups
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", "4097")
    err, _ = tk.run(kind, capfd, old=False)
    mx = mixsv_lines(err)
    assert len(mx) == 1 and int(mx[0]["items"]) == sum(ln <= 4097 for ln in lens)


CHILD_TIMEOUT = 12.0


@pytest.mark.skipif(CHILD, reason="the child process itself")
def test_verify_words_through_the_gather_in_child():
    """CFSEC_BATCH_DIRECT_FLAGS=0 (read once per process): the launch raises per-task words and the gather
    moves them to the bids -- the corruption case on device memory, the same statuses.  One child; ended by a
    signal, an abort or its time limit it ends the session: nothing more starts on the GPU after a fault."""
    env = dict(os.environ, CFSEC_REPAIR_BIDS_CHILD="1", CFSEC_BATCH_DIRECT_FLAGS="0")
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", __file__, "-k",
                            "test_one_flipped_byte and device"],
                           env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.exit(f"CFSEC_BATCH_DIRECT_FLAGS=0: the child ran into its time limit ({CHILD_TIMEOUT:.0f} s)",
                    returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        pytest.exit(f"CFSEC_BATCH_DIRECT_FLAGS=0: the child ended abnormally ({r.returncode})\n" + r.stdout[-2000:] +
                    r.stderr[-2000:], returncode=3)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert re.search(r"\b1 passed", r.stdout) and "failed" not in r.stdout, r.stdout[-2000:]


def test_failed_bids_between_good_ones(monkeypatch, capfd):
    calls = calls_for("EC12P4")
    lens = [2048, 3000, 4097, 17, 500]
    bads = [[3], [0, 1, 2, 3, 4], [15], [0, 1, 2, 3, 12], [0, 13]]  # five bad shards: too few survivors
    tk = Tasklet(calls, lens, bads, seed=81)
    assert [i for i, s in enumerate(tk.status) if s != 0] == [1, 3]
    trace_on(monkeypatch)
    err, _ = tk.run("device", capfd)
    one_launch(err, 3, tiles_of([2048, 4097, 500]), 3)


# ---------------------------------------------------------------- the Python methods

def test_python_methods_return_what_the_c_calls_return():
    rng = np.random.default_rng(91)
    lens = [2048, 17, 4097, 300]
    calls = calls_for("EC12P4")
    t, n = calls.t, calls.n
    bads = [[3], [0, 13], [], [1, 2, 3, 15]]
    bids, want = [], []
    for S, bad in zip(lens, bads):
        sh = EO.vector([rng.integers(0, 256, S, dtype=np.uint8) for _ in range(n)])
        assert calls.orc.encode(sh) == EO.OK
        want.append([zlib.crc32(s.buf.tobytes()) for s in sh])
        bids.append([np.zeros(S, np.uint8) if i in bad else s.buf.copy() for i, s in enumerate(sh)])
    bids[2][14][7] ^= 1
    status, words, mism = calls.enc.RepairBids(bids, bads, expect=want)
    assert status == [0, 0, ERR_VERIFY, 0] and mism == [-1, -1, 14, -1]
    want[2][14] = zlib.crc32(bids[2][14].tobytes())
    assert words == want
    assert [[zlib.crc32(np.asarray(a).tobytes()) for a in bid] for bid in bids] == want
    rs = reedsolomon.New(6, 3, device=0)
    stripes, want = [], []
    for S, miss in zip(lens, ([0], [4, 8], [], [1, 2, 3])):
        sh = EO.vector([rng.integers(0, 256, S, dtype=np.uint8) for _ in range(9)])
        assert EO.rs_encode(6, 3, sh) == EO.OK
        want.append([zlib.crc32(s.buf.tobytes()) for s in sh])
        stripes.append([None if i in miss else s.buf.copy() for i, s in enumerate(sh)])
    status, words = rs.RepairCRCStripes(stripes)
    assert status == [0] * 4 and words == want
    assert [[zlib.crc32(np.asarray(a).tobytes()) for a in st] for st in stripes] == want
