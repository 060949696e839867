"""Repair tasklets of mixed-size bids of the 16 + 20 code on the GPU: cfsec_ec_repair_bids_crc (EC16P20L2,
EC16P20) and cfsec_rs_repair_crc_stripes (RS(16, 20)) through the mixed-plan repair launch that drives the
16x16-dyadic product from an item table (gf_mix_sv16.hip), and the launch groups behind it.

The arena, the oracle and what is asserted are test_gpu_repair_bids.py's (Tasklet.run): for every bid of
every case, none left out, status for status against ECOracle.reconstruct + verify and against
cfsec_ec_repair_batch_crc on a second copy of the arena; the whole arena byte for byte (guard bytes and
failed bids' buffers included); every word against zlib.crc32 of the shard as it stands; mismatch[]; the
launches traced.  Every row sits at its own offset 0..15 from a 16-byte boundary.

Sizes are LENS, the seams of the kernel: rows shorter than a 16-byte piece (1, 15), a whole piece (16), the
overlapped last chunk (17, 31, 4095, 8197), the 4 KiB tile seam (4095, 4096, 4097), several tiles XOR-ed
into one word (8197, 65536), and 12388 where a flag must come from a non-first tile.  None is a workload
size.  Bad sets: every count of missing data rows 0..4, stand-ins in the first, the last and neighbouring
slots, nothing stored, nothing compared in the global code, stored rows in the 16x16 block and in the 4x4
row block.
"""
import os
import re
import subprocess
import sys

import pytest

from chubaofs_amd import _lib, ec
from chubaofs_amd.codemode import Tactic
from oracle.ec_oracle import ECOracle
from test_gpu_encode_blobs_crc import LENS, lines, tiles_of, trace_on
from test_gpu_repair_bids import EcCalls, RsCalls, Tasklet, mixsv_lines, other_launches

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ERR_VERIFY = _lib.ErrVerify.status
CHILD = os.environ.get("CFSEC_REPAIR_BIDS16_CHILD") == "1"

C5 = [0, 1, 16, 17]                               # BASELINE configs[3-4]: 2 data + 2 parity
TWENTY = [0, 1, 2, 3] + list(range(16, 32))       # 20 bad: exactly 16 survivors in the global code
FIVE = [0, 1, 2, 3, 4]                            # five missing data rows: no dy16 plan


def mixsv16_lines(err):
    return [dict(x.split("=") for x in ln.split()[2:]) for ln in lines(err, "cfsec: mixsv16 ")]


def one_launch16(err, items, tiles, plans):
    mx = mixsv16_lines(err)
    assert len(mx) == 1, err
    assert (int(mx[0]["items"]), int(mx[0]["tiles"]), int(mx[0]["plans"])) == (items, tiles, plans)
    assert mixsv_lines(err) == [] and other_launches(err) == [], err


ROWS = {
    "EC16P20L2-c5": ("EC16P20L2", C5),    # nd = 2, 2 stored + 16 compared parity rows, 2 local rows compared
    "EC16P20-1bad": ("EC16P20", [3]),     # nd = 1, 19 compared rows, no extra rows
    "rs16+20": ("rs16+20", [0, 17]),      # cfsec_rs_repair_crc_stripes
}
_CALLS = {}


class Ec16P20Calls(EcCalls):
    """EC16P20L2's RS sibling, 36 shards in one AZ: no code mode names it, so its Tactic is spelled out."""

    def __init__(self):
        self.t = Tactic(16, 20, 0, 1, 16, 0, 0)
        self.n = 36
        self.enc = ec.NewEncoder(ec.Config(CodeMode=self.t, EnableVerify=False))
        self.old_enc = self.enc
        self.orc = ECOracle.from_tactic(self.t)
        self.L = self.enc._L


def calls_for(name):
    if name not in _CALLS:
        _CALLS[name] = RsCalls(16, 20) if name == "rs16+20" else Ec16P20Calls() if name == "EC16P20" else EcCalls(name)
    return _CALLS[name]


# ---------------------------------------------------------------- 1. every length, one launch

@pytest.mark.parametrize("row", list(ROWS))
def test_every_length_in_one_launch_device(row, monkeypatch, capfd):
    name, bad = ROWS[row]
    calls = calls_for(name)
    assert {(5 * c + 3 * j) % 16 for c in range(len(LENS)) for j in range(calls.n)} == set(range(16))
    tk = Tasklet(calls, LENS, [bad] * len(LENS), seed=len(row) + calls.n)
    assert tk.status == [0] * len(LENS) and tk.mismatch == [-1] * len(LENS)
    trace_on(monkeypatch)
    err, err_old = tk.run("device", capfd)
    one_launch16(err, len(LENS), tiles_of(LENS), 1)
    assert mixsv16_lines(err_old) == [] and mixsv_lines(err_old) == [] and other_launches(err_old) != [], \
        "cfsec_ec_repair_batch_crc keeps its launches"
    # switched off: the launch groups, the same results (run() compares them with the same oracle values)
    trace_on(monkeypatch, limit=0)
    err, _ = tk.run("device", capfd, old=False)
    assert mixsv16_lines(err) == [] and mixsv_lines(err) == [] and other_launches(err) != []


# ---------------------------------------------------------------- 2. every nd, both seams

def test_every_count_of_missing_data_rows_and_a_generic_pair_beside(monkeypatch, capfd):
    calls = calls_for("EC16P20L2")
    sets = [[], [16, 17], [3], [0, 5, 15], [1, 2, 3, 4], [7, 8, 20, 33], TWENTY]
    #       nothing stored; nd = 0; 1; 3; 4; 2 with the 16x16 block and the 4x4 row block stored; nothing compared
    bads = sets[:4] + [FIVE] + sets[4:] + [FIVE, [3], [0, 5, 15]]
    assert len(bads) == len(LENS)
    tk = Tasklet(calls, LENS, bads, seed=52)
    assert tk.status == [0] * len(LENS) and tk.mismatch == [-1] * len(LENS)
    trace_on(monkeypatch)
    err, _ = tk.run("device", capfd)
    mine = [S for S, b in zip(LENS, bads) if b is not FIVE]
    theirs = [S for S, b in zip(LENS, bads) if b is FIVE]
    mx = mixsv16_lines(err)
    assert len(mx) == 1, err
    assert (int(mx[0]["items"]), int(mx[0]["tiles"]), int(mx[0]["plans"])) == (len(mine), tiles_of(mine), len(sets))
    g = mixsv_lines(err)  # five missing data rows: no dy16 plan, the generic launch takes the pair
    assert len(g) == 1 and (int(g[0]["items"]), int(g[0]["tiles"]), int(g[0]["plans"])) == (2, tiles_of(theirs), 1), err
    assert other_launches(err) == [], err


def test_every_count_of_missing_data_rows_without_local_parities(monkeypatch, capfd):
    calls = calls_for("EC16P20")  # e = 0: the extra rows' tables are zero and their mask bits empty
    sets = [[], [16, 17], [3], [0, 5, 15], [1, 2, 3, 4], [7, 8, 20, 33], TWENTY]
    bads = sets + sets[2:5] + [TWENTY]
    # and an input survivor's flipped byte in a bid with exactly 16 survivors: nothing is compared, the
    # status stays 0 and only mismatch[] tells
    tk = Tasklet(calls, LENS, bads, seed=53, flips=[(10, 5, 8190)])
    assert LENS[10] == 65536 and bads[10] is TWENTY
    assert tk.status == [0] * len(LENS) and tk.mismatch == [-1] * 10 + [5]
    trace_on(monkeypatch)
    err, _ = tk.run("pinned", capfd)
    one_launch16(err, len(LENS), tiles_of(LENS), len(sets))


# ---------------------------------------------------------------- 3. corruption

#        len    bad   flip (shard, byte)
BIDS = [(8197, C5, None),
        (8197, C5, (20, 5)),           # a compared parity row of the 16x16 block, tile 0
        (2048, C5, None),
        (12388, C5, (34, 12338)),      # one of the 4x4 row block, its last tile only: the flag from a non-first tile
        (4096, C5, (36, 77)),          # a local parity (an extra row)
        (4097, C5, None),
        (4097, C5, (21, 4096)),        # the last byte of a ragged row
        (31, C5, None),
        (8197, C5, (22, 8185)),        # inside the overlapped last chunk: read by two tiles, checksummed once
        (31, C5, (23, 15)),            # the same within one tile
        (15, C5, None),
        (15, C5, (24, 14)),            # a row shorter than 16 bytes
        (1, C5, (25, 0)),
        (4096, TWENTY, None),
        (4097, C5, (5, 4090)),         # an input survivor: every compared row differs
        (4097, TWENTY, (5, 4090)),     # the same with nothing compared in the global code
        (65536, C5, None)]


def corruption_tasklet():
    calls = calls_for("EC16P20L2")
    flips = [(b, f[0], f[1]) for b, (_, _, f) in enumerate(BIDS) if f]
    tk = Tasklet(calls, [b[0] for b in BIDS], [b[1] for b in BIDS], seed=71, flips=flips)
    n = calls.n
    for b, (_, bad, f) in enumerate(BIDS):  # on the oracle alone, before the GPU is touched
        if f is None:
            assert tk.status[b] == 0 and tk.mismatch[b] == -1, b
        else:
            # ErrVerify in the 20-bad bid too: the global code compares nothing there, but the local parities
            # are compared and data row 5 is under one of them (the 36-shard case, where only mismatch[]
            # tells, is in test_every_count_of_missing_data_rows_without_local_parities)
            assert tk.status[b] == ERR_VERIFY and tk.mismatch[b] == f[0], b
            assert tk.words[b * n + f[0]] != tk.expect[b * n + f[0]]  # the corrupt shard's own checksum
    return tk


@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_one_flipped_byte_per_bid_between_clean_neighbours(kind, monkeypatch, capfd):
    tk = corruption_tasklet()
    trace_on(monkeypatch)
    err, _ = tk.run(kind, capfd)
    lens = [b[0] for b in BIDS]
    one_launch16(err, len(BIDS), tiles_of(lens), 2)
    # the same with the bids on both sides of a limit: Verify words from the launch and from the groups
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", "4097")
    err, _ = tk.run(kind, capfd, old=False)
    mx = mixsv16_lines(err)
    assert len(mx) == 1 and int(mx[0]["items"]) == sum(ln <= 4097 for ln in lens), err
    assert other_launches(err) != [], "the long bids keep the launch groups"


# ---------------------------------------------------------------- 4. pageable host memory

def test_every_length_in_one_launch_pageable(monkeypatch, capfd):
    name, bad = ROWS["EC16P20L2-c5"]
    calls = calls_for(name)
    tk = Tasklet(calls, LENS, [bad] * len(LENS), seed=3 + calls.n)
    assert tk.status == [0] * len(LENS)
    trace_on(monkeypatch)
    err, _ = tk.run("pageable", capfd)
    one_launch16(err, len(LENS), tiles_of(LENS), 1)


# ---------------------------------------------------------------- 5. the gather route

CHILD_TIMEOUT = 20.0


@pytest.mark.skipif(CHILD, reason="the child process itself")
def test_verify_words_through_the_gather_in_child():
    """CFSEC_BATCH_DIRECT_FLAGS=0 (read once per process): the launch raises per-task words and the gather
    moves them to the bids -- the corruption case on device memory, the same statuses.  One child; ended by a
    signal, an abort or its time limit it ends the session: nothing more starts on the GPU after a fault."""
    env = dict(os.environ, CFSEC_REPAIR_BIDS16_CHILD="1", CFSEC_BATCH_DIRECT_FLAGS="0")
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
