"""Every route of the checksummed calls gives the right bytes and words, and is the route the CPU-pinned
table (tests/crc_routes.py, tests/test_crc_route.py) names for that job.

cfsec_rs_reconstruct_crc_batch over the (N, M) of every code mode plus (8, 1), (18, 1), (6, 8):
erasure classes x sizes on both sides of the 2 KiB bit-sliced tile and the 4 KiB lookup tile (and a
ragged multi-tile tail) x one stripe, pitched, misaligned and scattered stripes.  ec.ReconstructBatch
and ec.EncodeBatch with checksums for every code mode.  References: zlib for the words, the C oracle's
Encode for the codeword (a rebuilt shard must equal it), the ec oracle's Encode / repair at the ec
level -- never another path of the library.  With CFSEC_TRACE_CRC / CFSEC_TRACE_BATCH the library
names the route it took; "no fused launch" is asserted where the table has none (EC10P4, EC4P4, EC3P3
with outputs-only checksums: the product and the separate pass).

The masks that gate the routes are read once per process, so the module runs again in a child per
setting (CFSEC_BS_CRC=0 / 255, CFSEC_CRC_LDS=0, CFSEC_BATCH_FUSED_CRC=0).

Nothing here needs shards above 70 KiB: the 512 MiB limits of the bit-sliced kernels and the 2^32
tile counter are covered by the CPU test (tests/test_crc_route.py) only.
"""
import functools
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

import crc_routes as R
from chubaofs_amd import _lib, codemode as cm
from oracle import oracle as O
from oracle.ec_oracle import ECOracle, Slice

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CHILD = os.environ.get("CFSEC_CRC_ROUTES_CHILD") is not None
BS_MASK = int(os.environ.get("CFSEC_BS_CRC") or str(R.BS_CRC_DEFAULT), 0)
LDS = int(os.environ.get("CFSEC_CRC_LDS") or "1") != 0
BATCH_FUSED = not (os.environ.get("CFSEC_BATCH_FUSED_CRC") or "1").startswith("0")

MODES = cm.GetAllCodeModes()
RS_SHAPES = sorted({(cm.GetTactic(c).N, cm.GetTactic(c).M) for c in MODES} | {(8, 1), (18, 1), (6, 8)})
SIZES = [1, 2047, 2048, 2049, 3 * 2048 + 48, 70001]
LAYOUTS = ["one", "pitched", "misaligned", "scattered"]
CANARY, JUNK = 0xA5, 0xEE


def erasure_classes(k, m):
    """(name, erased, data_only); one data + one parity needs M >= 2 (not (8, 1), (18, 1))."""
    out = [("all_parity", list(range(k, k + m)), False), ("first_parity", [k], False),
           ("data", list(range(min(m, k))), False)]
    if m >= 2:
        out.append(("data_parity", [0, k], False))
    out.append(("all_parity_data_only", list(range(k, k + m)), True))
    return out


RS_CASES = [pytest.param(k, m, er, do, id=f"{k}p{m}-{name}") for k, m in RS_SHAPES for name, er, do in erasure_classes(k, m)]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def codeword(k, m, S):
    """5 stripes of the C oracle's Encode over seeded data: (5, k + m, S), computed once, read-only."""
    rng = np.random.default_rng(1000003 * k + 1009 * m + S)
    cw = np.zeros((5, k + m, S), np.uint8)
    cw[:, :k] = rng.integers(0, 256, (5, k, S), dtype=np.uint8)
    for s in range(5):
        rows = [cw[s, i].copy() for i in range(k + m)]
        assert O.encode(k, m, rows) == 0
        cw[s] = np.stack(rows)
    cw.setflags(write=False)
    return cw


@pytest.fixture(scope="module")
def rs():
    from chubaofs_amd import reedsolomon
    return reedsolomon


def place(k, m, S, layout):
    """Byte offsets of shard (s, i) in one buffer, its size, and the stripes."""
    total = k + m
    nst = 1 if layout == "one" else 5
    if layout == "misaligned":
        pitch = S + 1  # rows start at every alignment
    else:
        pitch = (S + 255) // 256 * 256
    if layout == "scattered":  # no common stripe stride: the launches go through the pointer table
        pitch += 256
        off = [[(s * total + i) * pitch + 256 * s * s for i in range(total)] for s in range(nst)]
        size = off[-1][-1] + pitch
    else:
        off = [[(s * total + i) * pitch for i in range(total)] for s in range(nst)]
        size = nst * total * pitch
    return nst, off, size


@pytest.mark.parametrize("k,m,erased,data_only", RS_CASES)
def test_reconstruct_crc_batch_routes(rs, k, m, erased, data_only, monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    total = k + m
    enc = rs.New(k, m)
    rebuilt = [i for i in erased if i < k or not data_only]
    for S in SIZES:
        for layout in LAYOUTS:
            nst, off, size = place(k, m, S, layout)
            cw = codeword(k, m, S)
            before = np.full(size, CANARY, np.uint8)  # every byte outside the shards is a canary
            want = before.copy()
            for s in range(nst):
                for i in range(total):
                    before[off[s][i]:off[s][i] + S] = JUNK if i in erased else cw[s, i]
                    want[off[s][i]:off[s][i] + S] = JUNK if i in erased and i not in rebuilt else cw[s, i]
            dev = torch.from_numpy(before).cuda()
            ptrs = [dev.data_ptr() + off[s][i] for s in range(nst) for i in range(total)]
            crcs = torch.full((nst * total,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            capfd.readouterr()
            enc.reconstruct_crc_batch(ptrs, S, nst, erased, crcs.data_ptr(), data_only=data_only)
            torch.cuda.synchronize()
            err = capfd.readouterr().err
            where = (k, m, erased, data_only, S, layout)
            # rebuilt rows equal the codeword; survivors, the rows not asked for and every pad byte
            # are what they were
            got = dev.cpu().numpy()
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                pytest.fail(f"{where}: {bad.size} bytes differ, first at {int(bad[0])}")
            words = crcs.cpu().numpy().view(np.uint32).reshape(nst, total)
            for s in range(nst):
                for i in range(total):
                    w = crc(cw[s, i]) if i in rebuilt else 0
                    assert int(words[s, i]) == w, (where, s, i, hex(int(words[s, i])), hex(w))
            route = R.expect_route(k, len(rebuilt), False, S, nst, bs_mask=BS_MASK, lds=LDS)
            if route == R.NONE:
                assert "crc route=" not in err and "bs crc" not in err, (where, err)
            else:
                line = f"cfsec: crc route={route} k={k} m={len(rebuilt)} cin=0 stripes={nst} len={S}\n"
                assert err.count("crc route=") == 1 and line in err, (where, err)


# ------------------------------------------------------------------ ec.Encoder batches

def ec_new(t):
    from chubaofs_amd import ec
    return ec.NewEncoder(ec.Config(CodeMode=t, EnableVerify=False), device=0)


@functools.lru_cache(maxsize=None)
def ec_codeword(mode, S, seed):
    """The ec oracle's Encode (global, then local parity) over seeded data, read-only."""
    t = cm.GetTactic(mode)
    rng = np.random.default_rng(7919 * mode + 31 * S + seed)
    sh = [Slice.of(rng.integers(0, 256, S, dtype=np.uint8)) for _ in range(t.N)] + \
         [Slice.of(np.zeros(S, np.uint8)) for _ in range(t.M + t.L)]
    assert ECOracle.from_tactic(t).encode(sh) == 0
    out = [x.view().copy() for x in sh]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def encode_matrix(mode):
    """The (M + L) x N matrix of the mode's Encode, read off the ec oracle one unit vector at a time."""
    t = cm.GetTactic(mode)
    cols = []
    for c in range(t.N):
        sh = [Slice.of(np.array([1 if i == c else 0], np.uint8)) for i in range(t.N)] + \
             [Slice.of(np.zeros(1, np.uint8)) for _ in range(t.M + t.L)]
        assert ECOracle.from_tactic(t).encode(sh) == 0
        cols.append([int(x.view()[0]) for x in sh[t.N:]])
    return bytes(cols[c][r] for r in range(t.M + t.L) for c in range(t.N))


def repair_reference(t, shards, bad, verify):
    work = [Slice.of(s.copy()) for s in shards]
    st = ECOracle.from_tactic(t).repair(work, list(bad), verify=verify)
    return st, [w.view().copy() for w in work]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def fused_lines(err):
    return [ln for ln in err.splitlines() if "fused crc group" in ln]


@pytest.mark.parametrize("mode", MODES, ids=cm.Name)
def test_ec_reconstruct_batch_routes(mode, monkeypatch, capfd):
    """Six equal-length device bids with every global parity shard lost (Reconstruct without Verify:
    one plain store group, k = N, m = M, the rebuilt shards checksummed), then a ragged host set."""
    monkeypatch.setenv("CFSEC_TRACE_BATCH", "1")
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    t = cm.GetTactic(mode)
    total, S = t.N + t.M + t.L, 2049
    enc = ec_new(t)
    bad = list(range(t.N, t.N + t.M))
    bids, want = [], []
    for b in range(6):
        good = ec_codeword(mode, S, b)
        src = [np.full(S, JUNK, np.uint8) if i in bad else good[i].copy() for i in range(total)]
        want.append(repair_reference(t, src, bad, False))
        bids.append([torch.from_numpy(x).cuda() for x in src])
    capfd.readouterr()
    st, crcs = enc.ReconstructBatch(bids, [bad] * 6, verify=False, crcs=True)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    for b, (exp, shards) in enumerate(want):
        assert exp == 0 and st[b] == 0, (b, st[b], exp)
        for i in range(total):
            assert np.array_equal(host(bids[b][i]), shards[i]), (b, i)
            assert np.array_equal(shards[i], ec_codeword(mode, S, b)[i]), (b, i)
            assert crcs[b][i] == (crc(shards[i]) if i in bad else 0), (cm.Name(mode), b, i, hex(crcs[b][i]))
    route = R.expect_route(t.N, t.M, False, S, 6, bs_mask=BS_MASK, lds=LDS)
    if BATCH_FUSED and route != R.NONE:
        assert fused_lines(err) == [f"cfsec batch: fused crc group k={t.N} m={t.M} tasks=6 len={S}"], err
        assert f"cfsec: crc route={route} k={t.N} m={t.M} cin=0 stripes=6 len={S}\n" in err, err
    else:
        assert not fused_lines(err) and "crc route=" not in err, err
    # ragged sizes in host memory, Reconstruct + Verify, seeded bad sets (a local parity among them)
    r = random.Random(mode)
    bids, bads, want = [], [], []
    for b, size in enumerate([1, 23, 2048, 4097]):
        good = ec_codeword(mode, size, 10 + b)
        bb = [2, total - 1] if t.L and b == 1 else sorted(r.sample(range(t.N + t.M), r.randint(1, t.M)))
        src = [np.zeros(size, np.uint8) if i in bb else good[i].copy() for i in range(total)]
        want.append(repair_reference(t, src, bb, True))
        bids.append(src)
        bads.append(bb)
    capfd.readouterr()
    st, crcs = enc.ReconstructBatch(bids, bads, crcs=True)
    err = capfd.readouterr().err
    for b, (exp, shards) in enumerate(want):
        assert st[b] == exp == 0, (b, st[b], exp)
        for i in range(total):
            assert np.array_equal(bids[b][i], shards[i]), (b, bads[b], i)
            assert crcs[b][i] == (crc(shards[i]) if i in bads[b] else 0), (cm.Name(mode), b, bads[b], i)
    for ln in fused_lines(err):  # a group that fused had a route
        f = dict(x.split("=") for x in ln.split()[5:])
        assert BATCH_FUSED and R.expect_route(int(f["k"]), int(f["m"]), False, int(f["len"]), int(f["tasks"]),
                                              bs_mask=BS_MASK, lds=LDS) != R.NONE, ln


@pytest.mark.parametrize("S", [2047, 2049])
@pytest.mark.parametrize("mode", MODES, ids=cm.Name)
def test_ec_encode_batch_routes(mode, S, monkeypatch, capfd):
    """Five device bids, every shard checksummed (the put path): the mode's network where its mask bit
    is set, else the lookup / v_perm kernels or the product and the separate pass."""
    monkeypatch.setenv("CFSEC_TRACE_BATCH", "1")
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    t = cm.GetTactic(mode)
    total, k, m = t.N + t.M + t.L, t.N, t.M + t.L
    enc = ec_new(t)
    stripes = []
    for b in range(5):
        good = ec_codeword(mode, S, 20 + b)
        stripes.append([torch.from_numpy(good[i].copy() if i < k else np.full(S, JUNK, np.uint8)).cuda()
                        for i in range(total)])
    capfd.readouterr()
    st, crcs = enc.EncodeBatch(stripes, crcs=True)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert st == [0] * 5
    for b in range(5):
        good = ec_codeword(mode, S, 20 + b)
        for i in range(total):
            assert np.array_equal(host(stripes[b][i]), good[i]), (cm.Name(mode), b, i)
            assert crcs[b][i] == crc(good[i]), (cm.Name(mode), b, i, hex(crcs[b][i]), hex(crc(good[i])))
    coef = encode_matrix(mode)
    route = R.expect_route(k, m, True, S, 5, R.match_bits(k, m, coef), m == 12 and k == 6 and R.dyadic_6x12(coef),
                           bs_mask=BS_MASK, lds=LDS)
    if BATCH_FUSED and route != R.NONE:
        assert fused_lines(err) == [f"cfsec batch: fused crc group k={k} m={m} tasks=5 len={S}"], err
        assert f"cfsec: crc route={route} k={k} m={m} cin=1 stripes=5 len={S}\n" in err, err
    else:
        assert not fused_lines(err) and "crc route=" not in err, err


# ------------------------------------------------------------------ the routes behind the env masks

# Measured on the MI355X: this module in-process (children excluded, 108 tests) 6.7 s of wall time for
# the whole python process (4.7 s inside pytest), `import torch` 1.6 s; a child gets three times the
# first plus the second.
MODULE_SECONDS = 6.7
IMPORT_SECONDS = 1.6
CHILD_TIMEOUT = 3 * MODULE_SECONDS + IMPORT_SECONDS


@pytest.mark.skipif(CHILD, reason="the child process itself")
@pytest.mark.parametrize("setting", ["CFSEC_BS_CRC=0", "CFSEC_BS_CRC=255", "CFSEC_CRC_LDS=0", "CFSEC_BATCH_FUSED_CRC=0"])
def test_routes_in_child(setting):
    """This module again under one setting of the masks, one child at a time.  A child that ends by a
    signal, an abort or its time limit ends the session: nothing more starts on the GPU after a fault."""
    name, value = setting.split("=")
    env = dict(os.environ, CFSEC_CRC_ROUTES_CHILD="1")
    env[name] = value
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", __file__],
                           env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{setting}: the child ran into its time limit ({CHILD_TIMEOUT:.0f} s)", returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        pytest.exit(f"{setting}: the child ended abnormally ({r.returncode})\n" + r.stdout[-2000:] + r.stderr[-2000:],
                    returncode=3)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
