"""Every family and every bit-sliced prefix of the plain product gives the right bytes, and the launches
it traces (CFSEC_TRACE_MATVEC) are the ones the CPU-pinned table (tests/matvec_routes.py,
tests/test_matvec_route.py) names for the job.

The shapes are the smallest at which each path, and each hand-over between a prefix and its tail, can
go wrong: a few KiB per shard, 2 stripes (8 where the pointer-table form needs more stripes than one
argument block holds).  References: the C oracle's Encode for the Reed-Solomon shapes, the ec oracle's
Encode / repair for the LRC ones -- never another path of the library.  Every shard is followed by
canary bytes, which must survive."""
import numpy as np
import pytest

import matvec_routes as MR
from chubaofs_amd import codemode as cm
from oracle import oracle as O
from oracle.ec_oracle import ECOracle, Slice

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CANARY, JUNK = 0xA5, 0xEE


def mode_of(name):
    (c,) = [c for c in cm.GetAllCodeModes() if cm.Name(c) == name]
    return cm.GetTactic(c)


def rs_codeword(k, m, S, nst):
    rng = np.random.default_rng(1000003 * k + 1009 * m + S)
    cw = np.zeros((nst, k + m, S), np.uint8)
    cw[:, :k] = rng.integers(0, 256, (nst, k, S), dtype=np.uint8)
    for s in range(nst):
        rows = [cw[s, i].copy() for i in range(k + m)]
        assert O.encode(k, m, rows) == 0
        cw[s] = np.stack(rows)
    return cw


def ec_codeword(t, S, nst):
    rng = np.random.default_rng(7919 * t.N + 31 * S + t.L)
    cw = np.zeros((nst, t.N + t.M + t.L, S), np.uint8)
    for s in range(nst):
        sh = [Slice.of(rng.integers(0, 256, S, dtype=np.uint8)) for _ in range(t.N)] + \
             [Slice.of(np.zeros(S, np.uint8)) for _ in range(t.M + t.L)]
        assert ECOracle.from_tactic(t).encode(sh) == 0
        cw[s] = np.stack([x.view() for x in sh])
    return cw


def place(total, S, nst, layout):
    """Byte offset of shard (s, i) in one buffer and its size; at least 256 canary bytes after every shard."""
    pitch = (S + 255) // 256 * 256 + 256
    off = [[(s * total + i) * pitch + 256 for i in range(total)] for s in range(nst)]
    if layout == "off1":  # one row 1 byte off in every stripe: still one stride, no longer aligned
        for s in range(nst):
            off[s][1] += 1
    if layout == "scattered":  # no common stride between the stripes
        off = [[o + 512 * s * s for o in off[s]] for s in range(nst)]
    return off, off[-1][-1] + pitch


def traced(err):
    out = []
    for ln in err.splitlines():
        if ln.startswith("cfsec: matvec "):
            out.append(dict(x.split("=") for x in ln.split()[2:]))
    return out


def want_trace(k, m, coef, mode, nstore, S, nst, layout):
    steps = MR.expect_plan(k, m, coef, mode, nstore, S, nst, affine=layout != "scattered" and nst > 1,
                           aligned=layout != "off1")
    return [dict(x.split("=") for x in MR.trace_line(s, layout != "scattered" and nst > 1).split()[2:]) for s in steps]


def run_store(call, k, m, coef, cw, S, nst, layout, capfd):
    """call(ptrs) computes the m output shards of every stripe from its k inputs; cw the codeword."""
    total = k + m
    off, size = place(total, S, nst, layout)
    before = np.full(size, CANARY, np.uint8)
    want = before.copy()
    for s in range(nst):
        for i in range(total):
            before[off[s][i]:off[s][i] + S] = cw[s, i] if i < k else JUNK
            want[off[s][i]:off[s][i] + S] = cw[s, i]
    dev = torch.from_numpy(before).cuda()
    assert dev.data_ptr() % 256 == 0
    capfd.readouterr()
    call([dev.data_ptr() + off[s][i] for s in range(nst) for i in range(total)])
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    got = dev.cpu().numpy()
    if not np.array_equal(got, want):  # shards and the canaries after every row
        bad = np.flatnonzero(got != want)
        pytest.fail(f"{(k, m, S, nst, layout)}: {bad.size} bytes differ, first at {int(bad[0])}")
    assert traced(err) == want_trace(k, m, coef, MR.STORE, 0, S, nst, layout), err
    return traced(err)


def ec_encoder(t):
    from chubaofs_amd import ec
    return ec.NewEncoder(ec.Config(CodeMode=t, EnableVerify=False), device=0)


@pytest.mark.parametrize("S,nst,layout,shape", [
    (2048 + 17, 2, "affine", [("dyadic-16", "encode", 2048, 17)]),
    (2048 + 17, 2, "off1", [("dyadic-16", "none", 0, 2048 + 17)]),
    (2048, 8, "scattered", [("dyadic-16", "table", 2048, 0)]),
    (2048 + 17, 8, "scattered", [("dyadic-16", "table", 2048, 0), ("dyadic-16", "none", 0, 17), ("dyadic-16", "none", 0, 17)]),
])
def test_ec16p20l2_fused_encode(S, nst, layout, shape, monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    t = mode_of("EC16P20L2")
    enc = ec_encoder(t)
    ins, rows = enc.repair_rows([], list(range(t.N, t.N + t.M + t.L)))
    assert ins == list(range(t.N))
    got = run_store(lambda p: enc.matvec_batch(rows, p, S, nst), t.N, t.M + t.L, b"".join(rows),
                    ec_codeword(t, S, nst), S, nst, layout, capfd)
    assert [(g["family"], g["bs"], int(g["prefix"]), int(g["tail"])) for g in got] == shape


@pytest.mark.parametrize("flip", [None, 100, 4096])
def test_ec16p20_verify(flip, monkeypatch, capfd):
    """Clean, then one flipped byte inside the bit-sliced prefix, then one in the tail."""
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    from chubaofs_amd import reedsolomon
    k, m, S, nst = 16, 20, 4096 + 1, 2
    enc = reedsolomon.New(k, m)
    cw = rs_codeword(k, m, S, nst)
    off, size = place(k + m, S, nst, "affine")
    buf = np.full(size, CANARY, np.uint8)
    for s in range(nst):
        for i in range(k + m):
            buf[off[s][i]:off[s][i] + S] = cw[s, i]
    if flip is not None:
        buf[off[1][k + 7] + flip] ^= 0x10
    dev = torch.from_numpy(buf).cuda()
    flags = torch.zeros(nst, dtype=torch.int32, device="cuda")
    capfd.readouterr()
    enc.verify_batch([dev.data_ptr() + off[s][i] for s in range(nst) for i in range(k + m)], S, nst, flags.data_ptr())
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert flags.cpu().tolist() == [0, 0 if flip is None else 1]
    assert np.array_equal(dev.cpu().numpy(), buf)  # a Verify writes nothing
    got = traced(err)
    assert got == want_trace(k, m, enc.matrix()[k:].tobytes(), MR.VERIFY, 0, S, nst, "affine"), err
    assert [(g["family"], g["bs"], g["prefix"], g["tail"]) for g in got] == [("dyadic-16", "verify", "4096", "1")]


@pytest.mark.parametrize("k,m,S,families", [
    (12, 4, 4097, ["dyadic"]), (6, 6, 4097, ["dyadic"]), (12, 9, 4097, ["lookup"]), (10, 4, 4097, ["fixed-k"]),
    (5, 2, 4097, ["runtime-k"]), (33, 2, 1025, ["runtime-k", "runtime-k"]), (4, 33, 1025, ["runtime-k", "fixed-k"]),
])
def test_rs_encode_families(k, m, S, families, monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    from chubaofs_amd import reedsolomon
    enc = reedsolomon.New(k, m)
    got = run_store(lambda p: enc.encode_batch(p, S, 2), k, m, enc.matrix()[k:].tobytes(), rs_codeword(k, m, S, 2), S, 2,
                    "affine", capfd)
    assert [g["family"] for g in got] == families
    if (k, m) == (33, 2):
        assert [(g["mode"], g["c0"], g["k"]) for g in got] == [("store", "0", "32"), ("accum", "32", "1")]
    if (k, m) == (4, 33):
        assert [(g["r0"], g["m"]) for g in got] == [("0", "32"), ("32", "1")]
    if (k, m) in ((12, 4), (6, 6)):
        B = 4 if k == 12 else 2
        assert MR.dyadic_form(enc.matrix()[k:].tobytes(), k, m) == (B, 0)


def test_ec6p6l9_fused_encode_is_the_bit_sliced_plain_product(monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    t = mode_of("EC6P6L9")
    enc = ec_encoder(t)
    ins, rows = enc.repair_rows([], list(range(t.N, t.N + t.M + t.L)))
    got = run_store(lambda p: enc.matvec_batch(rows, p, 2049, 2), t.N, t.M + t.L, b"".join(rows),
                    ec_codeword(t, 2049, 2), 2049, 2, "affine", capfd)
    assert [g["family"] for g in got] == ["bs-plain"]


def repair_case(t, S, nbid, bad, scattered):
    """nbid bids carved from one pool, at one pitch or (scattered) with uneven gaps between the bids, the
    bad shards junk and canary bytes after every shard; the bids, the ec oracle's status per bid, and
    the image of the whole pool after the oracle's repair."""
    total = t.N + t.M + t.L
    cw = ec_codeword(t, S, nbid)
    pitch = (S + 255) // 256 * 256 + 256
    base = [b * total * pitch + (512 * b * b if scattered else 0) for b in range(nbid)]
    before = np.full(base[-1] + total * pitch, CANARY, np.uint8)
    want = before.copy()
    status = []
    for b in range(nbid):
        work = [Slice.of(np.full(S, JUNK, np.uint8) if i in bad else cw[b, i].copy()) for i in range(total)]
        for i, w in enumerate(work):
            before[base[b] + i * pitch:base[b] + i * pitch + S] = w.view()
        status.append(ECOracle.from_tactic(t).repair(work, list(bad), verify=True))
        for i, w in enumerate(work):
            want[base[b] + i * pitch:base[b] + i * pitch + S] = w.view()
            assert np.array_equal(w.view(), cw[b, i])
    pool = torch.from_numpy(before).cuda()
    bids = [[pool[base[b] + i * pitch:base[b] + i * pitch + S] for i in range(total)] for b in range(nbid)]
    return bids, status, pool, want


def check_pool(pool, want):
    """Every shard equals the oracle's and every canary byte after every row is what it was."""
    got = pool.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail(f"{bad.size} bytes differ, first at {int(bad[0])}")


def test_ec12p4_reconstruct_and_verify_is_one_store_verify_launch(monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    t = mode_of("EC12P4")
    enc = ec_encoder(t)
    bids, status, pool, want = repair_case(t, 4097, 2, [3], scattered=False)
    capfd.readouterr()
    st = enc.ReconstructBatch(bids, [[3]] * 2, verify=True)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert status == [0, 0] and st == [0, 0]
    check_pool(pool, want)
    # 11 data rows and parity row 12 in, the rebuilt row stored and the other 3 parity rows compared:
    # 12 x 4 with the stored / compared split in one launch, which keeps the plain fixed-K kernel
    ins, rows = enc.repair_rows([3], [3, 13, 14, 15])
    assert ins == [0, 1, 2] + list(range(4, 13))
    exp = want_trace(12, 4, b"".join(rows), MR.STORE_VERIFY, 1, 4097, 2, "affine")
    assert traced(err) == exp and [(g["family"], g["mode"]) for g in exp] == [(MR.FIXED_K, "store-verify")], err


@pytest.mark.parametrize("scattered", [False, True], ids=["affine", "scattered"])
def test_c5_repair(scattered, monkeypatch, capfd):
    """EC16P20L2 with two data and two parity shards lost, 4 bids of 2 tiles: the bit-sliced repair
    (one affine launch, or the table launch for bids at unrelated addresses), rebuilt rows and the
    Verify status against the ec oracle."""
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    t = mode_of("EC16P20L2")
    enc = ec_encoder(t)
    bad = [0, 1, 16, 17]
    bids, status, pool, want = repair_case(t, 2048 * 2, 4, bad, scattered)
    capfd.readouterr()
    st = enc.ReconstructBatch(bids, [bad] * 4, verify=True)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert status == [0] * 4 and st == [0] * 4
    check_pool(pool, want)
    lines = [ln for ln in err.splitlines() if ln.startswith("cfsec: repair ")]
    assert lines and all(" nd=2 " in ln for ln in lines), err
    assert any(f" bs={'table' if scattered else 'affine'} " in ln for ln in lines), err
