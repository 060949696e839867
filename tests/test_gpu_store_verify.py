"""Every separately compiled kStoreVerify kernel against the C oracle, row by row.

A blobnode repair with Verify is one kStoreVerify launch (batch.cpp launch_group_run): the first nstore
rows of the product are stored, the others compared with the surviving parity.  The library ships one
such kernel per (k, m) of the fixed-K family (gf_fixed.hpp launch_k), one per (k, m) of the
lookup-product family (gf_lut_inst.hpp) and one per (rows per wave, waves per chunk) shape of the
runtime-k family (gf_kernels.hip launch_mode), and single instantiations have been wrong while every
other GPU test passed (tests/test_store_hazard.py).  For every (k, m) and every
nstore = 1 .. m - 1 this module runs a clean stripe and one stripe per compared row with one bit of
that row flipped, so a kernel that stores a wrong row, skips a compare or writes past a row fails here.

Entry point: ec.NewEncoder(ec.Config(CodeMode=Tactic(k, m, 0, 1, k, 0, 0), EnableVerify=False)) and
ReconstructBatch(bids, bad, verify=True) on shards carved from one device pool -- cfsec_ec_new takes any
valid tactic (tests/test_capi.py), and the call writes in place, so the canary bytes after every shard
are checked together with the shards.  One call per (k, m) carries the bids of every nstore; each bad
set is its own launch.  The 16 + 20 code with at most 4 data shards lost takes the 16x16-dyadic repair
kernel and its bit-sliced prefix instead of the product (launch_dy16_repair); its nstore = 1 .. 4 get
the same checks there, and nstore >= 5 lose at least 5 data shards so that fixed-K (16, 20) runs.

Reference: the C oracle's Reconstruct then Verify only, never another path of the library.  Everything
is bit-exact.  Before the GPU is touched the reference alone must give status 0 for every clean stripe
and ErrVerify for every corrupted one.

CFSEC_LUT=0 (read once per process) sends the lookup-product shapes to their fixed-K kernels, which no
other GPU test runs: test_sweep_in_child runs this module again in a child with the switch set.  For
those shapes the module also checks Encode, Verify (clean, a flipped last byte of the last parity, a
flipped first byte of the first data shard) and a Reconstruct of m shards (a general matrix).  In the
child every kStoreVerify launch and every such Reconstruct of these shapes is fixed-K; Encode and
Verify are fixed-K except where the encoding matrix has a dyadic-block form (k = 6 with m = 6, 8, 10,
12; (12, 8); k = 16 with m = 8, 12, 16), which plan_matvec gives to the dyadic kernel whatever the
switch says -- no public call reaches the fixed-K Store / Verify kernels with those matrices.  The last
test asserts that the launches traced are exactly the enumeration of tests/matvec_routes.py."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import matvec_routes as MR
from chubaofs_amd import _lib
from chubaofs_amd.codemode import Tactic
from oracle import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CHILD = os.environ.get("CFSEC_STORE_VERIFY_CHILD") == "1"
LUT = os.environ.get("CFSEC_LUT", "1")[:1] != "0"  # gf_kernels.hip env_switch("CFSEC_LUT", '0', true)

S = 8209  # two or four whole tiles of every family and a 17-byte ragged tail
PITCH = (S + 255) // 256 * 256 + 256  # at least 256 canary bytes after every shard
CANARY, JUNK = 0xA5, 0xEE
FLIP_AT = [0, 4095, 4096, 8191, 8192, S - 1]
FLIP_AT_BS = FLIP_AT + [2047, 2048]  # the bit-sliced repair's 2 KiB tile edge
BS_TILE = MR.BS_TILE
BS_REPAIR_MAX_ND = 2  # gf_launch.hpp kBsRepairMaxNd: missing data rows the bit-sliced repair takes

RUNTIME_M5 = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21, 24, 25, 32]
FIXED_CASES = [(k, m) for k, top in MR.FIXED_MAX_M.items() for m in range(2, top + 1)]
RUNTIME_CASES = [(5, m) for m in RUNTIME_M5] + [(3, 7), (18, 5), (32, 3)]
LOOKUP_CASES = [(k, m) for k, ms in MR.LOOKUP_M.items() for m in ms]

SEEN = set()         # (family, k, m, mode name) of every product launch traced
SEEN_SHAPES = set()  # (rows per wave, waves per chunk) of the runtime-k kStoreVerify launches
SEEN_REPAIR = set()  # missing data rows of the 16 + 20 repair launches


def sv_family(k, m):
    """The family a kStoreVerify launch of m rows over k inputs takes in this process."""
    if k in MR.FIXED_MAX_M and m <= MR.FIXED_MAX_M[k]:
        return MR.LOOKUP if LUT and m in MR.LOOKUP_M.get(k, ()) else MR.FIXED_K
    return MR.RUNTIME_K


def is_dy16_repair(k, m, nd):
    return (k, m) == (16, 20) and nd <= 4  # batch.cpp plan_dy16 (no extra rows: 16 nd + 117 < 320)


def bad_set(k, m, n, r):
    """n bad shards: at least one data shard and, where n >= 2, at least one parity shard."""
    if (k, m) == (16, 20):  # nd = 1, 1, 2, 3 for the repair kernel; then at least 5 for the product
        nd = max(1, n - 1) if n <= 4 else (5 if n == 5 else r.randint(5, min(k, n - 1)))
    else:
        nd = 1 if n == 1 else r.randint(1, min(k, n - 1))
    return sorted(r.sample(range(k), nd)) + sorted(r.sample(range(k, k + m), n - nd))


def reference_repair(k, m, shards, bad):
    """The reference's two calls on one stripe: Reconstruct, then Verify; (status, shards after)."""
    work = [s.copy() for s in shards]
    err, _ = O.reconstruct(k, m, work, [i not in bad for i in range(k + m)])
    if err:
        return err, work
    err, ok = O.verify(k, m, work)
    return (err if err else 0 if ok else _lib.ErrVerify.status), work


class Case:
    """The pool of one (k, m), nstore in ns: per nstore a clean stripe and one stripe per compared row
    with one flipped bit in it; the pool image before, the image the oracle leaves, its status per bid."""

    def __init__(self, k, m, ns):
        total = k + m
        self.k, self.m, self.total = k, m, total
        rng = np.random.default_rng(1000003 * k + 1009 * m)
        cw = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)] + [np.zeros(S, np.uint8) for _ in range(m)]
        assert O.encode(k, m, cw) == 0
        r = random.Random(7919 * k + m)
        self.groups = []  # (nstore, bad, compared rows, bids)
        self.bads, self.clean, stripes = [], [], []
        flip = k + m
        for n in ns:
            bad = bad_set(k, m, n, r)
            nd = sum(i < k for i in bad)
            present = [i for i in range(total) if i not in bad]
            assert nd >= 1 and (n < 2 or nd < n or (k, m, n) == (16, 20, 5)), (k, m, n, bad)
            compared = present[k:]  # the present parity shards that are no inputs
            assert len(compared) == m - n and all(i >= k for i in compared)
            self.groups.append((n, bad, compared, 1 + len(compared)))
            at = FLIP_AT_BS if is_dy16_repair(k, m, nd) else FLIP_AT
            for j in range(1 + len(compared)):
                src = [np.full(S, JUNK, np.uint8) if i in bad else cw[i].copy() for i in range(total)]
                if j:
                    src[compared[j - 1]][at[flip % len(at)]] ^= 1 << ((flip + flip // len(at)) % 8)
                    flip += 1
                stripes.append(src)
                self.bads.append(bad)
                self.clean.append(j == 0)
        self.nbid = len(stripes)
        self.before = np.full(256 + self.nbid * total * PITCH, CANARY, np.uint8)
        self.want = self.before.copy()
        self.status = []
        for b, src in enumerate(stripes):
            st, after = reference_repair(k, m, src, self.bads[b])
            self.status.append(st)
            for i in range(total):
                o = self.offset(b, i)
                self.before[o:o + S] = src[i]
                self.want[o:o + S] = after[i]
                # the reference rebuilds the bad shards and leaves every other one as it was
                assert np.array_equal(after[i], cw[i] if i in self.bads[b] else src[i]), (k, m, b, i)

    def offset(self, b, i):
        return 256 + (b * self.total + i) * PITCH

    def check_inputs(self):
        """The reference alone flags exactly the corrupted stripes."""
        for b in range(self.nbid):
            assert self.status[b] == (0 if self.clean[b] else _lib.ErrVerify.status), (self.k, self.m, b, self.bads[b])


def new_encoder(k, m):
    from chubaofs_amd import ec
    return ec.NewEncoder(ec.Config(CodeMode=Tactic(k, m, 0, 1, k, 0, 0), EnableVerify=False), device=0)


def fields(line):
    return dict(x.split("=") for x in line.split()[2:])


def want_lines(k, m, coef, mode, nstore, nst):
    steps = MR.expect_plan(k, m, coef, mode, nstore, S, nst, affine=nst > 1, lut=LUT)
    assert steps != "error"
    return [fields(MR.trace_line(s, nst > 1)) for s in steps]


def record(lines):
    for g in lines:
        SEEN.add((g["family"], int(g["k"]), int(g["m"]), g["mode"]))


def check_pool(pool, want, where):
    got = pool.cpu().numpy()
    if not np.array_equal(got, want):  # rebuilt shards, inputs, compared rows and every canary byte
        diff = np.flatnonzero(got != want)
        b, rest = divmod(int(diff[0]) - 256, where.total * PITCH)
        pytest.fail(f"{(where.k, where.m)}: {diff.size} bytes differ, first in bid {b} (bad {where.bads[b]}) "
                    f"shard {rest // PITCH} at byte {rest % PITCH}")


def sweep(k, m, ns, family, monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    case = Case(k, m, ns)
    case.check_inputs()  # before the GPU is touched
    enc = new_encoder(k, m)
    pool = torch.from_numpy(case.before).cuda()
    assert pool.data_ptr() % 256 == 0
    bids = [[pool[case.offset(b, i):case.offset(b, i) + S] for i in range(case.total)] for b in range(case.nbid)]
    capfd.readouterr()
    status = enc.ReconstructBatch(bids, case.bads, verify=True)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert status == case.status, [(b, case.bads[b], status[b], case.status[b]) for b in range(case.nbid)
                                   if status[b] != case.status[b]][:8]
    check_pool(pool, case.want, case)
    products = [fields(ln) for ln in err.splitlines() if ln.startswith("cfsec: matvec ")]
    repairs = [fields(ln) for ln in err.splitlines() if ln.startswith("cfsec: repair ")]
    want_products, want_repairs = [], []
    for n, bad, compared, nst in case.groups:
        nd = sum(i < k for i in bad)
        if is_dy16_repair(k, m, nd):
            net = nd <= BS_REPAIR_MAX_ND  # whole 2 KiB tiles bit-sliced, the dyadic repair kernel on the tail
            prefix = S // BS_TILE * BS_TILE if net else 0
            want_repairs.append(dict(bs="affine" if net else "none", nd=str(nd), e="0", s0="0", stripes=str(nst),
                                     prefix=str(prefix), tail=str(S - prefix), affine="1"))
            continue
        ins, rows = enc.repair_rows(bad, bad + compared)
        assert ins == [i for i in range(case.total) if i not in bad][:k]
        step = want_lines(k, m, b"".join(rows), MR.STORE_VERIFY, n, nst)
        assert [(g["family"], g["mode"], g["k"], g["m"]) for g in step] == [(family, "store-verify", str(k), str(m))]
        want_products += step
    assert products == want_products, err
    assert repairs == want_repairs, err
    record(products)
    SEEN_REPAIR.update(int(g["nd"]) for g in repairs)
    if family == MR.RUNTIME_K and products:
        SEEN_SHAPES.add(MR.runtime_shape(m))


# The largest cases, (16, 24) with 299 bids and (5, 32) with 527, take 0.45 s and 0.5 s on the MI355X
# machine, so no (k, m) is split over two cases.
@pytest.mark.parametrize("k,m", FIXED_CASES)
def test_a_sweep_fixed_k_and_lookup(k, m, monkeypatch, capfd):
    sweep(k, m, range(1, m), sv_family(k, m), monkeypatch, capfd)


@pytest.mark.parametrize("k,m", RUNTIME_CASES)
def test_a_sweep_runtime_k(k, m, monkeypatch, capfd):
    assert sv_family(k, m) == MR.RUNTIME_K
    sweep(k, m, range(1, m), MR.RUNTIME_K, monkeypatch, capfd)


# ------------------------------------------------ the lookup shapes in Store and Verify (fixed-K in the child)

def encode_family(k, m, coef):
    """Encode and Verify of a lookup shape: its dyadic-block kernel where the matrix has the form and
    the lookup kernel does not take it (k = 6 by default, every k under CFSEC_LUT=0)."""
    dy = MR.dyadic_form(coef, k, m)
    if LUT and not (k == 6 and dy):
        return MR.LOOKUP
    return MR.DYADIC if dy else MR.FIXED_K


@pytest.mark.parametrize("k,m", LOOKUP_CASES)
def test_a_lookup_shapes_encode_verify_reconstruct(k, m, monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    total = k + m
    rng = np.random.default_rng(64 * k + m)
    cw = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)] + [np.zeros(S, np.uint8) for _ in range(m)]
    assert O.encode(k, m, cw) == 0
    coef = O.encode_matrix_rows(k, total).tobytes()
    enc = new_encoder(k, m)
    image = np.full(256 + total * PITCH, CANARY, np.uint8)
    at = [256 + i * PITCH for i in range(total)]

    def run(shards, call):
        """call on a pool holding `shards`; (what it returned, the pool after, the launches traced)."""
        before = image.copy()
        for i in range(total):
            before[at[i]:at[i] + S] = shards[i]
        pool = torch.from_numpy(before).cuda()
        capfd.readouterr()
        ret = call([pool[at[i]:at[i] + S] for i in range(total)])
        torch.cuda.synchronize()
        lines = [fields(ln) for ln in capfd.readouterr().err.splitlines() if ln.startswith("cfsec: matvec ")]
        record(lines)
        return ret, pool.cpu().numpy(), before, lines

    full = image.copy()  # the image of the whole codeword
    for i in range(total):
        full[at[i]:at[i] + S] = cw[i]
    # Encode over junk parity
    _, got, _, lines = run(cw[:k] + [np.full(S, JUNK, np.uint8)] * m, enc.Encode)
    assert np.array_equal(got, full)
    assert lines == want_lines(k, m, coef, MR.STORE, 0, 1) and lines[0]["family"] == encode_family(k, m, coef), lines
    # Verify: clean, the last byte of the last parity, the first byte of the first data shard
    for shard, byte in ((None, 0), (total - 1, S - 1), (0, 0)):
        src = [x.copy() for x in cw]
        if shard is not None:
            src[shard][byte] ^= 0x10
        assert O.verify(k, m, src) == (0, shard is None)
        ok, got, before, lines = run(src, enc.Verify)
        assert ok == (shard is None), (shard, byte)
        assert np.array_equal(got, before)  # a Verify writes nothing
        assert lines == want_lines(k, m, coef, MR.VERIFY, 0, 1) and lines[0]["family"] == encode_family(k, m, coef), lines
    # Reconstruct of m shards, a data shard and a parity shard among them: a general m x k matrix
    r = random.Random(100 * k + m)
    nd = r.randint(1, min(k, m - 1))
    bad = sorted(r.sample(range(k), nd)) + sorted(r.sample(range(k, total), m - nd))
    src = [np.full(S, JUNK, np.uint8) if i in bad else cw[i].copy() for i in range(total)]
    work = [x.copy() for x in src]
    assert O.reconstruct(k, m, work, [i not in bad for i in range(total)])[0] == 0
    assert all(np.array_equal(work[i], cw[i]) for i in range(total))
    _, got, _, lines = run(src, lambda sh: enc.Reconstruct(sh, bad))
    assert np.array_equal(got, full)
    _, rows = enc.repair_rows(bad, bad)
    assert lines == want_lines(k, m, b"".join(rows), MR.STORE, 0, 1), lines
    assert [(g["family"], g["mode"]) for g in lines] == [(sv_family(k, m), "store")], lines


# ------------------------------------------------------------------ the module again under CFSEC_LUT=0

# Measured on the MI355X: this module in-process (the child excluded, 142 tests) 9.9 s of wall time for
# the whole python process (8.3 s inside pytest), `import torch` 1.7 s; the child gets three times the
# first plus the second.
MODULE_SECONDS = 9.9
IMPORT_SECONDS = 1.7
CHILD_TIMEOUT = 3 * MODULE_SECONDS + IMPORT_SECONDS


@pytest.mark.skipif(CHILD, reason="the child process itself")
@pytest.mark.parametrize("setting", ["CFSEC_LUT=0"])
def test_sweep_in_child(setting):
    """This module again with the lookup-product kernels switched off, one child at a time.  A child
    that ends by a signal, an abort or its time limit ends the session: nothing more starts on the GPU
    after a fault."""
    name, value = setting.split("=")
    env = dict(os.environ, CFSEC_STORE_VERIFY_CHILD="1")
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
    assert " 1 skipped" in r.stdout, r.stdout[-2000:]  # this test alone: the coverage test ran


# ------------------------------------------------------------------ coverage closes

def test_z_every_store_verify_instantiation_was_traced(request):
    """The launches the tests above traced are the enumeration of tests/matvec_routes.py: a kernel added
    later without a case here fails this test."""
    mine = {i.name for i in request.session.items if i.name.startswith("test_a_")}
    every = {f"{fn}[{k}-{m}]" for fn, cases in (("test_a_sweep_fixed_k_and_lookup", FIXED_CASES),
                                                ("test_a_sweep_runtime_k", RUNTIME_CASES),
                                                ("test_a_lookup_shapes_encode_verify_reconstruct", LOOKUP_CASES))
             for k, m in cases}
    if not every <= mine:
        pytest.skip("only part of the module was selected")
    in_lookup = lambda k, m: m in MR.LOOKUP_M.get(k, ())  # noqa: E731
    fixed = {(k, m) for k, top in MR.FIXED_MAX_M.items() for m in range(2, top + 1)}
    assert set(FIXED_CASES) == fixed and set(LOOKUP_CASES) <= fixed
    want = {((MR.LOOKUP if LUT and in_lookup(k, m) else MR.FIXED_K), k, m) for k, m in fixed}
    want |= {(MR.RUNTIME_K, k, m) for k, m in RUNTIME_CASES}
    got = {(f, k, m) for f, k, m, mode in SEEN if mode == "store-verify"}
    assert got == want, (sorted(want - got), sorted(got - want))
    assert sum(f == MR.LOOKUP for f, _, _ in got) == (33 if LUT else 0)
    assert sum(f == MR.FIXED_K for f, _, _ in got) == (86 - 33 if LUT else 86)
    assert SEEN_SHAPES == {s for s in MR.RUNTIME_SHAPES if s[0] * s[1] >= 2}, SEEN_SHAPES
    assert SEEN_REPAIR == {1, 2, 3}  # the 16 + 20 repair kernel, with and without its bit-sliced prefix
    # Store and Verify of the lookup shapes: the lookup kernels, or under CFSEC_LUT=0 their fixed-K ones
    for k, m in LOOKUP_CASES:
        enc = encode_family(k, m, O.encode_matrix_rows(k, k + m).tobytes())
        assert (sv_family(k, m), k, m, "store") in SEEN, (k, m)  # the Reconstruct's general matrix
        assert {(enc, k, m, "store"), (enc, k, m, "verify")} <= SEEN, (k, m, enc)
    others = {(f, k, m, mode) for f, k, m, mode in SEEN if mode != "store-verify"}
    assert {f for f, _, _, _ in others} <= ({MR.LOOKUP, MR.DYADIC} if LUT else {MR.FIXED_K, MR.DYADIC}), others
    if not LUT:
        dyadic = {(k, m) for f, k, m, _ in others if f == MR.DYADIC}
        assert dyadic == {(6, 6), (6, 8), (6, 10), (6, 12), (12, 8), (16, 8), (16, 12), (16, 16)}, dyadic
