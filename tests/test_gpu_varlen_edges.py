"""Batches of mixed stripe lengths, and batches split over launches, through every kernel body of the
plain product and of the 16 + 20 repair, bit-exact against the oracle.

The cases, their lengths and their reference images are tests/varlen_cases.py's (pinned on the CPU by
tests/test_varlen_geometry.py): one plan per case, three stripes more than one launch holds, so every
case is at least two launches and the second one carries slen[s] = lens[s0 + s] and flags + s0.  The
entry points are the batch calls real traffic takes -- ReedSolomon.EncodeStripes / VerifyStripes,
ec.EncodeBatch (EnableVerify off) for the fused LRC encodes, ec.ReconstructBatch with and without Verify
on Tactic(k, m, 0, 1, k, 0, 0) or the LRC mode -- one call per case.

Each case is one device pool: every shard a slice at pitch round_up(longest, 256) + 256 whatever its own
length, so a store or compare that takes the run's length, or a neighbour's, lands in that shard's own
slack and never outside the pool; the slack holds seeded random bytes, so a Verify that reads past a
stripe's end meets a non-codeword.  Asserted after the call, bit-exactly: the whole pool image is the
oracle's (stored shards, untouched inputs and compared rows, every slack byte), the per-stripe status
is the oracle's (one corrupted stripe per launch where rows are compared, every other one clean), the
traced launches are the restated plan, and there are at least two of them.  The reference is the C
oracle's Encode / Reconstruct / Verify and ECOracle for the LRC modes, never another path of the library.
The last test fails when a family x mode of the table was not seen in a trace.

Measured on the MI355X: the module's 42 tests take 2.6 s of wall time inside pytest, the slowest
(store-dyadic4-12x4, the first, which opens the device) 0.19 s, every other one at most 0.08 s.  A case
whose capacity the 32 length slots bind (store-runtime-5x2-1wave, 35 stripes) and one bound by the 288
pointer slots (store-dyadic16-16x20, 288 / 36 = 8, 11 stripes) trace
  cfsec: matvec family=runtime-k bs=none mode=store k=5 m=2 r0=0 c0=0 stripes=32 prefix=0 tail=8192 affine=0
  cfsec: matvec family=runtime-k bs=none mode=store k=5 m=2 r0=0 c0=0 stripes=3 prefix=0 tail=8209 affine=0
  cfsec: matvec family=dyadic-16 bs=none mode=store k=16 m=20 r0=0 c0=0 stripes=8 prefix=0 tail=4096 affine=0
  cfsec: matvec family=dyadic-16 bs=none mode=store k=16 m=20 r0=0 c0=0 stripes=3 prefix=0 tail=4113 affine=0
Mutants of the library, built apart and never committed, against this module (cases failing; the closing
test fails with each): dispatch_matvec copying lens[s] for lens[s0 + s]: all 32 product cases with
per-stripe lengths; dispatch_matvec passing flags without + s0: all 15 product cases that compare rows,
the 3 uniform ones among them; both slips in dispatch_repair: the 6 repair cases; matvec_dy taking a.len for
its stripe's length: the 5 dyadic cases with per-stripe lengths; repair_dy16 doing so: the 6 repair cases;
the runtime-k body reading stripe_len(a, 0): its 9 cases.  The suite without this module passes whole (1500
tests) on the flags mutant; the other mutants were not run against it, since outside these pools their
wrong lengths are not confined to memory the tests own.
"""
import numpy as np
import pytest

import matvec_routes as MR
import varlen_cases as V
from chubaofs_amd import _lib
from chubaofs_amd import codemode as cm
from chubaofs_amd.codemode import Tactic

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEEN = set()  # (family, mode name) of every launch traced


def tactic(c):
    if c.lrc is None:
        return Tactic(c.k, c.m, 0, 1, c.k, 0, 0)
    (t,) = [t for t in map(cm.GetTactic, cm.GetAllCodeModes()) if (t.N, t.M, t.L, t.AZCount) == c.lrc]
    return t


def call(c, stripes):
    """The case's one batch call; the status per stripe."""
    if c.api in ("encode", "verify"):
        from chubaofs_amd import reedsolomon
        enc = reedsolomon.New(c.k, c.m)
        return enc.EncodeStripes(stripes) if c.api == "encode" else enc.VerifyStripes(stripes)
    from chubaofs_amd import ec
    enc = ec.NewEncoder(ec.Config(CodeMode=tactic(c), EnableVerify=False), device=0)
    if c.api == "lrc-encode":
        return enc.EncodeBatch(stripes)
    return enc.ReconstructBatch(stripes, [list(c.bad)] * len(stripes), verify=c.verify)


def where(p, at):
    s, rest = divmod(at - 256, p.total * p.pitch)
    s = p.slot.index(s) if s in p.slot else -1
    return f"stripe {s} (length {p.lens[s] if s >= 0 else '-'}) shard {rest // p.pitch} byte {rest % p.pitch}"


@pytest.mark.parametrize("c", V.CASES, ids=lambda c: c.name)
def test_a_case(c, monkeypatch, capfd):
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    assert _lib.ErrVerify.status == V.ERR_VERIFY
    p = V.pool(c)
    p.check_reference()  # before the GPU is touched
    dev = torch.from_numpy(p.before.copy()).cuda()
    assert dev.data_ptr() % 256 == 0
    stripes = [[dev[p.offset(s, i):p.offset(s, i) + n] for i in range(p.total)] for s, n in enumerate(p.lens)]
    capfd.readouterr()
    status = call(c, stripes)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    got = dev.cpu().numpy()
    trace = V.parse_trace(err)
    print(c.name, *[ln for ln in err.splitlines() if ln.startswith("cfsec: ")], sep="\n")
    assert status == p.status, [(s, p.lens[s], status[s], p.status[s]) for s in range(len(status)) if status[s] != p.status[s]]
    if not np.array_equal(got, p.want):
        diff = np.flatnonzero(got != p.want)
        pytest.fail(f"{c.name}: {diff.size} bytes differ, first at {where(p, int(diff[0]))}, last at {where(p, int(diff[-1]))}")
    assert trace == V.expected_trace(c), err
    assert len(trace) >= 2
    for g in trace:
        SEEN.add((V.REPAIR, "store-verify") if g["kind"] == "repair" else (g["family"], g["mode"]))


def test_z_every_family_and_mode_was_traced(request):
    """A family x mode added to the table, or a kernel the table names, that no case launched fails here."""
    mine = {i.name for i in request.session.items if i.name.startswith("test_a_case[")}
    if not {f"test_a_case[{c.name}]" for c in V.CASES} <= mine:
        pytest.skip("only part of the module was selected")
    want = {(c.family, MR.MODE_NAMES[c.mode]) for c in V.CASES}
    assert len(want) == 15
    assert SEEN == want, (sorted(want - SEEN), sorted(SEEN - want))
