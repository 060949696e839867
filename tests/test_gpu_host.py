"""Host-memory calls (CFSEC_MEM_HOST, what the cgo shim uses) through the chunked two-stream
pipeline: shards larger than one chunk (1 MiB per row), pageable and pinned (cfsec_host_alloc)
buffers, shards carved from one buffer at stride S (ec.Buffer, common/ec/buf.go:83-84: the 2-D
copy path) and separate buffers (per-row copies).  Bytes must match the oracle exactly."""
import numpy as np
import pytest

from chubaofs_amd import _lib
from oracle import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def rs():
    from chubaofs_amd import reedsolomon
    return reedsolomon


def alloc(n, pinned):
    return _lib.pinned_empty(n) if pinned else np.zeros(n, np.uint8)


def make(k, m, S, pinned, contiguous, seed):
    r = np.random.default_rng(seed)
    if contiguous:
        buf = alloc((k + m) * S, pinned)
        buf[:k * S] = r.integers(0, 256, k * S, dtype=np.uint8)
        buf[k * S:] = 0
        return [buf[i * S:(i + 1) * S] for i in range(k + m)]
    out = []
    for i in range(k + m):
        a = alloc(S, pinned)
        a[:] = r.integers(0, 256, S, dtype=np.uint8) if i < k else 0
        out.append(a)
    return out


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("contiguous", [False, True])
@pytest.mark.parametrize("k,m,S", [(12, 4, 3 * (1 << 20) + 12345), (6, 6, (1 << 20) + 1), (16, 20, 2 * (1 << 20) + 256)])
def test_host_pipeline_encode_verify_reconstruct(pinned, contiguous, k, m, S):
    sh = make(k, m, S, pinned, contiguous, seed=S + k)
    want = [s.copy() for s in sh]
    assert O.encode(k, m, want) == 0
    enc = rs().New(k, m)
    enc.Encode(sh)
    for i in range(k + m):
        assert np.array_equal(sh[i], want[i]), i
    assert enc.Verify(sh)
    sh[k + m - 1][S - 1] ^= 1  # last byte of the last chunk
    assert not enc.Verify(sh)
    sh[k + m - 1][S - 1] ^= 1
    pos = min(S - 1, (1 << 20) + 7)  # second chunk of a data row
    sh[0][pos] ^= 0x80
    assert not enc.Verify(sh)
    sh[0][pos] ^= 0x80
    erased = list(range(min(m, 4)))
    work = [s[:0] if i in erased else s for i, s in enumerate(sh)]  # missing: len 0
    enc.Reconstruct(work)
    assert all(len(w) == S for w in work)
    for i in range(k + m):
        assert np.array_equal(work[i], want[i]), i
    # ec.Encoder style: the bad shards keep their (possibly pinned) buffers, rebuilt in place
    from chubaofs_amd import ec, codemode as cm
    if (k, m) == (12, 4):
        e = ec.NewEncoder(ec.Config(CodeMode=cm.GetTactic(cm.EC12P4), EnableVerify=True))
        for i in erased:
            sh[i][:] = 0
        e.Reconstruct(sh, erased)
        for i in range(k + m):
            assert np.array_equal(sh[i], want[i]), i


def test_pinned_alloc_roundtrip():
    a = _lib.pinned_empty(1 << 20)
    a[:] = 7
    assert int(a.sum()) == 7 << 20
    assert _lib.pinned_empty(0).size == 0


@pytest.mark.parametrize("k,m", [(12, 4), (6, 6)])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_small_pageable_staging_boundary(k, m, delta):
    """Pageable host calls moving at most 1 MiB (rows x S) are copied into page-locked staging on the
    CPU and coded there (round 6: a degraded range read's segments, ~130 -> ~20 us); one byte more per
    row takes the chunked pipeline.  Encode, Verify (a flipped byte caught), ReconstructData and
    Reconstruct at both sides of the boundary, bytes equal to the oracle."""
    S = (1 << 20) // (k + m) + delta
    sh = make(k, m, S, False, False, seed=S * 3 + k)
    want = [s.copy() for s in sh]
    assert O.encode(k, m, want) == 0
    enc = rs().New(k, m)
    enc.Encode(sh)
    for i in range(k + m):
        assert np.array_equal(sh[i], want[i]), i
    assert enc.Verify(sh)
    sh[k][S // 2] ^= 0x10
    assert not enc.Verify(sh)
    sh[k][S // 2] ^= 0x10
    work = [s[:0] if i in (0, 1) else s.copy() for i, s in enumerate(sh)]
    enc.ReconstructData(work)
    assert np.array_equal(work[0], want[0]) and np.array_equal(work[1], want[1])
    work = [s[:0] if i in (1, k) else s.copy() for i, s in enumerate(sh)]
    enc.Reconstruct(work)
    for i in range(k + m):
        assert np.array_equal(work[i], want[i]), i


def make_mixed(k, m, S, pinned_rows, seed):
    """Separate buffers per shard: page-locked for the shard indices in pinned_rows, pageable for the rest."""
    r = np.random.default_rng(seed)
    out = []
    for i in range(k + m):
        a = alloc(S, i in pinned_rows)
        a[:] = r.integers(0, 256, S, dtype=np.uint8) if i < k else 0
        out.append(a)
    return out


@pytest.fixture(scope="module")
def wide_codewords():
    """The oracle's 40 + 3 codewords, computed once per size and never changed."""
    k, m, out = 40, 3, {}
    for S in (1000, 4097):
        r = np.random.default_rng(S)
        want = [r.integers(0, 256, S, dtype=np.uint8) for _ in range(k)] + [np.zeros(S, np.uint8) for _ in range(m)]
        assert O.encode(k, m, want) == 0
        for w in want:
            w.setflags(write=False)
        out[S] = want
    return out


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("S", [1000, 4097])
def test_wide_host_verify_and_encode(wide_codewords, pinned, S):
    """k = 40: Verify of more inputs than one launch carries, two launches (store into staging, compare).
    Page-locked rows are coded in place (kPinnedInPlace); pageable rows go whole through the workspace
    (kStagedWhole), the one way through RSEngine::run that only this test takes.  Encode of the same
    rows (one launch) takes the small stage or runs in place."""
    k, m = 40, 3
    want = wide_codewords[S]
    sh = [alloc(S, pinned) for _ in range(k + m)]
    for i in range(k):
        sh[i][:] = want[i]
    for i in range(k, k + m):
        sh[i][:] = 0
    enc = rs().New(k, m)
    enc.Encode(sh)
    for i in range(k + m):
        assert np.array_equal(sh[i], want[i]), i
    assert enc.Verify(sh)
    sh[k + m - 1][S - 1] ^= 1
    assert not enc.Verify(sh)
    sh[k + m - 1][S - 1] ^= 1
    sh[39][S // 3] ^= 0x40
    assert not enc.Verify(sh)
    assert O.verify(k, m, [s.copy() for s in sh]) == (0, False)
    sh[39][S // 3] ^= 0x40
    assert enc.Verify(sh)
    assert O.verify(k, m, [s.copy() for s in sh]) == (0, True)


@pytest.mark.parametrize("pinned_rows", [range(0, 6), range(6, 12)], ids=["data_pinned", "parity_pinned"])
@pytest.mark.parametrize("delta", [-1, 1], ids=["small_stage", "pipeline"])
def test_mixed_pinned_and_pageable_rows(pinned_rows, delta):
    """A stripe whose rows are part page-locked, part pageable is not coded in place: one pageable row
    sends the call to the small stage (at most 1 MiB moved) or the pipeline (more).  EC6P6 at both
    sides of that boundary: Encode, Verify (clean, one flipped byte caught), Reconstruct of {1, 6};
    every shard's bytes equal the oracle's."""
    k, m = 6, 6
    S = (1 << 20) // (k + m) + delta
    sh = make_mixed(k, m, S, pinned_rows, seed=S + pinned_rows[0])
    want = [s.copy() for s in sh]
    assert O.encode(k, m, want) == 0
    enc = rs().New(k, m)
    enc.Encode(sh)
    for i in range(k + m):
        assert np.array_equal(sh[i], want[i]), i
    assert enc.Verify(sh)
    for i, pos in ((2, S - 1), (k + 1, S // 2)):  # a data row, a parity row: one of each kind of memory
        sh[i][pos] ^= 0x04
        assert not enc.Verify(sh), i
        sh[i][pos] ^= 0x04
    assert enc.Verify(sh)
    work = [s[:0] if i in (1, 6) else s for i, s in enumerate(sh)]
    enc.Reconstruct(work)
    assert all(len(w) == S for w in work)
    for i in range(k + m):
        assert np.array_equal(work[i], want[i]), i
    # the surviving rows were inputs only: unchanged
    for i in range(k + m):
        assert np.array_equal(sh[i], want[i]), i


@pytest.mark.parametrize("delta", [-1, 1], ids=["small", "pipeline_size"])
def test_no_parity_rows_host_encode_and_verify(delta):
    """New(k, 0): a call with no output rows is done before any path is chosen.  Pageable rows at both
    sides of the 1 MiB boundary: Encode returns and leaves the data as it was, Verify is true."""
    k = 6
    S = (1 << 20) // k + delta
    r = np.random.default_rng(S)
    sh = [r.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
    want = [s.copy() for s in sh]
    assert O.encode(k, 0, want) == 0 and O.verify(k, 0, want) == (0, True)
    enc = rs().New(k, 0)
    enc.Encode(sh)
    assert enc.Verify(sh)
    for i in range(k):
        assert np.array_equal(sh[i], want[i]), i
