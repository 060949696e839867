"""EncodeIdx, Update and ReconstructSome at the C ABI, without a device: every error return in the
reference's precedence (KRS/reedsolomon.go:631-647, 672-700, 1407-1444), the no-op returns, the new
status code, and the numpy reference helper (tests/rs_seam_ref.py) checked against the oracle.

Every call below returns before any device work, so the file passes on a machine without a GPU.
"""
import ctypes

import numpy as np
import pytest

import rs_seam_ref as R
from chubaofs_amd import _lib, reedsolomon
from oracle import oracle as O

K, M, S = 6, 3, 8


def ones(n=S):
    return np.ones(n, np.uint8)


def empty():
    return np.zeros(0, np.uint8)


@pytest.fixture(scope="module")
def enc():
    return reedsolomon.New(K, M)


def test_status_name_and_version():
    L = _lib.lib()
    assert L.cfsec_status_name(17) == b"ErrInvalidInput"
    assert _lib.ErrInvalidInput.status == 17 and _lib._BY_CODE[17] is _lib.ErrInvalidInput
    assert L.cfsec_version() == b"cfsec 0.5.1 (gfx950)"


# ---------------------------------------------------------------- EncodeIdx

def test_encode_idx_errors_in_reference_order(enc):
    par = [ones() for _ in range(M)]
    with pytest.raises(_lib.ErrTooFewShards):
        enc.EncodeIdx(ones(), 0, par[:M - 1])
    with pytest.raises(_lib.ErrTooFewShards):  # the parity count comes before idx
        enc.EncodeIdx(ones(), -1, par + [ones()])
    for idx in (-1, K, K + M):
        with pytest.raises(_lib.ErrInvShardNum):
            enc.EncodeIdx(ones(), idx, par)
    with pytest.raises(_lib.ErrInvShardNum):  # idx comes before checkShards(parity)
        enc.EncodeIdx(ones(), K, [empty()] * M)
    with pytest.raises(_lib.ErrShardNoData):
        enc.EncodeIdx(ones(), 0, [empty()] * M)
    with pytest.raises(_lib.ErrShardSize):  # nilok = false: an absent parity shard is a size error
        enc.EncodeIdx(ones(), 0, [ones(), empty(), ones()])
    with pytest.raises(_lib.ErrShardSize):
        enc.EncodeIdx(ones(), 0, [ones(), ones(S + 1), ones()])
    with pytest.raises(_lib.ErrShardSize):  # parity[0] against the data shard, last
        enc.EncodeIdx(ones(S - 1), 0, par)
    with pytest.raises(_lib.ErrShardSize):
        enc.EncodeIdx(empty(), 0, par)
    assert all((p == 1).all() for p in par)


def test_encode_idx_without_parity_is_a_noop():
    e = reedsolomon.New(4, 0)
    e.EncodeIdx(ones(), 0, [])
    e.EncodeIdx(ones(), 99, [])  # no parity shards: OK before idx is looked at
    with pytest.raises(_lib.ErrTooFewShards):
        e.EncodeIdx(ones(), 0, [ones()])


# ---------------------------------------------------------------- Update

def stripe():
    return [ones() for _ in range(K + M)]


def news(*present, size=S):
    return [ones(size) if i in present else None for i in range(K)]


def test_update_errors_in_reference_order(enc):
    with pytest.raises(_lib.ErrTooFewShards):
        enc.Update(stripe()[:-1], news(0))
    with pytest.raises(_lib.ErrTooFewShards):
        enc.Update(stripe(), news(0) + [None])
    with pytest.raises(_lib.ErrTooFewShards):  # the shard count comes before either checkShards
        enc.Update([empty()] * (K + M - 1), [None] * K)
    with pytest.raises(_lib.ErrShardNoData):
        enc.Update([empty()] * (K + M), news(0))
    sh = stripe()
    sh[4] = ones(S + 1)
    with pytest.raises(_lib.ErrShardSize):
        enc.Update(sh, news(0))
    with pytest.raises(_lib.ErrShardSize):  # checkShards(shards) comes before checkShards(new_data)
        enc.Update(sh, [None] * K)
    with pytest.raises(_lib.ErrShardNoData):  # an all-empty new_data, as in the reference
        enc.Update(stripe(), [None] * K)
    with pytest.raises(_lib.ErrShardNoData):
        enc.Update(stripe(), [empty()] * K)
    nw = news(0, 1)
    nw[1] = ones(S - 2)
    with pytest.raises(_lib.ErrShardSize):  # new_data among themselves
        enc.Update(stripe(), nw)
    sh = stripe()
    sh[K + 1] = empty()
    with pytest.raises(_lib.ErrShardNoData):  # both checkShards come before the presence checks
        enc.Update(sh, [None] * K)
    with pytest.raises(_lib.ErrInvalidInput):  # an absent parity shard
        enc.Update(sh, news(0))
    sh = stripe()
    sh[2] = empty()
    with pytest.raises(_lib.ErrInvalidInput):  # new data for an absent old shard
        enc.Update(sh, news(2))
    sh[K] = empty()
    with pytest.raises(_lib.ErrInvalidInput):
        enc.Update(sh, news(2, size=S + 3))  # the presence checks come before the cross size check
    with pytest.raises(_lib.ErrShardSize):  # the C seam's own check: new_data's size against the stripe's
        enc.Update(stripe(), news(0, 3, size=S + 3))


def test_update_without_parity_touches_nothing():
    e = reedsolomon.New(4, 0)
    sh = [ones() for _ in range(4)]
    e.Update(sh, [np.full(S, 7, np.uint8), None, None, None])
    assert all((s == 1).all() for s in sh)  # KRS/reedsolomon.go:713-715: no outputs, no delta formed


def test_update_batch_argument_errors(enc):
    ptrs, new = [0] * (K + M), [0, 0]
    for cols in ([1, 1], [2, 1], [-1, 0], [0, K]):
        with pytest.raises(_lib.ErrInvalidArg):
            enc.update_batch(ptrs, new, cols, 16, 1)
    with pytest.raises(_lib.ErrInvalidArg):
        enc.update_batch(ptrs, new, [0, 1], 16, -1)


# ---------------------------------------------------------------- ReconstructSome

def test_reconstruct_some_errors_and_noops(enc):
    req = [True] * K
    with pytest.raises(_lib.ErrTooFewShards):
        enc.ReconstructSome(stripe()[:-1], req)
    with pytest.raises(_lib.ErrTooFewShards):  # fewer mask entries than data shards
        enc.ReconstructSome(stripe(), req[:-1])
    with pytest.raises(_lib.ErrTooFewShards):  # the counts come before checkShards
        enc.ReconstructSome([empty()] * (K + M), req[:-1])
    with pytest.raises(_lib.ErrShardNoData):
        enc.ReconstructSome([empty()] * (K + M), req)
    sh = stripe()
    sh[1] = ones(S - 1)
    with pytest.raises(_lib.ErrShardSize):
        enc.ReconstructSome(sh, req)
    # the early OK returns (:1438-1441): nothing missing; no data shard missing; nothing required missing
    enc.ReconstructSome(stripe(), req)
    sh = stripe()
    sh[K] = sh[K + 2] = None
    enc.ReconstructSome(sh, req + [True] * M)  # even with the missing parity "required": dataOnly comes first
    assert sh[K] is None and sh[K + 2] is None
    sh = stripe()
    sh[0], sh[3] = None, empty()
    enc.ReconstructSome(sh, [False, True, True, False, True, True])
    assert sh[0] is None and sh[3].size == 0
    enc.ReconstructSome(sh, [False] * K + [True] * M)  # mask entries at present parity shards count for nothing
    # fewer than k present, something required missing
    sh = stripe()
    for i in (0, 1, 2, K):
        sh[i] = None
    with pytest.raises(_lib.ErrTooFewShards):
        enc.ReconstructSome(sh, req)
    enc.ReconstructSome(sh, [False, False, False, True, True, True])  # ... but nothing required: OK first


def test_required_missing_parity_defeats_the_early_ok(enc):
    """required[i] at a missing parity index counts towards missingRequired (:1427-1429), so the call
    goes past the early OK although no required data shard is missing -- here into numberPresent < k."""
    sh = stripe()
    for i in (0, 1, 2, K):
        sh[i] = None
    none = [False] * K
    enc.ReconstructSome(sh, none + [False] * M)
    enc.ReconstructSome(sh, none)  # entries from nrequired on count as false
    with pytest.raises(_lib.ErrTooFewShards):
        enc.ReconstructSome(sh, none + [True])


def test_reconstruct_some_stripes_status_per_stripe(enc):
    few = stripe()
    for i in (0, 1, 2, K):
        few[i] = None
    bad = stripe()
    bad[1] = ones(S - 1)
    unreq = stripe()
    unreq[0] = None
    stripes = [stripe(), few, bad, [empty()] * (K + M), unreq, list(few)]
    masks = [[True] * K, [True] * K, [True] * K, [True] * K, [False] + [True] * (K - 1), [False] * 3 + [True] * 3]
    got = enc.ReconstructSomeStripes(stripes, masks)
    assert got == [0, _lib.ErrTooFewShards.status, _lib.ErrShardSize.status, _lib.ErrShardNoData.status, 0, 0]
    assert unreq[0] is None
    assert enc.ReconstructSomeStripes([], []) == []


# ---------------------------------------------------------------- the reference helper against the oracle

@pytest.mark.parametrize("k,m", [(12, 4), (6, 6), (3, 3), (8, 1), (16, 20), (40, 3)])
def test_ref_encode_idx_steps_equal_encode(k, m):
    rng = np.random.default_rng(k * 100 + m)
    size = 257
    want = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(k)] + [np.zeros(size, np.uint8) for _ in range(m)]
    assert O.encode(k, m, want) == 0
    par = [np.zeros(size, np.uint8) for _ in range(m)]
    for idx in rng.permutation(k):
        R.encode_idx(k, m, want[idx], int(idx), par)
    assert all(np.array_equal(par[r], want[k + r]) for r in range(m))


@pytest.mark.parametrize("k,m,cols", [(12, 4, [0]), (12, 4, [3, 4]), (6, 6, list(range(6))), (6, 33, [5]), (40, 3, [0, 39])])
def test_ref_update_leaves_a_stripe_that_verifies(k, m, cols):
    rng = np.random.default_rng(k * 1000 + m + len(cols))
    size = 131
    sh = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(k)] + [np.zeros(size, np.uint8) for _ in range(m)]
    assert O.encode(k, m, sh) == 0
    old = [s.copy() for s in sh]
    new = [rng.integers(0, 256, size, dtype=np.uint8) if c in cols else None for c in range(k)]
    R.update(k, m, sh, new)
    for c in range(k):
        if c in cols:
            assert np.array_equal(sh[c], old[c] ^ new[c])  # the old shard holds the delta
            sh[c] = new[c].copy()
        else:
            assert np.array_equal(sh[c], old[c])
    err, ok = O.verify(k, m, sh)
    assert err == 0 and ok


def test_ref_reconstruct_some_writes_only_the_required_rows():
    k, m, size = 6, 3, 77
    rng = np.random.default_rng(5)
    want = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(k)] + [np.zeros(size, np.uint8) for _ in range(m)]
    assert O.encode(k, m, want) == 0
    sh = [w.copy() for w in want]
    present = [i not in (1, 4, k + 1) for i in range(k + m)]
    for i in (1, 4, k + 1):
        sh[i][:] = 0xA5
    assert R.reconstruct_some(k, m, sh, present, [False, False, False, False, True, False]) == [4]
    assert np.array_equal(sh[4], want[4]) and (sh[1] == 0xA5).all() and (sh[k + 1] == 0xA5).all()


def test_signatures_cover_the_new_entry_points():
    L = _lib.lib()
    for name in ("cfsec_rs_encode_idx", "cfsec_rs_update", "cfsec_rs_reconstruct_some",
                 "cfsec_rs_reconstruct_some_stripes", "cfsec_rs_update_batch"):
        assert name in _lib.SIGNATURES and isinstance(getattr(L, name), ctypes._CFuncPtr)
