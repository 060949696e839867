"""cfsec_ec_reconstruct_data_batch / cfsec_rs_reconstruct_data_stripes without a device: the argument
checks of the call itself, and the per-item statuses that are decided before any device work -- each
equal to what the single ReconstructData call returns for the same item.  No compute call runs here."""
import ctypes

import numpy as np
import pytest

from chubaofs_amd import _lib, codemode as cm, ec, reedsolomon

OK = 0
INVALID_ARG = _lib.ErrInvalidArg.status


def shard_array(items):
    """items: lists of numpy arrays (None / empty: missing, no capacity) -> one cfsec_shard array."""
    flat = [s for it in items for s in it]
    arr = (_lib.Shard * max(len(flat), 1))()
    for i, s in enumerate(flat):
        arr[i] = _lib.Shard(None, 0, 0) if s is None or s.size == 0 else _lib.Shard(s.ctypes.data, s.size, s.size)
    return arr


def ints(v):
    return (ctypes.c_int * max(len(v), 1))(*v)


def batch(enc, items, n, bad, nitems=None):
    flat = [i for b in bad for i in b]
    off = [0]
    for b in bad:
        off.append(off[-1] + len(b))
    status = (ctypes.c_int * max(len(items), 1))(*([-7] * max(len(items), 1)))
    rc = enc._L.cfsec_ec_reconstruct_data_batch(enc._h, shard_array(items), n, len(items) if nitems is None else nitems,
                                                ints(flat), ints(off), _lib.MEM_HOST, status)
    return rc, [int(status[i]) for i in range(len(items))]


def single(enc, item, n, bad):
    arr = shard_array([item])
    return enc._L.cfsec_ec_reconstruct_data(enc._h, arr, n, ints(bad), len(bad), _lib.MEM_HOST, None)


def full(n, size, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(n)]


@pytest.fixture(scope="module")
def rs_enc():
    return ec.NewEncoder(ec.Config(CodeMode=cm.GetTactic(cm.EC6P6)))


@pytest.fixture(scope="module")
def lrc_enc():
    return ec.NewEncoder(ec.Config(CodeMode=cm.GetTactic(cm.EC6P10L2)))


def test_null_pointers_and_negative_count(rs_enc):
    L, h = rs_enc._L, rs_enc._h
    arr = shard_array([full(12, 8)])
    st = (ctypes.c_int * 1)()
    off = ints([0, 0])
    f = L.cfsec_ec_reconstruct_data_batch
    assert f(None, arr, 12, 1, None, off, _lib.MEM_HOST, st) == INVALID_ARG
    assert f(h, None, 12, 1, None, off, _lib.MEM_HOST, st) == INVALID_ARG
    assert f(h, arr, 12, 1, None, None, _lib.MEM_HOST, st) == INVALID_ARG
    assert f(h, arr, 12, 1, None, off, _lib.MEM_HOST, None) == INVALID_ARG
    assert f(h, arr, 12, -1, None, off, _lib.MEM_HOST, st) == INVALID_ARG
    assert f(h, arr, 0, 1, None, off, _lib.MEM_HOST, st) == INVALID_ARG
    # a bad set without its indices, offsets that do not start at 0 or go down
    assert f(h, arr, 12, 1, None, ints([0, 1]), _lib.MEM_HOST, st) == INVALID_ARG
    assert f(h, arr, 12, 1, ints([0]), ints([1, 1]), _lib.MEM_HOST, st) == INVALID_ARG
    g = L.cfsec_rs_reconstruct_data_stripes
    e = reedsolomon.New(6, 6)
    assert g(None, arr, 1, _lib.MEM_HOST, st) == INVALID_ARG
    assert g(e._h, None, 1, _lib.MEM_HOST, st) == INVALID_ARG
    assert g(e._h, arr, 1, _lib.MEM_HOST, None) == INVALID_ARG
    assert g(e._h, arr, -1, _lib.MEM_HOST, st) == INVALID_ARG


def test_no_items_is_ok(rs_enc):
    L = rs_enc._L
    assert L.cfsec_ec_reconstruct_data_batch(rs_enc._h, None, 12, 0, None, None, _lib.MEM_HOST, None) == OK
    assert L.cfsec_ec_reconstruct_data_batch(rs_enc._h, None, 0, 0, None, None, _lib.MEM_HOST, None) == OK
    assert rs_enc.ReconstructDataBatch([], []) == []
    e = reedsolomon.New(6, 6)
    assert L.cfsec_rs_reconstruct_data_stripes(e._h, None, 0, _lib.MEM_HOST, None) == OK
    assert e.ReconstructDataStripes([]) == []


@pytest.mark.parametrize("n", [11, 13, 6])
def test_wrong_n_gives_the_single_calls_code_per_item(rs_enc, n):
    items = [full(n, 8, s) for s in range(3)]
    bad = [[0], [], [n + 5]]  # the last one: an index outside the n shards, initBadShards' error
    rc, st = batch(rs_enc, items, n, bad)
    want = [single(rs_enc, full(n, 8, s), n, b) for s, b in enumerate(bad)]
    assert rc == OK and st == want
    assert st[0] == st[1] == _lib.ErrTooFewShards.status and st[2] == INVALID_ARG


@pytest.mark.parametrize("n", [15, 12])
def test_lrc_wrong_n(lrc_enc, n):
    items = [full(n, 8, s) for s in range(2)]
    rc, st = batch(lrc_enc, items, n, [[0], []])
    assert rc == OK and st == [single(lrc_enc, full(n, 8, s), n, b) for s, b in enumerate([[0], []])]
    assert st == [_lib.ErrInvalidShards.status] * 2


def test_statuses_decided_before_the_device(rs_enc):
    """Too few shards, an all-empty item, two shard sizes, a missing shard without capacity, and the
    no-op items (nothing bad; only parity bad) -- the codes of the single call, item by item."""
    def cases():
        few = full(12, 16, 1)
        empty = [None] * 12
        sizes = full(12, 16, 2)
        sizes[3] = sizes[3][:9].copy()
        nocap = full(12, 16, 3)
        nocap[1] = None
        noop = full(12, 16, 4)
        parity = full(12, 16, 5)
        return [(few, list(range(7))), (empty, []), (sizes, [0]), (nocap, []), (noop, []), (parity, [7, 11])]

    items, bad = zip(*cases())
    keep = [[None if s is None else s.copy() for s in it] for it in items]
    rc, st = batch(rs_enc, list(items), 12, list(bad))
    want = [single(rs_enc, it, 12, b) for it, b in cases()]
    assert rc == OK and st == want
    assert st == [_lib.ErrTooFewShards.status, _lib.ErrShardNoData.status, _lib.ErrShardSize.status, INVALID_ARG, OK, OK]
    for it, k in zip(items, keep):  # no buffer of any of these items was written
        for a, b in zip(it, k):
            assert (a is None and b is None) or np.array_equal(a, b)


def test_rs_stripes_statuses_without_a_device():
    e = reedsolomon.New(6, 6)
    few = full(12, 16, 1)
    for i in range(7):
        few[i] = few[i][:0]
    noop = full(12, 16, 2)
    noop[9] = None  # only parity missing: ReconstructData has nothing to do
    assert e.ReconstructDataStripes([few, [None] * 12, noop, full(12, 16, 3)]) == [
        _lib.ErrTooFewShards.status, _lib.ErrShardNoData.status, OK, OK]
    assert noop[9] is None or len(noop[9]) == 0
