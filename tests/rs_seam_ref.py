"""Reference values for EncodeIdx, Update and ReconstructSome (KRS/reedsolomon.go:631-667, 672-734,
1395-1397), in numpy over the oracle's matrix and multiplication table.  Every function works on
arrays it is given (views into a test's pool image, say) and changes exactly the bytes the reference
changes."""
import functools

import numpy as np

from oracle import oracle as O


@functools.lru_cache(maxsize=None)
def _mul():
    return O.tables()["mulTable"].copy()


@functools.lru_cache(maxsize=None)
def matrix(k, m):
    return O.build_matrix(k, k + m).copy()


def encode_idx(k, m, data, idx, parity):
    """parity[r] ^= mul[M[k + r][idx]][data]"""
    M, mul = matrix(k, m), _mul()
    for r in range(m):
        parity[r][:] ^= mul[M[k + r][idx]][data]


def update(k, m, shards, new):
    """For every present new[c]: d = old ^ new; old = d; parity[r] ^= mul[M[k + r][c]][d]"""
    M, mul = matrix(k, m), _mul()
    for c in range(k):
        if new[c] is None or new[c].size == 0:
            continue
        shards[c][:] ^= new[c]
        for r in range(m):
            shards[k + r][:] ^= mul[M[k + r][c]][shards[c]]


def reconstruct_some(k, m, shards, present, required):
    """oracle.reconstruct(data_only=True) on a copy; the missing data rows i with required[i] are taken
    from it into shards[i] (buffers of the shard size), every other buffer is left as it is.  Returns
    the indices written."""
    size = next(s.size for s, p in zip(shards, present) if p)
    work = [s.copy() if p else np.zeros(size, np.uint8) for s, p in zip(shards, present)]
    err, _ = O.reconstruct(k, m, work, list(present), data_only=True)
    assert err == 0, err
    written = [i for i in range(k) if not present[i] and i < len(required) and required[i]]
    for i in written:
        shards[i][:size] = work[i]
    return written
