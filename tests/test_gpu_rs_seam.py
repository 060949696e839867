"""EncodeIdx, Update, ReconstructSome and their batch forms on the GPU, bit-exact against the numpy
reference over the oracle's matrix (tests/rs_seam_ref.py).

Every case carves its rows from one pool: row j starts 0, 1, 3 or 13 bytes past a 256-byte boundary,
with random slack between rows.  After every call the whole pool image is compared with the image the
reference leaves, which catches a write outside the written rows, a change to new_data, to the
EncodeIdx data shard or to a data row that did not change.  The shapes are the smallest at which
the kernels can go wrong: lengths around the 16-byte lane chunk and the 4 KiB tile, more than one
tile, every kernel instantiation's row count, the row-chunk ((6, 33)) and column-chunk ((40, 3), all
columns) launches, every memory path.
"""
import ctypes

import numpy as np
import pytest
import torch

import rs_seam_ref as R
from chubaofs_amd import _lib, reedsolomon
from oracle import oracle as O
from test_delta_plan import driver, run_driver  # noqa: F401  (the plan driver fixture: one build per module)

pytestmark = pytest.mark.gpu

ENGINES = [(12, 4), (6, 6), (16, 20), (10, 4), (3, 3), (8, 1), (6, 33), (40, 3)]
LENS = [1, 15, 16, 17, 4095, 4096, 4097, 8197]
OFFS = [0, 1, 3, 13]
KINDS = ["device", "pinned", "pageable"]
FILL = 0xA5


# ---------------------------------------------------------------- the pool

class Pool:
    """Rows carved from one image; place() puts the image into one kind of memory."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.size = 256
        self.rows = []

    def row(self, nbytes):
        """Offset of a new row of nbytes: the next of OFFS past a 256-byte boundary, after random slack."""
        pos = (self.size + int(self.rng.integers(0, 200)) + 255) // 256 * 256 + OFFS[len(self.rows) % 4]
        self.rows.append((pos, nbytes))
        self.size = pos + nbytes
        return pos

    def rows_of(self, n, nbytes):
        return [self.row(nbytes) for _ in range(n)]

    def image(self):
        return self.rng.integers(0, 256, self.size + 256, dtype=np.uint8)


_pinned = {}


def pinned_buffer(nbytes):
    """One page-locked block for the module, grown on demand (an allocation per case costs milliseconds)."""
    if _pinned.get("size", 0) < nbytes:
        _pinned["buf"] = _lib.pinned_empty(max(nbytes, 2 << 20))
        _pinned["size"] = _pinned["buf"].size
    return _pinned["buf"]


class Mem:
    """An image in one kind of memory, its first byte on a 256-byte boundary."""

    def __init__(self, kind, image):
        self.kind, self.n = kind, image.size
        if kind == "device":
            self.buf = torch.empty(image.size + 256, dtype=torch.uint8, device="cuda")
            base = self.buf.data_ptr()
        else:
            self.buf = pinned_buffer(image.size + 256) if kind == "pinned" else np.empty(image.size + 256, np.uint8)
            base = self.buf.ctypes.data
        self.off = (-base) % 256
        self.ptr = base + self.off
        if kind == "device":
            self.buf[self.off:self.off + self.n] = torch.from_numpy(image).cuda()
            torch.cuda.synchronize()
        else:
            self.buf[self.off:self.off + self.n] = image
        self.mem = _lib.MEM_DEVICE if kind == "device" else _lib.MEM_HOST

    def read(self):
        if self.kind == "device":
            torch.cuda.synchronize()
            return self.buf[self.off:self.off + self.n].cpu().numpy()
        return np.array(self.buf[self.off:self.off + self.n])


def shard(mem, pos, length, cap=None):
    return _lib.Shard(mem.ptr + pos, length, length if cap is None else cap)


def absent():
    return _lib.Shard(None, 0, 0)


def view(image, pos, S):
    return image[pos:pos + S]


_engines = {}


def engine(k, m):
    if (k, m) not in _engines:
        _engines[(k, m)] = reedsolomon.New(k, m, device=0)
    return _engines[(k, m)]


def check(st):
    assert st == 0, (_lib.lib().cfsec_status_name(st), _lib.lib().cfsec_last_error())


# ---------------------------------------------------------------- Update

def column_sets(k):
    sets = [[0], [k - 1], list(range(k))]
    if k >= 2:
        sets.insert(2, [k // 2 - 1, k // 2] if k >= 4 else [0, 1])
    return sets


def update_case(k, m, S, cols, kind, seed):
    """One cfsec_rs_update against the reference: the whole pool image, and the old rows hold the delta."""
    e = engine(k, m)
    pool = Pool(seed)
    rows = pool.rows_of(k + m, S)
    new = {c: pool.row(S) for c in cols}
    image = pool.image()
    mem = Mem(kind, image)
    sh = (_lib.Shard * (k + m))(*[shard(mem, p, S) for p in rows])
    nw = (_lib.Shard * k)(*[shard(mem, new[c], S) if c in new else absent() for c in range(k)])
    check(e._L.cfsec_rs_update(e._h, sh, k + m, nw, k, mem.mem, None))
    want = image.copy()
    R.update(k, m, [view(want, p, S) for p in rows], [view(want, new[c], S) if c in new else None for c in range(k)])
    got = mem.read()
    assert np.array_equal(got, want), (k, m, S, cols, kind, np.flatnonzero(got != want)[:8])
    for c in cols:
        assert np.array_equal(view(got, rows[c], S), view(image, rows[c], S) ^ view(image, new[c], S))
    assert all(sh[i].len == S for i in range(k + m))


@pytest.mark.parametrize("k,m", ENGINES)
def test_update_device_every_length_and_column_set(k, m):
    for S in LENS:
        for j, cols in enumerate(column_sets(k)):
            update_case(k, m, S, cols, "device", seed=(k * 64 + m) * 64 + j)


@pytest.mark.parametrize("kind", ["pinned", "pageable"])
@pytest.mark.parametrize("k,m", ENGINES)
def test_update_host_memory(k, m, kind):
    for S in LENS:
        for j, cols in enumerate((column_sets(k)[0], column_sets(k)[-1])):
            update_case(k, m, S, cols, kind, seed=(k * 64 + m) * 64 + 7 + j)


def test_update_partly_page_locked_stripe_takes_the_staged_path(monkeypatch, capfd):
    """Data rows page-locked, parity and new rows pageable: not every row aliases, so the call stages
    every row whole -- and still matches."""
    k, m, S, cols = 12, 4, 4097, [2, 3]
    e = engine(k, m)
    pa, pb = Pool(1), Pool(2)
    data_rows = pa.rows_of(k, S)
    par_rows = pb.rows_of(m, S)
    new = {c: pb.row(S) for c in cols}
    ia, ib = pa.image(), pb.image()
    ma, mb = Mem("pinned", ia), Mem("pageable", ib)
    sh = (_lib.Shard * (k + m))(*([shard(ma, p, S) for p in data_rows] + [shard(mb, p, S) for p in par_rows]))
    nw = (_lib.Shard * k)(*[shard(mb, new[c], S) if c in new else absent() for c in range(k)])
    monkeypatch.setenv("CFSEC_TRACE_DELTA", "1")
    capfd.readouterr()
    check(e._L.cfsec_rs_update(e._h, sh, k + m, nw, k, _lib.MEM_HOST, None))
    err = capfd.readouterr().err
    wa, wb = ia.copy(), ib.copy()
    R.update(k, m, [view(wa, p, S) for p in data_rows] + [view(wb, p, S) for p in par_rows],
             [view(wb, new[c], S) if c in new else None for c in range(k)])
    assert np.array_equal(ma.read(), wa) and np.array_equal(mb.read(), wb)
    assert delta_lines(err) == [dict(mode="delta", nc="2", m="4", r0="0", c0="0", stripes="1", s0="0", len=str(S), affine="0")]


# ---------------------------------------------------------------- EncodeIdx

def encode_idx_case(k, m, S, idx, kind, seed):
    e = engine(k, m)
    pool = Pool(seed)
    data = pool.row(S)
    par = pool.rows_of(m, S)
    image = pool.image()
    mem = Mem(kind, image)
    d = (_lib.Shard * 1)(shard(mem, data, S))
    p = (_lib.Shard * m)(*[shard(mem, q, S) for q in par])
    check(e._L.cfsec_rs_encode_idx(e._h, d, idx, p, m, mem.mem, None))
    want = image.copy()
    R.encode_idx(k, m, view(want, data, S), idx, [view(want, q, S) for q in par])
    got = mem.read()
    assert np.array_equal(got, want), (k, m, S, idx, kind, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,m", ENGINES)
def test_encode_idx(k, m, kind):
    idxs = range(k) if (k, m) in ((12, 4), (3, 3)) else (0, k - 1)
    for S in LENS:
        for idx in idxs:
            encode_idx_case(k, m, S, idx, kind, seed=(k * 64 + m) * 64 + idx)


def test_encode_idx_steps_build_the_encode():
    """k EncodeIdx calls from zeroed parity, data shards in any order, leave Encode's parity."""
    k, m, S = 12, 4, 4097
    rng = np.random.default_rng(3)
    want = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)] + [np.zeros(S, np.uint8) for _ in range(m)]
    assert O.encode(k, m, want) == 0
    dev = [torch.from_numpy(w).cuda() for w in want[:k]]
    par = [torch.zeros(S, dtype=torch.uint8, device="cuda") for _ in range(m)]
    e = engine(k, m)
    for idx in rng.permutation(k):
        e.EncodeIdx(dev[idx], int(idx), par)
    for r in range(m):
        assert np.array_equal(par[r].cpu().numpy(), want[k + r])


def test_update_through_the_wrapper_leaves_a_stripe_that_verifies():
    k, m, S = 6, 6, 8197
    rng = np.random.default_rng(4)
    host = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)] + [np.zeros(S, np.uint8) for _ in range(m)]
    e = engine(k, m)
    dev = [torch.from_numpy(h).cuda() for h in host]
    e.Encode(dev)
    new = [None] * k
    new[1] = torch.from_numpy(rng.integers(0, 256, S, dtype=np.uint8)).cuda()
    new[4] = torch.from_numpy(rng.integers(0, 256, S, dtype=np.uint8)).cuda()
    old1 = dev[1].clone()
    e.Update(dev, new)
    assert torch.equal(dev[1], old1 ^ new[1])  # the delta, as the reference leaves it
    dev[1], dev[4] = new[1], new[4]
    assert e.Verify(dev)


# ---------------------------------------------------------------- update_batch

def delta_lines(err):
    return [dict(x.split("=") for x in ln.split()[2:]) for ln in err.splitlines() if ln.startswith("cfsec: delta ")]


def plan_lines(steps):
    """A plan's steps as the trace prints them."""
    return [dict(mode="delta" if s["delta"] else "plain", nc=str(s["kc"]), m=str(s["mc"]), r0=str(s["r0"]), c0=str(s["c0"]),
                 stripes=str(s["ns"]), s0=str(s["s0"]), len=str(s["len"]), affine=str(s["affine"])) for s in steps]


def batch_case(k, m, S, cols, nstripes, affine, seed, stream=None):
    """Stripes in one device pool; returns (Mem, ptrs, new_ptrs, image, reference image)."""
    pool = Pool(seed)
    nc = len(cols)
    if affine:  # pitched: every stripe the same layout, one stride on
        first = pool.rows_of(k + m + nc, S)
        pitch = (pool.size + 255) // 256 * 256 + 768
        stripes = [[p + s * pitch for p in first] for s in range(nstripes)]
        pool.size = stripes[-1][-1] + S
    else:
        stripes = [pool.rows_of(k + m + nc, S) for _ in range(nstripes)]
    image = pool.image()
    mem = Mem("device", image)
    ptrs, new_ptrs = [], []
    for rows in stripes:
        # entries of unchanged data columns are never dereferenced: NULL
        ptrs += [mem.ptr + rows[i] if i >= k or i in cols else 0 for i in range(k + m)]
        new_ptrs += [mem.ptr + rows[k + m + j] for j in range(nc)]
    want = image.copy()
    for rows in stripes:
        R.update(k, m, [view(want, p, S) for p in rows[:k + m]],
                 [view(want, rows[k + m + cols.index(c)], S) if c in cols else None for c in range(k)])
    return mem, ptrs, new_ptrs, image, want


@pytest.mark.parametrize("S", [17, 4097])
def test_update_batch_affine_pitched_stripes(S, monkeypatch, capfd):
    k, m, cols = 12, 4, [0, 5]
    mem, ptrs, new_ptrs, _, want = batch_case(k, m, S, cols, 3, True, seed=S)
    monkeypatch.setenv("CFSEC_TRACE_DELTA", "1")
    capfd.readouterr()
    engine(k, m).update_batch(ptrs, new_ptrs, cols, S, 3)
    got = mem.read()
    err = capfd.readouterr().err
    assert np.array_equal(got, want)
    assert delta_lines(err) == [dict(mode="delta", nc="2", m="4", r0="0", c0="0", stripes="3", s0="0", len=str(S), affine="1")]


@pytest.mark.parametrize("side", [False, True], ids=["current stream", "side stream"])
def test_update_batch_scattered_stripes_split_as_the_plan_says(side, driver, monkeypatch, capfd):  # noqa: F811
    """41 scattered EC12P4 stripes, 2 changed columns, 4097 bytes: 8 pointers per stripe, 36 stripes per
    argument block, so two launches -- the trace against the plan driver's answer."""
    k, m, S, cols, n = 12, 4, 4097, [3, 4], 41
    mem, ptrs, new_ptrs, _, want = batch_case(k, m, S, cols, n, False, seed=41)
    (plan,) = run_driver(driver, [(len(cols), m, 1, S, "scat", n)])
    assert [s["ns"] for s in plan["steps"]] == [36, 5]
    monkeypatch.setenv("CFSEC_TRACE_DELTA", "1")
    capfd.readouterr()
    if side:
        stream = torch.cuda.Stream()
        engine(k, m).update_batch(ptrs, new_ptrs, cols, S, n, stream=stream)
        stream.synchronize()
        got = mem.buf[mem.off:mem.off + mem.n].cpu().numpy()
    else:
        engine(k, m).update_batch(ptrs, new_ptrs, cols, S, n)
        got = mem.read()
    err = capfd.readouterr().err
    assert np.array_equal(got, want)
    assert delta_lines(err) == plan_lines(plan["steps"])


def test_update_batch_row_and_column_chunks():
    """(6, 33): the 33rd row is a plain launch over the rewritten columns; (40, 3), every column: two
    column chunks -- both as batches of scattered stripes."""
    for k, m, cols, n in ((6, 33, [0, 5], 3), (40, 3, list(range(40)), 4)):
        mem, ptrs, new_ptrs, _, want = batch_case(k, m, 4097, cols, n, False, seed=k)
        engine(k, m).update_batch(ptrs, new_ptrs, cols, 4097, n)
        assert np.array_equal(mem.read(), want), (k, m)


# ---------------------------------------------------------------- ReconstructSome

SOME_ENGINES = [(12, 4), (6, 6), (16, 20), (40, 3)]
SOME_LENS = [1, 17, 4097]


def scenarios(k):
    """(missing shards, required data indices, mask length)"""
    a, b = 1, k - 1
    return {
        "one of two": ([a, b], [b], k),
        "both": ([a, b], [a, b], k),
        "none": ([a, b], [], k),
        "a present one too": ([a, b], [0, a], k),
        "missing parity alongside": ([a, b, k], [a], k),
        "missing parity required": ([a, b, k + 1], [b, k + 1], k + 2),
    }


def stripe_case(k, m, S, seed):
    """An encoded stripe's host rows."""
    rng = np.random.default_rng(seed)
    sh = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)] + [np.zeros(S, np.uint8) for _ in range(m)]
    assert O.encode(k, m, sh) == 0
    return sh


def some_layout(pool, k, m, S, missing):
    """Rows of one stripe in the pool; a missing shard's buffer has spare capacity."""
    return [pool.row(S + (5 if i in missing else 0)) for i in range(k + m)]


def fill_stripe(image, rows, data, S, missing):
    for i, p in enumerate(rows):
        if i in missing:
            image[p:p + S + 5] = FILL
        else:
            image[p:p + S] = data[i]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,m", SOME_ENGINES)
def test_reconstruct_some(k, m, kind):
    e = engine(k, m)
    for S in SOME_LENS:
        data = stripe_case(k, m, S, seed=k + S)
        for j, (name, (missing, required, nreq)) in enumerate(scenarios(k).items()):
            pool = Pool(seed=(k * 64 + S) * 8 + j)
            rows = some_layout(pool, k, m, S, missing)
            image = pool.image()
            fill_stripe(image, rows, data, S, missing)
            mem = Mem(kind, image)
            sh = (_lib.Shard * (k + m))(*[shard(mem, p, 0, S + 5) if i in missing else shard(mem, p, S)
                                          for i, p in enumerate(rows)])
            req = np.zeros(nreq, np.uint8)
            req[required] = 1
            check(e._L.cfsec_rs_reconstruct_some(e._h, sh, k + m, req.ctypes.data, nreq, mem.mem, None))
            want = image.copy()
            present = [i not in missing for i in range(k + m)]
            written = R.reconstruct_some(k, m, [view(want, p, S) for p in rows], present, list(req))
            assert written == [i for i in required if i in missing and i < k], name
            got = mem.read()
            assert np.array_equal(got, want), (k, m, S, name, kind, np.flatnonzero(got != want)[:8])
            for i in range(k + m):
                # rebuilt shards get the shard size, every other missing one keeps len 0 and its fill
                assert sh[i].len == (S if i in written or i not in missing else 0), (name, i)
                if i in missing and i not in written:
                    assert (view(got, rows[i], S + 5) == FILL).all(), (name, i)
                elif i in written:
                    assert np.array_equal(view(got, rows[i], S), data[i]), (name, i)


def mix_lines(err):
    return [dict(x.split("=") for x in ln.split()[2:]) for ln in err.splitlines() if ln.startswith("cfsec: mix ")]


@pytest.mark.parametrize("kind", KINDS)
def test_reconstruct_some_stripes_matches_the_single_calls(kind, monkeypatch, capfd):
    """20 EC12P4 segments of mixed lengths, erasure patterns and masks as one call: the statuses and the
    pool image of the single calls, through the mixed-plan launch."""
    k, m, n = 12, 4, 20
    e = engine(k, m)
    rng = np.random.default_rng(20)
    lens = [1, 15, 16, 17, 4095, 4096, 4097, 8197] + [int(x) for x in rng.integers(1, 8198, n - 8)]
    pool = Pool(seed=77)
    items = []
    for s, S in enumerate(lens):
        if s == 5:
            missing, required = [], [0, 1]                       # nothing missing
        elif s == 9:
            missing, required = [0, 1, 2, 3, k], [0]             # too few shards
        elif s == 13:
            missing, required = [2, 7], []                       # nothing required
        else:
            missing = sorted(int(x) for x in rng.choice(k + 2, size=int(rng.integers(1, 4)), replace=False))
            required = [i for i in missing if i < k and rng.integers(0, 2)] + [int(rng.integers(0, k))]
        items.append((S, missing, sorted(set(required)), some_layout(pool, k, m, S, missing)))
    image = pool.image()
    for s, (S, missing, _, rows) in enumerate(items):
        fill_stripe(image, rows, stripe_case(k, m, S, seed=1000 + s), S, missing)
    masks = np.zeros((n, k), np.uint8)
    for s, (_, _, required, _) in enumerate(items):
        masks[s, required] = 1

    def shards_of(mem):
        arr = (_lib.Shard * (n * (k + m)))()
        for s, (S, missing, _, rows) in enumerate(items):
            for i, p in enumerate(rows):
                arr[s * (k + m) + i] = shard(mem, p, 0, S + 5) if i in missing else shard(mem, p, S)
        return arr

    # the single calls
    # (the module's one page-locked block holds the batch below: its singles run on a pageable copy)
    one = Mem("pageable" if kind == "pinned" else kind, image)
    arr1 = shards_of(one)
    status1 = []
    for s in range(n):
        sub = (_lib.Shard * (k + m)).from_address(ctypes.addressof(arr1) + s * (k + m) * ctypes.sizeof(_lib.Shard))
        status1.append(e._L.cfsec_rs_reconstruct_some(e._h, sub, k + m, masks[s].ctypes.data, k, one.mem, None))
    want = one.read()
    # the reference, for the stripes that run
    ref = image.copy()
    for s, (S, missing, required, rows) in enumerate(items):
        if status1[s] == 0 and missing:
            R.reconstruct_some(k, m, [view(ref, p, S) for p in rows], [i not in missing for i in range(k + m)],
                               list(masks[s]))
    assert np.array_equal(want, ref)
    assert status1[9] == _lib.ErrTooFewShards.status and [st for i, st in enumerate(status1) if i != 9] == [0] * (n - 1)

    mem = Mem(kind, image)
    arr = shards_of(mem)
    status = (ctypes.c_int * n)(*([-7] * n))
    monkeypatch.delenv("CFSEC_MIX_MAX_LEN", raising=False)
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    capfd.readouterr()
    check(e._L.cfsec_rs_reconstruct_some_stripes(e._h, arr, n, masks.ctypes.data, mem.mem, status))
    got = mem.read()
    err = capfd.readouterr().err
    assert [int(x) for x in status] == status1
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert [arr[i].len for i in range(n * (k + m))] == [arr1[i].len for i in range(n * (k + m))]
    assert len(mix_lines(err)) >= 1, err  # every segment is below CFSEC_MIX_MAX_LEN's default: the mixed launch
