"""Batched degraded reads on the GPU: cfsec_ec_reconstruct_data_batch and cfsec_rs_reconstruct_data_stripes
(the mixed-plan launch of gf_mix.hip and the launch groups behind it).

Every case lays its shards out in one arena of random bytes: each row sits at a chosen byte offset (0,
1, 3 or 13) from a 16-byte boundary, inputs and outputs misaligned independently, with at least 64
untouched bytes on either side.  The call runs on one copy of the arena, a loop of single
ReconstructData calls on a second copy, and ECOracle.reconstruct_data / rs_reconstruct(data_only=True)
on host copies of the rows.  Asserted:

  * status for status: batch == loop of single calls (== the oracle, where the C ABI can do what Go
    does: an item whose missing shard has too little capacity is an error here and an allocation there);
  * byte for byte: the whole arena after the batch call equals the arena with the oracle's rebuilt data
    shards put in -- so every guard byte, every input row, every shard the call had no business with
    and every buffer of a failed item is unchanged, and every rebuilt row is the oracle's;
  * the shard headers (len) after the call equal the single calls' and the oracle's: rebuilt data
    shards get the shard size, bad parity shards stay at 0.

The shards are random bytes, not codewords (one case uses codewords to see the original data come
back): ReconstructData is the same linear function of the survivors either way, which is what the
reference computes, so every case is also the non-codeword case.

Sizes are the smallest at which the kernel can go wrong: lengths around the 16-byte chunk and the 4 KiB
tile, 17 tiles with a ragged end, more than 4 outputs (a second pass), more items than any argument
block holds.  None is a workload size.
"""
import ctypes
import itertools

import numpy as np
import pytest

from chubaofs_amd import _lib, codemode as cm, ec, reedsolomon
from oracle import ec_oracle as EO
from oracle.ec_oracle import ECOracle, Slice

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LENS = [1, 7, 15, 16, 17, 63, 4095, 4096, 4097, 8193, 65536 + 5]
ALIGN = [0, 1, 3, 13]
GUARD = 64
MIX_ALL = str(1 << 20)  # CFSEC_MIX_MAX_LEN that takes every length used here


def tactic(name):
    (c,) = [c for c in cm.GetAllCodeModes() if cm.Name(c) == name]
    return cm.GetTactic(c)


# ---------------------------------------------------------------- the arena

class Row:
    """One shard of one item: `size` bytes of buffer at arena offset `pos` (None: no buffer at all),
    header length `len` going into the call."""

    def __init__(self, size, length, mis):
        self.size, self.len, self.mis, self.pos = size, length, mis, None


class Case:
    def __init__(self, n, seed):
        self.n, self.items, self.bad, self.oracle_ok = n, [], [], []
        self.rng = np.random.default_rng(seed)
        self.size = 0

    def add(self, rows, bad, oracle_ok=True):
        assert len(rows) == self.n
        for r in rows:
            if r.size:
                r.pos = (self.size + GUARD + 15) // 16 * 16 + r.mis
                self.size = r.pos + r.size
        self.items.append(rows)
        self.bad.append(list(bad))
        self.oracle_ok.append(oracle_ok)

    def item(self, S, bad, lens=None, mis=None):
        """n full rows of S bytes (header length S, or lens[i]).  Row j of the c-th item sits at offset
        ALIGN[(c + j) % 4] from a 16-byte boundary, a row in `bad` two steps further round: over a few
        items every input and every output meets every offset, and an output never shares its
        neighbours' alignment."""
        c = len(self.items)
        rows = [Row(S, S if lens is None else lens[j], ALIGN[(c + j + (2 if j in bad else 0)) % 4] if mis is None else mis[j])
                for j in range(self.n)]
        self.add(rows, bad)

    def image(self):
        return self.rng.integers(0, 256, self.size + GUARD, dtype=np.uint8)


class Mem:
    """The arena in one kind of memory, its first byte on a 16-byte boundary."""

    def __init__(self, kind, image):
        self.kind, self.n = kind, image.size
        if kind == "device":
            self.buf = torch.empty(image.size + 16, dtype=torch.uint8, device="cuda")
            base = self.buf.data_ptr()
        else:
            self.buf = _lib.pinned_empty(image.size + 16) if kind == "pinned" else np.empty(image.size + 16, np.uint8)
            base = self.buf.ctypes.data
        self.off = (-base) % 16
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


def shard_array(case, mem):
    arr = (_lib.Shard * (len(case.items) * case.n))()
    for i, rows in enumerate(case.items):
        for j, r in enumerate(rows):
            arr[i * case.n + j] = _lib.Shard(mem.ptr + r.pos, r.len, r.size) if r.size else _lib.Shard(None, 0, 0)
    return arr


def ints(v):
    return (ctypes.c_int * max(len(v), 1))(*v)


# ---------------------------------------------------------------- the three ways to run a case

class EcCalls:
    """cfsec_ec_reconstruct_data_batch against cfsec_ec_reconstruct_data and ECOracle.reconstruct_data."""

    def __init__(self, t):
        self.t = t
        self.enc = ec.NewEncoder(ec.Config(CodeMode=t))
        self.orc = ECOracle.from_tactic(t)

    def batch(self, arr, n, nitems, bad, mem):
        flat = [i for b in bad for i in b]
        off = [0] + list(itertools.accumulate(len(b) for b in bad))
        status = (ctypes.c_int * max(nitems, 1))(*([-7] * max(nitems, 1)))
        rc = self.enc._L.cfsec_ec_reconstruct_data_batch(self.enc._h, arr, n, nitems, ints(flat), ints(off), mem, status)
        return rc, [int(status[i]) for i in range(nitems)]

    def single(self, sub, n, bad, mem):
        return self.enc._L.cfsec_ec_reconstruct_data(self.enc._h, sub, n, ints(bad), len(bad), mem, None)

    def oracle(self, shards, bad):
        return self.orc.reconstruct_data(shards, bad)


class RsCalls:
    """cfsec_rs_reconstruct_data_stripes against cfsec_rs_reconstruct_data and rs_reconstruct(data_only):
    the missing shards are the ones whose header length is 0 (the bad lists stay empty)."""

    def __init__(self, k, m):
        self.k, self.m = k, m
        self.enc = reedsolomon.New(k, m, device=0)

    def batch(self, arr, n, nitems, bad, mem):
        status = (ctypes.c_int * max(nitems, 1))(*([-7] * max(nitems, 1)))
        rc = self.enc._L.cfsec_rs_reconstruct_data_stripes(self.enc._h, arr, nitems, mem, status)
        return rc, [int(status[i]) for i in range(nitems)]

    def single(self, sub, n, bad, mem):
        return self.enc._L.cfsec_rs_reconstruct_data(self.enc._h, sub, n, mem, None)

    def oracle(self, shards, bad):
        return EO.rs_reconstruct(self.k, self.m, shards, data_only=True)


def expect(case, calls, image):
    """The oracle on host copies of every item: (statuses, arena afterwards, header lengths)."""
    want = image.copy()
    status, lens = [], []
    for rows, bad, ok in zip(case.items, case.bad, case.oracle_ok):
        if not ok:  # what Go would allocate for, the C ABI refuses: nothing written, decided by the single call
            status.append(None)
            lens.append(None)
            continue
        sh = [Slice(image[r.pos:r.pos + r.size].copy(), r.len) if r.size else Slice() for r in rows]
        st = calls.oracle(sh, bad)
        status.append(st)
        lens.append([s.len for s in sh])
        if st == EO.OK:
            for r, s in zip(rows, sh):
                if r.size:
                    assert s.buf.size == r.size, "the oracle allocated: the case needs oracle_ok=False"
                    want[r.pos:r.pos + r.size] = s.buf
    return status, want, lens


def run(case, calls, kind, capfd=None):
    """Run the case all three ways and compare; returns (trace of the batch call, statuses, arena)."""
    image = case.image()
    n, nitems = case.n, len(case.items)
    ostatus, want, olens = expect(case, calls, image)
    a, b = Mem(kind, image), Mem(kind, image)
    arr_a, arr_b = shard_array(case, a), shard_array(case, b)
    if capfd:
        capfd.readouterr()
    rc, status = calls.batch(arr_a, n, nitems, case.bad, a.mem)
    got = a.read()
    err = capfd.readouterr().err if capfd else ""
    assert rc == 0, _lib.lib().cfsec_last_error()
    one = []
    for i in range(nitems):
        sub = (_lib.Shard * n).from_address(ctypes.addressof(arr_b) + i * n * ctypes.sizeof(_lib.Shard))
        one.append(calls.single(sub, n, case.bad[i], b.mem))
    assert status == one, "batch statuses differ from the single calls'"
    assert all(o is None or o == s for o, s in zip(ostatus, status)), (ostatus, status)
    lens_a = [[arr_a[i * n + j].len for j in range(n)] for i in range(nitems)]
    lens_b = [[arr_b[i * n + j].len for j in range(n)] for i in range(nitems)]
    assert lens_a == lens_b, "shard headers differ from the single calls'"
    assert all(o is None or o == x for o, x in zip(olens, lens_a)), "shard headers differ from the oracle's"
    bad_at = np.flatnonzero(got != want)
    assert bad_at.size == 0, "arena differs from the oracle's at %d bytes, first at %d" % (bad_at.size, bad_at[0])
    assert np.array_equal(b.read(), want), "the single calls differ from the oracle"
    return err, status, got


def mix_lines(err):
    return [dict(x.split("=") for x in ln.split()[2:]) for ln in err.splitlines() if ln.startswith("cfsec: mix ")]


def product_lines(err):
    return [ln for ln in err.splitlines() if ln.startswith("cfsec: matvec ") or ln.startswith("cfsec: dy16")]


def tiles_of(lens):
    return sum(-(-ln // 4096) for ln in lens)


# ---------------------------------------------------------------- lengths, alignments, modes, memory kinds

def bad_sets(t):
    """1 and 2 bad data shards, data + parity, and for the LRC modes local indices that are ignored."""
    N, M, L = t.N, t.M, t.L
    sets = [[0], [N - 1], [1, N - 2], [2, N], [0, 3, N + M - 1]]
    if L:
        sets += [[1, N + M], [N - 1, N + M + L - 1, N + 1]]
    return sets


@pytest.mark.parametrize("kind", ["device", "pinned", "pageable"])
@pytest.mark.parametrize("name", ["EC6P6", "EC12P4"])
def test_every_length_in_one_call(name, kind, monkeypatch, capfd):
    t = tactic(name)
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", MIX_ALL)
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    case = Case(t.N + t.M, seed=len(name) + t.N)
    sets = bad_sets(t)
    for i, S in enumerate(LENS):
        case.item(S, sets[i % len(sets)])
    out_mis = {case.items[i][b].mis for i in range(len(LENS)) for b in case.bad[i] if b < t.N}
    in_mis = {r.mis for rows in case.items for r in rows}
    assert out_mis == set(ALIGN) and in_mis == set(ALIGN)
    err, status, _ = run(case, EcCalls(t), kind, capfd)
    assert status == [0] * len(LENS)
    (mix,) = mix_lines(err)  # one launch: in place, or the one staged chunk
    assert int(mix["items"]) == len(LENS) and int(mix["tiles"]) == tiles_of(LENS) and product_lines(err) == []


@pytest.mark.parametrize("name,n", [("EC6P10L2", 18), ("EC6P10L2", 16), ("EC16P20L2", 38)])
def test_lrc_modes(name, n, monkeypatch):
    t = tactic(name)
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", MIX_ALL)
    case = Case(n, seed=n)
    sets = bad_sets(t)
    for i, S in enumerate(LENS):
        case.item(S, sets[i % len(sets)])  # n = N+M: the local indices lie past the vector, and are ignored
    # fillFullShards: a global shard handed in with length 0 and enough room that is not in the bad list
    # counts as present (lrcencoder.go:190); a local shard's header is left alone
    S = 4097
    lens = [S] * n
    lens[2] = 0
    if n > t.N + t.M:
        lens[n - 1] = 0
    case.item(S, [0], lens=lens)
    _, status, _ = run(case, EcCalls(t), "device")
    assert status == [0] * len(case.items)


@pytest.mark.parametrize("name,nbad", [("EC6P6", 5), ("EC6P6", 6), ("EC16P20L2", 9), ("EC16P20L2", 16)])
def test_more_than_four_outputs_take_further_passes(name, nbad, monkeypatch, capfd):
    t = tactic(name)
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", MIX_ALL)
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    case = Case(t.N + t.M + t.L, seed=nbad)
    lens = [17, 4097, 8193, 15]
    for i, S in enumerate(lens):
        bad = [(i + j) % t.N for j in range(nbad)]
        spare = t.M - 1 >= nbad  # a bad parity shard on top leaves enough shards
        case.item(S, bad + ([t.N + 2] if i % 2 and spare else []))
    err, status, _ = run(case, EcCalls(t), "device", capfd)
    assert status == [0] * len(lens)
    (mix,) = mix_lines(err)
    assert int(mix["items"]) == len(lens) and product_lines(err) == []


@pytest.mark.parametrize("k,m", [(12, 4), (6, 6)])
@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_rs_reconstruct_data_stripes(k, m, kind, monkeypatch):
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", MIX_ALL)
    case = Case(k + m, seed=k)
    missing = [[0], [k - 1], [1, k - 2], [2, k], [0, 3, k + m - 1], [k, k + 1], []]
    for i, S in enumerate(LENS):
        miss = missing[i % len(missing)]
        case.item(S, [], lens=[0 if j in miss else S for j in range(k + m)])
    _, status, _ = run(case, RsCalls(k, m), kind)
    assert status == [0] * len(LENS)


# ---------------------------------------------------------------- many items, many plans, the routes

def seventy_patterns(t):
    sets = [list(p) for p in itertools.combinations(range(t.N), 2)] + [[i] for i in range(4)]
    assert len(sets) == 70
    return sets


SMALL = [17, 63, 4097, 1, 4096, 15]


@pytest.fixture(scope="module")
def ec12p4():
    t = tactic("EC12P4")
    return t, EcCalls(t)


def many(t, sets, seed):
    case = Case(t.N + t.M, seed=seed)
    for i, bad in enumerate(sets):
        case.item(SMALL[i % len(SMALL)], bad)
    return case


@pytest.mark.parametrize("which", ["70 patterns", "300 items one pattern"])
def test_one_mixed_launch_whatever_the_patterns(ec12p4, which, monkeypatch, capfd):
    t, calls = ec12p4
    sets = seventy_patterns(t) if which == "70 patterns" else [[1, 7]] * 300
    monkeypatch.delenv("CFSEC_MIX_MAX_LEN", raising=False)
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    err, status, got = run(many(t, sets, seed=len(sets)), calls, "device", capfd)
    assert status == [0] * len(sets)
    (mix,) = mix_lines(err)
    assert int(mix["items"]) == len(sets)
    assert int(mix["plans"]) == (70 if which == "70 patterns" else 1)
    assert int(mix["tiles"]) == tiles_of(SMALL[i % len(SMALL)] for i in range(len(sets)))
    assert product_lines(err) == []
    # the route switched off: the launch groups alone, the same bytes
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", "0")
    err, status, off = run(many(t, sets, seed=len(sets)), calls, "device", capfd)
    assert status == [0] * len(sets)
    assert mix_lines(err) == [] and len(product_lines(err)) >= 1
    assert np.array_equal(got, off)


def test_items_on_both_sides_of_the_length_limit(ec12p4, monkeypatch, capfd):
    t, calls = ec12p4
    lens = [4095, 4096, 4097, 8193, 17, 65536 + 5, 4096]
    sets = [[0], [1, 2], [0], [3, 11], [1, 2], [0], [5, 13]]

    def case():
        c = Case(t.N + t.M, seed=5)
        for S, bad in zip(lens, sets):
            c.item(S, bad)
        return c

    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", "4096")
    err, status, got = run(case(), calls, "device", capfd)
    assert status == [0] * len(lens)
    (mix,) = mix_lines(err)
    small = [S for S in lens if S <= 4096]
    assert int(mix["items"]) == len(small) and int(mix["tiles"]) == tiles_of(small)
    assert len(product_lines(err)) >= 1  # the longer items went through the launch groups
    for limit in ("0", MIX_ALL):
        monkeypatch.setenv("CFSEC_MIX_MAX_LEN", limit)
        _, _, other = run(case(), calls, "device")
        assert np.array_equal(got, other)


def test_a_lone_small_item_goes_to_the_group_path(ec12p4, monkeypatch, capfd):
    t, calls = ec12p4
    monkeypatch.delenv("CFSEC_MIX_MAX_LEN", raising=False)
    monkeypatch.setenv("CFSEC_TRACE_MATVEC", "1")
    case = Case(t.N + t.M, seed=1)
    case.item(4097, [0, 5])
    case.item(4097, [])  # a no-op beside it
    err, status, _ = run(case, calls, "device", capfd)
    assert status == [0, 0] and mix_lines(err) == [] and len(product_lines(err)) >= 1


# ---------------------------------------------------------------- errors between good items

@pytest.mark.parametrize("kind", ["device", "pageable"])
def test_failed_items_between_rebuilt_ones(kind, monkeypatch):
    t = tactic("EC6P6")
    n, S = 12, 4097
    monkeypatch.setenv("CFSEC_MIX_MAX_LEN", MIX_ALL)
    case = Case(n, seed=99)
    case.item(S, [0, 5])
    case.item(S, list(range(7)))  # too few shards left
    case.item(17, [3])
    rows = [Row(S, S, ALIGN[j % 4]) for j in range(n)]
    rows[1] = Row(S - 1, 0, 3)  # missing, and its buffer one byte too small
    case.add(rows, [], oracle_ok=False)
    case.add([Row(0, 0, 0) for _ in range(n)], [])  # every shard empty
    case.item(S, [])  # nothing bad: a no-op
    case.item(63, [7, 11])  # only parity bad: a no-op, the parity stays missing
    case.item(S, [4, 9])
    _, status, _ = run(case, EcCalls(t), kind)
    E = _lib
    assert status == [0, E.ErrTooFewShards.status, 0, E.ErrInvalidArg.status, E.ErrShardNoData.status, 0, 0, 0]


# ---------------------------------------------------------------- codewords, and the Python methods

def test_codewords_come_back_through_the_python_methods(monkeypatch):
    """Encoder.ReconstructDataBatch and ReedSolomon.ReconstructDataStripes on device tensors: the
    original data of real codewords comes back, the bad parity stays missing."""
    t = tactic("EC12P4")
    monkeypatch.delenv("CFSEC_MIX_MAX_LEN", raising=False)
    rng = np.random.default_rng(12)
    enc = ec.NewEncoder(ec.Config(CodeMode=t))
    lens = [1, 17, 4097, 8193]
    words = []
    for S in lens:
        sh = [Slice.of(rng.integers(0, 256, S, dtype=np.uint8)) for _ in range(t.N)] + \
             [Slice.of(np.zeros(S, np.uint8)) for _ in range(t.M)]
        assert ECOracle.from_tactic(t).encode(sh) == 0
        words.append([s.view().copy() for s in sh])
    bad = [[0], [3, 11], [2, 13], [5]]

    def items():
        out = []
        for w, b in zip(words, bad):
            out.append([torch.from_numpy(rng.integers(0, 256, x.size, dtype=np.uint8) if i in b else x).cuda()
                        for i, x in enumerate(w)])
        return out

    got = items()
    assert enc.ReconstructDataBatch(got, bad) == [0] * len(lens)
    for w, b, it in zip(words, bad, got):
        for i in range(t.N + t.M):
            if i >= t.N and i in b:
                assert it[i].numel() == 0
            else:
                assert np.array_equal(it[i].cpu().numpy(), w[i]), (len(w[0]), i)
    rs = reedsolomon.New(t.N, t.M, device=0)
    got = items()
    for it, b in zip(got, bad):
        for i in b:
            it[i] = None
    assert rs.ReconstructDataStripes(got) == [0] * len(lens)
    for w, b, it in zip(words, bad, got):
        for i in range(t.N + t.M):
            if i >= t.N and i in b:
                assert it[i] is None or it[i].numel() == 0
            else:
                assert np.array_equal(it[i].cpu().numpy(), w[i]), (len(w[0]), i)
