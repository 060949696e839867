"""crc32block framing at its alignment, seam, table and stride edges (crc32block.hip), by design:
tests/crc32block_cases.py holds the case tables and tests/test_crc32block_geometry.py proves on the CPU
that they reach every class of the kernel's per-block geometry.

Every case goes through crc32block.encode_batch / decode_batch with raw pointers into one device pool
per test, filled with 0xA5: objects sit at (first 4096-aligned address) + k * slot + offset, and after
the calls the whole pool must equal an image built on the host -- the oracle's bytes
(oracle.crc32block_encode / crc32block_decode, zlib.crc32) where an object belongs, 0xA5 everywhere
else.  Every comparison is bit-exact.

The stride tests read the launch's grid from CFSEC_TRACE_BLK and assert that every workgroup took at
least two blocks and some a third; test_module_in_child runs the module again under CFSEC_BLK_GRID=0,
the other assignment of blocks to workgroups.
"""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import crc32block_cases as G
from oracle import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CHILD = os.environ.get("CFSEC_BLK_EDGES_CHILD") == "1"
FULL = not os.environ.get("CFSEC_BLK_GRID", "1").startswith("0")  # as blk::launch reads it
CANARY = 0xA5
GAP = 256  # untouched bytes at least between two objects
LAUNCH = re.compile(r"cfsec: blk launch encode=(\d+) objects=(\d+) blocks=(\d+) items=(\d+) grid=(\d+) resident=(\d+)")
OK = 0xFFFFFFFF


@pytest.fixture(scope="module")
def C():
    from chubaofs_amd import crc32block
    return crc32block


def device_bytes(n):
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr()


def upload(t, host):
    t.copy_(torch.from_numpy(host))


def download(t):
    return t.cpu().numpy()


class Words:
    """n device words preset to `fill`."""

    def __init__(self, n, fill):
        self.t = torch.full((n,), fill, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr()

    def get(self):
        return [int(v) for v in download(self.t).view(np.uint32)]


class Pool:
    """`nslots` slots of `slot` bytes from the first 4096-aligned address of one device allocation."""

    def __init__(self, nslots, room):
        self.slot = G.ceil_div(room + G.TILE + GAP, G.TILE) * G.TILE  # any offset < 4096, and the gap
        total = nslots * self.slot + G.TILE
        self.t, ptr = device_bytes(total)
        self.base = -ptr % G.TILE
        self.ptr = ptr
        self.img = np.full(total, CANARY, np.uint8)
        self.free = []  # ranges whose content the contract leaves open

    def at(self, k, off):
        return self.base + k * self.slot + off

    def addr(self, k, off):
        return self.ptr + self.at(k, off)

    def put(self, k, off, data):
        """Bytes that belong at slot k + off: a source before upload(), an expected result after."""
        assert 0 <= off and off + len(data) + GAP <= self.slot
        o = self.at(k, off)
        self.img[o:o + len(data)] = data
        return self.ptr + o

    def open(self, k, off, n):
        self.free.append((self.at(k, off), n))

    def upload(self):
        upload(self.t, self.img)

    def check(self):
        got = download(self.t)
        for o, n in self.free:
            got[o:o + n] = self.img[o:o + n]
        if not np.array_equal(got, self.img):
            i = int(np.flatnonzero(got != self.img)[0])
            k, off = divmod(i - self.base, self.slot)
            raise AssertionError(f"pool byte {i} (slot {k} + {off}) is {got[i]:#x}, expected {self.img[i]:#x}; "
                                 f"{int((got != self.img).sum())} bytes differ")


def payloads(n, size, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, size), dtype=np.uint8)


def crc(a):
    return zlib.crc32(a.tobytes()) & 0xFFFFFFFF


def flip(framed, pos, bit=0x10):
    f = framed.copy()
    f[pos] ^= bit
    return f


def first_bad(framed, size, from_, to, block_len):
    """The word decode_batch must leave: the oracle's first bad block counted from block from / P."""
    b = O.crc32block_decode(framed, size, from_, to, block_len)[1]
    return OK if b < 0 else b - from_ // (block_len - 4)


def trace(capfd):
    return [tuple(map(int, g)) for g in LAUNCH.findall(capfd.readouterr().err)]


# ------------------------------------------------------------------ alignment, whole objects

@pytest.mark.parametrize("block_len,size", G.WHOLE_CASES)
def test_encode_alignment(C, block_len, size):
    """One object per h = (dst + 4) mod 4096 of the table x source misalignment, one launch."""
    objs = G.ENCODE_OBJECTS
    n, flen = len(objs), O.crc32block_encode_size(size, block_len)
    d = payloads(n, size, size ^ block_len)
    pool = Pool(2 * n, flen)
    srcs = [pool.put(2 * i, so, d[i]) for i, (_, so) in enumerate(objs)]
    pool.upload()
    dsts = [pool.put(2 * i + 1, do, O.crc32block_encode(d[i], block_len)) for i, (do, _) in enumerate(objs)]
    assert sorted({(p + 4) % G.TILE for p in dsts}) == G.D
    crcs = Words(n, 7)
    C.encode_batch(srcs, dsts, size, block_len=block_len, shard_crcs_ptr=crcs.ptr)
    assert crcs.get() == [crc(d[i]) for i in range(n)]
    pool.check()


@pytest.mark.parametrize("block_len,size", G.WHOLE_CASES)
def test_decode_alignment_whole(C, block_len, size):
    """Oracle-framed objects at every source misalignment into destinations over the offset table."""
    objs = G.DECODE_OBJECTS
    n, flen = len(objs), O.crc32block_encode_size(size, block_len)
    d = payloads(n, size, size ^ block_len ^ 1)
    pool = Pool(2 * n, flen)
    srcs = [pool.put(2 * i, so, O.crc32block_encode(d[i], block_len)) for i, (_, so) in enumerate(objs)]
    pool.upload()
    dsts = [pool.put(2 * i + 1, do, d[i]) for i, (do, _) in enumerate(objs)]
    assert sorted({p % G.TILE for p in dsts}) == G.D
    bad = Words(n, 0)
    C.decode_batch(srcs, dsts, size, bad.ptr, block_len=block_len)
    assert bad.get() == [OK] * n
    pool.check()


# ------------------------------------------------------------------ decode ranges

def test_decode_ranges(C):
    """Every (from, to) of the table at its four destination offsets, one launch per range; from == to
    also without destinations, and a block that from == to lies inside is still checked."""
    P, size, block_len = G.P4, G.RANGE_SIZE, 4096
    offs, nr = G.RANGE_OFFSETS, len(G.RANGES)
    d = payloads(2, size, 77)
    framed = [O.crc32block_encode(d[0], block_len), O.crc32block_encode(d[1], block_len)]
    nblk = G.ceil_div(size, P)
    pool = Pool(2 + nblk + nr * len(offs), len(framed[0]))
    src = [pool.put(0, 0, framed[0]), pool.put(1, 3, framed[1])]
    # one copy per block with a bit of that block's payload flipped
    broken_h = [flip(framed[0], b * block_len + 4 + 9) for b in range(nblk)]
    broken = [pool.put(2 + b, 5, broken_h[b]) for b in range(nblk)]
    pool.upload()
    inside = 0
    for r, (f, t) in enumerate(G.RANGES):
        which = [(r + j) & 1 for j in range(len(offs))]
        dsts = [pool.put(2 + nblk + r * len(offs) + j, o, d[which[j]][f:t]) for j, o in enumerate(offs)]
        bad = Words(len(offs), 0)
        C.decode_batch([src[w] for w in which], dsts, size, bad.ptr, from_=f, to=t, block_len=block_len)
        assert bad.get() == [OK] * len(offs), (f, t)
        if f == t:
            bad = Words(3, 0)  # no destinations; the middle object's block f / P is broken
            C.decode_batch([src[0], broken[f // P], src[1]], None, size, bad.ptr, from_=f, to=t, block_len=block_len)
            want = [first_bad(fr, size, f, t, block_len) for fr in (framed[0], broken_h[f // P], framed[1])]
            assert bad.get() == want, (f, t)
            if f % P:
                assert want == [OK, 0, OK], (f, t)
                inside += 1
            else:
                assert want == [OK] * 3, (f, t)  # a boundary: no block is read
    assert inside == 4
    pool.check()


# ------------------------------------------------------------------ corruption

def corruption_copies(framed, size, block_len, d0):
    """[(label, framed copy)]: per block one bit flipped in the header, the first and the last payload
    byte, a byte of the previous block's carry region (decode into d0), and pairs of flips."""
    P = block_len - 4
    blocks = G.geometry(P, size, 0, size, d0)
    out = []
    for k in blocks:
        o = k.b * block_len
        spots = {"header": o + 2, "first": o + 4, "last": o + 4 + k.plen - 1}
        if k.w > 0:
            carry = blocks[k.w - 1].send - blocks[k.w - 1].plen
            assert carry > 1, "the destination offset must leave a carry in front of every block"
            spots["carry"] = o + 4 + carry // 2
        if k.w + 1 == len(blocks):
            assert spots["last"] == len(framed) - 1
        for name, pos in spots.items():
            out.append((f"{name} of block {k.b}", flip(framed, pos)))
    nb = len(blocks)
    for b1, b2 in [(0, nb - 1), (1, 2), (nb - 2, nb - 1)]:
        two = flip(flip(framed, b2 * block_len + 4 + 100, 1), b1 * block_len + 1, 0x80)
        out.append((f"blocks {b1} and {b2}", two))
        out.append((f"blocks {b2} and {b1}", flip(flip(framed, b1 * block_len + 4 + 50), b2 * block_len + 3)))
    return out


@pytest.mark.parametrize("block_len,nblk", [(4096, 6), (65536, 3)])
def test_corruption_sweep(C, block_len, nblk):
    P = block_len - 4
    size, d0 = (nblk - 1) * P + 1000, 37
    d = payloads(1, size, block_len + nblk)[0]
    framed = O.crc32block_encode(d, block_len)
    copies = [("clean", framed)] + corruption_copies(framed, size, block_len, d0)
    n = len(copies)
    assert n <= G.SLOTS
    runs = [(0, size), (P + 1, size)]
    pool = Pool(n * (1 + len(runs)), len(framed))
    srcs = [pool.put(i, 11, f) for i, (_, f) in enumerate(copies)]
    pool.upload()
    for r, (f, t) in enumerate(runs):
        b0 = f // P
        want = [first_bad(fr, size, f, t, block_len) for _, fr in copies]
        dsts = []
        for i, (_, fr) in enumerate(copies):
            k = n * (1 + r) + i
            # a clean object byte-exact; a corrupted one may hold anything, inside its own bytes
            dsts.append(pool.put(k, d0, d[f:t]))
            if want[i] != OK:
                pool.open(k, d0, t - f)
        bad = Words(n, 0)
        C.decode_batch(srcs, dsts, size, bad.ptr, from_=f, to=t, block_len=block_len)
        got = bad.get()
        assert got == want, [(copies[i][0], got[i], want[i]) for i in range(n) if got[i] != want[i]]
        # the oracle's index, and with b0 = 1 a flip in block 0 is not seen
        for (label, _), w in zip(copies, want):
            if label == "clean":
                assert w == OK
            elif label.startswith("blocks"):
                lo = min(int(x) for x in re.findall(r"\d+", label) if int(x) >= b0)
                assert w == lo - b0, label
            else:
                b = int(label.split()[-1])
                assert w == (b - b0 if b >= b0 else OK), label
    pool.check()


# ------------------------------------------------------------------ the 128 objects of a launch

@pytest.mark.parametrize("n", [128, 129, 257])
def test_slot_boundary(C, n):
    """Objects of three blocks across the launches of 128: the `bad` and `whole` words advance."""
    block_len, P = 4096, G.P4
    size = 2 * P + 9
    flen = O.crc32block_encode_size(size, block_len)
    d = payloads(n, size, n)
    pool = Pool(3 * n, flen)
    srcs = [pool.put(3 * i, i % 16, d[i]) for i in range(n)]
    pool.upload()
    framed = [O.crc32block_encode(d[i], block_len) for i in range(n)]
    dsts = [pool.put(3 * i + 1, (5 * i) % 64, framed[i]) for i in range(n)]
    crcs = Words(n, 7)
    C.encode_batch(srcs, dsts, size, block_len=block_len, shard_crcs_ptr=crcs.ptr)
    assert crcs.get() == [crc(d[i]) for i in range(n)]
    pool.check()
    # corrupt the device's own framing of objects 127, 128 and n - 1, each in another block
    hit = {}
    for blk, i in enumerate([127, 128, n - 1]):
        if i < n:
            hit.setdefault(i, blk)
    for i, blk in hit.items():
        pos = blk * block_len + (4 + 2000 if blk < 2 else 4 + 8)
        pool.put(3 * i + 1, (5 * i) % 64 + pos, framed[i][pos:pos + 1] ^ 4)
    pool.upload()
    back = []
    for i in range(n):
        back.append(pool.put(3 * i + 2, (7 * i) % 128, d[i]))
        if i in hit:
            pool.open(3 * i + 2, (7 * i) % 128, size)
    bad = Words(n, 0)
    C.decode_batch(dsts, back, size, bad.ptr, block_len=block_len)
    assert bad.get() == [hit.get(i, OK) for i in range(n)]
    pool.check()


# ------------------------------------------------------------------ the whole-object checksum's table

@pytest.mark.parametrize("tail", ["1", "P"])
@pytest.mark.parametrize("nblk", [G.AFTER - 1, G.AFTER, G.AFTER + 1, G.AFTER + 2])
def test_whole_checksum_table_boundary(C, nblk, tail):
    """Around kAfter = 200 blocks: the one-multiply table against the xlast * xpow2 chain."""
    block_len, P = 4096, G.P4
    size = (nblk - 1) * P + (1 if tail == "1" else P)
    assert G.ceil_div(size, P) == nblk
    n, flen = 3, O.crc32block_encode_size(size, block_len)
    d = payloads(n, size, nblk + len(tail))
    pool = Pool(2 * n, flen)
    srcs = [pool.put(2 * i, [0, 9, 15][i], d[i]) for i in range(n)]
    pool.upload()
    dsts = [pool.put(2 * i + 1, [0, 12, 4091][i], O.crc32block_encode(d[i], block_len)) for i in range(n)]
    crcs = Words(n, 7)
    C.encode_batch(srcs, dsts, size, block_len=block_len, shard_crcs_ptr=crcs.ptr)
    assert crcs.get() == [crc(d[i]) for i in range(n)]
    pool.check()


# ------------------------------------------------------------------ the strided loop

def compute_units():
    return torch.cuda.get_device_properties(0).multi_processor_count


def resident_groups(C, capfd):
    """The resident workgroup count the launcher uses, from a one-block launch's trace line."""
    pool = Pool(2, 64)
    src = pool.put(0, 0, np.arange(16, dtype=np.uint8))
    pool.upload()
    capfd.readouterr()
    C.encode_batch([src], [pool.addr(1, 0)], 16, block_len=4096)
    torch.cuda.synchronize()
    ((enc, ny, nb, items, grid, resident),) = trace(capfd)
    assert (enc, ny, nb, items, grid) == (1, 1, 1, 1, 1) and resident > 0
    return resident


def pick_rounds(n, nb, grid):
    """{object: [launch blocks to corrupt]}: work item y * nb + w is of round item // grid.  Three objects
    with one block each of round 0, 1 and >= 2, one object with two blocks (of different rounds where
    an object spans two), then two more objects with one block each; the rest stay clean."""
    rnd = lambda y, w: min((y * nb + w) // grid, 2)  # noqa: E731
    rounds = {y: sorted({rnd(y, w) for w in range(nb)}) for y in range(n)}
    left = lambda: [y for y in range(n) if y not in picks]  # noqa: E731
    picks, seen = {}, set()

    def one(y, r):
        w = next(w for w in range(nb) if rnd(y, w) == r)
        deeper = w + 5 * len(picks)  # not always the block an object or a round begins with
        picks[y] = [deeper if deeper < nb and rnd(y, deeper) == r else w]
        seen.add(r)

    # the round fewest objects hold first, and an object of one round before one that spans two
    for r in sorted(range(3), key=lambda r: sum(r in v for v in rounds.values())):
        one(min((y for y in left() if r in rounds[y]), key=lambda y: len(rounds[y])), r)
    assert seen == {0, 1, 2}
    y = max(left(), key=lambda y: len(rounds[y]))
    picks[y] = [next(w for w in range(nb) if rnd(y, w) == rounds[y][0]), nb - 1]
    for r in (1, 2):
        y = next((y for y in left() if r in rounds[y]), left()[0])
        one(y, r if r in rounds[y] else rounds[y][0])
    assert len(picks) == 6 and len(left()) >= 1
    return picks


def stride_case(C, monkeypatch, capfd, n, nblk, last):
    block_len, P = 4096, G.P4
    size = (nblk - 1) * P + last
    flen = O.crc32block_encode_size(size, block_len)
    d = payloads(n, size, n * nblk)
    framed = [O.crc32block_encode(d[i], block_len) for i in range(n)]
    pool = Pool(3 * n, flen)
    srcs = [pool.put(3 * i, (3 * i) % 16, d[i]) for i in range(n)]
    pool.upload()
    dsts = [pool.put(3 * i + 1, (4 * i + 12) % 32, framed[i]) for i in range(n)]
    crcs = Words(n, 7)
    monkeypatch.setenv("CFSEC_TRACE_BLK", "1")
    capfd.readouterr()
    C.encode_batch(srcs, dsts, size, block_len=block_len, shard_crcs_ptr=crcs.ptr)
    torch.cuda.synchronize()
    ((enc, ny, nb, items, grid, resident),) = trace(capfd)
    assert (enc, ny, nb, items) == (1, n, nblk, n * nblk)
    assert grid == G.expected_grid(items, resident, FULL)
    assert items > 2 * grid  # every workgroup a second block, some a third
    assert crcs.get() == [crc(d[i]) for i in range(n)]
    pool.check()
    # decode what the device framed, blocks of rounds 0, 1 and >= 2 corrupted
    picks = pick_rounds(n, nblk, grid)
    want = [OK] * n
    for y, ws in picks.items():
        f = framed[y].copy()
        for j, w in enumerate(ws):  # a payload byte; of a second block, a header byte
            plen = P if w + 1 < nblk else last
            f[w * block_len + (4 + min(1 + 17 * y, plen - 1) if j == 0 else 1)] ^= 0x40
        pool.put(3 * y + 1, (4 * y + 12) % 32, f)
        want[y] = min(ws)
        assert want[y] == first_bad(f, size, 0, size, block_len), (y, ws)  # the oracle's answer
    pool.upload()
    back = []
    for i in range(n):
        back.append(pool.put(3 * i + 2, (37 * i) % 128, d[i]))
        if i in picks:
            pool.open(3 * i + 2, (37 * i) % 128, size)
    bad = Words(n, 0)
    capfd.readouterr()
    C.decode_batch(dsts, back, size, bad.ptr, block_len=block_len)
    torch.cuda.synchronize()
    ((enc, ny, nb, items2, grid2, resident2),) = trace(capfd)
    assert (enc, ny, nb, items2, grid2, resident2) == (0, n, nblk, items, grid, resident)
    assert bad.get() == want, picks
    pool.check()
    print(f"blk launches: objects={n} blocks={nblk} items={items} grid={grid} resident={resident} full={int(FULL)} "
          f"corrupted={picks}")
    return items, grid, resident


def test_stride_rounds_chain(C, monkeypatch, capfd):
    """7 objects of more than 200 blocks (the xpow2 chain), 16 * CUs + 1 work items at least: object
    boundaries fall inside a round, and every workgroup strides (a CU holds at most 8 workgroups)."""
    monkeypatch.setenv("CFSEC_TRACE_BLK", "1")
    nb = G.ceil_div(16 * compute_units() + 1, 7)
    assert nb > G.AFTER
    items, grid, _ = stride_case(C, monkeypatch, capfd, 7, nb + 1, 77)
    assert items > 16 * compute_units()


def test_stride_rounds_table(C, monkeypatch, capfd):
    """40 objects (more where the device holds more workgroups) of 160 blocks: the xafter table."""
    monkeypatch.setenv("CFSEC_TRACE_BLK", "1")
    resident = resident_groups(C, capfd)
    n = min(G.SLOTS, max(40, 2 * resident // 160 + 1))
    stride_case(C, monkeypatch, capfd, n, 160, 77)


# ------------------------------------------------------------------ the module again under CFSEC_BLK_GRID=0

# Measured on the MI355X: this module in-process (the child excluded, 42 tests) 6.0 s of wall time for
# the whole python process (4.1 s inside pytest), `import torch` 1.7 s; the child gets three times the
# first plus the second.
MODULE_SECONDS = 6.0
IMPORT_SECONDS = 1.7
CHILD_TIMEOUT = 3 * MODULE_SECONDS + IMPORT_SECONDS


@pytest.mark.skipif(CHILD, reason="the child process itself")
def test_module_in_child():
    """This module again with the A/B launch (the fewest workgroups with equal block counts: another
    grid, so another assignment of blocks to workgroups).  A child that ends by a signal, an abort or
    its time limit ends the session: nothing more starts on the GPU after a fault."""
    env = dict(os.environ, CFSEC_BLK_EDGES_CHILD="1", CFSEC_BLK_GRID="0")
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", __file__],
                           env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        pytest.exit(f"CFSEC_BLK_GRID=0: the child ran into its time limit ({CHILD_TIMEOUT:.0f} s)", returncode=3)
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        pytest.exit(f"CFSEC_BLK_GRID=0: the child ended abnormally ({r.returncode})\n" + r.stdout[-2000:] + r.stderr[-2000:],
                    returncode=3)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
    assert " 1 skipped" in r.stdout, r.stdout[-2000:]  # this test alone
