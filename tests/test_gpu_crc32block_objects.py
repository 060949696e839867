"""crc32block over objects of mixed sizes, ranges and alignments in one launch
(cfsec_crc32block_{check,decode,encode}_objects, crc32block_objects.hip) against the oracle
(oracle.crc32block_encode / crc32block_decode, zlib.crc32).  Every comparison is bit-exact.

Objects live in pools filled with 0xA5 -- device memory, page-locked host memory or a plain numpy array --
at (first 4096-aligned address) + k * slot + offset; after a call the whole pool must equal an image built
on the host: the oracle's bytes where an object belongs, 0xA5 everywhere else, so a source that changed or
a byte written outside a destination fails the test.  Launch counts, the grid and the stride rounds are
read from the CFSEC_TRACE_BLK lines.
"""
import ctypes
import re
import zlib

import numpy as np
import pytest

import crc32block_cases as G
from oracle import oracle as O

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CANARY = 0xA5
GAP = 256
OK, SHORT, INVALID, MISMATCH = 0, 6, 12, 16
BL, P = 4096, G.P4
OBJECTS = re.compile(r"cfsec: blk objects mode=(\w+) objects=(\d+) items=(\d+) grid=(\d+) resident=(\d+)")
LAUNCH = re.compile(r"cfsec: blk launch encode=(\d+) objects=(\d+) blocks=(\d+) items=(\d+) grid=(\d+) resident=(\d+)")

SIZES = [0, 1, 15, 16, 17, P - 1, P, P + 1, 3 * P + 1, 3 * P + 77, 4 * P]
SRC_OFFSETS = [0, 1, 7, 15]
DST_OFFSETS = [0, 1, 127, 129, 4095]


@pytest.fixture(scope="module")
def C():
    from chubaofs_amd import crc32block
    return crc32block


@pytest.fixture(scope="module")
def L():
    from chubaofs_amd import _lib
    return _lib


class Pool:
    """`nslots` slots of `slot` bytes from the first 4096-aligned address of one allocation of `kind`:
    "device", "pinned" (cfsec_host_alloc) or "numpy" (pageable)."""

    def __init__(self, nslots, room, kind="device"):
        self.kind = kind
        self.slot = G.ceil_div(room + G.TILE + GAP, G.TILE) * G.TILE  # any offset < 4096, and the gap
        total = nslots * self.slot + G.TILE
        if kind == "device":
            self.t = torch.empty(total, dtype=torch.uint8, device="cuda")
            self.ptr = self.t.data_ptr()
        else:
            from chubaofs_amd import _lib
            self.t = _lib.pinned_empty(total) if kind == "pinned" else np.empty(total, np.uint8)
            self.ptr = self.t.ctypes.data
        self.mem = 1 if kind == "device" else 0
        self.base = -self.ptr % G.TILE
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
        if self.kind == "device":
            self.t.copy_(torch.from_numpy(self.img))
        else:
            self.t[:] = self.img

    def check(self):
        got = self.t.cpu().numpy() if self.kind == "device" else self.t.copy()
        for o, n in self.free:
            got[o:o + n] = self.img[o:o + n]
        if not np.array_equal(got, self.img):
            i = int(np.flatnonzero(got != self.img)[0])
            k, off = divmod(i - self.base, self.slot)
            raise AssertionError(f"pool byte {i} (slot {k} + {off}) is {got[i]:#x}, expected {self.img[i]:#x}; "
                                 f"{int((got != self.img).sum())} bytes differ")


def crc(a):
    return zlib.crc32(a.tobytes()) & 0xFFFFFFFF


def flen(size, bl=BL):
    return O.crc32block_encode_size(size, bl)


def oracle_status(framed, size, f, t, bl=BL):
    """(status, bad_block) of Decoder.Reader(f, t) read to the end."""
    b = O.crc32block_decode(framed, size, f, t, bl)[1]
    return (MISMATCH, b) if b >= 0 else (OK, -1)


def traces(capfd):
    err = capfd.readouterr().err
    return [(m, int(a), int(b), int(c), int(d)) for m, a, b, c, d in OBJECTS.findall(err)], LAUNCH.findall(err)


# ------------------------------------------------------------------ the mixed object set, built once

class Mixed:
    """The issue's sizes x source offsets, whole range, then one object of RANGE_SIZE per table range."""

    def __init__(self):
        rng = np.random.default_rng(0xB10C)
        self.objs = []  # (size, payload, framed, src offset, dst offset, from, to)
        i = 0
        for size in SIZES:
            for so in SRC_OFFSETS:
                d = rng.integers(0, 256, size, dtype=np.uint8)
                self.objs.append((size, d, O.crc32block_encode(d, BL), so, DST_OFFSETS[i % len(DST_OFFSETS)], 0, size))
                i += 1
        self.nwhole = len(self.objs)
        for f, t in G.RANGES:
            d = rng.integers(0, 256, G.RANGE_SIZE, dtype=np.uint8)
            self.objs.append((G.RANGE_SIZE, d, O.crc32block_encode(d, BL), SRC_OFFSETS[i % 4],
                              DST_OFFSETS[i % len(DST_OFFSETS)], f, t))
            i += 1
        self.room = flen(4 * P)

    def whole_crcs(self):
        return [crc(d) if (f, t) == (0, size) else 0 for size, d, _, _, _, f, t in self.objs]


@pytest.fixture(scope="module")
def mixed():
    return Mixed()


def run_check(C, mixed, kind):
    n = len(mixed.objs)
    pool = Pool(n, mixed.room, kind)
    descs = []
    for k, (size, _, framed, so, _, f, t) in enumerate(mixed.objs):
        descs.append((pool.put(k, so, framed), len(framed), 0, size, f, t))
    pool.upload()
    status, bad, crcs = C.objects_call(C.CHECK, descs, BL, mem=pool.mem)
    assert status == [OK] * n and bad == [-1] * n
    assert crcs == mixed.whole_crcs()
    pool.check()  # the sources are byte-identical, nothing around them was written


def run_decode(C, mixed, kind):
    n = len(mixed.objs)
    pool = Pool(2 * n, mixed.room, kind)
    descs = []
    for k, (size, _, framed, so, _, f, t) in enumerate(mixed.objs):
        descs.append([pool.put(2 * k, so, framed), len(framed), 0, size, f, t])
    pool.upload()
    for k, (size, d, _, _, do, f, t) in enumerate(mixed.objs):
        descs[k][2] = pool.put(2 * k + 1, do, d[f:t])
    assert sorted({o[4] for o in mixed.objs}) == sorted(DST_OFFSETS)
    status, bad, crcs = C.objects_call(C.DECODE, descs, BL, mem=pool.mem)
    assert status == [OK] * n and bad == [-1] * n
    assert crcs == mixed.whole_crcs()  # written only for whole-range objects
    pool.check()


def run_encode(C, mixed, kind):
    objs = mixed.objs[:mixed.nwhole]
    n = len(objs)
    pool = Pool(2 * n, mixed.room, kind)
    descs = []
    for k, (size, d, _, so, _, _, _) in enumerate(objs):
        descs.append([pool.put(2 * k, so, d), 0, 0, size, 0, 0])
    pool.upload()
    for k, (size, _, framed, _, do, _, _) in enumerate(objs):
        descs[k][2] = pool.put(2 * k + 1, do, framed)
    status, _, crcs = C.objects_call(C.ENCODE, descs, BL, mem=pool.mem)
    assert status == [OK] * n
    assert crcs == [crc(o[1]) for o in objs]
    pool.check()


def test_check_mixed(C, mixed):
    run_check(C, mixed, "device")


def test_decode_mixed(C, mixed):
    run_decode(C, mixed, "device")


def test_encode_mixed(C, mixed):
    run_encode(C, mixed, "device")


@pytest.mark.parametrize("block_len,sizes", [(64 * 1024, [2 * G.P64 + 129, 3 * G.P64]), (1 << 20, [2 * G.PM + 5])])
def test_large_blocks(C, block_len, sizes):
    """64 KiB blocks, and a block above two rings of tiles: encode, check and decode of the same objects."""
    n = len(sizes)
    rng = np.random.default_rng(block_len)
    d = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    framed = [O.crc32block_encode(x, block_len) for x in d]
    pool = Pool(3 * n, max(len(f) for f in framed))
    srcs = [pool.put(3 * k, [1, 15][k % 2], d[k]) for k in range(n)]
    pool.upload()
    enc = [pool.put(3 * k + 1, [12, 129][k % 2], framed[k]) for k in range(n)]
    status, _, crcs = C.objects_call(C.ENCODE, [(srcs[k], 0, enc[k], sizes[k], 0, 0) for k in range(n)], block_len)
    assert status == [OK] * n and crcs == [crc(x) for x in d]
    pool.check()
    status, bad, crcs = C.objects_call(C.CHECK, [(enc[k], len(framed[k]), 0, sizes[k], 0, sizes[k]) for k in range(n)], block_len)
    assert status == [OK] * n and bad == [-1] * n and crcs == [crc(x) for x in d]
    pb = block_len - 4
    ranges = [(0, sizes[0]), (pb - 1, 2 * pb + 1)][:n]
    back = [pool.put(3 * k + 2, [4095, 127][k % 2], d[k][ranges[k][0]:ranges[k][1]]) for k in range(n)]
    status, bad, crcs = C.objects_call(C.DECODE, [(enc[k], len(framed[k]), back[k], sizes[k]) + ranges[k] for k in range(n)],
                                       block_len)
    assert status == [OK] * n and bad == [-1] * n
    assert crcs == [crc(d[k]) if ranges[k] == (0, sizes[k]) else 0 for k in range(n)]
    pool.check()


# ------------------------------------------------------------------ corruption

def corruption_set():
    """~40 objects: (label, size, payload, framed as stored, from, to).  A payload byte or a stored
    checksum byte flipped in a first, a middle and a last block; two bad blocks in one object; a bad block
    outside the requested range; clean objects in between."""
    rng = np.random.default_rng(0xBAD)
    sizes = [3 * P + 77, 4 * P, 6 * P + 1000, P + 1, 2 * P, 5 * P + 1, 100, 7 * P]
    out = []
    for i in range(40):
        size = sizes[i % len(sizes)]
        nblk = G.ceil_div(size, P)
        d = rng.integers(0, 256, size, dtype=np.uint8)
        f = O.crc32block_encode(d, BL)
        kind = i % 5
        last_len = size - (nblk - 1) * P
        spot = {"first": 0, "middle": nblk // 2, "last": nblk - 1}
        label, rng_ = "clean", (0, size)
        if kind == 1:    # a payload byte
            where = ["first", "middle", "last"][(i // 5) % 3]
            b = spot[where]
            f[b * BL + 4 + min(9 + i, (last_len if b == nblk - 1 else P) - 1)] ^= 0x10
            label = f"payload {where}"
        elif kind == 2:  # a stored checksum byte
            where = ["last", "first", "middle"][(i // 5) % 3]
            f[spot[where] * BL + (i % 4)] ^= 0x01
            label = f"header {where}"
        elif kind == 3 and nblk >= 3:  # two bad blocks: the lower index wins
            f[(nblk - 1) * BL + 4] ^= 0x80
            f[1 * BL + 2] ^= 0x04
            label = "two"
        elif kind == 4 and nblk >= 2:  # block 0 is bad, the range starts in block 1
            f[4 + 3] ^= 0x20
            rng_ = (P + 1, size)
            label = "outside"
        out.append((label, size, d, f, rng_[0], rng_[1]))
    return out


def test_corruption(C, L):
    objs = corruption_set()
    n = len(objs)
    pool = Pool(2 * n, flen(7 * P))
    descs = []
    for k, (_, size, _, f, a, b) in enumerate(objs):
        descs.append([pool.put(2 * k, k % 16, f), len(f), 0, size, a, b])
    pool.upload()
    want = [oracle_status(f, size, a, b) for _, size, _, f, a, b in objs]
    for k, (label, size, d, _, a, b) in enumerate(objs):
        descs[k][2] = pool.put(2 * k + 1, DST_OFFSETS[k % 5], d[a:b])
        if want[k][0] != OK:
            pool.open(2 * k + 1, DST_OFFSETS[k % 5], b - a)  # a corrupted object's bytes are not promised
    labels = [o[0] for o in objs]
    assert {"payload first", "payload middle", "payload last", "header first", "header middle", "header last", "two",
            "outside", "clean"} <= set(labels)
    for (label, size, _, _, _, _), (st, blk) in zip(objs, want):
        nblk = G.ceil_div(size, P)
        if label in ("clean", "outside"):
            assert (st, blk) == (OK, -1), label
        elif label == "two":
            assert (st, blk) == (MISMATCH, 1)
        else:
            assert st == MISMATCH and blk == {"first": 0, "middle": nblk // 2, "last": nblk - 1}[label.split()[1]]
    whole = [crc(d) if w[0] == OK and (a, b) == (0, size) else 0 for (_, size, d, _, a, b), w in zip(objs, want)]
    for mode in (C.CHECK, C.DECODE):
        status, bad, crcs = C.objects_call(mode, descs, BL)
        assert list(zip(status, bad)) == want, [(labels[k], status[k], bad[k], want[k]) for k in range(n)
                                                if (status[k], bad[k]) != want[k]]
        assert crcs == whole
    pool.check()
    # the single call, object by object
    for k, (_, size, _, f, a, b) in enumerate(objs):
        blk = ctypes.c_int64(-7)
        st = L.lib().cfsec_crc32block_decode(descs[k][0], len(f), size, BL, a, b, descs[k][2], ctypes.byref(blk),
                                             L.MEM_DEVICE, -1, None)
        assert (st, blk.value) == want[k], labels[k]
    pool.check()


def test_short_source_and_invalid_range_beside_valid_objects(C):
    size = 3 * P + 77
    rng = np.random.default_rng(5)
    d = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(7)]
    f = [O.crc32block_encode(x, BL) for x in d]
    pool = Pool(14, flen(size))
    src = [pool.put(2 * k, k, f[k]) for k in range(7)]
    pool.upload()
    dst = [pool.addr(2 * k + 1, 3 * k) for k in range(7)]
    descs = [(src[0], len(f[0]), dst[0], size, 0, size),
             (src[1], len(f[1]) - 1, dst[1], size, 0, size),        # short: nothing of it is read or written
             (src[2], 2 * BL, dst[2], size, 5, 2 * P),              # short source, but the range ends before
             (src[3], len(f[3]), dst[3], size, 0, size + 1),        # to > size
             (src[4], len(f[4]), 0, size, 0, size),                 # NULL dst
             (0, len(f[5]), dst[5], size, 0, size),                 # NULL src
             (src[6], len(f[6]), dst[6], size, P, size)]
    for k, (a, b) in {0: (0, size), 2: (5, 2 * P), 6: (P, size)}.items():
        pool.put(2 * k + 1, 3 * k, d[k][a:b])
    status, bad, crcs = C.objects_call(C.DECODE, descs, BL)
    assert status == [OK, SHORT, OK, INVALID, INVALID, INVALID, OK]
    assert bad == [-1] * 7 and crcs == [crc(d[0]), 0, 0, 0, 0, 0, 0]
    pool.check()
    status, bad, crcs = C.objects_call(C.CHECK, descs, BL)
    assert status == [OK, SHORT, OK, INVALID, OK, INVALID, OK]  # check needs no destination
    assert crcs == [crc(d[0]), 0, 0, 0, crc(d[4]), 0, 0]
    pool.check()


def test_call_level_errors(C, L):
    with pytest.raises(L.ErrInvalidBlock):
        C.objects_call(C.CHECK, [(1, 1, 0, 1, 0, 1)], 4095)
    with pytest.raises(L.ErrInvalidBlock):
        C.objects_call(C.ENCODE, [], 0)
    assert C.objects_call(C.DECODE, [], BL) == ([], [], [])
    st = L.lib().cfsec_crc32block_check_objects(None, 3, BL, None, None, None, L.MEM_DEVICE, -1, None)
    assert st == INVALID


# ------------------------------------------------------------------ above kSlots, and the strided loop

def test_300_objects_are_one_launch(C, monkeypatch, capfd):
    n = 300
    assert n > G.SLOTS
    rng = np.random.default_rng(300)
    sizes = [1 + (i * 37) % P for i in range(n)]
    d = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    f = [O.crc32block_encode(x, BL) for x in d]
    for k in (7, 128, 299):
        f[k][4] ^= 1
    pool = Pool(n, flen(P))
    descs = [(pool.put(k, k % 16, f[k]), len(f[k]), 0, sizes[k], 0, sizes[k]) for k in range(n)]
    pool.upload()
    monkeypatch.setenv("CFSEC_TRACE_BLK", "1")
    capfd.readouterr()
    status, bad, crcs = C.objects_call(C.CHECK, descs, BL)
    lines, old = traces(capfd)
    assert len(lines) == 1 and not old
    mode, objects, items, grid, resident = lines[0]
    assert (mode, objects, items) == ("check", n, n) and grid == min(items, resident)
    assert status == [MISMATCH if k in (7, 128, 299) else OK for k in range(n)]
    assert bad == [0 if k in (7, 128, 299) else -1 for k in range(n)]
    assert crcs == [0 if k in (7, 128, 299) else crc(d[k]) for k in range(n)]
    pool.check()


def resident_groups(C, mode, monkeypatch, capfd):
    pool = Pool(2, 64)
    d = np.arange(16, dtype=np.uint8)
    src = pool.put(0, 0, O.crc32block_encode(d, BL) if mode != C.ENCODE else d)
    pool.upload()
    monkeypatch.setenv("CFSEC_TRACE_BLK", "1")
    capfd.readouterr()
    status, _, _ = C.objects_call(mode, [(src, 20, pool.addr(1, 0), 16, 0, 16)], BL)
    (line,), _ = traces(capfd)
    assert status == [OK] and line[1:4] == (1, 1, 1) and line[4] > 0
    return line[4]


def test_stride_rounds(C, monkeypatch, capfd):
    """Enough blocks that every workgroup of the resident grid takes a second one and some a third,
    objects of different block counts so object boundaries fall inside the rounds."""
    resident = max(resident_groups(C, m, monkeypatch, capfd) for m in (C.CHECK, C.DECODE, C.ENCODE))
    n = 23
    per = G.ceil_div(2 * resident + resident // 3, n)
    nbs = [per + (k % 5) for k in range(n)]
    sizes = [(nb - 1) * P + [1, 77, P, 2000, P - 1][k % 5] for k, nb in enumerate(nbs)]
    items = sum(nbs)
    rng = np.random.default_rng(items)
    d = [rng.integers(0, 256, s, dtype=np.uint8) for s in sizes]
    framed = [O.crc32block_encode(x, BL) for x in d]
    pool = Pool(3 * n, max(len(f) for f in framed))
    srcs = [pool.put(3 * k, (3 * k) % 16, d[k]) for k in range(n)]
    pool.upload()
    enc = [pool.put(3 * k + 1, (4 * k + 12) % 32, framed[k]) for k in range(n)]

    def one(mode, descs):
        capfd.readouterr()
        res = C.objects_call(mode, descs, BL)
        (line,), old = traces(capfd)
        assert not old and line[0] == {C.CHECK: "check", C.DECODE: "decode", C.ENCODE: "encode"}[mode]
        assert line[1:3] == (n, items) and line[3] == min(items, line[4])
        assert items > 2 * line[3]  # every workgroup a second block, some a third
        return res, line[3]

    (status, _, crcs), _ = one(C.ENCODE, [(srcs[k], 0, enc[k], sizes[k], 0, 0) for k in range(n)])
    assert status == [OK] * n and crcs == [crc(x) for x in d]
    pool.check()
    whole = [(enc[k], len(framed[k]), 0, sizes[k], 0, sizes[k]) for k in range(n)]
    (status, bad, crcs), grid = one(C.CHECK, whole)
    assert status == [OK] * n and bad == [-1] * n and crcs == [crc(x) for x in d]
    # one block of round 0, 1 and 2 corrupted, each in another object, and the first and last objects
    item0 = [sum(nbs[:k]) for k in range(n)]
    owner = lambda item: max(k for k in range(n) if item0[k] <= item)  # noqa: E731
    hits = {}
    for item in (grid // 2, grid + grid // 3, 2 * grid + 1, 5, items - 1):
        k = owner(item)
        hits.setdefault(k, []).append(item - item0[k])
    assert len(hits) >= 4 and {i // grid for i in (grid // 2, grid + grid // 3, 2 * grid + 1)} == {0, 1, 2}
    for k, blocks in hits.items():
        f = framed[k].copy()
        for j, b in enumerate(blocks):
            f[b * BL + (4 if j == 0 else 1)] ^= 0x40
        pool.put(3 * k + 1, (4 * k + 12) % 32, f)
    pool.upload()
    back = []
    for k in range(n):
        back.append(pool.put(3 * k + 2, (37 * k) % 128, d[k]))
        if k in hits:
            pool.open(3 * k + 2, (37 * k) % 128, sizes[k])
    want = [(MISMATCH, min(hits[k])) if k in hits else (OK, -1) for k in range(n)]
    (status, bad, crcs), _ = one(C.CHECK, whole)
    assert list(zip(status, bad)) == want
    (status, bad, crcs), _ = one(C.DECODE, [(enc[k], len(framed[k]), back[k], sizes[k], 0, sizes[k]) for k in range(n)])
    assert list(zip(status, bad)) == want
    assert crcs == [0 if k in hits else crc(d[k]) for k in range(n)]
    pool.check()


# ------------------------------------------------------------------ host memory

def test_check_mixed_pinned(C, mixed):
    run_check(C, mixed, "pinned")


def test_decode_mixed_pinned(C, mixed):
    run_decode(C, mixed, "pinned")


def test_pinned_objects_run_in_place(C, mixed, monkeypatch, capfd):
    """Page-locked objects are one launch; pageable ones are staged and give the same results."""
    monkeypatch.setenv("CFSEC_TRACE_BLK", "1")
    capfd.readouterr()
    run_check(C, mixed, "pinned")
    lines, _ = traces(capfd)
    launched = sum(1 for o in mixed.objs if G.launch_blocks(P, o[0], o[5], o[6])[1] > 0 and o[0] > 0)
    assert [(ln[0], ln[1]) for ln in lines] == [("check", launched)]


@pytest.mark.parametrize("mode", ["check", "decode", "encode"])
def test_mixed_pageable_staged(C, mixed, mode):
    {"check": run_check, "decode": run_decode, "encode": run_encode}[mode](C, mixed, "numpy")


def test_pageable_objects_beyond_one_staging_run(C, monkeypatch, capfd):
    """Pageable objects are staged in runs of 64 MiB (source and destination bytes together): three objects
    of 17 MiB go one per run, each run its own launch, and every result lands on its own object."""
    bl, n = 1 << 20, 3
    size = 17 * G.PM + 12345
    assert 2 * (2 * size) > (64 << 20) > 2 * size
    rng = np.random.default_rng(64)
    d = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(n)]
    f = [O.crc32block_encode(x, bl) for x in d]
    f[1][5 * bl + 4 + 77] ^= 2
    pool = Pool(2 * n, len(f[0]), "numpy")
    descs = [[pool.put(2 * k, 3 * k + 1, f[k]), len(f[k]), 0, size, 0, size] for k in range(n)]
    pool.upload()
    for k in range(n):
        descs[k][2] = pool.put(2 * k + 1, 129 * k, d[k])
    pool.open(3, 129, size)
    monkeypatch.setenv("CFSEC_TRACE_BLK", "1")
    capfd.readouterr()
    status, bad, crcs = C.objects_call(C.DECODE, descs, bl, mem=0)
    lines, _ = traces(capfd)
    assert [(ln[0], ln[1], ln[2]) for ln in lines] == [("decode", 1, 18)] * 3
    assert status == [OK, MISMATCH, OK] and bad == [-1, 5, -1]
    assert crcs == [crc(d[0]), 0, crc(d[2])]
    pool.check()


# ------------------------------------------------------------------ the existing entry points

def test_existing_entry_points_trace_as_before(C, monkeypatch, capfd):
    size = 3 * G.P64 + 5
    d = torch.arange(size, dtype=torch.int32, device="cuda").to(torch.uint8)
    monkeypatch.setenv("CFSEC_TRACE_BLK", "1")
    capfd.readouterr()
    framed, whole = C.Encode(d)
    new, old = traces(capfd)
    assert not new and len(old) == 1
    enc, ny, nb, items, grid, resident = map(int, old[0])
    assert (enc, ny, nb, items) == (1, 1, 4, 4) and grid == G.expected_grid(4, resident, True) and resident > 0
    assert whole == crc(d.cpu().numpy())
    back = C.Decode(framed, size, G.P64 + 1, size)
    new, old = traces(capfd)
    assert not new and [tuple(map(int, o)) for o in old] == [(0, 1, 3, 3, 3, resident)]
    assert torch.equal(back, d[G.P64 + 1:])
    bad = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.empty(2 * size, dtype=torch.uint8, device="cuda")
    C.decode_batch([framed.data_ptr()] * 2, [out.data_ptr(), out.data_ptr() + size], size, bad.data_ptr())
    torch.cuda.synchronize()
    new, old = traces(capfd)
    assert not new and [tuple(map(int, o)) for o in old] == [(0, 2, 4, 8, 8, resident)]
    assert bad.cpu().numpy().view(np.uint32).tolist() == [0xFFFFFFFF] * 2


# ------------------------------------------------------------------ the array interface

def test_python_objects_interface(C, L):
    rng = np.random.default_rng(9)
    sizes = [0, 100, P, 2 * P + 3]
    d = [torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).cuda() for s in sizes]
    enc = C.EncodeObjects([(x, s) for x, s in zip(d, sizes)], block_len=BL)
    assert [r.status for r in enc] == [OK] * 4 and all(r.err is None and r.ok for r in enc)
    for r, x in zip(enc, d):
        assert np.array_equal(r.dst.cpu().numpy(), O.crc32block_encode(x.cpu().numpy(), BL))
        assert r.crc == crc(x.cpu().numpy())
    broken = enc[3].dst.clone()
    broken[BL + 9] ^= 1
    res = C.CheckObjects([(enc[1].dst, 100), (broken, sizes[3]), (broken, sizes[3], 0, P), (enc[2].dst[:-1], P)],
                         block_len=BL)
    assert [r.status for r in res] == [OK, MISMATCH, OK, SHORT]
    assert isinstance(res[1].err, L.ErrMismatchedCrc) and res[1].err.block == res[1].block == 1
    assert isinstance(res[3].err, L.ErrShortData) and res[0].crc == crc(d[1].cpu().numpy())
    dec = C.DecodeObjects([(enc[3].dst, sizes[3], 5, P + 9), (enc[1].dst, 100, 0, 100)], block_len=BL)
    assert torch.equal(dec[0].dst, d[3][5:P + 9]) and torch.equal(dec[1].dst, d[1])
    assert dec[0].crc == 0 and dec[1].crc == crc(d[1].cpu().numpy())
