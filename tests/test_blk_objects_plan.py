"""The object table of the mixed-size crc32block launch (pack_blk_objects, crc32block_objects.hpp), pinned
on the CPU: no device, nothing launched.

tests/blk_objects_driver.cpp links libcfsec.so, builds cfsec_blk_object records from the numbers given here
(the addresses are made up and never dereferenced), calls pack_blk_objects -- the sizing pass, a pass into a
buffer one byte short (nothing may be written) and the real one (nothing may be written past the size
reported) -- and prints the table decoded.  The expectations are restated here: the blocks
Decoder.Reader(from, to) touches, the statuses of the single call, one work item per touched block, and
the CRC constants computed from the polynomial by square-and-multiply, not by the library.
"""
import os
import subprocess

import pytest

import crc32block_cases as G
from test_crc_route import CSRC, LIBDIR, ROCM, ROOT, _compiler

pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")

CHECK, DECODE, ENCODE = 0, 1, 2
OK, SHORT, INVALID = 0, 6, 12  # CFSEC_OK, CFSEC_ERR_SHORT_DATA, CFSEC_ERR_INVALID_ARG
BL, P = 4096, G.P4
TILE = 4096


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("blk_objects") / "blk_objects_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-I" + CSRC, os.path.join(ROOT, "tests", "blk_objects_driver.cpp"),
                    "-o", str(exe), "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath," + os.path.join(ROCM, "lib")], check=True, timeout=300)
    return str(exe)


# ---- GF(2)[x] mod the CRC-32 polynomial, reflected: bit 31 is x^0

POLY = 0xEDB88320
X0, X1 = 0x80000000, 0x40000000
ONES = 0xFFFFFFFF


def mulmod(a, b):
    p = 0
    for i in range(32):
        if a & (X0 >> i):
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def xpow(e):
    """x^e, e >= 0, by square-and-multiply."""
    p, base = X0, X1
    while e:
        if e & 1:
            p = mulmod(p, base)
        base = mulmod(base, base)
        e >>= 1
    return p


def fin(n):
    """shift(~0, n) ^ ~0: a raw (zero-preset) CRC of n bytes XOR this is crc32.ChecksumIEEE."""
    return mulmod(xpow(8 * n), ONES) ^ ONES


def test_the_arithmetic_restated_here_is_crc32():
    import zlib
    # ChecksumIEEE(M) = f(0, M) ^ fin(|M|); a message of zero bytes has f(0, M) = 0
    for n in (1, 4, 4092, 65532):
        assert fin(n) == zlib.crc32(bytes(n))


# ---- the driver

def addr(i, off=0):
    return 0x7F0000000000 + i * 0x1000000 + off


def obj(i, size, from_=0, to=None, src_off=0, dst_off=0, src_len=None, src=None, dst=None, bl=BL):
    to = size if to is None else to
    framed = size + 4 * G.ceil_div(size, bl - 4)
    return dict(src=addr(2 * i, src_off) if src is None else src, src_len=framed if src_len is None else src_len,
                dst=addr(2 * i + 1, dst_off) if dst is None else dst, size=size, from_=from_, to=to)


def pack(driver, mode, objs, bl=BL):
    text = "blk %d %d %d\n" % (mode, bl, len(objs))
    for o in objs:
        text += "%d %d %d %d %d %d\n" % (o["src"], o["src_len"], o["dst"], o["size"], o["from_"], o["to"])
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    head = [int(x) for x in lines[0].split()[1:]]
    out = dict(objects=head[0], items=head[1], bytes=head[2], taken=head[4],
               status=[int(x) for x in lines[1].split()[1:]], index=[int(x) for x in lines[2].split()[1:]],
               objs=[], map=[], head=None)
    assert head[2] == head[3], "the sizing pass and the packing pass disagree on the table's size"
    names = "src dst size lo hi b0 nb item0 nblk last_len fin_last whole whole_fin xlast h".split()
    for line in lines[3:]:
        if line.startswith("head"):
            f = [int(x) for x in line.split()[1:]]
            out["head"] = dict(mode=f[0], P=f[1], fin_full=f[2], xpow2=f[3:])
        elif line.startswith("obj"):
            a, b = line[4:].split("|")
            rec = dict(zip(names, (int(x) for x in a.split())))
            rec["g"] = [int(x) for x in b.split()]  # [last][w mod 4][extra tile]
            out["objs"].append(rec)
        elif line.startswith("map"):
            out["map"] = [int(x) for x in line.split()[1:]]
    assert len(out["objs"]) == out["objects"] == len(out["index"]) and len(out["map"]) == out["items"]
    assert len(out["status"]) == out["taken"] == len(objs)
    return out


def touched(size, from_, to, p=P):
    """Decoder.Reader(from, to): (first block, block count); from == to inside a block reads that block."""
    b0 = from_ // p
    b1 = (to - 1) // p if from_ < to else (b0 if from_ % p else b0 - 1)
    return b0, b1 - b0 + 1


def g_at(rec, last, w, dt):
    return rec["g"][(last * 4 + w) * 2 + dt]


# ---- ranges

@pytest.mark.parametrize("mode", [CHECK, DECODE])
def test_launch_range_of_every_table_range(driver, mode):
    objs = [obj(i, G.RANGE_SIZE, f, t, src_off=i % 16, dst_off=(7 * i) % 4096) for i, (f, t) in enumerate(G.RANGES)]
    out = pack(driver, mode, objs)
    assert out["status"] == [OK] * len(objs)
    want = [(i,) + touched(G.RANGE_SIZE, f, t) for i, (f, t) in enumerate(G.RANGES)]
    inside = [(f, t) for f, t in G.RANGES if f == t and f % P]
    assert len(inside) == 4 and all(touched(G.RANGE_SIZE, f, t)[1] == 1 for f, t in inside)
    launched = [(i, b0, nb) for i, b0, nb in want if nb > 0]
    assert len(launched) < len(want)  # from == to on a block boundary: nothing to check
    assert out["index"] == [i for i, _, _ in launched]
    assert [(r["b0"], r["nb"]) for r in out["objs"]] == [(b0, nb) for _, b0, nb in launched]
    for r, (i, _, _) in zip(out["objs"], launched):
        f, t = G.RANGES[i]
        assert r["nblk"] == 4 and r["size"] == G.RANGE_SIZE and r["last_len"] == 77
        assert r["whole"] == int((f, t) == (0, G.RANGE_SIZE))
        assert (r["lo"], r["hi"]) == ((f, t) if mode == DECODE else (0, G.RANGE_SIZE))
        assert r["src"] == objs[i]["src"]
        # decode: the table holds where payload byte 0 would go, so payload byte q goes to dst + q
        assert r["dst"] == (objs[i]["dst"] - f if mode == DECODE else 0)


def test_block_map_and_first_items(driver):
    sizes = [1, P, P + 1, 3 * P + 77, 4 * P, 15]
    out = pack(driver, ENCODE, [obj(i, s) for i, s in enumerate(sizes)])
    nbs = [G.ceil_div(s, P) for s in sizes]
    assert nbs == [1, 1, 2, 4, 4, 1]
    assert [r["nb"] for r in out["objs"]] == nbs and [r["b0"] for r in out["objs"]] == [0] * len(sizes)
    assert [r["item0"] for r in out["objs"]] == [sum(nbs[:j]) for j in range(len(nbs))]
    assert out["map"] == [j for j, nb in enumerate(nbs) for _ in range(nb)]
    assert out["items"] == sum(nbs)
    # every work item resolves to its object and to its block, b0 + item - item0
    decode = pack(driver, DECODE, [obj(0, 4 * P, P + 1, 3 * P), obj(1, 4 * P, 0, 1), obj(2, 4 * P, 3 * P, 4 * P)])
    blocks = [(j, decode["objs"][j]["b0"] + t - decode["objs"][j]["item0"]) for t, j in enumerate(decode["map"])]
    assert blocks == [(0, 1), (0, 2), (1, 0), (2, 3)]


# ---- statuses

@pytest.mark.parametrize("mode", [CHECK, DECODE])
def test_bad_objects_beside_valid_neighbours(driver, mode):
    size = 3 * P + 77
    framed = size + 16
    objs = [obj(0, size),
            obj(1, size, src_len=framed - 1),                    # the last block is cut short
            obj(2, size, 0, 2 * P, src_len=2 * BL),              # ... but not for a range that ends before it
            obj(3, size, 0, 2 * P + 1, src_len=2 * BL),          # one byte more touches the third block
            obj(4, size, 0, size + 1),                           # to > size
            obj(5, size, 5, 4),                                  # from > to
            obj(6, size, -1, 4),
            obj(7, size, dst=0),                                 # NULL dst
            obj(8, size, src=0),                                 # NULL src
            obj(9, -1),
            obj(10, size, 7, 7, dst=0),                          # from == to: no destination needed
            obj(11, size)]
    out = pack(driver, mode, objs)
    null_dst = INVALID if mode == DECODE else OK                 # check ignores dst
    assert out["status"] == [OK, SHORT, OK, SHORT, INVALID, INVALID, INVALID, null_dst, INVALID, INVALID, OK, OK]
    keep = [i for i, s in enumerate(out["status"]) if s == OK]
    assert out["index"] == keep
    nbs = {0: 4, 2: 2, 7: 4, 10: 1, 11: 4}
    assert [r["nb"] for r in out["objs"]] == [nbs[i] for i in keep]
    assert out["map"] == [j for j, i in enumerate(keep) for _ in range(nbs[i])]


def test_encode_statuses(driver):
    objs = [obj(0, 100), obj(1, 100, dst=0), obj(2, 100, src=0), obj(3, -5), obj(4, 100, 9, 3, src_len=0), obj(5, 0, src=0, dst=0)]
    out = pack(driver, ENCODE, objs)
    # from, to and src_len are ignored; a size-0 payload frames to nothing and needs no buffer
    assert out["status"] == [OK, INVALID, INVALID, INVALID, OK, OK]
    assert out["index"] == [0, 4] and out["items"] == 2


@pytest.mark.parametrize("mode", [CHECK, DECODE, ENCODE])
def test_empty_objects_get_no_items(driver, mode):
    objs = [obj(0, 0), obj(1, 0, src=0, dst=0), obj(2, 2 * P, P, P), obj(3, 2 * P, 0, 0), obj(4, 2 * P, 2 * P, 2 * P)]
    out = pack(driver, mode, objs)
    assert out["status"] == [OK] * 5
    if mode == ENCODE:
        assert out["index"] == [2, 3, 4] and out["items"] == 6  # ranges are not encode's
    else:
        assert out["objects"] == 0 and out["items"] == 0 and out["bytes"] == 0 and out["map"] == []
    both = pack(driver, mode, objs + [obj(5, 10)])
    assert both["index"] == ([2, 3, 4, 5] if mode == ENCODE else [5])


def test_object_count_is_not_bounded_by_an_argument_block(driver):
    sizes = [1 + (i * 977) % (5 * P) for i in range(1000)]
    out = pack(driver, CHECK, [obj(i, s, src_off=i % 16) for i, s in enumerate(sizes)])
    assert out["status"] == [OK] * 1000 and out["objects"] == 1000 and out["index"] == list(range(1000))
    nbs = [G.ceil_div(s, P) for s in sizes]
    assert out["items"] == sum(nbs)
    assert out["map"] == [j for j, nb in enumerate(nbs) for _ in range(nb)]
    assert [r["item0"] for r in out["objs"]] == [sum(nbs[:j]) for j in range(1000)]


# ---- constants

def inverse_of(factor, nbytes):
    """factor == x^(-8 nbytes), shown without an inverse: factor * x^(8 nbytes) == x^0."""
    return mulmod(factor, xpow(8 * nbytes)) == X0


def test_head_constants(driver):
    for bl in (4096, 65536):
        out = pack(driver, CHECK, [obj(0, 10, bl=bl)], bl=bl)
        h = out["head"]
        assert h["mode"] == CHECK and h["P"] == bl - 4
        assert h["fin_full"] == fin(bl - 4)
        assert h["xpow2"] == [xpow(8 * (bl - 4) * (1 << i)) for i in range(32)]


SIZES = [1, 15, 16, 17, P - 1, P, P + 1, 3 * P + 1, 3 * P + 77, 4 * P]


@pytest.mark.parametrize("mode", [CHECK, ENCODE])
def test_per_object_constants_one_alignment_per_object(driver, mode):
    offs = [0, 1, 7, 12, 15, 4091, 4092, 4095]
    objs = [obj(i, s, src_off=offs[i % len(offs)], dst_off=offs[(i + 3) % len(offs)]) for i, s in enumerate(SIZES)]
    out = pack(driver, mode, objs)
    assert out["status"] == [OK] * len(objs)
    for r, o, size in zip(out["objs"], objs, SIZES):
        nblk = G.ceil_div(size, P)
        last = size - (nblk - 1) * P
        assert (r["nblk"], r["last_len"]) == (nblk, last)
        assert r["xlast"] == xpow(8 * last) and r["fin_last"] == fin(last)
        assert r["whole"] == 1 and r["whole_fin"] == fin(size)
        # check cuts pieces at the source's 16-byte boundaries, encode tiles at the destination's 4 KiB ones;
        # the payload of every block starts 4 bytes into a block and block_len is a multiple of 4096
        h = (o["src"] + 4) % 16 if mode == CHECK else (o["dst"] + 4) % TILE
        assert r["h"] == h
        assert r["dst"] == (0 if mode == CHECK else o["dst"])
        for i, plen in enumerate((P, last)):
            tiles = G.ceil_div(plen + h, TILE)
            assert inverse_of(g_at(r, i, 0, 0), tiles * TILE - plen - h), (size, h, i)


def test_per_object_constants_decode(driver):
    ranges = [(0, None), (0, None), (5, None), (P, None), (P + 1, 2 * P), (2 * P + 5, None)]
    objs = []
    for i, size in enumerate(SIZES):
        f, t = ranges[i % len(ranges)]
        t = size if t is None else t
        if not (f <= t <= size):
            f, t = 0, size
        objs.append(obj(i, size, f, t, src_off=i % 16, dst_off=[0, 1, 127, 129, 4095][i % 5]))
    out = pack(driver, DECODE, objs)
    assert out["objects"] == len(objs)
    for r, o, size in zip(out["objs"], objs, SIZES):
        nblk = G.ceil_div(size, P)
        last = size - (nblk - 1) * P
        assert r["xlast"] == xpow(8 * last) and r["fin_last"] == fin(last)
        whole = (o["from_"], o["to"]) == (0, size)
        assert r["whole"] == int(whole) and r["whole_fin"] == (fin(size) if whole else 0)
        b0, _ = touched(size, o["from_"], o["to"])
        assert r["b0"] == b0
        for w in range(4):
            # launch block w's payload byte 0 belongs at dst - from + (b0 + w) * P; the table's word covers
            # its misalignment mod 16, the kernel's shift table the rest of it mod 4096
            b16 = (o["dst"] - o["from_"] + (b0 + w) * P) % 16
            for i, plen in enumerate((P, last)):
                for dt in (0, 1):
                    tiles = G.ceil_div(plen + b16, TILE) + dt
                    assert inverse_of(g_at(r, i, w, dt), tiles * TILE - plen - b16), (size, w, i, dt)


def test_constants_at_64k_blocks(driver):
    bl, p = 65536, G.P64
    sizes = [2 * p + 129, 3 * p]
    out = pack(driver, CHECK, [obj(i, s, src_off=3 * i, bl=bl) for i, s in enumerate(sizes)], bl=bl)
    for r, size, i in zip(out["objs"], sizes, range(2)):
        last = size - 2 * p
        assert (r["nblk"], r["nb"], r["last_len"]) == (3, 3, last)
        assert r["xlast"] == xpow(8 * last) and r["fin_last"] == fin(last) and r["whole_fin"] == fin(size)
        h = (addr(2 * i, 3 * i) + 4) % 16
        for k, plen in enumerate((p, last)):
            assert inverse_of(g_at(r, k, 0, 0), G.ceil_div(plen + h, TILE) * TILE - plen - h)
