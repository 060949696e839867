"""The item table of the mixed-plan launch with checksums (pack_mix_crc, engine.hpp / gf_mix_crc.hpp),
pinned on the CPU: no device, nothing launched.

tests/mix_crc_plan_driver.cpp links libcfsec.so, builds plans and tasks from the numbers given here (the
addresses are made up and never dereferenced), calls pack_mix_crc -- the sizing pass, a pass into a buffer
one byte short (nothing may be written) and the real one (nothing may be written past the size reported)
-- and prints the table decoded.  The expectations are restated here from the table's definition: what
pack_mix pins (tiles of 4096 bytes, the tile map, one copy of a plan's rows, row addresses in plan order),
the rule for taking a task, each row's checksum word (crc_word + shard index), and the CRC constants,
checked against zlib: fin turns a raw CRC into crc32.ChecksumIEEE, gend takes the zero padding of the last
tile out again, xpow2[q] moves a register over 4096 * 2^q bytes.
"""
import os
import subprocess
import zlib

import pytest

from test_crc_route import CSRC, LIBDIR, ROCM, ROOT, _compiler

pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")

TILE = 4096
BIG = 1 << 40  # a length limit that excludes nothing
TABS, CRC = 0x7E0000001000, 0x7E0000100000
POLY = 0xEDB88320


def mulmod(a, b):
    """a * b mod P, reflected (bit 31 = x^0)."""
    p = 0
    for i in range(31, -1, -1):
        if a >> i & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def raw(data):
    """The zero-preset, unconditioned CRC register after `data`: zlib's value less the conditioning."""
    return zlib.crc32(data) ^ zlib.crc32(bytes(len(data)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mix_crc_plan") / "mix_crc_plan_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "mix_crc_plan_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


def plan(k, m, seed, nstore=None, dy16=0, rows_in=None, rows_out=None):
    """(k, m, nstore, dy16, input shard indices, output shard indices, m x k coefficient bytes)."""
    return (k, m, m if nstore is None else nstore, dy16, rows_in or list(range(k)),
            rows_out or list(range(k, k + m)), [(seed * 37 + 11 * i + 1) % 256 for i in range(m * k)])


def addrs(task, nrows):
    """Unrelated, unaligned row addresses, different for every (task, row)."""
    return [0x7F0000000000 + (task * 64 + r) * 0x10000 + (task * 5 + r * 3) % 16 for r in range(nrows)]


def pack(driver, max_len, plans, tasks, nwords=1 << 20):
    """tasks: (plan index, len, crc mode[, owner[, crc_word[, remap]]]); owner defaults to the task's index,
    crc_word to 40 * owner.  Returns (counts, left, head, items, tile map)."""
    text = "mixcrc %d %d %d %d %d %d\n" % (max_len, nwords, TABS, CRC, len(plans), len(tasks))
    for k, m, nstore, dy, rin, rout, coef in plans:
        text += "%d %d %d %d %s\n" % (k, m, nstore, dy, " ".join(map(str, rin + rout + coef)))
    for i, t in enumerate(tasks):
        p, ln, crc = t[:3]
        owner = t[3] if len(t) > 3 else i
        word = t[4] if len(t) > 4 else 40 * owner
        remap = t[5] if len(t) > 5 else 0
        text += "%d %d %d %d %d %d %s\n" % (p, ln, crc, owner, word, remap,
                                            " ".join(map(str, addrs(i, plans[p][0] + plans[p][1]))))
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    head = [int(x) for x in lines[0].split()[1:]]
    counts = dict(items=head[0], tiles=head[1], plans=head[2], bytes=head[3])
    assert head[3] == head[4], "the sizing pass and the packing pass disagree on the table's size"
    left = [int(x) for x in lines[1].split()[1:]]
    hd, items, tmap = None, [], []
    for line in lines[2:]:
        if line.startswith("head"):
            f = [int(x) for x in line.split()[1:]]
            hd = dict(tabs=f[0], crc=f[1], xpow2=f[2:])
        elif line.startswith("item"):
            a, b, w, c = line[5:].split("|")
            f = [int(x) for x in a.split()]
            items.append(dict(len=f[0], k=f[1], m=f[2], coef=f[3], tile0=f[4], ntiles=f[5], fin=f[6], gend=f[7],
                              rows=[int(x) for x in b.split()], words=[int(x) for x in w.split()],
                              bytes=[int(x) for x in c.split()]))
        elif line.startswith("map"):
            tmap = [int(x) for x in line.split()[1:]]
    assert len(items) == counts["items"] and len(tmap) == counts["tiles"]
    return counts, left, hd, items, tmap


LENS = [1, 15, 16, 17, 31, 2048, 4095, 4096, 4097, 8197, 65536]


def test_tile_counts_and_tile_map(driver):
    plans = [plan(6, 2, 1)]
    counts, left, _, items, tmap = pack(driver, BIG, plans, [(0, ln, 2) for ln in LENS])
    assert left == [] and counts["items"] == len(LENS)
    want = [-(-ln // TILE) for ln in LENS]
    assert want == [1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 16]
    assert [it["ntiles"] for it in items] == want
    assert [it["len"] for it in items] == LENS
    assert counts["tiles"] == sum(want)
    expect = [(j, q) for j, n in enumerate(want) for q in range(n)]
    assert [(j, t - items[j]["tile0"]) for t, j in enumerate(tmap)] == expect


def test_word_indices_and_row_addresses(driver):
    # an encode plan (shards 0..k+m-1 in order), a plan whose rows are scattered shard indices, one with no outputs
    plans = [plan(12, 4, 1), plan(3, 2, 2, rows_in=[4, 0, 2], rows_out=[1, 3]), plan(4, 0, 3)]
    tasks = [(0, 4097, 2, 0, 0), (1, 17, 2, 1, 16), (2, 100, 2, 2, 21), (0, 1, 2, 7, 16 * 7)]
    _, left, hd, items, _ = pack(driver, BIG, plans, tasks)
    assert left == []
    assert (hd["tabs"], hd["crc"]) == (TABS, CRC)
    for i, (it, t) in enumerate(zip(items, tasks)):
        k, m, _, _, rin, rout, _ = plans[t[0]]
        assert (it["k"], it["m"]) == (k, m)
        assert it["rows"] == addrs(i, k + m)  # k inputs, then m outputs
        assert it["words"] == [t[4] + s for s in rin + rout]  # crcs[item * n + shard]


def test_conditioning_and_tile_end_words_match_zlib(driver):
    plans = [plan(3, 1, 1)]
    counts, left, hd, items, _ = pack(driver, BIG, plans, [(0, ln, 2) for ln in LENS])
    assert left == []
    for it in items:
        ln = it["len"]
        data = bytes((i * 131 + ln) % 251 for i in range(ln))
        assert it["fin"] == zlib.crc32(bytes(ln)), ln  # raw ^ fin = crc32.ChecksumIEEE
        pad = it["ntiles"] * TILE - ln
        assert 0 <= pad < TILE
        assert mulmod(it["gend"], raw(data + bytes(pad))) == raw(data), ln  # takes the last tile's padding out
    # xpow2[q] = x^(8 * 4096 * 2^q): q = 0..3 against zlib, the rest by squaring
    x = hd["xpow2"]
    assert len(x) == 24
    for q in range(4):
        assert mulmod(x[q], raw(b"cubefs")) == raw(b"cubefs" + bytes(TILE << q))
    assert all(x[q + 1] == mulmod(x[q], x[q]) for q in range(23))


def test_items_sharing_a_plan_share_one_copy_of_its_rows(driver):
    plans = [plan(6, 2, 1), plan(6, 2, 2), plan(12, 1, 3), plan(16, 22, 4), plan(6, 2, 1)]
    order = [0, 1, 0, 2, 3, 1, 0, 3, 4]
    counts, left, _, items, _ = pack(driver, BIG, plans, [(p, 1000 + i, 2) for i, p in enumerate(order)])
    assert left == [] and counts["plans"] == 5  # plans are told apart by identity: 0 and 4 hold equal rows
    at = {}
    for it, p in zip(items, order):
        assert (it["k"], it["m"]) == plans[p][:2]
        assert it["bytes"] == plans[p][6]
        assert at.setdefault(p, it["coef"]) == it["coef"]  # one copy per plan
    spans = sorted((o, o + plans[p][0] * plans[p][1]) for p, o in at.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "different plans, overlapping coefficient rows"
    assert all(o % 16 == 0 for o in at.values())


def test_tasks_outside_the_rule_are_left_over(driver):
    plans = [plan(6, 2, 1), plan(33, 1, 2), plan(32, 1, 3), plan(6, 3, 4, nstore=2), plan(16, 2, 5, dy16=1),
             plan(4, 0, 6)]
    tasks = [(0, 4096, 2),        # in: at the limit
             (0, 4097, 2),        # over the length limit
             (1, 100, 2),         # 33 inputs: more than a launch carries
             (2, 100, 2),         # in: 32 inputs
             (3, 100, 2),         # a compared row: not store-only
             (4, 100, 2),         # a dy16 product
             (0, 100, 0),         # not checksummed
             (0, 100, 1),         # the stored rows only
             (0, 100, 3),         # every row, compared ones too
             (0, 100, 4),         # an AZ's local pass
             (0, 100, 2, 50),     # two checksummed tasks of one item: neither
             (0, 200, 2, 50),
             (0, 100, 2, 51, 40 * 51, 1),  # an index remap
             (5, 100, 2),         # in: no output rows
             (0, 0, 2),           # empty
             (0, 1, 2)]           # in
    counts, left, _, items, tmap = pack(driver, 4096, plans, tasks)
    assert left == [1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14]
    assert [(it["len"], it["k"], it["m"]) for it in items] == [(4096, 6, 2), (100, 32, 1), (100, 4, 0), (1, 6, 2)]
    assert counts["plans"] == 3 and tmap == [0, 1, 2, 3]
    # a limit of 0 takes nothing
    counts, left, _, items, _ = pack(driver, 0, plans, tasks)
    assert counts["items"] == 0 and left == list(range(len(tasks))) and items == []


def test_a_task_with_a_word_outside_the_call_is_left_over(driver):
    plans = [plan(6, 2, 1)]
    tasks = [(0, 100, 2, 0, 0), (0, 100, 2, 1, 8), (0, 100, 2, 2, 9), (0, 100, 2, 3, -1)]
    _, left, _, items, _ = pack(driver, BIG, plans, tasks, nwords=16)
    assert left == [2, 3] and [it["words"][0] for it in items] == [0, 8]


def test_item_count_is_not_bounded_by_an_argument_block(driver):
    plans = [plan(12, 4, s) for s in range(50)]
    tasks = [(i % 50, 1 + (i * 977) % 9000, 2) for i in range(2000)]
    counts, left, _, items, tmap = pack(driver, BIG, plans, tasks)
    assert left == [] and counts["items"] == 2000 and counts["plans"] == 50
    assert counts["tiles"] == sum(-(-ln // TILE) for _, ln, _ in tasks)
    assert [j for j, it in enumerate(items) for _ in range(it["ntiles"])] == tmap
    assert [it["words"] for it in items] == [[40 * i + s for s in range(16)] for i in range(2000)]
