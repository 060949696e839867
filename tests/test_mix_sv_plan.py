"""The item table of the mixed-plan launch that stores, compares and checksums (pack_mix_sv, engine.hpp /
gf_mix_sv.hpp), pinned on the CPU: no device, nothing launched.

tests/mix_sv_plan_driver.cpp links libcfsec.so, builds plans and tasks from the numbers given here (the
addresses are made up and never dereferenced), calls pack_mix_sv -- the sizing pass, a pass into a buffer
one byte short (nothing may be written) and the real one (nothing may be written past the size reported)
-- and prints the table decoded.  The expectations are restated here from the table's definition: the
rule for taking a task, clause by clause; tiles of 4096 bytes and the tile map; per item the plan's nstore
and the address of its Verify word; each row's checksum word (crc_word + shard index); one copy of a
plan's rows; the CRC constants against zlib.
"""
import os
import subprocess
import zlib

import pytest

from test_crc_route import CSRC, LIBDIR, ROCM, ROOT, _compiler
from test_mix_crc_plan import BIG, CRC, LENS, TABS, TILE, addrs, mulmod, plan, raw

pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mix_sv_plan") / "mix_sv_plan_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "mix_sv_plan_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


def flag_addr(task):
    return 0x7D0000000000 + 4 * (task * 7 + 3)


def pack(driver, max_len, plans, tasks, nwords=1 << 20):
    """tasks: (plan index, len, crc mode[, owner[, crc_word[, remap[, split]]]]); owner defaults to the
    task's index, crc_word to 40 * owner.  Returns (counts, left, head, items, tile map)."""
    text = "mixsv %d %d %d %d %d %d\n" % (max_len, nwords, TABS, CRC, len(plans), len(tasks))
    for k, m, nstore, dy, rin, rout, coef in plans:
        text += "%d %d %d %d %s\n" % (k, m, nstore, dy, " ".join(map(str, rin + rout + coef)))
    for i, t in enumerate(tasks):
        p, ln, crc = t[:3]
        owner = t[3] if len(t) > 3 else i
        word = t[4] if len(t) > 4 else 40 * owner
        remap = t[5] if len(t) > 5 else 0
        split = t[6] if len(t) > 6 else 0
        text += "%d %d %d %d %d %d %d %d %s\n" % (p, ln, crc, owner, word, remap, split, flag_addr(i),
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
                              nstore=f[8], flag=f[9], rows=[int(x) for x in b.split()],
                              words=[int(x) for x in w.split()], bytes=[int(x) for x in c.split()]))
        elif line.startswith("map"):
            tmap = [int(x) for x in line.split()[1:]]
    assert len(items) == counts["items"] and len(tmap) == counts["tiles"]
    return counts, left, hd, items, tmap


def test_tile_map_nstore_and_flag_address_per_item(driver):
    # 1 stored + 3 compared; 2 + 4 (the seam inside pass 0); nothing compared; nothing stored; 12 rows
    plans = [plan(12, 4, 1, nstore=1), plan(6, 6, 2, nstore=2), plan(6, 6, 3), plan(6, 6, 4, nstore=0),
             plan(6, 12, 5, nstore=1)]
    tasks = [(i % len(plans), ln, 3) for i, ln in enumerate(LENS)]
    counts, left, hd, items, tmap = pack(driver, BIG, plans, tasks)
    assert left == [] and counts["items"] == len(LENS) and counts["plans"] == len(plans)
    assert (hd["tabs"], hd["crc"]) == (TABS, CRC)
    want = [-(-ln // TILE) for ln in LENS]
    assert want == [1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 16]
    assert [it["ntiles"] for it in items] == want and [it["len"] for it in items] == LENS
    assert counts["tiles"] == sum(want)
    assert [(j, t - items[j]["tile0"]) for t, j in enumerate(tmap)] == [(j, q) for j, n in enumerate(want)
                                                                        for q in range(n)]
    for i, (it, t) in enumerate(zip(items, tasks)):
        k, m, nstore, _, rin, rout, coef = plans[t[0]]
        assert (it["k"], it["m"], it["nstore"]) == (k, m, nstore)
        assert it["flag"] == flag_addr(i)
        assert it["rows"] == addrs(i, k + m)  # k inputs, then m outputs
        assert it["words"] == [40 * i + s for s in rin + rout]  # crcs[item * n + shard]
        assert it["bytes"] == coef


def test_flag_addresses_follow_the_tasks_taken(driver):
    plans = [plan(6, 3, 1, nstore=1)]
    tasks = [(0, 100, 3), (0, 100, 2), (0, 17, 3), (0, 0, 3), (0, 4097, 3)]
    _, left, _, items, _ = pack(driver, BIG, plans, tasks)
    assert left == [1, 3]
    assert [it["flag"] for it in items] == [flag_addr(0), flag_addr(2), flag_addr(4)]


def test_conditioning_and_tile_end_words_match_zlib(driver):
    plans = [plan(3, 2, 1, nstore=1)]
    _, left, hd, items, _ = pack(driver, BIG, plans, [(0, ln, 3) for ln in LENS])
    assert left == []
    for it in items:
        ln = it["len"]
        data = bytes((i * 131 + ln) % 251 for i in range(ln))
        assert it["fin"] == zlib.crc32(bytes(ln)), ln  # raw ^ fin = crc32.ChecksumIEEE
        pad = it["ntiles"] * TILE - ln
        assert 0 <= pad < TILE
        assert mulmod(it["gend"], raw(data + bytes(pad))) == raw(data), ln  # takes the last tile's padding out
    x = hd["xpow2"]
    assert len(x) == 24
    for q in range(4):
        assert mulmod(x[q], raw(b"cubefs")) == raw(b"cubefs" + bytes(TILE << q))
    assert all(x[q + 1] == mulmod(x[q], x[q]) for q in range(23))


def test_items_sharing_a_plan_share_one_copy_of_its_rows(driver):
    plans = [plan(6, 2, 1, nstore=1), plan(6, 2, 2, nstore=0), plan(12, 3, 3, nstore=1), plan(16, 22, 4, nstore=2),
             plan(6, 2, 1, nstore=1)]
    order = [0, 1, 0, 2, 3, 1, 0, 3, 4]
    counts, left, _, items, _ = pack(driver, BIG, plans, [(p, 1000 + i, 3) for i, p in enumerate(order)])
    assert left == [] and counts["plans"] == 5  # plans are told apart by identity: 0 and 4 hold equal rows
    at = {}
    for it, p in zip(items, order):
        assert (it["k"], it["m"], it["nstore"]) == plans[p][:3]
        assert it["bytes"] == plans[p][6]
        assert at.setdefault(p, it["coef"]) == it["coef"]  # one copy per plan
    spans = sorted((o, o + plans[p][0] * plans[p][1]) for p, o in at.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "different plans, overlapping coefficient rows"
    assert all(o % 16 == 0 for o in at.values())


def test_tasks_outside_the_rule_are_left_over(driver):
    plans = [plan(6, 4, 1, nstore=1), plan(33, 2, 2, nstore=1), plan(32, 2, 3, nstore=1), plan(6, 3, 4),
             plan(16, 4, 5, nstore=1, dy16=1), plan(4, 0, 6), plan(6, 3, 7, nstore=0)]
    tasks = [(0, 4096, 3),        # in: at the limit (max_len)
             (0, 4097, 3),        # max_len + 1
             (1, 100, 3),         # 33 inputs: more than a launch carries
             (2, 100, 3),         # in: 32 inputs
             (3, 100, 3),         # in: nothing compared (exactly N survivors)
             (4, 100, 3),         # a dy16 product
             (0, 100, 0),         # not checksummed
             (0, 100, 1),         # the stored rows only
             (0, 100, 2),         # inputs and stored rows
             (0, 100, 4),         # an AZ's local pass
             (0, 100, 3, 50),     # two checksummed tasks of one item: neither
             (0, 200, 4, 50),
             (0, 100, 3, 51, 40 * 51, 1),     # an index remap (crc_map)
             (5, 100, 3),         # no output rows
             (0, 0, 3),           # empty
             (0, 1, 3),           # in
             (0, 100, 3, 60, 40 * 60, 0, 1),  # the Verify pass of a split Verify
             (0, 100, 3, 61, 40 * 61, 0, 2),  # its store pass
             (6, 100, 3)]         # in: nothing stored (nstore = 0)
    counts, left, _, items, tmap = pack(driver, 4096, plans, tasks)
    assert left == [1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 17]
    assert [(it["len"], it["k"], it["m"], it["nstore"]) for it in items] == [
        (4096, 6, 4, 1), (100, 32, 2, 1), (100, 6, 3, 3), (1, 6, 4, 1), (100, 6, 3, 0)]
    assert counts["plans"] == 4 and tmap == [0, 1, 2, 3, 4]
    # a limit of 0 takes nothing, and writes nothing
    counts, left, _, items, _ = pack(driver, 0, plans, tasks)
    assert counts["items"] == 0 and left == list(range(len(tasks))) and items == []


def test_a_task_with_a_word_outside_the_call_is_left_over(driver):
    plans = [plan(6, 2, 1, nstore=1)]
    tasks = [(0, 100, 3, 0, 0), (0, 100, 3, 1, 8), (0, 100, 3, 2, 9), (0, 100, 3, 3, -1)]
    _, left, _, items, _ = pack(driver, BIG, plans, tasks, nwords=16)
    assert left == [2, 3] and [it["words"][0] for it in items] == [0, 8]


def test_item_count_is_not_bounded_by_an_argument_block(driver):
    plans = [plan(12, 4, s, nstore=s % 5) for s in range(50)]
    tasks = [(i % 50, 1 + (i * 977) % 9000, 3) for i in range(2000)]
    counts, left, _, items, tmap = pack(driver, BIG, plans, tasks)
    assert left == [] and counts["items"] == 2000 and counts["plans"] == 50
    assert counts["tiles"] == sum(-(-ln // TILE) for _, ln, _ in tasks)
    assert [j for j, it in enumerate(items) for _ in range(it["ntiles"])] == tmap
    assert [it["nstore"] for it in items] == [(i % 50) % 5 for i in range(2000)]
    assert [it["flag"] for it in items] == [flag_addr(i) for i in range(2000)]
