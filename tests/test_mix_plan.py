"""The item table of the mixed-plan launch (pack_mix, engine.hpp / gf_mix.hpp), pinned on the CPU: no
device, nothing launched.

tests/mix_plan_driver.cpp links libcfsec.so, builds plans and tasks from the numbers given here (the row
addresses are made up and never dereferenced), calls pack_mix -- the sizing pass, a pass into a buffer
one byte short (nothing may be written) and the real one (nothing may be written past the size reported)
-- and prints the table decoded.  The expectations are restated here from the table's definition: a tile
is 4096 bytes of every row of one item, the tile map names each tile's item, an item's tile index is
tile - tile0, coefficient rows are stored once per plan, row addresses in plan order (in, then out).
"""
import os
import subprocess

import pytest

from test_crc_route import CSRC, LIBDIR, ROCM, ROOT, _compiler

pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")

TILE = 4096
BIG = 1 << 40  # a length limit that excludes nothing


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mix_plan") / "mix_plan_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "mix_plan_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


def plan(k, m, seed, nstore=None, dy16=0):
    """(k, m, nstore, dy16, coefficient bytes): m x k bytes that differ from plan to plan."""
    return (k, m, m if nstore is None else nstore, dy16, [(seed * 37 + 11 * i + 1) % 256 for i in range(m * k)])


def addrs(task, nrows):
    """Unrelated, unaligned row addresses, different for every (task, row)."""
    return [0x7F0000000000 + (task * 64 + r) * 0x10000 + (task * 5 + r * 3) % 16 for r in range(nrows)]


def pack(driver, max_len, plans, tasks):
    """tasks: (plan index, len, crc).  Returns (counts, left, items, tile map)."""
    text = "mix %d %d %d\n" % (max_len, len(plans), len(tasks))
    for k, m, nstore, dy, coef in plans:
        text += "%d %d %d %d %s\n" % (k, m, nstore, dy, " ".join(map(str, coef)))
    for i, (p, ln, crc) in enumerate(tasks):
        text += "%d %d %d %s\n" % (p, ln, crc, " ".join(map(str, addrs(i, plans[p][0] + plans[p][1]))))
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    head = [int(x) for x in lines[0].split()[1:]]
    counts = dict(items=head[0], tiles=head[1], plans=head[2], bytes=head[3])
    assert head[3] == head[4], "the sizing pass and the packing pass disagree on the table's size"
    left = [int(x) for x in lines[1].split()[1:]]
    items, tmap = [], []
    for line in lines[2:]:
        if line.startswith("item"):
            a, b, c = line[5:].split("|")
            f = [int(x) for x in a.split()]
            items.append(dict(len=f[0], k=f[1], m=f[2], coef=f[3], tile0=f[4], ntiles=f[5],
                              rows=[int(x) for x in b.split()], bytes=[int(x) for x in c.split()]))
        elif line.startswith("map"):
            tmap = [int(x) for x in line.split()[1:]]
    assert len(items) == counts["items"] and len(tmap) == counts["tiles"]
    return counts, left, items, tmap


LENS = [1, 15, 16, 17, 4095, 4096, 4097, 12289]


def test_tile_counts_and_tile_map(driver):
    plans = [plan(6, 2, 1)]
    counts, left, items, tmap = pack(driver, BIG, plans, [(0, ln, 0) for ln in LENS])
    assert left == [] and counts["items"] == len(LENS)
    want = [-(-ln // TILE) for ln in LENS]
    assert want == [1, 1, 1, 1, 1, 1, 2, 4]
    assert [it["ntiles"] for it in items] == want
    assert [it["len"] for it in items] == LENS
    assert counts["tiles"] == sum(want)
    # every launch tile resolves to its item and to its index within the item
    expect = [(j, q) for j, n in enumerate(want) for q in range(n)]
    assert [(j, t - items[j]["tile0"]) for t, j in enumerate(tmap)] == expect


def test_items_sharing_a_plan_share_one_copy_of_its_rows(driver):
    plans = [plan(6, 2, 1), plan(6, 2, 2), plan(12, 1, 3), plan(16, 16, 4)]
    order = [0, 1, 0, 2, 3, 1, 0, 3]
    counts, left, items, _ = pack(driver, BIG, plans, [(p, 1000 + i, 0) for i, p in enumerate(order)])
    assert left == [] and counts["plans"] == 4
    at = {}
    for it, p in zip(items, order):
        assert (it["k"], it["m"]) == plans[p][:2]
        assert it["bytes"] == plans[p][4]  # the plan's rows, row-major
        assert at.setdefault(p, it["coef"]) == it["coef"]  # one copy per plan
    spans = sorted((o, o + plans[p][0] * plans[p][1]) for p, o in at.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "different plans, overlapping coefficient rows"
    assert all(o % 16 == 0 for o in at.values())


def test_equal_rows_in_two_plans_are_two_copies(driver):
    # plans are told apart by identity, as make_groups tells them apart
    plans = [plan(6, 2, 1), plan(6, 2, 1)]
    counts, _, items, _ = pack(driver, BIG, plans, [(0, 100, 0), (1, 100, 0)])
    assert counts["plans"] == 2 and items[0]["coef"] != items[1]["coef"] and items[0]["bytes"] == items[1]["bytes"]


def test_row_addresses_in_plan_order(driver):
    plans = [plan(12, 2, 1), plan(6, 5, 2)]
    tasks = [(0, 4097, 0), (1, 17, 0), (0, 1, 0)]
    _, left, items, _ = pack(driver, BIG, plans, tasks)
    assert left == []
    for i, (it, (p, _, _)) in enumerate(zip(items, tasks)):
        assert it["rows"] == addrs(i, plans[p][0] + plans[p][1])  # k inputs, then m outputs


def test_tasks_outside_the_rule_are_left_over(driver):
    plans = [plan(6, 2, 1), plan(33, 1, 2), plan(32, 1, 3), plan(6, 3, 4, nstore=2), plan(16, 2, 5, dy16=1)]
    tasks = [(0, 4096, 0),   # in: at the limit
             (0, 4097, 0),   # over the length limit
             (1, 100, 0),    # 33 inputs: more than a launch carries
             (2, 100, 0),    # in: 32 inputs
             (3, 100, 0),    # a compared row: not store-only
             (4, 100, 0),    # a dy16 product
             (0, 100, 1),    # checksummed
             (0, 1, 0)]      # in
    counts, left, items, tmap = pack(driver, 4096, plans, tasks)
    assert left == [1, 2, 4, 5, 6]
    assert [(it["len"], it["k"]) for it in items] == [(4096, 6), (100, 32), (1, 6)]
    assert counts["plans"] == 2 and tmap == [0, 1, 2]
    # a limit of 0 takes nothing
    counts, left, items, _ = pack(driver, 0, plans, tasks)
    assert counts["items"] == 0 and left == list(range(len(tasks))) and items == []


def test_item_count_is_not_bounded_by_an_argument_block(driver):
    plans = [plan(12, 2, s) for s in range(50)]
    tasks = [(i % 50, 1 + (i * 977) % 9000, 0) for i in range(2000)]
    counts, left, items, tmap = pack(driver, BIG, plans, tasks)
    assert left == [] and counts["items"] == 2000 and counts["plans"] == 50
    assert counts["tiles"] == sum(-(-ln // TILE) for _, ln, _ in tasks)
    assert [j for j, it in enumerate(items) for _ in range(it["ntiles"])] == tmap
