"""The item table of the mixed-plan repair launch of the 16 + 20 code (pack_mix_sv16, engine.hpp /
gf_mix_sv16.hpp), pinned on the CPU: no device, nothing launched.

tests/mix_sv16_plan_driver.cpp links libcfsec.so, builds plans (with their Dy16Plan) and tasks from the
numbers given here (the addresses are made up and never dereferenced), calls pack_mix_sv16 -- the sizing
pass, a pass into a buffer one byte short (nothing may be written) and the real one (nothing may be written
past the size reported) -- and prints the table decoded.  The plans are laid out here as the engine lays
them out for a Reconstruct + Verify of EC16P20 (36 shards) or EC16P20L2's global stripe with its two local
parities as extra rows (38 shards); the expectations are restated from the table's definition: the rule for
taking a task, clause by clause; the inputs in data-row slot order with src[] and the decode rows' columns
permuted to match; the masks; one writer per shard; one coefficient block per plan; tiles of 4096 bytes and
the tile map; the CRC constants against zlib.
"""
import os
import subprocess
import zlib

import pytest

from test_crc_route import CSRC, LIBDIR, ROCM, ROOT, _compiler
from test_mix_crc_plan import BIG, CRC, LENS, TABS, TILE, addrs, mulmod, raw

pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")

NOWORD = 0xFFFFFFFF


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mix_sv16_plan") / "mix_sv16_plan_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "mix_sv16_plan_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


def repair(n, bad, seed, dy=True):
    """The plan of a Reconstruct + Verify of a 36- or 38-shard bid with `bad` missing, as the engine lays it
    out: the first 16 present shards in; the missing data, the missing parity, then the compared parity and
    the extra rows out; the Dy16Plan's rows, src, masks and (20 + e + nd) x 16 made-up coefficient bytes."""
    present = [i not in bad for i in range(36)]
    rin = [i for i in range(36) if present[i]][:16]
    miss_d = [i for i in range(16) if not present[i]]
    miss_p = [i for i in range(16, 36) if not present[i]]
    cmp_p = [i for i in range(16, 36) if present[i] and i not in rin]
    extras = [36, 37] if n == 38 else []
    nd, e = len(miss_d), len(extras)
    src, slot = [], 0
    for i in range(16):
        src.append(slot if present[i] else 16 + len([x for x in miss_d if x < i]))
        slot += present[i]
    d = dict(nd=nd, e=e, rows=miss_d + list(range(16, 36)) + extras, src=src,
             pstore=sum(1 << (i - 16) for i in miss_p),
             pcmp=sum(1 << (i - 16) for i in cmp_p) | sum(1 << (20 + j) for j in range(e)),
             coef=[(seed * 41 + 13 * i + 7) % 256 for i in range((20 + e + nd) * 16)])
    rout = miss_d + miss_p + cmp_p + extras
    return dict(k=16, m=len(rout), nstore=nd + len(miss_p), rin=rin, rout=rout, dy=d if dy else None, n=n)


def generic(k, m, seed):
    """A plan without a dy16 product."""
    return dict(k=k, m=m, nstore=1, rin=list(range(k)), rout=list(range(k, k + m)), dy=None, n=k + m)


def flag_addr(task):
    return 0x7D0000000000 + 4 * (task * 7 + 3)


def pack(driver, max_len, plans, tasks, nwords=1 << 20):
    """tasks: (plan index, len, crc mode[, owner[, crc_word[, remap[, split]]]]); owner defaults to the
    task's index, crc_word to 40 * owner.  Returns (counts, left, head, items, tile map)."""
    text = "mixsv16 %d %d %d %d %d %d\n" % (max_len, nwords, TABS, CRC, len(plans), len(tasks))
    for p in plans:
        f = [p["k"], p["m"], p["nstore"], int(p["dy"] is not None)] + p["rin"] + p["rout"]
        if p["dy"]:
            d = p["dy"]
            f += [d["nd"], d["e"], d["pstore"], d["pcmp"]] + d["src"] + d["rows"] + d["coef"]
        text += " ".join(map(str, f)) + "\n"
    for i, t in enumerate(tasks):
        p, ln, crc = t[:3]
        owner = t[3] if len(t) > 3 else i
        word = t[4] if len(t) > 4 else 40 * owner
        remap = t[5] if len(t) > 5 else 0
        split = t[6] if len(t) > 6 else 0
        text += "%d %d %d %d %d %d %d %d %s\n" % (p, ln, crc, owner, word, remap, split, flag_addr(i),
                                                  " ".join(map(str, addrs(i, plans[p]["k"] + plans[p]["m"]))))
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
            items.append(dict(len=f[0], coef=f[1], tile0=f[2], ntiles=f[3], fin=f[4], gend=f[5], flag=f[6], nd=f[7],
                              e=f[8], pstore=f[9], pcmp=f[10], src=f[11:15], rows=[int(x) for x in b.split()],
                              words=[int(x) for x in w.split()], bytes=[int(x) for x in c.split()]))
        elif line.startswith("map"):
            tmap = [int(x) for x in line.split()[1:]]
    assert len(items) == counts["items"] and len(tmap) == counts["tiles"]
    return counts, left, hd, items, tmap


def slot_cols(d):
    """Slot i's place among the plan's inputs: data row i's own, or the j-th stand-in's for missing row j."""
    return [s if s < 16 else 16 - d["nd"] + (s - 16) for s in d["src"]]


def check_item(it, p, task, word0):
    """One item against its plan, restated from gf_mix_sv16.hpp."""
    d, k = p["dy"], 16
    a = addrs(task, k + p["m"])
    col = slot_cols(d)
    assert sorted(col) == list(range(16))
    assert (it["nd"], it["e"], it["pstore"], it["pcmp"]) == (d["nd"], d["e"], d["pstore"], d["pcmp"])
    assert it["src"][:d["nd"]] == d["rows"][:d["nd"]] and it["src"][d["nd"]:] == [0] * (4 - d["nd"])
    assert it["flag"] == flag_addr(task)
    # the 16 inputs in slot order
    assert it["rows"][:16] == [a[c] for c in col]
    assert it["words"][:16] == [word0 + p["rin"][c] for c in col]
    for i in range(16):  # slot i is data row i, or a parity standing in for it
        shard = p["rin"][col[i]]
        assert shard == i or (shard >= 16 and i in d["rows"][:d["nd"]])
    # then Dy16Plan::rows: touched rows name their address and word, the others neither
    for r, idx in enumerate(d["rows"]):
        used = r < d["nd"] or ((d["pstore"] | d["pcmp"]) >> (r - d["nd"])) & 1
        if used:
            assert it["rows"][16 + r] == a[k + p["rout"].index(idx)]
            assert it["words"][16 + r] == word0 + idx
        else:
            assert (it["rows"][16 + r], it["words"][16 + r]) == (0, NOWORD)
    assert len(it["rows"]) == len(it["words"]) == 16 + len(d["rows"])
    # the coefficient block: parity and extra rows as they are, the decode rows' columns in slot order
    ne = (20 + d["e"]) * 16
    assert it["bytes"][:ne] == d["coef"][:ne]
    for q in range(d["nd"]):
        assert it["bytes"][ne + 16 * q:ne + 16 * q + 16] == [d["coef"][ne + 16 * q + c] for c in col]
    assert len(it["bytes"]) == ne + 16 * d["nd"]


def test_tasks_outside_the_rule_are_left_over(driver):
    ok = repair(38, [0, 1, 16, 17], 1)
    short = repair(38, [3], 2)
    short["rin"], short["k"] = short["rin"][:15], 15          # 15 inputs
    long = repair(38, [3], 3)
    long["rin"], long["k"] = long["rin"] + [35], 17           # 17 inputs
    plans = [ok, repair(38, [0, 1, 16, 17], 4, dy=False), short, long, generic(12, 4, 5)]
    tasks = [(0, 4096, 3),        # in: at the limit (max_len)
             (0, 4097, 3),        # max_len + 1
             (1, 100, 3),         # no dy16 product
             (2, 100, 3),         # 15 inputs
             (3, 100, 3),         # 17 inputs
             (4, 100, 3),         # another code's plan
             (0, 0, 3),           # empty
             (0, 100, 0),         # not checksummed
             (0, 100, 1),         # the stored rows only
             (0, 100, 2),         # inputs and stored rows
             (0, 100, 4),         # an AZ's local pass
             (0, 100, 3, 50),     # two checksummed tasks of one item: neither
             (0, 200, 4, 50),
             (0, 100, 3, 51, 40 * 51, 1),     # an index remap (crc_map)
             (0, 100, 3, 60, 40 * 60, 0, 1),  # the Verify pass of a split Verify
             (0, 100, 3, 61, 40 * 61, 0, 2),  # its store pass
             (0, 1, 3)]           # in
    counts, left, _, items, tmap = pack(driver, 4096, plans, tasks)
    assert left == list(range(1, 16))
    assert [it["len"] for it in items] == [4096, 1] and counts["plans"] == 1 and tmap == [0, 1]
    check_item(items[0], ok, 0, 0)
    check_item(items[1], ok, 16, 40 * 16)
    # a limit of 0 takes nothing, and writes nothing
    counts, left, _, items, _ = pack(driver, 0, plans, tasks)
    assert counts["items"] == 0 and left == list(range(len(tasks))) and items == []


def test_a_task_with_a_word_outside_the_call_is_left_over(driver):
    plans = [repair(38, [3], 1), repair(36, [3], 2)]
    #        38 shards: words [w, w + 38)                       36 shards
    tasks = [(0, 100, 3, 0, 0), (0, 100, 3, 1, 62), (0, 100, 3, 2, 63), (0, 100, 3, 3, -1), (1, 100, 3, 4, 64),
             (1, 100, 3, 5, 65)]
    _, left, _, items, _ = pack(driver, BIG, plans, tasks, nwords=100)
    assert left == [2, 3, 5]
    assert [min(w for w in it["words"] if w != NOWORD) for it in items] == [0, 62, 64]


@pytest.mark.parametrize("bad", [[15], [0], [7, 8], [0, 1, 16, 17], [1, 2, 3, 4], [7, 8, 20, 33], [], [16, 17]])
@pytest.mark.parametrize("n", [36, 38])
def test_stand_ins_sit_in_the_missing_rows_slots(driver, n, bad):
    p = repair(n, bad, 7 + len(bad))
    _, left, _, items, _ = pack(driver, BIG, [p], [(0, 1000, 3), (0, 17, 3, 5, 333)])
    assert left == []
    check_item(items[0], p, 0, 0)
    check_item(items[1], p, 1, 333)
    it, nd = items[0], len([i for i in bad if i < 16])
    standins = [s for s in range(16) if it["words"][s] >= 16]  # slots holding a parity shard
    assert standins == [i for i in bad if i < 16] == it["src"][:nd]
    # the stand-ins are the first parity shards present, in order, one per missing row
    alive = [i for i in range(16, 36) if i not in bad]
    assert [it["words"][s] for s in standins] == alive[:nd]
    assert [it["words"][s] for s in range(16) if s not in standins] == [i for i in range(16) if i not in bad]


@pytest.mark.parametrize("n,bad", [(36, [3]), (38, [0, 1, 16, 17]), (38, []), (36, [0, 5, 15]),
                                   (38, [0, 1, 2, 3] + list(range(16, 32))), (36, [7, 8, 20, 33])])
def test_masks_are_the_plans_and_every_shard_has_one_writer(driver, n, bad):
    p = repair(n, bad, 11)
    _, left, _, items, _ = pack(driver, BIG, [p], [(0, 4097, 3, 9, 1000), (0, 1, 3, 2, 80)])
    assert left == []
    for it, base in zip(items, (1000, 80)):
        assert (it["pstore"], it["pcmp"]) == (p["dy"]["pstore"], p["dy"]["pcmp"])
        writers = sorted(w - base for w in it["words"] if w != NOWORD)
        assert writers == list(range(n)), "a shard without a writer, or with two"
        # the rows the kernel stores are the bad shards, those it compares the parity outside the inputs
        stored = [w - base for r, w in enumerate(it["words"][16:]) if w != NOWORD and
                  (r < it["nd"] or (it["pstore"] >> (r - it["nd"])) & 1)]
        assert sorted(stored) == sorted(bad)


def test_items_sharing_a_plan_share_one_coefficient_block(driver):
    plans = [repair(38, [0, 1, 16, 17], 1), repair(36, [3], 2), repair(38, [1, 2, 3, 4], 3), repair(38, [16, 17], 4),
             repair(38, [0, 1, 16, 17], 1)]
    order = [0, 1, 0, 2, 3, 1, 0, 3, 4]
    counts, left, _, items, _ = pack(driver, BIG, plans, [(p, 1000 + i, 3) for i, p in enumerate(order)])
    assert left == [] and counts["plans"] == 5  # plans are told apart by identity: 0 and 4 hold equal rows
    at = {}
    for i, (it, p) in enumerate(zip(items, order)):
        check_item(it, plans[p], i, 40 * i)
        assert at.setdefault(p, it["coef"]) == it["coef"]  # one copy per plan
    size = lambda p: (20 + plans[p]["dy"]["e"] + plans[p]["dy"]["nd"]) * 16
    spans = sorted((o, o + size(p)) for p, o in at.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "different plans, overlapping coefficient rows"
    assert all(o % 16 == 0 for o in at.values())
    assert spans[-1][1] <= counts["bytes"]


def test_tile_map_and_flag_addresses_follow_the_tasks_taken(driver):
    plans = [repair(38, [0, 1, 16, 17], 1), repair(36, [2, 30], 2)]
    tasks = [(i % 2, ln, 3) for i, ln in enumerate(LENS)]
    tasks.insert(4, (0, 100, 2))  # not taken: the items after it keep their own tasks' flag words
    counts, left, hd, items, tmap = pack(driver, BIG, plans, tasks)
    assert left == [4] and counts["items"] == len(LENS) and counts["plans"] == 2
    assert (hd["tabs"], hd["crc"]) == (TABS, CRC)
    want = [-(-ln // TILE) for ln in LENS]
    assert want == [1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 16]
    assert [it["ntiles"] for it in items] == want and [it["len"] for it in items] == LENS
    assert counts["tiles"] == sum(want)
    assert [(j, t - items[j]["tile0"]) for t, j in enumerate(tmap)] == [(j, q) for j, n in enumerate(want)
                                                                        for q in range(n)]
    taken = [i for i in range(len(tasks)) if i != 4]
    for it, i in zip(items, taken):
        check_item(it, plans[tasks[i][0]], i, 40 * i)


def test_conditioning_and_tile_end_words_match_zlib(driver):
    plans = [repair(36, [3], 1)]
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


def test_item_count_is_not_bounded_by_an_argument_block(driver):
    sets = [[i % 16] + ([16 + i % 20] if i % 3 else []) for i in range(40)]
    plans = [repair(38 if s % 2 else 36, bad, s) for s, bad in enumerate(sets)]
    tasks = [(i % 40, 1 + (i * 977) % 9000, 3) for i in range(1500)]
    counts, left, _, items, tmap = pack(driver, BIG, plans, tasks)
    assert left == [] and counts["items"] == 1500 and counts["plans"] == 40
    assert counts["tiles"] == sum(-(-ln // TILE) for _, ln, _ in tasks)
    assert [j for j, it in enumerate(items) for _ in range(it["ntiles"])] == tmap
    assert [it["flag"] for it in items] == [flag_addr(i) for i in range(1500)]
    assert [it["nd"] for it in items] == [1] * 1500
