"""The launch geometry of the standalone CRC32 pass (plan_crc32: kernels.hpp, crc32.hip), pinned on the
CPU: no device, nothing launched.

tests/crc32_plan_driver.cpp prints the library's plans over the case tables of tests/crc32_cases.py and
a wider grid: lengths around every multiple of 16 tiles up to 64 tiles, 273 tiles, 6143..6161 and
6528..6529 tiles, BASELINE C2's 5592406 B and the 2^32 - 1 - 4096 limit, shard counts from 1 to 65536,
affine and pointer-table lists, and workgroup totals 1, 4096 and 2^20.  Asserted:

 (a) every plan equals crc32_cases.plan, the restatement;
 (b) independently of it: the groups' tile ranges partition [0, tiles) with no empty group, groups <=
     384, the constants, pointers and words of a launch fit the 800 flexible words, and the group ends
     are tile ends clipped to the shard's tiles;
 (c) the case tables reach every class the GPU module is meant to run -- every piece() path at every
     pointer-offset class, every (len % 16, length range) cell, the last group equal / shorter / one
     tile / one byte, tpw % 8 and last % 8 in {0, 1, 7, other}, the 384 clamp and both re-roundings,
     slots and slots + 1 at two values of pw, the affine strides and the 65535 / 65536 edge: a class no
     case reaches fails, by name;
 (d) known answers worked out by hand.
"""
import os
import shutil
import subprocess

import pytest

import crc32_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chubaofs_amd", "csrc")
LIBDIR = os.path.join(ROOT, "chubaofs_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

T = G.TILE
NS = [1, 2, 10, 11, 256, 4096, 4097, 65535, 65536]
TOTALS = [1, 4096, 1 << 20]


def grid_lengths():
    out = set(G.ONE_GROUP_LENGTHS + G.MULTI_GROUP_LENGTHS + [G.LIST_LEN, G.LIST5_LEN, G.CAP_LEN, G.PROBE_LEN])
    tiles = {16 * j + d for j in range(1, 5) for d in (-1, 0, 1)} | {273} | set(range(6143, 6162)) | {6528, 6529}
    for t in tiles:
        out |= {(t - 1) * T + 1, t * T - 1, t * T}  # the last tile one byte, one byte short, whole
    return sorted(out | {5592406, G.MAX_LEN})


def grid():
    """(len, n, affine, total): the wider grid, then every table case at its own shard count."""
    cases = {(length, n, aff, total) for length in grid_lengths() for n in NS for total in TOTALS
             for aff in ((0, 1) if 2 <= n <= G.AFFINE_MAX else (0,))}
    cases |= {(length, n, 0, total) for length, n, total in G.group_census()}
    cases |= {(G.LIST_LEN, G.AFFINE_N, 1, G.TOTAL)} | {(G.CAP_LEN, n, int(n <= G.AFFINE_MAX), G.TOTAL) for n in G.CAP_N}
    return sorted(cases)


def _compiler():
    return shutil.which("g++") or shutil.which("hipcc") or shutil.which(os.path.join(ROCM, "bin", "hipcc"))


needs_compiler = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    exe = tmp_path_factory.mktemp("crc32_plan") / "crc32_plan_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "crc32_plan_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFSEC_")}
    text = "".join("%d %d %d %d\n" % c for c in grid())
    r = subprocess.run([str(exe)], input=text, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        v = dict(zip(("tiles", "groups", "tpw", "pw", "slots", "per_launch"), map(int, f[4:10])))
        v["ends"] = [int(x) for x in f[10].split(",")]
        out[tuple(map(int, f[:4]))] = v
    return out


@needs_compiler
def test_plans_are_the_restatement(records):
    assert set(records) == set(grid())
    for key, got in records.items():
        length, n, aff, total = key
        p = G.plan(length, n, bool(aff), total)
        want = dict(tiles=p.tiles, groups=p.groups, tpw=p.tpw, pw=p.pw, slots=p.slots, per_launch=p.per_launch, ends=p.ends)
        assert got == want, key
    assert any(k[0] == G.MAX_LEN for k in records) and any(k[1] == 65536 for k in records)


@needs_compiler
def test_plans_partition_the_tiles(records):
    """(b), from the library's numbers alone."""
    for key, got in records.items():
        length, n, aff, _ = key
        tiles, groups, tpw, pw = got["tiles"], got["groups"], got["tpw"], got["pw"]
        assert tiles * T >= length > (tiles - 1) * T, key
        assert 1 <= groups <= 384 and groups * tpw >= tiles > (groups - 1) * tpw, key  # covered, no empty group
        assert got["ends"] == [min((g + 1) * tpw, tiles) * T for g in range(groups)], key
        assert got["ends"][-1] == tiles * T and got["ends"][-1] - length < T, key
        assert pw >= groups and pw % 2 == 0, key  # the pointers follow the constants, 8-byte aligned
        per = got["per_launch"]
        assert 1 <= per <= n and pw + 3 * (1 if aff else per) <= 800, key
        assert got["slots"] >= 1 and pw + 3 * got["slots"] <= 800 < pw + 3 * (got["slots"] + 1), key
        assert per == (n if aff else min(n, got["slots"])), key
        if tiles >= 16:
            assert tpw >= 16, key  # no workgroup's fixed cost over fewer tiles than that


def missing(want, seen):
    return sorted(map(str, want - seen))


def test_shard_tables_reach_every_class():
    seen = set()
    for length, off in G.shard_census():
        seen |= G.shard_classes(length, off)
    assert G.SHARD_WANT <= seen, missing(G.SHARD_WANT, seen)
    # the backward load over the piece before it: 16 <= len < 32 with a tail, at every offset class
    overlap = {G.offset_class(off) for length, off in G.shard_census() if 16 < length < 32}
    assert overlap == {"16", "4", "odd"}
    assert {G.offset_class(o) for o in G.MULTI_GROUP_OFFSETS} == {"16", "odd"}


def test_group_tables_reach_every_class():
    seen = set()
    for length, n, total in G.group_census():
        seen |= G.group_classes(length, n, total)
    assert G.GROUP_WANT <= seen, missing(G.GROUP_WANT, seen)
    assert ("groups", "one") in seen


def test_list_tables_reach_every_class():
    seen = G.list_classes()
    assert G.LIST_WANT <= seen, missing(G.LIST_WANT, seen)
    assert [len(G.launches(G.CAP_LEN, [16 * i for i in range(n)])) for n in G.CAP_N] == [G.CAP_LAUNCHES[n] for n in G.CAP_N]
    for value, groups, tpw in G.PROBES:
        p = G.plan(G.PROBE_LEN, G.PROBE_N, False, value)
        assert (p.groups, p.tpw) == (groups, tpw), value
    assert {v for v, _, _ in G.PROBES} >= {1, G.PROBE_N, 2 * G.PROBE_N}
    assert any(v // G.PROBE_N > G.plan(G.PROBE_LEN, 1, False).tiles // 16 for v, _, _ in G.PROBES)  # tiles / 16 binds


@pytest.mark.parametrize("length,n,want", [
    (4097, 1, dict(tiles=2, groups=1, tpw=2, pw=2, slots=266)),
    (32 * T - 1, 1, dict(tiles=32, groups=2, tpw=16, pw=2, slots=266)),
    (32 * T + 1, 1, dict(tiles=33, groups=2, tpw=17, ranges=[(0, 17), (17, 33)])),
    (45 * T + 7, 1, dict(tiles=46, groups=2, tpw=23)),
    (46 * T + 7, 1, dict(tiles=47, groups=2, tpw=24, ranges=[(0, 24), (24, 47)])),
    (49 * T - 15, 1, dict(tiles=49, groups=3, tpw=17, ranges=[(0, 17), (17, 34), (34, 49)])),
    (272 * T + 1, 1, dict(tiles=273, groups=17, tpw=17, pw=18, slots=260)),
    (6144 * T, 1, dict(tiles=6144, groups=384, tpw=16, pw=384, slots=138)),
    (6145 * T - 9, 1, dict(tiles=6145, groups=362, tpw=17)),
    (6161 * T - 5, 1, dict(tiles=6161, groups=363, tpw=17)),
    (6529 * T, 1, dict(tiles=6529, groups=363, tpw=18)),
    (349526, 264, dict(tiles=86, groups=5, tpw=18, pw=6, slots=264, per_launch=264)),
    (349526, 265, dict(tiles=86, groups=5, tpw=18, pw=6, slots=264, per_launch=264)),
    (349526, 7, dict(tiles=86, groups=5, tpw=18)),             # tests/test_gpu_crc.py's (7, 349526)
    (5592406, 128, dict(tiles=1366, groups=32, tpw=43)),       # 128 rows of BASELINE C2's length: 32 per row
    (262144, 256, dict(tiles=64, groups=4, tpw=16, pw=4, slots=265)),  # a tasklet's 256 rebuilt rows: one launch
])
def test_known_answers(length, n, want):
    """(d): the restatement on answers worked out by hand (the library equals it: (a))."""
    p = G.plan(length, n, False)
    assert {f: getattr(p, f) for f in want} == want
    assert p.ranges[-1][1] == p.tiles and p.ends[-1] == p.tiles * T


def test_known_lanes_and_launches():
    p = G.plan(272 * T + 1, 1, False)
    assert p.ranges[-1] == (272, 273) and p.last_lanes == [G.BACK] + [G.ZERO] * 255  # one tile of one byte
    assert G.plan(6145 * T - 9, 1, False).ranges[-1] == (6137, 6145) and G.plan(6161 * T - 5, 1, False).ranges[-1] == (6154, 6161)
    assert G.plan(1, 1, False).last_lanes[:2] == [G.BYTES, G.ZERO]
    assert G.plan(17, 1, False).last_lanes[:3] == [G.FULL, G.BACK, G.ZERO]
    assert G.plan(4096, 1, False).last_lanes == [G.FULL] * 256
    assert G.plan(4079, 1, False).last_lanes[253:] == [G.FULL, G.BACK, G.ZERO]
    assert G.plan(4080, 1, False).last_lanes[253:] == [G.FULL, G.FULL, G.ZERO]
    # launches: 533 scattered shards at pw = 2 are 266 + 266 + 1; an equally spaced list is one launch
    scattered = [4352 * i + (i % 3) for i in range(533)]
    assert [(d["s0"], d["shards"], d["affine"]) for d in G.launches(4097, scattered)] == [(0, 266, 0), (266, 266, 0), (532, 1, 0)]
    assert [(d["s0"], d["shards"], d["affine"]) for d in G.launches(4097, [-4352 * i for i in range(7)])] == [(0, 7, 1)]
    assert not G.is_affine([0, 8, 0, 16]) and not G.is_affine([5]) and G.is_affine([9, 2])
    assert not G.is_affine([0, 8, 16], [3, 4, 6]) and G.is_affine([0, 8, 16], [3, 4, 5])
