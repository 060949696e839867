"""The geometry and the case table of tests/varlen_cases.py, checked on the CPU: no device, nothing
launched.

 (a) The tiles.  tests/crc_route_driver.cpp ("matvec" mode, the driver of tests/test_matvec_route.py, given
     one generic matrix per shape of the table) prints plan_matvec's steps: for the runtime-k and fixed-K
     families their `tile` field must be the T restated here, for the lookup family the grid must be
     ceil(tail / T).  The dyadic, dyadic-16 and repair launchers size their own grid from the length (the
     plan's tile field is the fixed-K one there, unused), so their T is restated from DyShape / 256 lanes
     of 4 W bytes alone and the GPU cases at T - 1, T, T + 1 are its check.
 (b) Every case takes the family, mode and chunk it is listed for, in at least two launches, the
     capacity is the restated min(288 / (k + m), 32), and the lengths obey the order the table promises.
 (c) The table reaches every class, per family x mode (a class no case reaches fails by name): a launch
     with s0 > 0; a stripe shorter than a lane chunk next to a longer one; stripes ending at T - 1, T and
     T + 1; a clamped ragged end (an accumulate: the byte tail, which it keeps); the longest stripe of a
     launch not its first; where rows are compared, a corrupted stripe in the second launch whose twin
     index in the first launch is clean, and a corrupted byte-path stripe in the first.  Over the whole
     table (a family's shapes fix which one binds): a capacity bound by the 32 length slots and one bound
     by the 288 pointer slots, and a launch with s0 > 0 without per-stripe lengths.
 (d) The reference alone (the C oracle's Encode / Reconstruct / Verify, ECOracle for the LRC modes), before
     any GPU use: status 0 for every clean stripe, ErrVerify for exactly the corrupted ones, nothing
     written but the lost shards.
"""
import os
import subprocess

import pytest

import matvec_routes as MR
import varlen_cases as V
from test_crc_route import _compiler, driver  # noqa: F401  (the driver fixture: one build per module)
from test_matvec_route import STEP_FIELDS

needs_compiler = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")

VARLEN = [c for c in V.CASES if not c.uniform]
UNIFORM = [c for c in V.CASES if c.uniform]
KEYS = sorted({(c.family, c.mode) for c in VARLEN})


def shapes():
    """(k, m) of every product job of the table."""
    out = set()
    for c in V.CASES:
        if c.family != V.REPAIR:
            ins, outs, _ = V.rows_of(c)
            out.add((len(ins), len(outs)))
    return sorted(out)


@pytest.fixture(scope="module")
def steps(driver):  # noqa: F811
    """Every step the driver plans for a generic matrix of each shape, every mode, length and layout."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFSEC_")}
    r = subprocess.run([driver, "matvec"] + [f"gen:{k}:{m}" for k, m in shapes()], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "mv" and f[8] != "-":
            for s in f[8].split(";"):
                v = s.split(",")
                out.append(dict(zip(STEP_FIELDS, map(int, v[2:])), family=v[0], bs=v[1]))
    return out


@needs_compiler
def test_tiles_are_the_plans(steps):
    pinned = set()
    for c in V.CASES:
        C, T = V.geometry(c.family, c.mode, c.kc, c.mc)
        assert C in (8, 16) and T % C == 0 and 2 * T + 17 < V.MAX_LEN, c.name
        if c.family in (MR.DYADIC, MR.DYADIC16, V.REPAIR):
            continue
        mine = [s for s in steps if (s["family"], s["mode"], s["kc"], s["mc"]) == (c.family, c.mode, c.kc, c.mc)
                and s["bs"] == "none" and 0 < s["tail"] < 2 ** 31]
        assert mine, (c.name, "no such step in the driver's plans")
        if c.family == MR.LOOKUP:
            assert all(s["gx"] == -(-s["tail"] // T) for s in mine), (c.name, T)
            assert {s["tail"] for s in mine} >= {2049, 4097}  # 2048 and 4096 part there
        else:
            assert all(s["tile"] == T for s in mine), (c.name, T, {s["tile"] for s in mine})
            if c.family == MR.RUNTIME_K:
                M, OS = MR.runtime_shape(c.mc)
                assert all((s["M"], s["OS"]) == (M, OS) and s["tile"] == s["threads"] // OS * 16 *
                           (1 if c.mode in (V.STORE, V.ACCUM) else 2) for s in mine), c.name
        pinned.add((c.family, c.mode))
    assert pinned == {(c.family, c.mode) for c in V.CASES if c.family in (MR.FIXED_K, MR.LOOKUP, MR.RUNTIME_K)}
    # the chunk sizes the table names: 8 and 16 bytes in both the fixed-K and the lookup family, 1, 2 and 4 waves
    assert {V.geometry(c.family, c.mode, c.kc, c.mc)[0] for c in V.CASES if c.family == MR.FIXED_K} == {8, 16}
    assert {V.geometry(c.family, c.mode, c.kc, c.mc)[0] for c in V.CASES if c.family == MR.LOOKUP} == {8, 16}
    assert {MR.runtime_shape(c.mc)[1] for c in V.CASES if c.family == MR.RUNTIME_K} == {1, 2, 4}
    assert V.geometry(MR.RUNTIME_K, V.VERIFY, 5, 2) == (16, 128 * 16 * 2)


@pytest.mark.parametrize("c", V.CASES, ids=lambda c: c.name)
def test_case_is_what_the_table_says(c):
    C, T = V.geometry(c.family, c.mode, c.kc, c.mc)
    lens, cap = V.lengths(c), V.capacity(c)
    ins, outs, stored = V.rows_of(c)
    assert len(lens) == cap + V.EXTRA and max(lens) < V.MAX_LEN
    mine = V.primary_steps(c)
    assert [(s["s0"], s["ns"]) for s in mine] == [(0, cap), (cap, V.EXTRA)], (c.name, mine)
    assert all(s["bs"] == "none" and s["prefix"] == 0 for s in V.expected_steps(c))
    assert [s["tail"] for s in mine] == [max(lens[:cap]), max(lens[cap:])]
    if c.family == V.REPAIR:
        nd, e = V.repair_nd_e(c)
        assert len(ins) == 16 and len(outs) == nd + 1 + (19 - nd) + e and 16 * nd + 117 + 16 * e < 16 * len(outs)
        assert cap == min(288 // (16 + nd + 20 + e), 32) and 0 <= nd <= 4
    else:
        assert cap == (288 // (c.kc + c.mc) if c.uniform else min(288 // (c.kc + c.mc), 32))
        assert (c.kc, c.mc) == (len(ins), len(outs)) or c.name in ("store-runtime-4x33-row-chunks", "accum-runtime-33x2")
    if c.name == "accum-runtime-33x2":  # the store chunk: 32 inputs, 288 / 34 = 8 stripes per launch
        assert [(s["mode"], s["kc"], s["ns"]) for s in V.expected_steps(c)] == \
            [(V.STORE, 32, 8)] * 4 + [(V.STORE, 32, 3), (V.ACCUM, 1, 32), (V.ACCUM, 1, 3)]
    if c.uniform:
        assert set(lens) == {T + C - 1}
        at = V.bid_slots(c, len(lens))  # no three bids at one stride: split_runs keeps one run, not affine
        assert all(at[i + 2] - at[i + 1] != at[i + 1] - at[i] for i in range(len(lens) - 2))
    else:
        assert set(lens) <= set(V.edge_lengths(C, T))
        assert lens[cap - 1] < C and lens[cap] == max(lens) == 2 * T + 17 and lens[0] != max(lens[:cap])
        assert all(lens[cap + j] != lens[j] for j in range(V.EXTRA))
    flips = V.corruptions(c)
    assert bool(flips) == (stored < len(outs))
    for s, shard, byte in flips:
        assert shard in outs[stored:] and 0 <= byte < lens[s]
    if flips:
        (s1, _, b1), (s2, _, b2) = flips
        assert s1 < cap <= s2 and b1 == lens[s1] - 1 and b2 == lens[s2] - C
        assert lens[s2] > C and lens[s2] % C and s2 - cap not in [s for s, _, _ in flips]


def classes(c):
    """The classes of the docstring's (c) the case reaches."""
    C, T = V.geometry(c.family, c.mode, c.kc, c.mc)
    lens, cap = V.lengths(c), V.capacity(c)
    out = set()
    for s in V.primary_steps(c):
        run = lens[s["s0"]:s["s0"] + s["ns"]]
        if s["s0"] > 0:
            out.add("s0>0")
        if any((a < C) != (b < C) for a, b in zip(run, run[1:])):
            out.add("shorter than a chunk beside a longer one")
        if run.index(max(run)) > 0:
            out.add("longest not first")
    out |= {"ends at T%+d" % d for d in (-1, 0, 1) if T + d in lens}
    if any(n > C and n % C for n in lens):
        out.add("byte tail kept" if c.mode == V.ACCUM else "clamped ragged end")
    flips = V.corruptions(c)
    if flips:
        if lens[flips[0][0]] < C:
            out.add("corrupted byte-path stripe")
        if flips[1][0] >= cap and flips[1][0] - cap not in [s for s, _, _ in flips]:
            out.add("corrupted in the second launch, twin clean")
    return out


@pytest.mark.parametrize("family,mode", KEYS, ids=lambda v: MR.MODE_NAMES.get(v, v) if isinstance(v, int) else v)
def test_every_class_is_reached(family, mode):
    got = set().union(*[classes(c) for c in VARLEN if (c.family, c.mode) == (family, mode)])
    want = {"s0>0", "shorter than a chunk beside a longer one", "longest not first", "ends at T-1", "ends at T+0",
            "ends at T+1", "byte tail kept" if mode == V.ACCUM else "clamped ragged end"}
    if mode in (V.VERIFY, V.STORE_VERIFY):
        want |= {"corrupted byte-path stripe", "corrupted in the second launch, twin clean"}
    for name in sorted(want):
        assert name in got, f"{family} {MR.MODE_NAMES[mode]}: no case reaches the class '{name}'"


def test_table_wide_classes():
    assert {(f, MR.MODE_NAMES[m]) for f, m in KEYS} == {
        (MR.DYADIC, "store"), (MR.DYADIC, "verify"), (MR.DYADIC16, "store"), (MR.DYADIC16, "verify"),
        (MR.LOOKUP, "store"), (MR.LOOKUP, "verify"), (MR.LOOKUP, "store-verify"), (MR.FIXED_K, "store"),
        (MR.FIXED_K, "verify"), (MR.FIXED_K, "store-verify"), (MR.RUNTIME_K, "store"), (MR.RUNTIME_K, "accum"),
        (MR.RUNTIME_K, "verify"), (MR.RUNTIME_K, "store-verify"), (V.REPAIR, "store-verify")}
    bound = {V.slot_bound(c) for c in VARLEN}
    assert True in bound, "no case whose capacity the 32 length slots bind"
    assert False in bound, "no case whose capacity the 288 pointer slots bind"
    assert {len(V.lengths(c)) for c in VARLEN if V.slot_bound(c)} == {35}
    assert all(10 <= len(V.lengths(c)) <= 29 for c in VARLEN if not V.slot_bound(c))
    assert {V.repair_nd_e(c) for c in V.CASES if c.family == V.REPAIR} == {(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (2, 2)}
    assert sum(c.shift for c in V.CASES) == 2 and {c.mode for c in V.CASES if c.shift} == {V.STORE, V.VERIFY}
    for c in UNIFORM:
        assert "s0>0" in classes(c) and V.capacity(c) == 288 // (c.kc + c.mc) and V.expected_steps(c)[1]["s0"] > 0
    assert {(c.family, c.mode) for c in UNIFORM} == {(MR.DYADIC, V.VERIFY), (MR.FIXED_K, V.STORE_VERIFY),
                                                     (MR.RUNTIME_K, V.VERIFY)}
    # every edge length is run by every family x mode with more than one case or a long table
    for family, mode in KEYS:
        seen = set()
        for c in VARLEN:
            if (c.family, c.mode) == (family, mode):
                C, T = V.geometry(c.family, c.mode, c.kc, c.mc)
                seen |= {V.edge_lengths(C, T).index(n) for n in V.lengths(c)}
        assert len(seen) >= 10, (family, mode, seen)


@pytest.mark.parametrize("c", V.CASES, ids=lambda c: c.name)
def test_reference_alone(c):
    p = V.pool(c)
    p.check_reference()
    assert sum(not x for x in p.clean) == len(V.corruptions(c))
    assert V.ERR_VERIFY == 10
    # the image changes inside the lost shards only: inputs, compared rows and every slack byte stay
    ins, outs, stored = V.rows_of(c)
    lost = outs[:stored] if c.api != "verify" else []
    differs = p.before != p.want
    for s, n in enumerate(p.lens):
        for i in lost:
            differs[p.offset(s, i):p.offset(s, i) + n] = False
    assert not differs.any()
    assert p.pitch == V.round_up(max(p.lens), 256) + 256 and p.before.size == p.want.size
    last = p.offset(len(p.lens) - 1, p.total - 1)
    assert last + p.pitch - 1 <= p.before.size  # a store of the longest length at any shard stays in the pool
