"""The case table of tests/repair16_cases.py on the CPU: it reaches every class of the two 16 + 20 repair
kernels' run-time selected code, its restated plan agrees with the sets the suite already pins, and the
oracle alone gives every bid the outcome the GPU sweep (tests/test_gpu_repair16_sweep.py) relies on."""
import pytest

import repair16_cases as R
import varlen_cases as VC

K, M = R.K, R.M


def test_every_class_is_reached():
    cov = R.coverage(R.CASES)
    missing = [name for name in R.REQUIRED if not cov.get(name)]
    assert not missing, missing


@pytest.mark.parametrize("victim,lost", [("nd1-standin7-slot4", {"nd1-standin-7", "nd1-slot-4"}),
                                         ("nd1-standin19-slot15", {"nd1-standin-19", "cmp-0-nd1"}),
                                         ("cmp-3-nd0", {"cmp-3-nd0"}),
                                         ("nd2-standin2+3-slots0+1", {"nd2-sym", "nd2-pair-0", "nd2-standin0-2"}),
                                         ("dy-bytes-nd2", {"dy-bytes-nd2"})])
def test_a_removed_case_is_missed_by_name(victim, lost):
    """The coverage check is live: without the one case that alone holds a class, that class is named."""
    assert victim in R.BY_NAME
    cov = R.coverage([c for c in R.CASES if c.name != victim])
    assert {name for name in R.REQUIRED if not cov.get(name)} == lost


def test_table_limits():
    assert len(R.CASES) <= 130
    keys = [(c.mode, c.verify, c.bad) for c in R.CASES]
    assert len(set(keys)) == len(keys)  # one plan per case: the cases of one call never share a launch group
    for c in R.CASES:
        assert len(c.bad) <= 20 and len(set(c.bad)) == len(c.bad), c.name
        assert all(0 <= i < R.nshards(c) for i in c.bad), c.name
        assert len([i for i in range(K + M) if i not in c.bad]) >= K, c.name
        assert R.classes(c), c.name  # no case without a reason
        assert c.size in (R.S, R.S_SHORT, R.S_BYTES) and R.family(c) in R.FAMILIES
    for name in R.SCATTERED + R.TILES:
        assert R.plan_of(R.BY_NAME[name]).bitsliced, name


def test_known_sets():
    p = R.restate([0, 1, 16, 17], True, 0)  # C5's pattern
    assert (p.nd, p.slot, p.prow) == (2, [0, 1], [2, 3])
    assert p.src == [16, 17] + list(range(14))
    assert R.bits(p.pstore) == [0, 1] and R.bits(p.pcmp) == list(range(4, 20)) and p.dropped == 0
    assert p.takes and p.bitsliced and p.sym and p.eqdiag
    q = R.restate([0, 1, 16, 17], True, 2)
    assert R.bits(q.pcmp) == list(range(4, 22)) and q.pstore == p.pstore and q.takes and q.bitsliced and q.nout == 22
    assert not R.restate([0, 1, 16, 17], True, 0, size=2047).bitsliced
    # the sets of tests/varlen_cases.py
    for name, nd, slot, prow, stored, ncmp in (("repair-nd1", 1, [5], [0], [2], 18), ("repair-nd2", 2, [0, 9], [0, 1], [19], 17),
                                               ("repair-nd0", 0, [], [], [5], 19)):
        c = VC.BY_NAME[name]
        p = R.restate(c.bad, True, 0)
        assert (p.nd, p.slot, p.prow, R.bits(p.pstore), len(R.bits(p.pcmp))) == (nd, slot, prow, stored, ncmp), name
        ins, outs, nstored = VC.rows_of(c)  # plan_stripe as that module restates it
        assert ins[K - nd:] == [K + r for r in prow] and nstored == len(c.bad)
        assert sorted(outs[nstored:]) == [K + r for r in R.bits(p.pcmp)]
        assert VC.repair_nd_e(c) == (p.nd, p.e) and p.takes and p.bitsliced
    p = R.restate([0, 9, 35], True, 0)
    assert p.src == [16, 0, 1, 2, 3, 4, 5, 6, 7, 17, 8, 9, 10, 11, 12, 13] and p.sym is False
    # 5 data rows lost: the product; nd + 7 without Verify: the product; nd + 8: the repair kernel, nothing compared
    assert not R.restate([0, 3, 7, 11, 15], True, 0).takes
    assert not R.restate(list(range(16, 23)), False, 0).takes
    p = R.restate(list(range(16, 24)), False, 0)
    assert p.takes and p.pcmp == 0 and R.bits(p.dropped) == list(range(8, 20))


def test_symmetry_is_what_the_matrix_says():
    """A is symmetric with equal diagonals exactly when prow[0] ^ prow[1] == slot[0] ^ slot[1] and both
    stand-ins are among rows 0..15 (the 16 x 16 dyadic block): read from the matrix, against the rule."""
    seen = set()
    for c in R.CASES:
        p = R.plan_of(c)
        if p.nd == 2:
            rule = p.prow[1] < 16 and p.prow[0] ^ p.prow[1] == p.slot[0] ^ p.slot[1]
            assert (p.sym and p.eqdiag) == rule, c.name
            seen.add(rule)
    assert seen == {True, False}


def test_table_capacity():
    assert [R.tab_capacity(nd, e) for nd, e in ((0, 0), (1, 0), (2, 0), (0, 2), (1, 2), (2, 2))] == [24, 23, 22, 22, 22, 21]


def test_flips_hit_both_sides_of_the_tile_edge():
    bids = R.table_bids()
    at = {(R.family(c), b.kind, b.at) for c in R.CASES for b in bids[c.name] if b.shard is not None and c.size == R.S}
    for fam in ("nd1", "nd2", "cmp-order"):
        for kind in ("compared", "input"):
            assert {a for f, k, a in at if (f, k) == (fam, kind)} == set(R.FLIP_AT), (fam, kind)
    for c in R.CASES:
        kinds = [b.kind for b in bids[c.name]]
        ncmp = len(R.compared_rows(c)) + (2 - sum(i >= K + M for i in c.bad) if c.mode == "lrc" and R.plan_of(c).e == 0 else 0)
        assert kinds[0] == "clean" and kinds.count("compared") == min(ncmp, 3), c.name
        assert kinds.count("input") + kinds.count("blind") == (2 if R.plan_of(c).nd else 1), c.name
        assert ("blind" in kinds) == (ncmp == 0), c.name


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_the_oracle_alone_on_every_bid(fam):
    """Clean bids: status 0 and the codeword back.  A flipped compared row: ErrVerify, the rebuilt shards
    still the codeword's.  A flipped stand-in or data row: ErrVerify where anything is compared, else
    status 0 and rebuilt bytes that are not the codeword's."""
    blind = 0
    for c in R.cases_of(fam):
        for bid, src, status, after in R.results(c):
            R.check_bid(c, bid, src, status, after)
            blind += bid.kind == "blind"
    assert blind or fam in ("lrc", "dyadic")


def test_the_blind_case():
    """One data row and 19 parity rows lost: 16 survivors, nothing to compare; one flipped input returns
    status 0 with bytes that are not the codeword's."""
    c = R.BY_NAME["nd1-standin19-slot15"]
    assert len(c.bad) == 20 and R.plan_of(c).pcmp == 0
    got = [(bid.kind, status) for bid, _, status, _ in R.results(c)]
    assert got == [("clean", 0), ("blind", 0), ("blind", 0)]
