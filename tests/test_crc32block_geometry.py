"""The case tables of tests/crc32block_cases.py reach every class of the framing kernel's geometry
(crc32block.hip make(): destination alignment, tiles, the gc4k entry, decode's seam lines) that
tests/test_gpu_crc32block_edges.py is meant to run -- counted here, on the CPU, from the restated
geometry -- and the restated launch grid on hand-worked answers."""
import pytest

import crc32block_cases as G


def test_geometry_hand_worked():
    P = 4092
    # whole object of 2 blocks + 1 byte into an aligned destination: block 1 lands at 4092, 4 bytes
    # before the line at 4096, and block 0 carries those 4 bytes of block 1
    k0, k1, k2 = G.geometry(P, 2 * P + 1, 0, 2 * P + 1, 0)
    assert (k0.h, k0.tiles, k0.dt, k0.sbeg, k0.send, k0.lim, k0.nx) == (0, 1, 0, 0, P + 4, P - 12, 1)
    assert (k1.h, k1.b16, k1.h4, k1.tiles, k1.dt, k1.sbeg) == (4092, 12, 255, 2, 0, 4)
    # dt: the 16-byte pieces in front of the payload alone push it into another tile
    assert [(k.tiles, k.dt) for k in G.encode_geometry(P, P + 5, 12)] == [(2, 1), (1, 0)]
    assert [(k.tiles, k.dt) for k in G.encode_geometry(P, P + 5, 4091)] == [(2, 0), (2, 1)]
    # block 1 ends at 8184: 8 bytes of line left, the last block has 1 -- the short-block limit
    assert (k1.send - k1.plen, k1.lim, k1.nx) == (1, P - 8, 1)
    assert (k2.plen, k2.last, k2.h, k2.sbeg, k2.send, k2.lim, k2.nx) == (1, 1, 8184 % 4096, 8, 1, 1, 0)
    # a range from inside block 1: out_off is negative, the launch starts at block 1
    assert G.launch_blocks(P, 3 * P, P + 1, 3 * P) == (1, 2)
    (a, b) = G.geometry(P, 3 * P, P + 1, 3 * P, 1)
    assert (a.b, a.h, a.sbeg, b.h) == (1, 0, 0, 4092)
    # from == to: on a block boundary nothing is read, inside a block that block is
    assert G.launch_blocks(P, 3 * P, P, P) == (1, 0) and G.launch_blocks(P, 3 * P, P + 1, P + 1) == (1, 1)
    # encode: every block of an object at the same h
    assert {k.h for k in G.encode_geometry(P, 3 * P + 1, 4091)} == {4095}
    assert [k.plen for k in G.encode_geometry(P, 3 * P + 1, 0)] == [P, P, P, 1]


def test_encode_cases_reach_every_class():
    seen = set()
    for P, size, d0 in G.encode_census_cases():
        seen |= G.encode_classes(P, size, d0)
    assert G.BOTH <= seen, sorted(map(str, G.BOTH - seen))


def test_decode_cases_reach_every_class():
    seen = set()
    for case in G.decode_census_cases():
        seen |= G.decode_classes(*case)
    want = G.BOTH | G.DECODE_ONLY
    assert want <= seen, sorted(map(str, want - seen))


def test_encode_objects_run_h_over_every_offset():
    assert sorted({(d + 4) % G.TILE for d, _ in G.ENCODE_OBJECTS}) == G.D
    assert {s for _, s in G.ENCODE_OBJECTS} == set(G.SRC_OFFSETS) == {s for _, s in G.DECODE_OBJECTS}
    assert len(G.ENCODE_OBJECTS) <= G.SLOTS and len(G.DECODE_OBJECTS) <= G.SLOTS  # one launch per size
    assert all(f <= t <= G.RANGE_SIZE for f, t in G.RANGES) and len(set(G.RANGES)) == len(G.RANGES)


@pytest.mark.parametrize("items,resident,full,grid", [
    (1000, 1280, True, 1000), (1000, 1280, False, 1000),      # below: one block per workgroup either way
    (1280, 1280, True, 1280), (1280, 1280, False, 1280),
    (1281, 1280, True, 1280), (1281, 1280, False, 641),       # above: 2 blocks each needs only 641
    (4109, 1280, True, 1280), (4109, 1280, False, 1028),      # ceil(4109 / 4) = 1028
    (6400, 1280, True, 1280), (6400, 1280, False, 1280),
    (7, 0, True, 7), (7, 0, False, 7),                        # the occupancy query failed
])
def test_expected_grid(items, resident, full, grid):
    assert G.expected_grid(items, resident, full) == grid
    if resident:
        assert grid <= resident and G.ceil_div(items, grid) == G.ceil_div(items, resident)
