"""The standalone CRC32 pass's launch geometry, restated from chubaofs_amd/csrc/crc32.hip (plan_crc32,
launch_crc32_to's affine detection and launch loop, crc32_horner_kernel's tile ranges and piece()) without
calling the library, and the case tables aimed at its group, tail and launch-split edges.
tests/test_crc32_geometry.py asserts on the CPU that the library's plan equals this restatement and
that the tables reach every class of the geometry; tests/test_gpu_crc32_edges.py runs them on the GPU
against zlib and the oracle."""
import collections

TILE = 4096          # bytes of a shard per tile (crcdev::kTile)
LANE = 16            # bytes of a tile per thread (dev::kLaneBytes), 256 threads
MAX_GROUPS = 384     # group constants of an argument block (crcdev::kMaxGroups)
FLEX = 800           # flexible words of the argument block (kFlexWords)
TOTAL = 4096         # workgroups aimed at over a list (CFSEC_CRC32_GROUPS_PROBE overrides it)
MIN_TPW = 16         # tiles a workgroup folds at least, where the shard has them
AHEAD = 8            # tiles whose loads are in flight before the fold (CFSEC_CRC_AHEAD)
AFFINE_MAX = 65535   # shards of an affine launch (grid.y)
MAX_LEN = 0xFFFFFFFF - TILE

FULL, BACK, BYTES, ZERO = "ld16", "backward", "bytes", "zero"  # piece(): the three loads, and padding lanes

Plan = collections.namedtuple("Plan", "tiles groups tpw pw slots per_launch ends ranges last_lanes")


def ceil_div(a, b):
    return -(-a // b)


def lane_path(length, off):
    """piece() of the 16 bytes at `off`: the full load, ld_tail_row's backward load of the shard's last
    16 bytes, ld_tail's byte loads (a shard shorter than 16 bytes), or no load past the end."""
    if off + LANE <= length:
        return FULL
    if off >= length:
        return ZERO
    return BYTES if length < LANE else BACK


def plan(length, n, affine, total=TOTAL):
    """plan_crc32: `groups` workgroups of tpw consecutive tiles per shard, per_launch shards per launch.
    ranges: the tiles [t0, t1) of every group; last_lanes: piece()'s path per lane of the last tile."""
    tiles = ceil_div(length, TILE)
    want = max(1, min(total // n, tiles // MIN_TPW))
    groups = min(tiles, want, MAX_GROUPS)
    tpw = ceil_div(tiles, groups)
    groups = ceil_div(tiles, tpw)
    pw = (groups + 1) & ~1
    slots = (FLEX - pw) // 3
    per_launch = n if affine else min(n, slots)
    ranges = [(g * tpw, min((g + 1) * tpw, tiles)) for g in range(groups)]
    lanes = [lane_path(length, (tiles - 1) * TILE + LANE * j) for j in range(TILE // LANE)]
    return Plan(tiles, groups, tpw, pw, slots, per_launch, [t1 * TILE for _, t1 in ranges], ranges, lanes)


def is_affine(ptrs, idx=None):
    """launch_crc32_to: equally spaced pointers (any non-zero stride, two shards always are), consecutive
    words, at most 65535 shards."""
    n = len(ptrs)
    if n < 2 or n > AFFINE_MAX or ptrs[1] == ptrs[0]:
        return False
    stride = ptrs[1] - ptrs[0]
    return all(ptrs[i] - ptrs[0] == stride * i and (idx is None or idx[i] == idx[0] + i) for i in range(1, n))


def launches(length, ptrs, idx=None, total=TOTAL, fin=False):
    """The CFSEC_TRACE_CRC32 lines of one launch_crc32_to call, as dicts of the line's fields."""
    n = len(ptrs)
    aff = is_affine(ptrs, idx)
    p = plan(length, n, aff, total)
    return [dict(len=length, shards=min(p.per_launch, n - s0), s0=s0, tiles=p.tiles, groups=p.groups, tpw=p.tpw,
                 affine=int(aff), idx=int(idx is not None), fin=int(fin)) for s0 in range(0, n, p.per_launch)]


# ---- classes of the geometry, named as test_crc32_geometry.py reports them

def offset_class(off):
    return "16" if off % 16 == 0 else "4" if off % 4 == 0 else "odd"


def mod16_class(length):
    return {0: "0", 1: "1", 15: "15"}.get(length % 16, "mid")


def range_class(length):
    return "<16" if length < 16 else "16..31" if length < 32 else ">=32"


def mod8_class(v):
    return {0: "0", 1: "1", 7: "7"}.get(v % 8, "other")


def shard_classes(length, off, n=1, total=TOTAL):
    """Classes one shard of `length` bytes at pointer offset `off` (from a 256-aligned address) reaches."""
    p = plan(length, n, False, total)
    out = {("cell", mod16_class(length), range_class(length), offset_class(off))}
    out |= {("piece", path, offset_class(off)) for path in set(p.last_lanes) - {ZERO}}
    if p.tiles > 1:
        out.add(("piece", FULL, offset_class(off)))
    if ZERO in p.last_lanes:
        out.add(("padding lanes", offset_class(off)))
    return out


def group_classes(length, n=1, total=TOTAL):
    p = plan(length, n, False, total)
    out = set()
    if p.groups == 1:
        return {("groups", "one")}
    last = p.ranges[-1][1] - p.ranges[-1][0]
    out.add(("last group", "equal" if last == p.tpw else "shorter"))
    if last == 1 and p.tpw > 1:
        out.add(("last group", "one tile"))
        if length - (p.tiles - 1) * TILE == 1:
            out.add(("last group", "one byte"))
    out.add(("tpw % 8", mod8_class(p.tpw)))
    out.add(("last % 8", mod8_class(last)))
    want = max(1, min(total // n, p.tiles // MIN_TPW))
    if want >= MAX_GROUPS:
        if (p.groups, p.tpw) == (MAX_GROUPS, MIN_TPW):
            out.add(("clamp", "384 x 16"))
        if p.tpw == 17 and p.groups == 362:
            out.add(("re-rounding", "362 of 17"))
        if p.tpw == 17 and p.groups == 363:
            out.add(("re-rounding", "363 of 17, last shorter"))
    return out


GROUP_WANT = {("last group", c) for c in ("equal", "shorter", "one tile", "one byte")} \
    | {(f, c) for f in ("tpw % 8", "last % 8") for c in ("0", "1", "7", "other")} \
    | {("clamp", "384 x 16"), ("re-rounding", "362 of 17"), ("re-rounding", "363 of 17, last shorter")}
SHARD_WANT = {("piece", path, o) for path in (FULL, BACK, BYTES) for o in ("16", "4", "odd")} \
    | {("padding lanes", o) for o in ("16", "4", "odd")} \
    | {("cell", m, r, o) for m in ("0", "1", "15", "mid") for r in ("<16", "16..31", ">=32")
       for o in ("16", "4", "odd") if not (m == "0" and r == "<16")}


# ---- the case tables

ONE_GROUP_LENGTHS = [
    1,      # one byte: the byte loads, len % 16 = 1
    3,      # byte loads, a middle remainder
    15,     # byte loads, the longest
    16,     # one full piece, no tail
    17,     # the backward load overlaps 15 bytes of the piece before it
    24,     # 16..31 with a middle remainder: the backward load shifted down by two whole words
    31,     # the backward load overlaps one byte
    32,     # two full pieces
    33,     # the backward load clear of the first piece
    43,     # >= 32 with a middle remainder: shifted down by a word and a byte
    4079,   # the last lane of the tile is the tail lane, 15 bytes
    4080,   # the last lane of the tile is padding
    4081,   # the last lane holds one byte
    4095,   # one byte short of the tile
    4096,   # exactly one tile: no tail, no padding
    4097,   # a second tile of one byte
    8191,   # two tiles, the second one byte short
]
T = TILE
MULTI_GROUP_LENGTHS = [
    32 * T - 1,     # just below the 32-tile edge: one group of 32
    32 * T,         # 2 x 16
    32 * T + 1,     # 17 + 16, the last tile one byte
    45 * T + 7,     # 46 tiles: 23 + 23, tpw % 8 = 7, the last tile 7 bytes
    46 * T + 7,     # 47 tiles: 24 + 23, last % 8 = 7
    47 * T,         # 24 + 23, whole tiles
    49 * T - 15,    # 49 tiles: 3 groups of 17, the last 15
    272 * T + 1,    # 273 tiles: 17 x 17, the last group one tile of one byte
    6144 * T,       # 384 x 16: the clamp
    6145 * T - 9,   # 6145 tiles: 362 groups of 17, the last 8
    6161 * T - 5,   # 6161 tiles: 363 groups of 17, the last 7
]
BIG = [length for length in MULTI_GROUP_LENGTHS if length > (1 << 24)]  # one shard each, about 25 MB
MULTI_GROUP_OFFSETS = [0, 1]

OFFSETS = [
    0,      # 256-aligned
    1,      # odd
    3,      # odd, the byte before a word
    4,      # on a word, off a 16-byte line
    15,     # the byte before a 16-byte line
    16,     # on a 16-byte line, off a 64-byte one
    17,     # the byte after
    255,    # the byte before the next 256
]
# the lengths crossed with every offset: each (len % 16 class) x (len < 16, 16..31, >= 32) cell
OFFSET_LENGTHS = ONE_GROUP_LENGTHS

# pointer-table lists at len = 4097 (one group, pw = 2, 266 shards per launch): one shard, the pair (which
# is always equally spaced), slots, slots + 1, 2 slots + 1
LIST_LEN = 4097
LIST_N = [1, 2, 266, 267, 533]
# five groups (pw = 6, 264 shards per launch) of 86 tiles: slots and slots + 1
LIST5_LEN = 349526
LIST5_N = [264, 265]
# equally spaced lists of 7 shards of 4097 bytes: (name, stride)
AFFINE_N = 7
AFFINE_STRIDES = [
    ("pitched", 4352),      # len rounded up to 256
    ("contiguous", 4097),   # ec.Buffer's layout: stride == an odd len, every shard at another alignment
    ("descending", -4352),  # a negative stride
]
# the grid.y cap: 65535 shards of 16 bytes 16 apart are one launch, 65536 fall back to pointer tables
CAP_LEN = 16
CAP_N = [65535, 65536]
CAP_LAUNCHES = {65535: 1, 65536: 247}

# CFSEC_CRC32_GROUPS_PROBE over PROBE_N shards of 273 tiles: (value, groups, tpw)
PROBE_LEN = 272 * T + 1
PROBE_N = 3
PROBES = [
    (1, 1, 273),               # total / n = 0: one group of 273 tiles
    (PROBE_N, 1, 273),         # one workgroup per shard
    (2 * PROBE_N, 2, 137),     # 137 + 136
    (1 << 20, 17, 17),         # tiles / 16 binds: the shipped split
]

# the idx + fin form through the public calls: shard lengths, and the stripes each runs at
IDX_LENGTHS = [(17, 3), (4097, 3), (32 * T + 1, 2)]
# one tasklet of three bids whose lengths differ, one of them multi-group
TASKLET_LENGTHS = [17, 4097, 32 * T + 1]


def group_census():
    """(length, n, total) of every case whose group split the GPU module runs."""
    cases = [(length, 1, TOTAL) for length in ONE_GROUP_LENGTHS + MULTI_GROUP_LENGTHS]
    cases += [(LIST_LEN, n, TOTAL) for n in LIST_N] + [(LIST5_LEN, n, TOTAL) for n in LIST5_N]
    cases += [(PROBE_LEN, PROBE_N, v) for v, _, _ in PROBES]
    return cases


def shard_census():
    """(length, pointer offset) of every shard of the length x offset and the multi-group tables."""
    return [(length, off) for length in OFFSET_LENGTHS for off in OFFSETS] + \
           [(length, off) for length in MULTI_GROUP_LENGTHS for off in MULTI_GROUP_OFFSETS]


def list_classes():
    """Classes of the launch split the list tables reach, from the restated plan."""
    out = set()
    for length, ns in ((LIST_LEN, LIST_N), (LIST5_LEN, LIST5_N)):
        for n in ns:
            p = plan(length, n, False)
            for name, v in (("slots", p.slots), ("slots + 1", p.slots + 1), ("2 slots + 1", 2 * p.slots + 1)):
                if n == v:
                    out.add((name, "pw = %d" % p.pw))
    for name, stride in AFFINE_STRIDES:
        out.add(("affine", "negative" if stride < 0 else "stride == len" if stride == LIST_LEN else "positive"))
    for n in CAP_N:
        out.add(("cap", "at" if n == AFFINE_MAX else "above" if n == AFFINE_MAX + 1 else "below"))
    return out


LIST_WANT = {("slots", "pw = 2"), ("slots + 1", "pw = 2"), ("2 slots + 1", "pw = 2"), ("slots", "pw = 6"),
             ("slots + 1", "pw = 6"), ("affine", "positive"), ("affine", "negative"), ("affine", "stride == len"),
             ("cap", "at"), ("cap", "above")}
