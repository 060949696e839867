"""The crc32block framing kernel's per-block geometry and launch grid, restated from
chubaofs_amd/csrc/crc32block.hip (make() of crc32block_block_kernel, and blk::launch's b0, nb, out_off
and grid) without calling the library, and the case tables aimed at its alignment, seam and stride
edges.  tests/test_crc32block_geometry.py asserts on the CPU that the tables reach every class of that
geometry; tests/test_gpu_crc32block_edges.py runs them on the GPU against the oracle."""
import collections

TILE = 4096      # bytes of the destination per tile (crcdev::kTile)
LINE = 128       # decode: one writer per line of this many bytes
RING = 8         # tiles in flight per thread of the shipped kernel
SLOTS = 128      # objects per launch (blk::kSlots)
AFTER = 200      # blocks up to which a block's CRC moves to the object end in one multiply (blk::kAfter)

Block = collections.namedtuple("Block", "w b q0 plen last h b16 h4 tiles dt sbeg send lim nx")


def ceil_div(a, b):
    return -(-a // b)


def launch_blocks(P, size, from_, to):
    """blk::launch for decode: (b0, nb), the first block of the launch and its block count."""
    b0 = from_ // P
    b1 = (to - 1) // P if from_ < to else (b0 if from_ % P else b0 - 1)
    return b0, b1 - b0 + 1


def _block(P, size, w, b0, nb, D, decode):
    """make(): launch block w, whose payload byte 0 goes to address D (relative to a 4096-aligned one)."""
    b = b0 + w
    q0 = b * P
    plen = min(P, size - q0)
    last = int(plen != P)
    h = D % TILE
    tiles = ceil_div(plen + h, TILE)
    b16 = h & 15
    dt = tiles - ceil_div(plen + b16, TILE)
    sbeg, send, lim = 0, plen, plen
    if decode:
        if w > 0:
            sbeg = -D % LINE
        if w + 1 < nb:
            nxt = min(P, size - q0 - plen)
            send = plen + min(-(D + plen) % LINE, nxt)
            lim = plen - ((plen + h) & 15)
    nx = (send - lim + 15) >> 4 if send > lim else 0
    return Block(w, b, q0, plen, last, h, b16, h >> 4, tiles, dt, sbeg, send, lim, nx)


def geometry(P, size, from_, to, d0):
    """Decode of payload [from_, to) of an object of `size` bytes in blocks of P payload bytes into a
    destination whose byte 0 is at d0 relative to a 4096-aligned address (0 with no destination): one
    Block per launch block.  Block w's payload byte 0 belongs at d0 + out_off + w * P, out_off = b0 * P -
    from_ (negative when from_ lies inside block b0)."""
    b0, nb = launch_blocks(P, size, from_, to)
    return [_block(P, size, w, b0, nb, d0 + b0 * P - from_ + w * P, True) for w in range(max(nb, 0))]


def encode_geometry(P, size, d0):
    """Encode into a framed object at d0: block w's payload byte 0 belongs at d0 + w * (P + 4) + 4."""
    nb = ceil_div(size, P)
    return [_block(P, size, w, 0, nb, d0 + w * (P + 4) + 4, False) for w in range(nb)]


def expected_grid(items, resident, full):
    """blk::launch's grid of the resident strided kernel: the whole resident grid (CFSEC_BLK_GRID unset
    or 1: `full`), or the fewest workgroups that give every one ceil(items / resident) blocks."""
    if full and resident:
        return min(resident, items)
    per = ceil_div(items, resident) if resident else 1
    return ceil_div(items, per)


# ---- the case tables

K = 1024
P4, P64, PM = 4 * K - 4, 64 * K - 4, (1 << 20) - 4
# h = (address of a block's payload byte 0) mod 4096: h & 15 in {0, 15, between} x h >> 4 in {0, 255, between},
# and both sides of 128-byte lines and of the 2 KiB middle
D = [0, 1, 4, 15, 16, 17, 127, 128, 129, 2047, 2048, 4079, 4080, 4095]
SRC_OFFSETS = [0, 1, 7, 15]  # source misalignment: the unaligned 16-byte loads
SIZES = {
    4 * K: [3 * P4 + 1, 3 * P4 + 15, 3 * P4 + 16, 3 * P4 + 17, 3 * P4 + 127, 3 * P4 + 128, 3 * P4 + 129, 4 * P4 - 1, 4 * P4],
    64 * K: [2 * P64 + 1, 2 * P64 + 129, 3 * P64],
    1 << 20: [2 * PM + 5],  # more tiles than two rings
}
WHOLE_CASES = [(block_len, size) for block_len, sizes in SIZES.items() for size in sizes]

# encode: the payload of every block of an object lands at h = (dst + 4) mod 4096
ENCODE_OBJECTS = [((h - 4) % TILE, s) for h in D for s in SRC_OFFSETS]   # (destination offset, source offset)
DECODE_OBJECTS = [(d, s) for d in D for s in SRC_OFFSETS]

RANGE_SIZE = 3 * P4 + 77
RANGE_OFFSETS = [0, 1, 100, 127]


def _ranges():
    P, size, out = P4, RANGE_SIZE, []
    for f in [0, 1, P - 1, P, P + 1, 2 * P + 5]:
        for t in [0, 1, P, P + 1, P + 100, 2 * P - 1, 2 * P, 2 * P + 127, size - 1, size, f, f + 1]:
            if f <= t <= size and (f, t) not in out:
                out.append((f, t))
    return out


RANGES = _ranges()  # (from, to) on RANGE_SIZE at block_len 4096, each at every RANGE_OFFSETS destination


def encode_census_cases():
    """(P, size, d0) of every encoded object of the GPU module's alignment test."""
    return [(bl - 4, size, d) for bl, size in WHOLE_CASES for d, _ in ENCODE_OBJECTS]


def decode_census_cases():
    """(P, size, from, to, d0) of every decoded object of the alignment and the range tests."""
    out = [(bl - 4, size, 0, size, d) for bl, size in WHOLE_CASES for d, _ in DECODE_OBJECTS]
    out += [(P4, RANGE_SIZE, f, t, d) for f, t in RANGES for d in RANGE_OFFSETS]
    return out


def block_classes(k):
    """The classes of one block that both directions must reach."""
    out = {("b16", 0 if k.b16 == 0 else 15 if k.b16 == 15 else "mid"),
           ("h4", 0 if k.h4 == 0 else 255 if k.h4 == 255 else "mid"),
           ("dt,last", k.dt, k.last)}
    if k.tiles in (1, 2, 2 * RING, 2 * RING + 1):
        out.add(("tiles", k.tiles))
    elif k.tiles > 2 * RING + 1:
        out.add(("tiles", "above"))
    return out


BOTH = ({("b16", v) for v in (0, 15, "mid")} | {("h4", v) for v in (0, 255, "mid")}
        | {("dt,last", dt, last) for dt in (0, 1) for last in (0, 1)}
        | {("tiles", v) for v in (1, 2, 2 * RING, 2 * RING + 1, "above")})

DECODE_ONLY = {("w>0", "sbeg=0"), ("w>0", "sbeg>0"), ("carry", "zero"), ("carry", "line"), ("carry", "short last block"),
               ("plen-lim", "zero"), ("plen-lim", "positive"), ("nx", 0), ("nx", 1), ("nx", 8),
               ("to", "inside the carry"), ("from", "inside a block, off a piece boundary"),
               ("from == to", "inside a block"), ("to - from", "below 16")}


def decode_classes(P, size, from_, to, d0):
    blocks = geometry(P, size, from_, to, d0)
    out = set()
    for k in blocks:
        out |= block_classes(k)
        if k.w > 0:
            out.add(("w>0", "sbeg=0" if k.sbeg == 0 else "sbeg>0"))
        if k.w + 1 < len(blocks):
            carry, nxt = k.send - k.plen, min(P, size - k.q0 - k.plen)
            room = -(d0 + k.b * P - from_ + k.plen) % LINE  # to the end of the seam's line
            out.add(("carry", "zero" if carry == 0 else "line" if carry == room else "short last block"))
            assert carry == min(room, nxt) and (carry == room or nxt < room)
            out.add(("plen-lim", "zero" if k.lim == k.plen else "positive"))
            if k.plen < to - k.q0 < k.send:
                out.add(("to", "inside the carry"))
        assert 0 <= k.nx <= 8
        if k.nx in (0, 1, 8):
            out.add(("nx", k.nx))
    if from_ % P and d0 % 16:
        out.add(("from", "inside a block, off a piece boundary"))
    if from_ == to and from_ % P:
        out.add(("from == to", "inside a block"))
    if 0 < to - from_ < 16:
        out.add(("to - from", "below 16"))
    return out


def encode_classes(P, size, d0):
    out = set()
    for k in encode_geometry(P, size, d0):
        out |= block_classes(k)
    return out
