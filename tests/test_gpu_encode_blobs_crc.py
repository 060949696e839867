"""Put batches of mixed-size blobs on the GPU: cfsec_ec_encode_blobs_crc and cfsec_rs_encode_crc_stripes
(the mixed-plan launch with checksums of gf_mix_crc.hip, and the launch groups behind it).

Every case lays its shards out in one arena of random bytes: each row sits at its own byte offset 0..15
from a 16-byte boundary with at least 64 untouched bytes on either side.  The call runs on one copy of
the arena; ECOracle.encode (rs_encode for the reedsolomon-level call) runs on host copies of the rows.
Asserted for every stripe of every case, none left out:

  * status for status: the call == the oracle == the single Encode call on a second copy of the arena;
  * byte for byte: the whole arena after the call equals the arena with the oracle's parity put in -- so
    every guard byte, every data row and every buffer of a failed stripe is unchanged;
  * word for word: crcs[stripe * n + shard] == zlib.crc32 of that shard as the oracle left it, all-zero
    words for a stripe that failed;
  * the launches the call traces (CFSEC_TRACE_MATVEC, CFSEC_TRACE_CRC32, CFSEC_TRACE_CRC).

Sizes are the smallest at which the kernel can go wrong: rows shorter than a 16-byte chunk (1, 15), a
whole chunk (16), the overlapped last chunk (17, 31, 4095, 8197), the 4 KiB tile seam (4095, 4096, 4097),
several tiles XOR-ed into one word (8197, 65536), every pass count of the kernel (1, a partial one, 2, 3
and 6 passes), 16 inputs, no outputs.  None is a workload size.
"""
import ctypes
import zlib

import numpy as np
import pytest

from chubaofs_amd import _lib, codemode as cm, ec, reedsolomon
from oracle import ec_oracle as EO
from oracle.ec_oracle import ECOracle, Slice

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LENS = [1, 15, 16, 17, 31, 2048, 4095, 4096, 4097, 8197, 65536]
GUARD = 64
MODES = ["EC12P4", "EC6P3", "EC3P3", "EC6P6", "EC6P10L2", "EC16P20L2", "rs4+0"]


def tactic(name):
    (c,) = [c for c in cm.GetAllCodeModes() if cm.Name(c) == name]
    return cm.GetTactic(c)


# ---------------------------------------------------------------- the arena

class Case:
    """Stripes of n rows each; row j of stripe c has `sizes[j]` bytes of buffer (header length the same)
    at offset (5 c + 3 j) mod 16 from a 16-byte boundary."""

    def __init__(self, n, seed):
        self.n, self.items, self.size = n, [], 0
        self.rng = np.random.default_rng(seed)

    def stripe(self, S, sizes=None, n=None):
        c = len(self.items)
        rows = []
        for j in range(self.n if n is None else n):
            size = S if sizes is None else sizes[j]
            pos = (self.size + GUARD + 15) // 16 * 16 + (5 * c + 3 * j) % 16
            self.size = pos + size
            rows.append((pos, size))
        self.items.append(rows)

    def image(self):
        return self.rng.integers(0, 256, self.size + GUARD, dtype=np.uint8)


class Mem:
    """The arena in one kind of memory, its first byte on a 16-byte boundary."""

    def __init__(self, kind, image):
        self.kind, self.n = kind, image.size
        if kind == "device":
            self.buf = torch.empty(image.size + 16, dtype=torch.uint8, device="cuda")
            base = self.buf.data_ptr()
        else:
            self.buf = _lib.pinned_empty(image.size + 16) if kind == "pinned" else np.empty(image.size + 16, np.uint8)
            base = self.buf.ctypes.data
        self.off = (-base) % 16
        self.ptr = base + self.off
        if kind == "device":
            self.buf[self.off:self.off + self.n] = torch.from_numpy(image).cuda()
            torch.cuda.synchronize()
        else:
            self.buf[self.off:self.off + self.n] = image
        self.mem = _lib.MEM_DEVICE if kind == "device" else _lib.MEM_HOST

    def read(self):
        if self.kind == "device":
            torch.cuda.synchronize()
            return self.buf[self.off:self.off + self.n].cpu().numpy()
        return np.array(self.buf[self.off:self.off + self.n])


def shard_array(case, mem):
    arr = (_lib.Shard * sum(len(rows) for rows in case.items))()
    at = 0
    for rows in case.items:
        for pos, size in rows:
            arr[at] = _lib.Shard(mem.ptr + pos, size, size) if size else _lib.Shard(None, 0, 0)
            at += 1
    return arr


# ---------------------------------------------------------------- the calls

class EcCalls:
    """cfsec_ec_encode_blobs_crc against cfsec_ec_encode, cfsec_ec_encode_batch_crc and ECOracle.encode."""

    def __init__(self, name, enable_verify=False):
        self.t = tactic(name)
        self.n = self.t.N + self.t.M + self.t.L
        self.enc = ec.NewEncoder(ec.Config(CodeMode=self.t, EnableVerify=enable_verify))
        self.orc = ECOracle.from_tactic(self.t, enable_verify)
        self.L = self.enc._L

    def batch(self, arr, n, nstripes, mem, fn=None):
        status = (ctypes.c_int * max(nstripes, 1))(*([-7] * max(nstripes, 1)))
        words = (ctypes.c_uint32 * max(nstripes * n, 1))(*([0xA5A5A5A5] * max(nstripes * n, 1)))
        rc = (fn or self.L.cfsec_ec_encode_blobs_crc)(self.enc._h, arr, n, nstripes, mem, status, words)
        return rc, [int(status[i]) for i in range(nstripes)], [int(w) for w in words][:nstripes * n]

    def old(self, arr, n, nstripes, mem):
        return self.batch(arr, n, nstripes, mem, self.L.cfsec_ec_encode_batch_crc)

    def single(self, sub, n, mem):
        return self.L.cfsec_ec_encode(self.enc._h, sub, n, mem, None)

    def oracle(self, shards):
        return self.orc.encode(shards)


class RsCalls:
    """cfsec_rs_encode_crc_stripes against cfsec_rs_encode and rs_encode."""

    old = None

    def __init__(self, k, m):
        self.k, self.m, self.n = k, m, k + m
        self.enc = reedsolomon.New(k, m, device=0)
        self.L = self.enc._L

    def batch(self, arr, n, nstripes, mem):
        assert n == self.n
        status = (ctypes.c_int * max(nstripes, 1))(*([-7] * max(nstripes, 1)))
        words = (ctypes.c_uint32 * max(nstripes * n, 1))(*([0xA5A5A5A5] * max(nstripes * n, 1)))
        rc = self.L.cfsec_rs_encode_crc_stripes(self.enc._h, arr, nstripes, mem, status, words)
        return rc, [int(status[i]) for i in range(nstripes)], [int(w) for w in words][:nstripes * n]

    def single(self, sub, n, mem):
        return self.L.cfsec_rs_encode(self.enc._h, sub, n, mem, None)

    def oracle(self, shards):
        return EO.rs_encode(self.k, self.m, shards)


def calls_for(name, enable_verify=False):
    return RsCalls(4, 0) if name == "rs4+0" else EcCalls(name, enable_verify)


def expect(case, calls, image):
    """The oracle on host copies of every stripe: (statuses, arena afterwards, checksum words)."""
    want = image.copy()
    status, words = [], []
    for rows in case.items:
        sh = [Slice(image[pos:pos + size].copy(), size) for pos, size in rows]
        st = calls.oracle(sh)
        status.append(st)
        if st == EO.OK:
            for (pos, size), s in zip(rows, sh):
                assert s.buf.size == size, "the oracle allocated"
                want[pos:pos + size] = s.buf
            words += [zlib.crc32(s.buf.tobytes()) for s in sh]
        else:
            words += [0] * len(rows)
    return status, want, words


def run(case, calls, kind, capfd=None, n=None, single=True):
    """Run the case on the GPU and compare with the oracle; returns (trace, statuses, words, arena)."""
    image = case.image()
    n, nstripes = calls.n if n is None else n, len(case.items)
    ostatus, want, owords = expect(case, calls, image)
    a = Mem(kind, image)
    arr_a = shard_array(case, a)
    if capfd:
        capfd.readouterr()
    rc, status, words = calls.batch(arr_a, n, nstripes, a.mem)
    got = a.read()
    err = capfd.readouterr().err if capfd else ""
    assert rc == 0, _lib.lib().cfsec_last_error()
    assert status == ostatus, "statuses differ from the oracle's"
    bad_at = np.flatnonzero(got != want)
    assert bad_at.size == 0, "arena differs from the oracle's at %d bytes, first at %d" % (bad_at.size, bad_at[0])
    wrong = [(i // n, i % n) for i, (g, w) in enumerate(zip(words, owords)) if g != w]
    assert not wrong, "checksum words differ from zlib's at (stripe, shard) %s" % wrong[:8]
    if single:
        b = Mem(kind, image)
        arr_b = shard_array(case, b)
        one = []
        for i in range(nstripes):
            sub = (_lib.Shard * n).from_address(ctypes.addressof(arr_b) + i * n * ctypes.sizeof(_lib.Shard))
            one.append(calls.single(sub, n, b.mem))
        assert status == one, "statuses differ from the single calls'"
        assert np.array_equal(b.read(), want), "the single calls differ from the oracle"
    return err, status, words, got


def lines(err, *prefixes):
    return [ln for ln in err.splitlines() if any(ln.startswith(p) for p in prefixes)]


def mixcrc_lines(err):
    return [dict(x.split("=") for x in ln.split()[2:]) for ln in lines(err, "cfsec: mixcrc ")]


def other_launches(err):
    """Product launches, fused product + checksum launches, separate checksum launches, store-only mixed ones."""
    return lines(err, "cfsec: matvec ", "cfsec: dy16", "cfsec: crc32 ", "cfsec: crc ", "cfsec: bs ", "cfsec: mix ")


def tiles_of(lens):
    return sum(-(-ln // 4096) for ln in lens)


def trace_on(monkeypatch, limit=None):
    for v in ("CFSEC_TRACE_MATVEC", "CFSEC_TRACE_CRC32", "CFSEC_TRACE_CRC"):
        monkeypatch.setenv(v, "1")
    if limit is None:
        monkeypatch.delenv("CFSEC_MIX_MAX_LEN", raising=False)
    else:
        monkeypatch.setenv("CFSEC_MIX_MAX_LEN", str(limit))


def lens_case(calls, lens, seed):
    case = Case(calls.n, seed)
    for S in lens:
        case.stripe(S)
    return case


# ---------------------------------------------------------------- lengths, alignments, modes, memory kinds

@pytest.mark.parametrize("kind", ["device", "pinned", "pageable"])
@pytest.mark.parametrize("name", MODES)
def test_every_length_in_one_call(name, kind, monkeypatch, capfd):
    trace_on(monkeypatch)
    calls = calls_for(name)
    case = lens_case(calls, LENS, seed=len(name) + calls.n)
    assert {(5 * c + 3 * j) % 16 for c in range(len(LENS)) for j in range(calls.n)} == set(range(16))
    err, status, _, _ = run(case, calls, kind, capfd)
    assert status == [0] * len(LENS)
    # one launch codes and checksums the whole batch: no product launch, no checksum launch
    mx = mixcrc_lines(err)
    assert len(mx) == 1, err
    assert (int(mx[0]["items"]), int(mx[0]["tiles"]), int(mx[0]["plans"])) == (len(LENS), tiles_of(LENS), 1)
    assert other_launches(err) == [], err


@pytest.mark.parametrize("name", MODES)
def test_switched_off_the_old_path_gives_the_same_bytes_and_words(name, monkeypatch, capfd):
    calls = calls_for(name)
    case = lens_case(calls, LENS, seed=77 + calls.n)
    trace_on(monkeypatch)
    _, st_new, words_new, got_new = run(case, calls, "device", capfd, single=False)
    trace_on(monkeypatch, limit=0)
    case = lens_case(calls, LENS, seed=77 + calls.n)
    err, st_old, words_old, got_old = run(case, calls, "device", capfd, single=False)
    assert mixcrc_lines(err) == [] and other_launches(err) != []
    assert st_old == st_new and words_old == words_new and np.array_equal(got_old, got_new)
    if calls.old:  # and cfsec_ec_encode_batch_crc on the same batch
        monkeypatch.delenv("CFSEC_MIX_MAX_LEN")
        case = lens_case(calls, LENS, seed=77 + calls.n)
        a = Mem("device", case.image())
        capfd.readouterr()
        rc, st, words = calls.old(shard_array(case, a), calls.n, len(LENS), a.mem)
        err = capfd.readouterr().err
        assert rc == 0 and st == st_new and words == words_new and np.array_equal(a.read(), got_new)
        assert mixcrc_lines(err) == [], "cfsec_ec_encode_batch_crc keeps its launches"


# ---------------------------------------------------------------- the length limit

@pytest.mark.parametrize("name", ["EC12P4", "EC6P10L2"])
def test_items_on_both_sides_of_the_limit(name, monkeypatch, capfd):
    trace_on(monkeypatch, limit=4096)
    calls = calls_for(name)
    lens = [100, 4097, 4096, 20000, 3000, 8192]
    err, status, _, _ = run(lens_case(calls, lens, seed=5), calls, "device", capfd)
    assert status == [0] * len(lens)
    mx = mixcrc_lines(err)
    assert len(mx) == 1 and (int(mx[0]["items"]), int(mx[0]["tiles"])) == (3, 3)  # 100, 4096, 3000
    assert other_launches(err) != [], "the long stripes keep the launch groups"


def test_a_lone_small_item_goes_to_the_groups(monkeypatch, capfd):
    trace_on(monkeypatch, limit=4096)
    calls = calls_for("EC12P4")
    err, status, _, _ = run(lens_case(calls, [8000, 100, 9000], seed=6), calls, "device", capfd)
    assert status == [0, 0, 0] and mixcrc_lines(err) == [] and other_launches(err) != []
    trace_on(monkeypatch)
    err, status, _, _ = run(lens_case(calls, [2048], seed=7), calls, "pinned", capfd)
    assert status == [0] and mixcrc_lines(err) == [] and other_launches(err) != []


# ---------------------------------------------------------------- failed stripes

@pytest.mark.parametrize("kind", ["device", "pageable"])
@pytest.mark.parametrize("name", ["EC12P4", "EC6P10L2", "rs4+0"])
def test_failed_stripes_between_good_ones(name, kind, monkeypatch, capfd):
    trace_on(monkeypatch)
    calls = calls_for(name)
    n = calls.n
    case = Case(n, seed=11 + n)
    case.stripe(2048)
    case.stripe(0, sizes=[3000] * 2 + [2999] + [3000] * (n - 3))  # unequal shard sizes (a data shard)
    case.stripe(4097)
    case.stripe(0, sizes=[500, 4000] + [500] * (n - 2))           # one data shard longer than the rest
    case.stripe(17)
    if name == "EC6P10L2":
        case.stripe(0, sizes=[700] * 6 + [690] + [700] * (n - 7))  # a global parity shard shorter
    else:
        case.stripe(0, sizes=[0] + [600] * (n - 1))               # an empty shard among full ones
    bad = [1, 3, 5]
    case.stripe(31)
    err, status, words, _ = run(case, calls, kind, capfd)
    assert [i for i, s in enumerate(status) if s != 0] == bad
    for i in bad:
        assert words[i * n:(i + 1) * n] == [0] * n
    mx = mixcrc_lines(err)
    assert len(mx) == 1 and int(mx[0]["items"]) == 4, err


@pytest.mark.parametrize("name", ["EC12P4", "EC6P10L2"])
def test_a_wrong_shard_count_fails_every_stripe_and_touches_nothing(name, monkeypatch, capfd):
    trace_on(monkeypatch)
    calls = calls_for(name)
    n = calls.n - 1
    case = Case(calls.n, seed=13)
    for S in (2048, 100, 4097):
        case.stripe(S, n=n)
    err, status, words, _ = run(case, calls, "device", capfd, n=n)
    assert all(s != 0 for s in status) and words == [0] * (3 * n)
    assert mixcrc_lines(err) == [] and other_launches(err) == []


# ---------------------------------------------------------------- larger batches

def test_300_stripes_of_one_plan_are_one_launch(monkeypatch, capfd):
    trace_on(monkeypatch)
    calls = calls_for("EC12P4")
    lens = [2048 + 7 * i for i in range(300)]  # all distinct, across the 4 KiB seam
    err, status, _, _ = run(lens_case(calls, lens, seed=300), calls, "device", capfd, single=False)
    assert status == [0] * 300
    mx = mixcrc_lines(err)
    assert len(mx) == 1 and (int(mx[0]["items"]), int(mx[0]["tiles"])) == (300, tiles_of(lens))
    assert other_launches(err) == []


def test_70_stripes_over_lrc_and_rs_handles(monkeypatch, capfd):
    trace_on(monkeypatch)
    lens = [1 + 131 * i for i in range(70)]  # 1 .. 9040, all distinct
    share = {"EC6P10L2": lens[0::4], "EC16P20L2": lens[1::4], "EC6P6": lens[2::4], "EC3P3": lens[3::4]}
    for name, mine in share.items():
        calls = calls_for(name)
        err, status, _, _ = run(lens_case(calls, mine, seed=len(mine)), calls, "pinned", capfd, single=False)
        assert status == [0] * len(mine)
        mx = mixcrc_lines(err)
        assert len(mx) == 1 and (int(mx[0]["items"]), int(mx[0]["tiles"])) == (len(mine), tiles_of(mine)), name
        assert other_launches(err) == [], name


# ---------------------------------------------------------------- EnableVerify

@pytest.mark.parametrize("name", ["EC12P4", "EC6P10L2"])
def test_enable_verify_statuses_match_encode_batch_crc(name, monkeypatch, capfd):
    trace_on(monkeypatch)
    calls = calls_for(name, enable_verify=True)
    n = calls.n

    def make():
        case = Case(n, seed=17)
        for S in (2048, 17, 4097):
            case.stripe(S)
        case.stripe(0, sizes=[3000] * 2 + [2999] + [3000] * (n - 3))
        case.stripe(8197)
        return case

    err, status, words, got = run(make(), calls, "device", capfd)
    assert status == [0, 0, 0, status[3], 0] and status[3] != 0
    mx = mixcrc_lines(err)
    assert len(mx) == 1 and int(mx[0]["items"]) == 4
    assert other_launches(err) != [], "the Verify pass runs on the launch groups"
    case = make()
    b = Mem("device", case.image())
    rc, st_old, words_old = calls.old(shard_array(case, b), n, len(case.items), b.mem)
    assert rc == 0 and st_old == status and words_old == words and np.array_equal(b.read(), got)


# ---------------------------------------------------------------- the Python methods

def test_python_methods_return_the_words_of_the_c_call():
    rng = np.random.default_rng(23)
    lens = [2048, 17, 4097, 300]
    for name in ("EC12P4", "EC6P10L2"):
        calls = calls_for(name)
        t, n = calls.t, calls.n
        stripes = [[rng.integers(0, 256, S, dtype=np.uint8) for _ in range(t.N)] +
                   [np.zeros(S, np.uint8) for _ in range(n - t.N)] for S in lens]
        want = []
        for st in stripes:
            sh = EO.vector(st)
            assert calls.orc.encode(sh) == EO.OK
            want.append([zlib.crc32(s.buf.tobytes()) for s in sh])
        arr = (_lib.Shard * (len(lens) * n))()
        keep = [[a.copy() for a in st] for st in stripes]
        for i, st in enumerate(keep):
            for j, a in enumerate(st):
                arr[i * n + j] = _lib.Shard(a.ctypes.data, a.size, a.size)
        rc, status_c, words_c = calls.batch(arr, n, len(lens), _lib.MEM_HOST)
        status, words = calls.enc.EncodeBlobsCRC(stripes)
        assert rc == 0 and status == status_c == [0] * len(lens)
        assert words == want and [w for ws in words for w in ws] == words_c
        for st, kept in zip(stripes, keep):
            assert all(np.array_equal(a, b) for a, b in zip(st, kept))
    rs = reedsolomon.New(6, 3, device=0)
    stripes = [[rng.integers(0, 256, S, dtype=np.uint8) for _ in range(6)] + [np.zeros(S, np.uint8) for _ in range(3)]
               for S in lens]
    want = []
    for st in stripes:
        sh = EO.vector(st)
        assert EO.rs_encode(6, 3, sh) == EO.OK
        want.append([zlib.crc32(s.buf.tobytes()) for s in sh])
    arr = (_lib.Shard * (len(lens) * 9))()
    keep = [[a.copy() for a in st] for st in stripes]
    for i, st in enumerate(keep):
        for j, a in enumerate(st):
            arr[i * 9 + j] = _lib.Shard(a.ctypes.data, a.size, a.size)
    status_c = (ctypes.c_int * len(lens))()
    words_c = (ctypes.c_uint32 * (len(lens) * 9))()
    assert rs._L.cfsec_rs_encode_crc_stripes(rs._h, arr, len(lens), _lib.MEM_HOST, status_c, words_c) == 0
    status, words = rs.EncodeCRCStripes(stripes)
    assert status == list(status_c) == [0] * len(lens)
    assert words == want and [w for ws in words for w in ws] == list(words_c)
