"""The routing of the fused product + checksum kernels (matvec_crc_route, kernels.hpp), pinned on the
CPU: no device, nothing launched.

tests/crc_route_driver.cpp links libcfsec.so, plans the reconstruct of every erasure set of the small
Reed-Solomon shapes (classes of sets for the large ones) and the fused encode of every LRC mode, and
prints the library's route, matvec_crc_accepts and the bit-sliced predicates for each job over the
lengths around the 2 KiB tile, the 512 MiB limit of the bit-sliced kernels (64^3 tiles per row), the
largest length, and stripe counts up to the 32-bit tile counter.  Asserted for CFSEC_BS_CRC in
{default, 0, 255} x CFSEC_CRC_LDS in {1, 0}, one driver process per setting (the masks are read once):

 (a) matvec_crc_accepts == (route != none): launch_matvec_crc dispatches on the route, so every
     accepted job has a kernel;
 (b) the route equals tests/crc_routes.py, an independent restatement from the kernels that exist;
 (c) the shapes that used to be accepted without a kernel: EC10P4, EC4P4 and EC3P3 with every parity
     shard erased (outputs-only checksums) and with every shard checksummed past 512 MiB have no
     route; EC12P4 past 512 MiB takes the lookup kernel; EC6P6L9 / EC6P8L10 plain stores past 512 MiB
     are not taken by the bit-sliced product.
"""
import math
import os
import shutil
import subprocess

import pytest

import crc_routes as R
from chubaofs_amd import codemode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chubaofs_amd", "csrc")
LIBDIR = os.path.join(ROOT, "chubaofs_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

MIB512 = 512 << 20
LENS = [1, 2048, 2049, MIB512, MIB512 + 1, 0xFFFFFFFF - 4096]
SETTINGS = [(bs, lds) for bs in (None, 0, 255) for lds in (1, 0)]

TACTICS = [codemode.GetTactic(c) for c in codemode.GetAllCodeModes()]
RS_SHAPES = sorted({(t.N, t.M) for t in TACTICS} | {(8, 1), (18, 1), (6, 8)})
LRC_MODES = sorted({(t.N, t.M, t.L, t.AZCount, t.PutQuorum) for t in TACTICS if t.L})


def _compiler():
    return shutil.which("g++") or shutil.which("hipcc") or shutil.which(os.path.join(ROCM, "bin", "hipcc"))


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("crc_route") / "crc_route_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "crc_route_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


_tables = {}


def table(driver, bs, lds):
    """The driver's records under one env setting: (lens with their stripe counts, rs records, lrc records)."""
    if (bs, lds) in _tables:
        return _tables[bs, lds]
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFSEC_")}
    env["CFSEC_CRC_LDS"] = str(lds)
    if bs is not None:
        env["CFSEC_BS_CRC"] = str(bs)
    args = [f"rs:{n}:{m}" for n, m in RS_SHAPES] + ["lrc:" + ":".join(map(str, t)) for t in LRC_MODES]
    r = subprocess.run([driver] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    grid, rs, lrc = [], [], []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "L":
            grid.append((int(f[1]), [int(x) for x in f[2:5]]))
        elif f[0] == "rs":
            coef = b"" if f[7] == "-" else bytes.fromhex(f[7])
            rs.append(dict(N=int(f[1]), M=int(f[2]), data_only=int(f[3]), erased=tuple(map(int, f[4].split(","))),
                           k=int(f[5]), m=int(f[6]), coef=coef, cells=f[8]))
        elif f[0] == "lrc":
            lrc.append(dict(N=int(f[1]), M=int(f[2]), L=int(f[3]), k=int(f[5]), m=int(f[6]),
                            coef=bytes.fromhex(f[7]), plain_matches=int(f[8]), cells=f[9], plain=f[10]))
    _tables[bs, lds] = (grid, rs, lrc)
    return _tables[bs, lds]


def cell(cells, grid, cin_index, length, stripe_index):
    i = (cin_index * len(grid) + [g[0] for g in grid].index(length)) * 3 + stripe_index
    return cells[3 * i:3 * i + 3]


def expected_cells(grid, k, m, bits, dyadic, cins, bs, lds):
    mask = R.BS_CRC_DEFAULT if bs is None else bs
    out = []
    for cin in cins:
        for length, nsts in grid:
            for nst in nsts:
                route = R.expect_route(k, m, cin, length, nst, bits, dyadic, mask, bool(lds))
                out.append("%s%d%d" % ({v: d for d, v in R.ROUTE_DIGIT.items()}[route], route != R.NONE,
                                       route == R.BIT_SLICED))
    return "".join(out)


def test_the_grid_is_the_one_asked_for(driver):
    grid, rs, lrc = table(driver, None, 1)
    assert [g[0] for g in grid] == LENS
    for length, nsts in grid:
        tiles = -(-length // 2048)
        assert nsts[:2] == [1, 5]
        # the third count pushes tiles x stripes over 2^32 - 1 wherever an int count can
        assert tiles * nsts[2] > 2 ** 32 - 1 or nsts[2] == 2 ** 31 - 1
    assert any(tiles * n[2] > 2 ** 32 - 1 for length, n in grid for tiles in [-(-length // 2048)] if tiles <= 64 ** 3)
    assert {(r["N"], r["M"]) for r in rs} == set(RS_SHAPES)
    assert {(r["N"], r["M"], r["L"]) for r in lrc} == {t[:3] for t in LRC_MODES} and len(LRC_MODES) == 6
    for n, m in RS_SHAPES:
        sets = {r["erased"] for r in rs if (r["N"], r["M"]) == (n, m)}
        every = sum(math.comb(n + m, j) for j in range(1, m + 1))
        if every <= 3000:
            assert len(sets) == every, (n, m)
        else:  # all parity, each parity prefix, data only, 200 random sets (less the ones drawn twice)
            assert all(tuple(range(n, n + j)) in sets for j in range(1, m + 1)), (n, m)
            assert all(tuple(range(j)) in sets for j in range(1, min(n, m) + 1)), (n, m)
            assert len(sets) >= 150 and all(1 <= len(s) <= m for s in sets), (n, m)
        for flag in (0, 1):
            assert {r["erased"] for r in rs if (r["N"], r["M"], r["data_only"]) == (n, m, flag)} == sets
    exhaustive = {s for s in RS_SHAPES if sum(math.comb(sum(s), j) for j in range(1, s[1] + 1)) <= 3000}
    assert {(3, 3), (4, 4), (6, 3), (6, 6), (10, 4), (12, 4)} <= exhaustive


@pytest.mark.parametrize("bs,lds", SETTINGS)
def test_accepts_is_having_a_route(driver, bs, lds):
    grid, rs, lrc = table(driver, bs, lds)
    for r in rs + lrc:
        c = r["cells"]
        assert len(c) == 3 * 3 * len(grid) * (2 if "erased" in r else 1)
        for i in range(0, len(c), 3):
            assert (c[i] != "0") == (c[i + 1] == "1"), (r, i // 3)


@pytest.mark.parametrize("bs,lds", SETTINGS)
def test_route_is_the_restated_table(driver, bs, lds):
    grid, rs, lrc = table(driver, bs, lds)
    cache = {}
    for r in rs + lrc:
        bits = R.match_bits(r["k"], r["m"], r["coef"])
        dy = r["k"] == 6 and r["m"] == 12 and R.dyadic_6x12(r["coef"])
        cins = (False, True) if "erased" in r else (True,)
        key = (r["k"], r["m"], bits, dy, cins)
        if key not in cache:
            cache[key] = expected_cells(grid, r["k"], r["m"], bits, dy, cins, bs, lds)
        assert r["cells"] == cache[key], (r, key)
    mask = R.BS_CRC_DEFAULT if bs is None else bs
    for r in lrc:
        want = "".join("%d" % R.expect_plain(r["k"], r["m"], r["coef"], length, nst, bs_mask=mask)
                       for length, nsts in grid for nst in nsts)
        assert r["plain"] == want, r
    # the table is not vacuous: every route occurs somewhere under the default masks
    if bs is None and lds:
        seen = {c[i] for r in rs + lrc for c in [r["cells"]] for i in range(0, len(c), 3)}
        assert seen == {"0", "1", "2", "3"}


def encode_record(rs, n, m):
    (r,) = [r for r in rs if (r["N"], r["M"], r["data_only"]) == (n, m, 0) and r["erased"] == tuple(range(n, n + m))]
    assert r["m"] == m and R.match_bits(n, m, r["coef"]), "every parity shard erased: the encode rows"
    return r


@pytest.mark.parametrize("bs,lds", SETTINGS)
def test_named_regressions(driver, bs, lds):
    grid, rs, lrc = table(driver, bs, lds)
    mask = R.BS_CRC_DEFAULT if bs is None else bs
    for n, m in [(10, 4), (4, 4), (3, 3)]:
        r = encode_record(rs, n, m)
        for length in LENS:
            for si in range(3):
                # outputs-only checksums (RSEngine::reconstruct_crc_batch): no kernel for these input counts
                assert cell(r["cells"], grid, 0, length, si) == "000", (n, m, length, si)
        for si in range(3):
            assert cell(r["cells"], grid, 1, MIB512 + 1, si) == "000", (n, m, si)
            # (and below the limit the network takes them, where its mask bit is set)
            assert cell(r["cells"], grid, 1, 2049, si) == ("111" if mask & 16 else "000"), (n, m, si)
    r = encode_record(rs, 12, 4)
    for si in range(3):
        assert cell(r["cells"], grid, 1, MIB512 + 1, si) == ("210" if lds else "310"), si
        assert cell(r["cells"], grid, 1, MIB512, 0) == ("111" if mask & 10 else "210" if lds else "310")
    wide = [r for r in lrc if (r["N"], r["M"], r["L"]) in ((6, 6, 9), (6, 8, 10))]
    assert len(wide) == 2
    for r in wide:
        assert r["plain_matches"] == (1 if mask & 32 else 0)
        for length, want in ((MIB512 + 1, "000"), (0xFFFFFFFF - 4096, "000"),
                             (MIB512, ("110" if mask & 32 else "000"))):  # 512 MiB x 16384 stripes: 2^32 tiles
            i = 3 * LENS.index(length)
            assert r["plain"][i:i + 3] == want, (r["N"], r["M"], r["L"], length)
