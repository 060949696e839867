"""The launch geometry of the fused product + checksum kernels (plan_bs_crc, plan_matvec_crc:
kernels.hpp), pinned on the CPU: no device, nothing launched.

tests/crc_route_driver.cpp ("plan") prints the library's plans over the lengths around the 2 KiB and
4 KiB tiles, 8193 B (a last tile of one byte), a C4 put's and BASELINE C2's row lengths and the 512
MiB limit, stripe counts from 1 to 65536, affine and pointer-table jobs, and the resident workgroup
counts 1, 256, 768, 1024 and 0 (the occupancy query failed).  Asserted:

 (a) every plan equals tests/crc_routes.py's restatement (bs_plan, lk_plan);
 (b) independently of it, for every bit-sliced launch: replaying gf_bs_crc_kernel's indexing, every
     tile (stripe, column < tps) is taken by exactly one wave -- a strided wave (column = j mod W,
     below bend) or a tail wave --, bend + tail == tps, grid == the strided workgroups +
     ceil(tail * stripes / 4), and the launches' stripes partition [0, nstripes);
 (c) for the lookup / v_perm plans: groups x tpw covers the tiles with no empty group, groups <= 384,
     and the group ends are the tile ends clipped to the row's tiles;
 (d) known answers worked out by hand (the tail-wave tests' geometry on a 256-CU device).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import crc_routes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chubaofs_amd", "csrc")
LIBDIR = os.path.join(ROOT, "chubaofs_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

MIB512 = 512 << 20
NSTRIPES = [1, 5, 6, 7, 13, 48, 1536, 65536]
RESIDENT = [1, 256, 768, 1024, 0]
BS_SHAPES = [(12, 4), (6, 12), (3, 3), (16, 22), (6, 18)]
STEP_FIELDS = ("s0", "ns", "tab", "affine", "tps", "W", "groups", "bend", "tail", "tblk", "grid", "jump")


def lens(k):
    return [1, 2047, 2048, 2049, 8193, 4096 * k - 1, 4096 * k + 1, 699051, 5592406, MIB512]


def _compiler():
    return shutil.which("g++") or shutil.which("hipcc") or shutil.which(os.path.join(ROCM, "bin", "hipcc"))


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    exe = tmp_path_factory.mktemp("crc_plan") / "crc_route_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "crc_route_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFSEC_")}
    r = subprocess.run([str(exe), "plan"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    bs, lk = {}, {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "bs":
            runs = []
            for run in f[12].split(";") if len(f) > 12 else []:
                n, rest = run.split("*")
                runs.append((int(n), dict(zip(STEP_FIELDS, map(int, rest.split(","))))))
            bs[int(f[1]), int(f[2]), int(f[3]), f[4], int(f[5]), int(f[6])] = dict(
                resident=int(f[7]), pad=int(f[8]), pw=tuple(map(int, f[9:12])), runs=runs)
        elif f[0] == "lk":
            v = dict(zip(("tiles", "per", "dy", "affine", "groups", "tpw", "gx", "gy"), map(int, f[9:17])))
            v["ends"] = [int(x) for x in f[17].split(",")] if len(f) > 17 else []
            v["coef"] = bytes.fromhex(f[4])
            lk[R.ROUTE_DIGIT[f[1]], int(f[2]), int(f[3]), int(f[5]), f[6], int(f[7]), int(f[8])] = v
    return bs, lk


def run_length(steps):
    """Consecutive launches alike but for s0 (advancing by ns), as the driver prints them."""
    runs = []
    for st in steps:
        if runs:
            n, first = runs[-1]
            if {**st, "s0": 0} == {**first, "s0": 0} and st["s0"] == first["s0"] + n * first["ns"]:
                runs[-1] = (n + 1, first)
                continue
        runs.append((1, st))
    return runs


def test_bit_sliced_plans_are_the_restatement(records):
    bs, _ = records
    want_keys = set()
    for k, m in BS_SHAPES:
        for length in lens(k):
            for nst in NSTRIPES:
                if not R.bs_in_range(length, nst):
                    continue
                for lay in ("aff", "tab"):
                    for res in RESIDENT:
                        key = (k, m, length, lay, nst, res)
                        want_keys.add(key)
                        resident, pad, pw, steps = R.bs_plan(k, m, length, nst, lay == "aff", res)
                        got = bs[key]
                        assert (got["resident"], got["pad"], got["pw"]) == (resident, pad, pw), key
                        assert got["runs"] == run_length(steps), key
    assert set(bs) == want_keys
    assert any(key[2] == MIB512 for key in bs) and any(key[4] == 65536 for key in bs)


_checked = set()


def check_launch(st):
    """(b) for one launch, replaying the kernel's wave indexing."""
    ns, tps, W, groups, bend, tail, tblk, grid = (st[f] for f in ("ns", "tps", "W", "groups", "bend", "tail", "tblk", "grid"))
    key = (ns, tps, W, groups, bend, tail, tblk, grid)
    if key in _checked:
        return
    _checked.add(key)
    assert 1 <= W <= tps and 1 <= groups <= ns and bend + tail == tps and bend % W == 0 and tail < W, st
    assert tblk == R.ceil_div(groups * W, 4) and grid == tblk + R.ceil_div(tail * ns, 4), st
    assert st["jump"] == 2048 * W and grid < 2 ** 31, st
    if ns * tps > 1 << 20:  # past the replay's reach: the arithmetic above stands for it
        return
    count = np.zeros((ns, tps), np.int32)
    for wid in range(tblk * 4):      # strided waves: the workgroups below tblk
        g, j = divmod(wid, W)
        if g < groups and j < tps:
            count[g::groups, j:max(bend, j + 1):W] += 1   # (the kernel takes its first tile before testing bend)
    for q in range((grid - tblk) * 4):  # tail waves
        if q < tail * ns:
            count[q // tail, bend + q % tail] += 1
    assert (count == 1).all(), st


def test_bit_sliced_launches_cover_every_tile_once(records):
    bs, _ = records
    replayed = 0
    for key, plan in bs.items():
        nst, s = key[4], 0
        for n, first in plan["runs"]:
            assert first["s0"] == s and first["tab"] == (1 if first["affine"] else first["ns"]), key
            assert first["ns"] <= (nst if first["affine"] else 96 // (key[0] + key[1])), key
            check_launch(first)
            s += n * first["ns"]
        assert s == nst, key  # the launches' stripes partition [0, nstripes)
        replayed += 1
    assert replayed == len(bs) and any(c[0] * c[1] <= 1 << 20 and c[5] for c in _checked)  # tails were replayed


def test_lookup_plans(records):
    _, lk = records
    assert {k[0] for k in lk} == {R.LOOKUP, R.V_PERM} and {v["dy"] for v in lk.values()} == {-1, 0, 2, 4}
    for key, got in lk.items():
        route, k, m, length, lay, nst, res = key
        want = R.lk_plan(route, k, m, got["coef"], length, nst, lay == "aff", res)
        assert {f: got[f] for f in want} == want, key
        tiles, groups, tpw = got["tiles"], got["groups"], got["tpw"]
        assert 1 <= groups <= 384 and groups * tpw >= tiles > (groups - 1) * tpw, key  # covered, no empty group
        assert got["gx"] == groups and got["gy"] == min(nst, got["per"]) <= 65535, key
        assert got["ends"] == [min((g + 1) * tpw, tiles) * 4096 for g in range(groups)], key
    assert len(lk) == 9 * len(lens(6)) * len(NSTRIPES) * 2 * len(RESIDENT)


@pytest.mark.parametrize("k,m,length,lay,nst,res,want", [
    # tests/test_gpu_bs_crc_tail.py's pointer-table launches: 6 EC12P4 stripes of BASELINE C2's rows
    (12, 4, 5592406, "tab", 6, 768, dict(tps=2731, W=512, groups=6, bend=2560, tail=171, tblk=768, grid=768 + 257)),
    # C4's put batch: 48 affine EC6P10L2 stripes
    (6, 12, 699051, "aff", 48, 768, dict(tps=342, W=64, groups=48, bend=320, tail=22, tblk=768, grid=768 + 264)),
    # 1536 affine EC3P3 stripes of 8193 B: 3072 or 4096 waves over 1536 stripes are 2 per stripe either way
    (3, 3, 8193, "aff", 1536, 768, dict(tps=5, W=2, groups=1536, bend=4, tail=1, tblk=768, grid=768 + 384)),
    (3, 3, 8193, "aff", 1536, 1024, dict(tps=5, W=2, groups=1536, bend=4, tail=1, tblk=768, grid=768 + 384)),
    (3, 3, 1, "aff", 1, 768, dict(tps=1, W=1, groups=1, bend=1, tail=0, tblk=1, grid=1)),
    (3, 3, 1, "tab", 1, 0, dict(tps=1, W=1, groups=1, bend=1, tail=0, tblk=1, grid=1)),
])
def test_known_answers(records, k, m, length, lay, nst, res, want):
    bs, _ = records
    (n, st), = bs[k, m, length, lay, nst, res]["runs"]
    assert n == 1 and {f: st[f] for f in want} == want


@pytest.mark.skipif(shutil.which("nm") is None, reason="no nm")
def test_the_library_holds_exactly_the_networks_kernels():
    """One gf_bs_crc_kernel instantiation per (network, m) of crc_routes.NETWORKS, and the product-alone
    form for the two wide LRC modes only: the network table adds and drops none."""
    import re
    out = subprocess.run(["nm", "-C", os.path.join(LIBDIR, "libcfsec.so")], check=True, capture_output=True, text=True).stdout
    got = set(re.findall(r"__device_stub__gf_bs_crc_kernel<cfsec::dev::Bs(\w+), (\d+), (true|false)>", out))
    want = {(name.capitalize(), str(m), "true") for _, _, ms, name in R.NETWORKS for m in ms}
    want |= {("Ec6p6l9", "15", "false"), ("Ec6p8l10", "18", "false")}
    assert got == want
