"""The route, accepts and launch plan of Reconstruct + Verify jobs with every row checksummed
(MatVecMode::kStoreVerify through matvec_crc_route / plan_matvec_crc, kernels.hpp), pinned on the CPU:
no device, nothing launched.

tests/crc_sv_route_driver.cpp links libcfsec.so and prints the library's answers for k in {3, 4, 6, 8,
10, 12, 15, 16, 18}, m in 1..7, nstore in 0..m, in five variants -- every slot set with one length and
the Verify words given (full), a skipped input slot (skip), per-stripe lengths (lens), no Verify words
(noflags) and the same job as a kStore (store, the control: those answers must not move) -- over the
lengths of tests/test_crc_route.py and three stripe layouts (one stripe, 5 stripes at one pitch, 20
stripes without a common stride).  One driver process per CFSEC_SV_CRC setting (read once).

Asserted: accepts == (route != none); the route equals the restatement below (gf_crc_sv_kernel is
instantiated for k in {6, 8, 12, 16, 18} and m in 2..6 and needs a stored and a compared row, every row
checksummed, one length and the Verify words); the plan of a routed job is the v_perm kernels' plan
with the plain product (4 KiB tiles, ~1024 workgroups per launch, at most 384 per stripe, 96 / (k + m)
stripes per pointer-table launch); a job without a route has an empty plan."""
import os
import shutil
import subprocess

import pytest

import crc_routes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chubaofs_amd", "csrc")
LIBDIR = os.path.join(ROOT, "chubaofs_amd")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

MIB512 = 512 << 20
LENS = [1, 2048, 2049, MIB512, MIB512 + 1, 0xFFFFFFFF - 4096]  # tests/test_crc_route.py
EXTRA_LENS = [8209, 0xFFFFFFFF - 4095]  # the GPU tests' size; one byte past the largest length
KS = [3, 4, 6, 8, 10, 12, 15, 16, 18]
SV_K, SV_M = (6, 8, 12, 16, 18), (2, 3, 4, 5, 6)
VARIANTS = ["full", "skip", "lens", "noflags", "store"]
LAYOUTS = {"one": (1, False), "affine": (5, True), "table": (20, False)}
PITCH = 1 << 33
TILE, GROUPS, MAX_GROUPS, PTRS = 4096, 1024, 384, 96
MAX_LEN = 0xFFFFFFFF - 4096


def _compiler():
    return shutil.which("g++") or shutil.which("hipcc") or shutil.which(os.path.join(ROCM, "bin", "hipcc"))


pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("crc_sv_route") / "crc_sv_route_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "crc_sv_route_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


_records = {}


def records(driver, sv):
    if sv in _records:
        return _records[sv]
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFSEC_")}
    if sv is not None:
        env["CFSEC_SV_CRC"] = str(sv)
    r = subprocess.run([driver] + [str(x) for x in LENS + EXTRA_LENS], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        f = line.split()
        assert f[0] == "sv" and len(f) == 22, line
        out.append(dict(k=int(f[1]), m=int(f[2]), nstore=int(f[3]), variant=f[4], len=int(f[5]), layout=f[6],
                        nst=int(f[7]), route=f[8], accepts=int(f[9]), plan=tuple(int(x) for x in f[10:])))
    _records[sv] = out
    return out


def expect_sv_route(k, m, nstore, variant, length, on):
    """gf_crc_sv_kernel's conditions, from the kernel: K and M are template arguments instantiated for
    SV_K x SV_M; row 0 is always stored and the last row always compared; it checksums every row into
    the slot given, takes one length from its argument block and writes the launch's Verify words."""
    ok = (on and variant == "full" and k in SV_K and m in SV_M and 0 < nstore < m and length <= MAX_LEN)
    return "v_perm" if ok else "none"


def expect_plan(k, m, length, nst, affine):
    """(tiles, per, dy, sstride, groups, tpw, grid_x, grid_y, ends, end[0], end[-1], sum of ends)."""
    tiles = -(-length // TILE)
    sstride = (k + m) * PITCH if affine and nst > 1 else 0
    per = min(nst if sstride else PTRS // (k + m), 65535)
    fit = min(tiles, max(1, GROUPS // min(nst, per)), MAX_GROUPS)
    tpw = -(-tiles // fit)
    groups = -(-tiles // tpw)
    end = [min((g + 1) * tpw, tiles) * TILE for g in range(groups)]
    return (tiles, per, 0, sstride, groups, tpw, groups, min(nst, per), len(end), end[0], end[-1], sum(end))


def test_the_grid_is_the_one_asked_for(driver):
    rec = records(driver, None)
    want = {(k, m, ns, v, length, lay) for k in KS for m in range(1, 8) for ns in range(m + 1) for v in VARIANTS
            for length in LENS + EXTRA_LENS for lay in LAYOUTS}
    assert {(r["k"], r["m"], r["nstore"], r["variant"], r["len"], r["layout"]) for r in rec} == want
    assert len(rec) == len(want)
    assert all(r["nst"] == LAYOUTS[r["layout"]][0] for r in rec)


@pytest.mark.parametrize("sv", [None, 1, 0])
def test_accepts_is_having_a_route(driver, sv):
    for r in records(driver, sv):
        assert r["accepts"] == (r["route"] != "none"), r


@pytest.mark.parametrize("sv", [None, 1, 0])
def test_route_is_the_restated_table(driver, sv):
    on = sv != 0
    seen, seen_shapes = set(), set()
    for r in records(driver, sv):
        if r["variant"] == "store":  # the control: a kStore job's route, whatever the new switch says
            want = R.expect_route(r["k"], r["m"], True, r["len"], r["nst"])
            if (r["k"], r["m"]) not in seen_shapes:  # the driver's matrix matches no network
                seen_shapes.add((r["k"], r["m"]))
                coef = bytes(1 + (i * 37 + 11) % 255 for i in range(r["k"] * r["m"]))
                assert R.match_bits(r["k"], r["m"], coef) == 0
        else:
            want = expect_sv_route(r["k"], r["m"], r["nstore"], r["variant"], r["len"], on)
        assert r["route"] == want, r
        seen.add((r["variant"], r["route"]))
    assert (("full", "v_perm") in seen) == on
    assert {v for v, route in seen if route != "none"} == ({"full", "store"} if on else {"store"})


def test_routed_shapes_are_the_instantiated_ones(driver):
    got = {(r["k"], r["m"], r["nstore"]) for r in records(driver, None)
           if r["variant"] == "full" and r["route"] == "v_perm"}
    assert got == {(k, m, ns) for k in SV_K for m in SV_M for ns in range(1, m)}
    assert len(got) == 5 * (1 + 2 + 3 + 4 + 5)


@pytest.mark.parametrize("sv", [None, 0])
def test_plan_is_the_restated_one(driver, sv):
    for r in records(driver, sv):
        if r["variant"] == "store":
            continue  # pinned by tests/test_crc_plan.py
        if r["route"] == "none":
            assert r["plan"] == (0,) * 12, r
            continue
        nst, affine = LAYOUTS[r["layout"]]
        assert r["plan"] == expect_plan(r["k"], r["m"], r["len"], nst, affine), r


def test_plan_of_the_gpu_tests_sizes(driver):
    """S = 8209 is two whole tiles and a ragged one: a single stripe gets a workgroup per tile, and 1024
    stripes at one pitch get one workgroup each that walks all three."""
    assert expect_plan(12, 4, 8209, 1, False)[:6] == (3, 6, 0, 0, 3, 1)
    assert expect_plan(12, 4, 8209, 1024, True)[4:8] == (1, 3, 1, 1024)
    (r,) = [r for r in records(driver, None) if (r["k"], r["m"], r["nstore"], r["variant"], r["len"], r["layout"])
            == (12, 4, 1, "full", 8209, "affine")]
    assert r["plan"][:8] == (3, 5, 0, 16 * PITCH, 3, 1, 3, 5)
