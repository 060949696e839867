"""The launches of the delta-accumulate kernels (plan_delta, gf_delta.hpp), pinned on the CPU: no
device, nothing launched.

tests/delta_plan_driver.cpp links libcfsec.so and prints the plan of every job below: shapes (columns,
rows) x both input modes x lengths around the 16-byte lane chunk and the 4 KiB tile and the longest
shard x layouts -- one stripe; two affine stripes; the same with one row 1 byte off; scattered stripes
at the pointer-table capacity of the job's first launch and one above it.  Row addresses are
synthesised, never dereferenced.

Asserted: (a) the steps cover every (row, column, stripe, byte) exactly once; (b) every column's delta
is formed exactly once, in a launch that precedes every plain launch reading that column; (c) no
delta-forming step shares a column chunk between waves; (d) every step names a kernel that exists and
holds its rows; (e) a step's pointers fit the argument block, affine runs are found where the layout
is affine, and the capacity layouts split where they must.
"""
import os
import subprocess

import numpy as np
import pytest

from test_crc_route import CSRC, LIBDIR, ROCM, ROOT, _compiler

pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")

SHAPES = [(1, 4), (2, 4), (12, 4), (6, 6), (16, 20), (16, 22), (3, 33), (33, 2), (40, 3)]
LENS = [1, 15, 16, 17, 4095, 4096, 4097, 2 ** 32 - 1 - 4096]
PTR_SLOTS, MAX_COLS, MAX_ROWS, TILE = 288, 32, 32, 4096
STEP_FIELDS = ("delta", "r0", "mc", "c0", "kc", "s0", "ns", "M", "OS", "len", "affine", "tile", "gx", "gy", "exists")


def capacity(nc, m, delta):
    """Stripes the first launch of a scattered job holds: 2 kc + mc pointers each when it forms deltas."""
    return PTR_SLOTS // ((2 if delta else 1) * min(nc, MAX_COLS) + min(m, MAX_ROWS))


def jobs():
    out = []
    for nc, m in SHAPES:
        for delta in (1, 0):
            cap = capacity(nc, m, delta)
            for ln in LENS:
                out += [(nc, m, delta, ln, "aff", 1), (nc, m, delta, ln, "aff", 2), (nc, m, delta, ln, "aff1", 2),
                        (nc, m, delta, ln, "scat", cap), (nc, m, delta, ln, "scat", cap + 1)]
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("delta_plan") / "delta_plan_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "delta_plan_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


def run_driver(driver, specs):
    """The plans of the jobs `specs` (nc, m, delta, len, layout, nstripes), in order."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CFSEC_")}
    r = subprocess.run([driver] + [":".join(map(str, j)) for j in specs], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    plans = []
    for line in r.stdout.splitlines():
        f = line.split()
        assert f[0] == "job"
        steps = [dict(zip(STEP_FIELDS, map(int, s.split(",")))) for s in ([] if f[8] == "-" else f[8].split(";"))]
        plans.append(dict(nc=int(f[1]), m=int(f[2]), delta=int(f[3]), len=int(f[4]), layout=f[5], ns=int(f[6]),
                          error=int(f[7]), steps=steps))
    assert len(plans) == len(specs)
    return plans


@pytest.fixture(scope="module")
def plans(driver):
    return run_driver(driver, jobs())


def check_plan(p):
    nc, m, ns, ln = p["nc"], p["m"], p["ns"], p["len"]
    assert p["error"] == 0 and p["steps"], p
    cover = np.zeros((m, nc, ns), np.int32)       # launches coding (row, column, stripe)
    formed = np.zeros((nc, ns), np.int32)         # launches forming the delta of (column, stripe)
    formed_at = np.full((nc, ns), -1, np.int64)
    for i, s in enumerate(p["steps"]):
        rows, cols, stripes = slice(s["r0"], s["r0"] + s["mc"]), slice(s["c0"], s["c0"] + s["kc"]), slice(s["s0"], s["s0"] + s["ns"])
        assert 0 < s["mc"] <= MAX_ROWS and 0 < s["kc"] <= MAX_COLS and s["ns"] > 0
        assert s["r0"] + s["mc"] <= m and s["c0"] + s["kc"] <= nc and s["s0"] + s["ns"] <= ns
        # (a) every byte of the rows, once: one workgroup per tile of the whole length
        assert s["len"] == ln and s["tile"] == TILE and s["gx"] == -(-ln // TILE) and s["gy"] == s["ns"]
        assert s["gx"] < 2 ** 31 and s["gy"] <= 65535
        cover[rows, cols, stripes] += 1
        if s["delta"]:
            assert p["delta"] and s["OS"] == 1                       # (c)
            formed[cols, stripes] += 1
            formed_at[cols, stripes] = i
        else:
            # (b) a plain launch of a delta job reads columns whose delta an earlier launch has stored
            assert not p["delta"] or ((formed[cols, stripes] == 1).all() and (formed_at[cols, stripes] < i).all()), (p, i)
        assert s["exists"] == 1 and s["M"] >= s["mc"]                 # (d)
        if not s["affine"]:                                           # (e)
            assert s["ns"] * ((2 if s["delta"] else 1) * s["kc"] + s["mc"]) <= PTR_SLOTS, (p, s)
    assert (cover == 1).all(), p
    assert (formed == (1 if p["delta"] else 0)).all(), p
    return p["steps"]


def test_every_plan_covers_once_forms_each_delta_once_and_names_a_kernel(plans):
    assert len(plans) == len(SHAPES) * 2 * len(LENS) * 5
    for p in plans:
        check_plan(p)


def test_layouts_decide_affine_runs_and_table_splits(plans):
    for p in plans:
        chunks = -(-p["nc"] // MAX_COLS) * -(-p["m"] // MAX_ROWS)  # (column chunk, row chunk) pairs
        runs = [s for s in p["steps"] if s["c0"] == 0 and s["r0"] == 0]
        if p["layout"] == "aff":
            assert len(p["steps"]) == chunks and all(s["affine"] == (p["ns"] > 1) for s in p["steps"]), p
        elif p["layout"] == "aff1":
            # the odd row is the last output row: only the launches holding it lose the affine form
            last = [s for s in p["steps"] if s["r0"] + s["mc"] == p["m"]]
            assert last and all(not s["affine"] for s in last), p
            assert all(s["affine"] for s in p["steps"] if s not in last), p
        else:
            cap = capacity(p["nc"], p["m"], p["delta"])
            assert all(not s["affine"] for s in p["steps"]), p
            assert [s["ns"] for s in runs] == ([cap] if p["ns"] == cap else [cap, 1]), p


def test_named_edges(plans):
    def find(nc, m, delta, ln, layout, ns):
        (p,) = [p for p in plans if (p["nc"], p["m"], p["delta"], p["len"], p["layout"], p["ns"]) == (nc, m, delta, ln, layout, ns)]
        return p["steps"]
    # one changed column of EC12P4-like parity: one launch, the 4-row kernel
    (s,) = find(1, 4, 1, 4097, "aff", 1)
    assert (s["delta"], s["M"], s["gx"]) == (1, 4, 2)
    # 22 rows run on the 24-row instantiation; 20 on their own
    assert find(16, 22, 1, 4096, "aff", 1)[0]["M"] == 24 and find(16, 20, 0, 4096, "aff", 1)[0]["M"] == 20
    # 33 rows: the first 32 form the deltas, the 33rd is a plain launch over the rewritten columns
    a, b = find(3, 33, 1, 17, "aff", 1)
    assert (a["delta"], a["r0"], a["mc"], a["M"]) == (1, 0, 32, 32) and (b["delta"], b["r0"], b["mc"], b["M"]) == (0, 32, 1, 1)
    # 33 and 40 columns: two column chunks, each forming its own columns' deltas
    for nc, m in ((33, 2), (40, 3)):
        a, b = find(nc, m, 1, 4095, "aff", 2)
        assert (a["delta"], a["c0"], a["kc"]) == (1, 0, 32) and (b["delta"], b["c0"], b["kc"]) == (1, 32, nc - 32)
    # the longest shard: 2^20 tiles
    assert find(12, 4, 1, 2 ** 32 - 1 - 4096, "aff", 1)[0]["gx"] == 2 ** 20 - 1


def test_empty_jobs_plan_nothing(driver):
    for p in run_driver(driver, [(2, 4, 1, 0, "aff", 2), (2, 4, 1, 100, "aff", 0), (2, 0, 1, 100, "aff", 2)]):
        assert p["error"] == 0 and p["steps"] == []
