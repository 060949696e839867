"""Which way a single-stripe call takes (RSEngine::run), pinned on the CPU: no device, nothing launched.

tests/call_path_driver.cpp links libcfsec.so and calls single_call_path (engine.hpp), the host-only
decision run switches on.  The facts are made up here; the expected path of every row is written out
by hand: device memory in place; host memory with every row page-locked in place; other host calls
that move at most 1 MiB through a page-locked stage when there is a usable one, else through the
chunked pipeline; and the Verify of more than 32 inputs, which no single launch carries, through
whole-row staging.  tests/test_gpu_host.py runs each path against the oracle.
"""
import os
import subprocess

import pytest

from test_crc_route import CSRC, LIBDIR, ROCM, ROOT, _compiler

pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")

MIB = 1 << 20  # RSEngine::kSmallPageable, asked for below


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("call_path") / "call_path_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "call_path_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


def ask(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


# (host, rows_aliasable, stage_usable, moved_bytes, nin, mode) -> path
TABLE = [
    # one row per path
    ((0, 0, 0, 16 * 65536, 12, "store"), "in_place"),
    ((1, 1, 1, 16 * 65536, 12, "store"), "pinned_in_place"),
    ((1, 0, 1, 16 * 4096, 12, "store"), "small_stage"),
    ((1, 0, 1, 16 * MIB, 12, "store"), "pipeline"),
    ((1, 0, 1, 43 * 4096, 40, "verify"), "staged_whole"),
    # device memory is in place whatever else holds (the two-step Verify included: it stages only its product)
    ((0, 1, 1, 1, 40, "verify"), "in_place"),
    ((0, 0, 0, 64 * MIB, 40, "verify"), "in_place"),
    # moved_bytes at kSmallPageable and one byte over
    ((1, 0, 1, MIB, 6, "store"), "small_stage"),
    ((1, 0, 1, MIB + 1, 6, "store"), "pipeline"),
    ((1, 0, 1, MIB, 6, "verify"), "small_stage"),
    ((1, 0, 1, MIB + 1, 6, "verify"), "pipeline"),
    # Verify of 32 inputs is one launch, of 33 two steps; a store of 33 inputs is not two-step
    ((1, 0, 1, 35 * 1000, 32, "verify"), "small_stage"),
    ((1, 0, 1, 36 * 1000, 33, "verify"), "staged_whole"),
    ((1, 0, 1, 36 * 1000, 33, "store"), "small_stage"),
    ((1, 0, 1, 36 * MIB, 32, "verify"), "pipeline"),
    ((1, 0, 1, 36 * MIB, 33, "verify"), "staged_whole"),
    ((1, 0, 1, 36 * MIB, 33, "store"), "pipeline"),
    # the two-step Verify over page-locked rows stays in place
    ((1, 1, 1, 43 * 4096, 40, "verify"), "pinned_in_place"),
    ((1, 1, 0, 43 * MIB, 40, "verify"), "pinned_in_place"),
    # no usable stage: the pipeline takes the small call; the two-step Verify does not need one
    ((1, 0, 0, 16 * 4096, 12, "store"), "pipeline"),
    ((1, 0, 0, MIB, 6, "verify"), "pipeline"),
    ((1, 0, 0, 43 * 4096, 40, "verify"), "staged_whole"),
    # page-locked rows do not need a stage either
    ((1, 1, 0, 16 * 4096, 12, "store"), "pinned_in_place"),
]


def test_the_table_names_every_path():
    assert {want for _, want in TABLE} == {"in_place", "pinned_in_place", "small_stage", "pipeline", "staged_whole"}


def test_small_pageable_is_one_mib(driver):
    assert ask(driver, "small_pageable\n") == [str(MIB)]


@pytest.mark.parametrize("facts,want", TABLE, ids=["-".join(map(str, f)) for f, _ in TABLE])
def test_single_call_path(driver, facts, want):
    assert ask(driver, "%d %d %d %d %d %s\n" % facts) == [want]
