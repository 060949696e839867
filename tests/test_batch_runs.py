"""The host arithmetic of a batch call (batch.cpp), pinned on the CPU: no device, nothing launched.

tests/batch_runs_driver.cpp links libcfsec.so and calls the two pure functions engine.hpp declares:
split_runs, the stripe ranges [t0, t1) a launch group is launched in (affine runs of at least 4 stripes,
the rest gathered into pointer-table runs), and pack_chunk, which staged tasks share a staging lane and
at which offsets.  The addresses are made up here and never dereferenced; the expected ranges and
offsets are written out by hand.
"""
import os
import subprocess

import pytest

from test_crc_route import CSRC, LIBDIR, ROCM, ROOT, _compiler

pytestmark = pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")

PITCH = 1 << 20  # between the rows of one stripe
A, B, C = 0x10000000, 0x20000000, 0x30000000


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("batch_runs") / "batch_runs_driver"
    subprocess.run([_compiler(), "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + CSRC, os.path.join(ROOT, "tests", "batch_runs_driver.cpp"), "-o", str(exe),
                    "-L" + LIBDIR, "-lcfsec", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True, timeout=300)
    return str(exe)


def ask(driver, text):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def affine(base, stride, nt, rows):
    """nt stripes of `rows` rows: stripe t = stripe 0 + t * stride on every row."""
    return [[base + t * stride + r * PITCH for r in range(rows)] for t in range(nt)]


def scattered(t0, nt, rows):
    """Stripes whose rows sit at unrelated addresses: the step from any stripe differs from row to row."""
    return [[0x40000000 + (7 * t + 13 * r) ** 2 * 4096 for r in range(rows)] for t in range(t0, t0 + nt)]


def runs(driver, stripes, k=2, m=1, mo=0, lens=None):
    lens = lens or [4096] * len(stripes)
    assert all(len(s) == k + m + mo for s in stripes)
    text = "runs %d %d %d %d\n" % (k, m, mo, len(stripes))
    text += "".join("%d %s\n" % (n, " ".join(map(str, s))) for n, s in zip(lens, stripes))
    (line,) = ask(driver, text)
    f = [int(x) for x in line.split()]
    return list(zip(f[0::2], f[1::2]))


def test_under_three_stripes_there_is_no_splitting(driver):
    assert runs(driver, scattered(0, 2, 3)) == [(0, 2)]
    assert runs(driver, affine(A, 4096, 2, 3)) == [(0, 2)]


def test_affine_stripes_are_one_run(driver):
    assert runs(driver, affine(A, 4096, 8, 3)) == [(0, 8)]


def test_unrelated_addresses_are_one_pointer_table_run(driver):
    assert runs(driver, scattered(0, 8, 3)) == [(0, 8)]


def test_affine_scattered_affine(driver):
    stripes = affine(A, 4096, 4, 3) + scattered(4, 3, 3) + affine(B, 4096, 5, 3)
    assert runs(driver, stripes) == [(0, 4), (4, 7), (7, 12)]


def test_short_affine_pieces_merge(driver):
    stripes = affine(A, 4096, 2, 3) + affine(B, 8192, 2, 3) + affine(C, 12288, 2, 3)
    assert runs(driver, stripes) == [(0, 6)]


def test_two_long_runs_of_different_stride(driver):
    stripes = affine(A, 4096, 5, 3) + affine(B, 8192, 5, 3)
    assert runs(driver, stripes) == [(0, 5), (5, 10)]


def test_one_output_row_a_byte_off(driver):
    # stripes 4 -> 5 and 5 -> 6 both break the stride: the long run ends at 5; stripe 5 alone and the
    # run 6..7 behind it are both shorter than 4 stripes, so they are gathered into one table run
    stripes = affine(A, 4096, 8, 3)
    stripes[5][2] += 1
    assert runs(driver, stripes) == [(0, 5), (5, 8)]


def test_stride_zero_is_not_an_affine_run(driver):
    assert runs(driver, affine(A, 0, 8, 3)) == [(0, 8)]


def test_one_length_different_skips_splitting(driver):
    stripes = affine(A, 4096, 4, 3) + scattered(4, 4, 3)  # would split at 4 with one length
    assert runs(driver, stripes) == [(0, 4), (4, 8)]
    assert runs(driver, stripes, lens=[4096] * 6 + [2048, 4096]) == [(0, 8)]
    assert runs(driver, affine(A, 4096, 8, 3), lens=[4096] * 3 + [4095] + [4096] * 4) == [(0, 8)]


def test_dy16_output_rows_break_a_run(driver):
    # a 16-input plan with 2 product rows and the 22 rows of the dy16 launch (2 missing data rows + 20
    # parity rows); only one of those 22 is off, in stripe 6: 0..5 stay affine, 6 and 7..9 are short
    k, m, mo = 16, 2, 22
    stripes = affine(A, 8192, 10, k + m + mo)
    assert runs(driver, stripes, k, m, mo) == [(0, 10)]
    stripes[6][k + m + 3] += 256
    assert runs(driver, stripes, k, m, mo) == [(0, 6), (6, 10)]


def pack(driver, lane_bytes, tasks):
    """tasks: (len, nin, nout, nstore).  Returns [(i0, i1, [offsets])] per chunk."""
    text = "pack %d %d\n" % (lane_bytes, len(tasks)) + "".join("%d %d %d %d\n" % t for t in tasks)
    (line,) = ask(driver, text)
    out = []
    for part in line.split("|")[1:]:
        f = [int(x) for x in part.split()]
        out.append((f[0], f[1], f[2:]))
    return out


def test_a_lane_of_one_tasks_bytes_holds_one_task(driver):
    # 1000 bytes -> 1024-byte slots, 3 rows: 3072 bytes
    assert pack(driver, 3072, [(1000, 2, 1, 1)] * 3) == [(i, i + 1, [0, 1024, 2048]) for i in range(3)]
    assert pack(driver, 6144, [(1000, 2, 1, 1)] * 3) == [(0, 2, [0, 1024, 2048, 3072, 4096, 5120]),
                                                        (2, 3, [0, 1024, 2048])]


def test_a_task_larger_than_the_lane_goes_alone(driver):
    small, big = (100, 2, 1, 1), (1000, 2, 1, 1)  # 768 and 3072 bytes, lane of 1024
    assert pack(driver, 1024, [small, big, small]) == [(0, 1, [0, 256, 512]), (1, 2, [0, 1024, 2048]),
                                                       (2, 3, [0, 256, 512])]
    assert pack(driver, 1024, [big, big]) == [(0, 1, [0, 1024, 2048]), (1, 2, [0, 1024, 2048])]


def test_slots_are_the_length_rounded_up_to_256(driver):
    tasks = [(1, 2, 1, 1), (256, 2, 1, 1), (257, 2, 1, 1)]
    assert pack(driver, 1 << 20, tasks) == [(0, 3, [0, 256, 512, 768, 1024, 1280, 1536, 2048, 2560])]


def test_compared_rows_take_slots_too(driver):
    # Verify of whole stripes (nstore = 0): 2 inputs + 2 compared rows of 256 bytes fill a 1024-byte lane
    assert pack(driver, 1024, [(256, 2, 2, 0)] * 2) == [(0, 1, [0, 256, 512, 768]), (1, 2, [0, 256, 512, 768])]
