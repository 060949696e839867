"""Measure the mixed-size crc32block launch (cfsec_crc32block_*_objects) beside the batch forms and the
single call, on the GPU.

    python tools/blk_objects_probe.py [--out profiles/r09/blk_objects.txt]

Two child runs of this file, so that tracing does not slow the call timings:
  --part kernels  under `rocprofv3 --kernel-trace`: kernel times, median of REPS launches after WARM, the
                  forms alternating inside one run
                    equal   128 shards of S = 5,592,406 bytes at 64 KiB blocks (DESIGN 4.4's shape):
                            check_objects, decode_objects and decode_batch on the same framed shards,
                            encode_objects and encode_batch on the same payloads
                    mixed   1024 objects, sizes log-uniform in 4 KiB .. 4 MiB (seed 9): check_objects
  --part calls    no profiler, host clock around synchronous calls at the C ABI: one check_objects call over
                  the 1024 mixed objects against 1024 cfsec_crc32block_decode calls, same objects
Rates are payload bytes over kernel time; the share is of the 8 TB/s HBM peak.  check reads every framed
byte and writes none; decode and encode read and write every payload byte.
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 4, 24
N_EQUAL, S_EQUAL, BL = 128, 5592406, 64 * 1024
N_MIXED, SEED = 1024, 9
PEAK = 8e12


def mixed_sizes():
    import numpy as np
    rng = np.random.default_rng(SEED)
    return [int(x) for x in np.exp(rng.uniform(np.log(4096), np.log(4 << 20), N_MIXED))]


class Shards:
    """n payloads and their framed forms in device memory, framed by the library's own encode."""

    def __init__(self, sizes):
        import torch
        from chubaofs_amd import crc32block as C
        self.sizes = sizes
        self.flen = [C.EncodeSize(s, BL) for s in sizes]
        g = torch.Generator(device="cuda").manual_seed(SEED)
        self.pay = [torch.randint(0, 256, (s,), dtype=torch.uint8, device="cuda", generator=g) for s in sizes]
        self.framed = [torch.empty(f, dtype=torch.uint8, device="cuda") for f in self.flen]
        self.out = [torch.empty(s, dtype=torch.uint8, device="cuda") for s in sizes]
        self.enc = [torch.empty(f, dtype=torch.uint8, device="cuda") for f in self.flen]
        st, _, _ = C.objects_call(C.ENCODE, [(p.data_ptr(), 0, f.data_ptr(), s, 0, 0)
                                             for p, f, s in zip(self.pay, self.framed, sizes)], BL)
        assert not any(st)
        self.check = [(f.data_ptr(), n, 0, s, 0, s) for f, n, s in zip(self.framed, self.flen, sizes)]
        self.decode = [(f.data_ptr(), n, o.data_ptr(), s, 0, s) for f, n, o, s in zip(self.framed, self.flen, self.out, sizes)]
        self.encode = [(p.data_ptr(), 0, e.data_ptr(), s, 0, 0) for p, e, s in zip(self.pay, self.enc, sizes)]


def part_kernels(schedule_path):
    import torch
    from chubaofs_amd import crc32block as C
    schedule = []
    eq = Shards([S_EQUAL] * N_EQUAL)
    schedule.append("setup")
    bad = torch.zeros(N_EQUAL, dtype=torch.int32, device="cuda")
    crcs = torch.zeros(N_EQUAL, dtype=torch.int32, device="cuda")
    src = [f.data_ptr() for f in eq.framed]
    dst = [o.data_ptr() for o in eq.out]
    pay = [p.data_ptr() for p in eq.pay]
    enc = [e.data_ptr() for e in eq.enc]
    for _ in range(WARM + REPS):
        C.decode_batch(src, dst, S_EQUAL, bad.data_ptr(), block_len=BL)
        torch.cuda.synchronize()
        assert not any(C.objects_call(C.CHECK, eq.check, BL)[0])
        assert not any(C.objects_call(C.DECODE, eq.decode, BL)[0])
        schedule += ["equal decode_batch", "equal check_objects", "equal decode_objects"]
    assert bad.cpu().view(torch.uint8).min().item() == 255
    for _ in range(WARM + REPS):
        C.encode_batch(pay, enc, S_EQUAL, block_len=BL, shard_crcs_ptr=crcs.data_ptr())
        torch.cuda.synchronize()
        assert not any(C.objects_call(C.ENCODE, eq.encode, BL)[0])
        schedule += ["equal encode_batch", "equal encode_objects"]
    assert all(torch.equal(a, b) for a, b in zip(eq.enc[:4], eq.framed[:4]))
    del eq
    mx = Shards(mixed_sizes())
    schedule.append("setup")
    for _ in range(WARM + REPS):
        assert not any(C.objects_call(C.CHECK, mx.check, BL)[0])
        schedule.append("mixed check_objects")
    with open(schedule_path, "w") as f:
        json.dump(schedule, f)


def part_calls():
    from chubaofs_amd import _lib
    mx = Shards(mixed_sizes())
    L = _lib.lib()
    one, many = [], []
    blk = ctypes.c_int64(-1)
    scratch = mx.out[max(range(N_MIXED), key=lambda i: mx.sizes[i])].data_ptr()
    # the descriptor array is built once, outside the timed window: the C call alone is timed
    arr = (_lib.BlkObject * N_MIXED)()
    for rec, (src, n, _, s, f, t) in zip(arr, mx.check):
        rec.src, rec.src_len, rec.dst, rec.size, rec.from_, rec.to = src, n, None, s, f, t
    status, bad, crc = (ctypes.c_int * N_MIXED)(), (ctypes.c_int64 * N_MIXED)(), (ctypes.c_uint32 * N_MIXED)()
    for r in range(WARM + 20):
        t0 = time.perf_counter()
        st = L.cfsec_crc32block_check_objects(arr, N_MIXED, BL, status, bad, crc, _lib.MEM_DEVICE, -1, None)
        t1 = time.perf_counter()
        assert st == 0 and not any(status)
        if r >= WARM:
            one.append(t1 - t0)
    for r in range(2 + 5):
        t0 = time.perf_counter()
        for src, n, _, s, _, _ in mx.check:
            if L.cfsec_crc32block_decode(src, n, s, BL, 0, s, scratch, ctypes.byref(blk), _lib.MEM_DEVICE, -1, None):
                raise SystemExit("single decode failed")
        t1 = time.perf_counter()
        if r >= 2:
            many.append(t1 - t0)
    print(json.dumps({"payload": sum(mx.sizes), "one_call_s": statistics.median(one), "single_calls_s": statistics.median(many)}))


def kernel_times(trace_dir, schedule):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "crc32block" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    # "setup" is the one encode_objects launch that frames a shard set
    if len(rows) != len(schedule):
        raise SystemExit(f"{len(rows)} crc32block launches in the trace, {len(schedule)} scheduled")
    by = {}
    for (t0, t1, name), label in zip(rows, schedule):
        want = "objects_kernel" if "objects" in label or label == "setup" else "block_kernel"
        assert want in name, (label, name)
        by.setdefault(label, []).append((t1 - t0) * 1e-9)
    return {k: statistics.median(v[WARM:]) for k, v in by.items() if k != "setup"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "calls"])
    ap.add_argument("--schedule")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "blk_objects.txt"))
    a = ap.parse_args()
    if a.part == "kernels":
        return part_kernels(a.schedule)
    if a.part == "calls":
        return part_calls()
    me = os.path.abspath(__file__)
    calls = json.loads(subprocess.run([sys.executable, me, "--part", "calls"], check=True, capture_output=True, text=True,
                                      timeout=600).stdout.strip().splitlines()[-1])
    with tempfile.TemporaryDirectory() as tmp:
        sched = os.path.join(tmp, "schedule.json")
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, "trace"), "-o", "run", "--",
                        sys.executable, me, "--part", "kernels", "--schedule", sched], check=True, timeout=900,
                       stdout=subprocess.DEVNULL)
        with open(sched) as f:
            kt = kernel_times(os.path.join(tmp, "trace"), json.load(f))
    eq_bytes = N_EQUAL * S_EQUAL
    lines = [f"crc32block objects probe: kernel times from rocprofv3 --kernel-trace, median of {REPS} after {WARM} warm-up,",
             "forms alternating in one run; payload bytes over kernel time; share of the 8 TB/s HBM peak", "",
             f"equal sizes: {N_EQUAL} shards of {S_EQUAL} bytes, block_len {BL}",
             f"{'kernel':28s} {'us':>9s} {'payload TB/s':>13s} {'of 8 TB/s':>10s}"]
    for k in ("equal decode_batch", "equal check_objects", "equal decode_objects", "equal encode_batch", "equal encode_objects"):
        lines.append(f"{k[6:]:28s} {kt[k] * 1e6:9.1f} {eq_bytes / kt[k] / 1e12:13.2f} {eq_bytes / kt[k] / PEAK * 100:9.1f}%")
    lines += ["", f"check_objects / decode_batch kernel time: {kt['equal check_objects'] / kt['equal decode_batch']:.3f}",
              f"decode_objects / decode_batch: {kt['equal decode_objects'] / kt['equal decode_batch']:.3f}   "
              f"encode_objects / encode_batch: {kt['equal encode_objects'] / kt['equal encode_batch']:.3f}", ""]
    mp = calls["payload"]
    k = kt["mixed check_objects"]
    lines += [f"mixed sizes: {N_MIXED} objects, log-uniform 4 KiB .. 4 MiB (seed {SEED}), {mp} payload bytes, block_len {BL}",
              f"check_objects kernel {k * 1e6:.1f} us, {mp / k / 1e12:.2f} payload TB/s ({mp / k / PEAK * 100:.1f}% of 8 TB/s)",
              "synchronous calls at the C ABI, host clock, device memory (median of 20 / of 5 loops):",
              f"{'':34s} {'total us':>10s} {'us per object':>14s}",
              f"{'one check_objects call':34s} {calls['one_call_s'] * 1e6:10.1f} {calls['one_call_s'] * 1e6 / N_MIXED:14.2f}",
              f"{'1024 cfsec_crc32block_decode calls':34s} {calls['single_calls_s'] * 1e6:10.1f} "
              f"{calls['single_calls_s'] * 1e6 / N_MIXED:14.2f}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
