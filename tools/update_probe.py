#!/usr/bin/env python3
"""update_probe.py -- what Update, EncodeIdx and ReconstructSome cost beside the calls they replace.

One process on one GPU, three tables:

  update   cfsec_rs_update_batch of 1, 2 and k/2 changed columns against cfsec_rs_encode_batch of the
           same stripes (before Update existed a full re-encode was the only way to the same parity):
           EC12P4 and EC6P6 at 8 stripes of 5,592,406 bytes, EC16P20 at 64 stripes of 262,144 bytes,
           pitched stripes in HBM.  Device events around `inner` back-to-back calls on one stream; the
           bytes each side must move -- (3 nc + 2 m) S against (k + m) S per stripe -- over the time is
           its achieved rate, given as a share of the 8 TB/s HBM peak.
  idx      k cfsec_rs_encode_idx calls (one per data shard) against one cfsec_rs_encode of the same
           stripe in HBM: wall time around the synchronous calls, launch and wait included.
  some     cfsec_rs_reconstruct_some_stripes with one of two missing data shards required against
           cfsec_rs_reconstruct_data_stripes, 64 scattered EC12P4 segments of 16 KiB and 64 KiB in HBM:
           wall time per call over 64, microseconds per segment.

Every figure is the median of --reps samples after --warmup untimed turns of the same shape; the two
sides of a comparison take turns sample by sample.  There is no CPU path: without a GPU the tool fails.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chubaofs_amd import _lib, reedsolomon  # noqa: E402

HBM_PEAK = 8e12


def alternate(sides, warmup, reps):
    for _ in range(warmup):
        for s in sides:
            s()
    out = [[] for _ in sides]
    for _ in range(reps):
        for o, s in zip(out, sides):
            o.append(s())
    return [statistics.median(o) for o in out]


def event_timed(torch, fn, inner):
    """Microseconds per call of `inner` back-to-back calls of fn, by device events on the current stream."""
    def sample():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / inner
    return sample


def update_table(torch, a, emit):
    emit("update: us per call (device events), bytes-moved ratio, share of 8 TB/s; median of %d x %d calls" % (a.reps, a.inner))
    emit("%-8s %3s %9s %4s %10s %10s %7s %7s %8s %8s" % ("mode", "st", "S", "nc", "update", "encode", "t-ratio", "b-ratio",
                                                         "upd-bw", "enc-bw"))
    for k, m, ns, S in ((12, 4, 8, 5592406), (6, 6, 8, 5592406), (16, 20, 64, 262144)):
        enc = reedsolomon.New(k, m, device=0)
        pitch = (S + 255) // 256 * 256
        width = k + m + k // 2  # a stripe's rows, then room for the new columns
        buf = torch.randint(0, 256, (ns * width * pitch,), dtype=torch.uint8, device="cuda")
        base = buf.data_ptr()
        ptrs = _lib_ptrs([base + (s * width + i) * pitch for s in range(ns) for i in range(k + m)])
        enc.encode_batch(ptrs, S, ns)
        for nc in (1, 2, k // 2):
            cols = list(range(nc))
            new = _lib_ptrs([base + (s * width + k + m + j) * pitch for s in range(ns) for j in range(nc)])
            upd, full = alternate([event_timed(torch, lambda: enc.update_batch(ptrs, new, cols, S, ns), a.inner),
                                   event_timed(torch, lambda: enc.encode_batch(ptrs, S, ns), a.inner)], a.warmup, a.reps)
            ub, eb = (3 * nc + 2 * m) * S * ns, (k + m) * S * ns
            emit("EC%dP%-4d %3d %9d %4d %10.1f %10.1f %7.2f %7.2f %7.1f%% %7.1f%%" %
                 (k, m, ns, S, nc, upd, full, upd / full, ub / eb, 100 * ub / (upd * 1e-6) / HBM_PEAK,
                  100 * eb / (full * 1e-6) / HBM_PEAK))
        del buf
        torch.cuda.synchronize()


def _lib_ptrs(v):
    return (ctypes.c_void_p * len(v))(*v)


def wall(fn):
    def sample():
        t0 = time.perf_counter_ns()
        fn()
        return (time.perf_counter_ns() - t0) / 1e3
    return sample


def idx_table(torch, a, emit):
    emit("idx: us (wall, synchronous calls in HBM); median of %d" % a.reps)
    emit("%-8s %9s %12s %12s %7s" % ("mode", "S", "k EncodeIdx", "Encode", "ratio"))
    for k, m, S in ((12, 4, 5592406), (6, 6, 5592406)):
        enc = reedsolomon.New(k, m, device=0)
        sh = [torch.randint(0, 256, (S,), dtype=torch.uint8, device="cuda") for _ in range(k + m)]
        torch.cuda.synchronize()

        # the shard headers built once: the C calls alone are timed
        arr = (_lib.Shard * (k + m))(*[_lib.Shard(t.data_ptr(), S, S) for t in sh])
        one = [(_lib.Shard * 1)(arr[i]) for i in range(k)]
        par = (_lib.Shard * m)(*[arr[k + r] for r in range(m)])
        L, h = enc._L, enc._h

        def steps():
            for i in range(k):
                _lib.check(L.cfsec_rs_encode_idx(h, one[i], i, par, m, _lib.MEM_DEVICE, None))

        def encode():
            _lib.check(L.cfsec_rs_encode(h, arr, k + m, _lib.MEM_DEVICE, None))

        parts, whole = alternate([wall(steps), wall(encode)], a.warmup, a.reps)
        emit("EC%dP%-4d %9d %12.1f %12.1f %7.2f" % (k, m, S, parts, whole, parts / whole))


def some_table(torch, a, emit):
    emit("some: 64 scattered EC12P4 segments in HBM, data shards 0 and 1 missing; us per segment (wall); median of %d" % a.reps)
    emit("%8s %16s %16s" % ("seg", "some (1 required)", "ReconstructData"))
    k, m, B = 12, 4, 64
    n = k + m
    enc = reedsolomon.New(k, m, device=0)
    for S in (16 << 10, 64 << 10):
        pitch = (S + 255) // 256 * 256
        pos, at = [], 0
        for i in range(B):
            at += 256 * ((i * 7) % 5 + 1)
            pos.append(at)
            at += n * pitch
        buf = torch.randint(0, 256, (at,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        base = buf.data_ptr()
        arr = (_lib.Shard * (B * n))()
        status = (ctypes.c_int * B)()
        req = (ctypes.c_uint8 * (B * k))()
        for i in range(B):
            req[i * k] = 1

        def reset():
            for i in range(B):
                for j in range(n):
                    arr[i * n + j] = _lib.Shard(base + pos[i] + j * pitch, 0 if j < 2 else S, S)

        def call(fn, *extra):
            def sample():
                reset()
                t0 = time.perf_counter_ns()
                rc = fn(enc._h, arr, B, *extra, _lib.MEM_DEVICE, status)
                dt = time.perf_counter_ns() - t0
                if rc or any(status[i] for i in range(B)):
                    raise RuntimeError("stripes call failed: rc %d" % rc)
                return dt / 1e3 / B
            return sample

        some, data = alternate([call(enc._L.cfsec_rs_reconstruct_some_stripes, req),
                                call(enc._L.cfsec_rs_reconstruct_data_stripes)], a.warmup, a.reps)
        emit("%8d %16.2f %16.2f" % (S, some, data))
        del buf


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per event-timed sample")
    ap.add_argument("--out", help="also write the tables to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("update_probe: no GPU; nothing is measured without one")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(_lib.lib().cfsec_version().decode() + " on " + torch.cuda.get_device_name(0))
    update_table(torch, a, emit)
    emit("")
    idx_table(torch, a, emit)
    emit("")
    some_table(torch, a, emit)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
