#!/usr/bin/env python3
"""seg_batch_probe.py -- what a degraded read costs per segment, batched against one call per segment.

access rebuilds the byte range of a degraded Get with ReconstructData over every shard's segment
(access/stream_get.go:384-431).  This tool times, in one process on one GPU,

  * one cfsec_ec_reconstruct_data_batch call over B segments, divided by B, beside
  * a loop of B cfsec_ec_reconstruct_data calls over the same segments, divided by B

for EC6P6 and EC12P4 with two bad data shards, segments of 4 KiB and 64 KiB, B in {1, 16, 64, 256},
every segment with the same bad set ("one") or the bad sets cycling through every pair of data shards
("distinct": 15 patterns for EC6P6, 66 for EC12P4), on HBM and on page-locked host memory.  The
segments of a batch sit at irregular distances from each other, as separately read blobs do, so no
launch can treat them as one strided array.

--sweep times the 64-segment batch with the mixed launch forced on and off (CFSEC_MIX_MAX_LEN) at segment
lengths 16 KiB .. 1 MiB: the table kMixMaxLen (engine.hpp) is read from.

Each figure is the median wall time of --reps calls (default 30, at least 20) after --warmup calls of
the same shape; the two sides of a comparison alternate call by call.  Wall time around a synchronous
call: it includes the launch and the wait, which is the point.  There is no CPU path: without a GPU
the tool fails.
"""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chubaofs_amd import _lib, codemode as cm, ec  # noqa: E402


def tactic(name):
    (c,) = [c for c in cm.GetAllCodeModes() if cm.Name(c) == name]
    return cm.GetTactic(c)


class Batch:
    """B segments of n shards of S bytes in one buffer, irregularly spaced, and their bad sets."""

    def __init__(self, enc, t, S, B, distinct, pinned):
        import torch
        self.enc, self.n, self.B = enc, t.N + t.M, B
        n = self.n
        pairs = list(itertools.combinations(range(t.N), 2))
        self.bad = [list(pairs[i % len(pairs)]) if distinct else [0, 1] for i in range(B)]
        pitch = (S + 255) // 256 * 256
        pos, at = [], 0
        for i in range(B):
            at += 256 * ((i * 7) % 5 + 1)
            pos.append(at)
            at += n * pitch
        if pinned:
            self.buf = _lib.pinned_empty(at)
            self.buf[:] = 0x5A
            base, self.mem = self.buf.ctypes.data, _lib.MEM_HOST
        else:
            self.buf = torch.randint(0, 256, (at,), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            base, self.mem = self.buf.data_ptr(), _lib.MEM_DEVICE
        self.arr = (_lib.Shard * (B * n))()
        for i in range(B):
            for j in range(n):
                self.arr[i * n + j] = _lib.Shard(base + pos[i] + j * pitch, S, S)
        flat = [x for b in self.bad for x in b]
        self.flat = (ctypes.c_int * len(flat))(*flat)
        self.off = (ctypes.c_int * (B + 1))(*([0] + list(itertools.accumulate(len(b) for b in self.bad))))
        self.status = (ctypes.c_int * B)()
        self.sub = [(_lib.Shard * n).from_address(ctypes.addressof(self.arr) + i * n * ctypes.sizeof(_lib.Shard))
                    for i in range(B)]
        self.one = [(ctypes.c_int * len(b))(*b) for b in self.bad]

    def batch(self):
        L, h = self.enc._L, self.enc._h
        t0 = time.perf_counter_ns()
        rc = L.cfsec_ec_reconstruct_data_batch(h, self.arr, self.n, self.B, self.flat, self.off, self.mem, self.status)
        dt = time.perf_counter_ns() - t0
        if rc or any(self.status[i] for i in range(self.B)):
            raise RuntimeError("batch call failed: rc %d" % rc)
        return dt / 1e3 / self.B

    def loop(self):
        f, h, n, mem = self.enc._L.cfsec_ec_reconstruct_data, self.enc._h, self.n, self.mem
        t0 = time.perf_counter_ns()
        for sub, bad in zip(self.sub, self.one):
            if f(h, sub, n, bad, len(bad), mem, None):
                raise RuntimeError("single call failed")
        return (time.perf_counter_ns() - t0) / 1e3 / self.B


def alternate(sides, warmup, reps):
    """Median of `reps` timings of every side, the sides taking turns; `warmup` untimed turns first."""
    for _ in range(warmup):
        for s in sides:
            s()
    out = [[] for _ in sides]
    for _ in range(reps):
        for o, s in zip(out, sides):
            o.append(s())
    return [statistics.median(o) for o in out]


def with_limit(limit, fn):
    def call():
        os.environ["CFSEC_MIX_MAX_LEN"] = str(limit)
        try:
            return fn()
        finally:
            del os.environ["CFSEC_MIX_MAX_LEN"]
    return call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="the mixed launch against the launch groups by segment length")
    ap.add_argument("--json", help="also write the rows to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("seg_batch_probe: no GPU; nothing is measured without one")
    rows = []
    if a.sweep:
        print("64 segments, two bad data shards, HBM; us per segment, median of %d" % a.reps)
        print("%-7s %-9s %8s %10s %10s" % ("mode", "patterns", "seg", "mixed", "groups"))
        for name in ("EC12P4", "EC6P6"):
            t = tactic(name)
            enc = ec.NewEncoder(ec.Config(CodeMode=t))
            for distinct in (False, True):
                for S in (16 << 10, 64 << 10, 256 << 10, 1 << 20):
                    b = Batch(enc, t, S, 64, distinct, pinned=False)
                    mixed, groups = alternate([with_limit(1 << 30, b.batch), with_limit(0, b.batch)], a.warmup, a.reps)
                    rows.append(dict(sweep=True, mode=name, patterns="distinct" if distinct else "one", seg=S,
                                     mixed_us=mixed, groups_us=groups))
                    print("%-7s %-9s %8d %10.2f %10.2f" % (name, rows[-1]["patterns"], S, mixed, groups), flush=True)
                    del b
    else:
        print("two bad data shards; us per segment, median of %d; limit: the library's own" % a.reps)
        print("%-7s %-7s %6s %-9s %5s %10s %10s" % ("mode", "memory", "seg", "patterns", "B", "batch", "single"))
        for name in ("EC6P6", "EC12P4"):
            t = tactic(name)
            enc = ec.NewEncoder(ec.Config(CodeMode=t))
            for pinned in (False, True):
                for S in (4 << 10, 64 << 10):
                    for distinct in (False, True):
                        for B in (1, 16, 64, 256):
                            b = Batch(enc, t, S, B, distinct, pinned)
                            batch, single = alternate([b.batch, b.loop], a.warmup, a.reps)
                            rows.append(dict(mode=name, memory="pinned" if pinned else "HBM", seg=S,
                                             patterns="distinct" if distinct else "one", B=B, batch_us=batch,
                                             single_us=single))
                            print("%-7s %-7s %6d %-9s %5d %10.2f %10.2f" %
                                  (name, rows[-1]["memory"], S, rows[-1]["patterns"], B, batch, single), flush=True)
                            del b
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
