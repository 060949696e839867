#!/usr/bin/env python3
"""put_blobs_probe.py -- what a put costs per blob when the blobs of a batch differ in size.

access ends every put with Encode and crc32.ChecksumIEEE of every shard (access/stream_put.go:125-143,
249-253); a blob smaller than the blob size is one stripe of its own shard size, so a batch gathered
across requests is mostly small stripes of different lengths.  This tool times, in one process on one GPU,

  * one cfsec_ec_encode_blobs_crc call over B blobs (the mixed-plan launch with checksums), beside
  * one cfsec_ec_encode_batch_crc call over the same blobs (a product launch per 18 EC12P4 stripes and a
    checksum launch per distinct length), beside
  * the one-thread CPU port (oracle/cpu_simd.c) doing Encode + zlib.crc32 blob by blob,

each divided by B, for EC12P4, EC6P6 and EC6P10L2, B in {2, 16, 64, 256}, shard sizes log-uniform in
2 KiB .. 64 KiB and all distinct, on HBM and on page-locked host memory.  The blobs of a batch sit at
irregular distances from each other, as separately received blobs do.  The launch counts of the two GPU
calls are read from their traces in one extra, untimed call each.

--sweep times a batch of 64 blobs of ONE shard size with the mixed launch forced on and off
(CFSEC_MIX_MAX_LEN) at 16 KiB .. 1 MiB, on cfsec_ec_encode_blobs_crc: the table the route's length limit
is read from (the largest length at which the mixed launch is no slower on the one-size batch).

Each figure is the median wall time of --reps calls (default 30, at least 20) after --warmup calls of
the same shape; the sides of a comparison alternate call by call.  Wall time around a synchronous call:
it includes the launch and the wait, which is the point.  Without a GPU the tool fails.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chubaofs_amd import _lib, codemode as cm, ec, reedsolomon  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle.ec_oracle import layout_by_az  # noqa: E402


def tactic(name):
    (c,) = [c for c in cm.GetAllCodeModes() if cm.Name(c) == name]
    return cm.GetTactic(c)


def blob_sizes(B, rng, lo=2 << 10, hi=64 << 10):
    """B distinct shard sizes, log-uniform in [lo, hi]."""
    sizes = set()
    while len(sizes) < B:
        sizes.add(int(round(float(np.exp(rng.uniform(np.log(lo), np.log(hi)))))))
    return sorted(sizes, key=lambda s: (s * 2654435761) % 4093)  # not in order of size


class Batch:
    """B blobs of n shards in one buffer, irregularly spaced; the same bytes on the host for the CPU side."""

    def __init__(self, enc, t, sizes, pinned):
        import torch
        self.enc, self.t, self.n, self.B, self.sizes = enc, t, t.N + t.M + t.L, len(sizes), sizes
        n = self.n
        pos, at = [], 0
        for i, S in enumerate(sizes):
            at += 256 * ((i * 7) % 5 + 1)
            pos.append(at)
            at += n * ((S + 255) // 256 * 256)
        host = np.random.default_rng(len(sizes)).integers(0, 256, at, dtype=np.uint8)
        if pinned:
            self.buf = _lib.pinned_empty(at)
            self.buf[:] = host
            base, self.mem = self.buf.ctypes.data, _lib.MEM_HOST
        else:
            self.buf = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            base, self.mem = self.buf.data_ptr(), _lib.MEM_DEVICE
        self.arr = (_lib.Shard * (self.B * n))()
        self.host = []
        for i, S in enumerate(sizes):
            pitch = (S + 255) // 256 * 256
            for j in range(n):
                self.arr[i * n + j] = _lib.Shard(base + pos[i] + j * pitch, S, S)
            self.host.append([host[pos[i] + j * pitch:pos[i] + j * pitch + S].copy() for j in range(n)])
        self.status = (ctypes.c_int * self.B)()
        self.words = (ctypes.c_uint32 * (self.B * n))()
        # the CPU side: the global parity rows, and per AZ the local engine's rows (lrcencoder.go:35-82)
        self.grows = reedsolomon.New(t.N, t.M).matrix()[t.N:]
        self.az = layout_by_az(t.N, t.M, t.L, t.AZCount) if t.L else []
        ln, lm = (t.N + t.M) // t.AZCount, (t.L // t.AZCount if t.L else 0)
        self.lrows = reedsolomon.New(ln, lm).matrix()[ln:] if t.L else None
        self.ln = ln

    def _call(self, fn):
        t0 = time.perf_counter_ns()
        rc = fn(self.enc._h, self.arr, self.n, self.B, self.mem, self.status, self.words)
        dt = time.perf_counter_ns() - t0
        if rc or any(self.status[i] for i in range(self.B)):
            raise RuntimeError("batch call failed: rc %d" % rc)
        return dt / 1e3 / self.B

    def blobs(self):
        return self._call(self.enc._L.cfsec_ec_encode_blobs_crc)

    def batch(self):
        return self._call(self.enc._L.cfsec_ec_encode_batch_crc)

    def cpu(self):
        t, N, M = self.t, self.t.N, self.t.M
        t0 = time.perf_counter_ns()
        out = []
        for sh in self.host:
            O.simd_code(self.grows, sh[:N], sh[N:N + M], 1)
            for idx in self.az:
                loc = [sh[g] for g in idx]
                O.simd_code(self.lrows, loc[:self.ln], loc[self.ln:], 1)
            out.append([zlib.crc32(s) for s in sh])
        dt = time.perf_counter_ns() - t0
        self.cpu_words = out
        return dt / 1e3 / self.B

    def check(self):
        """The three sides agree (the GPU words against the CPU port's parity + zlib)."""
        self.cpu()
        for fn in (self.blobs, self.batch):
            fn()
            got = [[int(self.words[i * self.n + j]) for j in range(self.n)] for i in range(self.B)]
            if got != self.cpu_words:
                raise RuntimeError("checksums differ from the CPU port's")

    def launches(self, fn):
        """The kernel launches one call of fn traces: (mixcrc, product, fused product + crc, crc32)."""
        names = ("CFSEC_TRACE_MATVEC", "CFSEC_TRACE_CRC32", "CFSEC_TRACE_CRC")
        sys.stderr.flush()
        with tempfile.TemporaryFile() as f:
            keep = os.dup(2)
            os.dup2(f.fileno(), 2)
            for v in names:
                os.environ[v] = "1"
            try:
                fn()
            finally:
                for v in names:
                    del os.environ[v]
                os.dup2(keep, 2)
                os.close(keep)
            f.seek(0)
            ln = f.read().decode().splitlines()
        count = lambda *p: sum(1 for x in ln if any(x.startswith(q) for q in p))  # noqa: E731
        return (count("cfsec: mixcrc "), count("cfsec: matvec ", "cfsec: dy16"),
                count("cfsec: crc route", "cfsec: crc sv", "cfsec: bs launch"), count("cfsec: crc32 "))


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
    ap.add_argument("--sweep", action="store_true", help="the mixed launch against the launch groups by shard size")
    ap.add_argument("--modes", default="EC12P4,EC6P6,EC6P10L2")
    ap.add_argument("--batches", default="2,16,64,256")
    ap.add_argument("--json", help="also write the rows to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("put_blobs_probe: no GPU; nothing is measured without one")
    rows = []
    modes = a.modes.split(",")
    if a.sweep:
        print("64 blobs of one shard size, HBM; us per blob, median of %d" % a.reps)
        print("%-9s %8s %10s %10s" % ("mode", "shard", "mixed", "groups"))
        for name in modes:
            t = tactic(name)
            enc = ec.NewEncoder(ec.Config(CodeMode=t))
            for S in (16 << 10, 64 << 10, 256 << 10, 1 << 20):
                b = Batch(enc, t, [S] * 64, pinned=False)
                mixed, groups = alternate([with_limit(1 << 30, b.blobs), with_limit(0, b.blobs)], a.warmup, a.reps)
                rows.append(dict(sweep=True, mode=name, shard=S, mixed_us=mixed, groups_us=groups))
                print("%-9s %8d %10.2f %10.2f" % (name, S, mixed, groups), flush=True)
                del b
    else:
        print("shard sizes log-uniform in 2 KiB .. 64 KiB, all distinct; us per blob, median of %d; launches per call as "
              "mixcrc+product+fused+crc32" % a.reps)
        print("%-9s %-7s %5s %10s %10s %10s  %-12s %-12s" %
              ("mode", "memory", "B", "blobs_crc", "batch_crc", "cpu_1t", "launches new", "launches old"))
        for name in modes:
            t = tactic(name)
            enc = ec.NewEncoder(ec.Config(CodeMode=t))
            for pinned in (False, True):
                for B in [int(x) for x in a.batches.split(",")]:
                    b = Batch(enc, t, blob_sizes(B, np.random.default_rng(B)), pinned)
                    b.check()
                    new, old, cpu = alternate([b.blobs, b.batch, b.cpu], a.warmup, a.reps)
                    ln, lo = b.launches(b.blobs), b.launches(b.batch)
                    rows.append(dict(mode=name, memory="pinned" if pinned else "HBM", B=B, blobs_crc_us=new,
                                     batch_crc_us=old, cpu_1t_us=cpu, launches_new=ln, launches_old=lo))
                    print("%-9s %-7s %5d %10.2f %10.2f %10.2f  %-12s %-12s" %
                          (name, rows[-1]["memory"], B, new, old, cpu, "+".join(map(str, ln)), "+".join(map(str, lo))),
                          flush=True)
                    del b
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
