#!/usr/bin/env python3
"""repair_bids_probe.py -- what a repair costs per bid when the bids of a tasklet differ in size.

blobnode repairs a tasklet bid by bid: Reconstruct, then Verify, and crc32.ChecksumIEEE of every shard
around them (blobnode/work_shard_recover.go:708-771, 654-685, 335-342).  The bids are whatever blobs lived
on the broken disk: a blob smaller than the blob size is one stripe of its own shard size, so a tasklet is
mostly small stripes of different lengths.  This tool times, in one process on one GPU,

  * one cfsec_ec_repair_bids_crc call over B bids (the mixed-plan launch that stores, compares and
    checksums), beside
  * one cfsec_ec_repair_batch_crc call over the same bids (a product launch per bad set and a checksum
    launch per distinct length), beside
  * the one-thread CPU port (oracle/cpu_simd.c) doing per bid the decode rows over the survivors, the
    re-encode and compare of Verify, and zlib.crc32 of every shard,

each divided by B, for EC12P4, EC6P6 and EC6P10L2, B in {16, 64, 256}, shard sizes log-uniform in
2 KiB .. 64 KiB and all distinct, on HBM and on page-locked host memory, with one bad index for all bids
(a disk repair) and with a bad set per bid drawn from 16 distinct ones.  The bids sit at irregular distances
from each other, as separately downloaded shards do.  The shards hold valid codewords, so every Verify
holds.  The launch counts of the two GPU calls are read from their traces in one extra, untimed call each.

--modes EC16P20L2,EC16P20 times the 16 + 20 code, whose bids take the mixed-plan repair launch that drives
the 16x16-dyadic product from an item table (gf_mix_sv16.hip): EC16P20L2 with BASELINE configs[3-4]'s bad
set [0, 1, 16, 17] as the one bad set, EC16P20 (its RS sibling, 36 shards in one AZ; no code mode names it)
with one bad data shard.  Run in a process of its own with CFSEC_NO_DY16_REPAIR=1 (read once per process),
no plan carries a dy16 product and the bids_crc column is the generic launch (gf_mix_sv.hip) on the same
bids: the evidence for or against the dyadic body over the plain one.

--sweep times a tasklet of 64 bids of ONE shard size and one bad index with the mixed launch forced on and
off (CFSEC_MIX_MAX_LEN) at 16 KiB .. 1 MiB, on cfsec_ec_repair_bids_crc: the table the route's length limit
is read from (the largest length at which the mixed launch is no slower on the one-size tasklet).

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

from chubaofs_amd import _lib, ec, reedsolomon  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle.ec_oracle import layout_by_az  # noqa: E402
from chubaofs_amd.codemode import Tactic  # noqa: E402
from put_blobs_probe import alternate, blob_sizes, with_limit  # noqa: E402
from put_blobs_probe import tactic as mode_tactic  # noqa: E402


def tactic(name):
    return Tactic(16, 20, 0, 1, 16, 0, 0) if name == "EC16P20" else mode_tactic(name)


def one_bad(t):
    """The bad set of a disk repair: one data shard; for EC16P20L2 the set the project benchmarks (C5)."""
    return [0, 1, 16, 17] if (t.N, t.M, t.L) == (16, 20, 2) else [1]


def bad_sets(t, B, distinct, rng):
    """One bad data shard for every bid, or per bid one of 16 distinct sets of 1 .. min(M, 3) global shards."""
    if not distinct:
        return [one_bad(t)] * B
    sets = set()
    while len(sets) < 16:
        nb = int(rng.integers(1, min(t.M, 3) + 1))
        sets.add(tuple(sorted(int(x) for x in rng.choice(t.N + t.M, nb, replace=False))))
    sets = sorted(sets)
    return [list(sets[int(rng.integers(0, 16))]) for _ in range(B)]


class Tasklet:
    """B bids of n shards in one buffer, irregularly spaced, valid codewords; the same bytes on the host
    for the CPU side."""

    def __init__(self, enc, t, sizes, bads, pinned):
        import torch
        self.enc, self.t, self.n, self.B, self.sizes, self.bads = enc, t, t.N + t.M + t.L, len(sizes), sizes, bads
        n, N, M = self.n, t.N, t.M
        pos, at = [], 0
        for i, S in enumerate(sizes):
            at += 256 * ((i * 7) % 5 + 1)
            pos.append(at)
            at += n * ((S + 255) // 256 * 256)
        host = np.random.default_rng(len(sizes)).integers(0, 256, at, dtype=np.uint8)
        # the CPU side's rows: global parity, per AZ the local engine's, per bad set the decode rows
        self.grows = reedsolomon.New(N, M).matrix()[N:]
        self.az = layout_by_az(N, M, t.L, t.AZCount) if t.L else []
        self.ln = (N + M) // t.AZCount
        lm = t.L // t.AZCount if t.L else 0
        self.lrows = reedsolomon.New(self.ln, lm).matrix()[self.ln:] if t.L else None
        self.dec = {}
        for bad in bads:
            if tuple(bad) not in self.dec:
                ins, rows = enc.repair_rows(bad, bad)
                self.dec[tuple(bad)] = (ins, np.frombuffer(b"".join(rows), np.uint8).reshape(len(bad), N).copy())
        self.host = []
        for i, S in enumerate(sizes):
            pitch = (S + 255) // 256 * 256
            sh = [host[pos[i] + j * pitch:pos[i] + j * pitch + S] for j in range(n)]  # views: encoded in place
            O.simd_code(self.grows, sh[:N], sh[N:N + M], 1)
            for idx in self.az:
                loc = [sh[g] for g in idx]
                O.simd_code(self.lrows, loc[:self.ln], loc[self.ln:], 1)
            self.host.append([s.copy() for s in sh])
        self.clean = [[zlib.crc32(s) for s in sh] for sh in self.host]
        if pinned:
            self.buf = _lib.pinned_empty(at)
            self.buf[:] = host
            base, self.mem = self.buf.ctypes.data, _lib.MEM_HOST
        else:
            self.buf = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            base, self.mem = self.buf.data_ptr(), _lib.MEM_DEVICE
        self.arr = (_lib.Shard * (self.B * n))()
        for i, S in enumerate(sizes):
            pitch = (S + 255) // 256 * 256
            for j in range(n):
                self.arr[i * n + j] = _lib.Shard(base + pos[i] + j * pitch, S, S)
        flat = [x for b in bads for x in b]
        offs = [0]
        for b in bads:
            offs.append(offs[-1] + len(b))
        self.bad = (ctypes.c_int * len(flat))(*flat)
        self.off = (ctypes.c_int * len(offs))(*offs)
        self.status = (ctypes.c_int * self.B)()
        self.words = (ctypes.c_uint32 * (self.B * n))()
        self.scratch = [np.empty(max(sizes), np.uint8) for _ in range(max(M, lm, 1))]

    def _call(self, fn):
        for i in range(self.B * self.n):  # every call starts from whole headers (untimed)
            self.arr[i].len = self.arr[i].cap
        t0 = time.perf_counter_ns()
        rc = fn(self.enc._h, self.arr, self.n, self.B, self.bad, self.off, self.mem, self.status, self.words, None, None)
        dt = time.perf_counter_ns() - t0
        if rc or any(self.status[i] for i in range(self.B)):
            raise RuntimeError("repair call failed: rc %d, statuses %s" % (rc, sorted(set(self.status))))
        return dt / 1e3 / self.B

    def bids(self):
        return self._call(self.enc._L.cfsec_ec_repair_bids_crc)

    def batch(self):
        return self._call(self.enc._L.cfsec_ec_repair_batch_crc)

    def cpu(self):
        N, M = self.t.N, self.t.M
        t0 = time.perf_counter_ns()
        out = []
        for sh, bad, S in zip(self.host, self.bads, self.sizes):
            ins, rows = self.dec[tuple(bad)]
            O.simd_code(rows, [sh[g] for g in ins], [sh[g] for g in bad], 1)  # Reconstruct
            par = [s[:S] for s in self.scratch[:M]]  # Verify: re-encode and compare
            O.simd_code(self.grows, sh[:N], par, 1)
            ok = all(np.array_equal(p, s) for p, s in zip(par, sh[N:N + M]))
            for idx in self.az:
                loc = [sh[g] for g in idx]
                lp = [s[:S] for s in self.scratch[:len(loc) - self.ln]]
                O.simd_code(self.lrows, loc[:self.ln], lp, 1)
                ok = ok and all(np.array_equal(p, s) for p, s in zip(lp, loc[self.ln:]))
            if not ok:
                raise RuntimeError("the CPU port's Verify is false")
            out.append([zlib.crc32(s) for s in sh])
        dt = time.perf_counter_ns() - t0
        self.cpu_words = out
        return dt / 1e3 / self.B

    def check(self):
        """The three sides agree with the checksums of the clean codewords."""
        self.cpu()
        if self.cpu_words != self.clean:
            raise RuntimeError("the CPU port's repair differs from the codewords")
        for fn in (self.bids, self.batch):
            fn()
            got = [[int(self.words[i * self.n + j]) for j in range(self.n)] for i in range(self.B)]
            if got != self.clean:
                raise RuntimeError("checksums differ from the codewords'")

    def launches(self, fn):
        """The kernel launches one call of fn traces: (mixsv, product, fused product + crc, crc32)."""
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
        return (count("cfsec: mixsv ", "cfsec: mixsv16 "), count("cfsec: matvec ", "cfsec: dy16"),
                count("cfsec: crc route", "cfsec: crc sv", "cfsec: bs launch"), count("cfsec: crc32 "))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="the mixed launch against the launch groups by shard size")
    ap.add_argument("--modes", default="EC12P4,EC6P6,EC6P10L2")
    ap.add_argument("--batches", default="16,64,256")
    ap.add_argument("--json", help="also write the rows to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("repair_bids_probe: no GPU; nothing is measured without one")
    rows = []
    modes = a.modes.split(",")
    if a.sweep:
        print("64 bids of one shard size, one bad index, HBM; us per bid, median of %d" % a.reps)
        print("%-9s %8s %10s %10s" % ("mode", "shard", "mixed", "groups"))
        for name in modes:
            t = tactic(name)
            enc = ec.NewEncoder(ec.Config(CodeMode=t))
            for S in (16 << 10, 64 << 10, 256 << 10, 1 << 20):
                b = Tasklet(enc, t, [S] * 64, [one_bad(t)] * 64, pinned=False)
                mixed, groups = alternate([with_limit(1 << 30, b.bids), with_limit(0, b.bids)], a.warmup, a.reps)
                rows.append(dict(sweep=True, mode=name, shard=S, mixed_us=mixed, groups_us=groups))
                print("%-9s %8d %10.2f %10.2f" % (name, S, mixed, groups), flush=True)
                del b
    else:
        print("shard sizes log-uniform in 2 KiB .. 64 KiB, all distinct; us per bid, median of %d; launches per call as "
              "mixsv+product+fused+crc32" % a.reps)
        print("%-9s %-7s %-8s %5s %10s %10s %10s  %-12s %-12s" %
              ("mode", "memory", "bad sets", "B", "bids_crc", "batch_crc", "cpu_1t", "launches new", "launches old"))
        for name in modes:
            t = tactic(name)
            enc = ec.NewEncoder(ec.Config(CodeMode=t))
            for pinned in (False, True):
                for distinct in (False, True):
                    for B in [int(x) for x in a.batches.split(",")]:
                        rng = np.random.default_rng(B)
                        b = Tasklet(enc, t, blob_sizes(B, rng), bad_sets(t, B, distinct, rng), pinned)
                        b.check()
                        new, old, cpu = alternate([b.bids, b.batch, b.cpu], a.warmup, a.reps)
                        ln, lo = b.launches(b.bids), b.launches(b.batch)
                        rows.append(dict(mode=name, memory="pinned" if pinned else "HBM",
                                         bad_sets="distinct" if distinct else "one", B=B, bids_crc_us=new,
                                         batch_crc_us=old, cpu_1t_us=cpu, launches_new=ln, launches_old=lo))
                        print("%-9s %-7s %-8s %5d %10.2f %10.2f %10.2f  %-12s %-12s" %
                              (name, rows[-1]["memory"], rows[-1]["bad_sets"], B, new, old, cpu,
                               "+".join(map(str, ln)), "+".join(map(str, lo))), flush=True)
                        del b
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
