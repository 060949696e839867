#!/usr/bin/env python3
"""Times cfsec_ec_repair_batch_crc (Reconstruct + Verify + every shard's checksum, one call) against
what a caller did before it existed: cfsec_ec_reconstruct_batch_crc followed by cfsec_crc32_ieee_batch
over the survivors, and the fused route (gf_crc_sv_kernel) against CFSEC_SV_CRC=0 (the product and the
separate checksum pass).

Device memory, EC12P4 and EC6P6, 64 bids of the shard sizes of 1 MiB and 4 MiB blobs, one lost data
shard.  Each configuration cycles through enough batches that their bytes exceed the 256 MiB Infinity
Cache, so no call finds its inputs cached by the one before.  Times are host wall-clock around the
synchronous calls.  CFSEC_SV_CRC is read once per process, so the two routes run in child processes of
this script, alternated on/off/on/off..., each child timing every configuration; the parent prints per
configuration the median of each child and the spread over the children of a setting.

    python tools/repair_crc_probe.py [--rounds 3] [--reps 200] [--out FILE]

Needs a GPU; fails without one."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("EC12P4", 12, 4, 1 << 20), ("EC12P4", 12, 4, 4 << 20), ("EC6P6", 6, 6, 1 << 20), ("EC6P6", 6, 6, 4 << 20)]
NBIDS = 64
BAD = [1]
CHILD_SECONDS = 240


def shard_size(blob, n):
    return -(-blob // n)


def child(reps):
    import torch

    from chubaofs_amd import ec, reedsolomon
    from chubaofs_amd.codemode import Tactic

    assert torch.cuda.is_available(), "the probe needs a GPU"
    out = []
    for name, k, m, blob in CONFIGS:
        total, size = k + m, shard_size(blob, k)
        pitch = (size + 255) // 256 * 256
        enc = ec.NewEncoder(ec.Config(CodeMode=Tactic(k, m, 0, 1, k, 0, 0), EnableVerify=False), device=0)
        batch_bytes = NBIDS * total * pitch
        nbatch = max(2, -(-(320 << 20) // batch_bytes))  # rotated: past the 256 MiB Infinity Cache
        g = torch.Generator(device="cuda").manual_seed(k * 100 + m)
        pools, views = [], []
        for _ in range(nbatch):
            pool = torch.randint(0, 256, (NBIDS * total * pitch,), dtype=torch.uint8, device="cuda", generator=g)
            v = [[pool[(b * total + i) * pitch:(b * total + i) * pitch + size] for i in range(total)] for b in range(NBIDS)]
            pools.append(pool)
            views.append(v)
        rs = reedsolomon.New(k, m, device=0)
        for pool in pools:  # valid codewords: encode in place
            rs.encode_batch([pool.data_ptr() + j * pitch for j in range(NBIDS * total)], size, NBIDS)
        torch.cuda.synchronize()
        bads = [BAD] * NBIDS
        surv = [[pools[j].data_ptr() + (b * total + i) * pitch for b in range(NBIDS) for i in range(total) if i not in BAD]
                for j in range(nbatch)]
        # the two ways agree with each other and with zlib on one bid before anything is timed
        st, words, _ = enc.RepairBatch(views[0], bads)
        st2, words2 = enc.ReconstructBatch(views[0], bads, verify=True, crcs=True)
        sw = reedsolomon.crc32_ieee_batch(surv[0], size, device=0)
        assert st == [0] * NBIDS and st2 == [0] * NBIDS
        host = [views[0][0][i].cpu().numpy().tobytes() for i in range(total)]
        assert words[0] == [zlib.crc32(x) for x in host]
        assert [w for i, w in enumerate(words[0]) if i not in BAD] == [int(x) for x in sw[:total - len(BAD)]]
        assert words2[0][BAD[0]] == words[0][BAD[0]]

        # the timed calls go straight to the C ABI on arguments marshalled once, so the figures hold
        # the library's work and not the Python wrappers'
        import ctypes
        from chubaofs_amd import _lib
        from chubaofs_amd._shards import BatchMarshal, ptr_array
        L = _lib.lib()
        bms = [BatchMarshal(v, total, fill=True) for v in views]
        sptr = [ptr_array(p) for p in surv]
        badarr = (ctypes.c_int * NBIDS)(*(BAD * NBIDS))
        offs = (ctypes.c_int * (NBIDS + 1))(*range(NBIDS + 1))
        status = (ctypes.c_int * NBIDS)()
        cw = (ctypes.c_uint32 * (NBIDS * total))()
        sout = (ctypes.c_uint32 * len(surv[0]))()

        def new_call(j):
            rc = L.cfsec_ec_repair_batch_crc(enc._h, bms[j].arr, total, NBIDS, badarr, offs, bms[j].mem, status, cw,
                                             None, None)
            assert rc == 0

        def old_calls(j):
            rc = L.cfsec_ec_reconstruct_batch_crc(enc._h, bms[j].arr, total, NBIDS, badarr, offs, 1, bms[j].mem, status,
                                                  cw)
            assert rc == 0
            rc = L.cfsec_crc32_ieee_batch(sptr[j], size, len(surv[j]), sout, 0, None)
            assert rc == 0

        res = {"config": f"{name} {blob >> 20} MiB blobs", "shard": size, "batches": nbatch}
        for label, fn in (("new", new_call), ("old", old_calls)):
            for j in range(nbatch):
                fn(j)  # warm-up of every batch
            torch.cuda.synchronize()
            ts = []
            for r in range(reps):
                t0 = time.perf_counter()
                fn(r % nbatch)
                ts.append((time.perf_counter() - t0) * 1e6)
            res[label] = statistics.median(ts)
            res[label + "_min"] = min(ts)
        out.append(res)
        del pools, views
        torch.cuda.empty_cache()
    print("PROBE " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    runs = {"1": [], "0": []}
    for r in range(a.rounds):
        for setting in ("1", "0"):  # alternated
            env = dict(os.environ, CFSEC_SV_CRC=setting)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=env,
                               capture_output=True, text=True, timeout=CHILD_SECONDS)
            if p.returncode != 0:  # nothing more starts on the GPU after a failed child
                sys.exit(f"child CFSEC_SV_CRC={setting} ended with {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("PROBE ")][-1]
            runs[setting].append(json.loads(line[6:]))
    lines = ["# repair_crc_probe: 64 bids, one lost data shard, device memory; host wall-clock per call, us",
             "# new = cfsec_ec_repair_batch_crc; old = cfsec_ec_reconstruct_batch_crc + cfsec_crc32_ieee_batch(survivors)",
             f"# {a.rounds} child processes per setting, alternated; {a.reps} calls per figure (median); spread = max - min over the children",
             "config | shard B | new, fused (CFSEC_SV_CRC=1) | new, CFSEC_SV_CRC=0 | old, two calls"]
    for c in range(len(CONFIGS)):
        def col(setting, key):
            v = [run[c][key] for run in runs[setting]]
            return f"{statistics.median(v):8.1f} (spread {max(v) - min(v):5.1f})"
        old = [run[c]["old"] for s in ("1", "0") for run in runs[s]]
        lines.append(f"{runs['1'][0][c]['config']:20s} | {runs['1'][0][c]['shard']:7d} | {col('1', 'new')} | {col('0', 'new')} | "
                     f"{statistics.median(old):8.1f} (spread {max(old) - min(old):5.1f})")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
            f.write("# raw: " + json.dumps(runs) + "\n")


if __name__ == "__main__":
    main()
