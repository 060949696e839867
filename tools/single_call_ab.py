"""A/B of the single-stripe calls' host time between two builds of libcfsec.so (CFSEC_LIB_PATH picks
the library): the parent's engine.cpp / capi.cpp against the tree's, device code identical.

  python tools/single_call_ab.py probe > run.probe.json
      cfsec_rs_encode_crc (Encode + the 16 checksums, one synchronous call) of EC12P4 stripes of 64 KiB
      and 1 MiB shards in pageable, page-locked and device memory: median us per call of 200.
  python tools/single_call_ab.py table --a A1.json A2.json ... --b B1.json B2.json ...
      Every file holds JSON lines (bench.py --full's result line, a probe line).  For each figure of
      segment_reconstruct_data, host_path, the probe, sync_floor_us and the kernel figures (headline,
      C1, C4, C5): A's runs, B's runs, and whether B's median is inside A's own run-to-run spread --
      not above A's largest run for times, not below A's smallest for rates.
"""
import argparse
import json
import re
import statistics
import sys
import time

KEEP = re.compile(r"^(value$|ms_per_step$|roofline\.avg_launch_ms$|.*segment_reconstruct_data\.modes\..*\.(pageable|pinned|device)(_cabi)?_us$|"
                  r".*host_path\.(pinned|pageable)\.data_GBps$|encode_crc_single_call\..*_us$|.*sync_floor_us$|"
                  r".*(C1_EC6P6_1MiB_encode|C4_EC6P10L2_lrc_encode_local_repair|C5_EC16P20L2_repair_tasklet)"
                  r"\.[a-z_0-9]*kernel_ms[a-z_0-9]*$)")


def probe():
    import numpy as np
    import torch

    from chubaofs_amd import _lib, reedsolomon
    k, m, out = 12, 4, {}
    enc = reedsolomon.New(k, m, device=0)
    for S in (65536, 1 << 20):
        data = np.random.default_rng(S).integers(0, 256, (k + m, S), dtype=np.uint8)
        pin = _lib.pinned_empty((k + m) * S)
        pin[:] = data.reshape(-1)
        dev = torch.from_numpy(data).to("cuda:0")
        kinds = {"pageable": [data[i] for i in range(k + m)], "pinned": [pin[i * S:(i + 1) * S] for i in range(k + m)],
                 "device": [dev[i] for i in range(k + m)]}
        for kind, sh in kinds.items():
            want = enc.EncodeCRC(sh)
            ts = []
            for _ in range(200):
                t0 = time.perf_counter()
                got = enc.EncodeCRC(sh)
                ts.append(time.perf_counter() - t0)
            assert got == want
            out["%s_%d_us" % (kind, S)] = round(statistics.median(ts) * 1e6, 1)
    print(json.dumps({"encode_crc_single_call": out}))


def leaves(node, path, out):
    if isinstance(node, dict):
        for key, v in node.items():
            leaves(v, path + [str(key)], out)
    elif isinstance(node, (int, float)) and not isinstance(node, bool):
        name = ".".join(path)
        if KEEP.match(name):
            out[name] = float(node)


def load(files):
    runs = []
    for f in files:
        figures = {}
        for line in open(f):
            if line.startswith("{"):
                leaves(json.loads(line), [], figures)
        runs.append(figures)
    return runs


def table(a_files, b_files):
    a, b = load(a_files), load(b_files)
    names = sorted(set(a[0]) & set(b[0]))
    worse = 0
    print("# A: %d runs, B: %d runs" % (len(a), len(b)))
    print("%-86s %-42s %-42s %s" % ("figure", "A runs", "B runs", "B median vs A's spread"))
    for n in names:
        av, bv = [r[n] for r in a if n in r], [r[n] for r in b if n in r]
        rate = n.endswith("GBps") or n == "value"
        bm = statistics.median(bv)
        inside = bm >= min(av) if rate else bm <= max(av)
        worse += not inside
        print("%-86s %-42s %-42s %s" % (n, " ".join("%g" % x for x in av), " ".join("%g" % x for x in bv),
                                        "inside" if inside else "OUTSIDE (%g vs %g)" % (bm, min(av) if rate else max(av))))
    print("# %d figures, %d outside" % (len(names), worse))
    return worse


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=["probe", "table"])
    p.add_argument("--a", nargs="*", default=[])
    p.add_argument("--b", nargs="*", default=[])
    args = p.parse_args()
    if args.what == "probe":
        sys.path.insert(0, ".")
        probe()
    else:
        table(args.a, args.b)
