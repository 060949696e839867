"""The bit-sliced fused launches the device runs are the ones the host plan names (plan_bs_crc,
kernels.hpp; tests/test_crc_plan.py pins the plan itself on the CPU): with CFSEC_TRACE_CRC every
"cfsec: bs launch" line must equal tests/crc_routes.py's bs_plan for that line's own stripes, tps and
resident workgroup count, the checksum words must equal zlib's CRC-32 of the rows, and the parity the
plain encode's.

 (a) EC3P3, 1536 bids in one buffer (an affine job, one launch), S = 8193: five tiles, the last of
     one byte, k odd (no paired basis).  3072 to 4604 resident waves over 1536 stripes are W = 2 per
     stripe, so on a device holding 768..1151 of these workgroups the fifth tile of every stripe goes
     to a tail wave; the test asserts the plan, and tail > 0 only where the plan says so.
 (b) EC12P4, 13 stripes in separate allocations, S = 6139: pointer-table launches of 6 + 6 + 1
     stripes, every row at an odd address, three tiles with a partial last one.
"""
import re
import zlib

import numpy as np
import pytest

import crc_routes as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LAUNCH = re.compile(r"cfsec: bs launch stripes=(\d+) tps=(\d+) W=(\d+) groups=(\d+) resident=(\d+) tail=(\d+)")


def check_launches(err, k, m, S, want_stripes):
    """Every traced launch against the restated plan of a launch of that many stripes."""
    lines = [tuple(map(int, g)) for g in LAUNCH.findall(err)]
    assert [l[0] for l in lines] == want_stripes, err[-2000:]
    for stripes, tps, W, groups, resident, tail in lines:
        _, _, _, (st,) = R.bs_plan(k, m, S, stripes, True, resident)  # (one launch: the layout plays no part)
        assert (tps, W, groups, tail) == (st["tps"], st["W"], st["groups"], st["tail"]), (stripes, resident)
        assert tps == -(-S // 2048) and st["bend"] + tail == tps
    return lines


def test_ec3p3_affine_batch_matches_the_plan(monkeypatch, capfd):
    from chubaofs_amd import codemode as cm, ec
    t = cm.GetTactic(cm.EC3P3)
    nb, S, total = 1536, 8193, t.N + t.M
    enc = ec.NewEncoder(ec.Config(CodeMode=t, EnableVerify=False), device=0)
    g = torch.Generator(device="cuda").manual_seed(8193)
    buf = torch.zeros((nb, total, S), dtype=torch.uint8, device="cuda")
    buf[:, :t.N] = torch.randint(0, 256, (nb, t.N, S), dtype=torch.uint8, device="cuda", generator=g)
    plain = buf.clone()
    assert enc.EncodeBatch([[plain[b, i] for i in range(total)] for b in range(nb)]) == [0] * nb
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    capfd.readouterr()
    st, crcs = enc.EncodeBatch([[buf[b, i] for i in range(total)] for b in range(nb)], crcs=True)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert st == [0] * nb and "bs crc" in err
    ((_, tps, W, _, resident, tail),) = check_launches(err, t.N, t.M, S, [nb])
    assert tps == 5
    if 768 <= resident <= 1151:
        assert (W, tail) == (2, 1)
    assert torch.equal(buf, plain)
    got = buf.cpu().numpy()
    for b in range(nb):
        for i in range(total):
            assert crcs[b][i] == zlib.crc32(got[b, i].tobytes()) & 0xFFFFFFFF, (b, i)


def test_ec12p4_pointer_table_launches_match_the_plan(monkeypatch, capfd):
    from chubaofs_amd import reedsolomon
    k, m, S, nst = 12, 4, 6139, 13
    g = torch.Generator(device="cuda").manual_seed(6139)
    raw = [[torch.zeros(S + 64, dtype=torch.uint8, device="cuda") for _ in range(k + m)] for _ in range(nst)]
    # odd addresses, and no common stride between the stripes whatever the allocator does
    sh = [[raw[s][i][o:o + S] for i in range(k + m) for o in [2 * ((i + s * s) % 16) + 1]] for s in range(nst)]
    for st in sh:
        for t in st[:k]:
            t.copy_(torch.randint(0, 256, (S,), dtype=torch.uint8, device="cuda", generator=g))
    ptrs = [t.data_ptr() for st in sh for t in st]
    assert all(p & 1 for p in ptrs)
    enc = reedsolomon.New(k, m)
    monkeypatch.setenv("CFSEC_TRACE_CRC", "1")
    crcs = torch.zeros(nst * (k + m), dtype=torch.int32, device="cuda")
    capfd.readouterr()
    enc.encode_crc_batch(ptrs, S, nst, crcs.data_ptr())
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert "bs crc" in err
    check_launches(err, k, m, S, [6, 6, 1])
    fused = [[t.cpu().numpy() for t in st] for st in sh]
    for st in sh:
        for t in st[k:]:
            t.zero_()
    enc.encode_batch(ptrs, S, nst)
    torch.cuda.synchronize()
    words = crcs.cpu().numpy().view(np.uint32).reshape(nst, k + m)
    for s_ in range(nst):
        for i in range(k + m):
            assert np.array_equal(fused[s_][i], sh[s_][i].cpu().numpy()), (s_, i)
            assert int(words[s_][i]) == zlib.crc32(fused[s_][i].tobytes()) & 0xFFFFFFFF, (s_, i)
