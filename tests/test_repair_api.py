"""cfsec_ec_repair_batch_crc / cfsec_rs_repair_crc_batch without a GPU: the symbols are there with the
documented signatures, and argument errors come back as CFSEC_ERR_INVALID_ARG before any device use."""
import ctypes
import os
import re

import pytest

from chubaofs_amd import _lib, codemode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cfsec.h")
INVALID = _lib.ErrInvalidArg.status

EC_DECL = ("int cfsec_ec_repair_batch_crc(cfsec_ec* h, cfsec_shard* shards, int n, int nbids, const int* bad_idx, "
           "const int* bad_off, int mem, int* status, uint32_t* crcs, const uint32_t* expect, int* mismatch);")
RS_DECL = ("int cfsec_rs_repair_crc_batch(cfsec_rs* h, uint8_t* const* ptrs, size_t shard_size, int nstripes, "
           "const int* erased, int nerased, uint32_t* flags, uint32_t* crcs, void* stream);")


def header_declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {" ".join(d.split()) for d in re.findall(r"\bint\s+cfsec_[a-z0-9_]+\s*\([^;]*;", src)}


def test_symbols_and_signatures():
    L = _lib.lib()
    decl = header_declarations()
    assert EC_DECL in decl and RS_DECL in decl
    assert hasattr(L, "cfsec_ec_repair_batch_crc") and hasattr(L, "cfsec_rs_repair_crc_batch")
    V, I, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert _lib.SIGNATURES["cfsec_ec_repair_batch_crc"] == ([V, _lib.P_SHARD, I, I, V, V, I, V, V, V, V], I)
    assert _lib.SIGNATURES["cfsec_rs_repair_crc_batch"] == ([V, V, S, I, V, I, V, V, V], I)
    assert L.cfsec_version().startswith(b"cfsec 0.5.")


def test_python_mirrors_exist():
    from chubaofs_amd import ec, reedsolomon
    assert callable(ec.Encoder.RepairBatch) and callable(reedsolomon.ReedSolomon.repair_crc_batch)


def test_ec_argument_errors():
    from chubaofs_amd import ec
    L = _lib.lib()
    enc = ec.NewEncoder(ec.Config(CodeMode=codemode.GetTactic(codemode.EC6P3), EnableVerify=False))
    n, nb = 9, 2
    shards = (_lib.Shard * (n * nb))()
    status, mism = (ctypes.c_int * nb)(), (ctypes.c_int * nb)()
    crcs, expect = (ctypes.c_uint32 * (n * nb))(), (ctypes.c_uint32 * (n * nb))()
    bad, off = (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 3)(0, 1, 2)
    call = L.cfsec_ec_repair_batch_crc
    h = enc._h
    assert call(None, shards, n, nb, bad, off, _lib.MEM_HOST, status, crcs, None, None) == INVALID
    assert call(h, None, n, nb, bad, off, _lib.MEM_HOST, status, crcs, None, None) == INVALID
    assert call(h, shards, 0, nb, bad, off, _lib.MEM_HOST, status, crcs, None, None) == INVALID
    assert call(h, shards, -1, nb, bad, off, _lib.MEM_HOST, status, crcs, None, None) == INVALID
    assert call(h, shards, n, -1, bad, off, _lib.MEM_HOST, status, crcs, None, None) == INVALID
    assert call(h, shards, n, nb, bad, None, _lib.MEM_HOST, status, crcs, None, None) == INVALID
    assert call(h, shards, n, nb, bad, off, _lib.MEM_HOST, None, crcs, None, None) == INVALID
    assert call(h, shards, n, nb, bad, off, _lib.MEM_HOST, status, None, None, None) == INVALID
    assert call(h, shards, n, nb, None, off, _lib.MEM_HOST, status, crcs, None, None) == INVALID  # bad sets, no indices
    assert call(h, shards, n, nb, bad, off, _lib.MEM_HOST, status, crcs, expect, None) == INVALID  # expect, no mismatch
    assert call(h, shards, n, nb, bad, (ctypes.c_int * 3)(1, 1, 2), _lib.MEM_HOST, status, crcs, None, None) == INVALID
    assert call(h, shards, n, nb, bad, (ctypes.c_int * 3)(0, 2, 1), _lib.MEM_HOST, status, crcs, None, None) == INVALID


def test_rs_argument_errors():
    from chubaofs_amd import reedsolomon
    L = _lib.lib()
    e = reedsolomon.New(6, 3)
    ptrs = (ctypes.c_void_p * 9)()
    er = (ctypes.c_int * 1)(0)
    word = ctypes.c_uint32()
    f = c = ctypes.addressof(word)
    call = L.cfsec_rs_repair_crc_batch
    h = e._h
    assert call(None, ptrs, 16, 1, er, 1, f, c, None) == INVALID
    assert call(h, None, 16, 1, er, 1, f, c, None) == INVALID
    assert call(h, ptrs, 16, -1, er, 1, f, c, None) == INVALID
    assert call(h, ptrs, 16, 1, er, -1, f, c, None) == INVALID
    assert call(h, ptrs, 16, 1, None, 1, f, c, None) == INVALID
    assert call(h, ptrs, 16, 1, er, 1, None, c, None) == INVALID
    assert call(h, ptrs, 16, 1, er, 1, f, None, None) == INVALID
    assert call(h, ptrs, 16, 1, (ctypes.c_int * 1)(9), 1, f, c, None) == INVALID   # index past the stripe
    assert call(h, ptrs, 16, 1, (ctypes.c_int * 1)(-1), 1, f, c, None) == INVALID


def test_repair_batch_checks_its_lists():
    from chubaofs_amd import ec
    enc = ec.NewEncoder(ec.Config(CodeMode=codemode.GetTactic(codemode.EC6P3), EnableVerify=False))
    with pytest.raises(ValueError):
        enc.RepairBatch([[None] * 9], [[0], [1]])
    with pytest.raises(ValueError):
        enc.RepairBatch([[None] * 9], [[0]], expect=[[0] * 9, [0] * 9])
