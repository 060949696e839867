"""bench.py's command line and its --dump-outputs writer, on the CPU (no kernel runs here)."""
import os
import sys

import numpy as np
import pytest
import torch

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_options(monkeypatch):
    a = parse(monkeypatch, "--full", "--no-cpu", "--dump-outputs", "some/dir")
    assert a.full is True and a.no_cpu is True and a.dump_outputs == "some/dir"


@pytest.mark.parametrize("last", [0, 1, 5])
def test_dump_outputs_writes_the_last_steps_rows(tmp_path, last):
    """The arrays are the rows step `last` wrote: parity of batch last % 3, rows 0-3 of batch
    (last + 2) % 3; block sums exact over every byte (S no multiple of the block), samples seeded."""
    k, m, nb = bench.K_DATA, bench.M_PARITY, bench.NBATCH
    nst, S = 2, 2 * bench.DUMP_BLOCK + 37
    pitch = (S + 255) // 256 * 256
    g = torch.Generator().manual_seed(last)
    batch = torch.randint(0, 256, (nb, nst, k + m, pitch), generator=g, dtype=torch.uint8)
    keep = batch.clone()
    for d in ("a", "b"):  # twice: the same files
        bench.dump_outputs(str(tmp_path / d), torch, batch, last, S, rank=0, world=1)
    assert torch.equal(batch, keep), "the dump changed the batches"
    want = {"encode_parity": keep[last % nb, :, k:, :S].numpy(),
            "reconstruct_rows": keep[(last + 2) % nb, :, 0:4, :S].numpy()}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}_{kind}.npy" for n in want for kind in ("blocksum", "sample"))
    for n, (name, rows) in enumerate(want.items()):
        sums = np.load(tmp_path / "a" / f"{name}_blocksum.npy")
        assert sums.dtype == np.float64 and sums.shape == (nst, 4, 3)
        for blk in range(3):
            ref = rows[:, :, blk * bench.DUMP_BLOCK:(blk + 1) * bench.DUMP_BLOCK].astype(np.int64).sum(axis=2)
            assert np.array_equal(sums[:, :, blk], ref)
        sample = np.load(tmp_path / "a" / f"{name}_sample.npy")
        assert sample.dtype == np.float32 and sample.shape == (min(bench.DUMP_SAMPLE, rows.size),)
        pos = np.sort(np.random.default_rng(bench.DUMP_SEED + n).integers(0, rows.size, sample.size))
        assert np.array_equal(sample, rows.reshape(-1)[pos].astype(np.float32))
        for kind in ("blocksum", "sample"):
            assert np.array_equal(np.load(tmp_path / "a" / f"{name}_{kind}.npy"), np.load(tmp_path / "b" / f"{name}_{kind}.npy"))


def test_dump_outputs_names_the_rank_when_there_are_several(tmp_path):
    S = 100
    batch = torch.zeros((bench.NBATCH, 1, bench.K_DATA + bench.M_PARITY, 256), dtype=torch.uint8)
    bench.dump_outputs(str(tmp_path), torch, batch, 0, S, rank=1, world=2)
    assert sorted(os.listdir(tmp_path)) == ["encode_parity_blocksum_rank1.npy", "encode_parity_sample_rank1.npy",
                                            "reconstruct_rows_blocksum_rank1.npy", "reconstruct_rows_sample_rank1.npy"]
