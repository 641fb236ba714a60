"""tests/minibatch_ref.py against torch in float64 (mean, unbiased std, the normalised values of the
(adv - mean) / (std + eps) form, to 1e-12 of the magnitudes), and gym_macm.ppo.minibatches on CPU tensors:
a partition of range(n) into contiguous aligned blocks, lengths within one block of each other, block = 1,
deterministic under a seeded generator, with n not a multiple of the block and n below n_minibatches * block."""
import numpy as np
import pytest
import torch

import minibatch_ref as M

from gym_macm import ppo


@pytest.mark.parametrize("rows", [2, 65, 4097])
def test_reference_against_torch(rows):
    rng = np.random.default_rng([77, rows])
    src = (0.3 + rng.standard_normal(5000)).astype(np.float32)
    index = rng.integers(0, 5000, rows).astype(np.int32)
    ref = M.moments(src, index, 1e-8)
    t = torch.from_numpy(src).to(torch.float64)[torch.from_numpy(index).long()]
    assert ref["n"] == rows
    assert abs(ref["mean"] - float(t.mean())) <= 1e-12 * float(t.abs().mean())
    assert abs(ref["std"] - float(t.std())) <= 1e-12 * float(t.std())
    assert abs(ref["rstd"] - 1.0 / (float(t.std()) + 1e-8)) <= 1e-12 * ref["rstd"]
    want = (t - t.mean()) / (t.std() + 1e-8)
    got = M.normalise(src[index], ref["mean"], ref["rstd"])
    assert got.dtype == np.float32
    # float32's rounding of a value near 1 is 6e-8: compare before it, and the rounding itself after
    f64 = (src[index].astype(np.float64) - ref["mean"]) * ref["rstd"]
    assert np.abs(f64 - want.numpy()).max() <= 1e-12 * float(want.abs().max())
    assert np.array_equal(got, f64.astype(np.float32))


def test_reference_edges():
    x = np.array([0.5, -1.25, 3.0], np.float32)
    one = M.moments(x, np.array([1], np.int32), 1e-8)
    assert one["n"] == 1 and one["mean"] == -1.25 and one["std"] == 0.0 and one["rstd"] == 1.0 / 1e-8
    none = M.moments(x, np.array([], np.int32), 1e-8)
    assert none["n"] == 0 and none["mean"] == 0.0 and none["std"] == 0.0 and none["rstd"] == 1.0 / 1e-8
    skipped = M.moments(x, np.array([0, -1, 3, 2, 70], np.int32), 1e-8)
    assert skipped["n"] == 2 and skipped["mean"] == 1.75
    everything = M.moments(x, None, 0.0)
    assert everything["n"] == 3 and everything["mean"] == 0.75
    b = M.bounds(M.moments(x, None, 1e-8))
    assert 0 < b["mean"] < 1e-14 and 0 < b["std"] < 1e-14


SIZES = [(5000, 4, 64), (4097, 4, 64), (100, 4, 64), (1000, 7, 64), (37, 3, 1), (0, 2, 64), (64, 1, 64), (129, 32, 8)]


@pytest.mark.parametrize("n,m,block", SIZES)
def test_minibatches_partition_into_aligned_blocks(n, m, block):
    g = torch.Generator().manual_seed(5)
    mbs = ppo.minibatches(n, m, generator=g, block=block)
    assert len(mbs) == m
    for t in mbs:
        assert t.dtype == torch.int32 and t.dim() == 1 and t.device.type == "cpu"
    every = torch.cat(mbs)
    assert torch.equal(torch.sort(every).values, torch.arange(n, dtype=torch.int32)), "a partition of range(n)"
    for t in mbs:  # runs of consecutive rows that start at a multiple of block and end at the next one (or at n)
        v = t.tolist()
        i = 0
        while i < len(v):
            assert v[i] % block == 0, "a block starts at a multiple of block"
            size = min(block, n - v[i])
            assert v[i:i + size] == list(range(v[i], v[i] + size)), "a block's rows are consecutive and complete"
            i += size
    lengths = [t.numel() for t in mbs]
    assert max(lengths) - min(lengths) <= block


def test_minibatches_are_seeded():
    a = ppo.minibatches(5000, 4, generator=torch.Generator().manual_seed(1))
    b = ppo.minibatches(5000, 4, generator=torch.Generator().manual_seed(1))
    c = ppo.minibatches(5000, 4, generator=torch.Generator().manual_seed(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert any(not torch.equal(x, y) for x, y in zip(a, c))
    full = ppo.minibatches(5000, 1, generator=torch.Generator().manual_seed(1), block=1)[0]
    assert not torch.equal(full, torch.arange(5000, dtype=torch.int32)), "block = 1 shuffles the rows"
    with pytest.raises(ValueError):
        ppo.minibatches(10, 0)
    with pytest.raises(ValueError):
        ppo.minibatches(10, 2, block=0)
    with pytest.raises(ValueError):
        ppo.minibatches(2 ** 31, 2)
