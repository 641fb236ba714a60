"""Seeded random actions on the device, shared by the GPU tests (a helper, not a test). The draws are the ones
the tests have always made: one torch.Generator per call, seeded, randint first, TDM's attack flag from a
uniform draw after it, so a given (shape, seed) gives the same bits wherever it is asked for."""
import torch

DEV = "cuda:0"


def generator(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def random_flock_actions(shape, seed, continuous=False):
    """Flock actions of `shape` + (3,) uint8 in {0, 1, 2}, or continuous: `shape` + (2,) float32 in [-1, 1)."""
    g = generator(seed)
    if continuous:
        return torch.rand(tuple(shape) + (2,), device=DEV, generator=g) * 2 - 1
    return torch.randint(0, 3, tuple(shape) + (3,), dtype=torch.uint8, device=DEV, generator=g)


def random_tdm_actions(shape, seed, p_attack=0.5):
    """TDM actions of `shape` + (4,) uint8: three moves in {0, 1, 2} and the attack flag with probability p_attack."""
    g = generator(seed)
    a = torch.randint(0, 3, tuple(shape) + (4,), dtype=torch.uint8, device=DEV, generator=g)
    a[..., 3] = (torch.rand(tuple(shape), device=DEV, generator=g) < p_attack).to(torch.uint8)
    return a
