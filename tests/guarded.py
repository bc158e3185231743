"""Device buffers framed by guard bytes: [guard 4 KiB | body of exactly nbytes | guard 4 KiB] in one allocation, for the tests of
the exact workspace and full-output contracts of the library's exports (tests/test_gpu_workspace.py, tests/test_gpu_helpers.py).
Every write a test can provoke past the body lands in a guard of the same allocation."""
import numpy as np
import torch

GUARD = 4096


def _bytes(n, seed):
    return torch.as_tensor(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)).cuda()


class Guarded:
    """A body of exactly `nbytes` between two guards of fixed random bytes.  fill: a byte value (0xFF = NaN as float64, -1 as
    int64), or 'random' for seeded random bytes."""

    def __init__(self, nbytes, fill=0xFF, seed=0):
        self.nbytes = int(nbytes)
        self.seed = seed
        self.raw = torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device='cuda')
        self.lo, self.hi = _bytes(GUARD, 1000 + seed), _bytes(GUARD, 2000 + seed)
        self.raw[:GUARD] = self.lo
        self.raw[GUARD + self.nbytes:] = self.hi
        self.body = self.raw[GUARD:GUARD + self.nbytes]
        self.fill(fill)

    @classmethod
    def of(cls, dtype, shape, fill=0xFF, seed=0):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        g = cls(n, fill, seed)
        g.dtype, g.shape = dtype, tuple(shape)
        return g

    def fill(self, how):
        if how == 'random':
            self.body.copy_(_bytes(self.nbytes, 3000 + self.seed))
        else:
            self.body.fill_(int(how))
        return self

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def tensor(self, dtype=None, shape=None):
        dtype = dtype or self.dtype
        shape = shape if shape is not None else self.shape
        return self.body.view(dtype).view(shape)

    def host(self, dtype=None, shape=None):
        return self.tensor(dtype, shape).cpu().numpy()

    def untouched(self, byte, start=0):
        """Every byte of the body from `start` on still equals `byte`."""
        return bool(self.body[start:].eq(byte).all())

    def intact(self):
        return bool(torch.equal(self.raw[:GUARD], self.lo)) and bool(torch.equal(self.raw[GUARD + self.nbytes:], self.hi))


def same_bits(a, b):
    """Bit-for-bit equality of two numpy arrays (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
