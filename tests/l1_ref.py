"""References of the flat L1 family (`emd_l1_loss`, `emd_l1_loss_ws`, `emd_abs_mean_backward`, `emd_residual_l1_backward`; kernels in
csrc/standalone_ops.hip behind csrc/api.hip) for tests/test_l1_family_gpu.py.  TEST INFRASTRUCTURE ONLY.

    loss        mean |a - b| in float64 (torch, on the tensors' device); b = None: mean |a|
    gradient    sign(a - b) fp32(1/n)
    backward    up + sign(x) (fp32(g) fp32(1/n))

Bars.  The loss keeps the project's 2e-6 relative (all terms are non-negative and the kernels' summation tree is a few dozen deep).  The
gradient images are expected BIT-EXACT: each element is a sign times ONE fp32 product (fp32(g) fp32(1/n), with fp32(1/n) = 1.f / (float)n as
the launchers form it), or one correctly rounded fp32 add of `up` on top of it (standalone_ops.hip is built without fp contraction).  The
scalar is formed here on the host in np.float32; the per-element select and the one add are torch fp32 operations on the device, which are
the same IEEE operations (the largest case is 8.4 M elements per tensor and is generated on the device).  Compared with torch.equal on int32
views, so the sign of a zero is seen:
    d == 0 (a[i] == b[i], or x[i] = +0.0 / -0.0) yields +0.0 from emd_l1_loss / _ws and emd_abs_mean_backward whatever the sign of g, and
    up + (+0.0) from emd_residual_l1_backward (so up = -0.0 gives +0.0, as the IEEE add does); a NULL g is the factor +0.0, which a
    negative x turns into -0.0 (up = -0.0 then stays -0.0).
Known, harmless difference: the kernels map sign(NaN) to 0 where torch.sign gives NaN; the tests keep NaN out of x.

Observed on an MI355X (printed by test_l1_family_gpu.py):
    every gradient image of the four entry points and of the three wrappers: bit-exact, at every size and pointer form
    loss, worst relative error per size (bar 2e-6): <= 1.5e-7 up to 8195 elements on both paths; at 512*4096 and 512*4096+4096+7 elements
    8.9e-8 and 2.9e-8 through the granule table, up to 9.1e-7 and 1.07e-6 through the float atomics (512 adds in arrival order: the value
    moves from run to run, 3.9e-7 .. 9.1e-7 seen at 512*4096 in three runs)"""
import numpy as np
import torch

GUARD_WORDS = 8
GUARD_BITS = int(np.array([0xFFA5C3E1], dtype=np.uint32).view(np.int32)[0])       # a NaN payload; compared as int32
LOSS_REL = 2e-6


def inv_n32(n):
    """1.f / (float)n."""
    return np.float32(1.0) / np.float32(n)


def factor32(g, n):
    """fp32(g) * fp32(1/n) as one fp32 product; g = None (a NULL upstream scalar) is +0.0."""
    return np.float32(0.0) if g is None else np.float32(g) * inv_n32(n)


def loss64(a, b=None):
    if a.numel() == 0:
        return 0.0
    d = a.double() if b is None else a.double() - b.double()
    return float(d.abs().mean())


def signed(d, s):
    """fp32 tensor: +s where d > 0, -s where d < 0 (-0.0 for s = +0.0), +0.0 elsewhere (s: an np.float32)."""
    pos, neg, zero = (torch.tensor(float(v), dtype=torch.float32, device=d.device) for v in (np.float32(s), -np.float32(s), 0.0))
    return torch.where(d > 0, pos, torch.where(d < 0, neg, zero))


def backward32(up, x, s):
    """up + sign(x) s, one fp32 add; up = None is +0.0."""
    return (torch.zeros_like(x) if up is None else up) + signed(x, s)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Guarded:
    """n fp32 words, 16-byte aligned, with GUARD_WORDS guard words on both sides (`shift` words moves the start off the alignment)."""

    def __init__(self, n, device, shift=0):
        self.n, self.lo = n, GUARD_WORDS + shift
        self.buf = torch.full((GUARD_WORDS + shift + (n + 3) // 4 * 4 + GUARD_WORDS,), GUARD_BITS, dtype=torch.int32, device=device)
        self.t = self.buf[self.lo:self.lo + n].view(torch.float32)
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def guards_intact(self):
        return bool((self.buf[:self.lo] == GUARD_BITS).all()) and bool((self.buf[self.lo + self.n:] == GUARD_BITS).all())

    def untouched(self):
        return bool((self.buf == GUARD_BITS).all())
