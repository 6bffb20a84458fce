"""What the "per element against float64" tests share: seeded inputs, conversions, the guarded
output buffer and the checkers that turn (output, float64 reference, a-priori bound) into a
verdict.  A helper module, not a test module; nothing here touches a device at import time, so
the CPU tests that import the ``*_cases.py`` modules can import it without a GPU.
tests/test_elementwise_helpers_cpu.py shows that the checkers reject what they are there to
reject.

One definition of each, so a fix reaches every test file: where the earlier per-file copies
differed, this one is the stricter (``bitwise`` refuses a dtype mismatch, ``worst`` counts an
unwritten or a must-be-zero element as infinitely out of bound, ``Guarded.check`` compares
against the instance's own sentinel).
"""
import math

import numpy as np
import torch

from ddp_amd.ops.kernel_bounds import U  # noqa: F401  (2**-24, re-exported)

BF = torch.bfloat16
F32 = torch.float32
INF = float("inf")
GUARD = 8192       # sentinel elements on each side (a multiple of 8: 16-byte alignment kept)
SENTINEL = 1152.0  # 9 * 128: exact in bf16 and fp32
SENTINEL_U8 = 165


# ---------------------------------------------------------------------- inputs, conversions
def rnd(*shape, scale=1.0, seed=0, relu=False, dtype=BF, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g) * scale
    return (torch.relu(t) if relu else t).to(dtype).to(device)


def f64(t):
    return t.detach().cpu().double()


def bf(t):
    return t.detach().cpu().float().to(BF)


def n32(v):
    return float(np.float32(v))


def nchw(t, dtype=torch.float64):  # NHWC tensor -> ``dtype`` NCHW on the CPU
    return t.detach().cpu().to(dtype).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def bits(t):
    """The bit patterns of ``t`` (a tensor or a numpy array) as the integer of its element size."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ---------------------------------------------------------------------------- guarded buffer
class Guarded:
    """A tensor ``t`` between two sentinel bands of ``guard`` elements in one allocation ``buf``.

    ``fill`` None: NaN (uint8: 255) - every element the kernel should write is seen if it does
    not; a scalar or a tensor otherwise.  ``shape`` may be an int.  ``sentinel`` None: SENTINEL
    (uint8: SENTINEL_U8); integer buffers name their own.  ``skew`` None: the view starts on the
    16-byte grid.  0 / 1: the allocation is 8 bytes longer and, with 1, the view starts 8 bytes
    later - off the 16-byte grid."""

    def __init__(self, shape, dtype, fill=None, device="cuda", guard=GUARD, sentinel=None, skew=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        u8 = dtype == torch.uint8
        self.sent = (SENTINEL_U8 if u8 else SENTINEL) if sentinel is None else sentinel
        pad = 0 if skew is None else 8 // torch.empty(0, dtype=dtype).element_size()
        self.lo = guard + (pad if skew else 0)
        self.buf = torch.full((n + 2 * guard + pad,), self.sent, dtype=dtype, device=device)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if fill is None:
            assert u8 or dtype.is_floating_point, "an integer buffer names its fill"
            fill = 255 if u8 else float("nan")
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill)
        else:
            self.t.fill_(fill)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (8 if skew else 0)

    def check(self, what=""):
        lo, hi = self.buf[:self.lo], self.buf[self.lo + self.t.numel():]
        assert bool((lo == self.sent).all()) and bool((hi == self.sent).all()), f"write outside {what}"


# ---------------------------------------------------------------------------------- checkers
def worst(out, ref, bound, exact_zero=None):
    """(max |out - ref| / bound, index of the worst element); a non-finite output or a non-zero
    element under ``exact_zero`` counts as infinitely far out, and so does another shape than
    the reference's (the index then holds the two shapes)."""
    o = f64(out)
    if tuple(o.shape) != tuple(ref.shape):
        return INF, ("shape", tuple(o.shape), tuple(ref.shape))
    rr = (o - ref).abs() / (bound + 1e-300)
    rr = torch.where(torch.isfinite(o), rr, torch.full_like(rr, INF))
    if exact_zero is not None:
        rr = torch.where(exact_zero & (o != 0), torch.full_like(rr, INF), rr)
    if rr.numel() == 0:
        return 0.0, ()
    i = int(rr.reshape(-1).argmax())
    return rr.reshape(-1)[i].item(), tuple(int(v) for v in np.unravel_index(i, tuple(rr.shape)))


def bitwise(out, want):
    """(0 or inf, first differing index): a stage that must match bit for bit.  None, another
    shape or another dtype is a mismatch."""
    if out is None or want is None or tuple(out.shape) != tuple(want.shape) or out.dtype != want.dtype:
        return INF, ("shape / dtype",)
    a, b = bits(out).reshape(-1), bits(want).reshape(-1)
    d = torch.nonzero(a != b)
    return (0.0, ()) if d.numel() == 0 else (INF, (int(d[0]),))


def failing(res, order=None):
    """The stages of ``res`` {stage: (error / bound, index)} out of bound, in ``order`` (the order
    the stages depend on each other in; None: the order ``res`` holds them in)."""
    return [s for s in (res if order is None else order) if s in res and not res[s][0] <= 1.0]


def report(res, *labels, tag, order=None):
    """One ``<tag> <labels...> <stage> <error / bound>`` line per stage of ``res``, in ``order``."""
    head = " ".join(str(v) for v in (tag,) + labels)
    for s in (res if order is None else order):
        if s in res:
            print(f"{head} {s} {res[s][0]:.3e}")


def report_ratio(r, *labels, tag):
    """The ``<tag> <labels...> <error / bound>`` line of a test that asserts on one ratio itself."""
    print(" ".join(str(v) for v in (tag,) + labels) + f" {r:.4f}")
