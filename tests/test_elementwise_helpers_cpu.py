"""The shared checkers of tests/elementwise.py reject what they are there to reject (CPU only):
a write into either sentinel band of ``Guarded``, an unwritten, must-be-zero or misshapen output
in ``worst``, one flipped mantissa bit, a signed zero, another dtype or shape in ``bitwise``."""
import pytest
import torch

from elementwise import BF, F32, INF, SENTINEL, SENTINEL_U8, Guarded, U, bits, bitwise, worst

ISENT = 0x5A5A5A5A
# dtype, explicit fill, sentinel (None: the class default), a value that is neither
GUARDED = [pytest.param(F32, None, None, 3.0, id="float32"), pytest.param(BF, None, None, 3.0, id="bf16"),
           pytest.param(torch.uint8, None, None, 3, id="uint8"), pytest.param(torch.int32, 7, ISENT, 3, id="int32")]


@pytest.mark.parametrize("dtype,fill,sentinel,other", GUARDED)
def test_guarded_bands(dtype, fill, sentinel, other):
    def make(**kw):
        return Guarded((3, 5), dtype, fill, device="cpu", guard=64, sentinel=sentinel, **kw)

    g = make()
    assert g.t.shape == (3, 5) and g.buf.numel() == 15 + 2 * 64 and g.t.data_ptr() % 16 == 0
    assert g.sent == (sentinel if sentinel is not None else SENTINEL_U8 if dtype == torch.uint8 else SENTINEL)
    if fill is None:  # the default: NaN, 255 for uint8
        assert bool((g.t == 255).all()) if dtype == torch.uint8 else bool(torch.isnan(g.t).all())
    else:
        assert bool((g.t == fill).all())
    g.check("untouched")
    g.t.fill_(other)  # the view is the kernel's to write
    g.check("written inside")
    for at in (63, 64 + 15):  # the last element of the low band, the first of the high band
        g = make()
        g.buf[at] = other
        with pytest.raises(AssertionError, match="write outside here"):
            g.check("here")
    for skew in (0, 1):  # 8 bytes longer; with 1 the view starts 8 bytes off the 16-byte grid
        g = make(skew=skew)
        pad = 8 // g.buf.element_size()
        assert g.buf.numel() == 15 + 2 * 64 + pad and g.t.data_ptr() % 16 == 8 * skew
        g.check("skewed")
        for at in (g.lo - 1, g.lo + 15, g.buf.numel() - 1):
            g = make(skew=skew)
            g.buf[at] = other
            with pytest.raises(AssertionError):
                g.check()


def test_guarded_takes_a_tensor_fill_and_an_int_shape():
    v = torch.arange(6, dtype=F32)
    g = Guarded(6, F32, v, device="cpu", guard=8)
    assert g.t.shape == (6,) and torch.equal(g.t, v)
    g.check()
    with pytest.raises(AssertionError):
        Guarded(6, torch.int32, device="cpu")  # an integer buffer has no NaN: it names its fill


def test_worst():
    ref = torch.linspace(-1.0, 1.0, 12, dtype=torch.float64).view(3, 4)
    bound = torch.full((3, 4), 1e-3, dtype=torch.float64)
    out = ref.clone()
    out[1, 2] += 1.001e-3
    r, i = worst(out, ref, bound)
    assert 1.0 < r < 1.002 and i == (1, 2)
    out[1, 2] = ref[1, 2] + 0.999e-3
    r, i = worst(out, ref, bound)
    assert 0.998 < r < 1.0 and i == (1, 2)
    out[2, 0] = float("nan")  # one unwritten element among in-bound ones
    assert worst(out, ref, bound) == (INF, (2, 0))
    out = ref.clone()
    zero = torch.zeros(3, 4, dtype=torch.bool)
    zero[0, 3] = True
    assert ref[0, 3] != 0 and worst(out, ref, bound)[0] == 0.0
    assert worst(out, ref, bound, exact_zero=zero) == (INF, (0, 3))  # in bound, but must be exactly 0
    out[0, 3] = 0.0
    assert worst(out, ref, bound + 1.0, exact_zero=zero)[0] < 1.0
    r, i = worst(out.reshape(4, 3), ref, bound)
    assert r == INF and i == ("shape", (4, 3), (3, 4))
    assert worst(torch.empty(0, 4), torch.empty(0, 4, dtype=torch.float64), 1.0) == (0.0, ())
    assert worst(torch.ones(2).to(BF), torch.ones(2, dtype=torch.float64), U)[0] == 0.0  # any dtype in


def test_bitwise():
    a = torch.tensor([1.0, -2.5, 0.0, 3.0e-5])
    assert bitwise(a, a.clone()) == (0.0, ())
    b = (bits(a) ^ torch.tensor([0, 0, 0, 1], dtype=torch.int32)).view(F32)  # one low mantissa bit
    assert torch.allclose(a, b, rtol=1e-6) and bitwise(a, b) == (INF, (3,))
    z = a.clone()
    z[2] = -0.0
    assert bool((a == z).all()) and bitwise(a, z) == (INF, (2,))
    assert bitwise(a, a.double())[0] == INF and bitwise(a.to(BF), a)[0] == INF
    assert bitwise(a, a.view(2, 2))[0] == INF and bitwise(a, a[:3])[0] == INF
    assert bitwise(None, a)[0] == INF and bitwise(a, None)[0] == INF


@pytest.mark.parametrize("dtype,raw", [(BF, torch.int16), (F32, torch.int32), (torch.int32, torch.int32),
                                       (torch.int64, torch.int64), (torch.uint8, torch.uint8)])
def test_bits_round_trips(dtype, raw):
    t = (torch.arange(-3, 5).to(dtype) if dtype != torch.uint8 else torch.arange(250, 258).to(dtype))
    if dtype.is_floating_point:
        t = t * 1.37
    b = bits(t)
    assert b.dtype == raw and b.shape == t.shape and torch.equal(b.view(dtype), t)
    assert torch.equal(bits(t.numpy() if dtype != BF else t), b)  # numpy arrays too
