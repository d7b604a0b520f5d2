"""
The guard-band helper itself (tests/_guarded.py), on host memory: a byte written through a view into a guard, a pad column
or the last payload byte + 1 is reported with the right offset, and a clean buffer passes.  The device tests
(tests/test_gpu_guarded_*.py) rely on exactly these properties.
"""
import ctypes

import numpy
import pytest

import _guarded
from _guarded import GUARD_MIN, PATTERN, guard_bytes, guarded, guarded_2d, guarded_from

DEVICES = [None, "cpu"]          # numpy buffer, torch CPU tensor


def _poke(buf, rel, value=0):
    """Write one byte at payload offset `rel` (may be negative or >= nbytes) through the raw address."""
    ctypes.c_uint8.from_address(buf.ptr + rel).value = value


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("nbytes,align", [(0, 8), (1, 8), (8, 8), (24, 8), (4097, 16), (100000, 32), (7, 1)])
def test_payload_is_exact_aligned_and_clean(device, nbytes, align):
    g = guarded(nbytes, align, device, fill=0x11)
    assert g.ptr % align == 0 and g.ptr % (2 * align) == align           # the weakest alignment promised, no more
    assert g.bytes().shape[0] == nbytes
    assert g.off >= GUARD_MIN and g.base.shape[0] - g.off - nbytes >= GUARD_MIN
    assert bytes(g.get(numpy.uint8)) == b"\x11" * nbytes
    assert g.first_damage() is None
    g.check()
    # writing every payload byte is not damage
    if nbytes:
        g.bytes()[:] = 0
    g.check()


@pytest.mark.parametrize("device", DEVICES)
def test_guard_is_two_row_strides_at_least(device):
    assert guard_bytes(0) == GUARD_MIN and guard_bytes(GUARD_MIN) == 2 * GUARD_MIN
    assert guard_bytes(8192 * 8 + 24) >= 2 * (8192 * 8 + 24) and guard_bytes(1000001) % 256 == 0
    m = guarded_2d(3, 70000, 70003, numpy.float64, device=device)
    assert m.buf.guard >= 2 * 70003 * 8
    assert m.buf.off >= m.buf.guard and m.buf.base.shape[0] - m.buf.off - m.buf.nbytes >= m.buf.guard


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("rel_of", [lambda n, g: n, lambda n, g: -1, lambda n, g: n + g - 1, lambda n, g: -g,
                                    lambda n, g: n + 4095, lambda n, g: -4096])
def test_a_byte_in_a_guard_is_reported_with_its_offset(device, rel_of):
    nbytes = 808
    g = guarded(nbytes, 8, device, fill=0)
    rel = rel_of(nbytes, g.guard)
    _poke(g, rel, 0x00)
    assert g.first_damage() == rel
    with pytest.raises(AssertionError, match=r"payload offset %d " % rel):
        g.check("colsum")
    _poke(g, rel, PATTERN)
    g.check()


@pytest.mark.parametrize("device", DEVICES)
def test_the_first_of_several_damaged_bytes_is_named(device):
    g = guarded(64, 8, device)
    _poke(g, 64 + 9), _poke(g, 64 + 3), _poke(g, 64 + 100)
    assert g.first_damage() == 67
    _poke(g, -5)
    assert g.first_damage() == -5                                            # the front guard is looked at first


@pytest.mark.parametrize("device", DEVICES)
def test_the_last_payload_byte_is_payload_and_the_next_is_not(device):
    g = guarded(16, 8, device, fill=0)
    _poke(g, 15, 0x7F)
    g.check()
    assert g.get(numpy.uint8)[15] == 0x7F
    _poke(g, 16, 0x7F)
    with pytest.raises(AssertionError, match="0 bytes past its end"):
        g.check()


@pytest.mark.parametrize("device", DEVICES)
def test_typed_views_share_the_payload(device):
    vals = numpy.arange(12, dtype=numpy.float64) - 3.5
    g = guarded_from(vals, numpy.float64, 8, device)
    assert g.nbytes == 96 and numpy.array_equal(g.get(numpy.float64), vals)
    v = g.view(numpy.float64, (3, 4))
    v[2, 3] = 99.0
    assert g.get(numpy.float64, (3, 4))[2, 3] == 99.0
    g.check()
    i = guarded_from([1, -2, 3], numpy.int32, 8, device)
    assert i.nbytes == 12 and list(i.get(numpy.int32)) == [1, -2, 3]
    # what a read past the end sees: the pattern is NaN / -1 / a huge unsigned value
    past = numpy.frombuffer((ctypes.c_uint8 * 8).from_address(i.ptr + 12), dtype=numpy.uint8)
    assert numpy.isnan(past.view(numpy.float64)[0]) and numpy.isnan(past.view(numpy.float32)).all()
    assert past.view(numpy.int64)[0] == -1 and past.view(numpy.uint16)[0] == 65535
    with pytest.raises(ValueError):
        guarded(12, 8, device).view(numpy.float64)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype,width,ld", [(numpy.float64, 66, 69), (numpy.float32, 5, 12), (numpy.uint8, 3, 8),
                                           (numpy.float64, 4, 4)])
def test_2d_pads(device, dtype, width, ld):
    item = numpy.dtype(dtype).itemsize
    vals = (numpy.arange(7 * width) % 200).reshape(7, width).astype(dtype)
    m = guarded_2d(7, width, ld, dtype, device=device).put(vals)
    assert m.buf.nbytes == 7 * ld * item                                     # exactly [R][ld], the last row's pad included
    assert numpy.array_equal(m.get(), vals)
    m.check(pads="unchanged")
    if ld == width:
        m.check(pads="zero")                                                 # nothing to look at
        return
    if numpy.dtype(dtype).kind == "f":
        assert numpy.isnan(numpy.asarray(m.buf.get(dtype, (7, ld)))[:, width:]).all()   # an input's pads read as NaN
    with pytest.raises(AssertionError, match="must be zero"):
        m.check(pads="zero")
    # one byte of one pad column: row 4, the second byte of the last pad column
    rel = (4 * ld + ld - 1) * item + (1 if item > 1 else 0)
    _poke(m.buf, rel, 0x00)
    with pytest.raises(AssertionError, match=r"row 4 column %d \(byte %d of it\)" % (ld - 1, 1 if item > 1 else 0)):
        m.check(pads="unchanged")
    m.buf.check()                                                            # a pad column is payload, not guard
    # the pads written as 0 by a call
    m.mat()[:, width:] = 0
    m.check(pads="zero")
    with pytest.raises(AssertionError, match="must be unchanged"):
        m.check(pads="unchanged")
    assert numpy.array_equal(m.get(), vals)


@pytest.mark.parametrize("device", DEVICES)
def test_2d_defined_pads_and_the_byte_behind_the_last_row(device):
    m = guarded_2d(5, 66, 72, numpy.uint8, device=device, pad=0).put(numpy.full((5, 66), 65))      # E: "pad bytes 0"
    m.check(pads="zero")
    m.check(pads="unchanged")
    _poke(m.buf, 5 * 72)
    with pytest.raises(AssertionError, match="0 bytes past its end"):
        m.check()


def test_bad_arguments():
    with pytest.raises(ValueError):
        guarded(8, 12)
    with pytest.raises(ValueError):
        guarded(-1, 8)
    with pytest.raises(ValueError):
        guarded_2d(2, 9, 8, numpy.float64)
    with pytest.raises(ValueError):
        guarded_2d(2, 4, 8, numpy.float64).check_pads("maybe")
    assert _guarded.PATTERN == 0xFF
