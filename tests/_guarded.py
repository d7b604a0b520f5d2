"""
Red zones inside our own allocations: every buffer a test hands to the C ABI (include/mixemt_hip.h) is a view of EXACTLY
the documented size in the middle of one larger allocation whose front and back are filled with 0xFF bytes.

  - a write past either end lands in a guard -- our own memory, never a neighbour's -- and check() names the first changed
    byte by its offset relative to the payload (negative: before it; >= nbytes: behind it);
  - a read past either end sees 0xFF bytes: NaN as a double or a float, -1 as a signed index, a huge unsigned value, so it
    poisons the result or trips the library's own range checks -- which is why every guarded test also compares values;
  - the payload starts at an odd multiple of `align` (a multiple of `align` and not of 2 * align): the weakest alignment the
    header promises for the argument, not the 256 bytes and more an allocator hands out.

Works the same on numpy buffers (device=None: the host entries), torch CPU tensors and torch device tensors.  A helper
module, not a conftest: tests import it by name.
"""
import numpy

GUARD_MIN = 256 * 1024          # bytes of each guard at least; and at least two row strides of the buffer (guard_bytes())
PATTERN = 0xFF                  # the guards' byte, and the default pad of an input matrix


def guard_bytes(row_bytes=0):
    """Size of each guard: at least GUARD_MIN and at least two row strides, rounded up to 256 bytes.  A condition, not a
    measurement: an overrun of a row or less must stay inside the allocation it belongs to."""
    need = max(GUARD_MIN, 2 * int(row_bytes))
    return (need + 255) // 256 * 256


def _is_torch(device):
    return device is not None and str(device) != "numpy"


class Guarded:
    """One guarded buffer: `base` is the whole allocation (uint8), the payload is base[off : off + nbytes]."""

    def __init__(self, nbytes, align=8, device=None, fill=PATTERN, row_bytes=0):
        nbytes, align = int(nbytes), int(align)
        if nbytes < 0 or align < 1 or (align & (align - 1)):
            raise ValueError("guarded: nbytes >= 0 and a power-of-two align, got %d / %d" % (nbytes, align))
        self.nbytes, self.align, self.device = nbytes, align, device
        self.guard = guard_bytes(row_bytes)
        total = 2 * self.guard + nbytes + 2 * align
        if _is_torch(device):
            import torch
            self.base = torch.full((total,), PATTERN, dtype=torch.uint8, device=device)
            addr = self.base.data_ptr()
        else:
            self.base = numpy.full(total, PATTERN, dtype=numpy.uint8)
            addr = self.base.ctypes.data
        # the first address >= addr + guard that is an odd multiple of align
        first = addr + self.guard
        shift = (align - first % (2 * align)) % (2 * align)
        self.off = self.guard + shift
        self.ptr = addr + self.off
        assert self.ptr % align == 0 and self.ptr % (2 * align) == align and self.off >= self.guard
        assert total - self.off - nbytes >= self.guard
        if fill is not None and fill != PATTERN and nbytes:
            self.base[self.off:self.off + nbytes] = int(fill)

    # -- views ----------------------------------------------------------------------------------------------------
    def bytes(self):
        """The payload as uint8[nbytes] (a view)."""
        return self.base[self.off:self.off + self.nbytes]

    def view(self, dtype, shape=None):
        """The payload as `dtype` (a numpy dtype; torch buffers take the torch dtype of the same name), optionally reshaped."""
        dt = numpy.dtype(dtype)
        if self.nbytes % dt.itemsize:
            raise ValueError("guarded: %d bytes are no whole number of %s" % (self.nbytes, dt))
        if _is_torch(self.device):
            import torch
            v = self.bytes().view(getattr(torch, dt.name))
        else:
            v = self.bytes().view(dt)
        return v if shape is None else v.reshape(shape)

    def put(self, values, dtype=None):
        """Copy a numpy array into the payload (must fill it exactly)."""
        a = numpy.ascontiguousarray(values, dtype=dtype)
        if a.nbytes != self.nbytes:
            raise ValueError("guarded: %d bytes into a payload of %d" % (a.nbytes, self.nbytes))
        raw = a.reshape(-1).view(numpy.uint8)
        if _is_torch(self.device):
            import torch
            self.bytes().copy_(torch.from_numpy(raw.copy()))
        else:
            self.bytes()[:] = raw
        return self

    def get(self, dtype, shape=None):
        """The payload copied out as a numpy array."""
        dt = numpy.dtype(dtype)
        raw = self.bytes().cpu().numpy() if _is_torch(self.device) else self.bytes()
        v = raw.copy().view(dt)
        return v if shape is None else v.reshape(shape)

    # -- the check ------------------------------------------------------------------------------------------------
    def _first_changed(self, lo, hi):
        part = self.base[lo:hi]
        if _is_torch(self.device):
            bad = (part != PATTERN).nonzero()
            return None if bad.numel() == 0 else lo + int(bad[0, 0])
        bad = numpy.flatnonzero(part != PATTERN)
        return None if bad.size == 0 else lo + int(bad[0])

    def first_damage(self):
        """Offset relative to the payload of the first guard byte that no longer holds the pattern, or None."""
        for lo, hi in ((0, self.off), (self.off + self.nbytes, self.base.shape[0])):
            at = self._first_changed(lo, hi)
            if at is not None:
                return at - self.off
        return None

    def check(self, what="buffer"):
        at = self.first_damage()
        if at is not None:
            where = "%d bytes BEFORE its start" % -at if at < 0 else "%d bytes past its end" % (at - self.nbytes)
            raise AssertionError("%s (%d bytes): guard byte at payload offset %d was written (%s)"
                                 % (what, self.nbytes, at, where))


def guarded(nbytes, align=8, device=None, fill=PATTERN, row_bytes=0):
    """A view of exactly `nbytes` bytes inside ONE larger allocation with a 0xFF guard on either side (class Guarded).
    `fill` is the payload's byte (None or 0xFF: the pattern itself); `row_bytes` the row stride of the buffer it protects."""
    return Guarded(nbytes, align, device, fill, row_bytes)


def guarded_from(values, dtype, align=8, device=None, row_bytes=0):
    """A guarded buffer of exactly values.nbytes bytes holding `values`."""
    a = numpy.ascontiguousarray(values, dtype=dtype)
    return Guarded(a.nbytes, align, device, None, row_bytes).put(a)


class Guarded2D:
    """An [R][ld] matrix with ld >= width of exactly R * ld elements, guarded; columns [width, ld) are its PAD columns.

    pad: the byte the pad columns are filled with -- 0xFF for an input (NaN / -1: a kernel that reads them poisons its
    result) unless the header defines them (E's "pad bytes 0": pad=0), and a sentinel for an output, which check_pads()
    afterwards requires to be "zero" (the header says "written as 0") or "unchanged" (it says "left alone")."""

    def __init__(self, rows, width, ld, dtype, align=8, device=None, pad=PATTERN, fill=PATTERN):
        self.rows, self.width, self.ld, self.dtype, self.pad = int(rows), int(width), int(ld), numpy.dtype(dtype), int(pad)
        if self.ld < self.width:
            raise ValueError("guarded 2-D: ld %d < width %d" % (ld, width))
        item = self.dtype.itemsize
        self.buf = Guarded(self.rows * self.ld * item, align, device, fill, row_bytes=self.ld * item)
        self.ptr, self.device = self.buf.ptr, device
        self._pad_bytes()[...] = self.pad

    def _pad_bytes(self):
        item = self.dtype.itemsize
        return self.buf.bytes().reshape(self.rows, self.ld * item)[:, self.width * item:]

    def mat(self):
        """The whole [R][ld] matrix (a view)."""
        return self.buf.view(self.dtype, (self.rows, self.ld))

    def put(self, values):
        """Copy a numpy [R][width] array into the payload columns; the pad columns keep their byte."""
        a = numpy.ascontiguousarray(values, dtype=self.dtype)
        if a.shape != (self.rows, self.width):
            raise ValueError("guarded 2-D: shape %r into [%d][%d]" % (a.shape, self.rows, self.width))
        if _is_torch(self.device):
            import torch
            self.mat()[:, :self.width] = torch.from_numpy(a).to(self.device)
        else:
            self.mat()[:, :self.width] = a
        return self

    def get(self):
        """The payload columns [R][width] copied out as a numpy array."""
        v = self.mat()[:, :self.width]
        return v.cpu().numpy().copy() if _is_torch(self.device) else v.copy()

    def first_pad_damage(self, want):
        """(row, byte offset inside the row's pad) of the first pad byte that is not `want`, or None."""
        pads = self._pad_bytes()
        if pads.shape[1] == 0 or self.rows == 0:
            return None
        if _is_torch(self.device):
            bad = (pads != want).nonzero()
            return None if bad.numel() == 0 else (int(bad[0, 0]), int(bad[0, 1]))
        bad = numpy.argwhere(pads != want)
        return None if bad.shape[0] == 0 else (int(bad[0, 0]), int(bad[0, 1]))

    def check_pads(self, state, what="matrix"):
        """state "zero": every pad byte is 0 (the call writes its pad columns as 0); "unchanged": every pad byte still
        holds the byte it was given (the call leaves them alone)."""
        if state not in ("zero", "unchanged"):
            raise ValueError("check_pads: 'zero' or 'unchanged'")
        want = 0 if state == "zero" else self.pad
        at = self.first_pad_damage(want)
        if at is not None:
            item = self.dtype.itemsize
            raise AssertionError("%s [%d][%d] width %d: pad columns must be %s, but row %d column %d (byte %d of it) is not"
                                 % (what, self.rows, self.ld, self.width, state, at[0], self.width + at[1] // item,
                                    at[1] % item))

    def check(self, what="matrix", pads=None):
        self.buf.check(what)
        if pads is not None:
            self.check_pads(pads, what)


def guarded_2d(rows, width, ld, dtype, align=8, device=None, pad=PATTERN, fill=PATTERN):
    return Guarded2D(rows, width, ld, dtype, align, device, pad, fill)
