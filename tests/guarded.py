"""Guarded operands for the kernel tests (test-side only; launches nothing).

Every per-kernel test used to hand its kernel fresh, dense, allocator-aligned tensors, so a kernel that used a width where
it should use a leading dimension, stored a row or four columns past its tile, or read a row too many went unnoticed.
This module places an operand inside a larger buffer of ordinary allocated memory:

  strided(...)  a 2-D operand as a row-strided, column-offset view  buf[r0 : r0 + rows, c0 : c0 + width]  with
                ld = buf.stride(0) > width, at least GUARD_ROWS (256 = the largest row tile of any kernel,
                expert_gemm_g256.hip) rows above and below and guard columns left and right (ld = c0 + width is the
                smallest stride: the elements behind a row's end are then the next row's left guard).  The view's data pointer is
                16-byte aligned but neither 64- nor 128-byte aligned (c0 = 16 bytes; the rows above it are a multiple of
                1024 bytes).
  flat(...)     a dense operand of any shape with GUARD_ROWS * 64 guard elements before and after (operators whose ABI
                has no stride); the data pointer stays 256-byte aligned.

Inputs: the guard holds NaN (floating point) or a caller-chosen integer, the view holds the data.  A kernel that consumes
a guard element produces a wrong VALUE.  Integer guards are chosen per operand by the caller so that a consumed guard can
never become an out-of-range ADDRESS (see `int_guard` at the call sites).
Outputs: the whole buffer holds a fixed bit pattern -- for floating point a signalling-NaN payload no kernel produces --
and check() asserts bit for bit that every guard element still holds it, naming the first offender relative to the view.
"""
import torch

GUARD_ROWS = 256
FLAT_GUARD = GUARD_ROWS * 64

# bit patterns per element size (bytes): fp32 / int32 0x7fa5a5a5 and bf16 0x7fa5 are signalling NaNs (exponent all ones,
# quiet bit clear, payload non-zero)
_PATTERN = {4: 0x7FA5A5A5, 2: 0x7FA5, 1: 0xA5}
_INT_OF = {4: torch.int32, 2: torch.int16, 1: torch.uint8}


def _pattern(itemsize):
    return _PATTERN[itemsize]


def _bits(t):
    """the tensor's elements as integers of the same size (a view: no copy, no rounding)"""
    return t if t.dtype in (torch.int32, torch.int16, torch.uint8) else t.view(_INT_OF[t.element_size()])


def _fill_guard(buf, dtype, int_guard):
    if dtype.is_floating_point:
        buf.fill_(float("nan"))
    else:
        assert int_guard is not None, "integer inputs need a guard value chosen for the operand's use"
        buf.fill_(int_guard)


class Guarded:
    """An operand view inside its guard buffer.  `view` is what the kernel gets; `ld` its row stride in elements (2-D)."""

    def __init__(self, buf, view, origin, is_output):
        self.buf, self.view, self.origin, self.is_output = buf, view, origin, is_output
        self.ld = view.stride(0) if view.dim() == 2 else None

    def _mask(self):
        """True on guard elements of buf (2-D for strided placement, 1-D for flat)"""
        m = torch.ones(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        if self.buf.dim() == 2:
            (r0, c0), (rows, width) = self.origin, self.view.shape
            m[r0:r0 + rows, c0:c0 + width] = False
        else:
            m[self.origin:self.origin + self.view.numel()] = False
        return m

    def check(self, name="output"):
        """every guard element still holds the fill pattern, bit for bit"""
        assert self.is_output, "only output guards hold a pattern"
        bits = _bits(self.buf)
        bad = (bits != _pattern(self.buf.element_size())) & self._mask()
        if bool(bad.any()):
            first = bad.nonzero()[0].tolist()
            n = int(bad.sum())
            if self.buf.dim() == 2:
                where = "(row %d, column %d) relative to the view of %d x %d" % (
                    first[0] - self.origin[0], first[1] - self.origin[1], self.view.shape[0], self.view.shape[1])
            else:
                where = "element %d relative to the operand of %d elements" % (first[0] - self.origin, self.view.numel())
            raise AssertionError("%s: %d guard element(s) overwritten, first at %s" % (name, n, where))

    def untouched(self):
        """True where the VIEW still holds the fill pattern (an output the kernel must have written everywhere)"""
        return _bits(self.view) == _pattern(self.buf.element_size())


def strided(rows, width, dtype, device="cuda", data=None, ld=None, int_guard=None):
    """Row-strided, column-offset placement.  data=None: an output (pattern everywhere); else an input holding `data`
    with NaN / int_guard around it.  ld: row stride of the buffer in elements (default: 16 bytes of columns on either side,
    rounded up to 16 bytes)."""
    per16 = 16 // torch.empty((), dtype=dtype).element_size()
    c0 = per16
    if ld is None:
        ld = -(-(c0 + width + per16) // per16) * per16
    assert ld >= c0 + width, "no room for the guard columns"   # (row-major: the columns right of a row are the next row's left guard)
    r0 = GUARD_ROWS
    total = r0 + rows + GUARD_ROWS
    if data is None:
        isz = torch.empty((), dtype=dtype).element_size()
        buf = torch.full((total, ld), _pattern(isz), dtype=_INT_OF[isz], device=device)
        buf = buf if dtype == _INT_OF[isz] else buf.view(dtype)
    else:
        assert tuple(data.shape) == (rows, width) and data.dtype == dtype
        buf = torch.empty((total, ld), dtype=dtype, device=device)
        _fill_guard(buf, dtype, int_guard)
        buf[r0:r0 + rows, c0:c0 + width] = data.to(device)
    view = buf[r0:r0 + rows, c0:c0 + width]
    assert view.data_ptr() % 16 == 0
    return Guarded(buf, view, (r0, c0), data is None)


def strided_in(data, device="cuda", ld=None, int_guard=None):
    return strided(data.shape[0], data.shape[1], data.dtype, device, data=data, ld=ld, int_guard=int_guard)


def strided_out(rows, width, dtype=torch.float32, device="cuda", ld=None):
    return strided(rows, width, dtype, device, ld=ld)


def flat(shape, dtype, device="cuda", data=None, int_guard=None, guard=FLAT_GUARD):
    """Dense placement with flat guards before and after.  data=None: an output."""
    shape = tuple(shape)
    n = 1
    for s in shape:
        n *= s
    isz = torch.empty((), dtype=dtype).element_size()
    lead = -(-guard * isz // 256) * 256 // isz          # keeps the operand 256-byte aligned
    total = lead + n + guard
    if data is None:
        buf = torch.full((total,), _pattern(isz), dtype=_INT_OF[isz], device=device)
        buf = buf if dtype == _INT_OF[isz] else buf.view(dtype)
    else:
        assert tuple(data.shape) == shape and data.dtype == dtype
        buf = torch.empty((total,), dtype=dtype, device=device)
        _fill_guard(buf, dtype, int_guard)
        buf[lead:lead + n] = data.to(device).reshape(-1)
    view = buf[lead:lead + n].view(shape)
    return Guarded(buf, view, lead, data is None)


def flat_in(data, device="cuda", int_guard=None):
    return flat(data.shape, data.dtype, device, data=data, int_guard=int_guard)


def flat_out(shape, dtype=torch.float32, device="cuda"):
    return flat(shape, dtype, device)


def dense(view):
    """a dense copy of a (strided) view, for the comparison"""
    return view.contiguous().clone()


def same_bits(a, b):
    """bit-for-bit equality (NaN payloads and signed zeros included)"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))
