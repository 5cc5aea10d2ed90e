"""Guarded buffers for the containment tests: a logical [rows, cols] (or [B, rows, cols], or [n]) tensor carved out of one larger flat
allocation, at a non-zero element offset, with row stride ld >= cols and a band of ordinary allocated memory (>= 1 MiB) before and after it.
Everything that is not the logical extent -- both bands and the ld - cols gap behind every row -- is the GUARD and holds one fixed quiet-NaN
bit pattern.

    role 'out'  guard AND extent start as the pattern.  check() asserts afterwards that the guard is unchanged bit for bit (compared as
                integers, never as floats) and that no extent element still holds the pattern: an element the kernel never wrote, or one it
                computed from guard memory (a NaN operand hands its payload on), is reported like a stray write, as (row, column) relative to
                the extent.  With `fill` (a number or a tensor) the extent is pre-filled instead -- the outputs a contract says are
                accumulated into -- and only the guard carries the pattern.
    role 'in'   the extent holds `data`, the guard the pattern; a kernel whose result depends on memory around its input produces NaN, which
                the value comparison (assert_close) reports with its (row, column).

Nothing here provokes a fault: the guard is plain memory that is read back after the call."""
import torch

BAND_BYTES = 1 << 20
NAN32 = 0x7FC17FC1                      # quiet NaN as float32; each 16-bit half (0x7FC1) is a quiet NaN as bfloat16 / float16 too
NAN64 = 0x7FF87FC17FC17FC1              # quiet NaN as float64; its 32-bit halves are quiet NaNs as float32
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class GuardError(AssertionError):
    """A guard word changed, or an extent element was left holding the guard pattern.  row / col are relative to the extent (row -1 or
    col >= cols: in front of the base / in the gap behind a row); kind is 'guard' or 'extent'."""

    def __init__(self, name, kind, row, col, msg):
        super().__init__(f'{name}: {msg} at (row {row}, column {col})')
        self.name, self.kind, self.row, self.col = name, kind, row, col


def _pattern(nbytes, itemsize, device):
    """nbytes (a multiple of 8) of the pattern, as the integer type of `itemsize` bytes."""
    if itemsize == 8:
        return torch.full((nbytes // 8,), NAN64, dtype=torch.int64, device=device)
    return torch.full((nbytes // 4,), NAN32, dtype=torch.int32, device=device).view(_INT[itemsize])


class Guarded:
    def __init__(self, shape, ld=None, offset=64, band=BAND_BYTES, role='out', dtype=torch.float32, device='cpu', data=None, fill=None,
                 name='buffer'):
        shape = tuple(int(s) for s in shape)
        assert 1 <= len(shape) <= 3 and role in ('in', 'out') and offset > 0 and band >= BAND_BYTES
        self.shape, self.role, self.name, self.dtype = shape, role, name, dtype
        self.cols = shape[-1]
        self.rows = 1 if len(shape) == 1 else shape[-2]
        self.batch = shape[0] if len(shape) == 3 else 1
        self.ld = int(ld) if ld is not None else self.cols
        assert self.ld >= self.cols
        self.isz = torch.empty(0, dtype=dtype).element_size()
        self.idt = _INT[self.isz]
        band_el = -(-band // self.isz)
        self.base = band_el + int(offset)
        self.nrows = self.batch * self.rows                                   # rows of the flat [batch * rows, ld] picture
        self.span = (self.nrows - 1) * self.ld + self.cols if self.nrows and self.cols else 0
        total = self.base + self.span + band_el
        self.nbytes = -(-total * self.isz // 8) * 8
        self.flat = _pattern(self.nbytes, self.isz, device)                   # integer view of the whole allocation
        self.t = self._extent(self.flat.view(dtype))                          # the logical tensor the kernel is handed
        self.prefilled = role == 'in' or fill is not None
        if self.isz == 1:                  # byte buffers are compared as 16-bit halves of the pattern: even placement, no row gaps
            assert self.base % 2 == 0 and self.span % 2 == 0 and self.ld == self.cols
        if role == 'in':
            assert data is not None
            self.t.copy_(torch.as_tensor(data).to(device=device, dtype=dtype))
        elif fill is not None:
            if torch.is_tensor(fill):
                self.t.copy_(fill.to(device=device, dtype=dtype))
            else:
                self.t.fill_(fill)

    def _extent(self, flat):
        strides = {1: (1,), 2: (self.ld, 1), 3: (self.rows * self.ld, self.ld, 1)}[len(self.shape)]
        return torch.as_strided(flat, self.shape, strides, self.base)

    def _rowcol(self, index):
        rel = int(index) - self.base
        return rel // self.ld, rel % self.ld

    CHUNK = 1 << 26                        # elements compared at a time: the transient memory of a check is one boolean chunk

    def _scan(self, lo, hi):
        """flat[lo:hi] is guard: raise at the first element that is not the pattern."""
        pat = {2: 0x7FC1, 4: NAN32, 8: NAN64}.get(self.isz)
        for a in range(lo, hi, self.CHUNK):
            b = min(hi, a + self.CHUNK)
            if self.isz == 1:              # (a, b even) two bytes at a time: 0xC1 0x7F in memory
                bad = self.flat[a:b].view(torch.int16) != 0x7FC1
            else:
                bad = self.flat[a:b] != pat
            if bool(bad.any()):
                i = int(bad.to(torch.uint8).argmax())
                if self.isz == 1:
                    i = 2 * i + (0 if int(self.flat[a + 2 * i]) != 0xC1 else 1)
                row, col = self._rowcol(a + i)
                raise GuardError(self.name, 'guard', row, col, f'guard memory changed ({int(bad.sum())} elements in this stretch; first')

    def check(self, written=None):
        """Guard unchanged bit for bit; for an 'out' buffer that was not pre-filled also: no extent element still holds the pattern.  The
        bands are compared in place, chunk by chunk, and the row gaps through a strided view: no copy of the buffer is made."""
        self._scan(0, self.base)
        if self.ld > self.cols and self.nrows > 1:
            gap = torch.as_strided(self.flat, (self.nrows - 1, self.ld - self.cols), (self.ld, 1), self.base + self.cols)
            bad = gap != {2: 0x7FC1, 4: NAN32, 8: NAN64}[self.isz]
            if bool(bad.any()):
                i = int(bad.reshape(-1).to(torch.uint8).argmax())
                raise GuardError(self.name, 'guard', i // (self.ld - self.cols), self.cols + i % (self.ld - self.cols),
                                 f'guard memory changed ({int(bad.sum())} elements in the row gaps; first')
        self._scan(self.base + self.span, self.flat.numel())
        if written is None:
            written = not self.prefilled
        if written and self.span:
            assert self.isz > 1
            left = self._extent(self.flat).reshape(self.nrows, self.cols) == {2: 0x7FC1, 4: NAN32, 8: NAN64}[self.isz]
            if bool(left.any()):
                i = int(left.reshape(-1).to(torch.uint8).argmax())
                raise GuardError(self.name, 'extent', i // self.cols, i % self.cols,
                                 f'output still holds the guard NaN: never written, or computed from guard memory ({int(left.sum())} elements; first')
        return self


def out(shape, device, **kw):
    return Guarded(shape, role='out', device=device, **kw)


def inp(data, device, **kw):
    """Place `data` (1-D, 2-D or 3-D) as a guarded input; returns the Guarded (its .t is the tensor to pass)."""
    data = torch.as_tensor(data)
    kw.setdefault('dtype', data.dtype)
    return Guarded(data.shape, role='in', device=device, data=data, **kw)


def check_all(bufs):
    for g in bufs:
        g.check()


def assert_close(got, ref, tol, what=''):
    """The suite's per-tensor max-norm bound, |got - ref|_max / |ref|_max < tol, computed in float64 -- but an element that is not finite, and
    otherwise the worst element, is named by its (row, column)."""
    g = torch.as_tensor(got).detach().double().cpu()
    r = torch.as_tensor(ref).detach().double().cpu()
    assert g.shape == r.shape, (what, tuple(g.shape), tuple(r.shape))
    g2 = g.reshape(-1, g.shape[-1]) if g.dim() else g.reshape(1, 1)
    r2 = r.reshape(g2.shape)
    bad = (~torch.isfinite(g2)).nonzero()
    if bad.numel():
        raise GuardError(str(what), 'value', int(bad[0, 0]), int(bad[0, 1]), f'result is not finite ({bad.shape[0]} elements; first')
    err = (g2 - r2).abs()
    e = float(err.max() / (r2.abs().max() + 1e-30)) if err.numel() else 0.0
    if not e < tol:
        i = int(err.argmax())
        raise GuardError(str(what), 'value', i // g2.shape[1], i % g2.shape[1], f'relative error {e:.3g} >= {tol:g}, worst')
    return e
