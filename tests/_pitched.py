"""Pitched buffers with guard bands, for tests of the C ABI's leading dimensions (tests/test_gpu_abi_layout.py).

A `Pitched` is ONE flat allocation that holds a `rows x width` window with pitch `ld >= width`, `guard` rows of `ld` elements in
front of it and behind it, and a base that is `off` elements past a 16-byte boundary:

    buf[start + r * ld + c],   start = round_up(guard * ld, 16) + off,   0 <= r < rows, 0 <= c < width

Every element outside the window -- guard rows, the `ld - width` elements behind each row, the `off` elements in front -- holds a
SENTINEL, a fixed quiet-NaN bit pattern (a fixed integer for integer types).  `check()` compares all of them BITWISE (as integers)
with the sentinel, so a store of NaN with another payload, of -0.0 or of the value that was there "numerically" is still seen.

Two uses:
  poisoned input   `Pitched(data=...)`: the window holds the data.  The sentinel is a NaN, so padding that is read into arithmetic
                   makes the result NaN.
  canary output    `Pitched(rows=, width=)`: the window is pre-filled with a SECOND fixed NaN pattern, so `unwritten()` tells
                   "not written" from "written".  In/out arguments (the matrix of agp_potrf_jitter, the centres of agp_kmeans) are
                   canaries that hold data.

Works on torch tensors of any device; tests/test_pitched_host.py runs it on the CPU to show that each kind of violation is caught.
"""
import numpy as np
import torch

# dtype name -> (torch dtype, integer view dtype, sentinel bits, "unwritten" bits, numpy dtype)
_TYPES = {
    "f64": (torch.float64, torch.int64, 0x7FF8DEADBEEFC0DE, 0x7FF800000BADF00D, np.float64),
    "f32": (torch.float32, torch.int32, 0x7FC5A5A5, 0x7FC00BAD, np.float32),
    "i32": (torch.int32, torch.int32, 0x7EADBEEF, 0x7BADF00D, np.int32),
    "i64": (torch.int64, torch.int64, 0x7EADBEEF7EADBEEF, 0x7BADF00D7BADF00D, np.int64),
}
VEC = {"f64": 2, "f32": 4}  # elements per 16-byte vector load (Mfma<T>::VEC in csrc/agp_device.h)


def round_up(n, q):
    return (n + q - 1) // q * q


def layouts(width, dtype):
    """The (ld, off) pairs every case runs: a pitch that breaks ld % VEC, one that keeps it with padding, one far off the 64-grid
    of the library's internal tiles; each with an aligned base and a base one element past alignment."""
    v = VEC[dtype]
    return [(ld, off) for ld in (width + 1, width + v, round_up(width, 64) + 64) for off in (0, 1)]


class Pitched:
    def __init__(self, dtype, data=None, rows=None, width=None, ld=None, off=0, guard=2, device="cpu"):
        self.tdtype, self.idtype, self.sentinel, self.fresh, self.npdtype = _TYPES[dtype]
        if data is not None:
            data = np.asarray(data)
            if data.ndim == 1:
                data = data[None, :]
            rows, width = data.shape
        assert rows >= 1 and width >= 1
        ld = width if ld is None else ld
        assert ld >= width and off >= 0 and guard >= 0
        self.dtype, self.rows, self.width, self.ld, self.off, self.guard = dtype, rows, width, ld, off, guard
        self.start = round_up(guard * ld, 16) + off
        self.total = self.start + rows * ld + guard * ld
        self.ibuf = torch.empty(self.total, dtype=self.idtype, device=device)
        assert self.ibuf.data_ptr() % 16 == 0
        self.ibuf.fill_(self.sentinel)
        self.buf = self.ibuf.view(self.tdtype)  # the same memory in the element type
        self.itemsize = self.buf.element_size()
        self.ptr = self.buf.data_ptr() + self.start * self.itemsize  # what the C ABI is handed, together with self.ld
        if data is None:
            self._iwindow().fill_(self.fresh)
        else:
            self._window().copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=self.npdtype)))

    def _window(self):
        return self.buf.as_strided((self.rows, self.width), (self.ld, 1), self.start)

    def _iwindow(self):
        return self.ibuf.as_strided((self.rows, self.width), (self.ld, 1), self.start)

    def window(self):
        """The rows x width window as a NumPy array (a copy)."""
        return self._window().cpu().numpy().copy()

    def bits(self):
        """The window's bit patterns as integers: what 'bitwise equal' compares."""
        return self._iwindow().cpu().numpy().copy()

    def unwritten(self):
        """Boolean rows x width array: True where a canary window still holds its pre-fill."""
        return self.bits() == np.array(self.fresh).astype(self.bits().dtype)

    def violations(self):
        """Flat indices (into the allocation) of the elements outside the window that no longer hold the sentinel."""
        bad = self.ibuf != self.sentinel
        bad.as_strided((self.rows, self.width), (self.ld, 1), self.start).fill_(False)
        return torch.nonzero(bad).flatten().cpu().numpy()

    def describe(self, flat):
        """Where a flat index lies relative to the window: (row, column), rows < 0 / >= rows and columns >= width are padding."""
        rel = int(flat) - self.start
        return rel // self.ld, rel % self.ld

    def check(self, what="buffer"):
        bad = self.violations()
        if len(bad):
            where = ", ".join("(row %d, col %d)" % self.describe(b) for b in bad[:8])
            raise AssertionError(
                "%s: %d element(s) outside the %d x %d window (ld %d, off %d) were written; first at %s"
                % (what, len(bad), self.rows, self.width, self.ld, self.off, where))
        return True
