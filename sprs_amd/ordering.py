"""Twin of `sprs::sparse::linalg::ordering` (sprs/src/sparse/linalg/ordering.rs) and `sprs::sparse::symmetric::is_symmetric`
for device operands, under the reference's names: `reverse_cuthill_mckee(a)`, `cuthill_mckee_custom(a, start.X, order.Y)` with
`start.Next / MinimumDegree / PseudoPeripheral` and `order.Forward / Reversed`, `Ordering` with `.perm` and `.connected_parts`.

The matrix stays in HBM and so does the permutation: `Ordering.perm` is a DevicePerm, ready for `transform_mat_papt`.  The
permutation is the reference's with ties between vertices of equal degree broken by vertex id (the stable outcome of its
sort_unstable_by_key): one deterministic result.  Where the reference panics, SprsHipError carries the text."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import check, lib
from .device import _stream_arg
from .permutation import DevicePerm


class start:
    """Starting-vertex strategies (ordering.rs:14-267)."""

    class Next:
        code = _ffi.START_NEXT

    class MinimumDegree:
        code = _ffi.START_MINIMUM_DEGREE

    class PseudoPeripheral:
        code = _ffi.START_PSEUDO_PERIPHERAL

        @classmethod
        def new(cls):
            return cls()


class order:
    """Directions (ordering.rs:269-420)."""

    class Forward:
        reversed = 0

        @classmethod
        def new(cls):
            return cls()

    class Reversed:
        reversed = 1

        @classmethod
        def new(cls):
            return cls()


class Ordering:
    """ordering.rs:7-12: `perm` (a DevicePerm in the matrix's index type) and `connected_parts` (host uint64: indices inside
    the permutation delimiting the connected components).  `stats`: components, levels of the ordering pass, launches (a sort
    or a scan counts as one) and host read-backs of the call that made it."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        dim, n_parts, stats = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 4)()
        check(lib.sprs_hip_ordering_info(self._h, C.byref(dim), C.byref(n_parts), stats))
        self.dim = dim.value
        self.stats = dict(zip(("components", "levels", "launches", "readbacks"), (int(x) for x in stats)))
        parts = np.zeros(n_parts.value, dtype=np.uint64)
        check(lib.sprs_hip_ordering_parts(self._h, C.c_void_p(parts.ctypes.data)))
        self.connected_parts = parts
        h = C.c_void_p()
        check(lib.sprs_hip_ordering_perm(self._h, C.byref(h)))
        self.perm = DevicePerm._wrap(h.value)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.sprs_hip_ordering_free(h)
            self._h = C.c_void_p(0)


def _code(x, attr):
    return getattr(x, attr) if hasattr(x, attr) else int(x)


def cuthill_mckee_custom(mat, starting_strategy, directed_ordering, check_symmetric=False, stream=None):
    """ordering.rs:440-526.  A non-square matrix fails with the text of the reference's assert_eq!; check_symmetric=True is its
    debug_assert!(is_symmetric(&mat)): BAD_STRUCTURE "matrix is not symmetric"."""
    h = C.c_void_p()
    check(lib.sprs_hip_csmat_cuthill_mckee(mat._h, _code(starting_strategy, "code"), _code(directed_ordering, "reversed"),
                                           1 if check_symmetric else 0, C.byref(h), _stream_arg(stream)))
    return Ordering(h.value)


def reverse_cuthill_mckee(mat, check_symmetric=False, stream=None):
    """ordering.rs:546-559: cuthill_mckee_custom(mat, start::PseudoPeripheral::new(), order::Reversed::new())."""
    return cuthill_mckee_custom(mat, start.PseudoPeripheral, order.Reversed, check_symmetric, stream)


def is_symmetric(mat, stream=None):
    """symmetric.rs:7-34: square, every entry mirrored, values equal under f64 `!=` (a NaN anywhere: False)."""
    flag = C.c_int32()
    check(lib.sprs_hip_csmat_is_symmetric(mat._h, C.byref(flag), _stream_arg(stream)))
    return bool(flag.value)
