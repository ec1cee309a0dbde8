"""The f64 / f32 twin entries of the C ABI answer the same bad arguments alike: every pair below is handed the same NULL handles
and outputs, bad storage and layout tags, dimension mismatches (alone and together with a storage mismatch), short leading
dimensions and overlapping operands, and must return the same status with the same sprs_hip_last_error() text, in the same
order of checks.  The one intended difference is pinned too: a 2-byte host index array is uploaded for f64 and refused, with
its own message, for f32.

Handles cannot be made without a device, so the cases run in a child process on the emulator build of the library (tests/emu),
as the other *_emu_cpu.py tests do; every case but the accepted ones ends in the argument checks, before any device work."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
F32_WIDTH_MSG = b"index widths of an f32 matrix must be 4 or 8 bytes (2-byte host arrays are not supported for f32 handles)"
OK, DIM, STORAGE, OVERFLOW, STRUCTURE, INVALID = 0, 1, 2, 3, 4, 5


class Side:
    """one precision: its element size, its entry names and a few handles over an all-zero indptr (no stored entries)"""

    def __init__(self, lib, f32):
        import numpy as np
        self.lib, self.f32, self.e = lib, f32, 4 if f32 else 8
        self.dtype = np.float32 if f32 else np.float64
        self.zeros = self.block(4096)             # indptr of every handle below: up to 511 empty outer slices
        self.d = self.block(4096)                 # dense operands are cut from this one block
        self.csr, self.csc = self.wrap(0, 3, 4), self.wrap(1, 3, 4)
        self.sq, self.empty = self.wrap(0, 3, 3), self.wrap(0, 0, 0)
        self.big = self.wrap(0, 1 << 32, 1, idx_bytes=4)      # only ever reaches the index-type check of to_other_storage

    def name(self, kind, base):
        if kind == "csmat":
            return "sprs_hip_csmat_%s%s" % ("f32_" if self.f32 else "", base)
        return "sprs_hip_%s_%s" % (base, "f32" if self.f32 else "f64")

    def call(self, kind, base, *args):
        return getattr(self.lib, self.name(kind, base))(*args)

    def block(self, nbytes):
        p = C.c_void_p()
        assert self.lib.sprs_hip_malloc(C.byref(p), nbytes) == OK and self.lib.sprs_hip_memset(p, 0, nbytes, None) == OK
        assert self.lib.sprs_hip_synchronize(None) == OK
        return p.value

    def wrap(self, storage, rows, cols, idx_bytes=8):
        h = C.c_void_p()
        st = self.call("csmat", "wrap_device", C.byref(h), storage, rows, cols, 0, self.zeros, 8, None, idx_bytes, None)
        assert st == OK and h.value, self.lib.sprs_hip_last_error()
        return h.value

    def at(self, elements):
        return self.d + elements * self.e


def cases(s):
    """[(label, status, message, extra)] of one precision; `expect` is asserted on the spot"""
    import numpy as np
    lib, out = s.lib, []

    def rec(label, expect, kind, base, *args, extra=None):
        st = s.call(kind, base, *args)
        msg = lib.sprs_hip_last_error()
        assert st == expect, "%s %s: status %d, expected %d (%r)" % (s.name(kind, base), label, st, expect, msg)
        assert (msg == b"") == (st == OK), (s.name(kind, base), label, msg)
        out.append(("%s/%s: %s" % (kind, base, label), st, msg, extra() if extra else None))

    h, lay = C.c_void_p(), C.c_int32(7)
    ho, lo = C.byref(h), C.byref(lay)
    x, y = s.at(0), s.at(64)

    # ---- the container ----
    rec("NULL out", INVALID, "csmat", "wrap_device", None, 0, 3, 4, 0, s.zeros, 8, None, 8, None)
    rec("NULL indptr", INVALID, "csmat", "wrap_device", ho, 0, 3, 4, 0, None, 8, None, 8, None)
    rec("bad storage tag", INVALID, "csmat", "wrap_device", ho, 7, 3, 4, 0, s.zeros, 8, None, 8, None)
    rec("2-byte indptr", INVALID, "csmat", "wrap_device", ho, 0, 3, 4, 0, s.zeros, 2, None, 4, None)
    rec("3-byte indices", INVALID, "csmat", "wrap_device", ho, 0, 3, 4, 0, s.zeros, 4, None, 3, None)
    rec("NULL indices with nnz", INVALID, "csmat", "wrap_device", ho, 0, 3, 4, 2, s.zeros, 8, None, 8, s.d)
    rec("NULL data with nnz", INVALID, "csmat", "wrap_device", ho, 0, 3, 4, 2, s.zeros, 8, s.zeros, 8, None)
    rec("misaligned", INVALID, "csmat", "wrap_device", ho, 0, 3, 4, 0, s.zeros + 8, 8, None, 8, None)
    rec("NULL handle", INVALID, "csmat", "info", None, None, None, None, None, None, None)
    rec("NULL handle", INVALID, "csmat", "device_ptrs", None, None, None, None)
    rec("NULL handle", INVALID, "csmat", "download", None, None, None, None)
    rec("NULL handle", INVALID, "csmat", "transpose_view", None, ho)
    rec("NULL out", INVALID, "csmat", "transpose_view", s.csr, None)
    rec("NULL handle", INVALID, "csmat", "refresh", None)
    rec("NULL handle", INVALID, "csmat", "prepare", None, None)
    rec("NULL handle", OK, "csmat", "free", None)
    rec("NULL handle", INVALID, "csmat", "to_other_storage", None, ho)
    rec("NULL out", INVALID, "csmat", "to_other_storage", s.csr, None)
    rec("rows beyond the index type", OVERFLOW, "csmat", "to_other_storage", s.big, ho)

    def info_of(handle):
        r, c, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        pb, ib, stg = C.c_int32(), C.c_int32(), C.c_int32()
        assert s.call("csmat", "info", handle, C.byref(r), C.byref(c), C.byref(n), C.byref(pb), C.byref(ib), C.byref(stg)) == OK
        return r.value, c.value, n.value, pb.value, ib.value, stg.value
    rec("a wrapped handle", OK, "csmat", "info", s.csc, None, None, None, None, None, None, extra=lambda: info_of(s.csc))
    rec("of a CSC handle", OK, "csmat", "transpose_view", s.csc, ho, extra=lambda: info_of(h.value))
    assert out[-1][3] == (4, 3, 0, 8, 8, 0)
    rec("the view", OK, "csmat", "free", h.value)

    # ---- upload: everything but the widths ----
    vp = lambda a: C.c_void_p(a.ctypes.data)
    dt = np.ones(2, dtype=s.dtype)
    ip, down = np.array([0, 2], dtype=np.uint64), np.array([2, 0], dtype=np.uint64)
    ix, unsorted = np.array([0, 1], dtype=np.uint64), np.array([1, 0], dtype=np.uint64)
    wide = np.array([0, 5], dtype=np.uint32)
    rec("NULL out", INVALID, "csmat", "upload", None, 0, 1, 2, vp(ip), 8, vp(ix), 8, vp(dt), 1)
    rec("NULL indptr", INVALID, "csmat", "upload", ho, 0, 1, 2, None, 8, vp(ix), 8, vp(dt), 1)
    rec("bad storage tag", INVALID, "csmat", "upload", ho, 7, 1, 2, vp(ip), 8, vp(ix), 8, vp(dt), 1)
    rec("descending indptr", STRUCTURE, "csmat", "upload", ho, 0, 1, 2, vp(down), 8, vp(ix), 8, vp(dt), 1)
    rec("NULL indices with nnz", INVALID, "csmat", "upload", ho, 0, 1, 2, vp(ip), 8, None, 8, vp(dt), 1)
    rec("NULL data with nnz", INVALID, "csmat", "upload", ho, 0, 1, 2, vp(ip), 8, vp(ix), 8, None, 1)
    rec("unsorted indices", STRUCTURE, "csmat", "upload", ho, 0, 1, 2, vp(ip), 8, vp(unsorted), 8, vp(dt), 1)
    rec("index beyond inner", STRUCTURE, "csmat", "upload", ho, 1, 2, 1, vp(ip), 8, vp(wide), 4, vp(dt), 1)

    # ---- sparse times vector ----
    rec("NULL handle", INVALID, "op", "spmv", None, x, 4, y, 3, 0, None)
    rec("dimension and storage", DIM, "op", "spmv", s.csc, x, 5, y, 3, 0, None)
    rec("storage", STORAGE, "op", "spmv", s.csc, x, 4, y, 3, 0, None)
    rec("NULL x", INVALID, "op", "spmv", s.csr, None, 4, y, 3, 0, None)
    rec("NULL y", INVALID, "op", "spmv", s.csr, x, 4, None, 3, 0, None)
    rec("y inside x", INVALID, "op", "spmv", s.csr, x, 4, s.at(3), 3, 0, None)
    rec("x inside y", INVALID, "op", "spmv", s.csr, s.at(2), 4, x, 3, 0, None)
    rec("NULL handle", INVALID, "op", "mul_acc_mat_vec_csc", None, x, 4, y, 3, None)
    rec("dimension and storage", DIM, "op", "mul_acc_mat_vec_csc", s.csr, x, 4, y, 2, None)
    rec("storage", STORAGE, "op", "mul_acc_mat_vec_csc", s.csr, x, 4, y, 3, None)
    rec("NULL x", INVALID, "op", "mul_acc_mat_vec_csc", s.csc, None, 4, y, 3, None)
    rec("y inside x", INVALID, "op", "mul_acc_mat_vec_csc", s.csc, x, 4, s.at(3), 3, None)
    for tag, a in (("CSR", s.csr), ("CSC", s.csc)):
        rec(tag + " dimension", DIM, "op", "csmat_mul_vec", a, x, 3, y, 3, None)
        rec(tag + " NULL y", INVALID, "op", "csmat_mul_vec", a, x, 4, None, 3, None)
        rec(tag + " y inside x", INVALID, "op", "csmat_mul_vec", a, x, 4, s.at(3), 3, None)
    rec("NULL handle", INVALID, "op", "csmat_mul_vec", None, x, 4, y, 3, None)

    # ---- sparse times dense ----
    rec("NULL handle", INVALID, "op", "spmm_rowmaj", None, x, 4, 2, 2, y, 3, 2, 0, None)
    rec("dimension and storage", DIM, "op", "spmm_rowmaj", s.csc, x, 5, 2, 2, y, 3, 2, 0, None)
    rec("storage", STORAGE, "op", "spmm_rowmaj", s.csc, x, 4, 2, 2, y, 3, 2, 0, None)
    rec("short ld_rhs", INVALID, "op", "spmm_rowmaj", s.csr, x, 4, 3, 2, y, 3, 3, 0, None)
    rec("short ld_out", INVALID, "op", "spmm_rowmaj", s.csr, x, 4, 3, 3, y, 3, 2, 0, None)
    rec("NULL rhs", INVALID, "op", "spmm_rowmaj", s.csr, None, 4, 2, 2, y, 3, 2, 0, None)
    rec("NULL out", INVALID, "op", "spmm_rowmaj", s.csr, x, 4, 2, 2, None, 3, 2, 0, None)

    R, Cm = 0, 1                                   # layout tags
    rec("NULL handle", INVALID, "op", "csmat_mulacc_dense", None, x, 4, 2, R, 2, y, 3, R, 2, 0, None)
    rec("bad rhs layout", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, 2, 2, y, 3, R, 2, 0, None)
    rec("bad out layout", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 2, y, 3, 5, 2, 0, None)
    rec("bad layout and dimension", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 5, 2, 9, 2, y, 3, R, 2, 0, None)
    for tag, a in (("CSR", s.csr), ("CSC", s.csc)):
        rec(tag + " rhs rows", DIM, "op", "csmat_mulacc_dense", a, x, 5, 2, R, 2, y, 3, R, 2, 0, None)
        rec(tag + " out rows", DIM, "op", "csmat_mulacc_dense", a, x, 4, 2, R, 2, y, 4, R, 2, 0, None)
        rec(tag + " dimension and short ld", DIM, "op", "csmat_mulacc_dense", a, x, 5, 2, R, 1, y, 3, R, 2, 0, None)
    rec("short row-major ld_rhs", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 3, R, 2, y, 3, R, 3, 0, None)
    rec("short col-major ld_rhs", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, Cm, 3, y, 3, R, 2, 0, None)
    rec("short row-major ld_out", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 3, R, 3, y, 3, R, 2, 0, None)
    rec("short col-major ld_out", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 2, y, 3, Cm, 2, 0, None)
    rec("NULL rhs", INVALID, "op", "csmat_mulacc_dense", s.csr, None, 4, 2, R, 2, y, 3, R, 2, 0, None)
    rec("NULL out", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 2, None, 3, R, 2, 0, None)
    rec("out is rhs", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 2, x, 3, R, 2, 0, None)
    rec("out starts inside rhs", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 2, s.at(7), 3, R, 2, 0, None)
    rec("rhs starts inside out", INVALID, "op", "csmat_mulacc_dense", s.csr, s.at(5), 4, 2, R, 2, x, 3, R, 2, 0, None)
    rec("interleaved, other pitch", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 4, s.at(2), 3, R, 5, 0, None)
    rec("interleaved, other layout", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 4, s.at(2), 3, Cm, 4, 0, None)
    rec("same pitch, columns meet", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 4, s.at(1), 3, R, 4, 0, None)
    rec("same pitch, out wraps", INVALID, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 4, s.at(3), 3, R, 4, 0, None)
    rec("same pitch, out before rhs, meet", INVALID, "op", "csmat_mulacc_dense", s.csr, s.at(1), 4, 2, R, 4, x, 3, R, 4, 0, None)
    # accepted as far as the argument checks go (and, with no stored entries, all the way): rhs = buf[:, 0:2], out = buf[:, 2:4]
    rec("same pitch, disjoint columns", OK, "op", "csmat_mulacc_dense", s.csr, x, 4, 2, R, 4, s.at(2), 3, R, 4, 1, None)
    rec("same pitch, disjoint columns, out first", OK, "op", "csmat_mulacc_dense", s.csr, s.at(2), 4, 2, R, 4, x, 3, R, 4, 1, None)
    rec("same pitch, disjoint column blocks", OK, "op", "csmat_mulacc_dense", s.csc, x, 4, 2, Cm, 8, s.at(4), 3, Cm, 8, 1, None)

    val = lambda: lay.value
    rec("NULL handle", INVALID, "op", "csmat_mul_dense", None, x, 4, 2, R, 2, y, lo, None, extra=val)
    rec("NULL out_layout", INVALID, "op", "csmat_mul_dense", s.csr, x, 4, 2, R, 2, y, None, None)
    rec("bad layout", INVALID, "op", "csmat_mul_dense", s.csr, x, 4, 2, 3, 2, y, lo, None, extra=val)
    rec("dimension", DIM, "op", "csmat_mul_dense", s.csc, x, 5, 2, R, 2, y, lo, None, extra=val)
    rec("short ld", INVALID, "op", "csmat_mul_dense", s.csr, x, 4, 9, R, 8, y, lo, None, extra=val)
    rec("out is rhs", INVALID, "op", "csmat_mul_dense", s.csr, x, 4, 2, R, 2, x, lo, None, extra=val)
    lay.value = 7
    rec("NULL handle", INVALID, "op", "dense_dot_csmat", x, 2, 3, R, 3, None, y, lo, None, extra=val)
    rec("NULL out_layout", INVALID, "op", "dense_dot_csmat", x, 2, 3, R, 3, s.csr, y, None, None)
    rec("bad layout", INVALID, "op", "dense_dot_csmat", x, 2, 3, 4, 3, s.csr, y, lo, None, extra=val)
    for tag, a in (("CSC", s.csc), ("CSR", s.csr)):
        rec(tag + " dimension", DIM, "op", "dense_dot_csmat", x, 2, 4, R, 4, a, y, lo, None, extra=val)
        rec(tag + " short ld", INVALID, "op", "dense_dot_csmat", x, 2, 3, R, 2, a, y, lo, None, extra=val)
        rec(tag + " out is lhs", INVALID, "op", "dense_dot_csmat", x, 2, 3, R, 3, a, x, lo, None, extra=val)

    # ---- BiCGSTAB ----
    info = (C.c_uint8 * 64)()
    rec("NULL handle", INVALID, "op", "bicgstab", None, x, x, 3, 1e-6, 10, 0.1, y, None, None)
    rec("not square", DIM, "op", "bicgstab", s.csr, x, x, 3, 1e-6, 10, 0.1, y, None, None)
    rec("n", DIM, "op", "bicgstab", s.sq, x, x, 4, 1e-6, 10, 0.1, y, None, None)
    rec("NULL b", INVALID, "op", "bicgstab", s.sq, x, None, 3, 1e-6, 10, 0.1, y, None, None)
    rec("x is x0", INVALID, "op", "bicgstab", s.sq, x, y, 3, 1e-6, 10, 0.1, x, None, None)
    rec("x is b", INVALID, "op", "bicgstab", s.sq, x, y, 3, 1e-6, 10, 0.1, y, None, None)
    for tol, iters in ((1e-6, 10), (1e-6, 0), (0.0, 5), (-1.0, 5)):
        rec("n = 0, tol %g, %d iterations" % (tol, iters), OK, "op", "bicgstab", s.empty, x, x, 0, tol, iters, 0.1, y, info, None,
            extra=lambda: bytes(info)[:44])        # three counts, two norms and the flag; the struct's tail padding is not set
    return out


def run():
    """in the child process, on the emulator library"""
    import numpy as np
    from sprs_amd import _ffi
    lib = _ffi.lib
    d64, d32 = Side(lib, False), Side(lib, True)
    c64, c32 = cases(d64), cases(d32)
    assert len(c64) == len(c32) and len(c64) > 100
    diff = [(a, b) for a, b in zip(c64, c32) if a != b]
    assert not diff, "f64 and f32 twins answer differently:\n" + "\n".join("%r\n%r" % p for p in diff)

    # the upload widths: 2-byte host arrays are uploaded for f64 (and remembered as declared), refused for f32
    vp = lambda a: C.c_void_p(a.ctypes.data)
    ip16, ix16 = np.array([0, 1], dtype=np.uint16), np.array([0], dtype=np.uint16)
    ip32, ix64 = np.array([0, 1], dtype=np.uint32), np.array([0], dtype=np.uint64)
    for pb, ib in ((2, 2), (2, 8), (4, 2)):
        ip, ix = (ip16 if pb == 2 else ip32), (ix16 if ib == 2 else ix64)
        h = C.c_void_p()
        assert lib.sprs_hip_csmat_upload(C.byref(h), 0, 1, 1, vp(ip), pb, vp(ix), ib, vp(np.ones(1)), 1) == OK, lib.sprs_hip_last_error()
        got_pb, got_ib = C.c_int32(), C.c_int32()
        assert lib.sprs_hip_csmat_info(h, None, None, None, C.byref(got_pb), C.byref(got_ib), None) == OK
        assert (got_pb.value, got_ib.value) == (pb, ib)
        assert lib.sprs_hip_csmat_free(h) == OK
        h32 = C.c_void_p()
        assert lib.sprs_hip_csmat_f32_upload(C.byref(h32), 0, 1, 1, vp(ip), pb, vp(ix), ib, vp(np.ones(1, dtype=np.float32)), 1) == INVALID
        assert lib.sprs_hip_last_error() == F32_WIDTH_MSG and not h32.value
    # any other width is refused by both, each with its own text
    h = C.c_void_p()
    assert lib.sprs_hip_csmat_upload(C.byref(h), 0, 1, 1, vp(ip32), 3, vp(ix64), 8, vp(np.ones(1)), 1) == INVALID
    assert lib.sprs_hip_last_error() == b"index widths must be 2, 4 or 8 bytes"
    assert lib.sprs_hip_csmat_f32_upload(C.byref(h), 0, 1, 1, vp(ip32), 3, vp(ix64), 8, vp(np.ones(1, dtype=np.float32)), 1) == INVALID
    assert lib.sprs_hip_last_error() == F32_WIDTH_MSG
    # 4- and 8-byte uploads report the same widths from both
    for pre in ("", "f32_"):
        up, inf, fr = (getattr(lib, "sprs_hip_csmat_%s%s" % (pre, n)) for n in ("upload", "info", "free"))
        assert up(C.byref(h), 1, 1, 1, vp(ip32), 4, vp(ix64), 8, vp(np.ones(1, dtype=np.float32 if pre else np.float64)), 1) == OK
        got_pb, got_ib, stg = C.c_int32(), C.c_int32(), C.c_int32()
        assert inf(h, None, None, None, C.byref(got_pb), C.byref(got_ib), C.byref(stg)) == OK
        assert (got_pb.value, got_ib.value, stg.value) == (4, 8, 1) and fr(h) == OK
    print("twins agree on %d cases" % len(c64))


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ of the ROCm toolchain here")
    r = subprocess.run(["make", "-C", EMU, "-j8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(EMU, "libsprs_hip_emu.so")


def test_twin_entries_answer_bad_arguments_alike(emu_lib):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", "import test_f32_twins_emu_cpu as t; t.run()"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "twins agree on" in r.stdout
