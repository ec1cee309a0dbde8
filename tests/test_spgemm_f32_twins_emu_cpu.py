"""The f64 / f32 twin entries of SpGEMM answer the same bad arguments alike: each of the eight pairs (the product, symbolic,
numeric, plan_create, plan_structure, plan_product, plan_numeric, csmat_mul_csmat) is handed the same NULL handles and outputs,
dimension mismatches (alone and together with a storage mismatch), storage mismatches, operands and targets of other index
types, plans made for other operands, and must return the same status with the same sprs_hip_last_error() text, in the same
order of checks.  The accepted cases (empty matrices, all four storage pairs of `&lhs * &rhs`) must report the same results.

After the pattern of tests/test_f32_twins_emu_cpu.py, whose Side (one precision's entry names and a few empty handles) is
reused: the cases run in a child process on the emulator build of the library."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from test_f32_twins_emu_cpu import DIM, INVALID, OK, STORAGE, STRUCTURE, Side

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def entry(s, base):
    """sprs_hip_spgemm_f64 / sprs_hip_spgemm_f32; every other entry: the f64 name, with _f32 appended for f32"""
    if base == "spgemm":
        return getattr(s.lib, "sprs_hip_spgemm_f32" if s.f32 else "sprs_hip_spgemm_f64")
    return getattr(s.lib, "sprs_hip_%s%s" % (base, "_f32" if s.f32 else ""))


def cases(s):
    """[(label, status, message, extra)] of one precision; `expect` is asserted on the spot"""
    lib, out = s.lib, []

    def rec(label, expect, base, *args, extra=None):
        st = entry(s, base)(*args)
        msg = lib.sprs_hip_last_error()
        assert st == expect, "%s %s: status %d, expected %d (%r)" % (base, label, st, expect, msg)
        assert (msg == b"") == (st == OK), (base, label, msg)
        out.append(("%s: %s" % (base, label), st, msg, extra() if extra else None))

    def info_of(handle):
        r, c, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
        pb, ib, stg = C.c_int32(), C.c_int32(), C.c_int32()
        assert s.call("csmat", "info", handle, C.byref(r), C.byref(c), C.byref(n), C.byref(pb), C.byref(ib), C.byref(stg)) == OK
        return r.value, c.value, n.value, pb.value, ib.value, stg.value

    h, plan = C.c_void_p(), C.c_void_p()
    ho, po = C.byref(h), C.byref(plan)
    a34, b43, b43_csc, a34_csc = s.csr, s.wrap(0, 4, 3), s.wrap(1, 4, 3), s.csc       # 3 x 4 and 4 x 3, empty
    sq, sq_idx4 = s.sq, s.wrap(0, 3, 3, idx_bytes=4)
    sq_csc, c33_csc, c34 = s.wrap(1, 3, 3), s.wrap(1, 3, 3), s.wrap(0, 3, 4)

    for base in ("spgemm", "spgemm_symbolic", "csmat_mul_csmat"):
        rec("NULL a", INVALID, base, None, b43, ho)
        rec("NULL b", INVALID, base, a34, None, ho)
        rec("NULL out", INVALID, base, a34, b43, None)
        rec("dimension", DIM, base, a34, a34, ho)
        rec("dimension and storage", DIM, base, a34_csc, a34, ho)
        rec("index types", STORAGE, base, sq, sq_idx4, ho)
        rec("accepted", OK, base, a34, b43, ho, extra=lambda: info_of(h.value))
        assert out[-1][3] == (3, 3, 0, 8, 8, 0)
        assert s.call("csmat", "free", h.value) == OK
    for base in ("spgemm", "spgemm_symbolic"):
        rec("rhs CSC", STORAGE, base, a34, b43_csc, ho)
        rec("lhs CSC", STORAGE, base, sq_csc, sq, ho)
    for tag, lhs, rhs, storage in (("CSR x CSC", a34, b43_csc, 0), ("CSC x CSR", a34_csc, b43, 1), ("CSC x CSC", a34_csc, b43_csc, 1)):
        rec(tag, OK, "csmat_mul_csmat", lhs, rhs, ho, extra=lambda: info_of(h.value))
        assert out[-1][3] == (3, 3, 0, 8, 8, storage)
        assert s.call("csmat", "free", h.value) == OK

    # ---- numeric into an existing c ----
    rec("NULL a", INVALID, "spgemm_numeric", None, sq, sq)
    rec("NULL c", INVALID, "spgemm_numeric", sq, sq, None)
    rec("dimension", DIM, "spgemm_numeric", a34, a34, sq)
    rec("storage of b", STORAGE, "spgemm_numeric", sq, sq_csc, sq)
    rec("c of another shape", DIM, "spgemm_numeric", sq, sq, c34)
    rec("c CSC", STORAGE, "spgemm_numeric", sq, sq, c33_csc)
    rec("c of other index types", STORAGE, "spgemm_numeric", sq, sq, sq_idx4)
    c33 = s.wrap(0, 3, 3)
    rec("accepted", OK, "spgemm_numeric", sq, sq, c33)

    # ---- the kept plan ----
    rec("NULL a", INVALID, "spgemm_plan_create", None, sq, po)
    rec("NULL out", INVALID, "spgemm_plan_create", sq, sq, None)
    rec("dimension", DIM, "spgemm_plan_create", a34, a34, po)
    rec("storage", STORAGE, "spgemm_plan_create", sq, sq_csc, po)
    rec("index types", STORAGE, "spgemm_plan_create", sq, sq_idx4, po)
    assert not plan.value
    for base in ("spgemm_plan_structure", "spgemm_plan_product"):
        rec("NULL plan", INVALID, base, None, sq, sq, ho)
    rec("NULL plan", INVALID, "spgemm_plan_numeric", None, sq, sq, c33)
    rec("accepted", OK, "spgemm_plan_create", sq, sq, po)
    assert plan.value
    nnz = C.c_uint64(7)
    assert lib.sprs_hip_spgemm_plan_nnz(plan, C.byref(nnz)) == OK and nnz.value == 0         # (one entry for both precisions)
    for base in ("spgemm_plan_structure", "spgemm_plan_product"):
        rec("NULL a", INVALID, base, plan, None, sq, ho)
        rec("NULL out", INVALID, base, plan, sq, sq, None)
        rec("other operands", INVALID, base, plan, a34, b43, ho)
        rec("other index types", INVALID, base, plan, sq_idx4, sq_idx4, ho)
        rec("accepted", OK, base, plan, sq, sq, ho, extra=lambda: info_of(h.value))
        assert out[-1][3] == (3, 3, 0, 8, 8, 0)
        assert s.call("csmat", "free", h.value) == OK
    rec("NULL c", INVALID, "spgemm_plan_numeric", plan, sq, sq, None)
    rec("c of another shape", DIM, "spgemm_plan_numeric", plan, sq, sq, c34)
    rec("c CSC", STORAGE, "spgemm_plan_numeric", plan, sq, sq, c33_csc)
    rec("c of other index types", STORAGE, "spgemm_plan_numeric", plan, sq, sq, sq_idx4)
    rec("other operands", INVALID, "spgemm_plan_numeric", plan, a34, b43, c33)
    rec("accepted", OK, "spgemm_plan_numeric", plan, sq, sq, c33)
    assert lib.sprs_hip_spgemm_plan_free(plan) == OK
    return out


def run(only_f64=False):
    """in the child process, on the emulator library"""
    from sprs_amd import _ffi
    lib = _ffi.lib
    c64 = cases(Side(lib, False))
    assert len(c64) > 60
    if only_f64:
        print("f64 half: %d cases" % len(c64))
        return
    c32 = cases(Side(lib, True))
    assert len(c64) == len(c32)
    diff = [(a, b) for a, b in zip(c64, c32) if a != b]
    assert not diff, "f64 and f32 twins answer differently:\n" + "\n".join("%r\n%r" % p for p in diff)
    assert STRUCTURE == 4          # (BAD_STRUCTURE is reached only behind device work: tests/test_spgemm_f32_gpu.py)
    print("twins agree on %d cases" % len(c64))


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ of the ROCm toolchain here")
    r = subprocess.run(["make", "-C", EMU, "-j8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(EMU, "libsprs_hip_emu.so")


def test_spgemm_twin_entries_answer_bad_arguments_alike(emu_lib):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", "import test_spgemm_f32_twins_emu_cpu as t; t.run()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "twins agree on" in r.stdout
