"""Kernel LOGIC of the structure checks and of new_from_unsorted on the CPU: tests/test_structure_gpu.py against the emulator
build of the same sources (tests/emu), with the waves of a workgroup scheduled in three orders.  The indptr pass, the tiles of the
check, the flag pass, the masked length classes (lane groups, the LDS sorts, the hub route through the radix sort) and the
vector routes run as shipped; every device block of the emulator ends at a guard page, so a read past an array is a crash, not a
wrong number.  Speed and the real memory model are the job of the -m gpu run."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ of the ROCm toolchain here")
    r = subprocess.run(["make", "-C", EMU, "-j8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(EMU, "libsprs_hip_emu.so")


@pytest.mark.parametrize("order", ["default", "reverse", "rotate"])
def test_structure_under_wave_orders(emu_lib, order):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, HIPEMU_WAVE_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_structure_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "skipped" in r.stdout, r.stdout[-1000:]    # the torch cases skip there


# An indptr that points far outside the arrays.  The emulator's "device" memory is host memory: the case runs in a child process
# that binds the emulator library directly, and a kernel that followed the indptr into `indices` would end it with a signal.
_FAR_INDPTR = r"""
import ctypes as C, sys
import numpy as np
lib = C.CDLL(sys.argv[1])
lib.sprs_hip_last_error.restype = C.c_char_p
BAD_STRUCTURE = 4

def dev(arr):
    p = C.c_void_p()
    assert lib.sprs_hip_malloc(C.byref(p), C.c_uint64(max(arr.nbytes, 8))) == 0
    assert lib.sprs_hip_memcpy_h2d(p, C.c_void_p(arr.ctypes.data), C.c_uint64(arr.nbytes)) == 0
    return p

class Info(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("outer", C.c_uint64)]

def run(indptr, nnz, indices, data, sort):
    ip = dev(np.array(indptr, dtype=np.uint64))
    h, out, info = C.c_void_p(), C.c_void_p(), Info()
    st = lib.sprs_hip_csmat_wrap_device(C.byref(h), 0, C.c_uint64(len(indptr) - 1), C.c_uint64(8), C.c_uint64(nnz), ip, 8, indices, 8, data)
    assert st == 0, lib.sprs_hip_last_error()
    if sort:
        st = lib.sprs_hip_csmat_from_unsorted(h, C.byref(out), C.byref(info), None)
        assert bool(out.value) == (st == 0)          # no handle on any finding
    else:
        st = lib.sprs_hip_csmat_check_structure(h, C.byref(info), None)
    return st, lib.sprs_hip_last_error().decode(), info.kind, info.outer

ix, dt = dev(np.array([0, 1, 2], dtype=np.uint64)), dev(np.ones(3))
NO = (1 << 64) - 1
for sort in (False, True):
    # nnz = 3: a value of 10^12 in the middle, then at the end
    assert run([0, 1, 10**12, 3], 3, ix, dt, sort) == (BAD_STRUCTURE, "Unsorted indptr", 1, NO)
    assert run([0, 1, 2, 10**12], 3, ix, dt, sort) == (BAD_STRUCTURE, "Indices length and inpdtr's nnz do not match", 2, NO)
    assert run([0, 10**12, 10**12, 10**12 + 1], 3, ix, dt, sort) == (BAD_STRUCTURE, "Indices length and inpdtr's nnz do not match", 2, NO)
    # `indices` is never read before the indptr pass came back clean: a handle of nnz 0 without any indices array
    assert run([0, 10**12, 0], 0, None, None, sort) == (BAD_STRUCTURE, "Unsorted indptr", 1, NO)
    assert run([0, 5, 10**12], 0, None, None, sort) == (BAD_STRUCTURE, "Indices length and inpdtr's nnz do not match", 2, NO)
    assert run([0, 0, 0], 0, None, None, sort)[0] == 0
print("far-indptr cases passed")
"""


def test_indptr_far_beyond_nnz_never_reaches_the_indices(emu_lib, tmp_path):
    script = tmp_path / "far_indptr.py"
    script.write_text(_FAR_INDPTR)
    r = subprocess.run([sys.executable, str(script), emu_lib], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "far-indptr cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
