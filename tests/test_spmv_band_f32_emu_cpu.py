"""The banded SpMV plan of f32 handles on the CPU: the plan build with float values and every f32 kernel of the plan (hot slices of
8192, 16384 and 32768 labels, cold pieces, short rows, carries, the permutation of x, the reduction and the fused tail) compiled
for the host and run by the fiber emulator of tests/emu, on the cases of tests/test_spmv_band_f32_gpu.py — all of them but the
million-entry rounded one, which the device run covers.  Test infrastructure: the emulator says nothing about speed; the same
cases run on the device under -m gpu."""
import os
import re
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


def test_f32_banded_plan_in_the_emulator(emu_lib):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_spmv_band_f32_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and " failed" not in r.stdout
    # the one case the emulator leaves to the device: a million entries
    skipped = re.search(r"(\d+) skipped", r.stdout)
    assert skipped and int(skipped.group(1)) == 1, r.stdout[-500:]
