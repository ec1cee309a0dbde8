"""Kernel LOGIC of the scan, the radix sort, the storage conversion / slicing and the triplet assembly on the CPU: the cases
of tests/test_convert_gpu.py and tests/test_triplet_gpu.py against the emulator build of the same sources (tests/emu), with
the waves of a workgroup scheduled in three orders (the workgroup sort of long rows and the scans share LDS between waves).
The emulator hands out poisoned blocks, so an element that no thread writes shows here; speed and the real memory model are the
job of the -m gpu run."""
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
def test_convert_and_triplets_under_wave_orders(emu_lib, order):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, HIPEMU_WAVE_ORDER=order)
    files = [os.path.join(ROOT, "tests", f) for f in ("test_convert_gpu.py", "test_triplet_gpu.py")]
    r = subprocess.run([sys.executable, "-m", "pytest"] + files + ["-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "1 skipped" in r.stdout, r.stdout[-1000:]    # the 2^21-triplet case skips there
