"""The packed hot slices of the banded SpMV plan on the CPU: the plan build (keys per tile, verdict per slice, records) and both
instantiations of the hot kernel compiled for the host and run by the fiber emulator of tests/emu, on the cases of
tests/test_spmv_band_pack_gpu.py — values of one magnitude class, a slice kept raw by a tile with three keys, slices of 1, 511,
512, 513 and 1025 entries, hub rows over many segments, keys that differ in sign only, zeros, denormals, infinities and NaNs with payload, the accumulate and
the overwrite form, every index width, values updated in place, and the generator's own values, which must leave no hot slice
raw.  Everywhere y under spmv_band_pack = 1 equals y under = 2 bit for bit.  Test infrastructure: the emulator says nothing about
speed; the same cases run on the device under -m gpu."""
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


def test_packed_hot_slices_in_the_emulator(emu_lib):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_spmv_band_pack_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and " failed" not in r.stdout and " skipped" not in r.stdout

