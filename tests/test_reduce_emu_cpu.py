"""Kernel LOGIC of the sparse-vector reductions on the CPU: tests/test_reduce_gpu.py against the emulator build of the same
sources (tests/emu), with the waves of a workgroup scheduled in three orders.  The grid stage (terms and presence masks), the
one-wave chain with its chunks in flight, the order-free reductions, the divide and the look-ups run as shipped; speed, the
device's pow and the real memory model are the job of the -m gpu run."""
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
def test_reductions_under_wave_orders(emu_lib, order):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, HIPEMU_WAVE_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_reduce_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "1 skipped" in r.stdout, r.stdout[-1000:]    # the torch stream case skips there
