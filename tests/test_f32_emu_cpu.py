"""Kernel LOGIC of the single-precision path on the CPU: tests/test_f32_gpu.py against the emulator build of the same sources
(tests/emu), with the waves of a workgroup scheduled in three orders.  The f32 tile kernel and its carry pass, the casts, the
position gather behind to_other_storage and the templated BiCGSTAB run as shipped; speed and the real memory model are the job
of the -m gpu run.

Deselected here, and only this one:
  test_spmv_on_a_capturing_stream_needs_the_plan   stream capture is a feature of the HIP runtime; the emulator has no graphs
(the 10^6-entry random case takes about two seconds per wave order and stays in).  Everything else must pass, with no skips."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DESELECT = "not test_spmv_on_a_capturing_stream_needs_the_plan"


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ of the ROCm toolchain here")
    r = subprocess.run(["make", "-C", EMU, "-j8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(EMU, "libsprs_hip_emu.so")


@pytest.mark.parametrize("order", ["default", "reverse", "rotate"])
def test_f32_under_wave_orders(emu_lib, order):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, HIPEMU_WAVE_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_f32_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-k", DESELECT, "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
    assert "1 deselected" in r.stdout, r.stdout[-1000:]
