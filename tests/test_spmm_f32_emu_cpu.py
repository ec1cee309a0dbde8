"""Kernel LOGIC of the f32 SpMM on the CPU: tests/test_spmm_f32_gpu.py against the emulator build of the same sources
(tests/emu), with the waves of a workgroup scheduled in three orders.  Both lane forms of the f32 entry-stream kernel, its
fix-up and re-layout copy, and the row-walking kernels instantiated for float run as shipped; the emulator's guard page behind
every allocation turns a read past a caller's buffer (the other column of an odd k's last lane) into a fault.  Speed and the
real memory model are the job of the -m gpu run.

Deselected here, and only these two cases of one test:
  test_plan_built_on_a_nonblocking_stream[1], [0]   a torch.cuda.Stream needs a device; the emulator's streams are all one queue
The rounded cases run on smaller matrices under the emulator (gated on SPRS_HIP_LIBRARY in the test file: R-MAT 3000 x 16
instead of 60000 x 16, 10 ragged rows instead of 42), with the same bounds.  Everything else must pass, with no skips."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DESELECT = "not test_plan_built_on_a_nonblocking_stream"


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ of the ROCm toolchain here")
    r = subprocess.run(["make", "-C", EMU, "-j8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(EMU, "libsprs_hip_emu.so")


@pytest.mark.parametrize("order", ["default", "reverse", "rotate"])
def test_spmm_f32_under_wave_orders(emu_lib, order):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, HIPEMU_WAVE_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_spmm_f32_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-k", DESELECT, "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
    assert "2 deselected" in r.stdout, r.stdout[-1000:]
