"""Kernel LOGIC of the f32 SpGEMM on the CPU: tests/test_spgemm_f32_gpu.py against the emulator build of the same sources
(tests/emu), with the waves of a workgroup scheduled in three orders.  The numeric kernels instantiated for float — lane
groups, hash tables, wave per row, workgroup with its token hand-over — the 8-byte records of B, the f32 probe of the LDS add and
the three forms of the add run as shipped; the emulator's guard page behind every allocation turns a read past a buffer (a
record loaded across the end of bpack, an accumulator past ACC_CAP floats) into a fault.  Speed and the real LDS are the job of
the -m gpu run.

Deselected here, and only these:
  test_kept_plan_in_place_values_and_both_precisions_torch_tensors   torch CUDA tensors need a device
  test_iptr_overflow_u32                                              4.9e9 products through the counting kernels: the check it
                                                                      is about sits behind a walk only a device finishes
The kept-plan and determinism cases run on smaller R-MAT matrices under the emulator (gated on SPRS_HIP_LIBRARY in the test
file), with the same assertions.  Everything else must pass, with no skips."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
DESELECT = "not torch_tensors and not test_iptr_overflow_u32"


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ of the ROCm toolchain here")
    r = subprocess.run(["make", "-C", EMU, "-j8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(EMU, "libsprs_hip_emu.so")


@pytest.mark.parametrize("order", ["default", "reverse", "rotate"])
def test_spgemm_f32_under_wave_orders(emu_lib, order):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, HIPEMU_WAVE_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_spgemm_f32_gpu.py"), "-x", "-q", "-m", "gpu",
                        "-k", DESELECT, "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]
    assert "2 deselected" in r.stdout, r.stdout[-1000:]
