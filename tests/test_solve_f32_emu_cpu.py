"""Kernel LOGIC of the f32 triangular solves and the f32 Gauss-Seidel on the CPU: tests/test_trisolve_f32_gpu.py and
tests/test_gauss_seidel_f32_gpu.py against the emulator build of the same sources (tests/emu), with the waves of a workgroup
scheduled in three orders.  The float instantiations of tri_solve_kernel and gs_sweep_kernel, the 4-byte hand-off word with
its pending / quiet-NaN substitution, the f32 residual and the singular report run as shipped; speed and the real memory model
are the job of the -m gpu run."""
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


def _run(emu_lib, order, name):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib, HIPEMU_WAVE_ORDER=order)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", name), "-x", "-q", "-m", "gpu",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-1000:]
    return r.stdout


@pytest.mark.parametrize("order", ["default", "reverse", "rotate"])
def test_f32_triangular_solves_under_wave_orders(emu_lib, order):
    """the redraw cases need a real device and skip"""
    assert "skipped" in _run(emu_lib, order, "test_trisolve_f32_gpu.py")


@pytest.mark.parametrize("order", ["default", "reverse", "rotate"])
def test_f32_gauss_seidel_under_wave_orders(emu_lib, order):
    _run(emu_lib, order, "test_gauss_seidel_f32_gpu.py")
