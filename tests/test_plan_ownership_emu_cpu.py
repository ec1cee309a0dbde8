"""Who owns the device arrays a handle derives from its own — the SpMV plans (tile, XCD-sliced, banded), the SpMM plan, the
Gauss-Seidel and triangular-solve row orders, the sparse-vector scratch, the per-stream scratch, the vectors of
sprs_hip_spmv_f64_host — on the CPU, through the kernel emulator of tests/emu: every block, stream and event the library takes
is counted there, and its hipMalloc can be told to fail at the n-th call.  One case per owner (tests/plan_ownership_cases.py,
run as a subprocess on the emulator build of the shipped sources): nothing is left behind on the clean path, and nothing after
ANY of the N allocations of the sequence failed — which ends in OUT_OF_MEMORY with a message or in a documented fall-back, and
after which the same handle computes the right result.  A case that injects fewer than N failures fails."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CASES = ["tile", "sliced", "banded", "spmm_stream", "spmm_chunks", "spmm_relaid", "gauss_seidel", "upper_solve", "csmat_csvec", "spmv_host"]


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ of the ROCm toolchain here")
    r = subprocess.run(["make", "-C", EMU, "-j8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return os.path.join(EMU, "libsprs_hip_emu.so")


@pytest.mark.parametrize("case", CASES)
def test_no_block_is_left_behind(emu_lib, case):
    env = dict(os.environ, SPRS_HIP_LIBRARY=emu_lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plan_ownership_cases.py"), case], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["case"] == case and out["mallocs"] >= 5                   # (upload: three arrays; operands; at least one derived block)
    assert out["injections"] == out["mallocs"] == out["oom"] + out["fallback"]
    # the only fall-back these cases can reach: the re-laid-out rhs copy that does not fit (once: the copy is made once)
    assert out["fallback"] == (1 if case == "spmm_relaid" else 0)
