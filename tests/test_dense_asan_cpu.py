"""The host side of the dense <-> sparse entries under AddressSanitizer and UBSan: tests/cpp/dense_args_asan.cpp is a stand-alone
program (its own main, the library's sources compiled for the host) that drives every argument check of the new entries; it is
built and run here as a child process.  No device, nothing loaded into this interpreter."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_argument_checks_under_sanitizers():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ of the ROCm toolchain here")
    r = subprocess.run(["make", "-C", CPP, "-f", "dense_args_asan.mk", "-j8", "dense_args_asan.bin"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([os.path.join(CPP, "dense_args_asan.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dense_args_asan: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
