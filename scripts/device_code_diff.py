#!/usr/bin/env python3
"""Is the device code of two source trees the same, kernel by kernel?  A refactor of the host side must not move it.
Every translation unit of sprs_amd/csrc is compiled for the device only (the Makefile's flags + --cuda-device-only -S;
spgemm.hip also with -DSPRS_HIP_DEVTOOLS), the assembly is split per function symbol, and symbol sets, bodies and the
.amdhsa_* resource lines are compared.  Emission order may differ (local labels carry the function's number), tree B may hold
functions A does not have, and a template parameter that is `double` for the f64 code may have been added (see canonical()):
nothing else.
usage: device_code_diff.py <tree A> <tree B> [work dir]      exit status 1 when anything differs"""
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fPIC -Wall -Wno-unused-result --cuda-device-only -S".split()
UNITS = "abi spmv spmv_band spgemm scan convert spmm bicgstab gauss_seidel sort triplet dist".split()


def assembly(tree, work):
    out = {}
    procs = []
    for u in UNITS + ["spgemm:dev"]:
        name, dev = (u.split(":") + [""])[:2]
        dst = os.path.join(work, u.replace(":", "_") + ".s")
        cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + (["-DSPRS_HIP_DEVTOOLS"] if dev else []) + [name + ".hip", "-o", dst]
        procs.append((u, dst, subprocess.Popen(cmd, cwd=os.path.join(tree, "sprs_amd", "csrc"), stderr=subprocess.DEVNULL)))
    for u, dst, p in procs:
        if p.wait() != 0:
            sys.exit("compile failed: %s in %s" % (u, tree))
        out[u] = open(dst).read()
    return out


def split(text):
    bodies, resources = {}, {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", m.group(2))
        body = re.sub(r"\.L(tmp|func_begin|func_end)\d+", r".L\1", body)
        bodies[m.group(1)] = "\n".join(re.sub(r"\s*;.*$", "", l).rstrip() for l in body.splitlines()
                                       if not l.lstrip().startswith((";", ".loc", ".file", ".cfi")))
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M):
        resources[m.group(1)] = m.group(2)
    return bodies, resources


import shutil

CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")


def canonical(text):
    """Kernel templates may gain a defaulted or trailing scalar parameter (the SpGEMM kernels: `typename T`, double for the f64
    code) without their f64 bodies moving; the mangled names change all the same.  Every mangled symbol of the text is replaced
    by its demangled form with that parameter dropped where it is `double`: CsrView<I, P, double> -> CsrView<I, P> and a last
    template argument `, double>` of a function template.  Symbols instantiated for another scalar keep their own names and show up
    as added functions."""
    syms = sorted(set(re.findall(r"\b_Z[A-Za-z0-9_$.]+", text)), key=len, reverse=True)
    if not syms:
        return text
    dem = subprocess.run([CXXFILT], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.splitlines()
    names = {}
    for m, d in zip(syms, dem):
        d = re.sub(r"(CsrView<[^<>]*?), double>", r"\1>", d)
        d = re.sub(r", double>\(", ">(", d)
        names[m] = re.sub(r"[^A-Za-z0-9_]", "_", d)
    return re.sub(r"\b_Z[A-Za-z0-9_$.]+", lambda m: names[m.group(0)], text)


def main():
    a, b = sys.argv[1], sys.argv[2]
    work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp()
    os.makedirs(os.path.join(work, "a"), exist_ok=True)
    os.makedirs(os.path.join(work, "b"), exist_ok=True)
    asm_a, asm_b = assembly(a, os.path.join(work, "a")), assembly(b, os.path.join(work, "b"))
    same = True
    for u in asm_a:
        (ba, ra), (bb, rb) = split(canonical(asm_a[u])), split(canonical(asm_b[u]))
        # functions only tree B has (new instantiations) are reported, not counted as a difference: everything A has must be in B, unchanged
        added = sorted(set(bb) - set(ba))
        bad = sorted(set(ba) - set(bb)) + sorted(set(ra) - set(rb)) + [k for k in ba if k in bb and ba[k] != bb[k]] + \
            [k for k in ra if k in rb and ra[k] != rb[k]]
        same &= not bad
        print("%-14s functions %4d / %4d   kernels %4d / %4d   %s%s" % (u, len(ba), len(bb), len(ra), len(rb),
                                                                       "identical" if not bad else "DIFFERENT: " + ", ".join(bad[:4]),
                                                                       "   (+%d functions only in B)" % len(added) if added else ""))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
