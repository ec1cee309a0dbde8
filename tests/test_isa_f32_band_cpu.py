"""Guards of the compiler-level facts the f32 kernels of the banded SpMV plan depend on (hipcc cross-compiles without a GPU), the
twins of the f64 guard in tests/test_isa_cpu.py:

* the f32 hot kernel (band_hot_kernel_f32, slices of 16384 and 32768 labels) stays within 96 VGPRs without scratch — the budget that
  lets two 64-register gather waves sit beside each hot wave;
* gfx950 counts loads and stores on one in-order vmcnt: between the first non-temporal store of the deferred flush and the next
  tile's non-temporal loads no `s_waitcnt vmcnt(0)` may drain the stores with nothing in flight;
* a tile is requested as two 16-byte value loads and one 16-byte id load per lane, all non-temporal (8 floats + 8 ids);
* the f32 gather kernels (cold pieces, short rows) stay within 64 VGPRs: the gathers live on the number of waves in flight.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def band_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "spmv_band.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "--cuda-device-only", "-S",
                           os.path.join(ROOT, "sprs_amd", "csrc", "spmv_band.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = {}
    for m in re.finditer(r"^(_ZN8sprs_hip\S+):\s*; @\S+\n(.*?)^\s*s_endpgm", text, flags=re.S | re.M):
        kernels[m.group(1)] = m.group(2)
    return kernels, text


def resources(text, name):
    m = re.search(r"; NumVgprs: (\d+).*?; ScratchSize: (\d+)", text[text.index(name + ":"):], flags=re.S)
    assert m, name
    return int(m.group(1)), int(m.group(2))


def pick(kernels, part):
    names = [k for k in kernels if part in k]
    assert names, part
    return names


@pytest.mark.parametrize("width", [14, 15])
def test_f32_hot_kernel(band_isa, width):
    kernels, text = band_isa
    names = pick(kernels, "band_hot_kernel_f32ILi%dE" % width)
    assert len(names) == 1
    name = names[0]
    vgpr, scratch = resources(text, name)
    assert scratch == 0 and vgpr <= 96, (name, vgpr, scratch)
    lines = [ln.strip() for ln in kernels[name].splitlines()]

    def nt(i, prefix):
        return lines[i].startswith(prefix) and lines[i].endswith(" nt")

    stores = [i for i in range(len(lines)) if nt(i, "global_store_dword ")]          # the sums are floats: 4-byte stores
    loads = [i for i in range(len(lines)) if nt(i, "global_load_dwordx4")]
    assert stores, name
    first = stores[0]                                        # the deferred flush of the previous tile: the first nt store of the loop
    after = [i for i in loads if i > first]
    assert after, name
    between = lines[first:after[0]]
    assert not any(ln.startswith("s_waitcnt") and "vmcnt(0)" in ln for ln in between), \
        "%s: the flush's stores are drained before the next tile is requested:\n%s" % (name, "\n".join(between))
    # the request of a tile: three 16-byte loads per lane, back to back — in the loop (behind the flush) and once in front of it
    assert len(after) == 3 and len(loads) == 6, (name, len(after), len(loads))
    assert not any(ln.startswith("s_waitcnt") and "vmcnt" in ln for ln in lines[after[0]:after[-1]]), name
    # ... and nothing narrower streams the tile
    assert not any(nt(i, "global_load_dword") and not nt(i, "global_load_dwordx4") for i in range(len(lines))), name


def test_f32_gather_kernels_keep_eight_waves_per_simd(band_isa):
    kernels, text = band_isa
    names = pick(kernels, "band_cold_kernel_f32")
    assert len(names) == 3                                   # cold pieces, short rows in the accumulate and the operator form
    for name in names:
        vgpr, _ = resources(text, name)
        assert vgpr <= 64, (name, vgpr)
