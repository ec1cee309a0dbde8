"""Cases of tests/test_plan_ownership_emu_cpu.py: who owns the device arrays that a handle derives from its own (SpMV, SpMM,
Gauss-Seidel and triangular-solve plans, sparse-vector scratch, per-stream scratch), watched from outside through the two
hooks of the kernel emulator (tests/emu/hipemu.cpp): hipemu_live_count (live blocks + streams + events) and
hipemu_fail_malloc_in (the n-th hipMalloc from now fails with hipErrorOutOfMemory).

    python tests/plan_ownership_cases.py CASE        (SPRS_HIP_LIBRARY = the emulator build)

runs one case and prints one JSON line.  A case uploads its operands, runs its operation TWICE on the handle (the second
multiply is the one that builds a deferred plan; it takes fresh operands, so nothing stale passes) and compares with the
reference of the seam suite the matrix comes from: the int64 product for the SpMV and SpMM cases (test_spmv_seams_gpu.py,
test_spmm_gpu.py, and what check_band_exact's oracle equals on integer values), the oracle's exact iterates for Gauss-Seidel
(test_solver_seams_gpu.py), the restatements of trisolve_ref.py and csvec_ref.py.  Then:

  1. clean path: live count before the upload == live count after the handles went and the pool was trimmed;
  2. with N = the hipMalloc calls of that run, for every n in 1 .. N: the n-th hipMalloc fails.  The sequence ends in
     OUT_OF_MEMORY with a message, or — the re-laid-out rhs copy of the SpMM that does not fit — in the right result.  The handle
     that saw the failure (a fresh one when it was the upload that failed) then runs the sequence again with the switch off and
     gives the right result: a half-built plan or scratch must not poison it.  Everything is freed, the pool trimmed, and the
     live count is back where it started.

Step 2 runs with the option pool = 0: pool_alloc answers an out-of-memory by trimming the pool and asking again, which would hide
every failure at a pooled block whenever the pool holds anything; without the pool each of the N calls is one injection point
and none is masked.  (The other documented fall-back, the banded plan in auto mode, needs a matrix of 4 M entries to be tried at
all; the banded case forces the plan, so its failures are reported.)"""
import ctypes as C
import gc
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import sprs_amd                                                             # noqa: E402
from sprs_amd import _ffi, linalg, prod                                      # noqa: E402
from sprs_amd.device import DeviceCsMat, DeviceCsVec, DeviceVec             # noqa: E402

lib = _ffi.lib
lib.hipemu_live_count.restype = C.c_long
lib.hipemu_fail_malloc_in.restype = C.c_long
lib.hipemu_fail_malloc_in.argtypes = [C.c_long]
FAR = 1 << 40


def live():
    gc.collect()
    sprs_amd.pool_trim()
    return lib.hipemu_live_count()


class Case:
    """options: set before the first upload; upload() -> the handle(s); run(h): the operation twice, checked"""
    options = {}
    fallback = False                        # the sequence may absorb a failed allocation and still give the right result

    def __init__(self):
        self.rng = np.random.default_rng(1)


class Spmv(Case):
    kind = 1

    def __init__(self):
        super().__init__()
        from test_spmv_seams_gpu import int64_spmv, seam_csr
        self.int64_spmv = int64_spmv
        self.shape, self.ip, self.ix = seam_csr(self.lens, cols=self.cols, seed=3)
        self.dt = self.rng.integers(1, 5, size=self.ix.size).astype(np.float64)

    def upload(self):
        return DeviceCsMat.from_host(self.shape, self.ip, self.ix, self.dt)

    def run(self, a):
        for _ in range(2):
            x = (self.rng.permutation(self.shape[1]) + 1).astype(np.float64)
            y = (a * DeviceVec.from_host(x)).to_host()
            assert a.spmv_plan_info()[0] == self.kind
            assert np.array_equal(y, self.int64_spmv(self.ip, self.ix, self.dt, x).astype(np.float64))


class Tile(Spmv):
    """the plain tile plan: two tiles of 2048, a row of 2500 entries across them"""
    options = dict(spmv_band=2, spmv_xcs=2, spmv_tile=2048)
    lens, cols = [3] * 200 + [2500] + [0, 1, 5] * 30, 4000


class Sliced(Spmv):
    """the XCD-sliced plan with relabelled columns: short rows in two tiles, long rows whose slices span several tiles"""
    options = dict(spmv_band=2, spmv_xcs=1, spmv_xcs_split=8, spmv_relabel=1, spmv_tile=2048)
    lens, cols, kind = [7] * 300 + [2500] * 9 + [0, 40] * 20, 5000, 2


class Banded(Spmv):
    """the banded plan (a bucket seam case of test_spmv_band_gpu.py): hot slice, cold pieces, short piece, second stream"""
    options = dict(spmv_band=1, spmv_band_hot=1, spmv_band_phases=1, spmv_band_tile=8192, spmv_band_split=8, spmv_band_cold_tiles=1)
    lens, cols, kind = [5] * 201 + [3, 5] + [900] * 2, 20000, 3


class HostSpmv(Spmv):
    """sprs_hip_spmv_f64_host: upload, one multiply, download and release in one call"""
    options = dict(spmv_band=2, spmv_xcs=2, spmv_tile=2048)
    lens, cols = Tile.lens, Tile.cols

    def upload(self):
        return None

    def run(self, _):
        for acc in (0, 1):
            x = (self.rng.permutation(self.shape[1]) + 1).astype(np.float64)
            y0 = self.rng.integers(1, 9, size=self.shape[0]).astype(np.float64)
            y = y0.copy()
            vp = lambda v: v.ctypes.data_as(C.c_void_p)
            _ffi.check(lib.sprs_hip_spmv_f64_host(self.shape[0], self.shape[1], vp(self.ip), self.ip.dtype.itemsize, vp(self.ix),
                                                  self.ix.dtype.itemsize, vp(self.dt), vp(x), x.size, vp(y), y.size, acc))
            assert np.array_equal(y, (self.int64_spmv(self.ip, self.ix, self.dt, x) + (y0.astype(np.int64) if acc else 0)).astype(np.float64))


class Spmm(Case):
    """rows of 3, 2 and 0 entries and one of 700 (two chunks of 512; three tiles of 256) times 8 columns"""
    lens, cols, k = [3] * 200 + [700] + [0, 2] * 20, 800, 8

    def __init__(self):
        super().__init__()
        from test_spmm_gpu import exact_csr, exact_ints, int64_product
        self.exact_ints, self.int64_product = exact_ints, int64_product
        self.shape, self.ip, self.ix = exact_csr(self.lens, self.cols, seed=5)
        self.dt = exact_ints(self.rng, self.ix.size)

    def upload(self):
        return DeviceCsMat.from_host(self.shape, self.ip, self.ix, self.dt)

    def run(self, a):
        for _ in range(2):
            rhs = self.exact_ints(self.rng, (self.cols, self.k))
            got = (a * prod.DeviceMat.from_host(rhs)).to_host()
            assert np.array_equal(got, self.int64_product(self.shape, self.ip, self.ix, self.dt, rhs).astype(np.float64))


class SpmmStream(Spmm):
    options = dict(spmm_stream=1, spmm_relayout=2)


class SpmmChunks(Spmm):
    options = dict(spmm_stream=0, spmm_relayout=2)


class SpmmRelaid(Spmm):
    options = dict(spmm_stream=1, spmm_relayout=1)
    fallback = True


class GaussSeidel(Case):
    """two sweeps of gs_block_system(300): every iterate and the error bit for bit"""
    n, sweeps = 300, 2

    def __init__(self):
        super().__init__()
        import test_solver_seams_gpu as s
        self.ip, self.ix, self.dt = s.gs_block_system(self.n)[:3]
        self.x0, self.rhs, self.x_ref, self.error_ref, _ = s.gs_swept(self.n, self.sweeps)
        self.bits = s.bits

    def upload(self):
        return DeviceCsMat.from_host((self.n, self.n), self.ip, self.ix, self.dt)

    def run(self, a):
        for _ in range(2):
            x = DeviceVec.from_host(self.x0)
            res = linalg.gauss_seidel(a, x, DeviceVec.from_host(self.rhs), self.sweeps, -1.0)
            assert np.array_equal(x.to_host(), self.x_ref) and self.bits(res.error) == self.bits(self.error_ref)


class UpperSolve(Case):
    """usolve_csr on a full non-symmetric matrix of 200 rows, one of them with 60 more entries"""
    n = 200

    def __init__(self):
        super().__init__()
        import trisolve_ref as ref
        from test_gauss_seidel_gpu import _random_system
        from test_trisolve_gpu import arrays
        self.ip, self.ix, self.dt = arrays(_random_system(self.n, 11, 4, 60), "usolve_csr")
        self.solve = lambda b: ref.usolve_csr_dense_rhs(self.n, self.ip, self.ix, self.dt, b)

    def upload(self):
        return DeviceCsMat.from_host((self.n, self.n), self.ip, self.ix, self.dt)

    def run(self, a):
        for _ in range(2):
            b = self.rng.standard_normal(self.n)
            x = DeviceVec.from_host(b)
            linalg.usolve_csr_dense_rhs(a, x)
            assert np.array_equal(x.to_host(), self.solve(b))


class MatCsvec(Case):
    """CSR A x v on the ragged matrix of test_small_ragged_all_densities, v with 90 of 900 entries"""

    def __init__(self):
        super().__init__()
        from csvec_ref import bits, masked_dot_vec
        from test_csvec_gpu import _ragged
        self.shape, ip, self.ix, self.dt = _ragged(700, 900, 11)
        self.ip = ip.astype(np.uint64)
        self.bits, self.masked_dot_vec = bits, masked_dot_vec

    def upload(self):
        return DeviceCsMat.from_host(self.shape, self.ip, self.ix, self.dt)

    def run(self, a):
        for _ in range(2):
            vidx = np.sort(self.rng.choice(900, 90, replace=False)).astype(np.uint64)
            vval = self.rng.standard_normal(90)
            d, i, v = (a * DeviceCsVec.from_host(900, vidx, vval)).to_host()
            rd, ri, rv, _ = self.masked_dot_vec(self.ip, self.ix, self.dt, 700, 900, vidx, vval)
            assert d == rd and np.array_equal(i.astype(np.int64), np.asarray(ri, dtype=np.int64)) and np.array_equal(self.bits(v), self.bits(rv))


CASES = {"tile": Tile, "sliced": Sliced, "banded": Banded, "spmm_stream": SpmmStream, "spmm_chunks": SpmmChunks, "spmm_relaid": SpmmRelaid,
         "gauss_seidel": GaussSeidel, "upper_solve": UpperSolve, "csmat_csvec": MatCsvec, "spmv_host": HostSpmv}


def main(name):
    case = CASES[name]()
    for k, v in case.options.items():
        sprs_amd.set_option(k, v)
    start = live()

    def sequence(h=None):
        """-> (outcome, the handle if the upload got that far): "ok", or "oom" for OUT_OF_MEMORY with a message"""
        try:
            if h is None:
                h = case.upload()
            case.run(h)
            return "ok", h
        except sprs_amd.SprsHipError as e:
            assert e.status == _ffi.OUT_OF_MEMORY and str(e).strip(), "status %d, message %r" % (e.status, str(e))
            return "oom", h

    # 1. the clean path leaks nothing (the pool as shipped)
    outcome, h = sequence()
    assert outcome == "ok"
    del h
    assert live() == start, "clean path: %d live blocks / streams / events, %d before" % (live(), start)

    # 2. no failing allocation leaks anything
    sprs_amd.set_option("pool", 0)
    lib.hipemu_fail_malloc_in(FAR)
    outcome, h = sequence()
    mallocs = FAR - lib.hipemu_fail_malloc_in(0)
    assert outcome == "ok" and mallocs > 0
    del h
    assert live() == start
    count = {"oom": 0, "ok": 0}
    for n in range(1, mallocs + 1):
        lib.hipemu_fail_malloc_in(n)
        outcome, h = sequence()
        left = lib.hipemu_fail_malloc_in(0)
        assert left == 0, "injection %d of %d never fired (%d calls left)" % (n, mallocs, left)
        assert outcome == "oom" or case.fallback, "injection %d of %d was swallowed" % (n, mallocs)
        count[outcome] += 1
        outcome, h = sequence(h)                  # the switch is off: the handle that saw the failure gives the right result
        assert outcome == "ok"
        del h
        now = live()
        assert now == start, "injection %d of %d: %d live blocks / streams / events, %d before" % (n, mallocs, now, start)
    print(json.dumps({"case": name, "mallocs": mallocs, "injections": count["oom"] + count["ok"], "oom": count["oom"], "fallback": count["ok"]}))


if __name__ == "__main__":
    main(sys.argv[1])
