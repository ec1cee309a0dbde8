"""The f32 SpGEMM reference of tests/spgemm_f32_ref.py, pinned without a device: exact on the reference's golden products,
within the rounding bound of the f64 oracle on a random case, and DIFFERENT from an f64 product rounded once at the end on the
order-stress inputs — the property that makes bit-equality with it a test of the order of the additions."""
import numpy as np

from conftest import as_csr
from spgemm_f32_ref import as_f32, gamma_bound, mul_csr_csr_f32, product_counts_and_magnitudes
from test_spgemm_gpu import _order_stress_cases


def test_reference_is_exact_on_the_golden_products(golden):
    """small integer values: every f32 product and sum is exact, so the f32 chain equals the golden f64 values"""
    a, b = as_csr(golden["mat1"]), as_csr(golden["mat2"])
    for rhs, key in ((a, "mat1_self_matprod"), (b, "mat1_matprod_mat2")):
        exp = as_csr(golden[key])
        shape, ip, ix, dt = mul_csr_csr_f32(as_f32(a), as_f32(rhs))
        assert shape == exp[0] and np.array_equal(ip, exp[1]) and np.array_equal(ix, exp[2])
        assert dt.dtype == np.float32 and np.array_equal(dt.astype(np.float64), exp[3])


def test_reference_within_the_rounding_bound_of_the_f64_oracle():
    from oracle import oracle
    from helpers import ragged_csr
    rng = np.random.default_rng(3)
    b = ragged_csr([int(v) for v in rng.integers(0, 40, size=300)], 500, seed=4, positive=False)
    a = ragged_csr([int(v) for v in rng.integers(0, 60, size=80)], 300, seed=5, positive=False)
    a32, b32 = as_f32(a), as_f32(b)
    # the oracle on the f32 operands widened to f64: the same products, exact, summed in f64
    wide = lambda m: (m[0], m[1], m[2], m[3].astype(np.float64))
    ref64 = oracle.mul_csr_csr(*wide(a32), *wide(b32), threads=1)
    got = mul_csr_csr_f32(a32, b32, structure=ref64)
    counts, mag = product_counts_and_magnitudes(a32, b32)
    assert counts.max() > 4
    assert np.all(np.abs(got[3].astype(np.float64) - ref64[3]) <= gamma_bound(counts, mag))


def test_order_stress_inputs_tell_the_f32_chain_from_a_rounded_f64_product():
    from oracle import oracle
    for a, b in _order_stress_cases():
        a32, b32 = as_f32(a), as_f32(b)
        wide = lambda m: (m[0], m[1], m[2], m[3].astype(np.float64))
        ref64 = oracle.mul_csr_csr(*wide(a32), *wide(b32), threads=1)
        chain = mul_csr_csr_f32(a32, b32, structure=ref64)[3]
        assert np.all(np.isfinite(chain))                               # no product or sum overflows in f32: no rescaling needed
        assert np.any(chain.view(np.uint32) != ref64[3].astype(np.float32).view(np.uint32))
