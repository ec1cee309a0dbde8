// The LDL^T part of include/sprs_hip.hpp (C++ host mirror, namespace ldl) through the C ABI: the reference's own golden system
// (sprs-ldl/src/lib.rs:634-866), compared bit for bit.  Stand-alone: g++ and libsprs_hip.so, see ldl_mirror.mk.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/sprs_hip.hpp"

using namespace sprs_hip;

static int fails = 0;
#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                              \
        }                                                         \
    } while (0)

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

int main() {
    const uint64_t none = UINT64_MAX;
    // test_mat1, test_vec1 (lib.rs:634-652)
    const std::vector<uint64_t> indptr = {0, 2, 5, 6, 7, 13, 14, 17, 20, 24, 28};
    const std::vector<uint64_t> indices = {0, 8, 1, 4, 9, 2, 3, 1, 4, 6, 7, 8, 9, 5, 4, 6, 9, 4, 7, 8, 0, 4, 7, 8, 1, 4, 6, 9};
    const std::vector<double> data = {1.7, 0.13, 1.,  0.02, 0.01, 1.5,  1.1, 0.02, 2.6,  0.16, 0.09, 0.52, 0.53, 1.2,
                                      0.16, 1.3, 0.56, 0.09, 1.6, 0.11, 0.13, 0.52, 0.11, 1.4, 0.01, 0.53, 0.56, 3.1};
    const std::vector<double> b = {0.287, 0.22, 0.45, 0.44, 2.486, 0.72, 1.55, 1.424, 1.621, 3.759};
    // expected_factors1 (lib.rs:654-685)
    const std::vector<uint64_t> lp = {0, 1, 3, 3, 3, 7, 7, 10, 12, 13, 13};
    const std::vector<uint64_t> li = {8, 4, 9, 6, 7, 8, 9, 7, 8, 9, 8, 9, 9};
    const std::vector<double> lx = {0.076470588235294124,   0.02,                  0.01,
                                    0.061547930450838589,   0.034620710878596701,  0.20003077396522542,
                                    0.20380058470533929,    -0.0042935346524025902, -0.024807089102770519,
                                    0.40878266366119237,    0.05752526570865537,   -0.010068305077340346,
                                    -0.071852278207562709};
    const std::vector<double> d = {1.7, 1., 1.5, 1.1000000000000001, 2.5996000000000001, 1.2, 1.290152331127866, 1.5968603527854308,
                                   1.2799646117414738, 2.7695677698030283};
    // expected_lsolve_res1, expected_dsolve_res1, expected_res1 (lib.rs:687-730)
    const std::vector<double> after_l = {0.28699999999999998, 0.22, 0.45000000000000001, 0.44, 2.4816000000000003, 0.71999999999999997,
                                         1.3972626557931991,  1.3440844395148306, 1.0599997771886431, 2.7695677698030279};
    const std::vector<double> after_d = {0.16882352941176471, 0.22, 0.29999999999999999, 0.39999999999999997, 0.95460840129250657,
                                         0.59999999999999998, 1.0830214557467768, 0.84170443406044937, 0.82814772179243734,
                                         0.99999999999999989};
    const std::vector<double> res = {0.099999999999999992, 0.19999999999999998, 0.29999999999999999, 0.39999999999999997, 0.5,
                                     0.59999999999999998,  0.70000000000000007, 0.79999999999999993, 0.90000000000000002,
                                     0.99999999999999989};
    try {
        DeviceCsMat mat(SPRS_HIP_CSC, 10, 10, indptr, indices, data);
        ldl::LdlSymbolic sym(mat);
        EXPECT(sym.problem_size() == 10 && sym.nnz() == 13);
        EXPECT(sym.colptr() == lp);
        EXPECT((sym.parents() == std::vector<uint64_t>{8, 4, none, none, 6, none, 7, 8, 9, none}));
        EXPECT(sym.stats()[2] == 2);
        ldl::LdlNumeric num = sym.factor(mat);
        std::vector<uint64_t> gp, gi;
        std::vector<double> gx;
        DeviceCsMat l = num.l();
        l.to_host(gp, gi, gx);
        EXPECT(!l.is_csr() && gp == lp && gi == li && same_bits(gx, lx));
        EXPECT(same_bits(num.d().to_host(), d));
        EXPECT(same_bits(num.solve(DeviceVec(b)).to_host(), res));
        // test_solve1: the three stages through the free functions
        DeviceVec x(b);
        ldl::ldl_lsolve(l, x);
        EXPECT(same_bits(x.to_host(), after_l));
        ldl::diag_solve(num.d(), x);
        EXPECT(same_bits(x.to_host(), after_d));
        ldl::ldl_ltsolve(l, x);
        EXPECT(same_bits(x.to_host(), res));
        num.update(mat);
        EXPECT(same_bits(num.d().to_host(), d));
        // permuted_ldl_solve and cuthill_ldl_solve (lib.rs:814-866)
        DeviceCsMat m4(SPRS_HIP_CSC, 4, 4, std::vector<uint64_t>{0, 2, 4, 6, 8}, std::vector<uint64_t>{0, 3, 1, 2, 1, 2, 0, 3},
                       std::vector<double>{1., 2., 21., 6., 6., 2., 2., 8.});
        const std::vector<double> b4 = {9., 60., 18., 34.}, x4 = {1., 2., 3., 4.};
        DevicePerm p4(std::vector<uint64_t>{0, 2, 1, 3});
        ldl::LdlNumeric n4 = ldl::LdlSymbolic(m4, &p4).factor(m4);
        EXPECT(same_bits(n4.solve(DeviceVec(b4)).to_host(), x4));
        EXPECT(same_bits(n4.d().to_host(), x4));
        EXPECT(same_bits(ldl::Ldl().check_symmetry(false).numeric(m4).solve(DeviceVec(b4)).to_host(), x4));
        bool threw = false;
        try {
            DeviceCsMat ones(SPRS_HIP_CSC, 2, 2, std::vector<uint64_t>{0, 2, 4}, std::vector<uint64_t>{0, 1, 0, 1}, std::vector<double>{1., 1., 1., 1.});
            ldl::Ldl().fill_in_reduction(ldl::FillInReduction::NoReduction).numeric(ones);
        } catch (const ldl::SingularMatrix &e) {
            threw = e.index == 1 && e.status == SPRS_HIP_SINGULAR_MATRIX;
        }
        EXPECT(threw);
    } catch (const Error &e) {
        std::printf("FAILED: %s\n", e.what());
        return 1;
    }
    if (fails) return 1;
    std::printf("all passed\n");
    return 0;
}
