// The ordering part of include/sprs_hip.hpp (C++ host mirror) through the C ABI: the reference's own test data
// (sprs/src/sparse/linalg/ordering.rs:567-660).  Stand-alone: g++ and libsprs_hip.so, see ordering_mirror.mk.
#include <cstdio>
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

int main() {
    const double x = -1.0;
    const std::vector<uint64_t> indptr = {0, 4, 8, 12, 16, 20, 29, 31, 33, 37, 40, 44, 48};
    const std::vector<uint64_t> indices = {0, 4, 5, 8, 1, 5, 8, 10, 2, 3, 4, 5, 2, 3, 5, 11, 0, 2, 4, 5, 0, 1, 2, 3, 4, 5, 8, 10, 11, 6, 9, 7, 9,
                                           0, 1, 5, 8, 6, 7, 9, 1, 5, 10, 11, 3, 5, 10, 11};
    const std::vector<double> data = {3., x, x, x, 3., x, x, x, 3., x, x, x, x, 3., x, x, x, x, 3., x, x, x, x, x, x, 8., x, x, x, 1., x, 1., x,
                                      x, x, x, 3., x, x, 2., x, x, 3., x, x, x, x, 3.};
    try {
        DeviceCsMat lap(SPRS_HIP_CSR, 12, 12, indptr, indices, data);
        EXPECT(ordering::is_symmetric(lap));
        EXPECT(lap.max_outer_nnz() == 9);
        EXPECT((lap.degrees() == std::vector<uint64_t>{3, 3, 3, 3, 3, 8, 1, 1, 3, 2, 3, 3}));
        ordering::Ordering o = ordering::reverse_cuthill_mckee(lap);
        EXPECT((o.perm.vec() == std::vector<uint64_t>{7, 9, 6, 11, 10, 3, 1, 2, 5, 8, 4, 0}));
        EXPECT((o.connected_parts == std::vector<uint64_t>{0, 3, 12}));
        EXPECT(o.stats[0] == 2);
        DeviceCsMat banded = permutation::transform_mat_papt(lap, o.perm);
        EXPECT(banded.nnz() == lap.nnz());
        DeviceCsMat eye = DeviceCsMat::eye(3);
        EXPECT((ordering::reverse_cuthill_mckee(eye).perm.vec() == std::vector<uint64_t>{2, 1, 0}));
        EXPECT((ordering::cuthill_mckee_custom(eye, ordering::Start::PseudoPeripheral, ordering::Order::Forward).perm.vec() ==
                std::vector<uint64_t>{0, 1, 2}));
        EXPECT((ordering::cuthill_mckee_custom(lap, ordering::Start::MinimumDegree, ordering::Order::Forward).connected_parts.size() == 3));
        bool threw = false;
        try {
            DeviceCsMat wide(SPRS_HIP_CSR, 2, 3, std::vector<uint64_t>{0, 1, 2}, std::vector<uint64_t>{0, 1}, std::vector<double>{1.0, 1.0});
            ordering::reverse_cuthill_mckee(wide);
        } catch (const Error &e) {
            threw = e.status == SPRS_HIP_DIM_MISMATCH;
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
