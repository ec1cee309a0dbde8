// Stand-alone check of the HOST side of the dense <-> sparse entries (include/sprs_hip.h): every call below fails in its
// argument checks, before any device work, and the program is built — with the library's sources, compiled for the host as
// tests/emu does — under -fsanitize=address,undefined (make -C tests/cpp dense_args_asan.bin).  A sanitizer report aborts
// it; a wrong status or message makes it return 1.  It needs no device and is not loaded into any other process.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../include/sprs_hip.h"

static int failures = 0;

static void expect(int32_t status, int32_t want, const char *text, const char *what) {
    const char *msg = sprs_hip_last_error();
    if (status != want || (text && !strstr(msg, text))) {
        std::fprintf(stderr, "FAIL %s: status %d (want %d), message \"%s\" (want \"%s\")\n", what, status, want, msg, text ? text : "");
        ++failures;
    }
}

int main() {
    double cell[16] = {0};                          // never dereferenced by the library: the calls stop at their checks
    double other[16] = {0};
    sprs_hip_csmat *h = nullptr;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint64_t huge = ~0ull;

    // sprs_hip_csmat_from_dense_f64
    expect(sprs_hip_csmat_from_dense_f64(nullptr, SPRS_HIP_CSR, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, 0.0, 8, 8, nullptr), SPRS_HIP_INVALID_ARG, "NULL", "from_dense out");
    expect(sprs_hip_csmat_from_dense_f64(&h, 9, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, 0.0, 8, 8, nullptr), SPRS_HIP_INVALID_ARG, "storage", "from_dense storage");
    expect(sprs_hip_csmat_from_dense_f64(&h, SPRS_HIP_CSR, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, 0.0, 3, 8, nullptr), SPRS_HIP_INVALID_ARG, "2, 4 or 8", "from_dense iptr width");
    expect(sprs_hip_csmat_from_dense_f64(&h, SPRS_HIP_CSR, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, 0.0, 8, 16, nullptr), SPRS_HIP_INVALID_ARG, "2, 4 or 8", "from_dense idx width");
    expect(sprs_hip_csmat_from_dense_f64(&h, SPRS_HIP_CSR, cell, 3, 5, -1, 5, 0.0, 8, 8, nullptr), SPRS_HIP_INVALID_ARG, "layout", "from_dense layout");
    expect(sprs_hip_csmat_from_dense_f64(&h, SPRS_HIP_CSR, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 4, nan, 8, 8, nullptr), SPRS_HIP_INVALID_ARG, "leading dimension", "from_dense ld row-major");
    expect(sprs_hip_csmat_from_dense_f64(&h, SPRS_HIP_CSC, cell, 3, 5, SPRS_HIP_COL_MAJOR, 2, -1.0, 2, 2, nullptr), SPRS_HIP_INVALID_ARG, "leading dimension", "from_dense ld column-major");
    expect(sprs_hip_csmat_from_dense_f64(&h, SPRS_HIP_CSR, cell, huge, huge, SPRS_HIP_ROW_MAJOR, huge, 0.0, 8, 8, nullptr), SPRS_HIP_INVALID_ARG, "overflows", "from_dense rows * cols");
    expect(sprs_hip_csmat_from_dense_f64(&h, SPRS_HIP_CSR, nullptr, 3, 5, SPRS_HIP_ROW_MAJOR, 5, 0.0, 8, 8, nullptr), SPRS_HIP_INVALID_ARG, "NULL", "from_dense NULL matrix");
    if (h) {
        std::fprintf(stderr, "FAIL: *out written by a failing call\n");
        ++failures;
    }

    // sprs_hip_csmat_assign_to_dense_f64 / sprs_hip_csmat_to_dense_f64
    int32_t (*const assign[2])(const sprs_hip_csmat *, double *, uint64_t, uint64_t, int32_t, uint64_t, void *) = {
        sprs_hip_csmat_assign_to_dense_f64, sprs_hip_csmat_to_dense_f64};
    for (auto f : assign) {
        expect(f(nullptr, cell, 3, 5, 7, 5, nullptr), SPRS_HIP_INVALID_ARG, "layout", "assign layout");
        expect(f(nullptr, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 4, nullptr), SPRS_HIP_INVALID_ARG, "leading dimension", "assign ld");
        expect(f(nullptr, cell, 3, 5, SPRS_HIP_COL_MAJOR, 0, nullptr), SPRS_HIP_INVALID_ARG, "leading dimension", "assign ld 0");
        expect(f(nullptr, nullptr, 3, 5, SPRS_HIP_ROW_MAJOR, 5, nullptr), SPRS_HIP_INVALID_ARG, "NULL matrix", "assign NULL matrix");
        expect(f(nullptr, cell, huge, 2, SPRS_HIP_COL_MAJOR, huge, nullptr), SPRS_HIP_INVALID_ARG, "overflows", "assign rows * cols");
        expect(f(nullptr, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, nullptr), SPRS_HIP_INVALID_ARG, "NULL handle", "assign NULL handle");
        expect(f(nullptr, nullptr, 0, 5, SPRS_HIP_ROW_MAJOR, 5, nullptr), SPRS_HIP_INVALID_ARG, "NULL handle", "assign empty array, NULL handle");
    }

    // sprs_hip_csmat_binop_dense_f64 / sprs_hip_csmat_add_dense_f64
    expect(sprs_hip_csmat_binop_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, SPRS_HIP_BINOP_SUB, 1.0, 1.0, other, 5, nullptr), SPRS_HIP_INVALID_ARG, "op must be", "binop op");
    expect(sprs_hip_csmat_binop_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, 77, 1.0, 1.0, other, 5, nullptr), SPRS_HIP_INVALID_ARG, "op must be", "binop op 77");
    expect(sprs_hip_csmat_binop_dense_f64(nullptr, cell, 3, 5, 2, 5, SPRS_HIP_BINOP_ADD, 1.0, 1.0, other, 5, nullptr), SPRS_HIP_INVALID_ARG, "layout", "binop layout");
    expect(sprs_hip_csmat_binop_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 4, SPRS_HIP_BINOP_ADD, 1.0, 1.0, other, 5, nullptr), SPRS_HIP_INVALID_ARG, "leading dimension", "binop ld");
    expect(sprs_hip_csmat_binop_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, SPRS_HIP_BINOP_MUL, nan, nan, other, 4, nullptr), SPRS_HIP_INVALID_ARG, "leading dimension", "binop out_ld");
    expect(sprs_hip_csmat_binop_dense_f64(nullptr, nullptr, 3, 5, SPRS_HIP_ROW_MAJOR, 5, SPRS_HIP_BINOP_MUL, 1.0, 1.0, other, 5, nullptr), SPRS_HIP_INVALID_ARG, "NULL matrix", "binop NULL rhs");
    expect(sprs_hip_csmat_binop_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, SPRS_HIP_BINOP_MUL, 1.0, 1.0, nullptr, 5, nullptr), SPRS_HIP_INVALID_ARG, "NULL matrix", "binop NULL out");
    expect(sprs_hip_csmat_binop_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_ROW_MAJOR, 5, SPRS_HIP_BINOP_MUL, 1.0, 1.0, other, 5, nullptr), SPRS_HIP_INVALID_ARG, "NULL handle", "binop NULL handle");
    expect(sprs_hip_csmat_add_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_COL_MAJOR, 2, other, nullptr), SPRS_HIP_INVALID_ARG, "leading dimension", "add ld");
    expect(sprs_hip_csmat_add_dense_f64(nullptr, cell, 3, 5, 5, 5, other, nullptr), SPRS_HIP_INVALID_ARG, "layout", "add layout");
    expect(sprs_hip_csmat_add_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_COL_MAJOR, 3, nullptr, nullptr), SPRS_HIP_INVALID_ARG, "NULL matrix", "add NULL out");
    expect(sprs_hip_csmat_add_dense_f64(nullptr, cell, 3, 5, SPRS_HIP_COL_MAJOR, 3, other, nullptr), SPRS_HIP_INVALID_ARG, "NULL handle", "add NULL handle");

    // the option that publishes the tile
    int64_t tile = 0;
    expect(sprs_hip_get_option("dense_tile", &tile), SPRS_HIP_OK, nullptr, "get dense_tile");
    expect(sprs_hip_set_option("dense_tile", tile + 1), SPRS_HIP_INVALID_ARG, "dense_tile", "set dense_tile");
    if (tile != 2048) {
        std::fprintf(stderr, "FAIL: dense_tile is %lld\n", (long long)tile);
        ++failures;
    }
    std::printf(failures ? "dense_args_asan: %d failure(s)\n" : "dense_args_asan: ok\n", failures);
    return failures ? 1 : 0;
}
