// C ABI of libsprs_hip.so (include/sprs_hip.h): the thread-local status / error state, argument checking and the reference's
// contracts (which operands a call accepts, in which order it tests them, what a result inherits) around the internal
// functions, raw device buffers, options.  Handles are made and released in handle.hpp, where the pool lives; results arrive
// here inside their owners and are released to the caller's raw pointer in the extern "C" function.  Kernels live in the other
// translation units.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.hpp"

namespace sprs_hip {

static thread_local std::string tl_msg;
static thread_local int32_t tl_hip_code = 0;

void clear_error() {
    tl_msg.clear();
    tl_hip_code = 0;
}

void set_error(int32_t status, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    tl_msg = buf;
    if (status != SPRS_HIP_HIP_ERROR) tl_hip_code = 0;
}

int32_t fail_hip(hipError_t e, const char *what) {
    tl_hip_code = (int32_t)e;
    (void)hipGetLastError();   // clear the sticky error
    if (e == hipErrorOutOfMemory) {
        set_error(SPRS_HIP_OUT_OF_MEMORY, "out of device memory in %s", what);
        return SPRS_HIP_OUT_OF_MEMORY;
    }
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) {
        set_error(SPRS_HIP_NO_DEVICE, "no usable HIP device (%s) in %s", hipGetErrorString(e), what);
        tl_hip_code = (int32_t)e;
        return SPRS_HIP_NO_DEVICE;
    }
    char buf[400];
    snprintf(buf, sizeof buf, "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    tl_msg = buf;
    return SPRS_HIP_HIP_ERROR;
}

Options &options() {
    static Options o;
    return o;
}

// utils::check_compressed_structure (sprs/src/sparse.rs:300-358) on host arrays.
template <typename I, typename P>
static int32_t check_structure(uint64_t inner, uint64_t outer, const P *indptr, const I *indices) {
    // Iptr / I must be able to represent the dimensions (sparse.rs:314-324)
    if ((uint64_t)(I)inner != inner) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Index type not large enough for this matrix");
    if ((uint64_t)(P)(outer + 1) != outer + 1) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Iptr type not large enough for this matrix");
    const uint64_t off = (uint64_t)indptr[0];
    for (uint64_t i = 0; i < outer; ++i)
        if (indptr[i + 1] < indptr[i]) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Unsorted indptr");
    if ((uint64_t)indptr[outer] > (UINT64_MAX >> 1)) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "An indptr value is larger than allowed");
    for (uint64_t r = 0; r < outer; ++r) {
        const uint64_t s = (uint64_t)indptr[r] - off, e = (uint64_t)indptr[r + 1] - off;
        for (uint64_t p = s + 1; p < e; ++p)
            if (indices[p] <= indices[p - 1]) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Indices are not sorted");
        if (e > s && (uint64_t)indices[e - 1] >= inner)
            SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Indice is larger than inner dimension");
    }
    return SPRS_HIP_OK;
}

static bool widths_ok(int32_t iptr_bytes, int32_t idx_bytes) {
    return (iptr_bytes == 4 || iptr_bytes == 8) && (idx_bytes == 4 || idx_bytes == 8);
}

static bool host_widths_ok(int32_t iptr_bytes, int32_t idx_bytes) {     // what a host array may hold: u16 too (indexing.rs:124-130)
    return (iptr_bytes == 2 || iptr_bytes == 4 || iptr_bytes == 8) && (idx_bytes == 2 || idx_bytes == 4 || idx_bytes == 8);
}

static uint64_t width_max(int32_t bytes) { return bytes >= 8 ? ~0ull : ((1ull << (8 * bytes)) - 1ull); }

// A host index array as the device holds it: 2-byte indices (u16 / i16, indexing.rs:124-130) widened to 4 bytes, any other
// width as it is.
struct HostIndices {
    std::vector<uint32_t> wide;
    const void *p;
    int32_t bytes;                 // width on the device
    HostIndices(const HostIndices &) = delete;                    // p may point into wide
    HostIndices &operator=(const HostIndices &) = delete;
    HostIndices(const void *src, uint64_t count, int32_t decl_bytes) : p(src), bytes(decl_bytes == 2 ? 4 : decl_bytes) {
        if (decl_bytes != 2 || !count) return;
        wide.resize(count);
        for (uint64_t i = 0; i < count; ++i) wide[i] = ((const uint16_t *)src)[i];
        p = wide.data();
    }
    hipError_t upload(void *dst, uint64_t count) const { return count ? copy_to_device(dst, p, count * (uint64_t)bytes, nullptr) : hipSuccess; }
};

// element i of a host index array of the given width
static uint64_t host_index_at(const void *a, int32_t bytes, uint64_t i) {
    return dispatch_host_width(bytes, [&](auto t) { return (uint64_t)((const typename decltype(t)::type *)a)[i]; });
}

// count device indices to the host at the width the caller declared: a declared 2-byte array lives as 4 bytes on the device
// and is narrowed here (every value was range-checked when it was made)
static int32_t download_indices(void *dst, const void *src, uint64_t count, int32_t dev_bytes, int32_t user_bytes) {
    if (user_bytes == dev_bytes) {
        SPRS_TRY_HIP(copy_to_host(dst, src, count * (uint64_t)dev_bytes, nullptr));
        return SPRS_HIP_OK;
    }
    std::vector<uint32_t> wide(count);
    SPRS_TRY_HIP(copy_to_host(wide.data(), src, count * 4, nullptr));
    for (uint64_t i = 0; i < count; ++i) {
        if (wide[i] > 0xFFFFu) SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold %u", wide[i]);
        ((uint16_t *)dst)[i] = (uint16_t)wide[i];
    }
    return SPRS_HIP_OK;
}

int32_t inherit_declared_widths(sprs_hip_csmat *result, const sprs_hip_csmat *from) {
    result->decl_idx_bytes = from->decl_idx_bytes;
    result->decl_iptr_bytes = from->decl_iptr_bytes;
    // I::from_usize on the inner dimension / indices, Iptr::from_usize on the nnz (sparse.rs:314-324, smmp.rs:121, csmat.rs:1794)
    if (result->inner() && result->inner() - 1 > width_max(result->user_idx_bytes()))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the number of rows requested (required %llu)",
                  (unsigned long long)result->inner());
    if (result->nnz > width_max(result->user_iptr_bytes()))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the nnz of the result (%llu)", (unsigned long long)result->nnz);
    return SPRS_HIP_OK;
}

}  // namespace sprs_hip

using namespace sprs_hip;

// the ABI boundary of a result: it takes the declared index widths of the operand it derives from and leaves its owner (on
// overflow it goes with it)
static int32_t finish_result(OwnedCsmat &res, const sprs_hip_csmat *from, sprs_hip_csmat **out) {
    SPRS_TRY(inherit_declared_widths(res.get(), from));
    *out = res.release();
    return SPRS_HIP_OK;
}

// ---- what the f64 and the f32 matrix entries share -------------------------------------------------------------------------------
// Every entry that exists for both precisions has ONE body below: a template on the handle type H (sprs_hip_csmat or
// sprs_hip_csmat_f32), with the scalar T taken from it.  The extern "C" functions forward to it, so a check, its text and its
// place in the order of checks (the reference's assert order) are the same for both.  Where the two differ, the difference
// is a branch or an overload here.
template <typename H>
using Value = typename H::value_type;
template <typename H>
constexpr bool IS_F32 = std::is_same<H, sprs_hip_csmat_f32>::value;

// a handle counts its multiplies: the copy plans (banded, XCD-sliced) are built at the second one
template <typename H>
static void copy_spmv_calls(H *to, const H *from) { to->spmv_calls = from->spmv_calls; }

// CsMat::new / new_csc on host arrays (the checks of the upload entries that follow their argument checks)
template <typename H>
static int32_t csmat_upload(Owned<H> &out, int32_t storage, uint64_t rows, uint64_t cols, const void *indptr, int32_t iptr_bytes,
                            const void *indices, int32_t idx_bytes, const Value<H> *data, int32_t validate) {
    if (storage != SPRS_HIP_CSR && storage != SPRS_HIP_CSC) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "bad storage tag %d", storage);
    if (IS_F32<H>) {               // an f32 matrix takes 4- and 8-byte host arrays only: nothing below is narrow for it
        if (!widths_ok(iptr_bytes, idx_bytes))
            SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths of an f32 matrix must be 4 or 8 bytes (2-byte host arrays are not supported for f32 handles)");
    } else if (!host_widths_ok(iptr_bytes, idx_bytes)) {
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 2, 4 or 8 bytes");
    }
    const uint64_t outer = storage == SPRS_HIP_CSR ? rows : cols;
    const uint64_t inner = storage == SPRS_HIP_CSR ? cols : rows;
    const uint64_t first = host_index_at(indptr, iptr_bytes, 0), last = host_index_at(indptr, iptr_bytes, outer);
    if (last < first) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Unsorted indptr");
    const uint64_t nnz = last - first;
    if (nnz && (!indices || !data)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL indices/data with nnz > 0");   // before the widening loop reads them
    // 2-byte index types (u16 / i16 in sprs): widened to 4 bytes for the device, the declared widths remembered.  The inner
    // dimension is tested against the declared index width here, whatever `validate` says; check_structure below sees the
    // widened arrays, so inner == 65536 passes with u16 indices.
    // (a 2-byte indptr cannot hold a count above its own range: nothing to check for Iptr on the way in)
    const bool narrow = iptr_bytes == 2 || idx_bytes == 2;
    if (narrow && inner && inner - 1 > width_max(idx_bytes)) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Index type not large enough for this matrix");
    // (indices points at the element addressed by indptr[0])
    const HostIndices ip(indptr, outer + 1, iptr_bytes), ix(indices, nnz, idx_bytes);
    if (validate) {
        SPRS_TRY(dispatch_widths(ix.bytes, ip.bytes, [&](auto i, auto p) {
            return check_structure(inner, outer, (const typename decltype(p)::type *)ip.p, (const typename decltype(i)::type *)ix.p);
        }));
    }
    Owned<H> m;
    SPRS_TRY(make_csmat(m, storage, rows, cols, nnz, ip.bytes, ix.bytes));
    hipError_t e = hipSuccess;
    if (first == 0) {
        e = ip.upload(m->indptr, outer + 1);
    } else {
        // to_proper (sprs/src/sparse/indptr.rs:206-214): rebase on the way in
        std::vector<uint8_t> tmp((outer + 1) * (size_t)ip.bytes);
        for (uint64_t i = 0; i <= outer; ++i) {
            const uint64_t v = host_index_at(ip.p, ip.bytes, i) - first;
            if (ip.bytes == 8) ((uint64_t *)tmp.data())[i] = v;
            else ((uint32_t *)tmp.data())[i] = (uint32_t)v;
        }
        e = copy_to_device(m->indptr, tmp.data(), tmp.size(), nullptr);
    }
    if (e == hipSuccess) e = ix.upload(m->indices, nnz);
    if (e == hipSuccess && nnz) e = copy_to_device(m->data, data, nnz * sizeof(Value<H>), nullptr);
    if (e != hipSuccess) return fail_hip(e, IS_F32<H> ? "csmat_f32_upload" : "csmat_upload");
    if (narrow) {
        m->decl_iptr_bytes = iptr_bytes;
        m->decl_idx_bytes = idx_bytes;
    }
    out = std::move(m);
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_upload(H **out, int32_t storage, uint64_t rows, uint64_t cols, const void *indptr, int32_t iptr_bytes, const void *indices,
                            int32_t idx_bytes, const Value<H> *data, int32_t validate) {
    clear_error();
    if (!out || !indptr) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    Owned<H> m;
    SPRS_TRY(csmat_upload(m, storage, rows, cols, indptr, iptr_bytes, indices, idx_bytes, data, validate));
    *out = m.release();
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_wrap_device(H **out, int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, const void *dev_indptr, int32_t iptr_bytes,
                                 const void *dev_indices, int32_t idx_bytes, const Value<H> *dev_data) {
    clear_error();
    if (!out || !dev_indptr) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (storage != SPRS_HIP_CSR && storage != SPRS_HIP_CSC) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "bad storage tag %d", storage);
    if (!widths_ok(iptr_bytes, idx_bytes)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 4 or 8 bytes");
    if (nnz && (!dev_indices || !dev_data)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL indices/data with nnz > 0");
    if (((uintptr_t)dev_indptr | (uintptr_t)dev_indices | (uintptr_t)dev_data) & 15)
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "device buffers must be 16-byte aligned");
    int device = 0;
    const hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
    *out = view_csmat(storage, rows, cols, nnz, dev_indptr, iptr_bytes, dev_indices, idx_bytes, dev_data, device);
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_info(const H *m, uint64_t *rows, uint64_t *cols, uint64_t *nnz, int32_t *iptr_bytes, int32_t *idx_bytes, int32_t *storage) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (rows) *rows = m->rows;
    if (cols) *cols = m->cols;
    if (nnz) *nnz = m->nnz;
    if (iptr_bytes) *iptr_bytes = m->user_iptr_bytes();       // the widths the caller declared (2-byte arrays live widened on the device)
    if (idx_bytes) *idx_bytes = m->user_idx_bytes();
    if (storage) *storage = m->storage;
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_device_ptrs(const H *m, const void **indptr, const void **indices, const Value<H> **data) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (indptr) *indptr = m->indptr;
    if (indices) *indices = m->indices;
    if (data) *data = m->data;
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_download(const H *m, void *indptr, void *indices, Value<H> *data) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (indptr) SPRS_TRY(download_indices(indptr, m->indptr, m->outer() + 1, m->iptr_bytes, m->user_iptr_bytes()));
    if (indices && m->nnz) SPRS_TRY(download_indices(indices, m->indices, m->nnz, m->idx_bytes, m->user_idx_bytes()));
    if (data && m->nnz) SPRS_TRY_HIP(copy_to_host(data, m->data, m->nnz * sizeof(Value<H>), nullptr));
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_refresh(H *m) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    SPRS_TRY_HIP(hipDeviceSynchronize());     // nothing in flight may still read the plan copies or the CSR copy
    std::lock_guard<std::recursive_mutex> lock(m->mu);
    invalidate_caches(m);
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_transpose_view(const H *m, H **out) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = view_csmat(m, true);
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_free(H *m) {
    clear_error();
    delete m;
    return SPRS_HIP_OK;
}

// ---- products with dense operands: the storage dispatch of the reference below the ABI -----------------------------------------
// The CSR form of a handle: itself, or — for a CSC handle — its to_other_storage() copy (csmat.rs:1405-1426), made once and kept
// IN THE HANDLE (as_other): every later product of the same CSC matrix reuses it, from any host language.  The reference walks a
// CSC matrix column by column and scatters (prod.rs:74-99, 219-270): every result element receives its products by ascending
// column index, which is the order of the CSR kernels on the converted matrix.
template <typename H>
static int32_t other_form(const H *m, H **out) {
    auto *mm = const_cast<H *>(m);
    std::lock_guard<std::recursive_mutex> lock(mm->mu);
    if (!mm->as_other) {
        Owned<H> other;
        SPRS_TRY(to_other_storage(m, other));
        mm->as_other = other.release();
        // the plan policy (prepare flag, multiplies so far) is the OWNER's: a copy rebuilt after a refresh keeps it
        mm->as_other->prepared = mm->prepared;
        copy_spmv_calls(mm->as_other, mm);
    }
    *out = mm->as_other;
    return SPRS_HIP_OK;
}
template <typename H>
static int32_t csr_form(const H *m, H **out) {
    if (m->storage == SPRS_HIP_CSR) {
        *out = const_cast<H *>(m);
        return SPRS_HIP_OK;
    }
    return other_form(m, out);
}

template <typename H>
static int32_t entry_prepare(H *m, void *stream) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    H *csr = nullptr;
    {
        std::lock_guard<std::recursive_mutex> lock(m->mu);
        m->prepared = true;                    // kept on the handle the caller holds: survives a refresh of a CSC handle's CSR copy
    }
    SPRS_TRY(csr_form(m, &csr));               // a CSC handle multiplies through its CSR copy: that is the handle to prepare
    return spmv_prepare(csr, (hipStream_t)stream);
}

template <typename T>
static int32_t vec_args_ok(const T *x_dev, uint64_t x_len, T *y_dev, uint64_t y_len) {
    if ((x_len && !x_dev) || (y_len && !y_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    // &mut res_vec cannot alias &in_vec in the reference; here the kernels read x while they write y
    if (x_len && y_len && x_dev < y_dev + y_len && y_dev < x_dev + x_len)
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "the result vector overlaps the input vector");
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_spmv(const H *a, const Value<H> *x_dev, uint64_t x_len, Value<H> *y_dev, uint64_t y_len, int32_t accumulate, void *stream) {
    clear_error();
    if (!a) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    // prod.rs:114-118: dimension check first, then storage
    if (a->cols != x_len || a->rows != y_len) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (a->storage != SPRS_HIP_CSR) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    SPRS_TRY(vec_args_ok(x_dev, x_len, y_dev, y_len));
    return spmv(const_cast<H *>(a), x_dev, y_dev, accumulate != 0, (hipStream_t)stream);
}

// a multiply of either storage through the CSR form; a CSC owner takes the multiply count of its CSR copy back
template <typename H>
static int32_t spmv_csr_form(const H *a, const Value<H> *x_dev, Value<H> *y_dev, bool accumulate, void *stream) {
    H *csr = nullptr;
    SPRS_TRY(csr_form(a, &csr));
    const int32_t st = spmv(csr, x_dev, y_dev, accumulate, (hipStream_t)stream);
    if (csr != a) copy_spmv_calls(const_cast<H *>(a), csr);
    return st;
}

template <typename H>
static int32_t entry_mul_acc_mat_vec_csc(const H *a, const Value<H> *x_dev, uint64_t x_len, Value<H> *y_dev, uint64_t y_len, void *stream) {
    clear_error();
    if (!a) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    // prod.rs:88-92: dimensions first, then storage
    if (a->cols != x_len || a->rows != y_len) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (a->storage != SPRS_HIP_CSC) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    SPRS_TRY(vec_args_ok(x_dev, x_len, y_dev, y_len));
    return spmv_csr_form(a, x_dev, y_dev, true, stream);
}

template <typename H>
static int32_t entry_csmat_mul_vec(const H *a, const Value<H> *x_dev, uint64_t x_len, Value<H> *y_dev, uint64_t y_len, void *stream) {
    clear_error();
    if (!a) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    // csmat.rs:2119-2160 -> csr_/csc_mulacc_dense_colmaj with one column (prod.rs:284-289 / 257-259: "Dimension mismatch")
    if (a->cols != x_len || a->rows != y_len) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    SPRS_TRY(vec_args_ok(x_dev, x_len, y_dev, y_len));
    return spmv_csr_form(a, x_dev, y_dev, false, stream);
}

template <typename H>
static int32_t entry_spmm_rowmaj(const H *a, const Value<H> *rhs_dev, uint64_t rhs_rows, uint64_t k, uint64_t ld_rhs, Value<H> *out_dev,
                                 uint64_t out_rows, uint64_t ld_out, int32_t accumulate, void *stream) {
    clear_error();
    if (!a) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    // prod.rs:199-202: three dimension asserts, then storage
    if (a->cols != rhs_rows || a->rows != out_rows) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (a->storage != SPRS_HIP_CSR) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    if (ld_rhs < k || ld_out < k) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "leading dimension smaller than the column count");
    if (k && ((rhs_rows && !rhs_dev) || (out_rows && !out_dev))) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL matrix");
    return spmm_strided(const_cast<H *>(a), rhs_dev, k, ld_rhs, 1, out_dev, ld_out, 1, accumulate != 0, (hipStream_t)stream);
}

template <typename H>
static int32_t entry_mulacc_dense(const H *lhs, const Value<H> *rhs_dev, uint64_t rhs_rows, uint64_t k, int32_t rhs_layout, uint64_t ld_rhs,
                                  Value<H> *out_dev, uint64_t out_rows, int32_t out_layout, uint64_t ld_out, int32_t accumulate, void *stream) {
    clear_error();
    if (!lhs) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if ((rhs_layout != SPRS_HIP_ROW_MAJOR && rhs_layout != SPRS_HIP_COL_MAJOR) || (out_layout != SPRS_HIP_ROW_MAJOR && out_layout != SPRS_HIP_COL_MAJOR))
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "bad layout tag");
    // prod.rs:199-201, 228-230, 257-259, 284-289: the three dimension asserts of the four dense kernels (the column counts of rhs
    // and out are one argument here)
    if (lhs->cols != rhs_rows || lhs->rows != out_rows) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (ld_rhs < (rhs_layout == SPRS_HIP_ROW_MAJOR ? k : rhs_rows) || ld_out < (out_layout == SPRS_HIP_ROW_MAJOR ? k : out_rows))
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "leading dimension smaller than the extent it strides over");
    if (k && ((rhs_rows && !rhs_dev) || (out_rows && !out_dev))) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL matrix");
    if (k && rhs_rows && out_rows) {   // the two operands must not share an ELEMENT (as vec_args_ok for the vectors)
        const uint64_t span_r = (rhs_layout == SPRS_HIP_ROW_MAJOR ? rhs_rows - 1 : k - 1) * ld_rhs + (rhs_layout == SPRS_HIP_ROW_MAJOR ? k : rhs_rows);
        const uint64_t span_o = (out_layout == SPRS_HIP_ROW_MAJOR ? out_rows - 1 : k - 1) * ld_out + (out_layout == SPRS_HIP_ROW_MAJOR ? k : out_rows);
        if (rhs_dev < out_dev + span_o && out_dev < rhs_dev + span_r) {
            // the strided spans meet.  Two views of ONE buffer with the same layout and pitch — rhs = buf[:, 0:k], out = buf[:, k:2k],
            // or the same as column blocks; ndarray views the reference accepts — are still element-disjoint when the lines of one
            // fall into the gaps of the other: the offset between them, modulo the pitch, leaves both line extents apart.
            bool disjoint = false;
            if (rhs_layout == out_layout && ld_rhs == ld_out) {
                const uint64_t w_r = rhs_layout == SPRS_HIP_ROW_MAJOR ? k : rhs_rows, w_o = out_layout == SPRS_HIP_ROW_MAJOR ? k : out_rows;
                const uint64_t d = rhs_dev <= out_dev ? (uint64_t)(out_dev - rhs_dev) % ld_rhs : (ld_rhs - (uint64_t)(rhs_dev - out_dev) % ld_rhs) % ld_rhs;
                // inside one pitch: rhs lines occupy [0, w_r), out lines [d, d + w_o)
                disjoint = d >= w_r && d + w_o <= ld_rhs;
            }
            if (!disjoint) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "the result matrix overlaps the right-hand side");
        }
    }
    H *csr = nullptr;
    SPRS_TRY(csr_form(lhs, &csr));
    hipStream_t st = (hipStream_t)stream;
    if (rhs_layout == SPRS_HIP_COL_MAJOR && out_layout == SPRS_HIP_COL_MAJOR && k < 8) {
        // the shape `&CsMat * &Array2` gives csr_mulacc_dense_colmaj (fewer than 8 columns, csmat.rs:2002-2016): column by column
        // through the SpMV — a column of a column-major rhs is a separate line per entry, so the SpMM kernel would issue k gathers
        // per entry where it issues one for a row-major rhs (k x 5.5 ms against k x 1.04 ms of the banded f64 SpMV)
        for (uint64_t j = 0; j < k; ++j) SPRS_TRY(spmv(csr, rhs_dev + j * ld_rhs, out_dev + j * ld_out, accumulate != 0, st));
        return SPRS_HIP_OK;
    }
    const uint64_t rs_r = rhs_layout == SPRS_HIP_ROW_MAJOR ? ld_rhs : 1, cs_r = rhs_layout == SPRS_HIP_ROW_MAJOR ? 1 : ld_rhs;
    const uint64_t rs_o = out_layout == SPRS_HIP_ROW_MAJOR ? ld_out : 1, cs_o = out_layout == SPRS_HIP_ROW_MAJOR ? 1 : ld_out;
    return spmm_strided(csr, rhs_dev, k, rs_r, cs_r, out_dev, rs_o, cs_o, accumulate != 0, st);
}

template <typename H>
static int32_t entry_mul_dense(const H *lhs, const Value<H> *rhs_dev, uint64_t rhs_rows, uint64_t k, int32_t rhs_layout, uint64_t ld_rhs,
                               Value<H> *out_dev, int32_t *out_layout, void *stream) {
    clear_error();
    if (!lhs || !out_layout) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    // csmat.rs:2002-2045: Array::zeros((rows, cols)) for >= 8 columns, Array::zeros((rows, cols).f()) below — in both storages
    const int32_t lay = k >= 8 ? SPRS_HIP_ROW_MAJOR : SPRS_HIP_COL_MAJOR;
    *out_layout = lay;
    return entry_mulacc_dense(lhs, rhs_dev, rhs_rows, k, rhs_layout, ld_rhs, out_dev, lhs->rows, lay, lay == SPRS_HIP_ROW_MAJOR ? k : lhs->rows, 0,
                              stream);
}

template <typename H>
static int32_t entry_dense_dot(const Value<H> *lhs_dev, uint64_t lhs_rows, uint64_t lhs_cols, int32_t lhs_layout, uint64_t ld_lhs, const H *rhs,
                               Value<H> *out_dev, int32_t *out_layout, void *stream) {
    clear_error();
    if (!rhs || !out_layout) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    if (lhs_layout != SPRS_HIP_ROW_MAJOR && lhs_layout != SPRS_HIP_COL_MAJOR) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "bad layout tag");
    // csmat.rs:2064-2117: (rhs^T * lhs^T)^T with free transposes — rhs.transpose_view(), lhs.t(), res.reversed_axes()
    // the CSR form of rhs^T: the transpose view of a CSC rhs, or of the (cached) CSC copy of a CSR rhs — either way a view.
    // The view stays in the rhs handle (beside as_other): its tile / band plans are built once, not per call.
    // The owner's lock is held until the product's kernels are launched: a concurrent refresh / numeric SpGEMM on rhs frees the
    // view in invalidate_caches (behind a device synchronise), and must not do so between the look-up and the launches.
    H *owner = const_cast<H *>(rhs);
    std::lock_guard<std::recursive_mutex> lock(owner->mu);
    if (!owner->t_view) {
        H *src = owner;
        if (rhs->storage == SPRS_HIP_CSR) SPRS_TRY(other_form(rhs, &src));
        owner->t_view = view_csmat(src, true);
    }
    int32_t lay_t = 0;
    // lhs^T: lhs_cols x lhs_rows, the other layout over the same memory
    const int32_t st = entry_mul_dense(owner->t_view, lhs_dev, lhs_cols, lhs_rows, lhs_layout == SPRS_HIP_ROW_MAJOR ? SPRS_HIP_COL_MAJOR : SPRS_HIP_ROW_MAJOR,
                                       ld_lhs, out_dev, &lay_t, stream);
    if (st != SPRS_HIP_OK) return st;
    *out_layout = lay_t == SPRS_HIP_ROW_MAJOR ? SPRS_HIP_COL_MAJOR : SPRS_HIP_ROW_MAJOR;     // reversed_axes()
    return SPRS_HIP_OK;
}

// tol and the threshold travel as doubles for both precisions; the solve, and the empty case below, compare in T
template <typename H>
static int32_t entry_bicgstab(H *a, const Value<H> *x0_dev, const Value<H> *b_dev, uint64_t n, double tol, uint64_t max_iter,
                              double soft_restart_threshold, Value<H> *x_dev, sprs_hip_bicgstab_info *info, void *stream) {
    using T = Value<H>;
    clear_error();
    if (!a) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (a->rows != a->cols || a->rows != n) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (n && (!x0_dev || !b_dev || !x_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    if (x_dev == x0_dev || x_dev == b_dev) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "x_dev may not alias x0_dev / b_dev");
    const T tol_t = (T)tol, threshold_t = (T)soft_restart_threshold;
    if (n == 0) {
        // what solve() does with empty vectors (bicgstab.rs:158-172): every norm is sqrt(0) = 0.  Without an iteration the loop
        // falls through to Err; otherwise the first step's err = 0 passes any tol > 0, the hard restart confirms it: Ok after
        // one iteration and one hard restart.  With tol <= 0 (or NaN) nothing passes and the iterations run out: Err.
        // (|rho| / err^2 = 0 / 0 is below no threshold: no soft restart.)
        const bool passes = max_iter > 0 && T(0) < tol_t;
        const uint64_t it = passes ? 1 : max_iter;
        if (info) *info = sprs_hip_bicgstab_info{it, 0, passes ? 1ull : 0ull, 0.0, 0.0, passes ? 1 : 0};
        return SPRS_HIP_OK;
    }
    return bicgstab(a, x0_dev, b_dev, n, tol_t, max_iter, threshold_t, x_dev, info, (hipStream_t)stream);
}

template <typename H>
static int32_t entry_gauss_seidel(H *a, Value<H> *x_dev, const Value<H> *rhs_dev, uint64_t n, uint64_t max_iter, double eps,
                                  sprs_hip_gauss_seidel_info *info, void *stream) {
    clear_error();
    if (!a) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (a->rows != a->cols || a->rows != n) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");   // heat.rs:109-110
    if (a->storage != SPRS_HIP_CSR) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Gauss-Seidel sweeps the rows of a CSR matrix");
    if (n && (!x_dev || !rhs_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    if (x_dev && x_dev == rhs_dev) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "x_dev may not alias rhs_dev");
    return gauss_seidel(a, x_dev, rhs_dev, n, max_iter, eps, info, (hipStream_t)stream);
}

// The four dense-rhs solves of sprs::linalg::trisolve behind one entry: the handle's storage selects the CSR or CSC function, uplo
// lsolve or usolve.  A CSC handle is solved on its CSR form (the as_other copy above), where the row orders then live; a->mu is
// held for the whole (blocking) call, so a refresh on another thread cannot drop that copy under the solve.
template <typename H>
static int32_t entry_trisolve(H *a, int32_t uplo, Value<H> *x_dev, uint64_t n, sprs_hip_trisolve_info *info, void *stream) {
    clear_error();
    if (!a) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (uplo != SPRS_HIP_LOWER && uplo != SPRS_HIP_UPPER) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "uplo must be SPRS_HIP_LOWER or SPRS_HIP_UPPER");
    // check_solver_dimensions, trisolve.rs:10-21
    if (a->rows != a->cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Non square matrix passed to solver");
    if (a->cols != n) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (n && !x_dev) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    if (n >= (1ull << 32)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "triangular solve: 2^32 rows or more are not supported");
    if (info) *info = sprs_hip_trisolve_info{0, UINT64_MAX, 0};
    if (n == 0) return SPRS_HIP_OK;
    std::lock_guard<std::recursive_mutex> lock(a->mu);
    H *csr = nullptr;
    SPRS_TRY(csr_form(a, &csr));
    return trisolve(csr, uplo == SPRS_HIP_UPPER, a->storage == SPRS_HIP_CSC, x_dev, n, info, (hipStream_t)stream);
}

template <typename T>
static int32_t entry_diag_solve(const T *d_dev, T *x_dev, uint64_t n, void *stream) {
    clear_error();
    if (n && (!d_dev || !x_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    return diag_solve(d_dev, x_dev, n, (hipStream_t)stream);
}

extern "C" {

const char *sprs_hip_last_error(void) { return tl_msg.c_str(); }
int32_t sprs_hip_last_hip_code(void) { return tl_hip_code; }
const char *sprs_hip_version(void) { return "sprs_hip 0.1.0 gfx950 (twin of sprs 0.11.5 prod/smmp)"; }

int32_t sprs_hip_device_count(int32_t *count) {
    clear_error();
    if (!count) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail_hip(e, "hipGetDeviceCount");
    }
    *count = n;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_set_device(int32_t device) {
    clear_error();
    SPRS_TRY_HIP(hipSetDevice(device));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_malloc(void **dev_ptr, uint64_t bytes) {
    clear_error();
    if (!dev_ptr) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "dev_ptr is NULL");
    *dev_ptr = nullptr;
    SPRS_TRY_HIP(hipMalloc(dev_ptr, bytes ? bytes : 8));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_free(void *dev_ptr) {
    clear_error();
    if (dev_ptr) SPRS_TRY_HIP(hipFree(dev_ptr));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_memcpy_h2d(void *dev_dst, const void *host_src, uint64_t bytes) {
    clear_error();
    if (bytes) SPRS_TRY_HIP(copy_to_device(dev_dst, host_src, bytes, nullptr));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_memcpy_d2h(void *host_dst, const void *dev_src, uint64_t bytes) {
    clear_error();
    if (bytes) SPRS_TRY_HIP(copy_to_host(host_dst, dev_src, bytes, nullptr));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_memcpy_d2d(void *dev_dst, const void *dev_src, uint64_t bytes, void *stream) {
    clear_error();
    if (bytes) SPRS_TRY_HIP(hipMemcpyAsync(dev_dst, dev_src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_memset(void *dev_dst, int32_t byte_value, uint64_t bytes, void *stream) {
    clear_error();
    if (bytes) SPRS_TRY_HIP(hipMemsetAsync(dev_dst, byte_value, bytes, (hipStream_t)stream));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_pool_trim(uint64_t *freed_bytes) {
    clear_error();
    const uint64_t f = pool_trim();
    if (freed_bytes) *freed_bytes = f;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_synchronize(void *stream) {
    clear_error();
    if (stream) SPRS_TRY_HIP(hipStreamSynchronize((hipStream_t)stream));
    else SPRS_TRY_HIP(hipDeviceSynchronize());
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csmat_upload(sprs_hip_csmat **out, int32_t storage, uint64_t rows, uint64_t cols,
                              const void *indptr, int32_t iptr_bytes, const void *indices,
                              int32_t idx_bytes, const double *data, int32_t validate) {
    return entry_upload(out, storage, rows, cols, indptr, iptr_bytes, indices, idx_bytes, data, validate);
}

int32_t sprs_hip_csmat_wrap_device(sprs_hip_csmat **out, int32_t storage, uint64_t rows,
                                   uint64_t cols, uint64_t nnz, const void *dev_indptr,
                                   int32_t iptr_bytes, const void *dev_indices, int32_t idx_bytes,
                                   const double *dev_data) {
    return entry_wrap_device(out, storage, rows, cols, nnz, dev_indptr, iptr_bytes, dev_indices, idx_bytes, dev_data);
}

int32_t sprs_hip_csmat_info(const sprs_hip_csmat *m, uint64_t *rows, uint64_t *cols, uint64_t *nnz,
                            int32_t *iptr_bytes, int32_t *idx_bytes, int32_t *storage) {
    return entry_info(m, rows, cols, nnz, iptr_bytes, idx_bytes, storage);
}

int32_t sprs_hip_csmat_device_ptrs(const sprs_hip_csmat *m, const void **indptr,
                                   const void **indices, const double **data) {
    return entry_device_ptrs(m, indptr, indices, data);
}

int32_t sprs_hip_csmat_download(const sprs_hip_csmat *m, void *indptr, void *indices, double *data) {
    return entry_download(m, indptr, indices, data);
}

int32_t sprs_hip_csmat_download_outer(const sprs_hip_csmat *m, uint64_t start, uint64_t end,
                                      void *indptr_out, void *indices_out, double *data_out,
                                      uint64_t *nnz_out) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    // Range checks of slice_outer (sprs/src/sparse/slicing.rs:65-89 -> range.rs)
    if (start > end || end > m->outer()) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "slice_outer range out of bounds");
    uint64_t lo = 0, hi = 0;
    const uint64_t pb = (uint64_t)m->iptr_bytes;
    if (pb == 8) {
        SPRS_TRY_HIP(copy_to_host(&lo, (const uint8_t *)m->indptr + start * pb, 8, nullptr));
        SPRS_TRY_HIP(copy_to_host(&hi, (const uint8_t *)m->indptr + end * pb, 8, nullptr));
    } else {
        uint32_t a = 0, b = 0;
        SPRS_TRY_HIP(copy_to_host(&a, (const uint8_t *)m->indptr + start * pb, 4, nullptr));
        SPRS_TRY_HIP(copy_to_host(&b, (const uint8_t *)m->indptr + end * pb, 4, nullptr));
        lo = a;
        hi = b;
    }
    if (nnz_out) *nnz_out = hi - lo;
    if (indptr_out) SPRS_TRY(download_indices(indptr_out, (const uint8_t *)m->indptr + start * pb, end - start + 1, m->iptr_bytes, m->user_iptr_bytes()));
    if (indices_out && hi > lo)
        SPRS_TRY(download_indices(indices_out, (const uint8_t *)m->indices + lo * (uint64_t)m->idx_bytes, hi - lo, m->idx_bytes, m->user_idx_bytes()));
    if (data_out && hi > lo) SPRS_TRY_HIP(copy_to_host(data_out, m->data + lo, (hi - lo) * sizeof(double), nullptr));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csmat_refresh(sprs_hip_csmat *m) {
    return entry_refresh(m);
}

int32_t sprs_hip_csmat_spmv_plan_info(const sprs_hip_csmat *m, int32_t *kind, uint64_t *plan_bytes) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    auto *mm = const_cast<sprs_hip_csmat *>(m);
    std::lock_guard<std::recursive_mutex> lock(mm->mu);
    const SpmvPlan &pl = m->plan;
    int32_t k = 0;
    uint64_t bytes = 0;
    if (pl.built) {
        if (pl.band) {
            k = 3;
            bytes = band_plan_bytes(pl.band.get());
        } else if (pl.xcs) {
            k = 2;
            bytes = pl.main.nnz * (8 + (uint64_t)pl.idx_bytes);
            for (const auto &sl : pl.slice) bytes += sl.nnz * (8 + (uint64_t)pl.idx_bytes) + (sl.rows + 1) * 8;
        } else {
            k = 1;
            bytes = (pl.main.ntiles + 1) * 8;
        }
    }
    if (kind) *kind = k;
    if (plan_bytes) *plan_bytes = bytes;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csmat_transpose_view(const sprs_hip_csmat *m, sprs_hip_csmat **out) {
    return entry_transpose_view(m, out);
}

int32_t sprs_hip_csmat_free(sprs_hip_csmat *m) {
    return entry_free(m);
}

int32_t sprs_hip_spmv_f64(const sprs_hip_csmat *a, const double *x_dev, uint64_t x_len,
                          double *y_dev, uint64_t y_len, int32_t accumulate, void *stream) {
    return entry_spmv(a, x_dev, x_len, y_dev, y_len, accumulate, stream);
}

int32_t sprs_hip_spmv_f64_host(uint64_t rows, uint64_t cols, const void *indptr,
                               int32_t iptr_bytes, const void *indices, int32_t idx_bytes,
                               const double *data, const double *x, uint64_t x_len, double *y,
                               uint64_t y_len, int32_t accumulate) {
    clear_error();
    if (cols != x_len || rows != y_len) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (!indptr) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    OwnedCsmat m;
    SPRS_TRY(csmat_upload(m, SPRS_HIP_CSR, rows, cols, indptr, iptr_bytes, indices, idx_bytes, data, 0));
    DevBuf dx, dy;
    SPRS_TRY_HIP(dx.alloc(x_len ? x_len * 8 : 8));
    SPRS_TRY_HIP(dy.alloc(y_len ? y_len * 8 : 8));
    SPRS_TRY(sprs_hip_memcpy_h2d(dx.p, x, x_len * 8));
    if (accumulate) SPRS_TRY(sprs_hip_memcpy_h2d(dy.p, y, y_len * 8));
    // one multiply, then the handle goes: nothing would amortise a re-laid-out copy of the matrix (the banded plan takes
    // ~0.1 s to build on R-MAT 10M for a 1 ms SpMV), so this entry multiplies on the plain nnz-tiled plan
    m->one_shot = true;
    SPRS_TRY(sprs_hip_spmv_f64(m.get(), dx.as<double>(), x_len, dy.as<double>(), y_len, accumulate, nullptr));
    SPRS_TRY(sprs_hip_synchronize(nullptr));
    return sprs_hip_memcpy_d2h(y, dy.p, y_len * 8);   // (the vectors and m go with this scope: releasing them leaves the error state alone)
}

int32_t sprs_hip_spmm_rowmaj_f64(const sprs_hip_csmat *a, const double *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                 uint64_t ld_rhs, double *out_dev, uint64_t out_rows, uint64_t ld_out,
                                 int32_t accumulate, void *stream) {
    return entry_spmm_rowmaj(a, rhs_dev, rhs_rows, k, ld_rhs, out_dev, out_rows, ld_out, accumulate, stream);
}

}  // extern "C"

// ---- SpGEMM: one body per entry for both handle types ----------------------------------------------------------------------
template <typename H>
static int32_t spgemm_contract(const H *a, const H *b) {
    if (a->cols != b->rows) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");   // smmp.rs:207
    if (a->storage != SPRS_HIP_CSR || b->storage != SPRS_HIP_CSR) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    if (a->user_iptr_bytes() != b->user_iptr_bytes() || a->user_idx_bytes() != b->user_idx_bytes())
        SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "operands must share index types (smmp.rs:196-199)");
    return SPRS_HIP_OK;
}

// C as the target of a numeric phase: the asserts of numeric() on its shape (smmp.rs:161-166); then, under C's lock (which
// the caller holds until the kernels are launched), everything derived from its values goes
template <typename H>
static int32_t numeric_target(const H *a, const H *b, H *c) {
    if (c->rows != a->rows || c->cols != b->cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (c->storage != SPRS_HIP_CSR) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    if (c->user_iptr_bytes() != a->user_iptr_bytes() || c->user_idx_bytes() != a->user_idx_bytes())
        SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "C must share the operands' index types");
    SPRS_TRY_HIP(hipDeviceSynchronize());   // nothing in flight may still read the copies that go away
    invalidate_caches(c);                   // values are about to change: plans copy them, and so does the copy in the other storage order
    return SPRS_HIP_OK;
}

// the ABI boundary of a product for either handle type: the f64 result takes its operand's declared widths (and their overflow
// checks); an f32 handle declares none (its arrays are 4 or 8 bytes wide on the host as on the device)
static int32_t finish_product(OwnedCsmat &res, const sprs_hip_csmat *from, sprs_hip_csmat **out) { return finish_result(res, from, out); }
static int32_t finish_product(OwnedCsmatF32 &res, const sprs_hip_csmat_f32 *, sprs_hip_csmat_f32 **out) {
    *out = res.release();
    return SPRS_HIP_OK;
}

template <typename H>
static int32_t entry_spgemm(const H *a, const H *b, H **c) {
    clear_error();
    if (!a || !b || !c) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *c = nullptr;
    SPRS_TRY(spgemm_contract(a, b));
    Owned<H> res;
    SPRS_TRY(spgemm_product(a, b, res));
    return finish_product(res, a, c);
}

template <typename H>
static int32_t entry_spgemm_symbolic(const H *a, const H *b, H **c) {
    clear_error();
    if (!a || !b || !c) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *c = nullptr;
    SPRS_TRY(spgemm_contract(a, b));
    Owned<H> res;
    SPRS_TRY(spgemm_symbolic(a, b, res));
    return finish_product(res, a, c);
}

template <typename H>
static int32_t entry_spgemm_numeric(const H *a, const H *b, H *c) {
    clear_error();
    if (!a || !b || !c) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    SPRS_TRY(spgemm_contract(a, b));
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    SPRS_TRY(numeric_target(a, b, c));
    return spgemm_numeric(a, b, c);
}

template <typename H>
static int32_t entry_spgemm_plan_create(const H *a, const H *b, sprs_hip_spgemm_plan **plan) {
    clear_error();
    if (!a || !b || !plan) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *plan = nullptr;
    SPRS_TRY(spgemm_contract(a, b));
    return spgemm_plan_create(a, b, plan);
}

template <typename H>
static int32_t entry_spgemm_plan_structure(sprs_hip_spgemm_plan *plan, const H *a, const H *b, H **c, bool with_values) {
    clear_error();
    if (!plan || !a || !b || !c) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *c = nullptr;
    Owned<H> res;
    SPRS_TRY(spgemm_plan_structure(plan, a, b, res, with_values));
    return finish_product(res, a, c);
}

template <typename H>
static int32_t entry_spgemm_plan_numeric(sprs_hip_spgemm_plan *plan, const H *a, const H *b, H *c) {
    clear_error();
    if (!plan || !a || !b || !c) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    SPRS_TRY(numeric_target(a, b, c));
    return spgemm_plan_numeric(plan, a, b, c);
}

// to_other_storage with the index-type check of the reference on the DECLARED widths (csmat.rs:1794-1797)
static int32_t convert_checked(const sprs_hip_csmat *m, OwnedCsmat &out) {
    if (m->rows > width_max(m->user_idx_bytes()))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the number of rows requested (required %llu)",
                  (unsigned long long)m->rows);
    SPRS_TRY(to_other_storage(m, out));
    return inherit_declared_widths(out.get(), m);
}
static int32_t convert_checked(const sprs_hip_csmat_f32 *m, OwnedCsmatF32 &out) {
    if (m->rows > width_max(m->idx_bytes))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the number of rows requested (required %llu)",
                  (unsigned long long)m->rows);
    return to_other_storage(m, out);
}

// `&lhs * &rhs` for two sparse matrices: csmat_mul_csmat (csmat.rs:1895-1949) — the storage dispatch around
// smmp::mul_csr_csr; the result has the storage of the lhs.
template <typename H>
static int32_t entry_csmat_mul_csmat(const H *lhs, const H *rhs, H **out) {
    clear_error();
    if (!lhs || !rhs || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (lhs->cols != rhs->rows) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (lhs->user_iptr_bytes() != rhs->user_iptr_bytes() || lhs->user_idx_bytes() != rhs->user_idx_bytes())
        SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "operands must share index types (smmp.rs:196-199)");
    const bool l_csr = lhs->storage == SPRS_HIP_CSR, r_csr = rhs->storage == SPRS_HIP_CSR;
    Owned<H> conv, c;                                             // rhs.to_other_storage() where the storages call for it; the product
    if (l_csr) {                                                  // (CSR, CSR) and (CSR, CSC)
        if (!r_csr) SPRS_TRY(convert_checked(rhs, conv));
        SPRS_TRY(spgemm_product(lhs, r_csr ? rhs : conv.get(), c));
        return finish_product(c, lhs, out);
    }
    // lhs is CSC: (rhs^T * lhs^T)^T on the transpose views (csmat.rs:982-991), which are CSR; transpose_into flips the result back
    if (r_csr) SPRS_TRY(convert_checked(rhs, conv));              // (CSC, CSR): rhs.to_other_storage() first
    H rt, lt;                                                     // stack views: their destructors find no plan and no block to release
    view_csmat(r_csr ? conv.get() : rhs, true, &rt);
    view_csmat(lhs, true, &lt);
    SPRS_TRY(spgemm_product(&rt, &lt, c));
    c->storage = SPRS_HIP_CSC;                                    // transpose_into: same buffers, other tag
    std::swap(c->rows, c->cols);
    return finish_product(c, lhs, out);
}

extern "C" {

int32_t sprs_hip_spgemm_symbolic(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat **c) {
    return entry_spgemm_symbolic(a, b, c);
}

int32_t sprs_hip_spgemm_numeric(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat *c) {
    return entry_spgemm_numeric(a, b, c);
}

int32_t sprs_hip_spgemm_plan_create(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_spgemm_plan **plan) {
    return entry_spgemm_plan_create(a, b, plan);
}

int32_t sprs_hip_spgemm_plan_nnz(const sprs_hip_spgemm_plan *plan, uint64_t *nnz) {
    clear_error();
    if (!plan || !nnz) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *nnz = spgemm_plan_nnz(plan);
    return SPRS_HIP_OK;
}

int32_t sprs_hip_spgemm_plan_structure(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat *a, const sprs_hip_csmat *b,
                                       sprs_hip_csmat **c_structure) {
    return entry_spgemm_plan_structure(plan, a, b, c_structure, false);
}

int32_t sprs_hip_spgemm_plan_product(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat *a, const sprs_hip_csmat *b,
                                     sprs_hip_csmat **c) {
    return entry_spgemm_plan_structure(plan, a, b, c, true);
}

int32_t sprs_hip_spgemm_plan_numeric(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat *a, const sprs_hip_csmat *b,
                                     sprs_hip_csmat *c) {
    return entry_spgemm_plan_numeric(plan, a, b, c);
}

int32_t sprs_hip_spgemm_plan_free(sprs_hip_spgemm_plan *plan) {
    clear_error();
    spgemm_plan_free(plan);
    return SPRS_HIP_OK;
}

int32_t sprs_hip_bicgstab_f64(sprs_hip_csmat *a, const double *x0_dev, const double *b_dev, uint64_t n, double tol,
                              uint64_t max_iter, double soft_restart_threshold, double *x_dev,
                              sprs_hip_bicgstab_info *info, void *stream) {
    return entry_bicgstab(a, x0_dev, b_dev, n, tol, max_iter, soft_restart_threshold, x_dev, info, stream);
}

int32_t sprs_hip_gauss_seidel_f64(sprs_hip_csmat *a, double *x_dev, const double *rhs_dev, uint64_t n, uint64_t max_iter,
                                  double eps, sprs_hip_gauss_seidel_info *info, void *stream) {
    return entry_gauss_seidel(a, x_dev, rhs_dev, n, max_iter, eps, info, stream);
}

int32_t sprs_hip_spgemm_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat **c) {
    return entry_spgemm(a, b, c);
}

int32_t sprs_hip_csmat_to_other_storage(const sprs_hip_csmat *m, sprs_hip_csmat **out) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsmat res;
    SPRS_TRY(convert_checked(m, res));
    *out = res.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csmat_mul_csmat(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, sprs_hip_csmat **out) {
    return entry_csmat_mul_csmat(lhs, rhs, out);
}

int32_t sprs_hip_csmat_slice_outer(const sprs_hip_csmat *m, uint64_t start, uint64_t end, sprs_hip_csmat **out) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (start > end || end > m->outer()) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "slice_outer range out of bounds");
    OwnedCsmat res;
    SPRS_TRY(slice_outer(m, start, end, res));
    return finish_result(res, m, out);
}

int32_t sprs_hip_dist_unique_id(void *id_128_bytes) {
    clear_error();
    if (!id_128_bytes) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    return dist_unique_id(id_128_bytes);
}

int32_t sprs_hip_dist_create(sprs_hip_dist **d, const void *id_128_bytes, int32_t world, int32_t rank, uint64_t rows,
                             uint64_t cols, const uint64_t *row_starts, const sprs_hip_csmat *local_block, int32_t nsub) {
    clear_error();
    if (!d || !row_starts || !local_block) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");   // (no id with world > 1: a handle for the peer route only)
    *d = nullptr;
    return dist_create(d, id_128_bytes, world, rank, rows, cols, row_starts, local_block, nsub);
}

int32_t sprs_hip_dist_spmv_f64(sprs_hip_dist *d, const double *x_dev, uint64_t x_len, double *y_dev, uint64_t y_len, void *stream) {
    clear_error();
    if (!d) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (dist_cols(d) != x_len || dist_rows(d) != y_len) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if ((x_len && !x_dev) || (y_len && !y_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    return dist_spmv(d, x_dev, y_dev, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_prepare(sprs_hip_csmat *m, void *stream) {
    return entry_prepare(m, stream);
}

int32_t sprs_hip_trisolve_f64(sprs_hip_csmat *a, int32_t uplo, double *x_dev, uint64_t n, sprs_hip_trisolve_info *info, void *stream) {
    return entry_trisolve(a, uplo, x_dev, n, info, stream);
}

// lsolve_csc_sparse_rhs (trisolve.rs:286-358): the reach over l's own columns, the solve on its CSR form (where the level plan
// and the scratch live).  l->mu is held for the whole (blocking) call, like above.
int32_t sprs_hip_lsolve_csc_sparse_rhs_f64(sprs_hip_csmat *l, const sprs_hip_csvec *rhs, sprs_hip_csvec **out, sprs_hip_sptrisolve_info *info,
                                           void *stream) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (!l || !rhs) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (l->storage != SPRS_HIP_CSC) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "Storage mismatch");       // trisolve.rs:301
    if (l->rows != l->cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Non square matrix passed to solver");
    const uint64_t n = l->rows;
    if (rhs->dim != n) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (n >= (1ull << 32)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "triangular solve: 2^32 rows or more are not supported");
    if (info) *info = sprs_hip_sptrisolve_info{0, 0, 0, 0, UINT64_MAX, 0};
    // the result carries l's index type: its dimension must be representable there (I::from(n), vec.rs:446-451)
    if (n > width_max(l->user_idx_bytes())) SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index size is too small");
    OwnedCsvec res;
    if (n == 0 || rhs->nnz == 0) {
        SPRS_TRY(make_csvec(res, n, 0, l->idx_bytes, l->user_idx_bytes()));
    } else {
        std::lock_guard<std::recursive_mutex> lock(l->mu);
        sprs_hip_csmat *csr = nullptr;
        SPRS_TRY(csr_form(l, &csr));
        SPRS_TRY(sptrisolve_f64(l, csr, rhs, res, info, (hipStream_t)stream));
    }
    *out = res.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_mul_acc_mat_vec_csc_f64(const sprs_hip_csmat *a, const double *x_dev, uint64_t x_len, double *y_dev,
                                         uint64_t y_len, void *stream) {
    return entry_mul_acc_mat_vec_csc(a, x_dev, x_len, y_dev, y_len, stream);
}

int32_t sprs_hip_csmat_mul_vec_f64(const sprs_hip_csmat *a, const double *x_dev, uint64_t x_len, double *y_dev, uint64_t y_len,
                                   void *stream) {
    return entry_csmat_mul_vec(a, x_dev, x_len, y_dev, y_len, stream);
}

int32_t sprs_hip_csmat_mulacc_dense_f64(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                        int32_t rhs_layout, uint64_t ld_rhs, double *out_dev, uint64_t out_rows,
                                        int32_t out_layout, uint64_t ld_out, int32_t accumulate, void *stream) {
    return entry_mulacc_dense(lhs, rhs_dev, rhs_rows, k, rhs_layout, ld_rhs, out_dev, out_rows, out_layout, ld_out, accumulate, stream);
}

int32_t sprs_hip_csmat_mul_dense_f64(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                     int32_t rhs_layout, uint64_t ld_rhs, double *out_dev, int32_t *out_layout, void *stream) {
    return entry_mul_dense(lhs, rhs_dev, rhs_rows, k, rhs_layout, ld_rhs, out_dev, out_layout, stream);
}

int32_t sprs_hip_dense_dot_csmat_f64(const double *lhs_dev, uint64_t lhs_rows, uint64_t lhs_cols, int32_t lhs_layout, uint64_t ld_lhs,
                                     const sprs_hip_csmat *rhs, double *out_dev, int32_t *out_layout, void *stream) {
    return entry_dense_dot(lhs_dev, lhs_rows, lhs_cols, lhs_layout, ld_lhs, rhs, out_dev, out_layout, stream);
}

int32_t sprs_hip_dist_comm_count(const sprs_hip_dist *d, int32_t *ranks) {
    clear_error();
    if (!d || !ranks) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    return dist_comm_count(d, ranks);
}

int32_t sprs_hip_dist_peer_handle(sprs_hip_dist *d, void *handle_64_bytes) {
    clear_error();
    if (!d || !handle_64_bytes) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    return dist_peer_handle(d, handle_64_bytes);
}

int32_t sprs_hip_dist_peer_connect(sprs_hip_dist *d, const void *handles, int32_t world) {
    clear_error();
    if (!d || !handles) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    return dist_peer_connect(d, handles, world);
}

int32_t sprs_hip_dist_set_route(sprs_hip_dist *d, int32_t route) {
    clear_error();
    if (!d) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    return dist_set_route(d, route);
}

int32_t sprs_hip_dist_route(const sprs_hip_dist *d, int32_t *route) {
    clear_error();
    if (!d || !route) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    return dist_route(d, route);
}

int32_t sprs_hip_dist_free(sprs_hip_dist *d) {
    clear_error();
    dist_free(d);
    return SPRS_HIP_OK;
}

int32_t sprs_hip_triplets_to_cs(uint64_t rows, uint64_t cols, uint64_t n, const void *row_inds_dev, const void *col_inds_dev,
                                int32_t in_idx_bytes, const double *data_dev, int32_t storage, int32_t out_idx_bytes,
                                int32_t out_iptr_bytes, sprs_hip_csmat **out) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (storage != SPRS_HIP_CSR && storage != SPRS_HIP_CSC) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "bad storage tag %d", storage);
    if (!widths_ok(out_iptr_bytes, out_idx_bytes) || (in_idx_bytes != 4 && in_idx_bytes != 8))
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 4 or 8 bytes");
    if (n && (!row_inds_dev || !col_inds_dev || !data_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL triplet array with n > 0");
    const uint64_t inner = storage == SPRS_HIP_CSR ? cols : rows, outer = storage == SPRS_HIP_CSR ? rows : cols;
    if (out_idx_bytes == 4 && inner > 0xFFFFFFFFull) SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type not large enough for this matrix");
    if (out_iptr_bytes == 4 && outer + 1 > 0xFFFFFFFFull) SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Iptr type not large enough for this matrix");
    OwnedCsmat res;
    SPRS_TRY(triplets_to_cs(rows, cols, n, row_inds_dev, col_inds_dev, in_idx_bytes, data_dev, storage, out_idx_bytes, out_iptr_bytes, res));
    *out = res.release();
    return SPRS_HIP_OK;
}

namespace {
struct OptionDesc {
    const char *name;
    int64_t sprs_hip::Options::*field;
    int64_t lo, hi;
    bool devtools;
};
const OptionDesc kOptions[] = {
#define SPRS_X(name, def, lo, hi, dev) {#name, &sprs_hip::Options::name, (int64_t)(lo), (int64_t)(hi), (dev) != 0},
    SPRS_HIP_OPTIONS(SPRS_X)
#undef SPRS_X
};
const OptionDesc *find_option(const char *name) {
    for (const OptionDesc &d : kOptions)
        if (!strcmp(name, d.name)) return &d;
    return nullptr;
}
}  // namespace

int32_t sprs_hip_set_option(const char *name, int64_t value) {
    clear_error();
    if (!name) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL name");
    const OptionDesc *d = find_option(name);
    if (!d) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "unknown option '%s'", name);
    if (d->devtools && !DEVTOOLS)
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "option '%s' is a developer switch (wrong results / profiling printouts): this library was built without SPRS_HIP_DEVTOOLS", name);
    if (value < d->lo || value > d->hi)
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "%s must be in %lld .. %lld", name, (long long)d->lo, (long long)d->hi);
    // the few options whose legal values are not a range
    if (!strcmp(name, "spmv_tile") && value != 0 && value != 2048 && value != 4096) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "spmv_tile must be 0 (auto), 2048 or 4096");
    if (!strcmp(name, "spmv_band_tile") && value != 0 && value != 8192 && value != 16384) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "spmv_band_tile must be 0 (default), 8192 or 16384");
    if (!strcmp(name, "spmv_f32_band_tile") && value != 0 && value != 8192 && value != 16384 && value != 32768)
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "spmv_f32_band_tile must be 0 (default), 8192, 16384 or 32768");
    if (!strcmp(name, "spgemm_tokens") && value == 3) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "spgemm_tokens must be 1, 2 or 4");
    if (!strcmp(name, "spmv_band_split") && value == 1) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "spmv_band_split must be 0 (default) or >= 2");
    options().*(d->field) = value;
    if (!strcmp(name, "pool") && !value) (void)pool_trim();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_get_option(const char *name, int64_t *value) {
    clear_error();
    if (!name || !value) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    if (!strcmp(name, "pool_cached_bytes")) {
        *value = (int64_t)pool_cached_bytes();
        return SPRS_HIP_OK;
    }
    if (!strcmp(name, "spgemm_f32_lds_add")) {  // read-only: the verdict of the f32 probe of the LDS add on the current device (spgemm.hip)
        *value = spgemm_f32_lds_add_verdict();
        return SPRS_HIP_OK;
    }
    if (!strcmp(name, "devtools")) {           // 1 when the library was built with SPRS_HIP_DEVTOOLS
        *value = DEVTOOLS ? 1 : 0;
        return SPRS_HIP_OK;
    }
    const OptionDesc *d = find_option(name);
    if (!d) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "unknown option '%s'", name);
    *value = options().*(d->field);
    return SPRS_HIP_OK;
}

}  // extern "C"

// ---- device sparse vectors (CsVecBase, sparse.rs:165-173) and their products; kernels in csvec.hpp --------------------------

// CsVec::try_new (vec.rs:440-491) on host indices: sorted_indices (sparse.rs:360-369), then the last index against dim
template <typename I>
static int32_t check_csvec_host(uint64_t dim, uint64_t nnz, const I *idx) {
    for (uint64_t i = 1; i < nnz; ++i)
        if (idx[i] <= idx[i - 1]) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Unsorted indices");
    if (nnz && (uint64_t)idx[nnz - 1] >= dim) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "indices larger than vector size");
    return SPRS_HIP_OK;
}

// vectors up to this many entries are validated on the host; longer ones by csvec_check_kernel after the upload
static constexpr uint64_t CSVEC_HOST_CHECK_MAX = 1ull << 16;

extern "C" {

int32_t sprs_hip_csvec_upload(sprs_hip_csvec **out, uint64_t dim, uint64_t nnz, const void *indices, int32_t idx_bytes,
                              const double *data, int32_t validate) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (idx_bytes != 2 && idx_bytes != 4 && idx_bytes != 8) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 2, 4 or 8 bytes");
    if (nnz && (!indices || !data)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL indices/data with nnz > 0");
    if (validate) {
        // I::from(n) (vec.rs:446-451): the dimension itself must be representable
        if (dim > width_max(idx_bytes)) SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index size is too small");
        if (nnz <= CSVEC_HOST_CHECK_MAX) {
            SPRS_TRY(dispatch_host_width(idx_bytes, [&](auto t) { return check_csvec_host(dim, nnz, (const typename decltype(t)::type *)indices); }));
        }
    }
    const HostIndices ix(indices, nnz, idx_bytes);
    OwnedCsvec v;
    SPRS_TRY(make_csvec(v, dim, nnz, ix.bytes, idx_bytes));
    hipError_t e = ix.upload(v->indices, nnz);
    if (e == hipSuccess && nnz) e = copy_to_device(v->data, data, nnz * sizeof(double), nullptr);
    if (e != hipSuccess) return fail_hip(e, "csvec_upload");
    if (validate && nnz > CSVEC_HOST_CHECK_MAX) SPRS_TRY(csvec_check_device(v.get(), nullptr));
    *out = v.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csvec_wrap_device(sprs_hip_csvec **out, uint64_t dim, uint64_t nnz, const void *dev_indices, int32_t idx_bytes,
                                   const double *dev_data) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (idx_bytes != 4 && idx_bytes != 8) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 4 or 8 bytes");
    if (nnz && (!dev_indices || !dev_data)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL indices/data with nnz > 0");
    if (((uintptr_t)dev_indices % (uintptr_t)idx_bytes) | ((uintptr_t)dev_data & 7))
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "device buffers must be aligned to their element size");
    int device = 0;
    const hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
    *out = view_csvec(dim, nnz, dev_indices, idx_bytes, dev_data, device);
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csvec_info(const sprs_hip_csvec *v, uint64_t *dim, uint64_t *nnz, int32_t *idx_bytes) {
    clear_error();
    if (!v) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (dim) *dim = v->dim;
    if (nnz) *nnz = v->nnz;
    if (idx_bytes) *idx_bytes = v->user_idx_bytes();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csvec_device_ptrs(const sprs_hip_csvec *v, const void **indices, const double **data) {
    clear_error();
    if (!v) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (indices) *indices = v->indices;
    if (data) *data = v->data;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csvec_download(const sprs_hip_csvec *v, void *indices, double *data) {
    clear_error();
    if (!v) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (indices && v->nnz) SPRS_TRY(download_indices(indices, v->indices, v->nnz, v->idx_bytes, v->user_idx_bytes()));
    if (data && v->nnz) SPRS_TRY_HIP(copy_to_host(data, v->data, v->nnz * sizeof(double), nullptr));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csvec_free(sprs_hip_csvec *v) {
    clear_error();
    delete v;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csvec_scatter_f64(const sprs_hip_csvec *v, double *out_dev, uint64_t out_len, void *stream) {
    clear_error();
    if (!v) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (out_len != v->dim) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (out_len && !out_dev) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    return csvec_scatter(v, out_dev, (hipStream_t)stream);
}

// a vector result leaves its owner at the ABI boundary
static int32_t finish_csvec(int32_t status, OwnedCsvec &res, sprs_hip_csvec **out) {
    if (status == SPRS_HIP_OK) *out = res.release();
    return status;
}

// an empty result of dimension `dim` (no kernel)
static int32_t empty_csvec(sprs_hip_csvec **out, uint64_t dim, const sprs_hip_csmat *like) {
    OwnedCsvec res;
    return finish_csvec(make_csvec(res, dim, 0, like->idx_bytes, like->user_idx_bytes()), res, out);
}

int32_t sprs_hip_csmat_mul_csvec_f64(const sprs_hip_csmat *a, const sprs_hip_csvec *v, sprs_hip_csvec **out, void *stream) {
    clear_error();
    if (!a || !v || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsvec res;
    if (a->storage == SPRS_HIP_CSR) {
        if (v->dim == 0) return empty_csvec(out, 0, a);               // CsVecI::empty(0) (prod.rs:171-174)
        if (a->cols != v->dim) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");   // prod.rs:175
        return finish_csvec(csvec_masked_dot(a, v, true, a->idx_bytes, a->user_idx_bytes(), res, (hipStream_t)stream), res, out);
    }
    // CSC: a * v.col_view() (vec.rs:1127-1129) -> csmat_mul_csmat, structural, on the CSR form of a
    if (a->cols != v->dim) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (a->rows == 0 || v->nnz == 0 || a->nnz == 0) return empty_csvec(out, a->rows, a);
    sprs_hip_csmat *csr = nullptr;
    SPRS_TRY(other_form(a, &csr));
    return finish_csvec(csvec_masked_dot(csr, v, false, a->idx_bytes, a->user_idx_bytes(), res, (hipStream_t)stream), res, out);
}

int32_t sprs_hip_csvec_mul_csmat_f64(const sprs_hip_csvec *v, const sprs_hip_csmat *b, sprs_hip_csvec **out, void *stream) {
    clear_error();
    if (!v || !b || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    // (v.row_view() * b).outer_view(0) (vec.rs:1098-1100): mul_csr_csr asserts lhs.cols == rhs.rows
    if (v->dim != b->rows) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (b->cols == 0 || v->nnz == 0 || b->nnz == 0) return empty_csvec(out, b->cols, b);
    // entry o is the ordered dot of COLUMN o of b with v: b itself when CSC, its CSC form when CSR
    const sprs_hip_csmat *csc = b;
    if (b->storage == SPRS_HIP_CSR) {
        sprs_hip_csmat *c = nullptr;
        SPRS_TRY(other_form(b, &c));
        csc = c;
    }
    OwnedCsvec res;
    return finish_csvec(csvec_masked_dot(csc, v, false, b->idx_bytes, b->user_idx_bytes(), res, (hipStream_t)stream), res, out);
}

}  // extern "C"

// ---- sparse +, -, elementwise * and scale (binop.rs); kernels in binop.hpp -----------------------------------------------------

static int32_t binop_op_ok(int32_t op) {
    if (op != SPRS_HIP_BINOP_ADD && op != SPRS_HIP_BINOP_SUB && op != SPRS_HIP_BINOP_MUL)
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "op must be SPRS_HIP_BINOP_ADD, SPRS_HIP_BINOP_SUB or SPRS_HIP_BINOP_MUL");
    return SPRS_HIP_OK;
}

// csmat_binop's asserts (binop.rs:194-198) and the one I / Iptr of its signature
static int32_t binop_contract(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, bool same_storage) {
    if (lhs->rows != rhs->rows || lhs->cols != rhs->cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (same_storage && lhs->storage != rhs->storage) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    if (lhs->user_iptr_bytes() != rhs->user_iptr_bytes() || lhs->user_idx_bytes() != rhs->user_idx_bytes())
        SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "operands must share index types (binop.rs:178-182)");
    return SPRS_HIP_OK;
}

// `&lhs op &rhs` (binop.rs:52-64, 99-111): rhs.to_other_storage() first when the storages differ
static int32_t csmat_operator(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, int32_t op, sprs_hip_csmat **out, void *stream) {
    if (!lhs || !rhs || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    SPRS_TRY(binop_contract(lhs, rhs, false));
    OwnedCsmat conv, res;
    if (lhs->storage != rhs->storage) {
        // the conversion runs on the null stream: what the caller's stream still has to write into rhs comes first
        if (stream) SPRS_TRY_HIP(hipStreamSynchronize((hipStream_t)stream));
        SPRS_TRY(convert_checked(rhs, conv));
    }
    SPRS_TRY(csmat_binop_f64(lhs, conv ? conv.get() : rhs, op, res, (hipStream_t)stream));
    return finish_result(res, lhs, out);
}

extern "C" {

int32_t sprs_hip_csmat_binop_f64(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, int32_t op, sprs_hip_csmat **out, void *stream) {
    clear_error();
    SPRS_TRY(binop_op_ok(op));
    if (!lhs || !rhs || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    SPRS_TRY(binop_contract(lhs, rhs, true));
    OwnedCsmat res;
    SPRS_TRY(csmat_binop_f64(lhs, rhs, op, res, (hipStream_t)stream));
    return finish_result(res, lhs, out);
}

int32_t sprs_hip_csmat_add_csmat_f64(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, sprs_hip_csmat **out, void *stream) {
    clear_error();
    return csmat_operator(lhs, rhs, SPRS_HIP_BINOP_ADD, out, stream);
}

int32_t sprs_hip_csmat_sub_csmat_f64(const sprs_hip_csmat *lhs, const sprs_hip_csmat *rhs, sprs_hip_csmat **out, void *stream) {
    clear_error();
    return csmat_operator(lhs, rhs, SPRS_HIP_BINOP_SUB, out, stream);
}

int32_t sprs_hip_csmat_scale_f64(const sprs_hip_csmat *m, double alpha, sprs_hip_csmat **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsmat res;
    SPRS_TRY(csmat_scale_f64(m, alpha, res, (hipStream_t)stream));
    return finish_result(res, m, out);
}

int32_t sprs_hip_csvec_binop_f64(const sprs_hip_csvec *lhs, const sprs_hip_csvec *rhs, int32_t op, sprs_hip_csvec **out, void *stream) {
    clear_error();
    SPRS_TRY(binop_op_ok(op));
    if (!lhs || !rhs || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    // csvec_fix_zeros (binop.rs:469-479): a dimension of 0 takes the other operand's
    const uint64_t ldim = lhs->dim ? lhs->dim : rhs->dim, rdim = rhs->dim ? rhs->dim : lhs->dim;
    if (ldim != rdim) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (lhs->user_idx_bytes() != rhs->user_idx_bytes())
        SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "operands must share the index type (binop.rs:442-446)");
    OwnedCsvec res;
    return finish_csvec(csvec_binop_f64(lhs, rhs, op, ldim, res, (hipStream_t)stream), res, out);
}

}  // extern "C"

// ---- reductions and extraction (vec.rs:787-958, 1051-1061; prod.rs:14-70; csmat.rs:1017-1056, 1219-1256, 1312-1351);
// kernels in csvec_reduce.hpp and extract.hpp ------------------------------------------------------------------------------------

extern "C" {

int32_t sprs_hip_csvec_dot_f64(const sprs_hip_csvec *v, const sprs_hip_csvec *w, double *out_host, void *stream) {
    clear_error();
    if (!v || !w || !out_host) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    if (v->dim != w->dim) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");     // vec.rs:855
    return csvec_dot_f64(v, w, out_host, (hipStream_t)stream);
}

int32_t sprs_hip_csvec_dot_dense_f64(const sprs_hip_csvec *v, const double *x_dev, uint64_t x_len, double *out_host, void *stream) {
    clear_error();
    if (!v || !out_host) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    if (x_len != v->dim) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");      // vec.rs:855, 900
    if (x_len && !x_dev) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    return csvec_dot_dense_f64(v, x_dev, x_len, out_host, (hipStream_t)stream);
}

int32_t sprs_hip_csvec_norm_f64(const sprs_hip_csvec *v, int32_t kind, double p, double *out_host, void *stream) {
    clear_error();
    if (!v || !out_host) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    double sum = 0.0;
    switch (kind) {
    case SPRS_HIP_NORM_SQUARED_L2:
        return csvec_sum_f64(v, 0, 0.0, out_host, st);
    case SPRS_HIP_NORM_L2:
        SPRS_TRY(csvec_sum_f64(v, 0, 0.0, &sum, st));
        *out_host = std::sqrt(sum);
        return SPRS_HIP_OK;
    case SPRS_HIP_NORM_L1:
        return csvec_sum_f64(v, 1, 0.0, out_host, st);
    case SPRS_HIP_NORM_P:
        break;
    default:
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "kind must be SPRS_HIP_NORM_SQUARED_L2, SPRS_HIP_NORM_L2, SPRS_HIP_NORM_L1 or SPRS_HIP_NORM_P");
    }
    // norm(p), vec.rs:939-958
    if (std::isinf(p) || p == 0.0) {
        if (std::isinf(p) && v->nnz == 0) {
            *out_host = 0.0;
            return SPRS_HIP_OK;
        }
        double ext[3];
        SPRS_TRY(csvec_extrema_f64(v, ext, st));
        *out_host = p == 0.0 ? ext[2] : p > 0.0 ? ext[0] : ext[1];
        return SPRS_HIP_OK;
    }
    SPRS_TRY(csvec_sum_f64(v, 2, p, &sum, st));
    *out_host = std::pow(sum, 1.0 / p);                          // powf(p.powi(-1))
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csvec_unit_normalize_f64(const sprs_hip_csvec *v, sprs_hip_csvec **out, void *stream) {
    clear_error();
    if (!v || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    double norm_sq = 0.0;
    SPRS_TRY(csvec_sum_f64(v, 0, 0.0, &norm_sq, (hipStream_t)stream));
    OwnedCsvec res;
    return finish_csvec(csvec_divided_f64(v, norm_sq > 0.0 ? std::sqrt(norm_sq) : 0.0, res, (hipStream_t)stream), res, out);
}

int32_t sprs_hip_csvec_nnz_index(const sprs_hip_csvec *v, uint64_t nq, const uint64_t *q_dev, uint64_t *pos_dev, double *val_dev,
                                 void *stream) {
    clear_error();
    if (!v) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (nq && (!q_dev || !pos_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL query / position array with nq > 0");
    return csvec_lookup(v, nq, q_dev, pos_dev, val_dev, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_outer_view(const sprs_hip_csmat *m, uint64_t i, sprs_hip_csvec **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (i >= m->outer()) return SPRS_HIP_OK;                     // None (csmat.rs:1220-1222)
    return csmat_outer_view(m, i, out, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_diag_f64(const sprs_hip_csmat *m, sprs_hip_csvec **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsvec res;
    return finish_csvec(csmat_diag_f64(m, res, (hipStream_t)stream), res, out);
}

int32_t sprs_hip_csmat_nnz_index(const sprs_hip_csmat *m, uint64_t nq, const uint64_t *rows_dev, const uint64_t *cols_dev, uint64_t *pos_dev,
                                 double *val_dev, void *stream) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (nq && (!rows_dev || !cols_dev || !pos_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL query / position array with nq > 0");
    return csmat_lookup(m, nq, rows_dev, cols_dev, pos_dev, val_dev, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_to_inner_onehot_f64(const sprs_hip_csmat *m, sprs_hip_csmat **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsmat res;
    SPRS_TRY(csmat_onehot_f64(m, res, (hipStream_t)stream));
    return finish_result(res, m, out);
}

}  // extern "C"

// ---- permutations (permutation.rs); kernels in perm.hpp ----------------------------------------------------------------------

// perm_is_valid (permutation.rs:39-49) on a host array
template <typename I>
static bool perm_is_valid_host(uint64_t dim, const I *perm) {
    std::vector<bool> seen(dim, false);
    for (uint64_t i = 0; i < dim; ++i) {
        const uint64_t v = (uint64_t)perm[i];
        if (v >= dim || seen[v]) return false;
        seen[v] = true;
    }
    return true;
}

// permutations up to this many entries are validated on the host; longer ones on the device after the upload
static constexpr uint64_t PERM_HOST_CHECK_MAX = 1ull << 16;

// a handle whose perm array is already on the device: the inverse (and the validation), then it leaves its owner
static int32_t perm_finish(OwnedPerm &p, bool validate, hipStream_t stream, sprs_hip_perm **out) {
    SPRS_TRY(perm_build_inverse(p.get(), validate, stream));
    *out = p.release();
    return SPRS_HIP_OK;
}

// the array a side of the algorithm reads: null for "no permutation" and for the Identity variant
static const void *perm_array(const sprs_hip_perm *p, bool inverse) {
    if (!p || p->identity) return nullptr;
    return inverse ? p->perm_inv : p->perm;
}

// the reference's generics force one I on the matrix and its permutations
static int32_t perm_width_ok(const sprs_hip_csmat *m, const sprs_hip_perm *p) {
    if (p && p->user_idx_bytes() != m->user_idx_bytes())
        SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "the permutation must have the matrix's index type (permutation.rs:296-304)");
    return SPRS_HIP_OK;
}

extern "C" {

int32_t sprs_hip_perm_upload(sprs_hip_perm **out, uint64_t dim, const void *perm, int32_t idx_bytes, int32_t validate) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (idx_bytes != 2 && idx_bytes != 4 && idx_bytes != 8) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 2, 4 or 8 bytes");
    if (dim && !perm) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL perm with dim > 0");
    if (validate && dim <= PERM_HOST_CHECK_MAX) {
        const bool ok = dispatch_host_width(idx_bytes, [&](auto t) { return perm_is_valid_host(dim, (const typename decltype(t)::type *)perm); });
        if (!ok) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "invalid permutation");
    }
    const HostIndices host(perm, dim, idx_bytes);
    OwnedPerm p;
    SPRS_TRY(make_perm(p, dim, host.bytes, idx_bytes));
    const hipError_t e = host.upload(p->perm, dim);
    if (e != hipSuccess) return fail_hip(e, "perm_upload");
    return perm_finish(p, validate && dim > PERM_HOST_CHECK_MAX, nullptr, out);
}

int32_t sprs_hip_perm_from_device(sprs_hip_perm **out, uint64_t dim, const void *dev_perm, int32_t idx_bytes, int32_t validate,
                                  void *stream) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (idx_bytes != 4 && idx_bytes != 8) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 4 or 8 bytes");
    if (dim && !dev_perm) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL perm with dim > 0");
    if ((uintptr_t)dev_perm % (uintptr_t)idx_bytes) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "device buffers must be aligned to their element size");
    OwnedPerm p;
    SPRS_TRY(make_perm(p, dim, idx_bytes, idx_bytes));
    if (dim) {
        const hipError_t e = hipMemcpyAsync(p->perm, dev_perm, dim * (uint64_t)idx_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return fail_hip(e, "perm_from_device");
    }
    return perm_finish(p, validate != 0, (hipStream_t)stream, out);
}

int32_t sprs_hip_perm_identity(sprs_hip_perm **out, uint64_t dim, int32_t idx_bytes) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (idx_bytes != 2 && idx_bytes != 4 && idx_bytes != 8) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 2, 4 or 8 bytes");
    *out = identity_perm(dim, idx_bytes);
    return SPRS_HIP_OK;
}

int32_t sprs_hip_perm_info(const sprs_hip_perm *p, uint64_t *dim, int32_t *idx_bytes, int32_t *identity_variant) {
    clear_error();
    if (!p) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (dim) *dim = p->dim;
    if (idx_bytes) *idx_bytes = p->user_idx_bytes();
    if (identity_variant) *identity_variant = p->identity ? 1 : 0;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_perm_is_identity(const sprs_hip_perm *p, int32_t *flag, void *stream) {
    clear_error();
    if (!p || !flag) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    return perm_is_identity(p, flag, (hipStream_t)stream);
}

int32_t sprs_hip_perm_device_ptrs(const sprs_hip_perm *p, const void **perm, const void **perm_inv) {
    clear_error();
    if (!p) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (perm) *perm = p->identity ? nullptr : p->perm;
    if (perm_inv) *perm_inv = p->identity ? nullptr : p->perm_inv;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_perm_download(const sprs_hip_perm *p, void *perm, void *perm_inv) {
    clear_error();
    if (!p) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    void *dst[2] = {perm, perm_inv};
    const void *src[2] = {p->perm, p->perm_inv};
    for (int k = 0; k < 2; ++k) {
        if (!dst[k] || !p->dim) continue;
        if (!p->identity) {
            SPRS_TRY(download_indices(dst[k], src[k], p->dim, p->idx_bytes, p->user_idx_bytes()));
            continue;
        }
        const int32_t w = p->user_idx_bytes();      // (0..dim).collect() (permutation.rs:211-226)
        if (p->dim - 1 > width_max(w)) SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold %llu", (unsigned long long)(p->dim - 1));
        dispatch_host_width(w, [&](auto t) {
            using I = typename decltype(t)::type;
            for (uint64_t i = 0; i < p->dim; ++i) ((I *)dst[k])[i] = (I)i;
        });
    }
    return SPRS_HIP_OK;
}

int32_t sprs_hip_perm_inv(const sprs_hip_perm *p, sprs_hip_perm **out) {
    clear_error();
    if (!p || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (p->identity) {
        *out = identity_perm(p->dim, p->user_idx_bytes());
        return SPRS_HIP_OK;
    }
    OwnedPerm q;
    SPRS_TRY(make_perm(q, p->dim, p->idx_bytes, p->user_idx_bytes()));
    if (p->dim) {
        const uint64_t bytes = p->dim * (uint64_t)p->idx_bytes;
        hipError_t e = hipMemcpyAsync(q->perm, p->perm_inv, bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = hipMemcpyAsync(q->perm_inv, p->perm, bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return fail_hip(e, "perm_inv");
    }
    *out = q.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_perm_free(sprs_hip_perm *p) {
    clear_error();
    delete p;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_perm_mul_vec_f64(const sprs_hip_perm *p, const double *x_dev, double *y_dev, uint64_t n, void *stream) {
    clear_error();
    if (!p) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (n != p->dim) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (n && (!x_dev || !y_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    if (n && (uintptr_t)x_dev < (uintptr_t)(y_dev + n) && (uintptr_t)y_dev < (uintptr_t)(x_dev + n))
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "x and y must not overlap");
    return perm_mul_vec_f64(p, x_dev, y_dev, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_transform_paq(const sprs_hip_csmat *m, const sprs_hip_perm *row_perm, const sprs_hip_perm *col_perm,
                                     sprs_hip_csmat **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if ((row_perm && row_perm->dim != m->rows) || (col_perm && col_perm->dim != m->cols))
        SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");   // permutation.rs:506-507
    SPRS_TRY(perm_width_ok(m, row_perm));
    SPRS_TRY(perm_width_ok(m, col_perm));
    const bool csr = m->storage == SPRS_HIP_CSR, empty = m->rows == 0 || m->cols == 0;
    // CSR: (p, q_); CSC: (q, p_) (permutation.rs:544-547)
    const void *o = empty ? nullptr : perm_array(csr ? row_perm : col_perm, false);
    const void *g = empty ? nullptr : perm_array(csr ? col_perm : row_perm, true);
    OwnedCsmat res;
    SPRS_TRY(csmat_permute(m, o, g, res, (hipStream_t)stream));
    return finish_result(res, m, out);
}

int32_t sprs_hip_csmat_transform_papt(const sprs_hip_csmat *m, const sprs_hip_perm *p, sprs_hip_csmat **out, void *stream) {
    clear_error();
    if (!m || !p || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (m->rows != m->cols || m->rows != p->dim) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");   // permutation.rs:448-449
    SPRS_TRY(perm_width_ok(m, p));
    int32_t ident = 1;
    if (m->rows) SPRS_TRY(perm_is_identity(p, &ident, (hipStream_t)stream));   // perm.is_identity() || mat.rows() == 0 (permutation.rs:450)
    OwnedCsmat res;
    SPRS_TRY(csmat_permute(m, ident ? nullptr : p->perm, ident ? nullptr : p->perm_inv, res, (hipStream_t)stream));
    return finish_result(res, m, out);
}

}  // extern "C"

// ---- structure checks and unsorted input (sparse.rs:300-358, csmat.rs:311-401, vec.rs:536-557); kernels in structure.hpp -----

extern "C" {

int32_t sprs_hip_csmat_check_structure(const sprs_hip_csmat *m, sprs_hip_structure_info *info, void *stream) {
    clear_error();
    if (info) *info = sprs_hip_structure_info{0, 0, 0};
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    return csmat_check_structure(m, info, (hipStream_t)stream);
}

int32_t sprs_hip_csvec_check_structure(const sprs_hip_csvec *v, sprs_hip_structure_info *info, void *stream) {
    clear_error();
    if (info) *info = sprs_hip_structure_info{0, 0, 0};
    if (!v) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (v->dim > width_max(v->user_idx_bytes())) {      // I::from(n) (vec.rs:445-451)
        if (info) info->kind = 3;
        SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Index size is too small");
    }
    return csvec_check_device(v, (hipStream_t)stream, info);
}

int32_t sprs_hip_csmat_from_unsorted(const sprs_hip_csmat *m, sprs_hip_csmat **out, sprs_hip_structure_info *info, void *stream) {
    clear_error();
    if (info) *info = sprs_hip_structure_info{0, 0, 0};
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsmat res;
    SPRS_TRY(csmat_from_unsorted(m, res, info, (hipStream_t)stream));
    return finish_result(res, m, out);
}

int32_t sprs_hip_csvec_from_unsorted(const sprs_hip_csvec *v, sprs_hip_csvec **out, sprs_hip_structure_info *info, void *stream) {
    clear_error();
    if (info) *info = sprs_hip_structure_info{0, 0, 0};
    if (!v || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (v->dim > width_max(v->user_idx_bytes())) {
        if (info) info->kind = 3;
        SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Index size is too small");
    }
    OwnedCsvec res;
    return finish_csvec(csvec_from_unsorted(v, res, info, (hipStream_t)stream), res, out);
}

}  // extern "C"

// ---- orderings (linalg/ordering.rs, symmetric.rs, csmat.rs:1188-1216); kernels in ordering.hpp ----------------------------------

extern "C" {

int32_t sprs_hip_csmat_is_symmetric(const sprs_hip_csmat *m, int32_t *flag, void *stream) {
    clear_error();
    if (!m || !flag) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    return csmat_is_symmetric(m, flag, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_degrees(const sprs_hip_csmat *m, uint64_t *out_dev, void *stream) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (m->outer() && !out_dev) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL output");
    if ((uintptr_t)out_dev % 8) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "device buffers must be aligned to their element size");
    return csmat_degrees(m, out_dev, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_max_outer_nnz(const sprs_hip_csmat *m, uint64_t *out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    return csmat_max_outer_nnz(m, out, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_cuthill_mckee(const sprs_hip_csmat *m, int32_t start, int32_t reversed, int32_t check_symmetric,
                                     sprs_hip_ordering **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (start != SPRS_HIP_START_NEXT && start != SPRS_HIP_START_MINIMUM_DEGREE && start != SPRS_HIP_START_PSEUDO_PERIPHERAL)
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "bad start strategy %d", start);
    if (m->cols != m->rows)                          // assert_eq!(mat.cols(), mat.rows()), ordering.rs:453
        SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "assertion `left == right` failed\n  left: %llu\n right: %llu", (unsigned long long)m->cols,
                  (unsigned long long)m->rows);
    if (m->rows && m->rows - 1 > width_max(m->user_idx_bytes()))   // I::from_usize(vertex_index), ordering.rs:333
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold %llu", (unsigned long long)(m->rows - 1));
    if (check_symmetric) {                           // debug_assert!(is_symmetric(&mat)), ordering.rs:452
        int32_t sym = 0;
        SPRS_TRY(csmat_is_symmetric(m, &sym, (hipStream_t)stream));
        if (!sym) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "matrix is not symmetric");
    }
    std::unique_ptr<sprs_hip_ordering> o(make_ordering());
    SPRS_TRY(csmat_cuthill_mckee(m, start, reversed != 0, o.get(), (hipStream_t)stream));
    *out = o.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ordering_info(const sprs_hip_ordering *o, uint64_t *dim, uint64_t *n_parts, uint64_t *stats) {
    clear_error();
    if (!o) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (dim) *dim = o->dim;
    if (n_parts) *n_parts = o->parts.size();
    if (stats)
        for (int k = 0; k < 4; ++k) stats[k] = o->stats[k];
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ordering_perm(const sprs_hip_ordering *o, sprs_hip_perm **out) {
    clear_error();
    if (!o || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    const sprs_hip_perm *p = o->perm.get();
    OwnedPerm q;
    SPRS_TRY(make_perm(q, p->dim, p->idx_bytes, p->user_idx_bytes()));
    if (p->dim) {
        const uint64_t bytes = p->dim * (uint64_t)p->idx_bytes;
        hipError_t e = hipMemcpyAsync(q->perm, p->perm, bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = hipMemcpyAsync(q->perm_inv, p->perm_inv, bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return fail_hip(e, "ordering_perm");
    }
    *out = q.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ordering_parts(const sprs_hip_ordering *o, uint64_t *parts) {
    clear_error();
    if (!o || !parts) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    for (size_t k = 0; k < o->parts.size(); ++k) parts[k] = o->parts[k];
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ordering_free(sprs_hip_ordering *o) {
    clear_error();
    delete o;
    return SPRS_HIP_OK;
}

}  // extern "C"

// ---- LDL^T (sprs-ldl/src/lib.rs, sprs/src/sparse/linalg.rs:17-29); kernels in ldl.hpp --------------------------------------------

// the matrix a factor / update call takes against the analysis it is factored with
static int32_t ldl_matrix_ok(const LdlSym &s, const sprs_hip_csmat *m) {
    if (m->rows != m->cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "matrix should be square");      // lib.rs:262
    if (m->rows != s.n) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");                 // assert!(diag.len() == mat.outer_dims()), lib.rs:521
    if (m->idx_bytes != s.idx_bytes || m->user_idx_bytes() != (s.decl_idx_bytes ? s.decl_idx_bytes : s.idx_bytes))
        SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "the matrix must have the index type of the one that was analysed");
    // DStack::with_capacity(n) in LdlSymbolic::factor (lib.rs:313)
    if (s.n < 2) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "assertion failed: n > 1 (DStack::with_capacity, sprs/src/stack.rs:39)");
    return SPRS_HIP_OK;
}

extern "C" {

int32_t sprs_hip_ldl_symbolic(const sprs_hip_csmat *m, const sprs_hip_perm *perm, int32_t check_symmetry, sprs_hip_ldl_sym **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (m->rows != m->cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "matrix should be square");      // lib.rs:262
    if (perm && perm->dim != m->rows) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    SPRS_TRY(perm_width_ok(m, perm));
    if (m->rows >= (1ull << 31)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "LDL: 2^31 rows or more are not supported");
    std::unique_ptr<sprs_hip_ldl_sym> h(make_ldl_symbolic());
    if (check_symmetry) {                            // lib.rs:458-465
        int32_t sym = 0;
        SPRS_TRY(csmat_is_symmetric(m, &sym, (hipStream_t)stream));
        ++h->s->stats[2];
        if (!sym) SPRS_FAIL(SPRS_HIP_BAD_STRUCTURE, "Matrix is not symmetric");
    }
    SPRS_TRY(ldl_symbolic(m, perm, *h->s, (hipStream_t)stream));
    if (h->s->lnz > width_max(m->user_idx_bytes()))  // prev += l_nz[k] in I (lib.rs:493)
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold %llu", (unsigned long long)h->s->lnz);
    *out = h.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_symbolic_info(const sprs_hip_ldl_sym *s, uint64_t *n, uint64_t *nnz, uint64_t *stats) {
    clear_error();
    if (!s) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (n) *n = s->s->n;
    if (nnz) *nnz = s->s->lnz;
    if (stats)
        for (int k = 0; k < 4; ++k) stats[k] = s->s->stats[k];
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_symbolic_colptr(const sprs_hip_ldl_sym *s, uint64_t *colptr) {
    clear_error();
    if (!s || !colptr) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    SPRS_TRY_HIP(copy_to_host(colptr, s->s->colptr, (s->s->n + 1) * 8, nullptr));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_symbolic_parents(const sprs_hip_ldl_sym *s, uint64_t *parents) {
    clear_error();
    if (!s || (s->s->n && !parents)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    std::vector<uint32_t> p32(s->s->n);
    if (s->s->n) SPRS_TRY_HIP(copy_to_host(p32.data(), s->s->parents, s->s->n * sizeof(uint32_t), nullptr));
    for (uint64_t i = 0; i < s->s->n; ++i) parents[i] = p32[i] == 0xFFFFFFFFu ? UINT64_MAX : (uint64_t)p32[i];
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_symbolic_perm(const sprs_hip_ldl_sym *s, sprs_hip_perm **out) {
    clear_error();
    if (!s || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    const sprs_hip_perm *p = s->s->perm.get();
    if (p->identity) {
        *out = identity_perm(p->dim, p->user_idx_bytes());
        return SPRS_HIP_OK;
    }
    OwnedPerm q;
    SPRS_TRY(make_perm(q, p->dim, p->idx_bytes, p->user_idx_bytes()));
    if (p->dim) {
        const uint64_t bytes = p->dim * (uint64_t)p->idx_bytes;
        hipError_t e = hipMemcpyAsync(q->perm, p->perm, bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = hipMemcpyAsync(q->perm_inv, p->perm_inv, bytes, hipMemcpyDeviceToDevice, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return fail_hip(e, "ldl_symbolic_perm");
    }
    *out = q.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_symbolic_free(sprs_hip_ldl_sym *s) {
    clear_error();
    delete s;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_factor_f64(const sprs_hip_ldl_sym *s, const sprs_hip_csmat *m, sprs_hip_ldl_num **out, sprs_hip_trisolve_info *info,
                                void *stream) {
    clear_error();
    if (!s || !m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (info) *info = sprs_hip_trisolve_info{0, UINT64_MAX, 0};
    SPRS_TRY(ldl_matrix_ok(*s->s, m));
    std::unique_ptr<sprs_hip_ldl_num> f(make_ldl_numeric(s));
    SPRS_TRY(ldl_factor_f64(*f->s, m, f.get(), info, (hipStream_t)stream));
    *out = f.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_update_f64(sprs_hip_ldl_num *f, const sprs_hip_csmat *m, sprs_hip_trisolve_info *info, void *stream) {
    clear_error();
    if (!f || !m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    if (info) *info = sprs_hip_trisolve_info{0, UINT64_MAX, 0};
    SPRS_TRY(ldl_matrix_ok(*f->s, m));
    return ldl_factor_f64(*f->s, m, f, info, (hipStream_t)stream);
}

int32_t sprs_hip_ldl_solve_f64(sprs_hip_ldl_num *f, const double *b_dev, double *x_dev, uint64_t n, void *stream) {
    clear_error();
    if (!f) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (n != f->s->n) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (n && (!b_dev || !x_dev)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    return ldl_solve_f64(f, b_dev, x_dev, (hipStream_t)stream);
}

int32_t sprs_hip_ldl_d(const sprs_hip_ldl_num *f, double *d_dev, uint64_t n, void *stream) {
    clear_error();
    if (!f) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (n != f->s->n) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (n && !d_dev) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    if (n) SPRS_TRY_HIP(hipMemcpyAsync(d_dev, f->d.p, n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_l(const sprs_hip_ldl_num *f, sprs_hip_csmat **out, void *stream) {
    clear_error();
    if (!f || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsmat res;
    SPRS_TRY(ldl_export_l(f, res, (hipStream_t)stream));
    *out = res.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_ldl_numeric_free(sprs_hip_ldl_num *f) {
    clear_error();
    delete f;
    return SPRS_HIP_OK;
}

static int32_t ldl_tri_entry(sprs_hip_csmat *l, bool transposed, double *x_dev, uint64_t n, void *stream) {
    clear_error();
    if (!l) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (l->storage != SPRS_HIP_CSC) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    if (l->rows != l->cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Non square matrix passed to solver");
    if (l->cols != n) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (n && !x_dev) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL vector");
    if (n >= (1ull << 32)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "triangular solve: 2^32 rows or more are not supported");
    if (n == 0) return SPRS_HIP_OK;
    std::lock_guard<std::recursive_mutex> lock(l->mu);
    sprs_hip_csmat *csr = nullptr;
    if (!transposed) SPRS_TRY(csr_form(l, &csr));
    return ldl_tri_f64(l, csr, transposed, x_dev, (hipStream_t)stream);
}

int32_t sprs_hip_ldl_lsolve_f64(sprs_hip_csmat *l, double *x_dev, uint64_t n, void *stream) { return ldl_tri_entry(l, false, x_dev, n, stream); }

int32_t sprs_hip_ldl_ltsolve_f64(sprs_hip_csmat *l, double *x_dev, uint64_t n, void *stream) { return ldl_tri_entry(l, true, x_dev, n, stream); }

int32_t sprs_hip_diag_solve_f64(const double *d_dev, double *x_dev, uint64_t n, void *stream) {
    return entry_diag_solve(d_dev, x_dev, n, stream);
}

}  // extern "C"

// ---- construction (kronecker.rs, construct.rs); kernels in construct.hpp --------------------------------------------------------

// the one I / Iptr of the reference's signatures
static int32_t same_index_types(const sprs_hip_csmat *a, const sprs_hip_csmat *b, const char *where) {
    if (a->user_iptr_bytes() != b->user_iptr_bytes() || a->user_idx_bytes() != b->user_idx_bytes())
        SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "operands must share index types (%s)", where);
    return SPRS_HIP_OK;
}

static bool mul_overflows(uint64_t x, uint64_t y, uint64_t *prod) { return __builtin_mul_overflow(x, y, prod); }

// the form of m in `storage`: itself, or a to_other_storage() copy kept in `keep`.  The conversion runs on the null stream: what
// the caller's stream still has to write into m comes first.
static int32_t in_storage(const sprs_hip_csmat *m, int32_t storage, std::vector<OwnedCsmat> &keep, void *stream, const sprs_hip_csmat **out) {
    *out = m;
    if (m->storage == storage) return SPRS_HIP_OK;
    if (stream) SPRS_TRY_HIP(hipStreamSynchronize((hipStream_t)stream));
    OwnedCsmat conv;
    SPRS_TRY(convert_checked(m, conv));
    *out = conv.get();
    keep.push_back(std::move(conv));
    return SPRS_HIP_OK;
}

// what a stacked result must fit, tested before anything is allocated: I::from_usize on the inner dimension, Iptr::from_usize
// on the nnz, at the widths the operands declare
static int32_t stack_fits(const sprs_hip_csmat *like, uint64_t inner, uint64_t nnz) {
    if (inner && inner - 1 > width_max(like->user_idx_bytes()))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the number of rows requested (required %llu)",
                  (unsigned long long)inner);
    if (nnz > width_max(like->user_iptr_bytes()))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the nnz of the result (%llu)", (unsigned long long)nnz);
    return SPRS_HIP_OK;
}

// same_storage_fast_stack (construct.rs:19-45) on n >= 0 handles
static int32_t fast_stack(const sprs_hip_csmat *const *mats, uint64_t n, sprs_hip_csmat **out, void *stream) {
    if (n == 0) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "Empty stacking list");
    const uint64_t inner = mats[0]->inner();
    for (uint64_t k = 0; k < n; ++k)
        if (mats[k]->inner() != inner) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    const int32_t storage = mats[0]->storage;
    for (uint64_t k = 0; k < n; ++k)
        if (mats[k]->storage != storage) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    std::vector<StackItem> items(n);
    std::vector<uint64_t> outer_of(n);
    uint64_t outer = 0, nnz = 0;
    for (uint64_t k = 0; k < n; ++k) {
        items[k] = {mats[k], k, 0};
        outer_of[k] = mats[k]->outer();
        if (__builtin_add_overflow(outer, outer_of[k], &outer) || __builtin_add_overflow(nnz, mats[k]->nnz, &nnz))
            SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "the stacked dimensions overflow 64 bits");
    }
    SPRS_TRY(stack_fits(mats[0], inner, nnz));
    const bool csr = storage == SPRS_HIP_CSR;
    OwnedCsmat res;
    SPRS_TRY(csmat_stack(items, outer_of, storage, csr ? outer : inner, csr ? inner : outer, mats[0]->iptr_bytes, mats[0]->idx_bytes, res,
                         (hipStream_t)stream));
    SPRS_TRY(inherit_declared_widths(res.get(), mats[0]));
    *out = res.release();
    return SPRS_HIP_OK;
}

// the argument checks the three list entries share
static int32_t stack_args(const sprs_hip_csmat *const *mats, uint64_t n, sprs_hip_csmat **out) {
    if (!out || (n && !mats)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    for (uint64_t k = 0; k < n; ++k) {
        if (!mats[k]) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle in the stacking list");
        SPRS_TRY(same_index_types(mats[0], mats[k], "construct.rs:10-17"));
    }
    return SPRS_HIP_OK;
}

// vstack / hstack (construct.rs:48-81): every operand in `storage`, then the fast stack
static int32_t stack_in(const sprs_hip_csmat *const *mats, uint64_t n, int32_t storage, sprs_hip_csmat **out, void *stream) {
    SPRS_TRY(stack_args(mats, n, out));
    std::vector<OwnedCsmat> keep;
    std::vector<const sprs_hip_csmat *> forms(n);
    for (uint64_t k = 0; k < n; ++k) SPRS_TRY(in_storage(mats[k], storage, keep, stream, &forms[k]));
    return fast_stack(forms.data(), n, out, stream);
}

extern "C" {

int32_t sprs_hip_csmat_kronecker_f64(const sprs_hip_csmat *a, const sprs_hip_csmat *b, sprs_hip_csmat **out, void *stream) {
    clear_error();
    if (!a || !b || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    SPRS_TRY(same_index_types(a, b, "kronecker.rs:50-58"));
    // b in a's storage has the inner dimension b has along a's inner axis
    const uint64_t inner_a = a->inner(), inner_b = a->storage == SPRS_HIP_CSR ? b->cols : b->rows;
    uint64_t rows, cols, inner, nnz;
    if (mul_overflows(a->rows, b->rows, &rows) || mul_overflows(a->cols, b->cols, &cols) || rows == UINT64_MAX || cols == UINT64_MAX)
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "the shape of the Kronecker product overflows 64 bits");
    (void)mul_overflows(inner_a, inner_b, &inner);
    if (inner && inner - 1 > width_max(a->user_idx_bytes()))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold %llu", (unsigned long long)(inner - 1));
    if (mul_overflows(a->nnz, b->nnz, &nnz) || nnz > width_max(a->user_iptr_bytes()) || nnz > (UINT64_MAX >> 1))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the nnz of the result (%llu x %llu)",
                  (unsigned long long)a->nnz, (unsigned long long)b->nnz);
    std::vector<OwnedCsmat> keep;
    const sprs_hip_csmat *bf = nullptr;
    SPRS_TRY(in_storage(b, a->storage, keep, stream, &bf));
    OwnedCsmat res;
    SPRS_TRY(csmat_kronecker_f64(a, bf, res, (hipStream_t)stream));
    SPRS_TRY(inherit_declared_widths(res.get(), a));
    *out = res.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csmat_same_storage_fast_stack(const sprs_hip_csmat **mats, uint64_t n, sprs_hip_csmat **out, void *stream) {
    clear_error();
    SPRS_TRY(stack_args(mats, n, out));
    return fast_stack(mats, n, out, stream);
}

int32_t sprs_hip_csmat_vstack(const sprs_hip_csmat **mats, uint64_t n, sprs_hip_csmat **out, void *stream) {
    clear_error();
    return stack_in(mats, n, SPRS_HIP_CSR, out, stream);
}

int32_t sprs_hip_csmat_hstack(const sprs_hip_csmat **mats, uint64_t n, sprs_hip_csmat **out, void *stream) {
    clear_error();
    return stack_in(mats, n, SPRS_HIP_CSC, out, stream);
}

int32_t sprs_hip_csmat_bmat(const sprs_hip_csmat **blocks, uint64_t super_rows, uint64_t super_cols, sprs_hip_csmat **out, void *stream) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    if (super_rows == 0 || super_cols == 0) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "Empty stacking list");   // construct.rs:105-108
    uint64_t cells;
    if (!blocks || mul_overflows(super_rows, super_cols, &cells)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    auto at = [&](uint64_t i, uint64_t j) { return blocks[i * super_cols + j]; };
    const sprs_hip_csmat *first = nullptr;
    for (uint64_t c = 0; c < cells && !first; ++c) first = blocks[c];
    for (uint64_t c = 0; c < cells; ++c)
        if (blocks[c]) SPRS_TRY(same_index_types(first, blocks[c], "construct.rs:94-102"));
    for (uint64_t i = 0; i < super_rows; ++i) {     // construct.rs:116-119
        bool any = false;
        for (uint64_t j = 0; j < super_cols; ++j) any = any || at(i, j);
        if (!any) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "Empty bmat row");
    }
    for (uint64_t j = 0; j < super_cols; ++j) {     // construct.rs:120-123
        bool any = false;
        for (uint64_t i = 0; i < super_rows; ++i) any = any || at(i, j);
        if (!any) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "Empty bmat col");
    }
    // the shapes of the None elements (construct.rs:126-142)
    std::vector<uint64_t> rows_per_row(super_rows, 0), cols_per_col(super_cols, 0);
    for (uint64_t i = 0; i < super_rows; ++i)
        for (uint64_t j = 0; j < super_cols; ++j)
            if (at(i, j)) {
                rows_per_row[i] = std::max(rows_per_row[i], at(i, j)->rows);
                cols_per_col[j] = std::max(cols_per_col[j], at(i, j)->cols);
            }
    // hstack of every super-row (rows equal: its inner-dimension check), vstack of the results (total columns equal)
    std::vector<StackItem> items;
    uint64_t total_rows = 0, total_cols = 0, nnz = 0;
    for (uint64_t i = 0; i < super_rows; ++i) {
        uint64_t off = 0;
        for (uint64_t j = 0; j < super_cols; ++j) {
            const sprs_hip_csmat *m = at(i, j);
            if (m && m->rows != rows_per_row[i]) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
            if (m) items.push_back({m, i, off});
            if (__builtin_add_overflow(off, m ? m->cols : cols_per_col[j], &off) || (m && __builtin_add_overflow(nnz, m->nnz, &nnz)))
                SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "the stacked dimensions overflow 64 bits");
        }
        if (i == 0) total_cols = off;
        if (off != total_cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
        if (__builtin_add_overflow(total_rows, rows_per_row[i], &total_rows))
            SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "the stacked dimensions overflow 64 bits");
    }
    SPRS_TRY(stack_fits(first, total_cols, nnz));
    std::vector<OwnedCsmat> keep;
    for (StackItem &it : items) SPRS_TRY(in_storage(it.m, SPRS_HIP_CSR, keep, stream, &it.m));
    OwnedCsmat res;
    SPRS_TRY(csmat_stack(items, rows_per_row, SPRS_HIP_CSR, total_rows, total_cols, first->iptr_bytes, first->idx_bytes, res, (hipStream_t)stream));
    SPRS_TRY(inherit_declared_widths(res.get(), first));
    *out = res.release();
    return SPRS_HIP_OK;
}

}  // extern "C"

// ---- dense <-> sparse (csmat.rs:499-549, to_dense.rs, binop.rs:273-433); kernels in dense.hpp ------------------------------------

// a dense operand of the ABI: layout tag, leading dimension, base pointer
static int32_t dense_arg_ok(const void *p, uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld, const char *what) {
    if (layout != SPRS_HIP_ROW_MAJOR && layout != SPRS_HIP_COL_MAJOR) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "bad layout tag");
    if (ld < (layout == SPRS_HIP_ROW_MAJOR ? cols : rows)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "leading dimension smaller than the extent it strides over");
    uint64_t n;
    if (mul_overflows(rows, cols, &n)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "%s: rows * cols overflows 64 bits", what);
    if (n && !p) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL matrix");
    return SPRS_HIP_OK;
}

// elements from the first to the one behind the last of a rows x cols array (0: it has none)
static uint64_t dense_span(uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld) {
    if (!rows || !cols) return 0;
    return layout == SPRS_HIP_ROW_MAJOR ? (rows - 1) * ld + cols : (cols - 1) * ld + rows;
}

static bool storage_matches(int32_t storage, int32_t layout) { return (storage == SPRS_HIP_CSR) == (layout == SPRS_HIP_ROW_MAJOR); }

// the checks of csmat_binop_dense_raw (binop.rs:397-412) in its order, after the argument checks
static int32_t binop_dense_contract(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld,
                                    int32_t op, double *out_dev, uint64_t out_ld, bool same_ordering) {
    if (op != SPRS_HIP_BINOP_ADD && op != SPRS_HIP_BINOP_MUL) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "op must be SPRS_HIP_BINOP_ADD or SPRS_HIP_BINOP_MUL");
    SPRS_TRY(dense_arg_ok(rhs_dev, rows, cols, layout, ld, "binop_dense"));
    SPRS_TRY(dense_arg_ok(out_dev, rows, cols, layout, out_ld, "binop_dense"));
    if (!lhs) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (lhs->cols != cols || lhs->rows != rows) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (same_ordering && !storage_matches(lhs->storage, layout)) SPRS_FAIL(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    const uint64_t span_r = dense_span(rows, cols, layout, ld), span_o = dense_span(rows, cols, layout, out_ld);
    if (span_r && rhs_dev < out_dev + span_o && out_dev < rhs_dev + span_r)
        SPRS_FAIL(SPRS_HIP_INVALID_ARG, "the result matrix overlaps the right-hand side");
    return SPRS_HIP_OK;
}

extern "C" {

int32_t sprs_hip_csmat_from_dense_f64(sprs_hip_csmat **out, int32_t storage, const double *m_dev, uint64_t rows, uint64_t cols, int32_t layout,
                                      uint64_t ld, double epsilon, int32_t iptr_bytes, int32_t idx_bytes, void *stream) {
    clear_error();
    if (!out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    if (storage != SPRS_HIP_CSR && storage != SPRS_HIP_CSC) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "bad storage tag %d", storage);
    if (!host_widths_ok(iptr_bytes, idx_bytes)) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "index widths must be 2, 4 or 8 bytes");
    SPRS_TRY(dense_arg_ok(m_dev, rows, cols, layout, ld, "from_dense"));
    const double eps = epsilon > 0.0 ? epsilon : 0.0;               // csmat.rs:506-510: a negative or NaN epsilon is 0
    const int32_t dev_iptr = iptr_bytes == 2 ? 4 : iptr_bytes, dev_idx = idx_bytes == 2 ? 4 : idx_bytes;
    const uint64_t idx_max = width_max(idx_bytes), nnz_max = std::min(width_max(iptr_bytes), UINT64_MAX >> 1);
    const bool rowmaj = layout == SPRS_HIP_ROW_MAJOR;
    const uint64_t lines = rowmaj ? rows : cols, width = rowmaj ? cols : rows;
    OwnedCsmat res;
    if (storage_matches(storage, layout) || !rows || !cols) {
        // (an array without elements has no order: the requested storage at once)
        const bool csr = storage == SPRS_HIP_CSR;
        SPRS_TRY(csmat_from_dense_f64(m_dev, storage, csr ? rows : cols, csr ? cols : rows, ld, eps, idx_max, UINT64_MAX, nnz_max, dev_iptr,
                                      dev_idx, res, (hipStream_t)stream));
    } else {
        // csr_from_dense of an F-ordered view / csc_from_dense of a C-ordered one: the matched storage of the layout, then
        // to_other_storage — the same entries in the same order as the reference's strided walk.  The index that has to fit
        // the index type is the LINE: it becomes the result's inner index.
        if (dev_idx == 4 && width > (1ull << 32))
            SPRS_FAIL(SPRS_HIP_INVALID_ARG, "from_dense: 32-bit indices against the layout with more than 2^32 elements per line are not supported");
        OwnedCsmat matched;
        SPRS_TRY(csmat_from_dense_f64(m_dev, rowmaj ? SPRS_HIP_CSR : SPRS_HIP_CSC, lines, width, ld, eps, UINT64_MAX, idx_max, nnz_max, dev_iptr,
                                      dev_idx, matched, (hipStream_t)stream));
        SPRS_TRY(to_other_storage(matched.get(), res));              // (null stream; `matched` is complete)
    }
    if (iptr_bytes == 2 || idx_bytes == 2) {
        res->decl_iptr_bytes = iptr_bytes;
        res->decl_idx_bytes = idx_bytes;
    }
    *out = res.release();
    return SPRS_HIP_OK;
}

static int32_t assign_dense(const sprs_hip_csmat *m, bool zero_first, double *out_dev, uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld,
                            void *stream) {
    SPRS_TRY(dense_arg_ok(out_dev, rows, cols, layout, ld, "assign_to_dense"));
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    if (m->cols != cols) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");      // to_dense.rs:20
    if (m->rows != rows) SPRS_FAIL(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");      // to_dense.rs:21
    return csmat_assign_dense_f64(m, zero_first, out_dev, layout, ld, (hipStream_t)stream);
}

int32_t sprs_hip_csmat_assign_to_dense_f64(const sprs_hip_csmat *m, double *out_dev, uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld,
                                           void *stream) {
    clear_error();
    return assign_dense(m, false, out_dev, rows, cols, layout, ld, stream);
}

int32_t sprs_hip_csmat_to_dense_f64(const sprs_hip_csmat *m, double *out_dev, uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld,
                                    void *stream) {
    clear_error();
    return assign_dense(m, true, out_dev, rows, cols, layout, ld, stream);
}

int32_t sprs_hip_csmat_binop_dense_f64(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld,
                                       int32_t op, double alpha, double beta, double *out_dev, uint64_t out_ld, void *stream) {
    clear_error();
    SPRS_TRY(binop_dense_contract(lhs, rhs_dev, rows, cols, layout, ld, op, out_dev, out_ld, true));
    return csmat_binop_dense_f64(lhs, rhs_dev, layout, ld, op, alpha, beta, out_dev, out_ld, (hipStream_t)stream);
}

// `&CsMat + &Array2` (csmat.rs:1951-1987): alpha = beta = 1; lhs.to_other_storage() first when its storage does not match the
// layout — the copy lives for the call
int32_t sprs_hip_csmat_add_dense_f64(const sprs_hip_csmat *lhs, const double *rhs_dev, uint64_t rows, uint64_t cols, int32_t layout, uint64_t ld,
                                     double *out_dev, void *stream) {
    clear_error();
    const uint64_t out_ld = layout == SPRS_HIP_ROW_MAJOR ? cols : rows;
    SPRS_TRY(binop_dense_contract(lhs, rhs_dev, rows, cols, layout, ld, SPRS_HIP_BINOP_ADD, out_dev, out_ld, false));
    OwnedCsmat conv;
    if (!storage_matches(lhs->storage, layout)) {
        // the conversion runs on the null stream: what the caller's stream still has to write into lhs comes first
        if (stream) SPRS_TRY_HIP(hipStreamSynchronize((hipStream_t)stream));
        SPRS_TRY(convert_checked(lhs, conv));
    }
    SPRS_TRY(csmat_binop_dense_f64(conv ? conv.get() : lhs, rhs_dev, layout, ld, SPRS_HIP_BINOP_ADD, 1.0, 1.0, out_dev, out_ld, (hipStream_t)stream));
    if (conv) SPRS_TRY_HIP(hipStreamSynchronize((hipStream_t)stream));   // the kernels read the copy: it goes with this call
    return SPRS_HIP_OK;
}

}  // extern "C"

// ---- single precision: the f32 twins forward to the same bodies as the f64 entries (kernels: spmv_f32.hpp, spmm_f32.hpp, bicgstab.hip) ----
extern "C" {

int32_t sprs_hip_csmat_f32_upload(sprs_hip_csmat_f32 **out, int32_t storage, uint64_t rows, uint64_t cols, const void *indptr,
                                  int32_t iptr_bytes, const void *indices, int32_t idx_bytes, const float *data, int32_t validate) {
    return entry_upload(out, storage, rows, cols, indptr, iptr_bytes, indices, idx_bytes, data, validate);
}

int32_t sprs_hip_csmat_f32_wrap_device(sprs_hip_csmat_f32 **out, int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz,
                                       const void *dev_indptr, int32_t iptr_bytes, const void *dev_indices, int32_t idx_bytes,
                                       const float *dev_data) {
    return entry_wrap_device(out, storage, rows, cols, nnz, dev_indptr, iptr_bytes, dev_indices, idx_bytes, dev_data);
}

int32_t sprs_hip_csmat_f32_info(const sprs_hip_csmat_f32 *m, uint64_t *rows, uint64_t *cols, uint64_t *nnz, int32_t *iptr_bytes,
                                int32_t *idx_bytes, int32_t *storage) {
    return entry_info(m, rows, cols, nnz, iptr_bytes, idx_bytes, storage);
}

int32_t sprs_hip_csmat_f32_device_ptrs(const sprs_hip_csmat_f32 *m, const void **indptr, const void **indices, const float **data) {
    return entry_device_ptrs(m, indptr, indices, data);
}

int32_t sprs_hip_csmat_f32_download(const sprs_hip_csmat_f32 *m, void *indptr, void *indices, float *data) {
    return entry_download(m, indptr, indices, data);
}

int32_t sprs_hip_csmat_f32_transpose_view(const sprs_hip_csmat_f32 *m, sprs_hip_csmat_f32 **out) {
    return entry_transpose_view(m, out);
}

int32_t sprs_hip_csmat_f32_refresh(sprs_hip_csmat_f32 *m) {
    return entry_refresh(m);
}

int32_t sprs_hip_csmat_f32_prepare(sprs_hip_csmat_f32 *m, void *stream) {
    return entry_prepare(m, stream);
}

int32_t sprs_hip_csmat_f32_spmv_plan_info(const sprs_hip_csmat_f32 *m, int32_t *kind, uint64_t *plan_bytes) {
    clear_error();
    if (!m) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL handle");
    auto *mm = const_cast<sprs_hip_csmat_f32 *>(m);
    std::lock_guard<std::recursive_mutex> lock(mm->mu);
    // a CSC handle multiplies through its cached CSR form: the plan lives there
    const sprs_hip_csmat_f32 *csr = m->storage == SPRS_HIP_CSC && m->as_other ? m->as_other : m;
    const SpmvPlanF32 &pl = csr->plan;
    int32_t k = 0;
    uint64_t bytes = 0;
    if (pl.built) {
        k = pl.band ? 3 : 1;                   // (no XCD-sliced plan, kind 2, for f32)
        bytes = pl.band ? band_plan_bytes(pl.band.get()) : (pl.ntiles + 1) * 8;
    }
    if (kind) *kind = k;
    if (plan_bytes) *plan_bytes = bytes;
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csmat_f32_free(sprs_hip_csmat_f32 *m) {
    return entry_free(m);
}

int32_t sprs_hip_csmat_f32_to_other_storage(const sprs_hip_csmat_f32 *m, sprs_hip_csmat_f32 **out) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    // the index-type check of the reference (csmat.rs:1794-1797)
    if (m->rows > width_max(m->idx_bytes))
        SPRS_FAIL(SPRS_HIP_INDEX_OVERFLOW, "Index type is not large enough to hold the number of rows requested (required %llu)",
                  (unsigned long long)m->rows);
    OwnedCsmatF32 res;
    SPRS_TRY(csmat_f32_to_other_storage(m, res));
    *out = res.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csmat_f32_from_f64(const sprs_hip_csmat *m, sprs_hip_csmat_f32 **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsmatF32 res;
    SPRS_TRY(csmat_f32_from_f64(m, res, (hipStream_t)stream));
    SPRS_TRY_HIP(hipStreamSynchronize((hipStream_t)stream));
    *out = res.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_csmat_f32_to_f64(const sprs_hip_csmat_f32 *m, sprs_hip_csmat **out, void *stream) {
    clear_error();
    if (!m || !out) SPRS_FAIL(SPRS_HIP_INVALID_ARG, "NULL argument");
    *out = nullptr;
    OwnedCsmat res;
    SPRS_TRY(csmat_f32_to_f64(m, res, (hipStream_t)stream));
    SPRS_TRY_HIP(hipStreamSynchronize((hipStream_t)stream));
    *out = res.release();
    return SPRS_HIP_OK;
}

int32_t sprs_hip_spmv_f32(const sprs_hip_csmat_f32 *a, const float *x_dev, uint64_t x_len, float *y_dev, uint64_t y_len,
                          int32_t accumulate, void *stream) {
    return entry_spmv(a, x_dev, x_len, y_dev, y_len, accumulate, stream);
}

int32_t sprs_hip_mul_acc_mat_vec_csc_f32(const sprs_hip_csmat_f32 *a, const float *x_dev, uint64_t x_len, float *y_dev, uint64_t y_len,
                                         void *stream) {
    return entry_mul_acc_mat_vec_csc(a, x_dev, x_len, y_dev, y_len, stream);
}

int32_t sprs_hip_csmat_mul_vec_f32(const sprs_hip_csmat_f32 *a, const float *x_dev, uint64_t x_len, float *y_dev, uint64_t y_len,
                                   void *stream) {
    return entry_csmat_mul_vec(a, x_dev, x_len, y_dev, y_len, stream);
}

int32_t sprs_hip_bicgstab_f32(sprs_hip_csmat_f32 *a, const float *x0_dev, const float *b_dev, uint64_t n, double tol, uint64_t max_iter,
                              double soft_restart_threshold, float *x_dev, sprs_hip_bicgstab_info *info, void *stream) {
    return entry_bicgstab(a, x0_dev, b_dev, n, tol, max_iter, soft_restart_threshold, x_dev, info, stream);
}

int32_t sprs_hip_trisolve_f32(sprs_hip_csmat_f32 *a, int32_t uplo, float *x_dev, uint64_t n, sprs_hip_trisolve_info *info, void *stream) {
    return entry_trisolve(a, uplo, x_dev, n, info, stream);
}

int32_t sprs_hip_gauss_seidel_f32(sprs_hip_csmat_f32 *a, float *x_dev, const float *rhs_dev, uint64_t n, uint64_t max_iter, double eps,
                                  sprs_hip_gauss_seidel_info *info, void *stream) {
    return entry_gauss_seidel(a, x_dev, rhs_dev, n, max_iter, eps, info, stream);
}

int32_t sprs_hip_diag_solve_f32(const float *d_dev, float *x_dev, uint64_t n, void *stream) {
    return entry_diag_solve(d_dev, x_dev, n, stream);
}

int32_t sprs_hip_spmm_rowmaj_f32(const sprs_hip_csmat_f32 *a, const float *rhs_dev, uint64_t rhs_rows, uint64_t k, uint64_t ld_rhs,
                                 float *out_dev, uint64_t out_rows, uint64_t ld_out, int32_t accumulate, void *stream) {
    return entry_spmm_rowmaj(a, rhs_dev, rhs_rows, k, ld_rhs, out_dev, out_rows, ld_out, accumulate, stream);
}

int32_t sprs_hip_csmat_mulacc_dense_f32(const sprs_hip_csmat_f32 *lhs, const float *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                        int32_t rhs_layout, uint64_t ld_rhs, float *out_dev, uint64_t out_rows,
                                        int32_t out_layout, uint64_t ld_out, int32_t accumulate, void *stream) {
    return entry_mulacc_dense(lhs, rhs_dev, rhs_rows, k, rhs_layout, ld_rhs, out_dev, out_rows, out_layout, ld_out, accumulate, stream);
}

int32_t sprs_hip_csmat_mul_dense_f32(const sprs_hip_csmat_f32 *lhs, const float *rhs_dev, uint64_t rhs_rows, uint64_t k,
                                     int32_t rhs_layout, uint64_t ld_rhs, float *out_dev, int32_t *out_layout, void *stream) {
    return entry_mul_dense(lhs, rhs_dev, rhs_rows, k, rhs_layout, ld_rhs, out_dev, out_layout, stream);
}

int32_t sprs_hip_spgemm_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 **c) {
    return entry_spgemm(a, b, c);
}

int32_t sprs_hip_spgemm_symbolic_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 **c) {
    return entry_spgemm_symbolic(a, b, c);
}

int32_t sprs_hip_spgemm_numeric_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_csmat_f32 *c) {
    return entry_spgemm_numeric(a, b, c);
}

int32_t sprs_hip_spgemm_plan_create_f32(const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b, sprs_hip_spgemm_plan **plan) {
    return entry_spgemm_plan_create(a, b, plan);
}

int32_t sprs_hip_spgemm_plan_structure_f32(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b,
                                           sprs_hip_csmat_f32 **c_structure) {
    return entry_spgemm_plan_structure(plan, a, b, c_structure, false);
}

int32_t sprs_hip_spgemm_plan_product_f32(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b,
                                         sprs_hip_csmat_f32 **c) {
    return entry_spgemm_plan_structure(plan, a, b, c, true);
}

int32_t sprs_hip_spgemm_plan_numeric_f32(sprs_hip_spgemm_plan *plan, const sprs_hip_csmat_f32 *a, const sprs_hip_csmat_f32 *b,
                                         sprs_hip_csmat_f32 *c) {
    return entry_spgemm_plan_numeric(plan, a, b, c);
}

int32_t sprs_hip_csmat_mul_csmat_f32(const sprs_hip_csmat_f32 *lhs, const sprs_hip_csmat_f32 *rhs, sprs_hip_csmat_f32 **out) {
    return entry_csmat_mul_csmat(lhs, rhs, out);
}

int32_t sprs_hip_dense_dot_csmat_f32(const float *lhs_dev, uint64_t lhs_rows, uint64_t lhs_cols, int32_t lhs_layout, uint64_t ld_lhs,
                                     const sprs_hip_csmat_f32 *rhs, float *out_dev, int32_t *out_layout, void *stream) {
    return entry_dense_dot(lhs_dev, lhs_rows, lhs_cols, lhs_layout, ld_lhs, rhs, out_dev, out_layout, stream);
}

}  // extern "C"

// the pool and the handle constructors live in handle.hpp, compiled here so that the library and its emulator build (tests/emu,
// a fixed list of translation units) both carry them
#include "handle.hpp"
