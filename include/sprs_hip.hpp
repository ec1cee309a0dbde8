// sprs_hip.hpp — header-only C++ host mirror of the reference interface for
// the SpMV / SpGEMM path, on top of the C ABI (sprs_hip.h).
//
// The reference's host language is Rust; rustc is absent from this build
// environment, so this is the compiled-language host side (the Rust crates in
// rust/ are the same surface, source only).  Names, argument order and failure
// behaviour follow sprs:
//   sprs_hip::prod::mul_acc_mat_vec_csr(mat, in_vec, res_vec)   sprs/src/sparse/prod.rs:103-127
//   sprs_hip::smmp::mul_csr_csr(lhs, rhs)                       sprs/src/sparse/smmp.rs:196-416
//   mat * vec, mat * mat                                        sprs/src/sparse/csmat.rs:1866-1888, 2119-2160
//   DeviceCsMat::eye(n)                                         sprs/src/sparse/csmat.rs:416-426
// Where the reference panics ("Dimension mismatch", "Storage mismatch", "Index
// type is not large enough to hold ..."), sprs_hip::Error is thrown with the
// same text.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "sprs_hip.h"

namespace sprs_hip {

struct Error : std::runtime_error {
    int32_t status;
    Error(int32_t s, const std::string &m) : std::runtime_error(m), status(s) {}
};

inline void check(int32_t status) {
    if (status != SPRS_HIP_OK) throw Error(status, sprs_hip_last_error());
}

// A finding of the structure checks (StructureError, errors.rs): the reference's text, its kind (0 ok, 1 Unsorted,
// 2 SizeMismatch, 3 OutOfRange) and the first offending outer slice (~0 for the dimensions or the indptr, 0 for a vector)
struct StructureError : Error {
    int32_t kind;
    uint64_t outer;
    StructureError(int32_t s, const std::string &m, const sprs_hip_structure_info &i) : Error(s, m), kind(i.kind), outer(i.outer) {}
};

inline void check_structure_status(int32_t status, const sprs_hip_structure_info &info) {
    if (status == SPRS_HIP_BAD_STRUCTURE) throw StructureError(status, sprs_hip_last_error(), info);
    check(status);
}

// Dense f64 vector in HBM (what `&[f64]` / `Vec<f64>` / `Array1<f64>` are on the host,
// sprs/src/dense_vector.rs:10-29).
class DeviceVec {
public:
    explicit DeviceVec(uint64_t n) : n_(n) {
        check(sprs_hip_malloc(&p_, n * 8));
        check(sprs_hip_memset(p_, 0, n * 8, nullptr));
    }
    explicit DeviceVec(const std::vector<double> &v) : n_(v.size()) {
        check(sprs_hip_malloc(&p_, n_ * 8));
        check(sprs_hip_memcpy_h2d(p_, v.data(), n_ * 8));
    }
    DeviceVec(DeviceVec &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
    DeviceVec(const DeviceVec &) = delete;
    DeviceVec &operator=(const DeviceVec &) = delete;
    ~DeviceVec() {
        if (p_) sprs_hip_free(p_);
    }
    uint64_t dim() const { return n_; }
    double *ptr() { return static_cast<double *>(p_); }
    const double *ptr() const { return static_cast<const double *>(p_); }
    std::vector<double> to_host() const {
        std::vector<double> out(n_);
        check(sprs_hip_synchronize(nullptr));
        check(sprs_hip_memcpy_d2h(out.data(), p_, n_ * 8));
        return out;
    }

private:
    void *p_ = nullptr;
    uint64_t n_ = 0;
};

// Device twin of CsMatI<f64, I, Iptr> (sprs/src/sparse.rs:94-122).
class DeviceCsMat {
public:
    // CsMat::new / new_csc (validate = true) or new_trusted (validate = false)
    template <typename I, typename Iptr>
    DeviceCsMat(int32_t storage, uint64_t rows, uint64_t cols, const std::vector<Iptr> &indptr,
                const std::vector<I> &indices, const std::vector<double> &data, bool validate = true) {
        static_assert(std::is_integral<I>::value && std::is_integral<Iptr>::value, "SpIndex types");
        static_assert(sizeof(I) == 4 || sizeof(I) == 8, "I must be 4 or 8 bytes");
        static_assert(sizeof(Iptr) == 4 || sizeof(Iptr) == 8, "Iptr must be 4 or 8 bytes");
        check(sprs_hip_csmat_upload(&h_, storage, rows, cols, indptr.data(), (int32_t)sizeof(Iptr), indices.data(),
                                    (int32_t)sizeof(I), data.data(), validate ? 1 : 0));
    }
    explicit DeviceCsMat(sprs_hip_csmat *h) : h_(h) {}
    DeviceCsMat(DeviceCsMat &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DeviceCsMat(const DeviceCsMat &) = delete;
    DeviceCsMat &operator=(const DeviceCsMat &) = delete;
    ~DeviceCsMat() {
        if (h_) sprs_hip_csmat_free(h_);
    }

    // CsMat::new_from_unsorted / new_from_unsorted_csc (csmat.rs:374-401): uploaded as they are, sorted and validated on the
    // device; throws StructureError
    template <typename I, typename Iptr>
    static DeviceCsMat new_from_unsorted(uint64_t rows, uint64_t cols, const std::vector<Iptr> &indptr, const std::vector<I> &indices,
                                         const std::vector<double> &data, int32_t storage = SPRS_HIP_CSR, void *stream = nullptr) {
        // (the upload sizes its copies by the indptr)
        if (indptr.size() != (storage == SPRS_HIP_CSR ? rows : cols) + 1) throw Error(SPRS_HIP_BAD_STRUCTURE, "Indptr length does not match dimension");
        if (indices.size() != data.size()) throw Error(SPRS_HIP_BAD_STRUCTURE, "data and indices have different sizes");
        if ((uint64_t)indptr.back() - (uint64_t)indptr.front() != indices.size())
            throw Error(SPRS_HIP_BAD_STRUCTURE, "Indices length and inpdtr's nnz do not match");
        return DeviceCsMat(storage, rows, cols, indptr, indices, data, false).sort_indices(stream);
    }
    template <typename I, typename Iptr>
    static DeviceCsMat new_from_unsorted_csc(uint64_t rows, uint64_t cols, const std::vector<Iptr> &indptr, const std::vector<I> &indices,
                                             const std::vector<double> &data, void *stream = nullptr) {
        return new_from_unsorted(rows, cols, indptr, indices, data, SPRS_HIP_CSC, stream);
    }
    // utils::check_compressed_structure (sparse.rs:300-358) on the device arrays; throws StructureError
    void check_structure(void *stream = nullptr) const {
        sprs_hip_structure_info info{};
        check_structure_status(sprs_hip_csmat_check_structure(h_, &info, stream), info);
    }
    // a new matrix whose outer slices are sorted by inner index, validated; this one is only read
    DeviceCsMat sort_indices(void *stream = nullptr) const {
        sprs_hip_structure_info info{};
        sprs_hip_csmat *c = nullptr;
        check_structure_status(sprs_hip_csmat_from_unsorted(h_, &c, &info, stream), info);
        return DeviceCsMat(c);
    }

    static DeviceCsMat eye(uint64_t dim) {   // csmat.rs:416-426
        std::vector<uint64_t> indptr(dim + 1), indices(dim);
        for (uint64_t i = 0; i <= dim; ++i) indptr[i] = i;
        for (uint64_t i = 0; i < dim; ++i) indices[i] = i;
        return DeviceCsMat(SPRS_HIP_CSR, dim, dim, indptr, indices, std::vector<double>(dim, 1.0), false);
    }

    uint64_t rows() const { return info().rows; }
    uint64_t cols() const { return info().cols; }
    uint64_t nnz() const { return info().nnz; }
    bool is_csr() const { return info().storage == SPRS_HIP_CSR; }
    const sprs_hip_csmat *handle() const { return h_; }
    // build the full SpMV plan now instead of at the handle's second multiply (sprs_hip_csmat_prepare): for callers that iterate
    void prepare(void *stream = nullptr) { check(sprs_hip_csmat_prepare(h_, stream)); }

    // CsMat::degrees (csmat.rs:1205-1216): per outer index the stored entries off the diagonal
    std::vector<uint64_t> degrees(void *stream = nullptr) const {
        const Info i = info();
        const uint64_t outer = i.storage == SPRS_HIP_CSR ? i.rows : i.cols;
        std::vector<uint64_t> out(outer);
        DeviceVec buf(outer);                        // (8 bytes per word)
        check(sprs_hip_csmat_degrees(h_, (uint64_t *)buf.ptr(), stream));
        check(sprs_hip_synchronize(stream));
        if (outer) check(sprs_hip_memcpy_d2h(out.data(), buf.ptr(), outer * 8));
        return out;
    }
    // CsMat::max_outer_nnz (csmat.rs:1188-1193)
    uint64_t max_outer_nnz(void *stream = nullptr) const {
        uint64_t v = 0;
        check(sprs_hip_csmat_max_outer_nnz(h_, &v, stream));
        return v;
    }

    // into_raw_storage (csmat.rs:946-954) for 8-byte handles
    void to_host(std::vector<uint64_t> &indptr, std::vector<uint64_t> &indices, std::vector<double> &data) const {
        const Info i = info();
        if (i.iptr_bytes != 8 || i.idx_bytes != 8) throw Error(SPRS_HIP_INVALID_ARG, "to_host: 64-bit handles only");
        const uint64_t outer = i.storage == SPRS_HIP_CSR ? i.rows : i.cols;
        indptr.resize(outer + 1);
        indices.resize(i.nnz);
        data.resize(i.nnz);
        check(sprs_hip_csmat_download(h_, indptr.data(), indices.data(), data.data()));
    }

private:
    struct Info {
        uint64_t rows, cols, nnz;
        int32_t iptr_bytes, idx_bytes, storage;
    };
    Info info() const {
        Info i{};
        check(sprs_hip_csmat_info(h_, &i.rows, &i.cols, &i.nnz, &i.iptr_bytes, &i.idx_bytes, &i.storage));
        return i;
    }
    sprs_hip_csmat *h_ = nullptr;
};

// Dense f64 matrix in HBM in one of ndarray's two contiguous layouts: `Array2` in standard (row-major) order or
// `Array::zeros(shape.f())` (column-major) — what `&CsMat * &Array2` returns for fewer than 8 columns (csmat.rs:2017-2024).
class DeviceMat {
public:
    DeviceMat(uint64_t rows, uint64_t cols, bool col_major = false) : buf_(rows * cols), rows_(rows), cols_(cols), col_major_(col_major) {}
    // elements in memory order of the chosen layout
    DeviceMat(uint64_t rows, uint64_t cols, const std::vector<double> &elems, bool col_major = false)
        : buf_(elems), rows_(rows), cols_(cols), col_major_(col_major) {
        if (elems.size() != rows * cols) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    }
    uint64_t rows() const { return rows_; }
    uint64_t cols() const { return cols_; }
    bool is_standard_layout() const { return !col_major_; }
    int32_t layout() const { return col_major_ ? SPRS_HIP_COL_MAJOR : SPRS_HIP_ROW_MAJOR; }
    uint64_t ld() const { return col_major_ ? rows_ : cols_; }
    double *ptr() { return buf_.ptr(); }
    const double *ptr() const { return buf_.ptr(); }
    void set_layout(int32_t layout) { col_major_ = layout == SPRS_HIP_COL_MAJOR; }
    double at(const std::vector<double> &host, uint64_t i, uint64_t j) const { return col_major_ ? host[j * rows_ + i] : host[i * cols_ + j]; }
    std::vector<double> to_host() const { return buf_.to_host(); }       // memory order

private:
    DeviceVec buf_;
    uint64_t rows_, cols_;
    bool col_major_;
};

namespace prod {
// prod::mul_acc_mat_vec_csr (prod.rs:103-127): res_vec += mat * in_vec
inline void mul_acc_mat_vec_csr(const DeviceCsMat &mat, const DeviceVec &in_vec, DeviceVec &res_vec,
                                void *stream = nullptr) {
    check(sprs_hip_spmv_f64(mat.handle(), in_vec.ptr(), in_vec.dim(), res_vec.ptr(), res_vec.dim(), 1, stream));
}
// prod::mul_acc_mat_vec_csc (prod.rs:74-99): res_vec += mat * in_vec for a CSC matrix
inline void mul_acc_mat_vec_csc(const DeviceCsMat &mat, const DeviceVec &in_vec, DeviceVec &res_vec, void *stream = nullptr) {
    check(sprs_hip_mul_acc_mat_vec_csc_f64(mat.handle(), in_vec.ptr(), in_vec.dim(), res_vec.ptr(), res_vec.dim(), stream));
}
namespace detail {
inline void mulacc_dense(const DeviceCsMat &lhs, bool want_csr, const DeviceMat &rhs, DeviceMat &out, void *stream) {
    if (rhs.cols() != out.cols()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");       // prod.rs:201, 230, 259, 287
    if (lhs.is_csr() != want_csr) {                                                                // prod.rs:202, 231, 258, 288 (after the dimensions)
        if (lhs.cols() != rhs.rows() || lhs.rows() != out.rows()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
        throw Error(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    }
    check(sprs_hip_csmat_mulacc_dense_f64(lhs.handle(), rhs.ptr(), rhs.rows(), rhs.cols(), rhs.layout(), rhs.ld(), out.ptr(),
                                          out.rows(), out.layout(), out.ld(), 1, stream));
}
}  // namespace detail
// prod::csr_mulacc_dense_rowmaj / _colmaj (prod.rs:189-214, 274-298), csc_mulacc_dense_rowmaj / _colmaj (prod.rs:219-270):
// out += lhs * rhs.  In the reference the four differ in their loop order; the device entry is told by the operands' own
// layouts how to address them.
inline void csr_mulacc_dense_rowmaj(const DeviceCsMat &lhs, const DeviceMat &rhs, DeviceMat &out, void *stream = nullptr) { detail::mulacc_dense(lhs, true, rhs, out, stream); }
inline void csr_mulacc_dense_colmaj(const DeviceCsMat &lhs, const DeviceMat &rhs, DeviceMat &out, void *stream = nullptr) { detail::mulacc_dense(lhs, true, rhs, out, stream); }
inline void csc_mulacc_dense_rowmaj(const DeviceCsMat &lhs, const DeviceMat &rhs, DeviceMat &out, void *stream = nullptr) { detail::mulacc_dense(lhs, false, rhs, out, stream); }
inline void csc_mulacc_dense_colmaj(const DeviceCsMat &lhs, const DeviceMat &rhs, DeviceMat &out, void *stream = nullptr) { detail::mulacc_dense(lhs, false, rhs, out, stream); }
}  // namespace prod

namespace smmp {
// smmp::mul_csr_csr (smmp.rs:196-416)
inline DeviceCsMat mul_csr_csr(const DeviceCsMat &lhs, const DeviceCsMat &rhs) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_spgemm_f64(lhs.handle(), rhs.handle(), &c));
    return DeviceCsMat(c);
}
}  // namespace smmp

// `&A * &x` (csmat.rs:2119-2160): fresh result
namespace smmp {
// smmp::symbolic (smmp.rs:81-131): structure of lhs * rhs, values 0.0
inline DeviceCsMat symbolic(const DeviceCsMat &lhs, const DeviceCsMat &rhs) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_spgemm_symbolic(lhs.handle(), rhs.handle(), &c));
    return DeviceCsMat(c);
}
// smmp::numeric (smmp.rs:151-189): values of lhs * rhs into c, which must have the product's structure
inline void numeric(const DeviceCsMat &lhs, const DeviceCsMat &rhs, DeviceCsMat &c) {
    check(sprs_hip_spgemm_numeric(lhs.handle(), rhs.handle(), const_cast<sprs_hip_csmat *>(c.handle())));
}
}  // namespace smmp

inline DeviceVec operator*(const DeviceCsMat &a, const DeviceVec &x) {      // CSR or CSC: dispatched below the C ABI (csmat.rs:2140-2156)
    DeviceVec y(a.rows());
    check(sprs_hip_csmat_mul_vec_f64(a.handle(), x.ptr(), x.dim(), y.ptr(), y.dim(), nullptr));
    return y;
}

// `&A * &M` (csmat.rs:1989-2048): the four arms (CSR | CSC) x (>= 8 columns | fewer) below the C ABI; the result is in standard
// layout from 8 columns on and in `.f()` layout below, like the reference's
inline DeviceMat operator*(const DeviceCsMat &a, const DeviceMat &m) {
    DeviceMat out(a.rows(), m.cols());
    int32_t lay = SPRS_HIP_ROW_MAJOR;
    check(sprs_hip_csmat_mul_dense_f64(a.handle(), m.ptr(), m.rows(), m.cols(), m.layout(), m.ld(), out.ptr(), &lay, nullptr));
    out.set_layout(lay);
    return out;
}

// `Array2::dot(&CsMat)` (csmat.rs:2050-2117): dense . sparse
inline DeviceMat dot(const DeviceMat &lhs, const DeviceCsMat &rhs) {
    DeviceMat out(lhs.rows(), rhs.cols());
    int32_t lay = SPRS_HIP_ROW_MAJOR;
    check(sprs_hip_dense_dot_csmat_f64(lhs.ptr(), lhs.rows(), lhs.cols(), lhs.layout(), lhs.ld(), rhs.handle(), out.ptr(), &lay, nullptr));
    out.set_layout(lay);
    return out;
}

// TriMatBase::to_csr / to_csc (triplet_iter.rs:127-224) for triplets in HBM: sorted by (row, col), duplicates summed in
// triplet order — the device assembly kernel (sprs_hip_triplets_to_cs), usize indices
inline DeviceCsMat triplets_to_cs(uint64_t rows, uint64_t cols, const std::vector<uint64_t> &row_inds, const std::vector<uint64_t> &col_inds,
                                  const std::vector<double> &data, int32_t storage = SPRS_HIP_CSR) {
    if (row_inds.size() != data.size() || col_inds.size() != data.size()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    const uint64_t n = data.size();
    void *r = nullptr, *c = nullptr;
    DeviceVec v(data);
    check(sprs_hip_malloc(&r, n * 8));
    if (int32_t st = sprs_hip_malloc(&c, n * 8)) { sprs_hip_free(r); check(st); }
    sprs_hip_csmat *h = nullptr;
    int32_t st = sprs_hip_memcpy_h2d(r, row_inds.data(), n * 8);
    if (st == SPRS_HIP_OK) st = sprs_hip_memcpy_h2d(c, col_inds.data(), n * 8);
    if (st == SPRS_HIP_OK) st = sprs_hip_triplets_to_cs(rows, cols, n, r, c, 8, v.ptr(), storage, 8, 8, &h);
    sprs_hip_free(r);
    sprs_hip_free(c);
    check(st);
    return DeviceCsMat(h);
}

// Row-sharded SpMV over the GPUs of one node (no counterpart in the reference; the shard of a rank is a.slice_outer(r0..r1),
// slicing.rs:65-89): one process per GPU; DistSpMV::unique_id() on one rank, handed to all (MPI, a file, ...)
class DistSpMV {
public:
    static std::vector<unsigned char> unique_id() {
        std::vector<unsigned char> id(128);
        check(sprs_hip_dist_unique_id(id.data()));
        return id;
    }
    DistSpMV(const std::vector<unsigned char> &id, int32_t world, int32_t rank, uint64_t rows, uint64_t cols,
             const std::vector<uint64_t> &row_starts, const DeviceCsMat &local_block, int32_t nsub = 2) {
        if ((int64_t)row_starts.size() != (int64_t)world + 1) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
        check(sprs_hip_dist_create(&d_, world > 1 ? id.data() : nullptr, world, rank, rows, cols, row_starts.data(), local_block.handle(), nsub));
    }
    DistSpMV(const DistSpMV &) = delete;
    DistSpMV &operator=(const DistSpMV &) = delete;
    ~DistSpMV() {
        if (d_) sprs_hip_dist_free(d_);
    }
    void mul(const DeviceVec &x, DeviceVec &y, void *stream = nullptr) {     // collective: y = A * x
        check(sprs_hip_dist_spmv_f64(d_, x.ptr(), x.dim(), y.ptr(), y.dim(), stream));
    }
    int32_t comm_count() const {                                             // ranks of the RCCL communicator (ncclCommCount)
        int32_t n = 0;
        check(sprs_hip_dist_comm_count(d_, &n));
        return n;
    }
    // the peer-store route (sprs_hip.h): export this rank's window, connect with every rank's handle (rank order), choose the route
    std::vector<unsigned char> peer_handle() {
        std::vector<unsigned char> h(64);
        check(sprs_hip_dist_peer_handle(d_, h.data()));
        return h;
    }
    void peer_connect(const std::vector<unsigned char> &all_handles, int32_t world) {
        if ((int64_t)all_handles.size() != (int64_t)world * 64) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
        check(sprs_hip_dist_peer_connect(d_, all_handles.data(), world));
    }
    void set_route(int32_t route) { check(sprs_hip_dist_set_route(d_, route)); }
    int32_t route() const {
        int32_t r = 0;
        check(sprs_hip_dist_route(d_, &r));
        return r;
    }

private:
    sprs_hip_dist *d_ = nullptr;
};

// `&A * &B` (csmat.rs:1866-1888)
// `&A * &B`: csmat_mul_csmat (csmat.rs:1895-1949) — the storage dispatch is done below the C ABI
inline DeviceCsMat operator*(const DeviceCsMat &a, const DeviceCsMat &b) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_mul_csmat(a.handle(), b.handle(), &c));
    return DeviceCsMat(c);
}

// Device twin of CsVecI<f64, I> (sparse.rs:165-173): dim, sorted indices, data.
class DeviceCsVec {
public:
    // CsVec::new (validate = true, vec.rs:430-434) or new_trusted (validate = false); I of 2, 4 or 8 bytes
    template <typename I>
    DeviceCsVec(uint64_t dim, const std::vector<I> &indices, const std::vector<double> &data, bool validate = true) {
        static_assert(std::is_integral<I>::value, "SpIndex type");
        static_assert(sizeof(I) == 2 || sizeof(I) == 4 || sizeof(I) == 8, "I must be 2, 4 or 8 bytes");
        if (indices.size() != data.size()) throw Error(SPRS_HIP_BAD_STRUCTURE, "indices and data do not have compatible lengths");
        check(sprs_hip_csvec_upload(&h_, dim, indices.size(), indices.data(), (int32_t)sizeof(I), data.data(), validate ? 1 : 0));
    }
    explicit DeviceCsVec(sprs_hip_csvec *h) : h_(h) {}
    DeviceCsVec(DeviceCsVec &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DeviceCsVec(const DeviceCsVec &) = delete;
    DeviceCsVec &operator=(const DeviceCsVec &) = delete;
    ~DeviceCsVec() {
        if (h_) sprs_hip_csvec_free(h_);
    }

    // CsVec::new_from_unsorted (vec.rs:536-557): check, sort only on Unsorted, check again — on the device
    template <typename I>
    static DeviceCsVec new_from_unsorted(uint64_t dim, const std::vector<I> &indices, const std::vector<double> &data, void *stream = nullptr) {
        return DeviceCsVec(dim, indices, data, false).sort_indices(stream);
    }
    // the invariants of CsVec::try_new (vec.rs:440-491) on the device arrays; throws StructureError
    void check_structure(void *stream = nullptr) const {
        sprs_hip_structure_info info{};
        check_structure_status(sprs_hip_csvec_check_structure(h_, &info, stream), info);
    }
    DeviceCsVec sort_indices(void *stream = nullptr) const {
        sprs_hip_structure_info info{};
        sprs_hip_csvec *c = nullptr;
        check_structure_status(sprs_hip_csvec_from_unsorted(h_, &c, &info, stream), info);
        return DeviceCsVec(c);
    }

    uint64_t dim() const { return info().dim; }      // vec.rs:681
    uint64_t nnz() const { return info().nnz; }      // vec.rs:686
    const sprs_hip_csvec *handle() const { return h_; }

    // into_raw_storage (vec.rs:675) for 8-byte handles
    void to_host(std::vector<uint64_t> &indices, std::vector<double> &data) const {
        const Info i = info();
        if (i.idx_bytes != 8) throw Error(SPRS_HIP_INVALID_ARG, "to_host: 64-bit handles only");
        indices.resize(i.nnz);
        data.resize(i.nnz);
        check(sprs_hip_csvec_download(h_, indices.data(), data.data()));
    }
    // CsVec::to_dense (vec.rs:621)
    DeviceVec to_dense(void *stream = nullptr) const {
        DeviceVec out(dim());
        check(sprs_hip_csvec_scatter_f64(h_, out.ptr(), out.dim(), stream));
        return out;
    }

    // Reductions (vec.rs:787-958, 1051-1061; prod.rs:14-70): every sum is the reference's left-to-right chain from +0.0, bit for
    // bit; the one documented difference is the sign of a zero result of dot_dense and of the norms (sprs_hip.h).
    double dot(const DeviceCsVec &rhs, void *stream = nullptr) const {          // vec.rs:828-881; throws "Dimension mismatch"
        double out = 0.0;
        check(sprs_hip_csvec_dot_f64(h_, rhs.h_, &out, stream));
        return out;
    }
    double dot(const DeviceVec &rhs, void *stream = nullptr) const { return dot_dense(rhs, stream); }
    double dot_dense(const DeviceVec &rhs, void *stream = nullptr) const {      // vec.rs:894-904
        double out = 0.0;
        check(sprs_hip_csvec_dot_dense_f64(h_, rhs.ptr(), rhs.dim(), &out, stream));
        return out;
    }
    double squared_l2_norm(void *stream = nullptr) const { return norm_kind(SPRS_HIP_NORM_SQUARED_L2, 0.0, stream); }   // vec.rs:907-913
    double l2_norm(void *stream = nullptr) const { return norm_kind(SPRS_HIP_NORM_L2, 0.0, stream); }                   // vec.rs:916-922
    double l1_norm(void *stream = nullptr) const { return norm_kind(SPRS_HIP_NORM_L1, 0.0, stream); }                   // vec.rs:925-930
    double norm(double p, void *stream = nullptr) const { return norm_kind(SPRS_HIP_NORM_P, p, stream); }               // vec.rs:939-958
    // unit_normalize (vec.rs:1051-1061) as a NEW vector: handles are immutable snapshots; a zero vector comes back as a copy
    DeviceCsVec unit_normalize(void *stream = nullptr) const {
        sprs_hip_csvec *c = nullptr;
        check(sprs_hip_csvec_unit_normalize_f64(h_, &c, stream));
        return DeviceCsVec(c);
    }
    // nnz_index / get (vec.rs:787-805), batched: pos[q] = the position in the stored arrays or UINT64_MAX, val[q] = the value or 0.0
    void nnz_index(const std::vector<uint64_t> &indices, std::vector<uint64_t> &pos, std::vector<double> &val, void *stream = nullptr) const {
        const uint64_t nq = indices.size();
        DeviceVec q(nq ? nq : 1), p(nq ? nq : 1), v(nq ? nq : 1);
        if (nq) check(sprs_hip_memcpy_h2d(q.ptr(), indices.data(), nq * 8));
        check(sprs_hip_csvec_nnz_index(h_, nq, reinterpret_cast<const uint64_t *>(q.ptr()), reinterpret_cast<uint64_t *>(p.ptr()), v.ptr(), stream));
        check(sprs_hip_synchronize(stream));
        pos.resize(nq);
        val.resize(nq);
        if (nq) check(sprs_hip_memcpy_d2h(pos.data(), p.ptr(), nq * 8));
        if (nq) check(sprs_hip_memcpy_d2h(val.data(), v.ptr(), nq * 8));
    }

private:
    struct Info {
        uint64_t dim, nnz;
        int32_t idx_bytes;
    };
    Info info() const {
        Info i{};
        check(sprs_hip_csvec_info(h_, &i.dim, &i.nnz, &i.idx_bytes));
        return i;
    }
    double norm_kind(int32_t kind, double p, void *stream) const {
        double out = 0.0;
        check(sprs_hip_csvec_norm_f64(h_, kind, p, &out, stream));
        return out;
    }
    sprs_hip_csvec *h_ = nullptr;
};

namespace prod {
// prod::csvec_dot_by_binary_search (prod.rs:14-70): on the device the same function as CsVec::dot
inline double csvec_dot_by_binary_search(const DeviceCsVec &vec1, const DeviceCsVec &vec2, void *stream = nullptr) { return vec1.dot(vec2, stream); }
}  // namespace prod

// Extraction (csmat.rs:1017-1056, 1219-1256, 1312-1351).
// outer_view (csmat.rs:1219-1231): zero-copy — the vector BORROWS m's arrays and must not outlive m; `found` = false (and an
// empty handle that must not be used) when i >= outer dims, the reference's None
inline DeviceCsVec outer_view(const DeviceCsMat &m, uint64_t i, bool *found, void *stream = nullptr) {
    sprs_hip_csvec *c = nullptr;
    check(sprs_hip_csmat_outer_view(m.handle(), i, &c, stream));
    if (found) *found = c != nullptr;
    return DeviceCsVec(c);
}
// diag (csmat.rs:1234-1256): structural, an explicit 0.0 on the diagonal is kept
inline DeviceCsVec diag(const DeviceCsMat &m, void *stream = nullptr) {
    sprs_hip_csvec *c = nullptr;
    check(sprs_hip_csmat_diag_f64(m.handle(), &c, stream));
    return DeviceCsVec(c);
}
// nnz_index / get (csmat.rs:1312-1351), batched over (row, col) pairs: pos[q] = the global position or UINT64_MAX, val[q] = the
// value or 0.0
inline void nnz_index(const DeviceCsMat &m, const std::vector<uint64_t> &rows, const std::vector<uint64_t> &cols, std::vector<uint64_t> &pos,
                      std::vector<double> &val, void *stream = nullptr) {
    if (rows.size() != cols.size()) throw Error(SPRS_HIP_INVALID_ARG, "rows and cols differ in length");
    const uint64_t nq = rows.size();
    DeviceVec r(nq ? nq : 1), c(nq ? nq : 1), p(nq ? nq : 1), v(nq ? nq : 1);
    if (nq) check(sprs_hip_memcpy_h2d(r.ptr(), rows.data(), nq * 8));
    if (nq) check(sprs_hip_memcpy_h2d(c.ptr(), cols.data(), nq * 8));
    check(sprs_hip_csmat_nnz_index(m.handle(), nq, reinterpret_cast<const uint64_t *>(r.ptr()), reinterpret_cast<const uint64_t *>(c.ptr()),
                                   reinterpret_cast<uint64_t *>(p.ptr()), v.ptr(), stream));
    check(sprs_hip_synchronize(stream));
    pos.resize(nq);
    val.resize(nq);
    if (nq) check(sprs_hip_memcpy_d2h(pos.data(), p.ptr(), nq * 8));
    if (nq) check(sprs_hip_memcpy_d2h(val.data(), v.ptr(), nq * 8));
}
// to_inner_onehot (csmat.rs:1017-1056): the LAST of equal maxima, NaNs skipped
inline DeviceCsMat to_inner_onehot(const DeviceCsMat &m, void *stream = nullptr) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_to_inner_onehot_f64(m.handle(), &c, stream));
    return DeviceCsMat(c);
}

// `&CsMat * &CsVec` (vec.rs:1104-1131): csr_mul_csvec for CSR, structural for CSC; `&CsVec * &CsMat` (vec.rs:1084-1102)
inline DeviceCsVec operator*(const DeviceCsMat &a, const DeviceCsVec &v) {
    sprs_hip_csvec *c = nullptr;
    check(sprs_hip_csmat_mul_csvec_f64(a.handle(), v.handle(), &c, nullptr));
    return DeviceCsVec(c);
}
inline DeviceCsVec operator*(const DeviceCsVec &v, const DeviceCsMat &b) {
    sprs_hip_csvec *c = nullptr;
    check(sprs_hip_csvec_mul_csmat_f64(v.handle(), b.handle(), &c, nullptr));
    return DeviceCsVec(c);
}
namespace prod {
// prod::csr_mul_csvec (prod.rs:161-184)
inline DeviceCsVec csr_mul_csvec(const DeviceCsMat &a, const DeviceCsVec &v) {
    if (!a.is_csr()) throw Error(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    return a * v;
}
}  // namespace prod

// Twin of sprs::binop (sprs/src/sparse/binop.rs): one IEEE operation per result entry, the reference's bits.
namespace binop {
// csmat_binop (binop.rs:178-223), op = SPRS_HIP_BINOP_ADD | _SUB | _MUL: equal shapes and storages, entries with val == 0 dropped
inline DeviceCsMat csmat_binop(const DeviceCsMat &lhs, const DeviceCsMat &rhs, int32_t op, void *stream = nullptr) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_binop_f64(lhs.handle(), rhs.handle(), op, &c, stream));
    return DeviceCsMat(c);
}
// mul_mat_same_storage (binop.rs:115-130): the elementwise product
inline DeviceCsMat mul_mat_same_storage(const DeviceCsMat &lhs, const DeviceCsMat &rhs, void *stream = nullptr) {
    return csmat_binop(lhs, rhs, SPRS_HIP_BINOP_MUL, stream);
}
// csvec_binop (binop.rs:442-467): every merged index is kept; a dimension of 0 takes the other operand's
inline DeviceCsVec csvec_binop(const DeviceCsVec &lhs, const DeviceCsVec &rhs, int32_t op, void *stream = nullptr) {
    sprs_hip_csvec *c = nullptr;
    check(sprs_hip_csvec_binop_f64(lhs.handle(), rhs.handle(), op, &c, stream));
    return DeviceCsVec(c);
}
}  // namespace binop

// `&A + &B`, `&A - &B` (binop.rs:52-64, 99-111): rhs.to_other_storage() first when the storages differ, below the C ABI
inline DeviceCsMat operator+(const DeviceCsMat &a, const DeviceCsMat &b) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_add_csmat_f64(a.handle(), b.handle(), &c, nullptr));
    return DeviceCsMat(c);
}
inline DeviceCsMat operator-(const DeviceCsMat &a, const DeviceCsMat &b) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_sub_csmat_f64(a.handle(), b.handle(), &c, nullptr));
    return DeviceCsMat(c);
}
// `&A * s` (binop.rs:132-163): A.map(|x| x * s), the structure unchanged
inline DeviceCsMat operator*(const DeviceCsMat &a, double s) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_scale_f64(a.handle(), s, &c, nullptr));
    return DeviceCsMat(c);
}
// `&v + &w`, `&v - &w` (vec.rs:1133-1226)
inline DeviceCsVec operator+(const DeviceCsVec &v, const DeviceCsVec &w) { return binop::csvec_binop(v, w, SPRS_HIP_BINOP_ADD); }
inline DeviceCsVec operator-(const DeviceCsVec &v, const DeviceCsVec &w) { return binop::csvec_binop(v, w, SPRS_HIP_BINOP_SUB); }

// Device twin of PermOwnedI<I> (sparse/permutation.rs:12-28): the Identity variant or perm and perm_inv on the device.
class DevicePerm {
public:
    // PermOwned::new (permutation.rs:52-66); validate = true throws "invalid permutation" where the reference's assert fires
    template <typename I>
    explicit DevicePerm(const std::vector<I> &perm, bool validate = true) {
        static_assert(std::is_integral<I>::value, "SpIndex type");
        static_assert(sizeof(I) == 2 || sizeof(I) == 4 || sizeof(I) == 8, "I must be 2, 4 or 8 bytes");
        check(sprs_hip_perm_upload(&h_, perm.size(), perm.data(), (int32_t)sizeof(I), validate ? 1 : 0));
    }
    explicit DevicePerm(sprs_hip_perm *h) : h_(h) {}
    // Permutation::identity (permutation.rs:113-118): no arrays
    static DevicePerm identity(uint64_t dim, int32_t idx_bytes = 8) {
        sprs_hip_perm *h = nullptr;
        check(sprs_hip_perm_identity(&h, dim, idx_bytes));
        return DevicePerm(h);
    }
    // a copy of dim indices (4 or 8 bytes each) that already live on the device
    static DevicePerm from_device(uint64_t dim, const void *dev_perm, int32_t idx_bytes, bool validate = true, void *stream = nullptr) {
        sprs_hip_perm *h = nullptr;
        check(sprs_hip_perm_from_device(&h, dim, dev_perm, idx_bytes, validate ? 1 : 0, stream));
        return DevicePerm(h);
    }
    DevicePerm(DevicePerm &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DevicePerm(const DevicePerm &) = delete;
    DevicePerm &operator=(const DevicePerm &) = delete;
    ~DevicePerm() {
        if (h_) sprs_hip_perm_free(h_);
    }

    uint64_t dim() const {                           // permutation.rs:139
        uint64_t d = 0;
        check(sprs_hip_perm_info(h_, &d, nullptr, nullptr));
        return d;
    }
    bool is_identity(void *stream = nullptr) const {  // permutation.rs:144-152: the elementwise test
        int32_t flag = 0;
        check(sprs_hip_perm_is_identity(h_, &flag, stream));
        return flag != 0;
    }
    DevicePerm inv() const {                         // permutation.rs:120-137, as a new owning handle
        sprs_hip_perm *h = nullptr;
        check(sprs_hip_perm_inv(h_, &h));
        return DevicePerm(h);
    }
    // vec() / inv_vec() (permutation.rs:211-226) for 8-byte handles
    std::vector<uint64_t> vec() const { return download(false); }
    std::vector<uint64_t> inv_vec() const { return download(true); }
    const sprs_hip_perm *handle() const { return h_; }

private:
    std::vector<uint64_t> download(bool inverse) const {
        uint64_t d = 0;
        int32_t ib = 0;
        check(sprs_hip_perm_info(h_, &d, &ib, nullptr));
        if (ib != 8) throw Error(SPRS_HIP_INVALID_ARG, "vec: 64-bit handles only");
        std::vector<uint64_t> out(d);
        check(sprs_hip_perm_download(h_, inverse ? nullptr : out.data(), inverse ? out.data() : nullptr));
        return out;
    }
    sprs_hip_perm *h_ = nullptr;
};

// `&P * x` (permutation.rs:255-278): y[i] = x[p[i]]
inline DeviceVec operator*(const DevicePerm &p, const DeviceVec &x) {
    DeviceVec y(x.dim());
    check(sprs_hip_perm_mul_vec_f64(p.handle(), x.ptr(), y.ptr(), x.dim(), nullptr));
    return y;
}

// Twin of sprs::sparse::permutation (sprs/src/sparse/permutation.rs:296-581): values are moved, never computed.
namespace permutation {
// transform_mat_paq (permutation.rs:496-581): P * A * Q
inline DeviceCsMat transform_mat_paq(const DeviceCsMat &mat, const DevicePerm &row_perm, const DevicePerm &col_perm, void *stream = nullptr) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_transform_paq(mat.handle(), row_perm.handle(), col_perm.handle(), &c, stream));
    return DeviceCsMat(c);
}
// permute_rows (permutation.rs:407-420): P * A.  (The Identity variant gives a copy; the reference is unreachable!() there.)
inline DeviceCsMat permute_rows(const DeviceCsMat &mat, const DevicePerm &perm, void *stream = nullptr) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_transform_paq(mat.handle(), perm.handle(), nullptr, &c, stream));
    return DeviceCsMat(c);
}
// permute_cols (permutation.rs:423-436): A * P
inline DeviceCsMat permute_cols(const DeviceCsMat &mat, const DevicePerm &perm, void *stream = nullptr) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_transform_paq(mat.handle(), nullptr, perm.handle(), &c, stream));
    return DeviceCsMat(c);
}
// transform_mat_papt (permutation.rs:439-491): P * A * P^T, A square and of the permutation's dimension
inline DeviceCsMat transform_mat_papt(const DeviceCsMat &mat, const DevicePerm &perm, void *stream = nullptr) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_transform_papt(mat.handle(), perm.handle(), &c, stream));
    return DeviceCsMat(c);
}
}  // namespace permutation

// Twin of sprs::sparse::linalg::ordering (linalg/ordering.rs) and of sprs::sparse::symmetric::is_symmetric: the matrix stays on
// the device and the permutation arrives there, ready for permutation::transform_mat_papt.  The result is the reference's with
// ties between vertices of equal degree broken by vertex id (the stable outcome of its sort_unstable_by_key).
namespace ordering {
enum class Start : int32_t {                         // start::{Next, MinimumDegree, PseudoPeripheral} (ordering.rs:14-267)
    Next = SPRS_HIP_START_NEXT,
    MinimumDegree = SPRS_HIP_START_MINIMUM_DEGREE,
    PseudoPeripheral = SPRS_HIP_START_PSEUDO_PERIPHERAL,
};
enum class Order : int32_t { Forward = 0, Reversed = 1 };   // order::{Forward, Reversed} (ordering.rs:269-420)

struct Ordering {                                    // ordering.rs:7-12
    DevicePerm perm;
    std::vector<uint64_t> connected_parts;
    uint64_t stats[4];                               // components, levels of the ordering pass, launches, host read-backs
};

// cuthill_mckee_custom (ordering.rs:440-526); a non-square matrix throws the text of the reference's assert_eq!,
// check_symmetric = true is its debug_assert!(is_symmetric(&mat)): "matrix is not symmetric"
inline Ordering cuthill_mckee_custom(const DeviceCsMat &mat, Start start, Order order, bool check_symmetric = false, void *stream = nullptr) {
    struct Handle {
        sprs_hip_ordering *o = nullptr;
        ~Handle() {
            if (o) sprs_hip_ordering_free(o);
        }
    } h;
    check(sprs_hip_csmat_cuthill_mckee(mat.handle(), (int32_t)start, (int32_t)order, check_symmetric ? 1 : 0, &h.o, stream));
    uint64_t n_parts = 0, stats[4] = {0, 0, 0, 0};
    check(sprs_hip_ordering_info(h.o, nullptr, &n_parts, stats));
    std::vector<uint64_t> parts(n_parts);
    check(sprs_hip_ordering_parts(h.o, parts.data()));
    sprs_hip_perm *p = nullptr;
    check(sprs_hip_ordering_perm(h.o, &p));
    return Ordering{DevicePerm(p), std::move(parts), {stats[0], stats[1], stats[2], stats[3]}};
}
// reverse_cuthill_mckee (ordering.rs:546-559)
inline Ordering reverse_cuthill_mckee(const DeviceCsMat &mat, void *stream = nullptr) {
    return cuthill_mckee_custom(mat, Start::PseudoPeripheral, Order::Reversed, false, stream);
}
// is_symmetric (symmetric.rs:7-34)
inline bool is_symmetric(const DeviceCsMat &mat, void *stream = nullptr) {
    int32_t flag = 0;
    check(sprs_hip_csmat_is_symmetric(mat.handle(), &flag, stream));
    return flag != 0;
}
}  // namespace ordering

// Twin of the sprs-ldl crate (sprs-ldl/src/lib.rs): P A P^T = L D L^T on the device, f64.  l_colptr, the elimination tree,
// l_indices and every bit of l_data, d and the solutions are the reference's.  Its panics and its Err(SingularMatrix) arrive as
// exceptions with its text (SPRS_HIP_SINGULAR_MATRIX: SingularMatrix::index holds the pivot).
namespace ldl {
enum class FillInReduction { NoReduction, ReverseCuthillMcKee, CAMDSuiteSparse };

struct SingularMatrix : Error {                      // LinalgError::SingularMatrix (lib.rs:585-590)
    uint64_t index;
    SingularMatrix(const std::string &m, uint64_t k) : Error(SPRS_HIP_SINGULAR_MATRIX, m), index(k) {}
};

class LdlNumeric {                                   // lib.rs:102-111, 326-442
public:
    explicit LdlNumeric(sprs_hip_ldl_num *h, uint64_t n, uint64_t nnz) : h_(h), n_(n), nnz_(nnz) {}
    LdlNumeric(LdlNumeric &&o) noexcept : h_(o.h_), n_(o.n_), nnz_(o.nnz_) { o.h_ = nullptr; }
    LdlNumeric(const LdlNumeric &) = delete;
    LdlNumeric &operator=(const LdlNumeric &) = delete;
    ~LdlNumeric() {
        if (h_) sprs_hip_ldl_numeric_free(h_);
    }
    // update (lib.rs:364-381): new values on the pattern that was analysed
    void update(const DeviceCsMat &mat, void *stream = nullptr) {
        sprs_hip_trisolve_info info{};
        const int32_t st = sprs_hip_ldl_update_f64(h_, mat.handle(), &info, stream);
        if (st == SPRS_HIP_SINGULAR_MATRIX) throw SingularMatrix(sprs_hip_last_error(), info.singular_index);
        check(st);
    }
    // solve (lib.rs:388-410)
    DeviceVec solve(const DeviceVec &rhs, void *stream = nullptr) const {
        DeviceVec x(rhs.dim());
        check(sprs_hip_ldl_solve_f64(h_, rhs.ptr(), x.ptr(), rhs.dim(), stream));
        return x;
    }
    DeviceVec d(void *stream = nullptr) const {      // lib.rs:413
        DeviceVec out(n_);
        check(sprs_hip_ldl_d(h_, out.ptr(), n_, stream));
        check(sprs_hip_synchronize(stream));
        return out;
    }
    DeviceCsMat l(void *stream = nullptr) const {    // lib.rs:418-429: CSC, no diagonal stored
        sprs_hip_csmat *c = nullptr;
        check(sprs_hip_ldl_l(h_, &c, stream));
        return DeviceCsMat(c);
    }
    uint64_t problem_size() const { return n_; }     // lib.rs:433
    uint64_t nnz() const { return nnz_; }            // lib.rs:439

private:
    sprs_hip_ldl_num *h_ = nullptr;
    uint64_t n_ = 0, nnz_ = 0;
};

class LdlSymbolic {                                  // lib.rs:94-100, 228-324
public:
    // new_perm (lib.rs:252-284); perm = nullptr is the identity.  LdlSymbolic::new is (mat, nullptr, true)
    explicit LdlSymbolic(const DeviceCsMat &mat, const DevicePerm *perm = nullptr, bool check_symmetry = true, void *stream = nullptr) {
        check(sprs_hip_ldl_symbolic(mat.handle(), perm ? perm->handle() : nullptr, check_symmetry ? 1 : 0, &h_, stream));
        check(sprs_hip_ldl_symbolic_info(h_, &n_, &nnz_, stats_));
    }
    LdlSymbolic(LdlSymbolic &&o) noexcept : h_(o.h_), n_(o.n_), nnz_(o.nnz_) {
        o.h_ = nullptr;
        for (int k = 0; k < 4; ++k) stats_[k] = o.stats_[k];
    }
    LdlSymbolic(const LdlSymbolic &) = delete;
    LdlSymbolic &operator=(const LdlSymbolic &) = delete;
    ~LdlSymbolic() {
        if (h_) sprs_hip_ldl_symbolic_free(h_);
    }
    uint64_t problem_size() const { return n_; }     // lib.rs:288
    uint64_t nnz() const { return nnz_; }            // lib.rs:294
    const uint64_t *stats() const { return stats_; } // launches of the etree pass, all launches, host read-backs, 0
    std::vector<uint64_t> colptr() const {
        std::vector<uint64_t> out(n_ + 1);
        check(sprs_hip_ldl_symbolic_colptr(h_, out.data()));
        return out;
    }
    std::vector<uint64_t> parents() const {          // UINT64_MAX for a root
        std::vector<uint64_t> out(n_ ? n_ : 1);
        check(sprs_hip_ldl_symbolic_parents(h_, out.data()));
        out.resize(n_);
        return out;
    }
    DevicePerm perm() const {
        sprs_hip_perm *p = nullptr;
        check(sprs_hip_ldl_symbolic_perm(h_, &p));
        return DevicePerm(p);
    }
    // factor (lib.rs:300-323).  The reference consumes self; here the handle stays usable.
    LdlNumeric factor(const DeviceCsMat &mat, void *stream = nullptr) const {
        sprs_hip_ldl_num *f = nullptr;
        sprs_hip_trisolve_info info{};
        const int32_t st = sprs_hip_ldl_factor_f64(h_, mat.handle(), &f, &info, stream);
        if (st == SPRS_HIP_SINGULAR_MATRIX) throw SingularMatrix(sprs_hip_last_error(), info.singular_index);
        check(st);
        return LdlNumeric(f, n_, nnz_);
    }

private:
    sprs_hip_ldl_sym *h_ = nullptr;
    uint64_t n_ = 0, nnz_ = 0, stats_[4] = {0, 0, 0, 0};
};

// The builder (lib.rs:74-226).  Defaults: symmetry checked, reverse Cuthill-McKee; check_perm is kept for the signature and,
// as in the reference's native path, never read.
class Ldl {
public:
    Ldl check_symmetry(bool check) const { return Ldl(check, perm_, fill_); }
    Ldl check_perm(bool check) const { return Ldl(sym_, check, fill_); }
    Ldl fill_in_reduction(FillInReduction method) const { return Ldl(sym_, perm_, method); }
    Ldl() = default;
    LdlSymbolic symbolic(const DeviceCsMat &mat, void *stream = nullptr) const {       // lib.rs:139-170
        if (fill_ == FillInReduction::NoReduction) return LdlSymbolic(mat, nullptr, sym_, stream);
        if (fill_ == FillInReduction::CAMDSuiteSparse)
            throw Error(SPRS_HIP_INVALID_ARG, "Unavailable without the `sprs_suitesparse_camd` feature");
        const ordering::Ordering o = ordering::reverse_cuthill_mckee(mat, stream);
        return LdlSymbolic(mat, &o.perm, sym_, stream);
    }
    LdlNumeric numeric(const DeviceCsMat &mat, void *stream = nullptr) const { return symbolic(mat, stream).factor(mat, stream); }   // lib.rs:190-201

private:
    Ldl(bool sym, bool perm, FillInReduction fill) : sym_(sym), perm_(perm), fill_(fill) {}
    bool sym_ = true, perm_ = true;
    FillInReduction fill_ = FillInReduction::ReverseCuthillMcKee;
};

// ldl_lsolve (lib.rs:597-609), ldl_ltsolve (lib.rs:613-626): in place, l a strictly lower CSC matrix with an implied unit diagonal
inline void ldl_lsolve(const DeviceCsMat &l, DeviceVec &x, void *stream = nullptr) {
    check(sprs_hip_ldl_lsolve_f64(const_cast<sprs_hip_csmat *>(l.handle()), x.ptr(), x.dim(), stream));
}
inline void ldl_ltsolve(const DeviceCsMat &l, DeviceVec &x, void *stream = nullptr) {
    check(sprs_hip_ldl_ltsolve_f64(const_cast<sprs_hip_csmat *>(l.handle()), x.ptr(), x.dim(), stream));
}
// linalg::diag_solve (sprs/src/sparse/linalg.rs:17-29): x[i] /= d[i]
inline void diag_solve(const DeviceVec &d, DeviceVec &x, void *stream = nullptr) {
    if (d.dim() != x.dim()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    check(sprs_hip_diag_solve_f64(d.ptr(), x.ptr(), x.dim(), stream));
}
}  // namespace ldl

// sprs::kronecker_product (kronecker.rs:50-99) and sprs::sparse::construct (construct.rs:10-160) on device handles.  The
// reference's panics arrive as exceptions with its text; kronecker_product refuses by shape (SPRS_HIP_INDEX_OVERFLOW) what
// the reference refuses by stored index.
namespace construct {
namespace detail {
inline std::vector<const sprs_hip_csmat *> handles(const std::vector<const DeviceCsMat *> &mats) {
    std::vector<const sprs_hip_csmat *> h;
    for (const DeviceCsMat *m : mats) h.push_back(m ? m->handle() : nullptr);
    return h;
}
}  // namespace detail
// the result has the storage of a; nothing is dropped
inline DeviceCsMat kronecker_product(const DeviceCsMat &a, const DeviceCsMat &b, void *stream = nullptr) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_kronecker_f64(a.handle(), b.handle(), &c, stream));
    return DeviceCsMat(c);
}
inline DeviceCsMat same_storage_fast_stack(const std::vector<const DeviceCsMat *> &mats, void *stream = nullptr) {
    std::vector<const sprs_hip_csmat *> h = detail::handles(mats);
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_same_storage_fast_stack(h.data(), h.size(), &c, stream));
    return DeviceCsMat(c);
}
inline DeviceCsMat vstack(const std::vector<const DeviceCsMat *> &mats, void *stream = nullptr) {   // always CSR
    std::vector<const sprs_hip_csmat *> h = detail::handles(mats);
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_vstack(h.data(), h.size(), &c, stream));
    return DeviceCsMat(c);
}
inline DeviceCsMat hstack(const std::vector<const DeviceCsMat *> &mats, void *stream = nullptr) {   // always CSC
    std::vector<const sprs_hip_csmat *> h = detail::handles(mats);
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_hstack(h.data(), h.size(), &c, stream));
    return DeviceCsMat(c);
}
// blocks row-major, super_rows x super_cols, nullptr = None; the result is CSR
inline DeviceCsMat bmat(const std::vector<const DeviceCsMat *> &blocks, uint64_t super_rows, uint64_t super_cols, void *stream = nullptr) {
    if (blocks.size() != super_rows * super_cols) throw std::invalid_argument("Dimension mismatch");
    std::vector<const sprs_hip_csmat *> h = detail::handles(blocks);
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_bmat(h.data(), super_rows, super_cols, &c, stream));
    return DeviceCsMat(c);
}
}  // namespace construct

// The dense <-> sparse boundary on device operands: CsMat::csr_from_dense / csc_from_dense (csmat.rs:499-549), assign_to_dense
// and CsMat::to_dense (to_dense.rs:12-30, csmat.rs:1127-1134).  Contiguous DeviceMat operands; the C entries also take a
// leading dimension.
namespace dense {
namespace detail {
inline DeviceCsMat from_dense(int32_t storage, const DeviceMat &m, double epsilon, void *stream) {
    sprs_hip_csmat *c = nullptr;
    check(sprs_hip_csmat_from_dense_f64(&c, storage, m.ptr(), m.rows(), m.cols(), m.layout(), m.ld(), epsilon, 8, 8, stream));
    return DeviceCsMat(c);
}
}  // namespace detail
// the elements with |x| > max(epsilon, 0) (a negative or NaN epsilon is 0), usize indices
inline DeviceCsMat csr_from_dense(const DeviceMat &m, double epsilon, void *stream = nullptr) { return detail::from_dense(SPRS_HIP_CSR, m, epsilon, stream); }
inline DeviceCsMat csc_from_dense(const DeviceMat &m, double epsilon, void *stream = nullptr) { return detail::from_dense(SPRS_HIP_CSC, m, epsilon, stream); }
// array[row, col] = value for every stored entry; the array is not zeroed first
inline void assign_to_dense(DeviceMat &array, const DeviceCsMat &spmat, void *stream = nullptr) {
    check(sprs_hip_csmat_assign_to_dense_f64(spmat.handle(), array.ptr(), array.rows(), array.cols(), array.layout(), array.ld(), stream));
}
// Array::zeros((rows, cols)) — standard layout — then assign_to_dense
inline DeviceMat to_dense(const DeviceCsMat &spmat, void *stream = nullptr) {
    DeviceMat out(spmat.rows(), spmat.cols());
    check(sprs_hip_csmat_to_dense_f64(spmat.handle(), out.ptr(), out.rows(), out.cols(), out.layout(), out.ld(), stream));
    return out;
}
}  // namespace dense

namespace binop {
// csmat_binop_dense_raw (binop.rs:384-433) with one of the two closures the reference ships: op = SPRS_HIP_BINOP_ADD writes
// (alpha * l) + (beta * r), SPRS_HIP_BINOP_MUL (alpha * l) * r, into every element of out; "Dimension mismatch", then "Storage
// mismatch" unless CSR meets standard layout / CSC meets `.f()` layout in both rhs and out
inline void csmat_binop_dense_raw(const DeviceCsMat &lhs, const DeviceMat &rhs, int32_t op, DeviceMat &out, double alpha = 1.0, double beta = 1.0,
                                  void *stream = nullptr) {
    if (lhs.cols() != rhs.cols() || lhs.cols() != out.cols() || lhs.rows() != rhs.rows() || lhs.rows() != out.rows())
        throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (rhs.layout() != out.layout()) throw Error(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    check(sprs_hip_csmat_binop_dense_f64(lhs.handle(), rhs.ptr(), rhs.rows(), rhs.cols(), rhs.layout(), rhs.ld(), op, alpha, beta, out.ptr(),
                                         out.ld(), stream));
}
// add_dense_mat_same_ordering (binop.rs:279-323): alpha * lhs + beta * rhs in rhs' layout
inline DeviceMat add_dense_mat_same_ordering(const DeviceCsMat &lhs, const DeviceMat &rhs, double alpha, double beta, void *stream = nullptr) {
    DeviceMat out(rhs.rows(), rhs.cols(), !rhs.is_standard_layout());
    csmat_binop_dense_raw(lhs, rhs, SPRS_HIP_BINOP_ADD, out, alpha, beta, stream);
    return out;
}
// mul_dense_mat_same_ordering (binop.rs:331-371): the coefficient-wise alpha * lhs * rhs in rhs' layout
inline DeviceMat mul_dense_mat_same_ordering(const DeviceCsMat &lhs, const DeviceMat &rhs, double alpha, void *stream = nullptr) {
    DeviceMat out(rhs.rows(), rhs.cols(), !rhs.is_standard_layout());
    csmat_binop_dense_raw(lhs, rhs, SPRS_HIP_BINOP_MUL, out, alpha, 1.0, stream);
    return out;
}
}  // namespace binop

// `&A + &D` (csmat.rs:1951-1987): A.to_other_storage() first when its storage does not match D's layout, below the C ABI
inline DeviceMat operator+(const DeviceCsMat &a, const DeviceMat &d) {
    DeviceMat out(d.rows(), d.cols(), !d.is_standard_layout());
    check(sprs_hip_csmat_add_dense_f64(a.handle(), d.ptr(), d.rows(), d.cols(), d.layout(), d.ld(), out.ptr(), nullptr));
    return out;
}

// TriMatI<f64, usize> (sparse/triplet.rs:26-48) with the device assembly of `to_csr` (triplet.rs:270-276 ->
// triplet_iter.rs:127-224: rows sorted, duplicates summed).  No dedicated kernel: with n triplets the matrix
// is the product R * E of R (rows x n, one 1 per column at the triplet's row) and E (n x cols, one value per
// row at the triplet's column); the SpGEMM adds over k = triplet index ascending.
class TriMat {
public:
    TriMat(uint64_t rows, uint64_t cols) : rows_(rows), cols_(cols) {}
    void add_triplet(uint64_t row, uint64_t col, double val) {
        if (row >= rows_ || col >= cols_) throw Error(SPRS_HIP_INVALID_ARG, "index out of bounds");
        r_.push_back(row);
        c_.push_back(col);
        v_.push_back(val);
    }
    uint64_t nnz() const { return v_.size(); }
    DeviceCsMat to_csr() const {
        const uint64_t n = v_.size();
        if (n == 0) return DeviceCsMat(SPRS_HIP_CSR, rows_, cols_, std::vector<uint64_t>(rows_ + 1, 0),
                                       std::vector<uint64_t>(), std::vector<double>(), false);
        std::vector<uint64_t> ptr(n + 1);
        for (uint64_t i = 0; i <= n; ++i) ptr[i] = i;
        DeviceCsMat sel_csc(SPRS_HIP_CSC, rows_, n, ptr, r_, std::vector<double>(n, 1.0));
        sprs_hip_csmat *sel = nullptr;
        check(sprs_hip_csmat_to_other_storage(sel_csc.handle(), &sel));
        DeviceCsMat sel_csr(sel);
        DeviceCsMat ent(SPRS_HIP_CSR, n, cols_, ptr, c_, v_);
        return smmp::mul_csr_csr(sel_csr, ent);
    }

private:
    uint64_t rows_, cols_;
    std::vector<uint64_t> r_, c_;
    std::vector<double> v_;
};

namespace linalg {
// linalg::bicgstab::BiCGSTAB (sprs/src/sparse/linalg/bicgstab.rs): `solve` returns the solver object in
// both the Ok and the Err case of the reference (Err = iteration limit, results still inside); here
// `converged()` tells them apart.
class BiCGSTAB {
public:
    static BiCGSTAB solve(const DeviceCsMat &a, const DeviceVec &x0, const DeviceVec &b, double tol, uint64_t max_iter,
                          double soft_restart_threshold = 0.1) {
        if (x0.dim() != b.dim()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
        BiCGSTAB s(x0.dim());
        check(sprs_hip_bicgstab_f64(const_cast<sprs_hip_csmat *>(a.handle()), x0.ptr(), b.ptr(), x0.dim(), tol, max_iter,
                                    soft_restart_threshold, s.x_.ptr(), &s.info_, nullptr));
        return s;
    }
    bool converged() const { return info_.converged != 0; }
    uint64_t iteration_count() const { return info_.iteration_count; }
    uint64_t soft_restart_count() const { return info_.soft_restart_count; }
    uint64_t hard_restart_count() const { return info_.hard_restart_count; }
    double err() const { return info_.err; }
    double rho() const { return info_.rho; }
    const DeviceVec &x() const { return x_; }

private:
    explicit BiCGSTAB(uint64_t n) : x_(n) {}
    DeviceVec x_;
    sprs_hip_bicgstab_info info_{};
};
// gauss_seidel(mat, x, rhs, max_iter, eps) of the reference's heat example (sprs/examples/heat.rs:103-139): x is the start
// vector and receives the result (the reference's `mut x`); Ok((iterations, error)) <-> converged, Err(error) otherwise.
struct GaussSeidelResult {
    bool converged;
    uint64_t iterations;
    double error;
    uint64_t levels;      // longest chain of rows that must be swept one after the other (device-side information)
};
inline GaussSeidelResult gauss_seidel(const DeviceCsMat &mat, DeviceVec &x, const DeviceVec &rhs, uint64_t max_iter, double eps) {
    if (x.dim() != rhs.dim()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    sprs_hip_gauss_seidel_info info{};
    check(sprs_hip_gauss_seidel_f64(const_cast<sprs_hip_csmat *>(mat.handle()), x.ptr(), rhs.ptr(), x.dim(), max_iter, eps, &info,
                                    nullptr));
    return GaussSeidelResult{info.converged != 0, info.iterations, info.error, info.levels};
}

// The four dense-rhs solves of sprs::linalg::trisolve (sprs/src/sparse/linalg/trisolve.rs), in place on rhs.  Where the
// reference panics (check_solver_dimensions, "Storage mismatch") Error is thrown with its text; where it returns
// Err(LinalgError::SingularMatrix) SingularMatrix is thrown, with the reference's index and message.
struct SingularMatrix : Error {
    uint64_t index;
    int32_t reason;       // 1 a numeric zero (also a CSR diagonal that is not stored), 2 a structural zero (CSC only)
    SingularMatrix(const std::string &m, uint64_t i, int32_t r) : Error(SPRS_HIP_SINGULAR_MATRIX, m), index(i), reason(r) {}
};
struct TriSolveResult {
    uint64_t levels;      // longest chain of unknowns that must be solved one after the other (device-side information)
};
namespace detail {
inline TriSolveResult trisolve(const DeviceCsMat &mat, DeviceVec &rhs, bool csr, int32_t uplo) {
    if (mat.rows() != mat.cols()) throw Error(SPRS_HIP_DIM_MISMATCH, "Non square matrix passed to solver");
    if (mat.cols() != rhs.dim()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (mat.is_csr() != csr) throw Error(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    sprs_hip_trisolve_info info{};
    const int32_t status = sprs_hip_trisolve_f64(const_cast<sprs_hip_csmat *>(mat.handle()), uplo, rhs.ptr(), rhs.dim(), &info, nullptr);
    if (status == SPRS_HIP_SINGULAR_MATRIX) throw SingularMatrix(sprs_hip_last_error(), info.singular_index, info.singular_reason);
    check(status);
    return TriSolveResult{info.levels};
}
}  // namespace detail
inline TriSolveResult lsolve_csr_dense_rhs(const DeviceCsMat &lower_tri_mat, DeviceVec &rhs) {   // trisolve.rs:30-73
    return detail::trisolve(lower_tri_mat, rhs, true, SPRS_HIP_LOWER);
}
inline TriSolveResult lsolve_csc_dense_rhs(const DeviceCsMat &lower_tri_mat, DeviceVec &rhs) {   // trisolve.rs:85-149
    return detail::trisolve(lower_tri_mat, rhs, false, SPRS_HIP_LOWER);
}
inline TriSolveResult usolve_csc_dense_rhs(const DeviceCsMat &upper_tri_mat, DeviceVec &rhs) {   // trisolve.rs:161-210
    return detail::trisolve(upper_tri_mat, rhs, false, SPRS_HIP_UPPER);
}
inline TriSolveResult usolve_csr_dense_rhs(const DeviceCsMat &upper_tri_mat, DeviceVec &rhs) {   // trisolve.rs:219-262
    return detail::trisolve(upper_tri_mat, rhs, true, SPRS_HIP_UPPER);
}
// lsolve_csc_sparse_rhs (trisolve.rs:286-358) with a device-resident sparse rhs.  The reference leaves an unsorted stack and
// a dense workspace; here the solution is a new DeviceCsVec over the reach of rhs in ascending order (numeric zeros kept).
// Products go into an unknown by ascending column (identical bits wherever the arithmetic is exact), fill-in starts from
// +0.0, the smallest singular index of the reach is thrown as SingularMatrix; `info` (optional) receives the device-side counts.
inline DeviceCsVec lsolve_csc_sparse_rhs(const DeviceCsMat &lower_tri_mat, const DeviceCsVec &rhs, sprs_hip_sptrisolve_info *info = nullptr) {
    if (lower_tri_mat.is_csr()) throw Error(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    sprs_hip_sptrisolve_info local{};
    sprs_hip_csvec *x = nullptr;
    const int32_t status = sprs_hip_lsolve_csc_sparse_rhs_f64(const_cast<sprs_hip_csmat *>(lower_tri_mat.handle()), rhs.handle(), &x, &local, nullptr);
    if (info) *info = local;
    if (status == SPRS_HIP_SINGULAR_MATRIX) throw SingularMatrix(sprs_hip_last_error(), local.singular_index, local.singular_reason);
    check(status);
    return DeviceCsVec(x);
}
}  // namespace linalg

// Result blocks released by ~DeviceCsMat stay in the library's pool for the next result (sprs_hip.h);
// this hands them back to the driver.  Returns the bytes released.
inline uint64_t pool_trim() {
    uint64_t freed = 0;
    check(sprs_hip_pool_trim(&freed));
    return freed;
}

// ---- single precision: CsMatI<f32, I, Iptr>, `&A * &x` and BiCGSTAB::<f32> ------------------------------------------------
// Distinct classes over a distinct handle type: an f64 entry cannot be handed f32 buffers, and the compiler rejects a product
// of mixed precision.  Every other operation is reached through to_f64() / to_f32(), on the device.
class DeviceVecF32 {
public:
    explicit DeviceVecF32(uint64_t n) : n_(n) {
        check(sprs_hip_malloc(&p_, n * 4));
        check(sprs_hip_memset(p_, 0, n * 4, nullptr));
    }
    explicit DeviceVecF32(const std::vector<float> &v) : n_(v.size()) {
        check(sprs_hip_malloc(&p_, n_ * 4));
        check(sprs_hip_memcpy_h2d(p_, v.data(), n_ * 4));
    }
    DeviceVecF32(DeviceVecF32 &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
    DeviceVecF32(const DeviceVecF32 &) = delete;
    DeviceVecF32 &operator=(const DeviceVecF32 &) = delete;
    ~DeviceVecF32() {
        if (p_) sprs_hip_free(p_);
    }
    uint64_t dim() const { return n_; }
    float *ptr() { return static_cast<float *>(p_); }
    const float *ptr() const { return static_cast<const float *>(p_); }
    std::vector<float> to_host() const {
        std::vector<float> out(n_);
        check(sprs_hip_synchronize(nullptr));
        check(sprs_hip_memcpy_d2h(out.data(), p_, n_ * 4));
        return out;
    }

private:
    void *p_ = nullptr;
    uint64_t n_ = 0;
};

class DeviceCsMatF32 {
public:
    // CsMat::new / new_csc (validate = true) or new_trusted (validate = false); I and Iptr of 4 or 8 bytes
    template <typename I, typename Iptr>
    DeviceCsMatF32(int32_t storage, uint64_t rows, uint64_t cols, const std::vector<Iptr> &indptr, const std::vector<I> &indices,
                   const std::vector<float> &data, bool validate = true) {
        static_assert(std::is_integral<I>::value && std::is_integral<Iptr>::value, "SpIndex types");
        static_assert(sizeof(I) == 4 || sizeof(I) == 8, "I must be 4 or 8 bytes");
        static_assert(sizeof(Iptr) == 4 || sizeof(Iptr) == 8, "Iptr must be 4 or 8 bytes");
        check(sprs_hip_csmat_f32_upload(&h_, storage, rows, cols, indptr.data(), (int32_t)sizeof(Iptr), indices.data(), (int32_t)sizeof(I),
                                        data.data(), validate ? 1 : 0));
    }
    explicit DeviceCsMatF32(sprs_hip_csmat_f32 *h) : h_(h) {}
    // CsMat::map(|&v| v as f32) (csmat.rs:1289-1305)
    explicit DeviceCsMatF32(const DeviceCsMat &m, void *stream = nullptr) { check(sprs_hip_csmat_f32_from_f64(m.handle(), &h_, stream)); }
    DeviceCsMatF32(DeviceCsMatF32 &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DeviceCsMatF32(const DeviceCsMatF32 &) = delete;
    DeviceCsMatF32 &operator=(const DeviceCsMatF32 &) = delete;
    ~DeviceCsMatF32() {
        if (h_) sprs_hip_csmat_f32_free(h_);
    }
    uint64_t rows() const { return info().rows; }
    uint64_t cols() const { return info().cols; }
    uint64_t nnz() const { return info().nnz; }
    bool is_csr() const { return info().storage == SPRS_HIP_CSR; }
    const sprs_hip_csmat_f32 *handle() const { return h_; }
    void prepare(void *stream = nullptr) { check(sprs_hip_csmat_f32_prepare(h_, stream)); }
    void refresh() { check(sprs_hip_csmat_f32_refresh(h_)); }
    // (kind, plan bytes): 0 none yet, 1 nnz tiles, 3 banded copy
    std::pair<int32_t, uint64_t> spmv_plan_info() const {
        int32_t kind = 0;
        uint64_t bytes = 0;
        check(sprs_hip_csmat_f32_spmv_plan_info(h_, &kind, &bytes));
        return {kind, bytes};
    }
    DeviceCsMatF32 transpose_view() const {          // shares this matrix's buffers: must not outlive it
        sprs_hip_csmat_f32 *t = nullptr;
        check(sprs_hip_csmat_f32_transpose_view(h_, &t));
        return DeviceCsMatF32(t);
    }
    DeviceCsMatF32 to_other_storage() const {        // csmat.rs:1405-1426
        sprs_hip_csmat_f32 *t = nullptr;
        check(sprs_hip_csmat_f32_to_other_storage(h_, &t));
        return DeviceCsMatF32(t);
    }
    DeviceCsMat to_f64(void *stream = nullptr) const {   // CsMat::map(|&v| v as f64): exact
        sprs_hip_csmat *t = nullptr;
        check(sprs_hip_csmat_f32_to_f64(h_, &t, stream));
        return DeviceCsMat(t);
    }
    // into_raw_storage for 8-byte handles
    void to_host(std::vector<uint64_t> &indptr, std::vector<uint64_t> &indices, std::vector<float> &data) const {
        const Info i = info();
        if (i.iptr_bytes != 8 || i.idx_bytes != 8) throw Error(SPRS_HIP_INVALID_ARG, "to_host: 64-bit handles only");
        indptr.resize((i.storage == SPRS_HIP_CSR ? i.rows : i.cols) + 1);
        indices.resize(i.nnz);
        data.resize(i.nnz);
        check(sprs_hip_csmat_f32_download(h_, indptr.data(), indices.data(), data.data()));
    }

private:
    struct Info {
        uint64_t rows, cols, nnz;
        int32_t iptr_bytes, idx_bytes, storage;
    };
    Info info() const {
        Info i{};
        check(sprs_hip_csmat_f32_info(h_, &i.rows, &i.cols, &i.nnz, &i.iptr_bytes, &i.idx_bytes, &i.storage));
        return i;
    }
    sprs_hip_csmat_f32 *h_ = nullptr;
};

namespace prod {
inline void mul_acc_mat_vec_csr(const DeviceCsMatF32 &mat, const DeviceVecF32 &in_vec, DeviceVecF32 &res_vec, void *stream = nullptr) {
    check(sprs_hip_spmv_f32(mat.handle(), in_vec.ptr(), in_vec.dim(), res_vec.ptr(), res_vec.dim(), 1, stream));
}
inline void mul_acc_mat_vec_csc(const DeviceCsMatF32 &mat, const DeviceVecF32 &in_vec, DeviceVecF32 &res_vec, void *stream = nullptr) {
    check(sprs_hip_mul_acc_mat_vec_csc_f32(mat.handle(), in_vec.ptr(), in_vec.dim(), res_vec.ptr(), res_vec.dim(), stream));
}
}  // namespace prod

inline DeviceVecF32 operator*(const DeviceCsMatF32 &a, const DeviceVecF32 &x) {      // CSR or CSC
    DeviceVecF32 y(a.rows());
    check(sprs_hip_csmat_mul_vec_f32(a.handle(), x.ptr(), x.dim(), y.ptr(), y.dim(), nullptr));
    return y;
}

// Dense f32 matrix in HBM: DeviceMat for N = f32, the operand and result type of the dense products of a DeviceCsMatF32.  A
// type of its own: no overload below takes operands of two precisions.
class DeviceMatF32 {
public:
    DeviceMatF32(uint64_t rows, uint64_t cols, bool col_major = false) : buf_(rows * cols), rows_(rows), cols_(cols), col_major_(col_major) {}
    // elements in memory order of the chosen layout
    DeviceMatF32(uint64_t rows, uint64_t cols, const std::vector<float> &elems, bool col_major = false)
        : buf_(elems), rows_(rows), cols_(cols), col_major_(col_major) {
        if (elems.size() != rows * cols) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    }
    uint64_t rows() const { return rows_; }
    uint64_t cols() const { return cols_; }
    bool is_standard_layout() const { return !col_major_; }
    int32_t layout() const { return col_major_ ? SPRS_HIP_COL_MAJOR : SPRS_HIP_ROW_MAJOR; }
    uint64_t ld() const { return col_major_ ? rows_ : cols_; }
    float *ptr() { return buf_.ptr(); }
    const float *ptr() const { return buf_.ptr(); }
    void set_layout(int32_t layout) { col_major_ = layout == SPRS_HIP_COL_MAJOR; }
    float at(const std::vector<float> &host, uint64_t i, uint64_t j) const { return col_major_ ? host[j * rows_ + i] : host[i * cols_ + j]; }
    std::vector<float> to_host() const { return buf_.to_host(); }       // memory order

private:
    DeviceVecF32 buf_;
    uint64_t rows_, cols_;
    bool col_major_;
};

namespace prod {
namespace detail {
inline void mulacc_dense(const DeviceCsMatF32 &lhs, bool want_csr, const DeviceMatF32 &rhs, DeviceMatF32 &out, void *stream) {
    if (rhs.cols() != out.cols()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");       // prod.rs:201, 230, 259, 287
    if (lhs.is_csr() != want_csr) {                                                                // prod.rs:202, 231, 258, 288 (after the dimensions)
        if (lhs.cols() != rhs.rows() || lhs.rows() != out.rows()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
        throw Error(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    }
    check(sprs_hip_csmat_mulacc_dense_f32(lhs.handle(), rhs.ptr(), rhs.rows(), rhs.cols(), rhs.layout(), rhs.ld(), out.ptr(),
                                          out.rows(), out.layout(), out.ld(), 1, stream));
}
}  // namespace detail
// prod::csr_mulacc_dense_rowmaj / _colmaj (prod.rs:189-214, 274-298), csc_mulacc_dense_rowmaj / _colmaj (prod.rs:219-270) for N = f32
inline void csr_mulacc_dense_rowmaj(const DeviceCsMatF32 &lhs, const DeviceMatF32 &rhs, DeviceMatF32 &out, void *stream = nullptr) { detail::mulacc_dense(lhs, true, rhs, out, stream); }
inline void csr_mulacc_dense_colmaj(const DeviceCsMatF32 &lhs, const DeviceMatF32 &rhs, DeviceMatF32 &out, void *stream = nullptr) { detail::mulacc_dense(lhs, true, rhs, out, stream); }
inline void csc_mulacc_dense_rowmaj(const DeviceCsMatF32 &lhs, const DeviceMatF32 &rhs, DeviceMatF32 &out, void *stream = nullptr) { detail::mulacc_dense(lhs, false, rhs, out, stream); }
inline void csc_mulacc_dense_colmaj(const DeviceCsMatF32 &lhs, const DeviceMatF32 &rhs, DeviceMatF32 &out, void *stream = nullptr) { detail::mulacc_dense(lhs, false, rhs, out, stream); }
}  // namespace prod

// `&A * &M` for N = f32 (csmat.rs:1989-2048): standard layout from 8 columns on, `.f()` layout below
inline DeviceMatF32 operator*(const DeviceCsMatF32 &a, const DeviceMatF32 &m) {
    DeviceMatF32 out(a.rows(), m.cols());
    int32_t lay = SPRS_HIP_ROW_MAJOR;
    check(sprs_hip_csmat_mul_dense_f32(a.handle(), m.ptr(), m.rows(), m.cols(), m.layout(), m.ld(), out.ptr(), &lay, nullptr));
    out.set_layout(lay);
    return out;
}

// `Array2::dot(&CsMat)` for N = f32 (csmat.rs:2050-2117): dense . sparse
inline DeviceMatF32 dot(const DeviceMatF32 &lhs, const DeviceCsMatF32 &rhs) {
    DeviceMatF32 out(lhs.rows(), rhs.cols());
    int32_t lay = SPRS_HIP_ROW_MAJOR;
    check(sprs_hip_dense_dot_csmat_f32(lhs.ptr(), lhs.rows(), lhs.cols(), lhs.layout(), lhs.ld(), rhs.handle(), out.ptr(), &lay, nullptr));
    out.set_layout(lay);
    return out;
}

// `&A * &B` for N = f32 (csmat.rs:1866-1949) in any pair of storages; the result has the storage of the lhs.  Every product and
// every partial sum is rounded to f32, in the reference's order.  No overload takes one f64 and one f32 matrix.
inline DeviceCsMatF32 operator*(const DeviceCsMatF32 &a, const DeviceCsMatF32 &b) {
    sprs_hip_csmat_f32 *c = nullptr;
    check(sprs_hip_csmat_mul_csmat_f32(a.handle(), b.handle(), &c));
    return DeviceCsMatF32(c);
}

namespace smmp {
// smmp::mul_csr_csr / symbolic / numeric (smmp.rs:196-416, 81-131, 151-189) for N = f32
inline DeviceCsMatF32 mul_csr_csr(const DeviceCsMatF32 &lhs, const DeviceCsMatF32 &rhs) {
    sprs_hip_csmat_f32 *c = nullptr;
    check(sprs_hip_spgemm_f32(lhs.handle(), rhs.handle(), &c));
    return DeviceCsMatF32(c);
}
inline DeviceCsMatF32 symbolic(const DeviceCsMatF32 &lhs, const DeviceCsMatF32 &rhs) {
    sprs_hip_csmat_f32 *c = nullptr;
    check(sprs_hip_spgemm_symbolic_f32(lhs.handle(), rhs.handle(), &c));
    return DeviceCsMatF32(c);
}
inline void numeric(const DeviceCsMatF32 &lhs, const DeviceCsMatF32 &rhs, DeviceCsMatF32 &c) {
    check(sprs_hip_spgemm_numeric_f32(lhs.handle(), rhs.handle(), const_cast<sprs_hip_csmat_f32 *>(c.handle())));
}

// The symbolic phase of a product, kept (sprs_hip_spgemm_plan_*): structure() / product() / numeric() launch the value kernels
// only.  The plan holds structure alone, so ONE plan serves f64 and f32 operands over the same indptr / indices device arrays:
// every method is overloaded on the operand type.  The operands must keep their structure while the plan lives.
class SpgemmPlan {
public:
    SpgemmPlan(const DeviceCsMat &a, const DeviceCsMat &b) { check(sprs_hip_spgemm_plan_create(a.handle(), b.handle(), &p_)); }
    SpgemmPlan(const DeviceCsMatF32 &a, const DeviceCsMatF32 &b) { check(sprs_hip_spgemm_plan_create_f32(a.handle(), b.handle(), &p_)); }
    SpgemmPlan(SpgemmPlan &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    SpgemmPlan(const SpgemmPlan &) = delete;
    SpgemmPlan &operator=(const SpgemmPlan &) = delete;
    ~SpgemmPlan() {
        if (p_) sprs_hip_spgemm_plan_free(p_);
    }
    uint64_t nnz() const {
        uint64_t n = 0;
        check(sprs_hip_spgemm_plan_nnz(p_, &n));
        return n;
    }
    DeviceCsMat structure(const DeviceCsMat &a, const DeviceCsMat &b) {
        sprs_hip_csmat *c = nullptr;
        check(sprs_hip_spgemm_plan_structure(p_, a.handle(), b.handle(), &c));
        return DeviceCsMat(c);
    }
    DeviceCsMatF32 structure(const DeviceCsMatF32 &a, const DeviceCsMatF32 &b) {
        sprs_hip_csmat_f32 *c = nullptr;
        check(sprs_hip_spgemm_plan_structure_f32(p_, a.handle(), b.handle(), &c));
        return DeviceCsMatF32(c);
    }
    DeviceCsMat product(const DeviceCsMat &a, const DeviceCsMat &b) {
        sprs_hip_csmat *c = nullptr;
        check(sprs_hip_spgemm_plan_product(p_, a.handle(), b.handle(), &c));
        return DeviceCsMat(c);
    }
    DeviceCsMatF32 product(const DeviceCsMatF32 &a, const DeviceCsMatF32 &b) {
        sprs_hip_csmat_f32 *c = nullptr;
        check(sprs_hip_spgemm_plan_product_f32(p_, a.handle(), b.handle(), &c));
        return DeviceCsMatF32(c);
    }
    void numeric(const DeviceCsMat &a, const DeviceCsMat &b, DeviceCsMat &c) {
        check(sprs_hip_spgemm_plan_numeric(p_, a.handle(), b.handle(), const_cast<sprs_hip_csmat *>(c.handle())));
    }
    void numeric(const DeviceCsMatF32 &a, const DeviceCsMatF32 &b, DeviceCsMatF32 &c) {
        check(sprs_hip_spgemm_plan_numeric_f32(p_, a.handle(), b.handle(), const_cast<sprs_hip_csmat_f32 *>(c.handle())));
    }

private:
    sprs_hip_spgemm_plan *p_ = nullptr;
};
}  // namespace smmp

namespace linalg {
// BiCGSTAB::<f32>::solve (bicgstab.rs:148-171, :305)
class BiCGSTABF32 {
public:
    static BiCGSTABF32 solve(const DeviceCsMatF32 &a, const DeviceVecF32 &x0, const DeviceVecF32 &b, float tol, uint64_t max_iter,
                             float soft_restart_threshold = 0.1f) {
        if (x0.dim() != b.dim()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
        BiCGSTABF32 s(x0.dim());
        check(sprs_hip_bicgstab_f32(const_cast<sprs_hip_csmat_f32 *>(a.handle()), x0.ptr(), b.ptr(), x0.dim(), (double)tol, max_iter,
                                    (double)soft_restart_threshold, s.x_.ptr(), &s.info_, nullptr));
        return s;
    }
    bool converged() const { return info_.converged != 0; }
    uint64_t iteration_count() const { return info_.iteration_count; }
    uint64_t soft_restart_count() const { return info_.soft_restart_count; }
    uint64_t hard_restart_count() const { return info_.hard_restart_count; }
    float err() const { return (float)info_.err; }
    float rho() const { return (float)info_.rho; }
    const DeviceVecF32 &x() const { return x_; }

private:
    explicit BiCGSTABF32(uint64_t n) : x_(n) {}
    DeviceVecF32 x_;
    sprs_hip_bicgstab_info info_{};
};

// gauss_seidel::<f32> of the heat example, the four dense-rhs triangular solves and diag_solve for N = f32: overloads of the f64
// functions above on DeviceCsMatF32 / DeviceVecF32 (sprs_hip_gauss_seidel_f32, sprs_hip_trisolve_f32, sprs_hip_diag_solve_f32).
// Iterates and solutions are the reference's f32 bits; GaussSeidelResult::error holds the f32 scalar widened.
inline GaussSeidelResult gauss_seidel(const DeviceCsMatF32 &mat, DeviceVecF32 &x, const DeviceVecF32 &rhs, uint64_t max_iter, float eps) {
    if (x.dim() != rhs.dim()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    sprs_hip_gauss_seidel_info info{};
    check(sprs_hip_gauss_seidel_f32(const_cast<sprs_hip_csmat_f32 *>(mat.handle()), x.ptr(), rhs.ptr(), x.dim(), max_iter, (double)eps,
                                    &info, nullptr));
    return GaussSeidelResult{info.converged != 0, info.iterations, info.error, info.levels};
}
namespace detail {
inline TriSolveResult trisolve(const DeviceCsMatF32 &mat, DeviceVecF32 &rhs, bool csr, int32_t uplo) {
    if (mat.rows() != mat.cols()) throw Error(SPRS_HIP_DIM_MISMATCH, "Non square matrix passed to solver");
    if (mat.cols() != rhs.dim()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    if (mat.is_csr() != csr) throw Error(SPRS_HIP_STORAGE_MISMATCH, "Storage mismatch");
    sprs_hip_trisolve_info info{};
    const int32_t status = sprs_hip_trisolve_f32(const_cast<sprs_hip_csmat_f32 *>(mat.handle()), uplo, rhs.ptr(), rhs.dim(), &info, nullptr);
    if (status == SPRS_HIP_SINGULAR_MATRIX) throw SingularMatrix(sprs_hip_last_error(), info.singular_index, info.singular_reason);
    check(status);
    return TriSolveResult{info.levels};
}
}  // namespace detail
inline TriSolveResult lsolve_csr_dense_rhs(const DeviceCsMatF32 &lower_tri_mat, DeviceVecF32 &rhs) {
    return detail::trisolve(lower_tri_mat, rhs, true, SPRS_HIP_LOWER);
}
inline TriSolveResult lsolve_csc_dense_rhs(const DeviceCsMatF32 &lower_tri_mat, DeviceVecF32 &rhs) {
    return detail::trisolve(lower_tri_mat, rhs, false, SPRS_HIP_LOWER);
}
inline TriSolveResult usolve_csc_dense_rhs(const DeviceCsMatF32 &upper_tri_mat, DeviceVecF32 &rhs) {
    return detail::trisolve(upper_tri_mat, rhs, false, SPRS_HIP_UPPER);
}
inline TriSolveResult usolve_csr_dense_rhs(const DeviceCsMatF32 &upper_tri_mat, DeviceVecF32 &rhs) {
    return detail::trisolve(upper_tri_mat, rhs, true, SPRS_HIP_UPPER);
}
inline void diag_solve(const DeviceVecF32 &d, DeviceVecF32 &x, void *stream = nullptr) {
    if (d.dim() != x.dim()) throw Error(SPRS_HIP_DIM_MISMATCH, "Dimension mismatch");
    check(sprs_hip_diag_solve_f32(d.ptr(), x.ptr(), x.dim(), stream));
}
}  // namespace linalg

}  // namespace sprs_hip
