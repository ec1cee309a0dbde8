// The handles of libsprs_hip.so and the memory behind them: the pool of result blocks, the one constructor per kind of handle
// (owned, view, device copy) and what `delete` does to a matrix.  No other file says `new sprs_hip_...`.
// The f64 and the f32 matrix handle share their fields (CsmatCore, common.hpp), so each kind of matrix constructor is one
// template on the handle type H; make_csmat / view_csmat are overloads that forward to it.
// Host code only.  Included by abi.hip (one translation unit of the library and of the emulator build, tests/emu).
#pragma once
#include <map>

#include "common.hpp"

namespace sprs_hip {

// ---- pool of released result blocks ------------------------------------------------------------
// A product like config 5's is 2 x 26.5 GB.  The driver hands such blocks out in ~30 ms the first
// time, but takes SECONDS when the same amount has just been released (measured 2.0-3.4 s for the
// second A*A of a process, against 0.23 s of kernels: profiles/r01z_spgemm_v3_sweep.txt) — a loop
// that forms a product per iteration would spend 90 % of its time there.  Owned blocks of >= 1 MiB
// therefore go back to a per-device pool and the next result takes the best fit (<= 25 % slack).
// hipFree synchronises the device before a block can be reused; so does pool_free.
namespace {
struct Pool {
    std::mutex mu;
    std::multimap<std::pair<int, uint64_t>, void *> blocks;   // (device, bytes) -> block
    uint64_t cached = 0;
};
Pool &pool() {
    static Pool p;
    return p;
}
constexpr uint64_t POOL_MIN = 1ull << 20;      // from here on: best fit with <= 25 % slack
constexpr uint64_t POOL_SMALL = 256;            // below POOL_MIN: size classes, powers of two from this one
}  // namespace

uint64_t pool_trim() {
    Pool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    const uint64_t freed = p.cached;
    for (auto &kv : p.blocks) (void)hipFree(kv.second);
    p.blocks.clear();
    p.cached = 0;
    return freed;
}

uint64_t pool_cached_bytes() {
    Pool &p = pool();
    std::lock_guard<std::mutex> g(p.mu);
    return p.cached;
}

hipError_t pool_alloc(void **out, uint64_t bytes, uint64_t *cap, int device) {
    if (bytes == 0) bytes = 8;       // hipMalloc(0) returns nullptr; kernels never see NULL
    // small blocks (task lists of a few entries, block sums of a scan, key arrays) are pooled in power-of-two classes from 256 B:
    // a product made ~15 of them, each a hipMalloc and a hipFree (which waits for the device) of its own
    if (bytes < POOL_MIN) {
        uint64_t cls = POOL_SMALL;
        while (cls < bytes) cls <<= 1;
        bytes = cls;
    }
    if (options().pool) {
        Pool &p = pool();
        std::lock_guard<std::mutex> g(p.mu);
        auto it = p.blocks.lower_bound({device, bytes});
        if (it != p.blocks.end() && it->first.first == device && it->first.second <= bytes + bytes / 4) {
            *out = it->second;
            *cap = it->first.second;
            p.cached -= it->first.second;
            p.blocks.erase(it);
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipErrorOutOfMemory && pool_trim()) {
        (void)hipGetLastError();
        e = hipMalloc(out, bytes);
    }
    *cap = bytes;
    return e;
}

void pool_free(void *ptr, uint64_t cap, int device, bool stream_ordered) {
    if (!ptr) return;
    int current = -1;
    // a block of ANOTHER device than the calling thread's current one goes straight back to the driver:
    // the synchronisation below would wait on the wrong device
    if (options().pool && cap >= POOL_SMALL && hipGetDevice(&current) == hipSuccess && current == device) {
        Pool &p = pool();
        // the block may still be read by kernels in flight: same guarantee as hipFree — unless the caller vouches that all of
        // them, and every later use of a pooled block, are ordered by the null stream (the SpGEMM plan's temporaries: a product
        // dropped ~25 blocks, each behind its own device synchronisation)
        if (stream_ordered || hipDeviceSynchronize() == hipSuccess) {
            std::lock_guard<std::mutex> g(p.mu);
            if (p.cached + cap <= (uint64_t)options().pool_max_bytes) {
                p.blocks.insert({{device, cap}, ptr});
                p.cached += cap;
                return;
            }
        }
    }
    (void)hipFree(ptr);
}

// ---- owned handles ---------------------------------------------------------------------------------
// blocks for arrays of the given sizes on the current device; on failure the blocks taken so far go with their owners
static int32_t take_blocks(int *device, std::initializer_list<std::pair<PoolBlock *, uint64_t>> want, const char *what) {
    hipError_t e = hipGetDevice(device);
    for (const auto &w : want)
        if (e == hipSuccess) e = w.first->alloc(w.second, *device);
    return e == hipSuccess ? (int32_t)SPRS_HIP_OK : fail_hip(e, what);
}

template <typename H>
static void set_shape(H *m, int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, int32_t iptr_bytes, int32_t idx_bytes) {
    m->storage = storage;
    m->rows = rows;
    m->cols = cols;
    m->nnz = nnz;
    m->iptr_bytes = iptr_bytes;
    m->idx_bytes = idx_bytes;
}

template <typename H>
static int32_t make_matrix(Owned<H> &out, int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, int32_t iptr_bytes, int32_t idx_bytes,
                           const char *what) {
    using T = typename H::value_type;
    Owned<H> m(new H());
    set_shape(m.get(), storage, rows, cols, nnz, iptr_bytes, idx_bytes);
    SPRS_TRY(take_blocks(&m->device, {{&m->own_indptr, (m->outer() + 1) * (uint64_t)iptr_bytes}, {&m->own_indices, nnz * (uint64_t)idx_bytes},
                                      {&m->own_data, nnz * sizeof(T)}}, what));
    m->indptr = m->own_indptr.p;
    m->indices = m->own_indices.p;
    m->data = (T *)m->own_data.p;
    out = std::move(m);
    return SPRS_HIP_OK;
}
int32_t make_csmat(OwnedCsmat &out, int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, int32_t iptr_bytes, int32_t idx_bytes) {
    return make_matrix(out, storage, rows, cols, nnz, iptr_bytes, idx_bytes, "alloc_csmat");
}
int32_t make_csmat(OwnedCsmatF32 &out, int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, int32_t iptr_bytes, int32_t idx_bytes) {
    return make_matrix(out, storage, rows, cols, nnz, iptr_bytes, idx_bytes, "alloc_csmat_f32");
}

int32_t make_csvec(OwnedCsvec &out, uint64_t dim, uint64_t nnz, int32_t idx_bytes, int32_t decl_idx_bytes) {
    OwnedCsvec v(new sprs_hip_csvec());
    v->dim = dim;
    v->nnz = nnz;
    v->idx_bytes = idx_bytes;
    v->decl_idx_bytes = decl_idx_bytes == idx_bytes ? 0 : decl_idx_bytes;
    SPRS_TRY(take_blocks(&v->device, {{&v->own_indices, nnz * (uint64_t)idx_bytes}, {&v->own_data, nnz * sizeof(double)}}, "csvec_alloc"));
    v->indices = v->own_indices.p;
    v->data = (double *)v->own_data.p;
    out = std::move(v);
    return SPRS_HIP_OK;
}

int32_t make_perm(OwnedPerm &out, uint64_t dim, int32_t idx_bytes, int32_t decl_idx_bytes) {
    OwnedPerm p(new sprs_hip_perm());
    p->dim = dim;
    p->idx_bytes = idx_bytes;
    p->decl_idx_bytes = decl_idx_bytes == idx_bytes ? 0 : decl_idx_bytes;
    SPRS_TRY(take_blocks(&p->device, {{&p->own_perm, dim * (uint64_t)idx_bytes}, {&p->own_inv, dim * (uint64_t)idx_bytes}}, "perm_alloc"));
    p->perm = p->own_perm.p;
    p->perm_inv = p->own_inv.p;
    out = std::move(p);
    return SPRS_HIP_OK;
}

// the structure of `from` (an owned f64 matrix: a conversion result) moves into a new f32 handle; its values get a fresh block
int32_t adopt_structure_f32(sprs_hip_csmat *from, OwnedCsmatF32 &out) {
    OwnedCsmatF32 m(new sprs_hip_csmat_f32());
    set_shape(m.get(), from->storage, from->rows, from->cols, from->nnz, from->iptr_bytes, from->idx_bytes);
    SPRS_TRY(take_blocks(&m->device, {{&m->own_data, from->nnz * sizeof(float)}}, "alloc_csmat_f32"));
    m->own_indptr = std::move(from->own_indptr);
    m->own_indices = std::move(from->own_indices);
    from->indptr = from->indices = nullptr;
    m->indptr = m->own_indptr.p;
    m->indices = m->own_indices.p;
    m->data = (float *)m->own_data.p;
    out = std::move(m);
    return SPRS_HIP_OK;
}

// ---- views: the array pointers set, the owners empty ----------------------------------------------------
template <typename H>
static H *view_arrays(int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, const void *indptr, int32_t iptr_bytes, const void *indices,
                      int32_t idx_bytes, const typename H::value_type *data, int device, H *into) {
    H *t = into ? into : new H();
    set_shape(t, storage, rows, cols, nnz, iptr_bytes, idx_bytes);
    t->indptr = const_cast<void *>(indptr);
    t->indices = const_cast<void *>(indices);
    t->data = const_cast<typename H::value_type *>(data);
    t->device = device;
    return t;
}

template <typename H>
static H *view_handle(const H *m, bool transpose, H *into) {
    const int32_t other = m->storage == SPRS_HIP_CSR ? SPRS_HIP_CSC : SPRS_HIP_CSR;
    H *t = view_arrays(transpose ? other : m->storage, transpose ? m->cols : m->rows, transpose ? m->rows : m->cols, m->nnz, m->indptr, m->iptr_bytes,
                       m->indices, m->idx_bytes, m->data, m->device, into);
    t->decl_iptr_bytes = m->decl_iptr_bytes;
    t->decl_idx_bytes = m->decl_idx_bytes;
    return t;
}

sprs_hip_csmat *view_csmat(int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, const void *indptr, int32_t iptr_bytes,
                           const void *indices, int32_t idx_bytes, const double *data, int device, sprs_hip_csmat *into) {
    return view_arrays(storage, rows, cols, nnz, indptr, iptr_bytes, indices, idx_bytes, data, device, into);
}
sprs_hip_csmat_f32 *view_csmat(int32_t storage, uint64_t rows, uint64_t cols, uint64_t nnz, const void *indptr, int32_t iptr_bytes,
                               const void *indices, int32_t idx_bytes, const float *data, int device, sprs_hip_csmat_f32 *into) {
    return view_arrays(storage, rows, cols, nnz, indptr, iptr_bytes, indices, idx_bytes, data, device, into);
}
sprs_hip_csmat *view_csmat(const sprs_hip_csmat *m, bool transpose, sprs_hip_csmat *into) { return view_handle(m, transpose, into); }
sprs_hip_csmat_f32 *view_csmat(const sprs_hip_csmat_f32 *m, bool transpose, sprs_hip_csmat_f32 *into) { return view_handle(m, transpose, into); }

sprs_hip_csvec *view_csvec(uint64_t dim, uint64_t nnz, const void *indices, int32_t idx_bytes, const double *data, int device) {
    auto *v = new sprs_hip_csvec();
    v->dim = dim;
    v->nnz = nnz;
    v->idx_bytes = idx_bytes;
    v->indices = const_cast<void *>(indices);
    v->data = const_cast<double *>(data);
    v->device = device;
    return v;
}

sprs_hip_perm *identity_perm(uint64_t dim, int32_t idx_bytes) {
    auto *p = new sprs_hip_perm();
    p->dim = dim;
    p->idx_bytes = idx_bytes == 2 ? 4 : idx_bytes;
    p->decl_idx_bytes = idx_bytes == 2 ? 2 : 0;
    p->identity = true;
    return p;
}

sprs_hip_ordering *make_ordering() { return new sprs_hip_ordering(); }

sprs_hip_ldl_sym *make_ldl_symbolic() {
    auto *h = new sprs_hip_ldl_sym();
    h->s = std::make_shared<LdlSym>();
    return h;
}

sprs_hip_ldl_num *make_ldl_numeric(const sprs_hip_ldl_sym *sym) {
    auto *h = new sprs_hip_ldl_num();
    h->s = sym->s;
    return h;
}

// ---- device copy ------------------------------------------------------------------------------------
int32_t copy_csmat(const sprs_hip_csmat *m, bool with_data, OwnedCsmat &out, hipStream_t stream) {
    OwnedCsmat res;
    SPRS_TRY(make_csmat(res, m->storage, m->rows, m->cols, m->nnz, m->iptr_bytes, m->idx_bytes));
    SPRS_TRY_HIP(hipMemcpyAsync(res->indptr, m->indptr, (m->outer() + 1) * (uint64_t)m->iptr_bytes, hipMemcpyDeviceToDevice, stream));
    if (m->nnz) SPRS_TRY_HIP(hipMemcpyAsync(res->indices, m->indices, m->nnz * (uint64_t)m->idx_bytes, hipMemcpyDeviceToDevice, stream));
    if (m->nnz && with_data) SPRS_TRY_HIP(hipMemcpyAsync(res->data, m->data, m->nnz * sizeof(double), hipMemcpyDeviceToDevice, stream));
    out = std::move(res);
    return SPRS_HIP_OK;
}

// ---- release ----------------------------------------------------------------------------------------
// Everything a handle derives from its arrays: the SpMV / SpMM plans (they copy values), the Gauss-Seidel / triangular-solve row orders, the copy in the other
// storage order and the transpose view kept for dense . sparse products.  Called whenever the values (or the arrays) change:
// refresh, delete and BOTH numeric SpGEMM entries, which rewrite C's values in place (a stale CSC copy of C
// would otherwise serve later products).
template <typename H>
static void drop_shared_caches(H *m) {
    m->mm = SpmmPlan();
    delete m->t_view;
    m->t_view = nullptr;
    delete m->as_other;
    m->as_other = nullptr;
}

void invalidate_caches(sprs_hip_csmat *m) {
    m->plan = SpmvPlan();
    m->gs = GsPlan();
    m->tri_upper = GsPlan();
    m->cv = CsvecScratch();
    m->sp = SpTriScratch();
    drop_shared_caches(m);
}

void invalidate_caches(sprs_hip_csmat_f32 *m) {
    m->plan = SpmvPlanF32();
    m->gs = GsPlan();
    m->tri_upper = GsPlan();
    drop_shared_caches(m);
}

}  // namespace sprs_hip

sprs_hip_csmat_f32::~sprs_hip_csmat_f32() {
    // as for the f64 handle: a kernel in flight (on the banded plan's second stream too) may still read the plan, a carry array or the CSR copy
    if (t_view || as_other || plan.built || mm.built) (void)hipDeviceSynchronize();
    sprs_hip::invalidate_caches(this);
}

sprs_hip_csmat::~sprs_hip_csmat() {
    // a kernel launched through a cached copy (as_other, t_view) or a plan copy may still be reading it: a handle that holds
    // any of them waits for the device before they go (refresh does the same; a bare handle frees at once)
    if (t_view || as_other || plan.built || cv.bits || sp.bits) (void)hipDeviceSynchronize();
    sprs_hip::invalidate_caches(this);
}
