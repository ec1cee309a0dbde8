//! Safe wrapper over `sprs-hip-sys` (NOT COMPILED in this repository's build
//! environment: no rustc there).  Shape of the code follows
//! sprs_suitesparse_umfpack/src/lib.rs:30-46 (opaque handle + Drop) and
//! sprs_suitesparse_ldl/src/lib.rs:86-127 (cast index types, pass raw pointers).
//!
//! `DenseVector` / `DenseVectorMut` are sealed in sprs (dense_vector.rs:305-326),
//! so device buffers cannot be passed to `sprs::prod::*` itself; this crate
//! offers twins with the same names, argument order and panics.
use sprs::{CsMatI, CsMatViewI, CsVecI, CsVecViewI, SpIndex};
use sprs_hip_sys as sys;
use std::ffi::CStr;
use std::os::raw::c_void;

fn check(status: i32) {
    if status == sys::SPRS_HIP_OK {
        return;
    }
    let msg = unsafe { CStr::from_ptr(sys::sprs_hip_last_error()) }.to_string_lossy().into_owned();
    // Contract violations panic with the reference's own text
    // (prod.rs:114-118, smmp.rs:207, csmat.rs:1794-1797; Guidelines.rst:10-27).
    panic!("{msg}");
}

/// A dense f64 vector in HBM.
pub struct DeviceVec {
    ptr: *mut f64,
    len: usize,
}

impl DeviceVec {
    pub fn zeros(len: usize) -> Self {
        let mut p: *mut c_void = std::ptr::null_mut();
        unsafe {
            check(sys::sprs_hip_malloc(&mut p, (len * 8) as u64));
            check(sys::sprs_hip_memset(p, 0, (len * 8) as u64, std::ptr::null_mut()));
        }
        Self { ptr: p as *mut f64, len }
    }
    pub fn from_slice(x: &[f64]) -> Self {
        let v = Self::zeros(x.len());
        unsafe { check(sys::sprs_hip_memcpy_h2d(v.ptr as *mut c_void, x.as_ptr() as *const c_void, (x.len() * 8) as u64)) };
        v
    }
    pub fn to_vec(&self) -> Vec<f64> {
        let mut out = vec![0.0; self.len];
        unsafe {
            check(sys::sprs_hip_synchronize(std::ptr::null_mut()));
            check(sys::sprs_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, self.ptr as *const c_void, (self.len * 8) as u64));
        }
        out
    }
    pub fn dim(&self) -> usize {
        self.len
    }
}

impl Drop for DeviceVec {
    fn drop(&mut self) {
        unsafe { sys::sprs_hip_free(self.ptr as *mut c_void) };
    }
}

/// Device twin of `CsMatI<f64, I, Iptr>`.
pub struct DeviceCsMat {
    h: *mut sys::sprs_hip_csmat,
}

// A handle may be shared read-only across host threads (products take &self);
// the C side guards its lazily built SpMV plan with a mutex.
unsafe impl Send for DeviceCsMat {}
unsafe impl Sync for DeviceCsMat {}

impl DeviceCsMat {
    /// Upload a host matrix (any `SpIndex` types of 4 or 8 bytes).
    pub fn from_view<I: SpIndex, Iptr: SpIndex>(m: CsMatViewI<f64, I, Iptr>) -> Self {
        let indptr = m.indptr(); // may be non-proper (slice_outer): the C side rebases
        let mut h = std::ptr::null_mut();
        unsafe {
            check(sys::sprs_hip_csmat_upload(
                &mut h,
                if m.is_csr() { sys::SPRS_HIP_CSR } else { sys::SPRS_HIP_CSC },
                m.rows() as u64,
                m.cols() as u64,
                indptr.raw_storage().as_ptr() as *const c_void,
                std::mem::size_of::<Iptr>() as i32,
                m.indices().as_ptr() as *const c_void,
                std::mem::size_of::<I>() as i32,
                m.data().as_ptr(),
                0, // the CsMat invariants were already checked on the host
            ));
        }
        Self { h }
    }

    /// Build the full SpMV plan now instead of at the handle's second multiply (`sprs_hip_csmat_prepare`): for callers that
    /// iterate (a solver); a handle that multiplies once never pays for the re-laid-out copy.
    pub fn prepare(&mut self) {
        unsafe { check(sys::sprs_hip_csmat_prepare(self.h, std::ptr::null_mut())) };
    }

    pub fn shape(&self) -> (usize, usize) {
        let (mut r, mut c) = (0u64, 0u64);
        unsafe { check(sys::sprs_hip_csmat_info(self.h, &mut r, &mut c, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())) };
        (r as usize, c as usize)
    }

    pub fn nnz(&self) -> usize {
        let mut n = 0u64;
        unsafe { check(sys::sprs_hip_csmat_info(self.h, std::ptr::null_mut(), std::ptr::null_mut(), &mut n, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())) };
        n as usize
    }

    /// (rows, cols, nnz, indptr bytes, index bytes, storage) as the handle reports them.
    fn info(&self) -> (usize, usize, usize, i32, i32, i32) {
        let (mut r, mut c, mut n) = (0u64, 0u64, 0u64);
        let (mut pb, mut ib, mut st) = (0i32, 0i32, 0i32);
        unsafe { check(sys::sprs_hip_csmat_info(self.h, &mut r, &mut c, &mut n, &mut pb, &mut ib, &mut st)) };
        (r as usize, c as usize, n as usize, pb, ib, st)
    }

    /// Download as a host `CsMatI<f64, usize, usize>`.  The handle may be CSR or CSC and may hold 2-, 4- or 8-byte
    /// indices: the buffers are sized by the OUTER dimension and by the widths the handle reports, widened to usize,
    /// and the real storage order goes into the constructor.
    pub fn to_csmat(&self) -> Result<CsMatI<f64, usize, usize>, String> {
        let (rows, cols, nnz, pb, ib, st) = self.info();
        let storage = if st == sys::SPRS_HIP_CSR { sprs::CompressedStorage::CSR } else { sprs::CompressedStorage::CSC };
        let outer = if st == sys::SPRS_HIP_CSR { rows } else { cols };
        if ![2, 4, 8].contains(&pb) || ![2, 4, 8].contains(&ib) {
            return Err(format!("unsupported index widths {}/{}", pb, ib));
        }
        // raw byte buffers of exactly the size sprs_hip_csmat_download writes
        let mut ip_raw = vec![0u8; (outer + 1) * pb as usize];
        let mut ix_raw = vec![0u8; nnz * ib as usize];
        let mut data = vec![0f64; nnz];
        unsafe {
            check(sys::sprs_hip_csmat_download(self.h, ip_raw.as_mut_ptr() as *mut c_void, ix_raw.as_mut_ptr() as *mut c_void, data.as_mut_ptr()));
        }
        fn widen(raw: &[u8], bytes: i32) -> Vec<usize> {
            match bytes {
                2 => raw.chunks_exact(2).map(|c| u16::from_ne_bytes([c[0], c[1]]) as usize).collect(),
                4 => raw.chunks_exact(4).map(|c| u32::from_ne_bytes([c[0], c[1], c[2], c[3]]) as usize).collect(),
                _ => raw.chunks_exact(8).map(|c| u64::from_ne_bytes([c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]]) as usize).collect(),
            }
        }
        let indptr = widen(&ip_raw, pb);
        let indices = widen(&ix_raw, ib);
        // the checked constructor: a few passes over the host copy, and no undefined behaviour if the device side ever
        // handed back something malformed
        // (sprs has one checked constructor per storage — `try_new` / `try_new_csc`, csmat.rs:235-256; both hand the vectors
        // back beside the StructureError, its fourth tuple element)
        let built = match storage {
            sprs::CompressedStorage::CSR => CsMatI::try_new((rows, cols), indptr, indices, data),
            sprs::CompressedStorage::CSC => CsMatI::try_new_csc((rows, cols), indptr, indices, data),
        };
        built.map_err(|(_, _, _, e)| format!("{:?}", e))
    }
}

impl Drop for DeviceCsMat {
    fn drop(&mut self) {
        unsafe { sys::sprs_hip_csmat_free(self.h) };
    }
}

/// A dense f64 matrix in HBM with ndarray's two contiguous layouts: `Array2` in standard (row-major) order or `.f()` order.
pub struct DeviceMat {
    buf: DeviceVec,
    rows: usize,
    cols: usize,
    col_major: bool,
}

impl DeviceMat {
    pub fn zeros(shape: (usize, usize)) -> Self {
        DeviceMat { buf: DeviceVec::zeros(shape.0 * shape.1), rows: shape.0, cols: shape.1, col_major: false }
    }
    /// `Array::zeros(shape.f())`
    pub fn zeros_f(shape: (usize, usize)) -> Self {
        DeviceMat { buf: DeviceVec::zeros(shape.0 * shape.1), rows: shape.0, cols: shape.1, col_major: true }
    }
    /// from an ndarray in standard layout (`as_slice()` order)
    pub fn from_rows(shape: (usize, usize), row_major: &[f64]) -> Self {
        assert_eq!(shape.0 * shape.1, row_major.len(), "Dimension mismatch");
        DeviceMat { buf: DeviceVec::from_slice(row_major), rows: shape.0, cols: shape.1, col_major: false }
    }
    pub fn shape(&self) -> (usize, usize) { (self.rows, self.cols) }
    pub fn is_standard_layout(&self) -> bool { !self.col_major }
    /// the elements in memory order (row-major, or column-major when `!is_standard_layout()`)
    pub fn to_vec(&self) -> Vec<f64> { self.buf.to_vec() }
    fn layout(&self) -> i32 { if self.col_major { sys::SPRS_HIP_COL_MAJOR } else { sys::SPRS_HIP_ROW_MAJOR } }
    fn ld(&self) -> u64 { (if self.col_major { self.rows } else { self.cols }) as u64 }
}

pub mod prod {
    use super::*;
    /// Twin of `sprs::prod::csvec_dot_by_binary_search` (prod.rs:14-70): on the device the same function as `CsVec::dot`.
    pub fn csvec_dot_by_binary_search(vec1: &DeviceCsVec, vec2: &DeviceCsVec) -> f64 {
        vec1.dot(vec2)
    }
    /// Twin of `sprs::prod::mul_acc_mat_vec_csr` (prod.rs:103-127): `res_vec += mat * in_vec`.
    pub fn mul_acc_mat_vec_csr(mat: &DeviceCsMat, in_vec: &DeviceVec, res_vec: &mut DeviceVec) {
        unsafe {
            check(sys::sprs_hip_spmv_f64(mat.h, in_vec.ptr, in_vec.len as u64, res_vec.ptr, res_vec.len as u64, 1, std::ptr::null_mut()));
        }
    }
    /// Twin of `sprs::prod::mul_acc_mat_vec_csc` (prod.rs:74-99): `res_vec += mat * in_vec` for a CSC matrix.
    pub fn mul_acc_mat_vec_csc(mat: &DeviceCsMat, in_vec: &DeviceVec, res_vec: &mut DeviceVec) {
        unsafe {
            check(sys::sprs_hip_mul_acc_mat_vec_csc_f64(mat.h, in_vec.ptr, in_vec.len as u64, res_vec.ptr, res_vec.len as u64, std::ptr::null_mut()));
        }
    }
    fn mulacc_dense(lhs: &DeviceCsMat, rhs: &DeviceMat, out: &mut DeviceMat) {
        assert_eq!(rhs.cols, out.cols, "Dimension mismatch");                       // prod.rs:201
        unsafe {
            check(sys::sprs_hip_csmat_mulacc_dense_f64(lhs.h, rhs.buf.ptr, rhs.rows as u64, rhs.cols as u64, rhs.layout(), rhs.ld(),
                                                       out.buf.ptr, out.rows as u64, out.layout(), out.ld(), 1, std::ptr::null_mut()));
        }
    }
    /// Twins of `csr_mulacc_dense_rowmaj` / `_colmaj` (prod.rs:189-214, 274-298) and `csc_mulacc_dense_rowmaj` / `_colmaj`
    /// (prod.rs:219-270): `out += lhs * rhs`.  The four differ in their loop order in the reference; on the device one entry
    /// serves them, told by the operands' own layouts how to address them; the storage asserts are the reference's.
    pub fn csr_mulacc_dense_rowmaj(lhs: &DeviceCsMat, rhs: &DeviceMat, out: &mut DeviceMat) {
        assert!(lhs.is_csr(), "Storage mismatch");
        mulacc_dense(lhs, rhs, out)
    }
    pub fn csr_mulacc_dense_colmaj(lhs: &DeviceCsMat, rhs: &DeviceMat, out: &mut DeviceMat) {
        assert!(lhs.is_csr(), "Storage mismatch");
        mulacc_dense(lhs, rhs, out)
    }
    pub fn csc_mulacc_dense_rowmaj(lhs: &DeviceCsMat, rhs: &DeviceMat, out: &mut DeviceMat) {
        assert!(lhs.is_csc(), "Storage mismatch");
        mulacc_dense(lhs, rhs, out)
    }
    pub fn csc_mulacc_dense_colmaj(lhs: &DeviceCsMat, rhs: &DeviceMat, out: &mut DeviceMat) {
        assert!(lhs.is_csc(), "Storage mismatch");
        mulacc_dense(lhs, rhs, out)
    }
}

/// Twin of `TriMatBase::to_csr` / `to_csc` (triplet_iter.rs:127-224) for triplets already in HBM: sorted by (row, col),
/// duplicates summed in triplet order.
pub fn triplets_to_cs(shape: (usize, usize), rows: &DeviceIdx, cols: &DeviceIdx, data: &DeviceVec, csc: bool) -> DeviceCsMat {
    assert!(rows.len == cols.len && rows.len == data.len, "Dimension mismatch");
    let mut h = std::ptr::null_mut();
    unsafe {
        check(sys::sprs_hip_triplets_to_cs(shape.0 as u64, shape.1 as u64, data.len as u64, rows.ptr, cols.ptr, 8, data.ptr,
                                           if csc { sys::SPRS_HIP_CSC } else { sys::SPRS_HIP_CSR }, 8, 8, &mut h));
    }
    DeviceCsMat { h }
}

/// usize indices in HBM (the row / column arrays of a `TriMat`).
pub struct DeviceIdx {
    ptr: *mut c_void,
    len: usize,
}

impl DeviceIdx {
    pub fn from_slice(x: &[usize]) -> Self {
        let mut p: *mut c_void = std::ptr::null_mut();
        unsafe {
            check(sys::sprs_hip_malloc(&mut p, (x.len() * 8) as u64));
            check(sys::sprs_hip_memcpy_h2d(p, x.as_ptr() as *const c_void, (x.len() * 8) as u64));
        }
        DeviceIdx { ptr: p, len: x.len() }
    }
}

impl Drop for DeviceIdx {
    fn drop(&mut self) {
        unsafe { sys::sprs_hip_free(self.ptr) };
    }
}

/// Row-sharded SpMV over the GPUs of one node (no counterpart in the reference; the shard of a rank is
/// `a.slice_outer(r0..r1)`, slicing.rs:65-89): one process per GPU, `unique_id()` on one rank handed to all.
pub mod dist {
    use super::*;
    pub struct DistSpMV {
        d: *mut sys::sprs_hip_dist,
    }
    pub fn unique_id() -> [u8; 128] {
        let mut id = [0u8; 128];
        unsafe { check(sys::sprs_hip_dist_unique_id(id.as_mut_ptr() as *mut c_void)) };
        id
    }
    impl DistSpMV {
        /// collective: `local_block` = this rank's rows (all columns), `row_starts` = world + 1 global row offsets
        pub fn new(id: &[u8; 128], world: usize, rank: usize, shape: (usize, usize), row_starts: &[u64], local_block: &DeviceCsMat,
                   nsub: usize) -> Self {
            assert_eq!(row_starts.len(), world + 1, "Dimension mismatch");
            let mut d = std::ptr::null_mut();
            unsafe {
                check(sys::sprs_hip_dist_create(&mut d, id.as_ptr() as *const c_void, world as i32, rank as i32, shape.0 as u64,
                                                shape.1 as u64, row_starts.as_ptr(), local_block.h, nsub as i32));
            }
            DistSpMV { d }
        }
        /// collective: `y = A * x`, x replicated (length cols), y gathered on every rank (length rows)
        pub fn mul(&self, x: &DeviceVec, y: &mut DeviceVec) {
            unsafe { check(sys::sprs_hip_dist_spmv_f64(self.d, x.ptr, x.len as u64, y.ptr, y.len as u64, std::ptr::null_mut())) };
        }
        /// ranks of the RCCL communicator (ncclCommCount)
        pub fn comm_count(&self) -> usize {
            let mut n = 0i32;
            unsafe { check(sys::sprs_hip_dist_comm_count(self.d, &mut n)) };
            n as usize
        }
        /// the peer-store route: this rank's receive window as a 64-byte HIP IPC handle
        pub fn peer_handle(&mut self) -> [u8; 64] {
            let mut h = [0u8; 64];
            unsafe { check(sys::sprs_hip_dist_peer_handle(self.d, h.as_mut_ptr() as *mut c_void)) };
            h
        }
        /// collective: every rank's handle, in rank order
        pub fn peer_connect(&mut self, all_handles: &[[u8; 64]]) {
            unsafe { check(sys::sprs_hip_dist_peer_connect(self.d, all_handles.as_ptr() as *const c_void, all_handles.len() as i32)) };
        }
        /// 0: grouped ncclSend / ncclRecv, 1: stores into the peers' windows
        pub fn set_route(&mut self, route: i32) {
            unsafe { check(sys::sprs_hip_dist_set_route(self.d, route)) };
        }
        pub fn route(&self) -> i32 {
            let mut r = 0i32;
            unsafe { check(sys::sprs_hip_dist_route(self.d, &mut r)) };
            r
        }
    }
    impl Drop for DistSpMV {
        fn drop(&mut self) {
            unsafe { sys::sprs_hip_dist_free(self.d) };
        }
    }
}

pub mod smmp {
    use super::*;
    /// Twin of `sprs::smmp::mul_csr_csr` (smmp.rs:196-416).
    pub fn mul_csr_csr(lhs: &DeviceCsMat, rhs: &DeviceCsMat) -> DeviceCsMat {
        let mut h = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_spgemm_f64(lhs.h, rhs.h, &mut h)) };
        DeviceCsMat { h }
    }

    /// Twin of `sprs::smmp::symbolic` (smmp.rs:81-131): the structure of `lhs * rhs`, values 0.0.
    pub fn symbolic(lhs: &DeviceCsMat, rhs: &DeviceCsMat) -> DeviceCsMat {
        let mut h = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_spgemm_symbolic(lhs.h, rhs.h, &mut h)) };
        DeviceCsMat { h }
    }

    /// Twin of `sprs::smmp::numeric` (smmp.rs:151-189): the values of `lhs * rhs` into `c`, which must
    /// have the product's structure (panics with the library's message otherwise).
    pub fn numeric(lhs: &DeviceCsMat, rhs: &DeviceCsMat, c: &mut DeviceCsMat) {
        unsafe { check(sys::sprs_hip_spgemm_numeric(lhs.h, rhs.h, c.h)) };
    }
}

pub mod linalg {
    use super::*;
    /// Twin of `sprs::linalg::bicgstab::BiCGSTAB` (sparse/linalg/bicgstab.rs) with device-resident dense
    /// vectors.  `solve` returns `Ok(solver)` / `Err(solver)` like the reference (Err = iteration limit).
    pub struct BiCGSTAB {
        x: DeviceVec,
        info: sys::sprs_hip_bicgstab_info,
    }
    impl BiCGSTAB {
        pub fn solve(a: &DeviceCsMat, x0: &DeviceVec, b: &DeviceVec, tol: f64, max_iter: usize)
            -> Result<Box<BiCGSTAB>, Box<BiCGSTAB>> {
            assert_eq!(x0.len, b.len, "Dimension mismatch");
            let x = DeviceVec::zeros(x0.len);
            let mut info = sys::sprs_hip_bicgstab_info::default();
            unsafe {
                check(sys::sprs_hip_bicgstab_f64(a.h, x0.ptr, b.ptr, x0.len as u64, tol, max_iter as u64, 0.1, x.ptr,
                                                 &mut info, std::ptr::null_mut()));
            }
            let s = Box::new(BiCGSTAB { x, info });
            if s.info.converged != 0 { Ok(s) } else { Err(s) }
        }
        pub fn iteration_count(&self) -> usize { self.info.iteration_count as usize }
        pub fn soft_restart_count(&self) -> usize { self.info.soft_restart_count as usize }
        pub fn hard_restart_count(&self) -> usize { self.info.hard_restart_count as usize }
        pub fn err(&self) -> f64 { self.info.err }
        pub fn rho(&self) -> f64 { self.info.rho }
        pub fn x(&self) -> &DeviceVec { &self.x }
    }

    /// Twin of `gauss_seidel(mat, x, rhs, max_iter, eps)` of the reference's heat example (examples/heat.rs:103-139):
    /// `x` is the start vector and receives the result; `Ok((iterations, error))` / `Err(error)` like the reference.
    pub fn gauss_seidel(mat: &DeviceCsMat, x: &mut DeviceVec, rhs: &DeviceVec, max_iter: usize, eps: f64)
        -> Result<(usize, f64), f64> {
        assert_eq!(x.len, rhs.len, "Dimension mismatch");
        let mut info = sys::sprs_hip_gauss_seidel_info::default();
        unsafe {
            check(sys::sprs_hip_gauss_seidel_f64(mat.h, x.ptr, rhs.ptr, x.len as u64, max_iter as u64, eps, &mut info,
                                                 std::ptr::null_mut()));
        }
        if info.converged != 0 { Ok((info.iterations as usize, info.error)) } else { Err(info.error) }
    }

    /// The four dense-rhs solves of `sprs::linalg::trisolve` (sparse/linalg/trisolve.rs) with a device-resident `rhs`,
    /// solved in place: the same panics ("Non square matrix passed to solver", "Dimension mismatch", "Storage mismatch"),
    /// the same `Err(LinalgError::SingularMatrix)` with the reference's index and reason, bit-identical solutions.
    fn trisolve(mat: &DeviceCsMat, rhs: &mut DeviceVec, csr: bool, uplo: i32, csr_reason: &'static str)
        -> Result<(), sprs::errors::LinalgError> {
        let (rows, cols, _, _, _, st) = mat.info();
        // check_solver_dimensions (trisolve.rs:10-21) comes before the storage assert in all four functions
        assert_eq!(cols, rows, "Non square matrix passed to solver");
        assert_eq!(cols, rhs.len, "Dimension mismatch");
        assert!((st == sys::SPRS_HIP_CSR) == csr, "Storage mismatch");
        let mut info = sys::sprs_hip_trisolve_info::default();
        let status = unsafe { sys::sprs_hip_trisolve_f64(mat.h, uplo, rhs.ptr, rhs.len as u64, &mut info, std::ptr::null_mut()) };
        if status == sys::SPRS_HIP_SINGULAR_MATRIX {
            let reason = match (csr, info.singular_reason) {
                (true, _) => csr_reason,
                (false, 2) => "diagonal element is a structural 0",
                (false, _) => "diagonal element is a numeric 0",
            };
            return Err(sprs::errors::LinalgError::SingularMatrix(sprs::errors::SingularMatrixInfo {
                index: info.singular_index as usize,
                reason,
            }));
        }
        check(status);
        Ok(())
    }

    /// Twin of `lsolve_csr_dense_rhs` (trisolve.rs:30-73); the upper triangle of `lower_tri_mat` is ignored.
    pub fn lsolve_csr_dense_rhs(lower_tri_mat: &DeviceCsMat, rhs: &mut DeviceVec) -> Result<(), sprs::errors::LinalgError> {
        trisolve(lower_tri_mat, rhs, true, sys::SPRS_HIP_LOWER, "diagonal element is 0")
    }

    /// Twin of `lsolve_csc_dense_rhs` (trisolve.rs:85-149).
    pub fn lsolve_csc_dense_rhs(lower_tri_mat: &DeviceCsMat, rhs: &mut DeviceVec) -> Result<(), sprs::errors::LinalgError> {
        trisolve(lower_tri_mat, rhs, false, sys::SPRS_HIP_LOWER, "")
    }

    /// Twin of `usolve_csc_dense_rhs` (trisolve.rs:161-210).
    pub fn usolve_csc_dense_rhs(upper_tri_mat: &DeviceCsMat, rhs: &mut DeviceVec) -> Result<(), sprs::errors::LinalgError> {
        trisolve(upper_tri_mat, rhs, false, sys::SPRS_HIP_UPPER, "")
    }

    /// Twin of `usolve_csr_dense_rhs` (trisolve.rs:219-262); the lower triangle of `upper_tri_mat` is ignored.
    pub fn usolve_csr_dense_rhs(upper_tri_mat: &DeviceCsMat, rhs: &mut DeviceVec) -> Result<(), sprs::errors::LinalgError> {
        trisolve(upper_tri_mat, rhs, true, sys::SPRS_HIP_UPPER, "diagonal element is a numeric 0")
    }

    /// Twin of `lsolve_csc_sparse_rhs` (trisolve.rs:286-358) with a device-resident sparse `rhs`.  The reference leaves the
    /// pattern as an unsorted stack beside a dense workspace; here the solution comes back as a new `DeviceCsVec` whose
    /// pattern is the reach of `rhs` in ascending order (numeric zeros kept).  Unknown r receives its products by ascending
    /// column (identical bits wherever the arithmetic is exact), a fill-in unknown starts from +0.0, and of several
    /// singular columns in the reach the smallest index is reported; a singular column outside the reach is not an error.
    pub fn lsolve_csc_sparse_rhs(lower_tri_mat: &DeviceCsMat, rhs: &DeviceCsVec) -> Result<DeviceCsVec, sprs::errors::LinalgError> {
        let (rows, cols, _, _, _, st) = lower_tri_mat.info();
        assert!(st == sys::SPRS_HIP_CSC, "Storage mismatch");                      // trisolve.rs:301
        assert_eq!(cols, rows, "Non square matrix passed to solver");
        assert_eq!(rows, rhs.dim(), "Dimension mismatch");
        let mut info = sys::sprs_hip_sptrisolve_info::default();
        let mut h: *mut sys::sprs_hip_csvec = std::ptr::null_mut();
        let status = unsafe { sys::sprs_hip_lsolve_csc_sparse_rhs_f64(lower_tri_mat.h, rhs.h, &mut h, &mut info, std::ptr::null_mut()) };
        if status == sys::SPRS_HIP_SINGULAR_MATRIX {
            return Err(sprs::errors::LinalgError::SingularMatrix(sprs::errors::SingularMatrixInfo {
                index: info.singular_index as usize,
                reason: if info.singular_reason == 2 { "diagonal element is a structural 0" } else { "diagonal element is a numeric 0" },
            }));
        }
        check(status);
        Ok(DeviceCsVec { h })
    }
}

/// Result blocks released by `Drop for DeviceCsMat` stay pooled inside the library; this returns them to
/// the driver (bytes released).
pub fn pool_trim() -> u64 {
    let mut freed = 0u64;
    unsafe { check(sys::sprs_hip_pool_trim(&mut freed)) };
    freed
}

/// `&A * &x`  (csmat.rs:2119-2160): fresh result, no accumulation, CSR or CSC (the dispatch lives below the C ABI).
impl<'a, 'b> std::ops::Mul<&'b DeviceVec> for &'a DeviceCsMat {
    type Output = DeviceVec;
    fn mul(self, rhs: &'b DeviceVec) -> DeviceVec {
        let out = DeviceVec::zeros(self.shape().0);
        unsafe {
            check(sys::sprs_hip_csmat_mul_vec_f64(self.h, rhs.ptr, rhs.len as u64, out.ptr, out.len as u64, std::ptr::null_mut()));
        }
        out
    }
}

/// `&A * &M`  (csmat.rs:1989-2048): the four arms (CSR | CSC) x (>= 8 columns | fewer) below the C ABI; the result is in
/// standard layout for >= 8 columns and in `.f()` layout below, like the reference's.
impl<'a, 'b> std::ops::Mul<&'b DeviceMat> for &'a DeviceCsMat {
    type Output = DeviceMat;
    fn mul(self, rhs: &'b DeviceMat) -> DeviceMat {
        let mut out = DeviceMat::zeros((self.shape().0, rhs.cols));
        let mut lay = 0i32;
        unsafe {
            check(sys::sprs_hip_csmat_mul_dense_f64(self.h, rhs.buf.ptr, rhs.rows as u64, rhs.cols as u64, rhs.layout(), rhs.ld(),
                                                    out.buf.ptr, &mut lay, std::ptr::null_mut()));
        }
        out.col_major = lay == sys::SPRS_HIP_COL_MAJOR;
        out
    }
}

impl DeviceMat {
    /// `Array2::dot(&CsMat)` (csmat.rs:2050-2117): dense . sparse
    pub fn dot(&self, rhs: &DeviceCsMat) -> DeviceMat {
        let mut out = DeviceMat::zeros((self.rows, rhs.shape().1));
        let mut lay = 0i32;
        unsafe {
            check(sys::sprs_hip_dense_dot_csmat_f64(self.buf.ptr, self.rows as u64, self.cols as u64, self.layout(), self.ld(), rhs.h,
                                                    out.buf.ptr, &mut lay, std::ptr::null_mut()));
        }
        out.col_major = lay == sys::SPRS_HIP_COL_MAJOR;
        out
    }
}

/// `&A * &B`  (csmat.rs:1866-1888 -> csmat_mul_csmat -> smmp::mul_csr_csr).
impl<'a, 'b> std::ops::Mul<&'b DeviceCsMat> for &'a DeviceCsMat {
    type Output = DeviceCsMat;
    fn mul(self, rhs: &'b DeviceCsMat) -> DeviceCsMat {
        // the storage dispatch of csmat_mul_csmat (csmat.rs:1895-1949) lives below the C ABI
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_mul_csmat(self.h, rhs.h, &mut h)) };
        DeviceCsMat { h }
    }
}

/// Device twin of `CsVecI<f64, I>` (sprs/src/sparse.rs:165-173).
pub struct DeviceCsVec {
    h: *mut sys::sprs_hip_csvec,
}

unsafe impl Send for DeviceCsVec {}
unsafe impl Sync for DeviceCsVec {}

impl DeviceCsVec {
    /// Upload a host sparse vector (any `SpIndex` type of 2, 4 or 8 bytes; its invariants were checked by CsVec::new).
    pub fn from_view<I: SpIndex>(v: CsVecViewI<f64, I>) -> Self {
        let mut h = std::ptr::null_mut();
        unsafe {
            check(sys::sprs_hip_csvec_upload(
                &mut h,
                v.dim() as u64,
                v.nnz() as u64,
                v.indices().as_ptr() as *const c_void,
                std::mem::size_of::<I>() as i32,
                v.data().as_ptr(),
                0,
            ));
        }
        Self { h }
    }

    pub fn dim(&self) -> usize {
        let mut d = 0u64;
        unsafe { check(sys::sprs_hip_csvec_info(self.h, &mut d, std::ptr::null_mut(), std::ptr::null_mut())) };
        d as usize
    }

    pub fn nnz(&self) -> usize {
        let mut n = 0u64;
        unsafe { check(sys::sprs_hip_csvec_info(self.h, std::ptr::null_mut(), &mut n, std::ptr::null_mut())) };
        n as usize
    }

    /// Download into a host `CsVecI<f64, I>` (I of the width the vector was made with).
    pub fn to_host<I: SpIndex>(&self) -> CsVecI<f64, I> {
        let (mut d, mut n, mut ib) = (0u64, 0u64, 0i32);
        unsafe { check(sys::sprs_hip_csvec_info(self.h, &mut d, &mut n, &mut ib)) };
        assert_eq!(ib as usize, std::mem::size_of::<I>(), "index width of the device vector");
        let mut indices = vec![I::zero(); n as usize];
        let mut data = vec![0.0f64; n as usize];
        unsafe { check(sys::sprs_hip_csvec_download(self.h, indices.as_mut_ptr() as *mut c_void, data.as_mut_ptr())) };
        CsVecI::new(d as usize, indices, data)
    }
}

impl Drop for DeviceCsVec {
    fn drop(&mut self) {
        unsafe { sys::sprs_hip_csvec_free(self.h) };
    }
}

/// Reductions (vec.rs:787-958, 1051-1061; prod.rs:14-70).  Every sum is the reference's left-to-right chain from +0.0, bit for
/// bit; the one documented difference is the sign of a zero result of `dot_dense` and of the norms (include/sprs_hip.h).
impl DeviceCsVec {
    /// `CsVec::dot` with a sparse rhs (vec.rs:828-881); panics with "Dimension mismatch" like the reference's assert.
    pub fn dot(&self, rhs: &DeviceCsVec) -> f64 {
        let mut out = 0.0f64;
        unsafe { check(sys::sprs_hip_csvec_dot_f64(self.h, rhs.h, &mut out, std::ptr::null_mut())) };
        out
    }

    /// `CsVec::dot_dense` (vec.rs:894-904).
    pub fn dot_dense(&self, rhs: &DeviceVec) -> f64 {
        let mut out = 0.0f64;
        unsafe { check(sys::sprs_hip_csvec_dot_dense_f64(self.h, rhs.ptr, rhs.len as u64, &mut out, std::ptr::null_mut())) };
        out
    }

    fn norm_kind(&self, kind: i32, p: f64) -> f64 {
        let mut out = 0.0f64;
        unsafe { check(sys::sprs_hip_csvec_norm_f64(self.h, kind, p, &mut out, std::ptr::null_mut())) };
        out
    }

    /// vec.rs:907-913.
    pub fn squared_l2_norm(&self) -> f64 {
        self.norm_kind(sys::SPRS_HIP_NORM_SQUARED_L2, 0.0)
    }

    /// vec.rs:916-922: the square root is taken on the host.
    pub fn l2_norm(&self) -> f64 {
        self.norm_kind(sys::SPRS_HIP_NORM_L2, 0.0)
    }

    /// vec.rs:925-930.
    pub fn l1_norm(&self) -> f64 {
        self.norm_kind(sys::SPRS_HIP_NORM_L1, 0.0)
    }

    /// vec.rs:939-958, with its branches for p = +-inf and p = 0.
    pub fn norm(&self, p: f64) -> f64 {
        self.norm_kind(sys::SPRS_HIP_NORM_P, p)
    }

    /// `unit_normalize` (vec.rs:1051-1061) as a NEW vector: handles are immutable snapshots; a zero vector comes back as a copy.
    pub fn unit_normalize(&self) -> DeviceCsVec {
        let mut h: *mut sys::sprs_hip_csvec = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csvec_unit_normalize_f64(self.h, &mut h, std::ptr::null_mut())) };
        DeviceCsVec { h }
    }

    /// `nnz_index` / `get` (vec.rs:787-805), batched: per index the position in the stored arrays and the value, `None` where
    /// nothing is stored.
    pub fn get_many(&self, indices: &[usize]) -> Vec<Option<(usize, f64)>> {
        let q: Vec<u64> = indices.iter().map(|&i| i as u64).collect();
        let (pos, val) = lookup(q.len(), &[&q], |ptrs, pos, val| unsafe {
            sys::sprs_hip_csvec_nnz_index(self.h, q.len() as u64, ptrs[0], pos, val, std::ptr::null_mut())
        });
        pos.iter().zip(val).map(|(&p, v)| if p == u64::MAX { None } else { Some((p as usize, v)) }).collect()
    }

    /// vec.rs:800-805.
    pub fn nnz_index(&self, index: usize) -> Option<usize> {
        self.get_many(&[index])[0].map(|(p, _)| p)
    }

    /// vec.rs:787-792.
    pub fn get(&self, index: usize) -> Option<f64> {
        self.get_many(&[index])[0].map(|(_, v)| v)
    }
}

/// uploads the query arrays, runs `call(queries, pos, val)` and downloads the positions and values
fn lookup<F: FnOnce(&[*const u64], *mut u64, *mut f64) -> i32>(nq: usize, queries: &[&Vec<u64>], call: F) -> (Vec<u64>, Vec<f64>) {
    let bytes = (nq.max(1) * 8) as u64;
    let mut bufs: Vec<*mut c_void> = Vec::new();
    for _ in 0..queries.len() + 2 {
        let mut p: *mut c_void = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_malloc(&mut p, bytes)) };
        bufs.push(p);
    }
    for (k, q) in queries.iter().enumerate() {
        unsafe { check(sys::sprs_hip_memcpy_h2d(bufs[k], q.as_ptr() as *const c_void, (nq * 8) as u64)) };
    }
    let ptrs: Vec<*const u64> = bufs[..queries.len()].iter().map(|&p| p as *const u64).collect();
    let (pb, vb) = (bufs[queries.len()], bufs[queries.len() + 1]);
    let status = call(&ptrs, pb as *mut u64, vb as *mut f64);
    let (mut pos, mut val) = (vec![0u64; nq], vec![0.0f64; nq]);
    if status == sys::SPRS_HIP_OK {
        unsafe {
            check(sys::sprs_hip_synchronize(std::ptr::null_mut()));
            check(sys::sprs_hip_memcpy_d2h(pos.as_mut_ptr() as *mut c_void, pb, (nq * 8) as u64));
            check(sys::sprs_hip_memcpy_d2h(val.as_mut_ptr() as *mut c_void, vb, (nq * 8) as u64));
        }
    }
    for p in bufs {
        unsafe { sys::sprs_hip_free(p) };
    }
    check(status);
    (pos, val)
}

/// A `DeviceCsVec` that borrows the arrays of a matrix (`DeviceCsMat::outer_view`): it cannot outlive the matrix.
pub struct DeviceCsVecView<'a> {
    v: DeviceCsVec,
    _m: std::marker::PhantomData<&'a DeviceCsMat>,
}

impl<'a> std::ops::Deref for DeviceCsVecView<'a> {
    type Target = DeviceCsVec;
    fn deref(&self) -> &DeviceCsVec {
        &self.v
    }
}

/// Extraction (csmat.rs:1017-1056, 1219-1256, 1312-1351).
impl DeviceCsMat {
    /// `outer_view` (csmat.rs:1219-1231): zero-copy; `None` when `i >= outer_dims()`.
    pub fn outer_view(&self, i: usize) -> Option<DeviceCsVecView<'_>> {
        let mut h: *mut sys::sprs_hip_csvec = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_outer_view(self.h, i as u64, &mut h, std::ptr::null_mut())) };
        if h.is_null() {
            None
        } else {
            Some(DeviceCsVecView { v: DeviceCsVec { h }, _m: std::marker::PhantomData })
        }
    }

    /// `diag` (csmat.rs:1234-1256): structural, an explicit 0.0 on the diagonal is kept.
    pub fn diag(&self) -> DeviceCsVec {
        let mut h: *mut sys::sprs_hip_csvec = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_diag_f64(self.h, &mut h, std::ptr::null_mut())) };
        DeviceCsVec { h }
    }

    /// `nnz_index` / `get` (csmat.rs:1312-1351), batched over (row, col) pairs: the global position and the value, `None`
    /// where nothing is stored (out-of-range rows and cols included).
    pub fn get_many(&self, rows: &[usize], cols: &[usize]) -> Vec<Option<(usize, f64)>> {
        assert_eq!(rows.len(), cols.len());
        let r: Vec<u64> = rows.iter().map(|&i| i as u64).collect();
        let c: Vec<u64> = cols.iter().map(|&i| i as u64).collect();
        let (pos, val) = lookup(r.len(), &[&r, &c], |ptrs, pos, val| unsafe {
            sys::sprs_hip_csmat_nnz_index(self.h, r.len() as u64, ptrs[0], ptrs[1], pos, val, std::ptr::null_mut())
        });
        pos.iter().zip(val).map(|(&p, v)| if p == u64::MAX { None } else { Some((p as usize, v)) }).collect()
    }

    /// csmat.rs:1312-1330.
    pub fn nnz_index(&self, row: usize, col: usize) -> Option<usize> {
        self.get_many(&[row], &[col])[0].map(|(p, _)| p)
    }

    /// csmat.rs `get`.
    pub fn get(&self, row: usize, col: usize) -> Option<f64> {
        self.get_many(&[row], &[col])[0].map(|(_, v)| v)
    }

    /// `to_inner_onehot` (csmat.rs:1017-1056): the LAST of equal maxima, NaNs skipped.
    pub fn to_inner_onehot(&self) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_to_inner_onehot_f64(self.h, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }
}

/// `&A * &v` (vec.rs:1104-1131): prod::csr_mul_csvec for CSR, `A * v.col_view()` for CSC — dispatched below the C ABI.
impl<'a, 'b> std::ops::Mul<&'b DeviceCsVec> for &'a DeviceCsMat {
    type Output = DeviceCsVec;
    fn mul(self, rhs: &'b DeviceCsVec) -> DeviceCsVec {
        let mut h: *mut sys::sprs_hip_csvec = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_mul_csvec_f64(self.h, rhs.h, &mut h, std::ptr::null_mut())) };
        DeviceCsVec { h }
    }
}

/// `&v * &B` (vec.rs:1084-1102): `(v.row_view() * B).outer_view(0)`.
impl<'a, 'b> std::ops::Mul<&'b DeviceCsMat> for &'a DeviceCsVec {
    type Output = DeviceCsVec;
    fn mul(self, rhs: &'b DeviceCsMat) -> DeviceCsVec {
        let mut h: *mut sys::sprs_hip_csvec = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csvec_mul_csmat_f64(self.h, rhs.h, &mut h, std::ptr::null_mut())) };
        DeviceCsVec { h }
    }
}

/// Twin of `sprs::binop` (sprs/src/sparse/binop.rs) for device operands: one IEEE operation per result entry.
pub mod binop {
    use super::{check, sys, DeviceCsMat, DeviceCsVec};

    /// The operation of `csmat_binop` / `csvec_binop` (the reference takes a closure; the device offers the three it uses).
    #[derive(Clone, Copy, Debug, PartialEq, Eq)]
    pub enum Op {
        Add = sys::SPRS_HIP_BINOP_ADD as isize,
        Sub = sys::SPRS_HIP_BINOP_SUB as isize,
        Mul = sys::SPRS_HIP_BINOP_MUL as isize,
    }

    /// `binop::csmat_binop` (binop.rs:178-223): equal shapes ("Dimension mismatch") and storages ("Storage mismatch");
    /// an entry is kept iff `!val.is_zero()`.
    pub fn csmat_binop(lhs: &DeviceCsMat, rhs: &DeviceCsMat, op: Op) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_binop_f64(lhs.h, rhs.h, op as i32, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }

    /// `binop::mul_mat_same_storage` (binop.rs:115-130).
    pub fn mul_mat_same_storage(lhs: &DeviceCsMat, rhs: &DeviceCsMat) -> DeviceCsMat {
        csmat_binop(lhs, rhs, Op::Mul)
    }

    /// `binop::csvec_binop` (binop.rs:442-467): every merged index is kept; a dimension of 0 takes the other operand's.
    pub fn csvec_binop(lhs: &DeviceCsVec, rhs: &DeviceCsVec, op: Op) -> DeviceCsVec {
        let mut h: *mut sys::sprs_hip_csvec = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csvec_binop_f64(lhs.h, rhs.h, op as i32, &mut h, std::ptr::null_mut())) };
        DeviceCsVec { h }
    }

    /// `binop::csmat_binop_dense_raw` (binop.rs:384-433) with one of the two closures the reference ships: `Op::Add` writes
    /// `(alpha * l) + (beta * r)`, `Op::Mul` `(alpha * l) * r` into every element of `out`.  The reference's panics in its
    /// order: "Dimension mismatch", then "Storage mismatch" unless CSR meets standard layout / CSC meets `.f()` layout.
    pub fn csmat_binop_dense_raw(lhs: &DeviceCsMat, rhs: &super::DeviceMat, op: Op, alpha: f64, beta: f64, out: &mut super::DeviceMat) {
        let (rows, cols) = lhs.shape();
        if cols != rhs.cols || cols != out.cols || rows != rhs.rows || rows != out.rows {
            panic!("Dimension mismatch");
        }
        if rhs.col_major != out.col_major {
            panic!("Storage mismatch");
        }
        unsafe {
            check(sys::sprs_hip_csmat_binop_dense_f64(lhs.h, rhs.buf.ptr, rhs.rows as u64, rhs.cols as u64, rhs.layout(), rhs.ld(), op as i32,
                                                      alpha, beta, out.buf.ptr, out.ld(), std::ptr::null_mut()));
        }
    }

    fn like(rhs: &super::DeviceMat) -> super::DeviceMat {
        if rhs.col_major { super::DeviceMat::zeros_f(rhs.shape()) } else { super::DeviceMat::zeros(rhs.shape()) }
    }

    /// `binop::add_dense_mat_same_ordering` (binop.rs:279-323): `alpha * lhs + beta * rhs` in the layout of `rhs`.
    pub fn add_dense_mat_same_ordering(lhs: &DeviceCsMat, rhs: &super::DeviceMat, alpha: f64, beta: f64) -> super::DeviceMat {
        let mut out = like(rhs);
        csmat_binop_dense_raw(lhs, rhs, Op::Add, alpha, beta, &mut out);
        out
    }

    /// `binop::mul_dense_mat_same_ordering` (binop.rs:331-371): the coefficient-wise `alpha * lhs * rhs` in the layout of `rhs`.
    pub fn mul_dense_mat_same_ordering(lhs: &DeviceCsMat, rhs: &super::DeviceMat, alpha: f64) -> super::DeviceMat {
        let mut out = like(rhs);
        csmat_binop_dense_raw(lhs, rhs, Op::Mul, alpha, 1.0, &mut out);
        out
    }
}

/// `&A + &D` for a dense `D` (csmat.rs:1951-1987): `A.to_other_storage()` first when its storage does not match the layout of
/// `D` — done below the C ABI; the result has the layout of `D`.
impl<'a, 'b> std::ops::Add<&'b DeviceMat> for &'a DeviceCsMat {
    type Output = DeviceMat;
    fn add(self, rhs: &'b DeviceMat) -> DeviceMat {
        let out = if rhs.col_major { DeviceMat::zeros_f(rhs.shape()) } else { DeviceMat::zeros(rhs.shape()) };
        unsafe {
            check(sys::sprs_hip_csmat_add_dense_f64(self.h, rhs.buf.ptr, rhs.rows as u64, rhs.cols as u64, rhs.layout(), rhs.ld(), out.buf.ptr,
                                                    std::ptr::null_mut()));
        }
        out
    }
}

/// Twin of `sprs::sparse::to_dense` (to_dense.rs:12-30): `array[row, col] = value` for every stored entry; the array is not
/// zeroed first.  Panics with "Dimension mismatch" like the reference's two asserts.
pub fn assign_to_dense(array: &mut DeviceMat, spmat: &DeviceCsMat) {
    unsafe {
        check(sys::sprs_hip_csmat_assign_to_dense_f64(spmat.h, array.buf.ptr, array.rows as u64, array.cols as u64, array.layout(), array.ld(),
                                                      std::ptr::null_mut()));
    }
}

impl DeviceCsMat {
    /// `CsMat::to_dense` (csmat.rs:1127-1134): `Array::zeros((rows, cols))`, then `assign_to_dense`.
    pub fn to_dense(&self) -> DeviceMat {
        let out = DeviceMat::zeros(self.shape());
        unsafe {
            check(sys::sprs_hip_csmat_to_dense_f64(self.h, out.buf.ptr, out.rows as u64, out.cols as u64, out.layout(), out.ld(),
                                                   std::ptr::null_mut()));
        }
        out
    }

    fn from_dense(storage: i32, m: &DeviceMat, epsilon: f64) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        let w = std::mem::size_of::<usize>() as i32;
        unsafe {
            check(sys::sprs_hip_csmat_from_dense_f64(&mut h, storage, m.buf.ptr, m.rows as u64, m.cols as u64, m.layout(), m.ld(), epsilon, w, w,
                                                     std::ptr::null_mut()));
        }
        DeviceCsMat { h }
    }

    /// `CsMat::csr_from_dense` (csmat.rs:499-539): the elements with `|x| > epsilon`; a negative epsilon is clamped to zero.
    pub fn csr_from_dense(m: &DeviceMat, epsilon: f64) -> DeviceCsMat {
        Self::from_dense(sys::SPRS_HIP_CSR, m, epsilon)
    }

    /// `CsMat::csc_from_dense` (csmat.rs:541-549).
    pub fn csc_from_dense(m: &DeviceMat, epsilon: f64) -> DeviceCsMat {
        Self::from_dense(sys::SPRS_HIP_CSC, m, epsilon)
    }
}

/// `&A + &B` (binop.rs:52-64): `rhs.to_other_storage()` first when the storages differ — done below the C ABI.
impl<'a, 'b> std::ops::Add<&'b DeviceCsMat> for &'a DeviceCsMat {
    type Output = DeviceCsMat;
    fn add(self, rhs: &'b DeviceCsMat) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_add_csmat_f64(self.h, rhs.h, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }
}

/// `&A - &B` (binop.rs:99-111).
impl<'a, 'b> std::ops::Sub<&'b DeviceCsMat> for &'a DeviceCsMat {
    type Output = DeviceCsMat;
    fn sub(self, rhs: &'b DeviceCsMat) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_sub_csmat_f64(self.h, rhs.h, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }
}

/// `&A * s` (binop.rs:132-163): `A.map(|x| x * s)`, the structure unchanged.
impl<'a> std::ops::Mul<f64> for &'a DeviceCsMat {
    type Output = DeviceCsMat;
    fn mul(self, rhs: f64) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_scale_f64(self.h, rhs, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }
}

/// `&v + &w` (vec.rs:1133-1205).
impl<'a, 'b> std::ops::Add<&'b DeviceCsVec> for &'a DeviceCsVec {
    type Output = DeviceCsVec;
    fn add(self, rhs: &'b DeviceCsVec) -> DeviceCsVec {
        binop::csvec_binop(self, rhs, binop::Op::Add)
    }
}

/// `&v - &w` (vec.rs:1207-1226).
impl<'a, 'b> std::ops::Sub<&'b DeviceCsVec> for &'a DeviceCsVec {
    type Output = DeviceCsVec;
    fn sub(self, rhs: &'b DeviceCsVec) -> DeviceCsVec {
        binop::csvec_binop(self, rhs, binop::Op::Sub)
    }
}

/// Device twin of `PermOwnedI<I>` (sprs/src/sparse/permutation.rs:12-28): the Identity variant, or `perm` and `perm_inv` in HBM.
pub struct DevicePerm {
    h: *mut sys::sprs_hip_perm,
}

unsafe impl Send for DevicePerm {}
unsafe impl Sync for DevicePerm {}

impl DevicePerm {
    /// `PermOwned::new` (permutation.rs:52-66): panics with "invalid permutation" where the reference's assert fires.
    pub fn new<I: SpIndex>(perm: &[I]) -> Self {
        let mut h = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_perm_upload(&mut h, perm.len() as u64, perm.as_ptr() as *const c_void, std::mem::size_of::<I>() as i32, 1)) };
        Self { h }
    }

    /// From a host permutation whose invariants `PermOwned::new` already checked.
    pub fn from_view<I: SpIndex>(perm: sprs::PermViewI<I>) -> Self {
        let v = perm.vec();
        let mut h = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_perm_upload(&mut h, v.len() as u64, v.as_ptr() as *const c_void, std::mem::size_of::<I>() as i32, 0)) };
        Self { h }
    }

    /// `Permutation::identity` (permutation.rs:113-118): no arrays.
    pub fn identity<I: SpIndex>(dim: usize) -> Self {
        let mut h = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_perm_identity(&mut h, dim as u64, std::mem::size_of::<I>() as i32)) };
        Self { h }
    }

    pub fn dim(&self) -> usize {
        let mut d = 0u64;
        unsafe { check(sys::sprs_hip_perm_info(self.h, &mut d, std::ptr::null_mut(), std::ptr::null_mut())) };
        d as usize
    }

    /// permutation.rs:144-152: the elementwise test.
    pub fn is_identity(&self) -> bool {
        let mut flag = 0i32;
        unsafe { check(sys::sprs_hip_perm_is_identity(self.h, &mut flag, std::ptr::null_mut())) };
        flag != 0
    }

    /// permutation.rs:120-137, as a new owning handle.
    pub fn inv(&self) -> DevicePerm {
        let mut h = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_perm_inv(self.h, &mut h)) };
        DevicePerm { h }
    }

    fn download<I: SpIndex>(&self, inverse: bool) -> Vec<I> {
        let (mut d, mut ib) = (0u64, 0i32);
        unsafe { check(sys::sprs_hip_perm_info(self.h, &mut d, &mut ib, std::ptr::null_mut())) };
        assert_eq!(ib as usize, std::mem::size_of::<I>(), "index width of the device permutation");
        let mut out = vec![I::zero(); d as usize];
        let p = out.as_mut_ptr() as *mut c_void;
        let null = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_perm_download(self.h, if inverse { null } else { p }, if inverse { p } else { null })) };
        out
    }

    /// permutation.rs:211-217
    pub fn vec<I: SpIndex>(&self) -> Vec<I> {
        self.download(false)
    }

    /// permutation.rs:219-226
    pub fn inv_vec<I: SpIndex>(&self) -> Vec<I> {
        self.download(true)
    }
}

impl Drop for DevicePerm {
    fn drop(&mut self) {
        unsafe { sys::sprs_hip_perm_free(self.h) };
    }
}

/// `&P * &x` (permutation.rs:255-278): `y[i] = x[p[i]]`.
impl<'a, 'b> std::ops::Mul<&'b DeviceVec> for &'a DevicePerm {
    type Output = DeviceVec;
    fn mul(self, rhs: &'b DeviceVec) -> DeviceVec {
        let y = DeviceVec::zeros(rhs.len);
        unsafe {
            check(sys::sprs_hip_perm_mul_vec_f64(self.h, rhs.ptr as *const f64, y.ptr, rhs.len as u64, std::ptr::null_mut()));
            check(sys::sprs_hip_synchronize(std::ptr::null_mut()));
        }
        y
    }
}

/// Twin of `sprs::sparse::permutation` (sprs/src/sparse/permutation.rs:296-581) for device operands: one algorithm — result
/// outer slice r' is outer slice o[r'], inner index j becomes g[j], slices sorted — so results are the reference's bit for bit.
pub mod permutation {
    use super::{check, sys, DeviceCsMat, DevicePerm};

    /// `transform_mat_paq` (permutation.rs:496-581): P * A * Q.
    pub fn transform_mat_paq(mat: &DeviceCsMat, row_perm: &DevicePerm, col_perm: &DevicePerm) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_transform_paq(mat.h, row_perm.h, col_perm.h, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }

    /// `permute_rows` (permutation.rs:407-420): P * A.  (The Identity variant gives a copy; the reference is unreachable!() there.)
    pub fn permute_rows(mat: &DeviceCsMat, perm: &DevicePerm) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_transform_paq(mat.h, perm.h, std::ptr::null(), &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }

    /// `permute_cols` (permutation.rs:423-436): A * P.
    pub fn permute_cols(mat: &DeviceCsMat, perm: &DevicePerm) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_transform_paq(mat.h, std::ptr::null(), perm.h, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }

    /// `transform_mat_papt` (permutation.rs:439-491): P * A * P^T; panics with "Dimension mismatch" unless A is square and of
    /// the permutation's dimension.
    pub fn transform_mat_papt(mat: &DeviceCsMat, perm: &DevicePerm) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_transform_papt(mat.h, perm.h, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }
}

impl DeviceCsMat {
    /// `CsMat::degrees` (csmat.rs:1205-1216): per outer index the stored entries off the diagonal.
    pub fn degrees(&self) -> Vec<usize> {
        let (rows, cols, _, _, _, st) = self.info();
        let outer = if st == sys::SPRS_HIP_CSR { rows } else { cols };
        // (the words travel in a DeviceVec: 8 bytes each, released when it goes out of scope — also on a panic)
        let buf = DeviceVec::zeros(outer);
        unsafe { check(sys::sprs_hip_csmat_degrees(self.h, buf.ptr as *mut u64, std::ptr::null_mut())) };
        let host: Vec<u64> = buf.to_vec().into_iter().map(f64::to_bits).collect();
        host.into_iter().map(|d| d as usize).collect()
    }

    /// `CsMat::max_outer_nnz` (csmat.rs:1188-1193).
    pub fn max_outer_nnz(&self) -> usize {
        let mut v = 0u64;
        unsafe { check(sys::sprs_hip_csmat_max_outer_nnz(self.h, &mut v, std::ptr::null_mut())) };
        v as usize
    }
}

/// The finding of a structure check as the reference's error: the kind from the info struct, the text (one of the reference's
/// own `&'static str`s) from `sprs_hip_last_error()`.  Any other failure panics like every other call here.
fn structure_result(status: i32, info: &sys::sprs_hip_structure_info) -> Result<(), sprs::errors::StructureError> {
    use sprs::errors::StructureError;
    if status != sys::SPRS_HIP_BAD_STRUCTURE {
        check(status);
        return Ok(());
    }
    const TEXTS: [&str; 10] = [
        "Index type not large enough for this matrix",
        "Iptr type not large enough for this matrix",
        "Unsorted indptr",
        "An indptr value is larger than allowed",
        "Indices length and inpdtr's nnz do not match",
        "Indices are not sorted",
        "Indice is larger than inner dimension",
        "Index size is too small",
        "Unsorted indices",
        "indices larger than vector size",
    ];
    let msg = unsafe { CStr::from_ptr(sys::sprs_hip_last_error()) }.to_string_lossy().into_owned();
    let text = TEXTS.iter().copied().find(|t| *t == msg).unwrap_or("invalid structure");
    Err(match info.kind {
        1 => StructureError::Unsorted(text),
        2 => StructureError::SizeMismatch(text),
        _ => StructureError::OutOfRange(text),
    })
}

/// Structure checks and unsorted input on the device (include/sprs_hip.h, "structure checks and unsorted input").
impl DeviceCsMat {
    fn upload_unchecked<I: SpIndex, Iptr: SpIndex>(storage: i32, shape: (usize, usize), indptr: &[Iptr], indices: &[I], data: &[f64]) -> Self {
        let outer = if storage == sys::SPRS_HIP_CSR { shape.0 } else { shape.1 };
        assert_eq!(indptr.len(), outer + 1, "Indptr length does not match dimension");
        assert_eq!(indices.len(), data.len(), "data and indices have different sizes");
        // (the upload sizes its copies by the indptr)
        assert_eq!(indptr[outer].index() - indptr[0].index(), indices.len(), "Indices length and inpdtr's nnz do not match");
        let mut h = std::ptr::null_mut();
        unsafe {
            check(sys::sprs_hip_csmat_upload(
                &mut h, storage, shape.0 as u64, shape.1 as u64, indptr.as_ptr() as *const c_void, std::mem::size_of::<Iptr>() as i32,
                indices.as_ptr() as *const c_void, std::mem::size_of::<I>() as i32, data.as_ptr(), 0,
            ));
        }
        Self { h }
    }

    /// `CsMat::new_from_unsorted` (csmat.rs:374-384): the arrays are uploaded as they are, sorted and validated on the device.
    pub fn new_from_unsorted<I: SpIndex, Iptr: SpIndex>(
        shape: (usize, usize), indptr: &[Iptr], indices: &[I], data: &[f64],
    ) -> Result<Self, sprs::errors::StructureError> {
        Self::upload_unchecked(sys::SPRS_HIP_CSR, shape, indptr, indices, data).sort_indices()
    }

    /// `CsMat::new_from_unsorted_csc` (csmat.rs:391-401).
    pub fn new_from_unsorted_csc<I: SpIndex, Iptr: SpIndex>(
        shape: (usize, usize), indptr: &[Iptr], indices: &[I], data: &[f64],
    ) -> Result<Self, sprs::errors::StructureError> {
        Self::upload_unchecked(sys::SPRS_HIP_CSC, shape, indptr, indices, data).sort_indices()
    }

    /// `utils::check_compressed_structure` (sparse.rs:300-358) on the device arrays.
    pub fn check_compressed_structure(&self) -> Result<(), sprs::errors::StructureError> {
        let mut info = sys::sprs_hip_structure_info::default();
        let status = unsafe { sys::sprs_hip_csmat_check_structure(self.h, &mut info, std::ptr::null_mut()) };
        structure_result(status, &info)
    }

    /// A new matrix whose outer slices are sorted by inner index, validated; `self` is only read.
    pub fn sort_indices(&self) -> Result<DeviceCsMat, sprs::errors::StructureError> {
        let mut info = sys::sprs_hip_structure_info::default();
        let mut h = std::ptr::null_mut();
        let status = unsafe { sys::sprs_hip_csmat_from_unsorted(self.h, &mut h, &mut info, std::ptr::null_mut()) };
        structure_result(status, &info).map(|_| DeviceCsMat { h })
    }
}

impl DeviceCsVec {
    /// `CsVec::new_from_unsorted` (vec.rs:536-557): check, sort only on Unsorted, check again — on the device.
    pub fn new_from_unsorted<I: SpIndex>(n: usize, indices: &[I], data: &[f64]) -> Result<Self, sprs::errors::StructureError> {
        assert_eq!(indices.len(), data.len(), "indices and data do not have compatible lengths");
        let mut h = std::ptr::null_mut();
        unsafe {
            check(sys::sprs_hip_csvec_upload(
                &mut h, n as u64, indices.len() as u64, indices.as_ptr() as *const c_void, std::mem::size_of::<I>() as i32, data.as_ptr(), 0,
            ));
        }
        (Self { h }).sort_indices()
    }

    /// The invariants of `CsVec::try_new` (vec.rs:440-491) on the device arrays.
    pub fn check_structure(&self) -> Result<(), sprs::errors::StructureError> {
        let mut info = sys::sprs_hip_structure_info::default();
        let status = unsafe { sys::sprs_hip_csvec_check_structure(self.h, &mut info, std::ptr::null_mut()) };
        structure_result(status, &info)
    }

    /// A new sorted, validated vector; `self` is only read.
    pub fn sort_indices(&self) -> Result<DeviceCsVec, sprs::errors::StructureError> {
        let mut info = sys::sprs_hip_structure_info::default();
        let mut h = std::ptr::null_mut();
        let status = unsafe { sys::sprs_hip_csvec_from_unsorted(self.h, &mut h, &mut info, std::ptr::null_mut()) };
        structure_result(status, &info).map(|_| DeviceCsVec { h })
    }
}

/// Twin of `sprs::sparse::linalg::ordering` (linalg/ordering.rs) and of `sprs::sparse::symmetric::is_symmetric` for device
/// operands: the matrix stays in HBM and the permutation arrives there, ready for `permutation::transform_mat_papt`.  The result is
/// the reference's with ties between vertices of equal degree broken by vertex id (the stable outcome of its
/// sort_unstable_by_key).  The start strategies and directions are values, not type parameters: the device runs the three
/// strategies the reference ships.
pub mod ordering {
    use super::{check, sys, DeviceCsMat, DevicePerm};

    /// `start::{Next, MinimumDegree, PseudoPeripheral}` (ordering.rs:14-267)
    #[derive(Debug, Clone, Copy, PartialEq, Eq)]
    pub enum Start {
        Next = sys::SPRS_HIP_START_NEXT as isize,
        MinimumDegree = sys::SPRS_HIP_START_MINIMUM_DEGREE as isize,
        PseudoPeripheral = sys::SPRS_HIP_START_PSEUDO_PERIPHERAL as isize,
    }

    /// `order::{Forward, Reversed}` (ordering.rs:269-420)
    #[derive(Debug, Clone, Copy, PartialEq, Eq)]
    pub enum Order {
        Forward = 0,
        Reversed = 1,
    }

    /// `Ordering` (ordering.rs:7-12)
    pub struct Ordering {
        pub perm: DevicePerm,
        pub connected_parts: Vec<usize>,
    }

    /// `cuthill_mckee_custom` (ordering.rs:440-526); panics with the text of the reference's assert_eq! on a non-square matrix.
    pub fn cuthill_mckee_custom(mat: &DeviceCsMat, start: Start, order: Order) -> Ordering {
        struct Handle(*mut sys::sprs_hip_ordering);
        impl Drop for Handle {
            fn drop(&mut self) {
                unsafe { sys::sprs_hip_ordering_free(self.0) };
            }
        }
        let mut o = Handle(std::ptr::null_mut());
        unsafe { check(sys::sprs_hip_csmat_cuthill_mckee(mat.h, start as i32, order as i32, 0, &mut o.0, std::ptr::null_mut())) };
        let mut n_parts = 0u64;
        unsafe { check(sys::sprs_hip_ordering_info(o.0, std::ptr::null_mut(), &mut n_parts, std::ptr::null_mut())) };
        let mut parts = vec![0u64; n_parts as usize];
        unsafe { check(sys::sprs_hip_ordering_parts(o.0, parts.as_mut_ptr())) };
        let mut perm: *mut sys::sprs_hip_perm = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_ordering_perm(o.0, &mut perm)) };
        Ordering { perm: DevicePerm { h: perm }, connected_parts: parts.into_iter().map(|p| p as usize).collect() }
    }

    /// `reverse_cuthill_mckee` (ordering.rs:546-559)
    pub fn reverse_cuthill_mckee(mat: &DeviceCsMat) -> Ordering {
        cuthill_mckee_custom(mat, Start::PseudoPeripheral, Order::Reversed)
    }

    /// `is_symmetric` (symmetric.rs:7-34)
    pub fn is_symmetric(mat: &DeviceCsMat) -> bool {
        let mut flag = 0i32;
        unsafe { check(sys::sprs_hip_csmat_is_symmetric(mat.h, &mut flag, std::ptr::null_mut())) };
        flag != 0
    }
}

/// Twin of the `sprs-ldl` crate (sprs-ldl/src/lib.rs) for device operands: `Ldl`, `LdlSymbolic`, `LdlNumeric`, `ldl_lsolve`,
/// `ldl_ltsolve` and `diag_solve` under the reference's names, f64.  l_colptr, the elimination tree, l_indices and every bit of
/// l_data, d and the solutions are the reference's.  Its panics arrive as panics with its text, `Err(SingularMatrix)` as `Err`.
pub mod ldl {
    use super::{check, sys, DeviceCsMat, DevicePerm, DeviceVec};
    use sprs::errors::{LinalgError, SingularMatrixInfo};
    pub use sprs::{FillInReduction, PermutationCheck, SymmetryCheck};

    fn singular(info: &sys::sprs_hip_trisolve_info) -> LinalgError {
        LinalgError::SingularMatrix(SingularMatrixInfo { index: info.singular_index as usize, reason: "diagonal element is a numeric 0" })
    }

    /// `LdlSymbolic` (lib.rs:94-100, 228-324)
    pub struct LdlSymbolic {
        h: *mut sys::sprs_hip_ldl_sym,
        n: usize,
        nnz: usize,
    }

    /// `LdlNumeric` (lib.rs:102-111, 326-442)
    pub struct LdlNumeric {
        h: *mut sys::sprs_hip_ldl_num,
        n: usize,
        nnz: usize,
    }

    unsafe impl Send for LdlSymbolic {}
    unsafe impl Send for LdlNumeric {}

    impl LdlSymbolic {
        /// `LdlSymbolic::new` (lib.rs:234-241)
        pub fn new(mat: &DeviceCsMat) -> Self {
            Self::new_perm(mat, None, SymmetryCheck::CheckSymmetry)
        }

        /// `LdlSymbolic::new_perm` (lib.rs:252-284); `None` is the identity.
        pub fn new_perm(mat: &DeviceCsMat, perm: Option<&DevicePerm>, check_symmetry: SymmetryCheck) -> Self {
            let mut h = std::ptr::null_mut();
            let p = perm.map_or(std::ptr::null(), |p| p.h as *const sys::sprs_hip_perm);
            let chk = matches!(check_symmetry, SymmetryCheck::CheckSymmetry) as i32;
            unsafe { check(sys::sprs_hip_ldl_symbolic(mat.h, p, chk, &mut h, std::ptr::null_mut())) };
            let (mut n, mut nnz) = (0u64, 0u64);
            unsafe { check(sys::sprs_hip_ldl_symbolic_info(h, &mut n, &mut nnz, std::ptr::null_mut())) };
            Self { h, n: n as usize, nnz: nnz as usize }
        }

        /// lib.rs:288
        pub fn problem_size(&self) -> usize {
            self.n
        }

        /// lib.rs:294
        pub fn nnz(&self) -> usize {
            self.nnz
        }

        /// l_colptr
        pub fn colptr(&self) -> Vec<usize> {
            let mut out = vec![0u64; self.n + 1];
            unsafe { check(sys::sprs_hip_ldl_symbolic_colptr(self.h, out.as_mut_ptr())) };
            out.into_iter().map(|v| v as usize).collect()
        }

        /// the elimination tree, `None` for a root (etree.rs)
        pub fn parents(&self) -> Vec<Option<usize>> {
            let mut out = vec![0u64; self.n.max(1)];
            unsafe { check(sys::sprs_hip_ldl_symbolic_parents(self.h, out.as_mut_ptr())) };
            out.truncate(self.n);
            out.into_iter().map(|v| if v == u64::MAX { None } else { Some(v as usize) }).collect()
        }

        pub fn perm(&self) -> DevicePerm {
            let mut p: *mut sys::sprs_hip_perm = std::ptr::null_mut();
            unsafe { check(sys::sprs_hip_ldl_symbolic_perm(self.h, &mut p)) };
            DevicePerm { h: p }
        }

        /// `LdlSymbolic::factor` (lib.rs:300-323)
        pub fn factor(self, mat: &DeviceCsMat) -> Result<LdlNumeric, LinalgError> {
            let mut f = std::ptr::null_mut();
            let mut info = sys::sprs_hip_trisolve_info::default();
            let st = unsafe { sys::sprs_hip_ldl_factor_f64(self.h, mat.h, &mut f, &mut info, std::ptr::null_mut()) };
            if st == sys::SPRS_HIP_SINGULAR_MATRIX {
                return Err(singular(&info));
            }
            check(st);
            Ok(LdlNumeric { h: f, n: self.n, nnz: self.nnz })
        }
    }

    impl Drop for LdlSymbolic {
        fn drop(&mut self) {
            unsafe { sys::sprs_hip_ldl_symbolic_free(self.h) };
        }
    }

    impl LdlNumeric {
        /// `LdlNumeric::new` (lib.rs:332-338)
        pub fn new(mat: &DeviceCsMat) -> Result<Self, LinalgError> {
            LdlSymbolic::new(mat).factor(mat)
        }

        /// `LdlNumeric::new_perm` (lib.rs:349-359)
        pub fn new_perm(mat: &DeviceCsMat, perm: Option<&DevicePerm>, check_symmetry: SymmetryCheck) -> Result<Self, LinalgError> {
            LdlSymbolic::new_perm(mat, perm, check_symmetry).factor(mat)
        }

        /// `LdlNumeric::update` (lib.rs:364-381)
        pub fn update(&mut self, mat: &DeviceCsMat) -> Result<(), LinalgError> {
            let mut info = sys::sprs_hip_trisolve_info::default();
            let st = unsafe { sys::sprs_hip_ldl_update_f64(self.h, mat.h, &mut info, std::ptr::null_mut()) };
            if st == sys::SPRS_HIP_SINGULAR_MATRIX {
                return Err(singular(&info));
            }
            check(st);
            Ok(())
        }

        /// `LdlNumeric::solve` (lib.rs:388-410)
        pub fn solve(&self, rhs: &DeviceVec) -> DeviceVec {
            let x = DeviceVec::zeros(rhs.len);
            unsafe { check(sys::sprs_hip_ldl_solve_f64(self.h, rhs.ptr as *const f64, x.ptr, rhs.len as u64, std::ptr::null_mut())) };
            x
        }

        /// lib.rs:413
        pub fn d(&self) -> DeviceVec {
            let out = DeviceVec::zeros(self.n);
            unsafe {
                check(sys::sprs_hip_ldl_d(self.h, out.ptr, self.n as u64, std::ptr::null_mut()));
                check(sys::sprs_hip_synchronize(std::ptr::null_mut()));
            }
            out
        }

        /// lib.rs:418-429: CSC, no diagonal stored
        pub fn l(&self) -> DeviceCsMat {
            let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
            unsafe { check(sys::sprs_hip_ldl_l(self.h, &mut h, std::ptr::null_mut())) };
            DeviceCsMat { h }
        }

        /// lib.rs:433
        pub fn problem_size(&self) -> usize {
            self.n
        }

        /// lib.rs:439
        pub fn nnz(&self) -> usize {
            self.nnz
        }
    }

    impl Drop for LdlNumeric {
        fn drop(&mut self) {
            unsafe { sys::sprs_hip_ldl_numeric_free(self.h) };
        }
    }

    /// The builder (lib.rs:74-226); `check_perm` is kept and, as in the reference's native path, never read.
    #[derive(Copy, Clone, Debug)]
    pub struct Ldl {
        check_symmetry: SymmetryCheck,
        check_perm: PermutationCheck,
        fill_red_method: FillInReduction,
    }

    impl Default for Ldl {
        fn default() -> Self {
            Self {
                check_symmetry: SymmetryCheck::CheckSymmetry,
                fill_red_method: FillInReduction::ReverseCuthillMcKee,
                check_perm: PermutationCheck::CheckPerm,
            }
        }
    }

    impl Ldl {
        pub fn new() -> Self {
            Self::default()
        }

        pub fn check_symmetry(self, check: SymmetryCheck) -> Self {
            Self { check_symmetry: check, ..self }
        }

        pub fn check_perm(self, check: PermutationCheck) -> Self {
            Self { check_perm: check, ..self }
        }

        pub fn fill_in_reduction(self, method: FillInReduction) -> Self {
            Self { fill_red_method: method, ..self }
        }

        /// lib.rs:139-162: `None` stands for `PermOwnedI::identity`
        pub fn perm(&self, mat: &DeviceCsMat) -> Option<DevicePerm> {
            match self.fill_red_method {
                FillInReduction::NoReduction => None,
                FillInReduction::ReverseCuthillMcKee => Some(super::ordering::reverse_cuthill_mckee(mat).perm),
                FillInReduction::CAMDSuiteSparse => panic!("Unavailable without the `sprs_suitesparse_camd` feature"),
                _ => unreachable!("Unhandled method, report a bug at https://github.com/vbarrielle/sprs/issues/199"),
            }
        }

        /// lib.rs:164-170
        pub fn symbolic(self, mat: &DeviceCsMat) -> LdlSymbolic {
            let _ = self.check_perm;
            let perm = self.perm(mat);
            LdlSymbolic::new_perm(mat, perm.as_ref(), self.check_symmetry)
        }

        /// lib.rs:190-201
        pub fn numeric(self, mat: &DeviceCsMat) -> Result<LdlNumeric, LinalgError> {
            self.symbolic(mat).factor(mat)
        }
    }

    /// `ldl_lsolve` (lib.rs:597-609), in place: `l` a strictly lower CSC matrix with an implied unit diagonal.
    pub fn ldl_lsolve(l: &DeviceCsMat, x: &mut DeviceVec) {
        unsafe { check(sys::sprs_hip_ldl_lsolve_f64(l.h, x.ptr, x.len as u64, std::ptr::null_mut())) };
    }

    /// `ldl_ltsolve` (lib.rs:613-626)
    pub fn ldl_ltsolve(l: &DeviceCsMat, x: &mut DeviceVec) {
        unsafe { check(sys::sprs_hip_ldl_ltsolve_f64(l.h, x.ptr, x.len as u64, std::ptr::null_mut())) };
    }

    /// `linalg::diag_solve` (sprs/src/sparse/linalg.rs:17-29): `x[i] /= diag[i]`
    pub fn diag_solve(diag: &DeviceVec, x: &mut DeviceVec) {
        assert_eq!(diag.len, x.len);
        unsafe { check(sys::sprs_hip_diag_solve_f64(diag.ptr as *const f64, x.ptr, x.len as u64, std::ptr::null_mut())) };
    }
}

/// Twins of `sprs::kronecker_product` (kronecker.rs:50-99) and of `sprs::sparse::construct` (construct.rs:10-160) on device
/// handles: same names, same argument order, the reference's panic texts.  One departure: `kronecker_product` panics by SHAPE
/// (inner(a) * inner(b) - 1 or nnz(a) * nnz(b) beyond the index types) where the reference panics on a stored index.
pub mod construct {
    use super::{check, sys, DeviceCsMat};

    fn handles(mats: &[&DeviceCsMat]) -> Vec<*const sys::sprs_hip_csmat> {
        mats.iter().map(|m| m.h as *const sys::sprs_hip_csmat).collect()
    }

    /// `kronecker_product`: the result has the storage of `a`; nothing is dropped.
    pub fn kronecker_product(a: &DeviceCsMat, b: &DeviceCsMat) -> DeviceCsMat {
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_kronecker_f64(a.h, b.h, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }

    /// `same_storage_fast_stack` (construct.rs:10-45).
    pub fn same_storage_fast_stack(mats: &[&DeviceCsMat]) -> DeviceCsMat {
        let mut hs = handles(mats);
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_same_storage_fast_stack(hs.as_mut_ptr(), hs.len() as u64, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }

    /// `vstack` (construct.rs:48-63): always CSR.
    pub fn vstack(mats: &[&DeviceCsMat]) -> DeviceCsMat {
        let mut hs = handles(mats);
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_vstack(hs.as_mut_ptr(), hs.len() as u64, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }

    /// `hstack` (construct.rs:66-81): always CSC.
    pub fn hstack(mats: &[&DeviceCsMat]) -> DeviceCsMat {
        let mut hs = handles(mats);
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_hstack(hs.as_mut_ptr(), hs.len() as u64, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }

    /// `bmat` (construct.rs:94-160): `None` is a zero block.  The ragged list panics here with "Dimension mismatch", between
    /// "Empty stacking list" and "Empty bmat row" as in the reference; the C entry only sees rectangles.
    pub fn bmat<'a, Row: AsRef<[Option<&'a DeviceCsMat>]>>(mats: &[Row]) -> DeviceCsMat {
        assert_ne!(mats.len(), 0, "Empty stacking list");
        let super_cols = mats[0].as_ref().len();
        assert_ne!(super_cols, 0, "Empty stacking list");
        assert!(mats.iter().all(|r| r.as_ref().len() == super_cols), "Dimension mismatch");
        let mut hs: Vec<*const sys::sprs_hip_csmat> = mats
            .iter()
            .flat_map(|r| r.as_ref().iter().map(|m| m.map_or(std::ptr::null(), |m| m.h as *const sys::sprs_hip_csmat)))
            .collect();
        let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
        unsafe { check(sys::sprs_hip_csmat_bmat(hs.as_mut_ptr(), mats.len() as u64, super_cols as u64, &mut h, std::ptr::null_mut())) };
        DeviceCsMat { h }
    }
}

/// Single precision: `CsMat<f32>` on the device, `&A * &x`, the dense products (`&A * &M`, `M.dot(&A)`, the four `mulacc_dense`
/// functions), `BiCGSTAB::<f32>`, the four dense-rhs triangular solves, `gauss_seidel` and `diag_solve` — what the reference instantiates for f32 on
/// the product path (bicgstab.rs:304-305; MulAcc, mul_acc.rs:17-31).  Types of their own over a handle type of its own: the
/// compiler rejects a product of mixed precision.  Every other operation is reached through `to_f64` / `from_f64`, on the device.
pub mod single {
    use super::*;

    /// A dense f32 vector in HBM.
    pub struct DeviceVecF32 {
        ptr: *mut f32,
        len: usize,
    }

    impl DeviceVecF32 {
        pub fn zeros(len: usize) -> Self {
            let mut p: *mut c_void = std::ptr::null_mut();
            unsafe {
                check(sys::sprs_hip_malloc(&mut p, (len * 4) as u64));
                check(sys::sprs_hip_memset(p, 0, (len * 4) as u64, std::ptr::null_mut()));
            }
            Self { ptr: p as *mut f32, len }
        }
        pub fn from_slice(x: &[f32]) -> Self {
            let v = Self::zeros(x.len());
            unsafe { check(sys::sprs_hip_memcpy_h2d(v.ptr as *mut c_void, x.as_ptr() as *const c_void, (x.len() * 4) as u64)) };
            v
        }
        pub fn to_vec(&self) -> Vec<f32> {
            let mut out = vec![0.0f32; self.len];
            unsafe {
                check(sys::sprs_hip_synchronize(std::ptr::null_mut()));
                check(sys::sprs_hip_memcpy_d2h(out.as_mut_ptr() as *mut c_void, self.ptr as *const c_void, (self.len * 4) as u64));
            }
            out
        }
        pub fn dim(&self) -> usize {
            self.len
        }
    }

    impl Drop for DeviceVecF32 {
        fn drop(&mut self) {
            unsafe { sys::sprs_hip_free(self.ptr as *mut c_void) };
        }
    }

    /// Device twin of `CsMatI<f32, I, Iptr>` with 4- or 8-byte index types.
    pub struct DeviceCsMatF32 {
        h: *mut sys::sprs_hip_csmat_f32,
    }

    unsafe impl Send for DeviceCsMatF32 {}

    impl DeviceCsMatF32 {
        /// Upload of host arrays (`CsMat::new` / `new_csc` when `validate`); `I` and `Iptr` must be 4 or 8 bytes wide.
        pub fn from_raw<I: Copy, Iptr: Copy>(csr: bool, rows: usize, cols: usize, indptr: &[Iptr], indices: &[I], data: &[f32],
                                             validate: bool) -> Self {
            let mut h: *mut sys::sprs_hip_csmat_f32 = std::ptr::null_mut();
            unsafe {
                check(sys::sprs_hip_csmat_f32_upload(&mut h, if csr { sys::SPRS_HIP_CSR } else { sys::SPRS_HIP_CSC }, rows as u64,
                                                     cols as u64, indptr.as_ptr() as *const c_void, std::mem::size_of::<Iptr>() as i32,
                                                     indices.as_ptr() as *const c_void, std::mem::size_of::<I>() as i32, data.as_ptr(),
                                                     validate as i32));
            }
            Self { h }
        }
        /// `CsMat::map(|&v| v as f32)` (csmat.rs:1289-1305)
        pub fn from_f64(m: &DeviceCsMat) -> Self {
            let mut h: *mut sys::sprs_hip_csmat_f32 = std::ptr::null_mut();
            unsafe { check(sys::sprs_hip_csmat_f32_from_f64(m.h, &mut h, std::ptr::null_mut())) };
            Self { h }
        }
        /// `CsMat::map(|&v| v as f64)`: exact
        pub fn to_f64(&self) -> DeviceCsMat {
            let mut h: *mut sys::sprs_hip_csmat = std::ptr::null_mut();
            unsafe { check(sys::sprs_hip_csmat_f32_to_f64(self.h, &mut h, std::ptr::null_mut())) };
            DeviceCsMat { h }
        }
        fn info(&self) -> (u64, u64, u64, i32, i32, i32) {
            let (mut r, mut c, mut n, mut pb, mut ib, mut st) = (0u64, 0u64, 0u64, 0i32, 0i32, 0i32);
            unsafe { check(sys::sprs_hip_csmat_f32_info(self.h, &mut r, &mut c, &mut n, &mut pb, &mut ib, &mut st)) };
            (r, c, n, pb, ib, st)
        }
        pub fn rows(&self) -> usize { self.info().0 as usize }
        pub fn cols(&self) -> usize { self.info().1 as usize }
        pub fn nnz(&self) -> usize { self.info().2 as usize }
        pub fn is_csr(&self) -> bool { self.info().5 == sys::SPRS_HIP_CSR }
        /// csmat.rs:1405-1426
        pub fn to_other_storage(&self) -> Self {
            let mut h: *mut sys::sprs_hip_csmat_f32 = std::ptr::null_mut();
            unsafe { check(sys::sprs_hip_csmat_f32_to_other_storage(self.h, &mut h)) };
            Self { h }
        }
        pub fn prepare(&mut self) {
            unsafe { check(sys::sprs_hip_csmat_f32_prepare(self.h, std::ptr::null_mut())) };
        }
        pub fn refresh(&mut self) {
            unsafe { check(sys::sprs_hip_csmat_f32_refresh(self.h)) };
        }
        /// (kind, plan bytes): 0 none yet, 1 nnz tiles, 3 banded copy
        pub fn spmv_plan_info(&self) -> (i32, u64) {
            let (mut kind, mut bytes) = (0i32, 0u64);
            unsafe { check(sys::sprs_hip_csmat_f32_spmv_plan_info(self.h, &mut kind, &mut bytes)) };
            (kind, bytes)
        }
        /// `&A * &x` for either storage
        pub fn mul_vec(&self, x: &DeviceVecF32) -> DeviceVecF32 {
            let y = DeviceVecF32::zeros(self.rows());
            unsafe { check(sys::sprs_hip_csmat_mul_vec_f32(self.h, x.ptr, x.len as u64, y.ptr, y.len as u64, std::ptr::null_mut())) };
            y
        }
        /// values to the host (8-byte handles: the arrays as u64)
        pub fn data_to_vec(&self) -> Vec<f32> {
            let mut out = vec![0.0f32; self.nnz()];
            unsafe { check(sys::sprs_hip_csmat_f32_download(self.h, std::ptr::null_mut(), std::ptr::null_mut(), out.as_mut_ptr())) };
            out
        }
    }

    impl Drop for DeviceCsMatF32 {
        fn drop(&mut self) {
            unsafe { sys::sprs_hip_csmat_f32_free(self.h) };
        }
    }

    /// prod::mul_acc_mat_vec_csr (prod.rs:103-127) for N = f32
    pub fn mul_acc_mat_vec_csr(mat: &DeviceCsMatF32, in_vec: &DeviceVecF32, res_vec: &mut DeviceVecF32) {
        unsafe {
            check(sys::sprs_hip_spmv_f32(mat.h, in_vec.ptr, in_vec.len as u64, res_vec.ptr, res_vec.len as u64, 1, std::ptr::null_mut()))
        };
    }

    /// prod::mul_acc_mat_vec_csc (prod.rs:74-99) for N = f32
    pub fn mul_acc_mat_vec_csc(mat: &DeviceCsMatF32, in_vec: &DeviceVecF32, res_vec: &mut DeviceVecF32) {
        unsafe {
            check(sys::sprs_hip_mul_acc_mat_vec_csc_f32(mat.h, in_vec.ptr, in_vec.len as u64, res_vec.ptr, res_vec.len as u64,
                                                        std::ptr::null_mut()))
        };
    }

    /// A dense f32 matrix in HBM with ndarray's two contiguous layouts: `DeviceMat` for N = f32.
    pub struct DeviceMatF32 {
        buf: DeviceVecF32,
        rows: usize,
        cols: usize,
        col_major: bool,
    }

    impl DeviceMatF32 {
        pub fn zeros(shape: (usize, usize)) -> Self {
            DeviceMatF32 { buf: DeviceVecF32::zeros(shape.0 * shape.1), rows: shape.0, cols: shape.1, col_major: false }
        }
        /// `Array::zeros(shape.f())`
        pub fn zeros_f(shape: (usize, usize)) -> Self {
            DeviceMatF32 { buf: DeviceVecF32::zeros(shape.0 * shape.1), rows: shape.0, cols: shape.1, col_major: true }
        }
        /// from an ndarray in standard layout (`as_slice()` order)
        pub fn from_rows(shape: (usize, usize), row_major: &[f32]) -> Self {
            assert_eq!(shape.0 * shape.1, row_major.len(), "Dimension mismatch");
            DeviceMatF32 { buf: DeviceVecF32::from_slice(row_major), rows: shape.0, cols: shape.1, col_major: false }
        }
        pub fn shape(&self) -> (usize, usize) { (self.rows, self.cols) }
        pub fn is_standard_layout(&self) -> bool { !self.col_major }
        /// the elements in memory order (row-major, or column-major when `!is_standard_layout()`)
        pub fn to_vec(&self) -> Vec<f32> { self.buf.to_vec() }
        fn layout(&self) -> i32 { if self.col_major { sys::SPRS_HIP_COL_MAJOR } else { sys::SPRS_HIP_ROW_MAJOR } }
        fn ld(&self) -> u64 { (if self.col_major { self.rows } else { self.cols }) as u64 }
        /// `Array2::dot(&CsMat)` (csmat.rs:2050-2117) for N = f32: dense . sparse
        pub fn dot(&self, rhs: &DeviceCsMatF32) -> DeviceMatF32 {
            let mut out = DeviceMatF32::zeros((self.rows, rhs.cols()));
            let mut lay = 0i32;
            unsafe {
                check(sys::sprs_hip_dense_dot_csmat_f32(self.buf.ptr, self.rows as u64, self.cols as u64, self.layout(), self.ld(), rhs.h,
                                                        out.buf.ptr, &mut lay, std::ptr::null_mut()));
            }
            out.col_major = lay == sys::SPRS_HIP_COL_MAJOR;
            out
        }
    }

    /// `&A * &M` for N = f32 (csmat.rs:1989-2048): standard layout for >= 8 columns, `.f()` layout below.
    impl<'a, 'b> std::ops::Mul<&'b DeviceMatF32> for &'a DeviceCsMatF32 {
        type Output = DeviceMatF32;
        fn mul(self, rhs: &'b DeviceMatF32) -> DeviceMatF32 {
            let mut out = DeviceMatF32::zeros((self.rows(), rhs.cols));
            let mut lay = 0i32;
            unsafe {
                check(sys::sprs_hip_csmat_mul_dense_f32(self.h, rhs.buf.ptr, rhs.rows as u64, rhs.cols as u64, rhs.layout(), rhs.ld(),
                                                        out.buf.ptr, &mut lay, std::ptr::null_mut()));
            }
            out.col_major = lay == sys::SPRS_HIP_COL_MAJOR;
            out
        }
    }

    fn mulacc_dense(lhs: &DeviceCsMatF32, rhs: &DeviceMatF32, out: &mut DeviceMatF32) {
        assert_eq!(rhs.cols, out.cols, "Dimension mismatch");                       // prod.rs:201
        unsafe {
            check(sys::sprs_hip_csmat_mulacc_dense_f32(lhs.h, rhs.buf.ptr, rhs.rows as u64, rhs.cols as u64, rhs.layout(), rhs.ld(),
                                                       out.buf.ptr, out.rows as u64, out.layout(), out.ld(), 1, std::ptr::null_mut()));
        }
    }
    /// Twins of `csr_mulacc_dense_rowmaj` / `_colmaj` (prod.rs:189-214, 274-298) and `csc_mulacc_dense_rowmaj` / `_colmaj`
    /// (prod.rs:219-270) for N = f32: `out += lhs * rhs`.
    pub fn csr_mulacc_dense_rowmaj(lhs: &DeviceCsMatF32, rhs: &DeviceMatF32, out: &mut DeviceMatF32) {
        assert!(lhs.is_csr(), "Storage mismatch");
        mulacc_dense(lhs, rhs, out)
    }
    pub fn csr_mulacc_dense_colmaj(lhs: &DeviceCsMatF32, rhs: &DeviceMatF32, out: &mut DeviceMatF32) {
        assert!(lhs.is_csr(), "Storage mismatch");
        mulacc_dense(lhs, rhs, out)
    }
    pub fn csc_mulacc_dense_rowmaj(lhs: &DeviceCsMatF32, rhs: &DeviceMatF32, out: &mut DeviceMatF32) {
        assert!(!lhs.is_csr(), "Storage mismatch");
        mulacc_dense(lhs, rhs, out)
    }
    pub fn csc_mulacc_dense_colmaj(lhs: &DeviceCsMatF32, rhs: &DeviceMatF32, out: &mut DeviceMatF32) {
        assert!(!lhs.is_csr(), "Storage mismatch");
        mulacc_dense(lhs, rhs, out)
    }

    /// `&A * &B` for N = f32 (csmat.rs:1866-1888 -> csmat_mul_csmat -> smmp::mul_csr_csr) in any pair of storages: every product
    /// and every partial sum rounded to f32, in the reference's order.
    impl<'a, 'b> std::ops::Mul<&'b DeviceCsMatF32> for &'a DeviceCsMatF32 {
        type Output = DeviceCsMatF32;
        fn mul(self, rhs: &'b DeviceCsMatF32) -> DeviceCsMatF32 {
            let mut h: *mut sys::sprs_hip_csmat_f32 = std::ptr::null_mut();
            unsafe { check(sys::sprs_hip_csmat_mul_csmat_f32(self.h, rhs.h, &mut h)) };
            DeviceCsMatF32 { h }
        }
    }

    /// `sprs::smmp` for N = f32
    pub mod smmp {
        use super::*;
        /// Twin of `smmp::mul_csr_csr` (smmp.rs:196-416)
        pub fn mul_csr_csr(lhs: &DeviceCsMatF32, rhs: &DeviceCsMatF32) -> DeviceCsMatF32 {
            let mut h: *mut sys::sprs_hip_csmat_f32 = std::ptr::null_mut();
            unsafe { check(sys::sprs_hip_spgemm_f32(lhs.h, rhs.h, &mut h)) };
            DeviceCsMatF32 { h }
        }
        /// Twin of `smmp::symbolic` (smmp.rs:81-131): the structure of `lhs * rhs`, values 0.0f32
        pub fn symbolic(lhs: &DeviceCsMatF32, rhs: &DeviceCsMatF32) -> DeviceCsMatF32 {
            let mut h: *mut sys::sprs_hip_csmat_f32 = std::ptr::null_mut();
            unsafe { check(sys::sprs_hip_spgemm_symbolic_f32(lhs.h, rhs.h, &mut h)) };
            DeviceCsMatF32 { h }
        }
        /// Twin of `smmp::numeric` (smmp.rs:151-189): the values of `lhs * rhs` into `c`, which must have the product's structure
        pub fn numeric(lhs: &DeviceCsMatF32, rhs: &DeviceCsMatF32, c: &mut DeviceCsMatF32) {
            unsafe { check(sys::sprs_hip_spgemm_numeric_f32(lhs.h, rhs.h, c.h)) };
        }

        /// The symbolic phase of `lhs * rhs`, kept: `structure`, `product` and `numeric` run the value kernels only.  The plan
        /// holds structure alone; it is released when dropped.
        pub struct SpgemmPlan {
            p: *mut sys::sprs_hip_spgemm_plan,
        }
        impl SpgemmPlan {
            pub fn new(lhs: &DeviceCsMatF32, rhs: &DeviceCsMatF32) -> Self {
                let mut p: *mut sys::sprs_hip_spgemm_plan = std::ptr::null_mut();
                unsafe { check(sys::sprs_hip_spgemm_plan_create_f32(lhs.h, rhs.h, &mut p)) };
                SpgemmPlan { p }
            }
            pub fn nnz(&self) -> usize {
                let mut n = 0u64;
                unsafe { check(sys::sprs_hip_spgemm_plan_nnz(self.p, &mut n)) };
                n as usize
            }
            pub fn structure(&mut self, lhs: &DeviceCsMatF32, rhs: &DeviceCsMatF32) -> DeviceCsMatF32 {
                let mut h: *mut sys::sprs_hip_csmat_f32 = std::ptr::null_mut();
                unsafe { check(sys::sprs_hip_spgemm_plan_structure_f32(self.p, lhs.h, rhs.h, &mut h)) };
                DeviceCsMatF32 { h }
            }
            pub fn product(&mut self, lhs: &DeviceCsMatF32, rhs: &DeviceCsMatF32) -> DeviceCsMatF32 {
                let mut h: *mut sys::sprs_hip_csmat_f32 = std::ptr::null_mut();
                unsafe { check(sys::sprs_hip_spgemm_plan_product_f32(self.p, lhs.h, rhs.h, &mut h)) };
                DeviceCsMatF32 { h }
            }
            pub fn numeric(&mut self, lhs: &DeviceCsMatF32, rhs: &DeviceCsMatF32, c: &mut DeviceCsMatF32) {
                unsafe { check(sys::sprs_hip_spgemm_plan_numeric_f32(self.p, lhs.h, rhs.h, c.h)) };
            }
        }
        impl Drop for SpgemmPlan {
            fn drop(&mut self) {
                unsafe { sys::sprs_hip_spgemm_plan_free(self.p) };
            }
        }
    }

    /// `BiCGSTAB::<f32>::solve` (bicgstab.rs:148-171): `Ok(solver)` / `Err(solver)` like the reference.
    pub struct BiCGSTAB {
        x: DeviceVecF32,
        info: sys::sprs_hip_bicgstab_info,
    }
    impl BiCGSTAB {
        pub fn solve(a: &DeviceCsMatF32, x0: &DeviceVecF32, b: &DeviceVecF32, tol: f32, max_iter: usize)
            -> Result<Box<BiCGSTAB>, Box<BiCGSTAB>> {
            assert_eq!(x0.len, b.len, "Dimension mismatch");
            let x = DeviceVecF32::zeros(x0.len);
            let mut info = sys::sprs_hip_bicgstab_info::default();
            unsafe {
                check(sys::sprs_hip_bicgstab_f32(a.h, x0.ptr, b.ptr, x0.len as u64, tol as f64, max_iter as u64, 0.1f32 as f64, x.ptr,
                                                 &mut info, std::ptr::null_mut()));
            }
            let s = Box::new(BiCGSTAB { x, info });
            if s.info.converged != 0 { Ok(s) } else { Err(s) }
        }
        pub fn iteration_count(&self) -> usize { self.info.iteration_count as usize }
        pub fn soft_restart_count(&self) -> usize { self.info.soft_restart_count as usize }
        pub fn hard_restart_count(&self) -> usize { self.info.hard_restart_count as usize }
        pub fn err(&self) -> f32 { self.info.err as f32 }
        pub fn rho(&self) -> f32 { self.info.rho as f32 }
        pub fn x(&self) -> &DeviceVecF32 { &self.x }
    }

    /// `gauss_seidel::<f32>` of the reference's heat example (examples/heat.rs:103-139): every iterate in the reference's f32
    /// bits; `Ok((iterations, error))` / `Err(error)` like the reference.
    pub fn gauss_seidel(mat: &DeviceCsMatF32, x: &mut DeviceVecF32, rhs: &DeviceVecF32, max_iter: usize, eps: f32)
        -> Result<(usize, f32), f32> {
        assert_eq!(x.len, rhs.len, "Dimension mismatch");
        let mut info = sys::sprs_hip_gauss_seidel_info::default();
        unsafe {
            check(sys::sprs_hip_gauss_seidel_f32(mat.h, x.ptr, rhs.ptr, x.len as u64, max_iter as u64, eps as f64, &mut info,
                                                 std::ptr::null_mut()));
        }
        if info.converged != 0 { Ok((info.iterations as usize, info.error as f32)) } else { Err(info.error as f32) }
    }

    /// The four dense-rhs solves of `sprs::linalg::trisolve` for N = f32, in place on a device-resident `rhs`: the same panics
    /// and the same `Err(LinalgError::SingularMatrix)` as the f64 twins, solutions in the reference's f32 bits.
    fn trisolve(mat: &DeviceCsMatF32, rhs: &mut DeviceVecF32, csr: bool, uplo: i32, csr_reason: &'static str)
        -> Result<(), sprs::errors::LinalgError> {
        let (rows, cols, _, _, _, st) = mat.info();
        assert_eq!(cols, rows, "Non square matrix passed to solver");
        assert_eq!(cols as usize, rhs.len, "Dimension mismatch");
        assert!((st == sys::SPRS_HIP_CSR) == csr, "Storage mismatch");
        let mut info = sys::sprs_hip_trisolve_info::default();
        let status = unsafe { sys::sprs_hip_trisolve_f32(mat.h, uplo, rhs.ptr, rhs.len as u64, &mut info, std::ptr::null_mut()) };
        if status == sys::SPRS_HIP_SINGULAR_MATRIX {
            let reason = match (csr, info.singular_reason) {
                (true, _) => csr_reason,
                (false, 2) => "diagonal element is a structural 0",
                (false, _) => "diagonal element is a numeric 0",
            };
            return Err(sprs::errors::LinalgError::SingularMatrix(sprs::errors::SingularMatrixInfo {
                index: info.singular_index as usize,
                reason,
            }));
        }
        check(status);
        Ok(())
    }

    /// `lsolve_csr_dense_rhs::<f32>` (trisolve.rs:30-73)
    pub fn lsolve_csr_dense_rhs(lower_tri_mat: &DeviceCsMatF32, rhs: &mut DeviceVecF32) -> Result<(), sprs::errors::LinalgError> {
        trisolve(lower_tri_mat, rhs, true, sys::SPRS_HIP_LOWER, "diagonal element is 0")
    }

    /// `lsolve_csc_dense_rhs::<f32>` (trisolve.rs:85-149)
    pub fn lsolve_csc_dense_rhs(lower_tri_mat: &DeviceCsMatF32, rhs: &mut DeviceVecF32) -> Result<(), sprs::errors::LinalgError> {
        trisolve(lower_tri_mat, rhs, false, sys::SPRS_HIP_LOWER, "")
    }

    /// `usolve_csc_dense_rhs::<f32>` (trisolve.rs:161-210)
    pub fn usolve_csc_dense_rhs(upper_tri_mat: &DeviceCsMatF32, rhs: &mut DeviceVecF32) -> Result<(), sprs::errors::LinalgError> {
        trisolve(upper_tri_mat, rhs, false, sys::SPRS_HIP_UPPER, "")
    }

    /// `usolve_csr_dense_rhs::<f32>` (trisolve.rs:219-262)
    pub fn usolve_csr_dense_rhs(upper_tri_mat: &DeviceCsMatF32, rhs: &mut DeviceVecF32) -> Result<(), sprs::errors::LinalgError> {
        trisolve(upper_tri_mat, rhs, true, sys::SPRS_HIP_UPPER, "diagonal element is a numeric 0")
    }

    /// `linalg::diag_solve::<f32>` (sprs/src/sparse/linalg.rs:17-29): `x[i] /= diag[i]`
    pub fn diag_solve(diag: &DeviceVecF32, x: &mut DeviceVecF32) {
        assert_eq!(diag.len, x.len);
        unsafe { check(sys::sprs_hip_diag_solve_f32(diag.ptr as *const f32, x.ptr, x.len as u64, std::ptr::null_mut())) };
    }
}
