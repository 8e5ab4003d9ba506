//! `struct BLU` of the `blu` crate (rwl/blu 0.2.1, `src/blu.rs:9-335`) on an MI355X: the same public methods,
//! argument meaning and `Status` values, with all numerical work done by the HIP kernels behind the C ABI of
//! `include/blu_hip.h` (`libblu_hip.so`).  A caller of the reference switches by replacing `use blu::BLU`
//! with `use blu_hip::BLU`.
//!
//! What differs, and why:
//! * `BLU.lu` is a public field as in the reference (`blu.rs:10`), but `struct LU` is not a struct of arrays in host
//!   memory (all state of the factorization lives in HBM): it owns the device handle and has the reference's public
//!   parameter fields as setter / getter pairs (`blu.lu.set_droptol(..)`, `blu.lu.droptol()`; `src/lu/lu.rs:11-66`)
//!   and its getters (`src/lu/lu.rs:398-684`) under the same names.  `BLU.realloc_factor` is a plain public field
//!   (`blu.rs:18-20`), handed to the library before every call that may grow storage.
//! * `Status::Reallocate` never reaches the caller of the object API in the reference either
//!   (`blu.rs:105-115, 277-283, 324-330`); the library grows its device storage itself.
//! * Two more error values exist: `ErrorDevice` (a HIP call failed, `last_error()` has the text) and
//!   `ErrorOutOfMemory` (`BLU_ERROR_OUT_OF_MEMORY` of the reference's C ancestry).
//! * `new` takes the HIP device ordinal through `BLU::new_on(m, b_nz, device)`; `BLU::new(m, b_nz)` uses device 0.
//!
//! NOT COMPILED in this repository's environment (no Rust toolchain in the image); the identical
//! call sequence is tested through the Python mirror `blu_amd/blu.py`.
#![allow(clippy::too_many_arguments)]

pub mod maxvolume;
pub use maxvolume::maxvolume;

use std::ffi::CStr;
use std::os::raw::{c_char, c_double, c_int};

/// BLU integer type (`src/lib.rs:32`).
pub type LUInt = i64;

/// `enum Status` of the reference (`src/lib.rs:38-64`) plus the two device-side failures.
#[derive(PartialEq, Clone, Copy, Debug)]
pub enum Status {
    Reallocate,
    WarningSingularMatrix,
    ErrorInvalidCall,
    ErrorArgumentMissing,
    ErrorInvalidArgument,
    ErrorMaximumUpdates,
    ErrorSingularUpdate,
    ErrorOutOfMemory,
    ErrorDevice,
}

#[repr(C)]
pub struct BluHip {
    _private: [u8; 0],
}

// include/blu_hip.h -- every entry cites the reference interface it replaces there.
extern "C" {
    fn blu_hip_new(m: i64, b_nz: i64, device: c_int) -> *mut BluHip;
    fn blu_hip_free(h: *mut BluHip);
    fn blu_hip_set_param(h: *mut BluHip, key: c_int, value: c_double) -> c_int;
    fn blu_hip_get_param(h: *const BluHip, key: c_int) -> c_double;
    fn blu_hip_get_stat(h: *const BluHip, key: c_int) -> c_double;
    fn blu_hip_factorize(h: *mut BluHip, b_begin: *const u64, b_end: *const u64, b_i: *const u64, b_x: *const f64, b_i_len: u64) -> c_int;
    fn blu_hip_get_factors(
        h: *mut BluHip, rowperm: *mut i64, colperm: *mut i64, l_colptr: *mut i64, l_rowidx: *mut i64, l_value: *mut f64,
        u_colptr: *mut i64, u_rowidx: *mut i64, u_value: *mut f64,
    ) -> c_int;
    fn blu_hip_solve_dense(h: *mut BluHip, rhs: *const f64, lhs: *mut f64, trans: c_char) -> c_int;
    fn blu_hip_solve_dense_multi(
        h: *mut BluHip, nrhs: i64, rhs: *const f64, ldrhs: i64, lhs: *mut f64, ldlhs: i64, trans: c_char, inputs_on_device: c_int,
    ) -> c_int;
    fn blu_hip_solve_sparse(
        h: *mut BluHip, nzrhs: i64, irhs: *const u64, xrhs: *const f64, p_nzlhs: *mut i64, ilhs: *mut i64, lhs: *mut f64, trans: c_char,
    ) -> c_int;
    fn blu_hip_solve_for_update(
        h: *mut BluHip, nzrhs: i64, irhs: *const u64, xrhs: *const f64, p_nzlhs: *mut i64, ilhs: *mut i64, lhs: *mut f64, trans: c_char,
    ) -> c_int;
    fn blu_hip_update(h: *mut BluHip, xtbl: c_double) -> c_int;
    fn blu_hip_solve_for_update_batch(
        h: *mut *mut BluHip, n: c_int, nzrhs: *const i64, irhs: *const *const u64, xrhs: *const *const f64, nzlhs: *mut i64,
        ilhs: *const *mut i64, lhs: *const *mut f64, trans: c_char, status: *mut c_int,
    ) -> c_int;
    fn blu_hip_update_batch(h: *mut *mut BluHip, n: c_int, xtbl: *const c_double, status: *mut c_int) -> c_int;
    fn blu_hip_solve_sparse_batch(
        h: *mut *mut BluHip, n: c_int, nzrhs: *const i64, irhs: *const *const u64, xrhs: *const *const f64, nzlhs: *mut i64,
        ilhs: *const *mut i64, lhs: *const *mut f64, trans: c_char, status: *mut c_int,
    ) -> c_int;
    fn blu_hip_solve_sparse_multi(
        h: *mut BluHip, nrhs: i64, rhs_ptr: *const i64, irhs: *const u64, xrhs: *const f64, trans: c_char, lhs_ptr: *mut i64,
        status: *mut c_int,
    ) -> c_int;
    fn blu_hip_get_sparse_multi(h: *mut BluHip, ilhs: *mut i64, xlhs: *mut f64) -> c_int;
    fn blu_hip_maxvolume(
        h: *mut BluHip, ncol: i64, a_p: *const u64, a_i: *const u64, a_x: *const f64, basis: *mut i64, isbasic: *mut i64, volumetol: f64,
        p_nupdate: *mut i64,
    ) -> c_int;
    fn blu_hip_set_matrix(h: *mut BluHip, ncol: i64, a_p: *const u64, a_i: *const u64, a_x: *const f64) -> c_int;
    fn blu_hip_factorize_columns(h: *mut BluHip, basis: *const i64) -> c_int;
    fn blu_hip_solve_for_update_column(h: *mut BluHip, j: i64, p_nzlhs: *mut i64, ilhs: *mut i64, lhs: *mut f64) -> c_int;
    fn blu_hip_tableau_row(
        h: *mut BluHip, r: i64, prepare_update: c_int, skip: *const i64, alpha: *mut f64, p_nzlhs: *mut i64, ilhs: *mut i64, lhs: *mut f64,
    ) -> c_int;
    fn blu_hip_price(h: *mut BluHip, y: *const f64, skip: *const i64, z: *mut f64) -> c_int;
    fn blu_hip_dbg_matrix_counts(h: *const BluHip, out: *mut i64) -> c_int;
    fn blu_hip_copy_batch(src: *mut BluHip, dst: *mut *mut BluHip, n: c_int, status: *mut c_int) -> c_int;
    fn blu_hip_share_matrix(src: *mut BluHip, dst: *mut *mut BluHip, n: c_int, status: *mut c_int) -> c_int;
    fn blu_hip_dbg_matrix_holders(h: *const BluHip) -> c_int;
    fn blu_hip_tableau_row_batch(
        h: *mut *mut BluHip, n: c_int, r: *const i64, prepare_update: c_int, skip: *const *const i64, alpha: *const *mut f64, nzlhs: *mut i64,
        ilhs: *const *mut i64, lhs: *const *mut f64, status: *mut c_int,
    ) -> c_int;
    fn blu_hip_price_batch(
        h: *mut *mut BluHip, n: c_int, y: *const *const f64, skip: *const *const i64, z: *const *mut f64, status: *mut c_int,
    ) -> c_int;
    fn blu_hip_set_duals(h: *mut BluHip, d: *const f64, kind: *const i8) -> c_int;
    fn blu_hip_get_duals(h: *mut BluHip, d: *mut f64, kind: *mut i8) -> c_int;
    fn blu_hip_get_ratio_row(h: *mut BluHip, alpha: *mut f64) -> c_int;
    fn blu_hip_ratio_test(
        h: *mut BluHip, r: i64, prepare_update: c_int, sigma: f64, pivtol: f64, dualtol: f64, out: *mut RatioResult, p_nzlhs: *mut i64,
        ilhs: *mut i64, lhs: *mut f64,
    ) -> c_int;
    fn blu_hip_update_duals(h: *mut BluHip, theta: f64, nset: i64, jset: *const i64, dset: *const f64, kset: *const i8) -> c_int;
    fn blu_hip_copy_duals_batch(src: *mut BluHip, dst: *mut *mut BluHip, n: c_int, status: *mut c_int) -> c_int;
    fn blu_hip_ratio_test_batch(
        h: *mut *mut BluHip, n: c_int, r: *const i64, prepare_update: c_int, sigma: *const f64, pivtol: f64, dualtol: f64,
        out: *mut RatioResult, nzlhs: *mut i64, ilhs: *const *mut i64, lhs: *const *mut f64, status: *mut c_int,
    ) -> c_int;
    fn blu_hip_update_duals_batch(
        h: *mut *mut BluHip, n: c_int, theta: *const f64, nset: *const i64, jset: *const *const i64, dset: *const *const f64,
        kset: *const *const i8, status: *mut c_int,
    ) -> c_int;
    fn blu_hip_clone(src: *mut BluHip) -> *mut BluHip;
    fn blu_hip_last_error(h: *const BluHip) -> *const c_char;
}

fn status_of(code: c_int) -> Result<(), Status> {
    match code {
        0 => Ok(()),
        1 => Err(Status::Reallocate),
        2 => Err(Status::WarningSingularMatrix),
        -2 => Err(Status::ErrorInvalidCall),
        -3 => Err(Status::ErrorArgumentMissing),
        -4 => Err(Status::ErrorInvalidArgument),
        -5 => Err(Status::ErrorMaximumUpdates),
        -6 => Err(Status::ErrorSingularUpdate),
        -9 => Err(Status::ErrorOutOfMemory),
        _ => Err(Status::ErrorDevice),
    }
}

// enum blu_param / enum blu_stat of include/blu_hip.h
mod key {
    pub const DROPTOL: i32 = 0;
    pub const ABSTOL: i32 = 1;
    pub const RELTOL: i32 = 2;
    pub const NZBIAS: i32 = 3;
    pub const MAXSEARCH: i32 = 4;
    pub const PAD: i32 = 5;
    pub const STRETCH: i32 = 6;
    pub const COMPRESS_THRES: i32 = 7;
    pub const SPARSE_THRES: i32 = 8;
    pub const SEARCH_ROWS: i32 = 9;
    pub const REALLOC_FACTOR: i32 = 10;
    pub const M: i32 = 0;
    pub const NUPDATE: i32 = 1;
    pub const NFACTORIZE: i32 = 2;
    pub const L_NZ: i32 = 3;
    pub const U_NZ: i32 = 4;
    pub const MIN_PIVOT: i32 = 5;
    pub const MAX_PIVOT: i32 = 6;
    pub const CONDEST_L: i32 = 7;
    pub const CONDEST_U: i32 = 8;
    pub const NORM_L: i32 = 9;
    pub const NORM_U: i32 = 10;
    pub const NORMEST_L_INV: i32 = 11;
    pub const NORMEST_U_INV: i32 = 12;
    pub const ONENORM: i32 = 13;
    pub const INFNORM: i32 = 14;
    pub const RESIDUAL_TEST: i32 = 15;
    pub const MATRIX_NZ: i32 = 16;
    pub const RANK: i32 = 17;
    pub const BUMP_SIZE: i32 = 18;
    pub const BUMP_NZ: i32 = 19;
    pub const NSEARCH_PIVOT: i32 = 20;
    pub const NEXPAND: i32 = 21;
    pub const NGARBAGE: i32 = 22;
    pub const FACTOR_FLOPS: i32 = 23;
    pub const TIME_FACTORIZE: i32 = 24;
    pub const NFORREST: i32 = 35;
    pub const PIVOT_ERROR: i32 = 36;
    pub const UPDATE_COST: i32 = 124;
}

/// `struct LU` (`src/lu/lu.rs`) as a user of the object API sees it: parameters and getters.  Owns the device handle.
pub struct LU {
    h: *mut BluHip,
}

macro_rules! param {
    ($get:ident, $set:ident, $key:expr, $t:ty) => {
        pub fn $get(&self) -> $t {
            unsafe { blu_hip_get_param(self.h, $key) as $t }
        }
        pub fn $set(&mut self, v: $t) {
            unsafe {
                blu_hip_set_param(self.h, $key, v as f64);
            }
        }
    };
}
macro_rules! stat {
    ($name:ident, $key:expr, $t:ty) => {
        pub fn $name(&self) -> $t {
            unsafe { blu_hip_get_stat(self.h, $key) as $t }
        }
    };
}

impl LU {
    // public parameter fields, lu.rs:11-66 (defaults lu.rs:249-259)
    param!(droptol, set_droptol, key::DROPTOL, f64);
    param!(abstol, set_abstol, key::ABSTOL, f64);
    param!(reltol, set_reltol, key::RELTOL, f64);
    param!(maxsearch, set_maxsearch, key::MAXSEARCH, usize);
    param!(pad, set_pad, key::PAD, usize);
    param!(stretch, set_stretch, key::STRETCH, f64);
    param!(compress_thres, set_compress_thres, key::COMPRESS_THRES, f64);
    param!(sparse_thres, set_sparse_thres, key::SPARSE_THRES, f64);
    param!(search_rows, set_search_rows, key::SEARCH_ROWS, usize);
    /// `nzbias: Option<usize>` (lu.rs:33-41): `None` is passed as -1.
    pub fn nzbias(&self) -> Option<usize> {
        let v = unsafe { blu_hip_get_param(self.h, key::NZBIAS) };
        if v < 0.0 { None } else { Some(v as usize) }
    }
    pub fn set_nzbias(&mut self, v: Option<usize>) {
        unsafe {
            blu_hip_set_param(self.h, key::NZBIAS, v.map(|x| x as f64).unwrap_or(-1.0));
        }
    }
    // getters, lu.rs:398-684
    stat!(m, key::M, usize);
    stat!(nfactorize, key::NFACTORIZE, usize);
    stat!(l_nz, key::L_NZ, usize);
    stat!(u_nz, key::U_NZ, usize);
    stat!(min_pivot, key::MIN_PIVOT, f64);
    stat!(max_pivot, key::MAX_PIVOT, f64);
    stat!(condest_l, key::CONDEST_L, f64);
    stat!(condest_u, key::CONDEST_U, f64);
    stat!(norm_l, key::NORM_L, f64);
    stat!(norm_u, key::NORM_U, f64);
    stat!(normest_l_inv, key::NORMEST_L_INV, f64);
    stat!(normest_u_inv, key::NORMEST_U_INV, f64);
    stat!(onenorm, key::ONENORM, f64);
    stat!(infnorm, key::INFNORM, f64);
    stat!(residual_test, key::RESIDUAL_TEST, f64);
    stat!(matrix_nz, key::MATRIX_NZ, usize);
    stat!(rank, key::RANK, usize);
    stat!(bump_size, key::BUMP_SIZE, usize);
    stat!(bump_nz, key::BUMP_NZ, usize);
    stat!(nsearch_pivot, key::NSEARCH_PIVOT, usize);
    stat!(nexpand, key::NEXPAND, usize);
    stat!(ngarbage, key::NGARBAGE, usize);
    stat!(factor_flops, key::FACTOR_FLOPS, usize);
    stat!(time_factorize, key::TIME_FACTORIZE, f64);
    stat!(nforrest, key::NFORREST, usize);
    stat!(pivot_error, key::PIVOT_ERROR, f64);
    /// `LU::update_cost()` (lu.rs:324-326).
    stat!(update_cost, key::UPDATE_COST, f64);
    /// `nupdate: Option<usize>` (lu.rs:91): `None` while there is no valid factorization.
    pub fn nupdate(&self) -> Option<usize> {
        let v = unsafe { blu_hip_get_stat(self.h, key::NUPDATE) };
        if v < 0.0 { None } else { Some(v as usize) }
    }
}

impl Drop for LU {
    fn drop(&mut self) {
        unsafe { blu_hip_free(self.h) }
    }
}

/// `struct BLU` (`src/blu.rs:9-20`).
pub struct BLU {
    /// `pub lu: LU` (`blu.rs:10`).
    pub lu: LU,
    m: usize,
    device: i32,
    /// Solution of the last `solve_sparse` / `solve_for_update` (dense, `m` entries; `blu.rs:12`).
    pub lhs: Vec<f64>,
    /// Its pattern in the reference's order (`blu.rs:14`).
    pub ilhs: Vec<LUInt>,
    /// Number of nonzeros in `lhs` (`blu.rs:16`).
    pub nzlhs: usize,
    /// Columns of the resident constraint matrix (`set_matrix`); `None` while none is set through this object.
    ncol: Option<usize>,
    /// Arrays are reallocated for max(realloc_factor, 1.0) times the required size (`blu.rs:18-20`, default 1.5).
    pub realloc_factor: f64,
}

// The reference's BLU is `Send` (plain owned data); a handle is used by one thread at a time here as well.
unsafe impl Send for BLU {}

impl BLU {
    /// `BLU::new(m, b_nz)` (`blu.rs:61-91`) on HIP device 0.  Panics if no gfx950 device is usable: there is
    /// no CPU fallback.
    pub fn new(m: usize, b_nz: usize) -> BLU {
        Self::new_on(m, b_nz, 0).expect("blu_hip_new failed: no gfx950 device, bad argument or out of memory")
    }

    pub fn new_on(m: usize, b_nz: usize, device: i32) -> Option<BLU> {
        let h = unsafe { blu_hip_new(m as i64, b_nz as i64, device) };
        if h.is_null() {
            return None;
        }
        Some(BLU { lu: LU { h }, m, device, lhs: vec![0.0; m], ilhs: vec![0; m], nzlhs: 0, ncol: None, realloc_factor: 1.5 })
    }

    /// A new object with the complete logical state of this one (`blu_hip_clone`: factors, update state, a pending
    /// `solve_for_update`, parameters and statistics), independent of it afterwards; `None` on any failure.  `lhs` / `ilhs` /
    /// `nzlhs` are not carried over.  (Not `Clone`: the copy is device work and can fail.)
    pub fn try_clone(&mut self) -> Option<BLU> {
        self.push_realloc_factor();
        let h = unsafe { blu_hip_clone(self.lu.h) };
        if h.is_null() {
            return None;
        }
        let m = self.m;
        Some(BLU { lu: LU { h }, m, device: self.device, lhs: vec![0.0; m], ilhs: vec![0; m], nzlhs: 0, ncol: None, realloc_factor: self.realloc_factor })
    }

    // the library grows its device storage itself (the loops of blu.rs:105-115, 277-283, 324-330): it gets the factor
    fn push_realloc_factor(&mut self) {
        unsafe {
            blu_hip_set_param(self.lu.h, key::REALLOC_FACTOR, self.realloc_factor);
        }
    }

    pub fn last_error(&self) -> String {
        unsafe { CStr::from_ptr(blu_hip_last_error(self.lu.h)).to_string_lossy().into_owned() }
    }

    /// `BLU::factorize` (`blu.rs:95-118`): column j of B is `b_i[b_begin[j]..b_end[j]]`, `b_x[..]`.
    pub fn factorize(&mut self, b_begin: &[usize], b_end: &[usize], b_i: &[usize], b_x: &[f64]) -> Result<(), Status> {
        if b_begin.len() < self.m || b_end.len() < self.m || b_i.len() != b_x.len() {
            return Err(Status::ErrorInvalidArgument);
        }
        self.push_realloc_factor();
        // usize == u64 on the targets this back end exists for (x86-64 Linux hosts of MI355X nodes)
        let code = unsafe {
            blu_hip_factorize(
                self.lu.h, b_begin.as_ptr() as *const u64, b_end.as_ptr() as *const u64, b_i.as_ptr() as *const u64, b_x.as_ptr(), b_i.len() as u64,
            )
        };
        status_of(code)
    }

    /// `BLU::get_factors` (`blu.rs:139-160`, `get_factors.rs:48-180`): any `None` skips that output.
    pub fn get_factors(
        &mut self,
        rowperm: Option<&mut [LUInt]>, colperm: Option<&mut [LUInt]>,
        l_colptr: Option<&mut [LUInt]>, l_rowidx: Option<&mut [LUInt]>, l_value: Option<&mut [f64]>,
        u_colptr: Option<&mut [LUInt]>, u_rowidx: Option<&mut [LUInt]>, u_value: Option<&mut [f64]>,
    ) -> Result<(), Status> {
        fn p<T>(o: Option<&mut [T]>) -> *mut T {
            o.map(|s| s.as_mut_ptr()).unwrap_or(std::ptr::null_mut())
        }
        let code = unsafe {
            blu_hip_get_factors(self.lu.h, p(rowperm), p(colperm), p(l_colptr), p(l_rowidx), p(l_value), p(u_colptr), p(u_rowidx), p(u_value))
        };
        status_of(code)
    }

    /// `BLU::solve_dense` (`blu.rs:182-184`).
    pub fn solve_dense(&mut self, rhs: &[f64], lhs: &mut [f64], trans: char) -> Result<(), Status> {
        if rhs.len() < self.m || lhs.len() < self.m {
            return Err(Status::ErrorInvalidArgument);
        }
        status_of(unsafe { blu_hip_solve_dense(self.lu.h, rhs.as_ptr(), lhs.as_mut_ptr(), trans as c_char) })
    }

    /// `solve_dense` for `nrhs` right-hand sides in one call (no reference counterpart): right-hand side `j` is
    /// `rhs[j * ldrhs..j * ldrhs + m]`, its solution goes to `lhs[j * ldlhs..j * ldlhs + m]`, each bit-identical to
    /// `solve_dense` on the same right-hand side; what lies between `m` and a leading dimension is left alone.
    pub fn solve_dense_multi(&mut self, nrhs: usize, rhs: &[f64], ldrhs: usize, lhs: &mut [f64], ldlhs: usize, trans: char) -> Result<(), Status> {
        if nrhs > 1 && (ldrhs < self.m || ldlhs < self.m) {
            return Err(Status::ErrorInvalidArgument);
        }
        if nrhs > 0 && (rhs.len() < (nrhs - 1) * ldrhs + self.m || lhs.len() < (nrhs - 1) * ldlhs + self.m) {
            return Err(Status::ErrorInvalidArgument);
        }
        status_of(unsafe {
            blu_hip_solve_dense_multi(self.lu.h, nrhs as i64, rhs.as_ptr(), ldrhs as i64, lhs.as_mut_ptr(), ldlhs as i64, trans as c_char, 0)
        })
    }

    /// `solve_sparse` for `rhs_ptr.len() - 1` sparse right-hand sides in one call (no reference counterpart): right-hand
    /// side `j` is `irhs[rhs_ptr[j]..rhs_ptr[j + 1]]` / `xrhs[..]` (compressed columns).  Returns per right-hand side its
    /// status, and the compressed solutions `(lhs_ptr, ilhs, xlhs)`: solution `j` is `ilhs[lhs_ptr[j]..lhs_ptr[j + 1]]` in
    /// the reference's pattern order with its values, each bit-identical to `solve_sparse` on the same right-hand side.
    /// `self.lhs` / `self.ilhs` / `self.nzlhs` are not touched.  A call refused as a whole, a device failure or an
    /// allocation failure is the outer `Err`.
    #[allow(clippy::type_complexity)]
    pub fn solve_sparse_multi(
        &mut self, rhs_ptr: &[usize], irhs: &[usize], xrhs: &[f64], trans: char,
    ) -> Result<(Vec<Result<(), Status>>, Vec<usize>, Vec<usize>, Vec<f64>), Status> {
        // the C side reads rhs_ptr[0..=nrhs] and irhs / xrhs[rhs_ptr[0]..rhs_ptr[nrhs]): never hand it offsets beyond the slices
        if rhs_ptr.is_empty() || rhs_ptr.windows(2).any(|w| w[1] < w[0]) {
            return Err(Status::ErrorInvalidArgument);
        }
        let nrhs = rhs_ptr.len() - 1;
        if rhs_ptr[nrhs] > irhs.len() || rhs_ptr[nrhs] > xrhs.len() {
            return Err(Status::ErrorInvalidArgument);
        }
        let ptr: Vec<i64> = rhs_ptr.iter().map(|&p| p as i64).collect();
        let mut lhs_ptr = vec![0i64; nrhs + 1];
        let mut status = vec![-99 as c_int; nrhs.max(1)];
        let code = unsafe {
            blu_hip_solve_sparse_multi(
                self.lu.h, nrhs as i64, ptr.as_ptr(), irhs.as_ptr() as *const u64, xrhs.as_ptr(), trans as c_char, lhs_ptr.as_mut_ptr(),
                status.as_mut_ptr(),
            )
        };
        // refused as a whole (no status written), or a failure of the call itself
        if code < 0 && (code == -9 || status[..nrhs].iter().all(|&s| s != code)) {
            return Err(status_of(code).unwrap_err());
        }
        let total = lhs_ptr[nrhs] as usize;
        let mut ilhs = vec![0i64; total];
        let mut xlhs = vec![0f64; total];
        if total > 0 {
            status_of(unsafe { blu_hip_get_sparse_multi(self.lu.h, ilhs.as_mut_ptr(), xlhs.as_mut_ptr()) })?;
        }
        Ok((
            status[..nrhs].iter().map(|&s| status_of(s)).collect(),
            lhs_ptr.iter().map(|&p| p as usize).collect(),
            ilhs.iter().map(|&i| i as usize).collect(),
            xlhs,
        ))
    }

    /// One pass of `maxvolume` (`src/maxvolume.rs:64-224`) inside the library: the decisions, results and statistics of
    /// `crate::maxvolume(self, ...)`, the loop over `factorize` / `solve_for_update` / `update`, with the candidate columns
    /// priced in chunks on the device.  `basis` (`m` entries) and `isbasic` (`ncol` entries) are updated in place;
    /// `p_nupdate` is written on every exit the C entry writes it on.
    #[allow(clippy::too_many_arguments)]
    pub fn maxvolume(
        &mut self, ncol: usize, a_p: &[usize], a_i: &[usize], a_x: &[f64], basis: &mut [LUInt], isbasic: &mut [LUInt], volumetol: f64,
        p_nupdate: Option<&mut LUInt>,
    ) -> Result<(), Status> {
        // the C side reads a_p[0..=ncol], a_i / a_x[a_p[0]..a_p[ncol]), basis[0..m) and isbasic[0..ncol): never hand it less
        if a_p.len() != ncol + 1 || basis.len() != self.m || isbasic.len() != ncol || a_p.windows(2).any(|w| w[1] < w[0]) {
            return Err(Status::ErrorInvalidArgument);
        }
        if a_p[ncol] > a_i.len() || a_p[ncol] > a_x.len() {
            return Err(Status::ErrorInvalidArgument);
        }
        let mut nupdate: i64 = 0;
        let wants = p_nupdate.is_some();
        let code = unsafe {
            blu_hip_maxvolume(
                self.lu.h, ncol as i64, a_p.as_ptr() as *const u64, a_i.as_ptr() as *const u64, a_x.as_ptr(), basis.as_mut_ptr(),
                isbasic.as_mut_ptr(), volumetol, if wants { &mut nupdate } else { std::ptr::null_mut() },
            )
        };
        if let Some(p) = p_nupdate {
            *p = nupdate;
        }
        status_of(code)
    }

    /// Makes the rectangular `A` (`ncol` compressed columns, every row index below `m`) resident on the device
    /// (`blu_hip_set_matrix`; no reference counterpart).  It stays until the next `set_matrix` or `maxvolume` call on this
    /// object and is what `factorize_columns`, `solve_for_update_column`, `tableau_row` and `price` work on.
    pub fn set_matrix(&mut self, ncol: usize, a_p: &[usize], a_i: &[usize], a_x: &[f64]) -> Result<(), Status> {
        // the C side reads a_p[0..=ncol] and a_i / a_x[a_p[0]..a_p[ncol]): never hand it less
        if a_p.len() != ncol + 1 || a_p.windows(2).any(|w| w[1] < w[0]) || a_p[ncol] > a_i.len() || a_p[ncol] > a_x.len() {
            return Err(Status::ErrorInvalidArgument);
        }
        status_of(unsafe { blu_hip_set_matrix(self.lu.h, ncol as i64, a_p.as_ptr() as *const u64, a_i.as_ptr() as *const u64, a_x.as_ptr()) })?;
        self.ncol = Some(ncol);
        Ok(())
    }

    /// `factorize` of `A[:, basis]` from the resident matrix with an `m`-sized upload: the status, factors and statistics
    /// of `factorize` given the gathered columns.
    pub fn factorize_columns(&mut self, basis: &[LUInt]) -> Result<(), Status> {
        if basis.len() != self.m {
            return Err(Status::ErrorInvalidArgument);
        }
        self.push_realloc_factor();
        status_of(unsafe { blu_hip_factorize_columns(self.lu.h, basis.as_ptr()) })
    }

    /// The forward `solve_for_update` of column `j` of the resident matrix, nothing uploaded; the solution is left in
    /// `self.lhs` / `self.ilhs[..self.nzlhs]` when `want_solution`.
    pub fn solve_for_update_column(&mut self, j: usize, want_solution: bool) -> Result<(), Status> {
        self.clear_lhs();
        let mut nz: i64 = 0;
        let code = unsafe {
            if want_solution {
                blu_hip_solve_for_update_column(self.lu.h, j as i64, &mut nz, self.ilhs.as_mut_ptr(), self.lhs.as_mut_ptr())
            } else {
                blu_hip_solve_for_update_column(self.lu.h, j as i64, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
            }
        };
        status_of(code)?;
        if want_solution {
            self.nzlhs = nz as usize;
        }
        Ok(())
    }

    /// Row `r` of `B^-1 A` for the resident matrix into `alpha[..ncol]`: the transposed solve of `e_r` -- `solve_sparse`, or
    /// with `prepare_update` the transposed `solve_for_update`, the leaving row of a dual simplex iteration -- and the
    /// products with every column on the device.  `skip[j] != 0` (a caller passes its `isbasic`) gives `alpha[j] = +0.0`.
    /// With `want_solution` the solution of the solve is left in `self.lhs` / `self.ilhs[..self.nzlhs]`.
    pub fn tableau_row(
        &mut self, r: usize, prepare_update: bool, skip: Option<&[LUInt]>, alpha: &mut [f64], want_solution: bool,
    ) -> Result<(), Status> {
        let ncol = self.ncol.ok_or(Status::ErrorInvalidCall)?;
        if alpha.len() < ncol || skip.map_or(false, |s| s.len() < ncol) {
            return Err(Status::ErrorInvalidArgument);
        }
        let sk = skip.map_or(std::ptr::null(), |s| s.as_ptr());
        let mut nz: i64 = 0;
        let code = unsafe {
            if want_solution {
                self.clear_lhs();
                blu_hip_tableau_row(
                    self.lu.h, r as i64, prepare_update as c_int, sk, alpha.as_mut_ptr(), &mut nz, self.ilhs.as_mut_ptr(), self.lhs.as_mut_ptr(),
                )
            } else {
                blu_hip_tableau_row(
                    self.lu.h, r as i64, prepare_update as c_int, sk, alpha.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(),
                    std::ptr::null_mut(),
                )
            }
        };
        status_of(code)?;
        if want_solution {
            self.nzlhs = nz as usize;
        }
        Ok(())
    }

    /// `z[j]` = column `j` of the resident matrix dotted with the dense `y[..m]`, in the summation order of `tableau_row`;
    /// needs no factorization.
    pub fn price(&mut self, y: &[f64], skip: Option<&[LUInt]>, z: &mut [f64]) -> Result<(), Status> {
        let ncol = self.ncol.ok_or(Status::ErrorInvalidCall)?;
        if y.len() < self.m || z.len() < ncol || skip.map_or(false, |s| s.len() < ncol) {
            return Err(Status::ErrorInvalidArgument);
        }
        status_of(unsafe { blu_hip_price(self.lu.h, y.as_ptr(), skip.map_or(std::ptr::null(), |s| s.as_ptr()), z.as_mut_ptr()) })
    }

    /// The last `price`, or the last `tableau_row` behind its solve: kernel launches, synchronizes, host-to-device
    /// copies, bytes downloaded.
    pub fn dbg_matrix_counts(&self) -> [i64; 4] {
        let mut out = [0i64; 4];
        unsafe { blu_hip_dbg_matrix_counts(self.lu.h, out.as_mut_ptr()) };
        out
    }

    /// Objects that hold this object's resident matrix, itself included (`share_matrix`); 0 when none is set.
    pub fn dbg_matrix_holders(&self) -> usize {
        unsafe { blu_hip_dbg_matrix_holders(self.lu.h) as usize }
    }

    // lu_clear_lhs, blu.rs:380-395
    fn clear_lhs(&mut self) {
        let nzsparse = (self.lu.sparse_thres() * self.m as f64) as usize;
        if self.nzlhs != 0 {
            if self.nzlhs <= nzsparse {
                for p in 0..self.nzlhs {
                    self.lhs[self.ilhs[p] as usize] = 0.0;
                }
            } else {
                self.lhs.iter_mut().for_each(|x| *x = 0.0);
            }
            self.nzlhs = 0;
        }
    }

    /// `BLU::solve_sparse` (`blu.rs:207-225`): the solution is left in `self.lhs` / `self.ilhs[..self.nzlhs]`.
    pub fn solve_sparse(&mut self, nzrhs: LUInt, irhs: &[usize], xrhs: &[f64], trans: char) -> Result<(), Status> {
        // the C side reads irhs[0..nzrhs) and xrhs[0..nzrhs): never hand it a count beyond the slices
        if nzrhs < 0 || nzrhs as usize > irhs.len() || nzrhs as usize > xrhs.len() {
            return Err(Status::ErrorInvalidArgument);
        }
        self.clear_lhs();
        let mut nz: i64 = 0;
        let code = unsafe {
            blu_hip_solve_sparse(
                self.lu.h, nzrhs, irhs.as_ptr() as *const u64, xrhs.as_ptr(), &mut nz, self.ilhs.as_mut_ptr(), self.lhs.as_mut_ptr(), trans as c_char,
            )
        };
        status_of(code)?;
        self.nzlhs = nz as usize;
        Ok(())
    }

    /// `BLU::solve_for_update` (`blu.rs:257-288`).  With `want_solution != 0` the solution is left in
    /// `self.lhs` / `self.ilhs[..self.nzlhs]`; otherwise only the update is prepared.
    pub fn solve_for_update(&mut self, nzrhs: usize, irhs: &[usize], xrhs: Option<&[f64]>, trans: char, want_solution: LUInt) -> Result<(), Status> {
        // the C side reads irhs[0..nzrhs) / xrhs[0..nzrhs), and irhs[0] for a transposed solve even when nzrhs == 0
        let transposed = trans == 't' || trans == 'T';
        if nzrhs > irhs.len() || xrhs.map_or(false, |x| nzrhs > x.len()) || (transposed && irhs.is_empty()) {
            return Err(Status::ErrorInvalidArgument);
        }
        self.clear_lhs();
        self.push_realloc_factor();
        let xp = xrhs.map(|x| x.as_ptr()).unwrap_or(std::ptr::null());
        let mut nz: i64 = 0;
        let code = unsafe {
            if want_solution != 0 {
                blu_hip_solve_for_update(
                    self.lu.h, nzrhs as i64, irhs.as_ptr() as *const u64, xp, &mut nz, self.ilhs.as_mut_ptr(), self.lhs.as_mut_ptr(), trans as c_char,
                )
            } else {
                blu_hip_solve_for_update(
                    self.lu.h, nzrhs as i64, irhs.as_ptr() as *const u64, xp, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(),
                    trans as c_char,
                )
            }
        };
        status_of(code)?;
        if want_solution != 0 {
            self.nzlhs = nz as usize;
        }
        Ok(())
    }

    /// `BLU::update` (`blu.rs:319-335`).
    pub fn update(&mut self, xtbl: f64) -> Result<(), Status> {
        self.push_realloc_factor();
        status_of(unsafe { blu_hip_update(self.lu.h, xtbl) })
    }
}

/// `BLU::solve_for_update` for many objects of one device in one call (batch extension, no reference counterpart):
/// member k gets what `blus[k].solve_for_update(irhs[k].len(), irhs[k], xrhs[k], trans, want_solution)` gives, its
/// solution left in `blus[k].lhs` / `ilhs[..nzlhs]`.  `Err` is a refusal of the whole call (the same object twice
/// cannot be expressed here; objects on two devices, or a forward call without `xrhs`); otherwise one result per member.
pub fn solve_for_update_batch(
    blus: &mut [&mut BLU], irhs: &[&[usize]], xrhs: Option<&[&[f64]]>, trans: char, want_solution: LUInt,
) -> Result<Vec<Result<(), Status>>, Status> {
    let n = blus.len();
    let transposed = trans == 't' || trans == 'T';
    if irhs.len() != n || xrhs.map_or(false, |x| x.len() != n) {
        return Err(Status::ErrorInvalidArgument);
    }
    for k in 0..n {
        if (transposed && irhs[k].is_empty()) || xrhs.map_or(false, |x| x[k].len() < irhs[k].len()) {
            return Err(Status::ErrorInvalidArgument);
        }
    }
    for b in blus.iter_mut() {
        b.clear_lhs();
        b.push_realloc_factor();
    }
    let mut hs: Vec<*mut BluHip> = blus.iter().map(|b| b.lu.h).collect();
    let nzrhs: Vec<i64> = irhs.iter().map(|x| x.len() as i64).collect();
    // (an empty column: any non-NULL pointer, nothing is read through it)
    let ip: Vec<*const u64> = irhs.iter().map(|x| if x.is_empty() { 8 as *const u64 } else { x.as_ptr() as *const u64 }).collect();
    let xp: Option<Vec<*const f64>> = xrhs.map(|xs| xs.iter().map(|x| if x.is_empty() { 8 as *const f64 } else { x.as_ptr() }).collect());
    let il: Vec<*mut i64> = blus.iter_mut().map(|b| b.ilhs.as_mut_ptr()).collect();
    let lp: Vec<*mut f64> = blus.iter_mut().map(|b| b.lhs.as_mut_ptr()).collect();
    let mut nz = vec![0i64; n];
    let mut st = vec![0 as c_int; n];
    let want = want_solution != 0;
    let code = unsafe {
        blu_hip_solve_for_update_batch(
            hs.as_mut_ptr(), n as c_int, nzrhs.as_ptr(), ip.as_ptr(), xp.as_ref().map_or(std::ptr::null(), |v| v.as_ptr()),
            if want { nz.as_mut_ptr() } else { std::ptr::null_mut() }, if want { il.as_ptr() } else { std::ptr::null() },
            if want { lp.as_ptr() } else { std::ptr::null() }, trans as c_char, st.as_mut_ptr(),
        )
    };
    // -3 is returned by a refusal alone; -4 is also a member's status (an index out of range): a refusal only for two devices
    if code == -3 || (code == -4 && blus.iter().any(|b| b.device != blus[0].device)) {
        return status_of(code).map(|_| Vec::new());
    }
    for k in 0..n {
        if st[k] == 0 && want {
            blus[k].nzlhs = nz[k] as usize;
        }
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

/// `BLU::update` for many objects of one device in one call: `xtbl[k]` for `blus[k]`; results as by
/// `solve_for_update_batch`.
pub fn update_batch(blus: &mut [&mut BLU], xtbl: &[f64]) -> Result<Vec<Result<(), Status>>, Status> {
    let n = blus.len();
    if xtbl.len() != n {
        return Err(Status::ErrorInvalidArgument);
    }
    for b in blus.iter_mut() {
        b.push_realloc_factor();
    }
    let mut hs: Vec<*mut BluHip> = blus.iter().map(|b| b.lu.h).collect();
    let mut st = vec![0 as c_int; n];
    let code = unsafe { blu_hip_update_batch(hs.as_mut_ptr(), n as c_int, xtbl.as_ptr(), st.as_mut_ptr()) };
    if code == -3 || (code == -4 && blus.iter().any(|b| b.device != blus[0].device)) {
        return status_of(code).map(|_| Vec::new());
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

/// `BLU::solve_sparse` for many objects of one device in one call (batch extension, no reference counterpart): member k
/// gets what `blus[k].solve_sparse(irhs[k].len(), irhs[k], xrhs[k], trans)` gives, its solution left in `blus[k].lhs` /
/// `ilhs[..nzlhs]`.  `Err` is a refusal of the whole call (the same object twice cannot be expressed here; objects on two
/// devices); otherwise one result per member.
pub fn solve_sparse_batch(blus: &mut [&mut BLU], irhs: &[&[usize]], xrhs: &[&[f64]], trans: char) -> Result<Vec<Result<(), Status>>, Status> {
    let n = blus.len();
    if irhs.len() != n || xrhs.len() != n {
        return Err(Status::ErrorInvalidArgument);
    }
    // the C side reads irhs[k][0..nzrhs[k]) and xrhs[k][0..nzrhs[k]): never hand it a count beyond the slices
    if (0..n).any(|k| xrhs[k].len() < irhs[k].len()) {
        return Err(Status::ErrorInvalidArgument);
    }
    for b in blus.iter_mut() {
        b.clear_lhs();
    }
    let mut hs: Vec<*mut BluHip> = blus.iter().map(|b| b.lu.h).collect();
    let nzrhs: Vec<i64> = irhs.iter().map(|x| x.len() as i64).collect();
    // (an empty right-hand side may pass NULL for both arrays, as the single call allows)
    let ip: Vec<*const u64> = irhs.iter().map(|x| if x.is_empty() { std::ptr::null() } else { x.as_ptr() as *const u64 }).collect();
    let xp: Vec<*const f64> = xrhs.iter().zip(irhs).map(|(x, i)| if i.is_empty() { std::ptr::null() } else { x.as_ptr() }).collect();
    let il: Vec<*mut i64> = blus.iter_mut().map(|b| b.ilhs.as_mut_ptr()).collect();
    let lp: Vec<*mut f64> = blus.iter_mut().map(|b| b.lhs.as_mut_ptr()).collect();
    let mut nz = vec![0i64; n];
    let mut st = vec![0 as c_int; n];
    let code = unsafe {
        blu_hip_solve_sparse_batch(
            hs.as_mut_ptr(), n as c_int, nzrhs.as_ptr(), ip.as_ptr(), xp.as_ptr(), nz.as_mut_ptr(), il.as_ptr(), lp.as_ptr(), trans as c_char,
            st.as_mut_ptr(),
        )
    };
    // -3 is returned by a refusal alone; -4 is also a member's status (an index out of range): a refusal only for two devices
    if code == -3 || (code == -4 && blus.iter().any(|b| b.device != blus[0].device)) {
        return status_of(code).map(|_| Vec::new());
    }
    for k in 0..n {
        if st[k] == 0 {
            blus[k].nzlhs = nz[k] as usize;
        }
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

/// The complete logical state of `src` copied into every object of `dsts` (same `m`, same device) in one launch (batch
/// extension, no reference counterpart): each is afterwards observably `src` and independent of it; its `lhs` / `ilhs` /
/// `nzlhs` are cleared.  `Err` is a refusal of the whole call (another `m`, another device; the source among the
/// destinations or a destination twice cannot be expressed here); otherwise one result per member.
pub fn copy_batch(src: &mut BLU, dsts: &mut [&mut BLU]) -> Result<Vec<Result<(), Status>>, Status> {
    let n = dsts.len();
    src.push_realloc_factor();
    let mut hs: Vec<*mut BluHip> = dsts.iter().map(|b| b.lu.h).collect();
    let mut st = vec![0 as c_int; n];
    let code = unsafe { blu_hip_copy_batch(src.lu.h, hs.as_mut_ptr(), n as c_int, st.as_mut_ptr()) };
    if code == -3 || code == -4 {
        return status_of(code).map(|_| Vec::new()); // (codes only a refusal returns)
    }
    for (k, b) in dsts.iter_mut().enumerate() {
        if st[k] == 0 {
            b.realloc_factor = src.realloc_factor;
            for x in b.lhs.iter_mut() {
                *x = 0.0;
            }
            b.nzlhs = 0;
        }
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

/// Every object of `dsts` (same `m`, same device) holds the resident matrix `src` holds afterwards (batch extension, no
/// reference counterpart): one copy of `A` on the device for all of them, no device copy and no launch.  A destination
/// that has a matrix lets go of it first; a holder leaves through `set_matrix`, `maxvolume` or by being dropped, and the
/// last one frees the matrix.  `Err` is a refusal of the whole call (`src` without a matrix, another `m`, another device);
/// otherwise one result per member.
pub fn share_matrix(src: &mut BLU, dsts: &mut [&mut BLU]) -> Result<Vec<Result<(), Status>>, Status> {
    let n = dsts.len();
    let mut hs: Vec<*mut BluHip> = dsts.iter().map(|b| b.lu.h).collect();
    let mut st = vec![0 as c_int; n];
    let code = unsafe { blu_hip_share_matrix(src.lu.h, hs.as_mut_ptr(), n as c_int, st.as_mut_ptr()) };
    if code == -3 || code == -4 || code == -2 {
        return status_of(code).map(|_| Vec::new()); // (codes only a refusal returns)
    }
    for (k, b) in dsts.iter_mut().enumerate() {
        if st[k] == 0 {
            b.ncol = src.ncol;
        }
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

/// `tableau_row(rows[k], prepare_update, skips[k], alphas[k])` for objects that hold one matrix (`share_matrix`) in one
/// call: per member the status, the bits of `alpha`, the solution (left in `lhs` / `ilhs[..nzlhs]` with `want_solution`)
/// and the statistics of the single call.  `Err` is a refusal of the whole call; otherwise one result per member.
pub fn tableau_row_batch(
    blus: &mut [&mut BLU], rows: &[usize], prepare_update: bool, skips: Option<&[Option<&[LUInt]>]>, alphas: &mut [&mut [f64]],
    want_solution: bool,
) -> Result<Vec<Result<(), Status>>, Status> {
    let n = blus.len();
    if rows.len() != n || alphas.len() != n || skips.map_or(false, |s| s.len() != n) {
        return Err(Status::ErrorInvalidArgument);
    }
    for k in 0..n {
        let ncol = blus[k].ncol.unwrap_or(0);
        if alphas[k].len() < ncol || skips.map_or(false, |s| s[k].map_or(false, |x| x.len() < ncol)) {
            return Err(Status::ErrorInvalidArgument);
        }
        if want_solution {
            blus[k].clear_lhs();
        }
    }
    let mut hs: Vec<*mut BluHip> = blus.iter().map(|b| b.lu.h).collect();
    let r: Vec<i64> = rows.iter().map(|&x| x as i64).collect();
    let sk: Vec<*const i64> = (0..n).map(|k| skips.and_then(|s| s[k]).map_or(std::ptr::null(), |x| x.as_ptr())).collect();
    let al: Vec<*mut f64> = alphas.iter_mut().map(|a| a.as_mut_ptr()).collect();
    let il: Vec<*mut i64> = blus.iter_mut().map(|b| b.ilhs.as_mut_ptr()).collect();
    let xl: Vec<*mut f64> = blus.iter_mut().map(|b| b.lhs.as_mut_ptr()).collect();
    let mut nz = vec![0i64; n];
    let mut st = vec![0 as c_int; n];
    let code = unsafe {
        if want_solution {
            blu_hip_tableau_row_batch(
                hs.as_mut_ptr(), n as c_int, r.as_ptr(), prepare_update as c_int, sk.as_ptr(), al.as_ptr(), nz.as_mut_ptr(), il.as_ptr(), xl.as_ptr(),
                st.as_mut_ptr(),
            )
        } else {
            blu_hip_tableau_row_batch(
                hs.as_mut_ptr(), n as c_int, r.as_ptr(), prepare_update as c_int, sk.as_ptr(), al.as_ptr(), std::ptr::null_mut(), std::ptr::null(),
                std::ptr::null(), st.as_mut_ptr(),
            )
        }
    };
    // -3 is returned by a refusal alone; -4 is also a member's status (a row out of range): when every member carries it the
    // call may have been refused (two devices, two matrices), and the members' results say the same
    if code == -3 {
        return status_of(code).map(|_| Vec::new());
    }
    for k in 0..n {
        if st[k] == 0 && want_solution {
            blus[k].nzlhs = nz[k] as usize;
        }
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

/// `price(ys[k], skips[k], zs[k])` for objects that hold one matrix in one call; needs no factorization.
pub fn price_batch(
    blus: &mut [&mut BLU], ys: &[&[f64]], skips: Option<&[Option<&[LUInt]>]>, zs: &mut [&mut [f64]],
) -> Result<Vec<Result<(), Status>>, Status> {
    let n = blus.len();
    if ys.len() != n || zs.len() != n || skips.map_or(false, |s| s.len() != n) {
        return Err(Status::ErrorInvalidArgument);
    }
    for k in 0..n {
        let ncol = blus[k].ncol.unwrap_or(0);
        if ys[k].len() < blus[k].m || zs[k].len() < ncol || skips.map_or(false, |s| s[k].map_or(false, |x| x.len() < ncol)) {
            return Err(Status::ErrorInvalidArgument);
        }
    }
    let mut hs: Vec<*mut BluHip> = blus.iter().map(|b| b.lu.h).collect();
    let py: Vec<*const f64> = ys.iter().map(|y| y.as_ptr()).collect();
    let sk: Vec<*const i64> = (0..n).map(|k| skips.and_then(|s| s[k]).map_or(std::ptr::null(), |x| x.as_ptr())).collect();
    let pz: Vec<*mut f64> = zs.iter_mut().map(|z| z.as_mut_ptr()).collect();
    let mut st = vec![0 as c_int; n];
    let code = unsafe { blu_hip_price_batch(hs.as_mut_ptr(), n as c_int, py.as_ptr(), sk.as_ptr(), pz.as_ptr(), st.as_mut_ptr()) };
    if code == -3 || code == -4 {
        return status_of(code).map(|_| Vec::new()); // (codes only a refusal returns)
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

/// `blu_ratio_result` (include/blu_hip.h): what the ratio test on the device downloads, 64 bytes.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct RatioResult {
    pub q: i64,
    pub ncand: i64,
    pub alpha_q: f64,
    pub d_q: f64,
    pub step: f64,
    pub bound: f64,
    pub reserved: [i64; 2],
}

impl BLU {
    /// Upload the reduced costs and / or the bound status (0 no candidate, 1 at lower, -1 at upper, 2 free) of the columns
    /// of the resident matrix; `None` keeps the previous content, the first call needs both.
    pub fn set_duals(&mut self, d: Option<&[f64]>, kind: Option<&[i8]>) -> Result<(), Status> {
        let ncol = self.ncol.unwrap_or(0);
        if d.map_or(false, |x| x.len() < ncol) || kind.map_or(false, |x| x.len() < ncol) {
            return Err(Status::ErrorInvalidArgument);
        }
        status_of(unsafe { blu_hip_set_duals(self.lu.h, d.map_or(std::ptr::null(), |x| x.as_ptr()), kind.map_or(std::ptr::null(), |x| x.as_ptr())) })
    }

    pub fn get_duals(&mut self, d: &mut [f64], kind: &mut [i8]) -> Result<(), Status> {
        let ncol = self.ncol.unwrap_or(0);
        if d.len() < ncol || kind.len() < ncol {
            return Err(Status::ErrorInvalidArgument);
        }
        status_of(unsafe { blu_hip_get_duals(self.lu.h, d.as_mut_ptr(), kind.as_mut_ptr()) })
    }

    /// The row the last successful ratio test kept, +0.0 where kind was 0.
    pub fn ratio_row(&mut self, alpha: &mut [f64]) -> Result<(), Status> {
        if alpha.len() < self.ncol.unwrap_or(0) {
            return Err(Status::ErrorInvalidArgument);
        }
        status_of(unsafe { blu_hip_get_ratio_row(self.lu.h, alpha.as_mut_ptr()) })
    }

    /// The dual ratio test on row `r` of B^-1 A, on the device; the solution of the transposed solve is not downloaded.
    pub fn ratio_test(&mut self, r: usize, prepare_update: bool, sigma: f64, pivtol: f64, dualtol: f64) -> Result<RatioResult, Status> {
        let mut out = RatioResult::default();
        status_of(unsafe {
            blu_hip_ratio_test(
                self.lu.h, r as i64, prepare_update as c_int, sigma, pivtol, dualtol, &mut out, std::ptr::null_mut(), std::ptr::null_mut(),
                std::ptr::null_mut(),
            )
        })
        .map(|_| out)
    }

    /// d[j] -= theta * row[j] where kind[j] != 0 (row: the kept row), then d[jset[t]] = dset[t], kind[jset[t]] = kset[t].
    pub fn update_duals(&mut self, theta: f64, jset: &[i64], dset: &[f64], kset: &[i8]) -> Result<(), Status> {
        if dset.len() != jset.len() || kset.len() != jset.len() {
            return Err(Status::ErrorInvalidArgument);
        }
        status_of(unsafe { blu_hip_update_duals(self.lu.h, theta, jset.len() as i64, jset.as_ptr(), dset.as_ptr(), kset.as_ptr()) })
    }
}

/// d and kind of `src` into every object of `dsts` that holds its matrix, device to device in one launch.
pub fn copy_duals_batch(src: &mut BLU, dsts: &mut [&mut BLU]) -> Result<Vec<Result<(), Status>>, Status> {
    let mut hs: Vec<*mut BluHip> = dsts.iter().map(|b| b.lu.h).collect();
    let mut st = vec![0 as c_int; hs.len()];
    let code = unsafe { blu_hip_copy_duals_batch(src.lu.h, hs.as_mut_ptr(), hs.len() as c_int, st.as_mut_ptr()) };
    if code == -3 || code == -4 {
        return status_of(code).map(|_| Vec::new()); // (codes only a refusal returns)
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

/// `ratio_test(rows[k], prepare_update, sigmas[k], pivtol, dualtol)` for objects that hold one matrix in one call.
pub fn ratio_test_batch(
    blus: &mut [&mut BLU], rows: &[usize], prepare_update: bool, sigmas: &[f64], pivtol: f64, dualtol: f64,
) -> Result<Vec<Result<RatioResult, Status>>, Status> {
    let n = blus.len();
    if rows.len() != n || sigmas.len() != n {
        return Err(Status::ErrorInvalidArgument);
    }
    let mut hs: Vec<*mut BluHip> = blus.iter().map(|b| b.lu.h).collect();
    let r: Vec<i64> = rows.iter().map(|&x| x as i64).collect();
    let mut out = vec![RatioResult::default(); n];
    let mut st = vec![0 as c_int; n];
    let code = unsafe {
        blu_hip_ratio_test_batch(
            hs.as_mut_ptr(), n as c_int, r.as_ptr(), prepare_update as c_int, sigmas.as_ptr(), pivtol, dualtol, out.as_mut_ptr(),
            std::ptr::null_mut(), std::ptr::null(), std::ptr::null(), st.as_mut_ptr(),
        )
    };
    if code == -3 {
        return status_of(code).map(|_| Vec::new());
    }
    Ok((0..n).map(|k| status_of(st[k]).map(|_| out[k])).collect())
}

/// `update_duals(thetas[k], sets[k])` per member in one call; `sets[k]` is (jset, dset, kset).
pub fn update_duals_batch(blus: &mut [&mut BLU], thetas: &[f64], sets: &[(&[i64], &[f64], &[i8])]) -> Result<Vec<Result<(), Status>>, Status> {
    let n = blus.len();
    if thetas.len() != n || sets.len() != n || sets.iter().any(|s| s.1.len() != s.0.len() || s.2.len() != s.0.len()) {
        return Err(Status::ErrorInvalidArgument);
    }
    let mut hs: Vec<*mut BluHip> = blus.iter().map(|b| b.lu.h).collect();
    let ns: Vec<i64> = sets.iter().map(|s| s.0.len() as i64).collect();
    let pj: Vec<*const i64> = sets.iter().map(|s| s.0.as_ptr()).collect();
    let pd: Vec<*const f64> = sets.iter().map(|s| s.1.as_ptr()).collect();
    let pk: Vec<*const i8> = sets.iter().map(|s| s.2.as_ptr()).collect();
    let mut st = vec![0 as c_int; n];
    let code = unsafe {
        blu_hip_update_duals_batch(hs.as_mut_ptr(), n as c_int, thetas.as_ptr(), ns.as_ptr(), pj.as_ptr(), pd.as_ptr(), pk.as_ptr(), st.as_mut_ptr())
    };
    if code == -3 {
        return status_of(code).map(|_| Vec::new());
    }
    Ok(st.iter().map(|&s| status_of(s)).collect())
}

#[cfg(test)]
mod tests {
    use super::*;

    // examples/simple.rs:20-33 of the reference: x_i = 0.1 (i + 1).  Needs an MI355X.
    #[test]
    fn simple_rs() {
        let arow: Vec<usize> = vec![0, 7, 8, 1, 4, 9, 2, 9, 3, 6, 7, 8, 9, 1, 4, 5, 3, 6, 9, 0, 3, 7, 8, 0, 3, 7, 8, 1, 2, 3, 6, 9];
        let acolst: Vec<usize> = vec![0, 3, 6, 8, 13, 15, 16, 19, 23, 27, 32];
        let a = vec![
            2.1, 0.14, 0.09, 1.1, 0.06, 0.03, 1.7, 0.04, 1.0, 0.32, 0.19, 0.32, 0.44, 0.06, 1.6, 2.2, 0.32, 1.9, 0.43, 0.14, 0.19, 1.1, 0.22, 0.09,
            0.32, 0.22, 2.4, 0.03, 0.04, 0.44, 0.43, 3.2,
        ];
        let b = vec![0.403, 0.28, 0.55, 1.504, 0.812, 1.32, 1.888, 1.168, 2.473, 3.695];
        let mut blu = BLU::new(10, 32);
        blu.factorize(&acolst[..10], &acolst[1..], &arow, &a).unwrap();
        let mut x = vec![0.0; 10];
        blu.solve_dense(&b, &mut x, 'N').unwrap();
        for (i, xi) in x.iter().enumerate() {
            assert!((xi - 0.1 * (i as f64 + 1.0)).abs() < 1e-13);
        }
    }
}
