//! Raw bindings of `include/totsu_f32hip.h` (what `bindgen` emits).  AUTHORED, NOT COMPILED.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct thip_param { pub max_iter: i64, pub eps_acc: f32, pub eps_inf: f32, pub eps_zero: f32, pub log_period: i64,
                         pub state_arith: i32, pub reserved: i32 }
pub const THIP_STATE_COMPENSATED: i32 = 0;
pub const THIP_STATE_PLAIN: i32 = 1;

#[repr(C)]
pub struct thip_problem {
    pub n: usize, pub m: usize,
    pub mat_a: *const f32, pub vec_b: *const f32, pub vec_c: *const f32, pub vec_b_rowabs: *const f32,
    pub n_seg: usize, pub host_seg_type: *const i32, pub host_seg_len: *const i64,
}

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_status {
    pub state: i32, pub iter: i64, pub kind: i32, pub cri: [f32; 3],
    pub tau: f32, pub kappa: f32, pub norm_b: f32, pub norm_c: f32,
}

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_batch_info_t {
    pub n_inst: i32, pub max_group: i32, pub groups: i32, pub passes_per_iteration: i32, pub a_copies: i32, pub reserved: i32,
    pub a_bytes: usize, pub bytes_per_pass: usize, pub arena_bytes: usize, pub device_bytes: usize,
    pub plan_nj: [i32; 4], pub plan_blocks: [i32; 4], pub plan_ms: [f32; 4],
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_batch_counters_t {
    pub launches: [i64; 4], pub passes: i64, pub instance_iterations: i64, pub replaced: i64,
    pub live: i32, pub groups_now: i32,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_smallbatch_info_t {
    pub n_prob: i32, pub threads: i32, pub lds_bytes: i32, pub live: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_midbatch_info_t {
    pub n_prob: i32, pub threads: i32, pub lds_bytes: i32, pub live: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
    pub load_bytes: i32, pub reserved: i32,
    pub a_bytes_per_iter: usize,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_mid16batch_info_t {
    pub n_prob: i32, pub threads: i32, pub lds_bytes: i32, pub live: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
    pub load_bytes: i32, pub a_dtype: i32,
    pub a_bytes_per_iter: usize,
    pub a_store_bytes: usize,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_sdpbatch_info_t {
    pub n_prob: i32, pub threads: i32, pub lds_bytes: i32, pub live: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
    pub load_bytes: i32, pub reserved: i32,
    pub a_bytes_per_iter: usize,
    pub max_psd_order: i32, pub n_psd: i32,
    pub psd_lds_bytes: usize,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_widebatch_info_t {
    pub n_prob: i32, pub threads: i32, pub lds_bytes: i32, pub live: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
    pub load_bytes: i32, pub reserved: i32,
    pub a_bytes_per_iter: usize,
    pub max_psd_order: i32, pub n_psd: i32,
    pub psd_lds_bytes: usize,
    pub lds_bytes_per_problem: usize, pub arena_bytes_per_problem: usize,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_wide16batch_info_t {
    pub n_prob: i32, pub threads: i32, pub lds_bytes: i32, pub live: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
    pub load_bytes: i32, pub a_dtype: i32,
    pub a_bytes_per_iter: usize,
    pub max_psd_order: i32, pub n_psd: i32,
    pub psd_lds_bytes: usize,
    pub lds_bytes_per_problem: usize, pub arena_bytes_per_problem: usize,
    pub a_store_bytes: usize,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_sparsebatch_info_t {
    pub n_prob: i32, pub threads: i32, pub lds_bytes: i32, pub live: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
    pub a_bytes_per_iter: usize,
    pub max_psd_order: i32, pub n_psd: i32,
    pub psd_lds_bytes: usize,
    pub nnz_cap: usize, pub nnz_total: usize, pub blob_bytes: usize,
    pub resident: i32, pub reserved: i32,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_raggedsparse_class_t {
    pub n_prob: i32, pub live: i32, pub threads: i32, pub lds_bytes: i32,
    pub launches: i64, pub workgroups: i64,
    pub n_resident: i32, pub reserved: i32,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_raggedsparse_info_t {
    pub n_prob: i32, pub live: i32, pub n_layouts: i32, pub n_resident: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
    pub a_bytes_per_iter: usize,
    pub max_psd_order: i32, pub n_psd: i32,
    pub psd_lds_bytes: usize,
    pub nnz_total: usize, pub blob_bytes: usize,
    pub cls: [thip_raggedsparse_class_t; 2],
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_raggedbatch_class_t {
    pub n_prob: i32, pub live: i32, pub threads: i32, pub lds_bytes: i32,
    pub launches: i64, pub workgroups: i64,
}
#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct thip_raggedbatch_info_t {
    pub n_prob: i32, pub live: i32, pub n_layouts: i32, pub n_load16: i32,
    pub arena_bytes: usize, pub device_bytes: usize, pub device_bytes_all: usize,
    pub launches: i64, pub workgroups: i64,
    pub a_bytes_per_iter: usize,
    pub cls: [thip_raggedbatch_class_t; 2],
}
pub const THIP_BATCH_MAX: c_int = 64;
pub const THIP_BATCH_GROUP_DEFAULT: c_int = 8;

#[repr(C)]
pub struct thip_sweep_test {
    pub m: usize, pub n: usize, pub lda: usize,
    pub mat_a: *const f32, pub v: *const f32, pub xy: *const f32, pub c: *const f32, pub su: *const f32, pub tx: *const f32,
    pub u: *mut f32, pub ku: *mut f32,
    pub xx_in: *const f32, pub kx_in: *const f32,
    pub xx_out: *mut f32, pub kx_out: *mut f32, pub gp: *mut f32, pub hn: *mut f32, pub h3: *mut f32,
    pub kappa: f32, pub rtau: f32, pub first: i32, pub reps: i32,
    pub force_members: i32, pub pub_agent: i32, pub variant: i32, pub elem: i32,
    pub inv_s: *const f32,
    pub host_sums: *mut f32,
    pub pin_w: i32, pub pin_g: i32,
}

#[repr(C)]
pub struct thip_sweep_plan_rec {
    pub members: i32, pub ngroups: i32, pub rows_per_member: i32, pub cols_per_group: i32, pub npan: i32, pub nslot: i32,
    pub cols_per_panel: i32, pub elem: i32,
    pub mpad: usize, pub gran_words: usize,
}

#[repr(C)]
pub struct thip_gemv_plan_rec {
    pub vw: i32, pub nj: i32, pub ku: i32, pub tiles: i32, pub chunks: i32, pub cols_per_chunk: i32, pub m_load: i32,
    pub chunks2: i32, pub cols_per_chunk2: i32, pub reserved: i32,
}
pub const THIP_TEST_E_GUARD: c_int = 10901;

#[repr(C)]
pub struct thip_gemv_test {
    pub m: usize, pub n: usize, pub lda: usize,
    pub mat: *const c_void,
    pub inv_scale: *const f32,
    pub kind: i32, pub pad_zero: i32,
    pub xn: *const f32, pub xt: *const f32,
    pub out_n: *mut f32, pub out_t: *mut f32,
    pub do_n: i32, pub do_t: i32, pub abs_mode: i32, pub nj: i32, pub target_blocks: i32, pub stopped: i32,
    pub col_split: usize,
}

#[repr(C)]
pub struct thip_gemv_multi_test {
    pub m: usize, pub n: usize,
    pub mat: *const f32,
    pub nv: i32, pub nj: i32, pub target_blocks: i32, pub reserved: i32,
    pub xn: *const *const f32, pub xt: *const *const f32,
    pub out_n: *const *mut f32, pub out_t: *const *mut f32,
    pub stopped: *const i32,
}

pub enum thip_solver {}
pub enum thip_batch {}
pub enum thip_smallbatch {}
pub enum thip_midbatch {}
pub enum thip_mid16batch {}
pub enum thip_sdpbatch {}
pub enum thip_widebatch {}
pub enum thip_wide16batch {}
pub enum thip_raggedbatch {}
pub enum thip_sparsebatch {}
pub enum thip_raggedsparse {}
pub enum thip_sptile {}
pub enum thip_sptile_builder {}
pub type thip_allreduce_fn = Option<unsafe extern "C" fn(ctx: *mut c_void, dev_buf: *mut f32, n: usize, stream: *mut c_void) -> c_int>;

pub const THIP_CONE_ZERO: i32 = 0;
pub const THIP_CONE_RPOS: i32 = 1;
pub const THIP_CONE_SOC: i32 = 2;
pub const THIP_CONE_ROTSOC: i32 = 3;
pub const THIP_CONE_PSD: i32 = 4;
pub const THIP_SCHED_REFERENCE: c_int = 0;
pub const THIP_SCHED_FUSED: c_int = 1;
pub const THIP_SCHED_CARRIED: c_int = 2;
pub const THIP_SCHED_SWEEP: c_int = 3;
pub const THIP_OVERLAP_OFF: c_int = 0;
pub const THIP_OVERLAP_LOCAL_ROWS: c_int = 1;
pub const THIP_OVERLAP_COLUMN_PIPELINE: c_int = 2;
pub const THIP_OVERLAP_COLUMN_INORDER: c_int = 3;

extern "C" {
    pub fn thip_init(device: c_int) -> c_int;
    pub fn thip_shutdown() -> c_int;
    pub fn thip_sync() -> c_int;
    pub fn thip_last_error() -> *const c_char;
    pub fn thip_alloc(n: usize, out: *mut *mut f32) -> c_int;
    pub fn thip_free(p: *mut f32) -> c_int;
    pub fn thip_h2d(dst: *mut f32, host_src: *const f32, n: usize) -> c_int;
    pub fn thip_d2h(host_dst: *mut f32, src: *const f32, n: usize) -> c_int;
    pub fn thip_get(x: *const f32, idx: usize, host_out: *mut f32) -> c_int;
    pub fn thip_set(x: *mut f32, idx: usize, val: f32) -> c_int;

    pub fn thip_norm(n: usize, x: *const f32, host_out: *mut f32) -> c_int;
    pub fn thip_copy(n: usize, x: *const f32, y: *mut f32) -> c_int;
    pub fn thip_scale(n: usize, alpha: f32, x: *mut f32) -> c_int;
    pub fn thip_add(n: usize, alpha: f32, x: *const f32, y: *mut f32) -> c_int;
    pub fn thip_adds(n: usize, s: f32, y: *mut f32) -> c_int;
    pub fn thip_abssum(len: usize, x: *const f32, incx: usize, host_out: *mut f32) -> c_int;
    pub fn thip_transform_di(n: usize, alpha: f32, d: *const f32, x: *const f32, beta: f32, y: *mut f32) -> c_int;

    pub fn thip_transform_ge(transpose: c_int, n_row: usize, n_col: usize, alpha: f32, mat: *const f32,
                             x: *const f32, beta: f32, y: *mut f32) -> c_int;
    pub fn thip_transform_sp(n: usize, alpha: f32, mat: *const f32, x: *const f32, beta: f32, y: *mut f32) -> c_int;
    pub fn thip_map_eig_worklen(n: usize) -> usize;
    pub fn thip_map_eig(n: usize, mat: *mut f32, has_scale: c_int, scale_diag: f32, eps_zero: f32,
                        work: *mut f32, worklen: usize, map_kind: c_int) -> c_int;
    pub fn thip_eig_decompose(n: usize, mat: *mut f32, has_scale: c_int, scale_diag: f32, eps_zero: f32,
                              work: *mut f32, worklen: usize, host_w: *mut f32) -> c_int;
    pub fn thip_eig_rebuild(n: usize, mat: *mut f32, has_scale: c_int, scale_diag: f32, work: *mut f32,
                            worklen: usize, host_e: *const f32, host_keep: *const u8) -> c_int;
    pub fn thip_eig_engine_info(host_engine: *mut c_int, host_polish: *mut c_int, host_cert: *mut f32) -> c_int;

    pub fn thip_absadd_cols(n_row: usize, n_col: usize, mat: *const f32, tau: *mut f32) -> c_int;
    pub fn thip_absadd_rows(n_row: usize, n_col: usize, mat: *const f32, sigma: *mut f32) -> c_int;
    pub fn thip_recip_max(n: usize, eps_zero: f32, x: *mut f32) -> c_int;
    pub fn thip_copy_block(transposed: c_int, n_row: usize, n_col: usize, sign: f32, src: *const f32, dst: *mut f32,
                           ld_dst: usize) -> c_int;
    pub fn thip_set_lazy_gemv(on: c_int) -> c_int;
    pub fn thip_get_lazy_gemv(host_on: *mut c_int) -> c_int;
    pub fn thip_lazy_gemv_stats(host_deferred: *mut i64, host_flushes: *mut i64) -> c_int;
    pub fn thip_lazy_plan_stats(host_hits: *mut i64, host_misses: *mut i64) -> c_int;
    pub fn thip_lazy_read_stats(host_served: *mut i64, host_fetches: *mut i64) -> c_int;
    pub fn thip_proj_zero(dual_cone: c_int, n: usize, x: *mut f32) -> c_int;
    pub fn thip_proj_rpos(n: usize, x: *mut f32) -> c_int;
    pub fn thip_proj_soc(n: usize, x: *mut f32) -> c_int;
    pub fn thip_proj_rotsoc(n: usize, x: *mut f32) -> c_int;
    pub fn thip_proj_psd(sn: usize, x: *mut f32, eps_zero: f32, work: *mut f32, worklen: usize) -> c_int;

    pub fn thip_solver_create(prob: *const thip_problem, par: *const thip_param, schedule: c_int,
                              out: *mut *mut thip_solver) -> c_int;
    pub fn thip_solver_set_allreduce(s: *mut thip_solver, f: thip_allreduce_fn, ctx: *mut c_void) -> c_int;
    pub fn thip_solver_set_overlap(s: *mut thip_solver, mode: c_int) -> c_int;
    pub fn thip_solver_overlap_info(s: *mut thip_solver, host_mode: *mut c_int, host_launches_per_pass: *mut c_int,
                                    host_split_col: *mut usize) -> c_int;
    pub fn thip_solver_init(s: *mut thip_solver) -> c_int;
    pub fn thip_solver_run(s: *mut thip_solver, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_solver_solution(s: *mut thip_solver, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_solver_destroy(s: *mut thip_solver) -> c_int;

    // ---- the rest of include/totsu_f32hip.h: context, device-scalar reductions, batched cones, sparse and
    // ---- reduced-precision operators, solver controls, RCCL communicator, generators, profiling ----
    pub fn thip_version() -> *const c_char;
    pub fn thip_device_count(host_count: *mut c_int) -> c_int;
    pub fn thip_set_stream(hip_stream: *mut c_void) -> c_int;
    pub fn thip_get_stream() -> *mut c_void;
    pub fn thip_alloc_zeroed(n: usize, out: *mut *mut f32) -> c_int;

    pub fn thip_norm_dev(n: usize, x: *const f32, dev_out: *mut f32) -> c_int;
    pub fn thip_dot_dev(n: usize, x: *const f32, y: *const f32, dev_out: *mut f32) -> c_int;
    pub fn thip_abssum_dev(len: usize, x: *const f32, incx: usize, dev_out: *mut f32) -> c_int;
    pub fn thip_absadd_sympack(n: usize, mat: *const f32, y: *mut f32) -> c_int;
    pub fn thip_spmv_csr(n_row: usize, n_col: usize, nnz: usize, dev_rowptr: *const i64, dev_colidx: *const i32,
                         vals: *const f32, alpha: f32, x: *const f32, beta: f32, y: *mut f32, abs_mode: c_int) -> c_int;
    pub fn thip_sptile_create(n_row: usize, n_col: usize, nnz: usize, host_colptr: *const i64, host_rowidx: *const i32,
                              host_vals: *const f32, out: *mut *mut thip_sptile) -> c_int;
    pub fn thip_sptile_destroy(mat: *mut thip_sptile) -> c_int;
    pub fn thip_sptile_mv(mat: *mut thip_sptile, transpose: c_int, alpha: f32, x: *const f32, beta: f32, y: *mut f32,
                          abs_mode: c_int) -> c_int;
    pub fn thip_sptile_info(mat: *const thip_sptile, host_nnz_stored: *mut usize, host_tiles: *mut c_int,
                            host_items_n: *mut c_int, host_items_t: *mut c_int, host_slices_n: *mut c_int,
                            host_slices_t: *mut c_int, host_bytes: *mut usize) -> c_int;
    pub fn thip_sptile_layout(mat: *const thip_sptile, host_dense_tiles: *mut c_int, host_indexed_entries: *mut usize,
                              host_bytes_per_product: *mut usize) -> c_int;
    pub fn thip_sptile_builder_create(n_row: usize, n_col: usize, out: *mut *mut thip_sptile_builder) -> c_int;
    pub fn thip_sptile_builder_count(b: *mut thip_sptile_builder, c0: usize, ncols: usize, dev_panel: *const f32,
                                     ld: usize) -> c_int;
    pub fn thip_sptile_builder_plan(b: *mut thip_sptile_builder, host_nnz: *mut usize, host_dense_tiles: *mut c_int,
                                    host_indexed_entries: *mut usize, host_bytes_per_product: *mut usize) -> c_int;
    pub fn thip_sptile_builder_fill(b: *mut thip_sptile_builder, c0: usize, ncols: usize, dev_panel: *const f32,
                                    ld: usize) -> c_int;
    pub fn thip_sptile_builder_finish(b: *mut thip_sptile_builder, out: *mut *mut thip_sptile) -> c_int;
    pub fn thip_sptile_builder_destroy(b: *mut thip_sptile_builder) -> c_int;
    pub fn thip_sptile_from_dense(n_row: usize, n_col: usize, dev_mat: *const f32, ld: usize,
                                  out: *mut *mut thip_sptile) -> c_int;
    pub fn thip_to_bf16(n_row: usize, n_col: usize, mat: *const f32, mat16: *mut u16, ld16: usize) -> c_int;
    pub fn thip_transform_ge_bf16(transpose: c_int, n_row: usize, n_col: usize, alpha: f32, mat16: *const u16,
                                  ld16: usize, x: *const f32, beta: f32, y: *mut f32) -> c_int;

    pub fn thip_proj_soc_batched(x: *mut f32, dev_offs: *const i64, n_cones: usize, rotated: c_int, max_len: usize) -> c_int;
    pub fn thip_group_min_batched(dp_tau: *mut f32, dev_offs: *const i64, n_groups: usize, max_len: usize) -> c_int;

    pub fn thip_solver_set_csr(s: *mut thip_solver, nnz: usize, dev_rowptr: *const i64, dev_colidx: *const i32,
                               dev_vals: *const f32, dev_t_rowptr: *const i64, dev_t_colidx: *const i32,
                               dev_t_vals: *const f32) -> c_int;
    pub fn thip_solver_set_sptile(s: *mut thip_solver, mat: *mut thip_sptile) -> c_int;
    pub fn thip_solver_set_a_storage(s: *mut thip_solver, a_kind: c_int) -> c_int;
    pub fn thip_solver_set_a_bf16(s: *mut thip_solver, mat16: *const u16, ld16: usize) -> c_int;
    pub fn thip_solver_set_a_f16(s: *mut thip_solver, mat16: *const u16, ld16: usize, inv_scale: *const f32) -> c_int;
    pub fn thip_to_f16(n_row: usize, n_col: usize, mat: *const f32, mat16: *mut u16, ld16: usize, inv_scale: *mut f32) -> c_int;
    pub fn thip_transform_ge_f16(transpose: c_int, n_row: usize, n_col: usize, alpha: f32, mat16: *const u16, ld16: usize,
                                 inv_scale: *const f32, x: *const f32, beta: f32, y: *mut f32) -> c_int;
    pub fn thip_solver_set_param(s: *mut thip_solver, par: *const thip_param) -> c_int;
    pub fn thip_solver_resume(s: *mut thip_solver) -> c_int;
    pub fn thip_solver_status(s: *mut thip_solver, host_status: *mut thip_status) -> c_int;
    pub fn thip_solver_iterate(s: *mut thip_solver, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_solver_set_iterate(s: *mut thip_solver, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_solver_precond(s: *mut thip_solver, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_solver_passes(s: *const thip_solver, host_passes: *mut c_int, host_bytes_per_pass: *mut usize) -> c_int;
    pub fn thip_solver_schedule_in_use(s: *mut thip_solver, host_schedule: *mut c_int) -> c_int;
    pub fn thip_solver_set_sweep_min_bytes(s: *mut thip_solver, bytes: usize) -> c_int;
    pub fn thip_solver_set_column_shard(s: *mut thip_solver, on: c_int) -> c_int;
    pub fn thip_sweep_probe(m: usize, n_local: usize, lda: usize, elem: c_int, host_ok: *mut c_int) -> c_int;
    pub fn thip_solver_sweep_plan(s: *mut thip_solver, host_members: *mut c_int, host_cols_per_panel: *mut c_int, host_slots: *mut c_int, host_ms: *mut f32) -> c_int;
    pub fn thip_stream_probe(dev_ptr: *const c_void, bytes: usize, reps: c_int, host_best_ms: *mut f32, host_avg_ms: *mut f32) -> c_int;
    pub fn thip_solver_sweep_faults(s: *mut thip_solver, host_faults: *mut c_int, host_last_word: *mut c_int, host_restored_iter: *mut i64) -> c_int;
    pub fn thip_solver_set_sweep_publish(s: *mut thip_solver, agent_scope: c_int) -> c_int;
    pub fn thip_sweep_publish_selftest(mode: c_int, host_agent_scope: *mut c_int, host_info: *mut c_int) -> c_int;
    pub fn thip_solver_gemv_plan(s: *const thip_solver, host_nj: *mut c_int, host_blocks: *mut c_int, host_ms: *mut f32) -> c_int;

    pub fn thip_batch_create(prob_template: *const thip_problem, n_inst: c_int, host_vec_b: *const *const f32,
                             host_vec_c: *const *const f32, par: *const thip_param, out: *mut *mut thip_batch) -> c_int;
    pub fn thip_batch_set_a_storage(b: *mut thip_batch, a_kind: c_int) -> c_int;
    pub fn thip_batch_set_gemv_autotune(b: *mut thip_batch, on: c_int) -> c_int;
    pub fn thip_batch_set_max_group(b: *mut thip_batch, max_group: c_int) -> c_int;
    pub fn thip_batch_set_param(b: *mut thip_batch, par: *const thip_param) -> c_int;
    pub fn thip_batch_init(b: *mut thip_batch) -> c_int;
    pub fn thip_batch_run(b: *mut thip_batch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_batch_status(b: *mut thip_batch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_batch_solution(b: *mut thip_batch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_batch_iterate(b: *mut thip_batch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_batch_precond(b: *mut thip_batch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_batch_info(b: *const thip_batch, host_info: *mut thip_batch_info_t) -> c_int;
    pub fn thip_batch_grouping(n_inst: c_int, max_group: c_int, host_groups: *mut c_int, host_members: *mut c_int) -> c_int;
    pub fn thip_batch_destroy(b: *mut thip_batch) -> c_int;
    pub fn thip_batch_replace(b: *mut thip_batch, i: c_int, dev_vec_b: *const f32, dev_vec_c: *const f32) -> c_int;
    pub fn thip_batch_set_iterate(b: *mut thip_batch, i: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_batch_set_regroup(b: *mut thip_batch, on: c_int) -> c_int;
    pub fn thip_batch_run_until_any(b: *mut thip_batch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_batch_live_grouping(n_inst: c_int, max_group: c_int, host_live: *const c_int, host_groups: *mut c_int,
                                    host_group_sizes: *mut c_int, host_members: *mut c_int) -> c_int;
    pub fn thip_batch_counters(b: *const thip_batch, host: *mut thip_batch_counters_t) -> c_int;

    // many small problems, each with its own A, iterated on chip (thip_smallbatch.hip)
    pub fn thip_smallbatch_fits(n: usize, m: usize, n_seg: usize, host_seg_type: *const i32, host_seg_len: *const i64,
                                host_lds_bytes: *mut usize, host_threads: *mut c_int) -> c_int;
    pub fn thip_smallbatch_create(n: usize, m: usize, n_prob: usize, dev_mats_a: *const f32, dev_vecs_b: *const f32,
                                  dev_vecs_c: *const f32, dev_vecs_b_rowabs: *const f32, n_seg: usize, host_seg_type: *const i32,
                                  host_seg_len: *const i64, par: *const thip_param, out: *mut *mut thip_smallbatch) -> c_int;
    pub fn thip_smallbatch_set_param(h: *mut thip_smallbatch, par: *const thip_param) -> c_int;
    pub fn thip_smallbatch_init(h: *mut thip_smallbatch) -> c_int;
    pub fn thip_smallbatch_run(h: *mut thip_smallbatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_smallbatch_run_until_any(h: *mut thip_smallbatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_smallbatch_status(h: *mut thip_smallbatch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_smallbatch_solution(h: *mut thip_smallbatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_smallbatch_iterate(h: *mut thip_smallbatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_smallbatch_precond(h: *mut thip_smallbatch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_smallbatch_replace(h: *mut thip_smallbatch, i: c_int, dev_mat_a: *const f32, dev_vec_b: *const f32,
                                   dev_vec_c: *const f32, dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_smallbatch_set_iterates(h: *mut thip_smallbatch, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_smallbatch_set_bc(h: *mut thip_smallbatch, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_smallbatch_solutions(h: *mut thip_smallbatch, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_smallbatch_set_a(h: *mut thip_smallbatch, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_smallbatch_set_bc_dev(h: *mut thip_smallbatch, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_smallbatch_set_a_dev(h: *mut thip_smallbatch, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_smallbatch_set_iterates_dev(h: *mut thip_smallbatch, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_smallbatch_solutions_dev(h: *mut thip_smallbatch, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_smallbatch_info(h: *const thip_smallbatch, host_info: *mut thip_smallbatch_info_t) -> c_int;
    pub fn thip_smallbatch_destroy(h: *mut thip_smallbatch) -> c_int;
    pub fn thip_test_smallbatch_force_threads(h: *mut thip_smallbatch, threads: c_int) -> c_int;

    // many mid-size problems, each with its own A, streamed per workgroup (thip_midbatch.hip)
    pub fn thip_midbatch_fits(n: usize, m: usize, n_seg: usize, host_seg_type: *const i32, host_seg_len: *const i64,
                              host_lds_bytes: *mut usize, host_threads: *mut c_int) -> c_int;
    pub fn thip_midbatch_create(n: usize, m: usize, n_prob: usize, dev_mats_a: *const f32, dev_vecs_b: *const f32,
                                dev_vecs_c: *const f32, dev_vecs_b_rowabs: *const f32, n_seg: usize, host_seg_type: *const i32,
                                host_seg_len: *const i64, par: *const thip_param, out: *mut *mut thip_midbatch) -> c_int;
    pub fn thip_midbatch_set_param(h: *mut thip_midbatch, par: *const thip_param) -> c_int;
    pub fn thip_midbatch_init(h: *mut thip_midbatch) -> c_int;
    pub fn thip_midbatch_run(h: *mut thip_midbatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_midbatch_run_until_any(h: *mut thip_midbatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_midbatch_status(h: *mut thip_midbatch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_midbatch_solution(h: *mut thip_midbatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_midbatch_iterate(h: *mut thip_midbatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_midbatch_precond(h: *mut thip_midbatch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_midbatch_replace(h: *mut thip_midbatch, i: c_int, dev_mat_a: *const f32, dev_vec_b: *const f32,
                                 dev_vec_c: *const f32, dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_midbatch_set_iterates(h: *mut thip_midbatch, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_midbatch_set_bc(h: *mut thip_midbatch, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_midbatch_solutions(h: *mut thip_midbatch, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_midbatch_set_a(h: *mut thip_midbatch, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_midbatch_set_bc_dev(h: *mut thip_midbatch, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_midbatch_set_a_dev(h: *mut thip_midbatch, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_midbatch_set_iterates_dev(h: *mut thip_midbatch, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_midbatch_solutions_dev(h: *mut thip_midbatch, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_midbatch_info(h: *const thip_midbatch, host_info: *mut thip_midbatch_info_t) -> c_int;
    pub fn thip_midbatch_destroy(h: *mut thip_midbatch) -> c_int;
    pub fn thip_test_midbatch_force_threads(h: *mut thip_midbatch, threads: c_int) -> c_int;
    // the mid batch over a library-owned 16-bit copy of every A (thip_mid16batch.hip)
    pub fn thip_mid16batch_fits(n: usize, m: usize, n_seg: usize, host_seg_type: *const i32, host_seg_len: *const i64,
                              host_lds_bytes: *mut usize, host_threads: *mut c_int) -> c_int;
    pub fn thip_mid16batch_create(n: usize, m: usize, n_prob: usize, dev_mats_a: *const f32, dev_vecs_b: *const f32,
                                dev_vecs_c: *const f32, dev_vecs_b_rowabs: *const f32, n_seg: usize, host_seg_type: *const i32,
                                host_seg_len: *const i64, par: *const thip_param, out: *mut *mut thip_mid16batch) -> c_int;
    pub fn thip_mid16batch_set_param(h: *mut thip_mid16batch, par: *const thip_param) -> c_int;
    pub fn thip_mid16batch_init(h: *mut thip_mid16batch) -> c_int;
    pub fn thip_mid16batch_run(h: *mut thip_mid16batch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_mid16batch_run_until_any(h: *mut thip_mid16batch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_mid16batch_status(h: *mut thip_mid16batch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_mid16batch_solution(h: *mut thip_mid16batch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_mid16batch_iterate(h: *mut thip_mid16batch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_mid16batch_precond(h: *mut thip_mid16batch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_mid16batch_replace(h: *mut thip_mid16batch, i: c_int, dev_mat_a: *const f32, dev_vec_b: *const f32,
                                 dev_vec_c: *const f32, dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_mid16batch_set_iterates(h: *mut thip_mid16batch, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_mid16batch_set_bc(h: *mut thip_mid16batch, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_mid16batch_solutions(h: *mut thip_mid16batch, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_mid16batch_set_a(h: *mut thip_mid16batch, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_mid16batch_set_bc_dev(h: *mut thip_mid16batch, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_mid16batch_set_a_dev(h: *mut thip_mid16batch, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_mid16batch_set_iterates_dev(h: *mut thip_mid16batch, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_mid16batch_solutions_dev(h: *mut thip_mid16batch, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_mid16batch_info(h: *const thip_mid16batch, host_info: *mut thip_mid16batch_info_t) -> c_int;
    pub fn thip_mid16batch_destroy(h: *mut thip_mid16batch) -> c_int;
    pub fn thip_test_mid16batch_force_threads(h: *mut thip_mid16batch, threads: c_int) -> c_int;
    pub fn thip_mid16batch_create_kind(n: usize, m: usize, n_prob: usize, dev_mats_a: *const f32, dev_vecs_b: *const f32,
                                       dev_vecs_c: *const f32, dev_vecs_b_rowabs: *const f32, n_seg: usize, host_seg_type: *const i32,
                                       host_seg_len: *const i64, par: *const thip_param, a_kind: c_int, out: *mut *mut thip_mid16batch) -> c_int;
    pub fn thip_mid16batch_store_bytes(n: usize, m: usize, a_kind: c_int, host_bytes: *mut usize) -> c_int;
    pub fn thip_mid16batch_stored(h: *mut thip_mid16batch, i: c_int, host_words: *mut u16, host_inv_scale: *mut f32) -> c_int;

    // many small SDPs, each with its own A: the mid batch's iteration with the PSD cones projected on chip (thip_sdpbatch.hip)
    pub fn thip_sdpbatch_fits(n: usize, m: usize, n_seg: usize, host_seg_type: *const i32, host_seg_len: *const i64,
                              host_lds_bytes: *mut usize, host_threads: *mut c_int) -> c_int;
    pub fn thip_sdpbatch_create(n: usize, m: usize, n_prob: usize, dev_mats_a: *const f32, dev_vecs_b: *const f32,
                                dev_vecs_c: *const f32, dev_vecs_b_rowabs: *const f32, n_seg: usize, host_seg_type: *const i32,
                                host_seg_len: *const i64, par: *const thip_param, out: *mut *mut thip_sdpbatch) -> c_int;
    pub fn thip_sdpbatch_set_param(h: *mut thip_sdpbatch, par: *const thip_param) -> c_int;
    pub fn thip_sdpbatch_init(h: *mut thip_sdpbatch) -> c_int;
    pub fn thip_sdpbatch_run(h: *mut thip_sdpbatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_sdpbatch_run_until_any(h: *mut thip_sdpbatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_sdpbatch_status(h: *mut thip_sdpbatch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_sdpbatch_solution(h: *mut thip_sdpbatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_sdpbatch_iterate(h: *mut thip_sdpbatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_sdpbatch_precond(h: *mut thip_sdpbatch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_sdpbatch_replace(h: *mut thip_sdpbatch, i: c_int, dev_mat_a: *const f32, dev_vec_b: *const f32,
                                 dev_vec_c: *const f32, dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_sdpbatch_set_iterates(h: *mut thip_sdpbatch, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_sdpbatch_set_bc(h: *mut thip_sdpbatch, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_sdpbatch_solutions(h: *mut thip_sdpbatch, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_sdpbatch_set_a(h: *mut thip_sdpbatch, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_sdpbatch_set_bc_dev(h: *mut thip_sdpbatch, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_sdpbatch_set_a_dev(h: *mut thip_sdpbatch, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_sdpbatch_set_iterates_dev(h: *mut thip_sdpbatch, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_sdpbatch_solutions_dev(h: *mut thip_sdpbatch, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_sdpbatch_info(h: *const thip_sdpbatch, host_info: *mut thip_sdpbatch_info_t) -> c_int;
    pub fn thip_sdpbatch_destroy(h: *mut thip_sdpbatch) -> c_int;
    pub fn thip_test_sdpbatch_force_threads(h: *mut thip_sdpbatch, threads: c_int) -> c_int;
    pub fn thip_test_sdpbatch_project(k: c_int, count: c_int, dev_packed: *mut f32, dev_rx_or_null: *mut f32) -> c_int;
    pub fn thip_test_sdpbatch_project_form(k: c_int, count: c_int, threads: c_int, in_lds: c_int, dev_packed: *mut f32, dev_rx_or_null: *mut f32) -> c_int;
    // the SDP batch's iteration on every shape to 4096 x 4096: all but the pass vectors left in the arena (thip_widebatch.hip)
    pub fn thip_widebatch_fits(n: usize, m: usize, n_seg: usize, host_seg_type: *const i32, host_seg_len: *const i64,
                              host_lds_bytes: *mut usize, host_threads: *mut c_int) -> c_int;
    pub fn thip_widebatch_create(n: usize, m: usize, n_prob: usize, dev_mats_a: *const f32, dev_vecs_b: *const f32,
                                dev_vecs_c: *const f32, dev_vecs_b_rowabs: *const f32, n_seg: usize, host_seg_type: *const i32,
                                host_seg_len: *const i64, par: *const thip_param, out: *mut *mut thip_widebatch) -> c_int;
    pub fn thip_widebatch_set_param(h: *mut thip_widebatch, par: *const thip_param) -> c_int;
    pub fn thip_widebatch_init(h: *mut thip_widebatch) -> c_int;
    pub fn thip_widebatch_run(h: *mut thip_widebatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_widebatch_run_until_any(h: *mut thip_widebatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_widebatch_status(h: *mut thip_widebatch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_widebatch_solution(h: *mut thip_widebatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_widebatch_iterate(h: *mut thip_widebatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_widebatch_precond(h: *mut thip_widebatch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_widebatch_replace(h: *mut thip_widebatch, i: c_int, dev_mat_a: *const f32, dev_vec_b: *const f32,
                                 dev_vec_c: *const f32, dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_widebatch_set_iterates(h: *mut thip_widebatch, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_widebatch_set_bc(h: *mut thip_widebatch, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_widebatch_solutions(h: *mut thip_widebatch, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_widebatch_set_a(h: *mut thip_widebatch, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_widebatch_set_bc_dev(h: *mut thip_widebatch, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_widebatch_set_a_dev(h: *mut thip_widebatch, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_widebatch_set_iterates_dev(h: *mut thip_widebatch, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_widebatch_solutions_dev(h: *mut thip_widebatch, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_widebatch_info(h: *const thip_widebatch, host_info: *mut thip_widebatch_info_t) -> c_int;
    pub fn thip_widebatch_destroy(h: *mut thip_widebatch) -> c_int;
    pub fn thip_test_widebatch_force_threads(h: *mut thip_widebatch, threads: c_int) -> c_int;
    // the wide batch over a library-owned 16-bit copy of every A (thip_wide16batch.hip)
    pub fn thip_wide16batch_fits(n: usize, m: usize, n_seg: usize, host_seg_type: *const i32, host_seg_len: *const i64,
                              host_lds_bytes: *mut usize, host_threads: *mut c_int) -> c_int;
    pub fn thip_wide16batch_create(n: usize, m: usize, n_prob: usize, dev_mats_a: *const f32, dev_vecs_b: *const f32,
                                dev_vecs_c: *const f32, dev_vecs_b_rowabs: *const f32, n_seg: usize, host_seg_type: *const i32,
                                host_seg_len: *const i64, par: *const thip_param, out: *mut *mut thip_wide16batch) -> c_int;
    pub fn thip_wide16batch_set_param(h: *mut thip_wide16batch, par: *const thip_param) -> c_int;
    pub fn thip_wide16batch_init(h: *mut thip_wide16batch) -> c_int;
    pub fn thip_wide16batch_run(h: *mut thip_wide16batch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_wide16batch_run_until_any(h: *mut thip_wide16batch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_wide16batch_status(h: *mut thip_wide16batch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_wide16batch_solution(h: *mut thip_wide16batch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_wide16batch_iterate(h: *mut thip_wide16batch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_wide16batch_precond(h: *mut thip_wide16batch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_wide16batch_replace(h: *mut thip_wide16batch, i: c_int, dev_mat_a: *const f32, dev_vec_b: *const f32,
                                 dev_vec_c: *const f32, dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_wide16batch_set_iterates(h: *mut thip_wide16batch, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_wide16batch_set_bc(h: *mut thip_wide16batch, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_wide16batch_solutions(h: *mut thip_wide16batch, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_wide16batch_set_a(h: *mut thip_wide16batch, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_wide16batch_set_bc_dev(h: *mut thip_wide16batch, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_wide16batch_set_a_dev(h: *mut thip_wide16batch, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_wide16batch_set_iterates_dev(h: *mut thip_wide16batch, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_wide16batch_solutions_dev(h: *mut thip_wide16batch, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_wide16batch_info(h: *const thip_wide16batch, host_info: *mut thip_wide16batch_info_t) -> c_int;
    pub fn thip_wide16batch_destroy(h: *mut thip_wide16batch) -> c_int;
    pub fn thip_test_wide16batch_force_threads(h: *mut thip_wide16batch, threads: c_int) -> c_int;
    pub fn thip_wide16batch_create_kind(n: usize, m: usize, n_prob: usize, dev_mats_a: *const f32, dev_vecs_b: *const f32,
                                       dev_vecs_c: *const f32, dev_vecs_b_rowabs: *const f32, n_seg: usize, host_seg_type: *const i32,
                                       host_seg_len: *const i64, par: *const thip_param, a_kind: c_int, out: *mut *mut thip_wide16batch) -> c_int;
    pub fn thip_wide16batch_store_bytes(n: usize, m: usize, a_kind: c_int, host_bytes: *mut usize) -> c_int;
    pub fn thip_wide16batch_stored(h: *mut thip_wide16batch, i: c_int, host_words: *mut u16, host_inv_scale: *mut f32) -> c_int;

    // problems of different shapes and cone layouts in one batch: the SDP batch's iteration on a problem the workgroup looks up
    // (thip_raggedbatch.hip)
    pub fn thip_raggedbatch_fits(n_prob: usize, host_n: *const usize, host_m: *const usize, host_n_seg: *const usize,
                                 host_seg_type: *const i32, host_seg_len: *const i64, host_first_refused: *mut c_int,
                                 host_lds_bytes: *mut usize, host_threads: *mut c_int) -> c_int;
    pub fn thip_raggedbatch_create(n_prob: usize, host_n: *const usize, host_m: *const usize, dev_a: *const f32,
                                   host_at_a: *const i64, dev_b: *const f32, host_at_b: *const i64, dev_c: *const f32,
                                   host_at_c: *const i64, dev_b_rowabs: *const f32, host_at_rowabs: *const i64,
                                   host_n_seg: *const usize, host_seg_type: *const i32, host_seg_len: *const i64,
                                   par: *const thip_param, out: *mut *mut thip_raggedbatch) -> c_int;
    pub fn thip_raggedbatch_set_param(h: *mut thip_raggedbatch, par: *const thip_param) -> c_int;
    pub fn thip_raggedbatch_init(h: *mut thip_raggedbatch) -> c_int;
    pub fn thip_raggedbatch_run(h: *mut thip_raggedbatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_raggedbatch_run_until_any(h: *mut thip_raggedbatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_raggedbatch_status(h: *mut thip_raggedbatch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_raggedbatch_solution(h: *mut thip_raggedbatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_raggedbatch_iterate(h: *mut thip_raggedbatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_raggedbatch_precond(h: *mut thip_raggedbatch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_raggedbatch_replace(h: *mut thip_raggedbatch, i: c_int, dev_mat_a: *const f32, dev_vec_b: *const f32,
                                    dev_vec_c: *const f32, dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_raggedbatch_set_iterates(h: *mut thip_raggedbatch, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_raggedbatch_set_bc(h: *mut thip_raggedbatch, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_raggedbatch_solutions(h: *mut thip_raggedbatch, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_raggedbatch_set_a(h: *mut thip_raggedbatch, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_raggedbatch_set_bc_dev(h: *mut thip_raggedbatch, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_raggedbatch_set_a_dev(h: *mut thip_raggedbatch, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_raggedbatch_set_iterates_dev(h: *mut thip_raggedbatch, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_raggedbatch_solutions_dev(h: *mut thip_raggedbatch, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_raggedbatch_info(h: *const thip_raggedbatch, host_info: *mut thip_raggedbatch_info_t) -> c_int;
    pub fn thip_raggedbatch_destroy(h: *mut thip_raggedbatch) -> c_int;
    pub fn thip_test_raggedbatch_force_threads(h: *mut thip_raggedbatch, threads: c_int) -> c_int;
    pub fn thip_test_raggedbatch_plan(n_prob: usize, host_n: *const usize, host_m: *const usize, host_n_seg: *const usize,
                                      host_seg_type: *const i32, host_seg_len: *const i64, force_threads: c_int,
                                      host_class: *mut c_int, host_order: *mut c_int, host_layout: *mut c_int,
                                      host_arena_at: *mut i64, host_info: *mut thip_raggedbatch_info_t) -> c_int;
    // problems of one shape, each with its own sparse A held as packed entries (thip_sparsebatch.hip)
    pub fn thip_sparsebatch_fits(n: usize, m: usize, nnz_cap: usize, n_seg: usize, host_seg_type: *const i32, host_seg_len: *const i64,
                                 host_lds_bytes: *mut usize, host_threads: *mut c_int, host_resident: *mut c_int) -> c_int;
    pub fn thip_sparsebatch_create(n: usize, m: usize, n_prob: usize, host_colptr: *const i64, host_start: *const i64,
                                   host_rowidx: *const i32, host_values: *const f32, dev_vecs_b: *const f32, dev_vecs_c: *const f32,
                                   dev_vecs_b_rowabs: *const f32, nnz_cap: usize, n_seg: usize, host_seg_type: *const i32,
                                   host_seg_len: *const i64, par: *const thip_param, out: *mut *mut thip_sparsebatch) -> c_int;
    pub fn thip_sparsebatch_set_param(h: *mut thip_sparsebatch, par: *const thip_param) -> c_int;
    pub fn thip_sparsebatch_init(h: *mut thip_sparsebatch) -> c_int;
    pub fn thip_sparsebatch_run(h: *mut thip_sparsebatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_sparsebatch_run_until_any(h: *mut thip_sparsebatch, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_sparsebatch_status(h: *mut thip_sparsebatch, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_sparsebatch_solution(h: *mut thip_sparsebatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_sparsebatch_iterate(h: *mut thip_sparsebatch, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_sparsebatch_precond(h: *mut thip_sparsebatch, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_sparsebatch_replace(h: *mut thip_sparsebatch, i: c_int, host_colptr: *const i64, host_rowidx: *const i32,
                                    host_values: *const f32, dev_vec_b: *const f32, dev_vec_c: *const f32,
                                    dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_sparsebatch_set_iterates(h: *mut thip_sparsebatch, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_sparsebatch_set_bc(h: *mut thip_sparsebatch, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_sparsebatch_solutions(h: *mut thip_sparsebatch, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_sparsebatch_set_a(h: *mut thip_sparsebatch, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_sparsebatch_set_bc_dev(h: *mut thip_sparsebatch, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_sparsebatch_set_a_dev(h: *mut thip_sparsebatch, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_sparsebatch_set_iterates_dev(h: *mut thip_sparsebatch, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_sparsebatch_solutions_dev(h: *mut thip_sparsebatch, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_sparsebatch_info(h: *const thip_sparsebatch, host_info: *mut thip_sparsebatch_info_t) -> c_int;
    pub fn thip_sparsebatch_destroy(h: *mut thip_sparsebatch) -> c_int;
    pub fn thip_test_sparsebatch_force_threads(h: *mut thip_sparsebatch, threads: c_int) -> c_int;
    pub fn thip_test_sparsebatch_force_resident(h: *mut thip_sparsebatch, resident: c_int) -> c_int;
    pub fn thip_test_sparsebatch_blob(h: *mut thip_sparsebatch, i: c_int, host_words: *mut u32, cap_words: usize, host_used_words: *mut usize) -> c_int;
    pub fn thip_test_sparsebatch_pack(n: usize, m: usize, host_colptr: *const i64, host_rowidx: *const i32, host_values: *const f32,
                                      nnz_cap: usize, host_words: *mut u32, cap_words: usize, host_used_words: *mut usize,
                                      host_long: *mut c_int) -> c_int;
    // sparse problems of different shapes and cone layouts in one batch (thip_raggedsparse.hip)
    pub fn thip_raggedsparse_fits(n_prob: usize, host_n: *const usize, host_m: *const usize, host_nnz_cap: *const usize,
                                  host_n_seg: *const usize, host_seg_type: *const i32, host_seg_len: *const i64,
                                  host_first_refused: *mut c_int, host_lds_bytes: *mut usize, host_threads: *mut c_int,
                                  host_resident: *mut c_int) -> c_int;
    pub fn thip_raggedsparse_create(n_prob: usize, host_n: *const usize, host_m: *const usize, host_colptr: *const i64,
                                    host_start: *const i64, host_rowidx: *const i32, host_values: *const f32,
                                    host_nnz_cap: *const usize, dev_b: *const f32, host_at_b: *const i64, dev_c: *const f32,
                                    host_at_c: *const i64, dev_b_rowabs: *const f32, host_at_rowabs: *const i64,
                                    host_n_seg: *const usize, host_seg_type: *const i32, host_seg_len: *const i64,
                                    par: *const thip_param, out: *mut *mut thip_raggedsparse) -> c_int;
    pub fn thip_raggedsparse_set_param(h: *mut thip_raggedsparse, par: *const thip_param) -> c_int;
    pub fn thip_raggedsparse_init(h: *mut thip_raggedsparse) -> c_int;
    pub fn thip_raggedsparse_run(h: *mut thip_raggedsparse, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_raggedsparse_run_until_any(h: *mut thip_raggedsparse, max_steps: i64, poll_every: i64, host_status: *mut thip_status) -> c_int;
    pub fn thip_raggedsparse_status(h: *mut thip_raggedsparse, i: c_int, host_status: *mut thip_status) -> c_int;
    pub fn thip_raggedsparse_solution(h: *mut thip_raggedsparse, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_raggedsparse_iterate(h: *mut thip_raggedsparse, i: c_int, host_x: *mut f32, host_y: *mut f32) -> c_int;
    pub fn thip_raggedsparse_precond(h: *mut thip_raggedsparse, i: c_int, host_dp_tau: *mut f32, host_dp_sigma: *mut f32) -> c_int;
    pub fn thip_raggedsparse_replace(h: *mut thip_raggedsparse, i: c_int, host_colptr: *const i64, host_rowidx: *const i32,
                                     host_values: *const f32, dev_vec_b: *const f32, dev_vec_c: *const f32,
                                     dev_vec_b_rowabs: *const f32) -> c_int;
    pub fn thip_raggedsparse_set_iterates(h: *mut thip_raggedsparse, first: c_int, count: c_int, host_x: *const f32, host_y: *const f32) -> c_int;
    pub fn thip_raggedsparse_set_bc(h: *mut thip_raggedsparse, first: c_int, count: c_int, host_b: *const f32, host_c: *const f32, host_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_raggedsparse_solutions(h: *mut thip_raggedsparse, first: c_int, count: c_int, host_x: *mut f32, host_y: *mut f32, host_status: *mut thip_status) -> c_int;
    pub fn thip_raggedsparse_set_a(h: *mut thip_raggedsparse, first: c_int, count: c_int, host_values: *const f32, host_counts: *const i64, keep_iterate: c_int) -> c_int;
    pub fn thip_raggedsparse_set_bc_dev(h: *mut thip_raggedsparse, first: c_int, count: c_int, dev_b: *const f32, dev_c: *const f32, dev_b_rowabs: *const f32, host_has_rowabs: *const u8, keep_iterate: c_int) -> c_int;
    pub fn thip_raggedsparse_set_a_dev(h: *mut thip_raggedsparse, first: c_int, count: c_int, dev_values: *const f32, keep_iterate: c_int) -> c_int;
    pub fn thip_raggedsparse_set_iterates_dev(h: *mut thip_raggedsparse, first: c_int, count: c_int, dev_x: *const f32, dev_y: *const f32) -> c_int;
    pub fn thip_raggedsparse_solutions_dev(h: *mut thip_raggedsparse, first: c_int, count: c_int, dev_x: *mut f32, dev_y: *mut f32, dev_state: *mut i32) -> c_int;
    pub fn thip_raggedsparse_info(h: *const thip_raggedsparse, host_info: *mut thip_raggedsparse_info_t) -> c_int;
    pub fn thip_raggedsparse_destroy(h: *mut thip_raggedsparse) -> c_int;
    pub fn thip_test_raggedsparse_force_threads(h: *mut thip_raggedsparse, threads: c_int) -> c_int;
    pub fn thip_test_raggedsparse_force_resident(h: *mut thip_raggedsparse, resident: c_int) -> c_int;
    pub fn thip_test_raggedsparse_blob(h: *mut thip_raggedsparse, i: c_int, host_words: *mut u32, cap_words: usize, host_used_words: *mut usize) -> c_int;
    pub fn thip_test_raggedsparse_plan(n_prob: usize, host_n: *const usize, host_m: *const usize, host_nnz: *const usize,
                                       host_nnz_cap: *const usize, host_n_seg: *const usize, host_seg_type: *const i32,
                                       host_seg_len: *const i64, force_threads: c_int, force_resident: c_int, host_class: *mut c_int,
                                       host_order: *mut c_int, host_layout: *mut c_int, host_arena_at: *mut i64,
                                       host_blob_at: *mut i64, host_lds_at: *mut c_int, host_resident: *mut c_int,
                                       host_info: *mut thip_raggedsparse_info_t) -> c_int;
    pub fn thip_test_ownbatch_addresses(h: *mut c_void, host_addr: *mut u64, host_bytes: *mut u64) -> c_int;
    pub fn thip_test_ownbatch_last_transfer(h: *mut c_void, host_h2d_bytes: *mut u64, host_d2h_bytes: *mut u64) -> c_int;
    pub fn thip_test_ownbatch_overlap(a: u64, a_bytes: u64, b: u64, b_bytes: u64) -> c_int;
    pub fn thip_test_ownbatch_offsets(count: usize, host_n: *const usize, host_m: *const usize, host_at: *mut i64) -> c_int;
    pub fn thip_test_ownbatch_copy_chunk() -> c_int;

    pub fn thip_comm_unique_id(host_id128: *mut u8) -> c_int;
    pub fn thip_comm_init(rank: c_int, world: c_int, host_id128: *const u8) -> c_int;
    pub fn thip_comm_allreduce(dev_buf: *mut f32, n: usize) -> c_int;
    pub fn thip_comm_count(host_ranks: *mut c_int) -> c_int;
    pub fn thip_comm_destroy() -> c_int;
    pub fn thip_solver_use_rccl(s: *mut thip_solver) -> c_int;
    pub fn thip_oneshot_init(rank: c_int, world: c_int, max_floats: usize, host_handle64: *mut u8) -> c_int;
    pub fn thip_oneshot_connect(host_handles: *const u8) -> c_int;
    pub fn thip_oneshot_allreduce(dev_buf: *mut f32, n: usize) -> c_int;
    pub fn thip_oneshot_error(host_err: *mut c_int) -> c_int;
    pub fn thip_oneshot_destroy() -> c_int;
    pub fn thip_solver_use_oneshot(s: *mut thip_solver) -> c_int;
    pub fn thip_solver_set_gemv_autotune(s: *mut thip_solver, on: c_int) -> c_int;
    pub fn thip_solver_set_lda_pad(s: *mut thip_solver, floats: c_int) -> c_int;

    pub fn thip_gen_vector(out: *mut f32, n: usize, seed: u64, stream: u64, idx0: u64, kind: c_int, scale: f32, shift: f32) -> c_int;
    pub fn thip_gen_matrix(out: *mut f32, n_row: usize, n_col: usize, lda: usize, seed: u64, stream: u64, row0: u64,
                           col0: u64, ld_index: u64, kind: c_int, scale: f32, shift: f32) -> c_int;
    pub fn thip_gen_identity(out: *mut f32, n_row: usize, n_col: usize, lda: usize, row0: u64, value: f32) -> c_int;

    pub fn thip_prof_enable(on: c_int) -> c_int;
    pub fn thip_prof_read(host_launches: *mut i64, host_total_ms: *mut f64) -> c_int;
    pub fn thip_prof_read_psd(host_spans: *mut i64, host_total_ms: *mut f64) -> c_int;
}

/// Test hooks and timing probes (include/totsu_f32hip_test.h): exported by the same library, not part of the interface
/// this crate wraps -- declared only for the crate's own device tests.
#[cfg(feature = "test-hooks")]
extern "C" {
    pub fn thip_test_eig_force(engine: c_int) -> c_int;
    pub fn thip_test_gemv_multi(m: usize, n: usize, mat: *const f32, nv: c_int, host_xn: *const *const f32, host_xt: *const *const f32,
                                host_out_n: *const *mut f32, host_out_t: *const *mut f32, host_stopped: *const c_int, nj: c_int,
                                target_blocks: c_int, reps: c_int, host_ms: *mut f32) -> c_int;
    pub fn thip_test_dual_gemv(t: *const thip_gemv_test, host_plan: *mut thip_gemv_plan_rec) -> c_int;
    pub fn thip_test_gemv_plan(m: usize, n: usize, vw: c_int, nj: c_int, target_blocks: c_int, col0: usize, col1: usize,
                               host_plan: *mut thip_gemv_plan_rec, host_scratch_floats: *mut usize, host_split_col: *mut usize) -> c_int;
    pub fn thip_test_solver_pin_gemv_plan(s: *mut thip_solver, candidate_index: c_int) -> c_int;
    pub fn thip_test_gemv_multi_plan(m: usize, n: usize, instance: c_int, nj: c_int, target_blocks: c_int,
                                     host_plan: *mut thip_gemv_plan_rec, host_scratch_floats: *mut usize) -> c_int;
    pub fn thip_test_dual_gemv_multi(t: *const thip_gemv_multi_test, host_plan: *mut thip_gemv_plan_rec) -> c_int;
    pub fn thip_test_batch_pin_multi_plan(b: *mut thip_batch, instance: c_int, candidate_index: c_int) -> c_int;
    pub fn thip_test_batch_last_multi_plan(b: *const thip_batch, instance: c_int, host_plan: *mut thip_gemv_plan_rec) -> c_int;
    pub fn thip_test_spin_allreduce(s: *mut thip_solver, latency_us: c_int) -> c_int;
    pub fn thip_test_sweep(t: *const thip_sweep_test, host_ms: *mut f32, host_info: *mut c_int) -> c_int;
    pub fn thip_test_sweep_plan(m: usize, n: usize, lda: usize, elem: c_int, cols_per_panel: c_int, gmul: c_int, force_members: c_int,
                                host_plan: *mut thip_sweep_plan_rec, host_candidates: *mut thip_sweep_plan_rec,
                                host_n_candidates: *mut c_int) -> c_int;
    pub fn thip_test_solver_pin_sweep_plan(s: *mut thip_solver, candidate_index: c_int) -> c_int;
    pub fn thip_test_solver_kahan(s: *mut thip_solver, host_kx: *mut f32, host_ky: *mut f32, host_ks: *mut f32, host_ku: *mut f32,
                                  host_kv: *mut f32, host_mtail_form: *mut c_int) -> c_int;
    pub fn thip_test_sweep_fault(s: *mut thip_solver, kind: c_int, after_sweeps: i64, spin_max: c_int) -> c_int;
    pub fn thip_test_gemm_sym(n: c_int, ld: c_int, alpha: f32, a: *const f32, b: *const f32, beta: f32, d: *const f32,
                              gamma: f32, c: *mut f32) -> c_int;
    pub fn thip_test_gemm_chain(shape: c_int, kernel: c_int, n: c_int, ld: c_int, nb: c_int, alpha: f32, x: *const f32,
                                y: *const f32, beta: f32, d: *const f32, gamma: f32, c: *mut f32) -> c_int;
    pub fn thip_test_chain_probe(mode: c_int, ld: c_int, reps: c_int, host_us: *mut f32) -> c_int;
    pub fn thip_test_sptile_time(mat: *mut thip_sptile, reps: c_int, host_ms: *mut f32) -> c_int;
    pub fn thip_test_sptile_equal(a: *const thip_sptile, b: *const thip_sptile, host_first_difference: *mut c_int) -> c_int;
    pub fn thip_test_gemm_dual(kernel: c_int, n: c_int, ld: c_int, nb: c_int, a: *const f32, b0: *const f32, b1: *const f32,
                               coef: *const f32, o0: *mut f32, o1: *mut f32) -> c_int;
}

pub const THIP_A_F32: c_int = 0;
pub const THIP_A_BF16: c_int = 1;
pub const THIP_A_F16: c_int = 2;

/// The reference backends assert on library status (totsu_f32cuda/src/f32cuda.rs:38): so does this one.
pub fn chk(rc: c_int) {
    if rc != 0 {
        let msg = unsafe { std::ffi::CStr::from_ptr(thip_last_error()) }.to_string_lossy().into_owned();
        panic!("totsu_f32hip: error {}: {}", rc, msg);
    }
}
