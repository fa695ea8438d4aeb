// povar_lm.hip -- the stages of an LM iteration behind the C ABI: state, cost, linearise, prepare, apply (step 1 and step 2), exports.
#include "povar_ctx.hpp"

// every kernel of the LM iteration runs on the lane-per-landmark layout: nothing reads the legacy camera-major copies
static bool lpl_only(const povar_ctx* c) { return lpl_mode(c) && c->use_lpl_prepare; }

// the lane-per-landmark kernels of this unit share one signature and one launch shape
using LplKernel = void (*)(Dp, double*);
static void launch_lpl(povar_ctx* c, LplKernel k, size_t lds, const Dp& d, double* out) {
  hipLaunchKernelGGL(k, dim3(c->e0c_grid), dim3(E0C_BLOCK), lds, c->stream, d, out);
}

// dynamic LDS of the lane-per-landmark kernels this unit launches (povar_create)
hipError_t lm_set_lds_all() {
  const size_t prep = prep_lds_bytes(HOT_ACC_MAX), pass = pass_lds_bytes(HOT_ACC_MAX);
  const struct { LplKernel k; size_t bytes; } tab[] = {
      {prepare_lpl<false>, prep}, {prepare_lpl<true>, prep}, {lpl_pass_h<0>, pass}, {lpl_pass_h<1>, pass},
      {backsub_lpl_h<false>, back_lds_bytes_h(HOT_ACC_MAX)}, {backsub_lpl_h<true>, back_lds_bytes_h(HOT_ACC_MAX)},
      {lpl_pass<0>, pass}, {lpl_pass<1>, pass}, {backsub_lpl<false>, back_lds_bytes(HOT_ACC_MAX)},
      {backsub_lpl<true>, back_lds_bytes(HOT_ACC_MAX)}, {prepare_lpl_h<false>, prep}, {prepare_lpl_h<true>, prep}};
  hipError_t e = hipSuccess;
  for (const auto& t : tab)
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)t.k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.bytes);
  return e;
}

// mode 0: linearise, 1: cost
static void launch_lpl_pass(povar_ctx* c, int step, int mode) {
  launch_lpl(c, step == 1 ? (mode ? lpl_pass<1> : lpl_pass<0>) : (mode ? lpl_pass_h<1> : lpl_pass_h<0>),
             pass_lds_bytes(c->v2_max_slots), c->d, c->part.p);
}

static void launch_prepare_lpl(povar_ctx* c, int step, const Dp& da) {
  const bool r = c->opt.robust_norm;
  launch_lpl(c, step == 1 ? (r ? prepare_lpl<true> : prepare_lpl<false>) : (r ? prepare_lpl_h<true> : prepare_lpl_h<false>),
             prep_lds_bytes(c->v2_max_slots), da, c->v2_part.p);
}

static void launch_backsub_lpl(povar_ctx* c, int step, const Dp& da) {
  const bool r = c->opt.robust_norm;
  if (step == 1) launch_lpl(c, r ? backsub_lpl<true> : backsub_lpl<false>, back_lds_bytes(c->v2_max_slots), da, c->part.p);
  else launch_lpl(c, r ? backsub_lpl_h<true> : backsub_lpl_h<false>, back_lds_bytes_h(c->v2_max_slots), da, c->part.p);
}

// the N sums of a stage into scal: over the partials of the lane-per-landmark kernels or of launch_lm
template <int N>
static void reduce_sums(povar_ctx* c, bool lpl) {
  if (lpl) hipLaunchKernelGGL((reduce_partials<N>), dim3(1), dim3(1024), 0, c->stream, c->part.p, c->e0c_grid, c->scal.p);
  else launch_reduce<N>(c, c->scal.p);
}

// landmarks and cameras were written; mirror_current: the writer kept the lane-ordered landmark mirror (V2::lmx) in step
static void state_written(povar_ctx* c, bool mirror_current) {
  ++c->lms_ver;
  ++c->cams_ver;
  if (mirror_current) c->lmx_ver = c->lms_ver;
}

void build_views(povar_ctx* c) {
  const int hom = c->linearized_h ? 1 : 0;
  hipLaunchKernelGGL(cm_build_h, dim3(grid_for(c->n_obs, 256)), dim3(256), 0, c->stream, c->d, (const int*)c->cm_lm.p, c->cm_h.p, c->n_obs, hom);
  if (c->n_cold > 0)
    hipLaunchKernelGGL(cm_build_h, dim3(grid_for(c->n_cold, 256)), dim3(256), 0, c->stream, c->d, (const int*)c->cc_lm.p, c->cc_h.p, c->n_cold, hom);
  if (c->long_in_kernel && c->n_cold2 > 0)
    hipLaunchKernelGGL(cm_build_h, dim3(grid_for(c->n_cold2, 256)), dim3(256), 0, c->stream, c->d, (const int*)c->c2_lm.p, c->c2_h.p, c->n_cold2, hom);
  c->views_lin_id = c->lin_id;
}

// lane-ordered mirrors (V2::lmx / lml / lsc), rebuilt from the landmark-order masters when stale
void lanes_from(povar_ctx* c, const double4* src, double4* dst) {
  const int64_t n = (int64_t)c->d.v2.n_tiles * WAVE;
  if (n > 0) hipLaunchKernelGGL(lm_to_lanes, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->d.v2.lm_of, src, dst, n);
}

void ensure_lmx(povar_ctx* c) {
  if (c->lmx_ver == c->lms_ver) return;
  lanes_from(c, c->lms4.p, c->v2_lmx.p);
  c->lmx_ver = c->lms_ver;
}

void ensure_lin_mirrors(povar_ctx* c) {
  if (c->lml_lin_id != c->lin_id) { lanes_from(c, c->lms_lin4.p, c->v2_lml.p); c->lml_lin_id = c->lin_id; }
  if (c->lsc_lin_id != c->lin_id) { lanes_from(c, c->jl_scale4.p, c->v2_lsc.p); c->lsc_lin_id = c->lin_id; }
}

// a landmark-order master (jl_scale4, lms_lin4) from its lane-ordered mirror: the lane-per-landmark linearisation keeps
// only the lane-ordered copies (V2::lsc, V2::lml); the lane-per-observation kernels and the exports read the masters
static void ensure_master(povar_ctx* c, int64_t& have_lin_id, const double4* lanes, double4* master) {
  if (have_lin_id == c->lin_id) return;
  const int64_t n = (int64_t)c->d.v2.n_tiles * WAVE;
  if (n > 0) hipLaunchKernelGGL(lanes_to_lm, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->d.v2.lm_of, c->d.v2.seg, lanes, master, n);
  have_lin_id = c->lin_id;
}

// called by every entry point that may run a lane-per-observation ("legacy") kernel: the camera-major landmark copies
// (cm_scatter, the cold views of e0_lm_cached) and the per-slot sqrt(w) / weighted residual arrays, which the
// lane-per-landmark linearisation (lpl_pass<0>) does not write
void ensure_legacy(povar_ctx* c) {
  if (!(c->linearized || c->linearized_h)) return;
  ensure_master(c, c->jls_lin_id, c->v2_lsc.p, c->jl_scale4.p);
  ensure_master(c, c->lmslin_lin_id, c->v2_lml.p, c->lms_lin4.p);
  c->flag0_clean = false;  // the auxiliary linearisation below may raise the finiteness flag
  if (c->views_lin_id != c->lin_id) build_views(c);
  // the lazily rebuilt sqrt(w) / residual arrays and landmark records belong to the LINEARISATION: they are built
  // with its alpha, whatever alpha the caller (apply_pose, error_pose) has put into the context meanwhile
  struct AlphaGuard {
    povar_ctx* c;
    double sa, sb;
    explicit AlphaGuard(povar_ctx* c_) : c(c_), sa(c_->d.sa), sb(c_->d.sb) {
      if (c->linearized && !c->linearized_h) {
        c->d.sa = std::sqrt(c->alpha_lin);
        c->d.sb = std::sqrt(1.0 - c->alpha_lin);
      }
    }
    ~AlphaGuard() { c->d.sa = sa; c->d.sb = sb; }
  } guard(c);
  if (c->aux_lin_id != c->lin_id) {
    Dp da = c->d;
    da.lin_aux_only = 1;
    if (c->linearized_h) launch_lm(c, OpLinearizeH{}, da);
    else launch_lm(c, OpLinearize{}, da);
    c->aux_lin_id = c->lin_id;
  }
  if (c->prep_id && c->aux_prep_id != c->prep_id && c->prep_lin_id == c->lin_id) {
    // the landmark half of prepare_Hb again, on the lane-per-observation layout: Hll^-1 and the packed landmark records
    Dp da = c->d;
    da.prep_aux_only = 1;
    if (c->joint) launch_lm(c, OpPrepareH{}, da);
    else launch_lm(c, OpPrepare{}, da);
    c->aux_prep_id = c->prep_id;
  }
}

// flags[0] (finiteness / p2p time-out bits) is reset before every entry point that reads it back; when the last
// read-back was zero and nothing that can raise it has been enqueued since, the reset is skipped
int clear_flag0(povar_ctx* c) {
  if (!c->flag0_clean) HIP_TRY(hipMemsetAsync(c->flags.p, 0, sizeof(int), c->stream));
  c->flag0_clean = false;  // writers follow; clean again only after a read-back of zero (not when that read-back fails: ADVICE r03)
  return 0;
}

// what besides the state decides which kernels a cost evaluation runs
static int err_memo_mode(const povar_ctx* c) { return c->opt.e0_mode * 4 + (c->use_lpl ? 2 : 0) + (c->use_lpl_prepare ? 1 : 0); }

bool err_memo_hit(const povar_ctx* c, int kind, double alpha, povar_residual_info* out) {
  // (not while sharded: a hit returns before the all-reduce of the failure flag, and whether a rank's memo is valid
  // depends on rank-local events -- a rank that recomputes would enter the collective alone.  ADVICE r03.)
  if (sharded(c)) return false;
  const auto& m = c->err_memo;
  if (!m.valid || m.kind != kind || m.alpha != alpha || m.lms_ver != c->lms_ver || m.cams_ver != c->cams_ver ||
      m.mode != err_memo_mode(c))
    return false;
  *out = m.ri;
  return true;
}

void err_memo_store(povar_ctx* c, int kind, double alpha, const povar_residual_info& ri) {
  auto& m = c->err_memo;
  m.valid = !c->no_err_memo;
  m.kind = kind;
  m.alpha = alpha;
  m.lms_ver = c->lms_ver;
  m.cams_ver = c->cams_ver;
  m.mode = err_memo_mode(c);
  m.ri = ri;
}

// OR of a per-rank failure flag over the ranks (is_numerically_valid, linearisation failure)
int combine_flag(povar_ctx* c, int* flag) {
  if (!sharded(c)) return 0;
  double v = *flag ? 1.0 : 0.0;
  HIP_TRY(hipMemcpyAsync(c->scal.p + 7, &v, sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (int rc = allreduce(c, c->scal.p + 7, 1)) return rc;
  HIP_TRY(hipMemcpyAsync(&v, c->scal.p + 7, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *flag = v > 0 ? 1 : 0;
  return 0;
}

int ensure_tiles(povar_ctx* c) {
  if (c->opt.e0_mode != POVAR_E0_TILES && c->opt.e0_mode != POVAR_E0_TILES_LDSACC) return 0;
  if (!c->tiles.p) {
    HIP_TRY(c->tiles.alloc((size_t)c->n_bins * TILE_PAIRS * WAVE, &c->bytes));
    c->d.tiles = c->tiles.p;
    c->tiles_valid = false;
  }
  if (!c->tiles_valid) {
    ensure_legacy(c);
    hipLaunchKernelGGL(materialize_tiles, dim3(grid_for(c->n_slots, LM_BLOCK)), dim3(LM_BLOCK), 0,
                       c->stream, c->d);
    c->tiles_valid = true;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------
// the stages of an LM iteration, one body for step 1 (pOSE, affine landmarks) and step 2 (joint, homogeneous landmarks)
// ------------------------------------------------------------------------------------------
extern "C" void set_alpha(povar_ctx* c, double alpha) {
  c->d.sa = std::sqrt(alpha);
  c->d.sb = std::sqrt(1.0 - alpha);
}

static int check_linearized(const povar_ctx* c, int step, const char* who) {
  if (step == 1 ? c->linearized : c->linearized_h) return 0;
  return fail(-1, std::string(who) + " before " + (step == 1 ? "povar_linearize_pose" : "povar_linearize_homogeneous"));
}

// cost.  The memo kind is the step; step 2 has no alpha (its caller passes 0).
static int lm_error(povar_ctx* c, int step, double alpha, povar_residual_info* out) {
  TimeScope ts(c, 4);
  if (step == 1) set_alpha(c, alpha);
  if (err_memo_hit(c, step, alpha, out)) return 0;
  if (int rc = clear_flag0(c)) return rc;
  const bool lpl = lpl_mode(c);
  if (lpl) {
    ensure_lmx(c);
    launch_lpl_pass(c, step, 1);
  } else if (step == 1) {
    launch_lm(c, OpError{});
  } else {
    launch_lm(c, OpErrorH{});
  }
  // step 1: error, residual sum, count; step 2: the same over all observations, then over the valid projections
  const int n = step == 1 ? 3 : 6;
  if (step == 1) reduce_sums<3>(c, lpl);
  else reduce_sums<6>(c, lpl);
  HIP_TRY(hipGetLastError());
  if (int rc = allreduce(c, c->scal.p, n)) return rc;
  double h[6];
  int f[4];
  if (int rc = read_scal_flags(c, h, n, f)) return rc;
  c->flag0_clean = f[0] == 0;
  if (int rc = combine_flag(c, &f[0])) return rc;
  const int v = step == 1 ? 0 : 3;  // projection_valid is always true on pOSE (helper.cpp:263)
  out->all_error = h[0];
  out->all_residual_sum = h[1];
  out->all_num_obs = (int64_t)std::llround(h[2]);
  out->valid_error = h[v];
  out->valid_residual_sum = h[v + 1];
  out->valid_num_obs = (int64_t)std::llround(h[v + 2]);
  out->is_numerically_valid = f[0] ? 0 : 1;
  err_memo_store(c, step, alpha, *out);
  return 0;
}

static int lm_linearize(povar_ctx* c, int step, double alpha) {
  if (int rc = res_verify(c)) return rc;
  if (step == 1) {  // (step 2 has no alpha, and clears the other step's linearisation only at its end)
    c->linearized_h = false;
    set_alpha(c, alpha);
    c->alpha_lin = alpha;
  }
  if (int rc = swap_in_placed_rows(c, false); rc < 0) return rc;  // a new linearisation point: the row order may change
  TimeScope ts(c, 0);
  if (int rc = clear_flag0(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->cams_lin4.p, c->cams4.p, sizeof(double4) * 3 * c->n_cams, hipMemcpyDeviceToDevice, c->stream));
  ++c->lin_id;
  (step == 1 ? c->linearized : c->linearized_h) = true;
  // lane-per-landmark mode: one forward walk over the row stream; the per-slot arrays and the camera-major landmark
  // copies of the lane-per-observation kernels are built when one of them asks (ensure_legacy)
  const bool lazy = lpl_only(c);
  const int hom = step == 1 ? 0 : 1;
  Dp dl = c->d;  // the camera-major kernels of this call read the linearisation point where it is now
  if (lazy) {
    // the kernel reads the current lane-ordered mirror and leaves the linearisation point (V2::lml) and the scale
    // mirror behind; the landmark-order copies lms_lin4 and jl_scale4 follow when a lane-per-observation kernel asks
    // (ensure_legacy): until then the current landmarks ARE the linearisation point
    ensure_lmx(c);
    c->lml_lin_id = c->lsc_lin_id = c->lin_id;
    launch_lpl_pass(c, step, 0);
    if (!c->has_empty_lm) dl.lms_lin4 = c->lms4.p;
  }
  if (!lazy || c->has_empty_lm) {
    HIP_TRY(hipMemcpyAsync(c->lms_lin4.p, c->lms4.p, sizeof(double4) * c->n_lms, hipMemcpyDeviceToDevice, c->stream));
    c->lmslin_lin_id = c->lin_id;
  }
  if (!lazy) {
    if (step == 1) launch_lm(c, OpLinearize{});
    else launch_lm(c, OpLinearizeH{});
    c->aux_lin_id = c->jls_lin_id = c->lin_id;
    build_views(c);
  }
  if (c->n_cold3 > 0)
    hipLaunchKernelGGL(cm_build_h, dim3(grid_for(c->n_cold3, 256)), dim3(256), 0, c->stream, dl, (const int*)c->c3_lm.p, c->c3_h.p, c->n_cold3, hom);
  hipLaunchKernelGGL((step == 1 ? cm_gram : cm_gram_h), dim3(grid_for(c->n_items, 4)), dim3(256), 0, c->stream, dl, lazy ? 1 : 0);
  const auto finish = [&](const double* G) {
    if (step == 1) hipLaunchKernelGGL(cam_finish_linearize, dim3(c->n_cams), dim3(CFL_THREADS), 0, c->stream, c->d, G);
    else hipLaunchKernelGGL(cam_finish_linearize_h, dim3(c->n_cams), dim3(CFL_THREADS), 0, c->stream, c->d, G, c->ncw.p);
  };
  finish(nullptr);
  if (sharded(c)) {
    // per-camera Gram moments are partial sums over this rank's landmarks: sum, all-reduce, finish
    if (int rc = allreduce(c, c->d.G, 40 * (size_t)c->n_cams)) return rc;
    finish(c->d.G);
  }
  HIP_TRY(hipGetLastError());
  int f[4];
  if (int rc = read_flags(c, f)) return rc;
  c->flag0_clean = f[0] == 0;
  if (int rc = combine_flag(c, &f[0])) return rc;
  c->new_linearization_point = true;
  (step == 1 ? c->linearized : c->linearized_h) = true;
  if (step == 2) c->linearized = false;  // the step-1 linearisation is gone (step 1 dropped step 2's before the row swap)
  c->tiles_valid = false;
  return f[0] ? POVAR_NUMERIC_FAILURE : 0;
}

static int lm_prepare(povar_ctx* c, int step, double lambda, int32_t solver_type) {
  if (int rc = res_verify(c)) return rc;
  if (int rc = check_linearized(c, step, step == 1 ? "povar_prepare_pose" : "povar_prepare_joint")) return rc;
  if (step == 1) set_alpha(c, c->alpha_lin);
  c->joint = step == 2;
  ++c->prep_id;
  c->prep_lin_id = c->lin_id;
  TimeScope ts(c, 1);
  // scale_Jp_cols_pOSE on a new linearisation point (linearizor_power_varproj.cpp:192-195):
  // the scaling is part of the implicit tile; only stored tiles need (re)materialising.
  c->new_linearization_point = false;
  // step 1: cpp:197-200; step 2: set_landmark_damping_joint, linearizor_power_varproj.cpp:136
  c->d.lambda_lm = step == 2 || solver_type == POVAR_POWER_SCHUR_COMPLEMENT ? lambda : 0.0;
  const int hom = step == 1 ? 0 : 1;
  const double* ncw = c->ncw.p;
  hipLaunchKernelGGL(build_hot_rec, dim3(grid_for((int64_t)c->n_cams * 12, 256)), dim3(256), 0, c->stream, c->d, hom);
  if (lpl_only(c)) {
    // lane-per-landmark K7 / K7': Hll^-1, landmark records and the per-camera partial sums of b in one kernel, then the
    // per-camera sum of the partials and the cold observations (same kernel as the per-term one): into b (step 1), or
    // into the ambient 12-vector y and through the tangent projection N_c^T (step 2)
    Dp da = ldsacc_dp(c, true);
    da.prep_lpl_only = 1;
    ensure_lin_mirrors(c);
    // cam_cold_sum honours the series-done flag of the term loop: clear what an early exit of the last solve left
    HIP_TRY(hipMemsetAsync(c->flags.p + 1, 0, sizeof(int) * 3, c->stream));
    launch_prepare_lpl(c, step, da);
    da.y = step == 1 ? c->d.b : c->d.y;
    da.p2p_peer = nullptr;  // b goes through the ordinary exchange below, not the per-term push
    da.p2p_epoch = nullptr;
    hipLaunchKernelGGL(cam_cold_sum<CCS_THREADS>, dim3(c->n_cams), dim3(CCS_THREADS), 0, c->stream, da, hom);
    if (step == 2)
      hipLaunchKernelGGL(cam_nt_project, dim3(grid_for(c->n_cams, 256)), dim3(256), 0, c->stream, c->d, c->d.y, c->d.b, ncw);
    else if (c->fp32_terms)
      launch_ck32_records(c);  // (POVAR_FLAG_FP32_TERMS: the fp32 operands of e0_ck_f32)
  } else {
    c->aux_prep_id = c->prep_id;  // this branch writes them
    ensure_legacy(c);
    if (step == 1) launch_lm(c, OpPrepare{});
    else launch_lm(c, OpPrepareH{});
    hipLaunchKernelGGL(cm_scatter, dim3(grid_for(c->n_items, 4)), dim3(256), 0, c->stream, c->d, 0, hom);
    if (step == 1) hipLaunchKernelGGL(cam_sum_items, dim3(grid_for(c->n_cams, 4)), dim3(256), 0, c->stream, c->d, c->d.b, 1);
    else hipLaunchKernelGGL(cam_sum_items_h, dim3(grid_for(c->n_cams, 4)), dim3(256), 0, c->stream, c->d, c->d.b, ncw);
  }
  if (int rc = allreduce(c, c->d.b, (step == 1 ? 12 : 11) * (size_t)c->n_cams)) return rc;
  const dim3 k8_grid(grid_for(c->n_cams, K8_CAMS_PER_WG));
  if (c->fixed_dirty) {  // povar_set_fixed_cameras since the last preparation: this system is the first to see the set
    HIP_TRY(hipMemcpyAsync(c->fixed_mask.p, c->fixed_next.data(), c->fixed_next.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (fixed_next is pageable and may be rewritten by the caller's next call)
    c->n_fixed = (int)std::count(c->fixed_next.begin(), c->fixed_next.end(), (uint8_t)1);
    c->fixed_dirty = false;
    c->cam_row_dirty = true;
  }
  // the map of the dense matrix follows the set, the mode (povar_set_dense_compaction) and the step's dim
  const int map_dim = step == 1 ? 12 : 11;
  if (c->cam_row_dirty || c->compaction != c->compaction_next || c->cam_row_dim != map_dim) {
    c->cam_row_n = cam_row_map(c->fixed_next.data(), c->n_cams, map_dim, c->compaction_next, c->cam_row_host);
    if (c->n_cams > 0) {
      HIP_TRY(hipMemcpyAsync(c->cam_row.p, c->cam_row_host.data(), c->cam_row_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));  // (pageable, as fixed_next)
    }
    c->compaction = c->compaction_next;
    c->cam_row_dim = map_dim;
    c->cam_row_dirty = false;
  }
  const uint8_t* fixed = c->fixed_mask.p;
  if (step == 1) hipLaunchKernelGGL(cam_build_binv, k8_grid, dim3(K8_THREADS), 0, c->stream, c->d, lambda, fixed);
  else hipLaunchKernelGGL(cam_build_binv_h, k8_grid, dim3(K8_THREADS), 0, c->stream, c->d, lambda, ncw, fixed);
  if (step == 1)  // (only step 1 has stored tiles)
    if (int rc = ensure_tiles(c)) return rc;
  // the one-off choice between the term kernels is part of the preparation, not of the first solve's time
  // (solve_reduced_system_time of the caller's log: bal_bundle_adjustment.cpp:355-360)
  if (int rc = ck_autotune(c, step)) return rc;
  if (int rc = tune_agree(c, step - 1)) return rc;
  HIP_TRY(hipGetLastError());
  return 0;
}

// apply, shared pieces: the back-substitution on the lane-per-landmark layout (it keeps the lane-ordered landmark
// mirror current) or by the lane-per-observation operator ...
template <class Op>
static void lm_backsub(povar_ctx* c, int step, bool lpl, const Op& legacy) {
  if (lpl) {
    const Dp da = ldsacc_dp(c, true);
    ensure_lmx(c);
    ensure_lin_mirrors(c);
    launch_backsub_lpl(c, step, da);
  } else {
    ensure_legacy(c);
    launch_lm(c, legacy);
  }
}

// ... and the tail: the state has moved, the model decrease of the landmarks comes back
static int lm_apply_tail(povar_ctx* c, bool lpl_back, double* l_diff) {
  state_written(c, lpl_back);
  reduce_sums<1>(c, lpl_back);
  HIP_TRY(hipGetLastError());
  if (int rc = allreduce(c, c->scal.p, 1)) return rc;
  double h = 0;
  if (int rc = read_scal(c, &h, 1)) return rc;
  if (l_diff) *l_diff = h;
  return 0;
}

extern "C" {

int povar_set_cameras(povar_ctx* c, const double* cams) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->cams4.p, cams, sizeof(double) * 12 * c->n_cams, hipMemcpyHostToDevice, c->stream));
  ++c->cams_ver;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int povar_get_cameras(povar_ctx* c, double* cams) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipMemcpyAsync(cams, c->cams4.p, sizeof(double) * 12 * c->n_cams, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int povar_set_landmarks(povar_ctx* c, const double* lms) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->stage.p, lms, sizeof(double) * 3 * c->n_lms, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(lms3_to_4, dim3(grid_for(c->n_lms, 256)), dim3(256), 0, c->stream, c->stage.p,
                     c->lms4.p, c->n_lms);
  ++c->lms_ver;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int povar_get_landmarks(povar_ctx* c, double* lms) {
  if (int rc = check_ctx(c)) return rc;
  hipLaunchKernelGGL(lms4_to_3, dim3(grid_for(c->n_lms, 256)), dim3(256), 0, c->stream, c->lms4.p,
                     c->stage.p, c->n_lms);
  HIP_TRY(hipMemcpyAsync(lms, c->stage.p, sizeof(double) * 3 * c->n_lms, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int povar_backup_pose(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->cams_bak4.p, c->cams4.p, sizeof(double4) * 3 * c->n_cams, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->lms_bak4.p, c->lms4.p, sizeof(double4) * c->n_lms, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int povar_restore_pose(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->cams4.p, c->cams_bak4.p, sizeof(double4) * 3 * c->n_cams, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->lms4.p, c->lms_bak4.p, sizeof(double4) * c->n_lms, hipMemcpyDeviceToDevice, c->stream));
  state_written(c, false);
  return 0;
}

int povar_init_landmarks_pose(povar_ctx* c, double alpha) {
  if (int rc = check_ctx(c)) return rc;
  ++c->lms_ver;
  set_alpha(c, alpha);
  TimeScope ts(c, 4);
  if (c->k1_qr) {
    hipLaunchKernelGGL(init_landmarks_qr, dim3(grid_for(c->n_lms, 256)), dim3(256), 0, c->stream, c->d);
  } else {
    launch_lm(c, OpInit{});
    launch_lm(c, OpInitRefine{});
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int povar_error_pose(povar_ctx* c, double alpha, povar_residual_info* out) {
  if (int rc = check_ctx(c)) return rc;
  if (!out) return fail(-1, "null argument");
  return lm_error(c, 1, alpha, out);
}

int povar_linearize_pose(povar_ctx* c, double alpha) {
  if (int rc = check_ctx(c)) return rc;
  return lm_linearize(c, 1, alpha);
}

int povar_prepare_pose(povar_ctx* c, double lambda, int32_t solver_type) {
  if (int rc = check_ctx(c)) return rc;
  return lm_prepare(c, 1, lambda, solver_type);
}

int povar_apply_pose(povar_ctx* c, int32_t solver_type, double alpha, const double* inc, double* l_diff) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = res_verify(c)) return rc;  // (step 1 only: povar_apply_joint does not look)
  if (int rc = check_linearized(c, 1, "povar_apply_pose")) return rc;
  const size_t n = 12 * (size_t)c->n_cams;
  set_alpha(c, alpha);
  TimeScope ts(c, 3);
  if (int rc = write_cam_vector(c, c->inc.p, inc, n)) return rc;
  bool lpl_back = false;
  if (solver_type == POVAR_POWER_VARPROJ) {
    // cpp:250-256: scale, update cameras, unscale, back-substitute at the new cameras
    hipLaunchKernelGGL(cam_apply_inc, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->d, 0);
    lpl_back = lpl_only(c);
    lm_backsub(c, 1, lpl_back, OpBackVarproj{});
  } else {
    // cpp:260-270: back-substitute with the stored tiles, then update cameras
    hipLaunchKernelGGL(cam_apply_inc, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->d, 1);
    lm_backsub(c, 1, false, OpBackPoba{});
    hipLaunchKernelGGL(cam_apply_inc, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->d, 2);
  }
  return lm_apply_tail(c, lpl_back, l_diff);
}

// ------------------------------------------------------------------------------------------
// step 2
// ------------------------------------------------------------------------------------------
int povar_set_landmarks_homogeneous(povar_ctx* c, const double* lms_h) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->lms4.p, lms_h, sizeof(double) * 4 * c->n_lms, hipMemcpyHostToDevice, c->stream));
  ++c->lms_ver;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int povar_get_landmarks_homogeneous(povar_ctx* c, double* lms_h) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipMemcpyAsync(lms_h, c->lms4.p, sizeof(double) * 4 * c->n_lms, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int povar_backup_joint(povar_ctx* c) { return povar_backup_pose(c); }

int povar_restore_joint(povar_ctx* c) { return povar_restore_pose(c); }

int povar_error_homogeneous(povar_ctx* c, povar_residual_info* out) {
  if (int rc = check_ctx(c)) return rc;
  if (!out) return fail(-1, "null argument");
  return lm_error(c, 2, 0.0, out);
}

int povar_linearize_homogeneous(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  return lm_linearize(c, 2, 0.0);
}

int povar_prepare_joint(povar_ctx* c, double lambda) {
  if (int rc = check_ctx(c)) return rc;
  return lm_prepare(c, 2, lambda, 0);
}

int povar_apply_joint(povar_ctx* c, const double* inc, double* l_diff) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = check_linearized(c, 2, "povar_apply_joint")) return rc;
  TimeScope ts(c, 3);
  HIP_TRY(hipMemcpyAsync(c->inc.p, inc, sizeof(double) * 11 * c->n_cams, hipMemcpyHostToDevice, c->stream));
  // cpp:280: back-substitute first (old cameras), then update the cameras (cpp:283-305)
  const bool lpl_back = lpl_only(c);
  if (lpl_back)  // the record image: P of the linearisation point (12..23), then z = sigma * N_c inc by cam_apply_inc_h (0..11)
    hipLaunchKernelGGL(build_hot_rec, dim3(grid_for((int64_t)c->n_cams * 12, 256)), dim3(256), 0, c->stream, c->d, 1);
  hipLaunchKernelGGL(cam_apply_inc_h, dim3(grid_for(c->n_cams, 256)), dim3(256), 0, c->stream, c->d, 1, (const double*)c->ncw.p);
  lm_backsub(c, 2, lpl_back, OpBackJoint{});
  hipLaunchKernelGGL(cam_apply_inc_h, dim3(grid_for(c->n_cams, 256)), dim3(256), 0, c->stream, c->d, 2, (const double*)c->ncw.p);
  return lm_apply_tail(c, lpl_back, l_diff);
}

int povar_normalize_joint(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  // the lane-ordered mirror of the landmarks, when current, is normalised along (same division, same operands)
  const bool mirror = c->use_lpl && c->lmx_ver == c->lms_ver && c->d.v2.n_tiles > 0;
  const int64_t n_lanes = mirror ? (int64_t)c->d.v2.n_tiles * WAVE : 0;
  hipLaunchKernelGGL(normalize_joint, dim3(grid_for(std::max<int64_t>(std::max(c->n_cams, c->n_lms), n_lanes), 256)), dim3(256), 0,
                     c->stream, c->d, n_lanes);
  state_written(c, mirror);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the leading `dim` doubles of every camera's block of a [n_cams][144] device array
static int read_cam_blocks(povar_ctx* c, const double* src, size_t dim, double* out) {
  const size_t nc = c->n_cams;
  std::vector<double> h(144 * nc);
  HIP_TRY(hipMemcpyAsync(h.data(), src, 144 * nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t k = 0; k < nc; ++k) std::memcpy(out + dim * k, h.data() + 144 * k, dim * sizeof(double));
  return 0;
}

int povar_get_buffer(povar_ctx* c, int32_t which, double* out, int64_t n) {
  if (int rc = check_ctx(c)) return rc;
  ensure_legacy(c);  // exports rebuild the reference's tile from the per-slot arrays
  const size_t nc = c->n_cams, nl = c->n_lms;
  auto copy = [&](const void* src, size_t count) -> int {
    if ((size_t)n != count) return fail(-1, "povar_get_buffer: wrong size");
    HIP_TRY(hipMemcpyAsync(out, src, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  };
  switch (which) {
    case POVAR_BUF_DIAG2: return copy(c->diag2.p, 12 * nc);
    case POVAR_BUF_POSE_SCALING: return copy(c->sigma.p, 12 * nc);
    case POVAR_BUF_HLL_INV: return copy(c->hll_inv.p, 9 * nl);
    case POVAR_BUF_B: return copy(c->b.p, 12 * nc);
    case POVAR_BUF_B_INV: return copy(c->binv.p, 144 * nc);
    case POVAR_BUF_B_JOINT: return copy(c->b.p, 11 * nc);
    case POVAR_BUF_B_INV_JOINT:
      if ((size_t)n != 121 * nc) return fail(-1, "povar_get_buffer: wrong size");
      return read_cam_blocks(c, c->binv.p, 121, out);
    case POVAR_BUF_NC_HOUSEHOLDER: return copy(c->ncw.p, 13 * nc);
    case POVAR_BUF_SC_PRECOND:
    case POVAR_BUF_SC_BLOCKDIAG: {
      const size_t dim2 = c->joint ? 121 : 144;
      if ((size_t)n != dim2 * nc) return fail(-1, "povar_get_buffer: wrong size");
      if (!c->sc_s.p) return fail(-1, "povar_get_buffer: no explicit-SC solve yet");
      return read_cam_blocks(c, which == POVAR_BUF_SC_PRECOND ? c->sc_minv.p : c->sc_bmat.p, dim2, out);
    }
    case POVAR_BUF_SC_FACTOR: {
      if (c->sc_factor_dim == 0 || !c->sc_dense.p || !c->sc_xpad.p)
        return fail(-1, "povar_get_buffer: POVAR_BUF_SC_FACTOR: no factor in place (the last call that wrote the dense matrix "
                        "must be a CHOLESKY / RICHOLESKY solve that found it positive definite)");
      const DenseDims g = dense_dims(c->sc_factor_dim, c->sc_factor_n / c->sc_factor_dim);  // (the cameras in that matrix)
      const size_t N = g.N, ld = g.ld;
      if ((size_t)n != N * (N + 2)) return fail(-1, "povar_get_buffer: wrong size");
      std::vector<double> xh(N);
      HIP_TRY(hipMemcpy2DAsync(out, (N + 2) * sizeof(double), c->sc_dense.p, ld * sizeof(double), (N + 1) * sizeof(double), N,
                               hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(xh.data(), c->sc_xpad.p, N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      for (size_t i = 0; i < N; ++i) out[i * (N + 2) + N + 1] = xh[i];
      return 0;
    }
    case POVAR_BUF_COV_FACTOR:
    case POVAR_BUF_COV_INVERSE:
    case POVAR_BUF_COV_PANEL:
    case POVAR_BUF_COV_GAUGE: {
      if (c->cov.kind == 0 || !c->sc_dense.p)
        return fail(-1, "povar_get_buffer: POVAR_BUF_COV_*: no covariance in place (the last call that wrote the dense matrix "
                        "must be a povar_*_covariance_* call that returned 0)");
      const DenseDims g = dense_dims(1, c->cov.n);  // (cov.n: the rows of that call's matrix; the geometry depends on them alone)
      const size_t N = g.N, ld = g.ld;
      if (which == POVAR_BUF_COV_GAUGE) {
        if (c->cov.nq == 0 || !c->cov.q.p) return fail(-1, "povar_get_buffer: POVAR_BUF_COV_GAUGE: the last covariance call was damped");
        return copy(c->cov.q.p, (size_t)c->cov.n * (size_t)c->cov.nq);
      }
      if (which == POVAR_BUF_COV_PANEL) {
        if (c->cov.kind != 2 || !c->cov.panel.p)
          return fail(-1, "povar_get_buffer: POVAR_BUF_COV_PANEL: the last covariance call was not a landmark call with landmarks");
        return copy(c->cov.panel.p, N * CH_NB);
      }
      if (which == POVAR_BUF_COV_FACTOR && (!c->cov.kept || !c->cov.r.p))
        return fail(-1, "povar_get_buffer: POVAR_BUF_COV_FACTOR: povar_set_cov_inspect was off during the last covariance call");
      if ((size_t)n != N * N) return fail(-1, "povar_get_buffer: wrong size");
      if (which == POVAR_BUF_COV_FACTOR)
        HIP_TRY(hipMemcpyAsync(out, c->cov.r.p, N * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      else
        HIP_TRY(hipMemcpy2DAsync(out, N * sizeof(double), c->sc_dense.p, ld * sizeof(double), N * sizeof(double), N, hipMemcpyDeviceToHost,
                                 c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      return 0;
    }
    case POVAR_BUF_JL_COL_SCALE_H: {
      if ((size_t)n != 4 * nl) return fail(-1, "povar_get_buffer: wrong size");
      HIP_TRY(hipMemcpyAsync(out, c->jl_scale4.p, nl * sizeof(double4), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      return 0;
    }
    case POVAR_BUF_JL_COL_SCALE: {
      if ((size_t)n != 3 * nl) return fail(-1, "povar_get_buffer: wrong size");
      std::vector<double4> h(nl);
      HIP_TRY(hipMemcpyAsync(h.data(), c->jl_scale4.p, nl * sizeof(double4), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      for (size_t l = 0; l < nl; ++l) {
        out[3 * l] = h[l].x;
        out[3 * l + 1] = h[l].y;
        out[3 * l + 2] = h[l].z;
      }
      return 0;
    }
    case POVAR_BUF_STORAGE: {
      if ((size_t)n != 64 * (size_t)c->n_obs) return fail(-1, "povar_get_buffer: wrong size");
      if (!c->linearized) return fail(-1, "not linearized");
      set_alpha(c, c->alpha_lin);
      const size_t cnt = (size_t)c->n_bins * TILE_PAIRS * WAVE;
      DevBuf<double2> tmp_tiles;  // (not the context's: uncounted, freed on every return)
      Dp d = c->d;
      if (!c->tiles.p) {
        HIP_TRY(tmp_tiles.alloc(cnt, nullptr));
        d.tiles = tmp_tiles.p;
      }
      hipLaunchKernelGGL(materialize_tiles, dim3(grid_for(c->n_slots, LM_BLOCK)), dim3(LM_BLOCK), 0, c->stream, d);
      std::vector<double2> h(cnt);
      HIP_TRY(hipMemcpyAsync(h.data(), d.tiles, cnt * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (!tmp_tiles.p) c->tiles_valid = true;
      tmp_tiles.release();
      // blocked [bin][pair][lane] -> reference rows [4*obs + r][16] = [Jp(12) | Jl(3) | r]
      for (int64_t i = 0; i < c->n_obs; ++i) {
        const int s = c->slot_of_obs[i];
        const double2* t = h.data() + ((size_t)(s >> 6) * TILE_PAIRS) * WAVE + (s & 63);
        double v[64];
        for (int p = 0; p < TILE_PAIRS; ++p) {
          v[2 * p] = t[(size_t)p * WAVE].x;
          v[2 * p + 1] = t[(size_t)p * WAVE].y;
        }
        for (int r = 0; r < 4; ++r) {
          double* row = out + ((size_t)4 * i + r) * 16;
          for (int j = 0; j < 12; ++j) row[j] = v[12 * r + j];
          for (int j = 0; j < 3; ++j) row[12 + j] = v[48 + 3 * r + j];
          row[15] = v[60 + r];
        }
      }
      return 0;
    }
    default:
      return fail(-1, "povar_get_buffer: unknown buffer");
  }
}

}  // extern "C"
