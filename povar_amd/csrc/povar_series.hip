// povar_series.hip -- the term loop: the term's plan and its launcher, kernel choice by timing, hipGraph capture, the power-series entry points.
#include "povar_ctx.hpp"

static CkP ck_params(const povar_ctx* c, const povar_ctx::CkDev& D) {
  return CkP{D.packed ? reinterpret_cast<const double2*>(D.uvp.p) : D.uv.p, D.li.p, D.w.p, D.tile.p, D.lane_meta.p, D.bt_off.p, D.slot_rec.p,
             D.nb, D.slots, (unsigned)(D.src.n * (D.packed ? sizeof(int2) : sizeof(double2))), (unsigned)(D.li.n * sizeof(uint32_t)),
             D.lcnt.p, D.tick.p, D.max_acc, D.packed ? 1 : 0, D.cold_q ? D.cpos.p : nullptr, c->q4c.p,
             D.first_meta.p, D.first_hdr.p};
}

// an instantiation runs a layout whose batches fit its groups: the LDS holds ng batches at once
static bool ck_variant_fits(const povar_ctx* c, int variant) {
  const CkVariant v = ck_variant_info(variant);
  return c->ck.ready && c->ck.nb % v.ng == 0 && ck_lds_bytes(c->ck.slots, c->ck.max_acc, v.ng) <= (size_t)CK_LDS_BYTES;
}

// The kernels of one application of E0 for the system of `step` (1: pose, 2: joint), decided from the context's mode, layouts
// and switches.  variant >= 0 puts that camera-chunk choice in place of the context's (0: the lane-per-landmark kernel).
TermPlan term_plan(const povar_ctx* c, int step, TermUse use, int variant) {
  TermPlan p;
  p.step = step;
  p.use = use;
  const int mode = c->opt.e0_mode;
  const bool lpl = lpl_mode(c);
  const bool series = use == TermUse::series || use == TermUse::series_norms;
  if (step == 1) {
    if (variant < 0) variant = c->ck_variant;
    const povar_ctx::CkDev& D = c->ck;
    if (c->fp32_terms && use != TermUse::dense) {
      // POVAR_FLAG_FP32_TERMS: e0_ck_f32 on the chunk layout povar_create built for it (it refuses the flag where that layout
      // cannot be built; setters that would leave it refuse too); the explicit-SC solvers stay in fp64
      if (!c->deterministic && D.ready && lpl && c->ck32_lmrec.p && c->ck32_pimg.p && (D.packed || c->ck32_uv.p) &&
          ck32_lds_bytes(D.slots, D.max_acc) <= (size_t)CK_LDS_BYTES) {
        p.e0 = E0K::ck_f32;
        p.variant = variant;
      }
    } else if (c->deterministic) {
      // POVAR_DETERMINISTIC: the context is in the gather mode -- its linearisation and preparation kernels have no atomics --
      // and the terms run the fixed-point form of e0_ck on the records those kernels leave in lane order
      if (c->det_ck && D.ready && D.lcnt.p && D.tick.p && c->use_lpl && mode == POVAR_E0_IMPLICIT && D.nb >= 1 &&
          ck_lds_bytes_det(D.slots, D.max_acc) <= (size_t)CK_LDS_BYTES)
        p.e0 = E0K::ck_det;
    } else if (variant > 0 && D.ready && lpl && ck_variant_fits(c, variant)) {
      p.e0 = E0K::ck;
      p.variant = variant;
    }
    if (!p.ck()) {
      // (the lane-per-observation kernels of the LDS-accumulating mode walk the long landmarks themselves where
      // long_in_kernel; e0_lpl has no long/short distinction)
      const bool walks_long = mode == POVAR_E0_IMPLICIT_LDSACC && c->long_in_kernel;
      p.e0 = mode == POVAR_E0_TILES ? E0K::lm_tiles : mode == POVAR_E0_TILES_LDSACC ? E0K::tiles_cached
             : lpl ? E0K::lpl : mode == POVAR_E0_IMPLICIT_LDSACC ? E0K::lm_cached_acc : E0K::lm_cached;
      p.long_after = c->n_long > 0 && (mode == POVAR_E0_TILES || mode == POVAR_E0_TILES_LDSACC || !walks_long);
    }
  } else {
    if (variant < 0) variant = c->ckh_variant;
    const povar_ctx::CkDev& D = c->ckh;
    if (c->deterministic) {
      if (c->det_ck && D.ready && D.lcnt.p && D.tick.p && c->use_lpl && mode == POVAR_E0_IMPLICIT && D.stride == CKH_STRIDE &&
          D.slots <= CKH_STRIDE && ckh_lds_bytes_det(D.max_acc) <= (size_t)CK_LDS_BYTES)
        p.e0 = E0K::ck_h_det;
    } else if (variant > 0 && D.ready && lpl && (D.stride == CKH_STRIDE || D.stride == CKH_STRIDE_WIDE) &&
               D.slots <= D.stride && ckh_lds_bytes(D.max_acc, D.stride) <= (size_t)CK_LDS_BYTES) {
      p.e0 = E0K::ck_h;
      p.variant = 1;
    }
    if (!p.ck()) {
      p.e0 = lpl ? E0K::lpl_h : mode == POVAR_E0_IMPLICIT_LDSACC ? E0K::lm_cached_h : E0K::lm_h;
      p.long_after = c->n_long > 0 && (p.e0 == E0K::lm_h || (p.e0 == E0K::lm_cached_h && !c->long_in_kernel));
    }
  }
  // the LDS-accumulating kernels (and the camera-chunk kernels, the fixed-point ones included) leave partial records and a
  // cold view to cam_cold_sum; the unsharded term loop may run B^-1 + AXPY inside it.  What is timed is that fused pair.
  const bool acc = p.ck() || mode == POVAR_E0_IMPLICIT_LDSACC || (step == 1 && mode == POVAR_E0_TILES_LDSACC);
  if (acc)
    p.cam = use == TermUse::timing || (series && !sharded(c) && c->fuse_binv) ? CamStep::fused : CamStep::sum;
  else
    p.cam = sharded(c) ? CamStep::scatter_sum : CamStep::scatter;
  // peer-to-peer exchange: only inside the term loop of the step-1 lane-per-landmark kernels; every other caller wants the
  // dense, all-reduced y
  if (series && step == 1 && c->p2p && lpl && p.cam == CamStep::sum) p.exch = Exch::p2p;
  else if (use != TermUse::timing && sharded(c)) p.exch = Exch::allreduce;
  return p;
}

// the per-camera kernels behind e0_ck / e0_ck_h: partial records only (its own table), no per-observation cold view
static void ck_dp(const povar_ctx* c, int step, Dp& da) {
  const povar_ctx::CkDev& D = step == 2 ? c->ckh : c->ck;
  da.hot_part = D.part.p;
  da.part_range = D.part_range.p;
  da.cmv.src = nullptr;
  da.q_rows = 0;
  if (D.cold_q) return;  // e0_ck's cold lanes left q in the lane-per-landmark layout's cold view (camera-major, at their own
                         // positions): the per-camera kernel walks it as it does behind e0_lpl (ldsacc_dp has set h, n, cam_range, q4c)
  da.cmv.cam_range = c->ck_zero_range.p;
  da.cmv.n = 0;
}

// instantiations: wavefronts per workgroup, rows per chunk, chunks per lane, landmark slots per lane.  1024-thread
// workgroups (128 VGPRs per lane): one chunk of at most two rows; 512-thread ones (256): two chunks of up to four rows
#define POVAR_RES_VARIANTS(X) X(16, 1, 1, 1) X(16, 2, 1, 1) X(8, 1, 2, 1) X(8, 1, 2, 2) X(8, 2, 2, 1) X(8, 2, 2, 2) X(8, 4, 2, 1) X(8, 4, 2, 2)
// series_res_h: a table of its own -- the shapes whose code objects use no scratch (profiles/res_joint_isa.txt).  The two
// 1024-thread shapes are not in it: P_c (24 registers per chunk instead of P3's 18), s and Hll^-1 (20 per landmark slot
// instead of G's 12) and house4 between the passes do not fit 128 registers (7 to 21 spilt), so step 2 cuts its instance
// for 512-thread workgroups (res_build_for)
#define POVAR_RES_H_VARIANTS(X) X(8, 1, 2, 1) X(8, 1, 2, 2) X(8, 2, 2, 1) X(8, 2, 2, 2) X(8, 4, 2, 1) X(8, 4, 2, 2)
// the kernel of a step and shape
template <bool JOINT, int NW, int H, int RR, int LS, bool ROBUST>
const void* res_kernel() {
  if constexpr (JOINT) return (const void*)series_res_h<NW, H, RR, LS, ROBUST>;
  else return (const void*)series_res<NW, H, RR, LS, ROBUST>;
}
template <bool JOINT, int NW, int H, int RR, int LS>
void launch_res_t(povar_ctx* c, const ResP& k) {
  const double* ncw = c->ncw.p;
  void* args[] = {(void*)&c->d, (void*)&k, (void*)&ncw};  // (series_res has the first two parameters, series_res_h all three)
  const void* f = c->opt.robust_norm ? res_kernel<JOINT, NW, H, RR, LS, true>() : res_kernel<JOINT, NW, H, RR, LS, false>();
  (void)hipLaunchKernel(f, dim3(k.W), dim3(NW * 64), args, JOINT ? c->res_h_lds : c->res.lds_bytes, c->stream);
}

bool res_variant_exists(int nw, int h, int rr, int ls, bool joint) {
#define X(NW_, H_, R_, LS_) if (nw == NW_ && h == H_ && rr == R_ && ls == LS_) return true;
  if (joint) {
    POVAR_RES_H_VARIANTS(X)
  } else {
    POVAR_RES_VARIANTS(X)
  }
#undef X
  return false;
}

void launch_res(povar_ctx* c, const ResP& k) {
  const povar_ctx::ResDev& D = res_dev(c, c->joint);
#define X(NW_, H_, R_, LS_)                                                  \
  if (D.NW == NW_ && D.H == H_ && D.R == R_ && D.LS == LS_) {                \
    launch_res_t<JOINT, NW_, H_, R_, LS_>(c, k);                             \
    return;                                                                  \
  }
  if (c->joint) {
    constexpr bool JOINT = true;
    POVAR_RES_H_VARIANTS(X)
  } else {
    constexpr bool JOINT = false;
    POVAR_RES_VARIANTS(X)
  }
#undef X
}

template <bool JOINT, int NW, int H, int RR, int LS>
hipError_t res_set_lds_t() {
  hipError_t e = hipFuncSetAttribute(res_kernel<JOINT, NW, H, RR, LS, false>(), hipFuncAttributeMaxDynamicSharedMemorySize, RES_LDS_BYTES);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute(res_kernel<JOINT, NW, H, RR, LS, true>(), hipFuncAttributeMaxDynamicSharedMemorySize, RES_LDS_BYTES);
}

hipError_t res_set_lds_all() {
  hipError_t e = hipSuccess;
#define X(NW_, H_, R_, LS_) if (e == hipSuccess) e = res_set_lds_t<JOINT, NW_, H_, R_, LS_>();
  { constexpr bool JOINT = false; POVAR_RES_VARIANTS(X) }
  { constexpr bool JOINT = true; POVAR_RES_H_VARIANTS(X) }
#undef X
  return e;
}

// the context can run the resident series of a step now (whether it SHOULD is res_mode / the timing of res_autotune).  A
// give-up in either step (res_failed) keeps both on the per-term kernels: the workgroups were not on the device together,
// which is the device's load and not the step's
bool res_possible(const povar_ctx* c, bool joint) {
  // (a communicator of ONE rank exchanges nothing: such a context -- the one-GPU proxy of a shard, tools/shard_sweep.sh --
  // is as good as unsharded; with peers the resident kernel would need their sums inside the launch: not built)
  return res_ready(c, joint) && !c->res_failed && c->opt.e0_mode == POVAR_E0_IMPLICIT_LDSACC && !c->profile &&
         (!sharded(c) || (c->world == 1 && !c->p2p));
}

bool res_active(const povar_ctx* c, bool joint) {
  const povar_ctx::ResTune& tn = c->res_tune[joint];
  return res_possible(c, joint) && (c->res_mode == 1 || (c->res_mode < 0 && tn.tuned && tn.choice));  // (and m <= 250: run_series' caller)
}

ResP res_params(const povar_ctx* c, int m, double q_tol, double r_tol) {
  const povar_ctx::ResDev& D = res_dev(c, c->joint);
  ResP k{};
  k.lane_cam = D.lane_cam.p; k.lane_seg = D.lane_seg.p;
  k.uv = D.uv.p; k.lslot = D.lslot.p; k.oslot = D.oslot.p; k.wave_h = D.wave_h.p;
  k.lm_off = D.lm_off.p; k.lm_id = D.lm_id.p; k.cam_off = D.cam_off.p; k.cam_id = D.cam_id.p; k.cam_zi = D.cam_zi.p;
  k.own_off = D.own_off.p; k.own_cam = D.own_cam.p; k.own_zi = D.own_zi.p; k.own_q = D.own_q.p;
  k.oq_off = D.oq_off.p; k.oq_rec = D.oq_rec.p;
  k.part = D.part.p; k.zbuf = D.zbuf.p; k.nrm = D.nrm.p; k.launch = D.launch.p;
  k.part_bytes = (unsigned)(D.part.n * sizeof(uint4)); k.z_bytes = (unsigned)(D.zbuf.n * sizeof(uint4)); k.nrm_bytes = (unsigned)(D.nrm.n * sizeof(uint4));
  k.W = D.W; k.m = m;
  k.want_norms = (q_tol > 0 || r_tol > 0) ? 1 : 0;
  k.want_norm0 = r_tol > 0 ? 1 : 0;
  // the robust weights of the linearisation in force: per slot (sqrt, lane-per-observation linearisation) or in row order
  k.w_mode = c->aux_lin_id == c->lin_id ? 2 : 1;
  k.q_tol = q_tol; k.r_tol = r_tol;
  k.spin_limit = c->res_spin_limit;
  return k;
}

// the whole series as one launch (+ the node that numbers the next one): series_res, or series_res_h for a joint system
int enqueue_series_res(povar_ctx* c, int32_t m, double q_tol, double r_tol) {
  HIP_TRY(hipMemsetAsync(c->flags.p + 1, 0, sizeof(int) * 3, c->stream));
  const ResP k = res_params(c, m, q_tol, r_tol);
  launch_res(c, k);
  hipLaunchKernelGGL(res_bump_launch, dim3(1), dim3(1), 0, c->stream, k.launch);
  return 0;
}

void prof_mark(povar_ctx* c, int kind) {
  if (!c->profile) return;
  if (c->ev_used == c->ev.size()) {
    hipEvent_t e;
    (void)hipEventCreate(&e);
    c->ev.push_back(e);
    c->ev_kind.push_back(-1);
  }
  c->ev_kind[c->ev_used] = kind;
  (void)hipEventRecord(c->ev[c->ev_used], c->stream);
  ++c->ev_used;
}

// Dp of the per-term kernels in POVAR_E0_IMPLICIT_LDSACC mode: cold camera-major view + hot partials
Dp ldsacc_dp(povar_ctx* c, bool long_in_kernel) {
  Dp dt = c->d;
  dt.cmv = CmView{c->cc_slot.p, c->cc_h.p, c->n_cold, c->cc_item_off.p, c->cc_cam_item_off.p, c->cc_part.p,
                  c->n_cold_items, c->cc_cam_range.p};
  dt.hot_part = c->hot_part.p;
  dt.q4c = c->q4c.p;
  dt.cold_pos = c->cold_pos.p;
  if (lpl_mode(c)) {
    // e0_lpl: its own cold view (observations whose camera is not resident in their workgroup) and partial records
    dt.cmv.h = c->c3_h.p;
    dt.cmv.n = c->n_cold3;
    dt.cmv.cam_range = c->c3_range.p;
    dt.cmv.src = c->q_rows ? c->rows.cold_src.p : nullptr;
    dt.q_rows = c->q_rows ? 1 : 0;
    dt.hot_part = c->v2_part.p;
    dt.part_range = c->v2_part_range.p;
    dt.cold_pos = nullptr;
    dt.long_in_kernel = 1;
    return dt;
  }
  if (long_in_kernel && c->long_in_kernel) {
    // view "A": e0_lm_cached<true> walks the long landmarks itself, their LDS-accumulated observations are not cold
    dt.cmv.h = c->c2_h.p;
    dt.cmv.n = c->n_cold2;
    dt.cmv.cam_range = c->c2_range.p;
    dt.cold_pos = c->c2_pos.p;
    dt.long_in_kernel = 1;
  }
  return dt;
}


// what the plan's kernels see: the context's Dp, or the cold view and partial records of the accumulating kernels
// (e0_tiles_cached: without the long landmarks' view), the chunk layout's records behind e0_ck*, the peers' buffers
static Dp term_dp(povar_ctx* c, const TermPlan& p) {
  if (p.cam == CamStep::scatter || p.cam == CamStep::scatter_sum) return c->d;
  Dp d = ldsacc_dp(c, p.e0 != E0K::tiles_cached);
  if (p.ck()) {
    ck_dp(c, p.step, d);
    if (p.step == 1) d.long_in_kernel = 1;  // (e0_ck walks every landmark)
  }
  if (p.exch == Exch::p2p) p2p_dp(c, d);
  return d;
}

template <int NW, int SD, bool DB, int NG>
void launch_e0_ck_t(povar_ctx* c, const Dp& da) {
  const CkP k = ck_params(c, c->ck);
  const size_t lds = ck_lds_bytes(c->ck.slots, c->ck.max_acc, NG);
  const bool huber = c->opt.robust_norm == POVAR_NORM_HUBER;  // (the kernel recomputes the weights; CAUCHY's are 1: compute_error_weight)
  if (c->ck.packed) {
    if (huber) hipLaunchKernelGGL((e0_ck<NW, SD, DB, NG, true, true>), dim3(c->e0c_grid), dim3(NW * 64), lds, c->stream, da, k, c->ck.part.p);
    else hipLaunchKernelGGL((e0_ck<NW, SD, DB, NG, false, true>), dim3(c->e0c_grid), dim3(NW * 64), lds, c->stream, da, k, c->ck.part.p);
  } else {
    if (huber) hipLaunchKernelGGL((e0_ck<NW, SD, DB, NG, true, false>), dim3(c->e0c_grid), dim3(NW * 64), lds, c->stream, da, k, c->ck.part.p);
    else hipLaunchKernelGGL((e0_ck<NW, SD, DB, NG, false, false>), dim3(c->e0c_grid), dim3(NW * 64), lds, c->stream, da, k, c->ck.part.p);
  }
}

// fp32 landmark records and camera image of the system prepared last (povar_prepare_pose, after prepare_lpl / build_hot_rec)
void launch_ck32_records(povar_ctx* c) {
  const int64_t n_rec = (int64_t)c->d.v2.n_tiles * 9 * WAVE;
  const int64_t n = std::max<int64_t>(n_rec, (int64_t)c->n_cams * 12);
  hipLaunchKernelGGL(ck32_records, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, (const double*)c->v2_lmrec.p, c->ck32_lmrec.p,
                     n_rec, (const double*)c->hot_rec.p, c->ck32_pimg.p, c->n_cams);
}

// robust weights in chunk order (V2::w is written by the linearisation walk in lane-per-landmark order)
static void ensure_ck_w(povar_ctx* c, int step) {
  povar_ctx::CkDev& D = step == 2 ? c->ckh : c->ck;
  if (!c->opt.robust_norm || !D.ready || !D.w.p || !c->v2_w.p || D.w_lin_id == c->lin_id) return;
  const int64_t n = (int64_t)D.src.n;  // every row, the padding included (weight 0)
  hipLaunchKernelGGL(ck_gather_w, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, (const int*)D.src.p, (const double*)c->v2_w.p,
                     D.w.p, n);
  D.w_lin_id = c->lin_id;
}

// E0 x for the current term, as the plan says: the E0 kernel [+ lm_long], the per-camera kernel, the exchange of y.  What
// cam_binv_axpy does next is plan.binv_mode().
int launch_e0(povar_ctx* c, const TermPlan& p) {
  if (p.use != TermUse::timing) prof_mark(c, 0);
  if (!lpl_mode(c)) ensure_legacy(c);  // cm_scatter / legacy cold views
  if (p.ck()) ensure_ck_w(c, p.step);  // (a no-op inside the graph capture: the solve entry points have called it before)
  const Dp da = term_dp(c, p);
  const bool robust = c->opt.robust_norm != 0, huber = c->opt.robust_norm == POVAR_NORM_HUBER;
  const dim3 grid(c->e0c_grid);
  switch (p.e0) {
    case E0K::ck_f32: {  // (povar_kernels_ck_f32.hpp: its partial records and cold-view q are e0_ck's, in fp64)
      const CkP k = ck_params(c, c->ck);
      const Ck32 f{c->ck.packed ? nullptr : c->ck32_uv.p, c->ck32_lmrec.p, c->ck32_pimg.p,
                   (unsigned)(c->ck.src.n * sizeof(float2)), (unsigned)(c->ck.part.n * sizeof(double))};
      const size_t lds = ck32_lds_bytes(c->ck.slots, c->ck.max_acc);
      const dim3 block(CK32_NW * 64);  // (HUBER's weights are recomputed in registers; CAUCHY's are 1, as in e0_ck)
      if (c->ck.packed) {
        if (huber) hipLaunchKernelGGL((e0_ck_f32<true, true>), grid, block, lds, c->stream, da, k, f, c->ck.part.p);
        else hipLaunchKernelGGL((e0_ck_f32<false, true>), grid, block, lds, c->stream, da, k, f, c->ck.part.p);
      } else {
        if (huber) hipLaunchKernelGGL((e0_ck_f32<true, false>), grid, block, lds, c->stream, da, k, f, c->ck.part.p);
        else hipLaunchKernelGGL((e0_ck_f32<false, false>), grid, block, lds, c->stream, da, k, f, c->ck.part.p);
      }
      break;
    }
    case E0K::ck_det: {  // the bit-reproducible form (povar_kernels_ck_det.hpp)
      const size_t lds = ck_lds_bytes_det(c->ck.slots, c->ck.max_acc);
      if (huber) hipLaunchKernelGGL((e0_ck_det<16, 2, true>), grid, dim3(1024), lds, c->stream, da, ck_params(c, c->ck), c->ck.part.p);
      else hipLaunchKernelGGL((e0_ck_det<16, 2, false>), grid, dim3(1024), lds, c->stream, da, ck_params(c, c->ck), c->ck.part.p);
      break;
    }
    case E0K::ck:
      switch (p.variant) {
#define X(id, nw, sd, db, ng) case id: launch_e0_ck_t<nw, sd, db, ng>(c, da); break;
        POVAR_CK_VARIANTS(X)
#undef X
        default: break;
      }
      break;
    case E0K::lm_cached:
      hipLaunchKernelGGL(e0_lm_cached<false>, grid, dim3(E0C_BLOCK), (size_t)c->n_hot * HOT_REC * sizeof(double2), c->stream, da,
                         c->e0c_bins_per_wg, (double*)nullptr);
      break;
    case E0K::lm_cached_acc:  // cold observations write q to their camera-major position (q4c)
      hipLaunchKernelGGL(e0_lm_cached<true>, grid, dim3(E0C_BLOCK), (size_t)c->n_hot_acc * (HOT_REC * sizeof(double2) + 96), c->stream,
                         da, c->e0c_bins_per_wg, c->hot_part.p);
      break;
    case E0K::lm_tiles:
      hipLaunchKernelGGL((lm_regular<OpE0Tiles>), dim3(c->n_reg_blocks), dim3(LM_BLOCK), 0, c->stream, da, OpE0Tiles{}, c->part.p);
      break;
    case E0K::tiles_cached:
      hipLaunchKernelGGL(e0_tiles_cached, grid, dim3(E0T_BLOCK), (size_t)c->n_hot_acc * (HOT_REC_T * sizeof(double2) + 96), c->stream,
                         da, c->e0c_bins_per_wg, c->hot_part.p);
      break;
    case E0K::lpl:
      if (robust) hipLaunchKernelGGL(e0_lpl<true>, grid, dim3(E0C_BLOCK), lpl_lds_bytes(c->v2_max_slots), c->stream, da, c->v2_part.p);
      else hipLaunchKernelGGL(e0_lpl<false>, grid, dim3(E0C_BLOCK), lpl_lds_bytes(c->v2_max_slots), c->stream, da, c->v2_part.p);
      break;
    case E0K::lm_h:
      hipLaunchKernelGGL((lm_regular<OpE0H>), dim3(c->n_reg_blocks), dim3(LM_BLOCK), 0, c->stream, da, OpE0H{}, c->part.p);
      break;
    case E0K::lm_cached_h:
      hipLaunchKernelGGL(e0_lm_cached_h, grid, dim3(E0C_BLOCK), (size_t)c->n_hot_acc * (HOT_REC_H * sizeof(double2) + 96), c->stream,
                         da, c->e0c_bins_per_wg, c->hot_part.p);
      break;
    case E0K::lpl_h:
      if (robust) hipLaunchKernelGGL(e0_lpl_h<true>, grid, dim3(E0C_BLOCK), lpl_lds_bytes_h(c->v2_max_slots), c->stream, da, c->v2_part.p);
      else hipLaunchKernelGGL(e0_lpl_h<false>, grid, dim3(E0C_BLOCK), lpl_lds_bytes_h(c->v2_max_slots), c->stream, da, c->v2_part.p);
      break;
    case E0K::ck_h: {
      const CkP k = ck_params(c, c->ckh);
      const size_t lds = ckh_lds_bytes(c->ckh.max_acc, c->ckh.stride);
      if (c->ckh.stride == CKH_STRIDE_WIDE) {  // two landmark batches instead of three, fewer accumulators (povar_kernels_ck_joint.hpp)
        if (robust) hipLaunchKernelGGL((e0_ck_h<16, 2, true, CKH_STRIDE_WIDE>), grid, dim3(1024), lds, c->stream, da, k, c->ckh.part.p);
        else hipLaunchKernelGGL((e0_ck_h<16, 2, false, CKH_STRIDE_WIDE>), grid, dim3(1024), lds, c->stream, da, k, c->ckh.part.p);
      } else {
        if (robust) hipLaunchKernelGGL((e0_ck_h<16, 2, true>), grid, dim3(1024), lds, c->stream, da, k, c->ckh.part.p);
        else hipLaunchKernelGGL((e0_ck_h<16, 2, false>), grid, dim3(1024), lds, c->stream, da, k, c->ckh.part.p);
      }
      break;
    }
    case E0K::ck_h_det: {
      const size_t lds = ckh_lds_bytes_det(c->ckh.max_acc);
      if (robust) hipLaunchKernelGGL((e0_ck_h_det<16, 2, true>), grid, dim3(1024), lds, c->stream, da, ck_params(c, c->ckh), c->ckh.part.p);
      else hipLaunchKernelGGL((e0_ck_h_det<16, 2, false>), grid, dim3(1024), lds, c->stream, da, ck_params(c, c->ckh), c->ckh.part.p);
      break;
    }
  }
  if (p.long_after) {
    if (p.e0 == E0K::lm_tiles || p.e0 == E0K::tiles_cached)
      hipLaunchKernelGGL((lm_long<OpE0Tiles>), dim3(c->n_long), dim3(LM_BLOCK), 0, c->stream, da, OpE0Tiles{}, c->part.p);
    else if (p.step == 2)
      hipLaunchKernelGGL((lm_long<OpE0H>), dim3(c->n_long), dim3(LM_BLOCK), 0, c->stream, da, OpE0H{}, c->part.p);
    else
      hipLaunchKernelGGL((lm_long<OpE0>), dim3(c->n_long), dim3(LM_BLOCK), 0, c->stream, da, OpE0{}, c->part.p);
  }
  const int hom = p.step == 2 ? 1 : 0;
  const int norms = p.use == TermUse::series_norms ? 1 : 0;
  switch (p.cam) {
    case CamStep::fused:  // B^-1, AXPY and z too
      // 128 threads per camera: a camera's run is at most one partial record per workgroup (256) plus ~85 cold
      // observations; two wavefronts keep four loads per thread in flight and halve the cross-wavefront reduction
      // (256 threads: 71.7 us per term, 128: 69.5, 64: 69.6 on venice-1778)
      if (hom)
        hipLaunchKernelGGL(cam_cold_sum_binv_h<CCS_THREADS>, dim3(c->n_cams), dim3(CCS_THREADS), 0, c->stream, da, norms, (const double*)c->ncw.p);
      else
        hipLaunchKernelGGL(cam_cold_sum_binv<CCS_THREADS>, dim3(c->n_cams), dim3(CCS_THREADS), 0, c->stream, da, norms);
      break;
    case CamStep::sum:  // dense y (sigma applied); with the peer-to-peer exchange it pushes the partials to the peers
      hipLaunchKernelGGL(cam_cold_sum<CCS_THREADS>, dim3(c->n_cams), dim3(CCS_THREADS), 0, c->stream, da, hom);
      break;
    case CamStep::scatter:
    case CamStep::scatter_sum:
      hipLaunchKernelGGL(cm_scatter, dim3(grid_for(std::max(c->n_items, 1), 4)), dim3(256), 0, c->stream, c->d, 1, hom);
      if (p.cam == CamStep::scatter_sum)
        hipLaunchKernelGGL(cam_sum_items, dim3(grid_for(c->n_cams, 4)), dim3(256), 0, c->stream, c->d, c->d.y, 1);
      break;
  }
  if (p.exch == Exch::allreduce) return allreduce(c, c->d.y, 12 * (size_t)c->n_cams);
  return 0;
}

// dynamic LDS of the kernels this unit launches (povar_create)
template <int NW, int SD, bool DB, int NG>
hipError_t ck_set_lds_t() {
  hipError_t e = hipFuncSetAttribute((const void*)e0_ck<NW, SD, DB, NG, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, CK_LDS_BYTES);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)e0_ck<NW, SD, DB, NG, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, CK_LDS_BYTES);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)e0_ck<NW, SD, DB, NG, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CK_LDS_BYTES);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)e0_ck<NW, SD, DB, NG, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, CK_LDS_BYTES);
  return e;
}

hipError_t term_set_lds_all() {
  const auto set = [](const void* f, size_t bytes) { return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); };
  hipError_t e = set((const void*)e0_lm_cached<false>, HOT_MAX * HOT_REC * sizeof(double2));
  if (e == hipSuccess) e = set((const void*)e0_tiles_cached, HOT_ACC_MAX * (HOT_REC_T * sizeof(double2) + 96));
  if (e == hipSuccess) e = set((const void*)e0_lm_cached_h, HOT_ACC_MAX * (HOT_REC_H * sizeof(double2) + 96));
  if (e == hipSuccess) e = set((const void*)e0_lm_cached<true>, HOT_ACC_MAX * (HOT_REC * sizeof(double2) + 96));
  if (e == hipSuccess) e = set((const void*)e0_lpl<false>, lpl_lds_bytes(HOT_ACC_MAX));
  if (e == hipSuccess) e = set((const void*)e0_lpl<true>, lpl_lds_bytes(HOT_ACC_MAX));
  if (e == hipSuccess) e = set((const void*)e0_lpl_h<false>, lpl_lds_bytes_h(HOT_ACC_MAX));
  if (e == hipSuccess) e = set((const void*)e0_lpl_h<true>, lpl_lds_bytes_h(HOT_ACC_MAX));
  if (e == hipSuccess) e = set((const void*)e0_ck_det<16, 2, false>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_det<16, 2, true>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_h_det<16, 2, false>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_h_det<16, 2, true>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_f32<false, false>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_f32<true, false>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_f32<false, true>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_f32<true, true>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_h<16, 2, false>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_h<16, 2, true>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_h<16, 2, false, CKH_STRIDE_WIDE>, CK_LDS_BYTES);
  if (e == hipSuccess) e = set((const void*)e0_ck_h<16, 2, true, CKH_STRIDE_WIDE>, CK_LDS_BYTES);
#define X(id, nw, sd, db, ng) if (e == hipSuccess) e = ck_set_lds_t<nw, sd, db, ng>();
  POVAR_CK_VARIANTS(X)
#undef X
  return e;
}

void launch_binv(povar_ctx* c, int mode, int want_norms) {
  if (mode == 4) return;  // fused into cam_cold_sum_binv
  prof_mark(c, 1);
  if (c->joint) {
    hipLaunchKernelGGL(cam_binv_axpy_h, dim3(c->n_cam_blocks), dim3(K9_CAMS * 64), 0, c->stream, c->d, mode, want_norms,
                       (const double*)c->ncw.p);
  } else {
    Dp dt = c->d;
    if (mode == 5) p2p_dp(c, dt);
    hipLaunchKernelGGL(cam_binv_axpy, dim3(c->n_cam_blocks), dim3(K9_CAMS * 64), 0, c->stream, dt, mode, want_norms);
  }
}

// Which of a step's two E0 kernels is faster depends on the graph (e0_ck: venice-like camera counts, any share of
// observations whose camera has no LDS slot; e0_lpl: many cameras and few observations per (camera, batch), where a chunk
// is a single observation -- final-13682).  Unless the caller has forced one, both are timed once per layout on the
// problem itself: a warm-up and three launches each on the prepared system (they only write their partial records).
int ck_autotune(povar_ctx* c, int step) {
  bool& tuned = step == 2 ? c->ckh_tuned : c->ck_tuned;
  int& variant = step == 2 ? c->ckh_variant : c->ck_variant;
  if (!c->ck_auto || tuned || c->joint != (step == 2)) return 0;
  const TermPlan lpl = term_plan(c, step, TermUse::timing, 0), ck = term_plan(c, step, TermUse::timing, 1);
  if (ck.e0 != (step == 2 ? E0K::ck_h : E0K::ck)) {
    // (a step-2 chunk layout the kernel cannot run settles step 2 on e0_lpl_h; step 1 asks again)
    if (step == 2 && lpl.e0 == E0K::lpl_h && c->ckh.ready) {
      tuned = true;
      variant = 0;
    }
    return 0;
  }
  tuned = true;
  ensure_ck_w(c, step);
  HIP_TRY(hipMemsetAsync(c->flags.p + 1, 0, sizeof(int) * 3, c->stream));  // (a series that ended early leaves "done" set)
  // Two rounds of (warm-up + REPS launches) of each kernel, alternating, the FASTER round of each counts: one round's mean
  // was seen 18 % off on the same box (Zipf(0.5): e0_ck 80.2 against 67.9 us in two processes -- clocks still ramping, the
  // placement thread's uploads), enough to keep the slower kernel for the life of the layout.
  constexpr int ROUNDS = 2;
  EventSet<4 * ROUNDS> ev;
  HIP_TRY(ev.create());
  struct Restore {  // a failure below leaves the timing to be repeated (step 1 on its kernel, step 2 on e0_lpl_h)
    int& variant; bool& tuned; int keep; bool done = false;
    ~Restore() { if (!done) { variant = keep; tuned = false; } }
  } restore{variant, tuned, step == 2 ? 0 : variant};
  // What is timed is the PAIR of a term -- the E0 kernel and the per-camera kernel behind it --: e0_lpl leaves its cold
  // observations to the per-camera kernel (Zipf(0.5): 25 us there against 7 behind e0_ck; the E0 kernels alone were a draw
  // in some processes and the slower pair was kept).  The per-camera kernel's outputs (accum, tmp, z) are what the series'
  // first kernel writes anyway.
  constexpr int REPS = 3;
  for (int r = 0; r < ROUNDS; ++r) {
    if (int rc = launch_e0(c, lpl)) return rc;
    HIP_TRY(hipEventRecord(ev[4 * r], c->stream));
    for (int i = 0; i < REPS; ++i)
      if (int rc = launch_e0(c, lpl)) return rc;
    HIP_TRY(hipEventRecord(ev[4 * r + 1], c->stream));
    if (int rc = launch_e0(c, ck)) return rc;
    HIP_TRY(hipEventRecord(ev[4 * r + 2], c->stream));
    for (int i = 0; i < REPS; ++i)
      if (int rc = launch_e0(c, ck)) return rc;
    HIP_TRY(hipEventRecord(ev[4 * r + 3], c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipGetLastError());
  float ms_lpl = 1e30f, ms_ck = 1e30f;
  for (int r = 0; r < ROUNDS; ++r) {
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, ev[4 * r], ev[4 * r + 1]));
    HIP_TRY(hipEventElapsedTime(&b, ev[4 * r + 2], ev[4 * r + 3]));
    ms_lpl = std::min(ms_lpl, a);
    ms_ck = std::min(ms_ck, b);
  }
  restore.done = true;
  float* us = step == 2 ? c->ckh_tune_us : c->ck_tune_us;
  us[0] = 1e3f * ms_lpl / REPS;
  us[1] = 1e3f * ms_ck / REPS;
  variant = ms_ck < 0.98f * ms_lpl ? 1 : 0;
  c->ck_fresh[step - 1] = true;
  return 0;
}

// The ranks of a sharded run keep the SAME term kernel (each rank timed its own shard and ranks of one run could
// end on different kernels -- a term then takes as long as the slower choice, and two runs of the same problem need not agree).
// Every rank's prepare call ends in one all-reduce of four doubles through the context's exchange (RCCL or the host hook):
// the timings of the ranks that have just timed (their sum decides, for everybody), how many did, and how many ranks have no
// chunk layout (one is enough to keep every rank on e0_lpl).  Unconditional on anything a rank decides by itself -- when a
// rank's placed rows arrive, and with them a new timing, differs from rank to rank; the collective does not.
int tune_agree(povar_ctx* c, int step) {
  // (the condition holds on every rank or on none: options and environment are the run's, not the rank's)
  if (!sharded(c) || !c->ck_auto || c->deterministic || c->opt.e0_mode != POVAR_E0_IMPLICIT_LDSACC) return 0;
  if (step == 0 && c->fp32_terms) return 0;  // (step 1 is pinned to e0_ck_f32; a run's flags are every rank's)
  const bool fresh = c->ck_fresh[step];
  const float* us = step ? c->ckh_tune_us : c->ck_tune_us;
  const bool ready = c->use_lpl && (step ? c->ckh.ready : c->ck.ready);
  double h[4] = {fresh ? us[0] : 0.0, fresh ? us[1] : 0.0, fresh ? 1.0 : 0.0, ready ? 0.0 : 1.0};
  HIP_TRY(hipMemcpyAsync(c->scal.p, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (h is on this frame)
  if (int rc = allreduce(c, c->scal.p, 4)) return rc;
  HIP_TRY(hipMemcpyAsync(h, c->scal.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->ck_fresh[step] = false;
  int& variant = step ? c->ckh_variant : c->ck_variant;
  if (h[3] > 0) variant = 0;
  else if (h[2] > 0) variant = h[1] < 0.98 * h[0] ? 1 : 0;
  return 0;
}

extern "C" {


int povar_power_series_begin(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = res_verify(c)) return rc;  // (a resident series that gave up is repeated BEFORE its state is overwritten / continued)
  HIP_TRY(hipMemsetAsync(c->flags.p + 1, 0, sizeof(int) * 3, c->stream));
  launch_binv(c, 0, 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

int povar_power_series_step(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = res_verify(c)) return rc;  // (a resident series that gave up is repeated BEFORE its state is overwritten / continued)
  const TermPlan p = term_plan(c, c->joint ? 2 : 1, TermUse::series);
  if (p.step == 1) c->fp32_last = p.e0 == E0K::ck_f32 ? 1 : 0;
  if (int rc = launch_e0(c, p)) return rc;
  launch_binv(c, p.binv_mode(), 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

int enqueue_series(povar_ctx* c, int32_t m, double q_tol, double r_tol) {
  const bool norms = q_tol > 0 || r_tol > 0;
  const TermPlan p = term_plan(c, c->joint ? 2 : 1, norms ? TermUse::series_norms : TermUse::series);
  HIP_TRY(hipMemsetAsync(c->flags.p + 1, 0, sizeof(int) * 3, c->stream));
  launch_binv(c, 0, (m > 0 && r_tol > 0) ? 1 : 0);
  if (m > 0 && r_tol > 0)
    hipLaunchKernelGGL(series_check, dim3(1), dim3(64), 0, c->stream, c->d, c->n_cam_blocks, 0, q_tol, r_tol);
  for (int i = 1; i <= m; ++i) {
    if (int rc = launch_e0(c, p)) return rc;
    launch_binv(c, p.binv_mode(), norms ? 1 : 0);
    if (norms)  // the fused kernel leaves one norm partial per camera, cam_binv_axpy one per workgroup
      hipLaunchKernelGGL(series_check, dim3(1), dim3(64), 0, c->stream, c->d, p.cam == CamStep::fused ? c->n_cams : c->n_cam_blocks,
                         i, q_tol, r_tol);
  }
  prof_mark(c, -1);
  return 0;
}

// One series on the context's stream: the per-term kernels (use_res = false) or the resident kernel, through the cached
// hipGraph where the context allows a capture.
int run_series(povar_ctx* c, int32_t m, double q_tol, double r_tol, bool use_res) {
  const bool norms = q_tol > 0 || r_tol > 0;
  const TermPlan p = term_plan(c, c->joint ? 2 : 1, norms ? TermUse::series_norms : TermUse::series);
  // with a communicator the loop is launched kernel by kernel (the per-term all-reduce dominates and
  // RCCL-in-capture is not something a 1-GPU box can validate); POVAR_GRAPH_COMM=1 opts in
  if (c->use_graph && !c->profile && m > 0 && (use_res || p.p2p_check() || (!c->host_fn && (!c->comm || c->graph_with_comm)))) {
    // the whole loop (memset, B^-1, m x {E0 kernels, [all-reduce], B^-1 + AXPY, [check]}) is one graph
    // launch; it is re-captured only when a kernel argument changes
    const int key[6] = {m, (c->joint ? 1 : 0) | (use_res ? 2 : 0) | (use_res ? (res_params(c, m, q_tol, r_tol).w_mode << 2) : 0),
                        c->opt.e0_mode + 16 * ((int)p.e0 + 16 * p.variant), (p.exch != Exch::none ? 1 : 0) | (p.p2p_check() ? 2 : 0),
                        norms ? 1 : 0, r_tol > 0 ? 1 : 0};
    // (the landmark damping is an argument of the prepare / back-substitution kernels only: no kernel of the loop reads
    // it, and step 2 changes it with every LM iteration -- a capture + instantiation of 0.25 ms each time)
    Dp key_d = c->d;
    key_d.lambda_lm = 0;
    const bool same = c->series_graph && std::memcmp(key, c->series_graph_key, sizeof(key)) == 0 &&
                      std::memcmp(&key_d, &c->series_graph_d, sizeof(Dp)) == 0 &&
                      c->series_graph_tol[0] == q_tol && c->series_graph_tol[1] == r_tol;
    if (!same) {
      if (c->series_graph) (void)hipGraphExecDestroy(c->series_graph);
      c->series_graph = nullptr;
      hipGraph_t g = nullptr;
      std::lock_guard<std::mutex> lk(g_capture_mu);  // no HIP call of the row-placement thread inside the capture
      HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
      const int rc = use_res ? enqueue_series_res(c, m, q_tol, r_tol) : enqueue_series(c, m, q_tol, r_tol);
      hipError_t e = hipStreamEndCapture(c->stream, &g);
      if (rc) return rc;
      HIP_TRY(e);
      HIP_TRY(hipGraphInstantiate(&c->series_graph, g, nullptr, nullptr, 0));
      (void)hipGraphDestroy(g);
      std::memcpy(c->series_graph_key, key, sizeof(key));
      c->series_graph_d = key_d;
      c->series_graph_tol[0] = q_tol;
      c->series_graph_tol[1] = r_tol;
    }
    HIP_TRY(hipGraphLaunch(c->series_graph, c->stream));
  } else if (use_res) {
    if (int rc = enqueue_series_res(c, m, q_tol, r_tol)) return rc;
  } else {
    if (int rc = enqueue_series(c, m, q_tol, r_tol)) return rc;
  }
  if (use_res) {
    c->res_check = true;  // the give-up bit is looked at with the caller's next read-back (res_verify)
    c->res_last_m = m;
    c->res_last_tol[0] = q_tol;
    c->res_last_tol[1] = r_tol;
    c->flag0_clean = false;
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// A resident series gives up (bit 2 of flags[0]) when its workgroups were not all on the device together -- another
// context's kernels held CUs for longer than the bounded spins.  The result is then incomplete: the series is repeated
// with the per-term kernels and the context stays on them.  Called before anything reads what the series left.
int res_verify(povar_ctx* c) {
  if (c->det_check) {
    c->det_check = false;
    int f[4];
    if (int rc = read_flags(c, f)) return rc;
    if (f[0] & 8) {
      HIP_TRY(hipMemsetAsync(c->flags.p, 0, sizeof(int), c->stream));
      return fail(-3, "e0_ck_det: the accumulator tickets of the chunk layout do not match the kernel's tile walk");
    }
  }
  if (!c->res_check) return 0;
  c->res_check = false;
  int f[4];
  if (int rc = read_flags(c, f)) return rc;
  if (!(f[0] & 4)) return 0;
  c->res_failed = true;
  HIP_TRY(hipMemsetAsync(c->flags.p, 0, sizeof(int), c->stream));
  if (c->series_graph) { (void)hipGraphExecDestroy(c->series_graph); c->series_graph = nullptr; }
  return run_series(c, c->res_last_m, c->res_last_tol[0], c->res_last_tol[1], false);
}

// Which of the two forms of the series is faster is a property of the context (observations per workgroup, cameras per
// workgroup): unless one is forced (POVAR_RES, povar_set_series_kernel) both are run once on the caller's prepared system
// -- a warm-up and REPS timed solves each, the same m and tolerances -- and the faster one is kept.
int res_autotune(povar_ctx* c, int32_t m, double q_tol, double r_tol) {
  // (once per step, on the system prepared last: the two kernels and their per-term counterparts differ)
  bool& tuned = c->res_tune[c->joint].tuned;
  bool& choice = c->res_tune[c->joint].choice;
  float* tune_us = c->res_tune[c->joint].us;
  if (c->res_mode >= 0 || tuned || !res_possible(c, c->joint) || m < 4 || m > 250) return 0;
  tuned = true;
  struct Restore {  // a failure below leaves the choice open and the timing to be repeated (as ck_autotune)
    bool& tuned; bool& choice; bool done = false;
    ~Restore() { if (!done) { tuned = false; choice = false; } }
  } restore{tuned, choice};
  // Two alternating rounds of (warm-up + REPS series) of each form, the FASTER round of each counts -- one round's mean was
  // seen 18 % off in some processes (ck_autotune) --, and both forms run all m terms: the tolerances are off while timing (an
  // early exit would time a few terms of one form against a few of the other; the caller's series follows with its own)
  (void)q_tol; (void)r_tol;
  constexpr int ROUNDS = 2, REPS = 2;
  EventSet<4 * ROUNDS> ev;
  HIP_TRY(ev.create());
  for (int r = 0; r < ROUNDS; ++r)
    for (int which = 0; which < 2; ++which) {
      if (int rc = run_series(c, m, 0.0, -1.0, which == 1)) return rc;
      HIP_TRY(hipEventRecord(ev[4 * r + 2 * which], c->stream));
      for (int i = 0; i < REPS; ++i)
        if (int rc = run_series(c, m, 0.0, -1.0, which == 1)) return rc;
      HIP_TRY(hipEventRecord(ev[4 * r + 2 * which + 1], c->stream));
      if (which == 1) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (int rc = res_verify(c)) return rc;
        if (c->res_failed) { restore.done = true; choice = false; return 0; }
      }
    }
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms[2] = {1e30f, 1e30f};
  for (int r = 0; r < ROUNDS; ++r)
    for (int which = 0; which < 2; ++which) {
      float t = 0;
      HIP_TRY(hipEventElapsedTime(&t, ev[4 * r + 2 * which], ev[4 * r + 2 * which + 1]));
      ms[which] = std::min(ms[which], t);
    }
  restore.done = true;
  tune_us[0] = 1e3f * ms[0] / (REPS * m);
  tune_us[1] = 1e3f * ms[1] / (REPS * m);
  choice = ms[1] < 0.98f * ms[0];
  return 0;
}

int povar_power_series_pose(povar_ctx* c, int32_t m, double q_tol, double r_tol, int32_t* num_iterations,
                            int32_t* termination) {
  if (int rc = check_ctx(c)) return rc;
  if (m < 0) return fail(-1, "power_sc_iterations < 0");
  TimeScope ts(c, 2);
  if (!lpl_mode(c)) ensure_legacy(c);  // not inside the graph capture
  if (int rc = ck_autotune(c, c->joint ? 2 : 1)) return rc;
  const bool norms = q_tol > 0 || r_tol > 0;
  const TermPlan p = term_plan(c, c->joint ? 2 : 1, norms ? TermUse::series_norms : TermUse::series);
  if (p.ck()) ensure_ck_w(c, p.step);
  if (int rc = res_autotune(c, m, q_tol, r_tol)) return rc;
  const bool use_res = m > 0 && m <= 250 && res_active(c, c->joint);  // (a granule tag carries the term in 8 bits)
  if (p.step == 1) c->fp32_last = p.e0 == E0K::ck_f32 && !use_res ? 1 : 0;
  if (int rc = run_series(c, m, q_tol, r_tol, use_res)) return rc;
  int iters = m, status = POVAR_LINEAR_SOLVER_NO_CONVERGENCE;
  if (p.p2p_check()) c->flag0_clean = false;  // the waits of the exchange kernels raise bit 1 of flags[0] on a time-out
  if (p.det_check()) {  // e0_ck[_h]_det: a ticket that never came up raises bit 3 (bounded spins):
    c->flag0_clean = false;                // looked at where the caller next waits for the series (res_verify)
    c->det_check = true;
  }
  if (p.p2p_check()) {
    int f[4];
    if (int rc = read_flags(c, f)) return rc;
    if (f[0] & 2) {
      HIP_TRY(hipMemsetAsync(c->flags.p, 0, sizeof(int), c->stream));
      return fail(-3, "peer-to-peer exchange: a rank did not deliver its partial sums (wait timed out)");
    }
  }
  if (norms) {
    if (int rc = res_verify(c)) return rc;  // (the read-back below must see the flags of a complete series)
    int f[4];
    if (int rc = read_flags(c, f)) return rc;
    if (f[1]) {
      iters = f[2];
      status = POVAR_LINEAR_SOLVER_SUCCESS;
    }
  }
  if (num_iterations) *num_iterations = iters;
  if (termination) *termination = status;
  return 0;
}

int povar_get_increment(povar_ctx* c, double* inc) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = res_verify(c)) return rc;
  return read_cam_vector(c, inc, c->accum.p, (size_t)(c->joint ? 11 : 12) * c->n_cams);
}

int povar_get_term(povar_ctx* c, double* term) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = res_verify(c)) return rc;
  return read_cam_vector(c, term, c->tmp.p, (size_t)(c->joint ? 11 : 12) * c->n_cams);
}

int povar_solve_pose(povar_ctx* c, double lambda, int32_t solver_type, int32_t m, double q_tol,
                     double r_tol, double* inc, int32_t* num_iterations, int32_t* termination) {
  if (int rc = povar_prepare_pose(c, lambda, solver_type)) return rc;
  if (int rc = povar_power_series_pose(c, m, q_tol, r_tol, num_iterations, termination)) return rc;
  if (int rc = povar_get_increment(c, inc)) return rc;
  for (size_t i = 0; i < 12 * (size_t)c->n_cams; ++i)
    if (!std::isfinite(inc[i])) return POVAR_NUMERIC_FAILURE;  // bal_bundle_adjustment.cpp:362
  return 0;
}

int povar_right_mul_e0_pose(povar_ctx* c, const double* x, double* y) {
  if (int rc = check_ctx(c)) return rc;
  const size_t n = 12 * (size_t)c->n_cams;
  HIP_TRY(hipMemcpyAsync(c->tmp.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->flags.p + 1, 0, sizeof(int) * 3, c->stream));
  // z = sigma * x
  HIP_TRY(hipMemcpyAsync(c->inc.p, c->tmp.p, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(cam_apply_inc, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->d, 1);
  const TermPlan p = term_plan(c, c->joint ? 2 : 1, TermUse::right_mul);
  if (int rc = launch_e0(c, p)) return rc;
  if (p.cam == CamStep::scatter)
    hipLaunchKernelGGL(cam_sum_items, dim3(grid_for(c->n_cams, 4)), dim3(256), 0, c->stream, c->d, c->d.y, 1);
  HIP_TRY(hipMemcpyAsync(y, c->y.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemsetAsync(c->y.p, 0, sizeof(double) * n, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

int povar_solve_joint(povar_ctx* c, double lambda, int32_t m, double q_tol, double r_tol, double* inc,
                      int32_t* num_iterations, int32_t* termination) {
  if (int rc = povar_prepare_joint(c, lambda)) return rc;
  if (int rc = povar_power_series_pose(c, m, q_tol, r_tol, num_iterations, termination)) return rc;
  if (int rc = povar_get_increment(c, inc)) return rc;
  for (size_t i = 0; i < 11 * (size_t)c->n_cams; ++i)
    if (!std::isfinite(inc[i])) return POVAR_NUMERIC_FAILURE;
  return 0;
}

int povar_set_e0_mode(povar_ctx* c, int32_t mode) {
  if (int rc = check_ctx(c)) return rc;
  if (mode != POVAR_E0_IMPLICIT && mode != POVAR_E0_TILES && mode != POVAR_E0_IMPLICIT_LDSACC &&
      mode != POVAR_E0_TILES_LDSACC) return fail(-1, "bad e0 mode");
  if (c->deterministic) return 0;  // pinned (POVAR_DETERMINISTIC)
  if (c->fp32_terms && mode != POVAR_E0_IMPLICIT_LDSACC)
    return fail(-1, "POVAR_FLAG_FP32_TERMS: the fp32 terms run in the LDS-accumulating E0 mode only");
  c->opt.e0_mode = mode;
  if (c->linearized) return ensure_tiles(c);
  return 0;
}

int povar_profile_enable(povar_ctx* c, int32_t enable) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->profile = enable != 0;
  c->ev_used = 0;
  return 0;
}

int povar_profile_get(povar_ctx* c, povar_profile_info* out) {
  if (int rc = check_ctx(c)) return rc;
  if (!out) return fail(-1, "null argument");
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::memset(out, 0, sizeof(*out));
  for (size_t i = 0; i + 1 < c->ev_used; ++i) {
    const int kind = c->ev_kind[i];
    if (kind < 0) continue;
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
    if (kind == 0) { out->e0_ms += ms; out->e0_launches++; }
    else if (kind == 1) { out->binv_ms += ms; out->binv_launches++; }
    else { out->comm_ms += ms; out->comm_launches++; }
  }
  c->ev_used = 0;
  return 0;
}

int povar_e0_model_bytes(povar_ctx* c, int64_t* lm_kernel, int64_t* cam_kernel) {
  if (int rc = check_ctx(c)) return rc;
  if (!lm_kernel || !cam_kernel) return fail(-1, "null argument");
  // Bytes the E0 kernels of the current mode must move per application BY DESIGN (every array they stream, once;
  // arrays that stay in L2 -- camera records, z, the LDS image -- counted once, not per gather).  This is the
  // byte floor bench.py prices the measured kernel time against; the PMC-measured traffic is reported beside it.
  const int64_t ns = c->n_slots, nl = c->n_lms, nc = c->n_cams, no = c->n_obs;
  const int64_t robust = c->opt.robust_norm ? 8 : 0;
  const int64_t cam_static = nc * (96 + 96);            // z (12 doubles) + P (12 doubles) per camera
  const TermPlan p = term_plan(c, c->joint ? 2 : 1, TermUse::series);
  E0K k = p.e0;
  if (k == E0K::lm_h)  // (step 2 outside the LDS-accumulating mode is priced as step 1's kernel of the mode)
    k = c->opt.e0_mode == POVAR_E0_TILES ? E0K::lm_tiles : c->opt.e0_mode == POVAR_E0_TILES_LDSACC ? E0K::tiles_cached : E0K::lm_cached;
  const bool lpl = k == E0K::lpl || k == E0K::lpl_h;
  const bool lik = (k == E0K::lm_cached_acc || k == E0K::lm_cached_h) && c->long_in_kernel;
  const bool acc = k == E0K::lm_cached_acc || k == E0K::lm_cached_h || k == E0K::tiles_cached;
  const int64_t n_cold = lpl ? c->n_cold3 : lik ? c->n_cold2 : c->n_cold;
  const int64_t hot_flush = lpl ? (int64_t)c->v2_part.n * 8 : acc ? (int64_t)c->e0c_grid * c->n_hot_acc * 96 : 0;
  const int64_t tail = nc * (1152 + 96 /*sigma*/ + 3 * 96 /*accum rw, tmp*/ + 96 /*z*/);
  const int64_t part = (int64_t)(p.step == 2 ? c->ckh : c->ck).n_part_rec * 96;
  int64_t lm = 0, cm = 0;
  switch (k) {
    case E0K::ck_det:
      // e0_ck_det: as e0_ck below with the rows THREE times (two walks forward, one back), the landmark records twice (h~, G),
      // and 1 + 2 bytes of counts / tickets per landmark lane / chunk lane
      lm = 3 * c->ck.rows * WAVE * 18 + (int64_t)c->d.v2.n_tiles * WAVE * (72 + 1) + cam_static +
           4 * (int64_t)(c->ck.lane_meta.n) * 8 + (int64_t)c->ck.lane_meta.n * 2 + part;
      cm = part + tail;
      break;
    case E0K::ck_h_det:  // e0_ck_h_det: the 2-byte rows (+ 8 with a robust norm) three times, X / records twice
      lm = 3 * c->ckh.rows * WAVE * (2 + robust) + (int64_t)c->d.v2.n_tiles * WAVE * (112 + 1) + cam_static +
           4 * (int64_t)(c->ckh.lane_meta.n) * 8 + (int64_t)c->ckh.lane_meta.n * 2 + part;
      cm = part + tail;
      break;
    case E0K::ck_f32:
      // e0_ck_f32: the rows on both passes at 8 + 2 bytes (packed or fp32 image points + slot), the 36-byte fp32 landmark
      // records once, the camera image (z 96 in fp64 + P 48 in fp32), lane metadata on both passes, fp64 partial records
      lm = 2 * c->ck.rows * WAVE * 10 + (int64_t)c->d.v2.n_tiles * WAVE * 36 + nc * (96 + 48) + 2 * (int64_t)(c->ck.lane_meta.n) * 8 + part;
      cm = part + tail;
      if (c->ck.cold_q) {
        lm += 36 * c->n_cold3;
        cm += 56 * c->n_cold3;
      }
      break;
    case E0K::ck:
      // e0_ck: the chunk rows (uv 16 + landmark slot 2 bytes) on BOTH passes -- the kernel as built reads them twice --,
      // the 72-byte landmark records once, 8 bytes of lane metadata per chunk lane and pass, the partial records out
      // (one per workgroup slot + one per chunk of a camera without a slot); the per-camera kernel reads those back
      lm = 2 * c->ck.rows * WAVE * (c->ck.packed ? 10 : 18) /* image point 16 bytes (8 packed) + slot 2; no weight array: recomputed (ck_huber_w) */ + (int64_t)c->d.v2.n_tiles * WAVE * 72 + cam_static +
           2 * (int64_t)(c->ck.lane_meta.n) * 8 + part;
      cm = part + tail;
      if (c->ck.cold_q) {  // cold observations: position 4 + q 32 bytes out of e0_ck, q 32 + landmark copy 24 into the per-camera kernel
        lm += 36 * c->n_cold3;
        cm += 56 * c->n_cold3;
      }
      break;
    case E0K::ck_h:
      // e0_ck_h: landmark slot (2 bytes) [+ weight] per observation on both passes -- the step-2 operator does not read
      // the image coordinates --, the 112-byte landmark records once, lane metadata, partial records out and back
      lm = 2 * c->ckh.rows * WAVE * (2 + robust) + (int64_t)c->d.v2.n_tiles * WAVE * 112 + cam_static +
           2 * (int64_t)(c->ckh.lane_meta.n) * 8 + part;
      cm = part + tail;
      break;
    case E0K::lpl:
    case E0K::lpl_h:
    case E0K::lm_cached_acc:
    case E0K::lm_cached_h:
      if (lpl)  // e0_lpl: uv + camera slot per row slot, 72-byte landmark records; e0_lpl_h: the camera slot only (its
                // operator does not depend on uv: the loads are dead code), 112-byte records; cold: position + q out
        lm = c->v2_rows * WAVE * ((k == E0K::lpl_h ? 4 : 20) + robust) + (int64_t)c->d.v2.n_tiles * WAVE * (k == E0K::lpl_h ? 112 : 72) + cam_static +
             n_cold * (c->q_rows ? 32 : 36) + hot_flush;  // q_rows: no position load, the per-camera kernel reads the index
      else
        lm = ns * (E0_SLOT_BYTES + robust) + nl * E0_LMREC_BYTES + cam_static + n_cold * 32 + hot_flush;
      cm = hot_flush + n_cold * (32 + 24 + (lpl && c->q_rows ? 4 : 0)) + tail;
      break;
    case E0K::lm_cached:
      lm = ns * (28 + robust) + nl * 96 + cam_static + no * 32;   // uv, cam, lm, meta; q4 out
      cm = no * (4 + 32 + 24) + tail;                                // cm_slot, q4 gather, cm_h
      break;
    case E0K::lm_tiles:
      lm = ns * (12 + 480 + robust) + nl * 72 + nc * 96 + no * 32;
      cm = no * (4 + 32 + 24) + tail;
      break;
    case E0K::tiles_cached:
      lm = ns * (12 + 480 + robust) + nl * 72 + nc * 96 + n_cold * 32 + hot_flush;
      cm = hot_flush + n_cold * (4 + 32 + 24) + tail;
      break;
    case E0K::lm_h:
      break;
  }
  *lm_kernel = lm;
  *cam_kernel = cm;
  return 0;
}

int povar_set_e0_kernel(povar_ctx* c, int32_t kernel) {
  if (int rc = check_ctx(c)) return rc;
  if (kernel < -1 || kernel > CK_VARIANTS) return fail(-1, "unknown E0 kernel");
  if (kernel > 0 && !c->ck_zero_range.p) return fail(-1, "the camera-chunk layout was not built for this context");
  if (c->deterministic) return 0;  // pinned (POVAR_DETERMINISTIC)
  if (c->fp32_terms && kernel == 0) return fail(-1, "POVAR_FLAG_FP32_TERMS: step 1's terms run the camera-chunk kernel e0_ck_f32");
  if (c->fp32_terms) {  // step 1 stays on e0_ck_f32 (the layout of variant 1); the choice is step 2's
    c->ck_auto = kernel < 0;
    c->ckh_tuned = false;
    c->ckh_variant = kernel > 0 ? 1 : 0;
    return 0;
  }
  if (kernel < 0) {  // back to the library's own choice
    c->ck_auto = true;
    c->ck_tuned = c->ckh_tuned = false;
    c->ck_variant = c->ckh_variant = 0;
    return 0;
  }
  c->ck_auto = false;
  c->ck_variant = kernel;
  c->ckh_variant = kernel > 0 ? 1 : 0;  // (step 2 has one camera-chunk instantiation)
  return 0;
}

int povar_set_series_kernel(povar_ctx* c, int32_t mode) {
  if (int rc = check_ctx(c)) return rc;
  if (mode < -1 || mode > 1) return fail(-1, "unknown series kernel");
  if (mode == 1 && !c->res.ready && !res_ready(c, true)) return fail(-1, "the resident-series layout was not built for this context");
  if (mode == 1 && c->fp32_terms) return fail(-1, "POVAR_FLAG_FP32_TERMS: the resident series has no fp32 form");
  if (int rc = res_verify(c)) return rc;
  if (c->deterministic) return 0;  // pinned (POVAR_DETERMINISTIC)
  c->res_mode = mode;
  if (mode < 0) c->res_tune[0].tuned = c->res_tune[1].tuned = false;  // (both steps are timed again)
  return 0;
}

int povar_debug_ck_stamps(povar_ctx* c, uint64_t* out, int64_t n) {
  // (the diagnostic build -- tools/variants/ck_stamps.patch -- replaces this body; the shipped kernels execute no stamp)
  (void)c; (void)out; (void)n;
  return fail(-1, "diagnostic builds only (tools/variants/build_variant.sh ck_stamps)");
}

}  // extern "C"
