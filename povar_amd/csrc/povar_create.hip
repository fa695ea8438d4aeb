// povar_create.hip -- layout construction and upload, povar_create / povar_destroy, read-back helpers, timings, layout info.
#include "povar_ctx.hpp"

std::mutex g_capture_mu;  // see povar_ctx::placer_cancel

// ------------------------------------------------------------------------------------------
// layout construction (host)
// ------------------------------------------------------------------------------------------
struct Layout {
  std::vector<double2> uv, cm_uv;
  std::vector<int> cam, lm, meta, hot_cams, cam_hot, cc_slot, cc_lm, cc_item_off, cc_cam_item_off, long_lm, long_first, long_cnt, cm_slot, cm_lm, item_off,
      item_cam, cam_item_off, slot_of_obs, cold_pos;
  // cold view "A" of the default mode when the problem has long landmarks: their observations of LDS-accumulated
  // cameras are accumulated inside e0_lm_cached too, so they are not cold (empty when there is no long landmark)
  std::vector<int> c2_lm, c2_pos;
  std::vector<int2> c2_range;
  int n_bins = 0;
};

// Temporaries that part A of the layout construction hands to part B.
struct LayoutTmp {
  std::vector<int> seg_first, seg_last, rank;
  std::vector<char> is_long;
  std::vector<int64_t> cnt;  // prefix sums of the observations per camera
};

// Part A: what everything else needs first -- the wave-bin slot of every observation, the popularity rank of every
// camera (the order of the record image, the key of the lane-per-landmark layout) and the camera-major work items.
void build_layout_a(int n_cams, int n_lms, const int32_t* lm_off, const int32_t* cam_idx, Layout& L, LayoutTmp& T) {
  const int64_t n_obs = lm_off[n_lms];
  L.slot_of_obs.resize(n_obs);
  // pass 1: assign slots.  Regular landmarks are packed greedily, in order, into 64-lane wave
  // bins that never split a landmark; a landmark with more than 64 observations gets
  // ceil(k/64) bins of its own and is handled by the lm_long driver.
  int bin = 0, fill = 0;
  T.seg_first.resize(n_obs);
  T.seg_last.resize(n_obs);
  T.is_long.assign(n_obs, 0);
  for (int l = 0; l < n_lms; ++l) {
    const int b = lm_off[l], k = lm_off[l + 1] - b;
    if (k == 0) continue;
    if (k > WAVE) {
      if (fill > 0) { ++bin; fill = 0; }
      L.long_lm.push_back(l);
      L.long_first.push_back(bin * WAVE);
      L.long_cnt.push_back(k);
      for (int j = 0; j < k; ++j) {
        L.slot_of_obs[b + j] = bin * WAVE + j;
        T.is_long[b + j] = 1;
      }
      bin += (k + WAVE - 1) / WAVE;
      continue;
    }
    if (fill + k > WAVE) { ++bin; fill = 0; }
    for (int j = 0; j < k; ++j) {
      L.slot_of_obs[b + j] = bin * WAVE + fill + j;
      T.seg_first[b + j] = fill;
      T.seg_last[b + j] = fill + k - 1;
    }
    fill += k;
  }
  if (fill > 0) ++bin;
  L.n_bins = std::max(bin, 1);
  std::vector<int64_t>& cnt = T.cnt;
  cnt.assign(n_cams + 1, 0);
  for (int64_t i = 0; i < n_obs; ++i) cnt[cam_idx[i] + 1]++;
  for (int c = 0; c < n_cams; ++c) cnt[c + 1] += cnt[c];
  // popularity rank of EVERY camera (1-based; ties: lower index): the record image (Dp::hot_rec) is in this order, so
  // the first n records are the LDS image of a kernel that caches n cameras and colder cameras gather theirs by rank
  std::vector<int> order(n_cams);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return cnt[a + 1] - cnt[a] > cnt[b + 1] - cnt[b]; });
  T.rank.assign(n_cams, 0);
  L.hot_cams.assign(order.begin(), order.end());
  for (int r = 0; r < n_cams; ++r) T.rank[order[r]] = r + 1;
  L.cam_hot = T.rank;
  // camera-major work items of at most CM_ITEM_MAX observations of one camera
  L.cam_item_off.assign(n_cams + 1, 0);
  for (int c = 0; c < n_cams; ++c) {
    L.cam_item_off[c] = (int)L.item_cam.size();
    for (int64_t p = cnt[c]; p < cnt[c + 1]; p += CM_ITEM_MAX) {
      L.item_off.push_back((int)p);
      L.item_cam.push_back(c);
    }
  }
  L.cam_item_off[n_cams] = (int)L.item_cam.size();
  L.item_off.push_back((int)n_obs);
}

// Part B: the arrays of the lane-per-observation kernels (wave-bin slots, camera-major inverse index, cold views).
// Independent of the lane-per-landmark layout: povar_create builds the two side by side.  n_acc: CreatePlan::n_hot_acc
void build_layout_b(int n_cams, int n_lms, const int32_t* lm_off, const int32_t* cam_idx, const double* obs, int n_acc, Layout& L,
                    const LayoutTmp& T) {
  const int64_t n_obs = lm_off[n_lms];
  const std::vector<int>&seg_first = T.seg_first, &seg_last = T.seg_last, &rank = T.rank;
  const std::vector<char>& is_long = T.is_long;
  const std::vector<int64_t>& cnt = T.cnt;
  const size_t n_slots = (size_t)L.n_bins * WAVE;
  L.uv.assign(n_slots, make_double2(0, 0));
  L.cam.assign(n_slots, -1);
  L.lm.assign(n_slots, 0);
  L.meta.resize(n_slots);
  for (size_t s = 0; s < n_slots; ++s) {
    const int lane = (int)(s & 63);
    L.meta[s] = lane | (lane << 8);
  }
  for (int l = 0; l < n_lms; ++l)
    for (int i = lm_off[l]; i < lm_off[l + 1]; ++i) {
      const int s = L.slot_of_obs[i];
      L.uv[s] = make_double2(obs[2 * (size_t)i], obs[2 * (size_t)i + 1]);
      L.cam[s] = cam_idx[i];
      L.lm[s] = l;
      if (is_long[i]) {
        const int lane = s & 63;
        L.meta[s] = lane | (lane << 8) | META_REAL | META_LONG;
      } else {
        L.meta[s] = seg_first[i] | (seg_last[i] << 8) | META_REAL;
      }
    }
  // per bin: number of doubling steps the segmented scans need = ceil(log2(longest landmark))
  for (int b = 0; b < L.n_bins; ++b) {
    int mx = 1;
    for (int l = 0; l < WAVE; ++l) {
      const int m = L.meta[(size_t)b * WAVE + l];
      if ((m & META_REAL) && !(m & META_LONG)) mx = std::max(mx, ((m >> 8) & 255) - (m & 255) + 1);
    }
    int steps = 0;
    while ((1 << steps) < mx) ++steps;
    for (int l = 0; l < WAVE; ++l) L.meta[(size_t)b * WAVE + l] |= steps << META_STEPS_SHIFT;
  }
  L.cm_slot.resize(n_obs);
  L.cm_lm.resize(n_obs);
  L.cm_uv.resize(n_obs);
  {
    // slots ascend with the observation index, so a stable counting sort by camera over the
    // observations in order yields ascending slots per camera
    std::vector<int64_t> pos(cnt.begin(), cnt.end() - 1);
    for (int l = 0; l < n_lms; ++l)
      for (int i = lm_off[l]; i < lm_off[l + 1]; ++i) {
        const int64_t p = pos[cam_idx[i]]++;
        L.cm_slot[p] = L.slot_of_obs[i];
        L.cm_lm[p] = l;
        L.cm_uv[p] = make_double2(obs[2 * (size_t)i], obs[2 * (size_t)i + 1]);
      }
  }
  {
    const int n_hot = std::min(n_cams, HOT_MAX);
    for (size_t s = 0; s < n_slots; ++s)
      if ((L.meta[s] & META_REAL) && rank[L.cam[s]] <= n_hot) L.meta[s] |= rank[L.cam[s]] << META_HOT_SHIFT;
    // "cold" camera-major structure for POVAR_E0_IMPLICIT_LDSACC: only the observations whose
    // Jp^T s is NOT accumulated in LDS (camera outside the HOT_ACC_MAX hottest, or a long landmark,
    // which the lm_long driver handles through q4)
    L.cc_cam_item_off.assign(n_cams + 1, 0);
    for (int c = 0; c < n_cams; ++c) {
      L.cc_cam_item_off[c] = (int)L.cc_item_off.size();
      int64_t run = 0;
      for (int64_t p = cnt[c]; p < cnt[c + 1]; ++p) {
        const int s = L.cm_slot[p];
        const bool acc = rank[c] > 0 && rank[c] <= n_acc && !(L.meta[s] & META_LONG);
        if (acc) continue;
        if (run % CM_COLD_ITEM_MAX == 0) L.cc_item_off.push_back((int)L.cc_slot.size());
        L.cc_slot.push_back(s);
        L.cc_lm.push_back(L.cm_lm[p]);
        ++run;
      }
    }
    L.cc_cam_item_off[n_cams] = (int)L.cc_item_off.size();
    L.cc_item_off.push_back((int)L.cc_slot.size());
    // inverse of cc_slot: where a cold observation's scatter scalars go (Dp::q4c)
    L.cold_pos.assign(n_slots, -1);
    for (size_t p = 0; p < L.cc_slot.size(); ++p) L.cold_pos[L.cc_slot[p]] = (int)p;
    if (!L.long_lm.empty()) {
      L.c2_pos.assign(n_slots, -1);
      L.c2_range.resize(n_cams);
      for (int c = 0; c < n_cams; ++c) {
        const int first = (int)L.c2_lm.size();
        const bool acc = rank[c] > 0 && rank[c] <= n_acc;
        if (!acc)
          for (int64_t p = cnt[c]; p < cnt[c + 1]; ++p) {
            L.c2_pos[L.cm_slot[p]] = (int)L.c2_lm.size();
            L.c2_lm.push_back(L.cm_lm[p]);
          }
        L.c2_range[c] = make_int2(first, (int)L.c2_lm.size());
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// camera-chunk layout of e0_ck: upload, kernel parameters, launch
// ------------------------------------------------------------------------------------------
// locked: called by the row-placement thread -- its HIP calls go in short pieces under g_capture_mu (povar_ctx::placer_cancel)
// Returns false only on a HIP failure (allocation, copy).  A layout this kernel family cannot run -- more than 65535 cameras
// (the lane metadata keeps a popularity rank in 16 bits), a row array of 4 GiB or more (32-bit buffer offsets) -- is not
// an error: D.ready stays false, what was uploaded is released and the term loop stays on e0_lpl / e0_lpl_h.
static bool ck_upload(povar_ctx* c, povar_ctx::CkDev& D, const CkLayout& K, bool locked, size_t* bytes, bool need_uv = true) {
  const bool usable = K.n_uv * sizeof(double2) < (1ull << 32) && c->n_cams <= c->ck_max_cams;
  D.ready = false;
  if (!usable) return true;
  Uploader up{c, bytes, locked};
  auto room = [&](auto& buf, size_t count) {
    if (up.rc) return;
    const auto lk = capture_lock(locked);
    up.rc = buf.alloc(count, bytes) == hipSuccess ? 0 : -1;
  };
  std::vector<int2> meta(K.lane_cam.size());
  for (size_t i = 0; i < meta.size(); ++i) {
    const int sg = K.lane_seg[i];
    meta[i] = make_int2(K.lane_cam[i] < 0 ? -1 : (K.lane_cam[i] | ((sg & 63) << 16) | (((sg >> 8) & 63) << 22)), K.lane_acc[i]);
  }
  D.packed = need_uv && K.packed;
  if (D.packed) up(D.uvp, K.uvp);  // 8 bytes per observation where every image point is a six-decimal number (ck_pack_uv)
  else if (need_uv) up(D.uv, K.uv);  // (step 2's operator does not read the image coordinates)
  up(D.li, K.li)(D.src, K.src)(D.tile, K.tile)(D.lane_meta, meta)(D.bt_off, K.bt_off)(D.slot_rec, K.slot_rec)(D.part_range, K.part_range);
  if (c->det_ck) up(D.lcnt, K.lcnt_log2)(D.tick, K.tick);
  if (need_uv) {  // (step 1's e0_ck)
    std::vector<int2> fm;
    std::vector<int4> fh;
    ck_first_tables(K, K.nb > 0 ? (int)((K.bt_off.size() - 1) / K.nb) : 0, fm, fh);
    up(D.first_meta, fm)(D.first_hdr, fh);
  }
  D.cold_q = K.cold_q;
  if (K.cold_q) up(D.cpos, K.cpos);
  room(D.part, (size_t)std::max(K.n_part_rec, 1) * 12);
  if (c->opt.robust_norm && !need_uv)  // (step 2's kernel reads the weights in chunk order; step 1's recomputes them)
    room(D.w, std::max<size_t>(K.src.size(), 1));  // (padded like the rows)
  D.nb = K.nb; D.slots = K.slots; D.n_part_rec = K.n_part_rec; D.max_acc = K.max_acc; D.max_tiles_bt = K.max_tiles_bt;
  D.stride = K.stride; D.n_capped_obs = K.n_capped_obs;
  D.rows = K.rows; D.li_rows = K.li_rows; D.n_chunks = K.n_chunks; D.n_cold_chunks = K.n_cold_chunks;
  D.w_lin_id = -1;
  D.ready = !up.rc && !(locked && c->placer_cancel.load());
  if (up.rc) D.release();
  return !up.rc;
}

// ------------------------------------------------------------------------------------------
// resident power series (series_res): upload, kernel parameters, launch
// ------------------------------------------------------------------------------------------
static int res_upload(povar_ctx* c, povar_ctx::ResDev& D, const ResLayout& R) {
  Uploader up{c};
  up(D.lane_cam, R.lane_cam)(D.lane_seg, R.lane_seg);
  if (!R.uv.empty()) up(D.uv, R.uv);  // (step 2's rows carry none)
  up(D.lslot, R.lslot)(D.oslot, R.oslot)(D.wave_h, R.wave_h)(D.lm_off, R.lm_off)(D.lm_id, R.lm_id)(D.cam_off, R.cam_off)(D.cam_id, R.cam_id)
    (D.cam_zi, R.cam_zi)(D.own_off, R.own_off)(D.own_cam, R.own_cam)(D.own_zi, R.own_zi)(D.own_q, R.own_q)(D.oq_off, R.oq_off)(D.oq_rec, R.oq_rec);
  if (up.rc) return up.rc;
  // granule buffers: tag 0 everywhere (no launch has the number 0), the launch counter starts at 1
  const size_t n_part = (size_t)std::max(R.n_rec, 1) * 12, n_z = (size_t)c->n_cams * 12, n_nrm = (size_t)RES_MAX_WG * 2 * 2;  // (two halves: the norms are double-buffered by term parity)
  if (n_part * sizeof(uint4) >= (1ull << 32)) return fail(-1, "resident series: partial records exceed a buffer descriptor");
  HIP_TRY(D.part.alloc(n_part, &c->bytes));
  HIP_TRY(D.zbuf.alloc(n_z, &c->bytes));
  HIP_TRY(D.nrm.alloc(n_nrm, &c->bytes));
  HIP_TRY(D.launch.alloc(4, &c->bytes));
  HIP_TRY(hipMemset(D.part.p, 0, n_part * sizeof(uint4)));
  HIP_TRY(hipMemset(D.zbuf.p, 0, n_z * sizeof(uint4)));
  HIP_TRY(hipMemset(D.nrm.p, 0, n_nrm * sizeof(uint4)));
  const unsigned one[4] = {1u, 0u, 0u, 0u};
  HIP_TRY(hipMemcpy(D.launch.p, one, sizeof(one), hipMemcpyHostToDevice));
  D.W = R.W; D.NW = R.NW; D.H = R.H; D.R = R.R; D.LS = R.LS; D.n_rec = R.n_rec; D.max_lm = R.max_lm; D.max_cam = R.max_cam;
  D.max_oq = R.max_oq; D.max_own = R.max_own; D.max_chunks = R.max_chunks; D.order = R.order; D.lds_bytes = R.lds_bytes;
  D.ready = true;
  return 0;
}

// the layout for a context: the lightest instantiation that holds it (fewest rows in registers first)
static void res_build_for(int n_cams, int n_lms, const int32_t* lm_off, const int32_t* cam_idx, const double* obs, const std::vector<int>& rank1,
                          const std::vector<int>& slot_of_obs, int wgs, ResLayout& R, const ResShape& sh = ResShape()) {
  if (sh.has_uv) {  // (step 1; series_res_h has no 1024-thread instantiation: POVAR_RES_H_VARIANTS)
    build_res(n_cams, n_lms, lm_off, cam_idx, obs, rank1, slot_of_obs, wgs, 16, 1, 1, 2, 1, R, -1, sh);
    if (R.fits) return;
  }
  build_res(n_cams, n_lms, lm_off, cam_idx, obs, rank1, slot_of_obs, wgs, 8, 2, 1, 4, 2, R, -1, sh);
  // (fixed landmark arrays are charged at the slot capacity: with many cameras per workgroup the 512 slots of one per lane fit
  // where the 1024 of two do not)
  if (!R.fits && sh.lm_fixed) build_res(n_cams, n_lms, lm_off, cam_idx, obs, rank1, slot_of_obs, wgs, 8, 2, 1, 4, 1, R, -1, sh);
}

// The placed rows (povar_ctx::placer) replace the natural order.  Only between linearisations: everything lane-ordered
// that a linearisation leaves behind (V2::lml / lsc / w, the landmark records) belongs to the row order it was built on;
// the landmark mirror V2::lmx is regathered on demand.  wait: block until the host thread is done.
// Returns 1 when the rows were swapped in.
int swap_in_placed_rows(povar_ctx* c, bool wait) {
  if (c->placement != 2) return 0;
  if (!wait && c->placer_state.load(std::memory_order_acquire) < 2) return 0;
  if (c->placer.joinable()) c->placer.join();
  if (c->placer_state.load(std::memory_order_acquire) != 2) {  // the build or an upload failed: stay on the natural order
    c->pl_rows = {};
    c->pl_ck.release(); c->pl_ckh.release();
    c->placement = 0;
    return 0;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));  // nothing in flight reads the old rows
  c->rows = std::move(c->pl_rows);  // (frees the natural rows, leaves pl_rows empty; ldsacc_dp takes cold_src from the context at every launch)
  const povar_ctx::LplRows& r = c->rows;
  V2& v = c->d.v2;
  v.uv = r.uv.p; v.cw = r.cw.p; v.cpos = r.cpos.p; v.lm_pos = r.lm_pos.p; v.lm_of = r.lm_of.p;
  v.of_slot = r.of_slot.p;
  c->lmx_ver = 0;                          // lane-ordered landmark mirror: regather
  c->lml_lin_id = c->lsc_lin_id = -1;
  // the camera-chunk layout belongs to the row order it was derived from
  c->ck.release();
  if (c->pl_ck.ready) std::swap(c->ck, c->pl_ck);
  c->pl_ck.release();
  c->ckh.release();
  if (c->pl_ckh.ready) std::swap(c->ckh, c->pl_ckh);
  c->pl_ckh.release();
  c->ck_tuned = c->ckh_tuned = false;  // (the choice between the E0 kernels is timed again on the new rows)
  c->placement = 3;
  return 1;
}

// The body of povar_ctx::placer: the builder of the lane-per-landmark layout again, with the placement, on copies of the
// caller's arrays (they need not outlive povar_create), then the uploads into pl_rows and the chunk layouts cut from the
// placed rows.  Every HIP call under g_capture_mu (upload / ck_upload: locked).
// The job carries what povar_create alone knows.  n_cams, n_lms, n_slots, e0c_grid, n_hot_acc and opt.device the thread reads
// from the context: povar_create writes each of them once, before it starts the thread, and nothing may write them afterwards.
struct PlaceJob {
  std::vector<int32_t> lm_off, cam_idx;
  std::vector<double> obs;
  std::vector<int> rank1, slot_of_obs, cam_of_rank;
  int64_t rows = 0;     // of the natural order: the placed layout must have as many rows and tiles
  size_t n_tiles = 0;
  bool want_ck = false;
  CkCut cut;
};

// The camera-chunk layouts of one row order V: step 1's, cut for the instantiation that will run it (CkCut) and uploaded into D1,
// then step 2's (64 bytes of LDS per landmark slot, no image coordinates) into D2.  The one caller of build_ck.  H holds the host
// layouts between the stages a call is asked for (`what`): the natural rows are cut before the placement thread starts and
// uploaded after it, the fp32 image points go up between the two steps.  locked: the caller is the placement thread -- a
// cancelled placement stops at the next stage, a failed upload there only leaves that step's layout not ready.
// Returns 0, or the step (1, 2) whose upload failed.
enum : unsigned { CK_CUT1 = 1, CK_UP1 = 2, CK_CUT2 = 4, CK_UP2 = 8, CK_STEP1 = CK_CUT1 | CK_UP1, CK_STEP2 = CK_CUT2 | CK_UP2, CK_BOTH = 15 };
struct CkHost { CkLayout k1, k2; };
static int ck_layouts(povar_ctx* c, const LplLayout& V, const std::vector<int>& cam_of_rank, const CkCut& cut, povar_ctx::CkDev& D1,
                      povar_ctx::CkDev& D2, bool locked, CkHost& H, unsigned what = CK_BOTH) {
  size_t* const bytes = locked ? &c->pl_bytes : &c->bytes;
  const auto go = [&](unsigned stage) { return (what & stage) && !(locked && stage != CK_CUT1 && c->placer_cancel.load()); };
  if (go(CK_CUT1)) {
    const auto tk = std::chrono::steady_clock::now();
    build_ck(V, c->n_cams, c->e0c_grid, cam_of_rank, cut.nw, H.k1, cut.place, cut.hmax, cut.ng, cut.shape1, cut.pack);
    D1.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tk).count();
  }
  if (go(CK_UP1) && !ck_upload(c, D1, H.k1, locked, bytes) && !locked) return 1;
  if (go(CK_CUT2)) build_ck(V, c->n_cams, c->e0c_grid, cam_of_rank, 16, H.k2, cut.place, cut.hmax, 1, cut.shape2);
  if (go(CK_UP2) && !ck_upload(c, D2, H.k2, locked, bytes, false) && !locked) return 2;
  return 0;
}

static void place_rows(povar_ctx* c, std::shared_ptr<PlaceJob> job) {
  const auto t0 = std::chrono::steady_clock::now();
  LplLayout P;
  bool built = true;
  try {  // an allocation failure of this thread must not terminate the caller's process: stay on the natural order
    build_lpl(c->n_cams, c->n_lms, job->lm_off.data(), job->cam_idx.data(), job->obs.data(), job->rank1, job->slot_of_obs,
              (size_t)c->n_slots, c->e0c_grid, c->n_hot_acc, P, true, &c->placer_cancel);
  } catch (...) {
    built = false;
  }
  bool ok = built && !c->placer_cancel.load() && P.rows == job->rows && P.tile.size() == job->n_tiles;
  if (ok) {
    std::lock_guard<std::mutex> lk(g_capture_mu);
    ok = hipSetDevice(c->opt.device) == hipSuccess;
  }
  povar_ctx::LplRows& R = c->pl_rows;
  Uploader up{c, &c->pl_bytes, true, ok ? 0 : -1};
  up(R.uv, P.uv)(R.cw, P.cw)(R.cpos, P.cpos)(R.lm_pos, P.lm_pos)(R.lm_of, P.lm_of)(R.of_slot, P.of_slot)(R.cold_src, P.cold_src);
  ok = !up.rc;
  if (ok && job->want_ck) {  // the camera-chunk layouts of the placed rows (a failure here only leaves e0_lpl in charge)
    try {
      CkHost H;
      ck_layouts(c, P, job->cam_of_rank, job->cut, c->pl_ck, c->pl_ckh, true, H);
    } catch (...) {
      c->pl_ck.ready = false;
      c->pl_ckh.ready = false;
    }
  }
  c->placement_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  c->placer_state.store(ok ? 2 : 3, std::memory_order_release);
}

int check_ctx(povar_ctx* c) {
  if (!c) return fail(-1, "null context");
  HIP_TRY(hipSetDevice(c->opt.device));
  return 0;
}

// Small results come back through one pinned block: an asynchronous copy into pageable memory is staged by the
// runtime (a synchronisation per copy), two of those per API call were most of its latency.
// Layout of the block: [0, 16) the four flags, [64, 64 + 8 * 16) scalars, [256, ...) one 12 n_cams vector.
static int ensure_pin(povar_ctx* c) {
  if (c->pin) return 0;
  c->pin_bytes = 256 + sizeof(double) * 12 * (size_t)std::max(c->n_cams, 1);
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->pin), c->pin_bytes, hipHostMallocDefault));
  return 0;
}

int read_scal_flags(povar_ctx* c, double* h, int n, int (&f)[4]) {
  if (int rc = ensure_pin(c)) return rc;
  if (n > 0) HIP_TRY(hipMemcpyAsync(c->pin + 64, c->scal.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->pin, c->flags.p, sizeof(int) * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::memcpy(f, c->pin, sizeof(int) * 4);
  if (n > 0) std::memcpy(h, c->pin + 64, sizeof(double) * n);
  return 0;
}

int read_flags(povar_ctx* c, int (&f)[4]) { return read_scal_flags(c, nullptr, 0, f); }

int read_scal(povar_ctx* c, double* h, int n) {
  if (int rc = ensure_pin(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->pin + 64, c->scal.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::memcpy(h, c->pin + 64, sizeof(double) * n);
  return 0;
}

int write_cam_vector(povar_ctx* c, double* dst, const double* in, size_t n) {  // completes with the caller's next sync
  if (int rc = ensure_pin(c)) return rc;
  std::memcpy(c->pin + 256, in, sizeof(double) * n);
  HIP_TRY(hipMemcpyAsync(dst, c->pin + 256, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  return 0;
}

int read_cam_vector(povar_ctx* c, double* out, const double* src, size_t n) {
  if (int rc = ensure_pin(c)) return rc;
  HIP_TRY(hipMemcpyAsync(c->pin + 256, src, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::memcpy(out, c->pin + 256, sizeof(double) * n);
  return 0;
}

// Steps 1 to 4 of the teardown order (povar_ctx.hpp); the buffers and then the stream follow as the members are destroyed.
povar_ctx::~povar_ctx() {
  placer_cancel.store(true);  // do not finish a placement nobody will use
  if (placer.joinable()) placer.join();
  (void)hipSetDevice(opt.device);
  if (stream) (void)hipStreamSynchronize(stream);
  if (series_graph) (void)hipGraphExecDestroy(series_graph);
  if (pin) (void)hipHostFree(pin);
  if (comm) (void)ncclCommDestroy(comm);
  for (double* peer : peer_host)
    if (peer && peer != xbuf) (void)hipIpcCloseMemHandle(peer);
  if (xbuf) (void)hipFree(xbuf);
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : tev) (void)hipEventDestroy(e);
}

// ------------------------------------------------------------------------------------------
// povar_create: the phases (each reads the CreatePlan, none decides anything; create_plan.hpp)
// ------------------------------------------------------------------------------------------
// POVAR_LAYOUT_TIMING: the wall time of every phase on stderr (tools/create_time.py reads the lines)
struct Laps {
  using Clock = std::chrono::steady_clock;
  bool on = false;
  Clock::time_point t0 = Clock::now(), last = t0;
  void operator()(const char* what, Clock::time_point now = Clock::now()) {
    if (on) std::fprintf(stderr, "[povar_create] %-26s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};

// what the phases hand to each other
struct CreateJob {
  int n_cams, n_lms;
  int64_t n_obs;
  const int32_t *lm_off, *cam_idx;
  const double* obs;  // (the caller's problem)
  Layout L;
  LayoutTmp LT;
  LplLayout V;      // lane-per-landmark layout of e0_lpl (lpl_layout.hpp): the natural rows, or the rows placed in the call
  CkHost ck_nat;    // placement on a host thread: the chunk layouts cut from the natural rows before that thread starts
  size_t n_cold_lpl = 0, n_cold_q = 0;
  Laps lap;
};

static int check_arguments(povar_ctx** out, int32_t n_cams, int32_t n_lms, int64_t n_obs, const int32_t* lm_offsets,
                           const int32_t* cam_idx, const double* obs, const povar_options* options) {
  if (!out || !lm_offsets || !cam_idx || !obs || !options) return fail(-1, "null argument");
  if (n_cams <= 0 || n_lms <= 0 || n_obs <= 0 || lm_offsets[0] != 0 || lm_offsets[n_lms] != n_obs)
    return fail(-1, "invalid problem sizes");
  for (int l = 0; l < n_lms; ++l) {
    if (lm_offsets[l + 1] < lm_offsets[l]) return fail(-1, "lm_offsets not monotone");
    for (int i = lm_offsets[l]; i < lm_offsets[l + 1]; ++i) {
      if (cam_idx[i] < 0 || cam_idx[i] >= n_cams) return fail(-1, "camera index out of range");
      // duplicate (camera, landmark) pairs abort the reference loader (bal_problem.cpp:227)
      if (i > lm_offsets[l] && cam_idx[i] <= cam_idx[i - 1])
        return fail(-1, "camera indices of a landmark must be strictly ascending");
    }
  }
  return 0;
}

// there must be a device; the resolver wants its CU count (the one query of the device's properties)
static int select_device(const povar_options* options, int* cus) {
  int n_dev = 0;
  HIP_TRY(hipGetDeviceCount(&n_dev));
  if (n_dev <= 0) return fail(-2, "no HIP device: the MI355X path has no CPU fallback");
  HIP_TRY(hipSetDevice(options->device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, options->device));
  *cus = prop.multiProcessorCount;
  return 0;
}

// the stream (on the plan's CU range, if any) and the dynamic LDS of the kernels
static int open_device(povar_ctx* c, const CreatePlan& plan) {
  if (plan.cu_limit > 0) {
    std::vector<uint32_t> mask((plan.device_cus + 31) / 32, 0u);
    for (int i = plan.cu_first; i <= plan.cu_last; ++i) mask[i / 32] |= 1u << (i % 32);
    HIP_TRY(hipExtStreamCreateWithCUMask(&c->stream.s, (uint32_t)mask.size(), mask.data()));
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking));
  }
  // (dynamic LDS of the kernels each unit launches, set on that unit's instantiations)
  HIP_TRY(term_set_lds_all());
  HIP_TRY(lm_set_lds_all());
  return 0;
}

// part A of the layout and the counts that follow from it
static void layout_part_a(povar_ctx* c, const CreatePlan& plan, CreateJob& J) {
  build_layout_a(J.n_cams, J.n_lms, J.lm_off, J.cam_idx, J.L, J.LT);
  J.lap("slots, camera ranks");
  c->n_bins = J.L.n_bins; c->n_slots = J.L.n_bins * WAVE; c->n_items = (int)J.L.item_cam.size(); c->n_long = (int)J.L.long_lm.size();
  c->n_reg_blocks = grid_for(c->n_slots, LM_BLOCK); c->n_cam_blocks = grid_for(J.n_cams, K9_CAMS);
  c->slot_of_obs = J.L.slot_of_obs;
  c->e0c_bins_per_wg = std::max((c->n_bins + plan.e0_wgs - 1) / plan.e0_wgs, 1);
  c->e0c_grid = (c->n_bins + c->e0c_bins_per_wg - 1) / c->e0c_bins_per_wg;
  c->n_hot = std::min(J.n_cams, HOT_MAX);
}

// The lane-per-landmark rows.  Placed on a host thread (place_mode 2), the chunk layouts of the placed rows arrive with them --
// half a second later on venice-1778, i.e. after the first two hundred LM iterations.  e0_ck does not care which order the
// lane-per-landmark rows are in (its own bank placement is what counts: 16.0 k terms/s on the natural rows, 15.9 k
// without its placement on either; profiles/r05_experiments.txt), so step 1's layout is cut HERE from the natural
// rows -- before the host thread starts: the two would share the CPUs -- for e0_ck from the first solve on (0.09 s of
// povar_create; `bal` on venice: 96 -> 62 us per term).  POVAR_CKH_EARLY=1: step 2's instance likewise.
static void build_rows(povar_ctx* c, const CreatePlan& plan, CreateJob& J) {
  build_lpl(J.n_cams, J.n_lms, J.lm_off, J.cam_idx, J.obs, J.L.cam_hot, J.L.slot_of_obs, (size_t)c->n_slots, c->e0c_grid, c->n_hot_acc, J.V,
            plan.place_mode == 1);
  J.lap("build_lpl (lane/landmark)");
  c->placement = plan.place_mode;
  if (plan.place_mode != 2 || J.V.tile.empty()) return;
  if (plan.want_ck) {
    ck_layouts(c, J.V, J.L.hot_cams, plan.cut, c->ck, c->ckh, false, J.ck_nat, CK_CUT1 | (plan.ckh_early ? CK_CUT2 : 0u));
    J.lap("camera-chunk layout(s) from the natural rows");
  }
  // the same builder again, with the placement, on copies of the caller's arrays (they need not outlive this call)
  auto job = std::make_shared<PlaceJob>();
  job->lm_off.assign(J.lm_off, J.lm_off + J.n_lms + 1);
  job->cam_idx.assign(J.cam_idx, J.cam_idx + J.n_obs);
  job->obs.assign(J.obs, J.obs + 2 * J.n_obs);
  job->rank1 = J.L.cam_hot; job->slot_of_obs = J.L.slot_of_obs; job->cam_of_rank = J.L.hot_cams;
  job->rows = J.V.rows; job->n_tiles = J.V.tile.size();
  job->want_ck = plan.want_ck; job->cut = plan.cut;
  c->placer_state.store(1);
  c->placer = std::thread(place_rows, c, job);
  J.lap("row placement handed to a host thread");
}

static int upload_rows(povar_ctx* c, const CreatePlan& plan, CreateJob& J) {
  const LplLayout& V = J.V;
  if (V.max_slots > c->n_hot_acc) return fail(-1, "lpl layout: workgroup camera set exceeds the LDS capacity");
  c->v2_rows = V.rows; c->v2_max_slots = V.max_slots; c->v2_n_global = V.n_global; c->v2_strategy = V.strategy; c->v2_n_tail = V.n_tail;
  c->n_cold3 = (int64_t)V.cold_lm.size();
  Uploader up{c};
  up(c->rows.uv, V.uv)(c->rows.cw, V.cw)(c->rows.cpos, V.cpos)(c->rows.lm_pos, V.lm_pos)(c->rows.lm_of, V.lm_of)(c->rows.of_slot, V.of_slot)
    (c->v2_tile, V.tile)(c->v2_seg, V.seg)(c->v2_wg_tile_off, V.wg_tile_off)(c->v2_wg_cam_off, V.wg_cam_off)(c->v2_wg_cams, V.wg_cams)
    (c->v2_wg_slot_rec, V.wg_slot_rec)(c->v2_part_range, V.part_range)(c->c3_lm, V.cold_lm)(c->c3_range, V.cold_range)(c->rows.cold_src, V.cold_src);
  if (up.rc) return up.rc;
  J.n_cold_q = (size_t)V.cold_rows * WAVE;
  J.n_cold_lpl = V.cold_lm.size();
  c->q_rows = plan.q_rows >= 0 ? plan.q_rows == 1 : (double)V.cold_lm.size() >= 0.20 * (double)std::max<int64_t>(J.n_obs, 1);
  const int nt = (int)V.tile.size();
  HIP_TRY(c->v2_lmrec.alloc((size_t)std::max(nt, 1) * LPL_REC_H * WAVE, &c->bytes));  // 9 entries used by step 1
  HIP_TRY(c->v2_lmx.alloc((size_t)std::max(nt, 1) * WAVE, &c->bytes));
  HIP_TRY(c->v2_lml.alloc((size_t)std::max(nt, 1) * WAVE, &c->bytes));
  HIP_TRY(c->v2_lsc.alloc((size_t)std::max(nt, 1) * WAVE, &c->bytes));
  HIP_TRY(c->v2_part.alloc((size_t)std::max(V.n_part_rec, 1) * 12, &c->bytes));
  HIP_TRY(c->c3_h.alloc(4 * std::max<size_t>(V.cold_lm.size(), 1), &c->bytes));
  if (c->opt.robust_norm) HIP_TRY(c->v2_w.alloc((size_t)std::max<int64_t>(c->v2_rows, 1) * WAVE, &c->bytes));
  return 0;
}

// the camera-chunk layouts of the rows in use, and what the fp32 terms keep beside step 1's
static int chunk_layouts(povar_ctx* c, const CreatePlan& plan, CreateJob& J) {
  const LplLayout& V = J.V;
  const int n_cams = J.n_cams, nt = (int)V.tile.size();
  const bool want = plan.want_ck && !V.tile.empty();
  static const char* const failed[] = {nullptr, "camera-chunk layout: upload failed", "camera-chunk layout (step 2): upload failed"};
  if (want) {
    if (int rc = upload(c->ck_zero_range, std::vector<int2>((size_t)n_cams, make_int2(0, 0)), c)) return rc;
    if (plan.place_mode == 2) {  // (cut in build_rows; the layouts of the placed rows, and step 2's without POVAR_CKH_EARLY, come from the host thread)
      if (int step = ck_layouts(c, V, J.L.hot_cams, plan.cut, c->ck, c->ckh, false, J.ck_nat, CK_UP1 | (plan.ckh_early ? CK_UP2 : 0u))) return fail(-1, failed[step]);
      J.lap("camera-chunk layouts (natural rows): uploads");
    } else {
      CkHost H;
      if (int step = ck_layouts(c, V, J.L.hot_cams, plan.cut, c->ck, c->ckh, false, H, CK_STEP1)) return fail(-1, failed[step]);
      if (c->fp32_terms && c->ck.ready && !c->ck.packed) {  // fp32 image points where the rows do not pack (8 bytes per entry)
        std::vector<float2> u32(H.k1.uv.size());
        for (size_t i = 0; i < u32.size(); ++i) u32[i] = make_float2((float)H.k1.uv[i].x, (float)H.k1.uv[i].y);
        if (int rc = upload(c->ck32_uv, u32, c)) return rc;
      }
      if (int step = ck_layouts(c, V, J.L.hot_cams, plan.cut, c->ck, c->ckh, false, H, CK_STEP2)) return fail(-1, failed[step]);
      J.lap("camera-chunk layouts");
    }
  }
  if (c->fp32_terms) {
    // e0_ck_f32 addresses its partial records with 32-bit byte offsets (rec * 96) through a descriptor of their exact size:
    // the layout must keep them under 2^31 bytes -- checked here, not assumed (e0_ck's descriptor spans 2^31 whatever the size)
    const char* why = !want || !c->ck.ready ? "the camera-chunk layout could not be built for this problem"
                      : (uint64_t)c->ck.part.n * sizeof(double) >= (1ull << 31) ? "the partial records exceed 2^31 bytes"
                      : (uint64_t)c->ck.src.n * sizeof(float2) >= (1ull << 32) ? "the chunk rows exceed 2^32 bytes"
                      : ck32_lds_bytes(c->ck.slots, c->ck.max_acc) > (size_t)CK_LDS_BYTES ? "the landmark batches exceed the LDS"
                      : nullptr;
    if (why) return fail(-1, std::string("POVAR_FLAG_FP32_TERMS: ") + why);
    HIP_TRY(c->ck32_lmrec.alloc((size_t)std::max(nt, 1) * 9 * WAVE, &c->bytes));
    HIP_TRY(c->ck32_pimg.alloc((size_t)n_cams * 12, &c->bytes));
  }
  c->d.v2 = V2{c->rows.uv.p, c->rows.cw.p, c->rows.cpos.p, c->v2_w.p, c->v2_tile.p, c->v2_seg.p, c->v2_lmrec.p,
               c->rows.lm_of.p, c->v2_lmx.p, c->v2_lml.p, c->v2_lsc.p, c->rows.lm_pos.p, c->rows.of_slot.p, c->v2_wg_tile_off.p, c->v2_wg_cam_off.p, c->v2_wg_cams.p,
               c->v2_wg_slot_rec.p, nt, V.hubs};
  J.V = LplLayout();  // (the host copies of the rows and of their chunk layouts are done with)
  J.ck_nat = CkHost();
  return 0;
}

// resident power series (res_layout.hpp), both steps: the one caller of build_res (through res_build_for)
static int resident_layouts(povar_ctx* c, const CreatePlan& plan, CreateJob& J) {
  if (c->res_mode == 0 || J.n_obs > plan.res_max_obs) return 0;
  const auto tr = std::chrono::steady_clock::now();
  HIP_TRY(res_set_lds_all());
  ResLayout R;
  res_build_for(J.n_cams, J.n_lms, J.lm_off, J.cam_idx, J.obs, J.L.cam_hot, J.L.slot_of_obs, plan.res_wgs, R);
  if (R.fits && res_variant_exists(R.NW, R.H, R.R, R.LS)) {
    if (int rc = res_upload(c, c->res, R)) return rc;
    c->res.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr).count();
  }
  J.lap("resident-series layout");
  // step 2 (series_res_h): step 1's instance where its cut fits the step-2 LDS formula and series_res_h has the shape;
  // else a cut of its own (64 bytes per landmark slot at the instantiation's slot capacity, no image points)
  const auto th = std::chrono::steady_clock::now();
  if (c->res.ready && res_shared_fits(R) && res_variant_exists(R.NW, R.H, R.R, R.LS, true)) {
    c->res_h_shared = true;
    c->res_h_lds = res_lds_bytes_of(R, res_shape_step2());
  } else {
    ResLayout RH;
    res_build_for(J.n_cams, J.n_lms, J.lm_off, J.cam_idx, J.obs, J.L.cam_hot, J.L.slot_of_obs, plan.res_wgs, RH, res_shape_step2());
    if (RH.fits && res_variant_exists(RH.NW, RH.H, RH.R, RH.LS, true)) {
      if (int rc = res_upload(c, c->res_h, RH)) return rc;
      c->res_h_lds = RH.lds_bytes;
    }
  }
  c->res_h_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th).count();
  J.lap("resident-series layout (step 2)");
  return 0;
}

// part B's arrays, then the state and scratch of the lane-per-observation kernels (allocated, not uploaded), zeroed where read first
static int upload_lane_obs(povar_ctx* c, const CreatePlan& plan, CreateJob& J) {
  const Layout& L = J.L;
  const int n_cams = J.n_cams, n_lms = J.n_lms;
  const int64_t n_obs = J.n_obs;
  const size_t n_cold_lpl = J.n_cold_lpl, n_cold_q = J.n_cold_q;
  Uploader up{c};
  up(c->uv, L.uv)(c->cam, L.cam)(c->lm, L.lm)(c->meta, L.meta)(c->hot_cams, L.hot_cams)(c->cam_hot, L.cam_hot)(c->cc_slot, L.cc_slot)(c->cc_lm, L.cc_lm)
    (c->cc_item_off, L.cc_item_off)(c->cc_cam_item_off, L.cc_cam_item_off)(c->long_lm, L.long_lm)(c->long_first, L.long_first)(c->long_cnt, L.long_cnt)
    (c->cm_slot, L.cm_slot)(c->cm_lm, L.cm_lm)(c->cm_uv, L.cm_uv)(c->item_off, L.item_off)(c->item_cam, L.item_cam)(c->cam_item_off, L.cam_item_off);
  if (up.rc) return up.rc;
  J.lap("uploads (lane/obs)");
  const size_t nc = n_cams, nl = n_lms, ns = c->n_slots, ni = std::max(c->n_items, 1);
  const size_t n_part = (size_t)(c->n_reg_blocks + c->n_long) * 4;
  auto room = [&](auto& buf, size_t count) { return buf.alloc(count, &c->bytes); };
  HIP_TRY(room(c->cams4, 3 * nc)); HIP_TRY(room(c->cams_lin4, 3 * nc)); HIP_TRY(room(c->cams_bak4, 3 * nc));
  HIP_TRY(room(c->lms4, nl)); HIP_TRY(room(c->lms_lin4, nl)); HIP_TRY(room(c->lms_bak4, nl)); HIP_TRY(room(c->jl_scale4, nl));
  HIP_TRY(room(c->hll_inv, 9 * nl)); HIP_TRY(room(c->lmrec, 16 * nl));
  HIP_TRY(room(c->sw, ns)); HIP_TRY(room(c->rres, ns)); HIP_TRY(room(c->q4, ns));
  HIP_TRY(room(c->sigma, 12 * nc)); HIP_TRY(room(c->diag2, 12 * nc)); HIP_TRY(room(c->G, 40 * nc)); HIP_TRY(room(c->binv, 144 * nc));
  HIP_TRY(room(c->b, 12 * nc)); HIP_TRY(room(c->tmp, 12 * nc)); HIP_TRY(room(c->accum, 12 * nc)); HIP_TRY(room(c->z, 12 * nc)); HIP_TRY(room(c->y, 12 * nc));
  HIP_TRY(room(c->inc, 12 * nc));
  HIP_TRY(room(c->item_part, 12 * ni)); HIP_TRY(room(c->item_partG, 40 * ni)); HIP_TRY(room(c->cm_h, 4 * (size_t)n_obs)); HIP_TRY(room(c->ncw, 13 * nc));
  c->n_cold = (int64_t)L.cc_slot.size();
  c->n_cold_items = (int)L.cc_item_off.size() - 1;
  std::vector<int2> range(n_cams);
  for (int k = 0; k < n_cams; ++k)
    range[k] = make_int2(L.cc_item_off[L.cc_cam_item_off[k]], L.cc_item_off[L.cc_cam_item_off[k + 1]]);
  if (up(c->cc_cam_range, range)(c->cold_pos, L.cold_pos).rc) return up.rc;
  if (!L.long_lm.empty()) {
    c->n_cold2 = (int64_t)L.c2_lm.size();
    if (up(c->c2_lm, L.c2_lm)(c->c2_pos, L.c2_pos)(c->c2_range, L.c2_range).rc) return up.rc;
    HIP_TRY(c->c2_h.alloc(4 * std::max<size_t>(L.c2_lm.size(), 1), &c->bytes));
    // (e0_lpl has no long/short distinction and always uses this cold view)
    c->long_in_kernel = c->use_lpl || !plan.long_separate;
  }
  std::vector<int> s0(n_lms, 0), cnt(n_lms, 0);
  for (int l = 0; l < n_lms; ++l) {
    cnt[l] = J.lm_off[l + 1] - J.lm_off[l];
    s0[l] = cnt[l] > 0 ? L.slot_of_obs[J.lm_off[l]] : 0;
  }
  if (up(c->lm_slot0, s0)(c->lm_cnt_dev, cnt).rc) return up.rc;
  J.lap("uploads, allocations (lane/obs)");
  // scatter scalars of the cold observations: one buffer, sized for the largest of the cold views
  HIP_TRY(c->q4c.alloc(std::max<size_t>(std::max(std::max(std::max(L.cc_slot.size(), L.c2_lm.size()), n_cold_lpl), n_cold_q), 1), &c->bytes));
  HIP_TRY(room(c->cc_h, 4 * std::max<size_t>(L.cc_slot.size(), 1))); HIP_TRY(room(c->cc_part, 12 * (size_t)std::max(c->n_cold_items, 1)));
  HIP_TRY(room(c->hot_part, (size_t)c->e0c_grid * c->n_hot_acc * 12));
  HIP_TRY(room(c->hot_rec, (size_t)std::max(n_cams, HOT_MAX) * HOT_REC_STRIDE));  // every camera, in popularity order
  HIP_TRY(room(c->zimg, (size_t)n_cams * 12));  // z alone, by rank: what e0_ck gathers Z from (Dp::zimg)
  HIP_TRY(room(c->norm_part, 2 * (size_t)std::max(c->n_cam_blocks, n_cams))); HIP_TRY(room(c->norms, 4)); HIP_TRY(room(c->flags, 4));
  HIP_TRY(room(c->part, n_part * 2 + 8 * 1024)); HIP_TRY(room(c->scal, 8));  // + one slot set per workgroup of the lane-per-landmark kernels
  HIP_TRY(room(c->stage, std::max(3 * nl, 144 * nc)));
  HIP_TRY(room(c->fixed_mask, std::max<size_t>(nc, 1)));  // (povar_set_fixed_cameras: no camera is fixed)
  c->fixed_next.assign(nc, 0);
  HIP_TRY(hipMemsetAsync(c->fixed_mask.p, 0, std::max<size_t>(nc, 1), c->stream));
  HIP_TRY(room(c->cam_row, std::max<size_t>(nc, 1)));  // (povar_set_dense_compaction: the first preparation fills it)
  HIP_TRY(hipMemsetAsync(c->flags.p, 0, sizeof(int) * 4, c->stream));
  HIP_TRY(hipMemsetAsync(c->lms4.p, 0, sizeof(double4) * nl, c->stream));
  HIP_TRY(hipMemsetAsync(c->cams4.p, 0, sizeof(double4) * 3 * nc, c->stream));
  HIP_TRY(hipMemsetAsync(c->y.p, 0, sizeof(double) * 12 * nc, c->stream));
  HIP_TRY(hipMemsetAsync(c->q4.p, 0, sizeof(double4) * ns, c->stream));
  HIP_TRY(hipMemsetAsync(c->sw.p, 0, sizeof(double) * ns, c->stream));
  HIP_TRY(hipMemsetAsync(c->rres.p, 0, sizeof(double4) * ns, c->stream));
  // every initialisation above (uploads on the null stream, memsets on the context's non-blocking
  // stream) is complete before the context is handed out
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

static void fill_dp(povar_ctx* c) {
  Dp& d = c->d;
  d.n_cams = c->n_cams; d.n_lms = c->n_lms; d.n_bins = c->n_bins; d.n_items = c->n_items;
  d.n_long = c->n_long; d.n_reg_blocks = c->n_reg_blocks;
  d.uv = c->uv.p; d.cam = c->cam.p; d.lm = c->lm.p; d.meta = c->meta.p;
  d.long_lm = c->long_lm.p; d.long_first = c->long_first.p; d.long_cnt = c->long_cnt.p;
  d.cm_slot = c->cm_slot.p; d.cm_lm = c->cm_lm.p; d.cm_uv = c->cm_uv.p;
  d.item_off = c->item_off.p; d.item_cam = c->item_cam.p; d.cam_item_off = c->cam_item_off.p;
  d.cams4 = c->cams4.p; d.cams_lin4 = c->cams_lin4.p; d.lms4 = c->lms4.p; d.lms_lin4 = c->lms_lin4.p;
  d.jl_scale4 = c->jl_scale4.p; d.hll_inv = c->hll_inv.p; d.lmrec = c->lmrec.p;
  d.cmv = CmView{c->cm_slot.p, c->cm_h.p, c->n_obs, c->item_off.p, c->cam_item_off.p, c->item_part.p, c->n_items, nullptr};
  d.hot_part = nullptr; d.cam_hot = c->cam_hot.p; d.n_hot_acc = c->n_hot_acc; d.n_hot_wg = c->e0c_grid;
  d.hot_rec = c->hot_rec.p;
  d.zimg = c->zimg.p;
  d.hot_cams = c->hot_cams.p; d.n_hot = std::min(c->n_cams, HOT_MAX);
  d.part_range = nullptr;
  d.p2p_peer = nullptr; d.p2p_epoch = nullptr; d.p2p_world = 1; d.p2p_rank = 0;
  d.sw = c->sw.p; d.rres = c->rres.p; d.q4 = c->q4.p; d.q4c = nullptr; d.cold_pos = nullptr; d.long_in_kernel = 0; d.tiles = nullptr;
  d.sigma = c->sigma.p; d.diag2 = c->diag2.p; d.G = c->G.p; d.binv = c->binv.p; d.b = c->b.p;
  d.tmp = c->tmp.p; d.accum = c->accum.p; d.z = c->z.p; d.y = c->y.p; d.inc = c->inc.p;
  d.item_part = c->item_part.p; d.item_partG = c->item_partG.p; d.cm_h = c->cm_h.p; d.n_obs = c->n_obs;
  d.flags = c->flags.p; d.norm_part = c->norm_part.p; d.norms = c->norms.p;
  d.lm_slot0 = c->lm_slot0.p; d.lm_cnt = c->lm_cnt_dev.p;
  d.sa = 0; d.sb = 1; d.eps = c->opt.jacobi_scaling_eps; d.huber = c->opt.huber_parameter;
  d.lambda_lm = 0; d.robust = c->opt.robust_norm; d.scale_jl = 1;
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------

extern "C" {

const char* povar_last_error(void) { return g_err.c_str(); }

int povar_device_count(void) {
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  return n;
}

int povar_device_cu_count(int32_t device) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  return prop.multiProcessorCount;
}

int povar_shard_range(int32_t n_lms, const int32_t* lm_offsets, int32_t world, int32_t rank,
                      int32_t* lm_begin, int32_t* lm_end) {
  if (!lm_offsets || world < 1 || rank < 0 || rank >= world) return fail(-1, "bad shard arguments");
  // contiguous landmark ranges balanced by observation count (prefix sum over k_l): boundary r is
  // the first landmark whose observations start at or after r/world of the total.
  const int64_t n_obs = lm_offsets[n_lms];
  auto bound = [&](int r) -> int32_t {
    if (r <= 0) return 0;
    if (r >= world) return n_lms;
    const int64_t target = n_obs * (int64_t)r / world;
    return (int32_t)(std::lower_bound(lm_offsets, lm_offsets + n_lms + 1, (int32_t)target) - lm_offsets);
  };
  *lm_begin = bound(rank);
  *lm_end = bound(rank + 1);
  return 0;
}

int povar_create(povar_ctx** out, int32_t n_cams, int32_t n_lms, int64_t n_obs,
                 const int32_t* lm_offsets, const int32_t* cam_idx, const double* obs,
                 const povar_options* options) {
  CreateJob J{n_cams, n_lms, n_obs, lm_offsets, cam_idx, obs};
  if (int rc = check_arguments(out, n_cams, n_lms, n_obs, lm_offsets, cam_idx, obs, options)) return rc;
  const auto t_checked = Laps::Clock::now();
  int device_cus = 0;
  if (int rc = select_device(options, &device_cus)) return rc;
  CreatePlan plan;
  std::string refusal;
  if (int rc = resolve_create_plan(plan, *options, n_cams, n_obs, device_cus, &refusal)) return fail(rc, refusal);
  J.lap.on = plan.timing;
  J.lap("argument checks", t_checked);

  // every early return below destroys the context (declared before the Joiner of the second host thread: that thread is
  // joined first); *out takes it over at the end
  std::unique_ptr<povar_ctx, decltype(&povar_destroy)> owner(new povar_ctx(), &povar_destroy);
  povar_ctx* const c = owner.get();
  c->opt = *options;
  c->n_cams = n_cams; c->n_lms = n_lms; c->n_obs = n_obs;
  c->lm_off.assign(lm_offsets, lm_offsets + n_lms + 1);
  for (int l = 0; l < n_lms; ++l) c->has_empty_lm |= lm_offsets[l + 1] == lm_offsets[l];
  static_cast<CtxSwitches&>(*c) = plan;  // the switches the other units read
  c->opt.e0_mode = plan.e0_mode;
  if (int rc = open_device(c, plan)) return rc;
  J.lap("device, stream");
  layout_part_a(c, plan, J);

  // The arrays of the lane-per-observation kernels (part B) are built on a second host thread while this one builds
  // and uploads the lane-per-landmark layout: the two only share the slot numbers and camera ranks of part A.
  std::atomic<bool> part_b_failed{false};
  std::thread part_b([&]() {
    try {
      build_layout_b(n_cams, n_lms, lm_offsets, cam_idx, obs, plan.n_hot_acc, J.L, J.LT);
    } catch (...) {  // (an allocation failure of this thread must not terminate the caller's process)
      part_b_failed.store(true);
    }
  });
  struct Joiner {  // every early return below must wait for the thread
    std::thread& t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } joiner{part_b};
  build_rows(c, plan, J);
  if (int rc = upload_rows(c, plan, J)) return rc;
  if (int rc = chunk_layouts(c, plan, J)) return rc;
  J.lap("uploads (lane/landmark)");
  if (int rc = resident_layouts(c, plan, J)) return rc;
  part_b.join();
  if (part_b_failed.load()) return fail(-4, "out of host memory while building the lane-per-observation layout");
  J.lap("wait for the lane/obs arrays");
  if (int rc = upload_lane_obs(c, plan, J)) return rc;
  fill_dp(c);
  J.lap("allocations, memsets, sync");
  c->create_ms = std::chrono::duration<double, std::milli>(Laps::Clock::now() - J.lap.t0).count();
  if (plan.timing) std::fprintf(stderr, "[povar_create] total %.1f ms\n", c->create_ms);
  *out = owner.release();
  return 0;
}

void povar_destroy(povar_ctx* c) {
  if (c) delete c;
}

int64_t povar_device_bytes(povar_ctx* c) { return c ? (int64_t)c->bytes : 0; }

int povar_synchronize(povar_ctx* c) {
  if (int rc = check_ctx(c)) return rc;
  if (int rc = res_verify(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return 0;
}

int povar_timings_enable(povar_ctx* c, int32_t enable) {
  if (int rc = check_ctx(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->timings_on = enable != 0;
  c->tev_used = 0;
  c->tsum = povar_timings_info{};
  return 0;
}

int povar_timings(povar_ctx* c, povar_timings_info* out) {
  if (int rc = check_ctx(c)) return rc;
  if (!out) return fail(-1, "null argument");
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i + 1 < c->tev_used; i += 2) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->tev[i], c->tev[i + 1]));
    double* slot[5] = {&c->tsum.linearize_ms, &c->tsum.prepare_ms, &c->tsum.solve_ms, &c->tsum.apply_ms, &c->tsum.other_ms};
    int64_t* cnt[5] = {&c->tsum.linearize_calls, &c->tsum.prepare_calls, &c->tsum.solve_calls, &c->tsum.apply_calls, &c->tsum.other_calls};
    const int k = c->tev_kind[i];
    if (k >= 0 && k < 5) { *slot[k] += ms; ++*cnt[k]; }
  }
  c->tev_used = 0;
  *out = c->tsum;
  return 0;
}

int povar_get_layout_info(povar_ctx* c, povar_layout_info* out) {
  if (!c || !out) return fail(-1, "null argument");
  out->grid = c->e0c_grid;
  out->lds_slots = c->v2_max_slots;
  out->n_global = c->v2_n_global;
  out->n_tail = c->v2_n_tail;
  out->n_tiles = c->d.v2.n_tiles;
  out->n_rows = c->v2_rows;
  out->n_cold = c->n_cold3;
  out->n_obs = c->n_obs;
  out->lane_per_landmark = c->use_lpl ? 1 : 0;
  out->create_ms = c->create_ms;
  out->strategy = c->v2_strategy;
  out->hubs = c->d.v2.hubs;
  out->placement = c->placement;
  out->placement_ms = c->placer_state.load(std::memory_order_acquire) >= 2 ? c->placement_ms : 0.0;
  const TermPlan p1 = term_plan(c, 1, TermUse::series), p2 = term_plan(c, 2, TermUse::series);
  out->e0_kernel = p1.e0 == E0K::ck_det ? CK_VARIANTS + 1 : p1.variant;  // (e0_ck_f32 runs the layout of variant 1)
  out->ck_ready = c->ck.ready ? 1 : 0;
  out->ck_batches = c->ck.nb;
  out->ck_slots = c->ck.slots;
  out->ck_tiles_max = c->ck.max_tiles_bt;
  out->ck_rows = c->ck.rows;
  out->ck_chunks = c->ck.n_chunks;
  out->ck_cold_chunks = c->ck.n_cold_chunks;
  out->ck_part_rec = c->ck.n_part_rec;
  out->ck_build_ms = c->ck.build_ms;
  out->e0_auto = c->ck_auto ? (c->ck_tuned ? 2 : 1) : 0;
  out->tune_lpl_us = c->ck_tune_us[0];
  out->tune_ck_us = c->ck_tune_us[1];
  out->e0_kernel_h = p2.e0 == E0K::ck_h_det ? 2 : p2.e0 == E0K::ck_h ? 1 : 0;
  out->ckh_ready = c->ckh.ready ? 1 : 0;
  out->ckh_batches = c->ckh.nb;
  out->ckh_slots = c->ckh.slots;
  out->ckh_chunks = c->ckh.n_chunks;
  out->ckh_cold_chunks = c->ckh.n_cold_chunks;
  out->e0_auto_h = c->ck_auto ? (c->ckh_tuned ? 2 : 1) : 0;
  out->tune_lpl_h_us = c->ckh_tune_us[0];
  out->tune_ck_h_us = c->ckh_tune_us[1];
  out->res_ready = c->res.ready ? 1 : 0;
  out->res_active = !c->joint && res_active(c, false) ? 1 : 0;  // (the step-1 answer: 0 while the joint system is the prepared one)
  out->res_auto = c->res_mode < 0 ? (c->res_tune[0].tuned ? 2 : 1) : 0;
  out->res_wgs = c->res.W;
  out->res_waves = c->res.NW;
  out->res_rows = c->res.H;
  out->res_rounds = c->res.R;
  out->res_max_oq = c->res.max_oq;
  out->res_records = c->res.n_rec;
  out->res_max_cams = c->res.max_cam;
  out->res_max_lms = c->res.max_lm;
  out->res_max_chunks = c->res.max_chunks;
  out->res_order = c->res.order;
  out->res_lds_bytes = (int32_t)c->res.lds_bytes;
  out->res_build_ms = c->res.build_ms;
  out->tune_terms_us = c->res_tune[0].us[0];
  out->tune_res_us = c->res_tune[0].us[1];
  out->res_failed = c->res_failed ? 1 : 0;
  out->ck_packed = c->ck.ready && c->ck.packed ? 1 : 0;
  out->ck_cold_q = c->ck.ready && c->ck.cold_q ? 1 : 0;
  out->ckh_stride = c->ckh.ready ? c->ckh.stride : 0;
  out->ckh_accumulators = c->ckh.ready ? c->ckh.max_acc : 0;
  out->ckh_capped_obs = c->ckh.ready ? c->ckh.n_capped_obs : 0;
  out->fp32_terms = c->fp32_last;
  {
    const bool ready = res_ready(c, true);
    const povar_ctx::ResDev& D = res_dev(c, true);
    out->res_ready_h = ready ? 1 : 0;
    out->res_active_h = res_active(c, true) ? 1 : 0;
    out->res_auto_h = c->res_mode < 0 ? (c->res_tune[1].tuned ? 2 : 1) : 0;
    out->res_shared_h = ready && c->res_h_shared ? 1 : 0;
    out->res_wgs_h = ready ? D.W : 0;
    out->res_waves_h = ready ? D.NW : 0;
    out->res_rows_h = ready ? D.H : 0;
    out->res_rounds_h = ready ? D.R : 0;
    out->res_lds_bytes_h = ready ? (int32_t)c->res_h_lds : 0;
    out->res_build_h_ms = c->res_h_build_ms;
    out->tune_terms_h_us = c->res_tune[1].us[0];
    out->tune_res_h_us = c->res_tune[1].us[1];
  }
  return 0;
}

int povar_layout_finalize(povar_ctx* c, int32_t wait) {
  if (int rc = check_ctx(c)) return rc;
  if (c->placement == 2) {
    const int rc = swap_in_placed_rows(c, wait != 0);
    if (rc < 0) return rc;
    if (rc == 1) {
      // what the current linearisation left in the old row order is gone with it
      c->linearized = c->linearized_h = false;
      c->err_memo.valid = false;
    }
  }
  return c->placement == 1 || c->placement == 3 ? 1 : 0;
}

}  // extern "C"
