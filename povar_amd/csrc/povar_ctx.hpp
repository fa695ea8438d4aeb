// povar_ctx.hpp -- what the translation units of the host side share: the context behind the opaque povar_ctx of
// include/povar_hip.h, error / buffer helpers, launch helpers that are templates, and the declarations of the functions one
// unit defines and another calls.  The host side of the C ABI is cut by concern:
//   povar_create.hip   layout construction and upload, povar_create / povar_destroy, read-back helpers, layout info
//   povar_lm.hip       the stages of an LM iteration: state, cost, linearise, prepare, apply (both steps), exports
//   povar_series.hip   the term loop: E0 / B^-1 launchers, kernel choice by timing, hipGraph, the series entry points
//   povar_comm.hip     exchange steps: RCCL / host-hook all-reduce, the peer-to-peer term exchange
//   povar_sc.hip       explicit-Schur-complement solvers (PCG / CHOLESKY / RIPCG / RICHOLESKY)
//   povar_cov.hip      the covariance calls on CHOLESKY's factor: camera, landmark, observation rows, hat rows, pair blocks
//   cov_plan.hpp       what a covariance call decides on the host alone: argument rules, requests, gauge basis, pivot rule
//   dev_buf.hpp        DevBuf<T>, the self-freeing device allocation every buffer of the context is
// Device code: povar_kernels*.hpp (kernels that are not templates have internal linkage: every unit compiles what it launches).
#pragma once
#include "../../include/povar_hip.h"
#include "dev_buf.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "povar_kernels.hpp"
#include "povar_kernels_joint.hpp"
#include "povar_kernels_lpl.hpp"
#include "povar_kernels_cam.hpp"
#include "povar_kernels_sc.hpp"
#include "povar_kernels_chol.hpp"
#include "lpl_layout.hpp"
#include "ck_layout.hpp"
#include "povar_kernels_ck.hpp"
#include "povar_kernels_ck_det.hpp"
#include "povar_kernels_ck_joint.hpp"
#include "povar_kernels_ck_f32.hpp"
#include "res_layout.hpp"
#include "create_plan.hpp"
#include "cov_plan.hpp"
#include "povar_kernels_res.hpp"

using namespace povar;

inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(-(int)e_ - 1000, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

#define NCCL_TRY(expr)                                                                      \
  do {                                                                                      \
    ncclResult_t e_ = (expr);                                                               \
    if (e_ != ncclSuccess)                                                                  \
      return fail(-(int)e_ - 2000, std::string(#expr) + ": " + ncclGetErrorString(e_));     \
  } while (0)

extern std::mutex g_capture_mu;  // see povar_ctx::placer_cancel (defined in povar_create.hip)
// the row-placement thread (locked) makes every HIP call under g_capture_mu; the caller's thread takes no lock
inline std::unique_lock<std::mutex> capture_lock(bool locked) {
  return locked ? std::unique_lock<std::mutex>(g_capture_mu) : std::unique_lock<std::mutex>();
}

// Ownership: every device buffer of a context is a DevBuf member (dev_buf.hpp) and frees itself; povar_destroy is `delete`.
// Teardown order (~povar_ctx, povar_create.hip):
//   1. cancel and join the placement thread   2. hipSetDevice(opt.device)   3. synchronise the stream
//   4. destroy the graph exec, the pinned block, the communicator, the opened IPC mappings, xbuf and both event vectors
//      (1 to 4: the destructor's body, which runs before any member is destroyed)
//   5. every DevBuf member frees its memory   6. the stream is destroyed (OwnedStream, below)
struct povar_ctx : CtxSwitches {  // (create_plan.hpp: the switches povar_create resolves)
  povar_ctx() = default;
  povar_ctx(const povar_ctx&) = delete;
  ~povar_ctx();
  // destroyed after every buffer: members die in reverse order, so `stream` must stay declared BEFORE the first DevBuf member
  struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    operator hipStream_t() const { return s; }
    ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
  };
  int n_cams = 0, n_lms = 0;
  int64_t n_obs = 0;
  int n_bins = 0, n_slots = 0, n_items = 0, n_long = 0;
  int n_reg_blocks = 0, n_cam_blocks = 0;
  int n_hot = 0, e0c_grid = 0, e0c_bins_per_wg = 0;
  int64_t n_cold = 0;
  int n_cold_items = 0;
  povar_options opt{};
  OwnedStream stream;
  size_t bytes = 0;
  char* pin = nullptr;  // pinned host block of the small read-backs (read_scal_flags)
  size_t pin_bytes = 0;

  std::vector<int> slot_of_obs;  // host copy for exports in the reference's order
  std::vector<int> lm_off;

  // static
  DevBuf<double2> uv, cm_uv, tiles;
  DevBuf<int2> cc_cam_range;  // per camera: (first, end) position of its run in the cold camera-major view
  DevBuf<int> cold_pos;       // per slot: position in the cold view (-1: accumulated in LDS)
  // default mode with long landmarks: e0_lm_cached walks them itself (view "A" of the cold observations)
  DevBuf<int> c2_lm, c2_pos;
  DevBuf<int2> c2_range;
  DevBuf<double> c2_h;
  int64_t n_cold2 = 0;
  bool long_in_kernel = false;
  // lane-per-landmark layout of e0_lpl (struct V2)
  // the arrays that belong to a row order: the ones in use and the placed ones a host thread uploads (swap_in_placed_rows)
  struct LplRows {
    DevBuf<double2> uv;
    DevBuf<int> cw, cpos, lm_pos, lm_of, of_slot;
    DevBuf<int> cold_src;  // CmView::src of the lane-per-landmark cold view (row-major q: lpl_cold_q)
  } rows, pl_rows;
  DevBuf<int> v2_seg, v2_wg_tile_off, v2_wg_cam_off, v2_wg_cams, v2_wg_slot_rec, c3_lm;
  DevBuf<int2> v2_part_range, c3_range;
  // Cold observations of the lane-per-landmark kernels leave q row-major, side by side with the other lanes of their
  // row, and the per-camera kernels gather it -- instead of one scattered 32-byte store per lane into the camera-major
  // view (a third of the term on final-13682 with 24 % cold observations).  The gather costs the per-camera kernel a
  // dependent load, so graphs with fewer cold observations keep the direct store: from 20 % on (POVAR_COLD_Q_ROWS=0|1).
  // venice-1778 shape, cold share -> terms/s direct / row-major: Zipf(1) 3 % 14.8 / 14.3 k, 25 % long tracks 11 % 8.5 / 8.1 k,
  // Zipf(0.5) 18 % 9.76 / 9.77 k, uniform 31 % 6.46 / 7.11 k; final-13682 24 % 1.34 / 1.50 k.
  bool q_rows = false;
  DevBuf<double> c3_h, v2_part;
  int64_t n_cold3 = 0;
  int v2_max_slots = 0, v2_n_global = 0, v2_n_tail = 0, v2_strategy = 0;
  DevBuf<int4> v2_tile;
  DevBuf<double> v2_w, v2_lmrec;
  int64_t v2_rows = 0;
  // LDS bank placement of the rows (lpl_layout.hpp) on a host thread: povar_create returns on the natural row order,
  // the placed rows are swapped in at the next linearisation after they are ready (or by povar_layout_finalize).
  // POVAR_LPL_PLACE = sync | async | none; default: async from 2^20 observations on, sync below
  std::thread placer;
  std::atomic<int> placer_state{0};  // 0 no thread, 1 running, 2 rows uploaded and ready, 3 failed
  std::atomic<bool> placer_cancel{false};  // povar_destroy: do not finish a placement nobody will use
  // A hipMalloc / hipMemcpy of the host thread while the caller's thread captures the term loop into a hipGraph
  // invalidates the capture ("operation failed due to a previous error during capture", also in thread-local capture
  // mode): the thread makes its HIP calls in short pieces under g_capture_mu (one for the process: the check is not
  // per stream), the capture holds it from begin to end.
  size_t pl_bytes = 0;        // what the thread allocated (pl_rows, pl_ck, pl_ckh)
  int placement = 0;          // povar_layout_info::placement: 0 natural order, 1 placed in povar_create, 2 pending, 3 swapped in
  double placement_ms = 0;    // host wall time of the background build (valid from state 2 on)
  // camera-chunk layout of e0_ck (ck_layout.hpp): derived from the lane-per-landmark rows in use, so it is rebuilt
  // with them (pl_ck: built by the placement thread from the placed rows, swapped in together with them)
  struct CkBufs {                // (the buffers apart from the counts: CkDev::release frees them by assigning an empty CkBufs)
    DevBuf<double2> uv;
    DevBuf<int2> uvp;            // packed image points (CkLayout::uvp) instead of uv
    DevBuf<int> cpos;            // cold-view positions of the entries of chunks without an accumulator slot (CkLayout::cpos)
    DevBuf<uint32_t> li;
    DevBuf<int> src, bt_off, slot_rec;
    DevBuf<int2> lane_meta;
    DevBuf<int2> first_meta;     // e0_ck: the first requests of a launch (ck_first_tables; step 1 only)
    DevBuf<int4> first_hdr;
    DevBuf<int4> tile;
    DevBuf<int2> part_range;
    DevBuf<double> part, w;
    DevBuf<uint8_t> lcnt;        // e0_ck_det: ceil(log2(observations)) per landmark lane
    DevBuf<uint16_t> tick;       // e0_ck_det: ticket of every run total
  };
  struct CkDev : CkBufs {
    bool packed = false;         // uvp instead of uv
    bool cold_q = false;         // the chunks behind cpos leave q in the cold view instead of partial records of their own
    int nb = 0, slots = 0, n_part_rec = 0, max_acc = 0, max_tiles_bt = 0;
    int stride = 0;              // step 2: CKH_STRIDE or CKH_STRIDE_WIDE, whichever the layout was cut for (CkLayout::stride)
    int64_t n_capped_obs = 0;
    int64_t rows = 0, li_rows = 0, n_chunks = 0, n_cold_chunks = 0;
    double build_ms = 0;
    int64_t w_lin_id = -1;       // linearisation whose robust weights w holds
    bool ready = false;
    void release() {             // the counts stay: povar_get_layout_info reports them whatever `ready` says
      static_cast<CkBufs&>(*this) = CkBufs();
      packed = cold_q = ready = false;
    }
  } ck, pl_ck,       // step 1 (e0_ck): the layout in use / the one the placement thread built for the placed rows
    ckh, pl_ckh;     // step 2 (e0_ck_h): a second instance (64 bytes of LDS per landmark slot: more batches, other chunks)
  // resident power series (series_res, povar_kernels_res.hpp): the layout of res_layout.hpp on the device
  struct ResBufs {
    DevBuf<int> lane_cam, lane_seg, lslot, oslot, wave_h, lm_off, lm_id, cam_off, cam_id, cam_zi, own_off, own_cam, own_zi, oq_off, oq_rec;
    DevBuf<double2> uv;
    DevBuf<int2> own_q;
    DevBuf<uint4> part, zbuf, nrm;   // granule pairs (povar_kernels_res.hpp)
    DevBuf<unsigned> launch;         // launch counter: the high bits of the granule tags
  };
  struct ResDev : ResBufs {
    int W = 0, NW = 0, H = 0, R = 1, LS = 1, n_rec = 0, max_lm = 0, max_cam = 0, max_oq = 0, max_own = 0, max_chunks = 0, order = 0;
    size_t lds_bytes = 0;
    double build_ms = 0;
    bool ready = false;
    void release() {                 // (as CkDev::release)
      static_cast<ResBufs&>(*this) = ResBufs();
      ready = false;
    }
  } res,
    res_h;                       // step 2 (series_res_h): an instance of its own (no uv) where step 1's cut does not serve it
  // step 2 runs step 1's instance where that cut fits the LDS under the step-2 formula (res_layout.hpp: res_shared_fits) and
  // series_res_h has an instantiation for its shape: every array is shared, uv is simply not read
  bool res_h_shared = false;
  size_t res_h_lds = 0;          // dynamic LDS of series_res_h on the instance it runs
  double res_h_build_ms = 0;
  struct ResTune {               // res_autotune's answer for one step, timed on the system prepared for it
    bool tuned = false, choice = false;
    float us[2] = {0, 0};        // per term: per-term kernels (hipGraph), resident series
  } res_tune[2];                 // [0] step 1, [1] step 2 (the joint system)
  bool res_failed = false;
  bool res_check = false;        // a resident series is in flight whose give-up bit (flags[0] & 4) has not been looked at
  int res_last_m = 0;
  double res_last_tol[2] = {0, 0};
  bool det_check = false;        // deterministic: a series of e0_ck_det is in flight whose failure bit (flags[0] & 8) has not been looked at
  // fp32_terms: step 1's terms run e0_ck_f32 (povar_kernels_ck_f32.hpp) on the layout of variant 1
  int32_t fp32_last = 0;         // 1: the last step-1 power series ran its terms in fp32 (povar_layout_info.fp32_terms)
  DevBuf<float2> ck32_uv;        // [rows][64] fp32 image points of the chunk rows (only where the rows do not pack)
  DevBuf<float> ck32_lmrec;      // [lpl tiles][9][64] fp32 h~ and G of the landmark lanes (ck32_records, after every prepare)
  DevBuf<float> ck32_pimg;       // [n_cams][12] fp32 P3 and translation by rank (ck32_records)
  DevBuf<int2> ck_zero_range;    // [n_cams] empty runs: e0_ck leaves no per-observation cold view to the per-camera kernels
  bool ckh_tuned = false;
  float ckh_tune_us[2] = {0, 0}; // e0_lpl_h, e0_ck_h
  bool ck_tuned = false;
  bool ck_fresh[2] = {false, false};  // a timing of step 1 / step 2 finished on this rank since the ranks last agreed (tune_agree)
  float ck_tune_us[2] = {0, 0};  // what the timing saw: e0_lpl, e0_ck (microseconds per launch)
  DevBuf<double4> q4c;        // scatter scalars of the cold observations, in cold camera-major order
  DevBuf<int> lm_slot0, lm_cnt_dev;
  // stage timings (povar_timings): hipEvent pairs around the entry points, summed on demand
  bool timings_on = false;
  std::vector<hipEvent_t> tev;
  std::vector<int> tev_kind;
  size_t tev_used = 0;
  povar_timings_info tsum{};
  DevBuf<int> cam, lm, meta, hot_cams, cam_hot, cc_slot, cc_lm, cc_item_off, cc_cam_item_off, long_lm, long_first, long_cnt, cm_slot, cm_lm, item_off, item_cam,
      cam_item_off, flags;
  // state
  DevBuf<double4> cams4, cams_lin4, cams_bak4, lms4, lms_lin4, lms_bak4, jl_scale4, rres, q4;
  DevBuf<double> hll_inv, sw, sigma, diag2, G, binv, b, tmp, accum, z, y, inc, item_part,
      item_partG, norm_part, norms, part, scal, stage, cm_h, lmrec, ncw, cc_h, cc_part, hot_part, hot_rec, zimg;

  // explicit-SC solvers (PCG / CHOLESKY / RIPCG), allocated on first use
  DevBuf<double> sc_dm_part, sc_dm, sc_bmat, sc_minv, sc_x, sc_r, sc_p, sc_q, sc_zv, sc_part, sc_s;
  ScP sc{};
  DevBuf<double> sc_dense, sc_xpad;      // CHOLESKY / RICHOLESKY: augmented S (povar_kernels_chol.hpp) and the padded solution,
                                         // grown to the larger of the two systems a context solves (run_cholesky)
  DevBuf<int> sc_lm_slot0, sc_lm_cnt, sc_info;
  // assembly of the dense matrix (povar_set_sc_assembly / povar_sc_assembly): the caller's choice (-1: the library's -- ordered on
  // a deterministic context, atomics otherwise; 1: atomics, sc_dense_diag + sc_dense_offdiag[_h]; 2: ordered, sc_dense_ordered)
  // and what the last chol_factor ran (0: none yet)
  int sc_assembly = -1, sc_assembly_last = 0;
  int sc_factor_dim = 0;                 // POVAR_BUF_SC_FACTOR: the system whose R, y (sc_dense) and x (sc_xpad) are in place:
  int sc_factor_n = 0;                   // 12 (step 1) or 11 (step 2) and dim * n_cams; 0: none (chol_factor, the covariance calls)
  // the covariance calls (povar_cov.hip): their buffers, grown on demand and kept, and what POVAR_BUF_COV_* may hand out
  struct CovState {
    // camera calls: the gauge basis Q, (max A_kk, min R_kk^2), the N x 64 scratch panel of the triangular inverse, the
    // [n_cams][144] blocks
    DevBuf<double> q, stat, panel, blocks;
    DevBuf<double> lm;                   // povar_landmark_covariance_*: the requested landmark blocks and their ids
    DevBuf<int> ids;
    DevBuf<double> obs;                  // povar_observation_covariance_* / _hat_*: the rows (4, or 14 / 5 per observation) and the first
    DevBuf<int> row0;                    // row of every requested landmark (Sigma_l without the gauge part goes to lm)
    DevBuf<double> pair_out;             // povar_covariance_blocks_*: the blocks in request order, the three index lists (a, b,
    DevBuf<int> pair_items;              // transposed, -) one after the other and where every block starts
    DevBuf<long long> pair_off;
    // inspection of the covariance path (povar_set_cov_inspect, POVAR_BUF_COV_*).  kind: what the last call that wrote the dense
    // matrix left there: 0 nothing to hand out (chol_factor, a failure), 1 a camera call's W, 2 a landmark call's W, C and
    // panel; n as sc_factor_n (dim * n_cams of that call); nq: columns of the gauge basis of that call (0: damped); kept: that
    // call copied its R into r (N x N, row-major, allocated only with the switch on)
    int inspect = 0;
    int kind = 0, n = 0, nq = 0;
    bool kept = false;
    DevBuf<double> r;
    // the dense matrix, Q or the panel are about to be rewritten: nothing to hand out until a call is done
    void invalidate() {
      kind = n = nq = 0;
      kept = false;
    }
    // a covariance call has returned 0 (kind 1: W alone is in place, 2: W, C and the panel)
    void done(int kind_, int n_, int nq_) {
      kind = kind_;
      n = n_;
      nq = nq_;
    }
  } cov;

  // fixed cameras (povar_set_fixed_cameras): fixed_next is the caller's set, fixed_mask its device copy as of the last
  // preparation (lm_prepare uploads it when fixed_dirty: a system prepared earlier is what it was), n_fixed the cameras
  // that copy holds.  An explicit argument of cam_build_binv[_h], cam_build_sc, sc_fix_cameras, cov_diag_scan and
  // cov_fix_cameras: not part of Dp, whose term kernels do not read it.
  DevBuf<uint8_t> fixed_mask;
  std::vector<uint8_t> fixed_next;
  bool fixed_dirty = false;
  int n_fixed = 0;

  // layout of the dense matrix (povar_set_dense_compaction; cov_plan.hpp: cam_row_map): compaction_next is the caller's mode,
  // compaction / cam_row_dim / cam_row_n what the device map cam_row holds -- lm_prepare rebuilds and uploads it after the fixed
  // set, when the set, the mode or the step's dim changed: every dense call of a step reads the step's own map.  An explicit
  // argument of the assembly kernels, the scatter of the solution and the readers of C.  layout_*: the map of the matrix the
  // last dense call built (povar_dense_layout; layout_n = 0 and no rows: none yet).
  DevBuf<int> cam_row;
  std::vector<int32_t> cam_row_host, layout_rows;
  int compaction_next = 0, compaction = 0, cam_row_dim = 0, cam_row_n = 0, layout_n = 0;
  bool cam_row_dirty = true;

  Dp d{};
  bool new_linearization_point = false;  // linearizor_power_varproj.cpp:75, 192, 240
  bool linearized = false;
  bool tiles_valid = false;
  bool joint = false;        // system prepared last: step 2 (11-dim tangent) or step 1 (12-dim)
  bool linearized_h = false;
  double alpha_lin = 0;

  // multi-GPU
  // peer-to-peer term exchange (povar_p2p_export / povar_p2p_attach)
  double* xbuf = nullptr;              // this rank's exchange buffer [2][world][n_cams][16]
  size_t xbuf_count = 0;
  std::vector<double*> peer_host;      // opened peer mappings (index = rank; own entry = xbuf)
  DevBuf<double*> peer_dev;
  DevBuf<unsigned long long> p2p_epoch;
  bool p2p = false;
  ncclComm_t comm = nullptr;
  povar_allreduce_fn host_fn = nullptr;  // caller-supplied exchange (povar_comm_init_host)
  void* host_user = nullptr;
  std::vector<double> host_stage;
  int world = 1, rank = 0;

  // hipGraph of the m-term series loop (launch-bound on small problems and at 8 GPUs)
  double create_ms = 0;  // host wall time of povar_create (layout construction + uploads)
  DevBuf<double4> v2_lmx, v2_lml, v2_lsc;  // lane-ordered mirrors of lms4 / lms_lin4 / jl_scale4 (V2::lmx, lml, lsc)
  // Who is current.  Three clocks, and beside each the copies that are rebuilt lazily with the tick they hold:
  // the state: lms_ver / cams_ver count the writes to lms4 / cams4 (the cost memo below answers for an unchanged pair);
  //   lmx_ver: the landmarks the lane-ordered mirror v2_lmx holds
  uint64_t lms_ver = 1, cams_ver = 1, lmx_ver = 0;
  // the linearisation: lin_id counts them.  The lane-per-landmark kernels leave the mirrors v2_lml / v2_lsc (lml_lin_id,
  //   lsc_lin_id), the lane-per-observation ones the landmark-order masters lms_lin4 / jl_scale4 (lmslin_lin_id,
  //   jls_lin_id), the per-slot sqrt(w) / weighted residual arrays (aux_lin_id) and the camera-major landmark copies
  //   cm_h, cc_h, c2_h (views_lin_id); whichever family did not run gets its copies when it asks (povar_lm.hip)
  int64_t lin_id = 0, lml_lin_id = -1, lsc_lin_id = -1, lmslin_lin_id = -1, jls_lin_id = -1, aux_lin_id = -1, views_lin_id = -1;
  // the preparation: prep_id counts them, prep_lin_id is the linearisation the last one was taken on.  prepare_lpl[_h]
  //   writes only the lane-per-landmark records; hll_inv / lmrec of the legacy kernels (aux_prep_id) follow lazily
  int64_t prep_id = 0, aux_prep_id = 0, prep_lin_id = -1;
  // compute_error_* of an unchanged state: the LM loop asks again at the top of every iteration
  // (bal_bundle_adjustment.cpp:302-310 / 600-605)
  struct ErrMemo {
    bool valid = false;
    uint64_t lms_ver = 0, cams_ver = 0;
    double alpha = 0;
    int kind = 0, mode = 0;
    povar_residual_info ri{};
  } err_memo;
  bool has_empty_lm = false;  // a landmark without observations has no lane: lms_lin4 is then copied eagerly
  bool flag0_clean = false;  // flags[0] is known to be zero on the device (read back as zero, no writer launched since)
  hipGraphExec_t series_graph = nullptr;
  Dp series_graph_d{};
  int series_graph_key[6] = {0, 0, 0, 0, 0, 0};
  double series_graph_tol[2] = {0, 0};

  // profiling
  bool profile = false;
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_kind;  // 0 e0, 1 binv, 2 comm  (interval between ev[i], ev[i+1])
  size_t ev_used = 0;
};

// A host vector to a device buffer of its size (one element for an empty one), counted into *bytes (default: the context's).
// locked: the caller is the row-placement thread -- its HIP calls go in short pieces under g_capture_mu, and a cancelled
// placement (povar_ctx::placer_cancel) stops copying (nobody will read the buffer).
template <class T>
int upload(DevBuf<T>& buf, const std::vector<T>& v, povar_ctx* c, size_t* bytes = nullptr, bool locked = false) {
  if (!bytes) bytes = &c->bytes;
  {
    const auto lk = capture_lock(locked);
    HIP_TRY(buf.alloc(std::max<size_t>(v.size(), 1), bytes));
  }
  if (!locked) {
    if (!v.empty()) HIP_TRY(hipMemcpy(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
  const size_t piece = ((size_t)8 << 20) / sizeof(T);  // 8 MB per copy: a capture waits a millisecond at most
  for (size_t at = 0; at < v.size() && !c->placer_cancel.load(); at += piece) {
    const auto lk = capture_lock(true);
    HIP_TRY(hipMemcpy(buf.p + at, v.data() + at, std::min(piece, v.size() - at) * sizeof(T), hipMemcpyHostToDevice));
  }
  return 0;
}

// "upload these vectors, stop at the first failure": up(buf, v)(buf2, v2)...; then look at rc (what upload returned)
struct Uploader {
  povar_ctx* c;
  size_t* bytes = nullptr;
  bool locked = false;
  int rc = 0;
  template <class T>
  Uploader& operator()(DevBuf<T>& buf, const std::vector<T>& v) { if (!rc) rc = upload(buf, v, c, bytes, locked); return *this; }
};

inline int grid_for(int64_t n, int block) { return (int)((n + block - 1) / block); }


// ------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------
template <class Op>
void launch_lm(povar_ctx* c, const Op& op, const Dp& d) {
  hipLaunchKernelGGL((lm_regular<Op>), dim3(c->n_reg_blocks), dim3(LM_BLOCK), 0, c->stream, d, op, c->part.p);
  if (c->n_long > 0) hipLaunchKernelGGL((lm_long<Op>), dim3(c->n_long), dim3(LM_BLOCK), 0, c->stream, d, op, c->part.p);
}
template <class Op>
void launch_lm(povar_ctx* c, const Op& op) { launch_lm(c, op, c->d); }

template <int N>
void launch_reduce(povar_ctx* c, double* out) {
  hipLaunchKernelGGL((reduce_partials<N>), dim3(1), dim3(1024), 0, c->stream, c->part.p,
                     c->n_reg_blocks + c->n_long, out);
}

inline bool sharded(const povar_ctx* c) { return c->comm != nullptr || c->host_fn != nullptr; }

// the resident-series instance a step's series runs on
inline const povar_ctx::ResDev& res_dev(const povar_ctx* c, bool joint) { return joint && !c->res_h_shared ? c->res_h : c->res; }
inline bool res_ready(const povar_ctx* c, bool joint) { return joint ? (c->res_h_shared ? c->res.ready : c->res_h.ready) : c->res.ready; }

// the lane-per-landmark kernels run the context (use_lpl in the LDS-accumulating mode): e0_lpl[_h] / e0_ck* for the terms,
// lpl_pass[_h] for linearisation and cost, and ldsacc_dp's cold view and partial records are theirs
inline bool lpl_mode(const povar_ctx* c) { return c->use_lpl && c->opt.e0_mode == POVAR_E0_IMPLICIT_LDSACC; }

// ---- one application of E0 in a power-series term: which kernels run it (term_plan), and the one launcher (launch_e0)
// who applies E0: the term loop of a series (with the norms of its check or without), povar_right_mul_e0_pose (the fp32
// terms cover it), the explicit-SC solvers (e0_dense: always fp64), the timing of the two E0 kernels (ck_autotune)
enum class TermUse { series, series_norms, right_mul, dense, timing };
enum class E0K {
  lm_cached,      // e0_lm_cached<false>: lane per observation (POVAR_E0_IMPLICIT)
  lm_cached_acc,  // e0_lm_cached<true>: ... accumulating in LDS (POVAR_E0_IMPLICIT_LDSACC without lane per landmark)
  lm_tiles,       // lm_regular<OpE0Tiles> (POVAR_E0_TILES)
  tiles_cached,   // e0_tiles_cached (POVAR_E0_TILES_LDSACC)
  lpl,            // e0_lpl: lane per landmark, cameras in LDS
  ck,             // e0_ck<variant>: lane per camera chunk, landmarks in LDS
  ck_det,         // e0_ck_det (POVAR_DETERMINISTIC)
  ck_f32,         // e0_ck_f32 (POVAR_FLAG_FP32_TERMS)
  lm_h,           // step 2: lm_regular<OpE0H> (outside the LDS-accumulating mode)
  lm_cached_h,    // e0_lm_cached_h
  lpl_h,          // e0_lpl_h
  ck_h,           // e0_ck_h (stride CKH_STRIDE or CKH_STRIDE_WIDE)
  ck_h_det,       // e0_ck_h_det
};
enum class CamStep {  // the per-camera kernel behind the E0 kernel
  scatter,      // cm_scatter: item sums (cam_binv_axpy mode 1)
  scatter_sum,  // cm_scatter + cam_sum_items: dense y (sharded)
  sum,          // cam_cold_sum[_h]: dense y
  fused,        // cam_cold_sum_binv[_h]: B^-1, AXPY and z too
};
enum class Exch { none, allreduce, p2p };  // y across the ranks: ... or the peer-to-peer push of cam_cold_sum
struct TermPlan {
  int step = 1;
  TermUse use = TermUse::series;
  E0K e0 = E0K::lm_cached;
  int variant = 0;          // e0_ck / e0_ck_f32: the instantiation whose layout runs (POVAR_CK_VARIANTS); e0_ck_h: 1
  bool long_after = false;  // lm_long of the E0 kernel's operator follows (the long landmarks)
  CamStep cam = CamStep::scatter;
  Exch exch = Exch::none;
  bool ck() const { return e0 == E0K::ck || e0 == E0K::ck_det || e0 == E0K::ck_f32 || e0 == E0K::ck_h || e0 == E0K::ck_h_det; }
  // what the caller must look at once the series is done: the tickets of e0_ck[_h]_det (flags[0] & 8), the waits of the
  // peer-to-peer exchange (flags[0] & 2)
  bool det_check() const { return e0 == E0K::ck_det || e0 == E0K::ck_h_det; }
  bool p2p_check() const { return exch == Exch::p2p; }
  // what cam_binv_axpy does next: 1 item sums, 2 dense y, 4 nothing (fused), 5 wait for the world's slabs
  int binv_mode() const { return cam == CamStep::fused ? 4 : exch == Exch::p2p ? 5 : cam == CamStep::scatter ? 1 : 2; }
};

// the per-term exchange runs through the peer-to-peer kernels: no library / host call inside the term loop

// povar_timings: a pair of events on the context's stream around an entry point (kinds: 0 linearize, 1 prepare,
// 2 solve = the power series / PCG / CHOLESKY, 3 apply = camera update + back-substitution, 4 other)
struct TimeScope {
  povar_ctx* c;
  bool on;
  TimeScope(povar_ctx* c_, int kind) : c(c_), on(c_->timings_on) {
    if (!on) return;
    if (c->tev_used + 2 > c->tev.size()) {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        c->tev.push_back(e);
        c->tev_kind.push_back(-1);
      }
    }
    c->tev_kind[c->tev_used] = kind;
    (void)hipEventRecord(c->tev[c->tev_used], c->stream);
  }
  ~TimeScope() {
    if (!on) return;
    (void)hipEventRecord(c->tev[c->tev_used + 1], c->stream);
    c->tev_used += 2;
  }
};

// hipEvents that are destroyed on every return path (the HIP_TRY early returns of the timing functions included)
template <int N>
struct EventSet {
  hipEvent_t e[N] = {};
  hipError_t create() {
    for (auto& x : e) {
      hipError_t r = hipEventCreate(&x);
      if (r != hipSuccess) return r;
    }
    return hipSuccess;
  }
  hipEvent_t& operator[](int i) { return e[i]; }
  ~EventSet() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
};


// ---- functions one translation unit defines and another calls
TermPlan term_plan(const povar_ctx* c, int step, TermUse use, int variant = -1);  // povar_series.hip
int launch_e0(povar_ctx* c, const TermPlan& p);  // povar_series.hip
hipError_t term_set_lds_all();  // povar_series.hip
void launch_ck32_records(povar_ctx* c);  // povar_series.hip
bool res_variant_exists(int nw, int h, int rr, int ls, bool joint = false);  // povar_series.hip
hipError_t res_set_lds_all();  // povar_series.hip
bool res_active(const povar_ctx* c, bool joint);  // povar_series.hip
void prof_mark(povar_ctx* c, int kind);  // povar_series.hip
Dp ldsacc_dp(povar_ctx* c, bool long_in_kernel = false);  // povar_series.hip
int ck_autotune(povar_ctx* c, int step);  // povar_series.hip
int tune_agree(povar_ctx* c, int step);  // povar_series.hip
extern "C" int res_verify(povar_ctx* c);  // povar_series.hip
int swap_in_placed_rows(povar_ctx* c, bool wait);  // povar_create.hip
int check_ctx(povar_ctx* c);  // povar_create.hip
int read_scal_flags(povar_ctx* c, double* h, int n, int (&f)[4]);  // povar_create.hip
int read_flags(povar_ctx* c, int (&f)[4]);  // povar_create.hip
int read_scal(povar_ctx* c, double* h, int n);  // povar_create.hip
int write_cam_vector(povar_ctx* c, double* dst, const double* in, size_t n);  // povar_create.hip
int read_cam_vector(povar_ctx* c, double* out, const double* src, size_t n);  // povar_create.hip
hipError_t lm_set_lds_all();  // povar_lm.hip
void build_views(povar_ctx* c);  // povar_lm.hip
void lanes_from(povar_ctx* c, const double4* src, double4* dst);  // povar_lm.hip
void ensure_lmx(povar_ctx* c);  // povar_lm.hip
void ensure_lin_mirrors(povar_ctx* c);  // povar_lm.hip
void ensure_legacy(povar_ctx* c);  // povar_lm.hip
int clear_flag0(povar_ctx* c);  // povar_lm.hip
bool err_memo_hit(const povar_ctx* c, int kind, double alpha, povar_residual_info* out);  // povar_lm.hip
void err_memo_store(povar_ctx* c, int kind, double alpha, const povar_residual_info& ri);  // povar_lm.hip
int combine_flag(povar_ctx* c, int* flag);  // povar_lm.hip
int ensure_tiles(povar_ctx* c);  // povar_lm.hip
extern "C" void set_alpha(povar_ctx* c, double alpha);  // povar_lm.hip
int allreduce(povar_ctx* c, double* buf, size_t n);  // povar_comm.hip
void p2p_dp(povar_ctx* c, Dp& dt);  // povar_comm.hip
int ensure_sc(povar_ctx* c);  // povar_sc.hip
int e0_dense(povar_ctx* c);  // povar_sc.hip
int run_cholesky(povar_ctx* c, int dim, int32_t* num_iterations, int32_t* termination);  // povar_sc.hip (dim: 12 step 1, 11 step 2)
int prepare_sc(povar_ctx* c, int dim, double lambda);  // povar_sc.hip
int chol_factor(povar_ctx* c, int dim, const double* Q, int nq, double* stat);  // povar_sc.hip
int no_memory(int dim, int rows, const char* what, size_t bytes);  // povar_sc.hip

// The run-time block dimension (12: step 1, 11: step 2) to the step type of the dense kernels: fn(ScdPose()) or fn(ScdJoint()),
// so every launch templated on the step is written once
template <class F>
auto with_step(int dim, F fn) {
  return dim == 12 ? fn(ScdPose()) : fn(ScdJoint());
}

// A device buffer the context keeps (counted in povar_device_bytes), grown to `count` elements once the stream has drained.
// `headroom` > 0: the device must have that many bytes free beside the new buffer, else hipErrorOutOfMemory without trying.
// On an error the buffer is empty.
template <typename T>
hipError_t grow_buffer(povar_ctx* c, DevBuf<T>& buf, size_t count, size_t headroom = 0) {
  if (buf.p && buf.n >= count) return hipSuccess;
  if (buf.p) {
    if (hipError_t e = hipStreamSynchronize(c->stream)) return e;
    c->bytes -= buf.n * sizeof(T);
    buf.release();
  }
  size_t free_b = 0, total_b = 0;
  if (headroom > 0) {
    if (hipError_t e = hipMemGetInfo(&free_b, &total_b)) return e;
    if (count * sizeof(T) + headroom > free_b) return hipErrorOutOfMemory;
  }
  const hipError_t e = buf.alloc(count, &c->bytes);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}

// Geometry of the augmented dense matrix of CHOLESKY / RICHOLESKY and the covariance calls (povar_kernels_chol.hpp): n = dim *
// n_cams rows (n_cams: the cameras in the matrix -- all of them, or the free ones: povar_ctx::cam_row_n / dim), N = n rounded up
// to the 64-row panel, row stride ld, and the doubles of the allocation (slack rows / columns for the 128 x 128 update tiles)
struct DenseDims {
  int n, N;
  int64_t ld;
  size_t count;
};
inline DenseDims dense_dims(int dim, int n_cams) {
  const int n = dim * n_cams;
  const int N = (n + CH_NB - 1) / CH_NB * CH_NB;
  const int64_t ld = (int64_t)N + CH_T;
  return {n, N, ld, (size_t)(N + CH_NB) * (size_t)ld};
}
