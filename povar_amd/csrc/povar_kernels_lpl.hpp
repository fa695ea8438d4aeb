// povar_kernels_lpl.hpp -- the lane-per-landmark kernels of both steps: e0_lpl, prepare_lpl, backsub_lpl, lpl_pass and their
// step-2 twins *_h.  Lane = landmark; the cameras a workgroup keeps live in LDS, colder ones come from L2 (lpl_layout.hpp).
//   pieces      LplTiles      the workgroup's tile range, its on-demand counter and the tile table
//               LplStream2    the row stream of the two-pass kernels (e0 / prepare / backsub): rows requested three ahead
//               LplStream1    the same for the single forward walk of lpl_pass[_h]
//               lpl_read12 / lpl_read_cam   twelve consecutive doubles of a camera record
//               lpl_wg, lpl_stage, lpl_scatter, lpl_cold_at, lpl_flush*, lpl_acc_sum   what every kernel starts and ends with
//   kernels     lpl_pass[_h], prepare_lpl[_h], e0_lpl[_h]: one per step, on the pieces
//   step types  LplPose, LplJoint: what differs between step 1 and step 2 in back substitution -- the camera record, what a lane
//               carries of its landmark, the arithmetic of an observation
//   body        backsub_lpl_body<Step, ROBUST>, behind the kernels backsub_lpl[_h]
// Pieces, not a walker: every kernel keeps its own `while (c_t < t_end)` loop, its row loops and its LDS-or-global read form.
// Included from povar_ctx.hpp behind povar_kernels_joint.hpp (it needs the observation helpers
// of both steps), never on its own.  Every member function of the pieces is __forceinline__ and every member a value: the cursors
// are wave-uniform and have to stay in SGPRs, the row queue in VGPRs without a copy through memory.
#pragma once

namespace povar {

// The row stream of one wavefront is a static address sequence: tile t forward rows, tile t backward rows (the same
// rows again, now L2 hits), the next tile it takes ...  A scalar prefetch cursor runs LPL_DEPTH rows ahead of the consumer
// along that sequence, across the pass and tile boundaries, so the wavefront never waits for a load it has just
// issued (s_waitcnt vmcnt retires in issue order: the e0_lm_cached loop exposed two HBM latencies per bin that way).
constexpr int LPL_DEPTH = 3;

struct LplRow {
  double2 uv;
  int cw;
  double w;
};
struct LplCursor {  // wave-uniform (SGPRs)
  int t, pass, j, row0, k;
};

// The workgroup's tiles [t_begin, t_end) are sorted longest first; its wavefronts take them on demand (one LDS counter), so a
// wavefront's last tile is a short one.  The workgroups carry equal observation totals (lpl_layout.hpp).  t_end = no tile.
struct LplTiles {
  // tile table through the scalar cache (constant address space + wave-uniform index => s_load_dwordx4): a vector
  // load here would put a vmcnt(0) drain inside the row pipeline
  typedef const int __attribute__((address_space(4))) * cint_p;
  int t_begin, t_end;
  cint_p tile;
  int* ctr;  // LDS; the kernel sets it (to the number of tiles it deals statically) before the barrier in front of the first grab
  int lane;
  __device__ __forceinline__ LplTiles(const V2& v, int* ctr_, int lane_)
      : t_begin(__builtin_amdgcn_readfirstlane(v.wg_tile_off[blockIdx.x])),
        t_end(__builtin_amdgcn_readfirstlane(v.wg_tile_off[blockIdx.x + 1])),
        tile((cint_p)(uintptr_t)v.tile), ctr(ctr_), lane(lane_) {}
  // the workgroup's n-th tile (n wave-uniform)
  __device__ __forceinline__ int nth(int n) const {
    const long long t = (long long)t_begin + n;
    return t < t_end ? (int)t : t_end;
  }
  __device__ __forceinline__ int grab() const {
    int n = 0;
    if (lane == 0) n = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return nth(__builtin_amdgcn_readfirstlane(n));
  }
  // (lpl_layout.hpp) first row, rows, rows with an LDS-resident camera in every lane, flags | cold-q base
  __device__ __forceinline__ void info(int t, int& row0, int& k, int& nh, int& fl) const {
    row0 = tile[4 * t];
    k = tile[4 * t + 1];
    nh = tile[4 * t + 2];
    fl = tile[4 * t + 3];
  }
};

__device__ __forceinline__ void lpl_no_row(LplRow& r) {
  r.cw = -1;
  r.w = 1.0;
  r.uv = make_double2(0, 0);
}

// Two passes over every tile: k rows forward, the same k rows backward.  The queue holds the LPL_DEPTH = 3 rows behind
// the cursor; next() hands out the oldest and requests one more.
// INVARIANT (the one place it is stated): a tile has k >= 2 rows (POVAR_LPL_K0 >= 2, lpl_layout.hpp), that is at least
// 4 row steps here, and the cursor is at most 3 steps ahead of the consumer.  So while the consumer is inside tile c the
// cursor is inside c or the tile after it, never further: ONE tile ahead (nx_t) is enough.  And when the consumer enters c
// the cursor has not left c yet (it does with the request of c's last step, the fourth at the earliest): ahead() is due
// before the first next() of a tile, not sooner, and start() -- three requests -- may run with "no tile" ahead.
template <bool ROBUST>
struct LplStream2 {
  LplCursor pc;
  int nx_t;  // the tile after the one being consumed
  LplRow n1, n2, n3;

  // request the row under the prefetch cursor and advance it
  __device__ __forceinline__ void issue(const LplTiles& T, const V2& v, LplRow& r) {
    if (pc.t < T.t_end) {
      // the backward pass walks the rows in reverse: the rows read last are the ones most likely still in L2
      const size_t i = ((size_t)pc.row0 + (pc.pass ? pc.k - 1 - pc.j : pc.j)) * WAVE + T.lane;
      r.uv = v.uv[i];
      r.cw = v.cw[i];
      if (ROBUST) r.w = v.w[i];
      if (++pc.j == pc.k) {
        pc.j = 0;
        if (++pc.pass == 2) {
          pc.pass = 0;
          pc.t = nx_t;
          if (pc.t < T.t_end) {
            int nh_, fl_;
            T.info(pc.t, pc.row0, pc.k, nh_, fl_);
          }
        }
      }
    }
  }
  // start on tile t (row0, k: its T.info, anything when t is no tile) with tile nx after it; requests the first three rows
  __device__ __forceinline__ void start(const LplTiles& T, const V2& v, int t, int row0, int k, int nx) {
    pc.t = t;
    pc.pass = 0;
    pc.j = 0;
    pc.row0 = row0;
    pc.k = k;
    nx_t = nx;
    lpl_no_row(n1);
    lpl_no_row(n2);
    lpl_no_row(n3);
    issue(T, v, n1);
    issue(T, v, n2);
    issue(T, v, n3);
  }
  // the consumer has entered a tile: t is the one after it
  __device__ __forceinline__ void ahead(int t) { nx_t = t; }
  // the consumer's next row: tile c forward rows 0 .. k-1, then ITS rows k-1 .. 0, then tile nx_t
  __device__ __forceinline__ LplRow next(const LplTiles& T, const V2& v) {
    const LplRow cur = n1;
    n1 = n2;
    n2 = n3;
    issue(T, v, n3);
    return cur;
  }
};

// One forward pass over every tile (lpl_pass[_h]; V2::w is not read).
// INVARIANT: a tile has at least 2 row steps here and the cursor is up to 3 ahead of the consumer, so from tile c it can
// reach the tile after the next one: TWO tiles are taken ahead (q1, q2), and advance() takes a third before c is left.
struct LplStream1 {
  int q1, q2;  // the tiles after the one being consumed
  int pc_t, pc_ahead, pc_j, pc_row0, pc_k;  // the cursor; pc_ahead: 0 = the consumer's tile, 1 = q1, 2 = q2
  LplRow n1, n2, n3;

  __device__ __forceinline__ void seek(const LplTiles& T) {
    if (pc_t < T.t_end) {
      pc_row0 = T.tile[4 * pc_t];
      pc_k = T.tile[4 * pc_t + 1];
    }
  }
  __device__ __forceinline__ void issue(const LplTiles& T, const V2& v, LplRow& r) {
    if (pc_t < T.t_end) {
      const size_t i = ((size_t)pc_row0 + pc_j) * WAVE + T.lane;
      r.uv = v.uv[i];
      r.cw = v.cw[i];
      if (++pc_j == pc_k) {
        pc_j = 0;
        ++pc_ahead;
        pc_t = pc_ahead == 1 ? q1 : pc_ahead == 2 ? q2 : T.t_end;
        seek(T);
      }
    }
  }
  // start on tile t (just grabbed): takes the two tiles after it and requests the first three rows
  __device__ __forceinline__ void start(const LplTiles& T, const V2& v, int t) {
    q1 = t < T.t_end ? T.grab() : T.t_end;
    q2 = q1 < T.t_end ? T.grab() : T.t_end;
    pc_t = t;
    pc_ahead = 0;
    pc_j = 0;
    pc_row0 = 0;
    pc_k = 1;
    seek(T);
    lpl_no_row(n1);
    lpl_no_row(n2);
    lpl_no_row(n3);
    issue(T, v, n1);
    issue(T, v, n2);
    issue(T, v, n3);
  }
  __device__ __forceinline__ LplRow next(const LplTiles& T, const V2& v) {
    const LplRow cur = n1;
    n1 = n2;
    n2 = n3;
    issue(T, v, n3);
    return cur;
  }
  // the consumer has finished its tile: the next one (t_end: none), one more taken ahead
  __device__ __forceinline__ int advance(const LplTiles& T) {
    const int t = q1;
    q1 = q2;
    q2 = q1 < T.t_end ? T.grab() : T.t_end;
    --pc_ahead;
    return t;
  }
};

// Flush of the accumulators acc[12][n_slots] (lpl_acc_slot): entries 2m, 2m + 1 of camera slot r, the four replicas of a
// hub slot summed.  The caller stores the pair (16 bytes) into the slot's partial record, whose index it has loaded its own way.
__device__ __forceinline__ double2 lpl_acc_sum(const double* acc, int n_slots, int hubs, int r, int m) {
  const double* a0 = acc + 2 * m * n_slots;
  const double* a1 = a0 + n_slots;
  double2 s;
  if (r < hubs) {
    s.x = (a0[4 * r] + a0[4 * r + 1]) + (a0[4 * r + 2] + a0[4 * r + 3]);
    s.y = (a1[4 * r] + a1[4 * r + 1]) + (a1[4 * r + 2] + a1[4 * r + 3]);
  } else {
    s.x = a0[r + 3 * hubs];
    s.y = a1[r + 3 * hubs];
  }
  return s;
}

// 12 consecutive doubles of a camera record as six 16-byte reads.  hp is an LDS pointer or a global pointer, never a select
// of the two: a generic pointer makes every read a flat_load (texture path into the LDS, both wait counters).  The kernels
// that do pass a select (lpl_pass[_h], backsub_lpl_h) say why at the call.
__device__ __forceinline__ void lpl_read12(const double2* hp, double4 (&o)[3]) {
  const double2 b0 = hp[0], b1 = hp[1], b2 = hp[2], b3 = hp[3], b4 = hp[4], b5 = hp[5];
  o[0] = make_double4(b0.x, b0.y, b1.x, b1.y);
  o[1] = make_double4(b2.x, b2.y, b3.x, b3.y);
  o[2] = make_double4(b4.x, b4.y, b5.x, b5.y);
}
__device__ __forceinline__ void lpl_read_cam(const double2* hp, Cam& P) {  // P row-major
  const double2 b0 = hp[0], b1 = hp[1], b2 = hp[2], b3 = hp[3], b4 = hp[4], b5 = hp[5];
  P.r0 = make_double4(b0.x, b0.y, b1.x, b1.y);
  P.r1 = make_double4(b2.x, b2.y, b3.x, b3.y);
  P.r2 = make_double4(b4.x, b4.y, b5.x, b5.y);
}

// ------------------------------------------------------------------------------------------
// What every kernel of the family starts and ends with.
// ------------------------------------------------------------------------------------------
// The workgroup's camera slots -- the records of the cameras it keeps in LDS (lpl_layout.hpp) -- and its dynamic LDS:
// [n_hot][stride] records, then (ACC) the accumulators acc[12][n_slots] of Jp^T s, zeroed here, then the tile counter, set to
// the number of tiles the kernel deals without it.  The barrier behind the staging covers all three.  `hot` is the kernel's
// `extern __shared__` array itself, named in every body: the records are read through it, not through a pointer kept here.
struct LplWg {
  int cam0, n_hot, hubs, n_slots;
  double* acc;
  int* ctr;
};
template <bool ACC>
__device__ __forceinline__ LplWg lpl_wg(const V2& v, double2* hot, int stride, int dealt) {
  LplWg g;
  g.cam0 = v.wg_cam_off[blockIdx.x];
  g.n_hot = v.wg_cam_off[blockIdx.x + 1] - g.cam0;
  g.hubs = v.hubs;
  g.n_slots = g.n_hot + 3 * g.hubs;
  g.acc = reinterpret_cast<double*>(hot + g.n_hot * stride);
  g.ctr = reinterpret_cast<int*>(ACC ? g.acc + g.n_slots * 12 : g.acc);
  if (ACC)
    for (int i = threadIdx.x; i < g.n_slots * 12; i += E0C_BLOCK) g.acc[i] = 0;
  if (threadIdx.x == 0) *g.ctr = dealt;
  return g;
}
// the record of the camera with popularity rank `rank` in the rank-ordered image (z, then P row-major; cw < -1: rank -2 - cw)
__device__ __forceinline__ const double2* lpl_img(const Dp& d, int rank) {
  return reinterpret_cast<const double2*>(d.hot_rec) + (size_t)rank * (HOT_REC_STRIDE / 2);
}
// plain staging: piece j of slot r's record is src(rank of the slot's camera, j)
template <int REC, int STRIDE, class Src>
__device__ __forceinline__ void lpl_stage(const LplWg g, const V2& v, double2* hot, Src src) {
  for (int i = threadIdx.x; i < g.n_hot * REC; i += E0C_BLOCK) {
    const int r = i / REC, j = i - r * REC;
    hot[r * STRIDE + j] = src(v.wg_cams[g.cam0 + r], j);
  }
}
// Jp^T s of an observation of an LDS-resident camera: X (x) q into acc[m][slot] (consecutive slots on consecutive banks);
// X is the landmark, (hx, hy, hz, 1) in step 1
__device__ __forceinline__ void lpl_scatter(const LplWg g, int cw, const double4& X, const double4& q) {
  double* a = g.acc + lpl_acc_slot(cw, g.hubs);
  const double val[12] = {X.x * q.x, X.y * q.x, X.z * q.x, X.w * q.x, X.x * q.y, X.y * q.y,
                          X.z * q.y, X.w * q.y, X.x * q.z, X.y * q.z, X.z * q.z, X.w * q.z};
#pragma unroll
  for (int m = 0; m < 12; ++m) __hip_atomic_fetch_add(a + m * g.n_slots, val[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// where a cold observation's q goes in Dp::q4c: row-major next to the other lanes' (graphs with many cold observations: the
// per-camera kernel gathers, Dp::q_rows) or straight to its place in the camera-major cold view (few: one 32-byte store per lane)
__device__ __forceinline__ int lpl_cold_at(const Dp& d, int fl, int nh, int row0, int j, int lane) {
  return d.q_rows ? lpl_cold_q(fl, nh, j, lane) : d.v2.cpos[((size_t)row0 + j) * WAVE + lane];
}
// accumulators -> this workgroup's partial records (camera-major in hot_out: the per-camera kernel reads one run), 16-byte
// stores.  All record indices are requested first: one L2 round trip, not one per pass -- at the end (e0_lpl_h), or in the
// prologue, where the round trip hides behind the whole kernel (e0_lpl)
constexpr int LPL_FLUSH_PASSES = (HOT_ACC_MAX * 6 + E0C_BLOCK - 1) / E0C_BLOCK;
__device__ __forceinline__ void lpl_flush_request(const LplWg g, const V2& v, int (&rec)[LPL_FLUSH_PASSES]) {
#pragma unroll
  for (int u = 0; u < LPL_FLUSH_PASSES; ++u) {
    const int i = threadIdx.x + u * E0C_BLOCK;
    rec[u] = i < g.n_hot * 6 ? v.wg_slot_rec[g.cam0 + i / 6] : 0;
  }
}
__device__ __forceinline__ void lpl_flush_store(const LplWg g, const int (&rec)[LPL_FLUSH_PASSES], double* hot_out) {
#pragma unroll
  for (int u = 0; u < LPL_FLUSH_PASSES; ++u) {
    const int i = threadIdx.x + u * E0C_BLOCK;
    if (i < g.n_hot * 6)
      reinterpret_cast<double2*>(hot_out + (size_t)rec[u] * 12)[i % 6] = lpl_acc_sum(g.acc, g.n_slots, g.hubs, i / 6, i % 6);
  }
}
// the same as a plain loop (prepare_lpl[_h]: once per LM iteration, not once per term)
__device__ __forceinline__ void lpl_flush(const LplWg g, const V2& v, double* hot_out) {
  for (int i = threadIdx.x; i < g.n_hot * 6; i += E0C_BLOCK)
    reinterpret_cast<double2*>(hot_out + (size_t)v.wg_slot_rec[g.cam0 + i / 6] * 12)[i % 6] =
        lpl_acc_sum(g.acc, g.n_slots, g.hubs, i / 6, i % 6);
}
// red[0..5] += the upper triangle of Jl^T Jl, red[6..8] += Jl^T r over the four rows of a step-1 tile
__device__ __forceinline__ void acc_gram9(double* red, const double (&jl)[12], const double (&r)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    red[0] += jl[3 * k] * jl[3 * k];
    red[1] += jl[3 * k] * jl[3 * k + 1];
    red[2] += jl[3 * k] * jl[3 * k + 2];
    red[3] += jl[3 * k + 1] * jl[3 * k + 1];
    red[4] += jl[3 * k + 1] * jl[3 * k + 2];
    red[5] += jl[3 * k + 2] * jl[3 * k + 2];
    red[6] += jl[3 * k] * r[k];
    red[7] += jl[3 * k + 1] * r[k];
    red[8] += jl[3 * k + 2] * r[k];
  }
}

// ------------------------------------------------------------------------------------------
// Step types of back substitution: what differs between step 1 (pOSE, LplPose) and step 2 (joint, homogeneous, LplJoint).
// ------------------------------------------------------------------------------------------
struct LplPose {
  // ---- backsub_lpl: the arithmetic of OpBackVarproj.  Record: the UPDATED camera, its increment and the camera of the
  // linearisation point, from the camera-indexed arrays (record piece j: 0-5 cams4, 6-11 inc, 12-17 cams_lin4) ----
  static constexpr int BACK_REC = povar::BACK_REC, BACK_STRIDE = povar::BACK_STRIDE;
  __device__ static __forceinline__ const double* back_src(const Dp& d, int which) {
    return which == 0 ? reinterpret_cast<const double*>(d.cams4) : which == 1 ? d.inc : reinterpret_cast<const double*>(d.cams_lin4);
  }
  __device__ static __forceinline__ double2 back_piece(const Dp& d, int rank, int j) {
    return reinterpret_cast<const double2*>(back_src(d, j / 6) + 12 * (size_t)d.hot_cams[rank])[j % 6];
  }
  // which: 0 P_new, 1 inc, 2 P_lin, from the record (LDS) or from the camera-indexed global arrays (cold camera).  Two
  // branches, an LDS pointer or a global pointer, never a select of the two (lpl_read12)
  __device__ static __forceinline__ void back_part(const Dp& d, const double2* hot, int cw, int which, double4 (&o)[3]) {
    if (cw >= 0) lpl_read12(hot + lpl_cw_slot(cw) * BACK_STRIDE + 6 * which, o);
    else lpl_read12(reinterpret_cast<const double2*>(back_src(d, which) + 12 * (size_t)d.hot_cams[-2 - cw]), o);
  }
  struct BackLane {
    double4 h, hl, s4;  // the point, the linearisation point, the Jl column scale
    __device__ __forceinline__ void load(const V2& v, size_t li) {
      h = v.lmx[li];
      hl = v.lml[li];
      s4 = v.lsc[li];
    }
  };
  // H = Jl^T Jl and Jl^T res of the fresh, unweighted, unscaled tile
  template <bool ROBUST>
  __device__ static __forceinline__ void back_forward(const Dp& d, const double2* hot, const BackLane& L, const LplRow& cur, double* red) {
    double4 pp[3];
    back_part(d, hot, cur.cw, 0, pp);
    const Cam P = {pp[0], pp[1], pp[2]};
    double res[4], jl[12];
    pose_residual(d, P, L.h, cur.uv.x, cur.uv.y, res);
    pose_jl(d, P, cur.uv.x, cur.uv.y, 1.0, make_double4(1, 1, 1, 1), jl);
    acc_gram9(red, jl, res);
  }
  // the lane's delta and the updated point
  __device__ static __forceinline__ double4 back_solve(const Dp&, const V2&, size_t, const BackLane& L, const double* red, double (&dl)[4]) {
    double H[9], Hi[9];
    sym3(red, H);
    inv3(H, Hi);
    dl[0] = -(Hi[0] * red[6] + Hi[1] * red[7] + Hi[2] * red[8]);
    dl[1] = -(Hi[3] * red[6] + Hi[4] * red[7] + Hi[5] * red[8]);
    dl[2] = -(Hi[6] * red[6] + Hi[7] * red[7] + Hi[8] * red[8]);
    return make_double4(L.h.x + dl[0], L.h.y + dl[1], L.h.z + dl[2], L.h.w);
  }
  // the reference's model cost change (stored Jl and residual rebuilt from the linearisation point)
  template <bool ROBUST>
  __device__ static __forceinline__ void back_backward(const Dp& d, const double2* hot, const BackLane& L, const LplRow& cur,
                                                       const double (&dl)[4], double& sc) {
    double4 zz[3], pl[3];
    back_part(d, hot, cur.cw, 1, zz);
    back_part(d, hot, cur.cw, 2, pl);
    const Cam Pl = {pl[0], pl[1], pl[2]};
    const double sw = ROBUST ? sqrt(cur.w) : 1.0;
    double jinc[4], jls[12], rr[4];
    pose_jp_x(d, L.h, cur.uv.x, cur.uv.y, 1.0, zz, jinc);
    pose_jl(d, Pl, cur.uv.x, cur.uv.y, sw, L.s4, jls);
    pose_residual(d, Pl, L.hl, cur.uv.x, cur.uv.y, rr);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double ji = jinc[r] + (jls[3 * r] * dl[0] + jls[3 * r + 1] * dl[1] + jls[3 * r + 2] * dl[2]);
      sc -= ji * (0.5 * ji + sw * rr[r]);
    }
  }
};

struct LplJoint {
  // ---- backsub_lpl_h: OpBackJoint's arithmetic on e0_lpl_h's records (z = sigma * N_c inc, left in the record image by
  // cam_apply_inc_h, and P of the linearisation point) ----
  static constexpr int BACK_REC = HOT_REC_H, BACK_STRIDE = LPL_CAMREC_H;
  __device__ static __forceinline__ double2 back_piece(const Dp& d, int rank, int j) { return lpl_img(d, rank)[j]; }
  struct BackLane {
    double4 X, s4;  // the linearisation point and the Jl column scale: lane-ordered mirrors (V2)
    double hw[4], hbeta;
    __device__ __forceinline__ void load(const V2& v, size_t li) {
      X = v.lml[li];
      s4 = v.lsc[li];
      house4(X, hw, hbeta);
    }
  };
  // an observation's tile at the linearisation point and Jp * inc (z part of the record)
  struct BackObs {
    Hom h;
    double jl4[8], jl3[6], sw, jpi[2];
    template <bool ROBUST>
    __device__ __forceinline__ void set(const Dp& d, const double2* hot, const BackLane& L, const LplRow& cur) {
      // (select of an LDS and a global pointer: flat_loads; the split form spills here, see lpl_pass)
      const double2* hp = cur.cw >= 0 ? hot + lpl_cw_slot(cur.cw) * LPL_CAMREC_H : lpl_img(d, -2 - cur.cw);
      double4 zz[3];
      Cam P;
      lpl_read12(hp, zz);
      lpl_read_cam(hp + 6, P);
      sw = ROBUST ? sqrt(cur.w) : 1.0;
      h = hom_project(P, L.X, cur.uv.x, cur.uv.y);
      hom_jl4(P, h, sw, L.s4, jl4);
      jl3_of_jl4(jl4, L.hw, L.hbeta, jl3);
      hom_jp_x(h, L.X, sw, zz, jpi);
    }
  };
  // H = Jl3^T Jl3 and Jl3^T (r + Jp inc)
  template <bool ROBUST>
  __device__ static __forceinline__ void back_forward(const Dp& d, const double2* hot, const BackLane& L, const LplRow& cur, double* red) {
    BackObs o;
    o.template set<ROBUST>(d, hot, L, cur);
    acc_h6(red, o.jl3);
    const double a0 = o.sw * o.h.r0 + o.jpi[0], a1 = o.sw * o.h.r1 + o.jpi[1];
#pragma unroll
    for (int m = 0; m < 3; ++m) red[6 + m] += o.jl3[m] * a0 + o.jl3[3 + m] * a1;
  }
  // the damped increment, lifted with the landmark's tangent basis, and the updated point
  __device__ static __forceinline__ double4 back_solve(const Dp& d, const V2& v, size_t li, const BackLane& L, const double* red,
                                                       double (&dp)[4]) {
    OpBackJoint::delta4(d, L.X, red, dp);
    double4 Xc = v.lmx[li];
    Xc.x += dp[0] * L.s4.x; Xc.y += dp[1] * L.s4.y; Xc.z += dp[2] * L.s4.z; Xc.w += dp[3] * L.s4.w;
    return Xc;
  }
  template <bool ROBUST>
  __device__ static __forceinline__ void back_backward(const Dp& d, const double2* hot, const BackLane& L, const LplRow& cur,
                                                       const double (&dp)[4], double& sc) {
    BackObs o;
    o.template set<ROBUST>(d, hot, L, cur);
    const double rr[2] = {o.sw * o.h.r0, o.sw * o.h.r1};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const double ji = o.jpi[r] + (o.jl4[4 * r] * dp[0] + o.jl4[4 * r + 1] * dp[1] + o.jl4[4 * r + 2] * dp[2] + o.jl4[4 * r + 3] * dp[3]);
      sc -= ji * (0.5 * ji + rr[r]);
    }
  }
};
// the host sizes the launches with the *_lds_bytes functions: the single source of each size
static_assert(back_lds_bytes(3) == 3 * LplPose::BACK_STRIDE * sizeof(double2) + 16 && LplPose::BACK_REC <= LplPose::BACK_STRIDE, "step 1: backsub record");
static_assert(back_lds_bytes_h(3) == 3 * LplJoint::BACK_STRIDE * sizeof(double2) + 16 && LplJoint::BACK_REC <= LplJoint::BACK_STRIDE, "step 2: backsub record");
static_assert(pass_lds_bytes(3) == 3 * PASS_STRIDE * sizeof(double2) + 16 && PASS_REC <= PASS_STRIDE, "lpl_pass record");
static_assert(prep_lds_bytes(3) == 3 * PREP_STRIDE * sizeof(double2) + (3 + 3 * 3) * 96 + 16 && PREP_REC <= PREP_STRIDE, "prepare record");

// ------------------------------------------------------------------------------------------
// lpl_pass[_h] and prepare_lpl[_h]: one kernel per step, on the shared pieces.  One body per pair is not kept: the compiler
// simplifies a body and its step functions in their own context before it inlines them, that context orders the operands of
// commutative fadds, and the order decides which product is contracted into an fma: lpl_pass_h<0> and prepare_lpl came out
// with other last bits (profiles/lpl_steps_isa.txt).  backsub_lpl[_h] did not and is merged below.
// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// K2 / K3 + K5 on the lane-per-landmark layout: one forward walk over the rows, camera matrices in LDS (96 B per slot),
// no accumulators.
//   MODE 0  linearize_landmark_pOSE + scale_Jl_cols_pOSE (landmark_block.hpp:135-178, 284-295) at (cams_lin4, lms_lin4):
//           robust weight per observation (V2::w), Jl column scale per landmark, finiteness flag.  The per-slot
//           sqrt(w) / weighted residual arrays of the lane-per-observation kernels are NOT written: the lane-per-landmark
//           kernels rebuild both from (P, x, u, v, w); povar_lm.hip fills them when a legacy kernel asks (ensure_legacy).
//   MODE 1  compute_error_pOSE (bal_bundle_adjustment_helper.cpp:117-154) at (cams4, lms4): (error, |r|, count) summed per
//           workgroup into part[3 * blockIdx.x ..].
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(E0C_BLOCK) void lpl_pass(Dp d, double* part) {
  extern __shared__ double2 hot[];  // [n_hot][PASS_REC] records, then the tile counter
  __shared__ double sh[3 * (E0C_BLOCK / 64)];
  const V2& v = d.v2;
  const double4* cams = MODE == 0 ? d.cams_lin4 : d.cams4;
  const LplWg g = lpl_wg<false>(v, hot, PASS_STRIDE, 0);
  lpl_stage<PASS_REC, PASS_STRIDE>(g, v, hot, [&](int rank, int j) {
    return reinterpret_cast<const double2*>(cams + 3 * (size_t)d.hot_cams[rank])[j];
  });
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const LplTiles T(v, g.ctr, lane);
  const int t_end = T.t_end;
  int c_t = T.grab();
  LplStream1 rows;
  rows.start(T, v, c_t);
  double sc[3] = {0, 0, 0};
  int bad = 0;
  while (c_t < t_end) {
    int c_row0, c_k, c_nh, c_fl;
    T.info(c_t, c_row0, c_k, c_nh, c_fl);
    const double4 h = v.lmx[(size_t)c_t * WAVE + lane];
    if (MODE == 0) v.lml[(size_t)c_t * WAVE + lane] = h;  // the linearisation point, lane-ordered, is left behind
    double red[3] = {0, 0, 0};
    for (int j = 0; j < c_k; ++j) {
      const LplRow cur = rows.next(T, v);
      if (cur.cw == -1) continue;
      // (a select of an LDS and a global pointer: six flat_loads.  Measured against ds_read / global_load in two branches
      // -- profiles/r02_ablations.txt item 16 --: the branches join with a wait on both counters, which drains the row
      // prefetch every step: 50 instead of 44 us here; the two-pass kernels with their longer steps gain from the split)
      const double2* hp = cur.cw >= 0 ? hot + lpl_cw_slot(cur.cw) * PASS_STRIDE
                                      : reinterpret_cast<const double2*>(cams + 3 * (size_t)d.hot_cams[-2 - cur.cw]);
      Cam P;
      lpl_read_cam(hp, P);
      double res[4];
      pose_residual(d, P, h, cur.uv.x, cur.uv.y, res);
      const double r2 = res[0] * res[0] + res[1] * res[1] + res[2] * res[2] + res[3] * res[3];
      double e, w;
      error_weight(d, r2, e, w);
      if (MODE == 0) {
        const double sw = sqrt(w);
        bad |= !isfinite(r2) || !isfinite(sw);
        if (d.robust && v.w) v.w[((size_t)c_row0 + j) * WAVE + lane] = w;
        double jl[12];
        pose_jl(d, P, cur.uv.x, cur.uv.y, sw, make_double4(1, 1, 1, 1), jl);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          red[0] += jl[3 * r] * jl[3 * r];
          red[1] += jl[3 * r + 1] * jl[3 * r + 1];
          red[2] += jl[3 * r + 2] * jl[3 * r + 2];
        }
      } else {
        bad |= !isfinite(r2);
        sc[0] += e;
        sc[1] += sqrt(r2);
        sc[2] += 1.0;
      }
    }
    if (MODE == 0) {
      const int sg = v.seg[(size_t)c_t * WAVE + lane];
      if (c_fl & 1) seg_reduce_steps<3>(red, lane, sg & 255, (sg >> 8) & 255, 4);
      const double4 sc4 = d.scale_jl ? make_double4(1.0 / (d.eps + sqrt(red[0])), 1.0 / (d.eps + sqrt(red[1])),
                                                    1.0 / (d.eps + sqrt(red[2])), 0.0)
                                     : make_double4(1.0, 1.0, 1.0, 0.0);
      // every lane of the landmark holds the segment total.  The landmark-order copy (Dp::jl_scale4) is not written
      // here: lanes_to_lm fills it when a lane-per-observation kernel or an export asks (povar_lm.hip: ensure_legacy)
      v.lsc[(size_t)c_t * WAVE + lane] = sc4;
    }
    c_t = rows.advance(T);
  }
  if (bad) atomicOr(&d.flags[0], 1);
  if (MODE == 1) {
    block_sum<3, E0C_BLOCK>(sc, sh);
    if (threadIdx.x == 0) {
      part[3 * (size_t)blockIdx.x] = sc[0];
      part[3 * (size_t)blockIdx.x + 1] = sc[1];
      part[3 * (size_t)blockIdx.x + 2] = sc[2];
    }
  }
}

// K2' / K3' + K5' on the lane-per-landmark layout (the step-2 twins of lpl_pass, povar_kernels.hpp):
//   MODE 0  linearize_landmark_projective_space_homogeneous + scale_Jl_cols_homogeneous (landmark_block.hpp:180-225,
//           298-309) at (cams_lin4, lms_lin4): robust weight per observation (V2::w), the four Jl column scales per
//           landmark, finiteness flag; the per-slot arrays of the lane-per-observation kernels follow lazily.
//   MODE 1  compute_error_projective_space_homogeneous (helper.cpp:157-196) at (cams4, lms4): the six sums of OpErrorH
//           per workgroup into part[6 * blockIdx.x ..].
template <int MODE>
__global__ __launch_bounds__(E0C_BLOCK) void lpl_pass_h(Dp d, double* part) {
  extern __shared__ double2 hot[];  // [n_hot][PASS_REC] records (P_c row-major), then the tile counter
  __shared__ double sh[6 * (E0C_BLOCK / 64)];
  const V2& v = d.v2;
  const double4* cams = MODE == 0 ? d.cams_lin4 : d.cams4;
  const LplWg g = lpl_wg<false>(v, hot, PASS_STRIDE, 0);
  lpl_stage<PASS_REC, PASS_STRIDE>(g, v, hot, [&](int rank, int j) {
    return reinterpret_cast<const double2*>(cams + 3 * (size_t)d.hot_cams[rank])[j];
  });
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const LplTiles T(v, g.ctr, lane);
  const int t_end = T.t_end;
  int c_t = T.grab();
  LplStream1 rows;
  rows.start(T, v, c_t);
  double sc[6] = {0, 0, 0, 0, 0, 0};
  int bad = 0;
  while (c_t < t_end) {
    int c_row0, c_k, c_nh, c_fl;
    T.info(c_t, c_row0, c_k, c_nh, c_fl);
    const double4 X = v.lmx[(size_t)c_t * WAVE + lane];
    if (MODE == 0) v.lml[(size_t)c_t * WAVE + lane] = X;  // the linearisation point, lane-ordered, is left behind
    double red[4] = {0, 0, 0, 0};
    for (int j = 0; j < c_k; ++j) {
      const LplRow cur = rows.next(T, v);
      if (cur.cw == -1) continue;
      // (a select of an LDS and a global pointer: six flat_loads.  Measured against ds_read / global_load in two branches
      // -- profiles/r02_ablations.txt item 16 --: the branches join with a wait on both counters, which drains the row
      // prefetch every step: 50 instead of 44 us here; the two-pass kernels with their longer steps gain from the split)
      const double2* hp = cur.cw >= 0 ? hot + lpl_cw_slot(cur.cw) * PASS_STRIDE
                                      : reinterpret_cast<const double2*>(cams + 3 * (size_t)d.hot_cams[-2 - cur.cw]);
      Cam P;
      lpl_read_cam(hp, P);
      const Hom h = hom_project(P, X, cur.uv.x, cur.uv.y);
      const double r2 = h.r0 * h.r0 + h.r1 * h.r1;
      double e, w;
      error_weight(d, r2, e, w);
      if (MODE == 0) {
        const double sw = sqrt(w);
        bad |= !isfinite(r2) || !isfinite(sw) || !isfinite(h.D02) || !isfinite(h.D12);
        if (d.robust && v.w) v.w[((size_t)c_row0 + j) * WAVE + lane] = w;
        double jl[8];
        hom_jl4(P, h, sw, make_double4(1, 1, 1, 1), jl);
#pragma unroll
        for (int m = 0; m < 4; ++m) red[m] += jl[m] * jl[m] + jl[4 + m] * jl[4 + m];
      } else {
        bad |= !isfinite(r2);
        sc[0] += e; sc[1] += sqrt(r2); sc[2] += 1.0;
        if (h.valid) { sc[3] += e; sc[4] += sqrt(r2); sc[5] += 1.0; }
      }
    }
    if (MODE == 0) {
      const int sg = v.seg[(size_t)c_t * WAVE + lane];
      if (c_fl & 1) seg_reduce_steps<4>(red, lane, sg & 255, (sg >> 8) & 255, 4);
      // lane-ordered; the landmark-order copy (Dp::jl_scale4) is filled on demand (povar_lm.hip: ensure_legacy)
      v.lsc[(size_t)c_t * WAVE + lane] = make_double4(1.0 / (d.eps + sqrt(red[0])), 1.0 / (d.eps + sqrt(red[1])),
                                                      1.0 / (d.eps + sqrt(red[2])), 1.0 / (d.eps + sqrt(red[3])));
    }
    c_t = rows.advance(T);
  }
  if (bad) atomicOr(&d.flags[0], 1);
  if (MODE == 1) {
    block_sum<6, E0C_BLOCK>(sc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) part[6 * (size_t)blockIdx.x + k] = sc[k];
    }
  }
}

// ------------------------------------------------------------------------------------------
// K7 on the lane-per-landmark layout: get_Hll_inv_add_Hpp_b_pOSE / _poBA (landmark_block.hpp:510-572), the
// landmark half of prepare_Hb_pOSE.  Same structure as e0_lpl (lane = landmark, rows from an LplStream2,
// camera records and per-camera accumulators in LDS, cold observations through q4c): the forward
// pass accumulates Hll = Jl^T Jl and Jl^T r in registers, the lane then inverts Hll (+ lambda I for
// POWER_SCHUR_COMPLEMENT), stores Hll^-1 and the per-term landmark records, and the backward pass adds
// Jp^T (r - Jl w) into the camera accumulators.  The tile (Jl, r) is rebuilt from (P_c, x_l, u, v, sqrt(w), s_l):
// nothing per observation is read besides the 20-byte row.  Replaces lm_regular<OpPrepare> + cm_scatter +
// cam_sum_items (214 + 109 + 6 us on venice-1778) for the LDSACC mode.
// ------------------------------------------------------------------------------------------
template <bool ROBUST>
__global__ __launch_bounds__(E0C_BLOCK) void prepare_lpl(Dp d, double* hot_out) {
  extern __shared__ double2 hot[];  // [n_hot][PREP_REC] records, then acc[12][n_slots], then the tile counter
  const V2& v = d.v2;
  const LplWg g = lpl_wg<true>(v, hot, PREP_STRIDE, 0);
  const double2* rec_img = reinterpret_cast<const double2*>(d.hot_rec);
  lpl_stage<PREP_REC, PREP_STRIDE>(g, v, hot, [&](int rank, int j) { return lpl_img(d, rank)[6 + j]; });  // entries 12..23 of the image
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const LplTiles T(v, g.ctr, lane);
  const int t_end = T.t_end;
  int c_t = T.grab(), c_row0 = 0, c_k = 0, c_nh = 0, c_fl = 0;
  if (c_t < t_end) T.info(c_t, c_row0, c_k, c_nh, c_fl);
  LplStream2<ROBUST> rows;
  rows.start(T, v, c_t, c_row0, c_k, c_t < t_end ? T.grab() : t_end);
  while (c_t < t_end) {
    // the lane's landmark: coordinates and Jl column scale (gathers; once per tile)
    const int lm = v.lm_of[(size_t)c_t * WAVE + lane];
    const int sg = v.seg[(size_t)c_t * WAVE + lane];
    const double4 h4 = v.lml[(size_t)c_t * WAVE + lane], s4 = v.lsc[(size_t)c_t * WAVE + lane];
    const double hx = h4.x, hy = h4.y, hz = h4.z;
    double red[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < c_k; ++j) {
      const LplRow cur = rows.next(T, v);
      if (cur.cw == -1) continue;
      double P[12];
      if (cur.cw >= 0) prep_read_rec(hot + lpl_cw_slot(cur.cw) * PREP_STRIDE, P);
      else prep_read_rec(rec_img + (size_t)(-2 - cur.cw) * (HOT_REC_STRIDE / 2) + 6, P);
      PrepObs o;
      o.set(d, P, cur.uv, ROBUST ? cur.w : 1.0, hx, hy, hz, s4.x, s4.y, s4.z);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[0] += o.jl[3 * r] * o.jl[3 * r];
        red[1] += o.jl[3 * r] * o.jl[3 * r + 1];
        red[2] += o.jl[3 * r] * o.jl[3 * r + 2];
        red[3] += o.jl[3 * r + 1] * o.jl[3 * r + 1];
        red[4] += o.jl[3 * r + 1] * o.jl[3 * r + 2];
        red[5] += o.jl[3 * r + 2] * o.jl[3 * r + 2];
        red[6] += o.jl[3 * r] * o.r[r];
        red[7] += o.jl[3 * r + 1] * o.r[r];
        red[8] += o.jl[3 * r + 2] * o.r[r];
      }
    }
    if (c_fl & 1) seg_reduce_steps<9>(red, lane, sg & 255, (sg >> 8) & 255, 4);
    double Hi[9], w3[3] = {0, 0, 0};
    if (lm >= 0) {
      double H[9];
      sym3(red, H);
      H[0] += d.lambda_lm;
      H[4] += d.lambda_lm;
      H[8] += d.lambda_lm;
      inv3(H, Hi);
      w3[0] = Hi[0] * red[6] + Hi[1] * red[7] + Hi[2] * red[8];
      w3[1] = Hi[3] * red[6] + Hi[4] * red[7] + Hi[5] * red[8];
      w3[2] = Hi[6] * red[6] + Hi[7] * red[7] + Hi[8] * red[8];
      // per-term record of this lane (e0_lpl); Hll^-1 and the row-major record of the other kernels once per landmark
      double* r2 = v.lmrec + ((size_t)c_t * 9) * WAVE + lane;
      r2[0] = hx; r2[WAVE] = hy; r2[2 * WAVE] = hz;
      r2[3 * WAVE] = s4.x * Hi[0] * s4.x; r2[4 * WAVE] = s4.x * Hi[1] * s4.y; r2[5 * WAVE] = s4.x * Hi[2] * s4.z;
      r2[6 * WAVE] = s4.y * Hi[4] * s4.y; r2[7 * WAVE] = s4.y * Hi[5] * s4.z; r2[8 * WAVE] = s4.z * Hi[8] * s4.z;
      if (lane == (sg & 255) && !d.prep_lpl_only) {
#pragma unroll
        for (int m = 0; m < 9; ++m) d.hll_inv[9 * (size_t)lm + m] = Hi[m];
        double4* rec = reinterpret_cast<double4*>(d.lmrec) + 3 * (size_t)lm;
        rec[0] = make_double4(hx, hy, hz, s4.x);
        rec[1] = make_double4(s4.y, s4.z, Hi[0], Hi[1]);
        rec[2] = make_double4(Hi[2], Hi[4], Hi[5], Hi[8]);
      }
    }
    for (int jj = 0; jj < c_k; ++jj) {
      const int j = c_k - 1 - jj;
      const LplRow cur = rows.next(T, v);
      if (cur.cw == -1) continue;
      double P[12];
      if (cur.cw >= 0) prep_read_rec(hot + lpl_cw_slot(cur.cw) * PREP_STRIDE, P);
      else prep_read_rec(rec_img + (size_t)(-2 - cur.cw) * (HOT_REC_STRIDE / 2) + 6, P);
      PrepObs o;
      const double w = ROBUST ? cur.w : 1.0;
      o.set(d, P, cur.uv, w, hx, hy, hz, s4.x, s4.y, s4.z);
      double e[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = o.r[r] - (o.jl[3 * r] * w3[0] + o.jl[3 * r + 1] * w3[1] + o.jl[3 * r + 2] * w3[2]);
      const double4 q = pose_q(d, cur.uv.x, cur.uv.y, sqrt(w), e);
      if (cur.cw >= 0) {
        lpl_scatter(g, cur.cw, make_double4(hx, hy, hz, 1.0), q);
      } else {
        d.q4c[lpl_cold_at(d, c_fl, c_nh, c_row0, j, lane)] = make_double4(q.x, q.y, q.z, 0);
      }
    }
    c_t = rows.nx_t;
    if (c_t < t_end) {
      T.info(c_t, c_row0, c_k, c_nh, c_fl);
      rows.ahead(T.grab());
    }
  }
  __syncthreads();
  lpl_flush(g, v, hot_out);
}

// K7' on the lane-per-landmark layout: get_Hll_inv_add_Hpp_b_joint (landmark_block.hpp:474-507), the landmark half
// of prepare_Hb_joint -- prepare_lpl (povar_kernels.hpp) with the homogeneous tile.  Forward pass: Hll = Jl3^T Jl3
// and Jl3^T r in registers; the lane inverts Hll + lambda I, stores Hll^-1 and the landmark records of the per-term
// kernels; backward pass: Jp^T (r - Jl3 w) into the camera accumulators (12 ambient values per observation; the
// tangent projection N_c^T is applied per camera afterwards, cam_nt_project).  Replaces lm_regular<OpPrepareH> +
// cm_scatter + cam_sum_items_h (495 + 124 + 6 us on venice-1778) for the LDSACC mode.
template <bool ROBUST>
__global__ __launch_bounds__(E0C_BLOCK) void prepare_lpl_h(Dp d, double* hot_out) {
  extern __shared__ double2 hot[];  // [n_hot][PREP_REC] records (P_c row-major), then acc[12][n_slots], then the tile counter
  const V2& v = d.v2;
  const LplWg g = lpl_wg<true>(v, hot, PREP_STRIDE, 0);
  const double2* rec_img = reinterpret_cast<const double2*>(d.hot_rec);
  lpl_stage<PREP_REC, PREP_STRIDE>(g, v, hot, [&](int rank, int j) { return lpl_img(d, rank)[6 + j]; });  // entries 12..23 of the image
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const LplTiles T(v, g.ctr, lane);
  const int t_end = T.t_end;
  int c_t = T.grab(), c_row0 = 0, c_k = 0, c_nh = 0, c_fl = 0;
  if (c_t < t_end) T.info(c_t, c_row0, c_k, c_nh, c_fl);
  LplStream2<ROBUST> rows;
  rows.start(T, v, c_t, c_row0, c_k, c_t < t_end ? T.grab() : t_end);
  while (c_t < t_end) {
    const int lm = v.lm_of[(size_t)c_t * WAVE + lane];
    const int sg = v.seg[(size_t)c_t * WAVE + lane];
    const double4 X = v.lml[(size_t)c_t * WAVE + lane], s4 = v.lsc[(size_t)c_t * WAVE + lane];  // lane-ordered mirrors (V2)
    double hw[4], hbeta;
    house4(X, hw, hbeta);
    double red[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < c_k; ++j) {
      const LplRow cur = rows.next(T, v);
      if (cur.cw == -1) continue;
      Cam P;
      // LDS pointer or global pointer, never a select of the two (lpl_read12)
      if (cur.cw >= 0) lpl_read_cam(hot + lpl_cw_slot(cur.cw) * PREP_STRIDE, P);
      else lpl_read_cam(rec_img + (size_t)(-2 - cur.cw) * (HOT_REC_STRIDE / 2) + 6, P);
      const double sw = ROBUST ? sqrt(cur.w) : 1.0;
      const Hom h = hom_project(P, X, cur.uv.x, cur.uv.y);
      double jl4[8], jl3[6];
      hom_jl4(P, h, sw, s4, jl4);
      jl3_of_jl4(jl4, hw, hbeta, jl3);
      const double r0 = sw * h.r0, r1 = sw * h.r1;
      acc_h6(red, jl3);
#pragma unroll
      for (int m = 0; m < 3; ++m) red[6 + m] += jl3[m] * r0 + jl3[3 + m] * r1;
    }
    if (c_fl & 1) seg_reduce_steps<9>(red, lane, sg & 255, (sg >> 8) & 255, 4);
    double w3[3] = {0, 0, 0};
    if (lm >= 0) {
      double Hi[9];
      hinv_damped(red, d.lambda_lm, Hi);
      w3[0] = Hi[0] * red[6] + Hi[1] * red[7] + Hi[2] * red[8];
      w3[1] = Hi[3] * red[6] + Hi[4] * red[7] + Hi[5] * red[8];
      w3[2] = Hi[6] * red[6] + Hi[7] * red[7] + Hi[8] * red[8];
      // per-term record of this lane (e0_lpl_h); Hll^-1 and the row-major record of the other kernels once per landmark
      double* r2 = v.lmrec + ((size_t)c_t * LPL_REC_H) * WAVE + lane;
      const double rv[LPL_REC_H] = {X.x, X.y, X.z, X.w, s4.x, s4.y, s4.z, s4.w, Hi[0], Hi[1], Hi[2], Hi[4], Hi[5], Hi[8]};
#pragma unroll
      for (int m = 0; m < LPL_REC_H; ++m) r2[m * WAVE] = rv[m];
      if (lane == (sg & 255) && !d.prep_lpl_only) {
#pragma unroll
        for (int m = 0; m < 9; ++m) d.hll_inv[9 * (size_t)lm + m] = Hi[m];
        double4* rec = reinterpret_cast<double4*>(d.lmrec) + 4 * (size_t)lm;
        rec[0] = X;
        rec[1] = s4;
        rec[2] = make_double4(Hi[0], Hi[1], Hi[2], Hi[4]);
        rec[3] = make_double4(Hi[5], Hi[8], 0, 0);
      }
    }
    for (int jj = 0; jj < c_k; ++jj) {
      const int j = c_k - 1 - jj;
      const LplRow cur = rows.next(T, v);
      if (cur.cw == -1) continue;
      Cam P;
      // LDS pointer or global pointer, never a select of the two (lpl_read12)
      if (cur.cw >= 0) lpl_read_cam(hot + lpl_cw_slot(cur.cw) * PREP_STRIDE, P);
      else lpl_read_cam(rec_img + (size_t)(-2 - cur.cw) * (HOT_REC_STRIDE / 2) + 6, P);
      const double sw = ROBUST ? sqrt(cur.w) : 1.0;
      const Hom h = hom_project(P, X, cur.uv.x, cur.uv.y);
      double jl4[8], jl3[6];
      hom_jl4(P, h, sw, s4, jl4);
      jl3_of_jl4(jl4, hw, hbeta, jl3);
      const double e0 = sw * h.r0 - (jl3[0] * w3[0] + jl3[1] * w3[1] + jl3[2] * w3[2]);
      const double e1 = sw * h.r1 - (jl3[3] * w3[0] + jl3[4] * w3[1] + jl3[5] * w3[2]);
      const double4 q = hom_q(h, sw, e0, e1);
      if (cur.cw >= 0) {
        lpl_scatter(g, cur.cw, X, q);
      } else {
        d.q4c[lpl_cold_at(d, c_fl, c_nh, c_row0, j, lane)] = q;
      }
    }
    c_t = rows.nx_t;
    if (c_t < t_end) {
      T.info(c_t, c_row0, c_k, c_nh, c_fl);
      rows.ahead(T.grab());
    }
  }
  __syncthreads();
  lpl_flush(g, v, hot_out);
}

// ------------------------------------------------------------------------------------------
// K12 on the lane-per-landmark layout: back_substitute_pOSE (landmark_block.hpp:670-707), POWER_VARPROJ, and, step 2,
// back_substitute_joint (:574-623), on prepare_lpl's row stream.  Camera records in LDS (Step::BACK_REC), no accumulators.
// First pass: H and the right-hand side of the lane's 3 x 3 system; the lane solves for its landmark's update and stores the
// new point; second pass: the reference's model cost change, summed per workgroup into part[blockIdx.x].
// Replaces lm_regular<OpBackVarproj> (204 us on venice-1778) / lm_regular<OpBackJoint> for the LDSACC mode.
// ------------------------------------------------------------------------------------------
template <class Step, bool ROBUST>
__device__ __forceinline__ void backsub_lpl_body(const Dp& d, double* part) {
  __shared__ double sh[E0C_BLOCK / 64];
  const V2& v = d.v2;
  extern __shared__ double2 hot[];  // [n_hot][BACK_REC] records, then the tile counter
  const LplWg g = lpl_wg<false>(v, hot, Step::BACK_STRIDE, 0);
  lpl_stage<Step::BACK_REC, Step::BACK_STRIDE>(g, v, hot, [&](int rank, int j) { return Step::back_piece(d, rank, j); });
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const LplTiles T(v, g.ctr, lane);
  const int t_end = T.t_end;
  int c_t = T.grab(), c_row0 = 0, c_k = 0, c_nh = 0, c_fl = 0;
  if (c_t < t_end) T.info(c_t, c_row0, c_k, c_nh, c_fl);
  LplStream2<ROBUST> rows;
  rows.start(T, v, c_t, c_row0, c_k, c_t < t_end ? T.grab() : t_end);
  double sc = 0;
  while (c_t < t_end) {
    const size_t li = (size_t)c_t * WAVE + lane;
    const int lm = v.lm_of[li];
    const int sg = v.seg[li];
    typename Step::BackLane L;
    L.load(v, li);
    double red[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < c_k; ++j) {
      const LplRow cur = rows.next(T, v);
      if (cur.cw == -1) continue;
      Step::template back_forward<ROBUST>(d, hot, L, cur, red);
    }
    if (c_fl & 1) seg_reduce_steps<9>(red, lane, sg & 255, (sg >> 8) & 255, 4);
    double dl[4] = {0, 0, 0, 0};
    if (lm >= 0) {
      const double4 hn = Step::back_solve(d, v, li, L, red, dl);
      v.lmx[li] = hn;  // the mirror stays current: no rebuild after an accepted step
      if (lane == (sg & 255)) d.lms4[lm] = hn;
    }
    for (int jj = 0; jj < c_k; ++jj) {
      const LplRow cur = rows.next(T, v);
      if (cur.cw == -1) continue;
      Step::template back_backward<ROBUST>(d, hot, L, cur, dl, sc);
    }
    c_t = rows.nx_t;
    if (c_t < t_end) {
      T.info(c_t, c_row0, c_k, c_nh, c_fl);
      rows.ahead(T.grab());
    }
  }
  double sv[1] = {sc};
  block_sum<1, E0C_BLOCK>(sv, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = sv[0];
}

// ------------------------------------------------------------------------------------------
// The two back-substitution kernels the host launches.
// ------------------------------------------------------------------------------------------
template <bool ROBUST>
__global__ __launch_bounds__(E0C_BLOCK) void backsub_lpl(Dp d, double* part) { backsub_lpl_body<LplPose, ROBUST>(d, part); }
template <bool ROBUST>
__global__ __launch_bounds__(E0C_BLOCK) void backsub_lpl_h(Dp d, double* part) { backsub_lpl_body<LplJoint, ROBUST>(d, part); }

// ------------------------------------------------------------------------------------------
// K10, lane-per-landmark form (default of POVAR_E0_IMPLICIT_LDSACC): right_mul_e0_pOSE / right_mul_e0_joint
// (linearization_power_varproj.hpp:364-406, 408-453) with lane = landmark.  The per-landmark sum u = Jl^T t is a register
// accumulation over the rows of the tile (no wavefront scan, no segment metadata), v = Hll^-1 u is computed
// once per landmark instead of once per observation, and every global address is static, so the row stream is
// prefetched without dependent loads.  Per observation: 20 B from HBM (uv, camera rank), 72 B (step 2: 112 B) per landmark.
// Camera records of the cameras a workgroup keeps live in LDS together with their Jp^T s accumulators; observations of colder
// cameras gather the record from the rank-ordered image in L2 and leave their three scatter scalars in the cold view (q4c).
// The next tile's landmark record is requested when the backward pass starts.
// Two kernels on the shared pieces, not one body: step 1 has ONE backward arm for LDS-resident cameras (`j < c_nh || cw >= 0`),
// step 2 keeps the wave-uniform `j < c_nh` arm apart from the divergent one; folding them takes 71 of e0_lpl_h<false>'s 376
// fp64 instructions away (profiles/lpl_steps_isa.txt), so one body would need a second switch beside the prologue's.
// ------------------------------------------------------------------------------------------
// Step 1.  Records: z_c, P_c[:, :3] (HOT_REC double2, stride HOT_REC); the lane carries x and G = S Hll^-1 S (9 doubles of
// lmrec).  G is dead when the backward pass starts (g = G u is formed), so only the three coordinates need a second set of
// registers for the next tile's record.
template <bool ROBUST>
__global__ __launch_bounds__(E0C_BLOCK) void e0_lpl(Dp d, double* hot_out) {
  const int done = d.flags[1];  // requested first, tested after the LDS staging (no global side effects before)
  extern __shared__ double2 hot[];  // [n_hot][HOT_REC] records, then acc[12][n_slots], then the tile counter
  const V2& v = d.v2;
  // the first tile of every wavefront is dealt statically (tiles are sorted longest first: the same tiles the first
  // sixteen grabs would return), the counter serves the later ones
  const LplWg g = lpl_wg<true>(v, hot, HOT_REC, E0C_BLOCK / WAVE);
  // staging, part 1: slot -> camera rank (the record pieces, a second dependent round trip, are requested further down:
  // the wavefront's first rows and landmark record go out in between, so the three latencies overlap instead of adding
  // up -- they are the fixed cost of a launch, a third of the kernel on an 8-GPU shard)
  constexpr int PASSES = (HOT_ACC_MAX * HOT_REC + E0C_BLOCK - 1) / E0C_BLOCK;
  int rk[PASSES];
#pragma unroll
  for (int u = 0; u < PASSES; ++u) {
    const int i = threadIdx.x + u * E0C_BLOCK;
    rk[u] = i < g.n_hot * HOT_REC ? v.wg_cams[g.cam0 + i / HOT_REC] : 0;
  }
  // where the accumulators go at the end (partial record of each slot): requested now, used after the last tile
  int frec[LPL_FLUSH_PASSES];
  lpl_flush_request(g, v, frec);
  const int lane = threadIdx.x & 63;
  const LplTiles T(v, g.ctr, lane);
  const int t_end = T.t_end;
  int c_t = T.nth(__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))), c_row0 = 0, c_k = 0, c_nh = 0, c_fl = 0;
  if (c_t < t_end) T.info(c_t, c_row0, c_k, c_nh, c_fl);
  // the first rows go out now; the tile after this one is taken behind the staging barrier below (the counter lives in LDS)
  LplStream2<ROBUST> rows;
  rows.start(T, v, c_t, c_row0, c_k, t_end);
  double hx = 0, hy = 0, hz = 0, G00 = 0, G01 = 0, G02 = 0, G11 = 0, G12 = 0, G22 = 0;
  if (c_t < t_end) {
    const double* rp = v.lmrec + ((size_t)c_t * 9) * WAVE + lane;
    hx = rp[0]; hy = rp[WAVE]; hz = rp[2 * WAVE];
    G00 = rp[3 * WAVE]; G01 = rp[4 * WAVE]; G02 = rp[5 * WAVE]; G11 = rp[6 * WAVE]; G12 = rp[7 * WAVE]; G22 = rp[8 * WAVE];
  }
  {
    // staging, part 2: the record pieces into LDS
    double2 piece[PASSES];
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      const int i = threadIdx.x + u * E0C_BLOCK;
      piece[u] = lpl_img(d, rk[u])[i % HOT_REC];
    }
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      const int i = threadIdx.x + u * E0C_BLOCK;
      if (i < g.n_hot * HOT_REC) hot[i] = piece[u];
    }
  }
  __syncthreads();
  if (done) return;
  if (c_t < t_end) rows.ahead(T.grab());
  while (c_t < t_end) {
    double red[3] = {0, 0, 0};
    for (int j = 0; j < c_k; ++j) {
      const LplRow cur = rows.next(T, v);
      double zz[12], P3[9];
      LplObs o;
      o.set(d, cur.uv, ROBUST ? cur.w : 1.0);
      if (j < c_nh) {  // wave-uniform: every lane has an observation of an LDS-resident camera in this row
        const double2* h = hot + lpl_cw_slot(cur.cw) * HOT_REC;
        lpl_read_zz(h, zz);
        lpl_read_p3(h, P3);
        lpl_forward(o, zz, P3, hx, hy, hz, red);
      } else if (cur.cw != -1) {
        if (cur.cw >= 0) {
          const double2* h = hot + lpl_cw_slot(cur.cw) * HOT_REC;
          lpl_read_zz(h, zz);
          lpl_read_p3(h, P3);
        } else {  // cold: camera with popularity rank -2 - cw, record from the rank-ordered image (L2)
          const double2* h = lpl_img(d, -2 - cur.cw);
          lpl_read_zz(h, zz);
          lpl_read_p3(h, P3);
        }
        lpl_forward(o, zz, P3, hx, hy, hz, red);
      }
    }
    if (c_fl & 1) {  // landmarks dealt over several lanes: sum their partial u = Jl^T t (segmented wavefront scan)
      const int sg = v.seg[(size_t)c_t * WAVE + lane];
      seg_reduce_steps<3>(red, lane, sg & 255, (sg >> 8) & 255, 4);
    }
    const double gv[3] = {G00 * red[0] + G01 * red[1] + G02 * red[2], G01 * red[0] + G11 * red[1] + G12 * red[2],
                          G02 * red[0] + G12 * red[1] + G22 * red[2]};
    // the next tile's record: G into its own (now dead) registers, the coordinates into a second set
    const int n_t = rows.nx_t;
    double nhx = 0, nhy = 0, nhz = 0;
    if (n_t < t_end) {
      const double* rp = v.lmrec + ((size_t)n_t * 9) * WAVE + lane;
      nhx = rp[0]; nhy = rp[WAVE]; nhz = rp[2 * WAVE];
      G00 = rp[3 * WAVE]; G01 = rp[4 * WAVE]; G02 = rp[5 * WAVE]; G11 = rp[6 * WAVE]; G12 = rp[7 * WAVE]; G22 = rp[8 * WAVE];
    }
    for (int jj = 0; jj < c_k; ++jj) {
      const int j = c_k - 1 - jj;
      const LplRow cur = rows.next(T, v);
      double P3[9], q[3];
      LplObs o;
      o.set(d, cur.uv, ROBUST ? cur.w : 1.0);
      if (j < c_nh || cur.cw >= 0) {
        lpl_read_p3(hot + lpl_cw_slot(cur.cw) * HOT_REC, P3);
        lpl_backward(o, P3, gv, q);
        lpl_scatter(g, cur.cw, make_double4(hx, hy, hz, 1.0), make_double4(q[0], q[1], q[2], 0));
      } else if (cur.cw < -1) {
        const int cold_at = lpl_cold_at(d, c_fl, c_nh, c_row0, j, lane);
        lpl_read_p3(lpl_img(d, -2 - cur.cw), P3);
        lpl_backward(o, P3, gv, q);
        d.q4c[cold_at] = make_double4(q[0], q[1], q[2], 0);
      }
    }
    c_t = n_t;
    if (c_t < t_end) {
      T.info(c_t, c_row0, c_k, c_nh, c_fl);
      rows.ahead(T.grab());
    }
    hx = nhx; hy = nhy; hz = nhz;
  }
  __syncthreads();
  lpl_flush_store(g, frec, hot_out);
  if (d.p2p_epoch && blockIdx.x == 0 && threadIdx.x == 0) *d.p2p_epoch += 1;  // one tick per term, read by the next kernels
}

// Step 2, with the 2-row tiles.  Records: z = sigma * N_c x_c, then the full P_c (HOT_REC_H double2, stride LPL_CAMREC_H); the
// lane carries X, the Jl column scale and Hll^-1 (LPL_REC_H doubles of lmrec).  Plain prologue; register-tight: <true> spills
// 6 VGPRs (profiles/lpl_stream_isa.txt), so it does not get step 1's prologue.
template <bool ROBUST>
__global__ __launch_bounds__(E0C_BLOCK) void e0_lpl_h(Dp d, double* hot_out) {
  const int done = d.flags[1];  // requested first, tested after the LDS staging (no global side effects before)
  extern __shared__ double2 hot[];  // [n_hot][HOT_REC_H] records, then acc[12][n_slots], then the tile counter
  const V2& v = d.v2;
  const LplWg g = lpl_wg<true>(v, hot, LPL_CAMREC_H, 0);
  {
    // staging: slot -> camera rank -> record, two dependent L2 round trips; every thread first requests all its
    // ranks, then all its record pieces, then writes LDS (a plain loop pays the two latencies once per pass)
    constexpr int PASSES = (HOT_ACC_MAX * HOT_REC_H + E0C_BLOCK - 1) / E0C_BLOCK;
    int rk[PASSES];
    double2 piece[PASSES];
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      const int i = threadIdx.x + u * E0C_BLOCK;
      rk[u] = i < g.n_hot * HOT_REC_H ? v.wg_cams[g.cam0 + i / HOT_REC_H] : 0;
    }
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      const int i = threadIdx.x + u * E0C_BLOCK;
      piece[u] = lpl_img(d, rk[u])[i % HOT_REC_H];
    }
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      const int i = threadIdx.x + u * E0C_BLOCK;
      if (i < g.n_hot * HOT_REC_H) hot[(i / HOT_REC_H) * LPL_CAMREC_H + i % HOT_REC_H] = piece[u];
    }
  }
  __syncthreads();
  if (done) return;
  const int lane = threadIdx.x & 63;
  const LplTiles T(v, g.ctr, lane);
  const int t_end = T.t_end;
  int c_t = T.grab(), c_row0 = 0, c_k = 0, c_nh = 0, c_fl = 0;
  if (c_t < t_end) T.info(c_t, c_row0, c_k, c_nh, c_fl);
  LplStream2<ROBUST> rows;
  rows.start(T, v, c_t, c_row0, c_k, c_t < t_end ? T.grab() : t_end);
  // landmark record of the lane: X (4), Jl column scale s (4), Hll^-1 (6) = 14 entries of lmrec[tile][14][64];
  // the Householder vector of X (tangent basis N_l, landmark_block.hpp:227-269) is rebuilt once per tile
  auto load_rec = [&](int t, double4& X, double4& s4, double (&Hi)[6]) {
    const double* rp = v.lmrec + ((size_t)t * LPL_REC_H) * WAVE + lane;
    X = make_double4(rp[0], rp[WAVE], rp[2 * WAVE], rp[3 * WAVE]);
    s4 = make_double4(rp[4 * WAVE], rp[5 * WAVE], rp[6 * WAVE], rp[7 * WAVE]);
#pragma unroll
    for (int m = 0; m < 6; ++m) Hi[m] = rp[(8 + m) * WAVE];
  };
  double4 X = make_double4(0, 0, 0, 1), s4 = make_double4(1, 1, 1, 1);
  double Hi[6] = {0, 0, 0, 0, 0, 0};
  if (c_t < t_end) load_rec(c_t, X, s4, Hi);
  while (c_t < t_end) {
    double hw[4], hbeta;
    house4(X, hw, hbeta);
    double red[3] = {0, 0, 0};
    for (int j = 0; j < c_k; ++j) {
      const LplRow cur = rows.next(T, v);
      // LDS pointer or global pointer, never a select of the two (lpl_read12).  Rows [0, c_nh) have an LDS-resident
      // camera in every lane: wave-uniform branch, LDS reads only.
      auto fwd = [&](const Cam& P, const double4 (&zz)[3]) {
        const double sw = ROBUST ? sqrt(cur.w) : 1.0;
        const Hom h = hom_project(P, X, cur.uv.x, cur.uv.y);
        double jl4[8], jl3[6], t[2];
        hom_jl4(P, h, sw, s4, jl4);
        jl3_of_jl4(jl4, hw, hbeta, jl3);
        hom_jp_x(h, X, sw, zz, t);
#pragma unroll
        for (int m = 0; m < 3; ++m) red[m] += jl3[m] * t[0] + jl3[3 + m] * t[1];
      };
      Cam P;
      double4 zz[3];
      if (j < c_nh) {
        const double2* hp = hot + lpl_cw_slot(cur.cw) * LPL_CAMREC_H;
        lpl_read12(hp, zz);
        lpl_read_cam(hp + 6, P);
        fwd(P, zz);
      } else if (cur.cw != -1) {
        if (cur.cw >= 0) {
          const double2* hp = hot + lpl_cw_slot(cur.cw) * LPL_CAMREC_H;
          lpl_read12(hp, zz);
          lpl_read_cam(hp + 6, P);
        } else {
          const double2* hp = lpl_img(d, -2 - cur.cw);
          lpl_read12(hp, zz);
          lpl_read_cam(hp + 6, P);
        }
        fwd(P, zz);
      }
    }
    if (c_fl & 1) {  // landmarks dealt over several lanes: sum their partial u = Jl^T t (segmented wavefront scan)
      const int sg = v.seg[(size_t)c_t * WAVE + lane];
      seg_reduce_steps<3>(red, lane, sg & 255, (sg >> 8) & 255, 4);
    }
    const double gv[3] = {Hi[0] * red[0] + Hi[1] * red[1] + Hi[2] * red[2], Hi[1] * red[0] + Hi[3] * red[1] + Hi[4] * red[2],
                          Hi[2] * red[0] + Hi[4] * red[1] + Hi[5] * red[2]};
    // the next tile's record (Hll^-1 is dead by now; X and s are still needed: second set)
    const int n_t = rows.nx_t;
    double4 nX = make_double4(0, 0, 0, 1), ns4 = make_double4(1, 1, 1, 1);
    double nHi[6] = {0, 0, 0, 0, 0, 0};
    if (n_t < t_end) load_rec(n_t, nX, ns4, nHi);
    for (int jj = 0; jj < c_k; ++jj) {
      const int j = c_k - 1 - jj;
      const LplRow cur = rows.next(T, v);
      auto bwd = [&](const Cam& P) -> double4 {
        const double sw = ROBUST ? sqrt(cur.w) : 1.0;
        const Hom h = hom_project(P, X, cur.uv.x, cur.uv.y);
        double jl4[8], jl3[6];
        hom_jl4(P, h, sw, s4, jl4);
        jl3_of_jl4(jl4, hw, hbeta, jl3);
        const double s0 = jl3[0] * gv[0] + jl3[1] * gv[1] + jl3[2] * gv[2];
        const double s1 = jl3[3] * gv[0] + jl3[4] * gv[1] + jl3[5] * gv[2];
        return hom_q(h, sw, s0, s1);
      };
      Cam P;
      if (j < c_nh) {  // wave-uniform: LDS only
        lpl_read_cam(hot + lpl_cw_slot(cur.cw) * LPL_CAMREC_H + 6, P);
        lpl_scatter(g, cur.cw, X, bwd(P));
      } else if (cur.cw >= 0) {
        lpl_read_cam(hot + lpl_cw_slot(cur.cw) * LPL_CAMREC_H + 6, P);
        lpl_scatter(g, cur.cw, X, bwd(P));
      } else if (cur.cw < -1) {
        const int cold_at = lpl_cold_at(d, c_fl, c_nh, c_row0, j, lane);
        lpl_read_cam(lpl_img(d, -2 - cur.cw) + 6, P);
        d.q4c[cold_at] = bwd(P);
      }
    }
    c_t = n_t;
    if (c_t < t_end) {
      T.info(c_t, c_row0, c_k, c_nh, c_fl);
      rows.ahead(T.grab());
    }
    X = nX;
    s4 = ns4;
#pragma unroll
    for (int m = 0; m < 6; ++m) Hi[m] = nHi[m];
  }
  __syncthreads();
  int frec[LPL_FLUSH_PASSES];
  lpl_flush_request(g, v, frec);
  lpl_flush_store(g, frec, hot_out);
  if (d.p2p_epoch && blockIdx.x == 0 && threadIdx.x == 0) *d.p2p_epoch += 1;  // one tick per term, read by the next kernels
}
static_assert(lpl_lds_bytes(3) == 3 * HOT_REC * sizeof(double2) + (3 + 3 * 3) * 96 + 16, "e0_lpl: records, accumulators, counter");
static_assert(lpl_lds_bytes_h(3) == 3 * LPL_CAMREC_H * sizeof(double2) + (3 + 3 * 3) * 96 + 16 && HOT_REC_H <= LPL_CAMREC_H,
              "e0_lpl_h: records, accumulators, counter");

}  // namespace povar
