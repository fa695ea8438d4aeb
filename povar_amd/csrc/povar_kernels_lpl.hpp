// povar_kernels_lpl.hpp -- what the eight lane-per-landmark kernels share: e0_lpl, prepare_lpl, backsub_lpl, lpl_pass
// (povar_kernels.hpp) and their step-2 twins *_h (povar_kernels_joint.hpp).  Pieces, not a walker: every kernel keeps its own
// `while (c_t < t_end)` loop, its row loops, its LDS-or-global branches and its arithmetic.  Here are
//   LplTiles      the workgroup's tile range, its on-demand counter and the tile table
//   LplStream2    the row stream of the two-pass kernels (e0 / prepare / backsub): rows requested three ahead of the consumer
//   LplStream1    the same for the single forward walk of lpl_pass[_h]
//   lpl_acc_sum   one pair of a camera's accumulators at the flush (hub replicas summed)
//   lpl_read12 / lpl_read_cam   twelve consecutive doubles of a camera record
// Included by povar_kernels.hpp (it needs V2, Cam and WAVE from there), never on its own.  Every member function is
// __forceinline__ and every member a value: the cursors are wave-uniform and have to stay in SGPRs, the row queue in VGPRs
// without a copy through memory.
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

}  // namespace povar
