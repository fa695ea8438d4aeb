// povar_kernels_ck_det.hpp -- the BIT-REPRODUCIBLE forms of the camera-chunk E0 operators (POVAR_DETERMINISTIC=1; SURVEY.md 8(e):
// a fixed reduction order inside a GPU): e0_ck_det, step 1 -- right_mul_e0_pOSE (linearization_power_varproj.hpp:364-406) -- and
// e0_ck_h_det, step 2 -- right_mul_e0_poBA (:408-453) --, on the layouts and with the row / record helpers of e0_ck and e0_ck_h
// (povar_kernels_ck.hpp, povar_kernels_ck_joint.hpp, ck_layout.hpp).  ONE body (ckd_term) holds the protocol; the two steps
// (CkdPose, CkdJoint) say what a landmark's sum is made of and how an observation contributes to it.
//
// e0_ck adds in arrival order in two places: three ds_add_f64 per observation into the landmark's u = Jl^T Jp x (e0_ck_h: four,
// into the ambient U4), and twelve per (camera, tile) into the workgroup's accumulator of y_c -- the GPU's form of the
// reference's mutex order (:388-398).  Here neither sum depends on the order the wavefronts arrive in:
//   * u_l is summed in 64-bit FIXED POINT (ds_add_u64: integer addition is associative, every bit of the sum is the same
//     whatever the order).  The binary point of a landmark's sum comes from the data: the way forward is walked TWICE --
//     the first walk leaves the largest exponent of the landmark's contributions (ds_max_i32: order-free as well), the
//     second adds the contributions rounded once to the grid 2^(61 - that exponent - ceil(log2 n_l)) (n_l from the layout):
//     at least 61 - log2 n_l bits below the largest contribution, where fp64 keeps 53 below the running sum.
//     (A-priori bounds were built first -- exponents of max|z|, max|P3|, the image coordinates, |h~| --: the operator norm
//     of the pOSE residual's C(u, v) with pixel coordinates alone is 2^17 above what occurs; the sums kept 25 bits.)
//   * y_c: a chunk's sum is a register sum in row order and a segmented wavefront scan -- fixed already --; the run totals
//     are added into the camera's LDS accumulator in a FIXED ORDER: every (tile, run) has a ticket (CkP::tick, from the
//     layout: batches, then rounds of the tile walk, then the tiles of a round from the shortest to the tallest -- the
//     order they finish in), the accumulator slot carries a counter in LDS, and a run's last lane adds (read, fp64 add,
//     write -- no atomic) when the counter shows its ticket.  A wavefront waits only for tiles that are ahead of its own in
//     every wavefront's program order: no cycle.
// Everything else of the term (cam_cold_sum_binv, povar_kernels_cam.hpp: strided sums + a butterfly) has a fixed order anyway.
#pragma once

#include "povar_kernels_ck.hpp"
#include "povar_kernels_ck_joint.hpp"

namespace povar {

constexpr int CK_FIX_BITS = 61;
// |v| < 2^ck_xp(v) for v > 0; an exact ZERO contributes no exponent (INT_MIN: a no-op for the maximum) -- frexp's 0 for it
// would set the binary point of a landmark whose real contributions are tiny (late terms: 2^-40) forty bits too high and
// leave the sum ~ 20 bits; inf / nan: 0 (the sum is garbage either way and the finiteness test downstream says so)
__device__ inline int ck_xp(double v) { return v > 0.0 ? __builtin_amdgcn_frexp_exp(v) : (v == 0.0 ? INT_MIN : 0); }
__device__ inline unsigned long long ck_fix(double x, int e) {  // x 2^e to the nearest integer, two's complement (|x 2^e| < 2^62)
  const double xs = __builtin_ldexp(x, e) + 0.5;
  const double hi = __builtin_floor(xs * 0x1p-32);
  const double lo = __builtin_fma(hi, -0x1p32, xs);  // in [0, 2^32]
  const int ih = (int)hi;
  const unsigned il = (unsigned)lo;  // (v_cvt_u32_f64 truncates and saturates: any fixed function of x will do)
  return ((unsigned long long)(unsigned)ih << 32) | il;
}
__device__ inline double ck_unfix(unsigned long long v, int e) {
  const int ih = (int)(unsigned)(v >> 32);
  const unsigned il = (unsigned)v;
  return __builtin_ldexp(__builtin_fma((double)ih, 0x1p32, (double)il), -e);
}

// ---- the two steps.  A step's LDS holds, from ck_lds + 2: the landmarks' coordinates and their sums (NC components each, for
// slots(k) landmark slots), the accumulators [max_acc][13], then a 16-bit binary point per landmark slot and a 16-bit ticket
// counter per accumulator.  A row's 16-bit slot word s addresses the components (at) and the binary point (slot_of).

// step 1: u = Jl^T Jp x, three components slot-major (s = 3 x slot: e0_ck's arrays); the record is z (12) and P3 | t (9 + 3)
struct CkdPose {
  static constexpr int NC = 3, REC = 9, NG = 6;  // components of a sum; doubles per landmark lane in V2::lmrec; those after the coordinates (G)
  template <int D, bool ROBUST> using Stream = CkStream<D, ROBUST>;
  struct Cam { double zz[12], P3[12]; };
  typedef double2 Obs;  // what a row holds per observation: the image point
  __host__ __device__ static inline int slots(int k_slots) { return k_slots; }
  __device__ static inline int word(int slot) { return 3 * slot; }
  __device__ static inline uint32_t slot_of(uint32_t s) { return (s * 43691u) >> 17; }  // (s / 3 for s < 2^16)
  __device__ static inline int at(int s, int m) { return s + m; }
  template <int D, bool ROBUST> __device__ static inline Obs obs(const Stream<D, ROBUST>& st, int i) { return st.uv[i]; }
  template <bool ROBUST> __device__ static inline void load_cam(const Dp& d, int rank, Cam& c) {
    ck_load_z(d, rank, c.zz);
    ck_load_p<ROBUST>(d, rank, c.P3);
  }
  template <bool ROBUST> __device__ static inline void load_cam_back(const Dp& d, int rank, Cam& c) { ck_load_p<ROBUST>(d, rank, c.P3); }
  template <bool ROBUST>
  __device__ static inline void contribution(const Dp& d, const Cam& c, Obs uv, const double* lh, uint32_t s, double (&v)[NC]) {
    const double hx = lh[s], hy = lh[s + 1], hz = lh[s + 2];
    const double rw = ROBUST ? ck_huber_w(d, c.P3, hx, hy, hz, uv) : 1.0;
    LplObs o;
    o.set(d, uv, rw);
    ck_forward_math(o, c.zz, c.P3, hx, hy, hz, v);
  }
  // g = G u (over u)
  __device__ static inline void landmark_step(double*, double* lu, int s, const double (&u)[NC], const double (&g)[NG]) {
    lu[s] = g[0] * u[0] + g[1] * u[1] + g[2] * u[2];
    lu[s + 1] = g[1] * u[0] + g[3] * u[1] + g[4] * u[2];
    lu[s + 2] = g[2] * u[0] + g[4] * u[1] + g[5] * u[2];
  }
  template <int D, bool ROBUST>
  __device__ static inline void backward_rows(const Dp& d, const CkRows& R, Stream<D, ROBUST>& st, int row0, int li0, int h, int lane,
                                              const Cam& c, const double* lh, const double* lg, int S, double (&y)[12]) {
    ck_backward_rows<D, ROBUST>(d, R, st, row0, li0, h, lane, c.P3, lh, lg, S, y);
  }
};

// step 2: the ambient U4, four components component-major with e0_ck_h's compile-time stride; the record is z and P (3 x 4 each)
struct CkdJoint {
  static constexpr int NC = 4, REC = CKH_REC, NG = 10;  // (after X: s (4), Hll^-1 (6))
  template <int D, bool ROBUST> using Stream = CkStreamH<D, ROBUST>;
  struct Cam { double4 zz[3]; povar::Cam P; };
  typedef double Obs;  // the robust weight
  __host__ __device__ static inline int slots(int) { return CKH_STRIDE; }
  __device__ static inline int word(int slot) { return slot; }
  __device__ static inline uint32_t slot_of(uint32_t s) { return s; }
  __device__ static inline int at(int s, int m) { return m * CKH_STRIDE + s; }
  template <int D, bool ROBUST> __device__ static inline Obs obs(const Stream<D, ROBUST>& st, int i) { return ROBUST ? st.rw[i] : 1.0; }
  template <bool ROBUST> __device__ static inline void load_cam(const Dp& d, int rank, Cam& c) { ckh_load_rec(d, rank, c.zz, c.P); }
  template <bool ROBUST> __device__ static inline void load_cam_back(const Dp& d, int rank, Cam& c) { ckh_load_cam(d, rank, c.P); }
  // J4^T t, t = sw D (Z X): what e0_ck_h adds (ckh_forward_math)
  template <bool ROBUST>
  __device__ static inline void contribution(const Dp&, const Cam& c, Obs rw, const double* lx, uint32_t s, double (&v)[NC]) {
    ckh_forward_math<ROBUST>(c.P, c.zz, rw, lx, s, [&](int m, double x) { v[m] = x; });
  }
  // U4 -> G4 (ckh_landmark_step reads U4 where the sums were)
  __device__ static inline void landmark_step(double* lx, double* lu, int s, const double (&u)[NC], const double (&rec)[NG]) {
#pragma unroll
    for (int e = 0; e < NC; ++e) lu[e * CKH_STRIDE + s] = u[e];
    ckh_landmark_step(lx, lu, s, rec);
  }
  template <int D, bool ROBUST>
  __device__ static inline void backward_rows(const Dp&, const CkRows& R, Stream<D, ROBUST>& st, int row0, int li0, int h, int lane,
                                              const Cam& c, const double* lx, const double* lg, int, double (&y)[12]) {
    ckh_backward_rows<D, ROBUST>(R, st, row0, li0, h, lane, c.P, lx, lg, y);
  }
};

// LDS bytes: the arrays of e0_ck (one group) / e0_ck_h + a 16-bit binary point per landmark slot + a 16-bit ticket counter per
// accumulator slot
template <class Step>
__host__ __device__ inline size_t ckd_lds_bytes(int k_slots, int n_acc) {
  const size_t slots = (size_t)Step::slots(k_slots);
  return 16 + slots * (2 * Step::NC * 8) + (size_t)n_acc * CK_ACC_STRIDE * 8 + 64 + 2 * (slots + n_acc) + 16;
}
__host__ __device__ inline size_t ck_lds_bytes_det(int slots, int n_acc) { return ckd_lds_bytes<CkdPose>(slots, n_acc); }
__host__ __device__ inline size_t ckh_lds_bytes_det(int n_acc) { return ckd_lds_bytes<CkdJoint>(0, n_acc); }

// the rows of one tile on the way forward.  PASS 0: the largest exponent of the contributions to the landmark (in the first word
// of its sum); PASS 1: the contributions in fixed point
template <class Step, int D, bool ROBUST, int PASS>
__device__ inline void ckd_forward_rows(const Dp& d, const CkRows& R, typename Step::template Stream<D, ROBUST>& st, int row0, int li0, int h,
                                        int lane, const typename Step::Cam& c, const double* lx, double* lu, const short* lexp) {
  ck_walk_rows<D, 1>(h, [&](int j, int i) {
    const typename Step::Obs o = Step::template obs<D, ROBUST>(st, i);
    const uint32_t s = ck_slot(st.w[i], j);
    st.load(R, row0, li0, j + D, h, lane, i);
    if (s != CK_NONE) {
      double v[Step::NC];
      Step::template contribution<ROBUST>(d, c, o, lx, s, v);
      if (PASS == 0) {
        double a = fabs(v[0]);
#pragma unroll
        for (int m = 1; m < Step::NC; ++m) a = fmax(a, fabs(v[m]));
        __hip_atomic_fetch_max(reinterpret_cast<int*>(lu + s), ck_xp(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
        const int e = lexp[Step::slot_of(s)];
#pragma unroll
        for (int m = 0; m < Step::NC; ++m)
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(lu + Step::at(s, m)), ck_fix(v[m], e), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  });
}

// NW wavefronts per workgroup (the count the layout's tiles were scheduled for and its tickets numbered for), SD rows in flight
template <class Step, int NW, int SD, bool ROBUST>
__device__ inline void ckd_term(const Dp& d, const CkP& k, double* part_out) {
  constexpr int NC = Step::NC;
  const int done = d.flags[1];
  extern __shared__ double ck_lds[];
  const CkRows R = ck_rows(k);
  const int S = Step::slots(k.slots);
  const int lane0 = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double* lx = ck_lds + 2;      // [S][NC] landmark coordinates of the batch (step 2: [NC][S])
  double* lu = lx + NC * S;     // the same shape: the sums (first the exponent maximum, then fixed point), then what the way back reads
  double* acc = lu + NC * S;    // [n_acc][13] per-camera accumulators of the workgroup
  short* lexp = reinterpret_cast<short*>(acc + (size_t)k.max_acc * CK_ACC_STRIDE);  // [S] binary point of the sum per slot
  short* tick = lexp + S;                                                          // [n_acc] tickets served per accumulator
  const V2& v = d.v2;
  const int cam0 = v.wg_cam_off[blockIdx.x];
  const int n_acc = v.wg_cam_off[blockIdx.x + 1] - cam0;
  const int t0 = __builtin_amdgcn_readfirstlane(v.wg_tile_off[blockIdx.x]);
  const int t1 = __builtin_amdgcn_readfirstlane(v.wg_tile_off[blockIdx.x + 1]);
  for (int i = threadIdx.x; i < n_acc * CK_ACC_STRIDE; i += NW * 64) acc[i] = 0;
  for (int i = threadIdx.x; i < n_acc; i += NW * 64) tick[i] = 0;
  typedef const int __attribute__((address_space(4))) * cint_p;
  const cint_p tiles = (cint_p)(uintptr_t)k.tile;
  const cint_p bt = (cint_p)(uintptr_t)k.bt_off;
  if (done) return;  // wave-uniform, before any barrier and any side effect
  auto tile_of = [&](int tb0, int q) { return tb0 + q * NW + ((q & 1) ? NW - 1 - wave : wave); };  // (e0_ck's walk without its deal over the SIMDs: the layout's ticket order is cut for this one)
  for (int b = 0; b < k.nb; ++b) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));  // (per-lane addresses are not carried across the batches: povar_kernels_ck.hpp)
    const int tb0 = bt[blockIdx.x * k.nb + b], tb1 = bt[blockIdx.x * k.nb + b + 1];
    const bool one_tile = tile_of(tb0, 1) >= tb1;  // the wavefront's record stays in registers through the passes
    // ---- landmark coordinates of the batch; the first word of the sum: the exponent maximum of the first walk
    for (int m = wave; t0 + b + k.nb * m < t1; m += NW) {
      const double* rp = v.lmrec + ((size_t)(t0 + b + k.nb * m) * Step::REC) * WAVE + lane;
      const int s = Step::word(m * WAVE + lane);
#pragma unroll
      for (int e = 0; e < NC; ++e) {
        lx[Step::at(s, e)] = rp[e * WAVE];
        lu[Step::at(s, e)] = e == 0 ? __longlong_as_double((long long)(unsigned)INT_MIN) : 0.0;
      }
    }
    typename Step::Cam cam = {};
    typename Step::template Stream<SD, ROBUST> st;
    st.clear();
    // first tile of the first walk: in flight across the barrier
    {
      const int t = tile_of(tb0, 0);
      if (t < tb1) {
        const int rank = ck_rank(k.lane_meta[(size_t)t * WAVE + lane].x);
        Step::template load_cam<ROBUST>(d, rank < 0 ? 0 : rank, cam);
        st.template start<1>(R, tiles[4 * t], tiles[4 * t + 3], tiles[4 * t + 1], lane);
      }
    }
    ck_barrier();
    // ---- the way forward, twice
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      for (int q = 0;; ++q) {
        const int t = tile_of(tb0, q);
        if (t >= tb1) break;
        const int row0 = tiles[4 * t], h = tiles[4 * t + 1], li0 = tiles[4 * t + 3];
        if (q > 0 || (pass > 0 && !one_tile)) {
          const int rank = ck_rank(k.lane_meta[(size_t)t * WAVE + lane].x);
          Step::template load_cam<ROBUST>(d, rank < 0 ? 0 : rank, cam);
        }
        if (q > 0 || pass > 0) st.template start<1>(R, row0, li0, h, lane);
        if (pass == 0) ckd_forward_rows<Step, SD, ROBUST, 0>(d, R, st, row0, li0, h, lane, cam, lx, lu, lexp);
        else ckd_forward_rows<Step, SD, ROBUST, 1>(d, R, st, row0, li0, h, lane, cam, lx, lu, lexp);
      }
      if (pass == 0) {
        ck_barrier();
        // the binary point of every landmark's sum: 61 bits - the largest contribution's exponent - ceil(log2(their number))
        for (int m = wave; t0 + b + k.nb * m < t1; m += NW) {
          const int slot = m * WAVE + lane, s = Step::word(slot);
          const int e = (int)(unsigned)__double_as_longlong(lu[s]);
          const int lc = k.lcnt[(size_t)(t0 + b + k.nb * m) * WAVE + lane];
          lexp[slot] = (short)((e == INT_MIN || lc == 255) ? 0 : CK_FIX_BITS - (e + lc));
          lu[s] = 0;
        }
      }
      ck_barrier();
    }
    // ---- per landmark slot: the sum back from fixed point, then the step's landmark operator (over the sum)
    for (int m = wave; t0 + b + k.nb * m < t1; m += NW) {
      const double* rp = v.lmrec + ((size_t)(t0 + b + k.nb * m) * Step::REC + NC) * WAVE + lane;
      double rec[Step::NG];
#pragma unroll
      for (int e = 0; e < Step::NG; ++e) rec[e] = rp[e * WAVE];
      const int slot = m * WAVE + lane, s = Step::word(slot);
      const int ex = lexp[slot];
      double u[NC];
#pragma unroll
      for (int e = 0; e < NC; ++e) u[e] = ck_unfix(__double_as_longlong(lu[Step::at(s, e)]), ex);
      Step::landmark_step(lx, lu, s, u, rec);
    }
    // first tile of the way back: the record (if it has gone), metadata and rows in flight across the barrier
    asm volatile("" : "+v"(lane));
    ck_barrier();
    // ---- the way back: the wavefront's tiles in the order of the walk; run totals into the accumulators in ticket order
    for (int q = 0;; ++q) {
      const int t = tile_of(tb0, q);
      if (t >= tb1) break;
      const int row0 = tiles[4 * t], h = tiles[4 * t + 1], fl = tiles[4 * t + 2], li0 = tiles[4 * t + 3];
      const int2 me = k.lane_meta[(size_t)t * WAVE + lane];
      const int rank = ck_rank(me.x), seg = ck_seg(me.x), acc_slot = me.y;
      const int my_ticket = k.tick[(size_t)t * WAVE + lane];
      if (q > 0 || !one_tile) Step::template load_cam_back<ROBUST>(d, rank < 0 ? 0 : rank, cam);
      st.template start<-1>(R, row0, li0, h, lane);
      double y[12];
#pragma unroll
      for (int m = 0; m < 12; ++m) y[m] = 0;
      Step::template backward_rows<SD, ROBUST>(d, R, st, row0, li0, h, lane, cam, lx, lu, S, y);
      if (fl & 1) seg_scan_steps<12>(y, lane, seg & 255, 4);  // (inclusive scan: the run's total is in its LAST lane)
      bool pending = false;
      if (rank >= 0) {
        if (acc_slot >= 0) {
          pending = lane == ((seg >> 8) & 255);
        } else {  // a chunk with a partial record of its own (plain stores: one writer per record, no order to keep)
          double2* o = reinterpret_cast<double2*>(part_out + (size_t)(~acc_slot) * 12);
#pragma unroll
          for (int m = 0; m < 6; ++m) o[m] = make_double2(y[2 * m], y[2 * m + 1]);
        }
      }
      const int a_slot = pending ? acc_slot : 0;
      int spins = 0;
      while (__builtin_amdgcn_ballot_w64(pending) != 0) {
        // (every spin is bounded: a layout whose tickets do not match this walk -- which the host never builds -- must end
        // in a reported failure, flags[0] bit 3, not in a hung device)
        const bool give_up = ++spins > (1 << 20);
        if (pending && (give_up || __hip_atomic_load(tick + a_slot, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == (short)my_ticket)) {
          double* a = acc + a_slot * CK_ACC_STRIDE;
#pragma unroll
          for (int m = 0; m < 12; ++m) a[m] += y[m];
          __hip_atomic_store(tick + a_slot, (short)(my_ticket + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (give_up) atomicOr(&d.flags[0], 8);
          pending = false;
        } else if (pending) {
          __builtin_amdgcn_s_sleep(1);
        }
      }
    }
    ck_barrier();  // the next batch overwrites the coordinates and the sums; after the last one: the accumulators are complete
  }
  // ---- accumulators -> this workgroup's partial records (camera-major in part_out)
  for (int i = threadIdx.x; i < n_acc * 6; i += NW * 64) {
    const int r = i / 6, m = 2 * (i % 6);
    const int rec = k.slot_rec[cam0 + r];
    reinterpret_cast<double2*>(part_out + (size_t)rec * 12)[i % 6] = make_double2(acc[r * CK_ACC_STRIDE + m], acc[r * CK_ACC_STRIDE + m + 1]);
  }
}

template <int NW, int SD, bool ROBUST>
__global__ __launch_bounds__(NW * 64) void e0_ck_det(Dp d, CkP k, double* part_out) {
  ckd_term<CkdPose, NW, SD, ROBUST>(d, k, part_out);
}
template <int NW, int SD, bool ROBUST>
__global__ __launch_bounds__(NW * 64) void e0_ck_h_det(Dp d, CkP k, double* part_out) {
  ckd_term<CkdJoint, NW, SD, ROBUST>(d, k, part_out);
}

}  // namespace povar
