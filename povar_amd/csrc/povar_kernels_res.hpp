// povar_kernels_res.hpp -- gfx950 device code of the RESIDENT power series: the whole loop of solve_pOSE
// (linearization_power_varproj.hpp:191-237: x_0 = B^-1 (-b); x_i = B^-1 E0 x_{i-1}; sum, early exit) in ONE launch, for
// contexts whose term-invariant operands fit on the chip (res_layout.hpp): series_res; and series_res_h, the same for the
// loop of solve_joint (:240-287: x_i = B^-1 N_c^T sigma E0 sigma N_c x_{i-1}; step 2, RIPOBA).  ONE body, two steps:
// res_series holds the structure -- phase order, barriers B1-B7, hand-overs, bounded spins, give-up bit, norm sweep, the reuse
// of the region --, and ResPose / ResJoint say what a landmark slot, a lane and an owned camera hold and compute; the two
// kernels are wrappers.  What follows describes the body in step 1's terms; ResJoint's comment says what step 2 puts in
// their place.
//
// The per-term kernels re-read per term what does not change between the terms of a solve: rows, landmark records, tile
// metadata, B^-1 -- and pay a launch ramp, a flush and two kernel boundaries each time (29 us per term on a venice-1778
// shard of one rank in eight, where the rows cost 7; profiles/r04_shard_term_times.txt).  Here
//   * a LANE keeps its chunks of <= H observations of one camera each (uv, landmark slot, robust weight) and that camera's
//     P3 = P_c[:, :3] in REGISTERS for the whole solve;
//   * the workgroup's LANDMARKS live in LDS (h~ 24 bytes, u / g 24 bytes; G = diag(s) Hll^-1 diag(s) in the registers of
//     the lane that owns the slot);
//   * every camera has an OWNER workgroup that holds B_c^-1, sigma_c, the running sum and the last term in LDS.
// Per term only z = sigma x and the per-camera partial sums move (right_mul_e0_pOSE :364-406 + right_mul_b_inv_pOSE
// :322-340), through ONE region of LDS that is in turn
//   1. the z of the workgroup's cameras (gathered from the z table by all threads, one 16-byte granule pair each),
//   2. their accumulators: forward u_l += P3^T (w C (Z h~)) (LDS atomics on the landmark), g = G u, backward
//      y_c += h~ (x) (w C (P3 g)) (registers, one segmented wavefront sum, one LDS add per run of lanes),
//   3. after the accumulators have gone out as the workgroup's partial records (contiguous: a coalesced copy): the
//      records the workgroup reads as an OWNER -- all threads again, a granule pair each --, which it sums camera by
//      camera in a fixed order, applies B_c^-1 to, adds to the sum and publishes as the next z_c.
// The reference's mutex-guarded `res += Jp^T s` (:388-398) is the LDS accumulation + the owner's fixed-order sum.
// (A first version gave every lane its camera's z and its partial record to itself: twelve 16-byte accesses per chunk
// and hand-over, each wavefront instruction touching 64 lines -- the address pipes of the CUs, not a latency, set the
// term at 12 us on ladybug-49 and 44 us on a venice shard; profiles/r05_res_experiments.txt.)
//
// Hand-overs (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility", R2: "the data IS the
// flag"): every handed-over double travels as TWO 8-byte granules {32 bits of the value, tag} written by one 16-byte
// agent-scope (sc1: write-through, L1-bypassing) store; tag = launch number << 8 | term, so a granule of an earlier term or
// an earlier launch never matches.  The reader re-reads its granules (16-byte sc1 loads) until every tag is the one it
// waits for: no flag word, no fence, no drain of the producer's stores, no dependence on dispatch order or placement; a
// granule is written by ONE store and is never torn.  What may be overwritten when:
//   * z_c of term i replaces z_c of term i - 1 after the owner has seen ALL records of c of term i, i.e. after every
//     workgroup that reads z_c has used it;
//   * workgroup w's record of camera c of term i + 1 replaces that of term i after w has seen z_c of term i, which the
//     owner publishes after it has read the record.
//   * the norm granules of a workgroup (early-exit tests only) are DOUBLE-BUFFERED by the parity of the term their tag
//     names: workgroup g publishes the norms tagged i + 1 once it has z tag i and the records of its cameras -- which does not
//     wait for a workgroup s that contributes to none of g's cameras and may still be sweeping the norms tagged i.  With one
//     buffer s would find tag i + 1 in g's slot, never match and spin out (the resident path lost, silently: ADVICE r05).
//     With two, g cannot write tag i + 2 into the half of tag i before it has passed its own sweep of the norms tagged
//     i + 1, which needs s's granule tagged i + 1, which s publishes only after its sweep of tag i.
// Every spin is bounded (ResP::spin_limit): a launch whose workgroups are not all resident (another context's kernels on
// the device) gives up, raises bit 2 of flags[0] and the library repeats the solve with the per-term kernels.
#pragma once

#include "povar_kernels_ck.hpp"
#include "povar_kernels_ck_joint.hpp"
#include "res_layout.hpp"

namespace povar {

struct ResP {
  const int* lane_cam;    // [W][R][T] camera slot of the chunk
  const int* lane_seg;
  const double2* uv;      // [W][R][H][T]
  const int* lslot;
  const int* oslot;
  const int* wave_h;      // [W][R][NW]
  const int* lm_off;      // [W + 1]
  const int* lm_id;
  const int* cam_off;     // [W + 1] camera slots = partial records of the workgroup
  const int* cam_id;
  const int* cam_zi;
  const int* own_off;     // [W + 1]
  const int* own_cam;
  const int* own_zi;
  const int2* own_q;
  const int* oq_off;      // [W + 1]
  const int* oq_rec;
  uint4* part;            // [n_rec][12] partial records, workgroup-major, one 16-byte granule pair per entry
  uint4* zbuf;            // [n_cams][12] z = sigma x of the current term, rows in popularity order
  uint4* nrm;             // [2][RES_MAX_WG][2] squared norms of (term, sum) over the cameras a workgroup owns, by term parity
  unsigned* launch;       // launch counter (the high bits of the tags)
  unsigned part_bytes, z_bytes, nrm_bytes;
  int W, m, want_norms, want_norm0;
  int w_mode;             // robust weight of an observation: 1: V2::w through V2::of_slot, 2: Dp::sw squared
  double q_tol, r_tol;
  unsigned spin_limit;
};

typedef unsigned __attribute__((ext_vector_type(4))) res_u4;
struct ResBufs {
  __amdgpu_buffer_rsrc_t part, z, nrm;
};
__device__ inline ResBufs res_bufs(const ResP& k) {
  ResBufs B;
  B.part = __builtin_amdgcn_make_buffer_rsrc(k.part, 0, k.part_bytes, 0x00020000);
  B.z = __builtin_amdgcn_make_buffer_rsrc(k.zbuf, 0, k.z_bytes, 0x00020000);
  B.nrm = __builtin_amdgcn_make_buffer_rsrc(k.nrm, 0, k.nrm_bytes, 0x00020000);
  return B;
}
constexpr int RES_SC1 = 16;  // aux bits of the buffer instructions: sc1 (agent scope)
// byte offset of norm granule pair e (0: term, 1: sum) of workgroup w in the half of the tag's parity
__device__ inline unsigned res_nrm_off(unsigned tag, int w, int e) { return ((tag & 1u) * (unsigned)(2 * RES_MAX_WG) + (unsigned)(2 * w + e)) * 16u; }
// one double as a granule pair {lo, tag, hi, tag}
__device__ inline void res_put(__amdgpu_buffer_rsrc_t r, unsigned byte_off, double v, unsigned tag) {
  res_u4 g;
  g.x = (unsigned)__double2loint(v); g.y = tag; g.z = (unsigned)__double2hiint(v); g.w = tag;
  __builtin_amdgcn_raw_buffer_store_b128(g, r, byte_off, 0, RES_SC1);
}
// N granule pairs (one per byte offset; inactive entries are not loaded), re-read until every tag matches for every lane
// of the wavefront; false: the spin budget ran out
template <int N>
__device__ inline bool res_get(__amdgpu_buffer_rsrc_t r, const unsigned (&off)[N], const bool (&active)[N], unsigned tag, double (&v)[N],
                               unsigned limit) {
  for (unsigned spins = 0;; ++spins) {
    res_u4 g[N];
#pragma unroll
    for (int e = 0; e < N; ++e) g[e] = __builtin_amdgcn_raw_buffer_load_b128(r, active[e] ? off[e] : 0u, 0, RES_SC1);
    bool ok = true;
#pragma unroll
    for (int e = 0; e < N; ++e) ok = ok && (!active[e] || (g[e].y == tag && g[e].w == tag));
    if (__all(ok)) {
#pragma unroll
      for (int e = 0; e < N; ++e) v[e] = __hiloint2double((int)g[e].z, (int)g[e].x);
      return true;
    }
    if (spins >= limit) return false;
    __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");  // (the loads above are re-issued: the compiler must not keep their values)
  }
}

// All threads of the workgroup: granule pair i of a list of n (pair i is entry i % 12 of row row_of(i / 12) of the
// buffer) -> dst[(i / 12) * stride + i % 12], RES_GB pairs per thread in flight (all of a workgroup's in one round trip
// where the registers allow: 1024-thread workgroups have few cameras each)
template <int T, int RES_GB, class RowOf>
__device__ inline bool res_gather(__amdgpu_buffer_rsrc_t r, int n, RowOf row_of, unsigned tag, double* dst, int stride, int t, unsigned limit) {
  bool fine = true;
  for (int i0 = 0; i0 < n; i0 += RES_GB * T) {
    if (i0 + (t & ~63) >= n) break;  // (wave-uniform: nothing left for this wavefront)
    unsigned off[RES_GB];
    bool act[RES_GB];
    double v[RES_GB];
#pragma unroll
    for (int b = 0; b < RES_GB; ++b) {
      const int i = i0 + b * T + t;
      act[b] = i < n;
      off[b] = act[b] ? ((unsigned)row_of(i / 12) * 12u + (unsigned)(i % 12)) * 16u : 0u;
    }
    fine = res_get<RES_GB>(r, off, act, tag, v, limit) && fine;
#pragma unroll
    for (int b = 0; b < RES_GB; ++b) {
      const int i = i0 + b * T + t;
      if (act[b]) dst[(i / 12) * stride + i % 12] = v[b];
    }
  }
  return fine;
}

// ---- the two steps.  ONE body (res_series) holds the protocol; a step (ResPose, ResJoint) says what a landmark slot, a lane's
// chunk and an owned camera hold, and how an observation, a landmark and an owner's term are computed.  The body and the
// steps' members are __forceinline__ and the body takes Dp and ResP by value, as a kernel does: the compiler then sees what
// it saw when each kernel was written out (left to its own inlining order, series_res<8, 4, 2, 2, true> spills one more register
// and the early-exit test is compared twice; profiles/res_unify_isa.txt).  For the same reason the owner's step is ONE member,
// Step::solve, with x, the sum and the z entry in the one exec region each step had: with step 1's z entry in a region of
// its own behind the stores, its load of sigma was one more LDS round trip per term (profiles/res_unify_term_times.txt).

// the owner's arrays in LDS ([nO] records each), carved from a step's sizes: BINV doubles of B^-1, 12 of sigma, NCW of the
// reflector, NX each of the running sum and the last term, 12 of the E0 row of the term (sigma * sum of the camera's records),
// 2 squared norms (last term / sum) and the partial sums of the camera's records (five groups of twelve lanes)
template <class Step>
struct ResOwn {
  static constexpr int DOUBLES = Step::BINV + 12 + Step::NCW + 2 * Step::NX + 12 + 2 + 60;
  double *binv, *sig, *ncw, *acc, *tmp, *y, *nrm, *ps, *end;
  __device__ __forceinline__ ResOwn(double* p, int nO)
      : binv(p), sig(binv + Step::BINV * nO), ncw(sig + 12 * nO), acc(ncw + Step::NCW * nO), tmp(acc + Step::NX * nO),
        y(tmp + Step::NX * nO), nrm(y + 12 * nO), ps(nrm + 2 * nO), end(ps + 60 * nO) {}
};

// the per-lane state of one chunk: what the step keeps of the camera and the rows (Step::Lane), landmark slot word and
// robust weight of each row, camera slot, run of lanes, rows / segmented sum / scan steps of the wavefront
template <class Step, int H>
struct ResChunk {
  typename Step::template Lane<H> s;
  int ls[H];
  double rw[H];
  int ci, seg, hrows, dup, steps;
};

// step 1 (solve_pOSE).  Landmarks: h~ and u / g [nL][3], slot word = 3 x slot, G = diag(s) Hll^-1 diag(s) in the registers
// of the slot's lane.  Lane: image points and P3 = P_c[:, :3].  Owner: B^-1 12 x 12, x = B^-1 y, z = sigma x
struct ResPose {
  static constexpr int NX = 12;                                    // unknowns of a camera
  static constexpr int LM_BYTES = 48, NCO = 3, LMREC = 9, NREG = 6;  // LDS per slot; coordinates, rows of V2::lmrec, registers of a slot
  static constexpr int BINV = 144, NCW = 0;
  typedef ResOwn<ResPose> Own;
  template <int H> struct Lane { double2 uv[H]; double P3[9]; };
  struct Z { double v[12]; };
  __device__ static __forceinline__ int lm_count(int n, int) { return n; }
  __device__ static __forceinline__ int lm_cap(int nL, int) { return nL; }
  template <int STRIDE> __device__ static __forceinline__ int at(int slot, int e) { return 3 * slot + e; }
  __device__ static __forceinline__ int slot_word(int l3, int) { return l3; }
  template <int H> __device__ static __forceinline__ void load_row(const ResP& k, Lane<H>& L, int j, size_t row) { L.uv[j] = k.uv[row]; }
  template <int H> __device__ static __forceinline__ void load_p(const Dp& d, Lane<H>& L, int& ci, int, const int* cam_id) {
#pragma unroll
    for (int e = 0; e < 9; ++e) L.P3[e] = 0;
    if (ci >= 0) {
      const Cam P = load_cam(d.cams_lin4, cam_id[ci]);
      L.P3[0] = P.r0.x; L.P3[1] = P.r0.y; L.P3[2] = P.r0.z;
      L.P3[3] = P.r1.x; L.P3[4] = P.r1.y; L.P3[5] = P.r1.z;
      L.P3[6] = P.r2.x; L.P3[7] = P.r2.y; L.P3[8] = P.r2.z;
    }
  }
  __device__ static __forceinline__ void load_z(const double* zp, Z& zz) {
#pragma unroll
    for (int e = 0; e < 12; ++e) zz.v[e] = zp[e];
  }
  // u_l += P3^T (w C (Z h~_l))
  template <bool ROBUST, int STRIDE, int H>
  __device__ static __forceinline__ void obs_forward(const Dp& d, const Lane<H>& L, int j, double rw, int s, const Z& zz, const double* lh, double* lu) {
    ck_obs_forward(d, L.uv[j], rw, zz.v, L.P3, lh[s], lh[s + 1], lh[s + 2], lu, 0, (uint32_t)s);
  }
  // g = G u
  template <int STRIDE> __device__ static __forceinline__ void landmark_step(double*, double* lu, int s, const double (&G)[NREG]) {
    const double u0 = lu[3 * s], u1 = lu[3 * s + 1], u2 = lu[3 * s + 2];
    lu[3 * s] = G[0] * u0 + G[1] * u1 + G[2] * u2;
    lu[3 * s + 1] = G[1] * u0 + G[3] * u1 + G[4] * u2;
    lu[3 * s + 2] = G[2] * u0 + G[4] * u1 + G[5] * u2;
  }
  // y_c += h~_l (x) (w C (P3 g_l))
  template <bool ROBUST, int STRIDE, int H>
  __device__ static __forceinline__ void obs_backward(const Dp& d, const Lane<H>& L, int j, double rw, int s, const double* lh, const double* lu, double (&y)[12]) {
    const double gg[3] = {lu[s], lu[s + 1], lu[s + 2]};
    ck_obs_backward(d, L.uv[j], rw, L.P3, lh[s], lh[s + 1], lh[s + 2], gg, y);
  }
  // B^-1, sigma and (where the term will be) -b of camera c, by one wavefront
  __device__ static __forceinline__ void load_owner(const Dp& d, const double*, const Own& A, int o, int c, int lane) {
    for (int e = lane; e < 144; e += 64) A.binv[144 * o + e] = d.binv[144 * (size_t)c + e];
    if (lane < 12) A.sig[12 * o + lane] = d.sigma[12 * (size_t)c + lane];
    if (lane >= 32 && lane < 44) A.tmp[12 * o + lane - 32] = -d.b[12 * (size_t)c + lane - 32];
  }
  __device__ static __forceinline__ double binv_row(const Own& A, int o, int lane, const double* v) {
    const double* Bi = A.binv + 144 * o + 12 * lane;
    double s = 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) s += Bi[j] * v[j];
    return s;
  }
  // The owner's step, called by every lane of the wavefront.  s = entry `lane` (< NX; 0 in the other lanes) of x_0 = B^-1 (-b)
  // (FIRST: -b is where the term will be, and stays there) or of x_i = B^-1 y, a = that entry of the sum with it; term and
  // sum stored; entry `lane` (< 12) of z = sigma x handed to put
  template <bool FIRST, class Put>
  __device__ static __forceinline__ void solve(const Own& A, int o, int lane, double& s, double& a, Put put) {
    s = 0; a = 0;
    if (lane < 12) {
      s = binv_row(A, o, lane, (FIRST ? A.tmp : A.y) + 12 * o);
      a = FIRST ? s : A.acc[12 * o + lane] + s;
      if (!FIRST) A.tmp[12 * o + lane] = s;
      A.acc[12 * o + lane] = a;
      put(s * A.sig[12 * o + lane]);
    }
  }
  // sum, last term and its z = sigma x, where the per-term kernels leave them (povar_power_series_step goes on from there)
  template <int NW> __device__ static __forceinline__ void store(const Dp& d, const Own& A, const int* own_cam, int nO, int t, int, int) {
    for (int e = t; e < nO * 12; e += NW * 64) {
      const int c = own_cam[e / 12];
      d.accum[12 * (size_t)c + e % 12] = A.acc[e];
      d.tmp[12 * (size_t)c + e % 12] = A.tmp[e];
      store_z(d, c, e % 12, A.tmp[e] * A.sig[e]);
    }
  }
};

// step 2 (solve_joint), with the operator of e0_ck_h (povar_kernels_ck_joint.hpp) and the owner step of cam_cold_sum_binv_h
// (povar_kernels_cam.hpp).  Landmarks: X and U4 / G4 [4][STRIDE], component-major with the compile-time stride STRIDE = LS T
// (the instantiation's slot capacity), so that ckh_obs_forward, ckh_obs_backward and ckh_landmark_step run unchanged and the
// "ckh" error model of tests/rounding_bounds.py is this kernel's too; the slot's lane keeps s (4) and the upper triangle of
// Hll^-1 (6): entries 4..13 of the 14-double record of V2::lmrec, which both preparation paths write at every prepare.  Lane: the
// camera's whole P_c (3 x 4, from cams_lin4) and no image points: the step-2 operator does not read them.  Owner: z_c is the
// AMBIENT 12-vector sigma (N_c x_c); B^-1 11 x 11 (row stride 11), the reflector (w[12], beta) of N_c, sum and term of 11;
// y11 = N_c^T y (nt_apply), x = B^-1 y11 (binv_row11: the bits of cam_binv_axpy_h), z = sigma (N_c x) (nc_z_entry).  The clamps (landmark
// count, slot word, camera slot) are this step's: it may run on an instance cut for step 1 (res_shared_fits)
struct ResJoint {
  static constexpr int NX = 11;
  static constexpr int LM_BYTES = 64, NCO = 4, LMREC = CKH_REC, NREG = 10;
  static constexpr int BINV = 121, NCW = 13;
  typedef ResOwn<ResJoint> Own;
  template <int H> struct Lane { Cam P; };
  struct Z { double4 v[3]; };
  __device__ static __forceinline__ int lm_count(int n, int cap) { return min(n, cap); }
  __device__ static __forceinline__ int lm_cap(int, int cap) { return cap; }
  template <int STRIDE> __device__ static __forceinline__ int at(int slot, int e) { return e * STRIDE + slot; }
  // (the layout's rows carry 3 x slot: they are step 1's where the two steps share them)
  __device__ static __forceinline__ int slot_word(int l3, int nL) { return l3 < 0 || l3 >= 3 * nL ? -1 : l3 / 3; }
  template <int H> __device__ static __forceinline__ void load_row(const ResP&, Lane<H>&, int, size_t) {}
  template <int H> __device__ static __forceinline__ void load_p(const Dp& d, Lane<H>& L, int& ci, int nC, const int* cam_id) {
    L.P.r0 = L.P.r1 = L.P.r2 = make_double4(0, 0, 0, 0);
    if (ci >= nC) ci = -1;
    if (ci >= 0) L.P = load_cam(d.cams_lin4, cam_id[ci]);
  }
  __device__ static __forceinline__ void load_z(const double* zp, Z& zz) {
    zz.v[0] = make_double4(zp[0], zp[1], zp[2], zp[3]);
    zz.v[1] = make_double4(zp[4], zp[5], zp[6], zp[7]);
    zz.v[2] = make_double4(zp[8], zp[9], zp[10], zp[11]);
  }
  // U4_l += J4^T t, t = sw D (Z X) (four LDS adds per observation)
  template <bool ROBUST, int STRIDE, int H>
  __device__ static __forceinline__ void obs_forward(const Dp&, const Lane<H>& L, int, double rw, int s, const Z& zz, const double* lx, double* lu) {
    ckh_obs_forward<ROBUST, STRIDE>(L.P, zz.v, rw, lx, lu, (uint32_t)s);
  }
  // U4 -> G4
  template <int STRIDE> __device__ static __forceinline__ void landmark_step(double* lx, double* lu, int s, const double (&rec)[NREG]) {
    ckh_landmark_step<STRIDE>(lx, lu, s, rec);
  }
  // y_c += X_l (x) q
  template <bool ROBUST, int STRIDE, int H>
  __device__ static __forceinline__ void obs_backward(const Dp&, const Lane<H>& L, int, double rw, int s, const double* lx, const double* lu, double (&y)[12]) {
    ckh_obs_backward<ROBUST, STRIDE>(L.P, rw, lx, lu, (uint32_t)s, y);
  }
  __device__ static __forceinline__ void load_owner(const Dp& d, const double* ncw, const Own& A, int o, int c, int lane) {
    for (int e = lane; e < 121; e += 64) A.binv[121 * o + e] = d.binv[144 * (size_t)c + e];
    if (lane < 12) A.sig[12 * o + lane] = d.sigma[12 * (size_t)c + lane];
    if (lane >= 16 && lane < 29) A.ncw[13 * o + lane - 16] = ncw[13 * (size_t)c + lane - 16];
    if (lane >= 32 && lane < 43) A.tmp[11 * o + lane - 32] = -d.b[11 * (size_t)c + lane - 32];
  }
  // x_0 = B^-1 (-b) (the bits of cam_binv_axpy_h, mode 0) or x_i = B^-1 N_c^T y; z = sigma (N_c x)
  template <bool FIRST, class Put>
  __device__ static __forceinline__ void solve(const Own& A, int o, int lane, double& s, double& a, Put put) {
    s = 0; a = 0;
    if (lane < 11) {
      if (FIRST) {
        s = binv_row11(A.binv + 121 * o + 11 * lane, A.tmp + 11 * o);
      } else {
        double y[12], y11[11];
#pragma unroll
        for (int j = 0; j < 12; ++j) y[j] = A.y[12 * o + j];
        nt_apply(A.ncw + 13 * o, A.ncw[13 * o + 12], y, y11);
        s = binv_row11(A.binv + 121 * o + 11 * lane, y11);
      }
      a = FIRST ? s : A.acc[11 * o + lane] + s;
      if (!FIRST) A.tmp[11 * o + lane] = s;
      A.acc[11 * o + lane] = a;
    }
    const double zv = nc_z_entry(lane, s, A.ncw + 13 * o, A.sig + 12 * o);
    if (lane < 12) put(zv);
  }
  // sum, last term and its z = sigma N_c x (povar_power_series_step, povar_get_term and povar_apply_joint go on from there)
  template <int NW> __device__ static __forceinline__ void store(const Dp& d, const Own& A, const int* own_cam, int nO, int, int wave, int lane) {
    for (int o = wave; o < nO; o += NW) {
      const int c = own_cam[o];
      const double s = lane < 11 ? A.tmp[11 * o + lane] : 0.0;
      const double zv = nc_z_entry(lane, s, A.ncw + 13 * o, A.sig + 12 * o);
      if (lane < 11) {
        d.accum[11 * (size_t)c + lane] = A.acc[11 * o + lane];
        d.tmp[11 * (size_t)c + lane] = s;
      }
      if (lane < 12) store_z(d, c, lane, zv);
    }
  }
};

// the steps' sizes ARE the layout's: the host decides with these whether a workgroup fits the LDS (res_lds_bytes)
static_assert(ResPose::LM_BYTES == RES_LM_BYTES && ResPose::LM_BYTES == 2 * 8 * ResPose::NCO, "step 1: landmark bytes");
static_assert(ResJoint::LM_BYTES == RES_LM_BYTES_H && ResJoint::LM_BYTES == 2 * 8 * ResJoint::NCO, "step 2: landmark bytes");
static_assert(ResOwn<ResPose>::DOUBLES == RES_OWN_DOUBLES, "step 1: doubles per owned camera");
static_assert(ResOwn<ResJoint>::DOUBLES == RES_OWN_DOUBLES_H, "step 2: doubles per owned camera");

// NW wavefronts per workgroup, chunks of H rows, RR chunks per lane, LS landmark slots per lane
template <class Step, int NW, int H, int RR, int LS, bool ROBUST>
__device__ __forceinline__ void res_series(Dp d, ResP k, const double* ncw) {
  constexpr int T = NW * 64;
  constexpr int STRIDE = LS * T;
  constexpr int GB = NW >= 16 ? 4 : 8;
  constexpr int NX = Step::NX, NCO = Step::NCO;
  extern __shared__ double res_lds[];
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const ResBufs B = res_bufs(k);
  const unsigned tag0 = (*k.launch) << 8;  // (the counter is bumped by a kernel behind this one: stream order)
  const int L0 = k.lm_off[g], nL = Step::lm_count(k.lm_off[g + 1] - L0, STRIDE);
  const int C0 = k.cam_off[g], nC = k.cam_off[g + 1] - C0;
  const int O0 = k.own_off[g], nO = k.own_off[g + 1] - O0;
  const int Q0 = k.oq_off[g], nQ = k.oq_off[g + 1] - Q0;
  // LDS (res_lds_bytes): control words, the landmarks, the region, the owner's arrays, three index tables
  int* ctl = reinterpret_cast<int*>(res_lds);  // [0] a wait gave up, [1] series converged, [2] iterations, [4..5] |x_0|
  double* lx = res_lds + 8;                                 // landmark coordinates (Step::at)
  double* lu = lx + NCO * Step::lm_cap(nL, STRIDE);         // the landmarks' sums, then what the way back reads
  double* reg = lu + NCO * Step::lm_cap(nL, STRIDE);        // the region: z of the cameras [nC][13] -> accumulators [nC][13] -> owner's records [nQ][12]
  const typename Step::Own A(reg + res_region_doubles(nC, nQ), nO);
  int* lzi = reinterpret_cast<int*>(A.end);  // [nC] z-table row of each camera slot
  int* loq = lzi + nC;                  // [nQ] the records read as an owner
  int* lown = loq + nQ;                 // [nO][4] z-table row, first / end position of the records

  // ---------------- prologue: everything that does not change between the terms
  // owned cameras first (their registers are free again before the lane's own state is loaded): B^-1, sigma, the reflector;
  // x_0 = B^-1 (-b) (the series start); z_0 published
  if (t < 4) ctl[t] = 0;
  for (int e = t; e < nC; e += T) lzi[e] = k.cam_zi[C0 + e];
  for (int e = t; e < nQ; e += T) loq[e] = k.oq_rec[Q0 + e];
  for (int e = t; e < nO; e += T) {
    const int2 qr = k.own_q[O0 + e];
    lown[4 * e] = k.own_zi[O0 + e]; lown[4 * e + 1] = qr.x; lown[4 * e + 2] = qr.y;
  }
  for (int o = wave; o < nO; o += NW) Step::load_owner(d, ncw, A, o, k.own_cam[O0 + o], lane);
  __syncthreads();
  for (int o = wave; o < nO; o += NW) {
    const int zi = lown[4 * o];
    double s, a;
    Step::template solve<true>(A, o, lane, s, a, [&](double zv) { res_put(B.z, (unsigned)(12 * zi + lane) * 16u, zv, tag0 | 1u); });
    if (k.want_norm0) {
      double n2[1] = {s * s};
      wave_sum<1>(n2);
      if (lane == 0) { A.nrm[2 * o] = n2[0]; A.nrm[2 * o + 1] = n2[0]; }
    }
    // (the term's place = x_0 once every lane of the wavefront has read -b from it)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (lane < NX) A.tmp[NX * o + lane] = s;
  }
  if (k.want_norm0) {
    __syncthreads();
    if (t == 0) {
      double a = 0;
      for (int o = 0; o < nO; ++o) a += A.nrm[2 * o];
      res_put(B.nrm, res_nrm_off(tag0 | 1u, g, 0), a, tag0 | 1u);
      res_put(B.nrm, res_nrm_off(tag0 | 1u, g, 1), a, tag0 | 1u);
    }
  }
  // the lane's chunks: rows (slot word, weight, what the step keeps of them), camera slot, the camera
  ResChunk<Step, H> ch[RR];
#pragma unroll
  for (int r = 0; r < RR; ++r) {
    const size_t li = ((size_t)g * RR + r) * T + t;
    ch[r].ci = k.lane_cam[li];
    ch[r].seg = k.lane_seg[li];
    const int wh = __builtin_amdgcn_readfirstlane(k.wave_h[((size_t)g * RR + r) * NW + wave]);
    ch[r].hrows = wh & 255;
    ch[r].dup = (wh >> 8) & 1;
    ch[r].steps = (wh >> 12) & 15;
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const size_t row = (((size_t)g * RR + r) * H + j) * T + t;
      Step::load_row(k, ch[r].s, j, row);
      ch[r].ls[j] = Step::slot_word(k.lslot[row], nL);
      ch[r].rw[j] = 1.0;
      if (ROBUST) {
        const int os = k.oslot[row];
        if (os >= 0) {
          if (k.w_mode == 1) ch[r].rw[j] = d.v2.w[d.v2.of_slot[os]];
          else { const double s = d.sw[os]; ch[r].rw[j] = s * s; }
        }
      }
    }
    Step::load_p(d, ch[r].s, ch[r].ci, nC, k.cam_id + C0);
  }
  // the landmark slots of the lane: coordinates into LDS, sums = 0, the rest of the landmark's record in registers
  double rec[LS][Step::NREG];
#pragma unroll
  for (int q = 0; q < LS; ++q) {
#pragma unroll
    for (int e = 0; e < Step::NREG; ++e) rec[q][e] = 0;
    const int s = t + q * T;
    if (s < nL) {
      const int lm = k.lm_id[L0 + s];
      const int pos = d.v2.lm_pos[lm] & ((1 << 26) - 1);
      const double* rp = d.v2.lmrec + ((size_t)(pos >> 6) * Step::LMREC) * WAVE + (pos & 63);
#pragma unroll
      for (int e = 0; e < NCO; ++e) lx[Step::template at<STRIDE>(s, e)] = rp[e * WAVE];
#pragma unroll
      for (int e = 0; e < NCO; ++e) lu[Step::template at<STRIDE>(s, e)] = 0;
#pragma unroll
      for (int e = 0; e < Step::NREG; ++e) rec[q][e] = rp[(NCO + e) * WAVE];
    }
  }
  int iters = k.m;
  auto z_row = [&](int s) { return lzi[s]; };
  auto q_row = [&](int q) { return loq[q]; };

  // ---------------- the terms
  for (int i = 1; i <= k.m + 1; ++i) {
    const unsigned tag = tag0 | (unsigned)i;
    if (i == k.m + 1 && !k.want_norms) break;  // (with the tests on: the last term's norms are looked at too)
    // ---- the norms of term i - 1 (every owner's: the one step of a term that waits for ALL workgroups); the tests are
    // the reference's (:206-214 and :216-229; series_check's :259-283)
    if (k.want_norms && (i > 1 || k.want_norm0)) {
      if (wave == 0) {
        double v[2] = {0, 0};
        bool ok = true;
        for (int w0 = 0; w0 < k.W; w0 += 64) {
          const unsigned off[2] = {res_nrm_off(tag, w0 + lane, 0), res_nrm_off(tag, w0 + lane, 1)};
          const bool act[2] = {w0 + lane < k.W, w0 + lane < k.W};
          double e2[2];
          ok = res_get<2>(B.nrm, off, act, tag, e2, k.spin_limit) && ok;
          if (act[0]) { v[0] += e2[0]; v[1] += e2[1]; }
        }
        if (!ok && lane == 0) ctl[0] = 1;
        wave_sum<2>(v);
        const double iter_norm = sqrt(v[0]), acc_norm = sqrt(v[1]);
        if (i == 1) {
          if (lane == 0) reinterpret_cast<double*>(ctl)[2] = acc_norm;
          if (g == 0 && lane == 0) d.norms[0] = acc_norm;
        } else {
          const double n0 = reinterpret_cast<double*>(ctl)[2];
          bool conv = false;
          if (k.q_tol > 0 && (i - 1) * iter_norm / acc_norm < k.q_tol) conv = true;
          if (!conv && k.r_tol > 0 && iter_norm / n0 < k.r_tol) conv = true;
          if (ok && conv && lane == 0) { ctl[1] = 1; ctl[2] = i - 1; }
          if (g == 0 && lane == 0) { d.norms[1] = iter_norm; d.norms[2] = acc_norm; }
        }
      }
      __syncthreads();
      if (ctl[0] | ctl[1]) break;
    }
    if (i == k.m + 1) break;
    // ---- hand-over 2: z of the workgroup's cameras into the region
    // (the region's last readers were the owner sums of term i - 1: the barrier in front of them is B6 below, the one
    // behind them the barrier at the end of the term)
    if (!res_gather<T, GB>(B.z, nC * 12, z_row, tag, reg, RES_ACC_STRIDE, t, k.spin_limit) && lane == 0) ctl[0] = 1;
    __syncthreads();  // B1
    if (ctl[0]) break;
    // ---- forward: the landmarks' sums (Step::obs_forward: LDS adds on the landmark)
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      if (ch[r].hrows == 0) continue;  // (wave-uniform)
      typename Step::Z zz;
      Step::load_z(reg + (ch[r].ci < 0 ? 0 : ch[r].ci) * RES_ACC_STRIDE, zz);
#pragma unroll
      for (int j = 0; j < H; ++j)
        if (j < ch[r].hrows && ch[r].ls[j] >= 0)
          Step::template obs_forward<ROBUST, STRIDE>(d, ch[r].s, j, ch[r].rw[j], ch[r].ls[j], zz, lx, lu);
    }
    __syncthreads();  // B2
    // ---- the landmark step per slot (over the sums); the region becomes the accumulators
#pragma unroll
    for (int q = 0; q < LS; ++q) {
      const int s = t + q * T;
      if (s < nL) Step::template landmark_step<STRIDE>(lx, lu, s, rec[q]);
    }
    for (int e = t; e < nC * RES_ACC_STRIDE; e += T) reg[e] = 0;
    __syncthreads();  // B3
    // ---- backward (Step::obs_backward, registers); lanes of one camera are summed, the run's last lane adds to the
    // camera's accumulator
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      if (ch[r].hrows == 0) continue;
      double y[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < H; ++j)
        if (j < ch[r].hrows && ch[r].ls[j] >= 0)
          Step::template obs_backward<ROBUST, STRIDE>(d, ch[r].s, j, ch[r].rw[j], ch[r].ls[j], lx, lu, y);
      // (the run's LAST lane holds its sum after the scan: no broadcast)
      if (ch[r].dup) seg_scan_steps<12>(y, lane, ch[r].seg & 255, ch[r].steps);
      if (ch[r].ci >= 0 && lane == ((ch[r].seg >> 8) & 255)) {
        double* a = reg + ch[r].ci * RES_ACC_STRIDE;
        if (ch[r].seg & (1 << 16)) {  // the camera's only run in the workgroup: a plain store
#pragma unroll
          for (int e = 0; e < 12; ++e) a[e] = y[e];
        } else {
#pragma unroll
          for (int e = 0; e < 12; ++e) __hip_atomic_fetch_add(a + e, y[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
    __syncthreads();  // B4
    // ---- the workgroup's partial records: one contiguous run of granule pairs (hand-over 1, the producer's side);
    // the landmarks' sums back to zero for the next term (their last readers were the backward pass)
    for (int e = t; e < nC * 12; e += T)
      res_put(B.part, (unsigned)(C0 * 12 + e) * 16u, reg[(e / 12) * RES_ACC_STRIDE + e % 12], tag);
#pragma unroll
    for (int q = 0; q < LS; ++q) {
      const int s = t + q * T;
      if (s < nL) {
#pragma unroll
        for (int e = 0; e < NCO; ++e) lu[Step::template at<STRIDE>(s, e)] = 0;
      }
    }
    __syncthreads();  // B5 (the accumulators have been read: the region becomes the owner's records)
    // ---- owners (hand-over 1): the records of the cameras the workgroup owns into the region
    if (!res_gather<T, GB>(B.part, nQ * 12, q_row, tag, reg, 12, t, k.spin_limit) && lane == 0) ctl[0] = 1;
    __syncthreads();  // B6
    if (ctl[0]) break;
    // ---- x_i = Step::solve of sigma * sum of the records, sum += x_i, z published (:200-204, :322-340; :246-257, :342-360).
    // A camera's records are summed by five groups of twelve lanes (record q of the camera by group q % 5), then the five
    // partial sums in order
    for (int o = wave; o < nO; o += NW) {
      const int zi = lown[4 * o];
      const int2 qr = make_int2(lown[4 * o + 1], lown[4 * o + 2]);
      if (lane < 60) {
        const int e = lane % 12, grp = lane / 12;
        double a = 0;
        for (int q = qr.x + grp; q < qr.y; q += 5) a += reg[12 * q + e];
        A.ps[60 * o + lane] = a;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      if (lane < 12) {
        const double* ps = A.ps + 60 * o + lane;
        const double yl = (((ps[0] + ps[12]) + ps[24]) + ps[36]) + ps[48];
        A.y[12 * o + lane] = yl * A.sig[12 * o + lane];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      double s, a;
      Step::template solve<false>(A, o, lane, s, a, [&](double zv) { res_put(B.z, (unsigned)(12 * zi + lane) * 16u, zv, tag + 1u); });
      if (k.want_norms) {
        double n2[2] = {s * s, a * a};
        wave_sum<2>(n2);
        if (lane == 0) { A.nrm[2 * o] = n2[0]; A.nrm[2 * o + 1] = n2[1]; }
      }
    }
    __syncthreads();  // B7 (the owner sums have read the region: the next term's z may land in it)
    if (k.want_norms && t == 0) {
      double a = 0, b = 0;
      for (int o = 0; o < nO; ++o) { a += A.nrm[2 * o]; b += A.nrm[2 * o + 1]; }
      res_put(B.nrm, res_nrm_off(tag + 1u, g, 0), a, tag + 1u);
      res_put(B.nrm, res_nrm_off(tag + 1u, g, 1), b, tag + 1u);
    }
  }
  // ---------------- epilogue: sum and last term of the owned cameras, status
  __syncthreads();
  if (ctl[1]) iters = ctl[2];
  Step::template store<NW>(d, A, k.own_cam + O0, nO, t, wave, lane);
  if (t == 0) {
    if (ctl[0]) atomicOr(&d.flags[0], 4);
    if (g == 0 && ctl[1]) {
      d.flags[1] = 1;
      d.flags[2] = iters;
      d.flags[3] = 1;
    }
  }
}

template <int NW, int H, int RR, int LS, bool ROBUST>
__global__ __launch_bounds__(NW * 64) void series_res(Dp d, ResP k) {
  res_series<ResPose, NW, H, RR, LS, ROBUST>(d, k, nullptr);
}
template <int NW, int H, int RR, int LS, bool ROBUST>
__global__ __launch_bounds__(NW * 64) void series_res_h(Dp d, ResP k, const double* ncw) {
  res_series<ResJoint, NW, H, RR, LS, ROBUST>(d, k, ncw);
}

// the launch counter (the high bits of the granule tags of the NEXT launch): a one-thread kernel behind series_res in the
// stream -- inside the launch itself a workgroup that is late could still be reading the old value
POVAR_KERNEL void res_bump_launch(unsigned* launch) {
  unsigned v = *launch + 1u;
  if (v >= (1u << 24)) v = 1u;  // (a tag is launch << 8 | term: 24 bits; a wrap meets granules 16 M launches old)
  *launch = v;
}

}  // namespace povar
