// povar_kernels_res_joint.hpp -- series_res_h: the RESIDENT power series of step 2 (RIPOBA): the whole loop of solve_joint
// (sc/linearization_power_varproj.hpp:240-287: x_0 = B^-1 (-b); x_i = B^-1 N_c^T sigma E0 sigma N_c x_{i-1}; sum, early
// exit) in ONE launch.  series_res (povar_kernels_res.hpp) with the operator of e0_ck_h (povar_kernels_ck_joint.hpp) and the
// owner step of cam_cold_sum_binv_h (povar_kernels_joint.hpp): structure, phase order, barriers B1-B7, hand-overs (tagged
// granule pairs, bounded spins, give-up bit 2 of flags[0]) and the double-buffered norm sweep are series_res's, and
// res_put / res_get / res_gather / res_nrm_off / res_bump_launch are used as they are.  What differs:
//   * a LANE keeps, per chunk, the camera's whole P_c (3 x 4, from cams_lin4: what build_hot_rec copies into the records
//     of the per-term kernels), the landmark slot of each row and, with a robust norm, its weight.  No image points: the
//     step-2 operator does not read them (header of povar_kernels_ck_joint.hpp);
//   * the LANDMARKS of the workgroup live in LDS as X [4][STRIDE] and U4 / G4 [4][STRIDE], component-major with the
//     compile-time stride STRIDE = LS NW 64 (the instantiation's slot capacity), so that ckh_obs_forward, ckh_obs_backward
//     and ckh_landmark_step run unchanged and the "ckh" error model of tests/rounding_bounds.py is this kernel's too; the
//     slot's lane keeps s (4) and the upper triangle of Hll^-1 (6) -- entries 4..13 of the 14-double record of V2::lmrec,
//     which both preparation paths write (prepare_lpl_h per lane, OpPrepareH::finish_lm per landmark) at every prepare;
//   * z_c is the AMBIENT 12-vector sigma (N_c x_c); the owner of a camera holds B_c^-1 (11 x 11, row stride 11), sigma,
//     the reflector (w[12], beta) of N_c, the running sum (11) and the last term (11), and per term computes
//     y = sum of the records (.) sigma, y11 = N_c^T y (nt_apply), x = B^-1 y11 (binv_row11), sum += x, z = sigma (N_c x).
// LDS: res_layout.hpp, res_shape_step2().
#pragma once

#include "povar_kernels_res.hpp"
#include "povar_kernels_ck_joint.hpp"

namespace povar {

// the per-lane state of one chunk
template <int H>
struct ResChunkH {
  Cam P;
  int ls[H];
  double rw[H];
  int ci, seg, hrows, dup, steps;
};

// Entry `lane` (< 12) of z = sigma (.) (N_c x) with x's entry `lane` in s (lanes 0..10; 0 in the others): p = [0; x] -
// beta w (w[1:] . x), the products summed over lanes 0..15 as in cam_binv_axpy_h.  Every lane of the wavefront calls it.
__device__ inline double resh_z_entry(int lane, double s, const double* w13, const double* sig) {
  double wt = lane < 11 ? w13[lane + 1] * s : 0.0;
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) wt += shfl_xor_d(wt, m);
  const double prev = shfl_up_d(s, 1);
  const int l = lane < 12 ? lane : 0;
  const double p = (lane == 0 ? 0.0 : prev) - w13[12] * w13[l] * wt;
  return p * sig[l];
}

// NW wavefronts per workgroup, chunks of H rows, RR chunks per lane, LS landmark slots per lane
template <int NW, int H, int RR, int LS, bool ROBUST>
__global__ __launch_bounds__(NW * 64) void series_res_h(Dp d, ResP k, const double* ncw) {
  constexpr int T = NW * 64;
  constexpr int STRIDE = LS * T;
  constexpr int GB = NW >= 16 ? 4 : 8;
  extern __shared__ double res_lds[];
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const ResBufs B = res_bufs(k);
  const unsigned tag0 = (*k.launch) << 8;  // (the counter is bumped by a kernel behind this one: stream order)
  const int L0 = k.lm_off[g], nL = min(k.lm_off[g + 1] - L0, STRIDE);
  const int C0 = k.cam_off[g], nC = k.cam_off[g + 1] - C0;
  const int O0 = k.own_off[g], nO = k.own_off[g + 1] - O0;
  const int Q0 = k.oq_off[g], nQ = k.oq_off[g + 1] - Q0;
  int* ctl = reinterpret_cast<int*>(res_lds);  // [0] a wait gave up, [1] series converged, [2] iterations, [4..5] |x_0|
  double* lx = res_lds + 8;             // [4][STRIDE] X of the workgroup's landmarks
  double* lu = lx + 4 * STRIDE;         // [4][STRIDE] U4 = sum J4^T t, then G4
  double* reg = lu + 4 * STRIDE;        // the region: z of the cameras [nC][13] -> accumulators [nC][13] -> owner's records [nQ][12]
  double* obinv = reg + res_region_doubles(nC, nQ);  // [nO][121] B^-1 of the owned cameras
  double* osig = obinv + 121 * nO;      // [nO][12] sigma
  double* oncw = osig + 12 * nO;        // [nO][13] reflector of N_c: w (12), beta
  double* oacc = oncw + 13 * nO;        // [nO][11] running sum
  double* otmp = oacc + 11 * nO;        // [nO][11] last term
  double* oy = otmp + 11 * nO;          // [nO][12] E0 row of the term: sigma * sum of the camera's records (ambient)
  double* onrm = oy + 12 * nO;          // [nO][2] squared norms of the last term / the sum
  double* ops = onrm + 2 * nO;          // [nO][5][12] partial sums of the camera's records (five groups of twelve lanes)
  int* lzi = reinterpret_cast<int*>(ops + 60 * nO);  // [nC] z-table row of each camera slot
  int* loq = lzi + nC;                  // [nQ] the records read as an owner
  int* lown = loq + nQ;                 // [nO][4] z-table row, first / end position of the records

  // ---------------- prologue: everything that does not change between the terms
  // owned cameras first: B^-1, sigma, N_c; x_0 = B^-1 (-b) (the series start, :243); z_0 published
  if (t < 4) ctl[t] = 0;
  for (int e = t; e < nC; e += T) lzi[e] = k.cam_zi[C0 + e];
  for (int e = t; e < nQ; e += T) loq[e] = k.oq_rec[Q0 + e];
  for (int e = t; e < nO; e += T) {
    const int2 qr = k.own_q[O0 + e];
    lown[4 * e] = k.own_zi[O0 + e]; lown[4 * e + 1] = qr.x; lown[4 * e + 2] = qr.y;
  }
  for (int o = wave; o < nO; o += NW) {
    const int c = k.own_cam[O0 + o];
    for (int e = lane; e < 121; e += 64) obinv[121 * o + e] = d.binv[144 * (size_t)c + e];
    if (lane < 12) osig[12 * o + lane] = d.sigma[12 * (size_t)c + lane];
    if (lane >= 16 && lane < 29) oncw[13 * o + lane - 16] = ncw[13 * (size_t)c + lane - 16];
    if (lane >= 32 && lane < 43) otmp[11 * o + lane - 32] = -d.b[11 * (size_t)c + lane - 32];
  }
  __syncthreads();
  for (int o = wave; o < nO; o += NW) {
    const int zi = lown[4 * o];
    double s = 0;
    if (lane < 11) {
      s = binv_row11(obinv + 121 * o + 11 * lane, otmp + 11 * o);  // (the bits of cam_binv_axpy_h, mode 0)
      oacc[11 * o + lane] = s;
    }
    const double zv = resh_z_entry(lane, s, oncw + 13 * o, osig + 12 * o);
    if (lane < 12) res_put(B.z, (unsigned)(12 * zi + lane) * 16u, zv, tag0 | 1u);
    if (k.want_norm0) {
      double n2[1] = {s * s};
      wave_sum<1>(n2);
      if (lane == 0) { onrm[2 * o] = n2[0]; onrm[2 * o + 1] = n2[0]; }
    }
    // (otmp = x_0 once every lane of the wavefront has read -b from it)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if (lane < 11) otmp[11 * o + lane] = s;
  }
  if (k.want_norm0) {
    __syncthreads();
    if (t == 0) {
      double a = 0;
      for (int o = 0; o < nO; ++o) a += onrm[2 * o];
      res_put(B.nrm, res_nrm_off(tag0 | 1u, g, 0), a, tag0 | 1u);
      res_put(B.nrm, res_nrm_off(tag0 | 1u, g, 1), a, tag0 | 1u);
    }
  }
  // the lane's chunks: landmark slots, weights, camera slot, P_c
  ResChunkH<H> ch[RR];
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
      const int l3 = k.lslot[row];  // (3 x slot: the layout's rows are step 1's where the two steps share them)
      ch[r].ls[j] = l3 < 0 || l3 >= 3 * nL ? -1 : l3 / 3;
      ch[r].rw[j] = 1.0;
      if (ROBUST) {
        const int os = k.oslot[row];
        if (os >= 0) {
          if (k.w_mode == 1) ch[r].rw[j] = d.v2.w[d.v2.of_slot[os]];
          else { const double s = d.sw[os]; ch[r].rw[j] = s * s; }
        }
      }
    }
    ch[r].P.r0 = ch[r].P.r1 = ch[r].P.r2 = make_double4(0, 0, 0, 0);
    if (ch[r].ci >= nC) ch[r].ci = -1;
    if (ch[r].ci >= 0) ch[r].P = load_cam(d.cams_lin4, k.cam_id[C0 + ch[r].ci]);
  }
  // the landmark slots of the lane: X into LDS, U4 = 0, s and Hll^-1 in registers 
  double rec[LS][10];
#pragma unroll
  for (int q = 0; q < LS; ++q) {
#pragma unroll
    for (int e = 0; e < 10; ++e) rec[q][e] = 0;
    const int s = t + q * T;
    if (s < nL) {
      const int lm = k.lm_id[L0 + s];
      const int pos = d.v2.lm_pos[lm] & ((1 << 26) - 1);
      const double* rp = d.v2.lmrec + ((size_t)(pos >> 6) * CKH_REC) * WAVE + (pos & 63);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        lx[e * STRIDE + s] = rp[e * WAVE];
        lu[e * STRIDE + s] = 0;
      }
#pragma unroll
      for (int e = 0; e < 10; ++e) rec[q][e] = rp[(4 + e) * WAVE];
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
    // series_check's (:259-283)
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
    if (!res_gather<T, GB>(B.z, nC * 12, z_row, tag, reg, RES_ACC_STRIDE, t, k.spin_limit) && lane == 0) ctl[0] = 1;
    __syncthreads();  // B1
    if (ctl[0]) break;
    // ---- forward: U4_l += J4^T t, t = sw D (Z X) (four LDS adds per observation)
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      if (ch[r].hrows == 0) continue;  // (wave-uniform)
      const double* zp = reg + (ch[r].ci < 0 ? 0 : ch[r].ci) * RES_ACC_STRIDE;
      const double4 zz[3] = {make_double4(zp[0], zp[1], zp[2], zp[3]), make_double4(zp[4], zp[5], zp[6], zp[7]),
                             make_double4(zp[8], zp[9], zp[10], zp[11])};
#pragma unroll
      for (int j = 0; j < H; ++j)
        if (j < ch[r].hrows && ch[r].ls[j] >= 0)
          ckh_obs_forward<ROBUST, STRIDE>(ch[r].P, zz, ch[r].rw[j], lx, lu, (uint32_t)ch[r].ls[j]);
    }
    __syncthreads();  // B2
    // ---- U4 -> G4 per landmark slot; the region becomes the accumulators
#pragma unroll
    for (int q = 0; q < LS; ++q) {
      const int s = t + q * T;
      if (s < nL) ckh_landmark_step<STRIDE>(lx, lu, s, rec[q]);
    }
    for (int e = t; e < nC * RES_ACC_STRIDE; e += T) reg[e] = 0;
    __syncthreads();  // B3
    // ---- backward: y_c += X_l (x) q; lanes of one camera are summed, the run's last lane adds to the camera's accumulator
#pragma unroll
    for (int r = 0; r < RR; ++r) {
      if (ch[r].hrows == 0) continue;
      double y[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < H; ++j)
        if (j < ch[r].hrows && ch[r].ls[j] >= 0)
          ckh_obs_backward<ROBUST, STRIDE>(ch[r].P, ch[r].rw[j], lx, lu, (uint32_t)ch[r].ls[j], y);
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
    // U4 back to zero for the next term (its last readers were the backward pass)
    for (int e = t; e < nC * 12; e += T)
      res_put(B.part, (unsigned)(C0 * 12 + e) * 16u, reg[(e / 12) * RES_ACC_STRIDE + e % 12], tag);
#pragma unroll
    for (int q = 0; q < LS; ++q) {
      const int s = t + q * T;
      if (s < nL) {
#pragma unroll
        for (int e = 0; e < 4; ++e) lu[e * STRIDE + s] = 0;
      }
    }
    __syncthreads();  // B5 (the accumulators have been read: the region becomes the owner's records)
    // ---- owners (hand-over 1): the records of the cameras the workgroup owns into the region
    if (!res_gather<T, GB>(B.part, nQ * 12, q_row, tag, reg, 12, t, k.spin_limit) && lane == 0) ctl[0] = 1;
    __syncthreads();  // B6
    if (ctl[0]) break;
    // ---- x_i = B^-1 N_c^T (sigma * sum of the records), sum += x_i, z = sigma N_c x_i published (:246-257, :342-360).
    // A camera's records are summed by five groups of twelve lanes (record q of the camera by group q % 5), then the
    // five partial sums in order
    for (int o = wave; o < nO; o += NW) {
      const int zi = lown[4 * o];
      const int2 qr = make_int2(lown[4 * o + 1], lown[4 * o + 2]);
      if (lane < 60) {
        const int e = lane % 12, grp = lane / 12;
        double a = 0;
        for (int q = qr.x + grp; q < qr.y; q += 5) a += reg[12 * q + e];
        ops[60 * o + lane] = a;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      if (lane < 12) {
        const double yl = (((ops[60 * o + lane] + ops[60 * o + 12 + lane]) + ops[60 * o + 24 + lane]) + ops[60 * o + 36 + lane]) + ops[60 * o + 48 + lane];
        oy[12 * o + lane] = yl * osig[12 * o + lane];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      double s = 0, a = 0;
      if (lane < 11) {
        double y[12], y11[11];
#pragma unroll
        for (int j = 0; j < 12; ++j) y[j] = oy[12 * o + j];
        nt_apply(oncw + 13 * o, oncw[13 * o + 12], y, y11);
        s = binv_row11(obinv + 121 * o + 11 * lane, y11);
        a = oacc[11 * o + lane] + s;
        otmp[11 * o + lane] = s;
        oacc[11 * o + lane] = a;
      }
      const double zv = resh_z_entry(lane, s, oncw + 13 * o, osig + 12 * o);
      if (lane < 12) res_put(B.z, (unsigned)(12 * zi + lane) * 16u, zv, tag + 1u);
      if (k.want_norms) {
        double n2[2] = {s * s, a * a};
        wave_sum<2>(n2);
        if (lane == 0) { onrm[2 * o] = n2[0]; onrm[2 * o + 1] = n2[1]; }
      }
    }
    __syncthreads();  // B7 (the owner sums have read the region: the next term's z may land in it)
    if (k.want_norms && t == 0) {
      double a = 0, b = 0;
      for (int o = 0; o < nO; ++o) { a += onrm[2 * o]; b += onrm[2 * o + 1]; }
      res_put(B.nrm, res_nrm_off(tag + 1u, g, 0), a, tag + 1u);
      res_put(B.nrm, res_nrm_off(tag + 1u, g, 1), b, tag + 1u);
    }
  }
  // ---------------- epilogue: sum, last term and its z = sigma N_c x of the owned cameras (where the per-term kernels leave
  // them: povar_power_series_step, povar_get_term and povar_apply_joint go on from there), status
  __syncthreads();
  if (ctl[1]) iters = ctl[2];
  for (int o = wave; o < nO; o += NW) {
    const int c = k.own_cam[O0 + o];
    const double s = lane < 11 ? otmp[11 * o + lane] : 0.0;
    const double zv = resh_z_entry(lane, s, oncw + 13 * o, osig + 12 * o);
    if (lane < 11) {
      d.accum[11 * (size_t)c + lane] = oacc[11 * o + lane];
      d.tmp[11 * (size_t)c + lane] = s;
    }
    if (lane < 12) store_z(d, c, lane, zv);
  }
  if (t == 0) {
    if (ctl[0]) atomicOr(&d.flags[0], 4);
    if (g == 0 && ctl[1]) {
      d.flags[1] = 1;
      d.flags[2] = iters;
      d.flags[3] = 1;
    }
  }
}

}  // namespace povar
