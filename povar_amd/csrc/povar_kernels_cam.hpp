// povar_kernels_cam.hpp -- gfx950 device code of the PER-CAMERA step that ends every power-series term: sum camera c's row of
// E0 x (its cold observations + its partial records), then x = B_c^-1 y, the AXPY into the sum and z = sigma x for the next
// term (right_mul_b_inv_pOSE / _joint + the loop bodies of solve_pOSE / solve_joint, linearization_power_varproj.hpp:196-207,
// 246-257, 322-360).  ONE gather (cam_row_sum), ONE store of the results (cam_tail), two steps: CamPose / CamJoint say which
// operands a camera's workgroup requests ahead of the gather and how the twelve sums become an entry of x and of z.  The
// kernels are wrappers:
//   cam_cold_sum_binv[_h]   the whole step in one launch (unsharded LDSACC term loop): cam_cold_step<CamPose | CamJoint>
//   cam_cold_sum            the gather alone: dense y, or the peer-to-peer push of a sharded context's partial
//   cam_binv_axpy[_h]       B^-1, AXPY and z from y = -b, the scatter items, the dense y or the peers' slabs
//   cam_sum_items[_h]       the scatter items' sum alone
// The fused step is a latency chain: whatever depends on c only is requested before the series-done test
// and the gather, so that nothing behind the workgroup sum waits for memory.
#pragma once

#include "povar_kernels_joint.hpp"

namespace povar {

// ---- where camera c's partial records are: one contiguous run of Dp::hot_part (Dp::part_range: e0_lpl / e0_ck), or the
// n_hot_wg records of accumulator slot cam_hot[c] - 1 (the lane-per-observation kernels).  The loads (part_request: x, y =
// part_range[c], z = cam_hot[c]) are apart from the answer (part_run: first record, one past the last) so that a kernel
// can request them early
__device__ __forceinline__ int3 part_request(const Dp& d, int c) {
  const int2 rr = d.hot_part && d.part_range ? d.part_range[c] : make_int2(0, 0);
  return make_int3(rr.x, rr.y, d.hot_part ? d.cam_hot[c] : 0);
}
__device__ __forceinline__ int2 part_run(const Dp& d, int3 q) {
  if (d.hot_part && d.part_range) return make_int2(q.x, q.y);
  if (q.z > 0 && q.z <= d.n_hot_acc) return make_int2((q.z - 1) * d.n_hot_wg, q.z * d.n_hot_wg);
  return make_int2(0, 0);
}
// acc += the records w0, w0 + stride, ... of the run
__device__ __forceinline__ void part_add(const Dp& d, int2 run, int w0, int stride, double (&acc)[12]) {
  for (int w = run.x + w0; w < run.y; w += stride) {
    const double* ip = d.hot_part + (size_t)w * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] += ip[k];
  }
}

// fixed-order sum of a camera's scatter items (+ the LDS-accumulated workgroup partials of a cached
// camera): lanes stride over the parts, then a butterfly; every lane ends with the 12 sums
__device__ inline void camera_item_sum(const Dp& d, int c, int lane, double (&y)[12]) {
#pragma unroll
  for (int j = 0; j < 12; ++j) y[j] = 0;
  for (int it = d.cmv.cam_item_off[c] + lane; it < d.cmv.cam_item_off[c + 1]; it += WAVE) {
    const double* ip = d.cmv.part + 12 * (size_t)it;
#pragma unroll
    for (int j = 0; j < 12; ++j) y[j] += ip[j];
  }
  part_add(d, part_run(d, part_request(d, c)), lane, WAVE, y);
  wave_sum<12>(y);
}

// ---- LDSACC modes: the sums of camera c = sum over the camera's COLD observations of (h q0; h q1; h q2)
//                                            + sum of the workgroups' LDS-accumulated partials of a cached camera.
constexpr int CCS_THREADS = 128;  // threads per camera of the per-camera kernels of the term loop (cam_cold_sum[_binv][_h])
// One NT-thread workgroup per camera, fixed summation order: stride NT over the cold view, four observations per thread in
// flight, then stride NT over the records, then the workgroup sum; replaces cm_scatter + the item sums (a single wavefront
// walking a few hundred items per camera was a serial chain of dependent loads).
struct CamRow { int2 obs; int3 part; };
// one load instead of the two-level item index, and the records' range with it: the partial loop does not wait a round trip of its own
__device__ __forceinline__ CamRow cam_row_request(const Dp& d, int c) { return {d.cmv.cam_range[c], part_request(d, c)}; }
// HOM: h~ has a fourth component (step 2); it is 1 in step 1.  Every thread ends with the 12 sums
template <bool HOM, int NT>
__device__ __forceinline__ void cam_row_sum(const Dp& d, const CamRow& rq, int t, double (&acc)[12], double* sh /* [NT/64][12] */) {
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0;
  const int p0 = rq.obs.x, p1 = rq.obs.y;
  // index loads, then the dependent gathers, then the FMAs (8 with the gather through CmView::src: 1499 -> 1470 terms/s on final-13682)
  constexpr int U = 4;
  for (int pb = p0 + t; pb < p1; pb += U * NT) {
    double hx[U], hy[U], hz[U], hw[U];
    double4 q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = pb + u * NT;
      const bool in = p < p1;
      const int pc = in ? p : p0;
      hx[u] = d.cmv.h[pc];
      hy[u] = d.cmv.h[d.cmv.n + pc];
      hz[u] = d.cmv.h[2 * d.cmv.n + pc];
      if (HOM) hw[u] = d.cmv.h[3 * d.cmv.n + pc];
      q[u] = in ? d.q4c[d.cmv.src ? d.cmv.src[pc] : pc] : make_double4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc[0] += hx[u] * q[u].x; acc[1] += hy[u] * q[u].x; acc[2] += hz[u] * q[u].x; acc[3] += HOM ? hw[u] * q[u].x : q[u].x;
      acc[4] += hx[u] * q[u].y; acc[5] += hy[u] * q[u].y; acc[6] += hz[u] * q[u].y; acc[7] += HOM ? hw[u] * q[u].y : q[u].y;
      acc[8] += hx[u] * q[u].z; acc[9] += hy[u] * q[u].z; acc[10] += hz[u] * q[u].z; acc[11] += HOM ? hw[u] * q[u].z : q[u].z;
    }
  }
  part_add(d, part_run(d, rq.part), t, NT, acc);
  block_sum_dpp<12, NT>(acc, sh);
}

// ---- the end of every per-camera step, by the NT threads that reach it (64: one camera's first wavefront, a norm partial
// per camera; K9_CAMS * 64: a wavefront per camera, a partial per workgroup): lane l stores entry l of the term (s) and of the
// sum (a), l < NX, and of z = sigma x (zv), l < 12; norm_part[blockIdx.x] = squared norms of term and sum
template <int NX, int NT>
__device__ __forceinline__ void cam_tail(const Dp& d, int c, int l, bool in, double s, double a, double zv, int want_norms, double* sh) {
  double nrm[2] = {0, 0};
  if (in && l < NX) {
    const size_t idx = NX * (size_t)c + l;
    d.tmp[idx] = s;
    d.accum[idx] = a;
    nrm[0] = s * s;
    nrm[1] = a * a;
  }
  if (in && l < 12) store_z(d, c, l, zv);
  if (want_norms) {
    if (NT == 64) wave_sum<2>(nrm);
    else block_sum<2, NT>(nrm, sh);
    if (threadIdx.x == 0) {
      d.norm_part[2 * (size_t)blockIdx.x] = nrm[0];
      d.norm_part[2 * (size_t)blockIdx.x + 1] = nrm[1];
    }
  }
}

// One row of x = B_c^-1 y of step 1 (12 x 12, row stride 12)
template <class Y>
__device__ __forceinline__ double binv_row12(const double* Bi, const Y& y) {
  double s = 0;
#pragma unroll
  for (int j = 0; j < 12; ++j) s += Bi[j] * y[j];
  return s;
}

// ---- the two steps of the fused kernel.  request: what thread t needs behind the sum and that depends on c only, requested
// ahead of the series-done test and the gather (off the critical path: the kernel is 7 us with it and 9 without).  solve: from the
// twelve sums, entry t of x = B^-1 (sigma y) (s; t < NX, 0 in the other lanes), of the sum with it (a) and of z (zv; t < 12)
struct CamPose {
  static constexpr int NX = 12;
  static constexpr bool HOM = false;
  struct Ops { double bi[12], sg[12], acc_old, sg_t; };
  __device__ static __forceinline__ void request(const Dp& d, const double*, int c, int t, Ops& o) {
    o.acc_old = o.sg_t = 0;
    if (t < 12) {
      const size_t base = 12 * (size_t)c;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        o.bi[j] = d.binv[144 * (size_t)c + 12 * t + j];
        o.sg[j] = d.sigma[base + j];
      }
      o.acc_old = d.accum[base + t];
      o.sg_t = d.sigma[base + t];
    }
  }
  __device__ static __forceinline__ void solve(const Ops& o, const double (&acc)[12], int t, double& s, double& a, double& zv) {
    s = a = zv = 0;
    if (t < 12) {
      double y[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) y[j] = acc[j] * o.sg[j];
      s = binv_row12(o.bi, y);
      a = o.acc_old + s;
      zv = s * o.sg_t;
    }
  }
};

// step 2: y11 = N_c^T (sigma y) (nt_apply), B^-1 11 x 11 (binv_row11), z = sigma (N_c x) (nc_z_entry)
struct CamJoint {
  static constexpr int NX = 11;
  static constexpr bool HOM = true;
  struct Ops { double bi[11], sg[12], w[12], beta, acc_old, sg_t, w_t, w_next; };
  __device__ static __forceinline__ void request(const Dp& d, const double* ncw, int c, int t, Ops& o) {
    const size_t base = 12 * (size_t)c;
    const double* w13 = ncw + 13 * (size_t)c;
    o.beta = w13[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      o.sg[j] = d.sigma[base + j];
      o.w[j] = w13[j];
    }
    o.acc_old = o.sg_t = o.w_t = o.w_next = 0;
    if (t < 11) {
#pragma unroll
      for (int j = 0; j < 11; ++j) o.bi[j] = d.binv[144 * (size_t)c + 11 * t + j];
      o.acc_old = d.accum[11 * (size_t)c + t];
      o.w_next = w13[t + 1];
    }
    if (t < 12) {
      o.sg_t = d.sigma[base + t];
      o.w_t = w13[t];
    }
  }
  __device__ static __forceinline__ void solve(const Ops& o, const double (&acc)[12], int t, double& s, double& a, double& zv) {
    double y[12], y11[11];
#pragma unroll
    for (int j = 0; j < 12; ++j) y[j] = acc[j] * o.sg[j];
    nt_apply(o.w, o.beta, y, y11);
    s = a = 0;
    if (t < 11) {
      s = binv_row11(o.bi, y11);
      a = o.acc_old + s;
    }
    zv = nc_z_entry(t, s, o.w_next, o.w_t, o.beta, o.sg_t);
  }
};

// cam_cold_sum fused with cam_binv_axpy[_h] (mode 2) for the unsharded LDSACC term loop: the workgroup that has just summed
// camera c's E0 row applies B_c^-1, the AXPY and the sigma scaling itself, so the term needs one kernel less (the dense y is
// never materialised).  Norm partials are per camera (series_check then sums n_cams entries).
template <class Step, int NT>
__device__ __forceinline__ void cam_cold_step(const Dp& d, int want_norms, const double* ncw, double* sh /* [NT/64][12] */) {
  const int done = d.flags[1];  // tested after the first batch of loads is in flight
  const int c = blockIdx.x, t = threadIdx.x;
  const CamRow rq = cam_row_request(d, c);
  typename Step::Ops o;
  Step::request(d, ncw, c, t, o);
  if (done) return;
  double acc[12];
  cam_row_sum<Step::HOM, NT>(d, rq, t, acc, sh);
  if (t >= 64) return;
  double s, a, zv;
  Step::solve(o, acc, t, s, a, zv);
  cam_tail<Step::NX, 64>(d, c, t, true, s, a, zv, want_norms, sh);
}
template <int NT>
__global__ __launch_bounds__(NT) void cam_cold_sum_binv(Dp d, int want_norms) {
  __shared__ double sh[NT / 64 * 12];
  cam_cold_step<CamPose, NT>(d, want_norms, nullptr, sh);
}
template <int NT>
__global__ __launch_bounds__(NT) void cam_cold_sum_binv_h(Dp d, int want_norms, const double* ncw) {
  __shared__ double sh[NT / 64 * 12];
  cam_cold_step<CamJoint, NT>(d, want_norms, ncw, sh);
}

// y_c = sigma * (the sums of camera c), hom: step 2's rows
template <int NT>
__global__ __launch_bounds__(NT) void cam_cold_sum(Dp d, int hom) {
  const int done = d.flags[1];  // tested after the first batch of loads is in flight
  __shared__ double sh[NT / 64 * 12];
  const int c = blockIdx.x, t = threadIdx.x;
  const CamRow rq = cam_row_request(d, c);
  const double sg_t = t < 12 ? d.sigma[12 * (size_t)c + t] : 0.0;  // requested early, used last
  if (done) return;
  double acc[12];
  if (hom) cam_row_sum<true, NT>(d, rq, t, acc, sh);
  else cam_row_sum<false, NT>(d, rq, t, acc, sh);
  if (t < 12) {
    double v = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) v = (t == k) ? acc[k] : v;
    v *= sg_t;
    if (d.p2p_peer) {
      // push this rank's partial of camera c into the slab [parity][rank] of EVERY rank's exchange buffer, then
      // publish it with the epoch tag in the record's 13th entry.  Every store and every load of these bytes is a
      // system-scope (sc0 sc1, write-through / cache-bypassing) access and the storing wavefront drains its stores
      // (s_waitcnt vmcnt(0)) before the tag: no release fence -- a system-scope fence writes the whole L2 back,
      // 44 us per term with one per camera (MI355X_MICROARCH.md, "Valid forms").  Lanes 0..11 are one wavefront.
      const unsigned long long ep = *d.p2p_epoch;
      const size_t off = ((((size_t)(ep & 1) * d.p2p_world + d.p2p_rank) * d.n_cams) + c) * 16;
      for (int p = 0; p < d.p2p_world; ++p)
        __hip_atomic_store(d.p2p_peer[p] + off + t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (t == 0)
        for (int p = 0; p < d.p2p_world; ++p)
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(d.p2p_peer[p] + off + 12), ep, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
      d.y[12 * (size_t)c + t] = v;
    }
  }
}

// b_c = sigma * sum_items (scatter parts)   (landmark_block.hpp:529-534); one wavefront per camera
POVAR_KERNEL __launch_bounds__(256) void cam_sum_items(Dp d, double* out, int apply_sigma) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= d.n_cams) return;
  double y[12];
  camera_item_sum(d, c, lane, y);
  if (lane < 12) {
    double v = 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) v = (lane == j) ? y[j] : v;
    out[12 * (size_t)c + lane] = apply_sigma ? v * d.sigma[12 * (size_t)c + lane] : v;
  }
}

// b11_c = N_c^T (sigma * sum_items); one wavefront per camera
POVAR_KERNEL __launch_bounds__(256) void cam_sum_items_h(Dp d, double* out11, const double* ncw) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= d.n_cams) return;
  double y[12];
  camera_item_sum(d, c, lane, y);
#pragma unroll
  for (int j = 0; j < 12; ++j) y[j] *= d.sigma[12 * (size_t)c + j];
  double o[11];
  nt_apply(ncw + 13 * (size_t)c, ncw[13 * (size_t)c + 12], y, o);
  if (lane < 11) {
    double v = 0;
#pragma unroll
    for (int j = 0; j < 11; ++j) v = (lane == j) ? o[j] : v;
    out11[11 * (size_t)c + lane] = v;
  }
}

// K9 + K11: tmp = B^-1 y, accum (+)= tmp, z = sigma * tmp, optional squared-norm partials
// (right_mul_b_inv_pOSE + the loop body of solve_pOSE, linearization_power_varproj.hpp:196-207,
// 322-340).  mode 0: y = -b (series start); 1: y = sigma * sum of scatter items (implicit E0);
// 2: y = dense buffer d.y (the per-camera sums of the LDSACC modes, or the all-reduced vector).
POVAR_KERNEL __launch_bounds__(K9_CAMS * 64) void cam_binv_axpy(Dp d, int mode, int want_norms) {
  const int done = mode != 0 ? d.flags[1] : 0;  // tested before the first store: its round trip overlaps the loads
  __shared__ double sh[K9_CAMS * 2];
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * K9_CAMS + (threadIdx.x >> 6);
  const bool in = c < d.n_cams;
  double y[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) y[j] = 0;
  if (in) {
    const size_t base = 12 * (size_t)c;
    if (mode == 0) {
#pragma unroll
      for (int j = 0; j < 12; ++j) y[j] = -d.b[base + j];
    } else if (mode == 1) {
      camera_item_sum(d, c, lane, y);
#pragma unroll
      for (int j = 0; j < 12; ++j) y[j] *= d.sigma[base + j];
    } else if (mode == 5) {
      // peer-to-peer exchange: wait for every rank's slab of this camera (tag == epoch), sum in rank order
      const unsigned long long ep = *d.p2p_epoch;
      const double* mine = d.p2p_peer[d.p2p_rank];
      const bool gave_up = (d.flags[0] & 2) != 0;  // an earlier wait of this solve timed out: do not wait again
      for (int p = 0; p < d.p2p_world; ++p) {
        const double* rec = mine + ((((size_t)(ep & 1) * d.p2p_world + p) * d.n_cams) + c) * 16;
        int spins = 0;
        while (!gave_up && __hip_atomic_load(reinterpret_cast<const unsigned long long*>(rec + 12), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM) != ep) {  // relaxed poll; the data loads below bypass the caches too
          __builtin_amdgcn_s_sleep(8);
          if (++spins > (1 << 22)) {  // a peer never arrived: flag it and go on (the host reports the failure)
            if (lane == 0) atomicOr(&d.flags[0], 2);
            break;
          }
        }
#pragma unroll
        for (int j = 0; j < 12; ++j) y[j] += __hip_atomic_load(rec + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 12; ++j) y[j] = d.y[base + j];
    }
  }
  double s = 0, acc = 0, sg = 0;
  if (in && lane < 12) {
    const size_t idx = 12 * (size_t)c + lane;
    s = binv_row12(d.binv + 144 * (size_t)c + 12 * lane, y);
    acc = mode == 0 ? s : d.accum[idx] + s;
    sg = d.sigma[idx];
  }
  if (done) return;
  cam_tail<12, K9_CAMS * 64>(d, c, lane, in, s, acc, s * sg, want_norms, sh);
}

// K9' + K11': tmp11 = B^-1 y11, accum11 (+)= tmp11, z = sigma * (N_c tmp11)
// (right_mul_b_inv_joint + loop body of solve_joint, linearization_power_varproj.hpp:246-257, 342-360).
// mode 0: y11 = -b11; 1: y12 = sigma * sum of scatter items, y11 = N^T y12; 2: y12 = dense d.y (all-reduced)
POVAR_KERNEL __launch_bounds__(K9_CAMS * 64) void cam_binv_axpy_h(Dp d, int mode, int want_norms, const double* ncw) {
  if (mode != 0 && d.flags[1]) return;
  __shared__ double sh[K9_CAMS * 2];
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * K9_CAMS + (threadIdx.x >> 6);
  const bool in = c < d.n_cams;
  double y11[11];
#pragma unroll
  for (int j = 0; j < 11; ++j) y11[j] = 0;
  const double* w = ncw + 13 * (size_t)(in ? c : 0);
  if (in) {
    if (mode == 0) {
#pragma unroll
      for (int j = 0; j < 11; ++j) y11[j] = -d.b[11 * (size_t)c + j];
    } else {
      double y[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) y[j] = 0;
      if (mode == 1) {
        camera_item_sum(d, c, lane, y);
#pragma unroll
        for (int j = 0; j < 12; ++j) y[j] *= d.sigma[12 * (size_t)c + j];
      } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) y[j] = d.y[12 * (size_t)c + j];
      }
      nt_apply(w, w[12], y, y11);
    }
  }
  double s = 0, acc = 0;
  if (in && lane < 11) {
    s = binv_row11(d.binv + 144 * (size_t)c + 11 * lane, y11);
    acc = mode == 0 ? s : d.accum[11 * (size_t)c + lane] + s;
  }
  const double zv = nc_z_entry(lane, s, w, d.sigma + 12 * (size_t)(in ? c : 0));
  if (in && lane < 12 && mode == 2) d.y[12 * (size_t)c + lane] = 0;
  cam_tail<11, K9_CAMS * 64>(d, c, lane, in, s, acc, zv, want_norms, sh);
}

}  // namespace povar
