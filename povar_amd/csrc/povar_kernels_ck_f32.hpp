// povar_kernels_ck_f32.hpp -- gfx950 device code of the single-precision step-1 term (POVAR_FLAG_FP32_TERMS): the camera-chunk
// form of right_mul_e0_pOSE (linearization_power_varproj.hpp:364-406) of povar_kernels_ck.hpp with its per-observation
// arithmetic, its landmark slots and its camera records in fp32.
//
// What stays in fp64 (include/povar_hip.h states the contract): every sum across chunks of a camera -- the chunk's register sum
// is widened to fp64 before the segmented wavefront sum, the workgroup accumulators in LDS add doubles (ds_add_f64), the
// partial records and q of the cold view are the doubles the per-camera kernel behind e0_ck reads -- and with them B^-1, the
// running sum x and the z the per-camera kernel hands over (Dp::zimg, converted to fp32 where a chunk gathers it).  So the
// per-camera kernels of the term loop (povar_kernels_cam.hpp: cam_cold_sum_binv, cam_cold_sum + the exchange of a sharded context + cam_binv_axpy)
// run unchanged behind this kernel.
//
// What halves: the landmark slots in LDS (h~ and u / g: 12 + 12 bytes instead of 24 + 24; u accumulates with ds_add_f32),
// the landmark records read per batch (36 instead of 72 bytes: ck32_records), the P part of the camera record (48 instead
// of 96 bytes), the image points of rows that do not pack (float2, 8 instead of 16 bytes), and the vector work per row:
// the forward and backward arithmetic of an observation issues fp32 instructions, whose rate is twice fp64's.
#pragma once

#include "povar_kernels_ck.hpp"

namespace povar {

constexpr int CK32_NW = 16;  // wavefronts per workgroup: the layout is cut for variant 1 (16 wavefronts, one group)
constexpr int CK32_SD = 2;   // rows in flight ahead of the one being worked on

// the fp32 operands of the kernel
struct Ck32 {
  const float2* uv;    // [rows][64] image points where the rows do not pack; nullptr: packed rows (CkP::uv, int2 micro-units)
  const float* lmrec;  // [lpl tiles][9][64] h~ (3) and G (6) of every landmark lane (ck32_records, after every prepare)
  const float* pimg;   // [n_cams][12] by rank: P3 row-major (9), then the translation column (3) (ck32_records)
  unsigned uv_bytes;   // bytes of the row array the kernel reads (8 per entry: packed int2 or float2)
  unsigned part_bytes; // bytes of the partial records (checked against 2^31 by povar_create)
};

__host__ __device__ inline size_t ck32_lds_bytes(int slots, int n_acc) {
  return 16 + (size_t)slots * 24 + (size_t)n_acc * CK_ACC_STRIDE * 8 + 64;
}

struct Ck32Obs {
  float w, cu, cv, cuv;
  __device__ inline void set(float sb2, float2 uv, float w_) {
    w = w_;
    cu = sb2 * uv.x;
    cv = sb2 * uv.y;
    cuv = sb2 * (uv.x * uv.x + uv.y * uv.y);
  }
};

// ck_huber_w in fp32: the weight at the linearisation point from P = [P3 | t], the landmark and the image point
__device__ inline float ck32_huber_w(float sb2, float sa2, float t, const float* P, float hx, float hy, float hz, float2 uv) {
  const float p0 = P[0] * hx + P[1] * hy + P[2] * hz + P[9];
  const float p1 = P[3] * hx + P[4] * hy + P[5] * hz + P[10];
  const float p2 = P[6] * hx + P[7] * hy + P[8] * hz + P[11];
  const float a = p0 - uv.x * p2, b = p1 - uv.y * p2, c = p0 - uv.x, e = p1 - uv.y;
  const float r2 = sb2 * (a * a + b * b) + sa2 * (c * c + e * e);
  float y = __builtin_amdgcn_rsqf(r2);  // (about 1 ulp; one Newton step)
  y = y * __builtin_fmaf(-0.5f * r2 * y, y, 1.5f);
  return r2 < t * t ? 1.0f : t * y;
}

// (the rows: Ck32Stream, povar_kernels_ck_parts.hpp -- float2 image points or the packed words through CkRows::uv)
struct Ck32Scal {
  float sb2, sa2, huber;
};

// one observation forward: u_l += P3^T (w C (Z h~_l))
template <bool ROBUST>
__device__ inline void ck32_obs_forward(const Ck32Scal& sc, float2 uv, const float* zz, const float* P, const float* lh, float* lu,
                                        uint32_t s) {
  const float hx = lh[s], hy = lh[s + 1], hz = lh[s + 2];  // (s = 3 x slot: ck_layout.hpp)
  const float rw = ROBUST ? ck32_huber_w(sc.sb2, sc.sa2, sc.huber, P, hx, hy, hz, uv) : 1.0f;
  Ck32Obs o;
  o.set(sc.sb2, uv, rw);
  const float d0 = hx * zz[0] + hy * zz[1] + hz * zz[2] + zz[3];
  const float d1 = hx * zz[4] + hy * zz[5] + hz * zz[6] + zz[7];
  const float d2 = hx * zz[8] + hy * zz[9] + hz * zz[10] + zz[11];
  const float a0 = o.w * (d0 - o.cu * d2);
  const float a1 = o.w * (d1 - o.cv * d2);
  const float a2 = o.w * (o.cuv * d2 - o.cu * d0 - o.cv * d1);
  __hip_atomic_fetch_add(lu + s, P[0] * a0 + P[3] * a1 + P[6] * a2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(lu + s + 1, P[1] * a0 + P[4] * a1 + P[7] * a2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(lu + s + 2, P[2] * a0 + P[5] * a1 + P[8] * a2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// one observation backward: q = w C (P3 g_l); returns the landmark in h
template <bool ROBUST>
__device__ inline void ck32_obs_backward(const Ck32Scal& sc, float2 uv, const float* P, const float* lh, const float* lg, uint32_t s,
                                         float* h, float* q) {
  h[0] = lh[s]; h[1] = lh[s + 1]; h[2] = lh[s + 2];
  const float rw = ROBUST ? ck32_huber_w(sc.sb2, sc.sa2, sc.huber, P, h[0], h[1], h[2], uv) : 1.0f;
  Ck32Obs o;
  o.set(sc.sb2, uv, rw);
  const float g0 = lg[s], g1 = lg[s + 1], g2 = lg[s + 2];
  const float e0 = P[0] * g0 + P[1] * g1 + P[2] * g2;
  const float e1 = P[3] * g0 + P[4] * g1 + P[5] * g2;
  const float e2 = P[6] * g0 + P[7] * g1 + P[8] * g2;
  q[0] = o.w * (e0 - o.cu * e2);
  q[1] = o.w * (e1 - o.cv * e2);
  q[2] = o.w * (o.cuv * e2 - o.cu * e0 - o.cv * e1);
}

template <int D, bool ROBUST, bool PK>
__device__ inline void ck32_forward_rows(const Ck32Scal& sc, const CkRows& R, Ck32Stream<D, PK>& st, int row0, int li0, int h, int lane,
                                         const float* zz, const float* P, const float* lh, float* lu) {
  ck_walk_rows<D, 1>(h, [&](int j, int i) {
    const float2 uv = st.uv[i];
    const uint32_t s = ck_slot(st.w[i], j);
    st.load(R, row0, li0, j + D, h, lane, i);
    if (s != CK_NONE) ck32_obs_forward<ROBUST>(sc, uv, zz, P, lh, lu, s);
  });
}

template <int D, bool ROBUST, bool PK>
__device__ inline void ck32_backward_rows(const Ck32Scal& sc, const CkRows& R, Ck32Stream<D, PK>& st, int row0, int li0, int h, int lane,
                                          const float* P, const float* lh, const float* lg, float* y) {
  ck_walk_rows<D, -1>(h, [&](int j, int i) {
    const float2 uv = st.uv[i];
    const uint32_t s = ck_slot(st.w[i], j);
    st.load(R, row0, li0, j - D, h, lane, i);
    if (s != CK_NONE) {
      float hh[3], q[3];
      ck32_obs_backward<ROBUST>(sc, uv, P, lh, lg, s, hh, q);
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        y[4 * m] += hh[0] * q[m];
        y[4 * m + 1] += hh[1] * q[m];
        y[4 * m + 2] += hh[2] * q[m];
        y[4 * m + 3] += q[m];
      }
    }
  });
}

// the way back over a tile with lanes of cameras WITHOUT an accumulator slot that leave q in the cold view (ck_backward_rows_cold):
// rows read where they are used, q stored as the fp64 double4 the per-camera kernel reads
template <bool PK>
__device__ inline void ck32_backward_rows_cold(const Ck32Scal& sc, const CkP& k, const CkRows& R, int row0, int li0, int h, int lane,
                                               const float* P, const float* lh, const float* lg, bool cold_lane, float* y) {
  for (int j = h - 1; j >= 0; --j) {
    Ck32Stream<1, PK> one;
    one.load(R, row0, li0, j, h, lane, 0);
    const int cp = cold_lane ? k.cpos[(size_t)(row0 + j) * WAVE + lane] : -1;
    const uint32_t s = ck_slot(one.w[0], j);
    if (s != CK_NONE) {
      float hh[3], q[3];
      ck32_obs_backward<false>(sc, one.uv[0], P, lh, lg, s, hh, q);
      if (cp >= 0) {
        k.q4c[cp] = make_double4(q[0], q[1], q[2], 0.0);
      } else {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          y[4 * m] += hh[0] * q[m];
          y[4 * m + 1] += hh[1] * q[m];
          y[4 * m + 2] += hh[2] * q[m];
          y[4 * m + 3] += q[m];
        }
      }
    }
  }
}

// the camera record of a lane in fp32: Z from the fp64 z image the per-camera kernel has just written (ck_load_z_img), P3 and
// the translation from the fp32 image of the linearisation point (three 16-byte loads)
__device__ inline void ck32_load_z(const Dp& d, int rank, float* zz) {
  double z[12];
  ck_load_z_img(d, rank, z);
#pragma unroll
  for (int e = 0; e < 12; ++e) zz[e] = (float)z[e];
}
template <bool ROBUST>
__device__ inline void ck32_load_p(const Ck32& f, int rank, float* P) {
  const float4* r = reinterpret_cast<const float4*>(f.pimg + (size_t)rank * 12);
#pragma unroll
  for (int j = 0; j < (ROBUST ? 3 : 2); ++j) {
    const float4 v = r[j];
    P[4 * j] = v.x; P[4 * j + 1] = v.y; P[4 * j + 2] = v.z; P[4 * j + 3] = v.w;
  }
  if (!ROBUST) P[8] = f.pimg[(size_t)rank * 12 + 8];
}

// The fp32 term kernel: the phases of e0_ck (one group of CK32_NW wavefronts): per landmark batch, load h~ -> forward over the
// wavefront's chunk tiles -> g = G u per landmark slot -> backward over the same tiles in reverse; then the workgroup's
// accumulators -> partial records.  The tile walk is e0_ck's (tile_of: rounds of alternating direction over the wavefronts).
template <bool ROBUST, bool PK>
__global__ __launch_bounds__(CK32_NW * 64) void e0_ck_f32(Dp d, CkP k, Ck32 f, double* part_out) {
  constexpr int NW = CK32_NW, SD = CK32_SD;
  const int done = d.flags[1];
  extern __shared__ double ck_lds[];
  const int S = k.slots;
  const int lane0 = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* lh = reinterpret_cast<float*>(ck_lds + 2);  // [S][3] landmark coordinates of the batch
  float* lu = lh + 3 * S;                            // [S][3] u = Jl^T Jp x, then g = G u
  double* acc = ck_lds + 2 + (size_t)3 * S;          // [n_acc][13] per-camera accumulators of the workgroup (fp64)
  const V2& v = d.v2;
  const int cam0 = v.wg_cam_off[blockIdx.x];
  const int n_acc = v.wg_cam_off[blockIdx.x + 1] - cam0;
  const int t0 = __builtin_amdgcn_readfirstlane(v.wg_tile_off[blockIdx.x]);
  const int t1 = __builtin_amdgcn_readfirstlane(v.wg_tile_off[blockIdx.x + 1]);
  if (done) return;  // wave-uniform, before any barrier and any side effect
  CkRows R;
  R.uv = __builtin_amdgcn_make_buffer_rsrc(PK ? (void*)k.uv : (void*)f.uv, 0, f.uv_bytes, 0x00020000);
  R.li = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(k.li), 0, k.li_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t PR = __builtin_amdgcn_make_buffer_rsrc(part_out, 0, f.part_bytes, 0x00020000);
  const Ck32Scal sc{(float)(d.sb * d.sb), (float)(d.sa * d.sa), (float)d.huber};
  const int wave_t = (wave & ~3) | (((wave >> 2) & 1) ? 3 - (wave & 3) : (wave & 3));
  auto tile_of = [&](int tb0, int q) { return tb0 + q * NW + ((q & 1) ? NW - 1 - wave_t : wave_t); };
  for (int i = threadIdx.x; i < n_acc * CK_ACC_STRIDE; i += NW * 64) acc[i] = 0;
  for (int b = 0; b < k.nb; ++b) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int tb0 = __builtin_amdgcn_readfirstlane(k.bt_off[blockIdx.x * k.nb + b]);
    const int tb1 = __builtin_amdgcn_readfirstlane(k.bt_off[blockIdx.x * k.nb + b + 1]);
    // ---- landmark coordinates of the batch into LDS, u = 0
    for (int m = wave; t0 + b + k.nb * m < t1; m += NW) {
      const float* rp = f.lmrec + ((size_t)(t0 + b + k.nb * m) * 9) * WAVE + lane;
      const int s = m * WAVE + lane;
      lh[3 * s] = rp[0];
      lh[3 * s + 1] = rp[WAVE];
      lh[3 * s + 2] = rp[2 * WAVE];
      lu[3 * s] = 0;
      lu[3 * s + 1] = 0;
      lu[3 * s + 2] = 0;
    }
    ck_barrier();  // (the accumulators' zeros of the first batch too)
    // ---- forward
    int q_t = 0;
    for (int t = tile_of(tb0, 0); t < tb1; t = tile_of(tb0, ++q_t)) {
      const CkTile tl = CkTile::of(k.tile[t]);
      const int rank = CkLaneMeta::rank_of(k, t, lane);
      const int rk = rank < 0 ? 0 : rank;
      float zz[12], P[12];
      ck32_load_p<ROBUST>(f, rk, P);
      Ck32Stream<SD, PK> st;
      st.template start<1>(R, tl.row0, tl.li0, tl.h, lane);
      ck32_load_z(d, rk, zz);
      ck32_forward_rows<SD, ROBUST, PK>(sc, R, st, tl.row0, tl.li0, tl.h, lane, zz, P, lh, lu);
    }
    ck_barrier();
    // ---- g = G u per landmark slot
    asm volatile("" : "+v"(lane));
    for (int m = wave; t0 + b + k.nb * m < t1; m += NW) {
      const float* rp = f.lmrec + ((size_t)(t0 + b + k.nb * m) * 9 + 3) * WAVE + lane;
      const float g0 = rp[0], g1 = rp[WAVE], g2 = rp[2 * WAVE], g3 = rp[3 * WAVE], g4 = rp[4 * WAVE], g5 = rp[5 * WAVE];
      const int s = m * WAVE + lane;
      const float u0 = lu[3 * s], u1 = lu[3 * s + 1], u2 = lu[3 * s + 2];
      lu[3 * s] = g0 * u0 + g1 * u1 + g2 * u2;
      lu[3 * s + 1] = g1 * u0 + g3 * u1 + g4 * u2;
      lu[3 * s + 2] = g2 * u0 + g4 * u1 + g5 * u2;
    }
    ck_barrier();
    // ---- backward: the wavefront's tiles in reverse
    for (int q = q_t - 1; q >= 0; --q) {
      const int t = tile_of(tb0, q);
      const CkTile tl = CkTile::of(k.tile[t]);
      const CkLaneMeta me = CkLaneMeta::load(k, t, lane);
      const int rank = me.rank, seg = me.seg, acc_slot = me.acc;
      float P[12];
      ck32_load_p<ROBUST>(f, rank < 0 ? 0 : rank, P);
      float y[12];
#pragma unroll
      for (int m = 0; m < 12; ++m) y[m] = 0;
      // (2 = CK_FLAG_COLD; as in e0_ck, not with a robust norm: the layout keeps the records for those)
      const bool cold_q = !ROBUST && k.cpos != nullptr && (tl.fl & 2) != 0;
      if (cold_q) {
        ck32_backward_rows_cold<PK>(sc, k, R, tl.row0, tl.li0, tl.h, lane, P, lh, lu, rank >= 0 && acc_slot < 0, y);
      } else {
        Ck32Stream<SD, PK> st;
        st.template start<-1>(R, tl.row0, tl.li0, tl.h, lane);
        ck32_backward_rows<SD, ROBUST, PK>(sc, R, st, tl.row0, tl.li0, tl.h, lane, P, lh, lu, y);
      }
      // the chunk's sum leaves fp32 here: lanes of one camera are summed in fp64, then its accumulator or its own record
      double yd[12];
#pragma unroll
      for (int m = 0; m < 12; ++m) yd[m] = (double)y[m];
      if (tl.fl & 1) seg_scan_steps<12>(yd, lane, seg & 255, 4);  // (inclusive scan: the run's total is in its LAST lane)
      if (rank >= 0) {
        if (acc_slot >= 0) {
          if (lane == ((seg >> 8) & 255)) {
#pragma unroll
            for (int m = 0; m < 12; ++m)
              __hip_atomic_fetch_add(acc + acc_slot * CK_ACC_STRIDE + m, yd[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        } else if (!cold_q) {
          const unsigned o = (unsigned)(~acc_slot) * 96u;  // (< part_bytes <= 2^31: povar_create; the descriptor drops the rest)
#pragma unroll
          for (int m = 0; m < 6; ++m) ck_store_part(PR, o + 16u * m, yd[2 * m], yd[2 * m + 1]);
        }
      }
    }
    ck_barrier();  // the next batch overwrites h~ and u; after the last one: the accumulators are complete
  }
  if (k.nb == 0) ck_barrier();
  // ---- accumulators -> this workgroup's partial records (camera-major in part_out)
  ck_store_accumulators<NW>(PR, k, cam0, n_acc, acc);
  if (d.p2p_epoch && blockIdx.x == 0 && threadIdx.x == 0) *d.p2p_epoch += 1;  // one tick per term (as e0_ck)
}

// the fp32 operands of a prepared system: the landmark records of prepare_lpl (V2::lmrec, [lpl tiles][9][64] of step 1) and the
// static part of the camera records (Dp::hot_rec entries 12..23 by rank: build_hot_rec)
POVAR_KERNEL __launch_bounds__(256) void ck32_records(const double* lmrec, float* lmrec32, int64_t n_rec, const double* hot_rec,
                                                      float* pimg, int n_cams) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_rec) lmrec32[i] = (float)lmrec[i];
  if (i < (int64_t)n_cams * 12) pimg[i] = (float)hot_rec[(i / 12) * HOT_REC_STRIDE + 12 + i % 12];
}

}  // namespace povar
