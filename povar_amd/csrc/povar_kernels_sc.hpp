// povar_kernels_sc.hpp -- the explicit-Schur-complement solvers of the reference's LinearizorSC
// (solver/linearizor_sc.cpp): --solver-type-step-1 PCG | CHOLESKY and --solver-type-step-2 RIPCG.
//
// The reference materialises the reduced camera matrix S = (Hpp + lambda I) - E0 as a hash map of
// 12x12 (11x11) blocks (cg/block_sparse_matrix.hpp:66-69, filled by add_Hb_pOSE / add_Hb_joint,
// sc/landmark_block.hpp:360-472, under an n_cams^2 mutex array) and runs a Ceres-style
// preconditioned CG on it (cg/conjugate_gradient.hpp:112-470) with the Schur-Jacobi preconditioner
// = inverse of the diagonal blocks of S (cg/preconditioner.hpp:66-135).  Here the operator is
// applied matrix-free -- S p = B p - E0 p with the same per-term E0 kernels the power series uses
// -- and only the block diagonal of S is formed:
//     S_cc = sigma ( sum_obs  T_i (x) h_i h_i^T ) sigma + lambda I,
//     T_i  = w C_i - w^2 C_i (P3 s Hll^-1 s P3^T) C_i          (step 1; C, P3 as in E0Core)
//     T_i  = w Dm_i^T (I_2 - Jl3_i Hll^-1 Jl3_i^T) Dm_i        (step 2; Dm = [[D00,0,D02],[0,D00,D12]])
// i.e. sixty moments per camera (3x3 symmetric T times the 10 entries of h h^T) next to the forty
// Gram moments of Hpp.  CHOLESKY assembles the dense upper triangle of S with the same closed forms.
#pragma once
#include "../../include/povar_hip.h"
#include "povar_kernels_joint.hpp"

namespace povar {

// device pointers of the explicit-SC solvers (allocated on first use)
struct ScP {
  double* dm_part;   // [n_items][60] per-item moments of the E0 block diagonal
  double* dm;        // [n_cams][60]
  double* bmat;      // [n_cams][144] B_c = Hpp_c + lambda I, dim x dim row-major
  double* minv;      // [n_cams][144] Schur-Jacobi preconditioner S_cc^-1, dim x dim row-major
  double* x;         // PCG vectors, [dim * n_cams] each
  double* r;
  double* p;
  double* q;
  double* zv;
  double* part;      // [n_cam_blocks][4] per-workgroup partial dot products
  double* s;         // scalars, PS_*
  const double* ncw; // step 2: Householder vector (12) + beta of every camera's tangent basis
};
enum { PS_RHO = 0, PS_BETA, PS_PQ, PS_ALPHA, PS_Q0, PS_Q1, PS_NORM_R, PS_NORM_B, PS_ZETA, PS_COUNT = 16 };

__device__ inline int sym6(int a, int b) {  // index of (a,b) in the packed upper 3x3
  if (a > b) { const int t = a; a = b; b = t; }
  return a * 3 - (a * (a - 1)) / 2 + (b - a);
}

// ------------------------------------------------------------------------------------------
// block diagonal of E0: per-item moments  sum_obs K_i (x) h_i h_i^T,
// K_i = Jp-structure^T (Jl_i Hll^-1 Jl_i^T) Jp-structure (3x3 symmetric), camera-major, one
// wavefront per item, fixed order (the i == j terms of landmark_block.hpp:388-399 / 452-463)
// ------------------------------------------------------------------------------------------
template <bool HOM>
__global__ __launch_bounds__(256) void cm_gram_sc(Dp d, double* part) {
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (item >= d.n_items) return;
  const int b = d.item_off[item], e = d.item_off[item + 1];
  const Cam P = load_cam(d.cams_lin4, d.item_cam[item]);
  double acc[60];
#pragma unroll
  for (int k = 0; k < 60; ++k) acc[k] = 0;
  for (int p = b + lane; p < e; p += WAVE) {
    const double sw = d.robust ? d.sw[d.cm_slot[p]] : 1.0;
    const double w = sw * sw;
    const double2 uv = d.cm_uv[p];
    const int lm = d.cm_lm[p];
    double K[6], hv[4];
    if (HOM) {
      const double4* rec = reinterpret_cast<const double4*>(d.lmrec) + 4 * (size_t)lm;
      const double4 X = rec[0], s = rec[1], r2 = rec[2], r3 = rec[3];
      const double Hi[9] = {r2.x, r2.y, r2.z, r2.y, r2.w, r3.x, r2.z, r3.x, r3.y};
      const Hom h = hom_project(P, X, uv.x, uv.y);
      double jl4[8], jl3[6], hw[4], beta;
      hom_jl4(P, h, sw, s, jl4);
      house4(X, hw, beta);
      jl3_of_jl4(jl4, hw, beta, jl3);
      double V[6];  // Jl3 Hll^-1 (2x3)
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[3 * r + j] = jl3[3 * r] * Hi[j] + jl3[3 * r + 1] * Hi[3 + j] + jl3[3 * r + 2] * Hi[6 + j];
      const double W00 = V[0] * jl3[0] + V[1] * jl3[1] + V[2] * jl3[2];
      const double W01 = V[0] * jl3[3] + V[1] * jl3[4] + V[2] * jl3[5];
      const double W11 = V[3] * jl3[3] + V[4] * jl3[4] + V[5] * jl3[5];
      const double a = h.D00, b2 = h.D02, c2 = h.D12;
      K[0] = w * a * a * W00;
      K[1] = w * a * a * W01;
      K[2] = w * a * (b2 * W00 + c2 * W01);
      K[3] = w * a * a * W11;
      K[4] = w * a * (b2 * W01 + c2 * W11);
      K[5] = w * (b2 * b2 * W00 + 2.0 * b2 * c2 * W01 + c2 * c2 * W11);
      hv[0] = X.x; hv[1] = X.y; hv[2] = X.z; hv[3] = X.w;
    } else {
      const double4* rec = reinterpret_cast<const double4*>(d.lmrec) + 3 * (size_t)lm;
      const double4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
      const double s[3] = {r0.w, r1.x, r1.y};
      const double Hi[9] = {r1.z, r1.w, r2.x, r1.w, r2.y, r2.z, r2.x, r2.z, r2.w};
      const double P3[9] = {P.r0.x, P.r0.y, P.r0.z, P.r1.x, P.r1.y, P.r1.z, P.r2.x, P.r2.y, P.r2.z};
      double M[9], MH[9], A[9];  // M = P3 diag(s), A = M Hll^-1 M^T
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = P3[3 * i + j] * s[j];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) MH[3 * i + j] = M[3 * i] * Hi[j] + M[3 * i + 1] * Hi[3 + j] + M[3 * i + 2] * Hi[6 + j];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[3 * i + j] = MH[3 * i] * M[3 * j] + MH[3 * i + 1] * M[3 * j + 1] + MH[3 * i + 2] * M[3 * j + 2];
      const double sb2 = d.sb * d.sb;
      const double cu = sb2 * uv.x, cv = sb2 * uv.y, cuv = sb2 * (uv.x * uv.x + uv.y * uv.y);
      const double C[9] = {1, 0, -cu, 0, 1, -cv, -cu, -cv, cuv};
      double CA[9];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) CA[3 * i + j] = C[3 * i] * A[j] + C[3 * i + 1] * A[3 + j] + C[3 * i + 2] * A[6 + j];
      const double w2 = w * w;
      int k = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) K[k++] = w2 * (CA[3 * i] * C[j] + CA[3 * i + 1] * C[3 + j] + CA[3 * i + 2] * C[6 + j]);
      hv[0] = r0.x; hv[1] = r0.y; hv[2] = r0.z; hv[3] = 1.0;
    }
    const double hh[10] = {hv[0] * hv[0], hv[0] * hv[1], hv[0] * hv[2], hv[0] * hv[3], hv[1] * hv[1],
                           hv[1] * hv[2], hv[1] * hv[3], hv[2] * hv[2], hv[2] * hv[3], hv[3] * hv[3]};
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int j = 0; j < 10; ++j) acc[10 * k + j] += K[k] * hh[j];
  }
  wave_sum<60>(acc);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 60; ++k) part[60 * (size_t)item + k] = acc[k];
  }
}

// dm[c] = sum of the camera's item moments, fixed order: 16 wavefronts stride over the items (a hub
// camera of venice-1778 has ~800 of them), then a fixed-order sum of the 16 partials
POVAR_KERNEL __launch_bounds__(1024) void cam_sum_parts60(Dp d, const double* part, double* dm) {
  __shared__ double sh[16][60];
  const int c = blockIdx.x, e = threadIdx.x & 63, q = threadIdx.x >> 6;
  if (e < 60) {
    double s = 0;
    for (int it = d.cam_item_off[c] + q; it < d.cam_item_off[c + 1]; it += 16) s += part[60 * (size_t)it + e];
    sh[q][e] = s;
  }
  __syncthreads();
  if (threadIdx.x < 60) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += sh[k][threadIdx.x];
    dm[60 * (size_t)c + threadIdx.x] = s;
  }
}

// Per camera: A = sigma (Hpp-moments [- E0-diagonal moments]) sigma, projected on the tangent space
// in step 2 (N_c^T A N_c), + lambda I.  out_mat receives A (dim x dim row-major), out_inv its
// inverse by Cholesky of the upper triangle (preconditioner.hpp:104-107 / LPV:145-148).
// One thread per camera, matrices in LDS [element][thread] like cam_build_binv.
// fixed[c] != 0 (povar_set_fixed_cameras): out_inv's block is zero -- PCG then iterates on the free cameras' system alone;
// out_mat (B_c) is what it always is.
constexpr int K8_SC_THREADS = 32;  // one thread per camera (explicit-SC path: not tuned further)
template <bool HOM>
__global__ __launch_bounds__(K8_SC_THREADS) void cam_build_sc(Dp d, double lambda, const double* ncw, const double* dm,
                                                           double* out_inv, double* out_mat, const uint8_t* fixed) {
  __shared__ double A[144 * K8_SC_THREADS];
  __shared__ double X[144 * K8_SC_THREADS];
  const int t = threadIdx.x;
  const int c = blockIdx.x * K8_SC_THREADS + t;
  if (c >= d.n_cams) return;
  constexpr int DIM = HOM ? 11 : 12;
#define A_(i, j) A[((i) * 12 + (j)) * K8_SC_THREADS + t]
#define X_(i, j) X[((i) * 12 + (j)) * K8_SC_THREADS + t]
  const double* g = d.G + 40 * (size_t)c;
  const double* sg = d.sigma + 12 * (size_t)c;
  const double sb2 = d.sb * d.sb;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
          const int ij = sym10(i, j);
          double v;
          if (HOM) {
            if (a == b) v = a < 2 ? g[ij] : g[30 + ij];
            else if (a + b == 1) v = 0;
            else v = g[10 * ((a == 2 ? b : a) + 1) + ij];
          } else {
            if (a == b) v = a < 2 ? g[ij] : sb2 * g[30 + ij];
            else if (a + b == 1) v = 0;
            else v = -sb2 * g[10 * ((a == 2 ? b : a) + 1) + ij];
          }
          if (dm) v -= dm[60 * (size_t)c + 10 * sym6(a, b) + ij];
          A_(4 * a + i, 4 * b + j) = v * sg[4 * a + i] * sg[4 * b + j];
        }
  if (HOM) {
    const double* w = ncw + 13 * (size_t)c;
    const double beta = w[12];
    // T = A N (12 x 11) into X, then N^T T (11 x 11) back into A (row stride kept at 12)
    for (int i = 0; i < 12; ++i) {
      double aw = 0;
      for (int k = 0; k < 12; ++k) aw += A_(i, k) * w[k];
      for (int j = 0; j < 11; ++j) X_(i, j) = A_(i, j + 1) - beta * aw * w[j + 1];
    }
    for (int j = 0; j < 11; ++j) {
      double wt = 0;
      for (int k = 0; k < 12; ++k) wt += w[k] * X_(k, j);
      for (int i = 0; i < 11; ++i) A_(i, j) = X_(i + 1, j) - beta * w[i + 1] * wt;
    }
  }
  for (int j = 0; j < DIM; ++j) A_(j, j) += lambda;
  if (out_mat) {
    double* o = out_mat + 144 * (size_t)c;
    for (int i = 0; i < DIM; ++i)
      for (int j = 0; j < DIM; ++j) o[DIM * i + j] = A_(i, j);
  }
  if (out_inv && fixed[c] != 0) {
    double* o = out_inv + 144 * (size_t)c;
    for (int e = 0; e < DIM * DIM; ++e) o[e] = 0.0;
  } else if (out_inv) {
    for (int j = 0; j < DIM; ++j) {
      double dd = A_(j, j);
      for (int k = 0; k < j; ++k) dd -= A_(j, k) * A_(j, k);
      dd = sqrt(dd);
      A_(j, j) = dd;
      for (int i = j + 1; i < DIM; ++i) {
        double s = A_(j, i);
        for (int k = 0; k < j; ++k) s -= A_(i, k) * A_(j, k);
        A_(i, j) = s / dd;
      }
    }
    for (int col = 0; col < DIM; ++col) {
      for (int i = 0; i < DIM; ++i) {
        double s = (i == col) ? 1.0 : 0.0;
        for (int k = 0; k < i; ++k) s -= A_(i, k) * X_(k, col);
        X_(i, col) = s / A_(i, i);
      }
      for (int i = DIM - 1; i >= 0; --i) {
        double s = X_(i, col);
        for (int k = i + 1; k < DIM; ++k) s -= A_(k, i) * X_(k, col);
        X_(i, col) = s / A_(i, i);
      }
    }
    double* o = out_inv + 144 * (size_t)c;
    for (int i = 0; i < DIM; ++i)
      for (int j = 0; j < DIM; ++j) o[DIM * i + j] = X_(i, j);
  }
#undef A_
#undef X_
}

// ------------------------------------------------------------------------------------------
// PCG (conjugate_gradient.hpp:112-290 / 292-470, driven as linearizor_base.cpp:104-150):
// vectors are per-camera blocks of DIM doubles; one wavefront per camera, lane j < DIM owns
// component j; dot products go through per-workgroup partials and a one-wavefront scalar kernel,
// so the host reads one flag word per iteration.
// ------------------------------------------------------------------------------------------

// lane j < DIM: sum_k M[c][j][k] * v_k with v_k held by lane k
template <int DIM>
__device__ inline double block_row_times(const double* M, int c, int lane, double v) {
  double s = 0;
  const double* row = M + 144 * (size_t)c + DIM * (lane < DIM ? lane : 0);
#pragma unroll
  for (int k = 0; k < DIM; ++k) s += row[k] * shfl_d(v, k);
  return s;
}

// E0 input: z = sigma * v (step 1; plus v itself for the stored-tile forms) or sigma * (N_c v) (step 2)
// into the dense z + hot records
template <bool HOM>
__device__ inline void emit_z(const Dp& d, const double* ncw, int c, int lane, bool in, double v) {
  if (HOM) {
    const double* w = ncw + 13 * (size_t)(in ? c : 0);
    const double beta = w[12];
    double wt = (in && lane < 11) ? w[lane + 1] * v : 0.0;
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) wt += shfl_xor_d(wt, m);  // lanes 0..15 hold the 11 products
    const double prev = shfl_up_d(v, 1);
    if (in && lane < 12) {
      const double pa = (lane == 0 ? 0.0 : prev) - beta * w[lane] * wt;
      store_z(d, c, lane, pa * d.sigma[12 * (size_t)c + lane]);
    }
  } else {
    if (in && lane < 12) {
      store_z(d, c, lane, v * d.sigma[12 * (size_t)c + lane]);
      d.tmp[12 * (size_t)c + lane] = v;  // the stored-tile E0 forms take the unscaled vector (sigma is in the tile)
    }
  }
}

template <int N>
__device__ inline void store_partials(const ScP& s, double (&v)[N], double* sh) {
  block_sum<N, K9_CAMS * 64>(v, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) s.part[4 * (size_t)blockIdx.x + k] = v[k];
  }
}

// x = 0, r = b, z = M^-1 r; partials (x.(b+r) = 0, r.r, r.z)     (CG:146-147, 163, 168-176)
template <int DIM>
__global__ __launch_bounds__(K9_CAMS * 64) void pcg_init(Dp d, ScP s) {
  __shared__ double sh[K9_CAMS * 3];
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * K9_CAMS + (threadIdx.x >> 6);
  const bool in = c < d.n_cams, act = in && lane < DIM;
  const size_t idx = (size_t)DIM * (in ? c : 0) + (lane < DIM ? lane : 0);
  const double r = act ? d.b[idx] : 0.0;
  const double z = block_row_times<DIM>(s.minv, in ? c : 0, lane, r);
  double v[3] = {0, 0, 0};
  if (act) {
    s.x[idx] = 0;
    s.r[idx] = r;
    s.zv[idx] = z;
    v[1] = r * r;
    v[2] = r * z;
  }
  store_partials<3>(s, v, sh);
}

// end of iteration `it` (it == 0: after pcg_init): the termination tests of CG:243-301 and, when
// the loop goes on, rho / beta of the next iteration with their failure exits (CG:175-197)
POVAR_KERNEL __launch_bounds__(64) void pcg_check(Dp d, ScP s, int n_blocks, int it, int min_it, int max_it, double eta,
                                                double r_tol) {
  if (d.flags[1]) return;
  double v[3] = {0, 0, 0};
  for (int k = threadIdx.x; k < n_blocks; k += 64) {
    v[0] += s.part[4 * (size_t)k];
    v[1] += s.part[4 * (size_t)k + 1];
    v[2] += s.part[4 * (size_t)k + 2];
  }
  wave_sum<3>(v);
  if (threadIdx.x != 0) return;
  double* S = s.s;
  bool done = false;
  int status = POVAR_LINEAR_SOLVER_NO_CONVERGENCE, iters = it;
  const double norm_r = sqrt(v[1]);
  if (it == 0) {
    S[PS_NORM_B] = norm_r;
    S[PS_Q0] = 0.0;    // -x.(b + r) at x = 0
    S[PS_RHO] = 1.0;   // CG:160
    if (norm_r == 0.0) { done = true; status = POVAR_LINEAR_SOLVER_SUCCESS; }                        // CG:131-136
    else if (min_it == 0 && norm_r <= r_tol * norm_r) { done = true; status = POVAR_LINEAR_SOLVER_SUCCESS; }  // CG:149-158
  } else {
    const double q1 = -1.0 * v[0];
    const double zeta = it * (q1 - S[PS_Q0]) / q1;  // CG:268
    S[PS_Q1] = q1;
    S[PS_ZETA] = zeta;
    S[PS_NORM_R] = norm_r;
    if (zeta < eta && it >= min_it) { done = true; status = POVAR_LINEAR_SOLVER_SUCCESS; }            // CG:269-282
    else {
      S[PS_Q0] = q1;
      if (norm_r <= r_tol * S[PS_NORM_B] && it >= min_it) { done = true; status = POVAR_LINEAR_SOLVER_SUCCESS; }  // CG:288-297
      else if (it >= max_it) done = true;                                                            // CG:299-301
    }
  }
  if (!done) {
    const double last_rho = S[PS_RHO], rho = v[2];
    S[PS_RHO] = rho;
    if (rho == 0.0 || isinf(rho)) { done = true; status = POVAR_LINEAR_SOLVER_FAILURE; iters = it + 1; }  // CG:177-185
    else if (it >= 1) {
      const double beta = rho / last_rho;
      S[PS_BETA] = beta;
      if (beta == 0.0 || isinf(beta)) { done = true; status = POVAR_LINEAR_SOLVER_FAILURE; iters = it + 1; }  // CG:190-197
    }
  }
  if (done) {
    d.flags[1] = 1;
    d.flags[2] = iters;
    d.flags[3] = status;
  }
}

// p = z (first) or z + beta p; E0 input z-buffer = sigma * (N) p                       (CG:187-199)
template <int DIM, bool HOM>
__global__ __launch_bounds__(K9_CAMS * 64) void pcg_dir(Dp d, ScP s, int first) {
  if (d.flags[1]) return;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * K9_CAMS + (threadIdx.x >> 6);
  const bool in = c < d.n_cams, act = in && lane < DIM;
  const size_t idx = (size_t)DIM * (in ? c : 0) + (lane < DIM ? lane : 0);
  double p = 0;
  if (act) {
    p = first ? s.zv[idx] : s.zv[idx] + s.s[PS_BETA] * s.p[idx];
    s.p[idx] = p;
  }
  emit_z<HOM>(d, s.ncw, c, lane, in, p);
}

// res = B v - E0 v with E0 v in the dense ambient y (sigma applied); lane j < DIM gets component j
template <int DIM, bool HOM>
__device__ inline double schur_times(const Dp& d, const ScP& s, int c, int lane, bool in, double v) {
  const double bv = block_row_times<DIM>(s.bmat, in ? c : 0, lane, v);
  double e0;
  if (HOM) {
    double y[12], y11[11];
#pragma unroll
    for (int j = 0; j < 12; ++j) y[j] = d.y[12 * (size_t)(in ? c : 0) + j];
    nt_apply(s.ncw + 13 * (size_t)(in ? c : 0), s.ncw[13 * (size_t)(in ? c : 0) + 12], y, y11);
    e0 = 0;
#pragma unroll
    for (int j = 0; j < 11; ++j) e0 = (lane == j) ? y11[j] : e0;
  } else {
    e0 = d.y[12 * (size_t)(in ? c : 0) + (lane < 12 ? lane : 0)];
  }
  return bv - e0;
}

// q = S p, partial p.q                                                                    (CG:201-202)
template <int DIM, bool HOM>
__global__ __launch_bounds__(K9_CAMS * 64) void pcg_apply(Dp d, ScP s) {
  if (d.flags[1]) return;
  __shared__ double sh[K9_CAMS];
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * K9_CAMS + (threadIdx.x >> 6);
  const bool in = c < d.n_cams, act = in && lane < DIM;
  const size_t idx = (size_t)DIM * (in ? c : 0) + (lane < DIM ? lane : 0);
  const double p = act ? s.p[idx] : 0.0;
  const double q = schur_times<DIM, HOM>(d, s, c, lane, in, p);
  double v[1] = {0};
  if (act) {
    s.q[idx] = q;
    v[0] = p * q;
  }
  store_partials<1>(s, v, sh);
}

// alpha = rho / p.q with the exits of CG:204-223
POVAR_KERNEL __launch_bounds__(64) void pcg_alpha(Dp d, ScP s, int n_blocks, int it) {
  if (d.flags[1]) return;
  double v[1] = {0};
  for (int k = threadIdx.x; k < n_blocks; k += 64) v[0] += s.part[4 * (size_t)k];
  wave_sum<1>(v);
  if (threadIdx.x != 0) return;
  const double pq = v[0];
  s.s[PS_PQ] = pq;
  int status = -1;
  if (pq <= 0 || isinf(pq)) status = POVAR_LINEAR_SOLVER_NO_CONVERGENCE;  // "Matrix is indefinite" CG:204-215
  else {
    const double alpha = s.s[PS_RHO] / pq;
    s.s[PS_ALPHA] = alpha;
    if (isinf(alpha)) status = POVAR_LINEAR_SOLVER_FAILURE;  // CG:218-223
  }
  if (status >= 0) {
    d.flags[1] = 1;
    d.flags[2] = it;
    d.flags[3] = status;
  }
}

// x += alpha p.  reset == 0: r -= alpha q, z = M^-1 r and the partials of the iteration-end tests
// (CG:225, 237-239, 243, 286).  reset == 1 (every residual_reset_period-th iteration, CG:234-236):
// only x, and x goes to the E0 input so that pcg_residual can recompute r = b - S x.
template <int DIM, bool HOM>
__global__ __launch_bounds__(K9_CAMS * 64) void pcg_update(Dp d, ScP s, int reset) {
  if (d.flags[1]) return;
  __shared__ double sh[K9_CAMS * 3];
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * K9_CAMS + (threadIdx.x >> 6);
  const bool in = c < d.n_cams, act = in && lane < DIM;
  const size_t idx = (size_t)DIM * (in ? c : 0) + (lane < DIM ? lane : 0);
  const double alpha = s.s[PS_ALPHA];
  double x = 0, r = 0;
  if (act) {
    x = s.x[idx] + alpha * s.p[idx];
    s.x[idx] = x;
  }
  if (reset) {
    emit_z<HOM>(d, s.ncw, c, lane, in, x);
    return;
  }
  if (act) {
    r = s.r[idx] - alpha * s.q[idx];
    s.r[idx] = r;
  }
  const double z = block_row_times<DIM>(s.minv, in ? c : 0, lane, r);
  double v[3] = {0, 0, 0};
  if (act) {
    s.zv[idx] = z;
    v[0] = x * (d.b[idx] + r);
    v[1] = r * r;
    v[2] = r * z;
  }
  store_partials<3>(s, v, sh);
}

// r = b - S x after pcg_update(reset = 1) and E0 x; z = M^-1 r; iteration-end partials   (CG:234-236)
template <int DIM, bool HOM>
__global__ __launch_bounds__(K9_CAMS * 64) void pcg_residual(Dp d, ScP s) {
  if (d.flags[1]) return;
  __shared__ double sh[K9_CAMS * 3];
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * K9_CAMS + (threadIdx.x >> 6);
  const bool in = c < d.n_cams, act = in && lane < DIM;
  const size_t idx = (size_t)DIM * (in ? c : 0) + (lane < DIM ? lane : 0);
  const double x = act ? s.x[idx] : 0.0;
  const double sx = schur_times<DIM, HOM>(d, s, c, lane, in, x);
  const double bb = act ? d.b[idx] : 0.0;
  const double r = act ? bb - sx : 0.0;
  const double z = block_row_times<DIM>(s.minv, in ? c : 0, lane, r);
  double v[3] = {0, 0, 0};
  if (act) {
    s.r[idx] = r;
    s.zv[idx] = z;
    v[0] = x * (bb + r);
    v[1] = r * r;
    v[2] = r * z;
  }
  store_partials<3>(s, v, sh);
}

// inc = -x ("we solve H(-x) = b", linearizor_base.cpp:121-122) into the increment buffer
POVAR_KERNEL __launch_bounds__(256) void pcg_finish(const double* x, double* accum, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) accum[i] = -x[i];
}

// ------------------------------------------------------------------------------------------
// CHOLESKY (solve_direct_pOSE, sc/linearization_sc.hpp:236-245): dense S, row-major n x n with
// n = 12 n_cams; only the upper block triangle (camera_i <= camera_j) is formed, which is what the
// factorisation reads.  Off-diagonal part of add_Hb_pOSE (landmark_block.hpp:388-399) in closed form:
//     block(ci, cj) -= sigma_ci [ (F_i Hll^-1 F_j^T) (x) h h^T ] sigma_cj,   F_i = w_i C_i P3_i diag(s)
// One workgroup per landmark, observations staged 64 at a time in LDS, 16-lane groups take one
// camera pair each and add its 144 entries with fp64 atomics (hub cameras' blocks are shared by many
// landmarks).  S is the augmented row-major matrix of povar_kernels_chol.hpp (row stride ld).
// Every dense assembly kernel addresses the block of cameras (a, b) at (cam_row[a], cam_row[b]), the map of the step's matrix
// (povar_ctx::cam_row: dim c, or with povar_set_dense_compaction the rows of the free cameras and -1 for a fixed one), and skips
// a block with a member that is not in the matrix.
// The atomics land in arrival order, so this assembly is reproducible to rounding only; sc_dense_ordered below adds the same
// terms (ScdPose::term) in an order the layout fixes and is what a POVAR_FLAG_DETERMINISTIC context runs (povar_set_sc_assembly).
// ------------------------------------------------------------------------------------------
constexpr int SCD_CHUNK = 64;

// Whether any of the k observations from slot s0 on (one landmark's) has its camera in the dense matrix (cam_row[cam] >= 0,
// povar_set_dense_compaction): a landmark without one adds no block, and its workgroup returns before it stages anything.
// Uniform over the workgroup (every thread calls it).  The kernels ask only where the host says that some camera is out of the
// matrix (some_out): with every camera in it the walk could not end a workgroup and is not made.
__device__ inline bool scd_any_row(const Dp& d, const int* cam_row, int s0, int k) {
  int any = 0;
  for (int i = threadIdx.x; i < k; i += blockDim.x) any |= cam_row[d.cam[s0 + i]] >= 0;
  return __syncthreads_or(any) != 0;
}

struct ScdObs {
  double F[9], G[9];  // F_i and F_i Hll^-1
  int cam;
};
__device__ inline void scd_stage(const Dp& d, int slot, const double* s3, const double* Hi, ScdObs& o) {
  const int cam = d.cam[slot];
  const Cam P = load_cam(d.cams_lin4, cam);
  const double2 uv = d.uv[slot];
  const double sw = d.robust ? d.sw[slot] : 1.0;
  const double w = sw * sw;
  const double sb2 = d.sb * d.sb;
  const double cu = sb2 * uv.x, cv = sb2 * uv.y, cuv = sb2 * (uv.x * uv.x + uv.y * uv.y);
  const double C[9] = {1, 0, -cu, 0, 1, -cv, -cu, -cv, cuv};
  const double P3[9] = {P.r0.x, P.r0.y, P.r0.z, P.r1.x, P.r1.y, P.r1.z, P.r2.x, P.r2.y, P.r2.z};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o.F[3 * i + j] = w * (C[3 * i] * P3[j] + C[3 * i + 1] * P3[3 + j] + C[3 * i + 2] * P3[6 + j]) * s3[j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.G[3 * i + j] = o.F[3 * i] * Hi[j] + o.F[3 * i + 1] * Hi[3 + j] + o.F[3 * i + 2] * Hi[6 + j];
  o.cam = cam;
}

// ---- the two steps of the per-landmark dense kernels (sc_dense_offdiag[_h], and lm_cov / obs_cov of povar_kernels_cov.hpp):
// what a workgroup holds of its landmark (Head, by value: see LplWg), the one decode of the landmark record, the staging of
// an observation, the vectors u_a of an observation, the row of L_i and M_i of obs_cov.  Pieces, not a walker: the kernels keep
// their chunk loops, barriers, shuffles and pair arithmetic.  HOM and DIM also serve the host's dispatch (with_step, povar_sc.hip).
struct ScdPose {
  static constexpr int DIM = 12, CHUNK = SCD_CHUNK;
  static constexpr bool HOM = false;
  static constexpr int LM_STRIDE = 9;  // doubles per landmark block of lm_cov
  typedef ScdObs Obs;
  struct Head { double h[4], s4[4], Hi[9]; };  // (x, y, z, 1), the column scaling (s, 0), Hll^-1
  __device__ static __forceinline__ Head load(const Dp& d, int lm) {
    const double4* rec = reinterpret_cast<const double4*>(d.lmrec) + 3 * (size_t)lm;
    const double4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    return Head{{r0.x, r0.y, r0.z, 1.0}, {r0.w, r1.x, r1.y, 0.0}, {r1.z, r1.w, r2.x, r1.w, r2.y, r2.z, r2.x, r2.z, r2.w}};
  }
  __device__ static __forceinline__ void stage(const Dp& d, const double*, int slot, Head hd, Obs& o) {
    scd_stage(d, slot, hd.s4, hd.Hi, o);
  }
  // The term a pair of observations (a, b) of one landmark adds to entry (r, c) of the block (a.cam, b.cam) of S -- the one
  // expression of the atomic and the ordered assembly (sc_dense_offdiag, sc_dense_ordered) --, and what the entries of a pair
  // share (Pair).  h: the landmark's Head::h.
  struct Pair { const double *sgi, *sgj; };
  __device__ static __forceinline__ Pair pair(const Dp& d, const Obs& a, const Obs& b) {
    return Pair{d.sigma + 12 * (size_t)a.cam, d.sigma + 12 * (size_t)b.cam};
  }
  __device__ static __forceinline__ double term(const Pair& p, const Obs& oa, const Obs& ob, const double (&h)[4], int r, int c) {
    const int a = r >> 2, ii = r & 3, b = c >> 2, jj = c & 3;
    const double t = oa.G[3 * a] * ob.F[3 * b] + oa.G[3 * a + 1] * ob.F[3 * b + 1] + oa.G[3 * a + 2] * ob.F[3 * b + 2];
    return -t * h[ii] * h[jj] * p.sgi[r] * p.sgj[c];
  }
  // u[a] = entry r of u_a = sigma_c o (e_a (x) h).  h: the kernel's copy of Head::h (indexed at run time: not left in the Head)
  __device__ static inline void u(const Obs& o, const double* sigma, const double (&h)[4], int r, double (&u)[3]) {
    const double v = sigma[12 * (size_t)o.cam + r] * h[r & 3];
    u[0] = (r >> 2) == 0 ? v : 0.0;
    u[1] = (r >> 2) == 1 ? v : 0.0;
    u[2] = (r >> 2) == 2 ? v : 0.0;
  }
  // a row of L_i = P3 diag(s) from the row p4 of P_c
  __device__ static __forceinline__ void l_row(Head hd, const double (&p4)[4], double* L) {
#pragma unroll
    for (int y = 0; y < 3; ++y) L[y] = p4[y] * hd.s4[y];
  }
  // M_i = w C_i
  __device__ static __forceinline__ void gram_m(const Dp& d, const Cam&, Head, double2 uv, double w, double (&Mi)[9]) {
    const double sb2 = d.sb * d.sb;
    const double cu = sb2 * uv.x, cv = sb2 * uv.y, cuv = sb2 * (uv.x * uv.x + uv.y * uv.y);
    const double C9[9] = {1, 0, -cu, 0, 1, -cv, -cu, -cv, cuv};
#pragma unroll
    for (int e = 0; e < 9; ++e) Mi[e] = w * C9[e];
  }
  // A_i = sqrt(w) A(alpha, u, v), the RES x 3 weighted Jacobian of the residual with respect to y (A_i^T A_i = M_i), and the
  // weighted residual r_i = sqrt(w) (A y - (0, 0, sqrt(alpha) u, sqrt(alpha) v)) at y: the row of obs_hat
  static constexpr int RES = 4;
  __device__ static __forceinline__ void jac_a(const Dp& d, double2 uv, double sw, const double (&y)[3], double (&A)[12], double (&r)[4]) {
    const double wb = sw * d.sb, wa = sw * d.sa;
    const double a12[12] = {wb, 0, -(wb * uv.x), 0, wb, -(wb * uv.y), wa, 0, 0, 0, wa, 0};
#pragma unroll
    for (int e = 0; e < 12; ++e) A[e] = a12[e];
    r[0] = wb * (y[0] - uv.x * y[2]);
    r[1] = wb * (y[1] - uv.y * y[2]);
    r[2] = wa * (y[0] - uv.x);
    r[3] = wa * (y[1] - uv.y);
  }
};

POVAR_KERNEL __launch_bounds__(256) void sc_dense_offdiag(Dp d, const int* lm_slot0, const int* lm_cnt, const int* cam_row, int some_out,
                                                          double* S, int64_t ld) {
  __shared__ ScdObs oi[SCD_CHUNK], oj[SCD_CHUNK];
  const int lm = blockIdx.x;
  const int s0 = lm_slot0[lm], k = lm_cnt[lm];
  if (some_out && !scd_any_row(d, cam_row, s0, k)) return;
  const ScdPose::Head hd = ScdPose::load(d, lm);
  const double h[4] = {hd.h[0], hd.h[1], hd.h[2], hd.h[3]};  // (indexed at run time: not left inside the Head)
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
  for (int ic = 0; ic < k; ic += SCD_CHUNK) {
    const int ni = min(SCD_CHUNK, k - ic);
    __syncthreads();
    if ((int)threadIdx.x < ni) ScdPose::stage(d, nullptr, s0 + ic + threadIdx.x, hd, oi[threadIdx.x]);
    for (int jc = ic; jc < k; jc += SCD_CHUNK) {
      const int nj = min(SCD_CHUNK, k - jc);
      __syncthreads();
      if ((int)threadIdx.x < nj) ScdPose::stage(d, nullptr, s0 + jc + threadIdx.x, hd, oj[threadIdx.x]);
      __syncthreads();
      for (int pp = grp; pp < ni * nj; pp += 16) {
        const int i = pp / nj, j = pp - i * nj;
        if (ic == jc && i > j) continue;  // cameras ascend inside a landmark: keep camera_i <= camera_j
        const int ri = cam_row[oi[i].cam], rj = cam_row[oj[j].cam];
        if ((ri | rj) < 0) continue;  // a camera that is not in the matrix: no block
        const ScdPose::Pair pr = ScdPose::pair(d, oi[i], oj[j]);
        for (int e = gl; e < 144; e += 16) {
          const int r = e / 12, c = e - 12 * r;
          atomicAdd(S + ((int64_t)ri + r) * ld + (int64_t)rj + c, ScdPose::term(pr, oi[i], oj[j], h, r, c));
        }
      }
    }
  }
}

// S_cc += B_c = Hpp_c + lambda I (landmark_block.hpp:381-384 + linearization_sc.hpp:477-481; step 2: its tangent
// projection, cam_build_sc<true>'s out_mat) and the right-hand side -b into column N of the augmented matrix
// (povar_kernels_chol.hpp).  DIM = 12 (step 1) or 11 (step 2): B_c is DIM x DIM row-major at stride 144.
// WITH_B = false: the right-hand side alone (the ordered assembly adds B_c itself, without an atomic).
template <int DIM, bool WITH_B = true>
__global__ __launch_bounds__(256) void sc_dense_diag(Dp d, const double* bmat, const int* cam_row, double* S, int64_t ld, int N) {
  const int c = blockIdx.x, e = threadIdx.x;
  const int64_t r0 = cam_row[c];  // the camera's rows in the matrix (< 0: it is not in it)
  if (r0 < 0) return;
  if (WITH_B && e < DIM * DIM) {
    const int r = e / DIM, cc = e - DIM * r;
    atomicAdd(S + (r0 + r) * ld + r0 + cc, bmat[144 * (size_t)c + e]);
  }
  if (e < DIM) S[(r0 + e) * ld + N] = -d.b[DIM * (size_t)c + e];
}

// ------------------------------------------------------------------------------------------
// RICHOLESKY (step 2; the reference has no direct solve of the joint system): the dense S of the 11 n_cams tangent
// system in the same augmented layout, S = (N_c^T sigma Hpp sigma N_c + lambda I) - N_c^T sigma E0 sigma N_c.
// Off-diagonal and E0-diagonal part of add_Hb_joint (landmark_block.hpp:452-463) in closed form: with
//     F_i = sw_i Dm_i^T Jl3_i  (3 x 3; Dm = [[D00,0,D02],[0,D00,D12]], Jl3 = sw (D P) diag(s) N_l as cm_gram_sc<true>)
// the ambient 12 x 12 block of a pair of observations of one landmark is  -(F_i Hll^-1 F_j^T) (x) X X^T  between
// sigma_ci and sigma_cj, i.e.  -sum_ab T_ab u_a v_b^T  with T = F_i Hll^-1 F_j^T, u_a = sigma_ci o (e_a (x) X),
// v_b = sigma_cj o (e_b (x) X).  The tangent projection acts on the vectors, N_ci^T u_a and N_cj^T v_b, so each
// observation's three projected 11-vectors are formed once while it is staged and a pair costs 121 entries of a 3 x 3
// bilinear form; the reflector stays out of the pair loop.  The i == j terms are the E0 part of the diagonal block
// (what cm_gram_sc<true> + cam_build_sc<true> subtract for the preconditioner); B_c comes from sc_dense_diag<11>.
// Workgroup per landmark, chunks of 32 staged observations (two arrays: 26 KB of LDS), a 16-lane group per camera
// pair, camera_i <= camera_j only, fp64 atomics as in step 1 (so this assembly is not bit-reproducible either; the ordered one,
// sc_dense_ordered<ScdJoint>, adds the same ScdJoint::term in a fixed order).
// ------------------------------------------------------------------------------------------
constexpr int SCDH_CHUNK = 32;
struct ScdObsH {
  double U[33];       // N_c^T (sigma_c o (e_a (x) X)), a = 0..2: 11 entries each
  double F[9], G[9];  // F_i and F_i Hll^-1
  int cam;
};
static_assert(2 * SCDH_CHUNK * sizeof(ScdObsH) < 64 * 1024, "sc_dense_offdiag_h: static LDS");

__device__ inline void scdh_stage(const Dp& d, const double* ncw, int slot, const double4& X, const double4& s,
                                  const double* Hi, const double (&hw)[4], double hbeta, ScdObsH& o) {
  const int cam = d.cam[slot];
  const Cam P = load_cam(d.cams_lin4, cam);
  const double2 uv = d.uv[slot];
  const double sw = d.robust ? d.sw[slot] : 1.0;
  const Hom h = hom_project(P, X, uv.x, uv.y);
  double jl4[8], jl3[6];
  hom_jl4(P, h, sw, s, jl4);
  jl3_of_jl4(jl4, hw, hbeta, jl3);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o.F[j] = sw * h.D00 * jl3[j];
    o.F[3 + j] = sw * h.D00 * jl3[3 + j];
    o.F[6 + j] = sw * (h.D02 * jl3[j] + h.D12 * jl3[3 + j]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o.G[3 * i + j] = o.F[3 * i] * Hi[j] + o.F[3 * i + 1] * Hi[3 + j] + o.F[3 * i + 2] * Hi[6 + j];
  const double* w = ncw + 13 * (size_t)cam;
  const double beta = w[12];
  const double* sg = d.sigma + 12 * (size_t)cam;
  const double xs[4] = {X.x, X.y, X.z, X.w};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double v[4], wv = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = sg[4 * a + k] * xs[k];
      wv += w[4 * a + k] * v[k];
    }
#pragma unroll
    for (int j = 0; j < 11; ++j) {  // (N^T v)_j = v_{j+1} - beta w_{j+1} (w . v)
      const int i = j + 1;
      const double e = (i >= 4 * a && i < 4 * a + 4) ? v[i - 4 * a] : 0.0;
      o.U[11 * a + j] = e - beta * w[i] * wv;
    }
  }
  o.cam = cam;
}

struct ScdJoint {
  static constexpr int DIM = 11, CHUNK = SCDH_CHUNK;
  static constexpr bool HOM = true;
  static constexpr int LM_STRIDE = 16;
  typedef ScdObsH Obs;
  // X and s as the record holds them and as arrays, the damped tangent Hll^-1, the reflector of N_l (house4)
  struct Head {
    double h[4], s4[4], Hi[9], hw[4], hbeta;
    double4 X, s;
  };
  // (the landmark record povar_prepare_joint(lambda) leaves: X, s, damped tangent Hll^-1 -- as cm_gram_sc<true> reads it)
  __device__ static __forceinline__ Head load(const Dp& d, int lm) {
    const double4* rec = reinterpret_cast<const double4*>(d.lmrec) + 4 * (size_t)lm;
    const double4 X = rec[0], s = rec[1], r2 = rec[2], r3 = rec[3];
    Head hd{{X.x, X.y, X.z, X.w}, {s.x, s.y, s.z, s.w}, {r2.x, r2.y, r2.z, r2.y, r2.w, r3.x, r2.z, r3.x, r3.y}, {0, 0, 0, 0}, 0, X, s};
    house4(X, hd.hw, hd.hbeta);
    return hd;
  }
  __device__ static __forceinline__ void stage(const Dp& d, const double* ncw, int slot, Head hd, Obs& o) {
    scdh_stage(d, ncw, slot, hd.X, hd.s, hd.Hi, hd.hw, hd.hbeta, o);
  }
  // as ScdPose::pair / term: T = F_a Hll^-1 F_b^T is what the 121 entries share; entry (r, c) is -sum_pq U_a[p][r] T_pq U_b[q][c]
  struct Pair { double T[9]; };
  __device__ static __forceinline__ Pair pair(const Dp&, const Obs& a, const Obs& b) {
    Pair p;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int q = 0; q < 3; ++q) p.T[3 * i + q] = a.G[3 * i] * b.F[3 * q] + a.G[3 * i + 1] * b.F[3 * q + 1] + a.G[3 * i + 2] * b.F[3 * q + 2];
    return p;
  }
  __device__ static __forceinline__ double term(const Pair& p, const Obs& a, const Obs& b, const double (&)[4], int r, int c) {
    const double* T = p.T;
    const double v0 = b.U[c], v1 = b.U[11 + c], v2 = b.U[22 + c];
    const double t = a.U[r] * (T[0] * v0 + T[1] * v1 + T[2] * v2) + a.U[11 + r] * (T[3] * v0 + T[4] * v1 + T[5] * v2) +
                     a.U[22 + r] * (T[6] * v0 + T[7] * v1 + T[8] * v2);
    return -t;
  }
  // u[a] = entry r of u_a = N_c^T (sigma_c o (e_a (x) X)): the staged U
  __device__ static inline void u(const Obs& o, const double*, const double (&)[4], int r, double (&u)[3]) {
    u[0] = o.U[r];
    u[1] = o.U[11 + r];
    u[2] = o.U[22 + r];
  }
  // a row of L_i = P diag(s4) N_l, N_l = (I - beta w w^T)[:, 1:]
  __device__ static __forceinline__ void l_row(Head hd, const double (&p4)[4], double* L) {
    const double q4[4] = {p4[0] * hd.s4[0], p4[1] * hd.s4[1], p4[2] * hd.s4[2], p4[3] * hd.s4[3]};
    const double aw = q4[0] * hd.hw[0] + q4[1] * hd.hw[1] + q4[2] * hd.hw[2] + q4[3] * hd.hw[3];
#pragma unroll
    for (int y = 0; y < 3; ++y) L[y] = q4[y + 1] - hd.hbeta * aw * hd.hw[y + 1];
  }
  // M_i = w Dm^T Dm
  __device__ static __forceinline__ void gram_m(const Dp&, const Cam& P, Head hd, double2 uv, double w, double (&Mi)[9]) {
    const Hom hp = hom_project(P, hd.X, uv.x, uv.y);
    const double m9[9] = {hp.D00 * hp.D00, 0, hp.D00 * hp.D02, 0, hp.D00 * hp.D00, hp.D00 * hp.D12,
                          hp.D00 * hp.D02, hp.D00 * hp.D12, hp.D02 * hp.D02 + hp.D12 * hp.D12};
#pragma unroll
    for (int e = 0; e < 9; ++e) Mi[e] = w * m9[e];
  }
  // A_i = sqrt(w) d(y0 / y2, y1 / y2) / dy (2 x 3; A_i^T A_i = M_i) and r_i = sqrt(w) ((y0 / y2, y1 / y2) - (u, v)) at y: the row
  // of obs_hat.  One division, as obs_cov's row; y2 = 0 leaves both non-finite.
  static constexpr int RES = 2;
  __device__ static __forceinline__ void jac_a(const Dp&, double2 uv, double sw, const double (&y)[3], double (&A)[6], double (&r)[2]) {
    const double iz = 1.0 / y[2];
    const double px = y[0] * iz, py = y[1] * iz, wz = sw * iz;
    const double a6[6] = {wz, 0, -(wz * px), 0, wz, -(wz * py)};
#pragma unroll
    for (int e = 0; e < 6; ++e) A[e] = a6[e];
    r[0] = sw * (px - uv.x);
    r[1] = sw * (py - uv.y);
  }
};

POVAR_KERNEL __launch_bounds__(256) void sc_dense_offdiag_h(Dp d, const double* ncw, const int* lm_slot0, const int* lm_cnt,
                                                            const int* cam_row, int some_out, double* S, int64_t ld) {
  __shared__ ScdObsH oi[SCDH_CHUNK], oj[SCDH_CHUNK];
  const int lm = blockIdx.x;
  const int s0 = lm_slot0[lm], k = lm_cnt[lm];
  if (some_out && !scd_any_row(d, cam_row, s0, k)) return;
  const ScdJoint::Head hd = ScdJoint::load(d, lm);
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
  for (int ic = 0; ic < k; ic += SCDH_CHUNK) {
    const int ni = min(SCDH_CHUNK, k - ic);
    __syncthreads();
    if ((int)threadIdx.x < ni) ScdJoint::stage(d, ncw, s0 + ic + threadIdx.x, hd, oi[threadIdx.x]);
    for (int jc = ic; jc < k; jc += SCDH_CHUNK) {
      const int nj = min(SCDH_CHUNK, k - jc);
      __syncthreads();
      if ((int)threadIdx.x < nj) ScdJoint::stage(d, ncw, s0 + jc + threadIdx.x, hd, oj[threadIdx.x]);
      __syncthreads();
      for (int pp = grp; pp < ni * nj; pp += 16) {
        const int i = pp / nj, j = pp - i * nj;
        if (ic == jc && i > j) continue;  // cameras ascend inside a landmark: keep camera_i <= camera_j
        const ScdObsH& a = oi[i];
        const ScdObsH& b = oj[j];
        const int ri = cam_row[a.cam], rj = cam_row[b.cam];
        if ((ri | rj) < 0) continue;  // a camera that is not in the matrix: no block
        const ScdJoint::Pair pr = ScdJoint::pair(d, a, b);  // F_i Hll^-1 F_j^T
        double* blk = S + (int64_t)ri * ld + (int64_t)rj;
        for (int e = gl; e < 121; e += 16) {
          const int r = e / 11, c = e - 11 * r;
          atomicAdd(blk + r * ld + c, ScdJoint::term(pr, a, b, hd.h, r, c));
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Ordered dense assembly (povar_set_sc_assembly; the assembly of a POVAR_FLAG_DETERMINISTIC context): the same terms as
// sc_dense_offdiag[_h] (Step::stage, Step::pair, Step::term) and B_c, added without a floating-point atomic in an order that is a
// function of the context's layout alone, into the same block triangle camera_i <= camera_j; no buffer beside S.
//   ownership  a workgroup owns the blocks (ci, cj) of one row camera ci and SCO_T consecutive column cameras cj >= ci, as
//              accumulators in LDS.  A wavefront owns the columns with col % SCO_WAVES == its number, a lane the entries
//              e % 64 == its number of each: every entry has one thread from the first add to the store.
//   walk       ci's observations in the context's camera-major order (cam_item_off -> item_off -> cm_slot / cm_lm), SCO_WALK
//              at a time, one per thread: the partners of an observation are the slots of its landmark from its own on
//              (cameras ascend inside a landmark: two searches in Dp::cam give those inside the tile; its own slot is the
//              i == j term of the diagonal block).  An exclusive prefix sum over the counts -- integers: exact in any order --
//              numbers the pairs: by observation in camera-major order, then by column.
//   windows    SCO_PAIRS pairs at a time are staged (one wavefront the own observations, one the partners; every staging
//              thread decodes its landmark's record itself) and, after a barrier, every wavefront goes through the window in
//              order and adds the pairs of its columns.  The order of the terms of an entry is therefore the camera-major order
//              of ci's observations, whatever the timing, the number of CUs or the order of the workgroups.
//   write-out  B_c once per entry of the diagonal block (bmat: rank 0 only), then S += accumulator with plain loads and stores
//              (S holds zeros, or Q Q^T of the free gauge); columns no term touched are left alone.
// grid = n_cams * ceil(n_cams / SCO_T); the row cameras in popularity order (Dp::hot_cams: the long walks first); a workgroup
// whose tile lies left of the diagonal, or whose row camera is not in the matrix (cam_row), returns at once; a column camera that
// is not in it loses its accumulator at the write-out, so every other entry keeps its additions and their order.  On a sharded context the camera-major arrays hold the shard's
// observations: every rank adds its part in its order and the all-reduce sums the parts.
// ------------------------------------------------------------------------------------------
constexpr int SCO_T = 32, SCO_WALK = 256, SCO_WAVES = SCO_WALK / 64, SCO_PAIRS = 32;

// the first index in [lo, hi) whose camera is >= v (hi: none); cameras ascend over the slots of a landmark
__device__ inline int sco_lower(const int* cam, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cam[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <class Step>
__global__ __launch_bounds__(SCO_WALK) void sc_dense_ordered(Dp d, const double* ncw, const double* bmat, const int* cam_row, double* S,
                                                            int64_t ld) {
  constexpr int DIM = Step::DIM, DD = DIM * DIM;
  typedef typename Step::Obs Obs;
  __shared__ double acc[SCO_T * DD];
  __shared__ Obs oi[SCO_PAIRS], oj[SCO_PAIRS];
  __shared__ double hh[SCO_PAIRS][4];  // Head::h of every staged pair's landmark
  __shared__ int pre[SCO_WALK], own[SCO_WALK], first[SCO_WALK], wsum[SCO_WAVES];
  static_assert(sizeof(double) * SCO_T * DD + 2 * SCO_PAIRS * sizeof(Obs) + sizeof(double) * 4 * SCO_PAIRS +
                        sizeof(int) * (3 * SCO_WALK + SCO_WAVES) <= 64 * 1024, "sc_dense_ordered: static LDS");
  static_assert(SCO_T <= 32 && 2 * 64 <= SCO_WALK && SCO_PAIRS <= 64, "sc_dense_ordered: the touched mask, the two staging wavefronts");
  const int n_tiles = (d.n_cams + SCO_T - 1) / SCO_T;
  const int ci = d.hot_cams[blockIdx.x / n_tiles];
  const int t0 = SCO_T * (int)(blockIdx.x % n_tiles);
  if (t0 + SCO_T <= ci) return;
  const int64_t row_i = cam_row[ci];  // a row camera that is not in the matrix owns no block
  if (row_i < 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int col = wave; col < SCO_T; col += SCO_WAVES)
    for (int e = lane; e < DD; e += 64) acc[col * DD + e] = 0.0;
  unsigned touched = 0;  // (the same in every lane of a wavefront)
  const int pb = d.item_off[d.cam_item_off[ci]], pe = d.item_off[d.cam_item_off[ci + 1]];
  for (int p0 = pb; p0 < pe; p0 += SCO_WALK) {
    int s = 0, f = 0, n = 0;
    if (p0 + tid < pe) {
      s = d.cm_slot[p0 + tid];
      const int lm = d.cm_lm[p0 + tid];
      const int end = d.lm_slot0[lm] + d.lm_cnt[lm];
      f = sco_lower(d.cam, s, end, t0);
      n = sco_lower(d.cam, f, end, t0 + SCO_T) - f;
    }
    int inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    own[tid] = s;
    first[tid] = f;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCO_WAVES; ++w) {
      if (w < wave) base += wsum[w];
      total += wsum[w];
    }
    pre[tid] = base + inc - n;
    __syncthreads();
    for (int g0 = 0; g0 < total; g0 += SCO_PAIRS) {
      const int np = min(SCO_PAIRS, total - g0);
      if (g0 > 0) __syncthreads();  // (the window before has been added)
      if (wave < 2 && lane < np) {
        const int g = g0 + lane;
        int lo = 0, hi = SCO_WALK;  // the last observation whose first pair is <= g: the one pair g belongs to
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (pre[mid] <= g) lo = mid;
          else hi = mid;
        }
        const int slot = wave == 0 ? own[lo] : first[lo] + (g - pre[lo]);
        const typename Step::Head hd = Step::load(d, d.lm[slot]);
        Step::stage(d, ncw, slot, hd, wave == 0 ? oi[lane] : oj[lane]);
        if (wave == 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k) hh[lane][k] = hd.h[k];
        }
      }
      __syncthreads();
      for (int q = 0; q < np; ++q) {
        const int col = oj[q].cam - t0;
        if ((col & (SCO_WAVES - 1)) != wave) continue;
        const typename Step::Pair pr = Step::pair(d, oi[q], oj[q]);
        for (int e = lane; e < DD; e += 64) {
          const int r = e / DIM, c = e - DIM * r;
          acc[col * DD + e] += Step::term(pr, oi[q], oj[q], hh[q], r, c);
        }
        touched |= 1u << col;
      }
    }
  }
  if (bmat && ci >= t0 && ((ci - t0) & (SCO_WAVES - 1)) == wave) {  // the tile that holds the diagonal block (ci < t0 + SCO_T here)
    for (int e = lane; e < DD; e += 64) acc[(ci - t0) * DD + e] += bmat[144 * (size_t)ci + e];
    touched |= 1u << (ci - t0);
  }
  for (int col = wave; col < SCO_T; col += SCO_WAVES) {
    if (!((touched >> col) & 1u)) continue;
    const int row_j = cam_row[t0 + col];  // (touched: t0 + col < n_cams)
    if (row_j < 0) continue;  // a column camera that is not in the matrix: its terms are dropped here, the others' order is kept
    double* blk = S + row_i * ld + row_j;
    for (int e = lane; e < DD; e += 64) {
      const int r = e / DIM, c = e - DIM * r;
      blk[r * ld + c] += acc[col * DD + e];
    }
  }
}

// povar_right_mul_e0_joint: z = sigma (N_c x) of a caller's tangent vector (one wavefront per camera, as pcg_dir) ...
POVAR_KERNEL __launch_bounds__(K9_CAMS * 64) void sc_emit_z_h(Dp d, const double* ncw, const double* x) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * K9_CAMS + (threadIdx.x >> 6);
  const bool in = c < d.n_cams;
  const double v = (in && lane < 11) ? x[11 * (size_t)c + lane] : 0.0;
  emit_z<true>(d, ncw, c, lane, in, v);
}
// ... and out11 = N_c^T y of the dense ambient y (sigma applied) that E0 left
POVAR_KERNEL __launch_bounds__(256) void sc_project_y_h(Dp d, const double* ncw, double* out11) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d.n_cams) return;
  double y[12], o[11];
#pragma unroll
  for (int j = 0; j < 12; ++j) y[j] = d.y[12 * (size_t)c + j];
  nt_apply(ncw + 13 * (size_t)c, ncw[13 * (size_t)c + 12], y, o);
#pragma unroll
  for (int j = 0; j < 11; ++j) out11[11 * (size_t)c + j] = o[j];
}

}  // namespace povar
