// povar_kernels_cov.hpp -- marginal camera covariance from the dense factor (povar_camera_covariance_pose / _joint;
// the reference has no counterpart).  run_cholesky's assembly and factorisation leave the upper factor R (A = R^T R,
// layout of povar_kernels_chol.hpp) in the augmented matrix M; the diagonal blocks of A^-1 = W W^T with W = R^-1 are
//   cov_add_qqt    A += Q Q^T on the upper block triangle (free gauge: Q an orthonormal basis of the gauge null space)
//   cov_diag_scan  max_k A_kk before and min_k R_kk^2 after the factorisation (the pivot rule of the free gauge)
//   cov_diag_inv   W_jj = R_jj^-1 of a 64 x 64 diagonal block          one wavefront, row c of W_jj in lane c
//   cov_trmm       T = R[0:j, j] W_jj into the scratch panel, then W[0:j, j] = -W[0:j, 0:j] T      64 x 64 tiles, MFMA
//   cov_gram       block c = sum_k W[J, k] W[J, k]^T over the camera's rows J                       workgroup per camera
//   cov_finish     - Q_J Q_J^T, then the map to camera coordinates (D T D, or D N_c T N_c^T D with the reflector)
// W overwrites R in place, block column by block column from the left: when column j is formed, W[0:j, 0:j] is final
// (the leading block of the inverse of a triangular matrix is the inverse of its leading block) and R[0:j, j] is still
// untouched.  cov_trmm is the n^3/3 part and runs on v_mfma_f64_16x16x4_f64 with the fragment layout of chol_syrk.
#pragma once
#include "povar_kernels_chol.hpp"

namespace povar {

constexpr int CV_ALDS = 66;  // LDS row stride (doubles) of the A tile, read down its columns: lanes (l & 15, l >> 4) of
                             // a 32-lane half land on 2 (l & 15) + (l >> 4) mod 32: 32 different bank pairs

// A[i][j] += sum_k Q[i][k] Q[j][k] on the 64 x 64 tiles of the upper block triangle, rows / columns < n.  Q is n x nq
// row-major.  Launched on rank 0 only, before the all-reduce (the rule of sc_dense_diag).  grid = (N / 64, N / 64).
POVAR_KERNEL __launch_bounds__(256) void cov_add_qqt(double* M, int64_t ld, int n, const double* Q, int nq) {
  const int it = blockIdx.y, jt = blockIdx.x;
  if (jt < it) return;
  for (int e = threadIdx.x; e < CH_NB * CH_NB; e += 256) {
    const int i = it * CH_NB + (e >> 6), j = jt * CH_NB + (e & 63);
    if (i >= n || j >= n) continue;
    const double* qi = Q + (size_t)i * nq;
    const double* qj = Q + (size_t)j * nq;
    double s = 0;
    for (int k = 0; k < nq; ++k) s += qi[k] * qj[k];
    M[(int64_t)i * ld + j] += s;
  }
}

// out[which] = max_k M_kk (which = 0: the diagonal of A, before the factorisation) or min_k M_kk^2 (which = 1: the
// pivots R_kk^2, after it) over k < n.  One workgroup.
POVAR_KERNEL __launch_bounds__(256) void cov_diag_scan(const double* M, int64_t ld, int n, int which, double* out) {
  __shared__ double sh[256];
  double v = which == 0 ? -INFINITY : INFINITY;
  for (int k = threadIdx.x; k < n; k += 256) {
    const double a = M[(int64_t)k * ld + k];
    v = which == 0 ? fmax(v, a) : fmin(v, a * a);
  }
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = which == 0 ? fmax(sh[threadIdx.x], sh[threadIdx.x + s]) : fmin(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[which] = sh[0];
}

// W_jj = R_jj^-1 of the 64 x 64 upper triangular block at (k0, k0), in place.  One wavefront; lane c forms row c of
// W_jj from W R = I, left to right: W[c][j] = -(sum_{p < j} W[c][p] R[p][j]) / R[j][j].  Every lane reads the same
// R[p][j] (an LDS broadcast), the row stays in registers.
POVAR_KERNEL __launch_bounds__(64) void cov_diag_inv(double* M, int64_t ld, int k0) {
  __shared__ double R[CH_NB][CH_NB + 1];
  const int c = threadIdx.x;
  double* blk = M + (int64_t)k0 * ld + k0;
  for (int r = 0; r < CH_NB; ++r) R[r][c] = blk[(int64_t)r * ld + c];
  __syncthreads();
  double w[CH_NB];
#pragma unroll
  for (int j = 0; j < CH_NB; ++j) {
    double s = 0;
#pragma unroll
    for (int p = 0; p < j; ++p) s += w[p] * R[p][j];  // (w[p] = 0 for p < c)
    const double d = R[j][j];
    w[j] = j == c ? 1.0 / d : (j > c ? -s / d : 0.0);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CH_NB; ++j) R[c][j] = w[j];
  __syncthreads();
  for (int r = 0; r < CH_NB; ++r) blk[(int64_t)r * ld + c] = R[r][c];
}

// C_i = alpha * sum_{kb = k_first .. k_end - 1} A[i][kb] B[kb] for block row i = blockIdx.x: A[i][kb] the 64 x 64 block
// of the row-major A at rows 64 i, columns 64 kb; B[kb] the 64 x 64 block of the 64-column panel B at rows 64 kb;
// k_first = i when `tri` (A upper block triangular), else 0.  The two products of a block column j:
//   T = R[0:j, j] W_jj            A = M + 64 j (one block per row), B = the diagonal block, C = the scratch panel
//   W[0:j, j] = -W[0:j, 0:j] T    A = M (tri), B = the scratch panel, C = M + 64 j
// The second product never reads what another workgroup writes: it reads columns < 64 j of M and the scratch panel
// and writes column block j only -- the N x 64 scratch panel is what keeps R[0:j, j] readable until every row is done.
// 4 wavefronts, each a 32 x 32 quadrant = 2 x 2 MFMA tiles; fragments as chol_syrk, with A held row-major in LDS:
// A (16x4): lane l holds A[i + (l & 15)][kk + (l >> 4)], B (4x16): B[kk + (l >> 4)][j + (l & 15)].
// 73 KiB of static LDS (As 64 x 66, Bs 64 x 80 doubles: chol_syrk's B stride, the only one under 96 that keeps the two
// rows of a 32-lane half on different banks): within gfx950's 160 KiB per workgroup, two workgroups per CU, as chol_syrk's 80.
POVAR_KERNEL __launch_bounds__(256) void cov_trmm(const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                                                  int64_t ldc, int tri, int k_end, double alpha) {
  __shared__ double As[CH_NB][CV_ALDS];
  __shared__ double Bs[CH_NB][CH_LDS];
  const int i = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wi = (w >> 1) * 32, wj = (w & 1) * 32;
  const int lr = lane >> 4, lc = lane & 15;
  ch_d4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = ch_d4{0, 0, 0, 0};
  const double* arow = A + (int64_t)i * CH_NB * lda;
  // software pipeline, as chol_syrk_outer: the global loads of block kb + 1 are in flight while the MFMAs of block kb run
  constexpr int NLD = CH_NB * CH_NB / 2 / 256;  // double2 per thread and operand
  double2 ra[NLD], rb[NLD];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = threadIdx.x + 256 * u;
      const int p = e >> 5, q = (e & 31) * 2;
      ra[u] = *reinterpret_cast<const double2*>(arow + (int64_t)p * lda + (int64_t)kb * CH_NB + q);
      rb[u] = *reinterpret_cast<const double2*>(B + ((int64_t)kb * CH_NB + p) * ldb + q);
    }
  };
  const int k_first = tri ? i : 0;  // (< k_end: the launches cover block rows above the diagonal block only)
  fetch(k_first);
  for (int kb = k_first; kb < k_end; ++kb) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = threadIdx.x + 256 * u;
      const int p = e >> 5, q = (e & 31) * 2;
      As[p][q] = ra[u].x; As[p][q + 1] = ra[u].y;
      Bs[p][q] = rb[u].x; Bs[p][q + 1] = rb[u].y;
    }
    __syncthreads();
    if (kb + 1 < k_end) fetch(kb + 1);
#pragma unroll 4
    for (int kk = 0; kk < CH_NB; kk += 4) {
      const double a0 = As[wi + lc][kk + lr], a1 = As[wi + 16 + lc][kk + lr];
      const double b0 = Bs[kk + lr][wj + lc], b1 = Bs[kk + lr][wj + 16 + lc];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
  double* crow = C + (int64_t)i * CH_NB * ldc;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        crow[(int64_t)(wi + 16 * x + lr + 4 * r) * ldc + wj + 16 * y + lc] = alpha * acc[x][y][r];
}

// Solver-coordinate block of camera c: T[a][b] = sum_k W[J_a][k] W[J_b][k], J_a = DIM c + a, over the columns
// k < n (the padding columns of these rows are zero: they contribute nothing).  W is upper triangular, but below the
// diagonal M still holds what the assembly left there (a camera block that straddles a 64-panel edge), so entries with
// k < row are masked, not read.  One workgroup per camera: thread t walks columns DIM c + t, + 256, ... (coalesced row
// reads), keeps the DIM (DIM + 1) / 2 products of the upper triangle, one deterministic workgroup sum, mirrored on
// the way out so the block is symmetric bit for bit.  out: DIM x DIM row-major at stride 144.
template <int DIM>
__global__ __launch_bounds__(256) void cov_gram(const double* M, int64_t ld, int n, double* out) {
  constexpr int NP = DIM * (DIM + 1) / 2;
  __shared__ double sh[4 * NP];
  const int c = blockIdx.x;
  const int r0 = DIM * c;
  double acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0;
  for (int k = r0 + threadIdx.x; k < n; k += 256) {
    double v[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) v[a] = k >= r0 + a ? M[(int64_t)(r0 + a) * ld + k] : 0.0;
    int p = 0;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int b = a; b < DIM; ++b) acc[p++] += v[a] * v[b];
  }
  block_sum<NP, 256>(acc, sh);
  int p = 0;
#pragma unroll
  for (int a = 0; a < DIM; ++a)
#pragma unroll
    for (int b = a; b < DIM; ++b, ++p)
      if ((int)threadIdx.x == p) {
        out[144 * (size_t)c + DIM * a + b] = acc[p];
        out[144 * (size_t)c + DIM * b + a] = acc[p];
      }
}

// Last step, per camera (one workgroup of 256): T -= Q_J Q_J^T (free gauge; nq = 0 otherwise), then
//   coords = 1 (solver):  T as it is, DIM x DIM;
//   coords = 0 (camera):  the block carried through the map cam_apply_inc / cam_apply_inc_h apply to an increment,
//                         12 x 12: DIM = 12: D T D, D = diag(sigma_c);  DIM = 11: D N_c T N_c^T D with
//                         N_c = (I - beta w w^T)[:, 1:] from ncw = (w[12], beta).
// One thread per entry of the upper triangle, mirrored, so the result is symmetric bit for bit.  In place on `blk`
// (stride 144 per camera).
template <int DIM>
__global__ __launch_bounds__(256) void cov_finish(double* blk, const double* Q, int nq, const double* sigma, const double* ncw,
                                                  int coords) {
  __shared__ double T[DIM][DIM];
  __shared__ double Nm[12][DIM];
  const int c = blockIdx.x, t = threadIdx.x;
  double* o = blk + 144 * (size_t)c;
  if (t < DIM * DIM) {
    const int a = t / DIM, b = t - DIM * a;
    if (a <= b) {
      const double* qa = Q + (size_t)(DIM * c + a) * nq;
      const double* qb = Q + (size_t)(DIM * c + b) * nq;
      double s = 0;
      for (int k = 0; k < nq; ++k) s += qa[k] * qb[k];
      const double v = o[DIM * a + b] - s;
      T[a][b] = v;
      T[b][a] = v;
    }
  }
  if (DIM == 11 && t < 12 * DIM) {  // N_c: N[i][p] = delta(i, p + 1) - beta w_i w_{p+1}
    const int i = t / DIM, p = t - DIM * i;
    const double* w = ncw + 13 * (size_t)c;
    Nm[i][p] = (i == p + 1 ? 1.0 : 0.0) - w[12] * w[i] * w[p + 1];
  }
  __syncthreads();
  if (coords == 1) {
    if (t < DIM * DIM) o[t] = T[t / DIM][t % DIM];
    return;
  }
  if (t >= 144) return;
  const int i = t / 12, j = t - 12 * i;
  if (i > j) return;
  const double* sg = sigma + 12 * (size_t)c;
  double v = 0;
  if constexpr (DIM == 12) {
    v = T[i][j];
  } else {
    for (int p = 0; p < DIM; ++p) {
      double s = 0;
      for (int q = 0; q < DIM; ++q) s += T[p][q] * Nm[j][q];
      v += Nm[i][p] * s;
    }
    // the double sum is not symmetric in (i, j) to the last bit, the mirrored store is
  }
  v = sg[i] * v * sg[j];
  o[12 * i + j] = v;
  o[12 * j + i] = v;
}

}  // namespace povar
