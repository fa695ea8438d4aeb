// povar_kernels_cov.hpp -- marginal camera covariance from the dense factor (povar_camera_covariance_pose / _joint;
// the reference has no counterpart).  run_cholesky's assembly and factorisation leave the upper factor R (A = R^T R,
// layout of povar_kernels_chol.hpp) in the augmented matrix M; the diagonal blocks of A^-1 = W W^T with W = R^-1 are
//   cov_add_qqt    A += Q Q^T on the upper block triangle (free gauge: Q an orthonormal basis of the gauge null space)
//   cov_diag_scan  max_k A_kk before and min_k R_kk^2 after the factorisation (the pivot rule of the free gauge)
//   cov_diag_inv   W_jj = R_jj^-1 of a 64 x 64 diagonal block          one wavefront, row c of W_jj in lane c
//   cov_trmm       T = R[0:j, j] W_jj into the scratch panel, then W[0:j, j] = -W[0:j, 0:j] T      64 x 64 tiles, MFMA
//   cov_fix_cameras  W_kk = 0 on the rows of the fixed cameras (povar_set_fixed_cameras), after the W loop
//   cov_gram       block c = sum_k W[J, k] W[J, k]^T over the camera's rows J                       workgroup per camera
//   cov_finish     - Q_J Q_J^T, then the map to camera coordinates (D T D, or D N_c T N_c^T D with the reflector)
// W overwrites R in place, block column by block column from the left: when column j is formed, W[0:j, 0:j] is final
// (the leading block of the inverse of a triangular matrix is the inverse of its leading block) and R[0:j, j] is still
// untouched.  cov_trmm is the n^3/3 part and runs on v_mfma_f64_16x16x4_f64 with the fragment layout of chol_syrk.
//
// Landmark covariance (povar_landmark_covariance_pose / _joint) goes on from W:
//   cov_lauum      C = W W^T: the strictly lower 64 x 64 blocks into M, the diagonal blocks into the scratch panel     MFMA
//   cov_at         entry (r, c) of C in that layout; by camera pair through the map cam_row (povar_set_dense_compaction: a camera
//                  that is not in the matrix reads as exact zeros)
//   lm_cov         Sigma_l = Hll^-1 + sum_ij G_i^T K_ij G_j - T_l^T T_l, then the map to landmark coordinates   workgroup per landmark
// Observation leverage and predicted-point covariance (povar_observation_covariance_pose / _joint) go on from Sigma_l:
//   obs_cov        (h_i, c_uu, c_uv, c_vv) of every observation of a landmark from K_ii, R_i = sum_j K_ij G_j and Sigma_l   workgroup per landmark
//   obs_hat        the same walk with another row: the weighted residual r_i and the block P_ii of the hat matrix (povar_observation_hat_*)
// Covariance blocks of parameter pairs (povar_covariance_blocks_pose / _joint) go on from C as well:
//   pair_cc, pair_cl, pair_ll   the block of a camera-camera, camera-landmark, landmark-landmark pair              workgroup per pair
#pragma once
#include "povar_kernels_chol.hpp"
#include "povar_kernels_sc.hpp"

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
// pivots R_kk^2, after it) over the rows k < n of the free cameras (fixed[k / dim] == 0: a decoupled row holds the 1 that
// sc_fix_cameras put there and says nothing about the system; fixed null: the compacted matrix, which holds no such row, and no
// row is skipped).  One workgroup.
POVAR_KERNEL __launch_bounds__(256) void cov_diag_scan(const double* M, int64_t ld, int n, int which, double* out, const uint8_t* fixed,
                                                       int dim) {
  __shared__ double sh[256];
  double v = which == 0 ? -INFINITY : INFINITY;
  for (int k = threadIdx.x; k < n; k += 256) {
    if (fixed && fixed[k / dim]) continue;
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

// Fixed cameras, after the W loop: row k of R is e_k^T on a decoupled row (sc_fix_cameras), so row and column k of W = R^-1 hold
// W_kk = 1 and nothing else; with W_kk = 0 the row and the column of C = W W^T are zero and every kernel after this one sees
// the covariance of the free cameras, zero-padded.  One thread per row k < n.
POVAR_KERNEL __launch_bounds__(256) void cov_fix_cameras(double* M, int64_t ld, int n, int dim, const uint8_t* fixed) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n && fixed[k / dim]) M[(int64_t)k * ld + k] = 0.0;
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
// The product is Mma64's (povar_kernels_chol.hpp) with A held row-major in LDS (K along its columns) and B as chol_syrk's.
// 73 KiB of static LDS (As 64 x 66, Bs 64 x 80 doubles: chol_syrk's B stride, the only one under 96 that keeps the two
// rows of a 32-lane half on different banks): within gfx950's 160 KiB per workgroup, two workgroups per CU, as chol_syrk's 80.
POVAR_KERNEL __launch_bounds__(256) void cov_trmm(const double* A, int64_t lda, const double* B, int64_t ldb, double* C,
                                                  int64_t ldc, int tri, int k_end, double alpha) {
  __shared__ double As[CH_NB][CV_ALDS];
  __shared__ double Bs[CH_NB][CH_LDS];
  const int i = blockIdx.x;
  Mma64 t;
  const double* arow = A + (int64_t)i * CH_NB * lda;
  // software pipeline, as chol_syrk_outer: the global loads of block kb + 1 are in flight while the MFMAs of block kb run
  double2 ra[Mma64::NLD], rb[Mma64::NLD];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int u = 0; u < Mma64::NLD; ++u) {
      int p, q;
      Mma64::share(u, p, q);
      ra[u] = *reinterpret_cast<const double2*>(arow + (int64_t)p * lda + (int64_t)kb * CH_NB + q);
      rb[u] = *reinterpret_cast<const double2*>(B + ((int64_t)kb * CH_NB + p) * ldb + q);
    }
  };
  const int k_first = tri ? i : 0;  // (< k_end: the launches cover block rows above the diagonal block only)
  fetch(k_first);
  for (int kb = k_first; kb < k_end; ++kb) {
    __syncthreads();
    Mma64::stage(As, Bs, ra, rb);
    __syncthreads();
    if (kb + 1 < k_end) fetch(kb + 1);
    t.mma<false, true>(As, Bs);
  }
  double* crow = C + (int64_t)i * CH_NB * ldc;
  t.store([&](int r, int c, double v) { crow[(int64_t)r * ldc + c] = alpha * v; });
}

// Solver-coordinate block of camera c: T[a][b] = sum_k W[J_a][k] W[J_b][k], J_a = cam_row[c] + a (a camera that is not in the
// matrix keeps the zeros `out` holds), over the columns
// k < n (the padding columns of these rows are zero: they contribute nothing).  W is upper triangular.  Inside a 64 x 64
// diagonal block cov_diag_inv has stored its zeros below the diagonal, but the strictly lower 64 x 64 blocks of M still
// hold what the assembly left there (or C, after cov_lauum), and a camera block that straddles a 64-edge reaches into
// one: entries with k < row are masked, not read.  One workgroup per camera: thread t walks columns DIM c + t, + 256, ... (coalesced row
// reads), keeps the DIM (DIM + 1) / 2 products of the upper triangle, one deterministic workgroup sum, mirrored on
// the way out so the block is symmetric bit for bit.  out: DIM x DIM row-major at stride 144.
template <int DIM>
__global__ __launch_bounds__(256) void cov_gram(const double* M, int64_t ld, int n, const int* cam_row, double* out) {
  constexpr int NP = DIM * (DIM + 1) / 2;
  __shared__ double sh[4 * NP];
  const int c = blockIdx.x;
  const int r0 = cam_row[c];
  if (r0 < 0) return;
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

// C = W W^T after the W loop: C[I][J] = sum_{K >= I} W[I][K] W[J][K]^T for the 64 x 64 blocks I >= J (W upper block
// triangular, K >= I >= J).  The strictly lower blocks go to their natural place in M, the N / 64 diagonal blocks to the
// N x 64 scratch panel (free once the W loop has ended: block I at rows 64 I), so no n^2 buffer is needed.
// One launch reads only the upper block triangle of M (blocks [I][K], [J][K] with K >= I >= J) and writes only the strictly
// lower one and the panel: no workgroup reads what another workgroup of the launch writes, and W itself stays in place.
// The K = I block of W[I][.] (and of W[J][.] when J = I) is masked below its diagonal, as cov_gram masks.
// Both operands are row-major along K (an A B^T product), so both sit in LDS as cov_trmm's A tile (stride CV_ALDS) and
// both fragments read A[i + (l & 15)][kk + (l >> 4)] (Mma64 with K along the columns of both tiles); the global
// loads of block K + 1 are in flight under the MFMAs of block K.  A tile of block row I takes N / 64 - I K steps: the
// linear blockIdx walks the rows I upwards (tile t = I (I + 1) / 2 + J), so the long tiles start first.
// grid = nb (nb + 1) / 2 with nb = N / 64.  66 KiB of static LDS: two workgroups per CU.
POVAR_KERNEL __launch_bounds__(256) void cov_lauum(double* M, int64_t ld, double* panel, int nb) {
  __shared__ double As[CH_NB][CV_ALDS];
  __shared__ double Bs[CH_NB][CV_ALDS];
  const int t = blockIdx.x;
  int I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  Mma64 tile;
  const double* arow = M + (int64_t)I * CH_NB * ld;
  const double* brow = M + (int64_t)J * CH_NB * ld;
  double2 ra[Mma64::NLD], rb[Mma64::NLD];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int u = 0; u < Mma64::NLD; ++u) {
      int p, q;
      Mma64::share(u, p, q);
      ra[u] = *reinterpret_cast<const double2*>(arow + (int64_t)p * ld + (int64_t)kb * CH_NB + q);
      rb[u] = *reinterpret_cast<const double2*>(brow + (int64_t)p * ld + (int64_t)kb * CH_NB + q);
      if (kb == I) {  // the diagonal block of W: upper triangular
        if (q < p) ra[u].x = 0.0;
        if (q + 1 < p) ra[u].y = 0.0;
      }
      if (kb == J) {
        if (q < p) rb[u].x = 0.0;
        if (q + 1 < p) rb[u].y = 0.0;
      }
    }
  };
  fetch(I);
  for (int kb = I; kb < nb; ++kb) {
    __syncthreads();
    Mma64::stage(As, Bs, ra, rb);
    __syncthreads();
    if (kb + 1 < nb) fetch(kb + 1);
    tile.mma<false, false>(As, Bs);
  }
  double* crow = I == J ? panel + (int64_t)I * CH_NB * CH_NB : M + (int64_t)I * CH_NB * ld + (int64_t)J * CH_NB;
  const int64_t ldc = I == J ? (int64_t)CH_NB : ld;
  tile.store([&](int r, int c, double v) { crow[(int64_t)r * ldc + c] = v; });
}

// Entry (r, c) of the symmetric C = W W^T as cov_lauum leaves it: the one place that knows the layout (a camera block of
// 12 or 11 rows straddles the 64-edges, so a block's entries may come from up to four tiles).
__device__ inline double cov_at(const double* M, int64_t ld, const double* panel, int r, int c) {
  if (r < c) { const int t = r; r = c; c = t; }
  if ((r >> 6) == (c >> 6)) return panel[(int64_t)r * CH_NB + (c & 63)];
  return M[(int64_t)r * ld + c];
}
// Entry (r, c) of the block of a camera pair whose cameras start at rows ra and rb of the matrix (cam_row of each: the map of
// povar_set_dense_compaction); a camera that is not in the matrix (< 0) is a fixed one, whose rows and columns of C are exactly 0.
__device__ inline double cov_at(const double* M, int64_t ld, const double* panel, int ra, int r, int rb, int c) {
  if ((ra | rb) < 0) return 0.0;
  return cov_at(M, ld, panel, ra + r, rb + c);
}

// Per-landmark contraction.  With C the camera covariance (S(lambda)^-1, or S0^+ = (S0 + Q Q^T)^-1 - Q Q^T), E_i the
// DIM x 3 block of Hpl of observation i and G_i = F_i Hll^-1 (scd_stage / scdh_stage):
//   Sigma_l = Hll^-1 + sum_{i,j in obs(l)} (E_i Hll^-1)^T C[c_i, c_j] (E_j Hll^-1),    E_i Hll^-1 = sum_a u_a G_i[a][:],
//   u_a = sigma_ci o (e_a (x) h) (ScdPose) or N_ci^T (sigma_ci o (e_a (x) X)) (ScdJoint: the staged U)   -- Step::u,
// so a camera pair costs the 3 x 3 bilinear form K_ij[a][b] = u_a^T C[c_i, c_j] v_b (DIM^2 entries of C through cov_at, a
// 16-lane group per pair) and G_i^T K_ij G_j, plus its transpose for i != j (pairs i <= j only).  C here is (S0 + Q Q^T)^-1
// in the free gauge; the - Q Q^T part is T_l^T T_l with T_l = sum_i Q[rows of c_i, :]^T (E_i Hll^-1) (nq x 3), gathered per
// observation by 64 threads (column k of Q, every fourth observation) and subtracted once.
// One workgroup per requested landmark (ids null: landmark blockIdx.x), the observations staged in chunks with the two
// chunk loops of sc_dense_offdiag[_h].  No atomics: every thread keeps its own partial, one fixed-order workgroup sum,
// so the block is reproducible given C.  Then + Hll^-1 and the coords map:
//   coords = 1 (solver):    Sigma (3 x 3) in the first 9 of the stride, the rest zero;
//   coords = 0 (landmark):  the block carried through the map back-substitution applies to a landmark increment:
//                           step 1: D Sigma D, D = diag(s_l) (stride 9); step 2: the 4 x 4 D4 N_l Sigma N_l^T D4 with
//                           N_l = (I - beta w w^T)[:, 1:] from house4(X_l) (stride 16; rank 3, null vector X_l / s_l).
// The upper triangle is written mirrored: every block is symmetric bit for bit.
// Step = ScdPose / ScdJoint (povar_kernels_sc.hpp) supplies the landmark head, the staging and u_a.  What this kernel and obs_cov
// keep as their own text, because the compiler's output moved when it was shared (profiles/dense_parts_isa.txt): the bilinear
// form's loop over the DIM^2 entries, K G_j, and the two arms of the map to landmark coordinates below.
template <class Step>
__global__ __launch_bounds__(256) void lm_cov(Dp d, const double* ncw, const int* lm_slot0, const int* lm_cnt, const int* ids,
                                              const double* M, int64_t ld, const double* panel, const int* cam_row, const double* Q,
                                              int nq, int coords, double* out) {
  typedef typename Step::Obs Obs;
  constexpr int DIM = Step::DIM, CHUNK = Step::CHUNK, STRIDE = Step::LM_STRIDE;
  __shared__ Obs oi[CHUNK], oj[CHUNK];
  __shared__ double sh[4 * 9];
  __shared__ double shT[4][16][3];
  const int lm = ids ? ids[blockIdx.x] : (int)blockIdx.x;
  const int s0 = lm_slot0[lm], k = lm_cnt[lm];
  const typename Step::Head hd = Step::load(d, lm);
  const double h[4] = {hd.h[0], hd.h[1], hd.h[2], hd.h[3]};  // (Step::u indexes it at run time: not left inside the Head)
  // (a closure: called directly, the staging compiles to other code -- the same values; profiles/dense_parts_isa.txt)
  auto stage = [&](int slot, Obs& o) { Step::stage(d, ncw, slot, hd, o); };
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double tacc[3] = {0, 0, 0};  // threads < 64: T_l[k = t & 15][:] over the observations t >> 4, + 4, ...
  for (int ic = 0; ic < k; ic += CHUNK) {
    const int ni = min(CHUNK, k - ic);
    __syncthreads();
    if ((int)threadIdx.x < ni) stage(s0 + ic + threadIdx.x, oi[threadIdx.x]);
    for (int jc = ic; jc < k; jc += CHUNK) {
      const int nj = min(CHUNK, k - jc);
      __syncthreads();
      if ((int)threadIdx.x < nj) stage(s0 + jc + threadIdx.x, oj[threadIdx.x]);
      __syncthreads();
      if (nq > 0 && jc == ic && threadIdx.x < 64 && gl < nq) {
        for (int i = grp; i < ni; i += 4) {
          const Obs& a = oi[i];
          const double* qrow = Q + (size_t)DIM * a.cam * nq + gl;
          double ta[3] = {0, 0, 0};
          for (int r = 0; r < DIM; ++r) {
            double u[3];
            Step::u(a, d.sigma, h, r, u);
            const double qv = qrow[(size_t)r * nq];
            ta[0] += qv * u[0];
            ta[1] += qv * u[1];
            ta[2] += qv * u[2];
          }
#pragma unroll
          for (int b = 0; b < 3; ++b) tacc[b] += ta[0] * a.G[b] + ta[1] * a.G[3 + b] + ta[2] * a.G[6 + b];
        }
      }
      // (the trip count and the shuffles are uniform over the workgroup; a group without a pair adds zeros)
      for (int p0 = 0; p0 < ni * nj; p0 += 16) {
        const int pp = p0 + grp;
        const int i = pp / nj, j = pp - i * nj;
        const bool live = pp < ni * nj && !(ic == jc && i > j);  // pairs i <= j: the transpose stands for the other half
        double K[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (live) {
          const Obs& a = oi[i];
          const Obs& b = oj[j];
          const int ra = cam_row[a.cam], rb = cam_row[b.cam];
          for (int e = gl; e < DIM * DIM; e += 16) {
            const int r = e / DIM, c = e - DIM * r;
            const double cv = cov_at(M, ld, panel, ra, r, rb, c);
            double u[3], v[3];
            Step::u(a, d.sigma, h, r, u);
            Step::u(b, d.sigma, h, c, v);
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
              for (int y = 0; y < 3; ++y) K[3 * x + y] += u[x] * cv * v[y];
          }
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1)
#pragma unroll
          for (int e = 0; e < 9; ++e) K[e] += shfl_xor_d(K[e], m);
        if (live && gl == 0) {
          const Obs& a = oi[i];
          const Obs& b = oj[j];
          double KG[9], P[9];  // K G_j, then G_i^T (K G_j)
#pragma unroll
          for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) KG[3 * x + y] = K[3 * x] * b.G[y] + K[3 * x + 1] * b.G[3 + y] + K[3 * x + 2] * b.G[6 + y];
#pragma unroll
          for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) P[3 * x + y] = a.G[x] * KG[y] + a.G[3 + x] * KG[3 + y] + a.G[6 + x] * KG[6 + y];
          const bool same = ic == jc && i == j;
#pragma unroll
          for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) acc[3 * x + y] += same ? P[3 * x + y] : P[3 * x + y] + P[3 * y + x];
        }
      }
    }
  }
  block_sum<9, 256>(acc, sh);
  if (threadIdx.x < 64) {
#pragma unroll
    for (int b = 0; b < 3; ++b) shT[grp][gl][b] = tacc[b];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double Sg[9];
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int y = x; y < 3; ++y) {
      double tt = 0;
      for (int q = 0; q < nq; ++q) {
        const double tx = ((shT[0][q][x] + shT[1][q][x]) + shT[2][q][x]) + shT[3][q][x];
        const double ty = ((shT[0][q][y] + shT[1][q][y]) + shT[2][q][y]) + shT[3][q][y];
        tt += tx * ty;
      }
      const double v = hd.Hi[3 * x + y] + acc[3 * x + y] - tt;
      Sg[3 * x + y] = v;
      Sg[3 * y + x] = v;
    }
  double* o = out + (size_t)STRIDE * blockIdx.x;
  if (coords == 1) {
#pragma unroll
    for (int e = 0; e < STRIDE; ++e) o[e] = e < 9 ? Sg[e] : 0.0;
    return;
  }
  if constexpr (!Step::HOM) {
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = x; y < 3; ++y) {
        const double v = hd.s4[x] * Sg[3 * x + y] * hd.s4[y];
        o[3 * x + y] = v;
        o[3 * y + x] = v;
      }
  } else {
    double Nl[4][3];  // N_l[i][p] = delta(i, p + 1) - beta w_i w_{p+1}
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) Nl[i][p] = (i == p + 1 ? 1.0 : 0.0) - hd.hbeta * hd.hw[i] * hd.hw[p + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j) {
        double v = 0;
#pragma unroll
        for (int p = 0; p < 3; ++p) v += Nl[i][p] * (Sg[3 * p] * Nl[j][0] + Sg[3 * p + 1] * Nl[j][1] + Sg[3 * p + 2] * Nl[j][2]);
        v = hd.s4[i] * v * hd.s4[j];
        o[4 * i + j] = v;
        o[4 * j + i] = v;
      }
  }
}

// Per-observation block of the hat matrix J H^+ J^T (povar_observation_covariance_pose / _joint).  With y = P_c X_l the
// projected homogeneous point of observation i of landmark l, dy = U_i^T dp_c + L_i dl (U_i the three vectors Step::u
// reads; L_i = P3 diag(s) (step 1) or P diag(s4) N_l (step 2): Step::l_row) and M_i (Step::gram_m) the 3 x 3 Gram matrix of the weighted residual
// Jacobian with respect to y (w C, or w Dm^T Dm: F_i = M_i L_i), the covariance of y is
//   Syy_i = K_ii - R_i L_i^T - L_i R_i^T + L_i Sigma_l L_i^T,   K_ij = U_i^T C[c_i, c_j] U_j,   R_i = sum_{j in obs(l)} K_ij G_j
// (- C F_l is the camera-landmark cross covariance), and the row is
//   h_i = tr(M_i Syy_i)  (leverage)   and   J Syy_i J^T,  J = d(y0 / y2, y1 / y2) / dy  (2 x 2: c_uu, c_uv, c_vv; unweighted).
// C is (S0 + Q Q^T)^-1 as it stands in the free gauge: [Q; -Hll^-1 Hlp Q] lies in the null space of J, so the - Q Q^T
// part cancels in Syy_i -- provided Sigma_l carries none of it either: `sig` is lm_cov's output with nq = 0, coords = 1
// (9 numbers at stride 9 / 16), and no Q is read here.
// One workgroup per requested landmark, staged as lm_cov stages; a 16-lane group owns observation i and walks every j of
// the track (all k^2 pairs: K_ji = K_ij^T is not reused), each lane keeping its share of the DIM^2 entries of every K_ij:
// R_i is linear in K_ij, so the lanes' partial R_i and K_ii stay in registers and meet in one butterfly after the walk --
// no atomics, a fixed order, the row reproducible given C.  Lane 0 of the group then forms the row at
// out + 4 (row0[blockIdx.x] + i): the rows of a landmark in the order of its observations.  y2 = 0 leaves c_* non-finite
// by IEEE rules (step 1: h_i does not depend on J).
//
// The same Syy_i gives the whole block of the hat matrix (povar_observation_hat_pose / _joint): with A_i (Step::jac_a) the
// RES x 3 weighted Jacobian of the residual with respect to y (A_i^T A_i = M_i) and r_i the weighted residual,
//   P_ii = A_i Syy_i A_i^T   (RES x RES: h_i is its trace),
// so the walk is one body, obs_rows, and the row is a policy: ObsCovRow (the row above, stride 4) or ObsHatRow
// (r_i, then the upper triangle of P_ii by rows: stride 14 in step 1, 5 in step 2).  A policy is built from the linearisation
// point as the staging reads it (the camera, the landmark head, uv, the stored sqrt(w)) and writes the row from y and the mirrored
// Syy_i.
template <class Step>
struct ObsCovRow {
  static constexpr int STRIDE = 4;
  double Mi[9];
  __device__ __forceinline__ ObsCovRow(const Dp& d, const Cam& P, const typename Step::Head& hd, double2 uv, double sw) {
    const double w = sw * sw;
    Step::gram_m(d, P, hd, uv, w, Mi);
  }
  __device__ __forceinline__ void write(const double (&yv)[3], const double (&Syy)[9], double* o) const {
    double lev = 0;
#pragma unroll
    for (int e = 0; e < 9; ++e) lev += Mi[e] * Syy[e];  // (both symmetric)
    const double iz = 1.0 / yv[2];
    const double j0 = -yv[0] * iz * iz, j1 = -yv[1] * iz * iz;  // J = [[iz, 0, j0], [0, iz, j1]]
    const double a0[3] = {iz * Syy[0] + j0 * Syy[6], iz * Syy[1] + j0 * Syy[7], iz * Syy[2] + j0 * Syy[8]};  // J Syy
    const double a1[3] = {iz * Syy[3] + j1 * Syy[6], iz * Syy[4] + j1 * Syy[7], iz * Syy[5] + j1 * Syy[8]};
    o[0] = lev;
    o[1] = a0[0] * iz + a0[2] * j0;
    o[2] = a0[1] * iz + a0[2] * j1;
    o[3] = a1[1] * iz + a1[2] * j1;
  }
};

// r_i, then P_ii = (A_i Syy_i) A_i^T on the upper triangle only: the caller mirrors it, so the block is symmetric by construction
template <class Step>
struct ObsHatRow {
  static constexpr int RES = Step::RES, STRIDE = RES + RES * (RES + 1) / 2;
  const Dp& d;
  const double2 uv;
  const double sw;
  __device__ __forceinline__ ObsHatRow(const Dp& d_, const Cam&, const typename Step::Head&, double2 uv_, double sw_)
      : d(d_), uv(uv_), sw(sw_) {}
  __device__ __forceinline__ void write(const double (&yv)[3], const double (&Syy)[9], double* o) const {
    double A[3 * RES], r[RES], T[3 * RES];
    Step::jac_a(d, uv, sw, yv, A, r);
#pragma unroll
    for (int p = 0; p < RES; ++p)
#pragma unroll
      for (int x = 0; x < 3; ++x) T[3 * p + x] = A[3 * p] * Syy[x] + A[3 * p + 1] * Syy[3 + x] + A[3 * p + 2] * Syy[6 + x];
#pragma unroll
    for (int p = 0; p < RES; ++p) o[p] = r[p];
    int e = RES;
#pragma unroll
    for (int p = 0; p < RES; ++p)
#pragma unroll
      for (int q = p; q < RES; ++q) o[e++] = T[3 * p] * A[3 * q] + T[3 * p + 1] * A[3 * q + 1] + T[3 * p + 2] * A[3 * q + 2];
  }
};

template <class Step, class Row>
__device__ __forceinline__ void obs_rows(Dp d, const double* ncw, const int* lm_slot0, const int* lm_cnt, const int* ids,
                                         const int* row0, const double* M, int64_t ld, const double* panel, const int* cam_row,
                                         const double* sig, double* out) {
  typedef typename Step::Obs Obs;
  constexpr int DIM = Step::DIM, CHUNK = Step::CHUNK, STRIDE = Step::LM_STRIDE;
  __shared__ Obs oi[CHUNK], oj[CHUNK];
  const int lm = ids ? ids[blockIdx.x] : (int)blockIdx.x;
  const int s0 = lm_slot0[lm], k = lm_cnt[lm];
  const typename Step::Head hd = Step::load(d, lm);
  const double h[4] = {hd.h[0], hd.h[1], hd.h[2], hd.h[3]};  // (Step::u indexes it at run time: not left inside the Head)
  auto stage = [&](int slot, Obs& o) { Step::stage(d, ncw, slot, hd, o); };  // (a closure: see lm_cov)
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
  int staged = -1;  // the chunk oj holds: a track of one chunk stages it once
  for (int ic = 0; ic < k; ic += CHUNK) {
    const int ni = min(CHUNK, k - ic);
    __syncthreads();
    if ((int)threadIdx.x < ni) stage(s0 + ic + threadIdx.x, oi[threadIdx.x]);
    __syncthreads();
    // (the trip counts, the barriers and the shuffles are uniform over the workgroup; a group without an observation adds zeros)
    for (int i0 = 0; i0 < ni; i0 += 16) {
      const int i = i0 + grp;
      const bool live = i < ni;
      double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Kii[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int jc = 0; jc < k; jc += CHUNK) {
        const int nj = min(CHUNK, k - jc);
        if (staged != jc) {
          __syncthreads();
          if ((int)threadIdx.x < nj) stage(s0 + jc + threadIdx.x, oj[threadIdx.x]);
          __syncthreads();
          staged = jc;
        }
        if (!live) continue;
        const Obs& a = oi[i];
        const int ra = cam_row[a.cam];
        for (int j = 0; j < nj; ++j) {
          const Obs& b = oj[j];
          const int rb = cam_row[b.cam];
          double K[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
          for (int e = gl; e < DIM * DIM; e += 16) {
            const int r = e / DIM, c = e - DIM * r;
            const double cv = cov_at(M, ld, panel, ra, r, rb, c);
            double u[3], v[3];
            Step::u(a, d.sigma, h, r, u);
            Step::u(b, d.sigma, h, c, v);
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
              for (int y = 0; y < 3; ++y) K[3 * x + y] += u[x] * cv * v[y];
          }
#pragma unroll
          for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) R[3 * x + y] += K[3 * x] * b.G[y] + K[3 * x + 1] * b.G[3 + y] + K[3 * x + 2] * b.G[6 + y];
          if (jc == ic && j == i) {
#pragma unroll
            for (int e = 0; e < 9; ++e) Kii[e] = K[e];
          }
        }
      }
#pragma unroll
      for (int m = 8; m >= 1; m >>= 1)
#pragma unroll
        for (int e = 0; e < 9; ++e) {
          R[e] += shfl_xor_d(R[e], m);
          Kii[e] += shfl_xor_d(Kii[e], m);
        }
      if (!live || gl != 0) continue;
      // the row of observation ic + i: L_i and y from the linearisation point, as the staging reads them
      const int slot = s0 + ic + i;
      const Cam P = load_cam(d.cams_lin4, oi[i].cam);
      const double2 uv = d.uv[slot];
      const double sw = d.robust ? d.sw[slot] : 1.0;
      const double4 pr[3] = {P.r0, P.r1, P.r2};
      double L[9], yv[3];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const double p4[4] = {pr[x].x, pr[x].y, pr[x].z, pr[x].w};
        yv[x] = p4[0] * h[0] + p4[1] * h[1] + p4[2] * h[2] + p4[3] * h[3];
        Step::l_row(hd, p4, L + 3 * x);
      }
      const Row row(d, P, hd, uv, sw);  // (what the row needs of the linearisation point besides y)
      const double* Sg = sig + (size_t)STRIDE * blockIdx.x;
      double SL[9], Syy[9];  // Sigma_l L_i^T, then the upper triangle of Syy_i, mirrored
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) SL[3 * x + y] = Sg[3 * x] * L[3 * y] + Sg[3 * x + 1] * L[3 * y + 1] + Sg[3 * x + 2] * L[3 * y + 2];
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = x; y < 3; ++y) {
          const double rl = R[3 * x] * L[3 * y] + R[3 * x + 1] * L[3 * y + 1] + R[3 * x + 2] * L[3 * y + 2];
          const double lr = L[3 * x] * R[3 * y] + L[3 * x + 1] * R[3 * y + 1] + L[3 * x + 2] * R[3 * y + 2];
          const double lsl = L[3 * x] * SL[y] + L[3 * x + 1] * SL[3 + y] + L[3 * x + 2] * SL[6 + y];
          const double v = Kii[3 * x + y] - rl - lr + lsl;
          Syy[3 * x + y] = v;
          Syy[3 * y + x] = v;
        }
      row.write(yv, Syy, out + Row::STRIDE * ((size_t)row0[blockIdx.x] + ic + i));
    }
  }
}

template <class Step>
__global__ __launch_bounds__(256) void obs_cov(Dp d, const double* ncw, const int* lm_slot0, const int* lm_cnt, const int* ids,
                                               const int* row0, const double* M, int64_t ld, const double* panel,
                                               const int* cam_row, const double* sig, double* out) {
  obs_rows<Step, ObsCovRow<Step>>(d, ncw, lm_slot0, lm_cnt, ids, row0, M, ld, panel, cam_row, sig, out);
}

template <class Step>
__global__ __launch_bounds__(256) void obs_hat(Dp d, const double* ncw, const int* lm_slot0, const int* lm_cnt, const int* ids,
                                               const int* row0, const double* M, int64_t ld, const double* panel,
                                               const int* cam_row, const double* sig, double* out) {
  obs_rows<Step, ObsHatRow<Step>>(d, ncw, lm_slot0, lm_cnt, ids, row0, M, ld, panel, cam_row, sig, out);
}

// ------------------------------------------------------------------------------------------
// Covariance blocks of parameter pairs (povar_covariance_blocks_pose / _joint): the off-diagonal blocks of the joint covariance
// the calls above take diagonal blocks of.  With W_i = E_i Hll^-1 (DIM x 3: row r is sum_a u_a[r] G_i[a][:], pair_w) and C as
// cov_lauum leaves it ((S0 + Q Q^T)^-1 in the free gauge, whose - n n^T part, n = [Q; -F^T Q], is taken off explicitly with
// T_l = sum_i Q[c_i]^T W_i, as lm_cov does):
//   pair_cc   camera a, camera b        C[a, b] - Q_a Q_b^T
//   pair_cl   camera c, landmark l      -sum_{j in obs(l)} C[c, c_j] W_j + Q_c T_l                                   (DIM x 3)
//   pair_ll   landmark l, landmark m    delta_lm Hll_l^-1 + sum_{i in obs(l), j in obs(m)} W_i^T C[c_i, c_j] W_j - T_l^T T_m
// then the maps of cov_finish and lm_cov on either side in parameter coordinates (M_cam = D or D N_c, M_lm = diag(s) or D4 N_l).
// One workgroup per pair.  The host hands every pair over in a canonical order (cameras: a >= b; landmarks: l <= m; the camera
// of a mixed pair first) with the flag `tr`: the block is then stored transposed, so (b, a) is the bitwise transpose of (a, b).
// A block with a == b evaluates entry (i, j), i > j, as entry (j, i): symmetric bit for bit.
// C is read through cov_at alone.  Its lower block triangle is row-major, so the lanes of a 16-lane group lie along the index
// of the camera with the smaller id: a group reads contiguous runs of a row of C whichever camera of a pair comes first.
// No floating-point atomics: every thread keeps its partial sums in registers and every sum has a fixed order (one block_sum,
// and a fixed-order sum over the 16 groups for T_l): a block is reproducible given C.
// items[p] = (a, b, tr, -), off[p] = where the block of pair p starts in `out`.
// ------------------------------------------------------------------------------------------

// row r of W_i = E_i Hll^-1
template <class Step>
__device__ inline void pair_w(const typename Step::Obs& o, const double* sigma, const double (&h)[4], int r, double (&w)[3]) {
  double u[3];
  Step::u(o, sigma, h, r, u);
#pragma unroll
  for (int x = 0; x < 3; ++x) w[x] = u[0] * o.G[x] + u[1] * o.G[3 + x] + u[2] * o.G[6 + x];
}

// tacc += the part of T_l[k = gl][:] of the staged observations grp, grp + 16, ... (lm_cov's gather, a 16-lane group per observation)
template <class Step>
__device__ inline void pair_t_add(const typename Step::Obs* os, int n, const double* sigma, const double (&h)[4], const double* Q,
                                  int nq, int grp, int gl, double (&tacc)[3]) {
  if (gl >= nq) return;
  for (int i = grp; i < n; i += 16) {
    const typename Step::Obs& a = os[i];
    const double* qrow = Q + (size_t)Step::DIM * a.cam * nq + gl;
    for (int r = 0; r < Step::DIM; ++r) {
      double w[3];
      pair_w<Step>(a, sigma, h, r, w);
      const double qv = qrow[(size_t)r * nq];
#pragma unroll
      for (int b = 0; b < 3; ++b) tacc[b] += qv * w[b];
    }
  }
}

// T_l[k][b] from the 16 groups' partials, in the order of the groups
__device__ inline double pair_t_sum(const double (&shT)[16][16][3], int k, int b) {
  double s = 0;
#pragma unroll
  for (int g = 0; g < 16; ++g) s += shT[g][k][b];
  return s;
}

// N_c[i][p] = delta(i, p + 1) - beta w_i w_{p+1} from ncw = (w[12], beta) (cov_finish's Nm)
__device__ inline double pair_nc(const double* w, int i, int p) { return (i == p + 1 ? 1.0 : 0.0) - w[12] * w[i] * w[p + 1]; }

template <class Step>
__global__ __launch_bounds__(192) void pair_cc(const int4* items, const long long* off, const double* M, int64_t ld, const double* panel,
                                               const int* cam_row, const double* Q, int nq, const double* sigma, const double* ncw,
                                               int coords, double* out) {
  constexpr int DIM = Step::DIM;
  __shared__ double T[DIM][DIM + 1];
  const int4 it = items[blockIdx.x];
  const int a = it.x, b = it.y, t = threadIdx.x;
  const bool tr = it.z != 0, same = a == b;
  double* o = out + off[blockIdx.x];
  if (t < DIM * DIM) {  // lanes along the columns: a >= b, a row of the block is a run of a row of C
    int i = t / DIM, j = t - DIM * i;
    if (same && i > j) { const int s = i; i = j; j = s; }
    const double* qa = Q + (size_t)(DIM * a + i) * nq;
    const double* qb = Q + (size_t)(DIM * b + j) * nq;
    double s = 0;
    for (int k = 0; k < nq; ++k) s += qa[k] * qb[k];
    T[t / DIM][t % DIM] = cov_at(M, ld, panel, cam_row[a], i, cam_row[b], j) - s;
  }
  __syncthreads();
  if (coords == 1) {
    if (t < DIM * DIM) {
      const int i = t / DIM, j = t - DIM * i;
      o[tr ? DIM * j + i : t] = T[i][j];
    }
    return;
  }
  if (t >= 144) return;
  const int i0 = t / 12, j0 = t - 12 * i0;
  int i = i0, j = j0;
  if (same && i > j) { i = j0; j = i0; }
  double v = 0;
  if constexpr (!Step::HOM) {
    v = T[i][j];
  } else {
    const double* wa = ncw + 13 * (size_t)a;
    const double* wb = ncw + 13 * (size_t)b;
    for (int p = 0; p < DIM; ++p) {
      double s = 0;
      for (int q = 0; q < DIM; ++q) s += T[p][q] * pair_nc(wb, j, q);
      v += pair_nc(wa, i, p) * s;
    }
  }
  v = sigma[12 * (size_t)a + i] * v * sigma[12 * (size_t)b + j];
  o[tr ? 12 * j0 + i0 : t] = v;
}

template <class Step>
__global__ __launch_bounds__(256) void pair_cl(Dp d, const double* ncw, const int* lm_slot0, const int* lm_cnt, const int4* items,
                                               const long long* off, const double* M, int64_t ld, const double* panel, const int* cam_row,
                                               const double* Q, int nq, int coords, double* out) {
  typedef typename Step::Obs Obs;
  constexpr int DIM = Step::DIM, CHUNK = Step::CHUNK, NX = 3 * DIM;
  __shared__ Obs oj[CHUNK];
  __shared__ double sh[4 * NX];
  __shared__ double shT[16][16][3];
  __shared__ double X[DIM][3];
  const int4 it = items[blockIdx.x];
  const int cam = it.x, lm = it.y, t = threadIdx.x;
  const bool tr = it.z != 0;
  const int s0 = lm_slot0[lm], k = lm_cnt[lm];
  const int rc = cam_row[cam];
  const typename Step::Head hd = Step::load(d, lm);
  const double h[4] = {hd.h[0], hd.h[1], hd.h[2], hd.h[3]};
  auto stage = [&](int slot, Obs& o) { Step::stage(d, ncw, slot, hd, o); };
  const int grp = t >> 4, gl = t & 15;
  double acc[NX];  // lane r of a group: its share of sum_j C[c p, c_j r] W_j[r][b] for every (p, b)  (c >= c_j)
#pragma unroll
  for (int e = 0; e < NX; ++e) acc[e] = 0;
  double accp[3] = {0, 0, 0};  // lane p of a group: sum_j sum_r C[c p, c_j r] W_j[r][b]  (c < c_j)
  double tacc[3] = {0, 0, 0};
  for (int jc = 0; jc < k; jc += CHUNK) {
    const int nj = min(CHUNK, k - jc);
    __syncthreads();
    if (t < nj) stage(s0 + jc + t, oj[t]);
    __syncthreads();
    if (nq > 0) pair_t_add<Step>(oj, nj, d.sigma, h, Q, nq, grp, gl, tacc);
    if (gl >= DIM) continue;  // (no shuffle below: the lanes past the block's edge wait at the next barrier)
    for (int j = grp; j < nj; j += 16) {
      const Obs& b = oj[j];
      const int rb = cam_row[b.cam];
      if (cam >= b.cam) {
        double w[3];
        pair_w<Step>(b, d.sigma, h, gl, w);
#pragma unroll
        for (int p = 0; p < DIM; ++p) {
          const double cv = cov_at(M, ld, panel, rc, p, rb, gl);
#pragma unroll
          for (int x = 0; x < 3; ++x) acc[3 * p + x] += cv * w[x];
        }
      } else {
        for (int r = 0; r < DIM; ++r) {
          double w[3];
          pair_w<Step>(b, d.sigma, h, r, w);
          const double cv = cov_at(M, ld, panel, rc, gl, rb, r);
#pragma unroll
          for (int x = 0; x < 3; ++x) accp[x] += cv * w[x];
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < DIM; ++p)
#pragma unroll
    for (int x = 0; x < 3; ++x) acc[3 * p + x] += gl == p ? accp[x] : 0.0;
  block_sum<NX, 256>(acc, sh);
#pragma unroll
  for (int b = 0; b < 3; ++b) shT[grp][gl][b] = tacc[b];
  __syncthreads();
  if (t < NX) {
    const int p = t / 3, b = t - 3 * p;
    double v = 0;
#pragma unroll
    for (int e = 0; e < NX; ++e) v = t == e ? acc[e] : v;
    v = -v;
    const double* qc = Q + (size_t)(DIM * cam + p) * nq;
    for (int q = 0; q < nq; ++q) v += qc[q] * pair_t_sum(shT, q, b);
    X[p][b] = v;
  }
  __syncthreads();
  double* o = out + off[blockIdx.x];
  const double* sg = d.sigma + 12 * (size_t)cam;
  if (coords == 1) {
    if (t < NX) {
      const int p = t / 3, b = t - 3 * p;
      o[tr ? DIM * b + p : t] = X[p][b];
    }
    return;
  }
  if constexpr (!Step::HOM) {
    if (t < NX) {
      const int p = t / 3, b = t - 3 * p;
      const double sl = b == 0 ? hd.s4[0] : b == 1 ? hd.s4[1] : hd.s4[2];  // (not indexed at run time inside the Head)
      o[tr ? 12 * b + p : t] = sg[p] * X[p][b] * sl;
    }
  } else {
    if (t < 48) {  // D N_c X N_l^T D4, 12 x 4
      const int i = t >> 2, y = t & 3;
      const double* wc = ncw + 13 * (size_t)cam;
      const double hw[4] = {hd.hw[0], hd.hw[1], hd.hw[2], hd.hw[3]}, s4[4] = {hd.s4[0], hd.s4[1], hd.s4[2], hd.s4[3]};
      double nl[3];
#pragma unroll
      for (int b = 0; b < 3; ++b) nl[b] = (y == b + 1 ? 1.0 : 0.0) - hd.hbeta * hw[y] * hw[b + 1];
      double v = 0;
      for (int p = 0; p < DIM; ++p) v += pair_nc(wc, i, p) * (X[p][0] * nl[0] + X[p][1] * nl[1] + X[p][2] * nl[2]);
      o[tr ? 12 * y + i : t] = sg[i] * v * s4[y];
    }
  }
}

template <class Step>
__global__ __launch_bounds__(256) void pair_ll(Dp d, const double* ncw, const int* lm_slot0, const int* lm_cnt, const int4* items,
                                               const long long* off, const double* M, int64_t ld, const double* panel, const int* cam_row,
                                               const double* Q, int nq, int coords, double* out) {
  typedef typename Step::Obs Obs;
  constexpr int DIM = Step::DIM, CHUNK = Step::CHUNK;
  __shared__ Obs oi[CHUNK], oj[CHUNK];
  __shared__ double sh[4 * 9];
  __shared__ double shTl[16][16][3], shTm[16][16][3];
  const int4 it = items[blockIdx.x];
  const int l = it.x, m = it.y, t = threadIdx.x;
  const bool tr = it.z != 0, same = l == m;
  const int sl = lm_slot0[l], kl = lm_cnt[l], sm = lm_slot0[m], km = lm_cnt[m];
  const typename Step::Head hl = Step::load(d, l), hm = Step::load(d, m);
  const double hhl[4] = {hl.h[0], hl.h[1], hl.h[2], hl.h[3]}, hhm[4] = {hm.h[0], hm.h[1], hm.h[2], hm.h[3]};
  auto stage_l = [&](int slot, Obs& o) { Step::stage(d, ncw, slot, hl, o); };
  auto stage_m = [&](int slot, Obs& o) { Step::stage(d, ncw, slot, hm, o); };
  const int grp = t >> 4, gl = t & 15;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double tl[3] = {0, 0, 0}, tm[3] = {0, 0, 0};
  // the rectangle obs(l) x obs(m): both chunk loops run in full, each side staged with its own landmark's head
  for (int ic = 0; ic < kl; ic += CHUNK) {
    const int ni = min(CHUNK, kl - ic);
    __syncthreads();
    if (t < ni) stage_l(sl + ic + t, oi[t]);
    for (int jc = 0; jc < km; jc += CHUNK) {
      const int nj = min(CHUNK, km - jc);
      __syncthreads();
      if (t < nj) stage_m(sm + jc + t, oj[t]);
      __syncthreads();
      if (nq > 0 && jc == 0) pair_t_add<Step>(oi, ni, d.sigma, hhl, Q, nq, grp, gl, tl);
      if (nq > 0 && ic == 0) pair_t_add<Step>(oj, nj, d.sigma, hhm, Q, nq, grp, gl, tm);
      for (int pp = grp; pp < ni * nj; pp += 16) {
        const int i = pp / nj, j = pp - i * nj;
        const Obs& a = oi[i];
        const Obs& b = oj[j];
        const bool by_rows = a.cam >= b.cam;  // the lanes along the index of the camera with the smaller id
        const int ra = cam_row[a.cam], rb = cam_row[b.cam];
        for (int e = gl; e < DIM * DIM; e += 16) {
          const int e1 = e / DIM, e2 = e - DIM * e1;
          const int r = by_rows ? e1 : e2, c = by_rows ? e2 : e1;
          const double cv = cov_at(M, ld, panel, ra, r, rb, c);
          double wi[3], wj[3];
          pair_w<Step>(a, d.sigma, hhl, r, wi);
          pair_w<Step>(b, d.sigma, hhm, c, wj);
#pragma unroll
          for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) acc[3 * x + y] += wi[x] * cv * wj[y];
        }
      }
    }
  }
  block_sum<9, 256>(acc, sh);
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    shTl[grp][gl][b] = tl[b];
    shTm[grp][gl][b] = tm[b];
  }
  __syncthreads();
  if (t != 0) return;
  // (l == m: the upper triangle stands for the lower one, here and after the map)
  double Sg[9];
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int y = 0; y < 3; ++y) {
      double tt = 0;
      for (int q = 0; q < nq; ++q) tt += pair_t_sum(shTl, q, x) * pair_t_sum(shTm, q, y);
      Sg[3 * x + y] = (same ? hl.Hi[3 * x + y] : 0.0) + acc[3 * x + y] - tt;
    }
#pragma unroll
  for (int x = 0; x < 3; ++x)
#pragma unroll
    for (int y = x + 1; y < 3; ++y) Sg[3 * y + x] = same ? Sg[3 * x + y] : Sg[3 * y + x];
  double* o = out + off[blockIdx.x];
  if (coords == 1) {
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 3; ++y) o[tr ? 3 * y + x : 3 * x + y] = Sg[3 * x + y];
    return;
  }
  if constexpr (!Step::HOM) {
    double V[9];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 3; ++y) V[3 * x + y] = hl.s4[x] * Sg[3 * x + y] * hm.s4[y];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 3; ++y) o[tr ? 3 * y + x : 3 * x + y] = same && x > y ? V[3 * y + x] : V[3 * x + y];
  } else {
    double Nl[4][3], Nm[4][3];  // N[i][p] = delta(i, p + 1) - beta w_i w_{p+1}
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        Nl[i][p] = (i == p + 1 ? 1.0 : 0.0) - hl.hbeta * hl.hw[i] * hl.hw[p + 1];
        Nm[i][p] = (i == p + 1 ? 1.0 : 0.0) - hm.hbeta * hm.hw[i] * hm.hw[p + 1];
      }
    double V[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double v = 0;
#pragma unroll
        for (int p = 0; p < 3; ++p) v += Nl[i][p] * (Sg[3 * p] * Nm[j][0] + Sg[3 * p + 1] * Nm[j][1] + Sg[3 * p + 2] * Nm[j][2]);
        V[4 * i + j] = hl.s4[i] * v * hm.s4[j];
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[tr ? 4 * j + i : 4 * i + j] = same && i > j ? V[4 * j + i] : V[4 * i + j];
  }
}

}  // namespace povar
