// mik_k_lik.h -- the kernels of libmiklik.so (include/miklik.h): the covariance matrix of a station set and its blocked right-looking
// Cholesky factorisation, carried through the rows W^T below it.  Self-contained: includes nothing of the other libraries.
//
// The matrix is the lower triangle of the augmented NP x NP square [[C, .], [W^T, 0]], NP = n + mpad, row-major with leading dimension
// ld = NP.  One block column k0 .. k0 + jb (jb = min(NB, n - k0)) is three launches:
//   k_lik_potrf  the jb x jb diagonal block, unblocked in LDS by one workgroup; finds the bad pivot
//   k_lik_trsm   the rows below it, X = A L^-T, 64 rows per workgroup (one wave, one row per lane, forward substitution in registers)
//   k_lik_syrk   the trailing lower-triangle tiles, A22 -= P P^T, 128 x 128 per workgroup on v_mfma_f64_16x16x4_f64
// The elimination stops after the first n columns: the rows of W^T have become Y = W^T L^-T and the bottom-right block -Y Y^T = -G.
// Lane map of v_mfma_f64_16x16x4_f64 (D = A B + C, 16 x 16 x 4): A lane l holds A[i = l & 15][k = l >> 4], B lane l holds
// B[k = l >> 4][j = l & 15], D lane l holds D[(l >> 4) + 4 r][l & 15] in element r of its four accumulators.
// Every sum has a fixed order; there is no atomic in this library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mlk {

constexpr int NB = 64;          // columns of one block column (the K of one trailing update)
constexpr int TS = 128;         // rows and columns of one update tile: 4 waves as 2 x 2, a wave 64 x 64 = 4 x 4 MFMA tiles
constexpr int KT = 32;          // k staged through LDS at a time by k_lik_syrk
constexpr int SP = KT + 4;      // its LDS row stride: lane (i, kq) reads double 36 i + kq -- 64 different banks pairs for i < 16, kq < 4
constexpr int TRSM_ROWS = 64;   // rows of one k_lik_trsm workgroup
constexpr int LS = NB + 1;      // LDS row stride where every lane walks a row of its own
constexpr int AT = 64;          // tile of k_lik_assemble
constexpr int LDS_CU = 163840;  // bytes of LDS of a gfx950 compute unit
enum { GAUSSIAN = 0, EXPONENTIAL = 1, SPHERICAL = 2, HOLE_EFFECT = 3 };

constexpr size_t potrf_lds_bytes() { return sizeof(double) * NB * LS; }
constexpr size_t trsm_lds_bytes() { return sizeof(double) * (NB * NB + TRSM_ROWS * LS); }
constexpr size_t syrk_lds_bytes() { return sizeof(double) * 2 * TS * SP; }
static_assert(NB % KT == 0 && KT % 4 == 0 && TS == 128 && NB <= 64, "the tiling k_lik_syrk and k_lik_trsm are written for");
static_assert(potrf_lds_bytes() <= LDS_CU, "k_lik_potrf does not fit the LDS of a CU");
static_assert(2 * trsm_lds_bytes() <= LDS_CU, "two k_lik_trsm workgroups do not fit the LDS of a CU");
static_assert(2 * syrk_lds_bytes() <= LDS_CU, "two k_lik_syrk workgroups do not fit the LDS of a CU");

typedef double d4 __attribute__((ext_vector_type(4)));

struct Model {
  int id;
  double psill, range, nugget;
};

// C_ij of two distinct stations at distance d: (psill + nugget) - gamma(d), the formulas of include/miklik.h operation for operation
__device__ inline double covariance(const Model& mo, double d) {
#pragma clang fp contract(off)
  const double sill = mo.psill + mo.nugget;
  double g;
  if (mo.id == GAUSSIAN) {
    const double s = mo.range * 4.0 / 7.0;
    g = mo.psill * (1.0 - exp(-(d * d) / (s * s))) + mo.nugget;
  } else if (mo.id == EXPONENTIAL) {
    g = mo.psill * (1.0 - exp(-d / (mo.range / 3.0))) + mo.nugget;
  } else if (mo.id == SPHERICAL) {
    g = d <= mo.range ? mo.psill * ((3.0 * d) / (2.0 * mo.range) - (d * d * d) / (2.0 * (mo.range * mo.range * mo.range))) + mo.nugget : sill;
  } else {
    const double q = d / (mo.range / 3.0);
    g = mo.psill * (1.0 - (1.0 - q) * exp(-q)) + mo.nugget;
  }
  return sill - g;
}

// The lower triangle of [[C, .], [W^T, 0]], one AT x AT tile per workgroup (tiles above the diagonal return at once).
// coords: ndim x n; W: m x n; rows n + m .. NP - 1 and the bottom-right block are zero.
__global__ __launch_bounds__(256) void k_lik_assemble(double* __restrict__ A, int64_t ld, int n, int NP, int ndim,
                                                      const double* __restrict__ coords, Model mo, const double* __restrict__ W, int m) {
#pragma clang fp contract(off)
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj > ti) return;
  const int j = tj * AT + (threadIdx.x & (AT - 1));
  if (j >= NP) return;
  double xj = 0.0, yj = 0.0, zj = 0.0;
  if (j < n) {
    xj = coords[j];
    yj = coords[(int64_t)n + j];
    if (ndim == 3) zj = coords[2 * (int64_t)n + j];
  }
  for (int r = threadIdx.x / AT; r < AT; r += 256 / AT) {
    const int i = ti * AT + r;
    if (i >= NP || j > i) continue;
    double v = 0.0;
    if (i < n) {
      if (i == j) {
        v = mo.psill + mo.nugget;
      } else {
        const double dx = coords[i] - xj, dy = coords[(int64_t)n + i] - yj;
        double d2 = dx * dx + dy * dy;
        if (ndim == 3) {
          const double dz = coords[2 * (int64_t)n + i] - zj;
          d2 = d2 + dz * dz;
        }
        v = covariance(mo, sqrt(d2));
      }
    } else if (j < n && i - n < m) {
      v = W[(int64_t)(i - n) * n + j];
    }
    A[(int64_t)i * ld + j] = v;
  }
}

// The diagonal block A[k0 .. k0 + jb)^2 -> its Cholesky factor, in place; diag[k0 + i] = L_ii.  One workgroup; the block sits in LDS.
// A pivot <= 0 or not finite: *info = its 1-based column, and the workgroup returns without writing anything else.
__global__ __launch_bounds__(256) void k_lik_potrf(double* __restrict__ A, int64_t ld, int k0, int jb, double* __restrict__ diag,
                                                   int* __restrict__ info) {
  __shared__ double S[NB * LS];
  const int t = threadIdx.x;
  for (int e = t; e < NB * NB; e += 256) {
    const int i = e / NB, j = e % NB;
    S[i * LS + j] = (i < jb && j <= i) ? A[(int64_t)(k0 + i) * ld + k0 + j] : 0.0;
  }
  __syncthreads();
  const int i = t >> 2, jq = t & 3;  // the lane's row and its columns jq, jq + 4, ...
  for (int k = 0; k < jb; ++k) {
    const double p = S[k * LS + k];
    if (!(p > 0.0) || !isfinite(p)) {  // (the same p in every lane: the whole workgroup leaves)
      if (t == 0) *info = k0 + k + 1;
      return;
    }
    const double l = sqrt(p);
    __syncthreads();
    if (t == k)
      S[k * LS + k] = l;
    else if (t > k && t < jb)
      S[t * LS + k] /= l;
    __syncthreads();
    if (i > k && i < jb) {
      const double lik = S[i * LS + k];
      for (int j = jq + ((k + 1 - jq + 3) & ~3); j <= i; j += 4) S[i * LS + j] -= lik * S[j * LS + k];
    }
    __syncthreads();
  }
  for (int e = t; e < NB * NB; e += 256) {
    const int r = e / NB, j = e % NB;
    if (r < jb && j <= r) A[(int64_t)(k0 + r) * ld + k0 + j] = S[r * LS + j];
  }
  if (t < jb) diag[k0 + t] = S[t * LS + t];
}

// The rows r0 .. NP below the factored block: X = A[:, k0 .. k0 + jb) L^-T in place, TRSM_ROWS rows per workgroup of one wave.
// Lane t solves row t by forward substitution with the row in registers; L is read as LDS broadcasts.
__global__ __launch_bounds__(64) void k_lik_trsm(double* __restrict__ A, int64_t ld, int k0, int jb, int r0, int NP) {
  __shared__ double L[NB * NB];
  __shared__ double X[TRSM_ROWS * LS];
  const int t = threadIdx.x;
  const int row0 = r0 + blockIdx.x * TRSM_ROWS;
  for (int e = t; e < NB * NB; e += 64) {
    const int i = e / NB, j = e % NB;
    double v = i == j ? 1.0 : 0.0;  // (a short last block: an identity below it, so that the columns past jb stay zero)
    if (i < jb && j <= i) v = A[(int64_t)(k0 + i) * ld + k0 + j];
    L[i * NB + j] = v;
  }
  for (int e = t; e < TRSM_ROWS * NB; e += 64) {
    const int i = e / NB, j = e % NB;
    const int gi = row0 + i;
    X[i * LS + j] = (gi < NP && j < jb) ? A[(int64_t)gi * ld + k0 + j] : 0.0;
  }
  __syncthreads();
  double x[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    double s = X[t * LS + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= x[k] * L[j * NB + k];
    x[j] = s / L[j * NB + j];
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) X[t * LS + j] = x[j];
  __syncthreads();
  for (int e = t; e < TRSM_ROWS * NB; e += 64) {
    const int i = e / NB, j = e % NB;
    const int gi = row0 + i;
    if (gi < NP && j < jb) A[(int64_t)gi * ld + k0 + j] = X[i * LS + j];
  }
}

// The trailing update: for the rows and columns r0 .. NP, A[i][j] -= sum_k P[i][k] P[j][k] with P = A[:, k0 .. k0 + jb), lower triangle
// only.  Workgroup b owns tile (ti, tj), tj <= ti, b = ti (ti + 1) / 2 + tj, of TS x TS entries; its 4 waves are 2 x 2, each 64 x 64.
__global__ __launch_bounds__(256, 2) void k_lik_syrk(double* __restrict__ A, int64_t ld, int k0, int jb, int r0, int NP) {
  __shared__ double sA[TS * SP];
  __shared__ double sB[TS * SP];
  const int t = threadIdx.x, l = t & 63, w = t >> 6, wi = w >> 1, wj = w & 1;
  const int b = blockIdx.x;
  int ti = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((int64_t)(ti + 1) * (ti + 2) / 2 <= b) ++ti;
  while ((int64_t)ti * (ti + 1) / 2 > b) --ti;
  const int tj = b - (int)((int64_t)ti * (ti + 1) / 2);
  const int rowA = r0 + ti * TS, rowB = r0 + tj * TS;
  const bool idle = ti == tj && wj > wi;  // the wave's 64 x 64 lies above the diagonal
  d4 acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int kp = 0; kp < jb; kp += KT) {
    for (int e = t; e < TS * KT; e += 256) {
      const int r = e / KT, k = e % KT;
      const bool ink = kp + k < jb;
      const int ga = rowA + r, gb = rowB + r;
      sA[r * SP + k] = (ink && ga < NP) ? A[(int64_t)ga * ld + k0 + kp + k] : 0.0;
      sB[r * SP + k] = (ink && gb < NP) ? A[(int64_t)gb * ld + k0 + kp + k] : 0.0;
    }
    __syncthreads();
    if (!idle) {
#pragma unroll
      for (int ks = 0; ks < KT; ks += 4) {
        double a[4], bb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = sA[(wi * 64 + 16 * u + (l & 15)) * SP + ks + (l >> 4)];
#pragma unroll
        for (int v = 0; v < 4; ++v) bb[v] = sB[(wj * 64 + 16 * v + (l & 15)) * SP + ks + (l >> 4)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], bb[v], acc[u][v], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (idle) return;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = rowA + wi * 64 + 16 * u + 4 * r + (l >> 4), gj = rowB + wj * 64 + 16 * v + (l & 15);
        if (gi < NP && gj <= gi) A[(int64_t)gi * ld + gj] -= acc[u][v][r];
      }
}

}  // namespace mlk
