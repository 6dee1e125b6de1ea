// mik_k_cvfolds.h -- leave-group-out cross-validation from the inverse (mik_cross_validate_folds).  Included by mik_k_predict.h after
// mik_k_fields.h.  One kernel: k_cv_folds<FB, BIG>.
//
// A fold S of m stations, R everything else (border and drift rows included).  The kriging matrix has a zero diagonal on the station
// rows, so with B = A^-1 and c = B[:, :N] v the block inverse gives  B_SS^-1 = A_SS - A_SR A_RR^-1 A_RS  and hence
//     zhat_S = v_S - B_SS^-1 c_S,    sigma^2_S = diag(B_SS^-1).
// B_SS is symmetric positive definite (its inverse is the kriging-error covariance of the held-out group).  One workgroup of 256 threads
// per fold: gather G = B[S, S] (lower triangle), G = L L^T, W = L^-1 in place, then per block of FB fields  t = W c_S,  y = W^T t  and
// d_j = sum_i W_ij^2;  zhat = v_S - y and sigma^2 = d go straight to the station positions.  Every sum has one fixed order that depends on
// the fold's station list alone (not on the number of fields, the fold's label or its place in the grid): plane f is bit for bit the
// one-field result.  A non-positive or non-finite pivot gives NaN in the fold's entries and leaves the other folds alone.
//
//   BIG = false  m <= MIK_CVF_LDS: the block lives in LDS (row stride odd: rows and columns are both conflict-free for ds_read_b64,
//                whose bank is (byte address / 4) mod 64 over each half wave).
//   BIG = true   any m: the block lives in global scratch (m x m doubles, row stride m) and is worked in MIK_CVF_NB-column panels --
//                diagonal block factored and inverted in LDS, panel solve, trailing symmetric update, then the blocked triangular
//                inverse -- all by the fold's own workgroup, 64 x 64 tiles staged in LDS and a 4 x 4 register tile per thread.
#pragma once
#include "mik_k_fields.h"

namespace mik {

#define MIK_CVF_LDS 96  // largest fold factored whole in LDS: 96 x 97 doubles = 73 KB, under the 100 KB the sweep's diagonal kernel asks for
#define MIK_CVF_NB 64   // panel width and tile edge of the blocked class
#define MIK_CVF_TLD 65  // row stride of a 64 x 64 LDS tile (odd, see above)

struct CvfArgs {
  const double* B;    // the inverse, row stride ldb
  long ldb;
  const double* C;    // c = B[:, :N] V: plane f at C + f n (k_cvec_fields<FB>)
  const double* V;    // the fields, plane f at V + f n, zero planes up to a multiple of FB
  const int* idx;     // station positions (factor order) fold after fold, ascending inside a fold
  const long* desc;   // per workgroup of this launch: first entry of idx, m, first double of its block in scratch
  double* scratch;    // BIG: the m x m blocks
  double* wc;         // FB planes of n: c_S of the current block of fields, at the fold's place in idx
  double* wt;         // FB planes of n: t = W c_S likewise
  double* zhat;       // plane f at zhat + f n
  double* ss;
  long n;
  int nfb;            // blocks of FB fields
  int ldw;            // BIG = false: row stride of the LDS block (odd, >= the launch's largest m)
};

// Cholesky factor of the leading n x n lower triangle of D (LDS, row stride ld), in place; the upper triangle is neither read nor
// written.  False -- for every thread alike -- at a pivot that is not a positive finite number.  The caller has synchronised after
// filling D; D is synchronised on return.
__device__ __forceinline__ bool cvf_chol_lds(double* D, int ld, int n) {
  const int tid = threadIdx.x, tj = tid & 31, ti = tid >> 5;
  for (int k = 0; k < n; ++k) {
    const double p = D[k * ld + k];
    if (!(p > 0.0) || !(p <= 1.7976931348623157e308)) return false;
    const double r = sqrt(p);
    __syncthreads();  // every thread has read the pivot
    for (int i = k + 1 + tid; i < n; i += 256) D[i * ld + k] /= r;
    if (tid == 0) D[k * ld + k] = r;
    __syncthreads();
    for (int i = k + 1 + ti; i < n; i += 8) {  // a half wave walks one row: 32 consecutive doubles, the column entries ld apart
      const double a = D[i * ld + k];
      for (int j = k + 1 + tj; j <= i; j += 32) D[i * ld + j] -= a * D[j * ld + k];
    }
    __syncthreads();
  }
  return true;
}

// W = L^-1 of the leading n x n lower triangle of D (LDS), in place, column by column from the last (n <= 257: one thread per row
// below the diagonal).  Synchronised on return.
__device__ __forceinline__ void cvf_trinv_lds(double* D, int ld, int n) {
  const int tid = threadIdx.x;
  for (int j = n - 1; j >= 0; --j) {
    const double ajj = 1.0 / D[j * ld + j];
    const int i = j + 1 + tid;
    double s = 0.0;
    if (i < n)
      for (int k = j + 1; k <= i; ++k) s += D[i * ld + k] * D[k * ld + j];
    __syncthreads();  // column j and the diagonal entry have been read
    if (i < n) D[i * ld + j] = -s * ajj;
    if (tid == 0) D[j * ld + j] = ajj;
    __syncthreads();
  }
}

// 64 x 64 tile into LDS: T[r][c] (TR: T[c][r]) = src[r ld + c] for r < nr, c < nc (LOW: and c <= r), zero elsewhere
template <bool LOW, bool TR>
__device__ __forceinline__ void cvf_load(double* T, const double* src, long ld, int nr, int nc) {
  const int c = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < MIK_CVF_NB; r += 4) {
    double v = 0.0;
    if (r < nr && c < nc && (!LOW || c <= r)) v = src[(long)r * ld + c];
    T[TR ? c * MIK_CVF_TLD + r : r * MIK_CVF_TLD + c] = v;
  }
}

// acc[p][q] += sum_k A[tr + 16 p][k] Bt[tc + 16 q][k], k ascending (the rows a thread owns are 16 apart: the 16 rows of Bt a half
// wave reads lie on 16 different bank pairs, its two rows of A on two)
__device__ __forceinline__ void cvf_nt(const double* A, const double* Bt, double (&acc)[4][4]) {
  const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll 4
  for (int k = 0; k < MIK_CVF_NB; ++k) {
    double a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a[q] = A[(tr + 16 * q) * MIK_CVF_TLD + k];
      b[q] = Bt[(tc + 16 * q) * MIK_CVF_TLD + k];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[p][q] += a[p] * b[q];
  }
}

__device__ __forceinline__ void cvf_zero(double (&acc)[4][4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
}

// dst[r ld + c] = sign acc (SUB: dst -= acc) for the thread's entries with r < nr, c < nc
template <bool SUB>
__device__ __forceinline__ void cvf_store(double* dst, long ld, int nr, int nc, const double (&acc)[4][4], double sign) {
  const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = tr + 16 * p, c = tc + 16 * q;
      if (r < nr && c < nc) {
        double* d = dst + (long)r * ld + c;
        *d = SUB ? *d - acc[p][q] : sign * acc[p][q];
      }
    }
}

// The blocked class: G (global, m x m, row stride m, lower triangle filled) -> W = L^-1 in its lower triangle.  ta, tb: two LDS tiles.
// False for every thread at a bad pivot.
__device__ __forceinline__ bool cvf_factor_blocked(double* G, int m, double* ta, double* tb) {
  const int NB = MIK_CVF_NB, nblk = (m + NB - 1) / NB;
  const long ld = m;
  // G = L L^T, right-looking; the diagonal blocks are left as L_kk^-1 (what the panel solve and the inverse below both want)
  for (int kb = 0; kb < nblk; ++kb) {
    const int j0 = kb * NB, jb = min(NB, m - j0);
    double* gkk = G + (long)j0 * ld + j0;
    cvf_load<true, false>(ta, gkk, ld, jb, jb);
    __syncthreads();
    if (!cvf_chol_lds(ta, MIK_CVF_TLD, jb)) return false;
    cvf_trinv_lds(ta, MIK_CVF_TLD, jb);
    for (int r = threadIdx.x >> 6; r < jb; r += 4) {
      const int c = threadIdx.x & 63;
      if (c <= r) gkk[(long)r * ld + c] = ta[r * MIK_CVF_TLD + c];
    }
    // panel: L_ik = G_ik L_kk^-T, one 64-row tile after the other
    for (int ib = kb + 1; ib < nblk; ++ib) {
      const int nr = min(NB, m - ib * NB);
      double* gik = G + (long)ib * NB * ld + j0;
      cvf_load<false, false>(tb, gik, ld, nr, NB);
      __syncthreads();
      double acc[4][4];
      cvf_zero(acc);
      cvf_nt(tb, ta, acc);
      __syncthreads();  // tb has been read
      cvf_store<false>(gik, ld, nr, NB, acc, 1.0);
    }
    __syncthreads();  // the panel is in global memory (and ta free)
    // trailing update of the lower triangle: G_ij -= L_ik L_jk^T
    for (int ib = kb + 1; ib < nblk; ++ib) {
      const int nr = min(NB, m - ib * NB);
      cvf_load<false, false>(ta, G + (long)ib * NB * ld + j0, ld, nr, NB);
      for (int jbk = kb + 1; jbk <= ib; ++jbk) {
        const int nc = min(NB, m - jbk * NB);
        cvf_load<false, false>(tb, G + (long)jbk * NB * ld + j0, ld, nc, NB);
        __syncthreads();
        double acc[4][4];
        cvf_zero(acc);
        cvf_nt(ta, tb, acc);
        cvf_store<true>(G + (long)ib * NB * ld + (long)jbk * NB, ld, nr, nc, acc, 1.0);
        __syncthreads();  // tb (and, after the last one, ta) has been read; the update is in global memory
      }
    }
  }
  // W = L^-1, block column by block column from the last but one: X = L[j+1:, j];  X <- X W_jj;  X <- -W[j+1:, j+1:] X (block rows from
  // the last up, so that every block row still finds the old X of the rows above it)
  for (int jb = nblk - 2; jb >= 0; --jb) {
    const int j0 = jb * NB;
    cvf_load<true, true>(tb, G + (long)j0 * ld + j0, ld, NB, NB);  // tb[c][k] = W_jj[k][c]
    for (int ib = jb + 1; ib < nblk; ++ib) {
      const int nr = min(NB, m - ib * NB);
      double* gij = G + (long)ib * NB * ld + j0;
      cvf_load<false, false>(ta, gij, ld, nr, NB);
      __syncthreads();
      double acc[4][4];
      cvf_zero(acc);
      cvf_nt(ta, tb, acc);
      __syncthreads();  // ta has been read
      cvf_store<false>(gij, ld, nr, NB, acc, 1.0);
    }
    __syncthreads();
    for (int ib = nblk - 1; ib > jb; --ib) {
      const int nr = min(NB, m - ib * NB);
      double acc[4][4];
      cvf_zero(acc);
      for (int kb = jb + 1; kb <= ib; ++kb) {
        const int nk = min(NB, m - kb * NB);
        const double* wik = G + (long)ib * NB * ld + (long)kb * NB;
        if (kb == ib)
          cvf_load<true, false>(ta, wik, ld, nr, nk);
        else
          cvf_load<false, false>(ta, wik, ld, nr, nk);
        cvf_load<false, true>(tb, G + (long)kb * NB * ld + j0, ld, nk, NB);  // tb[c][k] = X_k[k][c]
        __syncthreads();
        cvf_nt(ta, tb, acc);
        __syncthreads();  // both tiles have been read (and, at kb == ib, the old X_i)
      }
      cvf_store<false>(G + (long)ib * NB * ld + j0, ld, nr, NB, acc, -1.0);
      __syncthreads();
    }
  }
  return true;
}

// zhat and sigma^2 of one fold from W = L^-1 (lower triangle, row stride ld; LDS or global), FB fields at a time.  idx: the fold's station
// positions, o0: its place in the work planes.
//   t_i = sum_{k <= i} W_ik c_k     one wave per row, lane k mod 64, then the xor butterfly (k_cvec's order)
//   y_j = sum_{i >= j} W_ij t_i     lane = column, wave w takes the rows 64 (j / 64) + w, + 4, ... in ascending order, then wave 0 + 1 + 2 + 3
//   d_j = sum_{i >= j} W_ij^2       likewise
template <int FB>
__device__ __forceinline__ void cvf_apply(const CvfArgs& a, const double* W, long ld, int m, const int* idx, long o0, bool ok) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long n = a.n;
  for (int fb = 0; fb < a.nfb; ++fb) {
    const long f0 = (long)fb * FB;
    if (!ok) {
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      for (int i = threadIdx.x; i < m; i += 256) {
        const long p = idx[i];
#pragma unroll
        for (int f = 0; f < FB; ++f) a.zhat[(f0 + f) * n + p] = nan;
        if (fb == 0) a.ss[p] = nan;
      }
      continue;
    }
    for (int i = threadIdx.x; i < m; i += 256) {
      const long p = idx[i];
#pragma unroll
      for (int f = 0; f < FB; ++f) a.wc[f * n + o0 + i] = a.C[(f0 + f) * n + p];
    }
    __syncthreads();
    for (int i = wave; i < m; i += 4) {
      double s[FB];
#pragma unroll
      for (int f = 0; f < FB; ++f) s[f] = 0.0;
      const double* w = W + (long)i * ld;
      for (int k = lane; k <= i; k += 64) {
        const double wk = w[k];
#pragma unroll
        for (int f = 0; f < FB; ++f) s[f] += wk * a.wc[f * n + o0 + k];
      }
#pragma unroll
      for (int f = 0; f < FB; ++f)
        for (int o = 32; o > 0; o >>= 1) s[f] += __shfl_xor(s[f], o);
      if (lane == 0) {
#pragma unroll
        for (int f = 0; f < FB; ++f) a.wt[f * n + o0 + i] = s[f];
      }
    }
    __syncthreads();
    for (int jc = 0; jc < m; jc += 64) {
      const int j = jc + lane;
      double y[FB + 1];  // y[FB] = d
#pragma unroll
      for (int f = 0; f <= FB; ++f) y[f] = 0.0;
      if (j < m) {
        for (int i = jc + wave; i < m; i += 4) {
          if (i < j) continue;
          const double wij = W[(long)i * ld + j];
#pragma unroll
          for (int f = 0; f < FB; ++f) y[f] += wij * a.wt[f * n + o0 + i];
          y[FB] += wij * wij;
        }
      }
      const long p = j < m ? (long)idx[j] : 0;
#pragma unroll
      for (int f = 0; f <= FB; ++f) {
        red[wave][lane] = y[f];
        __syncthreads();
        if (wave == 0 && j < m) {
          const double r = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
          if (f < FB)
            a.zhat[(f0 + f) * n + p] = a.V[(f0 + f) * n + p] - r;
          else if (fb == 0)
            a.ss[p] = r;
        }
        __syncthreads();
      }
    }
  }
}

// One workgroup per fold of the launch (a.desc: three longs per workgroup).  Dynamic LDS: BIG two 64 x 65 tiles, else m rows of a.ldw.
template <int FB, bool BIG>
__global__ void __launch_bounds__(256) k_cv_folds(const CvfArgs a) {
  extern __shared__ double cvf_lds[];
  const long* d = a.desc + 3 * (long)blockIdx.x;
  const long o0 = d[0];
  const int m = (int)d[1];
  const int* idx = a.idx + o0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (BIG) {
    double* G = a.scratch + d[2];
    for (int i = wave; i < m; i += 4) {
      const double* brow = a.B + (long)idx[i] * a.ldb;
      for (int j = lane; j <= i; j += 64) G[(long)i * m + j] = brow[idx[j]];
    }
    __syncthreads();
    const bool ok = cvf_factor_blocked(G, m, cvf_lds, cvf_lds + MIK_CVF_NB * MIK_CVF_TLD);
    __syncthreads();
    cvf_apply<FB>(a, G, (long)m, m, idx, o0, ok);
  } else {
    const int ldw = a.ldw;
    for (int i = wave; i < m; i += 4) {
      const double* brow = a.B + (long)idx[i] * a.ldb;
      for (int j = lane; j <= i; j += 64) cvf_lds[i * ldw + j] = brow[idx[j]];
    }
    __syncthreads();
    const bool ok = cvf_chol_lds(cvf_lds, ldw, m);
    if (ok) cvf_trinv_lds(cvf_lds, ldw, m);
    __syncthreads();
    cvf_apply<FB>(a, cvf_lds, (long)ldw, m, idx, o0, ok);
  }
}

}  // namespace mik
