// mik_k_cov.h -- the kriging error covariance between the resident points (mik_predict_cov) from the one resident inverse.  Included by
// mik_predict.hip after mik_k_predict.h.  Kernels: k_cov_gamma (stage 0), k_cov_gemm (stages 1 and 2).
//
// b(p) the right-hand side of point p exactly as k_rhs writes it (drift rows, the border row and the exact_values zeroing included),
// B = A^-1, e_p = Z(p) - z^(p).  Then
//     cov(e_p, e_q) = -gamma*(d_pq) - b(p)^T B b(q),      gamma*(d) = 0 if d <= eps (the exact-hit eps), else the variogram at d
// for ordinary and universal kriging alike; p = q is sigma^2 = -b^T B b.  A dense predict writes its panels into ONE point-major panel of
// all Pp = 128 ceil(P / 128) points (Bt_all, row stride Mp) and contracts from there, so z and sigma^2 are the ordinary predict's bits.
// A range-aware predict (compact-support variogram on a Hilbert-ordered factor) runs as always, for the same reason -- its panels hold
// delta on the candidate tiles only -- and Bt_all is written by one more dense k_rhs pass over the points (mik_predict.hip, predict_body).
//
//   stage 0   k_cov_gamma<MODEL, NDIM>                 C[p][q] = -gamma*(d_pq) for p < q < P, elementwise from the adjusted coordinates
//   stage 1   k_cov_gemm<NAI, 1>                       Yt = Bt_all B^T (Pp x Mp, row-major): gemm_core(A = Bt_all rows, B = rows of B),
//                                                      Yt[p][i] = sum_k b(p)_k B[i][k] = (B b(p))_i, a plain store
//   stage 2   k_cov_gemm<NAI, 2>                       the upper block triangle of 128 x 128 point tiles: acc = Bt_all[pblk] Yt[qblk]^T;
//                                                      for p < q (inside diagonal tiles too) C[p][q] - acc goes to [p][q] AND [q][p]:
//                                                      every off-diagonal element is computed once and written twice, so C is exactly
//                                                      symmetric; C[p][p] = the predict's sigma^2
// Both products run over k in [0, kend), kend = 16 ceil(M / 16), and rely on what k_contract relies on: k_rhs writes every column
// j < Mp of every row t < palloc of a launch's panel -- zeros in the padding columns [M, Mp) and in the rows of the points that do not
// exist [nvalid, palloc) (its `ok[q] ? val[q] : 0.0`).  Launches are equal multiples of 128 points and only the last one is short, so
// the rows [P, Pp) of Bt_all are that launch's zero rows: finite, and their products are never stored (the epilogues stop at P).
// Tiles are popped from k_contract's persistent per-XCD queues (pop_super_tile, mik_k_gaps.h), as k_gap_contract does; stage 2 walks the
// square of point blocks and drops the tiles below the diagonal at the pop (a queue position costs one atomic and two barriers).
// Every sum has one fixed order that depends on the point's place in the list alone, not on how the predict was cut into launches.
#pragma once
#include "mik_k_predict.h"

namespace mik {

struct CovGammaArgs {
  const double *px, *py, *pz;  // the resident adjusted coordinates (geographic: lon, lat in degrees)
  long npt;
  Vario v;
  double eps;
  double* C;  // row stride ldc
  long ldc;
};

// blockIdx.x = p, blockIdx.y = 256 consecutive q; distances exactly as k_rhs forms them (point p in the place of the point, q of the station)
template <int MODEL, int NDIM>
__global__ void __launch_bounds__(256) k_cov_gamma(const CovGammaArgs a) {
  const long p = blockIdx.x, q = (long)blockIdx.y * 256 + threadIdx.x;
  if (q <= p || q >= a.npt) return;
  double d, s2;
  if (NDIM == 1) {
    const double lp = a.py[p] * MIK_PI / 180.0, lq = a.py[q] * MIK_PI / 180.0;
    d = gc_dist(a.px[p], cos(lp), sin(lp), a.px[q], cos(lq), sin(lq));
    s2 = d * d;
  } else {
    const double dx = a.px[p] - a.px[q], dy = a.py[p] - a.py[q];
    if (NDIM == 3) {
      const double dz = a.pz[p] - a.pz[q];
      s2 = dz * dz + dy * dy + dx * dx;
    } else {
      s2 = dx * dx + dy * dy;
    }
    d = (MODEL == 2) ? 0.0 : sqrt(s2);  // gaussian needs d^2 only (k_rhs)
  }
  const bool hit = (MODEL == 2 && NDIM != 1) ? (s2 <= a.eps * a.eps) : (d <= a.eps);
  a.C[p * a.ldc + q] = hit ? 0.0 : -vario<MODEL, true>(a.v, d, s2);
}

struct CovGemmArgs {
  const double* Bt;  // Bt_all: Pp rows, row stride ld
  const double* T;   // the inverse, row stride ld (stage 1)
  double* Yt;        // Pp rows, row stride ld: written by stage 1, read by stage 2
  long ld;
  double* C;  // row stride ldc (stage 2)
  long ldc;
  const double* ss;  // the predict's sigma^2 (stage 2: the diagonal)
  long npt;
  int nPblk, nIblk, kend;
  unsigned long long* queue;
};

// Accumulator acc[ai][bi][r] is row 16 ai + 4 r + (lane >> 4) of the wave's rows (wm * 16 NAI ..), column wn * 64 + 16 bi + (lane & 15)
// of the block tile (gemm_core).
template <int NAI, int STAGE>
__global__ void __launch_bounds__(64 * 2 * (8 / NAI), 2 * (4 / NAI)) k_cov_gemm(const CovGemmArgs a) {
  __shared__ GemmSmem sm;
  const int xcd = xcd_id();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, lq = lane >> 4, lc = lane & 15;
  const int nBblk = STAGE == 1 ? a.nIblk : a.nPblk;  // blocks of the B operand: rows of the inverse / point blocks of Yt
  int steal = 0;
  for (;;) {
    int ablk = 0, bblk = 0;
    const int kind = pop_super_tile(a.queue, (xcd + steal) & 7, sm, a.nPblk, nBblk, ablk, bblk);
    if (kind == 2) {
      if (++steal == 8) return;
      continue;
    }
    if (kind == 1 || (STAGE == 2 && ablk > bblk)) continue;
    d4 acc[NAI][4];
#pragma unroll
    for (int x = 0; x < NAI; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) acc[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
    const double* Bg = STAGE == 1 ? a.T : a.Yt;
    gemm_core<NAI>(a.Bt + (long)ablk * MIK_BM * a.ld, a.ld, Bg + (long)bblk * MIK_BN * a.ld, a.ld, 0, a.kend, acc, sm);
#pragma unroll
    for (int ai = 0; ai < NAI; ++ai)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long p = (long)ablk * MIK_BM + wm * (16 * NAI) + 16 * ai + 4 * r + lq;
#pragma unroll
        for (int bi = 0; bi < 4; ++bi) {
          const long q = (long)bblk * MIK_BN + wn * 64 + 16 * bi + lc;
          if (STAGE == 1) {
            a.Yt[p * a.ld + q] = acc[ai][bi][r];  // (p < Pp, q < Mp: whole tiles)
          } else if (q < a.npt) {
            if (p < q) {
              const double v = a.C[p * a.ldc + q] - acc[ai][bi][r];
              a.C[p * a.ldc + q] = v;
              a.C[q * a.ldc + p] = v;
            } else if (p == q) {
              a.C[p * a.ldc + p] = a.ss[p];
            }
          }
        }
      }
  }
}

}  // namespace mik
