// mik_k_grad.h -- the kernels of libmikgrad.so (include/mikgrad.h) beside the four elimination kernels it takes from mik_k_lik.h:
//   k_grad_seed   the identity rows and the zero blocks below [[C, .], [W^T, 0]]
//   k_grad_pairs  one pass over the lower triangle of -Q = -C^-1: per 64 x 64 tile the sums of M_ij D_k,ij and a_if a_jf D_k,ij
// The matrix is the lower triangle of the NQ x NQ square [[C, ., .], [W^T, 0, .], [I, 0, 0]], NQ = 2 n + mpad, row-major, ld = NQ.
// Identity row i is zero left of column i, so at block column k0 (width jb) the rows that take part are the contiguous range
// [k0 + jb, n + mpad + k0 + jb): the host passes that upper end to k_lik_trsm and k_lik_syrk as their NP.
// Every sum has a fixed order; there is no atomic in this library.
#pragma once
#include "mik_k_lik.h"

namespace mlg {

using mlk::Model;

constexpr int GT = 64;                 // rows and columns of one k_grad_pairs tile: lane = column, the 4 waves take the rows 4 apart
constexpr int FC = 8;                  // fields of one chunk (blockIdx.y)
constexpr int MAXG = 5;                // geometry parameters
constexpr int MAXP = 8;                // trend columns
constexpr int ROWS = 2 + MAXG + 1;     // rows of a tile's partial sums: psill, range, geometry 0 .. 4 (pairs i > j), the diagonal
constexpr int COLS = 1 + FC;           // columns: the trace term, then the chunk's fields
constexpr int NV = ROWS * COLS;        // 72 numbers per tile and chunk
constexpr int LDS_CU = 163840;         // bytes of LDS of a gfx950 compute unit
constexpr size_t pairs_lds_bytes() { return sizeof(double) * 4 * NV; }
static_assert(pairs_lds_bytes() <= LDS_CU, "k_grad_pairs does not fit the LDS of a CU");
static_assert(GT == 64 && FC == 8, "k_grad_pairs is written for a column per lane and eight fields per chunk");

struct Factors {
  double cp, cr, cg;
};

// The three factors of include/mikgrad.h at distance d of two distinct stations, operation for operation.
__device__ inline Factors factors(const Model& mo, double d) {
#pragma clang fp contract(off)
  Factors f;
  if (mo.id == mlk::GAUSSIAN) {
    const double s = mo.range * 4.0 / 7.0;
    const double E = exp(-(d * d) / (s * s));
    f.cp = E;
    f.cr = mo.psill * E * ((2.0 * (d * d)) / ((s * s) * mo.range));
    f.cg = -(mo.psill * E * (2.0 / (s * s)));
  } else if (mo.id == mlk::EXPONENTIAL) {
    const double s = mo.range / 3.0;
    const double E = exp(-d / s);
    f.cp = E;
    f.cr = mo.psill * E * (d / (s * mo.range));
    f.cg = -((mo.psill * E / s) / d);
  } else if (mo.id == mlk::SPHERICAL) {
    const double r = mo.range;
    if (d <= r) {
      f.cp = 1.0 - ((3.0 * d) / (2.0 * r) - (d * d * d) / (2.0 * (r * r * r)));
      f.cr = mo.psill * ((3.0 * d) / (2.0 * (r * r)) - (3.0 * (d * d * d)) / (2.0 * (r * r * r * r)));
      f.cg = -((mo.psill * (3.0 / (2.0 * r) - (3.0 * (d * d)) / (2.0 * (r * r * r)))) / d);
    } else {
      f.cp = 0.0;
      f.cr = 0.0;
      f.cg = 0.0;
    }
  } else {
    const double q = d / (mo.range / 3.0);
    const double E = exp(-q);
    f.cp = (1.0 - q) * E;
    f.cr = mo.psill * (((2.0 - q) * E * q) / mo.range);
    f.cg = -((mo.psill * ((2.0 - q) * E / (mo.range / 3.0))) / d);
  }
  if (d == 0.0) f.cg = 0.0;
  return f;
}

// Rows nw .. nw + n of the square (nw = n + mpad): row nw + i holds 1 in column i and 0 in every other column of its lower triangle.
__global__ __launch_bounds__(256) void k_grad_seed(double* __restrict__ A, int64_t ld, int n, int nw) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int i = blockIdx.y; i < n; i += gridDim.y)
    if (j <= (int64_t)nw + i) A[((int64_t)nw + i) * ld + j] = j == i ? 1.0 : 0.0;
}

// Tile b = ti (ti + 1) / 2 + tj, tj <= ti, of the lower triangle of Qn = -Q (n x n inside the square, leading dimension ld); chunk
// blockIdx.y holds the fields FC blockIdx.y .. of a (F x n).  For the pairs i > j of the tile, with D_k the derivative factors of
// include/mikgrad.h and M_ij = Q_ij - sum_c U_ci U_cj (reml; U is p x n) or Q_ij:
//   part[row k][0] = sum M_ij D_k,ij,  part[row k][1 + f] = sum a_fi a_fj D_k,ij,  k = psill, range, geometry 0 .. ng - 1
// and for i = j, in the last row, sum M_ii and sum a_fi^2.  Each thread adds its pairs in row order, a wave adds its lanes by a fixed
// tree of shuffles, the four waves are added in order; part: (chunks x tiles x NV), added by the host in tile order.
__global__ __launch_bounds__(256) void k_grad_pairs(const double* __restrict__ Qn, int64_t ld, int n, int ndim,
                                                    const double* __restrict__ coords, int ng, const double* __restrict__ dcoords, Model mo,
                                                    int reml, int p, const double* __restrict__ U, int F, const double* __restrict__ a,
                                                    double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4 * NV];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = blockIdx.x;
  int ti = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((int64_t)(ti + 1) * (ti + 2) / 2 <= b) ++ti;
  while ((int64_t)ti * (ti + 1) / 2 > b) --ti;
  const int tj = b - (int)((int64_t)ti * (ti + 1) / 2);
  const int f0 = blockIdx.y * FC;
  const int j = tj * GT + lane;
  const bool jin = j < n;
  double xj[3] = {0.0, 0.0, 0.0}, ej[MAXG][3], uj[MAXP], aj[FC];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (jin && c < ndim) xj[c] = coords[(int64_t)c * n + j];
#pragma unroll
  for (int g = 0; g < MAXG; ++g)
#pragma unroll
    for (int c = 0; c < 3; ++c) ej[g][c] = (jin && g < ng && c < ndim) ? dcoords[((int64_t)g * ndim + c) * n + j] : 0.0;
#pragma unroll
  for (int c = 0; c < MAXP; ++c) uj[c] = (jin && reml && c < p) ? U[(int64_t)c * n + j] : 0.0;
#pragma unroll
  for (int f = 0; f < FC; ++f) aj[f] = (jin && f0 + f < F) ? a[(int64_t)(f0 + f) * n + j] : 0.0;
  double acc[ROWS][COLS];
#pragma unroll
  for (int k = 0; k < ROWS; ++k)
#pragma unroll
    for (int c = 0; c < COLS; ++c) acc[k][c] = 0.0;

  for (int r = w; r < GT; r += 4) {
    const int i = ti * GT + r;  // (the same row in every lane of the wave)
    if (i >= n) break;
    if (!jin || j > i) continue;
    double m = 0.0 - Qn[(int64_t)i * ld + j];
    if (reml) {
#pragma unroll
      for (int c = 0; c < MAXP; ++c)
        if (c < p) m = m - U[(int64_t)c * n + i] * uj[c];
    }
    double ww[FC];
#pragma unroll
    for (int f = 0; f < FC; ++f) ww[f] = (f0 + f < F ? a[(int64_t)(f0 + f) * n + i] : 0.0) * aj[f];
    if (j == i) {
      acc[ROWS - 1][0] = acc[ROWS - 1][0] + m;
#pragma unroll
      for (int f = 0; f < FC; ++f) acc[ROWS - 1][1 + f] = acc[ROWS - 1][1 + f] + ww[f];
      continue;
    }
    double h[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < ndim) h[c] = coords[(int64_t)c * n + i] - xj[c];
    double d2 = h[0] * h[0] + h[1] * h[1];
    if (ndim == 3) d2 = d2 + h[2] * h[2];
    const Factors fa = factors(mo, sqrt(d2));
    double D[2 + MAXG];
    D[0] = fa.cp;
    D[1] = fa.cr;
#pragma unroll
    for (int g = 0; g < MAXG; ++g) {
      D[2 + g] = 0.0;
      if (g < ng) {
        double wg = h[0] * (dcoords[((int64_t)g * ndim + 0) * n + i] - ej[g][0]) + h[1] * (dcoords[((int64_t)g * ndim + 1) * n + i] - ej[g][1]);
        if (ndim == 3) wg = wg + h[2] * (dcoords[((int64_t)g * ndim + 2) * n + i] - ej[g][2]);
        D[2 + g] = fa.cg * wg;
      }
    }
#pragma unroll
    for (int k = 0; k < 2 + MAXG; ++k) {
      if (k < 2 + ng) {
        acc[k][0] = acc[k][0] + m * D[k];
#pragma unroll
        for (int f = 0; f < FC; ++f) acc[k][1 + f] = acc[k][1 + f] + ww[f] * D[k];
      }
    }
  }
  // lanes -> lane 0 of each wave by a fixed tree; every lane of the workgroup is here
#pragma unroll
  for (int k = 0; k < ROWS; ++k)
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
      double v = acc[k][c];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
      if (lane == 0) red[w * NV + k * COLS + c] = v;
    }
  __syncthreads();
  if (t < NV) {
    const double s = ((red[t] + red[NV + t]) + red[2 * NV + t]) + red[3 * NV + t];
    part[((int64_t)blockIdx.y * gridDim.x + b) * NV + t] = s;
  }
}

}  // namespace mlg
