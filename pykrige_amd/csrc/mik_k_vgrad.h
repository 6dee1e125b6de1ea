// mik_k_vgrad.h -- the kernels libmikvgrad.so (include/mikvgrad.h) adds to those of mik_k_vecchia.h, which it includes unchanged: the
// derivatives of the conditional variances and residuals of Vecchia's local systems, and their fixed-order reduction to d logdet and dG.
//
//   k_vgrad_solve<KPAD, MODEL>  k_vec_solve's layout -- one station per group of KPAD lanes, lane i holds row i of L in registers.  After the
//                               factorisation and y = L^-1 s it back-substitutes beta = L^-T y (for i = k_p - 1 .. 0 every lane k > i adds
//                               L_ki beta_k to a group sum and lane i finishes beta_i), forms t = D u for every parameter (each lane its row:
//                               distances against the shuffled coordinates, the three factors once per pair), takes the up to eight t_c
//                               through the factor together and writes d_k d_p and, against z = L^-1 w_c of every W column, d_k r_p(w)
//   k_vgrad_reduce              phase 0: one workgroup per (block of RB consecutive positions, parameter) adds the terms in position order;
//                               phase 1: one thread per entry adds the partials in block order
// The positions are worked in slabs of a multiple of RB positions; a partial sum never spans two slabs, so the bits do not depend on the
// slab length.  Every sum has a fixed order that depends on n alone; there is no atomic in this library.
#pragma once
#include "mik_k_vecchia.h"

namespace mvg {

using mvc::CG;
using mvc::MAXCOLS;
using mvc::Par;
using mvc::RB;
using mvc::RT;
using mvc::SOLVE_WAVES;
using mvc::group_sum;
using mvc::GAUSSIAN;
using mvc::EXPONENTIAL;
using mvc::SPHERICAL;
using mvc::HOLE_EFFECT;

constexpr int MAXGEOM = 5;           // MVG_MAXGEOM
constexpr int MAXPAR = 3 + MAXGEOM;  // psill, range, nugget, the geometry parameters
constexpr int DSTRIDE = MAXCOLS + 1;
constexpr int LDS_CU = 163840;  // bytes of LDS of a gfx950 compute unit
constexpr size_t vreduce_lds_bytes() { return sizeof(double) * RT * (mvc::RSTRIDE + DSTRIDE); }
static_assert(MAXPAR == CG, "the vectors t_c of all parameters go through the factor as one group of CG");
static_assert(vreduce_lds_bytes() <= 65536 && vreduce_lds_bytes() <= LDS_CU && LDS_CU == 163840, "k_vgrad_reduce does not fit the LDS of a CU");
static_assert(MAXCOLS * (MAXCOLS + 1) / 2 + 1 <= 4 * 256, "k_vgrad_reduce gives a thread at most four entries");

// The three factors of include/mikgrad.h at distance d of two distinct stations, operation for operation: dC_ij / dpsill = cp,
// dC_ij / drange = cr, dC_ij / dtheta_g = cg * w_g.
template <int MODEL>
__device__ inline void factors(const Par& mo, double d, double& cp, double& cr, double& cg) {
#pragma clang fp contract(off)
  if (MODEL == GAUSSIAN) {
    const double s = mo.range * 4.0 / 7.0;
    const double E = exp(-(d * d) / (s * s));
    cp = E;
    cr = mo.psill * E * ((2.0 * (d * d)) / ((s * s) * mo.range));
    cg = -(mo.psill * E * (2.0 / (s * s)));
  } else if (MODEL == EXPONENTIAL) {
    const double s = mo.range / 3.0;
    const double E = exp(-d / s);
    cp = E;
    cr = mo.psill * E * (d / (s * mo.range));
    cg = -((mo.psill * E / s) / d);
  } else if (MODEL == SPHERICAL) {
    const double r = mo.range;
    const bool in = d <= r;  // beyond the range every derivative is exactly 0
    cp = in ? 1.0 - ((3.0 * d) / (2.0 * r) - (d * d * d) / (2.0 * (r * r * r))) : 0.0;
    cr = in ? mo.psill * ((3.0 * d) / (2.0 * (r * r)) - (3.0 * (d * d * d)) / (2.0 * (r * r * r * r))) : 0.0;
    cg = in ? -((mo.psill * (3.0 / (2.0 * r) - (3.0 * (d * d)) / (2.0 * (r * r * r)))) / d) : 0.0;
  } else {
    const double q = d / (mo.range / 3.0);
    const double E = exp(-q);
    cp = (1.0 - q) * E;
    cr = mo.psill * (((2.0 - q) * E * q) / mo.range);
    cg = -((mo.psill * ((2.0 - q) * E / (mo.range / 3.0))) / d);
  }
  if (d == 0.0) cg = 0.0;
}

// The positions p0 .. p0 + np, one per group of KPAD lanes.  DR[(p - p0) * npar * (mcols + 1) + k * (mcols + 1) + c]: d_k r_p of column c,
// and in place mcols d_k d_p; npar = 3 + ng.  coords: ndim x n, dco: ng x ndim x n and W: mcols x n, all by station.  A position whose
// local system is not positive definite never gets here: mvg_plan_grad has answered it from k_vec_reduce before.
template <int KPAD, int MODEL>
__global__ __launch_bounds__(64 * SOLVE_WAVES) void k_vgrad_solve(const double* __restrict__ coords, int ndim, const double* __restrict__ dco,
                                                                  int ng, const int* __restrict__ order, const int* __restrict__ nbr, int n,
                                                                  int m, Par mo, const double* __restrict__ W, int mcols, int p0, int np,
                                                                  double* __restrict__ DR) {
#pragma clang fp contract(off)
  static_assert(KPAD == 16 || KPAD == 32 || KPAD == 64, "a size class divides the wave");
  constexpr int GROUPS = 64 / KPAD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane % KPAD;
  const int64_t q64 = ((int64_t)blockIdx.x * SOLVE_WAVES + wave) * GROUPS + lane / KPAD;
  const bool live = q64 < np;
  const int p = live ? p0 + (int)q64 : p0;  // (a group past the end repeats the slab's first position and writes nothing)
  const int kp = p < m ? p : m;
  const int st = order[p];
  const int listed = i < kp ? nbr[(int64_t)p * m + i] : -1;
  const bool mine = listed >= 0;
  const int si = mine ? listed : st;
  const double sill = mo.psill + mo.nugget;
  const double cx = coords[si], cy = coords[(int64_t)n + si], cz = ndim == 3 ? coords[2 * (int64_t)n + si] : 0.0;
  const double px = coords[st], py = coords[(int64_t)n + st], pz = ndim == 3 ? coords[2 * (int64_t)n + st] : 0.0;

  // row i of the neighbours' covariance matrix, its factor and y = L^-1 s: k_vec_solve's steps
  double x[KPAD];
#pragma unroll
  for (int j = 0; j < KPAD; ++j) {
    x[j] = j == i ? (mine ? sill : 1.0) : 0.0;
    if (j < m) {
      const double dx = cx - __shfl(cx, j, KPAD), dy = cy - __shfl(cy, j, KPAD);
      double d2 = dx * dx + dy * dy;
      if (ndim == 3) {
        const double dz = cz - __shfl(cz, j, KPAD);
        d2 = d2 + dz * dz;
      }
      const double c = mvc::covariance<MODEL>(mo, sqrt(d2));
      if (mine && j < i) x[j] = c;
    }
  }
#pragma unroll
  for (int j = 0; j < KPAD; ++j) {
    if (j < m) {
      double s = x[j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= x[k] * __shfl(x[k], j, KPAD);
      const double piv = __shfl(s, j, KPAD);
      const bool ok = piv > 0.0 && isfinite(piv);
      const double ljj = sqrt(ok ? piv : 1.0);
      x[j] = i == j ? ljj : (i > j ? s / ljj : 0.0);
    }
  }
  // the station's own column of the derivative matrices comes with its covariance: hx, d and the factors of the pair (i, p)
  double y, ocp, ocr, ocg, ohx, ohy, ohz = 0.0;
  {
    ohx = cx - px;
    ohy = cy - py;
    double d2 = ohx * ohx + ohy * ohy;
    if (ndim == 3) {
      ohz = cz - pz;
      d2 = d2 + ohz * ohz;
    }
    const double d = sqrt(d2);
    y = mine ? mvc::covariance<MODEL>(mo, d) : 0.0;
    factors<MODEL>(mo, d, ocp, ocr, ocg);
#pragma unroll
    for (int k = 0; k < KPAD; ++k) {
      if (k < m) {
        const double f = y / (i == k ? x[k] : 1.0);
        const double yk = __shfl(f, k, KPAD);
        y = i == k ? f : (i > k ? y - x[k] * yk : y);
      }
    }
  }
  // beta = L^-T y, from the last row up: lane i holds L_ij, so column j of L lies across the lanes and needs no transposition
  double beta = 0.0;
#pragma unroll
  for (int j = KPAD - 1; j >= 0; --j) {
    if (j < m) {
      const double s = group_sum<KPAD>(i > j ? x[j] * beta : 0.0);
      if (i == j) beta = (y - s) / x[j];
    }
  }
  // t = D u, u = [-beta ; 1]: t[k] is this lane's row of t_c -- the own column first, then the neighbours in list order -- and tp[k] the
  // station's own row
  double ex[MAXGEOM], ey[MAXGEOM], ez[MAXGEOM];  // the geometry sets' coordinates of this lane's station
#pragma unroll
  for (int g = 0; g < MAXGEOM; ++g) {
    const bool on = g < ng;
    const int64_t base = (int64_t)g * ndim * n;
    ex[g] = on ? dco[base + si] : 0.0;
    ey[g] = on ? dco[base + n + si] : 0.0;
    ez[g] = on && ndim == 3 ? dco[base + 2 * (int64_t)n + si] : 0.0;
  }
  double t[MAXPAR], tp[MAXPAR];
  t[0] = mine ? ocp : 0.0;
  t[1] = mine ? ocr : 0.0;
  t[2] = 0.0;
#pragma unroll
  for (int g = 0; g < MAXGEOM; ++g) {
    const bool on = g < ng;
    const int64_t base = (int64_t)g * ndim * n;
    const double fx = ex[g] - (on ? dco[base + st] : 0.0), fy = ey[g] - (on ? dco[base + n + st] : 0.0);
    double w = ohx * fx + ohy * fy;
    if (ndim == 3) {
      const double fz = ez[g] - (on ? dco[base + 2 * (int64_t)n + st] : 0.0);
      w = w + ohz * fz;
    }
    t[3 + g] = mine && on ? ocg * w : 0.0;
  }
#pragma unroll
  for (int k = 0; k < MAXPAR; ++k) tp[k] = (k == 0 || k == 2 ? 1.0 : 0.0) - (k == 2 ? 0.0 : group_sum<KPAD>(t[k] * beta));
  for (int j = 0; j < m; ++j) {
    const double bj = __shfl(beta, j, KPAD);
    const double hx = cx - __shfl(cx, j, KPAD), hy = cy - __shfl(cy, j, KPAD);
    double hz = 0.0;
    double d2 = hx * hx + hy * hy;
    if (ndim == 3) {
      hz = cz - __shfl(cz, j, KPAD);
      d2 = d2 + hz * hz;
    }
    double cp, cr, cg;
    factors<MODEL>(mo, sqrt(d2), cp, cr, cg);
    const bool pair = mine && j < kp && j != i;
    t[0] = t[0] - (pair ? cp : (mine && j == i ? 1.0 : 0.0)) * bj;
    t[1] = t[1] - (pair ? cr : 0.0) * bj;
#pragma unroll
    for (int g = 0; g < MAXGEOM; ++g) {
      if (g < ng) {  // (uniform)
        const double fx = ex[g] - __shfl(ex[g], j, KPAD), fy = ey[g] - __shfl(ey[g], j, KPAD);
        double w = hx * fx + hy * fy;
        if (ndim == 3) {
          const double fz = ez[g] - __shfl(ez[g], j, KPAD);
          w = w + hz * fz;
        }
        t[3 + g] = t[3 + g] - (pair ? cg * w : 0.0) * bj;
      }
    }
  }
  t[2] = mine ? 0.0 - beta : 0.0;  // dC / dnugget = I
  const int npar = 3 + ng, dstride = mcols + 1;
  const int64_t row = q64 * npar * dstride;
#pragma unroll
  for (int k = 0; k < MAXPAR; ++k) {
    if (k < npar) {
      const double dd = tp[k] - group_sum<KPAD>(beta * t[k]);  // d_k d_p = u^T t
      if (live && i == 0) DR[row + (int64_t)k * dstride + mcols] = dd;
    }
  }
  // the t_c of all parameters through the factor together: t <- L^-1 t_c
#pragma unroll
  for (int k = 0; k < KPAD; ++k) {
    if (k < m) {
      const double den = i == k ? x[k] : 1.0;
#pragma unroll
      for (int u = 0; u < MAXPAR; ++u) {
        const double f = t[u] / den;
        const double tk = __shfl(f, k, KPAD);
        t[u] = i == k ? f : (i > k ? t[u] - x[k] * tk : t[u]);
      }
    }
  }
  // the columns of W, CG at a time: z = L^-1 w_c, and d_k r_p(w) = -(z^T L^-1 t_c)
  for (int c0 = 0; c0 < mcols; c0 += CG) {
    double z[CG];
#pragma unroll
    for (int u = 0; u < CG; ++u) z[u] = (mine && c0 + u < mcols) ? W[(int64_t)(c0 + u) * n + si] : 0.0;
#pragma unroll
    for (int k = 0; k < KPAD; ++k) {
      if (k < m) {
        const double den = i == k ? x[k] : 1.0;
#pragma unroll
        for (int u = 0; u < CG; ++u) {
          const double f = z[u] / den;
          const double zk = __shfl(f, k, KPAD);
          z[u] = i == k ? f : (i > k ? z[u] - x[k] * zk : z[u]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < MAXPAR; ++k) {
      if (k < npar) {
#pragma unroll
        for (int u = 0; u < CG; ++u) {
          if (c0 + u < mcols) {  // (uniform)
            const double dot = group_sum<KPAD>(z[u] * t[k]);
            if (live && i == 0) DR[row + (int64_t)k * dstride + c0 + u] = 0.0 - dot;
          }
        }
      }
    }
  }
}

// phase 0: workgroup (blockIdx.x, k = blockIdx.y) adds, over the positions of block b = p0 / RB + blockIdx.x in position order, for every
// (a, b) of the lower triangle (dr_a r_b + r_a dr_b) / d - ((r_a r_b) dd) / (d d), and as entry ntri dd / d:
// part[(b * npar + k) * (ntri + 1) + e].  R: k_vec_solve's rows of all positions; DR: k_vgrad_solve's rows of the slab that starts at p0.
// phase 1: thread e of the grid adds the nblk partials of entry e in block order into out[e], e < npar (ntri + 1).
__global__ __launch_bounds__(256) void k_vgrad_reduce(const double* __restrict__ R, const double* __restrict__ DR, int n, int mcols, int npar,
                                                      int phase, int p0, double* __restrict__ part, int nblk, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double T[RT * mvc::RSTRIDE];
  __shared__ double TD[RT * DSTRIDE];
  const int t = threadIdx.x;
  const int ntri = mcols * (mcols + 1) / 2;
  if (phase == 1) {
    const int64_t e = (int64_t)blockIdx.x * 256 + t, all = (int64_t)npar * (ntri + 1);
    if (e < all) {
      double s = 0.0;
      for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * all + e];
      out[e] = s;
    }
    return;
  }
  const int stride = mcols + 2, dstride = mcols + 1, k = blockIdx.y;
  int ea[4], eb[4];
  double acc[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int e = t + 256 * v;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;  // e = a (a + 1) / 2 + b, b <= a
    ea[v] = a < mcols ? a : 0;               // (an entry past the triangle reads place 0 and is not stored)
    eb[v] = a < mcols ? e - a * (a + 1) / 2 : 0;
    acc[v] = 0.0;
  }
  const int64_t q0 = (int64_t)p0 + (int64_t)blockIdx.x * RB;  // the block's first position
  const int np = n - q0 < RB ? (int)(n - q0) : RB;
  for (int t0 = 0; t0 < np; t0 += RT) {
    const int rows = np - t0 < RT ? np - t0 : RT;
    __syncthreads();
    for (int e = t; e < rows * stride; e += 256) T[e] = R[(q0 + t0) * stride + e];
    for (int e = t; e < rows * dstride; e += 256) {
      const int r = e / dstride, c = e - r * dstride;
      TD[e] = DR[(((int64_t)blockIdx.x * RB + t0 + r) * npar + k) * dstride + c];
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const double d = T[r * stride + mcols], dd = TD[r * dstride + mcols];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int e = t + 256 * v;
        if (e < ntri) {
          const double ra = T[r * stride + ea[v]], rb = T[r * stride + eb[v]];
          const double da = TD[r * dstride + ea[v]], db = TD[r * dstride + eb[v]];
          acc[v] += (da * rb + ra * db) / d - ((ra * rb) * dd) / (d * d);
        } else if (e == ntri) {
          acc[v] += dd / d;
        }
      }
    }
  }
  const int64_t b = q0 / RB;
#pragma unroll
  for (int v = 0; v < 4; ++v)
    if (t + 256 * v <= ntri) part[(b * npar + k) * (int64_t)(ntri + 1) + t + 256 * v] = acc[v];
}

}  // namespace mvg
