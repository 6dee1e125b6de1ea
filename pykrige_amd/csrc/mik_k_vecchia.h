// mik_k_vecchia.h -- the kernels of libmikvecchia.so (include/mikvecchia.h): the neighbour sets of Vecchia's approximation, the small
// Cholesky factorisations of the local systems, and the fixed-order reduction to log det C^ and W^T C^-1 W.  Self-contained: includes nothing
// of the other libraries.
//
//   k_vec_knn<NDIM>          for 64 consecutive positions per workgroup (one wave, one query per lane) the m nearest predecessors by
//                            brute force: candidate coordinates go through LDS in tiles of TC, each lane keeps its m best sorted by
//                            (d2, position) in LDS columns of its own and rejects against its m-th best first
//   k_vec_solve<KPAD, MODEL> one station per group of KPAD lanes (64 / KPAD stations per wave): lane i holds row i of the neighbours'
//                            covariance matrix in registers, the factorisation runs left-looking with the rows of L broadcast between the
//                            lanes, the station's own row and the columns of W (8 at a time) go through the factor by forward substitution
//   k_vec_reduce             phase 0: partial sums over RB consecutive positions per workgroup; phase 1: one workgroup adds the partials in
//                            block order.  Also the smallest failing position.
// Every sum has a fixed order that depends on n alone; there is no atomic in this library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvc {

constexpr int MAXNB = 64;       // MVC_MAXNB: the neighbour bound, and the lanes of a wave
constexpr int MAXCOLS = 40;     // MVC_MAXCOLS
constexpr int CG = 8;           // columns of W taken through a factor together
constexpr int QB = 64;          // query positions of one k_vec_knn workgroup
constexpr int TC = 256;         // candidates staged through LDS at a time
constexpr int SOLVE_WAVES = 4;  // waves of one k_vec_solve workgroup
constexpr int RB = 1024;        // consecutive positions of one k_vec_reduce partial
constexpr int RT = 32;          // positions it stages through LDS at a time
constexpr int RSTRIDE = MAXCOLS + 2;
constexpr int LDS_CU = 163840;  // bytes of LDS of a gfx950 compute unit
enum { GAUSSIAN = 0, EXPONENTIAL = 1, SPHERICAL = 2, HOLE_EFFECT = 3 };

// k_vec_knn's dynamic LDS: the candidate tile, then m x QB distances and m x QB positions (slot-major: lane l's list is column l)
constexpr size_t knn_lds_bytes(int ndim, int m) { return sizeof(double) * ((size_t)ndim * TC + (size_t)m * QB) + sizeof(int) * (size_t)m * QB; }
constexpr size_t reduce_lds_bytes() { return sizeof(double) * RT * RSTRIDE; }
static_assert(knn_lds_bytes(3, MAXNB) <= 65536 && 2 * knn_lds_bytes(3, MAXNB) <= 163840, "two k_vec_knn workgroups do not fit the LDS of a CU");
static_assert(reduce_lds_bytes() <= 163840, "k_vec_reduce does not fit the LDS of a CU");
static_assert(LDS_CU == 163840 && MAXNB == 64 && QB == 64 && TC % QB == 0 && MAXCOLS % CG == 0, "the shapes the kernels are written for");
static_assert(MAXCOLS * (MAXCOLS + 1) / 2 + 1 <= 4 * 256, "k_vec_reduce gives a thread at most four entries");

struct Par {
  double psill, range, nugget;
};

// C_ij of two distinct stations at distance d: (psill + nugget) - gamma(d), the formulas of include/mikvecchia.h operation for operation
template <int MODEL>
__device__ inline double covariance(const Par& mo, double d) {
#pragma clang fp contract(off)
  const double sill = mo.psill + mo.nugget;
  double g;
  if (MODEL == GAUSSIAN) {
    const double s = mo.range * 4.0 / 7.0;
    g = mo.psill * (1.0 - exp(-(d * d) / (s * s))) + mo.nugget;
  } else if (MODEL == EXPONENTIAL) {
    g = mo.psill * (1.0 - exp(-d / (mo.range / 3.0))) + mo.nugget;
  } else if (MODEL == SPHERICAL) {
    g = d <= mo.range ? mo.psill * ((3.0 * d) / (2.0 * mo.range) - (d * d * d) / (2.0 * (mo.range * mo.range * mo.range))) + mo.nugget : sill;
  } else {
    const double q = d / (mo.range / 3.0);
    g = mo.psill * (1.0 - (1.0 - q) * exp(-q)) + mo.nugget;
  }
  return sill - g;
}

// nbr[p * m + j]: the station index of the j-th nearest predecessor of position p, -1 beyond min(m, p).  coords: NDIM x n by station;
// order[p]: the station at position p.  Workgroup blockIdx.x owns the positions of block gridDim.x - 1 - blockIdx.x: the blocks with the
// most predecessors to scan are handed out first.
template <int NDIM>
__global__ __launch_bounds__(QB) void k_vec_knn(const double* __restrict__ coords, const int* __restrict__ order, int n, int m,
                                                int* __restrict__ nbr) {
#pragma clang fp contract(off)
  extern __shared__ double smem[];
  double* tile = smem;                                   // [NDIM][TC]
  double* bd2 = smem + NDIM * TC;                        // [m][QB]
  int* bpos = reinterpret_cast<int*>(bd2 + (size_t)m * QB);  // [m][QB]
  const int lane = threadIdx.x;
  const int b = (int)(gridDim.x - 1 - blockIdx.x);
  const int64_t p64 = (int64_t)b * QB + lane;
  const bool live = p64 < n;
  const int p = live ? (int)p64 : 0;  // (a lane past the end scans nothing)
  double q[NDIM];
  {
    const int s = order[p];
#pragma unroll
    for (int c = 0; c < NDIM; ++c) q[c] = coords[(int64_t)c * n + s];
  }
  const int64_t last64 = (int64_t)b * QB + QB - 1;  // the candidates of this block are the positions below `last`
  const int last = last64 < n ? (int)last64 : n;
  int count = 0;
  double kth = INFINITY;  // the m-th best once the list is full
  for (int q0 = 0; q0 < last; q0 += TC) {
    __syncthreads();
    for (int e = lane; e < TC; e += QB) {
      if (q0 + e < last) {
        const int s = order[q0 + e];
#pragma unroll
        for (int c = 0; c < NDIM; ++c) tile[c * TC + e] = coords[(int64_t)c * n + s];
      }
    }
    __syncthreads();
    const int width = last - q0 < TC ? last - q0 : TC;
    const int mine = p - q0;  // this lane's candidates of the tile: e < mine
    for (int e = 0; e < width; ++e) {
      const double dx = tile[e] - q[0], dy = tile[TC + e] - q[1];
      double d2 = dx * dx + dy * dy;
      if (NDIM == 3) {
        const double dz = tile[2 * TC + e] - q[NDIM - 1];
        d2 = d2 + dz * dz;
      }
      if (e < mine && (count < m || d2 < kth)) {  // (a list that is not full takes every predecessor, also one at d2 = inf)
        // candidates come in ascending position, so an equal distance stays behind the entries already there
        int j = count < m ? count : m - 1;
        while (j > 0 && bd2[(j - 1) * QB + lane] > d2) {
          bd2[j * QB + lane] = bd2[(j - 1) * QB + lane];
          bpos[j * QB + lane] = bpos[(j - 1) * QB + lane];
          --j;
        }
        bd2[j * QB + lane] = d2;
        bpos[j * QB + lane] = q0 + e;
        if (count < m) ++count;
        if (count == m) kth = bd2[(m - 1) * QB + lane];
      }
    }
  }
  if (live)
    for (int j = 0; j < m; ++j) nbr[(int64_t)p * m + j] = j < count ? order[bpos[j * QB + lane]] : -1;
}

template <int KPAD>
__device__ inline double group_sum(double v) {  // the same bits in every lane of the group: a butterfly of commutative additions
#pragma unroll
  for (int o = KPAD / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, KPAD);
  return v;
}

// One station per group of KPAD lanes.  R[p * (mcols + 2) + c]: the residual of column c at position p, then d_p and log d_p; a position
// whose local system has a pivot <= 0 or not finite writes d_p = -1.  coords: ndim x n and W: mcols x n, both by station.
template <int KPAD, int MODEL>
__global__ __launch_bounds__(64 * SOLVE_WAVES) void k_vec_solve(const double* __restrict__ coords, int ndim, const int* __restrict__ order,
                                                                const int* __restrict__ nbr, int n, int m, Par mo,
                                                                const double* __restrict__ W, int mcols, double* __restrict__ R) {
#pragma clang fp contract(off)
  static_assert(KPAD == 16 || KPAD == 32 || KPAD == 64, "a size class divides the wave");
  constexpr int GROUPS = 64 / KPAD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane % KPAD;
  const int64_t p64 = ((int64_t)blockIdx.x * SOLVE_WAVES + wave) * GROUPS + lane / KPAD;
  const bool live = p64 < n;
  const int p = live ? (int)p64 : n - 1;  // (a group past the end repeats the last position and writes nothing)
  const int kp = p < m ? p : m;
  const int st = order[p];
  const int listed = i < kp ? nbr[(int64_t)p * m + i] : -1;
  const bool mine = listed >= 0;
  const int si = mine ? listed : st;
  const double sill = mo.psill + mo.nugget;
  const double cx = coords[si], cy = coords[(int64_t)n + si], cz = ndim == 3 ? coords[2 * (int64_t)n + si] : 0.0;
  const double px = coords[st], py = coords[(int64_t)n + st], pz = ndim == 3 ? coords[2 * (int64_t)n + st] : 0.0;

  // row i of the neighbours' covariance matrix; a lane beyond kp holds a row of the identity
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
      const double c = covariance<MODEL>(mo, sqrt(d2));
      if (mine && j < i) x[j] = c;
    }
  }
  // L L^T = S, left-looking: in step j every lane i >= j forms L_ij from its own row and row j of L, which lane j broadcasts
  bool bad = false;
#pragma unroll
  for (int j = 0; j < KPAD; ++j) {
    if (j < m) {
      double s = x[j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= x[k] * __shfl(x[k], j, KPAD);
      const double piv = __shfl(s, j, KPAD);
      const bool ok = piv > 0.0 && isfinite(piv);
      bad = bad || !ok;
      const double ljj = sqrt(ok ? piv : 1.0);
      x[j] = i == j ? ljj : (i > j ? s / ljj : 0.0);
    }
  }
  // the station's own row through the factor: y = L^-1 s, and the conditional variance d = C_pp - y^T y
  double y;
  {
    const double dx = cx - px, dy = cy - py;
    double d2 = dx * dx + dy * dy;
    if (ndim == 3) {
      const double dz = cz - pz;
      d2 = d2 + dz * dz;
    }
    y = mine ? covariance<MODEL>(mo, sqrt(d2)) : 0.0;
#pragma unroll
    for (int k = 0; k < KPAD; ++k) {
      if (k < m) {
        const double f = y / (i == k ? x[k] : 1.0);
        const double yk = __shfl(f, k, KPAD);
        y = i == k ? f : (i > k ? y - x[k] * yk : y);
      }
    }
  }
  const double d = sill - group_sum<KPAD>(y * y);
  bad = bad || !(d > 0.0) || !isfinite(d);
  const int64_t row = (int64_t)p * (mcols + 2);
  if (live && i == 0) {
    R[row + mcols] = bad ? -1.0 : d;
    R[row + mcols + 1] = bad ? 0.0 : log(d);
  }
  // the columns of W, CG at a time: z = L^-1 w_c, and the residual w_p - y^T z
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
    for (int u = 0; u < CG; ++u) {
      const double dot = group_sum<KPAD>(y * z[u]);
      if (live && i == 0 && c0 + u < mcols) R[row + c0 + u] = bad ? 0.0 : W[(int64_t)(c0 + u) * n + st] - dot;
    }
  }
}

// phase 0: workgroup b adds (r_a r_b) / d over the positions b RB .. (b + 1) RB in position order, one (a, b) of the lower triangle per
// thread and pass, entry ntri the sum of log d: part[b * (ntri + 1) + e]; partbad[b]: its smallest position with d not > 0, or INT_MAX.
// phase 1: one workgroup adds the nblk partials in block order into out[0 .. ntri], and the smallest failing position into outbad.
__global__ __launch_bounds__(256) void k_vec_reduce(const double* __restrict__ R, int n, int mcols, int phase, double* __restrict__ part,
                                                    int* __restrict__ partbad, int nblk, double* __restrict__ out, int* __restrict__ outbad) {
#pragma clang fp contract(off)
  __shared__ double T[RT * RSTRIDE];
  const int t = threadIdx.x;
  const int ntri = mcols * (mcols + 1) / 2;
  const int stride = mcols + 2;
  if (phase == 1) {
    for (int e = t; e <= ntri; e += 256) {
      double s = 0.0;
      for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * (ntri + 1) + e];
      out[e] = s;
    }
    if (t == 0) {
      int bad = INT_MAX;
      for (int b = 0; b < nblk; ++b) bad = partbad[b] < bad ? partbad[b] : bad;
      *outbad = bad;
    }
    return;
  }
  int ea[4], eb[4];
  double acc[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int e = t + 256 * v;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;  // e = a (a + 1) / 2 + b, b <= a
    ea[v] = a;
    eb[v] = e - a * (a + 1) / 2;
    if (e == ntri) ea[v] = eb[v] = mcols + 1;  // the sum of log d
    acc[v] = 0.0;
  }
  const int64_t p0 = (int64_t)blockIdx.x * RB;
  const int np = n - p0 < RB ? (int)(n - p0) : RB;
  int bad = INT_MAX;
  for (int t0 = 0; t0 < np; t0 += RT) {
    const int rows = np - t0 < RT ? np - t0 : RT;
    __syncthreads();
    for (int e = t; e < rows * stride; e += 256) T[e] = R[(p0 + t0) * stride + e];
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const double d = T[r * stride + mcols];
      if (!(d > 0.0) && bad == INT_MAX) bad = (int)(p0 + t0 + r);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int e = t + 256 * v;
        if (e < ntri)
          acc[v] += (T[r * stride + ea[v]] * T[r * stride + eb[v]]) / d;
        else if (e == ntri)
          acc[v] += T[r * stride + mcols + 1];
      }
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v)
    if (t + 256 * v <= ntri) part[(int64_t)blockIdx.x * (ntri + 1) + t + 256 * v] = acc[v];
  if (t == 0) partbad[blockIdx.x] = bad;  // (every thread saw the same rows)
}

}  // namespace mvc
