// mik_k_block.h -- block kriging (mik_predict_block): the estimate and the error variance of the arithmetic mean of Z over the nd
// discretisation nodes of a block, from the one resident inverse.  Included by mik_predict.hip after mik_k_predict.h.  Kernels:
// k_rhs_block (bbar), k_block_gamma (gbar), k_block_ss (sigma^2 - gbar).
//
// The resident points are the block centres (adjusted); node u of a block is centre + off[u], off the nd ADJUSTED offsets (T u, T =
// stretch . rot: the adjustment is linear, so one table serves every block).  With b(.) the right-hand side exactly as k_rhs forms it at
// a node (the exact_values zeroing per node, drift rows, the border row) and B = A^-1:
//     bbar   = (sum_u b(node_u)) / nd                      summed in node order, one division
//     z_V    = c . bbar
//     s2_V   = -gbar - bbar^T B bbar                       k_contract and k_ss_reduce unchanged on the panel of bbar (dense path)
//     gbar   = (sum_u sum_v gamma*(|off_u - off_v|)) / nd^2,   gamma*(d) = 0 if d <= eps, else the variogram at d
// which is the mean of the nd x nd block of mik_predict_cov's matrix on the nodes: the error variance of the mean of Z over the nodes
// (a nugget is variation of Z itself and averages down with nd).
//
//   k_rhs_block<MODEL, NDIM>                k_rhs's layout -- 8 blocks per workgroup, threads stride over j, point-major stores with
//                                           ld = Mp, the z reduction at the end, lane for lane in k_rhs's order -- with the offsets in LDS
//                                           and, per station column, a loop over the nodes.  nd = 1 (offset 0) is k_rhs bit for bit.
//   k_block_gamma<MODEL, NDIM>              one workgroup: gbar, once per call, in one fixed order
//   k_block_ss                              s2_V = ss - gbar behind the unchanged dense reduce: per point, whatever launch the point is in
#pragma once
#include "mik_k_predict.h"

namespace mik {

#define MIK_BLOCK_MAXND 512

struct BlockRhsArgs {
  RhsArgs r;
  const double* off;  // nd x ndim adjusted node offsets, row-major, node order (x fastest)
  int nd;
};

template <int MODEL, int NDIM>
__global__ void __launch_bounds__(256) k_rhs_block(const BlockRhsArgs ba) {
  const RhsArgs& a = ba.r;
  const int nd = ba.nd;
  __shared__ double red[4][MIK_TP];
  __shared__ double so[3][MIK_BLOCK_MAXND];
  for (int u = threadIdx.x; u < nd; u += 256) {
    so[0][u] = ba.off[(long)u * NDIM];
    so[1][u] = ba.off[(long)u * NDIM + 1];
    so[2][u] = (NDIM == 3) ? ba.off[(long)u * NDIM + 2] : 0.0;
  }
  __syncthreads();
  const int t0 = blockIdx.x * MIK_TP;
  double qx[MIK_TP], qy[MIK_TP], qz[MIK_TP];
  bool ok[MIK_TP];
#pragma unroll
  for (int q = 0; q < MIK_TP; ++q) {
    ok[q] = (t0 + q) < a.nvalid;
    const long idx = (long)(ok[q] ? t0 + q : 0);
    qx[q] = a.px[idx];
    qy[q] = a.py[idx];
    qz[q] = (NDIM == 3) ? a.pz[idx] : 0.0;
  }
  double zacc[MIK_TP];
#pragma unroll
  for (int q = 0; q < MIK_TP; ++q) zacc[q] = 0.0;
  const double rnd = (double)nd;

  for (int j = threadIdx.x; j < a.Mp; j += 256) {
    double val[MIK_TP];
#pragma unroll
    for (int q = 0; q < MIK_TP; ++q) val[q] = 0.0;
    if (j < a.N) {
      const double sx = a.xs[j], sy = a.ys[j], sz = (NDIM == 3) ? a.zs[j] : 0.0;
      for (int u = 0; u < nd; ++u) {
        const double ox = so[0][u], oy = so[1][u], oz = so[2][u];
#pragma unroll
        for (int q = 0; q < MIK_TP; ++q) {
          const double dx = (qx[q] + ox) - sx, dy = (qy[q] + oy) - sy;
          // the fused forms the compiler gives k_rhs's `dz * dz + dy * dy + dx * dx` / `dx * dx + dy * dy`, spelled out: which product of
          // a sum is left unfused is the compiler's choice per kernel, and nd = 1 has to round as k_rhs does
          double s2;
          if (NDIM == 3) {
            const double dz = (qz[q] + oz) - sz;
            s2 = fma(dx, dx, fma(dy, dy, dz * dz));
          } else {
            s2 = fma(dx, dx, dy * dy);
          }
          const double d = (MODEL == 2) ? 0.0 : sqrt(s2);  // gaussian needs d^2 only (k_rhs)
          double g = -vario<MODEL, true>(a.v, d, s2);
          if (a.exact && ((MODEL == 2) ? (s2 <= a.eps * a.eps) : (d <= a.eps))) g = 0.0;  // per node
          val[q] = u ? val[q] + g : g;
        }
      }
#pragma unroll
      for (int q = 0; q < MIK_TP; ++q) val[q] = val[q] / rnd;
    } else if (j < a.N + a.p) {
      int c = j - a.N;
      const double dc = a.dsc ? a.dsc[2 * c] : 0.0, ds = a.dsc ? a.dsc[2 * c + 1] : 1.0;
      int kind = 2;  // 0 regional-linear, 1 well, 2 extra (the host's, already averaged over the nodes)
      if (a.rl) {
        if (c < a.ndim) kind = 0; else c -= a.ndim;
      }
      if (kind == 2) {
        if (c < a.nwells) kind = 1; else c -= a.nwells;
      }
      if (kind == 2) {
#pragma unroll
        for (int q = 0; q < MIK_TP; ++q) val[q] = ok[q] ? a.extra[(long)c * a.extra_stride + (long)(t0 + q)] : 0.0;
      } else {  // the mean of the node coordinate / of the well term at the nodes, in node order
        for (int u = 0; u < nd; ++u) {
          const double ox = so[0][u], oy = so[1][u], oz = so[2][u];
#pragma unroll
          for (int q = 0; q < MIK_TP; ++q) {
            double dv;
            if (kind == 0) dv = (c == 0) ? qx[q] + ox : (c == 1 ? qy[q] + oy : qz[q] + oz);
            else dv = well_drift(qx[q] + ox, qy[q] + oy, a.wells + 3 * c);
            val[q] = u ? val[q] + dv : dv;
          }
        }
#pragma unroll
        for (int q = 0; q < MIK_TP; ++q) val[q] = val[q] / rnd;
      }
#pragma unroll
      for (int q = 0; q < MIK_TP; ++q) val[q] = a.dsc ? (val[q] - dc) * ds : val[q];
    } else {
      const double one = (j == a.N + a.p) ? 1.0 : 0.0;
#pragma unroll
      for (int q = 0; q < MIK_TP; ++q) val[q] = one;
    }
    const double cj = (j < a.M) ? a.cvec[j] : 0.0;
#pragma unroll
    for (int q = 0; q < MIK_TP; ++q) {
      const double v = ok[q] ? val[q] : 0.0;
      a.Bt[(long)(t0 + q) * a.ld + j] = v;
      zacc[q] += cj * v;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < MIK_TP; ++q) {
    double s = zacc[q];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < MIK_TP && (t0 + (int)threadIdx.x) < a.nvalid)
    a.zout[t0 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

struct BlockGammaArgs {
  const double* off;  // nd x ndim, as BlockRhsArgs
  int nd;
  Vario v;
  double eps;
  double* gbar;  // one double
};

// One workgroup of 256 threads: thread t sums the pairs k = t, t + 256, ... (k = u nd + v) in ascending order, the 256 sums meet in a
// binary tree, one division by nd^2.  Distances as the covariance's stage 0 forms them.
template <int MODEL, int NDIM>
__global__ void __launch_bounds__(256) k_block_gamma(const BlockGammaArgs a) {
  __shared__ double s[256];
  const long np = (long)a.nd * a.nd;
  double acc = 0.0;
  for (long k = threadIdx.x; k < np; k += 256) {
    const long u = k / a.nd, v = k - u * a.nd;
    const double dx = a.off[u * NDIM] - a.off[v * NDIM], dy = a.off[u * NDIM + 1] - a.off[v * NDIM + 1];
    double s2;
    if (NDIM == 3) {
      const double dz = a.off[u * NDIM + 2] - a.off[v * NDIM + 2];
      s2 = dz * dz + dy * dy + dx * dx;
    } else {
      s2 = dx * dx + dy * dy;
    }
    const double d = (MODEL == 2) ? 0.0 : sqrt(s2);
    const bool hit = (MODEL == 2) ? (s2 <= a.eps * a.eps) : (d <= a.eps);
    acc += hit ? 0.0 : vario<MODEL, true>(a.v, d, s2);
  }
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.gbar[0] = s[0] / ((double)a.nd * (double)a.nd);
}

// sigma^2_V = ss - gbar behind the dense reduce of a launch (ss = -sum_iblk part[iblk][t], k_ss_reduce's): a pass of its own, per point,
// whatever launch the point is in
__global__ void __launch_bounds__(256) k_block_ss(double* __restrict__ ss, int nvalid, const double* __restrict__ gbar) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nvalid) return;
  ss[t] = ss[t] - gbar[0];
}

}  // namespace mik
