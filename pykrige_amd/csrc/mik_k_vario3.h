// mik_k_vario3.h -- device code of libmikvario3.so (include/mikvario3.h): directional semivariograms and variogram maps of F value fields
// over one 3-D station set, all pairs i < j.  Self-contained: nothing of mik_k_vario.h (the 2-D tool) is included or shared.
//
//   k_vario3_dir   lag bin x direction histogram of one chunk of <= 8 fields
//   k_vario3_map   lag-vector cell histogram (one half of the point-symmetric 3-D map) of one chunk of <= 8 fields
//   k_vario3_sum   the workgroups' partial sums added in workgroup order;  k_vario3_sum_cnt  the same for the 64-bit counts
//
// Both histogram kernels are persistent: the grid is a few workgroups per CU and strides over the upper-triangle tiles of 64 x 64 pairs.  A
// tile's coordinates and its chunk of values sit in LDS; a thread owns one column station (x, y, z and eight values in registers) and walks
// 16 row stations, which are wave-uniform LDS reads (broadcasts).  The bin (or cell) and the direction membership of a pair are computed
// once and serve every field of the chunk.  The unit vectors of the directions stay in the kernel arguments: the loop over them is uniform,
// so they are read into scalar registers and cost no vector register.  The histogram lives in LDS for the whole kernel -- 32-bit counts,
// flushed to the workgroup's 64-bit partial counts every 2^19 tiles (a tile adds at most 4096 to a cell), a float64 lag sum and one float64
// semivariance sum per field -- and is written out once.  Small histograms are kept in 2 or 4 copies, one per wave (pair), which divides
// the collisions of the LDS atomics.
// The arithmetic of the decisions is the header's, operation for operation: no contraction into fused multiply-adds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mkv3 {

constexpr int TILE = 64, THREADS = 256, FCHUNK = 8, MAXDIRS = 16, MAXLAGS = 64;
constexpr long FLUSH_TILES = 1L << 19;

struct Vario3Args {
  const double *x, *y, *z, *v;  // stations; v: the chunk's fields, nfc x n
  long n, ntiles;               // stations, upper-triangle tiles nt (nt + 1) / 2
  int nt, nfc, first;           // tiles per side, fields of this chunk, first chunk (counts and lag sums are accumulated)
  int cells, copies;            // histogram cells (directions x lags, or half the map), copies of the histogram in LDS (1, 2 or 4)
  // directions
  const double* edges;
  int nlags, na, all, band;     // all: tol_deg == 90, every pair belongs to every direction; band: a bandwidth was given
  double ux[MAXDIRS], uy[MAXDIRS], uz[MAXDIRS], tan2, bw2;
  // map
  int mnx, mny, mnz;
  double cdx, cdy, cdz;
  // per workgroup partials: semi nfc x cells, lag cells, cnt cells (zeroed before the first chunk)
  double *part_semi, *part_lag;
  unsigned long long* part_cnt;
};

// LDS of one workgroup in bytes: the float64 arrays first (histogram sums, edges, 6 coordinate tiles, 2 x FCHUNK value tiles), the 32-bit
// counts behind them
__host__ __device__ constexpr size_t vario3_lds_doubles(bool map, int cells, int copies, int nfc) {
  return (size_t)copies * cells * (nfc + (map ? 0 : 1)) + (map ? 0 : MAXLAGS + 1) + 6 * TILE + 2 * FCHUNK * TILE;
}
__host__ __device__ constexpr size_t vario3_lds_bytes(bool map, int cells, int copies, int nfc) {
  return vario3_lds_doubles(map, cells, copies, nfc) * sizeof(double) + (size_t)copies * cells * sizeof(unsigned);
}

// tile t of the upper triangle, rows first: row ti holds the tiles (ti, ti) .. (ti, nt - 1)
__device__ inline void tile3_of(long t, long nt, long& ti, long& tj) {
  const double b = 2.0 * (double)nt + 1.0;
  long r = (long)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  r = r < 0 ? 0 : (r > nt - 1 ? nt - 1 : r);
  while (r > 0 && r * nt - r * (r - 1) / 2 > t) --r;
  while (r + 1 < nt && (r + 1) * nt - (r + 1) * r / 2 <= t) ++r;
  ti = r;
  tj = r + (t - (r * nt - r * (r - 1) / 2));
}

template <bool MAP>
__device__ __forceinline__ void vario3_body(const Vario3Args& a) {
#pragma clang fp contract(off)
  extern __shared__ double smem3[];
  const int tid = threadIdx.x, cells = a.cells, copies = a.copies, nfc = a.nfc;
  const int hist = copies * cells;
  double* semi = smem3;                                  // [copy][field][cell]
  double* lag = semi + (size_t)hist * nfc;               // [copy][cell] (directions only)
  double* se = lag + (MAP ? 0 : hist);                   // edges (directions only)
  double* xi = se + (MAP ? 0 : MAXLAGS + 1);
  double *yi = xi + TILE, *zi = yi + TILE, *xj = zi + TILE, *yj = xj + TILE, *zj = yj + TILE;
  double* vi = zj + TILE;                                // [field][row station]
  double* vj = vi + FCHUNK * TILE;
  unsigned* cnt = reinterpret_cast<unsigned*>(vj + FCHUNK * TILE);  // [copy][cell]

  for (int k = tid; k < hist * nfc; k += THREADS) semi[k] = 0.0;
  for (int k = tid; k < hist; k += THREADS) {
    if (!MAP) lag[k] = 0.0;
    cnt[k] = 0u;
  }
  if (!MAP)
    for (int k = tid; k <= a.nlags; k += THREADS) se[k] = a.edges[k];

  const int c = tid & (TILE - 1), w = tid >> 6;
  const int cp = w & (copies - 1);
  double* my_semi = semi + (size_t)cp * nfc * cells;
  double* my_lag = lag + (size_t)cp * cells;
  unsigned* my_cnt = cnt + (size_t)cp * cells;
  const bool first = a.first != 0;
  const int W = 2 * a.mnx + 1, H = 2 * a.mny + 1, ncell = W * H * (2 * a.mnz + 1);
  long since = 0;

  for (long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    long ti, tj;
    tile3_of(t, a.nt, ti, tj);
    const long i0 = ti * TILE, j0 = tj * TILE;
    __syncthreads();  // the previous tile has been read (and, before the first tile, the histogram is zero)
    if (first && ++since > FLUSH_TILES) {  // uniform over the workgroup: the 32-bit counts move to the 64-bit partials
      for (int k = tid; k < cells; k += THREADS) {
        unsigned long long s = 0;
        for (int q = 0; q < copies; ++q) {
          s += cnt[q * cells + k];
          cnt[q * cells + k] = 0u;
        }
        a.part_cnt[(size_t)blockIdx.x * cells + k] += s;
      }
      since = 1;
      __syncthreads();
    }
    if (tid < TILE) {
      const long i = i0 + tid;
      xi[tid] = i < a.n ? a.x[i] : 0.0;
      yi[tid] = i < a.n ? a.y[i] : 0.0;
      zi[tid] = i < a.n ? a.z[i] : 0.0;
    } else if (tid < 2 * TILE) {
      const long j = j0 + (tid - TILE);
      xj[tid - TILE] = j < a.n ? a.x[j] : 0.0;
      yj[tid - TILE] = j < a.n ? a.y[j] : 0.0;
      zj[tid - TILE] = j < a.n ? a.z[j] : 0.0;
    }
    for (int k = tid; k < nfc * TILE; k += THREADS) {
      const int f = k >> 6, s = k & (TILE - 1);
      vi[k] = i0 + s < a.n ? a.v[(size_t)f * a.n + i0 + s] : 0.0;
      vj[k] = j0 + s < a.n ? a.v[(size_t)f * a.n + j0 + s] : 0.0;
    }
    __syncthreads();
    const long j = j0 + c;
    if (j >= a.n) continue;
    const double pxj = xj[c], pyj = yj[c], pzj = zj[c];
    double vc[FCHUNK];
#pragma unroll
    for (int f = 0; f < FCHUNK; ++f) vc[f] = f < nfc ? vj[f * TILE + c] : 0.0;
    for (int r = w; r < TILE; r += THREADS / TILE) {
      const long i = i0 + r;
      if (i >= j) break;  // (i < j < n; rows ascend)
      const double dx = pxj - xi[r], dy = pyj - yi[r], dz = pzj - zi[r];
      double g[FCHUNK];
#pragma unroll
      for (int f = 0; f < FCHUNK; ++f) {
        const double dv = vi[f * TILE + r] - vc[f];
        g[f] = 0.5 * (dv * dv);
      }
      if (MAP) {
        const double qx = floor(dx / a.cdx + 0.5), qy = floor(dy / a.cdy + 0.5), qz = floor(dz / a.cdz + 0.5);
        if (!(fabs(qx) <= (double)a.mnx) || !(fabs(qy) <= (double)a.mny) || !(fabs(qz) <= (double)a.mnz)) continue;
        int cell = ((a.mnz + (int)qz) * H + (a.mny + (int)qy)) * W + (a.mnx + (int)qx);
        if (cell > ncell / 2) cell = ncell - 1 - cell;  // the mirror cell of -h: one half of the map is kept
        if (first) atomicAdd(&my_cnt[cell], 1u);
#pragma unroll
        for (int f = 0; f < FCHUNK; ++f)
          if (f < nfc) atomicAdd(&my_semi[f * cells + cell], g[f]);
      } else {
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        if (!(d >= se[0]) || !(d < se[a.nlags])) continue;
        int lo = 0, hi = a.nlags;  // se[lo] <= d < se[hi]
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (d >= se[mid]) lo = mid;
          else hi = mid;
        }
        for (int q = 0; q < a.na; ++q) {
          if (!a.all || a.band) {
            const double ux = a.ux[q], uy = a.uy[q], uz = a.uz[q];
            const double cx = dy * uz - dz * uy, cy = dz * ux - dx * uz, cz = dx * uy - dy * ux;
            const double across2 = cx * cx + cy * cy + cz * cz;
            if (!a.all) {
              const double along = dx * ux + dy * uy + dz * uz;
              if (!(across2 <= (along * along) * a.tan2)) continue;
            }
            if (a.band && !(across2 <= a.bw2)) continue;
          }
          const int cell = q * a.nlags + lo;
          if (first) {
            atomicAdd(&my_cnt[cell], 1u);
            atomicAdd(&my_lag[cell], d);
          }
#pragma unroll
          for (int f = 0; f < FCHUNK; ++f)
            if (f < nfc) atomicAdd(&my_semi[f * cells + cell], g[f]);
        }
      }
    }
  }
  __syncthreads();
  for (int k = tid; k < cells; k += THREADS) {
    for (int f = 0; f < nfc; ++f) {
      double s = 0.0;
      for (int q = 0; q < copies; ++q) s += semi[((size_t)q * nfc + f) * cells + k];
      a.part_semi[((size_t)blockIdx.x * nfc + f) * cells + k] = s;
    }
    if (first) {
      unsigned long long n = 0;
      double s = 0.0;
      for (int q = 0; q < copies; ++q) {
        n += cnt[q * cells + k];
        if (!MAP) s += lag[q * cells + k];
      }
      a.part_cnt[(size_t)blockIdx.x * cells + k] += n;
      if (!MAP) a.part_lag[(size_t)blockIdx.x * cells + k] = s;
    }
  }
}

__global__ void __launch_bounds__(THREADS) k_vario3_dir(const Vario3Args a) { vario3_body<false>(a); }
__global__ void __launch_bounds__(THREADS) k_vario3_map(const Vario3Args a) { vario3_body<true>(a); }

// out[k] = part[0][k] + part[1][k] + ... in workgroup order, k < m
__global__ void __launch_bounds__(THREADS) k_vario3_sum(const double* __restrict__ part, int nwg, long m, double* __restrict__ out) {
  const long k = (long)blockIdx.x * THREADS + threadIdx.x;
  if (k >= m) return;
  double s = 0.0;
  for (int g = 0; g < nwg; ++g) s += part[(size_t)g * m + k];
  out[k] = s;
}

__global__ void __launch_bounds__(THREADS) k_vario3_sum_cnt(const unsigned long long* __restrict__ part, int nwg, long m,
                                                            long long* __restrict__ out) {
  const long k = (long)blockIdx.x * THREADS + threadIdx.x;
  if (k >= m) return;
  unsigned long long s = 0;
  for (int g = 0; g < nwg; ++g) s += part[(size_t)g * m + k];
  out[k] = (long long)s;
}

}  // namespace mkv3
