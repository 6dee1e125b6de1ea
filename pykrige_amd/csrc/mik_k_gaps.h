// mik_k_gaps.h -- value fields with missing stations (mik_set_field_gaps) kriged from the one resident inverse.  Included by
// mik_k_predict.h after mik_k_cvfolds.h.  Kernels: k_gap_factor, k_gap_w, k_gap_g, k_gap_coef (set-up); k_gap_contract, k_gap_ss (per launch).
//
// A field whose stations S (m of them) are missing, R everything else (border and drift rows included), B = A^-1, b(p) the right-hand
// side of point p as k_rhs writes it, v0 the field with zeros at S and c0 = B[:, :N] v0 (k_cvec_fields<MIK_FB>).  The block inverse gives
//     L L^T = B_SS,   W = L^-1 B[S, :]  (m x M),   g = L^-1 c0_S,   c~ = c0 - W^T g  with  c~_S := 0 (exact zeros),
//     z_R(p) = c~ . b(p),        sigma^2_R(p) = sigma^2(p) + |W b(p)|^2
// -- what an object built from the stations of R alone returns -- for ANY value of b_S, so the exact_values zeroing at a missing
// station needs no special case.  Fields with the same S form one PATTERN and share L, W and the sigma^2 plane.
//
//   set-up, once per predict      k_gap_factor<BIG>    one workgroup per pattern: gather B[S, S], Cholesky, L^-1 (mik_k_cvfolds.h's device
//                                                      functions; false: m <= MIK_CVF_LDS in LDS, true: any m in 64-column panels), L^-1 to a.linv
//                                 k_gap_w              W = L^-1 B[S, :]: one workgroup per 16-row group x 256 columns, k ascending
//                                 k_gap_g              g = L^-1 c0_S: one workgroup per gappy field, a wave per row (k_cvec's order)
//                                 k_gap_coef           c~ into the field's column of fc: one thread per row of c, i ascending
//   per launch                    k_gap_contract<NAI>  Q = W_all Bt^T on the matrix cores (gemm_core, k_contract<false, 2>'s persistent queue),
//                                                      epilogue part[16-row group][t] = sum over the group's rows of Q^2
//                                 k_gap_ss             plane of pattern p = sigma^2 + its groups' partial sums in ascending order
// The rows of a pattern in W_all are padded with zero rows to a multiple of 16 (a 16-row MFMA group belongs to one pattern), all rows
// to a multiple of 128 (the block tile).  Every sum has one fixed order that depends on the pattern's station list alone: plane f of F
// fields is bit for bit the one-field result.  A pattern whose B_SS is not numerically positive definite gets NaN in L^-1, hence in W, c~,
// z and sigma^2 of its fields only (the fold kernels' rule).
#pragma once
#include "mik_k_cvfolds.h"

namespace mik {

#define MIK_GAP_DESC 4  // longs per pattern in GapArgs::desc

struct GapArgs {
  const double* B;  // the inverse, row stride ldb
  long ldb;
  int Mp;
  const int* idx;            // missing-station positions (factor order), pattern after pattern, ascending inside a pattern
  const long* desc;          // per pattern: first entry of idx, m, first double of its L^-1 block in linv (row stride m), first row in W
  const int* grp;            // per 16-row group of W: its pattern
  double* linv;
  double* W;                 // row stride Mp
  const unsigned char* inS;  // per pattern Mp bytes: 1 at the rows of S
  const int* fpat;           // per gappy field: its pattern
  const int* fcol;           //   ... its column of fc
  double* fc;                // the coefficient block (column stride ldc): c0 in, c~ out
  long ldc;
  double* g;  // per gappy field: gld doubles
  long gld;
  int ldw;  // k_gap_factor<false>: row stride of the LDS block (odd, >= the launch's largest m)
};

// One workgroup per pattern of the launch's part of desc (blockIdx.x): gather B[S, S], Cholesky, L^-1 to a.linv (NaN at a bad pivot).
// BIG = false: m <= MIK_CVF_LDS, the block in dynamic LDS (m rows of a.ldw); BIG = true: any m, in place in a.linv, two 64 x 65 tiles of LDS.
template <bool BIG>
__global__ void __launch_bounds__(256) k_gap_factor(const GapArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  extern __shared__ double cvf_lds[];
  const long* d = a.desc + MIK_GAP_DESC * (long)blockIdx.x;
  const int m = (int)d[1];
  const int* idx = a.idx + d[0];
  double* G = a.linv + d[2];
  bool ok;
  if (BIG) {
    for (int i = wave; i < m; i += 4) {
      const double* brow = a.B + (long)idx[i] * a.ldb;
      for (int j = lane; j <= i; j += 64) G[(long)i * m + j] = brow[idx[j]];
    }
    __syncthreads();
    ok = cvf_factor_blocked(G, m, cvf_lds, cvf_lds + MIK_CVF_NB * MIK_CVF_TLD);
    __syncthreads();
  } else {
    const int ldw = a.ldw;
    for (int i = wave; i < m; i += 4) {
      const double* brow = a.B + (long)idx[i] * a.ldb;
      for (int j = lane; j <= i; j += 64) cvf_lds[i * ldw + j] = brow[idx[j]];
    }
    __syncthreads();
    ok = cvf_chol_lds(cvf_lds, ldw, m);
    if (ok) cvf_trinv_lds(cvf_lds, ldw, m);
    __syncthreads();
    if (ok)
      for (int i = wave; i < m; i += 4)
        for (int j = lane; j <= i; j += 64) G[(long)i * m + j] = cvf_lds[i * ldw + j];
  }
  if (!ok) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = wave; i < m; i += 4)
      for (int j = lane; j <= i; j += 64) G[(long)i * m + j] = nan;
  }
}

// W = L^-1 B[S, :]: blockIdx.y = 16-row group, blockIdx.x = 256 columns, k ascending
__global__ void __launch_bounds__(256) k_gap_w(const GapArgs a) {
  const long* d = a.desc + MIK_GAP_DESC * (long)a.grp[blockIdx.y];
  const int m = (int)d[1];
  const int* idx = a.idx + d[0];
  const double* L = a.linv + d[2];
  const long row0 = 16L * blockIdx.y;
  const int r0 = (int)(row0 - d[3]);  // first row of the group inside its pattern
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.Mp) return;
  double acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0;
  const int kend = r0 + 16 < m ? r0 + 16 : m;
  for (int k = 0; k < kend; ++k) {
    const double b = a.B[(long)idx[k] * a.ldb + j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = r0 + r;
      if (i < m && k <= i) acc[r] += L[(long)i * m + k] * b;
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) a.W[(row0 + r) * a.Mp + j] = acc[r];  // (rows m .. of the pattern: zeros)
}

// g = L^-1 c0_S: blockIdx.x = gappy field, a wave per row (k_cvec's order)
__global__ void __launch_bounds__(256) k_gap_g(const GapArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long* d = a.desc + MIK_GAP_DESC * (long)a.fpat[blockIdx.x];
  const int m = (int)d[1];
  const int* idx = a.idx + d[0];
  const double* L = a.linv + d[2];
  const double* c0 = a.fc + (long)a.fcol[blockIdx.x] * a.ldc;
  for (int i = wave; i < m; i += 4) {
    double s = 0.0;
    for (int k = lane; k <= i; k += 64) s += L[(long)i * m + k] * c0[idx[k]];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) a.g[(long)blockIdx.x * a.gld + i] = s;
  }
}

// c~ into the field's column of fc: blockIdx.y = gappy field, blockIdx.x = 256 rows of c, i ascending
__global__ void __launch_bounds__(256) k_gap_coef(const GapArgs a) {
  const int pat = a.fpat[blockIdx.y];
  const long* d = a.desc + MIK_GAP_DESC * (long)pat;
  const int m = (int)d[1];
  const double* w = a.W + d[3] * a.Mp;
  const double* g = a.g + (long)blockIdx.y * a.gld;
  double* c = a.fc + (long)a.fcol[blockIdx.y] * a.ldc;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.Mp) return;
  double s = 0.0;
  for (int i = 0; i < m; ++i) s += w[(long)i * a.Mp + j] * g[i];
  c[j] = a.inS[(long)pat * a.Mp + j] ? 0.0 : c[j] - s;
}

struct GapGemmArgs {
  const double* W;  // rows (a multiple of 128) x ldw
  long ldw;
  const double* Bt;  // the launch's point-major panel
  long ldb;
  double* part;  // [16-row group][palloc]
  int palloc, nRblk, kend;
  unsigned long long* queue;
};

// The XCD this workgroup runs on, and one pop from queue xq of k_contract's persistent per-XCD tile queues: thread 0 takes the next
// position, everyone decodes it (super_tile_at: 0 = tile (ablk, bblk), 1 = padding slot, 2 = the queue is exhausted).  Two barriers.
__device__ __forceinline__ int xcd_id() {
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  return (int)(xcc & 7);
}
__device__ __forceinline__ int pop_super_tile(unsigned long long* queue, int xq, GemmSmem& sm, int nAblk, int nBblk, int& ablk, int& bblk) {
  if (threadIdx.x == 0) sm.next = (long)__hip_atomic_fetch_add(&queue[xq], 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const long seq = sm.next;
  const int kind = super_tile_at(nAblk, nBblk, xq, seq, ablk, bblk);
  __syncthreads();  // everyone has read sm.next before it is written again
  return kind;
}

// part[group][t] = sum over the 16 rows i of the group of (sum_k W[i][k] Bt[t][k])^2.  Tile 128 rows x 128 points on gemm_core, the K loop
// over [0, kend); persistent over k_contract's per-XCD tile queues (super_tile_at).  Accumulator acc[ai][bi][r] is row 16 ai + 4 r +
// (lane >> 4), column 16 bi + (lane & 15) of the wave tile: a group's sum is the lane's four squares in r order, then the two xor steps
// over lane >> 4 -- registers only, nothing of another group or pattern enters.
template <int NAI>
__global__ void __launch_bounds__(64 * 2 * (8 / NAI), 2 * (4 / NAI)) k_gap_contract(const GapGemmArgs a) {
  __shared__ GemmSmem sm;
  const int xcd = xcd_id();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, lq = lane >> 4, lc = lane & 15;
  const int nTblk = a.palloc / MIK_BN;
  int steal = 0;
  for (;;) {
    int iblk = 0, tblk = 0;
    const int kind = pop_super_tile(a.queue, (xcd + steal) & 7, sm, a.nRblk, nTblk, iblk, tblk);
    if (kind == 2) {
      if (++steal == 8) return;
      continue;
    }
    if (kind == 1) continue;
    d4 acc[NAI][4];
#pragma unroll
    for (int x = 0; x < NAI; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) acc[x][y] = (d4){0.0, 0.0, 0.0, 0.0};
    gemm_core<NAI>(a.W + (long)iblk * MIK_BM * a.ldw, a.ldw, a.Bt + (long)tblk * MIK_BN * a.ldb, a.ldb, 0, a.kend, acc, sm);
#pragma unroll
    for (int ai = 0; ai < NAI; ++ai)
#pragma unroll
      for (int bi = 0; bi < 4; ++bi) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) s += acc[ai][bi][r] * acc[ai][bi][r];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (lq == 0) a.part[(long)(iblk * (MIK_BM / 16) + wm * NAI + ai) * a.palloc + tblk * MIK_BN + wn * 64 + bi * 16 + lc] = s;
      }
  }
}

struct GapRedArgs {
  const double* part;  // [16-row group][palloc]
  int palloc, nvalid;
  const double* ss;    // the launch's all-stations sigma^2
  const long* desc;    // per pattern (GapArgs::desc): [1] = m, [3] = first row in W
  double* out;         // plane of pattern p at out + p * ldo, this launch's points from 0
  long ldo;
};

// blockIdx.y = pattern: its plane = sigma^2 + the partial sums of its 16-row groups, ascending
__global__ void __launch_bounds__(256) k_gap_ss(const GapRedArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.nvalid) return;
  const long* d = a.desc + MIK_GAP_DESC * (long)blockIdx.y;
  const long g0 = d[3] / 16, ng = (d[1] + 15) / 16;
  double s = a.ss[t];
  for (long g = 0; g < ng; ++g) s += a.part[(g0 + g) * a.palloc + t];
  a.out[(long)blockIdx.y * a.ldo + t] = s;
}

}  // namespace mik
