// mik_k_fields.h -- several value fields on one station set (mik_set_fields): the coefficient block C = A_inv[:, :N] V and the
// z sums of the fields after the first, read back from the right-hand-side panel k_rhs has just written.
// Included by mik_k_predict.h (after RhsArgs).  Kernels: k_cvec_fields (the coefficient block), k_cv_loo (leave-one-out); the z sums are
// instantiations of k_rhs (rhs_fields below).
#pragma once
#include "mik_dev.h"

namespace mik {

#define MIK_FB 8  // fields per block of k_cvec_fields<FB> and per read-back launch of k_rhs (FC): the columns of one block share each read of A_inv / B

// C[f][i] = sum_{j<N} Ainv[i][j] * V[f][j] for the FB fields f0 .. f0 + FB - 1 of blockIdx.y (field-major V, ldv; C column stride ldc).
// One wave per row, as k_cvec: every column is summed in k_cvec's order (lane j mod 64, then the xor butterfly), so column f is
// bit for bit k_cvec of V[f]; the row of A_inv is read once for the FB columns.  V carries zero columns up to a multiple of FB.
template <int FB>
__global__ void __launch_bounds__(256) k_cvec_fields(const double* __restrict__ Ainv, long ld, int M, int N, const double* __restrict__ V,
                                                     long ldv, double* __restrict__ C, long ldc, int Mp) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const long f0 = (long)blockIdx.y * FB;
  if (row >= Mp) return;
  double s[FB];
#pragma unroll
  for (int f = 0; f < FB; ++f) s[f] = 0.0;
  if (row < M) {
    const double* r = Ainv + (long)row * ld;
    const double* v = V + f0 * ldv;
    for (int j = lane; j < N; j += 64) {
      const double a = r[j];
#pragma unroll
      for (int f = 0; f < FB; ++f) s[f] += a * v[f * ldv + j];
    }
#pragma unroll
    for (int f = 0; f < FB; ++f)
      for (int o = 32; o > 0; o >>= 1) s[f] += __shfl_xor(s[f], o);
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < FB; ++f) C[(f0 + f) * ldc + row] = s[f];
  }
}

// Leave-one-out cross-validation from the inverse (mik_cross_validate, global form): the kriging matrix has a zero diagonal, so the block
// inverse gives station i kriged from all the others as zhat_i = v_i - c_i / B_ii with sigma^2_i = 1 / B_ii, B = A_inv and c = B[:, :N] v --
// ordinary and universal kriging alike (the drift and border rows belong to "the others").  The sums are k_cvec_fields's (same lanes,
// same butterfly), so plane f is bit for bit the one-field result; the epilogue of a station row reads B[row][row] and V[f][row] and writes
// zhat (plane stride ldz) and, from the first block of fields, 1 / B_ii.  B_ii is used as computed: zero or non-finite gives IEEE inf / nan.
template <int FB>
__global__ void __launch_bounds__(256) k_cv_loo(const double* __restrict__ Ainv, long ld, int N, const double* __restrict__ V, long ldv,
                                                double* __restrict__ zhat, long ldz, double* __restrict__ ss) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const long f0 = (long)blockIdx.y * FB;
  if (row >= N) return;
  double s[FB];
#pragma unroll
  for (int f = 0; f < FB; ++f) s[f] = 0.0;
  const double* r = Ainv + (long)row * ld;
  const double* v = V + f0 * ldv;
  for (int j = lane; j < N; j += 64) {
    const double a = r[j];
#pragma unroll
    for (int f = 0; f < FB; ++f) s[f] += a * v[f * ldv + j];
  }
#pragma unroll
  for (int f = 0; f < FB; ++f)
    for (int o = 32; o > 0; o >>= 1) s[f] += __shfl_xor(s[f], o);
  if (lane == 0) {
    const double bii = r[row];
#pragma unroll
    for (int f = 0; f < FB; ++f) zhat[(f0 + f) * ldz + row] = v[f * ldv + row] - s[f] / bii;
    if (blockIdx.y == 0) ss[row] = 1.0 / bii;
  }
}

// z of FC fields from the panel a.Bt that k_rhs wrote for this launch (the body of k_rhs<.., FC>): no variogram is evaluated again.
// a.cvec = column 0 of this chunk of fields (column stride a.cf_ld, zero rows M .. Mp - 1), a.zout = its plane 0 (plane stride a.zf_ld),
// a.nfc = fields of the chunk that exist.  The walk over j, the per-lane sums and the 4-wave reduction are k_rhs's own, so the z of a
// field is bit for bit what k_rhs gives with that field's coefficients.  SP: the block walks its point block's candidate list, exactly the
// tiles k_rhs wrote (the flags are a subset of the candidates; tiles outside the list hold an earlier launch's values and are not read).
template <bool SP, int FC>
__device__ __forceinline__ void rhs_fields(const RhsArgs& a) {
  __shared__ double red[4][FC * MIK_TP];
  __shared__ unsigned short slist[SP ? MIK_SP_MAXK16 : 16];
  __shared__ int sncand;
  const int t0 = blockIdx.x * MIK_TP;
  double zacc[FC][MIK_TP];
#pragma unroll
  for (int f = 0; f < FC; ++f)
#pragma unroll
    for (int q = 0; q < MIK_TP; ++q) zacc[f][q] = 0.0;
  if (SP) {  // k_rhs's list of the point block's candidate K tiles
    if (threadIdx.x < 64) {
      const unsigned char* crow = a.cand + (long)(t0 >> 7) * a.nK16;
      int nc = 0;
      for (int base = 0; base < a.nK16; base += 64) {
        const int k = base + (int)threadIdx.x;
        const bool on = k < a.nK16 && crow[k] != 0;
        const unsigned long long m = __ballot(on);
        if (on) slist[nc + __popcll(m & ((1ULL << threadIdx.x) - 1ULL))] = (unsigned short)k;
        nc += __popcll(m);
      }
      if (threadIdx.x == 0) sncand = nc;
    }
    __syncthreads();
  }
  const int nit = SP ? sncand : a.Mp;
  for (int it = SP ? (int)(threadIdx.x >> 4) : (int)threadIdx.x; it < nit; it += SP ? 16 : 256) {
    const int j = SP ? 16 * (int)slist[it] + (int)(threadIdx.x & 15) : it;
    double v[MIK_TP], c[FC];
#pragma unroll
    for (int q = 0; q < MIK_TP; ++q) v[q] = a.Bt[(long)(t0 + q) * a.ld + j];
#pragma unroll
    for (int f = 0; f < FC; ++f) c[f] = a.cvec[(long)f * a.cf_ld + j];
#pragma unroll
    for (int f = 0; f < FC; ++f)
#pragma unroll
      for (int q = 0; q < MIK_TP; ++q) zacc[f][q] += c[f] * v[q];
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int f = 0; f < FC; ++f)
#pragma unroll
    for (int q = 0; q < MIK_TP; ++q) {
      double s = zacc[f][q];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) red[wave][f * MIK_TP + q] = s;
    }
  __syncthreads();
  const int f = (int)threadIdx.x / MIK_TP, q = (int)threadIdx.x % MIK_TP;
  if (f < FC && f < a.nfc && (t0 + q) < a.nvalid) {
    const long o = (SP && a.perm) ? (long)a.perm[t0 + q] : (long)(t0 + q);
    a.zout[(long)f * a.zf_ld + o] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
  }
}

}  // namespace mik
