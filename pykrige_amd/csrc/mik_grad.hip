// mik_grad.hip -- host side + C ABI (include/mikgrad.h) of libmikgrad.so: log det C, W^T C^-1 W and the analytic gradient of the ML / REML
// objective of a station set under a variogram model.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -Iinclude pykrige_amd/csrc/mik_grad.hip
// Links nothing of the other libraries and keeps no state: the call selects its device, uploads, runs, copies back and frees.  The
// elimination kernels are those of mik_k_lik.h, compiled into this library and run on the larger square of mik_k_grad.h.
#include "mik_k_grad.h"
#include "../../include/mikgrad.h"

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using namespace mlk;
using namespace mlg;

static_assert(MLG_GAUSSIAN == GAUSSIAN && MLG_EXPONENTIAL == EXPONENTIAL && MLG_SPHERICAL == SPHERICAL && MLG_HOLE_EFFECT == HOLE_EFFECT,
              "mikgrad.h and mik_k_lik.h disagree");
static_assert((MLG_MAXFIELDS + MLG_MAXTREND + 15) / 16 * 16 == 48, "the memory bound of mikgrad.h is written for at most 48 padded rows");
static_assert(MLG_MAXGEOM == MAXG && MLG_MAXTREND == MAXP && MLG_MAXFIELDS % FC == 0, "mikgrad.h and mik_k_grad.h disagree");
static_assert(pairs_lds_bytes() == 2304 && pairs_lds_bytes() <= 163840, "k_grad_pairs: the LDS budget is not the documented one");
static_assert(syrk_lds_bytes() <= 163840 && trsm_lds_bytes() <= 163840 && potrf_lds_bytes() <= 163840, "a kernel does not fit the LDS of a CU");

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPC(x)                                                                                              \
  do {                                                                                                       \
    hipError_t e_ = (x);                                                                                     \
    if (e_ != hipSuccess) {                                                                                  \
      char b_[512];                                                                                          \
      snprintf(b_, sizeof b_, "HIP error '%s' at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #x); \
      return fail(MLG_EHIP, b_);                                                                             \
    }                                                                                                        \
  } while (0)

struct Dev {  // device memory of one call
  void* p = nullptr;
  Dev() = default;
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() {
    if (p) (void)hipFree(p);
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

bool all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace

extern "C" {

int mlg_abi_version(void) { return MLG_ABI_VERSION; }
const char* mlg_last_error(void) { return g_err.c_str(); }

int mlg_grad(int device, int64_t n, int32_t ndim, const double* coords, int32_t ng, const double* dcoords, int32_t model, double psill,
             double range, double nugget, const double* V, int32_t F, const double* X, int32_t p, int32_t reml, double* logdet, double* G,
             double* grad, int32_t* info) {
  if (!coords || !V || !X || !logdet || !G || !grad || !info) return fail(MLG_EINVAL, "mlg_grad: NULL argument");
  *info = 0;
  if (n < 2) return fail(MLG_EINVAL, "mlg_grad: need at least two stations");
  if (ndim != 2 && ndim != 3) return fail(MLG_EINVAL, "mlg_grad: ndim must be 2 or 3");
  if (ng < 0 || ng > MLG_MAXGEOM) return fail(MLG_EINVAL, "mlg_grad: ng must be in 0..5 (MLG_MAXGEOM)");
  if (ng > 0 && !dcoords) return fail(MLG_EINVAL, "mlg_grad: NULL dcoords with ng > 0");
  if (F < 1 || F > MLG_MAXFIELDS) return fail(MLG_EINVAL, "mlg_grad: F must be in 1..32 (MLG_MAXFIELDS)");
  if (p < 1 || p > MLG_MAXTREND) return fail(MLG_EINVAL, "mlg_grad: p must be in 1..8 (MLG_MAXTREND)");
  if (reml != 0 && reml != 1) return fail(MLG_EINVAL, "mlg_grad: reml must be 0 or 1");
  if (model < MLG_GAUSSIAN || model > MLG_HOLE_EFFECT)
    return fail(MLG_EINVAL, "mlg_grad: model must be one of MLG_GAUSSIAN, MLG_EXPONENTIAL, MLG_SPHERICAL, MLG_HOLE_EFFECT");
  if (!(psill > 0.0 && range > 0.0 && nugget >= 0.0) || !std::isfinite(psill) || !std::isfinite(range) || !std::isfinite(nugget))
    return fail(MLG_EINVAL, "mlg_grad: need finite psill > 0, range > 0 and nugget >= 0");
  if (n > ((int64_t)1 << 30) - 64 - TS) return fail(MLG_EINVAL, "mlg_grad: the matrix of this many stations fits no device");
  if (!all_finite(coords, (size_t)n * ndim)) return fail(MLG_EINVAL, "mlg_grad: station coordinates must be finite");
  if (ng > 0 && !all_finite(dcoords, (size_t)n * ndim * ng)) return fail(MLG_EINVAL, "mlg_grad: dcoords must be finite");
  if (!all_finite(V, (size_t)n * F)) return fail(MLG_EINVAL, "mlg_grad: V must be finite");
  if (!all_finite(X, (size_t)n * p)) return fail(MLG_EINVAL, "mlg_grad: X must be finite");
  HIPC(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, device));
  if ((double)(2 * n + 48) * (double)(2 * n + 48) * 8.0 > (double)prop.totalGlobalMem / 4.0)
    return fail(MLG_EINVAL, "mlg_grad: (2n + 48)^2 * 8 bytes pass a quarter of this device's memory");
  const int m = F + p, mpad = (m + 15) / 16 * 16;
  const int N = (int)n, NW = N + mpad, NQ = NW + N;
  const int64_t ld = NQ;
  const int nk = 3 + ng;

  Dev dA, dc, de, dw, ddiag, dinfo;
  HIPC(hipMalloc(&dA.p, sizeof(double) * (size_t)NQ * (size_t)ld));
  HIPC(hipMalloc(&dc.p, sizeof(double) * (size_t)N * ndim));
  HIPC(hipMalloc(&de.p, sizeof(double) * (size_t)N * ndim * (ng > 0 ? ng : 1)));
  HIPC(hipMalloc(&dw.p, sizeof(double) * (size_t)N * m));
  HIPC(hipMalloc(&ddiag.p, sizeof(double) * (size_t)N));
  HIPC(hipMalloc(&dinfo.p, sizeof(int)));
  HIPC(hipMemcpy(dc.p, coords, sizeof(double) * (size_t)N * ndim, hipMemcpyHostToDevice));
  if (ng > 0) HIPC(hipMemcpy(de.p, dcoords, sizeof(double) * (size_t)N * ndim * ng, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dw.p, V, sizeof(double) * (size_t)N * F, hipMemcpyHostToDevice));  // W = [V | X], one column per row
  HIPC(hipMemcpy(dw.as<double>() + (size_t)N * F, X, sizeof(double) * (size_t)N * p, hipMemcpyHostToDevice));
  HIPC(hipMemset(dinfo.p, 0, sizeof(int)));

  const Model mo{model, psill, range, nugget};
  const unsigned at = (unsigned)((NW + AT - 1) / AT);
  hipLaunchKernelGGL(k_lik_assemble, dim3(at, at), dim3(256), 0, 0, dA.as<double>(), ld, N, NW, (int)ndim, dc.as<double>(), mo,
                     dw.as<double>(), m);
  HIPC(hipGetLastError());
  hipLaunchKernelGGL(k_grad_seed, dim3((unsigned)((NQ + 255) / 256), (unsigned)(N < 32768 ? N : 32768)), dim3(256), 0, 0, dA.as<double>(), ld, N,
                     NW);
  HIPC(hipGetLastError());
  for (int k0 = 0; k0 < N; k0 += NB) {
    const int jb = N - k0 < NB ? N - k0 : NB;
    hipLaunchKernelGGL(k_lik_potrf, dim3(1), dim3(256), 0, 0, dA.as<double>(), ld, k0, jb, ddiag.as<double>(), dinfo.as<int>());
    HIPC(hipGetLastError());
    // the pivots of this block decide whether anything further is launched
    int bad = 0;
    HIPC(hipMemcpy(&bad, dinfo.p, sizeof(int), hipMemcpyDeviceToHost));
    if (bad) {
      *info = bad;
      char b[160];
      snprintf(b, sizeof b, "mlg_grad: the covariance matrix is not positive definite (pivot of column %d)", bad);
      return fail(MLG_ENOTPD, b);
    }
    // the active rows: identity row i is zero left of column i, so the rows from NW + r0 on have nothing in this block column
    const int r0 = k0 + jb, rows = NW, top = NW + r0;
    hipLaunchKernelGGL(k_lik_trsm, dim3((unsigned)((rows + TRSM_ROWS - 1) / TRSM_ROWS)), dim3(64), 0, 0, dA.as<double>(), ld, k0, jb, r0, top);
    const int64_t tt = (rows + TS - 1) / TS;
    hipLaunchKernelGGL(k_lik_syrk, dim3((unsigned)(tt * (tt + 1) / 2)), dim3(256), 0, 0, dA.as<double>(), ld, k0, jb, r0, top);
    HIPC(hipGetLastError());
  }
  std::vector<double> diag((size_t)N), blk((size_t)mpad * mpad), qw((size_t)N * mpad);
  HIPC(hipMemcpy(diag.data(), ddiag.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy2D(blk.data(), sizeof(double) * mpad, dA.as<double>() + (size_t)N * ld + N, sizeof(double) * (size_t)ld, sizeof(double) * mpad,
                   (size_t)mpad, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy2D(qw.data(), sizeof(double) * mpad, dA.as<double>() + (size_t)NW * ld + N, sizeof(double) * (size_t)ld, sizeof(double) * mpad,
                   (size_t)N, hipMemcpyDeviceToHost));
  double s = 0.0;  // in station order: the same bits every run
  for (int i = 0; i < N; ++i) s += std::log(diag[i]);
  // the (W, W) block holds -G in its lower triangle, the (I, W) block -Q W
  std::vector<double> Gm((size_t)m * m);
  for (int a = 0; a < m; ++a)
    for (int b = 0; b <= a; ++b) Gm[(size_t)a * m + b] = Gm[(size_t)b * m + a] = 0.0 - blk[(size_t)a * mpad + b];

  // the small algebra, field by field in a fixed order: L L^T = G_xx, U = Q X L^-T (n x p, kept as p x n) and a_f = Q v_f - Q X beta_f
  double L[MAXP][MAXP] = {};
  for (int c = 0; c < p; ++c) {
    double d = Gm[(size_t)(F + c) * m + F + c];
    for (int k = 0; k < c; ++k) d -= L[c][k] * L[c][k];
    if (!(d > 0.0) || !std::isfinite(d)) {
      *info = N + c + 1;
      char b[160];
      snprintf(b, sizeof b, "mlg_grad: X^T C^-1 X is not positive definite (pivot of its column %d)", c + 1);
      return fail(MLG_ENOTPD, b);
    }
    L[c][c] = std::sqrt(d);
    for (int r = c + 1; r < p; ++r) {
      double v = Gm[(size_t)(F + r) * m + F + c];
      for (int k = 0; k < c; ++k) v -= L[r][k] * L[c][k];
      L[r][c] = v / L[c][c];
    }
  }
  std::vector<double> U((size_t)p * N), av((size_t)F * N);
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < p; ++c) {
      double v = 0.0 - qw[(size_t)i * mpad + F + c];
      for (int k = 0; k < c; ++k) v -= L[c][k] * U[(size_t)k * N + i];
      U[(size_t)c * N + i] = v / L[c][c];
    }
  for (int f = 0; f < F; ++f) {
    double y[MAXP], beta[MAXP];
    for (int c = 0; c < p; ++c) {
      double v = Gm[(size_t)(F + c) * m + f];
      for (int k = 0; k < c; ++k) v -= L[c][k] * y[k];
      y[c] = v / L[c][c];
    }
    for (int c = p - 1; c >= 0; --c) {
      double v = y[c];
      for (int k = c + 1; k < p; ++k) v -= L[k][c] * beta[k];
      beta[c] = v / L[c][c];
    }
    for (int i = 0; i < N; ++i) {
      double v = 0.0 - qw[(size_t)i * mpad + f];
      for (int c = 0; c < p; ++c) v -= (0.0 - qw[(size_t)i * mpad + F + c]) * beta[c];
      av[(size_t)f * N + i] = v;
    }
  }

  const int64_t tiles1 = (N + GT - 1) / GT, tiles = tiles1 * (tiles1 + 1) / 2;
  const int chunks = (F + FC - 1) / FC;
  Dev du, da, dpart;
  HIPC(hipMalloc(&du.p, sizeof(double) * (size_t)p * N));
  HIPC(hipMalloc(&da.p, sizeof(double) * (size_t)F * N));
  HIPC(hipMalloc(&dpart.p, sizeof(double) * (size_t)chunks * (size_t)tiles * NV));
  HIPC(hipMemcpy(du.p, U.data(), sizeof(double) * (size_t)p * N, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(da.p, av.data(), sizeof(double) * (size_t)F * N, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_grad_pairs, dim3((unsigned)tiles, (unsigned)chunks), dim3(256), 0, 0, dA.as<double>() + (size_t)NW * ld + NW, ld, N,
                     (int)ndim, dc.as<double>(), (int)ng, de.as<double>(), mo, (int)reml, (int)p, du.as<double>(), (int)F, da.as<double>(),
                     dpart.as<double>());
  HIPC(hipGetLastError());
  std::vector<double> part((size_t)chunks * (size_t)tiles * NV);
  HIPC(hipMemcpy(part.data(), dpart.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost));

  // the tiles in order; a pair i > j stands for (i, j) and (j, i)
  for (int ch = 0; ch < chunks; ++ch) {
    double sum[NV];
    for (int v = 0; v < NV; ++v) sum[v] = 0.0;
    for (int64_t b = 0; b < tiles; ++b) {
      const double* pt = part.data() + ((size_t)ch * (size_t)tiles + (size_t)b) * NV;
      for (int v = 0; v < NV; ++v) sum[v] += pt[v];
    }
    for (int fc = 0; fc < FC && ch * FC + fc < F; ++fc) {
      double* g = grad + (size_t)(ch * FC + fc) * nk;
      const double* dg = sum + (ROWS - 1) * COLS;  // the diagonal
      for (int k = 0; k < nk; ++k) {
        double S, T;
        if (k == 2) {  // the nugget: the diagonal only
          S = dg[0];
          T = dg[1 + fc];
        } else {
          const double* row = sum + (k < 2 ? k : k - 1) * COLS;
          S = 2.0 * row[0];
          T = 2.0 * row[1 + fc];
          if (k == 0) {  // the partial sill: 1 on the diagonal
            S += dg[0];
            T += dg[1 + fc];
          }
        }
        g[k] = 0.5 * S - 0.5 * T;
      }
    }
  }
  *logdet = 2.0 * s;
  for (size_t e = 0; e < (size_t)m * m; ++e) G[e] = Gm[e];
  return MLG_OK;
}

}  // extern "C"
