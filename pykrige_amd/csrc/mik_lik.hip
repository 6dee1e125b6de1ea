// mik_lik.hip -- host side + C ABI (include/miklik.h) of libmiklik.so: log det C and W^T C^-1 W of a station set under a variogram model.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -Iinclude pykrige_amd/csrc/mik_lik.hip
// Links nothing of the other three libraries and keeps no state: the call selects its device, uploads, runs, copies back and frees.
#include "mik_k_lik.h"
#include "../../include/miklik.h"

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using namespace mlk;

static_assert(MLK_GAUSSIAN == GAUSSIAN && MLK_EXPONENTIAL == EXPONENTIAL && MLK_SPHERICAL == SPHERICAL && MLK_HOLE_EFFECT == HOLE_EFFECT,
              "miklik.h and mik_k_lik.h disagree");
static_assert((MLK_MAXCOLS + 15) / 16 * 16 == 48, "the memory bound of miklik.h is written for at most 48 padded rows");
// the LDS of the three elimination kernels: 33 280, 66 048 and 73 728 bytes -- two workgroups of each on a CU of 163 840
static_assert(potrf_lds_bytes() == 33280 && trsm_lds_bytes() == 66048 && syrk_lds_bytes() == 73728, "the LDS budgets are not the documented ones");
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
      return fail(MLK_EHIP, b_);                                                                             \
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

int mlk_abi_version(void) { return MLK_ABI_VERSION; }
const char* mlk_last_error(void) { return g_err.c_str(); }

int mlk_gram(int device, int64_t n, int32_t ndim, const double* coords, int32_t model, double psill, double range, double nugget,
             const double* W, int32_t m, double* logdet, double* G, int32_t* info) {
  if (!coords || !W || !logdet || !G || !info) return fail(MLK_EINVAL, "mlk_gram: NULL argument");
  *info = 0;
  if (n < 2) return fail(MLK_EINVAL, "mlk_gram: need at least two stations");
  if (ndim != 2 && ndim != 3) return fail(MLK_EINVAL, "mlk_gram: ndim must be 2 or 3");
  if (m < 1 || m > MLK_MAXCOLS) return fail(MLK_EINVAL, "mlk_gram: m must be in 1..40 (MLK_MAXCOLS)");
  if (model < MLK_GAUSSIAN || model > MLK_HOLE_EFFECT)
    return fail(MLK_EINVAL, "mlk_gram: model must be one of MLK_GAUSSIAN, MLK_EXPONENTIAL, MLK_SPHERICAL, MLK_HOLE_EFFECT");
  if (!(psill > 0.0 && range > 0.0 && nugget >= 0.0) || !std::isfinite(psill) || !std::isfinite(range) || !std::isfinite(nugget))
    return fail(MLK_EINVAL, "mlk_gram: need finite psill > 0, range > 0 and nugget >= 0");
  if (n > ((int64_t)1 << 31) - 1 - 64 - TS) return fail(MLK_EINVAL, "mlk_gram: the matrix of this many stations fits no device");
  if (!all_finite(coords, (size_t)n * ndim)) return fail(MLK_EINVAL, "mlk_gram: station coordinates must be finite");
  if (!all_finite(W, (size_t)n * m)) return fail(MLK_EINVAL, "mlk_gram: W must be finite");
  HIPC(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, device));
  if ((double)(n + 48) * (double)(n + 48) * 8.0 > (double)prop.totalGlobalMem / 4.0)
    return fail(MLK_EINVAL, "mlk_gram: (n + 48)^2 * 8 bytes pass a quarter of this device's memory");
  const int mpad = (m + 15) / 16 * 16;
  const int N = (int)n, NP = N + mpad;
  const int64_t ld = NP;

  Dev dA, dc, dw, ddiag, dinfo;
  HIPC(hipMalloc(&dA.p, sizeof(double) * (size_t)NP * (size_t)ld));
  HIPC(hipMalloc(&dc.p, sizeof(double) * (size_t)N * ndim));
  HIPC(hipMalloc(&dw.p, sizeof(double) * (size_t)N * m));
  HIPC(hipMalloc(&ddiag.p, sizeof(double) * (size_t)N));
  HIPC(hipMalloc(&dinfo.p, sizeof(int)));
  HIPC(hipMemcpy(dc.p, coords, sizeof(double) * (size_t)N * ndim, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dw.p, W, sizeof(double) * (size_t)N * m, hipMemcpyHostToDevice));
  HIPC(hipMemset(dinfo.p, 0, sizeof(int)));

  const Model mo{model, psill, range, nugget};
  const unsigned at = (unsigned)((NP + AT - 1) / AT);
  hipLaunchKernelGGL(k_lik_assemble, dim3(at, at), dim3(256), 0, 0, dA.as<double>(), ld, N, NP, (int)ndim, dc.as<double>(), mo,
                     dw.as<double>(), (int)m);
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
      snprintf(b, sizeof b, "mlk_gram: the covariance matrix is not positive definite (pivot of column %d)", bad);
      return fail(MLK_ENOTPD, b);
    }
    const int r0 = k0 + jb, rows = NP - r0;
    hipLaunchKernelGGL(k_lik_trsm, dim3((unsigned)((rows + TRSM_ROWS - 1) / TRSM_ROWS)), dim3(64), 0, 0, dA.as<double>(), ld, k0, jb, r0, NP);
    const int64_t tt = (rows + TS - 1) / TS;
    hipLaunchKernelGGL(k_lik_syrk, dim3((unsigned)(tt * (tt + 1) / 2)), dim3(256), 0, 0, dA.as<double>(), ld, k0, jb, r0, NP);
    HIPC(hipGetLastError());
  }
  std::vector<double> diag((size_t)N), blk((size_t)mpad * mpad);
  HIPC(hipMemcpy(diag.data(), ddiag.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy2D(blk.data(), sizeof(double) * mpad, dA.as<double>() + (size_t)N * ld + N, sizeof(double) * (size_t)ld, sizeof(double) * mpad,
                   (size_t)mpad, hipMemcpyDeviceToHost));
  double s = 0.0;  // in station order: the same bits every run
  for (int i = 0; i < N; ++i) s += std::log(diag[i]);
  *logdet = 2.0 * s;
  // the bottom-right block holds -Y Y^T in its lower triangle; both halves of G from it
  for (int a = 0; a < m; ++a)
    for (int b = 0; b <= a; ++b) G[(size_t)a * m + b] = G[(size_t)b * m + a] = 0.0 - blk[(size_t)a * mpad + b];
  return MLK_OK;
}

}  // extern "C"
