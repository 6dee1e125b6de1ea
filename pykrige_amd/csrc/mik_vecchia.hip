// mik_vecchia.hip -- host side + C ABI (include/mikvecchia.h) of libmikvecchia.so: log det C^ and W^T C^-1 W under Vecchia's approximation.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -Iinclude pykrige_amd/csrc/mik_vecchia.hip
// Links nothing of the other five libraries.  A plan owns its device memory: the order, the neighbour lists, and the buffers of a call
// (coordinates, W, residuals, partial sums), which grow with the widest W seen and are reused from call to call.
#include "mik_k_vecchia.h"
#include "../../include/mikvecchia.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using namespace mvc;

static_assert(MVC_GAUSSIAN == GAUSSIAN && MVC_EXPONENTIAL == EXPONENTIAL && MVC_SPHERICAL == SPHERICAL && MVC_HOLE_EFFECT == HOLE_EFFECT,
              "mikvecchia.h and mik_k_vecchia.h disagree");
static_assert(MVC_MAXNB == MAXNB && MVC_MAXCOLS == MAXCOLS, "mikvecchia.h and mik_k_vecchia.h disagree");
// the LDS of the kernels: k_vec_knn at most 55 296 bytes (3-D, m = 64), k_vec_reduce 10 752, k_vec_solve none -- of the 163840 of a CU
static_assert(knn_lds_bytes(3, MAXNB) == 55296 && reduce_lds_bytes() == 10752, "the LDS budgets are not the documented ones");
static_assert(knn_lds_bytes(3, MAXNB) <= 163840 && reduce_lds_bytes() <= 163840, "a kernel does not fit the LDS of a CU");

struct mvc_plan {
  int device = 0;
  int n = 0, ndim = 0, m = 0;
  std::vector<int32_t> order;
  int* d_order = nullptr;
  int* d_nbr = nullptr;
  double* d_coords = nullptr;
  int cols = 0;  // the columns d_W and d_R are sized for
  double* d_W = nullptr;
  double* d_R = nullptr;
  double* d_part = nullptr;
  int* d_partbad = nullptr;
  double* d_out = nullptr;
  int* d_bad = nullptr;
};

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
      return fail(MVC_EHIP, b_);                                                                             \
    }                                                                                                        \
  } while (0)

bool all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

void release(mvc_plan* p) {
  if (!p) return;
  for (void* q : {(void*)p->d_order, (void*)p->d_nbr, (void*)p->d_coords, (void*)p->d_W, (void*)p->d_R, (void*)p->d_part, (void*)p->d_partbad,
                  (void*)p->d_out, (void*)p->d_bad})
    if (q) (void)hipFree(q);
  delete p;
}

int nblocks(int n) { return (n + RB - 1) / RB; }

// the buffers of a call, for m_cols columns
int reserve(mvc_plan* p, int m_cols) {
  if (m_cols <= p->cols) return MVC_OK;
  for (void* q : {(void*)p->d_W, (void*)p->d_R, (void*)p->d_part})
    if (q) (void)hipFree(q);
  p->d_W = p->d_R = p->d_part = nullptr;
  p->cols = 0;
  const size_t n = (size_t)p->n, ntri1 = (size_t)m_cols * (m_cols + 1) / 2 + 1;
  HIPC(hipMalloc(&p->d_W, sizeof(double) * n * m_cols));
  HIPC(hipMalloc(&p->d_R, sizeof(double) * n * (m_cols + 2)));
  HIPC(hipMalloc(&p->d_part, sizeof(double) * (size_t)nblocks(p->n) * ntri1));
  p->cols = m_cols;
  return MVC_OK;
}

template <int KPAD, int MODEL>
void launch_solve(const mvc_plan* p, const Par& mo, int m_cols) {
  const int per = SOLVE_WAVES * (64 / KPAD);
  hipLaunchKernelGGL((k_vec_solve<KPAD, MODEL>), dim3((unsigned)((p->n + per - 1) / per)), dim3(64 * SOLVE_WAVES), 0, 0, p->d_coords, p->ndim,
                     p->d_order, p->d_nbr, p->n, p->m, mo, p->d_W, m_cols, p->d_R);
}

template <int KPAD>
void launch_solve_model(const mvc_plan* p, int model, const Par& mo, int m_cols) {
  if (model == GAUSSIAN)
    launch_solve<KPAD, GAUSSIAN>(p, mo, m_cols);
  else if (model == EXPONENTIAL)
    launch_solve<KPAD, EXPONENTIAL>(p, mo, m_cols);
  else if (model == SPHERICAL)
    launch_solve<KPAD, SPHERICAL>(p, mo, m_cols);
  else
    launch_solve<KPAD, HOLE_EFFECT>(p, mo, m_cols);
}

}  // namespace

extern "C" {

int mvc_abi_version(void) { return MVC_ABI_VERSION; }
const char* mvc_last_error(void) { return g_err.c_str(); }

int mvc_plan_create(int device, int64_t n, int32_t ndim, const double* coords, const int32_t* order, int32_t m, mvc_plan** plan) {
  if (!coords || !order || !plan) return fail(MVC_EINVAL, "mvc_plan_create: NULL argument");
  *plan = nullptr;
  if (n < 2) return fail(MVC_EINVAL, "mvc_plan_create: need at least two stations");
  if (ndim != 2 && ndim != 3) return fail(MVC_EINVAL, "mvc_plan_create: ndim must be 2 or 3");
  if (m < 1 || m > MVC_MAXNB) return fail(MVC_EINVAL, "mvc_plan_create: m must be in 1..64 (MVC_MAXNB)");
  if (n > ((int64_t)1 << 31) - 1 - RB) return fail(MVC_EINVAL, "mvc_plan_create: the plan of this many stations fits no device");
  if (!all_finite(coords, (size_t)n * ndim)) return fail(MVC_EINVAL, "mvc_plan_create: station coordinates must be finite");
  {
    std::vector<bool> seen((size_t)n, false);
    for (int64_t p = 0; p < n; ++p) {
      const int64_t s = order[p];
      if (s < 0 || s >= n || seen[(size_t)s]) return fail(MVC_EINVAL, "mvc_plan_create: order must be a permutation of 0 .. n - 1");
      seen[(size_t)s] = true;
    }
  }
  HIPC(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, device));
  if ((double)n * (8.0 * ndim + 4.0 + 4.0 * m + 8.0 * MAXCOLS + 8.0 * (MAXCOLS + 2)) > (double)prop.totalGlobalMem / 4.0)
    return fail(MVC_EINVAL, "mvc_plan_create: coordinates, neighbour lists, W and residuals pass a quarter of this device's memory");
  mvc_plan* p = new mvc_plan;
  p->device = device;
  p->n = (int)n;
  p->ndim = ndim;
  p->m = m;
  p->order.assign(order, order + n);
#define TRY(x)                    \
  do {                            \
    hipError_t t_ = (x);          \
    if (t_ != hipSuccess) {       \
      release(p);                 \
      HIPC(t_);                   \
    }                             \
  } while (0)
  TRY(hipMalloc(&p->d_order, sizeof(int) * (size_t)n));
  TRY(hipMalloc(&p->d_nbr, sizeof(int) * (size_t)n * m));
  TRY(hipMalloc(&p->d_coords, sizeof(double) * (size_t)n * ndim));
  TRY(hipMalloc(&p->d_partbad, sizeof(int) * (size_t)nblocks(p->n)));
  TRY(hipMalloc(&p->d_out, sizeof(double) * (MAXCOLS * (MAXCOLS + 1) / 2 + 1)));
  TRY(hipMalloc(&p->d_bad, sizeof(int)));
  TRY(hipMemcpy(p->d_order, order, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  TRY(hipMemcpy(p->d_coords, coords, sizeof(double) * (size_t)n * ndim, hipMemcpyHostToDevice));
  const unsigned blocks = (unsigned)((n + QB - 1) / QB);
  if (ndim == 2)
    hipLaunchKernelGGL((k_vec_knn<2>), dim3(blocks), dim3(QB), knn_lds_bytes(2, m), 0, p->d_coords, p->d_order, p->n, (int)m, p->d_nbr);
  else
    hipLaunchKernelGGL((k_vec_knn<3>), dim3(blocks), dim3(QB), knn_lds_bytes(3, m), 0, p->d_coords, p->d_order, p->n, (int)m, p->d_nbr);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
#undef TRY
  *plan = p;
  return MVC_OK;
}

int mvc_plan_neighbours(const mvc_plan* plan, int32_t* out) {
  if (!plan || !out) return fail(MVC_EINVAL, "mvc_plan_neighbours: NULL argument");
  HIPC(hipSetDevice(plan->device));
  const size_t n = (size_t)plan->n, m = (size_t)plan->m;
  std::vector<int32_t> rows(n * m);  // by position on the device; by station for the caller
  HIPC(hipMemcpy(rows.data(), plan->d_nbr, sizeof(int32_t) * n * m, hipMemcpyDeviceToHost));
  for (size_t p = 0; p < n; ++p)
    for (size_t j = 0; j < m; ++j) out[(size_t)plan->order[p] * m + j] = rows[p * m + j];
  return MVC_OK;
}

int mvc_plan_gram(mvc_plan* plan, const double* coords, int32_t model, double psill, double range, double nugget, const double* W,
                  int32_t m_cols, double* logdet, double* G, int32_t* info) {
  if (!coords || !W || !logdet || !G || !info) return fail(MVC_EINVAL, "mvc_plan_gram: NULL argument");
  *info = 0;
  if (m_cols < 1 || m_cols > MVC_MAXCOLS) return fail(MVC_EINVAL, "mvc_plan_gram: m_cols must be in 1..40 (MVC_MAXCOLS)");
  if (model < MVC_GAUSSIAN || model > MVC_HOLE_EFFECT)
    return fail(MVC_EINVAL, "mvc_plan_gram: model must be one of MVC_GAUSSIAN, MVC_EXPONENTIAL, MVC_SPHERICAL, MVC_HOLE_EFFECT");
  if (!(psill > 0.0 && range > 0.0 && nugget >= 0.0) || !std::isfinite(psill) || !std::isfinite(range) || !std::isfinite(nugget))
    return fail(MVC_EINVAL, "mvc_plan_gram: need finite psill > 0, range > 0 and nugget >= 0");
  if (!plan) return fail(MVC_EINVAL, "mvc_plan_gram: NULL plan");
  const int n = plan->n, ndim = plan->ndim;
  if (!all_finite(coords, (size_t)n * ndim)) return fail(MVC_EINVAL, "mvc_plan_gram: station coordinates must be finite");
  if (!all_finite(W, (size_t)n * m_cols)) return fail(MVC_EINVAL, "mvc_plan_gram: W must be finite");
  HIPC(hipSetDevice(plan->device));
  if (int rc = reserve(plan, m_cols)) return rc;
  HIPC(hipMemcpy(plan->d_coords, coords, sizeof(double) * (size_t)n * ndim, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(plan->d_W, W, sizeof(double) * (size_t)n * m_cols, hipMemcpyHostToDevice));
  const Par mo{psill, range, nugget};
  if (plan->m <= 16)
    launch_solve_model<16>(plan, model, mo, m_cols);
  else if (plan->m <= 32)
    launch_solve_model<32>(plan, model, mo, m_cols);
  else
    launch_solve_model<64>(plan, model, mo, m_cols);
  HIPC(hipGetLastError());
  const int nblk = nblocks(n), ntri = m_cols * (m_cols + 1) / 2;
  hipLaunchKernelGGL(k_vec_reduce, dim3((unsigned)nblk), dim3(256), 0, 0, plan->d_R, n, (int)m_cols, 0, plan->d_part, plan->d_partbad, nblk,
                     plan->d_out, plan->d_bad);
  hipLaunchKernelGGL(k_vec_reduce, dim3(1), dim3(256), 0, 0, plan->d_R, n, (int)m_cols, 1, plan->d_part, plan->d_partbad, nblk, plan->d_out,
                     plan->d_bad);
  HIPC(hipGetLastError());
  int bad = INT_MAX;
  HIPC(hipMemcpy(&bad, plan->d_bad, sizeof(int), hipMemcpyDeviceToHost));
  if (bad != INT_MAX) {
    *info = plan->order[(size_t)bad] + 1;
    char b[200];
    snprintf(b, sizeof b, "mvc_plan_gram: the local system of station %d (position %d) is not positive definite", (int)*info, bad);
    return fail(MVC_ENOTPD, b);
  }
  std::vector<double> out((size_t)ntri + 1);
  HIPC(hipMemcpy(out.data(), plan->d_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
  *logdet = out[(size_t)ntri];
  for (int a = 0; a < m_cols; ++a)
    for (int b = 0; b <= a; ++b) G[(size_t)a * m_cols + b] = G[(size_t)b * m_cols + a] = out[(size_t)a * (a + 1) / 2 + b];
  return MVC_OK;
}

void mvc_plan_destroy(mvc_plan* plan) {
  if (!plan) return;
  (void)hipSetDevice(plan->device);
  release(plan);
}

}  // extern "C"
