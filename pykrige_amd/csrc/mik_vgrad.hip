// mik_vgrad.hip -- host side + C ABI (include/mikvgrad.h) of libmikvgrad.so: log det C^ and W^T C^-1 W under Vecchia's approximation and
// their derivatives with respect to the parameters of the covariance.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -Iinclude pykrige_amd/csrc/mik_vgrad.hip
// Links nothing of the other six libraries: the kernels of mik_k_vecchia.h are compiled into this object from their header, unchanged, as
// libmikgrad.so compiles those of mik_k_lik.h.  A plan owns its device memory: the order, the neighbour lists, and the buffers of a call
// (coordinates, geometry sets, W, residuals, the derivative rows of one slab, partial sums), which grow with the widest call seen.
#include "mik_k_vgrad.h"
#include "../../include/mikvgrad.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace mvc;
using mvg::MAXGEOM;
using mvg::MAXPAR;

static_assert(MVG_GAUSSIAN == GAUSSIAN && MVG_EXPONENTIAL == EXPONENTIAL && MVG_SPHERICAL == SPHERICAL && MVG_HOLE_EFFECT == HOLE_EFFECT,
              "mikvgrad.h and mik_k_vecchia.h disagree");
static_assert(MVG_MAXNB == MAXNB && MVG_MAXCOLS == MAXCOLS && MVG_MAXGEOM == MAXGEOM, "mikvgrad.h and the kernel headers disagree");
// the LDS of the kernels: k_vec_knn at most 55 296 bytes, k_vec_reduce 10 752, k_vgrad_reduce 21 248, the solvers none -- of the 163840 of a CU
static_assert(knn_lds_bytes(3, MAXNB) == 55296 && reduce_lds_bytes() == 10752 && mvg::vreduce_lds_bytes() == 21248,
              "the LDS budgets are not the documented ones");
static_assert(knn_lds_bytes(3, MAXNB) <= 163840 && mvg::vreduce_lds_bytes() <= 163840, "a kernel does not fit the LDS of a CU");

constexpr int SLAB = 64 * RB;  // positions whose derivative rows are held at a time: MVG_SLAB
static_assert(SLAB == MVG_SLAB && SLAB % RB == 0, "a slab is a whole number of reduction blocks");

struct mvg_plan {
  int device = 0;
  int n = 0, ndim = 0, m = 0;
  std::vector<int32_t> order;
  int* d_order = nullptr;
  int* d_nbr = nullptr;
  double* d_coords = nullptr;
  double* d_dco = nullptr;  // MAXGEOM x ndim x n
  int cols = 0;             // the columns d_W, d_R and d_part are sized for
  double* d_W = nullptr;
  double* d_R = nullptr;
  double* d_part = nullptr;
  size_t dr_size = 0, dpart_size = 0;  // doubles of d_DR and d_dpart
  double* d_DR = nullptr;
  double* d_dpart = nullptr;
  int* d_partbad = nullptr;
  double* d_out = nullptr;
  double* d_dout = nullptr;
  int* d_bad = nullptr;
};

namespace {

constexpr int NTRI1 = MAXCOLS * (MAXCOLS + 1) / 2 + 1;

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
      return fail(MVG_EHIP, b_);                                                                             \
    }                                                                                                        \
  } while (0)

bool all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

void release(mvg_plan* p) {
  if (!p) return;
  for (void* q : {(void*)p->d_order, (void*)p->d_nbr, (void*)p->d_coords, (void*)p->d_dco, (void*)p->d_W, (void*)p->d_R, (void*)p->d_part,
                  (void*)p->d_DR, (void*)p->d_dpart, (void*)p->d_partbad, (void*)p->d_out, (void*)p->d_dout, (void*)p->d_bad})
    if (q) (void)hipFree(q);
  delete p;
}

int nblocks(int n) { return (n + RB - 1) / RB; }

// The positions of a slab: MVG_SLAB, or what the environment variable MIK_VGRAD_SLAB names, rounded up to a multiple of RB (a knob for
// the tests: the results do not depend on it).
int slab_positions() {
  const char* s = std::getenv("MIK_VGRAD_SLAB");
  if (!s || !*s) return SLAB;
  const long v = std::strtol(s, nullptr, 10);
  if (v < 1 || v > SLAB) return SLAB;
  return (int)((v + RB - 1) / RB) * RB;
}

// the buffers of a call, for m_cols columns, npar parameters and slabs of `slab` positions
int reserve(mvg_plan* p, int m_cols, int npar, int slab) {
  const size_t n = (size_t)p->n, ntri1 = (size_t)m_cols * (m_cols + 1) / 2 + 1;
  if (m_cols > p->cols) {
    for (void* q : {(void*)p->d_W, (void*)p->d_R, (void*)p->d_part})
      if (q) (void)hipFree(q);
    p->d_W = p->d_R = p->d_part = nullptr;
    p->cols = 0;
    HIPC(hipMalloc(&p->d_W, sizeof(double) * n * m_cols));
    HIPC(hipMalloc(&p->d_R, sizeof(double) * n * (m_cols + 2)));
    HIPC(hipMalloc(&p->d_part, sizeof(double) * (size_t)nblocks(p->n) * ntri1));
    p->cols = m_cols;
  }
  const size_t rows = (size_t)(slab < p->n ? slab : p->n);
  const size_t dr = rows * (size_t)npar * (m_cols + 1), dpart = (size_t)nblocks(p->n) * npar * ntri1;
  if (dr > p->dr_size) {
    if (p->d_DR) (void)hipFree(p->d_DR);
    p->d_DR = nullptr;
    p->dr_size = 0;
    HIPC(hipMalloc(&p->d_DR, sizeof(double) * dr));
    p->dr_size = dr;
  }
  if (dpart > p->dpart_size) {
    if (p->d_dpart) (void)hipFree(p->d_dpart);
    p->d_dpart = nullptr;
    p->dpart_size = 0;
    HIPC(hipMalloc(&p->d_dpart, sizeof(double) * dpart));
    p->dpart_size = dpart;
  }
  return MVG_OK;
}

template <int KPAD, int MODEL>
void launch_solve(const mvg_plan* p, const Par& mo, int m_cols) {
  const int per = SOLVE_WAVES * (64 / KPAD);
  hipLaunchKernelGGL((k_vec_solve<KPAD, MODEL>), dim3((unsigned)((p->n + per - 1) / per)), dim3(64 * SOLVE_WAVES), 0, 0, p->d_coords, p->ndim,
                     p->d_order, p->d_nbr, p->n, p->m, mo, p->d_W, m_cols, p->d_R);
}

template <int KPAD, int MODEL>
void launch_vgrad(const mvg_plan* p, const Par& mo, int m_cols, int ng, int p0, int np) {
  const int per = SOLVE_WAVES * (64 / KPAD);
  hipLaunchKernelGGL((mvg::k_vgrad_solve<KPAD, MODEL>), dim3((unsigned)((np + per - 1) / per)), dim3(64 * SOLVE_WAVES), 0, 0, p->d_coords,
                     p->ndim, p->d_dco, ng, p->d_order, p->d_nbr, p->n, p->m, mo, p->d_W, m_cols, p0, np, p->d_DR);
}

// ng < 0: k_vec_solve over all positions; otherwise k_vgrad_solve over the np positions from p0
template <int KPAD>
void launch_model(const mvg_plan* p, int model, const Par& mo, int m_cols, int ng, int p0, int np) {
#define MVG_ONE(MODEL)                                \
  do {                                                \
    if (ng < 0)                                       \
      launch_solve<KPAD, MODEL>(p, mo, m_cols);       \
    else                                              \
      launch_vgrad<KPAD, MODEL>(p, mo, m_cols, ng, p0, np); \
  } while (0)
  if (model == GAUSSIAN)
    MVG_ONE(GAUSSIAN);
  else if (model == EXPONENTIAL)
    MVG_ONE(EXPONENTIAL);
  else if (model == SPHERICAL)
    MVG_ONE(SPHERICAL);
  else
    MVG_ONE(HOLE_EFFECT);
#undef MVG_ONE
}

void launch_class(const mvg_plan* p, int model, const Par& mo, int m_cols, int ng, int p0, int np) {
  if (p->m <= 16)
    launch_model<16>(p, model, mo, m_cols, ng, p0, np);
  else if (p->m <= 32)
    launch_model<32>(p, model, mo, m_cols, ng, p0, np);
  else
    launch_model<64>(p, model, mo, m_cols, ng, p0, np);
}

}  // namespace

extern "C" {

int mvg_abi_version(void) { return MVG_ABI_VERSION; }
const char* mvg_last_error(void) { return g_err.c_str(); }

int mvg_plan_create(int device, int64_t n, int32_t ndim, const double* coords, const int32_t* order, int32_t m, mvg_plan** plan) {
  if (!coords || !order || !plan) return fail(MVG_EINVAL, "mvg_plan_create: NULL argument");
  *plan = nullptr;
  if (n < 2) return fail(MVG_EINVAL, "mvg_plan_create: need at least two stations");
  if (ndim != 2 && ndim != 3) return fail(MVG_EINVAL, "mvg_plan_create: ndim must be 2 or 3");
  if (m < 1 || m > MVG_MAXNB) return fail(MVG_EINVAL, "mvg_plan_create: m must be in 1..64 (MVG_MAXNB)");
  if (n > ((int64_t)1 << 31) - 1 - RB) return fail(MVG_EINVAL, "mvg_plan_create: the plan of this many stations fits no device");
  if (!all_finite(coords, (size_t)n * ndim)) return fail(MVG_EINVAL, "mvg_plan_create: station coordinates must be finite");
  {
    std::vector<bool> seen((size_t)n, false);
    for (int64_t p = 0; p < n; ++p) {
      const int64_t s = order[p];
      if (s < 0 || s >= n || seen[(size_t)s]) return fail(MVG_EINVAL, "mvg_plan_create: order must be a permutation of 0 .. n - 1");
      seen[(size_t)s] = true;
    }
  }
  HIPC(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, device));
  const double blocks = (double)((n + RB - 1) / RB);
  if ((double)n * (8.0 * ndim + 4.0 + 4.0 * m + 8.0 * MAXCOLS + 8.0 * (MAXCOLS + 2) + 8.0 * MAXGEOM * ndim) +
          blocks * 8.0 * (MAXPAR + 1) * NTRI1 + 8.0 * SLAB * MAXPAR * (MAXCOLS + 1) >
      (double)prop.totalGlobalMem / 4.0)
    return fail(MVG_EINVAL,
                "mvg_plan_create: coordinates, geometry sets, neighbour lists, W, residuals, a slab of derivative rows and the partial sums "
                "pass a quarter of this device's memory");
  mvg_plan* p = new mvg_plan;
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
  TRY(hipMalloc(&p->d_dco, sizeof(double) * (size_t)n * ndim * MAXGEOM));
  TRY(hipMalloc(&p->d_partbad, sizeof(int) * (size_t)nblocks(p->n)));
  TRY(hipMalloc(&p->d_out, sizeof(double) * NTRI1));
  TRY(hipMalloc(&p->d_dout, sizeof(double) * MAXPAR * NTRI1));
  TRY(hipMalloc(&p->d_bad, sizeof(int)));
  TRY(hipMemcpy(p->d_order, order, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
  TRY(hipMemcpy(p->d_coords, coords, sizeof(double) * (size_t)n * ndim, hipMemcpyHostToDevice));
  const unsigned blocks_q = (unsigned)((n + QB - 1) / QB);
  if (ndim == 2)
    hipLaunchKernelGGL((k_vec_knn<2>), dim3(blocks_q), dim3(QB), knn_lds_bytes(2, m), 0, p->d_coords, p->d_order, p->n, (int)m, p->d_nbr);
  else
    hipLaunchKernelGGL((k_vec_knn<3>), dim3(blocks_q), dim3(QB), knn_lds_bytes(3, m), 0, p->d_coords, p->d_order, p->n, (int)m, p->d_nbr);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
#undef TRY
  *plan = p;
  return MVG_OK;
}

int mvg_plan_neighbours(const mvg_plan* plan, int32_t* out) {
  if (!plan || !out) return fail(MVG_EINVAL, "mvg_plan_neighbours: NULL argument");
  HIPC(hipSetDevice(plan->device));
  const size_t n = (size_t)plan->n, m = (size_t)plan->m;
  std::vector<int32_t> rows(n * m);  // by position on the device; by station for the caller
  HIPC(hipMemcpy(rows.data(), plan->d_nbr, sizeof(int32_t) * n * m, hipMemcpyDeviceToHost));
  for (size_t p = 0; p < n; ++p)
    for (size_t j = 0; j < m; ++j) out[(size_t)plan->order[p] * m + j] = rows[p * m + j];
  return MVG_OK;
}

int mvg_plan_grad(mvg_plan* plan, const double* coords, int32_t ng, const double* dcoords, int32_t model, double psill, double range,
                  double nugget, const double* W, int32_t m_cols, double* logdet, double* G, double* dlogdet, double* dG, int32_t* info) {
  if (!coords || !W || !logdet || !G || !dlogdet || !dG || !info) return fail(MVG_EINVAL, "mvg_plan_grad: NULL argument");
  *info = 0;
  if (m_cols < 1 || m_cols > MVG_MAXCOLS) return fail(MVG_EINVAL, "mvg_plan_grad: m_cols must be in 1..40 (MVG_MAXCOLS)");
  if (ng < 0 || ng > MVG_MAXGEOM) return fail(MVG_EINVAL, "mvg_plan_grad: ng must be in 0..5 (MVG_MAXGEOM)");
  if (ng > 0 && !dcoords) return fail(MVG_EINVAL, "mvg_plan_grad: dcoords may be NULL only when ng = 0");
  if (model < MVG_GAUSSIAN || model > MVG_HOLE_EFFECT)
    return fail(MVG_EINVAL, "mvg_plan_grad: model must be one of MVG_GAUSSIAN, MVG_EXPONENTIAL, MVG_SPHERICAL, MVG_HOLE_EFFECT");
  if (!(psill > 0.0 && range > 0.0 && nugget >= 0.0) || !std::isfinite(psill) || !std::isfinite(range) || !std::isfinite(nugget))
    return fail(MVG_EINVAL, "mvg_plan_grad: need finite psill > 0, range > 0 and nugget >= 0");
  if (!plan) return fail(MVG_EINVAL, "mvg_plan_grad: NULL plan");
  const int n = plan->n, ndim = plan->ndim;
  if (!all_finite(coords, (size_t)n * ndim)) return fail(MVG_EINVAL, "mvg_plan_grad: station coordinates must be finite");
  if (ng > 0 && !all_finite(dcoords, (size_t)n * ndim * ng)) return fail(MVG_EINVAL, "mvg_plan_grad: dcoords must be finite");
  if (!all_finite(W, (size_t)n * m_cols)) return fail(MVG_EINVAL, "mvg_plan_grad: W must be finite");
  HIPC(hipSetDevice(plan->device));
  const int npar = 3 + ng, slab = slab_positions();
  if (int rc = reserve(plan, m_cols, npar, slab)) return rc;
  HIPC(hipMemcpy(plan->d_coords, coords, sizeof(double) * (size_t)n * ndim, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(plan->d_W, W, sizeof(double) * (size_t)n * m_cols, hipMemcpyHostToDevice));
  if (ng > 0) HIPC(hipMemcpy(plan->d_dco, dcoords, sizeof(double) * (size_t)n * ndim * ng, hipMemcpyHostToDevice));
  const Par mo{psill, range, nugget};
  // logdet and G: mvc_plan_gram's launches of the same kernels
  launch_class(plan, model, mo, m_cols, -1, 0, n);
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
    snprintf(b, sizeof b, "mvg_plan_grad: the local system of station %d (position %d) is not positive definite", (int)*info, bad);
    return fail(MVG_ENOTPD, b);
  }
  // the derivatives, slab by slab; a slab is a whole number of reduction blocks, so no partial sum sees the cut
  for (int p0 = 0; p0 < n; p0 += slab) {
    const int np = n - p0 < slab ? n - p0 : slab;
    launch_class(plan, model, mo, m_cols, ng, p0, np);
    hipLaunchKernelGGL(mvg::k_vgrad_reduce, dim3((unsigned)nblocks(np), (unsigned)npar), dim3(256), 0, 0, plan->d_R, plan->d_DR, n, (int)m_cols,
                       npar, 0, p0, plan->d_dpart, nblk, plan->d_dout);
    HIPC(hipGetLastError());
  }
  const int all = npar * (ntri + 1);
  hipLaunchKernelGGL(mvg::k_vgrad_reduce, dim3((unsigned)((all + 255) / 256)), dim3(256), 0, 0, plan->d_R, plan->d_DR, n, (int)m_cols, npar, 1, 0,
                     plan->d_dpart, nblk, plan->d_dout);
  HIPC(hipGetLastError());
  std::vector<double> out((size_t)ntri + 1), dout((size_t)all);
  HIPC(hipMemcpy(out.data(), plan->d_out, sizeof(double) * out.size(), hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(dout.data(), plan->d_dout, sizeof(double) * dout.size(), hipMemcpyDeviceToHost));
  *logdet = out[(size_t)ntri];
  for (int a = 0; a < m_cols; ++a)
    for (int b = 0; b <= a; ++b) G[(size_t)a * m_cols + b] = G[(size_t)b * m_cols + a] = out[(size_t)a * (a + 1) / 2 + b];
  const size_t mm = (size_t)m_cols * m_cols;
  for (int k = 0; k < npar; ++k) {
    const double* o = dout.data() + (size_t)k * (ntri + 1);
    dlogdet[k] = o[ntri];
    for (int a = 0; a < m_cols; ++a)
      for (int b = 0; b <= a; ++b) dG[k * mm + (size_t)a * m_cols + b] = dG[k * mm + (size_t)b * m_cols + a] = o[(size_t)a * (a + 1) / 2 + b];
  }
  return MVG_OK;
}

void mvg_plan_destroy(mvg_plan* plan) {
  if (!plan) return;
  (void)hipSetDevice(plan->device);
  release(plan);
}

}  // extern "C"
