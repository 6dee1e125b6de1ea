// mik_vario3.hip -- host side + C ABI (include/mikvario3.h) of libmikvario3.so: directional semivariograms and variogram maps in 3-D.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -Iinclude pykrige_amd/csrc/mik_vario3.hip
// Links nothing of libmikrige.so or libmikvario.so and keeps no state: every call selects its device, uploads, runs, copies back and frees.
#include "mik_k_vario3.h"
#include "../../include/mikvario3.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using namespace mkv3;

static_assert(MKV3_MAXLAGS == MAXLAGS && MKV3_MAXDIRS == MAXDIRS && MKV3_FCHUNK == FCHUNK, "mikvario3.h and mik_k_vario3.h disagree");
// the largest map: one half, 2113 cells x (8 sums + a 32-bit count) = 143 684 bytes, beside 6 coordinate and 16 value tiles = 11 264 bytes
static_assert(vario3_lds_bytes(true, (MKV3_MAXCELLS + 1) / 2, 1, FCHUNK) == 143684 + 11264, "the LDS budget of the largest map is not the documented one");
static_assert(vario3_lds_bytes(true, (MKV3_MAXCELLS + 1) / 2, 1, FCHUNK) <= 160 * 1024, "the largest map does not fit the LDS of a CU");
static_assert(vario3_lds_bytes(false, MKV3_MAXLAGS * MKV3_MAXDIRS, 1, FCHUNK) <= 160 * 1024, "the largest histogram does not fit the LDS of a CU");

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
      return fail(MKV3_EHIP, b_);                                                                            \
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

int check_stations(const char* who, int64_t n, const double* x, const double* y, const double* z, const double* values, int32_t nf) {
  const std::string w(who);
  if (!x || !y || !z || !values) return fail(MKV3_EINVAL, w + ": NULL argument");
  if (n < 2) return fail(MKV3_EINVAL, w + ": need at least two stations");
  if (n >= (int64_t)1 << 31) return fail(MKV3_EINVAL, w + ": n must be below 2^31");
  if (nf < 1) return fail(MKV3_EINVAL, w + ": need at least one field");
  if (!all_finite(x, (size_t)n) || !all_finite(y, (size_t)n) || !all_finite(z, (size_t)n))
    return fail(MKV3_EINVAL, w + ": station coordinates must be finite");
  if (!all_finite(values, (size_t)n * (size_t)nf)) return fail(MKV3_EINVAL, w + ": values must be finite");
  return MKV3_OK;
}

// The passes over the pairs (one per chunk of FCHUNK fields) and the sums of the workgroups' partials.  `a` arrives with the geometry set;
// cells = histogram cells a workgroup keeps.  Results: semi (nf x cells), lag (cells, directions only), cnt (cells), on the host.
template <bool MAP>
int run_passes(int device, Vario3Args a, int64_t n, const double* x, const double* y, const double* z, const double* values, int32_t nf,
               const double* edges, std::vector<double>& semi, std::vector<double>& lag, std::vector<long long>& cnt) {
  HIPC(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, device));
  const int cells = a.cells;
  const int fmax = std::min<int>(nf, FCHUNK);
  // copies of the histogram, one per wave (pair), while a workgroup stays within a quarter of the CU's LDS
  int copies = 4;
  while (copies > 1 && vario3_lds_bytes(MAP, cells, copies, fmax) > 40 * 1024) copies >>= 1;
  const size_t lds = vario3_lds_bytes(MAP, cells, copies, fmax);
  const size_t lds_cu = std::max<size_t>(prop.sharedMemPerBlock, prop.maxSharedMemoryPerMultiProcessor);
  if (lds > lds_cu) return fail(MKV3_EHIP, "this device has less LDS per workgroup than the histogram needs");
  const long nt = (long)((n + TILE - 1) / TILE), ntiles = nt * (nt + 1) / 2;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, lds_cu / lds));
  const int nwg = (int)std::min<long>(ntiles, (long)per_cu * prop.multiProcessorCount);
  auto kernel = MAP ? k_vario3_map : k_vario3_dir;
  HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

  Dev dx, dy, dz, dv, de, psemi, plag, pcnt, osemi, olag, ocnt;
  const size_t nb = sizeof(double) * (size_t)n;
  HIPC(hipMalloc(&dx.p, nb));
  HIPC(hipMalloc(&dy.p, nb));
  HIPC(hipMalloc(&dz.p, nb));
  HIPC(hipMalloc(&dv.p, nb * nf));
  HIPC(hipMalloc(&psemi.p, sizeof(double) * (size_t)nwg * fmax * cells));
  HIPC(hipMalloc(&plag.p, sizeof(double) * (size_t)nwg * cells));
  HIPC(hipMalloc(&pcnt.p, sizeof(unsigned long long) * (size_t)nwg * cells));
  HIPC(hipMalloc(&osemi.p, sizeof(double) * (size_t)nf * cells));
  HIPC(hipMalloc(&olag.p, sizeof(double) * cells));
  HIPC(hipMalloc(&ocnt.p, sizeof(long long) * cells));
  HIPC(hipMemcpy(dx.p, x, nb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dy.p, y, nb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dz.p, z, nb, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dv.p, values, nb * nf, hipMemcpyHostToDevice));
  if (!MAP) {
    HIPC(hipMalloc(&de.p, sizeof(double) * (a.nlags + 1)));
    HIPC(hipMemcpy(de.p, edges, sizeof(double) * (a.nlags + 1), hipMemcpyHostToDevice));
  }
  HIPC(hipMemset(pcnt.p, 0, sizeof(unsigned long long) * (size_t)nwg * cells));
  a.x = dx.as<double>();
  a.y = dy.as<double>();
  a.z = dz.as<double>();
  a.edges = de.as<double>();
  a.n = n;
  a.nt = (int)nt;
  a.ntiles = ntiles;
  a.copies = copies;
  a.part_semi = psemi.as<double>();
  a.part_lag = plag.as<double>();
  a.part_cnt = pcnt.as<unsigned long long>();
  for (int f0 = 0; f0 < nf; f0 += FCHUNK) {
    a.v = dv.as<double>() + (size_t)f0 * n;
    a.nfc = std::min<int>(FCHUNK, nf - f0);
    a.first = f0 == 0;
    // (the layout of a later, shorter chunk needs no more LDS than the first)
    hipLaunchKernelGGL(kernel, dim3(nwg), dim3(THREADS), vario3_lds_bytes(MAP, cells, copies, a.nfc), 0, a);
    const long m = (long)a.nfc * cells;
    hipLaunchKernelGGL(k_vario3_sum, dim3((unsigned)((m + THREADS - 1) / THREADS)), dim3(THREADS), 0, 0, (const double*)a.part_semi, nwg, m,
                       osemi.as<double>() + (size_t)f0 * cells);
    if (a.first) {
      const unsigned gb = (unsigned)((cells + THREADS - 1) / THREADS);
      if (!MAP) hipLaunchKernelGGL(k_vario3_sum, dim3(gb), dim3(THREADS), 0, 0, (const double*)a.part_lag, nwg, (long)cells, olag.as<double>());
      hipLaunchKernelGGL(k_vario3_sum_cnt, dim3(gb), dim3(THREADS), 0, 0, (const unsigned long long*)a.part_cnt, nwg, (long)cells,
                         ocnt.as<long long>());
    }
    HIPC(hipGetLastError());
  }
  semi.resize((size_t)nf * cells);
  cnt.resize(cells);
  HIPC(hipMemcpy(semi.data(), osemi.p, sizeof(double) * semi.size(), hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(cnt.data(), ocnt.p, sizeof(long long) * cells, hipMemcpyDeviceToHost));
  if (!MAP) {
    lag.resize(cells);
    HIPC(hipMemcpy(lag.data(), olag.p, sizeof(double) * cells, hipMemcpyDeviceToHost));
  }
  return MKV3_OK;
}

}  // namespace

extern "C" {

int mkv3_abi_version(void) { return MKV3_ABI_VERSION; }
const char* mkv3_last_error(void) { return g_err.c_str(); }

int mkv3_directional(int device, int64_t n, const double* x, const double* y, const double* z, const double* values, int32_t nf,
                     const double* dirs, int32_t na, double tol_deg, double bandwidth, const double* edges, int32_t nlags, double* lag_sum,
                     double* semi_sum, int64_t* count) {
  if (int rc = check_stations("mkv3_directional", n, x, y, z, values, nf)) return rc;
  if (!dirs || !edges || !lag_sum || !semi_sum || !count) return fail(MKV3_EINVAL, "mkv3_directional: NULL argument");
  if (nlags < 1 || nlags > MKV3_MAXLAGS) return fail(MKV3_EINVAL, "mkv3_directional: nlags must be in 1..64 (MKV3_MAXLAGS)");
  if (na < 1 || na > MKV3_MAXDIRS) return fail(MKV3_EINVAL, "mkv3_directional: the number of directions must be in 1..16 (MKV3_MAXDIRS)");
  if (!(tol_deg > 0.0 && tol_deg <= 90.0)) return fail(MKV3_EINVAL, "mkv3_directional: tol_deg must be in (0, 90]");
  if (!std::isfinite(bandwidth)) return fail(MKV3_EINVAL, "mkv3_directional: bandwidth must be finite (<= 0: none)");
  if (!all_finite(dirs, (size_t)na * 3)) return fail(MKV3_EINVAL, "mkv3_directional: directions must be finite");
  for (int q = 0; q < na; ++q) {
    const double* u = dirs + 3 * q;
    if (!(std::fabs(std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - 1.0) <= MKV3_UNIT_TOL))
      return fail(MKV3_EINVAL, "mkv3_directional: every direction must be a unit vector (norm within 1e-12 of 1)");
  }
  if (!all_finite(edges, (size_t)nlags + 1)) return fail(MKV3_EINVAL, "mkv3_directional: edges must be finite");
  for (int b = 0; b < nlags; ++b)
    if (!(edges[b] < edges[b + 1])) return fail(MKV3_EINVAL, "mkv3_directional: edges must be ascending");
  Vario3Args a{};
  a.nlags = nlags;
  a.na = na;
  a.cells = na * nlags;
  a.all = tol_deg == 90.0;
  for (int q = 0; q < na; ++q) {
    a.ux[q] = dirs[3 * q];
    a.uy[q] = dirs[3 * q + 1];
    a.uz[q] = dirs[3 * q + 2];
  }
  const double t = std::tan(tol_deg * (M_PI / 180.0));
  a.tan2 = t * t;
  a.band = bandwidth > 0.0;
  a.bw2 = a.band ? bandwidth * bandwidth : 0.0;
  std::vector<double> semi, lag;
  std::vector<long long> cnt;
  if (int rc = run_passes<false>(device, a, n, x, y, z, values, nf, edges, semi, lag, cnt)) return rc;
  std::copy(semi.begin(), semi.end(), semi_sum);
  std::copy(lag.begin(), lag.end(), lag_sum);
  std::copy(cnt.begin(), cnt.end(), count);
  return MKV3_OK;
}

int mkv3_map(int device, int64_t n, const double* x, const double* y, const double* z, const double* values, int32_t nf, int32_t nx,
             int32_t ny, int32_t nz, double dx, double dy, double dz, double* semi_sum, int64_t* count) {
  if (int rc = check_stations("mkv3_map", n, x, y, z, values, nf)) return rc;
  if (!semi_sum || !count) return fail(MKV3_EINVAL, "mkv3_map: NULL argument");
  if (nx < 0 || ny < 0 || nz < 0) return fail(MKV3_EINVAL, "mkv3_map: nx, ny and nz must not be negative");
  if (nx > MKV3_MAXCELLS || ny > MKV3_MAXCELLS || nz > MKV3_MAXCELLS ||
      (2 * (int64_t)nx + 1) * (2 * (int64_t)ny + 1) * (2 * (int64_t)nz + 1) > MKV3_MAXCELLS)
    return fail(MKV3_EINVAL, "mkv3_map: (2 nx + 1)(2 ny + 1)(2 nz + 1) must be at most 4225 cells (MKV3_MAXCELLS)");
  if (!(dx > 0.0 && dy > 0.0 && dz > 0.0) || !std::isfinite(dx) || !std::isfinite(dy) || !std::isfinite(dz))
    return fail(MKV3_EINVAL, "mkv3_map: dx, dy and dz must be positive and finite");
  const int ncell = (2 * nx + 1) * (2 * ny + 1) * (2 * nz + 1), half = ncell / 2 + 1;
  Vario3Args a{};
  a.mnx = nx;
  a.mny = ny;
  a.mnz = nz;
  a.cdx = dx;
  a.cdy = dy;
  a.cdz = dz;
  a.cells = half;
  std::vector<double> semi, lag;
  std::vector<long long> cnt;
  if (int rc = run_passes<true>(device, a, n, x, y, z, values, nf, nullptr, semi, lag, cnt)) return rc;
  // a pair was binned once, at the cell of h or of -h whichever comes first; both cells get it (the centre cell twice)
  for (int c = 0; c < ncell; ++c) {
    const int s = c < half ? c : ncell - 1 - c;
    const int twice = c == half - 1 ? 2 : 1;
    count[c] = (int64_t)cnt[s] * twice;
    for (int f = 0; f < nf; ++f) semi_sum[(size_t)f * ncell + c] = semi[(size_t)f * half + s] * twice;
  }
  return MKV3_OK;
}

}  // extern "C"
