// mik_mw.hip -- moving-window kriging: neighbour search, solver dispatch, prediction
// One translation unit of libmikrige.so (pykrige_amd/build.py compiles them in parallel).
#include "mik_k_mw.h"
#include "mik_host.h"

// Sort the stations into a uniform grid of cells for the moving-window neighbour search (counting sort on the host, O(N)).
// The cell edge aims at `target` stations per cell; geographic problems are binned by their unit-sphere vectors.
static int build_mw_grid(mik_handle* h, int target) {
  if (h->grid.target == target) return MIK_OK;
  const int N = h->N, D = (h->geo || h->ndim == 3) ? 3 : 2;
  std::vector<double> c[3];
  if (h->geo) {
    for (int d = 0; d < 3; ++d) c[d].resize(N);
    for (int i = 0; i < N; ++i) {  // k_geo_unit's formula
      const double lo = h->hxs[i] * MIK_PI / 180.0, la = h->hys[i] * MIK_PI / 180.0;
      c[0][i] = cos(lo) * cos(la);
      c[1][i] = sin(lo) * cos(la);
      c[2][i] = sin(la);
    }
  } else {
    c[0] = h->hxs;
    c[1] = h->hys;
    if (D == 3) c[2] = h->hzs;
  }
  double lo[3] = {0, 0, 0}, ext[3] = {0, 0, 0};
  double vol = 1.0;
  int live = 0;
  for (int d = 0; d < D; ++d) {
    const auto mm = std::minmax_element(c[d].begin(), c[d].end());
    lo[d] = *mm.first;
    ext[d] = *mm.second - *mm.first;
    if (ext[d] > 0.0 && std::isfinite(ext[d])) {
      vol *= ext[d];
      ++live;
    }
  }
  int n[3] = {1, 1, 1};
  double cell = 1.0;
  if (live > 0 && N > 4 * target) {
    cell = pow(vol * (double)target / (double)N, 1.0 / live);
    for (;;) {  // keep the grid below ~4M cells
      double cells = 1.0;
      for (int d = 0; d < D; ++d) cells *= (ext[d] > 0.0 && std::isfinite(ext[d])) ? std::max(1.0, ceil(ext[d] / cell)) : 1.0;
      if (cells <= 4.0e6) break;
      cell *= 1.5;
    }
    for (int d = 0; d < D; ++d)
      if (ext[d] > 0.0 && std::isfinite(ext[d])) n[d] = (int)std::max(1.0, ceil(ext[d] / cell));
  }
  const long ncell = (long)n[0] * n[1] * n[2];
  std::vector<int> cellof(N), start(ncell + 1, 0), orig(N);
  for (int i = 0; i < N; ++i) {
    long id[3] = {0, 0, 0};
    for (int d = 0; d < D; ++d)
      if (n[d] > 1) id[d] = std::min<long>(n[d] - 1, std::max<long>(0, (long)floor((c[d][i] - lo[d]) / cell)));
    const long ci = (id[2] * n[1] + id[1]) * n[0] + id[0];
    cellof[i] = (int)ci;
    ++start[ci + 1];
  }
  for (long k = 0; k < ncell; ++k) start[k + 1] += start[k];
  std::vector<int> fill(start.begin(), start.end() - 1);
  std::vector<double> g[3];
  for (int d = 0; d < D; ++d) g[d].resize(N);
  for (int i = 0; i < N; ++i) {  // stable: stations of a cell stay in index order
    const int pos = fill[cellof[i]]++;
    orig[pos] = i;
    for (int d = 0; d < D; ++d) g[d][pos] = c[d][i];
  }
  auto& G = h->grid;
  MIKC(G.gx.ensure(sizeof(double) * N));
  MIKC(G.gy.ensure(sizeof(double) * N));
  MIKC(G.gz.ensure(sizeof(double) * N));
  MIKC(G.orig.ensure(sizeof(int) * N));
  MIKC(G.cstart.ensure(sizeof(int) * (size_t)(ncell + 1)));
  HIPC(hipMemcpyAsync(G.gx.p, g[0].data(), sizeof(double) * N, hipMemcpyHostToDevice, h->stream));
  HIPC(hipMemcpyAsync(G.gy.p, g[1].data(), sizeof(double) * N, hipMemcpyHostToDevice, h->stream));
  if (D == 3) HIPC(hipMemcpyAsync(G.gz.p, g[2].data(), sizeof(double) * N, hipMemcpyHostToDevice, h->stream));
  HIPC(hipMemcpyAsync(G.orig.p, orig.data(), sizeof(int) * N, hipMemcpyHostToDevice, h->stream));
  HIPC(hipMemcpyAsync(G.cstart.p, start.data(), sizeof(int) * (size_t)(ncell + 1), hipMemcpyHostToDevice, h->stream));
  HIPC(hipStreamSynchronize(h->stream));  // the host vectors go out of scope
  G.nx = n[0], G.ny = n[1], G.nz = n[2];
  G.x0 = lo[0], G.y0 = lo[1], G.z0 = lo[2];
  G.cell = cell;
  G.target = target;
  G.live = live;
  G.per_cell = (double)N / ((double)n[0] * n[1] * n[2]);
  return MIK_OK;
}

// (dispatch_mw_solve: mik_mw_solve.hip)
// the classes of k_mw_chol live in mik_mw_chol.hip (four translation units): class = 100 G + RI
static int launch_mw_chol_class(mik_handle* h, const MwArgs& a, long pc, int cls) {
  for (int part = 0; part < MIK_MWC_PARTS; ++part) {
    const int rc = mw_chol_part(part, cls, h->stream, h->opt_mw_static != 0, a, pc);
    if (rc != MIK_MWC_NOCLASS) return rc;
  }
  return fail(MIK_EINVAL, "mw_class: no such LDL^T class");
}

// thread-grid / register-tile classes of k_mw_chol: {G, RI} covers K <= G * RI; returns 100 G + RI
#define MIK_MW_CHOL_KMAX 256
static int mw_chol_class(const mik_handle* h, int K) {
  if (h->opt_mw_class) {  // "mw_class" = 100 G + RI: a class forced for A/B runs (scripts/mw_classes.py)
    // (round 4: the classes that lost every A/B of rounds 2-3 -- {8,14}, {8,16}, {16,4..6}, {16,15}, {16,16}, {32,5..7} -- are no longer
    // built: each was a 100 000-instruction kernel; profiles/r03_mw_classes_*.txt keep their measurements)
    return h->opt_mw_class;
  }
  // measured per window size (scripts/mw_classes.py, profiles/r03_mw_classes_after_kernel_changes.txt): one wavefront per point
  // as long as the register tile stays at RI <= 13 (RI = 13 only with the lean update below; beyond that the kernel needs more
  // than 256 registers and the occupancy halves: 2 x slower), then 256 threads per point up to RI = 12, 1024 threads for the last two
  if (K <= 16) return 100 * 4 + 4;    // 16 threads per point, 4 points per wavefront
  // round 4 (profiles/r04_mw_classes_g4.txt): 16 threads per point keep winning while the tile fits -- k = 24: {4,6} 0.37 ms per
  // 2e5 points against {8,4} 0.76; k = 32: {4,8} 0.70 / 0.93; k = 40: {4,10} 1.39 / {8,6} 1.50; k = 50: {4,13} 2.15 / {8,8} 2.54
  if (K <= 24) return 100 * 4 + 6;
  if (K <= 32) return 100 * 4 + 8;
  if (K <= 40) return 100 * 4 + 10;
  if (K <= 48) return 100 * 8 + 6;    // one wavefront per point from here to K = 104: no workgroup barrier
  if (K <= 52) return 100 * 4 + 13;
  if (K <= 64) return 100 * 8 + 8;
  if (K <= 80) return 100 * 8 + 10;
  if (K <= 88) return 100 * 8 + 11;
  if (K <= 96) return 100 * 8 + 12;
  // RI = 13 in one wavefront (round 3, second session): held to 2 wavefronts per SIMD by its launch bound, row factors read as
  // they are used (MIK_MWC_LEAN): 8 spilled registers instead of 24 AGPRs and half the occupancy -- k = 100: 10.9 ms per 2e5
  // points against 13.5 for {16,7}.  {8,14} ties with {16,7} at k = 112 (14.5 / 14.2 ms): not used.
  if (K <= 104) return 100 * 8 + 13;
  if (K <= 112) return 100 * 16 + 7;  // 256 threads per point
  if (K <= 128) return 100 * 16 + 8;
  if (K <= 144) return 100 * 16 + 9;
  if (K <= 160) return 100 * 16 + 10;
  if (K <= 176) return 100 * 16 + 11;
  if (K <= 192) return 100 * 16 + 12;
  // second session of round 3: RI = 13 / 14 on 256 threads, held to 2 wavefronts per SIMD (launch bound + lean update): k = 200
  // 113 -> 65 ms per 2e5 points, k = 224 123 -> 88 ms -- they replace the 1024-thread class {32,7}
  if (K <= 208) return 100 * 16 + 13;
  if (K <= 224) return 100 * 16 + 14;
  return 100 * 32 + 8;                // K <= 256: 1024 threads per point
}

// byte bounds of a job's work arrays (not options)
static constexpr double MW_LIST_BYTES = 2e9;   // K > MIK_MW_KMAX: the neighbour lists of a chunk (12 K bytes per point, twice over)
static constexpr double MW_TABLE_BYTES = 1e9;  // custom variogram: a chunk's K x K pair distances, which visit the host
static constexpr double MW_CHOLB_BYTES = 6e9;  // blocked Cholesky: the per-block scratch systems in total
static constexpr double MW_BIG_BYTES = 4e9;    // pivoting LU in HBM: likewise
static constexpr double MW_PLANE_BYTES = 2e9;  // several value fields: the planes of a field group

// candidate buffer of the wave-per-point neighbour search: a power of two >= K + 256 (beyond "mw_lds_cap" the lists live in HBM)
static int mw_knn_cap(int K) {
  int cap = 512;
  while (cap < K + 256) cap <<= 1;
  return cap;
}
// value fields per group: the planes (npt doubles per field, twice over where the job runs in an order of its own) are bounded to ~2 GB
static int mw_field_group(int nf, long npt, bool permuted) {
  const long per = (long)(MW_PLANE_BYTES / (8.0 * (double)npt * (permuted ? 2.0 : 1.0)));
  return (int)std::max(1L, std::min<long>(nf, per));
}

// One moving-window job: a list of queries, each kriged from its K nearest stations.  mik_predict_moving_window's job is the resident
// points; mik_cross_validate_window's is the stations themselves in the cell-sorted order of the search grid, each left out of its own
// window (self).  run_mw_job is the loop over field groups and point chunks that both share; what it runs is decided once (plan_mw_job)
// and issued stage by stage: mw_search, mw_rhs, mw_solve per chunk, mw_deliver per group, mw_read_back at the end.
struct MwJob {
  long npt = 0;
  const double *qx = nullptr, *qy = nullptr, *qz = nullptr;  // search coordinates in job order (geographic: unit vectors)
  const double *lon = nullptr, *lat = nullptr;               // geographic: the queries in degrees, job order (k_mw_geo_dist)
  const int* self = nullptr;      // per query the station that is the query itself and stays out of its window; nullptr = none
  bool lane = false;              // 64 consecutive queries share a few cells of the station grid (k_mw_knn_lane applies for K <= 16)
  const unsigned* perm = nullptr; // job order -> caller's order (k_ps_unsort); nullptr = the job runs in the caller's order
  double *zs = nullptr, *sss = nullptr;  // z, sigma^2 as the solvers write them (job order)
  double *z = nullptr, *ss = nullptr;    // z, sigma^2 in the caller's order (== zs, sss without perm)
  int fg = 1;                            // fields per group
  double *fs = nullptr, *fz = nullptr;   // the group's field planes, fg x npt: job order (with perm only) / caller's order
  bool landing = true;                   // the planes leave for the landing zones (pin_out / pin_fz); false: for hz (nf x npt, caller's memory)
  double* hz = nullptr;
  const double* off = nullptr;           // block kriging (mik_predict_block_window): the nd x ndim adjusted node offsets on the device; the
  int nd = 0;                            // queries are block centres and the right-hand sides are averaged over the nodes.  nd = 0: points
  // a pattern of mik_predict_window_gaps: the stations the pattern has, the value rows of its fields and where their planes go
  const unsigned char* live = nullptr;   // per SORTED station (the grid's order) 1 = the pattern has it; nullptr = every station (KnnArgs::live)
  double live_frac = 1.0;                // the share of stations it has: scales the density behind the first-pass bound, nothing else
  const double* fv = nullptr;            // the job's own nfl value rows (N each, caller's station order) instead of the handle's fields
  int nfl = 0;
  const int* fields = nullptr;           // with hz: the caller's plane of each of the job's fields (host); nullptr = plane f is field f
};

// the solver of a job's local systems; the values are timing()'s "mw_kernel"
//   MW_CHOL   LDL^T of the SPD-shifted system in registers, no pivot search (k_mw_chol's classes; windows up to MIK_MW_CHOL_KMAX)
//   MW_PIVOT  Gauss-Jordan in registers with implicit partial pivoting (dispatch_mw_solve; windows up to MIK_MW_KMAX)
//   MW_BIG    LU with partial pivoting in HBM scratch (k_mw_solve_big; any window)
//   MW_CHOLB  blocked Cholesky of the shifted system, one block per point, panels of 64 in LDS, the matrix in an L2-resident scratch slot
//             (k_mw_chol_blocked; beyond the register classes, and for smaller windows under "mw_class" 1)
enum MwSolver { MW_CHOL = 1, MW_PIVOT = 2, MW_BIG = 3, MW_CHOLB = 4 };

// what one job runs (plan_mw_job): decided before the first launch, the same for every chunk and group -- and decided anew by the redo
struct MwPlan {
  int K, nb, nf;  // window, rows of a local system, value fields (mik_set_fields; 0 = the problem's values)
  long npt, chunk, nchunks;
  bool custom, three, permuted;
  MwSolver solver;
  bool mw_piv;              // the systems are solved with a pivot search
  int cap;                  // candidate buffer of the wave-per-point search
  bool wave_knn, lane;      // the search runs in LDS over the station grid (else: the list scan in HBM); the lane pass runs in front of it
  int rows, fg, ngroups;    // value rows per solver pass; fields per group, groups
  int ldc, sgrid;       // MW_CHOLB: leading dimension of a scratch system; MW_CHOLB / MW_BIG: blocks of a solver launch
  long cslot;           // MW_CHOLB: doubles of a scratch slot
  size_t sys_bytes, knn_lds, solve_lds;  // all scratch slots; dynamic LDS of k_mw_knn and of k_mw_chol_blocked / k_mw_solve_big
};

// the work buffers of one call and the station coordinates the list scan reads (geographic: unit vectors in su).  Scoped: released when
// run_mw_job returns, and it returns only after the stream has drained.
struct MwWork {
  DevBuf su, wd, wi, sysbuf, gtab, gvec, todo;
  const double *sx = nullptr, *sy = nullptr, *sz = nullptr;
};

// the job's buffers in the sizes of its plan, the cleared singularity flag and, for the list scan, the stations' unit vectors
static int size_mw_work(mik_handle* h, const MwPlan& p, const MwJob& J, MwWork& w) {
  const size_t ck = (size_t)p.chunk * (size_t)p.K;
  MIKC(h->mw_idx.ensure(sizeof(int) * ck));
  MIKC(h->mw_dist.ensure(sizeof(double) * ck));
  MIKC(h->flag.ensure(sizeof(int)));
  HIPC(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  if (p.custom) {
    MIKC(w.gtab.ensure(sizeof(double) * ck * (size_t)p.K));
    MIKC(w.gvec.ensure(sizeof(double) * ck));
  }
  w.sx = h->xs.as<double>(), w.sy = h->ys.as<double>(), w.sz = h->zs.as<double>();
  if (!p.wave_knn) {
    if (J.self || J.live) return fail(MIK_EINVAL, "moving window: the list search in HBM leaves no station out");  // (the entry points refuse such a K)
    MIKC(w.wd.ensure(sizeof(double) * ck));
    MIKC(w.wi.ensure(sizeof(int) * ck));
    if (h->geo) {  // station unit vectors for the plain scan
      MIKC(w.su.ensure(sizeof(double) * 3 * (size_t)h->N));
      double* s3 = w.su.as<double>();
      hipLaunchKernelGGL(k_geo_unit, dim3((h->N + 255) / 256), dim3(256), 0, h->stream, w.sx, w.sy, h->N, s3, s3 + h->N,
                         s3 + 2 * (size_t)h->N);
      w.sx = s3, w.sy = s3 + h->N, w.sz = s3 + 2 * (size_t)h->N;
    }
  }
  MIKC(w.sysbuf.ensure(p.sys_bytes));
  if (p.lane) MIKC(w.todo.ensure(sizeof(int) * ((size_t)p.chunk + 1)));
  return MIK_OK;
}

// solver, chunk, search and field groups of a job of J.npt queries with windows of K; the work buffers in those sizes
static int plan_mw_job(mik_handle* h, int K, const MwJob& J, MwPlan& p, MwWork& w) {
  const long npt = J.npt;
  p = MwPlan{};
  p.K = K, p.nb = K + 1, p.nf = J.fv ? J.nfl : h->nf, p.npt = npt;
  p.custom = h->model == MIK_MODEL_CUSTOM, p.three = h->geo || h->ndim == 3, p.permuted = J.perm != nullptr;
  // The reference cuts each point's system out of a_all = self._get_kriging_matrix(n); here its entries are computed from the selected
  // stations' coordinates, so no N x N matrix exists on this path (and a factor held by the handle stays valid).
  // Small windows are solved without a pivot search on the SPD-shifted local system unless the model cannot promise a positive definite
  // station block (hole-effect), has no device functor for the shift (custom), or a previous attempt of this call hit a bad pivot.
  p.mw_piv = p.custom || h->model == MIK_MODEL_HOLE_EFFECT || h->mw_force_piv || h->opt_mw_pivot;
  const bool chol = !p.mw_piv && K <= MIK_MW_CHOL_KMAX && h->opt_mw_class != 1;
  const bool cholb = !p.mw_piv && !chol && K >= 8;
  p.solver = chol ? MW_CHOL : cholb ? MW_CHOLB : K > MIK_MW_KMAX ? MW_BIG : MW_PIVOT;
  // K <= MIK_MW_KMAX: candidate lists in registers, systems in LDS, all points in one pass.  Larger K: working sets in HBM, points in
  // chunks that bound the neighbour lists (12 K bytes per point, twice over); custom: the table of pair distances as well
  long chunk = npt;  // (whole multiples of 256 points, at least 256, at most all)
  if (K > MIK_MW_KMAX) chunk = std::min(chunk, std::max(256L, ((long)(MW_LIST_BYTES / (24.0 * K)) / 256) * 256));
  if (p.custom) chunk = std::min(chunk, std::max(256L, ((long)(MW_TABLE_BYTES / (8.0 * K * (K + 1.0))) / 256) * 256));
  p.chunk = chunk, p.nchunks = (npt + chunk - 1) / chunk;
  p.cap = mw_knn_cap(K);
  p.wave_knn = p.cap <= h->opt_mw_lds_cap;  // default 8192 = 96 KB of LDS; beyond that the lists live in HBM
  p.knn_lds = (size_t)p.cap * (sizeof(double) + sizeof(int));
  // (measured, profiles/r04_mw_knn_ab.txt: rows of a grid, k = 10: search + rhs 2.65 -> 0.62 ms per 1e6 points, bit-identical; a
  // 32-entry list per lane only ties with the wave-per-point search, and a shuffled point list sends every lane to the list --
  // one same-address atomic per wavefront, +0.3 ms -- hence K <= 16 and the coherence test: 64 consecutive points must span
  // few cells, judged by the job's owner -- one_predict_mw from the median step between consecutive points that mik_set_points /
  // mik_set_grid recorded; the cell-sorted stations of the cross-validation job are coherent by construction)
  p.lane = p.wave_knn && h->opt_mw_knn_lane && K <= 16 && (long)h->grid.nx * h->grid.ny * h->grid.nz > 1 && J.lane && !J.live;
  if (p.solver == MW_CHOLB) {
    p.ldc = ((K + MIK_MWP - 1) / MIK_MWP) * MIK_MWP;
    p.cslot = (long)(p.ldc + MIK_MWP) * p.ldc + 3L * K;
    p.cslot += p.cslot & 1;
    const long g = std::min<long>((long)(MW_CHOLB_BYTES / (8.0 * (double)p.cslot)), 2L * h->n_cu);
    p.sgrid = (int)std::max(1L, std::min(g, chunk));
    p.sys_bytes = sizeof(double) * (size_t)p.cslot * (size_t)p.sgrid;
    p.solve_lds = sizeof(double) * 2 * MIK_MWP * MIK_MWP_LD;
  } else if (p.solver == MW_BIG) {
    const double per = 8.0 * p.nb * (p.nb + 1.0);
    const long g = std::min<long>((long)(MW_BIG_BYTES / per), 4L * h->n_cu);
    p.sgrid = (int)std::max(1L, std::min(g, chunk));
    p.sys_bytes = (size_t)per * (size_t)p.sgrid;
    p.solve_lds = sizeof(double) * 2 * (size_t)p.nb + sizeof(int) * (size_t)p.nb;
  }
  // Several value fields: a point's local system does not depend on the values, so the neighbour search and the right-hand sides run once
  // per point chunk and the fields enter only the solver -- k_mw_chol eliminates up to G - 2 of them per pass as further right-hand-side
  // rows (the arithmetic of the single value row, hence the same bits), the other solvers take one field per launch.  The planes (npt
  // doubles per field, twice over for a job in an order of its own) are bounded to ~2 GB by groups of fields; a group after the first
  // repeats the search.  Plane f leaves -- for the page-locked landing zones (plane 0 in pin_out, the others in pin_fz) or for the caller's
  // array -- as soon as its group is done.
  p.rows = chol ? mw_chol_class(h, K) / 100 - 2 : 1;
  p.fg = J.fg;
  p.ngroups = p.nf > 0 ? (p.nf + p.fg - 1) / p.fg : 1;
  return size_mw_work(h, p, J, w);
}

// the value fields on the device and, for a job that delivers to them, the landing zones in the size of this job
static int mw_stage_fields(mik_handle* h, const MwJob& J) {
  if (!J.fv) MIKC(upload_fields(h, 0));  // the caller's station order: the neighbour lists hold the caller's station indices
  if (J.landing) {
    HIPC(hipEventSynchronize(h->ev_d2h));  // an earlier predict's copies may still write the landing zones
    MIKC(h->pin_out.ensure(sizeof(double) * 2 * (size_t)J.npt));
    if (h->nf > 1) MIKC(h->pin_fz.ensure(sizeof(double) * (size_t)(h->nf - 1) * (size_t)J.npt));
  }
  return MIK_OK;
}

// what the solvers of chunk [p0, p0 + pc) are told: the problem, the chunk's lists and its place in z and sigma^2.  One value row, the
// problem's; the field loop sets Z, z and nrow per pass, mw_rhs the table of a custom variogram
static MwArgs mw_args(mik_handle* h, const MwPlan& p, const MwJob& J, long p0, long pc) {
  MwArgs a{};
  a.sx = h->xs.as<double>(), a.sy = h->ys.as<double>(), a.sz = h->zs.as<double>();
  a.mode = h->geo ? 1 : h->ndim, a.K = p.K, a.npt = (int)pc;
  a.idx = h->mw_idx.as<int>(), a.dist = h->mw_dist.as<double>();
  a.Z = h->vals.as<double>(), a.v = h->v, a.exact = h->exact, a.eps = h->eps;
  a.z = J.zs + p0, a.ss = J.sss + p0, a.flag = h->flag.as<int>();
  a.nrow = 1, a.zstride = h->N, a.pstride = p.npt;
  return a;
}

// what the searches over the station grid are told about the grid and the chunk's queries (todo: the lane pass sets it)
static KnnArgs knn_args(mik_handle* h, const MwPlan& p, const MwJob& J, long p0, long pc) {
  const auto& G = h->grid;
  KnnArgs ka{};
  ka.px = J.qx + p0, ka.py = J.qy + p0, ka.pz = p.three ? J.qz + p0 : nullptr, ka.npt = (int)pc;
  ka.gx = G.gx.as<double>(), ka.gy = G.gy.as<double>(), ka.gz = G.gz.as<double>();
  ka.orig = G.orig.as<int>(), ka.cstart = G.cstart.as<int>();
  ka.N = h->N, ka.K = p.K, ka.CAP = p.cap;
  ka.nx = G.nx, ka.ny = G.ny, ka.nz = G.nz;
  ka.x0 = G.x0, ka.y0 = G.y0, ka.z0 = G.z0;
  ka.inv_cell = 1.0 / G.cell, ka.cell2 = G.cell * G.cell, ka.tau0 = 0.0;
  if (h->opt_mw_knn_bound && !h->geo && G.live >= 2 && (long)G.nx * G.ny * G.nz > 1) {
    // radius of the disc / ball expected to hold K + 4 sqrt(K) + 2 of the ~per_cell stations a cell holds; it must stay
    // inside the 3 x 3 (x 3) cells around the point's cell
    const double m = p.K + 4.0 * std::sqrt((double)p.K) + 2.0, T = std::max(1.0, G.per_cell * J.live_frac);
    const double r2 = G.live == 3 ? std::pow(m / (4.18879020478639 * T), 2.0 / 3.0) : m / (3.14159265358979 * T);
    if (r2 <= 1.0) ka.tau0 = r2 * ka.cell2;
  }
  ka.idx_out = h->mw_idx.as<int>(), ka.dist_out = h->mw_dist.as<double>();
  if (J.self) ka.self = J.self + p0;
  ka.live = J.live;
  return ka;
}

// host code of the calls that are not hot is built for size: the library has a size bar (tests/test_abi_and_host.py)
#define MIK_SMALL __attribute__((minsize, noinline))

// the search over the station grid in NDIM dimensions, SELF: with the query's own station left out.  Small windows: one lane per point
// over the box of cells its wavefront's 64 consecutive points share (k_mw_knn_lane); the wave-per-point kernel then only walks the list
// of points that pass left unfinished
template <int NDIM, bool SELF>
static int mw_search_grid(mik_handle* h, const MwPlan& p, MwWork& w, KnnArgs ka, long pc) {
  if (p.lane) {
    ka.todo_count = w.todo.as<int>();
    ka.todo = w.todo.as<int>() + 1;
    HIPC(hipMemsetAsync(ka.todo_count, 0, sizeof(int), h->stream));
    const unsigned lgrid = (unsigned)std::min<long>((pc + 63) / 64, 64L * h->n_cu);
    hipLaunchKernelGGL((k_mw_knn_lane<NDIM, 16, SELF>), dim3(lgrid), dim3(64), 0, h->stream, ka);
  }
  const unsigned wgrid = (unsigned)std::min<long>(pc, 32L * h->n_cu);
  HIPC(hipFuncSetAttribute((const void*)k_mw_knn<NDIM, SELF>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.knn_lds));
  hipLaunchKernelGGL((k_mw_knn<NDIM, SELF>), dim3(wgrid), dim3(64), p.knn_lds, h->stream, ka);
  return MIK_OK;
}

// ... and under a pattern's mask (ka.live): the wave-per-point kernel takes every point.  The lane pass is only an accelerator and has no
// masked form in the library (its two forms did not fit under the library's size bar beside the entry point): plan_mw_job leaves
// p.lane off for a masked job
MIK_SMALL static int mw_search_live(mik_handle* h, const MwPlan& p, const KnnArgs& ka, long pc) {
  void (*const wave)(KnnArgs) = p.three ? k_mw_knn<3 + MIK_MW_LIVE, false> : k_mw_knn<2 + MIK_MW_LIVE, false>;
  HIPC(hipFuncSetAttribute((const void*)wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.knn_lds));
  hipLaunchKernelGGL(wave, dim3((unsigned)std::min<long>(pc, 32L * h->n_cu)), dim3(64), p.knn_lds, h->stream, ka);
  return MIK_OK;
}

// the K nearest stations of queries [p0, p0 + pc) into mw_idx / mw_dist: the list scan in HBM, or the searches over the station grid;
// geographic: the chord lengths the search ordered by become great-circle distances
static int mw_search(mik_handle* h, const MwPlan& p, MwWork& w, const MwJob& J, long p0, long pc) {
  int* idx = h->mw_idx.as<int>();
  double* dist = h->mw_dist.as<double>();
  if (!p.wave_knn) {
    hipLaunchKernelGGL(p.three ? k_mw_knn_big<3> : k_mw_knn_big<2>, dim3((unsigned)((pc + 255) / 256)), dim3(256), 0, h->stream, J.qx + p0,
                       J.qy + p0, p.three ? J.qz + p0 : (const double*)nullptr, (int)pc, w.sx, w.sy, p.three ? w.sz : (const double*)nullptr,
                       h->N, p.K, w.wd.as<double>(), w.wi.as<int>(), idx, dist);
  } else {
    const KnnArgs ka = knn_args(h, p, J, p0, pc);
    if (J.live) MIKC(mw_search_live(h, p, ka, pc));
    else if (p.three) MIKC((J.self ? mw_search_grid<3, true>(h, p, w, ka, pc) : mw_search_grid<3, false>(h, p, w, ka, pc)));
    else MIKC((J.self ? mw_search_grid<2, true>(h, p, w, ka, pc) : mw_search_grid<2, false>(h, p, w, ka, pc)));
  }
  if (h->geo)
    hipLaunchKernelGGL(k_mw_geo_dist, dim3((unsigned)((pc * p.K + 255) / 256)), dim3(256), 0, h->stream, J.lon + p0, J.lat + p0, pc, p.K,
                       (const double*)h->xs.as<double>(), (const double*)h->ys.as<double>(), (const int*)idx, dist);
  return MIK_OK;
}

// k_mw_rhs<model, BLOCK> over rg workgroups (BLOCK 0: points; 2 / 3: block centres in that many dimensions)
template <int BLOCK>
static void launch_mw_rhs(mik_handle* h, unsigned rg, const MwRhsArgs& ra) {
  switch (h->model) {
    case 0: hipLaunchKernelGGL((k_mw_rhs<0, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;
    case 1: hipLaunchKernelGGL((k_mw_rhs<1, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;
    case 2: hipLaunchKernelGGL((k_mw_rhs<2, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;
    case 3: hipLaunchKernelGGL((k_mw_rhs<3, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;
    case 4: hipLaunchKernelGGL((k_mw_rhs<4, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;
    default: hipLaunchKernelGGL((k_mw_rhs<5, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;
  }
}

// the right-hand sides of the chunk in place over its distances; a custom variogram also leaves the table of its pair semivariances in a
static int mw_rhs(mik_handle* h, const MwPlan& p, MwWork& w, const MwJob& J, MwArgs& a, long p0, long pc) {
  const long ne = pc * p.K;
  const unsigned rg = (unsigned)((ne + 255) / 256);
  double* dist = h->mw_dist.as<double>();
  if (p.custom) {
    // d -> gamma(d) on the host for the point-station distances and for the K x K station pairs of every point
    HIPC(hipMemcpyAsync(w.gvec.p, dist, sizeof(double) * ne, hipMemcpyDeviceToDevice, h->stream));
    MIKC(custom_roundtrip(h, w.gvec.as<double>(), pc, p.K, p.K));
    hipLaunchKernelGGL(k_mw_rhs_table, dim3(rg), dim3(256), 0, h->stream, dist, (const double*)w.gvec.as<double>(), ne, h->exact, h->eps);
    hipLaunchKernelGGL(k_mw_pairdist, dim3((unsigned)((ne * p.K + 255) / 256)), dim3(256), 0, h->stream, (const int*)a.idx, pc, p.K, a.sx,
                       a.sy, a.sz, a.mode, w.gtab.as<double>());
    MIKC(custom_roundtrip(h, w.gtab.as<double>(), pc * p.K, p.K, p.K));
    a.gtab = w.gtab.as<double>();
    return MIK_OK;
  }
  MwRhsArgs ra{};
  ra.dist = dist, ra.n = ne, ra.v = h->v, ra.exact = h->exact, ra.eps = h->eps;
  if (J.nd > 1) {  // block centres: the mean of the nodes' right-hand sides (the job's owner admits Euclidean named models only)
    ra.idx = a.idx, ra.K = p.K;
    ra.qx = J.qx + p0, ra.qy = J.qy + p0, ra.qz = p.three ? J.qz + p0 : nullptr;
    ra.sx = a.sx, ra.sy = a.sy, ra.sz = a.sz;
    ra.off = J.off, ra.nd = J.nd;
    if (h->ndim == 3) launch_mw_rhs<3>(h, rg, ra);
    else launch_mw_rhs<2>(h, rg, ra);
  } else {
    launch_mw_rhs<0>(h, rg, ra);
  }
  return MIK_OK;
}

// one solver pass over the chunk: a.nrow value rows from a.Z into a.z, sigma^2 into a.ss
static int mw_solve(mik_handle* h, const MwPlan& p, MwWork& w, const MwArgs& a, long pc) {
  const int grid = (int)std::min<long>(p.sgrid, pc);
  switch (p.solver) {
    case MW_BIG:
      if (p.solve_lds > 150 * 1024) return fail(MIK_EINVAL, "n_closest_points too large for the device path (> ~7600)");
      HIPC(hipFuncSetAttribute((const void*)k_mw_solve_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.solve_lds));
      hipLaunchKernelGGL(k_mw_solve_big, dim3(grid), dim3(256), p.solve_lds, h->stream, a, w.sysbuf.as<double>());
      return MIK_OK;
    case MW_CHOLB:
      HIPC(hipFuncSetAttribute((const void*)k_mw_chol_blocked, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.solve_lds));
      hipLaunchKernelGGL(k_mw_chol_blocked, dim3(grid), dim3(256), p.solve_lds, h->stream, a, w.sysbuf.as<double>(), p.cslot, p.ldc);
      return MIK_OK;
    case MW_CHOL: return launch_mw_chol_class(h, a, pc, mw_chol_class(h, p.K));
    default: return dispatch_mw_solve(h, a, pc);  // (always the pivoting form: valid for every window, the only one built)
  }
}

// a group's results back in the caller's order, then its gn planes (fields g0 ..) on their way to the host
static int mw_deliver(mik_handle* h, const MwPlan& p, const MwJob& J, int g0, int gn) {
  const long npt = p.npt;
  const unsigned ugrid = (unsigned)((npt + 255) / 256);
  if (p.nf == 0) {
    if (p.permuted)
      hipLaunchKernelGGL(k_ps_unsort, dim3(ugrid), dim3(256), 0, h->stream, J.perm, npt, (const double*)J.zs, (const double*)J.sss, J.z, J.ss);
    return MIK_OK;
  }
  if (p.permuted) {  // sigma^2 and the group's planes, two per launch (sigma^2 again beside an odd last plane)
    for (int q = -1; q < gn; q += 2) {
      const double* s0 = q < 0 ? J.sss : J.fs + (size_t)q * npt;
      double* d0 = q < 0 ? J.ss : J.fz + (size_t)q * npt;
      const bool pair = q + 1 < gn;
      const double* s1 = pair ? J.fs + (size_t)(q + 1) * npt : J.sss;
      double* d1 = pair ? J.fz + (size_t)(q + 1) * npt : J.ss;
      hipLaunchKernelGGL(k_ps_unsort, dim3(ugrid), dim3(256), 0, h->stream, J.perm, npt, s0, s1, d0, d1);
    }
  }
  if (J.landing) {
    // the group's planes leave for the landing zones behind the solves
    HIPC(hipEventRecord(h->evpool[1], h->stream));
    HIPC(hipStreamWaitEvent(h->stream_d2h, h->evpool[1], 0));
    for (int f = 0; f < gn; ++f) {
      const int fi = g0 + f;
      double* dst = fi == 0 ? h->pin_out.as<double>() : h->pin_fz.as<double>() + (size_t)(fi - 1) * npt;
      HIPC(hipMemcpyAsync(dst, J.fz + (size_t)f * npt, sizeof(double) * npt, hipMemcpyDeviceToHost, h->stream_d2h));
    }
    HIPC(hipEventRecord(h->ev_d2h, h->stream_d2h));
  } else {
    // ... or for the caller's planes, in stream order (the next group overwrites the device planes only behind these copies)
    if (!J.fields) HIPC(hipMemcpyAsync(J.hz + (size_t)g0 * npt, J.fz, sizeof(double) * (size_t)gn * npt, hipMemcpyDeviceToHost, h->stream));
    for (int f = 0; J.fields && f < gn; ++f)
      HIPC(hipMemcpyAsync(J.hz + (size_t)J.fields[g0 + f] * npt, J.fz + (size_t)f * npt, sizeof(double) * npt, hipMemcpyDeviceToHost, h->stream));
  }
  return MIK_OK;
}

// the singularity flag and the event times of a job whose `solves` chunk solves have been issued; waits for the stream
static int mw_read_back(mik_handle* h, const MwPlan& p, long solves, int* flag) {
  HIPC(hipMemcpyAsync(flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPC(hipEventRecord(h->evpool[1], h->stream));
  HIPC(hipStreamSynchronize(h->stream));  // also: the scoped work buffers are released only after the stream drained
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, h->evpool[0], h->evpool[1]));
  h->tm.predict_ms = ms;
  for (long c = 0; c < solves; ++c) {  // the per-point solves (the dominant kernel of this path) on their own
    HIPC(hipEventElapsedTime(&ms, h->evpool[2 + 2 * c], h->evpool[3 + 2 * c]));
    h->tm.contract_ms += ms;
  }
  h->tm.contract_launches = solves;
  h->tm.mw_kernel = p.solver;
  h->tm.rhs_ms = h->tm.predict_ms - h->tm.contract_ms;  // neighbour search + right-hand sides
  return MIK_OK;
}

// (the caller has recorded evpool[0] on the stream and built the station grid if the search runs in LDS)
static int run_mw_job(mik_handle* h, int K, const MwJob& J) {
  reset_predict_timing(h);
  MwPlan p;
  MwWork w;
  MIKC(plan_mw_job(h, K, J, p, w));
  if (p.nf > 0) MIKC(mw_stage_fields(h, J));
  MIKC(get_events(h, 2 + 2 * (size_t)p.ngroups * (size_t)p.nchunks));
  const double* fv = J.fv ? J.fv : h->fv.as<double>();
  long solves = 0;
  for (int g0 = 0; g0 < std::max(p.nf, 1); g0 += p.fg) {
    const int gn = p.nf > 0 ? std::min(p.fg, p.nf - g0) : 0;  // fields of this group
    double* zpl = p.permuted ? J.fs : J.fz;
    if (g0 > 0 && J.landing) HIPC(hipStreamWaitEvent(h->stream, h->ev_d2h, 0));  // the previous group's planes have left
    for (long p0 = 0; p0 < p.npt; p0 += p.chunk) {
      const long pc = std::min(p.chunk, p.npt - p0);
      MIKC(mw_search(h, p, w, J, p0, pc));
      MwArgs a = mw_args(h, p, J, p0, pc);
      MIKC(mw_rhs(h, p, w, J, a, p0, pc));
      HIPC(hipEventRecord(h->evpool[2 + 2 * solves], h->stream));
      if (p.nf == 0) MIKC(mw_solve(h, p, w, a, pc));
      for (int f = 0; f < gn; f += p.rows) {  // field g0 + f .. in the rows of one pass
        a.nrow = std::min(p.rows, gn - f);
        a.Z = fv + (size_t)(g0 + f) * (size_t)h->N;
        a.z = zpl + (size_t)f * (size_t)p.npt + p0;
        MIKC(mw_solve(h, p, w, a, pc));
      }
      HIPC(hipEventRecord(h->evpool[3 + 2 * solves], h->stream));
      ++solves;
      HIPC(hipGetLastError());
    }
    MIKC(mw_deliver(h, p, J, g0, gn));
  }
  int flag = 0;
  MIKC(mw_read_back(h, p, solves, &flag));
  if ((flag & 2) && !p.mw_piv) {  // a local system was not positive definite after the shift: redo with partial pivoting
    HIPC(hipEventRecord(h->evpool[0], h->stream));
    h->mw_force_piv = true;
    const int rc = run_mw_job(h, K, J);
    h->mw_force_piv = false;
    return rc;
  }
  if (flag) return fail(MIK_ESINGULAR, "Singular matrix");  // cok.pyx:176-177
  return MIK_OK;
}

// Small windows over a point list in no spatial order (round 4, second session): the lane-per-point search needs 64
// consecutive points to share a few cells of the station grid.  The points are then put in Hilbert-curve order on the device
// (k_ps_*: the sorter of the range-aware contraction), searched and solved in that order -- coordinates gathered once, z and
// sigma^2 scattered back at the end -- so a shuffled list costs what the rows of a grid cost.  Decides whether this job is such a
// one (*sorted) and, if so, sorts: J's queries, results and perm are then the sorted ones.  (The station grid is built.)
static int mw_sort_points(mik_handle* h, int K, MwJob& J, bool* sorted) {
  const long npt = h->npt;
  *sorted = false;
  const bool cells = (long)h->grid.nx * h->grid.ny * h->grid.nz > 1;
  const bool coherent = h->pts_step >= 0.0 && 64.0 * h->pts_step <= 10.0 * h->grid.cell;
  if (!(h->opt_mw_knn_lane && h->opt_sort_points != 0 && K <= 16 && cells && !h->geo && h->model != MIK_MODEL_CUSTOM && !coherent &&
        h->pts_extent > 0.0 && npt >= 4096))
    return MIK_OK;
  const double spacing = h->pts_extent / std::pow((double)npt, 1.0 / h->ndim);  // of a sorted list: a wavefront's 64 points are a patch
  if (!(12.0 * spacing <= 10.0 * h->grid.cell)) return MIK_OK;                    // ~8 spacings across
  // (segments of 131 072 points like the contraction's launches: the bounding box and the scan of a segment are ONE workgroup
  // each -- a single 2^20-point segment spent 0.53 + 2 x 0.39 ms in them, eight segments side by side 0.2 ms in all)
  const long schunk = std::min<long>(((npt + 127) / 128) * 128, 131072L);
  if (!(h->ps_valid && h->ps_chunk == schunk)) MIKC(sort_points(h, schunk, (npt + schunk - 1) / schunk));
  const size_t nbp = sizeof(double) * (size_t)npt;
  MIKC(h->ps_x.ensure(nbp));
  MIKC(h->ps_y.ensure(nbp));
  if (h->ndim == 3) MIKC(h->ps_z.ensure(nbp));
  MIKC(h->ps_zs.ensure(nbp));
  MIKC(h->ps_sss.ensure(nbp));
  hipLaunchKernelGGL(k_ps_gather, dim3((unsigned)((npt + 255) / 256)), dim3(256), 0, h->stream, (const unsigned*)h->ps_idx[0].as<unsigned>(),
                     npt, J.qx, J.qy, h->ndim == 3 ? J.qz : (const double*)nullptr, h->ps_x.as<double>(), h->ps_y.as<double>(),
                     h->ndim == 3 ? h->ps_z.as<double>() : (double*)nullptr);
  J.qx = h->ps_x.as<double>(), J.qy = h->ps_y.as<double>();
  if (h->ndim == 3) J.qz = h->ps_z.as<double>();
  J.zs = h->ps_zs.as<double>(), J.sss = h->ps_sss.as<double>();
  J.perm = (const unsigned*)h->ps_idx[0].as<unsigned>();
  *sorted = true;
  return MIK_OK;
}

// blocks: sigma^2_V = (-lam . bbar - mu) - gbar: once, behind the job -- a redo with pivoting re-enters run_mw_job and must not subtract
// twice.  Waits for the stream: the result copies run on another one, and the caller's offsets and gbar go out of scope.
static int mw_block_epilogue(mik_handle* h, const MwJob& J, double* gbar) {
  HIPC(hipEventRecord(h->evpool[0], h->stream));
  MIKC(launch_block_gamma(h, J.off, J.nd, gbar));
  MIKC(launch_block_ss(h, J.ss, J.npt, gbar));
  HIPC(hipEventRecord(h->evpool[1], h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, h->evpool[0], h->evpool[1]));
  h->tm.predict_ms += ms;
  h->tm.rhs_ms += ms;  // (everything of the call that is not a solve)
  return MIK_OK;
}

// Fields with gaps through the window (mik_predict_window_gaps): what the caller handed over, and the loop over patterns around the job.
struct MwGaps {
  const uint8_t* valid;  // nf x N in the caller's station order, 1 = measured; nullptr = no gaps
  double *z_out, *ss_out;  // nf x npt each, caller's memory
};

// Fields with the same valid column form a pattern; patterns in order of first appearance, each with its fields in order.  A pattern shares
// one search, one set of right-hand sides and one sigma^2: run_mw_job once per pattern over that pattern's value rows (J.fv: the rows of
// the pattern side by side, so its fields take the solver's row groups as the fields of mik_predict_moving_window do), with the byte mask of
// the pattern in the grid's station order (J.live; a pattern without a gap has none and runs the unmasked searches).  The redo with pivoting
// happens inside run_mw_job: it redoes that one pattern.  Times are summed over the patterns.  (J is the job of the resident points as
// predict_mw_body set it up: queries, order, planes of J.fg fields.)
MIK_SMALL static int run_mw_gaps(mik_handle* h, int K, MwJob J, const MwGaps& gp) {
  auto copy = [](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDefault); };
  const size_t N = (size_t)h->N, npt = (size_t)J.npt;
  const int nf = std::max(h->nf, 1);
  std::vector<int> iw(2 * (size_t)nf + (gp.valid ? N : 0));
  int *pat = iw.data(), *fl = pat + nf, *orig = fl + nf;  // field -> pattern; the first fields while grouping, then a pattern's fields; G.orig
  int npat = 0;
  for (int f = 0; f < nf; ++f) {
    int q = 0;
    while (gp.valid && q < npat && memcmp(gp.valid + f * N, gp.valid + fl[q] * N, N)) ++q;
    if (q == npat) fl[npat++] = f;
    pat[f] = q;
  }
  DevBuf rows, live;
  std::vector<unsigned char> lv(gp.valid ? N : 0);
  if (h->nf > 0) MIKC(rows.ensure(sizeof(double) * nf * N));
  if (gp.valid) {
    MIKC(live.ensure(N));
    HIPC(copy(orig, h->grid.orig.p, sizeof(int) * N));
  }
  J.landing = false;
  J.hz = gp.z_out;
  J.fields = fl;
  double ms[3] = {0.0, 0.0, 0.0};
  long launches = 0;
  for (int q = 0, r0 = 0; q < npat; ++q, r0 += J.nfl) {
    J.nfl = 0;
    for (int f = 0; f < nf; ++f)
      if (pat[f] == q) fl[J.nfl++] = f;
    // the pattern's value rows side by side, and its byte mask in the grid's station order
    J.fv = h->nf > 0 ? rows.as<double>() + r0 * N : h->vals.as<double>();
    for (int i = 0; h->nf > 0 && i < J.nfl; ++i)
      HIPC(copy(const_cast<double*>(J.fv) + i * N, &h->hfields[fl[i] * N], sizeof(double) * N));
    size_t have = N;
    if (gp.valid) {
      const uint8_t* col = gp.valid + fl[0] * N;
      have = 0;
      for (size_t j = 0; j < N; ++j) have += (lv[j] = col[orig[j]] != 0);
    }
    J.live = nullptr, J.live_frac = 1.0;
    if (have < N) {
      HIPC(copy(live.p, lv.data(), N));
      J.live = live.as<unsigned char>(), J.live_frac = (double)have / (double)N;
    }
    HIPC(hipEventRecord(h->evpool[0], h->stream));
    MIKC(run_mw_job(h, K, J));
    double* ss0 = gp.ss_out + fl[0] * npt;
    HIPC(copy(ss0, J.ss, sizeof(double) * npt));
    for (int i = 1; i < J.nfl; ++i) memcpy(gp.ss_out + fl[i] * npt, ss0, sizeof(double) * npt);
    ms[0] += h->tm.rhs_ms, ms[1] += h->tm.contract_ms, ms[2] += h->tm.predict_ms, launches += h->tm.contract_launches;
  }
  h->tm.rhs_ms = ms[0], h->tm.contract_ms = ms[1], h->tm.predict_ms = ms[2], h->tm.contract_launches = launches;
  return MIK_OK;
}

// The moving window over the resident points: mik_predict_moving_window (nd = 0) and mik_predict_block_window (the points are block
// centres, offsets the nd x ndim adjusted node offsets on the host).  nd = 1 is a block of one node at its centre: the point form.
// gaps (mik_predict_window_gaps): the same job once per pattern, results to the caller's planes instead of the landing zones.
// The entry points have made the refusals (one_predict_mw, one_predict_window_gaps; mik_predict_block_window, mikrige.hip).
static int predict_mw_body(mik_handle* h, int K, const double* offsets, int nd, const MwGaps* gaps = nullptr) {
  HIPC(hipSetDevice(h->device));
  MIKC(get_events(h, 2));
  const long npt = h->npt;
  const int nf = gaps ? std::max(h->nf, 1) : h->nf;
  reset_predict_timing(h);
  h->nf_done = 0;
  if (gaps) h->have_results = false;  // z / ss on the device become the last pattern's; nothing reaches the landing zones
  if (npt == 0 && gaps) return MIK_OK;
  if (npt == 0) {
    h->have_results = true;
    h->nf_done = nf;
    return MIK_OK;
  }
  HIPC(hipStreamWaitEvent(h->stream, h->ev_d2h, 0));
  HIPC(hipEventRecord(h->evpool[0], h->stream));
  MwJob J;
  J.npt = npt;
  J.qx = h->px.as<double>(), J.qy = h->py.as<double>(), J.qz = h->pz.as<double>();
  J.lon = h->px.as<double>(), J.lat = h->py.as<double>();
  DevBuf pu, splanes;
  if (h->geo) {
    // neighbours by chord length on the unit sphere (same ordering as great-circle), distances recomputed below
    MIKC(pu.ensure(sizeof(double) * 3 * (size_t)npt));
    double* p3 = pu.as<double>();
    hipLaunchKernelGGL(k_geo_unit, dim3((unsigned)((npt + 255) / 256)), dim3(256), 0, h->stream, J.qx, J.qy, (int)npt, p3,
                       p3 + npt, p3 + 2 * (size_t)npt);
    J.qx = p3, J.qy = p3 + npt, J.qz = p3 + 2 * (size_t)npt;
  }
  bool mw_sorted = false;
  J.zs = J.z = h->z.as<double>(), J.sss = J.ss = h->ss.as<double>();
  if (mw_knn_cap(K) <= h->opt_mw_lds_cap) {
    MIKC(build_mw_grid(h, std::max(8, std::min(K, 256))));
    MIKC(mw_sort_points(h, K, J, &mw_sorted));
    J.lane = mw_sorted || (h->pts_step >= 0.0 && 64.0 * h->pts_step * (h->geo ? MIK_PI / 180.0 : 1.0) <= 10.0 * h->grid.cell);
  }
  if (nf > 0) {
    J.fg = mw_field_group(nf, npt, mw_sorted);
    MIKC(h->zf.ensure(sizeof(double) * (size_t)J.fg * (size_t)npt));
    J.fz = h->zf.as<double>();
    if (mw_sorted) {
      MIKC(splanes.ensure(sizeof(double) * (size_t)J.fg * (size_t)npt));
      J.fs = splanes.as<double>();
    }
  }
  h->tm.points_sorted = mw_sorted ? 1 : 0;
  DevBuf blk;  // blocks: the node offsets and, behind them, gbar -- this call's
  if (nd > 1) {
    const size_t noff = (size_t)nd * (size_t)h->ndim;
    MIKC(blk.ensure(sizeof(double) * (noff + 1)));
    HIPC(hipMemcpy(blk.p, offsets, sizeof(double) * noff, hipMemcpyHostToDevice));
    J.off = blk.as<double>(), J.nd = nd;
  }
  if (gaps) return run_mw_gaps(h, K, J, *gaps);
  MIKC(run_mw_job(h, K, J));
  if (nd > 1) MIKC(mw_block_epilogue(h, J, blk.as<double>() + (size_t)nd * (size_t)h->ndim));
  MIKC(h->pin_out.ensure(sizeof(double) * 2 * (size_t)npt));
  if (nf == 0) HIPC(hipMemcpyAsync(h->pin_out.as<double>(), h->z.p, sizeof(double) * npt, hipMemcpyDeviceToHost, h->stream_d2h));
  HIPC(hipMemcpyAsync(h->pin_out.as<double>() + npt, h->ss.p, sizeof(double) * npt, hipMemcpyDeviceToHost, h->stream_d2h));
  HIPC(hipEventRecord(h->ev_d2h, h->stream_d2h));
  h->have_results = true;
  h->nf_done = nf;
  return MIK_OK;
}

int one_predict_mw(mik_handle* h, int n_closest) {
  if (!h || !h->have_problem) return fail(MIK_ESTATE, "mik_predict_moving_window: set the problem first");
  if (!h->have_points) return fail(MIK_ESTATE, "mik_predict_moving_window: set points first");
  MIKC(window_refusals(h, n_closest, true));
  return predict_mw_body(h, n_closest, nullptr, 0);
}

int one_predict_block_mw(mik_handle* h, const double* offsets, int nd, int n_closest) { return predict_mw_body(h, n_closest, offsets, nd); }

// mik_predict_window_gaps: the refusals that need the window -- all before anything is launched -- then the job per pattern
MIK_SMALL int one_predict_window_gaps(mik_handle* h, int K, const uint8_t* valid, double* z_out, double* ss_out) {
  MIKC(window_refusals(h, K, true));
  char msg[200];
  if (mw_knn_cap(K) > h->opt_mw_lds_cap) {
    snprintf(msg, sizeof msg, "mik_predict_window_gaps: a window of %d stations is beyond the neighbour search in LDS (\"mw_lds_cap\" %d: n_closest_points <= %d)",
             K, h->opt_mw_lds_cap, h->opt_mw_lds_cap - 256);
    return fail(MIK_EINVAL, msg);
  }
  for (int f = 0; valid && f < std::max(h->nf, 1); ++f) {
    long have = 0;
    for (long i = 0; i < h->N; ++i) have += valid[(size_t)f * h->N + i] != 0;
    if (have < K) {
      snprintf(msg, sizeof msg, "mik_predict_window_gaps: field %d has %ld valid stations, fewer than n_closest_points = %d", f, have, K);
      return fail(MIK_EINVAL, msg);
    }
  }
  const MwGaps gp{valid, z_out, ss_out};
  return predict_mw_body(h, K, nullptr, 0, &gp);
}

// Windowed leave-one-out cross-validation (mik_cross_validate_window): the job is the stations themselves, in the cell-sorted order the
// search grid already holds them in (G.gx / gy / gz, G.orig) -- 64 consecutive queries share a few cells by construction, so the lane
// search applies for K <= 16 on any grid of more than one cell, without a point sort.  Query t is station orig[t] and stays out of its own
// window by index (KnnArgs::self).  Results land in buffers of this call (cvw) and are scattered back through orig (k_ps_unsort); the
// resident points, h->z / h->ss, the landing zones, have_results and a resident factor are not touched.
int one_cross_validate_window(mik_handle* h, int n_closest, double* zhat_out, double* ss_out) {
  MIKC(window_refusals(h, n_closest, false));  // (every station but the query: the bound on the window is this function's)
  const long N = h->N;
  const int K = n_closest;
  if (K > N - 1)
    return fail(MIK_EINVAL, "mik_cross_validate_window: n_closest_points = " + std::to_string(K) + " exceeds the number of OTHER stations (" +
                                std::to_string(N - 1) + ")");
  if (mw_knn_cap(K) > h->opt_mw_lds_cap)
    return fail(MIK_EINVAL, "mik_cross_validate_window: a window of " + std::to_string(K) + " stations is beyond the neighbour search in LDS (\"mw_lds_cap\" " +
                                std::to_string(h->opt_mw_lds_cap) + " candidates: n_closest_points <= " + std::to_string(h->opt_mw_lds_cap - 256) +
                                "); at that window size the global form, mik_cross_validate, is the tool");
  HIPC(hipSetDevice(h->device));
  MIKC(get_events(h, 2));
  const int nf = h->nf;
  HIPC(hipStreamWaitEvent(h->stream, h->ev_d2h, 0));
  HIPC(hipEventRecord(h->evpool[0], h->stream));
  MIKC(build_mw_grid(h, std::max(8, std::min(K, 256))));
  const auto& G = h->grid;
  MwJob J;
  J.npt = N;
  J.qx = G.gx.as<double>(), J.qy = G.gy.as<double>(), J.qz = G.gz.as<double>();
  J.self = G.orig.as<int>();
  J.perm = (const unsigned*)G.orig.as<unsigned>();  // (station indices: non-negative)
  J.lane = true;
  J.landing = false;
  J.hz = zhat_out;
  if (nf > 0) J.fg = mw_field_group(nf, N, true);
  // one buffer of this call: z, sigma^2 in job order and in the caller's order | geographic: lon, lat of the queries | the field planes twice
  const size_t n = (size_t)N, planes = 4 + (h->geo ? 2 : 0) + (nf > 0 ? 2 * (size_t)J.fg : 0);
  MIKC(h->cvw.ensure(sizeof(double) * planes * n));
  double* w = h->cvw.as<double>();
  J.zs = w, J.sss = w + n, J.z = w + 2 * n, J.ss = w + 3 * n;
  w += 4 * n;
  if (h->geo) {  // the queries' lon / lat for the great-circle distances, gathered once
    hipLaunchKernelGGL(k_ps_gather, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, J.perm, N, (const double*)h->xs.as<double>(),
                       (const double*)h->ys.as<double>(), (const double*)nullptr, w, w + n, (double*)nullptr);
    J.lon = w, J.lat = w + n;
    w += 2 * n;
  }
  if (nf > 0) J.fs = w, J.fz = w + (size_t)J.fg * n;
  MIKC(run_mw_job(h, K, J));
  if (nf == 0) HIPC(hipMemcpyAsync(zhat_out, J.z, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipMemcpyAsync(ss_out, J.ss, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return MIK_OK;
}
