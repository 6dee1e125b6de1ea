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

// candidate buffer of the wave-per-point neighbour search: a power of two >= K + 256 (beyond "mw_lds_cap" the lists live in HBM)
static int mw_knn_cap(int K) {
  int cap = 512;
  while (cap < K + 256) cap <<= 1;
  return cap;
}
// value fields per group: the planes (npt doubles per field, twice over where the job runs in an order of its own) are bounded to ~2 GB
static int mw_field_group(int nf, long npt, bool permuted) {
  const long per = (long)(2e9 / (8.0 * (double)npt * (permuted ? 2.0 : 1.0)));
  return (int)std::max(1L, std::min<long>(nf, per));
}

// One moving-window job: a list of queries, each kriged from its K nearest stations.  mik_predict_moving_window's job is the resident
// points; mik_cross_validate_window's is the stations themselves in the cell-sorted order of the search grid, each left out of its own
// window (self).  run_mw_job is the chunk loop both share: search, right-hand sides, solver choice, field groups, the redo with
// pivoting and the singular-matrix answer.
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
};

// k_mw_rhs<model, BLOCK> over rg workgroups (BLOCK 0: points; 2 / 3: block centres in that many dimensions)
#define MW_RHS(BLOCK, rg, ra)                                                                                  \
  switch (h->model) {                                                                                          \
    case 0: hipLaunchKernelGGL((k_mw_rhs<0, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;            \
    case 1: hipLaunchKernelGGL((k_mw_rhs<1, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;            \
    case 2: hipLaunchKernelGGL((k_mw_rhs<2, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;            \
    case 3: hipLaunchKernelGGL((k_mw_rhs<3, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;            \
    case 4: hipLaunchKernelGGL((k_mw_rhs<4, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;            \
    default: hipLaunchKernelGGL((k_mw_rhs<5, BLOCK>), dim3(rg), dim3(256), 0, h->stream, ra); break;           \
  }

// (the caller has recorded evpool[0] on the stream and built the station grid if the search runs in LDS)
static int run_mw_job(mik_handle* h, int K, const MwJob& J) {
  const long npt = J.npt;
  const int nf = h->nf;  // value fields (mik_set_fields); 0 = the problem's values
  long solve_chunks = 0;
  h->tm.rhs_ms = h->tm.contract_ms = h->tm.predict_ms = 0.0;
  h->tm.contract_launches = 0;
  h->tm.contract_flops_executed = 0.0;
  // The reference cuts each point's system out of a_all = self._get_kriging_matrix(n); here its entries are computed
  // from the selected stations' coordinates, so no N x N matrix exists on this path (and a factor held by the handle
  // stays valid).
  // K <= MIK_MW_KMAX: candidate lists in registers, systems in LDS, all points in one pass.  Larger K: working sets in
  // HBM, points in chunks that bound those work arrays to ~2 GB.
  const int nb = K + 1;
  const bool custom = h->model == MIK_MODEL_CUSTOM;
  // small windows are solved without a pivot search on the SPD-shifted local system unless the model cannot promise a
  // positive definite station block (hole-effect), has no device functor for the shift (custom), or a previous attempt
  // of this call hit a bad pivot
  const bool mw_piv = custom || h->model == MIK_MODEL_HOLE_EFFECT || h->mw_force_piv || h->opt_mw_pivot;
  // three solvers: LDL^T of the shifted system in registers (no pivot search; windows up to 256), Gauss-Jordan in registers
  // with implicit partial pivoting (when the model cannot promise a positive definite
  // station block; windows up to 127), LU with partial pivoting in HBM scratch (any window)
  const bool chol = !mw_piv && K <= MIK_MW_CHOL_KMAX && h->opt_mw_class != 1;
  // beyond the register classes: blocked Cholesky of the shifted system (one block per point, panels of 64 in LDS, the matrix
  // in an L2-resident scratch slot); "mw_class" 1 forces it for smaller windows too (A/B runs)
  const bool cholb = !mw_piv && !chol && K >= 8;
  const bool big = !chol && !cholb && K > MIK_MW_KMAX;
  long chunk = npt;
  if (K > MIK_MW_KMAX) {  // neighbour lists of 12 K bytes per point: bound them to ~2 GB
    chunk = ((long)(2e9 / (24.0 * K)) / 256) * 256;
    if (chunk < 256) chunk = 256;
    if (chunk > npt) chunk = npt;
  }
  if (custom) {  // the K x K pair distances of every point visit the host: bound that table to ~1 GB
    long cc = ((long)(1e9 / (8.0 * K * (K + 1.0))) / 256) * 256;
    if (cc < 256) cc = 256;
    if (chunk > cc) chunk = cc;
    if (chunk > npt) chunk = npt;
  }
  MIKC(h->mw_idx.ensure(sizeof(int) * (size_t)chunk * K));
  MIKC(h->mw_dist.ensure(sizeof(double) * (size_t)chunk * K));
  MIKC(h->flag.ensure(sizeof(int)));
  HIPC(hipMemsetAsync(h->flag.p, 0, sizeof(int), h->stream));
  DevBuf su, wd, wi, sysbuf, gtab, gvec, todo;
  if (custom) {
    MIKC(gtab.ensure(sizeof(double) * (size_t)chunk * K * K));
    MIKC(gvec.ensure(sizeof(double) * (size_t)chunk * K));
  }
  const double *sx = h->xs.as<double>(), *sy = h->ys.as<double>(), *sz = h->zs.as<double>();
  const double *qx = J.qx, *qy = J.qy, *qz = J.qz;
  const bool three = h->geo || h->ndim == 3;
  int sgrid = 0;
  const int cap = mw_knn_cap(K);
  const bool wave_knn = cap <= h->opt_mw_lds_cap;  // default 8192 = 96 KB of LDS; beyond that the lists live in HBM
  const bool permuted = J.perm != nullptr;
  if (!wave_knn) {
    if (J.self) return fail(MIK_EINVAL, "moving window: the list search in HBM leaves no station out");  // (mik_cross_validate_window refuses such a K)
    MIKC(wd.ensure(sizeof(double) * (size_t)chunk * K));
    MIKC(wi.ensure(sizeof(int) * (size_t)chunk * K));
    if (h->geo) {  // station unit vectors for the plain scan
      MIKC(su.ensure(sizeof(double) * 3 * (size_t)h->N));
      double* s3 = su.as<double>();
      hipLaunchKernelGGL(k_geo_unit, dim3((h->N + 255) / 256), dim3(256), 0, h->stream, sx, sy, h->N, s3, s3 + h->N,
                         s3 + 2 * (size_t)h->N);
      sx = s3, sy = s3 + h->N, sz = s3 + 2 * (size_t)h->N;
    }
  }
  int ldc = 0;
  long cslot = 0;
  if (cholb) {
    ldc = ((K + MIK_MWP - 1) / MIK_MWP) * MIK_MWP;
    cslot = (long)(ldc + MIK_MWP) * ldc + 3L * K;
    cslot += cslot & 1;
    long g = (long)(6e9 / (8.0 * (double)cslot));  // per-block scratch systems, <= ~6 GB in total
    if (g > 2L * h->n_cu) g = 2L * h->n_cu;
    if (g > chunk) g = chunk;
    if (g < 1) g = 1;
    sgrid = (int)g;
    MIKC(sysbuf.ensure(sizeof(double) * (size_t)cslot * (size_t)sgrid));
  }
  if (big) {
    const double per = 8.0 * nb * (nb + 1.0);
    long g = (long)(4e9 / per);  // per-block scratch systems, <= ~4 GB in total
    if (g > 4L * h->n_cu) g = 4L * h->n_cu;
    if (g > chunk) g = chunk;
    if (g < 1) g = 1;
    sgrid = (int)g;
    MIKC(sysbuf.ensure((size_t)per * (size_t)sgrid));
  }
  // Several value fields: a point's local system does not depend on the values, so the neighbour search and the right-hand sides run once
  // per point chunk and the fields enter only the solver -- k_mw_chol eliminates up to G - 2 of them per pass as further right-hand-side
  // rows (the arithmetic of the single value row, hence the same bits), the other solvers take one field per launch.  The planes (npt
  // doubles per field, twice over for a job in an order of its own) are bounded to ~2 GB by groups of fields; a group after the first
  // repeats the search.  Plane f leaves -- for the page-locked landing zones (plane 0 in pin_out, the others in pin_fz) or for the caller's
  // array -- as soon as its group is done.
  int rows = 1;  // value rows per solver pass
  if (chol) rows = mw_chol_class(h, K) / 100 - 2;
  const int fg = J.fg;
  const double* fv = nullptr;
  if (nf > 0) {
    MIKC(upload_fields(h, 0));  // the caller's station order: the neighbour lists hold the caller's station indices
    fv = h->fv.as<double>();
    if (J.landing) {
      HIPC(hipEventSynchronize(h->ev_d2h));  // an earlier predict's copies may still write the landing zones
      MIKC(h->pin_out.ensure(sizeof(double) * 2 * (size_t)npt));
      if (nf > 1) MIKC(h->pin_fz.ensure(sizeof(double) * (size_t)(nf - 1) * (size_t)npt));
    }
  }
  auto solve = [&](const MwArgs& a, long pc) -> int {
    if (big) {
      const size_t lds = sizeof(double) * 2 * (size_t)nb + sizeof(int) * (size_t)nb;
      if (lds > 150 * 1024) return fail(MIK_EINVAL, "n_closest_points too large for the device path (> ~7600)");
      const int grid = (int)(pc < sgrid ? pc : sgrid);
      HIPC(hipFuncSetAttribute((const void*)k_mw_solve_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(k_mw_solve_big, dim3(grid), dim3(256), lds, h->stream, a, sysbuf.as<double>());
    } else if (cholb) {
      const size_t lds = sizeof(double) * 2 * MIK_MWP * MIK_MWP_LD;
      const int grid = (int)std::min<long>(sgrid, pc);
      HIPC(hipFuncSetAttribute((const void*)k_mw_chol_blocked, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(k_mw_chol_blocked, dim3(grid), dim3(256), lds, h->stream, a, sysbuf.as<double>(), cslot, ldc);
    } else if (chol) {
      MIKC(launch_mw_chol_class(h, a, pc, mw_chol_class(h, K)));
    } else {
      MIKC(dispatch_mw_solve(h, a, pc));  // (always the pivoting form: valid for every window, the only one built)
    }
    return MIK_OK;
  };
  const int ngroups = nf > 0 ? (nf + fg - 1) / fg : 1;
  MIKC(get_events(h, 2 + 2 * (size_t)ngroups * (size_t)((npt + chunk - 1) / chunk)));
  for (int g0 = 0; g0 < std::max(nf, 1); g0 += fg) {
    const int gn = nf > 0 ? std::min(fg, nf - g0) : 0;  // fields of this group
    double* zpl = nf > 0 ? (permuted ? J.fs : J.fz) : nullptr;
    if (g0 > 0 && J.landing) HIPC(hipStreamWaitEvent(h->stream, h->ev_d2h, 0));  // the previous group's planes have left
    for (long p0 = 0; p0 < npt; p0 += chunk) {
      const long pc = (npt - p0 < chunk) ? npt - p0 : chunk;
      const unsigned kgrid = (unsigned)((pc + 255) / 256);
      int* idx = h->mw_idx.as<int>();
      double* dist = h->mw_dist.as<double>();
      if (!wave_knn) {
        if (three)
          hipLaunchKernelGGL(k_mw_knn_big<3>, dim3(kgrid), dim3(256), 0, h->stream, qx + p0, qy + p0, qz + p0, (int)pc, sx, sy, sz,
                             h->N, K, wd.as<double>(), wi.as<int>(), idx, dist);
        else
          hipLaunchKernelGGL(k_mw_knn_big<2>, dim3(kgrid), dim3(256), 0, h->stream, qx + p0, qy + p0, (const double*)nullptr,
                             (int)pc, sx, sy, (const double*)nullptr, h->N, K, wd.as<double>(), wi.as<int>(), idx, dist);
      } else {
        const long wg = 32L * h->n_cu;
        const unsigned wgrid = (unsigned)(pc < wg ? pc : wg);
        const size_t klds = (size_t)cap * (sizeof(double) + sizeof(int));
        KnnArgs ka{};
        ka.px = qx + p0;
        ka.py = qy + p0;
        ka.pz = three ? qz + p0 : nullptr;
        ka.npt = (int)pc;
        ka.gx = h->grid.gx.as<double>();
        ka.gy = h->grid.gy.as<double>();
        ka.gz = h->grid.gz.as<double>();
        ka.orig = h->grid.orig.as<int>();
        ka.cstart = h->grid.cstart.as<int>();
        ka.N = h->N, ka.K = K, ka.CAP = cap;
        ka.nx = h->grid.nx, ka.ny = h->grid.ny, ka.nz = h->grid.nz;
        ka.x0 = h->grid.x0, ka.y0 = h->grid.y0, ka.z0 = h->grid.z0;
        ka.inv_cell = 1.0 / h->grid.cell;
        ka.cell2 = h->grid.cell * h->grid.cell;
        ka.tau0 = 0.0;
        if (h->opt_mw_knn_bound && !h->geo && h->grid.live >= 2 && (long)h->grid.nx * h->grid.ny * h->grid.nz > 1) {
          // radius of the disc / ball expected to hold K + 4 sqrt(K) + 2 of the ~per_cell stations a cell holds; it must stay
          // inside the 3 x 3 (x 3) cells around the point's cell
          const double m = K + 4.0 * std::sqrt((double)K) + 2.0, T = std::max(1.0, h->grid.per_cell);
          const double r2 = h->grid.live == 3 ? std::pow(m / (4.18879020478639 * T), 2.0 / 3.0) : m / (3.14159265358979 * T);
          if (r2 <= 1.0) ka.tau0 = r2 * ka.cell2;
        }
        ka.idx_out = idx;
        ka.dist_out = dist;
        const bool self = J.self != nullptr;
        if (self) ka.self = J.self + p0;
        // (measured, profiles/r04_mw_knn_ab.txt: rows of a grid, k = 10: search + rhs 2.65 -> 0.62 ms per 1e6 points, bit-identical; a
        // 32-entry list per lane only ties with the wave-per-point search, and a shuffled point list sends every lane to the list --
        // one same-address atomic per wavefront, +0.3 ms -- hence K <= 16 and the coherence test: 64 consecutive points must span
        // few cells, judged by the job's owner -- one_predict_mw from the median step between consecutive points that mik_set_points /
        // mik_set_grid recorded; the cell-sorted stations of the cross-validation job are coherent by construction)
        if (h->opt_mw_knn_lane && K <= 16 && (long)h->grid.nx * h->grid.ny * h->grid.nz > 1 && J.lane) {
          // small windows: one lane per point over the box of cells its wavefront's 64 consecutive points share (k_mw_knn_lane); the
          // wave-per-point kernel below then only walks the list of points that pass left unfinished
          MIKC(todo.ensure(sizeof(int) * ((size_t)pc + 1)));
          ka.todo_count = todo.as<int>();
          ka.todo = todo.as<int>() + 1;
          HIPC(hipMemsetAsync(ka.todo_count, 0, sizeof(int), h->stream));
          const unsigned lgrid = (unsigned)std::min<long>((pc + 63) / 64, 64L * h->n_cu);
          if (self) {
            if (three) hipLaunchKernelGGL((k_mw_knn_lane<3, 16, true>), dim3(lgrid), dim3(64), 0, h->stream, ka);
            else hipLaunchKernelGGL((k_mw_knn_lane<2, 16, true>), dim3(lgrid), dim3(64), 0, h->stream, ka);
          } else {
            if (three) hipLaunchKernelGGL((k_mw_knn_lane<3, 16, false>), dim3(lgrid), dim3(64), 0, h->stream, ka);
            else hipLaunchKernelGGL((k_mw_knn_lane<2, 16, false>), dim3(lgrid), dim3(64), 0, h->stream, ka);
          }
        }
        const void* kfn = three ? (self ? (const void*)k_mw_knn<3, true> : (const void*)k_mw_knn<3, false>)
                                : (self ? (const void*)k_mw_knn<2, true> : (const void*)k_mw_knn<2, false>);
        HIPC(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)klds));
        if (three) {
          if (self) hipLaunchKernelGGL((k_mw_knn<3, true>), dim3(wgrid), dim3(64), klds, h->stream, ka);
          else hipLaunchKernelGGL((k_mw_knn<3, false>), dim3(wgrid), dim3(64), klds, h->stream, ka);
        } else {
          if (self) hipLaunchKernelGGL((k_mw_knn<2, true>), dim3(wgrid), dim3(64), klds, h->stream, ka);
          else hipLaunchKernelGGL((k_mw_knn<2, false>), dim3(wgrid), dim3(64), klds, h->stream, ka);
        }
      }
      if (h->geo)
        hipLaunchKernelGGL(k_mw_geo_dist, dim3((unsigned)((pc * K + 255) / 256)), dim3(256), 0, h->stream, J.lon + p0, J.lat + p0, pc, K,
                           (const double*)h->xs.as<double>(), (const double*)h->ys.as<double>(), (const int*)idx, dist);
      MwArgs a{};
      a.sx = h->xs.as<double>();
      a.sy = h->ys.as<double>();
      a.sz = h->zs.as<double>();
      a.mode = h->geo ? 1 : h->ndim;
      a.K = K;
      a.npt = (int)pc;
      a.idx = idx;
      a.dist = dist;
      a.Z = h->vals.as<double>();
      a.v = h->v;
      a.exact = h->exact;
      a.eps = h->eps;
      a.z = J.zs + p0;
      a.ss = J.sss + p0;
      a.flag = h->flag.as<int>();
      a.nrow = 1;
      a.zstride = h->N;
      a.pstride = npt;
      {  // right-hand sides in place over the distances
        const long ne = pc * K;
        const unsigned rg = (unsigned)((ne + 255) / 256);
        if (custom) {
          // d -> gamma(d) on the host for the point-station distances and for the K x K station pairs of every point
          HIPC(hipMemcpyAsync(gvec.p, dist, sizeof(double) * ne, hipMemcpyDeviceToDevice, h->stream));
          MIKC(custom_roundtrip(h, gvec.as<double>(), pc, K, K));
          hipLaunchKernelGGL(k_mw_rhs_table, dim3(rg), dim3(256), 0, h->stream, dist, (const double*)gvec.as<double>(), ne, h->exact,
                             h->eps);
          hipLaunchKernelGGL(k_mw_pairdist, dim3((unsigned)((ne * K + 255) / 256)), dim3(256), 0, h->stream, (const int*)idx, pc, K,
                             a.sx, a.sy, a.sz, a.mode, gtab.as<double>());
          MIKC(custom_roundtrip(h, gtab.as<double>(), pc * K, K, K));
          a.gtab = gtab.as<double>();
        } else {
          MwRhsArgs ra{};
          ra.dist = dist, ra.n = ne, ra.v = h->v, ra.exact = h->exact, ra.eps = h->eps;
          if (J.nd > 1) {  // block centres: the mean of the nodes' right-hand sides (the job's owner admits Euclidean named models only)
            ra.idx = idx, ra.K = K;
            ra.qx = qx + p0, ra.qy = qy + p0, ra.qz = three ? qz + p0 : nullptr;
            ra.sx = a.sx, ra.sy = a.sy, ra.sz = a.sz;
            ra.off = J.off, ra.nd = J.nd;
            if (h->ndim == 3) { MW_RHS(3, rg, ra) } else { MW_RHS(2, rg, ra) }
          } else {
            MW_RHS(0, rg, ra)
          }
        }
      }
      HIPC(hipEventRecord(h->evpool[2 + 2 * solve_chunks], h->stream));
      if (nf == 0) {
        MIKC(solve(a, pc));
      } else {
        for (int f = 0; f < gn; f += rows) {  // field g0 + f .. in the rows of one pass
          a.nrow = std::min(rows, gn - f);
          a.Z = fv + (size_t)(g0 + f) * (size_t)h->N;
          a.z = zpl + (size_t)f * (size_t)npt + p0;
          MIKC(solve(a, pc));
        }
      }
      HIPC(hipEventRecord(h->evpool[3 + 2 * solve_chunks], h->stream));
      ++solve_chunks;
      HIPC(hipGetLastError());
    }
    const unsigned ugrid = (unsigned)((npt + 255) / 256);
    if (nf == 0) {
      if (permuted)  // back to the caller's order
        hipLaunchKernelGGL(k_ps_unsort, dim3(ugrid), dim3(256), 0, h->stream, J.perm, npt, (const double*)J.zs, (const double*)J.sss, J.z, J.ss);
    } else {
      if (permuted) {  // sigma^2 and the group's planes back to the caller's order, two per launch (sigma^2 again beside an odd last plane)
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
        HIPC(hipMemcpyAsync(J.hz + (size_t)g0 * npt, J.fz, sizeof(double) * (size_t)gn * npt, hipMemcpyDeviceToHost, h->stream));
      }
    }
  }
  int flag = 0;
  HIPC(hipMemcpyAsync(&flag, h->flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPC(hipEventRecord(h->evpool[1], h->stream));
  HIPC(hipStreamSynchronize(h->stream));  // also: the scoped work buffers are released only after the stream drained
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, h->evpool[0], h->evpool[1]));
  h->tm.predict_ms = ms;
  for (long c = 0; c < solve_chunks; ++c) {  // the per-point solves (the dominant kernel of this path) on their own
    HIPC(hipEventElapsedTime(&ms, h->evpool[2 + 2 * c], h->evpool[3 + 2 * c]));
    h->tm.contract_ms += ms;
  }
  h->tm.contract_launches = solve_chunks;
  h->tm.mw_kernel = chol ? 1 : cholb ? 4 : (big ? 3 : 2);
  h->tm.rhs_ms = h->tm.predict_ms - h->tm.contract_ms;  // neighbour search + right-hand sides
  if ((flag & 2) && !mw_piv) {  // a local system was not positive definite after the shift: redo with partial pivoting
    HIPC(hipEventRecord(h->evpool[0], h->stream));
    h->mw_force_piv = true;
    const int rc = run_mw_job(h, K, J);
    h->mw_force_piv = false;
    return rc;
  }
  if (flag) return fail(MIK_ESINGULAR, "Singular matrix");  // cok.pyx:176-177
  return MIK_OK;
}

// The moving window over the resident points: mik_predict_moving_window (nd = 0) and mik_predict_block_window (the points are block
// centres, offsets the nd x ndim adjusted node offsets on the host).  nd = 1 is a block of one node at its centre: the point form.
static int predict_mw_body(mik_handle* h, int n_closest, const double* offsets, int nd, const char* name) {
  if (!h || !h->have_problem) return fail(MIK_ESTATE, std::string(name) + ": set the problem first");
  if (!h->have_points) return fail(MIK_ESTATE, std::string(name) + ": set points first");
  if (h->p != 0) return fail(MIK_EINVAL, "moving-window kriging exists for ordinary kriging only (ok.py:929, ok3d.py:901)");
  if (n_closest < 2) return fail(MIK_EINVAL, "n_closest_points has to be at least two!");
  if (n_closest > h->N) return fail(MIK_EINVAL, "n_closest_points exceeds the number of stations");
  HIPC(hipSetDevice(h->device));
  MIKC(get_events(h, 2));
  const long npt = h->npt;
  const int K = n_closest;
  const int nf = h->nf;
  h->tm.rhs_ms = h->tm.contract_ms = h->tm.predict_ms = 0.0;
  h->tm.contract_launches = 0;
  h->tm.contract_flops_executed = 0.0;
  h->nf_done = 0;
  if (npt == 0) {
    h->have_results = true;
    h->nf_done = nf;
    return MIK_OK;
  }
  HIPC(hipStreamWaitEvent(h->stream, h->ev_d2h, 0));
  HIPC(hipEventRecord(h->evpool[0], h->stream));
  const bool custom = h->model == MIK_MODEL_CUSTOM;
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
  // Small windows over a point list in no spatial order (round 4, second session): the lane-per-point search needs 64
  // consecutive points to share a few cells of the station grid.  The points are then put in Hilbert-curve order on the device
  // (k_ps_*: the sorter of the range-aware contraction), searched and solved in that order -- coordinates gathered once, z and
  // sigma^2 scattered back at the end -- so a shuffled list costs what the rows of a grid cost.
  bool mw_sorted = false;
  J.zs = J.z = h->z.as<double>(), J.sss = J.ss = h->ss.as<double>();
  if (mw_knn_cap(K) <= h->opt_mw_lds_cap) {
    MIKC(build_mw_grid(h, std::max(8, std::min(K, 256))));
    const bool cells = (long)h->grid.nx * h->grid.ny * h->grid.nz > 1;
    const bool coherent = h->pts_step >= 0.0 && 64.0 * h->pts_step <= 10.0 * h->grid.cell;
    if (h->opt_mw_knn_lane && h->opt_sort_points != 0 && K <= 16 && cells && !h->geo && !custom && !coherent && h->pts_extent > 0.0 &&
        npt >= 4096) {
      const double spacing = h->pts_extent / std::pow((double)npt, 1.0 / h->ndim);  // of a sorted list: a wavefront's 64 points are a patch
      if (12.0 * spacing <= 10.0 * h->grid.cell) {                                   // ~8 spacings across
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
        mw_sorted = true;
      }
    }
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
  MIKC(run_mw_job(h, K, J));
  if (nd > 1) {
    // sigma^2_V = (-lam . bbar - mu) - gbar: once, behind the job -- a redo with pivoting re-enters run_mw_job and must not subtract twice
    double* gbar = blk.as<double>() + (size_t)nd * (size_t)h->ndim;
    HIPC(hipEventRecord(h->evpool[0], h->stream));
    MIKC(launch_block_gamma(h, J.off, nd, gbar));
    MIKC(launch_block_ss(h, J.ss, npt, gbar));
    HIPC(hipEventRecord(h->evpool[1], h->stream));
    HIPC(hipStreamSynchronize(h->stream));  // the copies below run on another stream, and blk goes out of scope
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, h->evpool[0], h->evpool[1]));
    h->tm.predict_ms += ms;
    h->tm.rhs_ms += ms;  // (everything of the call that is not a solve)
  }
  MIKC(h->pin_out.ensure(sizeof(double) * 2 * (size_t)npt));
  if (nf == 0) HIPC(hipMemcpyAsync(h->pin_out.as<double>(), h->z.p, sizeof(double) * npt, hipMemcpyDeviceToHost, h->stream_d2h));
  HIPC(hipMemcpyAsync(h->pin_out.as<double>() + npt, h->ss.p, sizeof(double) * npt, hipMemcpyDeviceToHost, h->stream_d2h));
  HIPC(hipEventRecord(h->ev_d2h, h->stream_d2h));
  h->have_results = true;
  h->nf_done = nf;
  return MIK_OK;
}

int one_predict_mw(mik_handle* h, int n_closest) { return predict_mw_body(h, n_closest, nullptr, 0, "mik_predict_moving_window"); }

int one_predict_block_mw(mik_handle* h, const double* offsets, int nd, int n_closest) {
  return predict_mw_body(h, n_closest, offsets, nd, "mik_predict_block_window");
}

// Windowed leave-one-out cross-validation (mik_cross_validate_window): the job is the stations themselves, in the cell-sorted order the
// search grid already holds them in (G.gx / gy / gz, G.orig) -- 64 consecutive queries share a few cells by construction, so the lane
// search applies for K <= 16 on any grid of more than one cell, without a point sort.  Query t is station orig[t] and stays out of its own
// window by index (KnnArgs::self).  Results land in buffers of this call (cvw) and are scattered back through orig (k_ps_unsort); the
// resident points, h->z / h->ss, the landing zones, have_results and a resident factor are not touched.
int one_cross_validate_window(mik_handle* h, int n_closest, double* zhat_out, double* ss_out) {
  if (h->p != 0) return fail(MIK_EINVAL, "moving-window kriging exists for ordinary kriging only (ok.py:929, ok3d.py:901)");
  if (n_closest < 2) return fail(MIK_EINVAL, "n_closest_points has to be at least two!");
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
