// mik_predict.hip -- K3: right-hand sides + dense / range-aware contraction of the resident points
// One translation unit of libmikrige.so (pykrige_amd/build.py compiles them in parallel).
#include "mik_k_predict.h"
#include "mik_k_cov.h"
#include "mik_host.h"

// unit vectors of the resident (geographic) points, gu[0 .. npt) x, [npt .. 2 npt) y, [2 npt .. 3 npt) z; on the handle's stream
static int geo_point_vectors(mik_handle* h) {
  const long npt = h->npt;
  MIKC(h->gu.ensure(sizeof(double) * 3 * (size_t)npt));
  double* u = h->gu.as<double>();
  hipLaunchKernelGGL(k_geo_unit_p, dim3((unsigned)((npt + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->px.as<double>(),
                     (const double*)h->py.as<double>(), npt, u, u + npt, u + 2 * npt);
  return MIK_OK;
}

// Hilbert-curve order of the resident points inside every launch of `chunk` points (k_ps_*, mik_kernels.h): ps_idx[0][s] = index of
// the point at sorted position s.  On the handle's stream; two radix passes of 10-bit digits, all segments side by side.
int sort_points(mik_handle* h, long chunk, long nchunks) {
  const long npt = h->npt;
  const int kd = h->ndim;  // (geographic points: the curve runs through (lon, lat), like the stations' -- mikrige.hip, station_order)
  const int bits = ps_bits(kd), bps = (int)((chunk + MIK_PS_TILE - 1) / MIK_PS_TILE);
  for (int q = 0; q < 2; ++q) {
    MIKC(h->ps_key[q].ensure(sizeof(unsigned) * (size_t)npt));
    MIKC(h->ps_idx[q].ensure(sizeof(unsigned) * (size_t)npt));
  }
  MIKC(h->ps_table.ensure(sizeof(unsigned) * (size_t)nchunks * (1u << MIK_PS_DB) * (size_t)bps));
  MIKC(h->ps_box.ensure(sizeof(double) * 4 * (size_t)nchunks));
  const double *px = h->px.as<double>(), *py = h->py.as<double>(), *pz = h->ndim == 3 ? h->pz.as<double>() : nullptr;
  hipStream_t st = h->stream;
  hipLaunchKernelGGL(k_ps_bbox, dim3((unsigned)nchunks), dim3(1024), 0, st, px, py, pz, npt, chunk, bits, h->ps_box.as<double>());
  hipLaunchKernelGGL(k_ps_keys, dim3((unsigned)((npt + 255) / 256)), dim3(256), 0, st, px, py, pz, npt, chunk, kd, bits,
                     (const double*)h->ps_box.as<double>(), h->ps_key[0].as<unsigned>(), h->ps_idx[0].as<unsigned>());
  for (int pass = 0; pass < 2; ++pass) {
    const unsigned* kin = h->ps_key[pass].as<unsigned>();
    const unsigned* iin = h->ps_idx[pass].as<unsigned>();
    hipLaunchKernelGGL(k_ps_hist, dim3((unsigned)(nchunks * bps)), dim3(256), 0, st, kin, npt, chunk, bps, MIK_PS_DB * pass,
                       h->ps_table.as<unsigned>());
    hipLaunchKernelGGL(k_ps_scan, dim3((unsigned)nchunks), dim3(1 << MIK_PS_DB), 0, st, h->ps_table.as<unsigned>(), bps);
    hipLaunchKernelGGL(k_ps_scatter, dim3((unsigned)(nchunks * bps)), dim3(256), 0, st, kin, iin, npt, chunk, bps, MIK_PS_DB * pass,
                       (const unsigned*)h->ps_table.as<unsigned>(), h->ps_key[pass ^ 1].as<unsigned>(), h->ps_idx[pass ^ 1].as<unsigned>());
  }
  HIPC(hipGetLastError());
  h->ps_valid = true;
  h->ps_chunk = chunk;
  return MIK_OK;
}

// nf value fields on the host -- the fields of mik_set_fields, else (none set) the problem's own values -- as nfp planes of N with zero
// planes from nf on; sorted: in the factor's station order (position i holds caller station sort_perm[i]), else the caller's
static std::vector<double> stage_fields(const mik_handle* h, int nf, int nfp, bool sorted) {
  const long N = h->N;
  std::vector<double> v((size_t)nfp * (size_t)N, 0.0);
  for (int f = 0; f < nf; ++f) {
    const double* src = h->nf > 0 ? h->hfields.data() + (size_t)f * N : h->hvals.data();
    double* dst = v.data() + (size_t)f * N;
    if (sorted) {
      for (long i = 0; i < N; ++i) dst[i] = src[h->sort_perm[(size_t)i]];
    } else {
      memcpy(dst, src, sizeof(double) * (size_t)N);
    }
  }
  return v;
}

// nf planes of zhat and sigma^2 behind them, from the device (zd, sd: planes of N in the factor's station order) to the caller's arrays in
// the caller's station order; waits for the handle's stream
static int cv_copy_back(mik_handle* h, const double* zd, const double* sd, int nf, bool sorted, double* zhat_out, double* ss_out) {
  const long N = h->N;
  std::vector<double> out((size_t)(nf + 1) * (size_t)N);
  HIPC(hipMemcpyAsync(out.data(), zd, sizeof(double) * (size_t)nf * (size_t)N, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipMemcpyAsync(out.data() + (size_t)nf * N, sd, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  for (int f = 0; f <= nf; ++f) {
    const double* src = out.data() + (size_t)f * N;
    double* dst = f < nf ? zhat_out + (size_t)f * N : ss_out;
    if (sorted) {
      for (long i = 0; i < N; ++i) dst[h->sort_perm[(size_t)i]] = src[i];
    } else {
      memcpy(dst, src, sizeof(double) * (size_t)N);
    }
  }
  return MIK_OK;
}

// V in fv: field f at fv + f N, in the caller's station order (want = 0: the moving window's too) or the factor's (1)
int upload_fields(mik_handle* h, int want) {
  // columns: a multiple of MIK_FB that also holds the last read-back launch's (fields 1 + MIK_FB k .. MIK_FB (k + 1), see launch_rhs)
  const int nf = h->nf, nfp = ((nf - 1 + MIK_FB - 1) / MIK_FB) * MIK_FB + MIK_FB;
  const long N = h->N;
  if (h->fv_sorted != want) {
    if (want && (long)h->sort_perm.size() != N) return fail(MIK_ESTATE, "mik_predict: station order of the factor unknown");
    const std::vector<double> v = stage_fields(h, nf, nfp, want != 0);
    MIKC(h->fv.ensure(sizeof(double) * v.size()));
    HIPC(hipMemcpyAsync(h->fv.p, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, h->stream));
    HIPC(hipStreamSynchronize(h->stream));  // v is a local
    h->fv_sorted = want;
  }
  return MIK_OK;
}

// Several value fields (mik_set_fields): C = A_inv[:, :N] V from this device's own copy of the inverse, MIK_FB columns per block of
// k_cvec_fields<MIK_FB> (column f is bit for bit the k_cvec of field f).  V goes up once per set of fields and station order.
static int fields_coefficients(mik_handle* h) {
  const int nf = h->nf, nfp = ((nf - 1 + MIK_FB - 1) / MIK_FB) * MIK_FB + MIK_FB;
  const long N = h->N;
  MIKC(upload_fields(h, h->factor_sorted ? 1 : 0));
  MIKC(h->fc.ensure(sizeof(double) * (size_t)nfp * (size_t)h->Mp));
  hipLaunchKernelGGL((k_cvec_fields<MIK_FB>), dim3((h->Mp + 3) / 4, nfp / MIK_FB), dim3(256), 0, h->stream, (const double*)h->T.as<double>(),
                     (long)h->Mp, h->M, h->N, (const double*)h->fv.as<double>(), (long)N, h->fc.as<double>(), (long)h->Mp, h->Mp);
  HIPC(hipGetLastError());
  return MIK_OK;
}

// Leave-one-out cross-validation from the resident inverse (mik_cross_validate, global form): one launch of k_cv_loo<MIK_FB> (k_cvec_fields's sums with a
// diagonal epilogue) over the station rows -- the fields of mik_set_fields, else the problem's values, in the factor's station order -- then
// one copy back and, for a factor in Hilbert-curve order, the un-permutation on the host.  Touches neither the resident points nor results.
// zhat_out: max(nf, 1) planes of N in the caller's station order; ss_out: N.
int one_cross_validate(mik_handle* h, double* zhat_out, double* ss_out) {
  if (!h->have_factor) return fail(MIK_ESTATE, "mik_cross_validate: no factor");
  if (h->pinv) return fail(MIK_EINVAL, "mik_cross_validate: the leave-one-out identity needs a regular inverse (pseudo_inv is set)");
  HIPC(hipSetDevice(h->device));
  const long N = h->N;
  const int nf = std::max(h->nf, 1), nfp = ((nf + MIK_FB - 1) / MIK_FB) * MIK_FB;
  const bool sorted = h->factor_sorted;
  if (sorted && (long)h->sort_perm.size() != N) return fail(MIK_ESTATE, "mik_cross_validate: station order of the factor unknown");
  const std::vector<double> v = stage_fields(h, nf, nfp, sorted);
  DevBuf dv, dout;  // V (padded to a multiple of MIK_FB fields); the zhat planes and 1 / B_ii behind them.  Freed after the stream drained
  MIKC(dv.ensure(sizeof(double) * v.size()));
  MIKC(dout.ensure(sizeof(double) * (size_t)(nfp + 1) * (size_t)N));
  HIPC(hipMemcpyAsync(dv.p, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, h->stream));
  double* zd = dout.as<double>();
  double* sd = zd + (size_t)nfp * (size_t)N;
  hipLaunchKernelGGL((k_cv_loo<MIK_FB>), dim3((unsigned)((N + 3) / 4), nfp / MIK_FB), dim3(256), 0, h->stream, (const double*)h->T.as<double>(),
                     (long)h->Mp, (int)N, (const double*)dv.as<double>(), N, zd, N, sd);
  HIPC(hipGetLastError());
  return cv_copy_back(h, zd, sd, nf, sorted, zhat_out, ss_out);
}

// Leave-group-out cross-validation from the resident inverse (mik_cross_validate_folds): fold[i] in [0, nfolds) is the group of caller
// station i; every group is kriged from all the others (mik_k_cvfolds.h).  The per-fold station lists are built in the FACTOR's station
// order (a Hilbert-ordered factor holds caller station sort_perm[p] at position p), ascending, so that a fold's sums depend on its members
// alone.  c = B[:, :N] V by k_cvec_fields<MIK_FB> (leave-one-out's sums), then one launch of k_cv_folds per size class: folds of
// up to MIK_CVF_LDS stations factor their block in LDS, larger ones in m x m doubles of scratch (sum of m^2 over those folds, at most N^2,
// one allocation with the two work planes, freed after the stream drained).  Copy back and un-permutation as one_cross_validate (cv_copy_back).
int one_cross_validate_folds(mik_handle* h, const int32_t* fold, int nfolds, double* zhat_out, double* ss_out) {
  if (!h->have_factor) return fail(MIK_ESTATE, "mik_cross_validate_folds: no factor");
  if (h->pinv) return fail(MIK_EINVAL, "mik_cross_validate_folds: the block-inverse identity needs a regular inverse (pseudo_inv is set)");
  HIPC(hipSetDevice(h->device));
  const long N = h->N;
  const int nf = std::max(h->nf, 1), nfp = ((nf + MIK_FB - 1) / MIK_FB) * MIK_FB;
  const bool sorted = h->factor_sorted;
  if (sorted && (long)h->sort_perm.size() != N) return fail(MIK_ESTATE, "mik_cross_validate_folds: station order of the factor unknown");
  std::vector<long> off((size_t)nfolds + 1, 0);
  for (long i = 0; i < N; ++i) {
    if (fold[i] < 0 || fold[i] >= nfolds) return fail(MIK_EINVAL, "mik_cross_validate_folds: fold index outside [0, nfolds)");
    ++off[(size_t)fold[i] + 1];
  }
  for (int f = 0; f < nfolds; ++f) {
    if (off[(size_t)f + 1] >= N) return fail(MIK_EINVAL, "mik_cross_validate_folds: a fold holds every station (nothing is left to krige from)");
    off[(size_t)f + 1] += off[(size_t)f];
  }
  std::vector<int> idx((size_t)N);
  {
    std::vector<long> fill(off.begin(), off.end() - 1);
    for (long p = 0; p < N; ++p) idx[(size_t)fill[(size_t)fold[sorted ? h->sort_perm[(size_t)p] : p]]++] = (int)p;
  }
  // the two launches' descriptors (first entry of idx, m, first double in scratch), small folds first; empty folds take no part
  std::vector<long> desc;
  int nsmall = 0, nbig = 0, msmall = 0;
  size_t gtot = 0;
  for (int big = 0; big < 2; ++big)
    for (int f = 0; f < nfolds; ++f) {
      const long m = off[(size_t)f + 1] - off[(size_t)f];
      if (m == 0 || (m > MIK_CVF_LDS) != (big == 1)) continue;
      desc.insert(desc.end(), {off[(size_t)f], m, (long)gtot});
      if (big) {
        gtot += (size_t)m * (size_t)m;
        ++nbig;
      } else {
        msmall = std::max(msmall, (int)m);
        ++nsmall;
      }
    }
  const std::vector<double> v = stage_fields(h, nf, nfp, sorted);
  // V and c (nfp planes each); zhat (nfp planes) and sigma^2; scratch and the two work planes; the lists.  Freed after the stream drained
  DevBuf dv, dout, dwork, dlist;
  MIKC(dv.ensure(sizeof(double) * 2 * v.size()));
  MIKC(dout.ensure(sizeof(double) * (size_t)(nfp + 1) * (size_t)N));
  MIKC(dwork.ensure(sizeof(double) * (gtot + 2 * (size_t)MIK_FB * (size_t)N)));
  MIKC(dlist.ensure(sizeof(long) * desc.size() + sizeof(int) * idx.size()));
  HIPC(hipMemcpyAsync(dv.p, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, h->stream));
  HIPC(hipMemcpyAsync(dlist.p, desc.data(), sizeof(long) * desc.size(), hipMemcpyHostToDevice, h->stream));
  int* didx = reinterpret_cast<int*>(dlist.as<long>() + desc.size());
  HIPC(hipMemcpyAsync(didx, idx.data(), sizeof(int) * idx.size(), hipMemcpyHostToDevice, h->stream));
  double* cd = dv.as<double>() + v.size();
  hipLaunchKernelGGL((k_cvec_fields<MIK_FB>), dim3((unsigned)((N + 3) / 4), nfp / MIK_FB), dim3(256), 0, h->stream, (const double*)h->T.as<double>(),
                     (long)h->Mp, (int)N, (int)N, (const double*)dv.as<double>(), N, cd, N, (int)N);
  CvfArgs a;
  a.B = h->T.as<double>(), a.ldb = h->Mp, a.C = cd, a.V = dv.as<double>(), a.idx = didx, a.desc = dlist.as<long>();
  a.scratch = dwork.as<double>(), a.wc = a.scratch + gtot, a.wt = a.wc + (size_t)MIK_FB * (size_t)N;
  a.zhat = dout.as<double>(), a.ss = a.zhat + (size_t)nfp * (size_t)N, a.n = N, a.nfb = nfp / MIK_FB, a.ldw = msmall | 1;
  if (nsmall) {
    const size_t lds = sizeof(double) * (size_t)msmall * (size_t)a.ldw;
    HIPC(hipFuncSetAttribute((const void*)k_cv_folds<MIK_FB, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_cv_folds<MIK_FB, false>), dim3((unsigned)nsmall), dim3(256), lds, h->stream, a);
  }
  if (nbig) {
    const size_t lds = sizeof(double) * 2 * MIK_CVF_NB * MIK_CVF_TLD;
    a.desc += 3 * (size_t)nsmall;
    HIPC(hipFuncSetAttribute((const void*)k_cv_folds<MIK_FB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_cv_folds<MIK_FB, true>), dim3((unsigned)nbig), dim3(256), lds, h->stream, a);
  }
  HIPC(hipGetLastError());
  return cv_copy_back(h, a.zhat, a.ss, nf, sorted, zhat_out, ss_out);
}

// point blocks per group of k_sp_tiles_g's queue order (a group's tiles run on one XCD, tile position ascending, point block fast;
// round 5: 4 -> 16, contraction 35.7 -> 35.3 ms at config 5)
static constexpr int SP_GROUP = 16;

// what one predict runs (plan_predict): launches of `chunk` points on the dense or the range-aware path, on one lane or two
struct Plan {
  long npt, chunk, nchunks;
  int Mp, nIblk, nK16, nKt, kend, nf;
  bool sparse, gathered, sortpts, lanes2;
  const unsigned* perm;  // the points of every launch in Hilbert-curve order: ps_idx[0] (else nullptr)
  // fields with missing stations (gaps_setup): patterns with a gap, 128-row blocks of W_all, the patterns' descriptors on the device
  bool gaps;
  int gap_np, gap_nRblk;
  const long* gap_desc;
  // a predict with the error covariance (one_predict_cov) on the dense path: every launch writes its panel into the one panel of all
  // points, at t0 * Mp, and contracts from there (nullptr: the lane's panel)
  double* panel;
};

// launch c of a plan: points [t0, t0 + nvalid), padded to palloc = 128 nTb
struct Launch {
  long c, t0;
  int nvalid, palloc, nTb;
  Launch(const Plan& p, long c_)
      : c(c_), t0(c_ * p.chunk), nvalid((int)std::min<long>(p.chunk, p.npt - t0)), palloc(((nvalid + 127) / 128) * 128), nTb(palloc / 128) {}
};

// chunk size and count, path, lanes and point sort of this predict; the timing fields that describe them; the work buffers and events
static int plan_predict(mik_handle* h, Plan& p, bool cov) {
  const long npt = h->npt;
  const int Mp = h->Mp, nIblk = Mp / 128, nf = h->nf;
  p.npt = npt, p.Mp = Mp, p.nIblk = nIblk, p.nK16 = Mp / 16, p.nf = nf;
  p.kend = ((h->M + MIK_BK - 1) / MIK_BK) * MIK_BK;
  if (nf > 1) {  // value fields (mik_set_fields): field 0 goes to z, the others to the planes of zf
    MIKC(h->zf.ensure(sizeof(double) * (size_t)(nf - 1) * (size_t)npt));
    // page-locked landing zone of fields 1 .. nf - 1, filled chunk by chunk like pin_out (an earlier predict's copies may still write it)
    HIPC(hipEventSynchronize(h->ev_d2h));
    MIKC(h->pin_fz.ensure(sizeof(double) * (size_t)(nf - 1) * (size_t)npt));
  }
  if (nf > 0 && h->gaps_any) HIPC(hipEventSynchronize(h->ev_d2h));  // (pin_gss likewise: gaps_setup sizes it)
  long chunk = std::min<long>(h->opt_chunk, ((npt + 127) / 128) * 128);
  if (h->model == MIK_MODEL_CUSTOM) chunk = std::min<long>(chunk, 16384);  // each chunk's distances visit the host
  // range-aware contraction (k_contract_sp): the factor is in Hilbert-curve station order and the variogram has compact support
  // fields with missing stations (mik_set_field_gaps) take the dense path: W b needs the whole right-hand side, and the range-aware panel
  // holds only the candidate tiles (a Hilbert-ordered factor is fine: the dense path accepts it)
  p.gaps = nf > 0 && h->gaps_any;
  p.sparse = h->factor_sorted && h->opt_sparse != 2 && h->opt_sparse != 0 && !p.gaps;
  // a predict with the error covariance on the dense path needs no panel of a launch: its launches write into the panel of all points
  // (a range-aware one keeps its own panels of delta and writes the panel of all points in a pass of its own: predict_body)
  const bool shared_panel = cov && !p.sparse;
  if (p.sparse) chunk = std::min<long>(chunk, 131072);  // k_sp_tiles: at most 1024 point blocks per launch
  // tiles of gathered 16-row groups (k_contract_spg) wherever 32-bit LDS-DMA offsets reach every row of the inverse
  p.gathered = p.sparse && h->opt_sparse_rows != 128 && (double)Mp * (double)Mp * 8.0 < 4294967296.0;
  // gathered row groups (round 5): flags and lists per 8 stations (candidates stay per 16), a K step = a pair of list-adjacent 8-station tiles
  // (k_contract_spg H8); the aligned-block fallback keeps 16-station lists.  nKt = tiles per point block in the units of this launch's lists.
  // (Round 4's 16-station lists under gathered groups and the epilogue from global memory -- "sparse_ktile" 16, "sparse_epilogue" 0 -- lost
  // their A/B in round 5 and left the library in round 6.)
  p.nKt = p.gathered ? Mp / 8 : p.nK16;
  h->tm.sparse_ktile = !p.sparse ? 0 : p.gathered ? 8 : 16;
  h->tm.sparse = p.sparse ? 1 : 0;
  h->tm.sparse_rows = p.sparse ? (p.gathered ? 16 : 128) : 0;
  h->tm.stations_sorted = h->factor_sorted ? 1 : 0;
  h->tm.sparse_tiles = h->tm.sparse_tiles_dense = h->tm.sparse_ktiles = h->tm.sparse_ktiles_dense = h->tm.sparse_lists_ms = 0.0;
  h->tm.sparse_diag_products = 0.0;
  // the points of every launch in Hilbert-curve order among themselves (compact point blocks: option "sort_points")
  // (auto: not for small jobs -- seven more launches, 0.07 ms, against a contraction of microseconds; one tile per point block anyway
  // while the matrix has fewer than 512 rows)
  p.sortpts = p.sparse && (h->opt_sort_points == 1 || (h->opt_sort_points < 0 && npt >= 4096 && Mp >= 512));
  h->tm.points_sorted = p.sortpts ? 1 : 0;
  h->tm.sort_points_ms = 0.0;
  const bool lanes2_wanted = p.sparse && h->opt_sparse_lanes == 2;
  // keep the RHS panels under ~1/4 of device memory
  size_t freeb = 0, totalb = 0;
  HIPC(hipMemGetInfo(&freeb, &totalb));
  const size_t have = h->lane[0].Bt.bytes + h->lane[1].Bt.bytes;
  while (!shared_panel && chunk > 128 && (size_t)chunk * Mp * sizeof(double) * (lanes2_wanted ? 2 : 1) > std::max(freeb + have, have) / 2) chunk = ((chunk / 2 + 127) / 128) * 128;
  // equal chunks: ceil(npt / chunk) launches of the same size (a short last launch drains as long as a full one)
  long nchunks = (npt + chunk - 1) / chunk;
  chunk = (((npt + nchunks - 1) / nchunks + 127) / 128) * 128;
  nchunks = (npt + chunk - 1) / chunk;
  p.chunk = chunk, p.nchunks = nchunks;
  p.lanes2 = lanes2_wanted && nchunks > 1;
  MIKC(h->pin_out.ensure(sizeof(double) * 2 * (size_t)npt));  // (a previous result may have left with mik_take_results)
  if ((long)h->pr_launch.size() < nchunks) h->pr_launch.resize((size_t)nchunks);
  for (LaunchEvents& ev : h->pr_launch)
    for (hipEvent_t* e : ev.all())
      if (!*e) HIPC(hipEventCreate(e));
  const size_t nTb = (size_t)chunk / 128;
  for (int L = 0; L < (p.lanes2 ? 2 : 1); ++L) {
    PredictLane& ln = h->lane[L];
    if (!shared_panel) MIKC(ln.Bt.ensure(sizeof(double) * (size_t)chunk * Mp));
    MIKC(ln.part.ensure(sizeof(double) * (size_t)chunk * nIblk));
    MIKC(ln.queue.ensure(8 * sizeof(unsigned long long)));
    if (!p.sparse) break;
    MIKC(ln.cand.ensure(nTb * p.nK16));
    MIKC(ln.flags.ensure(nTb * p.nKt));
    MIKC(ln.klist.ensure(sizeof(unsigned short) * nTb * p.nKt));
    MIKC(ln.kcount.ensure(sizeof(int) * nTb));
    MIKC(ln.nrows.ensure(sizeof(int) * nTb));
    if (p.gathered) {
      MIKC(ln.recs.ensure(48 * nTb * nIblk));  // ceil(nk / 8) <= nK16 / 8 = nIblk tiles per point block
    } else {
      MIKC(ln.rows.ensure(sizeof(unsigned short) * nTb * nIblk));
      MIKC(ln.rstart.ensure(sizeof(unsigned short) * nTb * nIblk));
      MIKC(ln.tiles.ensure(sizeof(unsigned) * nTb * nIblk));
    }
    MIKC(ln.xoff.ensure(sizeof(int) * 9));
  }
  if (p.sparse) MIKC(h->sp_stats.ensure(sizeof(unsigned long long) * 4 * (size_t)nchunks));
  return MIK_OK;
}

// what every right-hand-side kernel of launch l is told about the problem and the launch's points; the panel Bt, the coefficients cvec
// and the place zout of z are the caller's, and what only the range-aware path and the fields' read-back read stays zero
static RhsArgs rhs_args(mik_handle* h, const Plan& p, const Launch& l) {
  const long t0 = l.t0;
  RhsArgs a{};
  a.ld = p.Mp;
  a.palloc = l.palloc;
  a.nvalid = l.nvalid;
  a.px = h->px.as<double>() + t0;
  a.py = h->py.as<double>() + t0;
  a.pz = h->ndim == 3 ? h->pz.as<double>() + t0 : nullptr;
  a.N = h->N;
  a.p = h->p;
  a.M = h->M;
  a.Mp = p.Mp;
  a.ndim = h->ndim;
  a.xs = h->factor_sorted ? h->xs_s.as<double>() : h->xs.as<double>();
  a.ys = h->factor_sorted ? h->ys_s.as<double>() : h->ys.as<double>();
  a.zs = h->factor_sorted ? h->zs_s.as<double>() : h->zs.as<double>();
  a.dsc = h->factor_eq ? h->dsc.as<double>() : nullptr;
  a.v = h->v;
  a.exact = h->exact;
  a.eps = h->eps;
  a.rl = h->rl;
  a.nwells = h->nwells;
  a.nextra = h->nextra;
  a.wells = h->wells.as<double>();
  a.extra = h->nextra ? h->extra_rows.as<double>() + t0 : nullptr;
  a.extra_stride = p.npt;
  return a;
}

// the right-hand sides of launch l into lane ln's panel on stream st, with z of every field; the range-aware path first marks the
// candidate station tiles of every point block and then writes delta for those only
// zscratch (a dense plan only): a pass that is there for its panel alone -- z goes to zscratch, no event is recorded
static int launch_rhs(mik_handle* h, const Plan& p, const Launch& l, PredictLane& ln, hipStream_t st, double* zscratch = nullptr) {
  const LaunchEvents& ev = h->pr_launch[(size_t)l.c];
  const long t0 = l.t0, npt = p.npt;
  RhsArgs a = rhs_args(h, p, l);
  a.Bt = p.panel ? p.panel + (size_t)t0 * (size_t)p.Mp : ln.Bt.as<double>();
  a.cvec = p.nf > 0 ? (const double*)h->fc.as<double>() : (const double*)h->cvec.as<double>();
  a.zout = (zscratch ? zscratch : h->z.as<double>()) + t0;
  const dim3 grid(l.palloc / MIK_TP), block(256);
  if (!p.sparse) {
    if (!zscratch) HIPC(hipEventRecord(ev.rhs_begin, st));
    if (h->model == MIK_MODEL_CUSTOM) {
      DISPATCH_NDIM_FIXED(7, h->geo ? 1 : h->ndim, k_rhs, grid, block, st, a);
      MIKC(custom_roundtrip(h, a.Bt, l.nvalid, h->N, p.Mp));
      DISPATCH_NDIM_FIXED(6, h->geo ? 1 : h->ndim, k_rhs, grid, block, st, a);
    } else {
      DISPATCH_MODEL_NDIM(h->model, h->geo ? 1 : h->ndim, k_rhs, grid, block, st, a);
    }
  } else {  // candidates (bounding boxes), cleared flags, then delta for the candidate blocks only
    a.cand = ln.cand.as<unsigned char>();
    a.flags = ln.flags.as<unsigned char>();
    a.nIblk = p.nIblk;
    a.nK16 = p.nK16;
    a.nKf = p.nKt;
    a.sill = h->v.p0 + h->v.p2;
    if (p.perm) {  // sorted order: the chunk's points are reached through perm, from the list's base pointers
      a.perm = p.perm + t0;
      a.px = h->px.as<double>();
      a.py = h->py.as<double>();
      a.pz = h->ndim == 3 ? h->pz.as<double>() : nullptr;
      a.extra = h->nextra ? h->extra_rows.as<double>() : nullptr;
      a.zout = h->z.as<double>();
    }
    HIPC(hipEventRecord(ev.cand_begin, st));
    // candidates by bounding boxes: Euclidean coordinates against the range; geographic: unit vectors against the CHORD of the range
    // (2 sin(arc / 2), the range being degrees of arc; beyond 180 degrees everything is in range)
    const double *cx = a.px, *cy = a.py, *cz = a.pz;
    double radius = std::max(h->v.p1, h->eps);
    if (h->geo) {
      const long off = p.perm ? 0 : t0;
      cx = h->gu.as<double>() + off, cy = cx + npt, cz = cy + npt;
      radius = radius >= 180.0 ? 4.0 : 2.0 * std::sin(radius * 3.14159265358979323846 / 360.0) * (1.0 + 1e-12) + 1e-15;
    }
    hipLaunchKernelGGL(k_sp_cand, dim3(l.palloc / 128), dim3(128), 0, st, cx, cy, cz, l.nvalid, (const double*)h->sbox.as<double>(), p.nK16,
                       h->N / 16, (h->M + 15) / 16, radius, ln.cand.as<unsigned char>(), a.perm, p.gathered ? 0 : 1, ln.flags.as<unsigned char>(), p.nKt);
    HIPC(hipEventRecord(ev.rhs_begin, st));
    if (p.gathered) {
      if (h->geo) hipLaunchKernelGGL((k_rhs<3, 1, true, true>), grid, block, 0, st, a);
      else if (h->ndim == 3) hipLaunchKernelGGL((k_rhs<3, 3, true, true>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((k_rhs<3, 2, true, true>), grid, block, 0, st, a);
    } else if (h->geo) hipLaunchKernelGGL((k_rhs<3, 1, true>), grid, block, 0, st, a);
    else if (h->ndim == 3) hipLaunchKernelGGL((k_rhs<3, 3, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_rhs<3, 2, true>), grid, block, 0, st, a);
  }
  // fields 1 .. nf - 1: MIK_FB per launch, read back from the panel the launch of field 0 has just written (same stream, right after it)
  for (int f0 = 1; f0 < p.nf; f0 += MIK_FB) {
    RhsArgs b = a;
    b.cvec = h->fc.as<double>() + (size_t)f0 * p.Mp;
    b.cf_ld = p.Mp;
    b.nfc = std::min(MIK_FB, p.nf - f0);
    b.zout = h->zf.as<double>() + (size_t)(f0 - 1) * npt + (b.perm ? 0 : t0);
    b.zf_ld = npt;
    if (p.sparse) hipLaunchKernelGGL((k_rhs<0, 0, true, false, MIK_FB>), grid, block, 0, st, b);
    else hipLaunchKernelGGL((k_rhs<0, 0, false, false, MIK_FB>), grid, block, 0, st, b);
  }
  HIPC(hipGetLastError());
  if (!zscratch) HIPC(hipEventRecord(ev.rhs_end, st));
  return MIK_OK;
}

// dense contraction of launch l on the handle's stream with lane 0's buffers: row-block partial sums of b^T A_inv b, reduced to sigma^2
static int contract_dense(mik_handle* h, const Plan& p, const Launch& l) {
  const LaunchEvents& ev = h->pr_launch[(size_t)l.c];
  PredictLane& ln = h->lane[0];
  hipStream_t sc = h->stream;
  const int nIblk = p.nIblk, kend = p.kend;
  HIPC(hipEventRecord(ev.contract_begin, sc));
  const double* Ai = h->T.as<double>();
  const double* Bi = p.panel ? p.panel + (size_t)l.t0 * (size_t)p.Mp : ln.Bt.as<double>();
  double* pp = ln.part.as<double>();
  const long ldm = p.Mp;
  const unsigned sgrid = (unsigned)super_grid(nIblk, l.nTb);
  // persistent launch: 2 blocks per CU pop tiles from per-XCD sequences (8 counters, zeroed per launch); 8 wavefronts per tile
  // (wave tile 32 x 64).  Three forms: the symmetric half product with triangular diagonal blocks (default), with whole
  // diagonal blocks ("tri" 0) and the reference's full product w = A_inv b ("symmetric" 0) -- the cross-checks of the parity tests.
  // (The 4-wave tiles, the v_fma_f64 engine, pair units, popped-ahead tiles: every A/B of rounds 2-5 lost; tools/kernel_bench.)
  HIPC(hipMemsetAsync(ln.queue.p, 0, 8 * sizeof(unsigned long long), sc));
  unsigned long long* qp = ln.queue.as<unsigned long long>();
  const unsigned pgrid = (unsigned)std::min<long>(2L * h->n_cu, (long)sgrid);
  if (h->opt_sym && h->opt_tri) hipLaunchKernelGGL((k_contract<true, 2, true, false, true>), dim3(pgrid), dim3(512), 0, sc, Ai, ldm, Bi, ldm, pp, l.palloc, nIblk, kend, qp);
  else if (h->opt_sym) hipLaunchKernelGGL((k_contract<true, 2>), dim3(pgrid), dim3(512), 0, sc, Ai, ldm, Bi, ldm, pp, l.palloc, nIblk, kend, qp);
  else hipLaunchKernelGGL((k_contract<false, 2>), dim3(pgrid), dim3(512), 0, sc, Ai, ldm, Bi, ldm, pp, l.palloc, nIblk, kend, qp);
  HIPC(hipEventRecord(ev.contract_end, sc));
  hipLaunchKernelGGL(k_ss_reduce, dim3((l.nvalid + 255) / 256), dim3(256), 0, sc, (const double*)pp, l.palloc, nIblk, l.nvalid,
                     h->ss.as<double>() + l.t0);
  if (p.gaps) {  // Q = W_all Bt^T against the panel this launch has just written, squared and summed per 16-row group; then the patterns' planes
    HIPC(hipMemsetAsync(ln.queue.p, 0, 8 * sizeof(unsigned long long), sc));
    GapGemmArgs g{};
    g.W = h->gap_W.as<double>(), g.ldw = ldm, g.Bt = Bi, g.ldb = ldm, g.part = h->gap_part.as<double>();
    g.palloc = l.palloc, g.nRblk = p.gap_nRblk, g.kend = kend, g.queue = qp;
    const unsigned ggrid = (unsigned)std::min<long>(2L * h->n_cu, super_grid(p.gap_nRblk, l.nTb));
    hipLaunchKernelGGL((k_gap_contract<2>), dim3(ggrid), dim3(512), 0, sc, g);
    GapRedArgs r{};
    r.part = g.part, r.palloc = l.palloc, r.nvalid = l.nvalid, r.ss = h->ss.as<double>() + l.t0, r.desc = p.gap_desc;
    r.out = h->gap_ss.as<double>() + l.t0, r.ldo = p.npt;
    hipLaunchKernelGGL(k_gap_ss, dim3((l.nvalid + 255) / 256, p.gap_np), dim3(256), 0, sc, r);
  }
  return MIK_OK;
}

// Set-up of a predict whose fields have missing stations (mik_k_gaps.h), on the handle's stream behind fields_coefficients: the fields
// are grouped by identical valid column; every pattern with a gap gets its station list in the FACTOR's order, ascending (as
// one_cross_validate_folds builds the folds'), L^-1 of its block of the inverse, its rows of W_all and a sigma^2 plane; every field of
// such a pattern gets c~ in its column of fc.  A pattern without a gap does no work.
static int gaps_setup(mik_handle* h, Plan& p) {
  const long N = h->N;
  const int nf = h->nf, Mp = h->Mp;
  const bool sorted = h->factor_sorted;
  if (h->pinv) return fail(MIK_EINVAL, "mik_predict: fields with gaps need a regular inverse (pseudo_inv is set)");
  if (h->is_kid || !h->kids.empty()) return fail(MIK_EINVAL, "mik_predict: fields with gaps are not kriged by a device group");
  if ((long)h->hgaps.size() != (long)nf * N) return fail(MIK_ESTATE, "mik_predict: the gaps do not belong to these fields");
  if (sorted && (long)h->sort_perm.size() != N) return fail(MIK_ESTATE, "mik_predict: station order of the factor unknown");
  // patterns in the order their first field comes in, then the small ones (factored in LDS) in front of the large ones
  std::map<std::string, int> seen;
  std::vector<int> first, fraw((size_t)nf, -1);
  std::vector<long> msize;
  for (int f = 0; f < nf; ++f) {
    const uint8_t* col = h->hgaps.data() + (size_t)f * N;
    long m = 0;
    for (long i = 0; i < N; ++i) m += col[i] == 0;
    if (m == 0) continue;
    std::string key((size_t)N, '0');
    for (long i = 0; i < N; ++i) key[(size_t)i] = col[i] ? '1' : '0';
    auto it = seen.find(key);
    if (it == seen.end()) {
      it = seen.emplace(std::move(key), (int)first.size()).first;
      first.push_back(f);
      msize.push_back(m);
    }
    fraw[(size_t)f] = it->second;
  }
  const int np = (int)first.size();
  std::vector<int> order, place((size_t)np);
  for (int big = 0; big < 2; ++big)
    for (int q = 0; q < np; ++q)
      if ((msize[(size_t)q] > MIK_CVF_LDS) == (big == 1)) order.push_back(q);
  std::vector<long> desc((size_t)MIK_GAP_DESC * np);
  std::vector<int> idx, grp, fpat, fcol;
  std::vector<unsigned char> inS((size_t)np * Mp, 0);
  long rows = 0, gld = 1;
  size_t ltot = 0;
  int nsmall = 0, msmall = 0;
  for (int q = 0; q < np; ++q) {
    const int raw = order[(size_t)q];
    place[(size_t)raw] = q;
    const long m = msize[(size_t)raw];
    const uint8_t* col = h->hgaps.data() + (size_t)first[(size_t)raw] * N;
    desc[(size_t)MIK_GAP_DESC * q] = (long)idx.size(), desc[(size_t)MIK_GAP_DESC * q + 1] = m;
    desc[(size_t)MIK_GAP_DESC * q + 2] = (long)ltot, desc[(size_t)MIK_GAP_DESC * q + 3] = rows;
    for (long pos = 0; pos < N; ++pos)
      if (!col[sorted ? h->sort_perm[(size_t)pos] : pos]) {
        idx.push_back((int)pos);
        inS[(size_t)q * Mp + (size_t)pos] = 1;
      }
    for (long g = 0; g < (m + 15) / 16; ++g) grp.push_back(q);
    rows += ((m + 15) / 16) * 16;
    ltot += (size_t)m * (size_t)m;
    gld = std::max(gld, m);
    if (m <= MIK_CVF_LDS) ++nsmall, msmall = std::max(msmall, (int)m);
  }
  h->gap_plane.assign((size_t)nf, -1);
  for (int f = 0; f < nf; ++f)
    if (fraw[(size_t)f] >= 0) {
      h->gap_plane[(size_t)f] = place[(size_t)fraw[(size_t)f]];
      fpat.push_back(place[(size_t)fraw[(size_t)f]]);
      fcol.push_back(f);
    }
  const int nq = (int)fpat.size(), ngroups = (int)grp.size();
  const long rowsp = ((rows + MIK_BM - 1) / MIK_BM) * MIK_BM;
  if (ngroups > 65535) return fail(MIK_EINVAL, "mik_predict: more than 65535 16-row groups of missing stations");
  size_t freeb = 0, totalb = 0;
  HIPC(hipMemGetInfo(&freeb, &totalb));
  if (sizeof(double) * (double)rowsp * (double)Mp > (double)totalb / 4.0)
    return fail(MIK_EINVAL, "mik_predict: the rows of W for the missing stations (" + std::to_string(rowsp) + " x " + std::to_string(Mp) +
                                " doubles) would exceed a quarter of device memory");
  p.gap_np = np, p.gap_nRblk = (int)(rowsp / MIK_BM);
  // one list: the descriptors (longs), then idx, grp, fpat, fcol (ints), then the S masks (bytes)
  const size_t nint = idx.size() + grp.size() + fpat.size() + fcol.size();
  std::vector<char> blob(sizeof(long) * desc.size() + sizeof(int) * nint + inS.size());
  {
    char* w = blob.data();
    auto put = [&](const void* src, size_t bytes) {
      if (bytes) memcpy(w, src, bytes);
      w += bytes;
    };
    put(desc.data(), sizeof(long) * desc.size());
    put(idx.data(), sizeof(int) * idx.size());
    put(grp.data(), sizeof(int) * grp.size());
    put(fpat.data(), sizeof(int) * fpat.size());
    put(fcol.data(), sizeof(int) * fcol.size());
    put(inS.data(), inS.size());
  }
  MIKC(h->gap_list.ensure(blob.size()));
  MIKC(h->gap_W.ensure(sizeof(double) * (size_t)rowsp * (size_t)Mp));
  MIKC(h->gap_work.ensure(sizeof(double) * (ltot + (size_t)nq * (size_t)gld)));
  MIKC(h->gap_part.ensure(sizeof(double) * (size_t)(rowsp / 16) * (size_t)p.chunk));
  MIKC(h->gap_ss.ensure(sizeof(double) * (size_t)np * (size_t)p.npt));
  MIKC(h->pin_gss.ensure(sizeof(double) * (size_t)np * (size_t)p.npt));
  hipStream_t st = h->stream;
  HIPC(hipMemcpyAsync(h->gap_list.p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
  GapArgs a{};
  a.B = h->T.as<double>(), a.ldb = Mp, a.Mp = Mp;
  a.desc = h->gap_list.as<long>();
  a.idx = reinterpret_cast<const int*>(a.desc + desc.size());
  a.grp = a.idx + idx.size(), a.fpat = a.grp + grp.size(), a.fcol = a.fpat + fpat.size();
  a.inS = reinterpret_cast<const unsigned char*>(a.fcol + fcol.size());
  a.linv = h->gap_work.as<double>(), a.g = a.linv + ltot, a.gld = gld;
  a.W = h->gap_W.as<double>(), a.fc = h->fc.as<double>(), a.ldc = Mp, a.ldw = msmall | 1;
  p.gap_desc = a.desc;
  if (rowsp > 16L * ngroups)  // the rows that pad W_all to whole block tiles
    HIPC(hipMemsetAsync(a.W + (size_t)16 * ngroups * Mp, 0, sizeof(double) * (size_t)(rowsp - 16L * ngroups) * Mp, st));
  if (nsmall) {
    const size_t lds = sizeof(double) * (size_t)msmall * (size_t)a.ldw;
    HIPC(hipFuncSetAttribute((const void*)k_gap_factor<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_gap_factor<false>), dim3((unsigned)nsmall), dim3(256), lds, st, a);
  }
  if (np > nsmall) {
    const size_t lds = sizeof(double) * 2 * MIK_CVF_NB * MIK_CVF_TLD;
    GapArgs b = a;
    b.desc += (size_t)MIK_GAP_DESC * nsmall;
    HIPC(hipFuncSetAttribute((const void*)k_gap_factor<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_gap_factor<true>), dim3((unsigned)(np - nsmall)), dim3(256), lds, st, b);
  }
  const unsigned ncb = (unsigned)((Mp + 255) / 256);
  hipLaunchKernelGGL(k_gap_w, dim3(ncb, (unsigned)ngroups), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_gap_g, dim3((unsigned)nq), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_gap_coef, dim3(ncb, (unsigned)nq), dim3(256), 0, st, a);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(st));  // blob is a local
  return MIK_OK;
}

// sigma^2 of every field of the last predict from the landing zones, scattered through the mask like one_get_field_results: the plane of
// the field's pattern, or the all-stations sigma^2 for a field without gaps
int one_get_field_sigmasq(mik_handle* h, double* out, long ntot) {
  HIPC(hipSetDevice(h->device));
  HIPC(hipEventSynchronize(h->ev_d2h));
  const long n = h->npt;
  if (n == 0) return MIK_OK;
  for (int f = 0; f < h->nf_done; ++f) {
    const int pl = f < (int)h->gap_plane.size() ? h->gap_plane[(size_t)f] : -1;
    const double* src = pl < 0 ? h->pin_out.as<double>() + n : h->pin_gss.as<double>() + (size_t)pl * n;
    double* dst = out + (size_t)f * ntot;
    if (h->scatter32 || !h->scatter.empty()) {
      parallel_chunks(n, [&](int, long b, long e) {
        if (h->scatter32) {
          for (long i = b; i < e; ++i) dst[h->scatter32[i]] = src[i];
        } else {
          for (long i = b; i < e; ++i) dst[h->scatter[(size_t)i]] = src[i];
        }
      });
    } else {
      host_copy(dst + h->out_off, src, sizeof(double) * n);
    }
  }
  return MIK_OK;
}

// diagnostic (MIK_SPG_PROF=1): the contraction of one launch in k_contract_spg's profiling instantiation; cycle sums per phase of the
// tile loop, printed to stderr
static int spg_profile(SpgArgs ga, unsigned nb, hipStream_t sc) {
  static DevBuf pb;
  MIKC(pb.ensure(sizeof(unsigned long long) * nb * 96));
  HIPC(hipMemsetAsync(pb.p, 0, pb.bytes, sc));
  ga.prof = pb.as<unsigned long long>();
  hipLaunchKernelGGL((k_contract_spg<2, true, true, true>), dim3(nb), dim3(512), 0, sc, ga);
  std::vector<unsigned long long> hp((size_t)nb * 96);
  HIPC(hipMemcpyAsync(hp.data(), pb.p, sizeof(unsigned long long) * hp.size(), hipMemcpyDeviceToHost, sc));
  HIPC(hipStreamSynchronize(sc));
  static const char* names[8] = {"top drain+barrier", "off-diagonal K steps", "triangle K steps", "acquire", "adopt", "epilogue loads+sums", "reduce+store", "-"};
  {
    double c[16] = {0};
    for (unsigned b = 0; b < nb; ++b)
      for (int i = 0; i < 16; ++i) c[i] += (double)hp[(size_t)nb * 80 + (size_t)b * 16 + i];
    fprintf(stderr, "spg triangle steps (cycles per visit):");
    for (int w = 7; w >= 0; --w) fprintf(stderr, "  w=%d %.0f", w, c[w] / std::max(1.0, c[8 + w]));
    fprintf(stderr, "\n");
  }
  for (int wv : {0, 6}) {
    double sum[10] = {0};
    for (unsigned b = 0; b < nb; ++b)
      for (int i = 0; i < 10; ++i) sum[i] += (double)hp[((size_t)b * 8 + wv) * 10 + i];
    double tot = 0;
    for (int i = 0; i < 7; ++i) tot += sum[i];
    fprintf(stderr, "spg phases, wavefront %d: %.0f tiles of the launch, %.1f per block, %.1f off-diagonal steps per tile, %.0f cycles per tile\n", wv, sum[8], sum[8] / nb, sum[9] / std::max(1.0, sum[8]), tot / std::max(1.0, sum[8]));
    for (int i = 0; i < 7; ++i) fprintf(stderr, "   %-22s %8.0f cycles per tile  %5.1f %%\n", names[i], sum[i] / std::max(1.0, sum[8]), 100.0 * sum[i] / tot);
    fprintf(stderr, "   per off-diagonal step %.0f cycles\n", sum[1] / std::max(1.0, sum[9]));
  }
  return MIK_OK;
}

// range-aware launch l on lane ln (stream sc): the lists of active K tiles and the tile records / sequences, the contraction of the
// active tiles, sigma^2
static int contract_sparse(mik_handle* h, const Plan& p, const Launch& l, PredictLane& ln, hipStream_t sc) {
  const LaunchEvents& ev = h->pr_launch[(size_t)l.c];
  const int nTb = l.nTb, nIblk = p.nIblk;
  unsigned long long* stats = h->sp_stats.as<unsigned long long>() + 4 * l.c;
  if (p.gathered) {
    hipLaunchKernelGGL(k_sp_lists_g, dim3(nTb), dim3(64), 0, sc, (const unsigned char*)ln.flags.as<unsigned char>(), p.nKt,
                       ln.klist.as<unsigned short>(), ln.kcount.as<int>(), ln.nrows.as<int>(), 1);
    hipLaunchKernelGGL(k_sp_tiles_g<true>, dim3((unsigned)((nTb + SP_GROUP - 1) / SP_GROUP)), dim3(256), 0, sc, (const int*)ln.nrows.as<int>(),
                       (const int*)ln.kcount.as<int>(), (const unsigned short*)ln.klist.as<unsigned short>(), p.nKt, nTb, ln.recs.as<uint4>(),
                       ln.xoff.as<int>(), stats, SP_GROUP, ln.queue.as<unsigned long long>());
  } else {
    hipLaunchKernelGGL(k_sp_lists, dim3(nTb), dim3(64), 0, sc, (const unsigned char*)ln.flags.as<unsigned char>(), p.nK16, nIblk,
                       ln.klist.as<unsigned short>(), ln.kcount.as<int>(), ln.rows.as<unsigned short>(), ln.rstart.as<unsigned short>(),
                       ln.nrows.as<int>());
    hipLaunchKernelGGL(k_sp_tiles, dim3(1), dim3(1024), 0, sc, (const int*)ln.nrows.as<int>(), (const int*)ln.kcount.as<int>(),
                       (const unsigned short*)ln.rstart.as<unsigned short>(), nIblk, nTb, ln.tiles.as<unsigned>(), ln.xoff.as<int>(), stats);
  }
  HIPC(hipEventRecord(ev.lists_end, sc));
  if (!p.gathered) HIPC(hipMemsetAsync(ln.queue.p, 0, 8 * sizeof(unsigned long long), sc));  // (gathered: k_sp_tiles_g zeroes the queues)
  // two lanes: the CONTRACTIONS run one after the other (this one behind the other lane's previous one); what overlaps a contraction is the
  // other lane's candidate / right-hand-side / list kernels in its tail.  Two persistent launches side by side share every CU and mix two
  // tile queues in every XCD's L2: measured 3.5 % slower per pair (profiles/r06_predict_timeline_c5.txt; rounds 4-5 got this order by accident:
  // the queue memset in front of the contraction waited for a free CU).
  if (p.lanes2 && l.c > 0) HIPC(hipStreamWaitEvent(sc, h->pr_launch[(size_t)l.c - 1].contract_end, 0));
  HIPC(hipEventRecord(ev.contract_begin, sc));
  // (2 n_cu persistent blocks: leaving 32 .. 128 of the slots to the other lane's preparation kernels was tried -- they then run beside the
  // contraction at a fraction of the chip -- and measured a tie at 32 and 1 - 3 % slower beyond: profiles/r06_predict_timeline_c5_after.txt)
  const unsigned nb = (unsigned)std::min<long>(2L * h->n_cu, (long)nTb * nIblk);
  if (p.gathered) {
    SpgArgs ga{};
    ga.Ainv = h->T.as<double>();
    ga.lda = p.Mp;
    ga.Bt = ln.Bt.as<double>();
    ga.ldb = p.Mp;
    ga.part = ln.part.as<double>();
    ga.palloc = l.palloc;
    ga.nK16 = p.nKt;
    ga.klist = ln.klist.as<unsigned short>();
    ga.recs = ln.recs.as<uint4>();
    ga.xoff = ln.xoff.as<int>();
    ga.queue = ln.queue.as<unsigned long long>();
    static const bool spg_prof = getenv("MIK_SPG_PROF") && atoi(getenv("MIK_SPG_PROF")) != 0;
    if (spg_prof) MIKC(spg_profile(ga, nb, sc));
    else hipLaunchKernelGGL((k_contract_spg<2, true, true>), dim3(nb), dim3(512), 0, sc, ga);
  } else {
    SpArgs sa{};
    sa.Ainv = h->T.as<double>();
    sa.lda = p.Mp;
    sa.Bt = ln.Bt.as<double>();
    sa.ldb = p.Mp;
    sa.part = ln.part.as<double>();
    sa.palloc = l.palloc;
    sa.kend = p.kend;
    sa.nIblk = nIblk;
    sa.nK16 = p.nK16;
    sa.klist = ln.klist.as<unsigned short>();
    sa.kcount = ln.kcount.as<int>();
    sa.rows = ln.rows.as<unsigned short>();
    sa.rstart = ln.rstart.as<unsigned short>();
    sa.tiles = ln.tiles.as<unsigned>();
    sa.xoff = ln.xoff.as<int>();
    sa.queue = ln.queue.as<unsigned long long>();
    hipLaunchKernelGGL((k_contract_sp<2>), dim3(nb), dim3(512), 0, sc, sa);
  }
  HIPC(hipEventRecord(ev.contract_end, sc));
  hipLaunchKernelGGL(k_ss_reduce_sp, dim3((l.nvalid + 255) / 256), dim3(256), 0, sc, (const double*)ln.part.as<double>(), l.palloc,
                     (const int*)ln.nrows.as<int>(), l.nvalid, 2.0 * (h->v.p0 + h->v.p2),
                     p.perm ? h->ss.as<double>() : h->ss.as<double>() + l.t0, p.perm ? p.perm + l.t0 : (const unsigned*)nullptr);
  if (p.lanes2 && (l.c & 1)) HIPC(hipEventRecord(h->ev_lane1, sc));  // lane 1's latest launch (joined at the end of the predict)
  return MIK_OK;
}

// launch l's z and sigma^2, and z of fields 1 .. nf - 1, leave for the page-locked landing zones while the next launch is computed (on
// stream_d2h, behind ev_chunk on the launch's stream st)
static int copy_out(mik_handle* h, const Plan& p, const Launch& l, hipStream_t st) {
  const size_t bytes = sizeof(double) * l.nvalid;
  HIPC(hipEventRecord(h->ev_chunk, st));
  HIPC(hipStreamWaitEvent(h->stream_d2h, h->ev_chunk, 0));
  HIPC(hipMemcpyAsync(h->pin_out.as<double>() + l.t0, h->z.as<double>() + l.t0, bytes, hipMemcpyDeviceToHost, h->stream_d2h));
  HIPC(hipMemcpyAsync(h->pin_out.as<double>() + p.npt + l.t0, h->ss.as<double>() + l.t0, bytes, hipMemcpyDeviceToHost, h->stream_d2h));
  for (int f = 1; f < p.nf; ++f)
    HIPC(hipMemcpyAsync(h->pin_fz.as<double>() + (size_t)(f - 1) * p.npt + l.t0, h->zf.as<double>() + (size_t)(f - 1) * p.npt + l.t0, bytes,
                        hipMemcpyDeviceToHost, h->stream_d2h));
  for (int q = 0; q < (p.gaps ? p.gap_np : 0); ++q)
    HIPC(hipMemcpyAsync(h->pin_gss.as<double>() + (size_t)q * p.npt + l.t0, h->gap_ss.as<double>() + (size_t)q * p.npt + l.t0, bytes,
                        hipMemcpyDeviceToHost, h->stream_d2h));
  return MIK_OK;
}

// after the handle's stream has finished: the event-timed durations, the range-aware path's tile counts, the executed flops
static int read_back(mik_handle* h, const Plan& p, bool sorted_now) {
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, h->ev_predict0, h->ev_predict1));
  h->tm.predict_ms = ms;
  if (sorted_now) {
    HIPC(hipEventElapsedTime(&ms, h->ev_predict0, h->ev_sort));
    h->tm.sort_points_ms = ms;
  }
  std::vector<unsigned long long> sp(p.sparse ? 4 * (size_t)p.nchunks : 0);
  if (p.sparse) HIPC(hipMemcpy(sp.data(), h->sp_stats.p, sizeof(unsigned long long) * sp.size(), hipMemcpyDeviceToHost));
  // dense: executed flops of a launch: per tile 2*128*128*(k extent)
  // (triangular diagonal blocks: nt (nt + 1) / 2 products of 16 rows x 16 k instead of 8 nt, nt = K tiles of the block)
  const bool tri = h->opt_sym && h->opt_tri;
  double kext = 0.0;
  for (int ib = 0; ib < p.nIblk; ++ib) {
    const int ext = h->opt_sym ? std::max(0, p.kend - ib * 128) : p.kend;
    if (tri) {
      const int nt = std::min(ext, 128) / 16;
      kext += (ext - 16 * nt) + 16.0 * (nt * (nt + 1) / 2) / 8.0;
    } else kext += ext;
  }
  const int ntl = (p.kend - (p.nIblk - 1) * 128) / 16;  // K tiles of the (short) last block
  for (long c = 0; c < p.nchunks; ++c) {
    const LaunchEvents& ev = h->pr_launch[(size_t)c];
    const int nTb = Launch(p, c).nTb;
    HIPC(hipEventElapsedTime(&ms, ev.rhs_begin, ev.rhs_end));
    h->tm.rhs_ms += ms;
    HIPC(hipEventElapsedTime(&ms, ev.contract_begin, ev.contract_end));
    h->tm.contract_ms += ms;
    if (!p.sparse) {
      h->tm.contract_flops_executed += 2.0 * 128.0 * 128.0 * kext * nTb;
      continue;
    }
    HIPC(hipEventElapsedTime(&ms, ev.cand_begin, ev.rhs_begin));
    h->tm.sparse_lists_ms += ms;
    HIPC(hipEventElapsedTime(&ms, ev.rhs_end, ev.lists_end));
    h->tm.sparse_lists_ms += ms;
    h->tm.sparse_tiles_dense += (double)nTb * p.nIblk;
    h->tm.sparse_ktiles_dense += (double)nTb * (p.kend / 16.0) * (p.nIblk - 1) / 2.0;  // off-diagonal K tiles of the dense symmetric form (about)
    const double tiles = (double)sp[4 * c], offk = (double)sp[4 * c + 1];
    h->tm.sparse_tiles += tiles;
    h->tm.sparse_ktiles += offk;
    // executed flops: off-diagonal K tiles are 128 x 16 x 128 products; a diagonal block is nt (nt + 1) / 2 products of 16 rows x 16 k
    // x 128 points (nt = 8, or the short last block's -- every point block has that row block: the last row is the 1 of ok.py:673;
    // gathered groups: k_sp_tiles_g counted the products of the triangular parts, short last tiles included)
    const double diagp = p.gathered ? (double)sp[4 * c + 2] : 36.0 * std::max(0.0, tiles - (double)nTb) + (ntl * (ntl + 1) / 2) * (double)nTb;
    h->tm.sparse_diag_products += diagp;
    h->tm.contract_flops_executed += 2.0 * 128.0 * 16.0 * 128.0 * offk + 2.0 * 16.0 * 16.0 * 128.0 * diagp;
  }
  h->tm.contract_launches = p.nchunks;
  return MIK_OK;
}

// The error covariance of a predict whose launches have filled the panel of all points (mik_k_cov.h), on the handle's stream behind the
// last launch: stage 0 (-gamma* above the diagonal), stage 1 (Yt = Bt_all B^T), stage 2 (the upper block triangle, mirrored; the diagonal
// from sigma^2), then the P x P corner of C leaves row block by row block through two page-locked pieces of about 32 MB: piece i + 1 is
// on its way while the host copies piece i into the caller's array.  MIK_COV_PROF=1 prints the event-timed stages to stderr.
static int cov_stages(mik_handle* h, const Plan& p, long Pp, double* Yt, double* C, double* cov_out) {
  static const bool prof = getenv("MIK_COV_PROF") && atoi(getenv("MIK_COV_PROF")) != 0;
  const long P = h->npt;
  hipStream_t st = h->stream;
  for (hipEvent_t& e : h->ev_cov)
    if (!e) HIPC(hipEventCreate(&e));
  PredictLane& ln = h->lane[0];
  const int nPblk = (int)(Pp / 128);
  HIPC(hipEventRecord(h->ev_cov[0], st));
  CovGammaArgs g{};
  g.px = h->px.as<double>(), g.py = h->py.as<double>(), g.pz = h->ndim == 3 ? h->pz.as<double>() : nullptr;
  g.npt = P, g.v = h->v, g.eps = h->eps, g.C = C, g.ldc = Pp;
  const dim3 ggrid((unsigned)P, (unsigned)((P + 255) / 256)), gblock(256);
  DISPATCH_MODEL_NDIM(h->model, h->geo ? 1 : h->ndim, k_cov_gamma, ggrid, gblock, st, g);
  HIPC(hipEventRecord(h->ev_cov[1], st));
  CovGemmArgs a{};
  a.Bt = p.panel, a.T = h->T.as<double>(), a.Yt = Yt, a.ld = p.Mp, a.C = C, a.ldc = Pp, a.ss = h->ss.as<double>(), a.npt = P;
  a.nPblk = nPblk, a.nIblk = p.nIblk, a.kend = p.kend, a.queue = ln.queue.as<unsigned long long>();
  HIPC(hipMemsetAsync(ln.queue.p, 0, 8 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL((k_cov_gemm<2, 1>), dim3((unsigned)std::min<long>(2L * h->n_cu, super_grid(nPblk, p.nIblk))), dim3(512), 0, st, a);
  HIPC(hipEventRecord(h->ev_cov[2], st));
  HIPC(hipMemsetAsync(ln.queue.p, 0, 8 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL((k_cov_gemm<2, 2>), dim3((unsigned)std::min<long>(2L * h->n_cu, super_grid(nPblk, nPblk))), dim3(512), 0, st, a);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(h->ev_cov[3], st));
  const long rb = std::min<long>(Pp, std::max<long>(128, (((32L << 20) / (8 * P)) / 128) * 128));  // rows per piece
  MIKC(h->pin_cov.ensure(sizeof(double) * 2 * (size_t)rb * (size_t)P));
  const long npiece = (P + rb - 1) / rb;
  if (prof) HIPC(hipEventSynchronize(h->ev_cov[3]));  // (the copy's time alone)
  const auto t0 = std::chrono::steady_clock::now();
  for (long i = 0; i <= npiece; ++i) {
    if (i < npiece) {
      const long r0 = i * rb, rows = std::min(rb, P - r0);
      HIPC(hipMemcpy2DAsync(h->pin_cov.as<double>() + (size_t)(i & 1) * rb * P, sizeof(double) * P, C + (size_t)r0 * Pp, sizeof(double) * Pp,
                            sizeof(double) * P, (size_t)rows, hipMemcpyDeviceToHost, st));
      HIPC(hipEventRecord(h->ev_cov[4 + (i & 1)], st));
    }
    if (i > 0) {
      const long j = i - 1, r0 = j * rb, rows = std::min(rb, P - r0);
      HIPC(hipEventSynchronize(h->ev_cov[4 + (j & 1)]));
      host_copy(cov_out + (size_t)r0 * P, h->pin_cov.as<double>() + (size_t)(j & 1) * rb * P, sizeof(double) * (size_t)rows * (size_t)P);
    }
  }
  if (prof) {
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    HIPC(hipEventElapsedTime(&m0, h->ev_cov[0], h->ev_cov[1]));
    HIPC(hipEventElapsedTime(&m1, h->ev_cov[1], h->ev_cov[2]));
    HIPC(hipEventElapsedTime(&m2, h->ev_cov[2], h->ev_cov[3]));
    const double mc = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "mik_predict_cov: P %ld Pp %ld Mp %d kend %d stage0_ms %.4f stage1_ms %.4f stage2_ms %.4f copy_ms %.4f\n", P, Pp, p.Mp, p.kend,
            m0, m1, m2, mc);
  }
  return MIK_OK;
}

// What a predict of the resident points starts with (who: the entry point, for the messages): the state checks, the device, the timing
// fields of a fresh run, no planes of gappy fields.  *empty: there are no points -- the (empty) results are there and the caller returns.
static int predict_prologue(mik_handle* h, const char* who, bool* empty) {
  if (!h || !h->have_factor) return fail(MIK_ESTATE, std::string(who) + ": factor first");
  if (!h->have_points) return fail(MIK_ESTATE, std::string(who) + ": set points first");
  HIPC(hipSetDevice(h->device));
  reset_predict_timing(h);
  h->tm.symmetric = h->opt_sym;
  h->tm.engine = 0;  // (the v_fma_f64 contraction left the library in round 6: tools/kernel_bench)
  h->tm.mw_kernel = 0;
  h->nf_done = h->nf;
  h->gap_plane.clear();
  *empty = h->npt == 0;
  if (*empty) h->have_results = true;
  return MIK_OK;
}

// cov_out != nullptr: the predict with the error covariance (one_predict_cov; mik_k_cov.h)
static int predict_body(mik_handle* h, double* cov_out) {
  bool empty = false;
  MIKC(predict_prologue(h, "mik_predict", &empty));
  if (empty) return MIK_OK;
  Plan p{};
  MIKC(plan_predict(h, p, cov_out != nullptr));
  const long Pp = ((h->npt + 127) / 128) * 128;
  DevBuf cov_bt, cov_yt, cov_c, cov_z;  // Bt_all and Yt (Pp x Mp), C (Pp x Pp): this call's, freed after the stream has drained
  if (cov_out) {
    MIKC(cov_bt.ensure(sizeof(double) * (size_t)Pp * (size_t)p.Mp));
    MIKC(cov_yt.ensure(sizeof(double) * (size_t)Pp * (size_t)p.Mp));
    MIKC(cov_c.ensure(sizeof(double) * (size_t)Pp * (size_t)Pp));
    if (!p.sparse) p.panel = cov_bt.as<double>();
  }
  HIPC(hipStreamWaitEvent(h->stream, h->ev_d2h, 0));  // an earlier predict's result copies still read z / ss
  if (p.sparse && h->geo) MIKC(geo_point_vectors(h));  // what the candidate boxes of a geographic problem are built from
  // C of the fields first: the second lane starts at ev_predict0, and every k_rhs reads C
  if (p.nf > 0) MIKC(fields_coefficients(h));
  HIPC(hipEventRecord(h->ev_predict0, h->stream));
  if (p.gaps) MIKC(gaps_setup(h, p));
  bool sorted_now = false;
  if (p.sortpts && !(h->ps_valid && h->ps_chunk == p.chunk)) {
    MIKC(sort_points(h, p.chunk, p.nchunks));
    HIPC(hipEventRecord(h->ev_sort, h->stream));
    sorted_now = true;
  }
  if (p.sortpts) p.perm = h->ps_idx[0].as<unsigned>();
  if (p.lanes2) HIPC(hipStreamWaitEvent(h->stream2, h->ev_predict0, 0));
  if (p.lanes2 && sorted_now) HIPC(hipStreamWaitEvent(h->stream2, h->ev_sort, 0));
  for (long c = 0; c < p.nchunks; ++c) {
    const Launch l(p, c);
    const int L = p.lanes2 ? (int)(c & 1) : 0;  // lane 0 on the handle's stream, lane 1 on stream2
    hipStream_t st = L ? h->stream2 : h->stream;
    MIKC(launch_rhs(h, p, l, h->lane[L], st));
    MIKC(p.sparse ? contract_sparse(h, p, l, h->lane[L], st) : contract_dense(h, p, l));
    MIKC(copy_out(h, p, l, st));
  }
  HIPC(hipGetLastError());
  if (p.lanes2) HIPC(hipStreamWaitEvent(h->stream, h->ev_lane1, 0));  // the handle's stream ends behind both lanes
  HIPC(hipEventRecord(h->ev_predict1, h->stream));
  HIPC(hipEventRecord(h->ev_d2h, h->stream_d2h));
  if (cov_out && p.sparse) {
    // The range-aware predict has run as always -- z and sigma^2 are mik_predict's bits -- but its panels hold delta on the candidate tiles
    // only: the right-hand sides of all points are written by one more dense k_rhs pass (its z, the dense path's rounding of the same
    // number, goes to a scratch plane).
    MIKC(cov_z.ensure(sizeof(double) * (size_t)Pp));
    Plan d = p;
    d.sparse = d.gathered = d.sortpts = d.lanes2 = false;
    d.perm = nullptr, d.nf = 0, d.panel = cov_bt.as<double>();
    for (long c = 0; c < d.nchunks; ++c) MIKC(launch_rhs(h, d, Launch(d, c), h->lane[0], h->stream, cov_z.as<double>()));
    p.panel = d.panel;
  }
  if (cov_out) MIKC(cov_stages(h, p, Pp, cov_yt.as<double>(), cov_c.as<double>(), cov_out));
  HIPC(hipStreamSynchronize(h->stream));
  MIKC(read_back(h, p, sorted_now));
  h->have_results = true;
  return MIK_OK;
}

int one_predict(mik_handle* h) { return predict_body(h, nullptr); }

int one_predict_cov(mik_handle* h, double* cov_out) { return predict_body(h, cov_out); }

// ------------------------------------------------------------------------------------------------------------------------------------
// Block kriging (mik_predict_block; mik_k_block.h).  A path of its own beside predict_body: the plan, the dense contraction, the copies
// and the timing are the point predict's functions, called as they are; the right-hand sides (bbar), gbar and the pass that subtracts
// it are the block's.
#include "mik_k_block.h"

// the six named models x NDIM 2 / 3 -- no geographic form, no custom variogram (DISPATCH_MODEL_NDIM would instantiate those as well)
#define DISPATCH_BLOCK_NDIM(model, NDIM, KERNEL, grid, block, stream, args)                          \
  switch (model) {                                                                                   \
    case 0: hipLaunchKernelGGL((KERNEL<0, NDIM>), grid, block, 0, stream, args); break;              \
    case 1: hipLaunchKernelGGL((KERNEL<1, NDIM>), grid, block, 0, stream, args); break;              \
    case 2: hipLaunchKernelGGL((KERNEL<2, NDIM>), grid, block, 0, stream, args); break;              \
    case 3: hipLaunchKernelGGL((KERNEL<3, NDIM>), grid, block, 0, stream, args); break;              \
    case 4: hipLaunchKernelGGL((KERNEL<4, NDIM>), grid, block, 0, stream, args); break;              \
    default: hipLaunchKernelGGL((KERNEL<5, NDIM>), grid, block, 0, stream, args); break;             \
  }
#define DISPATCH_BLOCK(model, ndim, KERNEL, grid, block, stream, args)                               \
  do {                                                                                               \
    if ((ndim) == 3) { DISPATCH_BLOCK_NDIM(model, 3, KERNEL, grid, block, stream, args) }            \
    else { DISPATCH_BLOCK_NDIM(model, 2, KERNEL, grid, block, stream, args) }                        \
  } while (0)

// bbar of launch l into lane 0's panel on the handle's stream, with z (the dense branch of launch_rhs with the node offsets)
static int launch_rhs_block(mik_handle* h, const Plan& p, const Launch& l, const double* off, int nd) {
  const LaunchEvents& ev = h->pr_launch[(size_t)l.c];
  const long t0 = l.t0;
  hipStream_t st = h->stream;
  BlockRhsArgs ba{};
  RhsArgs& a = ba.r;
  a = rhs_args(h, p, l);
  a.Bt = h->lane[0].Bt.as<double>();
  a.cvec = h->cvec.as<double>();  // (no fields; no candidate tiles and no point order: the dense path)
  a.zout = h->z.as<double>() + t0;
  ba.off = off, ba.nd = nd;
  const dim3 grid(l.palloc / MIK_TP), block(256);
  HIPC(hipEventRecord(ev.rhs_begin, st));
  DISPATCH_BLOCK(h->model, h->ndim, k_rhs_block, grid, block, st, ba);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(ev.rhs_end, st));
  return MIK_OK;
}

// gbar does not depend on the block: once per call, one workgroup (also mik_predict_block_window's, mik_mw.hip)
int launch_block_gamma(mik_handle* h, const double* off, int nd, double* gbar) {
  BlockGammaArgs g{};
  g.off = off, g.nd = nd, g.v = h->v, g.eps = h->eps, g.gbar = gbar;
  DISPATCH_BLOCK(h->model, h->ndim, k_block_gamma, dim3(1), dim3(256), h->stream, g);
  HIPC(hipGetLastError());
  return MIK_OK;
}

// ss[0 .. n) -= gbar; k_block_ss counts in int, so a longer range goes in pieces
int launch_block_ss(mik_handle* h, double* ss, long n, const double* gbar) {
  const long piece = 1L << 30;
  for (long t0 = 0; t0 < n; t0 += piece) {
    const int m = (int)std::min(piece, n - t0);
    hipLaunchKernelGGL(k_block_ss, dim3((m + 255) / 256), dim3(256), 0, h->stream, ss + t0, m, gbar);
  }
  HIPC(hipGetLastError());
  return MIK_OK;
}

int one_predict_block(mik_handle* h, const double* offsets, int nd) {
  bool empty = false;
  MIKC(predict_prologue(h, "mik_predict_block", &empty));
  if (empty) return MIK_OK;
  Plan p{};
  MIKC(plan_predict(h, p, false));
  // always the dense path, also on a factor in Hilbert-curve order (as the gaps predict): sigma^2 = 2 s - delta^T A_inv delta is an
  // identity of one point's right-hand side, not of a mean of them.  The lane's panel, partial sums and queue are sized either way.
  p.sparse = p.gathered = p.sortpts = p.lanes2 = false;
  p.perm = nullptr;
  h->tm.sparse = h->tm.sparse_ktile = h->tm.sparse_rows = h->tm.points_sorted = 0;
  const size_t noff = (size_t)nd * (size_t)h->ndim;
  DevBuf blk;  // the node offsets and, behind them, gbar: this call's, freed after the stream has drained
  MIKC(blk.ensure(sizeof(double) * (noff + 1)));
  HIPC(hipMemcpy(blk.p, offsets, sizeof(double) * noff, hipMemcpyHostToDevice));
  const double* off = blk.as<double>();
  double* gbar = blk.as<double>() + noff;
  HIPC(hipStreamWaitEvent(h->stream, h->ev_d2h, 0));  // an earlier predict's result copies still read z / ss
  HIPC(hipEventRecord(h->ev_predict0, h->stream));
  MIKC(launch_block_gamma(h, off, nd, gbar));
  for (long c = 0; c < p.nchunks; ++c) {
    const Launch l(p, c);
    MIKC(launch_rhs_block(h, p, l, off, nd));
    MIKC(contract_dense(h, p, l));
    MIKC(launch_block_ss(h, h->ss.as<double>() + l.t0, l.nvalid, gbar));
    MIKC(copy_out(h, p, l, h->stream));
  }
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(h->ev_predict1, h->stream));
  HIPC(hipEventRecord(h->ev_d2h, h->stream_d2h));
  HIPC(hipStreamSynchronize(h->stream));
  MIKC(read_back(h, p, false));
  h->have_results = true;
  return MIK_OK;
}
