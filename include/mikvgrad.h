/* mikvgrad.h -- C ABI of libmikvgrad.so: the pieces of the Gaussian log-likelihood of a variogram model under Vecchia's approximation and
 * their analytic derivatives with respect to the parameters of the covariance, on one AMD GPU (gfx950).
 *
 * A seventh library beside libmikrige.so, libmikvario.so, libmikvario3.so, libmiklik.so, libmikgrad.so and libmikvecchia.so, with no state
 * or symbols in common with any of them.  It compiles the kernels of the sixth (csrc/mik_k_vecchia.h, unchanged) into itself, as
 * libmikgrad.so compiles those of the fourth, and adds two of its own.  A plan keeps the neighbour sets on the device across the calls of
 * a fit.  Arrays are host pointers, float64 unless said otherwise, row-major.  Returns MVG_OK or a negative code; mvg_last_error() holds
 * the text (per thread).
 *
 * Definitions.  Positions, neighbour sets (k_p = min(m, p) nearest predecessors, ascending by (d2, position)), local systems and
 * covariances are those of include/mikvecchia.h; logdet = sum_p log d_p and G_ab = sum_p r_p(a) r_p(b) / d_p come from the same kernels
 * in the same launches and are bit for bit mvc_plan_gram's on the same inputs.
 *   The derivative matrices D_k = dC / dtheta_k are those of include/mikgrad.h: the factors c_p, c_r, c_g of the model at d_ij, w_g of
 *   geometry set g from `coords` and `dcoords`, dC_ij / dpsill = c_p, dC_ij / drange = c_r, dC_ij / dnugget = 0, dC_ij / dtheta_g =
 *   c_g * w_g; on the diagonal 1 for psill and nugget and 0 otherwise; at d = 0 of two distinct stations c_p = 1, c_r = 0 and c_g = 0;
 *   beyond the range every derivative is exactly 0 for the spherical model.  In float64, operation for operation without contraction
 *   into fused multiply-adds.  k runs over: 0 psill, 1 range, 2 nugget, 3 .. 3 + ng - 1 the geometry parameters.
 *   For position p with neighbour list c of length k_p write Sigma = [[S, s], [s^T, sigma]] with sigma = psill + nugget,
 *   beta = S^-1 s, u = [-beta ; 1], d_p = sigma - s^T beta, and for a column w, r_p(w) = u^T [w_c ; w_p].  With S = L L^T,
 *   y = L^-1 s and beta = L^-T y.  For parameter k let D be the local (k_p + 1)^2 block of D_k and t = D u
 *   (t_i = D_ip - sum_j D_ij beta_j, the neighbours j in list order).  Then
 *     d_k d_p = u^T t = t_p - sum_i beta_i t_i,
 *     d_k r_p(w) = -(S^-1 w_c)^T t_c = -(L^-1 w_c)^T (L^-1 t_c).
 *   A position with k_p = 0 has d_k d_p = d_k sigma (1 for psill and nugget, 0 otherwise) and d_k r_p(w) = 0.
 *   Results:
 *     dlogdet[k] = sum_p d_k d_p / d_p
 *     dG[k][a][b] = sum_p [ (d_k r_p(a) r_p(b) + r_p(a) d_k r_p(b)) / d_p - r_p(a) r_p(b) d_k d_p / d_p^2 ],
 *   each term spelled ((dr_a r_b) + (r_a dr_b)) / d - ((r_a r_b) dd) / (d d) in float64 products.  dG[k] is m_cols x m_cols; both
 *   halves are written and it is exactly symmetric.
 *   Failure: if any pivot of a local system is <= 0 or not finite the call returns MVG_ENOTPD and *info holds the 1-based station index of
 *   the earliest such position.  The call writes none of its results, as mvc_plan_gram does.
 *   Reproducibility: every sum has a fixed order that depends on n only, not on the launch geometry or on the slab length; there are no
 *   atomics, and the results are the same bits from run to run.  dG[k][a][b] depends only on columns a and b of W, not on where they
 *   stand in W or on the columns beside them.
 *   Slabs: the per-position derivative rows -- (3 + ng) (m_cols + 1) doubles -- are held for MVG_SLAB positions at a time; a slab is a
 *   whole number of the 1024-position blocks of the reduction, so no partial sum sees the cut.  The environment variable MIK_VGRAD_SLAB,
 *   read by every call, names a shorter slab (positions, rounded up to a multiple of 1024): a knob for the tests.
 */
#ifndef MIKVGRAD_H
#define MIKVGRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVG_ABI_VERSION 1

#define MVG_OK 0
#define MVG_EINVAL (-1) /* an argument outside what is documented here; nothing was launched */
#define MVG_ENOTPD (-2) /* a local system is not positive definite in float64: *info holds the station */
#define MVG_EHIP (-3)   /* a HIP call failed (no device among them) */

#define MVG_MAXNB 64   /* neighbours of a station */
#define MVG_MAXCOLS 40 /* columns of W: 32 fields and 8 trend columns */
#define MVG_MAXGEOM 5  /* geometry parameters: 2 in the plane (scaling, angle), 5 in space */
#define MVG_SLAB 65536 /* positions whose derivative rows are held at a time */

/* models: the numbers of mikvecchia.h */
#define MVG_GAUSSIAN 0
#define MVG_EXPONENTIAL 1
#define MVG_SPHERICAL 2
#define MVG_HOLE_EFFECT 3

typedef struct mvg_plan mvg_plan;

int mvg_abi_version(void);
const char *mvg_last_error(void);

/* mvc_plan_create's arguments, bounds and refusals, and the same neighbour search.  n >= 2; coords finite; order a permutation of
 * 0 .. n - 1; 1 <= m <= MVG_MAXNB.  The footprint of a plan at MVG_MAXCOLS columns and MVG_MAXGEOM geometry sets -- coordinates, order,
 * neighbour lists, W, the residuals, the geometry sets, the partial sums of G and dG per 1024 positions and one slab of derivative rows:
 * n (8 ndim + 4 + 4 m + 8 * 40 + 8 * 42 + 8 * 5 ndim) + ceil(n / 1024) * 8 * 9 * 821 + 65536 * 8 * 8 * 41 bytes -- must not pass a
 * quarter of the device's memory (MVG_EINVAL). */
int mvg_plan_create(int device, int64_t n, int32_t ndim, const double *coords /* ndim x n */, const int32_t *order /* n */, int32_t m,
                    mvg_plan **plan);

/* The neighbour sets: n x m station indices, row = station index, in list order; entries beyond k_p are -1.  The lists of
 * mvc_plan_neighbours for the same inputs. */
int mvg_plan_neighbours(const mvg_plan *plan, int32_t *out /* n x m */);

/* logdet, G, dlogdet and dG.  coords may differ from the plan's: the neighbour sets stay those of the plan's metric.  Inputs must be
 * finite; 0 <= ng <= MVG_MAXGEOM, dcoords may be NULL only when ng = 0; psill > 0, range > 0, nugget >= 0; 1 <= m_cols <= MVG_MAXCOLS.
 * Each call uploads the coordinates, the geometry sets and W (((1 + ng) ndim + m_cols) n 8 bytes) and nothing else.  *info: 0, or with
 * MVG_ENOTPD the 1-based station index. */
int mvg_plan_grad(mvg_plan *plan, const double *coords /* ndim x n */, int32_t ng, const double *dcoords /* ng x ndim x n */, int32_t model,
                  double psill, double range, double nugget, const double *W /* m_cols x n, one column per row */, int32_t m_cols,
                  double *logdet, double *G /* m_cols x m_cols */, double *dlogdet /* 3 + ng */,
                  double *dG /* (3 + ng) x m_cols x m_cols */, int32_t *info);

void mvg_plan_destroy(mvg_plan *plan);

#ifdef __cplusplus
}
#endif
#endif
