/* mikvecchia.h -- C ABI of libmikvecchia.so: the pieces of the Gaussian log-likelihood of a variogram model under Vecchia's approximation,
 * on one AMD GPU (gfx950).
 *
 * A sixth library beside libmikrige.so, libmikvario.so, libmikvario3.so, libmiklik.so and libmikgrad.so, with no code or state in common
 * with any of them.  Where miklik.h factors the n x n covariance matrix, this library conditions every station on at most m earlier
 * stations: p(v) ~ prod_i p(v_i | v_c(i)).  That product is the exact density of a Gaussian with a covariance C^ whose precision matrix
 * is sparse; it costs n Cholesky factorisations of size <= m + 1 and equals the exact likelihood for m >= n - 1.  The call returns what
 * mlk_gram returns: log det C^ and W^T C^-1 W.  A plan keeps the neighbour sets on the device (n * m * 4 bytes) across the hundreds of
 * calls of a fit.  Arrays are host pointers, float64 unless said otherwise, row-major.  Returns MVC_OK or a negative code;
 * mvc_last_error() holds the text (per thread).
 *
 * Definitions.
 *   Inputs: n stations with anisotropy-adjusted Euclidean coordinates coords (ndim x n, ndim 2 or 3), a permutation order (the
 *   position p holds station order[p]) and a neighbour bound 1 <= m <= MVC_MAXNB.
 *   Neighbour sets: the station at position p has k_p = min(m, p) neighbours, the k_p predecessors (positions q < p) with the smallest
 *   squared distance d2 = dx*dx + dy*dy in 2-D and (dx*dx + dy*dy) + dz*dz in 3-D, in float64 and unfused.  Ties go to the smaller
 *   position.  The neighbours are listed ascending by (d2, position).
 *   Local system of position p: the stations [its neighbours in list order, the station itself]; the covariances are those of
 *   miklik.h, evaluated in float64 with the library exp, operation for operation without contraction into fused multiply-adds:
 *     C_ii = psill + nugget, and C_ij = (psill + nugget) - gamma(d_ij) also at d = 0, with d_ij = sqrt(d2) and
 *     gaussian     psill (1 - exp(-(d*d) / (range 4/7)^2)) + nugget
 *     exponential  psill (1 - exp(-d / (range / 3))) + nugget
 *     spherical    psill ((3 d) / (2 range) - d^3 / (2 range^3)) + nugget  for d <= range,  psill + nugget beyond (C_ij = 0 exactly)
 *     hole-effect  psill (1 - (1 - d / (range / 3)) exp(-d / (range / 3))) + nugget
 *   The (k_p + 1)^2 matrix is factored by Cholesky.  The last pivot squared is the conditional variance d_p.  For a column w,
 *   forward-substituting the local [w_c ; w_p] leaves the residual r_p(w) = w_p - s^T S^-1 w_c in the last place, before its division.
 *   Results: logdet = sum_p log d_p and G_ab = sum_p r_p(a) r_p(b) / d_p.  G is m_cols x m_cols; both halves are written and it is
 *   exactly symmetric.
 *   Failure: if any pivot of a local system is <= 0 or not finite the call returns MVC_ENOTPD and *info holds the 1-based station index
 *   of the earliest such position.  The call writes neither result.  This is an answer, not an error: the likelihood of such a model
 *   is zero.
 *   Reproducibility: every sum has a fixed order that depends on n only, not on the launch geometry; the results are the same bits from
 *   run to run, and an entry of G depends only on its two columns, not on where they stand in W or on the columns beside them.
 */
#ifndef MIKVECCHIA_H
#define MIKVECCHIA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVC_ABI_VERSION 1

#define MVC_OK 0
#define MVC_EINVAL (-1) /* an argument outside what is documented here; nothing was launched */
#define MVC_ENOTPD (-2) /* a local system is not positive definite in float64: *info holds the station */
#define MVC_EHIP (-3)   /* a HIP call failed (no device among them) */

#define MVC_MAXNB 64   /* neighbours of a station */
#define MVC_MAXCOLS 40 /* columns of W: 32 fields and 8 trend columns */

/* models */
#define MVC_GAUSSIAN 0
#define MVC_EXPONENTIAL 1
#define MVC_SPHERICAL 2
#define MVC_HOLE_EFFECT 3

typedef struct mvc_plan mvc_plan;

int mvc_abi_version(void);
const char *mvc_last_error(void);

/* Uploads the coordinates and the order, finds all neighbour sets on the device and keeps them there.  n >= 2; coords finite; order a
 * permutation of 0 .. n - 1; 1 <= m <= MVC_MAXNB.  The footprint of a plan at MVC_MAXCOLS columns -- coordinates, order, neighbour lists,
 * W and the residuals: n (8 ndim + 4 + 4 m + 8 * 40 + 8 * 42) bytes -- must not pass a quarter of the device's memory (MVC_EINVAL). */
int mvc_plan_create(int device, int64_t n, int32_t ndim, const double *coords /* ndim x n */, const int32_t *order /* n */, int32_t m,
                    mvc_plan **plan);

/* The neighbour sets: n x m station indices, row = station index, in list order; entries beyond k_p are -1. */
int mvc_plan_neighbours(const mvc_plan *plan, int32_t *out /* n x m */);

/* logdet = log det C^ and G = W^T C^-1 W.  coords may differ from the plan's (a search that moves the anisotropy): the neighbour sets stay
 * those of the plan's metric.  Inputs must be finite; psill > 0, range > 0, nugget >= 0; 1 <= m_cols <= MVC_MAXCOLS.  Each call uploads
 * the coordinates and W ((ndim + m_cols) n 8 bytes) and nothing else.  *info: 0, or with MVC_ENOTPD the 1-based station index. */
int mvc_plan_gram(mvc_plan *plan, const double *coords /* ndim x n */, int32_t model, double psill, double range, double nugget,
                  const double *W /* m_cols x n, one column per row */, int32_t m_cols, double *logdet, double *G /* m_cols x m_cols */,
                  int32_t *info);

void mvc_plan_destroy(mvc_plan *plan);

#ifdef __cplusplus
}
#endif
#endif
