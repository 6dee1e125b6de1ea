/* miklik.h -- C ABI of libmiklik.so: the pieces of the Gaussian log-likelihood of a variogram model on one AMD GPU (gfx950).
 *
 * A fourth library beside libmikrige.so (include/mikrige.h), libmikvario.so (include/mikvario.h) and libmikvario3.so
 * (include/mikvario3.h), with no code or state in common with any of them: coordinates, a model and columns go in, log det C and
 * W^T C^-1 W come out.  The one call is stateless like mkv_directional: it selects `device`, uploads, runs, copies back and frees; the
 * Cholesky factor is formed, used and thrown away inside it.  Arrays are host pointers to float64, row-major.  Returns MLK_OK or a
 * negative code; mlk_last_error() holds the text (per thread).
 *
 * Definitions.  For n stations with anisotropy-adjusted Euclidean coordinates and a bounded variogram model gamma with partial sill
 * psill, range and nugget, the covariance matrix C (n x n) is
 *   C_ii = psill + nugget.
 *   For i != j, C_ij = (psill + nugget) - gamma(d_ij).
 *   d_ij is the Euclidean distance, sqrt(dx*dx + dy*dy (+ dz*dz)).
 *   gamma is the model formula of core.variogram_value, evaluated in float64 with the library exp (not the moving window's short
 *   exponential), operation for operation without contraction into fused multiply-adds:
 *     gaussian     psill (1 - exp(-(d*d) / (range 4/7)^2)) + nugget
 *     exponential  psill (1 - exp(-d / (range / 3))) + nugget
 *     spherical    psill ((3 d) / (2 range) - d^3 / (2 range^3)) + nugget  for d <= range,  psill + nugget beyond (C_ij = 0 exactly)
 *     hole-effect  psill (1 - (1 - d / (range / 3)) exp(-d / (range / 3))) + nugget
 *   The formula is applied at d = 0 too: two coincident distinct stations have C_ij = psill -- a nugget is measurement or micro-scale
 *   variance, as everywhere else in this project.
 *   With C = L L^T (L lower triangular): logdet = 2 sum_i log L_ii, and G = W^T C^-1 W (m x m, symmetric, both halves written; the
 *   upper half is a copy of the lower, so G is exactly symmetric).
 *   If a pivot is <= 0 or not finite the call returns MLK_ENOTPD with the column (1-based, LAPACK's convention) in *info; it launches
 *   nothing further and writes neither logdet nor G.  This is an answer, not an error: the likelihood of such a model is zero.
 * logdet and G are reproducible run to run: every sum has a fixed order and nothing is accumulated by atomics.  An entry of G depends
 * only on the two columns of W it is formed from, not on where they stand in W.
 */
#ifndef MIKLIK_H
#define MIKLIK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLK_ABI_VERSION 1

#define MLK_OK 0
#define MLK_EINVAL (-1) /* an argument outside what is documented here; nothing was launched */
#define MLK_ENOTPD (-2) /* C is not positive definite in float64: *info holds the column of the pivot that failed */
#define MLK_EHIP (-3)   /* a HIP call failed (no device among them) */

#define MLK_MAXCOLS 40 /* columns of W: 32 fields and 8 trend columns */

/* models */
#define MLK_GAUSSIAN 0
#define MLK_EXPONENTIAL 1
#define MLK_SPHERICAL 2
#define MLK_HOLE_EFFECT 3

/* n: 2 <= n; (n + 48)^2 * 8 bytes must not pass a quarter of the device's memory (MLK_EINVAL otherwise): the call holds the lower
 * triangle of the (n + mpad) x (n + mpad) matrix [[C, .], [W^T, 0]], mpad = m rounded up to 16, as a full square. */

int mlk_abi_version(void);
const char *mlk_last_error(void);

/* logdet = log det C and G = W^T C^-1 W.  Inputs must be finite; ndim 2 or 3; psill > 0, range > 0, nugget >= 0;
 * 1 <= m <= MLK_MAXCOLS.  *info: 0, or with MLK_ENOTPD the 1-based column of the failed pivot. */
int mlk_gram(int device, int64_t n, int32_t ndim, const double *coords /* ndim x n */, int32_t model, double psill, double range,
             double nugget, const double *W /* m x n, column vectors of C's space, one per row */, int32_t m, double *logdet,
             double *G /* m x m */, int32_t *info);

#ifdef __cplusplus
}
#endif
#endif
