/* mikgrad.h -- C ABI of libmikgrad.so: the Gaussian ML / REML objective of a variogram model and its analytic gradient on one AMD GPU
 * (gfx950).
 *
 * A fifth library beside libmikrige.so (include/mikrige.h), libmikvario.so (include/mikvario.h), libmikvario3.so (include/mikvario3.h)
 * and libmiklik.so (include/miklik.h).  It links nothing of the first three and keeps no state; it compiles the elimination kernels of the
 * fourth (csrc/mik_k_lik.h, unchanged) into itself and runs them on a larger square.  The one call is stateless like mlk_gram: it selects
 * `device`, uploads, runs, copies back and frees.  Arrays are host pointers to float64, row-major.  Returns MLG_OK or a negative code;
 * mlg_last_error() holds the text (per thread).
 *
 * Definitions.  C, gamma, d_ij, logdet and G = W^T C^-1 W of W = [V | X] are those of include/miklik.h, and the two results are
 * mlk_gram's bit for bit on the same inputs.  With Q = C^-1, G_xx = X^T Q X, P = Q - Q X G_xx^-1 X^T Q and, for field f with values v_f,
 * a_f = P v_f, the derivative of the objective of field f (likelihood.nll_from_gram) with respect to a parameter theta_k of C is
 *   grad[f][k] = 1/2 S_k - 1/2 T_kf,  S_k = sum_ij M_ij D_k,ij,  T_kf = sum_ij a_if a_jf D_k,ij,  D_k = dC / dtheta_k,
 *   M = P under REML (reml = 1) and M = Q under ML (reml = 0); X is held fixed.
 * k runs over: 0 the partial sill, 1 the range, 2 the nugget, 3 .. 3 + ng - 1 the geometry parameters.
 *
 * The derivative matrices, in float64, operation for operation without contraction into fused multiply-adds.  For a pair i != j:
 *   h = x_i - x_j per axis (the adjusted coordinates `coords`), d = sqrt(hx*hx + hy*hy (+ hz*hz)), as in miklik.h;
 *   for geometry set g, e = dcoords_g,i - dcoords_g,j per axis and w_g = hx*ex + hy*ey (+ hz*ez).
 *   Three factors of the model at d:  c_p = 1 - f(d)  with gamma = psill f(d) + nugget;  c_r = -psill df/drange;
 *   c_g = -psill f'(d) / d, defined as 0 where d = 0 (there w_g is 0 as well: both vectors are linear in the same raw difference).
 *     gaussian     s = range 4/7, E = exp(-(d*d) / (s*s)):  c_p = E;  c_r = psill * E * ((2 (d*d)) / ((s*s) * range));
 *                  c_g = -(psill * E * (2 / (s*s)))
 *     exponential  s = range / 3, E = exp(-d / s):  c_p = E;  c_r = psill * E * (d / (s * range));  c_g = -((psill * E / s) / d)
 *     spherical    for d <= range:  c_p = 1 - ((3 d) / (2 range) - d^3 / (2 range^3));
 *                  c_r = psill * ((3 d) / (2 range^2) - (3 d^3) / (2 range^4));
 *                  c_g = -((psill * (3 / (2 range) - (3 (d*d)) / (2 range^3))) / d);
 *                  beyond the range every derivative is exactly 0 (f' is continuous there: f'(range) = 0)
 *     hole-effect  q = d / (range / 3), E = exp(-q):  c_p = (1 - q) * E;  c_r = psill * (((2 - q) * E * q) / range);
 *                  c_g = -((psill * ((2 - q) * E / (range / 3))) / d)
 *   dC_ij / dpsill = c_p,  dC_ij / drange = c_r,  dC_ij / dnugget = 0,  dC_ij / dtheta_g = c_g * w_g.
 * On the diagonal dC_ii / dpsill = 1, dC_ii / dnugget = 1 (dC / dnugget = I: the diagonal only) and every other derivative is 0.  The
 * formulas are applied at d = 0 too: two coincident distinct stations keep C_ij = psill, so c_p = 1 and c_r = 0 there.
 *
 * If a pivot of C is <= 0 or not finite the call returns MLG_ENOTPD with the column (1-based) in *info, launches nothing further and
 * writes no result, as mlk_gram does; if G_xx is not positive definite in float64 it returns MLG_ENOTPD with *info = n + the column of
 * G_xx (1-based).  Every sum has a fixed order and nothing is accumulated by atomics: two calls return the same bits, and row f of grad
 * depends only on field f, not on the fields beside it.
 */
#ifndef MIKGRAD_H
#define MIKGRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLG_ABI_VERSION 1

#define MLG_OK 0
#define MLG_EINVAL (-1) /* an argument outside what is documented here; nothing was launched */
#define MLG_ENOTPD (-2) /* C (or X^T C^-1 X) is not positive definite in float64: *info holds the column of the pivot that failed */
#define MLG_EHIP (-3)   /* a HIP call failed (no device among them) */

#define MLG_MAXFIELDS 32 /* rows of V */
#define MLG_MAXTREND 8   /* rows of X */
#define MLG_MAXGEOM 5    /* geometry parameters: 2 in the plane (scaling, angle), 5 in space */

/* models: the numbers of miklik.h */
#define MLG_GAUSSIAN 0
#define MLG_EXPONENTIAL 1
#define MLG_SPHERICAL 2
#define MLG_HOLE_EFFECT 3

/* n: 2 <= n; (2n + 48)^2 * 8 bytes must not pass a quarter of the device's memory (MLG_EINVAL otherwise): the call holds the lower
 * triangle of the (2n + mpad) x (2n + mpad) matrix [[C, ., .], [W^T, 0, .], [I, 0, 0]], mpad = F + p rounded up to 16, as a full square.
 * Eliminated over its first n columns the trailing block ends as -G in (W, W), -C^-1 W in (I, W) and -C^-1 in (I, I). */

int mlg_abi_version(void);
const char *mlg_last_error(void);

/* logdet, G ((F + p) x (F + p)) and grad (F x (3 + ng)).  Inputs must be finite; ndim 2 or 3; 0 <= ng <= MLG_MAXGEOM; psill > 0,
 * range > 0, nugget >= 0; 1 <= F <= MLG_MAXFIELDS; 1 <= p <= MLG_MAXTREND; reml 0 or 1.  dcoords may be NULL when ng = 0.
 * *info: 0, or with MLG_ENOTPD the 1-based column of the failed pivot. */
int mlg_grad(int device, int64_t n, int32_t ndim, const double *coords /* ndim x n */, int32_t ng,
             const double *dcoords /* ng x ndim x n */, int32_t model, double psill, double range, double nugget,
             const double *V /* F x n */, int32_t F, const double *X /* p x n */, int32_t p, int32_t reml, double *logdet,
             double *G /* (F + p) x (F + p) */, double *grad /* F x (3 + ng) */, int32_t *info);

#ifdef __cplusplus
}
#endif
#endif
