/* mikvario3.h -- C ABI of libmikvario3.so: directional semivariograms and variogram maps of 3-D station sets on one AMD GPU (gfx950).
 *
 * A third library beside libmikrige.so (include/mikrige.h) and libmikvario.so (include/mikvario.h, the 2-D tool), with no code or state
 * in common with either: coordinates and values go in, bins come out.  Every call is stateless like mkv_directional: it selects
 * `device`, uploads, runs, copies back and frees.  Arrays are host pointers to float64 / int64, row-major.  Returns MKV3_OK or a negative
 * code; mkv3_last_error() holds the text (per thread).
 *
 * For a pair i < j of the caller's station order: dx = x[j] - x[i], dy = y[j] - y[i], dz = z[j] - z[i],
 * d = sqrt(dx*dx + dy*dy + dz*dz), g_f = 0.5 (v_f[i] - v_f[j])^2.  The device evaluates every expression here operation for operation,
 * left to right, without contraction into fused multiply-adds.
 *   lag bin b:    edges[b] <= d < edges[b+1]; a pair outside every bin is dropped (the rule of mkv_directional, bisection included)
 *   direction a:  a unit vector u_a = (ux, uy, uz) = dirs[3a .. 3a+2], axial (u and -u are the same direction);
 *                 along = dx*ux + dy*uy + dz*uz;  c = h x u:  cx = dy*uz - dz*uy, cy = dz*ux - dx*uz, cz = dx*uy - dy*ux;
 *                 across2 = cx*cx + cy*cy + cz*cz;
 *                 the pair belongs to a if across2 <= (along*along) * tan2 (tol_deg == 90: always) and, with a bandwidth > 0,
 *                 across2 <= bw2.  tan2 = tan(tol_deg * (pi / 180))^2 and bw2 = bandwidth^2 are formed once on the host (the C library's
 *                 tan; one multiplication each).  The cross product avoids the cancellation of d^2 - along^2, and the squares save one
 *                 float64 square root per pair and direction.
 *                 A pair may belong to several directions; a coincident pair (d == 0) belongs to all of them.
 *                 From an azimuth (degrees counter-clockwise from +x in the x-y plane, the 2-D tool's convention) and a dip (degrees
 *                 upward from that plane toward +z, in [-90, 90]):  u = (cos(dip) cos(az), cos(dip) sin(az), sin(dip)) -- formed by the
 *                 caller; the unit vector is what crosses this boundary.
 *   map cell:     ix = nx + floor(dx / cell_dx + 0.5), iy = ny + floor(dy / cell_dy + 0.5), iz = nz + floor(dz / cell_dz + 0.5); the pair
 *                 falls into (iz, iy, ix) and into the mirror cell (2 nz - iz, 2 ny - iy, 2 nx - ix) of -h, or is dropped when outside the
 *                 map.  A coincident pair counts twice in the centre cell.  One half of the map is accumulated and the host writes both
 *                 halves from it: mirrored cells hold the same bits by construction.
 * Counts are exact.  The floating sums are accumulated in float64 in an order that may differ from run to run.
 */
#ifndef MIKVARIO3_H
#define MIKVARIO3_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKV3_ABI_VERSION 1

#define MKV3_OK 0
#define MKV3_EINVAL (-1) /* an argument outside what is documented here; nothing was launched */
#define MKV3_EHIP (-3)   /* a HIP call failed (no device among them) */

/* limits; anything beyond one of them is MKV3_EINVAL */
#define MKV3_MAXLAGS 64    /* lag bins of mkv3_directional */
#define MKV3_MAXDIRS 16    /* directions of one mkv3_directional call */
#define MKV3_MAXCELLS 4225 /* cells (2 nz + 1)(2 ny + 1)(2 nx + 1) of mkv3_map: a workgroup keeps the count and eight field sums of one
                              half of the map, 2113 cells x 68 bytes = 143 684 bytes, in LDS beside its station tiles (6 x 64 coordinates
                              + 2 x 8 x 64 values = 11 264 bytes): 154 948 of 163 840 bytes */
#define MKV3_FCHUNK 8      /* fields binned by one pass over the pairs (any nf >= 1 is accepted: ceil(nf / 8) passes) */
#define MKV3_UNIT_TOL 1e-12 /* a direction whose Euclidean norm differs from 1 by more than this is refused */
/* n: 2 <= n < 2^31 */

int mkv3_abi_version(void);
const char *mkv3_last_error(void);

/* Directional semivariogram sums of nf fields over one 3-D station set.  Inputs must be finite; edges ascending (strictly), 1 <= nlags <=
 * MKV3_MAXLAGS, 1 <= na <= MKV3_MAXDIRS, every direction a unit vector, 0 < tol_deg <= 90, bandwidth <= 0 = none.  Outputs: count[a][b]
 * pairs of direction a in bin b, lag_sum[a][b] the sum of their d, semi_sum[f][a][b] the sum of their g_f. */
int mkv3_directional(int device, int64_t n, const double *x, const double *y, const double *z,
                     const double *values /* nf x n, field-major */, int32_t nf,
                     const double *dirs /* na x 3 unit vectors */, int32_t na, double tol_deg, double bandwidth /* <= 0: none */,
                     const double *edges /* nlags + 1, ascending */, int32_t nlags,
                     double *lag_sum /* na x nlags */, double *semi_sum /* nf x na x nlags */, int64_t *count /* na x nlags */);

/* Variogram map of nf fields: (2 nz + 1) x (2 ny + 1) x (2 nx + 1) cells of dx x dy x dz centred on lag zero; nx, ny, nz >= 0, dx, dy,
 * dz > 0 and finite, (2 nz + 1)(2 ny + 1)(2 nx + 1) <= MKV3_MAXCELLS. */
int mkv3_map(int device, int64_t n, const double *x, const double *y, const double *z, const double *values, int32_t nf,
             int32_t nx, int32_t ny, int32_t nz, double dx, double dy, double dz,
             double *semi_sum /* nf x (2nz+1) x (2ny+1) x (2nx+1) */, int64_t *count /* (2nz+1) x (2ny+1) x (2nx+1) */);

#ifdef __cplusplus
}
#endif
#endif
