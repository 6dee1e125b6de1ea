/* mikvario.h -- C ABI of libmikvario.so: directional semivariograms and variogram maps on one AMD GPU (gfx950).
 *
 * A second library beside libmikrige.so (include/mikrige.h), with no code or state in common: coordinates and values go in, bins come
 * out.  Every call is stateless like mik_krige_execute: it selects `device`, uploads, runs, copies back and frees.  Arrays are host
 * pointers to float64 / int64, row-major.  Returns MKV_OK or a negative code; mkv_last_error() holds the text (per thread).
 *
 * For a pair i < j of the caller's station order: dx = x[j] - x[i], dy = y[j] - y[i], d = sqrt(dx*dx + dy*dy),
 * g_f = 0.5 (v_f[i] - v_f[j])^2.
 *   lag bin b:    edges[b] <= d < edges[b+1]; a pair outside every bin is dropped
 *   direction a:  theta = azimuth_deg[a], counter-clockwise from +x (the convention of anisotropy_angle), axial (theta = theta + 180);
 *                 along = |dx cos(theta) + dy sin(theta)|, across = |-dx sin(theta) + dy cos(theta)|;
 *                 the pair belongs to a if across <= along * tan(tol) (tol_deg == 90: always) and, with a bandwidth > 0, across <= bandwidth.
 *                 cos, sin and tan are the C library's, of azimuth_deg[a] * (pi / 180) and tol_deg * (pi / 180), evaluated once on the host.
 *                 A pair may belong to several directions; a coincident pair (d == 0) belongs to all of them.
 *   map cell:     ix = nx + floor(dx / cell_dx + 0.5), iy = ny + floor(dy / cell_dy + 0.5); the pair falls into (iy, ix) and into the
 *                 mirror cell (2 ny - iy, 2 nx - ix) of -h, or is dropped when outside the map.  A coincident pair counts twice in the
 *                 centre cell.  The map is exactly point-symmetric, sums included.
 * Counts are exact.  The floating sums are accumulated in float64 in an order that may differ from run to run.
 */
#ifndef MIKVARIO_H
#define MIKVARIO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKV_ABI_VERSION 1

#define MKV_OK 0
#define MKV_EINVAL (-1) /* an argument outside what is documented here; nothing was launched */
#define MKV_EHIP (-3)   /* a HIP call failed (no device among them) */

/* limits; anything beyond one of them is MKV_EINVAL */
#define MKV_MAXLAGS 64    /* lag bins of mkv_directional (= MIK_VG_MAXLAGS of the constructor's semivariogram) */
#define MKV_MAXDIRS 16    /* directions of one mkv_directional call */
#define MKV_MAXCELLS 4225 /* cells (2 ny + 1)(2 nx + 1) of mkv_map, 65 x 65: a workgroup keeps the count and eight field sums of one
                             half of the map, (cells + 1) / 2 x 68 bytes, in the 160 KB of LDS beside its station tiles */
#define MKV_FCHUNK 8      /* fields binned by one pass over the pairs (any nf >= 1 is accepted: ceil(nf / 8) passes) */
/* n: 2 <= n < 2^31 */

int mkv_abi_version(void);
const char *mkv_last_error(void);

/* Directional semivariogram sums of nf fields over one station set.  Inputs must be finite; edges ascending (strictly), 1 <= nlags <=
 * MKV_MAXLAGS, 1 <= na <= MKV_MAXDIRS, 0 < tol_deg <= 90, bandwidth <= 0 = none.  Outputs: count[a][b] pairs of direction a in bin b,
 * lag_sum[a][b] the sum of their d, semi_sum[f][a][b] the sum of their g_f. */
int mkv_directional(int device, int64_t n, const double *x, const double *y,
                    const double *values /* nf x n, field-major */, int32_t nf,
                    const double *azimuth_deg, int32_t na, double tol_deg, double bandwidth /* <= 0: none */,
                    const double *edges /* nlags + 1, ascending */, int32_t nlags,
                    double *lag_sum /* na x nlags */, double *semi_sum /* nf x na x nlags */, int64_t *count /* na x nlags */);

/* Variogram map of nf fields: (2 ny + 1) x (2 nx + 1) cells of dx x dy centred on lag zero; nx, ny >= 0, dx, dy > 0 and finite,
 * (2 ny + 1)(2 nx + 1) <= MKV_MAXCELLS. */
int mkv_map(int device, int64_t n, const double *x, const double *y, const double *values, int32_t nf,
            int32_t nx, int32_t ny, double dx, double dy,
            double *semi_sum /* nf x (2ny+1) x (2nx+1) */, int64_t *count /* (2ny+1) x (2nx+1) */);

#ifdef __cplusplus
}
#endif
#endif
