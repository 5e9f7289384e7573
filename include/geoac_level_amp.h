/* geoac_level_amp.h - level amplitudes: the geometric spreading of a ray at a receiver altitude, from a finite-difference ray tube.
 *
 * Level crossings, level stations, level refinement and level tube maps (geoac_levels.h, geoac_lstations.h, geoac_level_refine.h,
 * geoac_ltubemap.h) give a receiver above the ground its eigenray's launch angles, travel time, absorption and slowness - and no amplitude,
 * because a path row carries no Jacobian.  This header supplies it without integrating anything new.  The ray-coordinate determinant D of
 * GeoAc_Jacobian, det d(position) / d(s, theta, phi), does not change when multiples of the tangent column are added to the launch-angle
 * columns; adding the multiples that keep the height fixed leaves |t_h| * |det d(c0, c1) / d(theta, phi)| at fixed level (times the metric
 * factor of the set), t_h the height component of the unit group-velocity direction.  The 2 x 2 determinant is the one
 * geoac_fan_level_refine already forms per seed by forward differences of three rays' crossing points: the trial and two probes, one launch
 * angle each moved by probe_deg.  geoac_fan_level_amp reads those three crossing records of the refinement's final launch and makes no launch;
 * geoac_fan_level_amp_at is the primitive, for launch angles, levels and branches the caller names, at the cost of one fan of 3 n rays.
 *
 * What the amplitude is - and is not.  On the Cartesian sets AMP agrees with the amplitude of a calc_amp = 1 state row interpolated at the
 * crossing to the difference of two discretisations (the integrator's own map against the integrated variational system): 1e-5 .. 3e-4 on an
 * upward first passage, 1e-3 .. 8e-3 behind a turning point, whatever probe_deg is; central differences do not help, so there is no such
 * mode.  ON THE SPHERICAL SETS THE LEVEL AMPLITUDE IS THE GEOMETRIC ONE AND IS NOT CONTINUOUS WITH GEOAC_REC_AMP: the reference's own D
 * divides dp_ds by r sin(lat) where the metric is r cos(lat) (quirk Q3), GEOAC_REC_AMP keeps that for parity, and the term drops out of a
 * fixed-level determinant.  The reference's D differs from the geometric determinant by +11 % .. +114 % at a source at 30 N; the tube agrees
 * with the geometric one.  A caustic between the base ray and a probe gives a wrong, finite amplitude (no test can see it from three rays).
 * On a range-dependent medium the ray map is rougher than on a stratified one and the forward difference amplifies that: over a whole table of
 * rays on the Cartesian ragged test grid 12 of 97 crossings lie 2e-2 .. 4.1e-2 off the Jacobian amplitude, all behind a turning point.  On the
 * spherical ragged grid the tube is not converged in probe_deg there at all (85 of 108 crossings beyond 2e-2, gaps up to 5.5, values that move
 * by factors between h = 0.02 and 0.04) and a row could not say so: GEOAC_EQ_GLOBAL_RNGDEP IS REFUSED until the tube can judge itself.
 *
 * Definition.  IEEE double, no fused multiply-adds, every operation in the order written, left to right; SIN, COS, SINCOSD, WRAP and Pi are
 * those of geoac_refine.h.  A row names a member m, a level l and a branch (leg, dir, ord); BRANCH(ray) is the walk of geoac_level_refine.h over
 * the kept crossings of (m, ray, l).  With N rays per block, ray i is the base ray, N + i the theta probe (theta + h), 2 N + i the phi probe
 * (phi + h), h = probe_deg; (c0, c1), (ct0, ct1), (cp0, cp1) are their crossing points in the stations' axes, exactly as geoac_level_refine.h
 * takes them, and P0 .. P5 the base record's GEOAC_LVL_P0 .. + 5.
 *   1. a00 = (ct0 - c0) / h, a10 = (ct1 - c1) / h, a01 = (cp0 - c0) / h, a11 = (cp1 - c1) / h; on the spherical sets a10 = WRAP(ct1 - c1) / h,
 *      a11 = WRAP(cp1 - c1) / h.  DET = a00 * a11 - a01 * a10.
 *   2. Medium: (c, u, v, rho) at the crossing point and (c_s, u_s, v_s, rho_s) at the member's own source point, as geoac_probe_atmo_1d
 *      (out9[0], out9[3], out9[6], rho) or geoac_probe_grid with coop = 0 (api7[0], [2], [3], [1]) return them - the same kernels, the same bits.
 *      Abscissae: stratified Cartesian z = P2 and z_s = max(src z, z_grnd); stratified spherical r = P0 and r_s = max(src z, z_grnd) + r_earth;
 *      Cartesian grid (P0, P1, P2) and (src x, src y, z_s).  The source point, z_grnd and r_earth are those of the launch the records come from, not
 *      the parameters at the time of the call (geoac_set_params ends no result).
 *   3. Launch direction: (sth, cth) = SINCOSD(theta), (sph, cph) = SINCOSD(phi) of the row's launch angles [deg].  (The launch convention's azimuth is
 *      90 deg - phi: its cosine is sph, its sine cph.)
 *      GEOAC_EQ_3D (Eq3D::init and amp_jac):
 *        e0 = cth * sph, e1 = cth * cph;  MS = 1.0 + (e0 * (u_s / c_s) + e1 * (v_s / c_s));  nx = e0 / MS, ny = e1 / MS, nz = P3
 *        nu = (c_s - nx * u - ny * v) / c;  nu_s = 1.0 - (nx * u_s - ny * v_s) / c_s                                         (Q4 kept)
 *        g0 = c * nx / nu + u, g1 = c * ny / nu + v, g2 = c * nz / nu;  G = sqrt(g0 * g0 + g1 * g1 + g2 * g2);  TZ = g2 / G
 *        q0 = c_s * nx / nu_s + u_s, q1 = c_s * ny / nu_s + v_s, qx = nx / nu_s, qy = ny / nu_s, q2 = c_s * sqrt(1.0 - qx * qx - qy * qy)
 *        Q = sqrt(q0 * q0 + q1 * q1 + q2 * q2);  num = rho * nu * (c * c * c) * Q * cth;  den = rho_s * nu_s * (c_s * c_s * c_s) * G * D
 *      GEOAC_EQ_3D_RNGDEP (Eq3DRngDep::amp_jac), n0 .. n2 = P3 .. P5:
 *        nm = sqrt(n0 * n0 + n1 * n1 + n2 * n2);  j0 = c * n0 / nm + u, j1 = c * n1 / nm + v, j2 = c * n2 / nm
 *        J = sqrt(j0 * j0 + j1 * j1 + j2 * j2);  TZ = j2 / J
 *        nu = (c_s - n0 * u - n1 * v) / c;  nu_s = 1.0 - n0 * u_s / c_s - n1 * v_s / c_s
 *        g0 = c * n0 / nu + u, g1 = c * n1 / nu + v, g2 = c * n2 / nu;  G = sqrt(g0 * g0 + g1 * g1 + g2 * g2)
 *        q0 = c_s * cth * sph + u_s, q1 = c_s * cth * cph + v_s, q2 = c_s * sth;  Q = sqrt(q0 * q0 + q1 * q1 + q2 * q2)
 *        num = rho * nu * (c * c * c) * Q * cth;  den = rho_s * nu_s * (c_s * c_s * c_s) * G * D
 *      spherical sets (global_jacobian, global_amplitude, EqGlobal::init), n0 .. n2 = P3 .. P5 (radial, meridional, zonal):
 *        nm = sqrt(n0 * n0 + n1 * n1 + n2 * n2);  j0 = c * n0 / nm, j1 = c * n1 / nm + v, j2 = c * n2 / nm + u
 *        J = sqrt(j0 * j0 + j1 * j1 + j2 * j2);  TZ = j0 / J                                                     (the radial component)
 *        e1 = cth * cph, e2 = cth * sph;  MS = 1.0 + (e1 * (v_s / c_s) + e2 * (u_s / c_s));  nu_s = 1.0 / MS
 *        nu = (c_s - n1 * v - n2 * u) / c;  g0 = c * n0 / nu, g1 = c * n1 / nu + v, g2 = c * n2 / nu + u;  G = sqrt(g0 * g0 + g1 * g1 + g2 * g2)
 *        q0 = c_s * sth / nu_s, q1 = c_s * e1 / nu + v_s, q2 = c_s * e2 / nu + u_s;  Q = sqrt(q0 * q0 + q1 * q1 + q2 * q2)             (Q4 kept)
 *        num = rho * nu * (c * c * c) * Q * cth;  den = rho_s * nu_s * (c_s * c_s * c_s) * G * D
 *   4. D, formed before den:  Cartesian sets  D = fabs(TZ * DET) * (180.0 / Pi) * (180.0 / Pi);
 *      spherical sets  D = r * r * COS(c0 * Pi / 180.0) * fabs(TZ * DET), r = r_earth + z_km[l] as the host added it (the degree factors of the
 *      launch angles and of the crossing angles cancel).
 *   5. AMP = 1.0 / (4.0 * Pi) * sqrt(fabs(num / den)).
 *
 * Rows: GEOAC_LAMP_STRIDE doubles, columns below.  STATUS: SKIPPED - geoac_fan_level_amp only, the refinement row is not CONVERGED; ABSENT - the
 * base ray's branch is absent (a ray that turns below the level); NO_PROBE - a probe's branch is absent; SINGULAR - DET, D or AMP is zero or not
 * finite; OK otherwise.  They are tested in that order.  A row that is not OK carries zeros after PHI.  TTIME and ATTEN are the base record's
 * GEOAC_LVL_TTIME and GEOAC_LVL_ATTEN, bit for bit.  The level in dB is left to the caller (20 log10(AMP) - ATTEN): log10 has no bit-stable
 * restatement here.  AMP does not depend on frequency, so a frequency set gives the rows of the plain context.
 *
 * Members.  Plain contexts, source sets (every source's own source point in step 2) and frequency sets are served; calc_amp may be 0 or 1.
 * GEOAC_E_UNSUPPORTED: ensembles and grid ensembles with K > 1 - the probe evaluators read member 0's medium only -, GEOAC_EQ_GLOBAL_RNGDEP
 * (above) and GEOAC_EQ_2D.
 * GEOAC_E_INVALID: sample capture (WriteRays / WriteCaustics); no level list, or (geoac_fan_level_amp) no current refinement result - a launch, new
 * angles, an upload, geoac_set_sources, geoac_set_frequencies or geoac_set_levels since it; level_of outside the list; dir not +1 or -1; negative
 * leg or ord; probe_deg not finite or outside (0, 1]; n <= 0.  GEOAC_E_CAPACITY: 3 * n * M > GEOAC_RFN_MAX_RAY_MEMBERS, before anything is launched.
 *
 * Effect on the context.  geoac_fan_level_amp_at replaces the launch angles and the last launch (n_rays becomes 3 * n), as a round of
 * geoac_fan_level_refine does; geoac_fan_level_amp changes nothing.  The rows of either stay valid until the next geoac_fan_launch,
 * geoac_fan_set_angles, atmosphere upload, geoac_set_sources, geoac_set_frequencies or geoac_set_levels.  All device work goes to the context's
 * stream; a context that never calls an entry point of this header allocates nothing and launches nothing for it.
 *
 * Not covered: ensembles with K > 1 (they need a member view of the probe evaluators); GEOAC_EQ_GLOBAL_RNGDEP (it needs a convergence test of the
 * tube in probe_deg, a second pair of probes, and a status for its failure); the pool and the command-line drivers; the 2-D set.  (A first-order
 * amplitude of a whole lattice fan per map cell, for ensembles too, is geoac_lampmap.h's.)
 */
#ifndef GEOAC_LEVEL_AMP_H_
#define GEOAC_LEVEL_AMP_H_

#include "geoac_level_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GEOAC_LAMP_STRIDE 16
enum {
    GEOAC_LAMP_MEMBER = 0,     /* member of the launch, m = source * K + profile                              */
    GEOAC_LAMP_INDEX  = 1,     /* seed index (geoac_fan_level_amp) or ray index i < n (geoac_fan_level_amp_at) */
    GEOAC_LAMP_LEG    = 2,     /* the branch: leg,                                                            */
    GEOAC_LAMP_DIR    = 3,     /*   direction (+1 upward, -1 downward)                                        */
    GEOAC_LAMP_ORD    = 4,     /*   and ordinal                                                               */
    GEOAC_LAMP_STATUS = 5,     /* GEOAC_LAMP_OK ..                                                            */
    GEOAC_LAMP_THETA  = 6,     /* launch inclination [deg]                                                    */
    GEOAC_LAMP_PHI    = 7,     /* launch azimuth [deg], launch convention                                     */
    GEOAC_LAMP_DET    = 8,     /* from here on: OK rows only.  Finite-difference determinant                  */
    GEOAC_LAMP_TZ     = 9,     /* height component of the unit group velocity                                 */
    GEOAC_LAMP_D      = 10,    /* tube determinant                                                            */
    GEOAC_LAMP_AMP    = 11,    /* tube amplitude                                                              */
    GEOAC_LAMP_C      = 12,    /* sound speed at the crossing [km/s]                                          */
    GEOAC_LAMP_RHO    = 13,    /* density at the crossing                                                     */
    GEOAC_LAMP_TTIME  = 14,    /* GEOAC_LVL_TTIME of the base crossing record                                 */
    GEOAC_LAMP_ATTEN  = 15     /* GEOAC_LVL_ATTEN of the base crossing record                                 */
};
enum { GEOAC_LAMP_OK = 1, GEOAC_LAMP_ABSENT = 2, GEOAC_LAMP_NO_PROBE = 3, GEOAC_LAMP_SINGULAR = 4, GEOAC_LAMP_SKIPPED = 5 };

/* host-only validation (no device needed): GEOAC_OK, GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D and GEOAC_EQ_GLOBAL_RNGDEP, GEOAC_E_INVALID for an unknown set or a probe_deg that is
 * not finite or outside (0, 1]; fault (may be NULL) receives a string literal naming the fault, or NULL */
int  geoac_level_amp_check(int eqset, double probe_deg, const char** fault);

/* rows [M][n] for n rays: ray i at (theta_deg[i], phi_deg[i]), level level_of[i] of the context's level list, branch (leg[i], dir[i], ord[i]).
 * Launches one fan of 3 * n rays (see above). */
int  geoac_fan_level_amp_at(geoac_ctx* ctx, int n, const double* theta_deg, const double* phi_deg, const int* level_of, const int* leg, const int* dir,
                            const int* ord, double probe_deg);
/* rows [n_seeds] of the current geoac_fan_level_refine result, from its final launch's crossing tables and its probe_deg: no launch */
int  geoac_fan_level_amp(geoac_ctx* ctx);
/* shape of the current result: rows in all (M * n, or n_seeds) and the members M of the launch they were read from */
int  geoac_fan_level_amp_shape(geoac_ctx* ctx, int* n_rows, int* members);
/* rows [n_rows][GEOAC_LAMP_STRIDE] f64 to the host */
int  geoac_fan_level_amp_fetch(geoac_ctx* ctx, double* rows);
/* device pointer of the rows (NULL when there are none), valid until the next call that makes rows, ordered on the context's stream */
int  geoac_fan_level_amp_dev(geoac_ctx* ctx, void** dev_ptr, size_t* bytes);
/* HIP-event times of the last call that made rows [ms]: [0] its launch (0 for geoac_fan_level_amp), [1] its own kernels and the probe kernel */
int  geoac_fan_level_amp_timing(geoac_ctx* ctx, double ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_LEVEL_AMP_H_ */
