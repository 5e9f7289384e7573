/* geoac_lampmap.h - level loudness maps: the ray-tube amplitude of one launch's crossing triangles per cell at altitude, on the device.
 *
 * geoac_fan_level_tubemap (geoac_ltubemap.h) says where a source is heard at an altitude, over how many paths and when; geoac_fan_level_amp
 * (geoac_level_amp.h) gives the spreading amplitude of a refined eigenray at three extra rays per receiver.  geoac_fan_level_ampmap answers "how loud
 * is the source across a region at that altitude" from the launch alone.  A crossing triangle already is a ray tube: three neighbouring lattice rays on
 * one branch cross the level at three points, and the area of that triangle over the area of the triangle of their launch angles is the fixed-level
 * determinant that geoac_level_amp.h forms from probes.  Everything else the amplitude formula needs is interpolated at a hit by the level-station
 * rule.  One more rasterising pass over data already on the device yields geometric and received amplitude per (member, level, cell), at about the cost
 * of a level tube map instead of a refinement per cell.
 *
 * IT IS A FIRST-ORDER AMPLITUDE, in the sense in which a level-station row is a first-order eigenray: DET is the mean of the ray map's determinant over
 * the lattice triangle and the slowness, launch angles, time and attenuation are linear interpolants, so its error is the truncation of the lattice step:
 * first order in the step, because the determinant changes by O(step) across the triangle whose mean a centre is given (measured in DESIGN.md 8q).  A caustic between the corners of a triangle gives a wrong, finite
 * amplitude that no test on three rays can see; det_floor only removes the triangles that are folded or nearly so.  Behind turning points on a
 * range-dependent medium the ray map is rough on the scale of a lattice cell and the amplitude must not be trusted.
 *
 * Definition (normative).  geoac_lampmap_spec has every field of geoac_ltube_spec with the same meaning and the same validation, and two more.  A hit
 * of cell (m, l, i0, i1) is exactly a hit of geoac_ltubemap.h: the same cell centres s_a = origin[a] + (i_a + 0.5) * step[a], branch table, corner
 * matching by branch, edge_max, dir_mask, level_mask, longitude wrap and triangle rule, the same weights Wk = wk / s and the same corner order 0, 1, 2
 * (lattice triangle 2 cell: rays a, b, c; 2 cell + 1: rays a, c, d).  For a hit, in IEEE double with no fused multiply-adds, every operation in the
 * order written; SIN, COS, SINCOSD, WRAP and Pi are those of geoac_refine.h:
 *   1. Crossing area.  (ck0, ck1) is corner k's crossing point in the stations' axes (geoac_lstations.h).  ex1 = c10 - c00, ey1 = c11 - c01,
 *      ex2 = c20 - c00, ey2 = c21 - c01; on the spherical sets ey1 = WRAP(c11 - c01), ey2 = WRAP(c21 - c01).  AX = ex1 * ey2 - ex2 * ey1.
 *   2. Launch-angle area, from the corners' launch angles as the launch received them: at1 = th1 - th0, at2 = th2 - th0, ap1 = WRAP(ph1 - ph0),
 *      ap2 = WRAP(ph2 - ph0), AA = at1 * ap2 - at2 * ap1.  DET = AX / AA, in the units of GEOAC_LAMP_DET: axis units squared per degree squared.
 *      AX, AA and DET belong to the triangle, not to the cell.
 *   3. THETA, PHI, TTIME, ATTEN, N0 .. N2 are those of the level-station row of this hit, bit for bit: ((W0 * v0) + (W1 * v1)) + (W2 * v2), and the
 *      phi_periodic rule of geoac_lstations.h for PHI.
 *   4. Medium, from the kernels behind geoac_probe_atmo_1d (out9[0], out9[3], out9[6], rho) / geoac_probe_grid with coop = 0 (api7[0], [2], [3], [1]),
 *      the same bits: (c, u, v, rho) on the stratified Cartesian set at z_km[l], on the stratified spherical set at r_earth + z_km[l], on
 *      GEOAC_EQ_3D_RNGDEP at (s_0, s_1, z_km[l]), the cell centre; (c_s, u_s, v_s, rho_s) at member m's own source point, formed as step 2 of
 *      geoac_level_amp.h forms it.  Both in profile m % K of an ensemble or a grid ensemble.  The source point, z_grnd and r_earth are those of the
 *      launch (geoac_set_params ends no result).
 *   5. TZ, nu, nu_s, G, Q, num, den, D and AMP are steps 3 to 5 of geoac_level_amp.h for the equation set, with P3 .. P5 := N0 .. N2, the row's launch
 *      angles THETA, PHI, DET the value of step 2 and, on the spherical sets, the latitude in D the cell centre's: D = r * r * COS(s_0 * Pi / 180.0) *
 *      fabs(TZ * DET), r = r_earth + z_km[l].
 *   6. RAMP = AMP * EXP(-(ATTEN * (LN10 / 20.0))), LN10 = 2.302585092994045684.  EXP is the series of geoac_rfn_series.h (rfn_exp), normative, not libm:
 *        a NaN returns itself; x < -700.0 returns 0.0 (so that no subnormal rounding enters: EXP(-700) = 9.8e-305 is normal); x > 700.0 returns +inf;
 *        q = floor(x / LN2 + 0.5);  r = (x - q * LN2_HI) - q * LN2_LO;  s = 1.0, then for k = 14 down to 1: s = 1.0 + (r * s) / k;  EXP = s * 2^q,
 *        2^q exact.  LN2 = 0.693147180559945309417, LN2_HI = 6.93147180369123816490e-01 (31 significant bits: q * LN2_HI is exact),
 *        LN2_LO = 1.90821492927058770002e-10.  Against a correctly rounded exp it is within 2 ulp on [-700, 0] (tests/test_lampmap_host.py measures
 *        1 ulp against numpy.exp and pins 2).
 * A hit is usable when AA != 0, |DET| > det_floor, DET, D and AMP are finite and not zero, and TTIME, ATTEN and RAMP are finite.
 *
 * Layers, 8 bytes per cell, [M][Ls][n0][n1], row-major, axis 1 fastest (M, Ls as in geoac_ltubemap.h):
 *   GEOAC_LAMPMAP_COUNT    u64  usable hits                                                                        empty: 0
 *   GEOAC_LAMPMAP_WEAK     u64  hits that are not usable; COUNT + WEAK equals GEOAC_LTUBE_COUNT of the same spec   empty: 0
 *   GEOAC_LAMPMAP_AMP_MAX  f64  largest AMP of the usable hits                                                     empty: -inf
 *   GEOAC_LAMPMAP_RAMP_MAX f64  largest RAMP of the usable hits                                                    empty: -inf
 *   GEOAC_LAMPMAP_LOUDEST  i64  b * n_tri + tri of the usable hit holding RAMP_MAX, the smallest on a tie          empty: -1
 *   DETECT                 [Ls][n0][n1] u32  members with RAMP_MAX >= detect_amp; absent when detect_amp is NaN
 * Maxima are taken on the order-preserving 64-bit key of the double (geoac_map.h), and every reduction is an integer atomic: a map is the same bits
 * on every run.  The level in dB is left to the caller (20 log10(RAMP_MAX)).  With a frequency set ATTEN, and so RAMP, is that of frequency 0, as in
 * the crossing records.  calc_amp may be 0 or 1.
 *
 * Served: GEOAC_EQ_3D, GEOAC_EQ_GLOBAL, GEOAC_EQ_3D_RNGDEP; plain contexts, source sets, frequency sets, 1-D ensembles and grid ensembles with K > 1.
 * Refused (geoac_lampmap_fault names the first): GEOAC_EQ_2D and GEOAC_EQ_GLOBAL_RNGDEP with GEOAC_E_UNSUPPORTED - on a range-dependent spherical
 * grid the probe tube of geoac_level_amp.h is not converged behind a turning point, and a coarse lattice tube is no better conditioned -; everything
 * geoac_ltube_check refuses; det_floor that is not finite or is negative; detect_amp that is neither NaN nor finite and > 0.  At call time also
 * everything geoac_fan_level_tubemap refuses, and sample capture (WriteRays / WriteCaustics) with GEOAC_E_INVALID.  GEOAC_E_NOMEM names the size it
 * asked for.  A refused call allocates nothing.
 *
 * Call order and invalidation are those of geoac_ltubemap.h: geoac_fan_launch with levels, then geoac_fan_level_ampmap any number of times; a new
 * launch, geoac_fan_set_angles, an atmosphere upload, geoac_set_sources, geoac_set_frequencies and geoac_set_levels end the map, geoac_set_params
 * does not.  The branch table is the one geoac_fan_level_stations and geoac_fan_level_tubemap form: formed once per launch for the same leg_min,
 * leg_max and ord_max.  All device work goes to the context's stream.  A context that never calls an entry point of this header allocates nothing
 * and launches nothing for it.  The pool (geoac_multi.h) has no such call.
 */
#ifndef GEOAC_LAMPMAP_H_
#define GEOAC_LAMPMAP_H_

#include "geoac_ltubemap.h"
#include "geoac_level_amp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GEOAC_LAMPMAP_COUNT    = 0,
    GEOAC_LAMPMAP_WEAK     = 1,
    GEOAC_LAMPMAP_AMP_MAX  = 2,
    GEOAC_LAMPMAP_RAMP_MAX = 3,
    GEOAC_LAMPMAP_LOUDEST  = 4,
    GEOAC_LAMPMAP_LAYERS   = 5
};

typedef struct {
    double origin[2];        /* the fields of geoac_ltube_spec, in its order, with its meaning and its validation                              */
    double step[2];
    int    n[2];
    int    wrap_lon;
    int    n_theta, n_phi;
    int    phi_periodic;
    int    leg_min, leg_max;
    int    ord_max;
    double edge_max;
    int    dir_mask;
    int    level_mask;
    double det_floor;        /* finite, >= 0: a hit with |DET| <= det_floor carries no amplitude (a folded or near-caustic tube)                */
    double detect_amp;       /* NaN: no DETECT layer; otherwise finite and > 0: DETECT counts the members with RAMP_MAX >= detect_amp          */
} geoac_lampmap_spec;

/* host-only validation (no device needed) against a launch of n_rays rays and n_levels levels: GEOAC_OK and the cell count n[0] * n[1] and the number
 * of selected levels Ls (either pointer may be NULL); GEOAC_E_UNSUPPORTED for GEOAC_EQ_2D and GEOAC_EQ_GLOBAL_RNGDEP; GEOAC_E_INVALID for anything
 * else that is wrong.  geoac_lampmap_fault names the first fault (NULL: none; a string literal, valid for ever). */
int         geoac_lampmap_check(int eqset, const geoac_lampmap_spec* spec, int n_rays, int n_levels, int64_t* cells, int* n_selected);
const char* geoac_lampmap_fault(int eqset, const geoac_lampmap_spec* spec, int n_rays, int n_levels);

/* rasterise the crossing triangles of the last completed launch into amplitude layers.  Statuses as listed under Refused. */
int  geoac_fan_level_ampmap(geoac_ctx* ctx, const geoac_lampmap_spec* spec);
/* shape of the current map: M, Ls, n0, n1, and whether it has a DETECT layer */
int  geoac_fan_level_ampmap_shape(geoac_ctx* ctx, int* n_members, int* n_selected, int* n0, int* n1, int* has_detect);
/* one layer (GEOAC_LAMPMAP_*) to the host / its device pointer (valid until the next geoac_fan_level_ampmap, ordered on the context's stream) */
int  geoac_fan_level_ampmap_fetch(geoac_ctx* ctx, int layer, void* host);
int  geoac_fan_level_ampmap_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes);
/* DETECT [Ls][n0][n1] u32; GEOAC_E_INVALID when the map was made with detect_amp = NaN */
int  geoac_fan_level_ampmap_fetch_detect(geoac_ctx* ctx, uint32_t* detect_host);
/* HIP-event time of the last geoac_fan_level_ampmap on the context's stream [ms] (waits for it; the medium probes and a branch table formed by the
 * call are inside) */
int  geoac_fan_level_ampmap_timing(geoac_ctx* ctx, double* ms);
/* work counters of the last geoac_fan_level_ampmap, four u64, as geoac_fan_level_tubemap_stats gives them (pass 0 of the walk) */
int  geoac_fan_level_ampmap_stats(geoac_ctx* ctx, uint64_t* stats4);

#ifdef __cplusplus
}
#endif
#endif /* GEOAC_LAMPMAP_H_ */
