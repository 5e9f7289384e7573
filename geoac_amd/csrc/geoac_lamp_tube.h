// geoac_lamp_tube.h - steps 3 to 5 of include/geoac_level_amp.h, which is normative for this arithmetic: from the medium at the crossing and at the
// member's source, the launch angles, the slowness at the crossing and a fixed-level determinant DET to TZ, D and AMP.  Defined once, for
// geoac_level_amp.hip (DET from two probes of a refined eigenray) and geoac_lampmap.hip (DET from a crossing triangle of the launch lattice, the
// slowness and the launch angles interpolated at a cell centre).  Restated in tests/level_amp_reference.py (tube): every product is rounded before it
// is added, so contraction is off from here on in whatever file includes this.
#ifndef GEOAC_LAMP_TUBE_H_
#define GEOAC_LAMP_TUBE_H_

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/geoac_hip.h"
#include "geoac_rfn_series.h"

#pragma clang fp contract(off)

namespace {

struct LampMedium { double c, u, v, rho; };

// m: the medium at the crossing, s: at the member's source; th, ph: launch angles [deg]; n0 .. n2: GEOAC_LVL_P0 + 3 .. + 5 of the crossing;
// lat_deg, r: the latitude [deg] and the level radius in D (spherical sets only)
__device__ inline void lamp_tube(int eqset, const LampMedium& m, const LampMedium& s, double th, double ph, double n0, double n1, double n2, double det,
                                 double lat_deg, double r, double* tz_out, double* dd_out, double* amp_out){
    double sth, cth, sph, cph;
    rfn_sincosd(th, &sth, &cth); rfn_sincosd(ph, &sph, &cph);
    const double c3 = m.c * m.c * m.c, cs3 = s.c * s.c * s.c;
    double nu, nu_s, G, Qm, tz, dd;
    if(eqset == GEOAC_EQ_3D){
        const double e0 = cth * sph, e1 = cth * cph;
        const double MS = 1.0 + (e0 * (s.u / s.c) + e1 * (s.v / s.c));
        const double nx = e0 / MS, ny = e1 / MS, nz = n0;
        nu = (s.c - nx * m.u - ny * m.v) / m.c;
        nu_s = 1.0 - (nx * s.u - ny * s.v) / s.c;
        const double g0 = m.c * nx / nu + m.u, g1 = m.c * ny / nu + m.v, g2 = m.c * nz / nu;
        G = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
        tz = g2 / G;
        const double q0 = s.c * nx / nu_s + s.u, q1 = s.c * ny / nu_s + s.v, qx = nx / nu_s, qy = ny / nu_s;
        const double q2 = s.c * sqrt(1.0 - qx * qx - qy * qy);
        Qm = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
    } else if(eqset == GEOAC_EQ_3D_RNGDEP){
        const double nm = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        const double j0 = m.c * n0 / nm + m.u, j1 = m.c * n1 / nm + m.v, j2 = m.c * n2 / nm;
        const double J = sqrt(j0 * j0 + j1 * j1 + j2 * j2);
        tz = j2 / J;
        nu = (s.c - n0 * m.u - n1 * m.v) / m.c;
        nu_s = 1.0 - n0 * s.u / s.c - n1 * s.v / s.c;
        const double g0 = m.c * n0 / nu + m.u, g1 = m.c * n1 / nu + m.v, g2 = m.c * n2 / nu;
        G = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
        const double q0 = s.c * cth * sph + s.u, q1 = s.c * cth * cph + s.v, q2 = s.c * sth;
        Qm = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
    } else {
        const double nm = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        const double j0 = m.c * n0 / nm, j1 = m.c * n1 / nm + m.v, j2 = m.c * n2 / nm + m.u;
        const double J = sqrt(j0 * j0 + j1 * j1 + j2 * j2);
        tz = j0 / J;
        const double e1 = cth * cph, e2 = cth * sph;
        const double MS = 1.0 + (e1 * (s.v / s.c) + e2 * (s.u / s.c));
        nu_s = 1.0 / MS;
        nu = (s.c - n1 * m.v - n2 * m.u) / m.c;
        const double g0 = m.c * n0 / nu, g1 = m.c * n1 / nu + m.v, g2 = m.c * n2 / nu + m.u;
        G = sqrt(g0 * g0 + g1 * g1 + g2 * g2);
        const double q0 = s.c * sth / nu_s, q1 = s.c * e1 / nu + s.v, q2 = s.c * e2 / nu + s.u;
        Qm = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
    }
    if(eqset == GEOAC_EQ_GLOBAL || eqset == GEOAC_EQ_GLOBAL_RNGDEP) dd = r * r * rfn_cos(lat_deg * kRfnPi / 180.0) * fabs(tz * det);
    else dd = fabs(tz * det) * (180.0 / kRfnPi) * (180.0 / kRfnPi);
    const double num = m.rho * nu * c3 * Qm * cth;
    const double den = s.rho * nu_s * cs3 * G * dd;
    *tz_out = tz; *dd_out = dd;
    *amp_out = 1.0 / (4.0 * kRfnPi) * sqrt(fabs(num / den));
}

}  // namespace

#endif
