// geoac_tri_rule.h - the station rule of include/geoac_stations.h, which is normative for this arithmetic: whether a point lies in a landing
// triangle, and the weights of the corners.  Used by geoac_lattice_list.h (a station, on the ground for geoac_stations.hip and at a level for
// geoac_lstations.hip), geoac_tubemap.hip (a cell centre) and geoac_refine.hip (the longitude difference).  Restated in
// tests/station_reference.py: every product is rounded before it is added, so contraction is off from here on in whatever file includes this.
#ifndef GEOAC_TRI_RULE_H_
#define GEOAC_TRI_RULE_H_

#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

__device__ inline double wrap180(double d){ return d - 360.0 * floor((d + 180.0) / 360.0); }
__device__ inline double cross2(double ax, double ay, double bx, double by){ return ax * by - ay * bx; }
__device__ inline double len2(double ax, double ay, double bx, double by){ const double dx = bx - ax, dy = by - ay; return dx * dx + dy * dy; }
__device__ inline double dmax(double a, double b){ return a > b ? a : b; }
__device__ inline double dmin(double a, double b){ return a < b ? a : b; }
__device__ inline double interp(double W0, double W1, double W2, double v0, double v1, double v2){ return ((W0 * v0) + (W1 * v1)) + (W2 * v2); }

struct Tri { double w0, w1, w2, s; bool hit; };

// corners relative to the point (longitudes already within 180 degrees of it): edge filter, cross products, sign rule.  The weights of a hit
// are w0 / s, w1 / s, w2 / s.
__device__ inline Tri tri_rule(double x0, double y0, double x1, double y1, double x2, double y2, double edge2){
    Tri T;
    T.w0 = T.w1 = T.w2 = T.s = 0.0; T.hit = false;
    const double e2 = dmax(dmax(len2(x0, y0, x1, y1), len2(x1, y1, x2, y2)), len2(x2, y2, x0, y0));
    if(!(e2 <= edge2)) return T;
    T.w0 = cross2(x1, y1, x2, y2);
    T.w1 = cross2(x2, y2, x0, y0);
    T.w2 = cross2(x0, y0, x1, y1);
    T.s = (T.w0 + T.w1) + T.w2;
    T.hit = T.s != 0.0 && ((T.w0 >= 0.0 && T.w1 >= 0.0 && T.w2 >= 0.0) || (T.w0 <= 0.0 && T.w1 <= 0.0 && T.w2 <= 0.0));
    return T;
}

#endif
