// geoac_tube_walk.h - the triangle-outward walk of a tube map, apart from where a corner comes from and what a hit reduces: the candidate box
// of a triangle on a map grid, the enumeration of its candidates, and the walk of one wave over the boxes of its 64 lanes.  The rules are those
// of include/geoac_tubemap.h, stated there for landing triangles: geoac_tubemap.hip runs them over the landing triangles of a leg,
// geoac_ltubemap.hip over the crossing triangles of a branch plane.  (This is the way geoac_lattice_list.h serves the two station files.)
//
// The caller gives:
//   a WalkGrid                         the grid, the square of the pre-test's bound, the cooperative threshold
//   three double4 corners              (c0, c1, caller's own, present / valid) in the map's coordinates; the caller has tested .w and its own filters
//   hit(const WalkTri&, i0, i1)        the exact rule at the centre of cell (i0, i1), i0 < n0, i1 < n1, and the reductions of a hit
// The box only proposes: it has to be conservative and nothing more.
//
// The arithmetic is that of geoac_tri_rule.h: contraction is off from here on.
#ifndef GEOAC_TUBE_WALK_H_
#define GEOAC_TUBE_WALK_H_

#include <hip/hip_runtime.h>
#include <math.h>

#include "geoac_tri_rule.h"

#pragma clang fp contract(off)

namespace {

const double kWalkSlack = 1.0 / 1099511627776.0;       // 2^-40: slack of the centre-independent side test, relative to the coordinates' size

struct WalkGrid {
    double o0, o1, s0, s1;                        // origin and step per axis
    double pre2;                                  // the square of the bound of walk_box's side test (walk_pre2)
    int n0, n1, spherical;
    int coop_min;                                 // a box above this many centres is walked by the wave
};

// a triangle on its way through the walk: its corners (c0, c1 and the caller's third value), where they came from, and its box
struct WalkTri {
    double x0, y0, z0, x1, y1, z1, x2, y2, z2;
    int r0, r1, r2;                               // ray indices of the corners
    int tri, plane, m;                            // triangle index, the caller's plane (a leg; a level and a branch), member
    int row_lo, n_rows;                           // rows of centres proposed
    int c0, w0, c1, w1, c2, w2;                   // up to three disjoint runs of columns: first column, width
};

// the square of the pre-test's bound: twice edge_max plus 2^-40 of the largest coordinate a corner of a hit can have (host)
inline double walk_pre2(const double origin[2], const double step[2], const int n[2], double edge_max, bool on_sphere){
    const double mag = (fabs(origin[0]) + n[0] * step[0]) + (fabs(origin[1]) + n[1] * step[1]) + (on_sphere ? 720.0 : 0.0);
    const double pre = 2.0 * edge_max + kWalkSlack * (mag + edge_max);
    return pre * pre;
}

// cell index of a coordinate, clamped to -1 .. n (a NaN gives n: an empty run)
__device__ inline int walk_cell_of(double c, double o, double s, int n){
    const double q = floor((c - o) / s);
    if(!(q >= -1.0)) return q < 0.0 ? -1 : n;
    return q < (double)n ? (int)q : n;
}

// columns lo - 1 .. hi + 1 clipped to the grid and to the columns after `after`: first column and width (first >= 0, first + width <= n1)
__device__ inline void walk_col_run(double lo, double hi, const WalkGrid& G, int after, int* first, int* width){
    int a = walk_cell_of(lo, 0.0, G.s1, G.n1) - 1, b = walk_cell_of(hi, 0.0, G.s1, G.n1) + 1;
    if(a <= after) a = after + 1;
    if(b > G.n1 - 1) b = G.n1 - 1;
    *first = a; *width = b >= a ? b - a + 1 : 0;
}

// the box of a triangle.  false: it proposes nothing.  The side test is not the exact rule's: it uses longitudes relative to corner 0 instead
// of relative to the centre, and its bound is looser (walk_pre2), so that rounding never removes a triangle the exact test would keep at some
// centre.  Rows row_lo .. row_lo + n_rows - 1 lie in 0 .. n0 - 1, every column run in 0 .. n1 - 1.
__device__ inline bool walk_box(const WalkGrid& G, const double4& a, const double4& b, const double4& c, WalkTri* T){
    // offsets along axis 1 from the grid's origin; spherical: corner 0 into 0 .. 360, corners 1 and 2 within 180 degrees of it
    double l0 = a.y - G.o1, l1, l2;
    if(G.spherical){
        l0 = l0 - 360.0 * floor(l0 / 360.0);
        l1 = l0 + wrap180(b.y - a.y);
        l2 = l0 + wrap180(c.y - a.y);
    } else { l1 = b.y - G.o1; l2 = c.y - G.o1; }
    const double e2 = dmax(dmax(len2(a.x, l0, b.x, l1), len2(b.x, l1, c.x, l2)), len2(c.x, l2, a.x, l0));
    if(!(e2 <= G.pre2)) return false;
    const double xlo = dmin(dmin(a.x, b.x), c.x), xhi = dmax(dmax(a.x, b.x), c.x);
    int r_lo = walk_cell_of(xlo, G.o0, G.s0, G.n0) - 1, r_hi = walk_cell_of(xhi, G.o0, G.s0, G.n0) + 1;
    if(r_lo < 0) r_lo = 0;
    if(r_hi > G.n0 - 1) r_hi = G.n0 - 1;
    T->row_lo = r_lo; T->n_rows = r_hi >= r_lo ? r_hi - r_lo + 1 : 0;
    const double llo = dmin(dmin(l0, l1), l2), lhi = dmax(dmax(l0, l1), l2);
    T->w0 = 0; T->w2 = 0; T->c0 = 0; T->c2 = 0;
    if(G.spherical){
        // a centre at offset u is proposed when u + 360 k lies in the box for k = 1, 0 or -1: three runs in ascending column order, kept disjoint
        walk_col_run(llo - 360.0, lhi - 360.0, G, -1, &T->c0, &T->w0);
        walk_col_run(llo, lhi, G, T->w0 ? T->c0 + T->w0 - 1 : -1, &T->c1, &T->w1);
        const int last = T->w1 ? T->c1 + T->w1 - 1 : (T->w0 ? T->c0 + T->w0 - 1 : -1);
        walk_col_run(llo + 360.0, lhi + 360.0, G, last, &T->c2, &T->w2);
    } else walk_col_run(llo, lhi, G, -1, &T->c1, &T->w1);
    T->x0 = a.x; T->y0 = a.y; T->z0 = a.z; T->x1 = b.x; T->y1 = b.y; T->z1 = b.z; T->x2 = c.x; T->y2 = c.y; T->z2 = c.z;
    return T->n_rows > 0 && (T->w0 + T->w1 + T->w2) > 0;
}

// candidate k of a triangle's box, k < n_rows * (w0 + w1 + w2) -> the cell (i0, i1), i0 < n0, i1 < n1
__device__ inline void walk_cand(const WalkTri& T, int k, int* i0, int* i1){
    const int w = T.w0 + T.w1 + T.w2;
    const int r = k / w, c = k - r * w;
    *i0 = T.row_lo + r;
    *i1 = c < T.w0 ? T.c0 + c : (c < T.w0 + T.w1 ? T.c1 + (c - T.w0) : T.c2 + (c - T.w0 - T.w1));
}

__device__ inline int walk_bcast(int v, int src){ return __shfl(v, src, 64); }
// (a broadcast triangle travels through vector registers: in scalar registers, beside the kernel's arguments, it would spill)
__device__ inline double walk_bcast(double v, int src){ return __shfl(v, src, 64); }

// the work counters of a lane, summed over the wave at the end (walk_totals)
struct WalkCount { unsigned n_tri = 0, n_coop = 0, n_cand = 0; };

// one triangle per lane (ok: the lane has one with a box), all 64 lanes of the wave here together: a box of at most coop_min centres is
// walked by its lane, the lanes with larger boxes are balloted and the wave takes them one at a time, corners and box broadcast, 64 centres per
// trip.  hit(T, i0, i1) runs the exact rule at a proposed centre.
template <class Hit>
__device__ inline void walk_wave(const WalkGrid& G, bool ok, const WalkTri& T, int lane, WalkCount* C, Hit hit){
    const int n = ok ? T.n_rows * (T.w0 + T.w1 + T.w2) : 0;
    const bool big = n > G.coop_min;
    if(ok){ C->n_tri++; C->n_cand += (unsigned)n; }
    if(ok && !big)
        for(int k = 0; k < n; k++){
            int i0, i1;
            walk_cand(T, k, &i0, &i1);
            hit(T, i0, i1);
        }
    unsigned long long todo = __ballot(big);
    while(todo){
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        if(lane == src) C->n_coop++;
        WalkTri U;
        U.x0 = walk_bcast(T.x0, src); U.y0 = walk_bcast(T.y0, src); U.z0 = walk_bcast(T.z0, src);
        U.x1 = walk_bcast(T.x1, src); U.y1 = walk_bcast(T.y1, src); U.z1 = walk_bcast(T.z1, src);
        U.x2 = walk_bcast(T.x2, src); U.y2 = walk_bcast(T.y2, src); U.z2 = walk_bcast(T.z2, src);
        U.r0 = walk_bcast(T.r0, src); U.r1 = walk_bcast(T.r1, src); U.r2 = walk_bcast(T.r2, src);
        U.tri = walk_bcast(T.tri, src); U.plane = walk_bcast(T.plane, src); U.m = walk_bcast(T.m, src);
        U.row_lo = walk_bcast(T.row_lo, src); U.n_rows = walk_bcast(T.n_rows, src);
        U.c0 = walk_bcast(T.c0, src); U.w0 = walk_bcast(T.w0, src); U.c1 = walk_bcast(T.c1, src); U.w1 = walk_bcast(T.w1, src);
        U.c2 = walk_bcast(T.c2, src); U.w2 = walk_bcast(T.w2, src);
        const int nu = U.n_rows * (U.w0 + U.w1 + U.w2);
        for(int k = lane; k < nu; k += 64){
            int i0, i1;
            walk_cand(U, k, &i0, &i1);
            hit(U, i0, i1);
        }
    }
}

// the wave's counters into stats[0 .. 2]: triangles with a box, triangles walked by the wave, candidate centres
__device__ inline void walk_totals(const WalkCount& C, int lane, unsigned long long* stats){
    unsigned n_tri = C.n_tri, n_coop = C.n_coop;
    for(int off = 32; off > 0; off >>= 1){
        n_tri += (unsigned)__shfl_xor((int)n_tri, off, 64);
        n_coop += (unsigned)__shfl_xor((int)n_coop, off, 64);
    }
    unsigned long long c64 = C.n_cand;
    for(int off = 32; off > 0; off >>= 1){
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(c64 & 0xffffffffull), off, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(c64 >> 32), off, 64);
        c64 += ((unsigned long long)hi << 32) | lo;
    }
    if(lane == 0 && n_tri){
        atomicAdd(&stats[0], (unsigned long long)n_tri);
        if(n_coop) atomicAdd(&stats[1], (unsigned long long)n_coop);
        atomicAdd(&stats[2], c64);
    }
}

}  // namespace

#endif
