// geoac_tubemap.hip - tube maps (include/geoac_tubemap.h): the landing triangles of the last completed launch rasterised on a regular grid,
// on the device.
//
// Reads the record table, the level table of geoac_map.hip and the lattice axes of the launch angles; writes only buffers of its own.  No
// kernel of the launch plan is involved.
//
// Kernels:
//   k_tube_prep     landing table land[M][legs][n_rays] of (c0, c1, turn, valid), 32 B per corner, in the map's coordinates: the file's own
//                   table, formed once per launch.
//   k_tube_fill     initial values of all layers and of the work counters in one pass.
//   k_tube_raster   <0>: one lane per (member, leg, lattice cell), the cell's two triangles one after the other.  A triangle that passes the
//                   filters that do not depend on the cell centre proposes a box of centres: the bounding box of its corners in cell-index
//                   space, widened by one cell on every side, clipped to the grid; on the spherical sets the longitudes are first brought within
//                   180 degrees of corner 0 and the box is mapped to the grid's columns modulo 360 (up to three disjoint runs of columns).
//                   The box only proposes: at every proposed centre the exact filters and sign rule of geoac_stations.h decide, so the box has
//                   to be conservative and nothing more.  A box of at most coop_min centres is walked by its lane; the lanes with larger
//                   boxes are balloted, and the wave takes them one at a time: corners and box broadcast, 64 centres per trip.  A hit adds 1
//                   to COUNT and takes part in the key minima / maxima.
//                   <1>: the same walk again; hits whose level equals their cell's LEVEL_MAX compete for BEST with leg * n_tri + tri.
//   k_tube_finish   keys back to doubles in place, empty-cell markers.
//   k_tube_detect   members with LEVEL_MAX >= detect_db.
// Every reduction is an integer atomic (u64 add; u64 min / max on the order-preserving key of a double; u64 min on the hit's key), so the
// layers do not depend on the order the hits are seen in.
//
// The arithmetic of the test and of the interpolated values is fixed by the headers and restated in tests/station_reference.py and
// tests/tubemap_reference.py: every product is rounded before it is added, so this file is compiled with contraction off (the pragma below; the
// Makefile gives the same flag).  The inline triangle functions restate those of geoac_stations.hip; that file is not touched.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "../../include/geoac_tubemap.h"
#include "geoac_tubemap_int.h"

#pragma clang fp contract(off)

namespace {

const double kTubePi = 3.141592653589793238462643;
const unsigned long long kSign = 0x8000000000000000ull;
const double kTubeSlack = 1.0 / 1099511627776.0;      // 2^-40: slack of the station-independent side test, relative to the coordinates' size

// order-preserving key of a double, as in geoac_map.hip
__device__ inline unsigned long long tube_key(double v){
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | kSign);
}
__device__ inline double tube_unkey(unsigned long long k){
    return __longlong_as_double((long long)((k >> 63) ? (k & ~kSign) : ~k));
}

struct TubeDev {
    const double* rec; const double* level;       // the launch's tables
    double4* land;                                // [M][legs][n_rays]: c0, c1, turn, valid
    unsigned long long *count, *lvl, *stats;      // COUNT | TTIME_MIN | CEL_MAX follow one another, M * cells words each; LEVEL_MAX | BEST, M * F * cells each
    unsigned* detect;
    double o0, o1, s0, s1;                        // the grid
    double turn_tol, edge2, pre2;                 // edge2 = edge_max * edge_max; pre2: the square of the bound of tube_box's side test
    double turn_min, turn_max, detect_db;
    int n0, n1, spherical;
    int M, F, n_rays, legs, n_theta, n_phi;
    int leg0, n_legs, n_cells, coop_min;          // legs leg0 .. leg0 + n_legs - 1 take part; cells of the lattice
    long long cells;                              // n0 * n1
};

// one thread per (m, leg, ray): the landing point in the map's coordinates
__global__ void k_tube_prep(TubeDev D){
    const long long n = (long long)D.M * D.legs * D.n_rays;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride){
        const int ray = (int)(t % D.n_rays);
        const long long ml = t / D.n_rays;
        const int leg = (int)(ml % D.legs);
        const long long m = ml / D.legs;
        const double* R = D.rec + ((m * D.n_rays + ray) * D.legs + leg) * GEOAC_REC_STRIDE;
        double4 o;
        if(D.spherical){
            o.x = R[GEOAC_REC_STATE + 1] * 180.0 / kTubePi;
            o.y = R[GEOAC_REC_STATE + 2] * 180.0 / kTubePi;
        } else {
            o.x = R[GEOAC_REC_STATE + 0];
            o.y = R[GEOAC_REC_STATE + 1];
        }
        o.z = R[GEOAC_REC_TURN];
        o.w = R[GEOAC_REC_VALID];
        D.land[t] = o;
    }
}

// initial values of the layers, back to back in one allocation: COUNT 0 | TTIME key ~0 | CEL key 0 | LEVEL key 0 | BEST max | stats 0 | DETECT 0
__global__ void k_tube_fill(unsigned long long* w, long long n_mc, long long n_mfc, long long n_words){
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride){
        unsigned long long v = 0;
        if(i >= n_mc && i < 2 * n_mc) v = ~0ull;
        else if(i >= 3 * n_mc + n_mfc && i < 3 * n_mc + 2 * n_mfc) v = 0x7fffffffffffffffull;
        w[i] = v;
    }
}

__device__ inline double wrap180(double d){ return d - 360.0 * floor((d + 180.0) / 360.0); }
__device__ inline double cross2(double ax, double ay, double bx, double by){ return ax * by - ay * bx; }
__device__ inline double len2(double ax, double ay, double bx, double by){ const double dx = bx - ax, dy = by - ay; return dx * dx + dy * dy; }
__device__ inline double dmax(double a, double b){ return a > b ? a : b; }
__device__ inline double dmin(double a, double b){ return a < b ? a : b; }
__device__ inline double interp(double W0, double W1, double W2, double v0, double v1, double v2){ return ((W0 * v0) + (W1 * v1)) + (W2 * v2); }

// a triangle on its way through the walk: the landing points and turning heights of its corners, where its records are, and its box
struct TubeTri {
    double x0, y0, t0, x1, y1, t1, x2, y2, t2;
    int r0, r1, r2;                               // ray indices of the corners
    int tri, leg, m;
    int row_lo, n_rows;                           // rows of centres proposed
    int c0, w0, c1, w1, c2, w2;                   // up to three disjoint runs of columns: first column, width
};

// cell index of a coordinate, clamped to -1 .. n (a NaN gives n: an empty run)
__device__ inline int cell_of(double c, double o, double s, int n){
    const double q = floor((c - o) / s);
    if(!(q >= -1.0)) return q < 0.0 ? -1 : n;
    return q < (double)n ? (int)q : n;
}

// columns lo - 1 .. hi + 1 clipped to the grid and to the columns after `after`: first column and width
__device__ inline void col_run(double lo, double hi, const TubeDev& D, int after, int* first, int* width){
    int a = cell_of(lo, 0.0, D.s1, D.n1) - 1, b = cell_of(hi, 0.0, D.s1, D.n1) + 1;
    if(a <= after) a = after + 1;
    if(b > D.n1 - 1) b = D.n1 - 1;
    *first = a; *width = b >= a ? b - a + 1 : 0;
}

// the filters that do not depend on the centre, and the box.  false: the triangle proposes nothing.
// The side test here is not the header's: it uses longitudes relative to corner 0 instead of relative to the centre, and its bound is twice
// edge_max plus 2^-40 of the largest coordinate a corner of a hit can have (the grid's extent plus edge_max), so that rounding never makes it
// remove a triangle the exact test (tube_test) would keep at some centre.
__device__ inline bool tube_box(const TubeDev& D, const double4& a, const double4& b, const double4& c, TubeTri* T){
    if(!(a.w != 0.0 && b.w != 0.0 && c.w != 0.0)) return false;
    const double tmx = dmax(dmax(a.z, b.z), c.z), tmn = dmin(dmin(a.z, b.z), c.z);
    if(!(tmx - tmn <= D.turn_tol)) return false;
    // offsets along axis 1 from the grid's origin; spherical: corner 0 into 0 .. 360, corners 1 and 2 within 180 degrees of it
    double l0 = a.y - D.o1, l1, l2;
    if(D.spherical){
        l0 = l0 - 360.0 * floor(l0 / 360.0);
        l1 = l0 + wrap180(b.y - a.y);
        l2 = l0 + wrap180(c.y - a.y);
    } else { l1 = b.y - D.o1; l2 = c.y - D.o1; }
    const double e2 = dmax(dmax(len2(a.x, l0, b.x, l1), len2(b.x, l1, c.x, l2)), len2(c.x, l2, a.x, l0));
    if(!(e2 <= D.pre2)) return false;
    const double xlo = dmin(dmin(a.x, b.x), c.x), xhi = dmax(dmax(a.x, b.x), c.x);
    int r_lo = cell_of(xlo, D.o0, D.s0, D.n0) - 1, r_hi = cell_of(xhi, D.o0, D.s0, D.n0) + 1;
    if(r_lo < 0) r_lo = 0;
    if(r_hi > D.n0 - 1) r_hi = D.n0 - 1;
    T->row_lo = r_lo; T->n_rows = r_hi >= r_lo ? r_hi - r_lo + 1 : 0;
    const double llo = dmin(dmin(l0, l1), l2), lhi = dmax(dmax(l0, l1), l2);
    T->w0 = 0; T->w2 = 0; T->c0 = 0; T->c2 = 0;
    if(D.spherical){
        // a centre at offset u is proposed when u + 360 k lies in the box for k = 1, 0 or -1: three runs in ascending column order, kept disjoint
        col_run(llo - 360.0, lhi - 360.0, D, -1, &T->c0, &T->w0);
        col_run(llo, lhi, D, T->w0 ? T->c0 + T->w0 - 1 : -1, &T->c1, &T->w1);
        const int last = T->w1 ? T->c1 + T->w1 - 1 : (T->w0 ? T->c0 + T->w0 - 1 : -1);
        col_run(llo + 360.0, lhi + 360.0, D, last, &T->c2, &T->w2);
    } else col_run(llo, lhi, D, -1, &T->c1, &T->w1);
    T->x0 = a.x; T->y0 = a.y; T->t0 = a.z; T->x1 = b.x; T->y1 = b.y; T->t1 = b.z; T->x2 = c.x; T->y2 = c.y; T->t2 = c.z;
    return T->n_rows > 0 && (T->w0 + T->w1 + T->w2) > 0;
}

// candidate k of a triangle's box -> the cell (i0, i1)
__device__ inline void tube_cand(const TubeTri& T, int k, int* i0, int* i1){
    const int w = T.w0 + T.w1 + T.w2;
    const int r = k / w, c = k - r * w;
    *i0 = T.row_lo + r;
    *i1 = c < T.w0 ? T.c0 + c : (c < T.w0 + T.w1 ? T.c1 + (c - T.w0) : T.c2 + (c - T.w0 - T.w1));
}

// the exact test of geoac_stations.h at the centre of cell (i0, i1), the turning band, and the reductions of a hit
template <int PASS>
__device__ inline void tube_test(const TubeDev& D, const TubeTri& T, int i0, int i1){
    const double s0 = D.o0 + ((double)i0 + 0.5) * D.s0, s1 = D.o1 + ((double)i1 + 0.5) * D.s1;
    const double x0 = T.x0 - s0, x1 = T.x1 - s0, x2 = T.x2 - s0;
    double y0 = T.y0 - s1, y1 = T.y1 - s1, y2 = T.y2 - s1;
    if(D.spherical){ y0 = wrap180(y0); y1 = wrap180(y1); y2 = wrap180(y2); }
    const double e2 = dmax(dmax(len2(x0, y0, x1, y1), len2(x1, y1, x2, y2)), len2(x2, y2, x0, y0));
    if(!(e2 <= D.edge2)) return;
    const double w0 = cross2(x1, y1, x2, y2), w1 = cross2(x2, y2, x0, y0), w2 = cross2(x0, y0, x1, y1);
    const double s = (w0 + w1) + w2;
    if(!(s != 0.0 && ((w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) || (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0)))) return;
    const double W0 = w0 / s, W1 = w1 / s, W2 = w2 / s;
    const double turn = interp(W0, W1, W2, T.t0, T.t1, T.t2);
    if(!(turn >= D.turn_min && turn < D.turn_max)) return;
    const long long per_m = (long long)D.n_rays * D.legs;
    const long long q0 = (long long)T.r0 * D.legs + T.leg, q1 = (long long)T.r1 * D.legs + T.leg, q2 = (long long)T.r2 * D.legs + T.leg;
    const long long cell = (long long)i0 * D.n1 + i1;
    if(PASS == 0){
        const double* R0 = D.rec + ((long long)T.m * per_m + q0) * GEOAC_REC_STRIDE;
        const double* R1 = D.rec + ((long long)T.m * per_m + q1) * GEOAC_REC_STRIDE;
        const double* R2 = D.rec + ((long long)T.m * per_m + q2) * GEOAC_REC_STRIDE;
        const double tt = interp(W0, W1, W2, R0[GEOAC_REC_TTIME], R1[GEOAC_REC_TTIME], R2[GEOAC_REC_TTIME]);
        const double rg = interp(W0, W1, W2, R0[GEOAC_REC_RANGE], R1[GEOAC_REC_RANGE], R2[GEOAC_REC_RANGE]);
        const long long b = (long long)T.m * D.cells + cell;
        const long long mc = (long long)D.M * D.cells;
        atomicAdd(&D.count[b], 1ull);
        atomicMin(&D.count[mc + b], tube_key(tt));
        atomicMax(&D.count[2 * mc + b], tube_key(rg / tt));
    }
    const unsigned long long key = (unsigned long long)((long long)T.leg * (2ll * D.n_cells) + T.tri);
    for(int f = 0; f < D.F; f++){
        const double* L = D.level + ((long long)T.m * D.F + f) * per_m;
        const double lv = interp(W0, W1, W2, L[q0], L[q1], L[q2]);
        if(!isfinite(lv)) continue;
        const long long b = ((long long)T.m * D.F + f) * D.cells + cell;
        if(PASS == 0) atomicMax(&D.lvl[b], tube_key(lv));
        else if(D.lvl[b] == tube_key(lv)) atomicMin(&D.lvl[(long long)D.M * D.F * D.cells + b], key);
    }
}

__device__ inline int bcast(int v, int src){ return __shfl(v, src, 64); }
// (a broadcast triangle travels through vector registers: in scalar registers, beside the kernel's arguments, it would spill)
__device__ inline double bcast(double v, int src){ return __shfl(v, src, 64); }

// the walk's arguments into device memory: k_tube_raster reads them from there as it needs them (as kernel arguments they would all be held
// in scalar registers at once, more than the walk leaves free)
__global__ void k_tube_args(TubeDev D, TubeDev* out){
    if(blockIdx.x == 0 && threadIdx.x == 0) *out = D;
}

// one lane per (member, leg, lattice cell); every lane of a wave makes the same number of trips, so that the ballots below see whole waves.
// Blocks of one wave: a fan has few thousand waves of work and their cost is uneven, so the waves are spread over the CUs one by one.
template <int PASS>
__global__ void __launch_bounds__(64) k_tube_raster(const TubeDev* __restrict__ Dp, long long n_items){
    const TubeDev& D = *Dp;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    const int nt1 = D.n_theta - 1;
    unsigned n_tri = 0, n_coop = 0, n_cand = 0;
    for(long long base = wave * 64; base < n_items; base += n_waves * 64){
        const long long item = base + lane;
        const bool live = item < n_items;
        int cell = 0, li = 0, m = 0;
        if(live){ cell = (int)(item % D.n_cells); const long long ml = item / D.n_cells; li = (int)(ml % D.n_legs); m = (int)(ml / D.n_legs); }
        const int leg = D.leg0 + li;
        const int i = cell % nt1, j = cell / nt1;
        const int jn = (j + 1 == D.n_phi) ? 0 : j + 1;       // (only a periodic lattice has a cell in its last column)
        const int ra = j * D.n_theta + i, rb = ra + 1, rd = jn * D.n_theta + i, rc = rd + 1;
        const double4* land = D.land + ((long long)m * D.legs + leg) * D.n_rays;
        double4 ca = make_double4(0.0, 0.0, 0.0, 0.0), cc = ca;
        if(live){ ca = land[ra]; cc = land[rc]; }
        const bool ac = live && ca.w != 0.0 && cc.w != 0.0;   // (both triangles hold corners a and c)
#pragma unroll 1
        for(int t = 0; t < 2; t++){
            TubeTri T;
            bool ok = false;
            if(ac){
                const double4 co = land[t == 0 ? rb : rd];
                ok = t == 0 ? tube_box(D, ca, co, cc, &T) : tube_box(D, ca, cc, co, &T);
                T.r0 = ra; T.r1 = t == 0 ? rb : rc; T.r2 = t == 0 ? rc : rd;
                T.tri = 2 * cell + t; T.leg = leg; T.m = m;
            }
            const int n = ok ? T.n_rows * (T.w0 + T.w1 + T.w2) : 0;
            const bool big = n > D.coop_min;
            if(ok){ n_tri++; n_cand += (unsigned)n; }
            if(ok && !big)
                for(int k = 0; k < n; k++){
                    int i0, i1;
                    tube_cand(T, k, &i0, &i1);
                    tube_test<PASS>(D, T, i0, i1);
                }
            unsigned long long todo = __ballot(big);
            while(todo){
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1;
                if(lane == src) n_coop++;
                TubeTri U;
                U.x0 = bcast(T.x0, src); U.y0 = bcast(T.y0, src); U.t0 = bcast(T.t0, src);
                U.x1 = bcast(T.x1, src); U.y1 = bcast(T.y1, src); U.t1 = bcast(T.t1, src);
                U.x2 = bcast(T.x2, src); U.y2 = bcast(T.y2, src); U.t2 = bcast(T.t2, src);
                U.r0 = bcast(T.r0, src); U.r1 = bcast(T.r1, src); U.r2 = bcast(T.r2, src);
                U.tri = bcast(T.tri, src); U.leg = bcast(T.leg, src); U.m = bcast(T.m, src);
                U.row_lo = bcast(T.row_lo, src); U.n_rows = bcast(T.n_rows, src);
                U.c0 = bcast(T.c0, src); U.w0 = bcast(T.w0, src); U.c1 = bcast(T.c1, src); U.w1 = bcast(T.w1, src); U.c2 = bcast(T.c2, src); U.w2 = bcast(T.w2, src);
                const int nu = U.n_rows * (U.w0 + U.w1 + U.w2);
                for(int k = lane; k < nu; k += 64){
                    int i0, i1;
                    tube_cand(U, k, &i0, &i1);
                    tube_test<PASS>(D, U, i0, i1);
                }
            }
        }
    }
    if(PASS == 0){
        for(int off = 32; off > 0; off >>= 1){
            n_tri += (unsigned)__shfl_xor((int)n_tri, off, 64);
            n_coop += (unsigned)__shfl_xor((int)n_coop, off, 64);
        }
        unsigned long long c64 = n_cand;
        for(int off = 32; off > 0; off >>= 1){
            const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(c64 & 0xffffffffull), off, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(c64 >> 32), off, 64);
            c64 += ((unsigned long long)hi << 32) | lo;
        }
        if(lane == 0 && n_tri){
            atomicAdd(&D.stats[0], (unsigned long long)n_tri);
            if(n_coop) atomicAdd(&D.stats[1], (unsigned long long)n_coop);
            atomicAdd(&D.stats[2], c64);
        }
    }
}

// one thread per (m, f, cell): keys back to doubles in place, empty-cell markers
__global__ void k_tube_finish(TubeDev D){
    const long long n = D.cells * D.M * D.F;
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned long long* ttime = D.count + D.cells * D.M; unsigned long long* cel = ttime + D.cells * D.M; unsigned long long* best = D.lvl + n;
    const unsigned long long p_inf = 0x7ff0000000000000ull, m_inf = 0xfff0000000000000ull;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride){
        const unsigned long long k = D.lvl[i];
        if(k == 0ull){ D.lvl[i] = m_inf; best[i] = ~0ull; }
        else D.lvl[i] = (unsigned long long)__double_as_longlong(tube_unkey(k));
        const long long c = i % D.cells, mf = i / D.cells;
        if(mf % D.F == 0){
            const long long b = (mf / D.F) * D.cells + c;
            const bool any = D.count[b] != 0ull;
            ttime[b] = any ? (unsigned long long)__double_as_longlong(tube_unkey(ttime[b])) : p_inf;
            cel[b] = any ? (unsigned long long)__double_as_longlong(tube_unkey(cel[b])) : m_inf;
        }
    }
}

// one thread per (f, cell): members whose LEVEL_MAX reaches detect_db
__global__ void k_tube_detect(TubeDev D){
    const long long n = D.cells * D.F;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride){
        const long long c = i % D.cells, f = i / D.cells;
        unsigned hits = 0;
        for(int m = 0; m < D.M; m++){
            const double lv = __longlong_as_double((long long)D.lvl[((long long)m * D.F + f) * D.cells + c]);
            hits += lv >= D.detect_db ? 1u : 0u;
        }
        D.detect[i] = hits;
    }
}

static_assert(sizeof(TubeDev) <= 512, "TubeState::args holds one TubeDev");

struct TubeState {
    void* layers = nullptr; size_t layers_cap = 0;
    void* land = nullptr; size_t land_cap = 0;
    void* args = nullptr; size_t args_cap = 0;           // the walk's arguments (k_tube_args)
    unsigned long long tube_gen = 0, land_gen = 0;        // the context's invalidation counter they were made at (0: never)
    geoac_tube_spec spec{};
    int M = 0, F = 0;
    long long cells = 0;
    bool detect = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    size_t mc() const { return (size_t)M * (size_t)cells; }
    size_t mfc() const { return mc() * (size_t)F; }
};

unsigned blocks_for(long long n, long long cap){ long long b = (n + 255) / 256; if(b < 1) b = 1; if(b > cap) b = cap; return (unsigned)b; }

int grow(void** p, size_t* cap, size_t need){
    if(*p && *cap >= need) return GEOAC_OK;
    if(*p){ hipFree(*p); *p = nullptr; *cap = 0; }                  // (hipFree waits for the work that may still read it)
    if(hipMalloc(p, need ? need : 8) != hipSuccess){ (void)hipGetLastError(); *p = nullptr; return GEOAC_E_NOMEM; }
    *cap = need;
    return GEOAC_OK;
}

bool spherical(int eqset){ return eqset == GEOAC_EQ_GLOBAL || eqset == GEOAC_EQ_GLOBAL_RNGDEP; }

// the first thing wrong with a spec, or NULL; *code the status it earns
const char* spec_fault(int eqset, const geoac_tube_spec* s, int n_rays, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){
        *code = GEOAC_E_UNSUPPORTED;
        return "not implemented for the 2-D set: a fan on one axis has no landing triangles (geoac_fan_map bins its arrivals)";
    }
    if(!s) return "spec is NULL";
    // the grid and the bands, as geoac_map_check has them
    for(int a = 0; a < 2; a++){
        if(!std::isfinite(s->origin[a])) return "origin must be finite";
        if(!std::isfinite(s->step[a]) || !(s->step[a] > 0.0)) return "step must be finite and greater than 0";
        if(s->n[a] < 1) return "n must be at least 1 per axis";
    }
    if((long long)s->n[0] * s->n[1] > (long long)GEOAC_MAP_MAX_CELLS) return "n[0] * n[1] exceeds GEOAC_MAP_MAX_CELLS (2^24)";
    if(s->wrap_lon != 0 && s->wrap_lon != 1) return "wrap_lon must be 0 or 1";
    if(s->wrap_lon && !spherical(eqset)) return "wrap_lon is for the spherical sets only (a Cartesian set has no longitude)";
    if(std::isnan(s->turn_min) || std::isnan(s->turn_max) || !(s->turn_min < s->turn_max)) return "turning-height band: need turn_min < turn_max, neither NaN (-inf / +inf: no bound)";
    // the lattice and the triangle filters: geoac_station_check's own verdict on the shared fields
    geoac_station_spec st;
    st.n_theta = s->n_theta; st.n_phi = s->n_phi; st.phi_periodic = s->phi_periodic; st.leg_min = s->leg_min; st.leg_max = s->leg_max;
    st.turn_tol = s->turn_tol; st.edge_max = s->edge_max; st.cap = 1;
    if(const char* f = geoac_station_fault(eqset, &st, n_rays, 1)) return f;
    if(!std::isfinite(s->edge_max)) return "edge_max must be finite: it bounds the cells a landing triangle can cover";
    if(spherical(eqset)){
        if(!(s->edge_max < 180.0)) return "edge_max must be below 180 degrees on the spherical sets";
        if(!((double)s->n[1] * s->step[1] <= 360.0)) return "n[1] * step[1] must not exceed 360 degrees on the spherical sets";
    }
    const double span = (2.0 * s->edge_max / s->step[0] + 3.0) * (2.0 * s->edge_max / s->step[1] + 3.0);
    if(!(span <= (double)GEOAC_TUBE_MAX_SPAN)) return "candidate span (2 edge_max / step[0] + 3) * (2 edge_max / step[1] + 3) exceeds GEOAC_TUBE_MAX_SPAN (2^20): lower edge_max or coarsen the grid";
    return nullptr;
}

bool same_bits(double a, double b){ uint64_t x, y; memcpy(&x, &a, 8); memcpy(&y, &b, 8); return x == y; }

struct Bound { geoac_ctx* ctx; GeoacTubeView v; TubeState* st; };

int bind(geoac_ctx* ctx, const char* what, bool create, Bound* b){
    if(!ctx) return GEOAC_E_INVALID;
    b->ctx = ctx;
    int rc = geoac_tube_view(ctx, &b->v);
    if(rc) return rc;
    if(!b->v.map.fresh)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no completed launch, or new angles, an atmosphere upload, geoac_set_sources or "
                                                     "geoac_set_frequencies have come since it (launch again)").c_str());
    if(!*b->v.state && create) *b->v.state = new TubeState();
    b->st = (TubeState*)*b->v.state;
    if(hipSetDevice(b->v.map.device) != hipSuccess) return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": hipSetDevice failed").c_str());
    return GEOAC_OK;
}

// a current tube map, or GEOAC_E_INVALID
int bind_map(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = bind(ctx, what, false, b);
    if(rc) return rc;
    if(!b->st || b->st->tube_gen != b->v.map.gen)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no tube map of the last completed launch (call geoac_fan_tubemap after geoac_fan_launch)").c_str());
    return GEOAC_OK;
}

int hip_fail(geoac_ctx* ctx, const char* what, hipError_t e){
    return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}
#define TUBECHK(what, call) do { hipError_t e_ = (call); if(e_ != hipSuccess) return hip_fail(b.ctx, what, e_); } while(0)

// byte offset and size of a layer inside the allocation
void layer_span(const TubeState* st, int layer, size_t* off, size_t* bytes){
    const size_t mc = st->mc() * 8, mfc = st->mfc() * 8;
    switch(layer){
    case GEOAC_TUBE_COUNT:     *off = 0;            *bytes = mc;  break;
    case GEOAC_TUBE_TTIME_MIN: *off = mc;           *bytes = mc;  break;
    case GEOAC_TUBE_CEL_MAX:   *off = 2 * mc;       *bytes = mc;  break;
    case GEOAC_TUBE_LEVEL_MAX: *off = 3 * mc;       *bytes = mfc; break;
    default:                   *off = 3 * mc + mfc; *bytes = mfc; break;
    }
}
size_t stats_off(const TubeState* st){ return 3 * st->mc() * 8 + 2 * st->mfc() * 8; }
size_t detect_off(const TubeState* st){ return stats_off(st) + 4 * 8; }
size_t detect_bytes(const TubeState* st){ return (size_t)st->F * (size_t)st->cells * 4; }

int fetch(Bound& b, const char* what, void* host, size_t off, size_t bytes){
    TUBECHK(what, hipMemcpyAsync(host, (const char*)b.st->layers + off, bytes, hipMemcpyDeviceToHost, (hipStream_t)b.v.map.stream));
    TUBECHK(what, hipStreamSynchronize((hipStream_t)b.v.map.stream));
    return GEOAC_OK;
}

}  // namespace

extern "C" void geoac_tube_release(void* state){
    TubeState* st = (TubeState*)state;
    if(!st) return;
    if(st->layers) hipFree(st->layers);
    if(st->land) hipFree(st->land);
    if(st->args) hipFree(st->args);
    if(st->e0) hipEventDestroy(st->e0);
    if(st->e1) hipEventDestroy(st->e1);
    delete st;
}

extern "C" const char* geoac_tube_fault(int eqset, const geoac_tube_spec* spec, int n_rays){
    int code;
    return spec_fault(eqset, spec, n_rays, &code);
}

extern "C" int geoac_tube_check(int eqset, const geoac_tube_spec* spec, int n_rays, int64_t* cells){
    int code;
    if(spec_fault(eqset, spec, n_rays, &code)) return code;
    if(cells) *cells = (int64_t)spec->n[0] * spec->n[1];
    return GEOAC_OK;
}

extern "C" int geoac_fan_tubemap(geoac_ctx* ctx, const geoac_tube_spec* spec){
    const char* what = "fan_tubemap";
    Bound b;
    int rc = bind(ctx, what, true, &b);
    if(rc) return rc;
    const GeoacMapView& v = b.v.map;
    int code;
    if(const char* fault = spec_fault(v.eqset, spec, v.n_rays, &code)) return geoac_map_fail(ctx, code, (std::string("fan_tubemap: ") + fault).c_str());
    const int nt = spec->n_theta, np = spec->n_phi;
    if(b.v.n_ang != v.n_rays || !b.v.theta_deg || !b.v.phi_deg) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_tubemap: the context holds no launch angles for the records");
    for(int j = 0; j < np; j++)
        for(int i = 0; i < nt; i++)
            if(!same_bits(b.v.theta_deg[(size_t)j * nt + i], b.v.theta_deg[i]) || !same_bits(b.v.phi_deg[(size_t)j * nt + i], b.v.phi_deg[(size_t)j * nt]))
                return geoac_map_fail(ctx, GEOAC_E_INVALID, ("fan_tubemap: the launch angles are not an n_theta x n_phi lattice (ray " + std::to_string((size_t)j * nt + i) +
                                                             " differs from its row's theta or its column's phi; ray = j * n_theta + i, the order of geoac_fan_enumerate)").c_str());
    TubeState* st = b.st;
    hipStream_t s = (hipStream_t)v.stream;
    st->tube_gen = 0;                                  // (no current tube map until this one is complete)
    if(!st->e0){ TUBECHK(what, hipEventCreate(&st->e0)); TUBECHK(what, hipEventCreate(&st->e1)); }
    TUBECHK(what, hipEventRecord(st->e0, s));
    void* level = nullptr; size_t level_bytes = 0;
    if((rc = geoac_fan_level_dev(ctx, &level, &level_bytes))) return rc;         // (formed on first use after a launch, geoac_map.hip)
    st->spec = *spec; st->M = v.M; st->F = v.F;
    st->cells = (long long)spec->n[0] * spec->n[1];
    st->detect = !std::isnan(spec->detect_db);
    const size_t n_land = (size_t)v.M * v.legs * v.n_rays;
    const size_t need = detect_off(st) + ((detect_bytes(st) + 7) & ~(size_t)7);
    if(grow(&st->layers, &st->layers_cap, need) || grow(&st->land, &st->land_cap, sizeof(double4) * n_land) || grow(&st->args, &st->args_cap, 512))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_tubemap: no device memory for the layers (" + std::to_string(need >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(v.F) + " frequencies x " + std::to_string(st->cells) + " cells)").c_str());
    TubeDev D{};
    D.rec = v.rec; D.level = (const double*)level; D.land = (double4*)st->land;
    char* base = (char*)st->layers;
    size_t off, bytes;
    layer_span(st, GEOAC_TUBE_COUNT, &off, &bytes);     D.count = (unsigned long long*)(base + off);
    layer_span(st, GEOAC_TUBE_LEVEL_MAX, &off, &bytes); D.lvl = (unsigned long long*)(base + off);
    D.stats = (unsigned long long*)(base + stats_off(st));
    D.detect = (unsigned*)(base + detect_off(st));
    D.o0 = spec->origin[0]; D.o1 = spec->origin[1]; D.s0 = spec->step[0]; D.s1 = spec->step[1]; D.n0 = spec->n[0]; D.n1 = spec->n[1];
    D.turn_tol = spec->turn_tol; D.edge2 = spec->edge_max * spec->edge_max; 
    const double mag = (fabs(spec->origin[0]) + spec->n[0] * spec->step[0]) + (fabs(spec->origin[1]) + spec->n[1] * spec->step[1]) + (spherical(v.eqset) ? 720.0 : 0.0);
    const double pre = 2.0 * spec->edge_max + kTubeSlack * (mag + spec->edge_max);
    D.pre2 = pre * pre;
    D.turn_min = spec->turn_min; D.turn_max = spec->turn_max; D.detect_db = spec->detect_db;
    D.spherical = spherical(v.eqset) ? 1 : 0;
    D.M = v.M; D.F = v.F; D.n_rays = v.n_rays; D.legs = v.legs; D.n_theta = nt; D.n_phi = np;
    D.leg0 = spec->leg_min;
    const int leg_last = spec->leg_max < v.legs - 1 ? spec->leg_max : v.legs - 1;
    D.n_legs = leg_last >= D.leg0 ? leg_last - D.leg0 + 1 : 0;
    D.n_cells = (nt - 1) * (spec->phi_periodic ? np : np - 1);
    D.cells = st->cells;
    // GEOAC_TUBE_COOP (diagnostic, tools/perf_tubemap.py): another threshold for the cooperative walk; the layers do not depend on it
    D.coop_min = GEOAC_TUBE_COOP_MIN;
    if(const char* e = getenv("GEOAC_TUBE_COOP")){ const long t = strtol(e, nullptr, 10); if(t >= 0 && t <= 0x7fffffffl) D.coop_min = (int)t; }
    const long long n_items = (long long)v.M * D.n_legs * D.n_cells;
    const long long n_mc = (long long)st->mc(), n_mfc = (long long)st->mfc(), n_words = (long long)(need / 8);
    if(st->land_gen != v.gen){
        hipLaunchKernelGGL(k_tube_prep, dim3(blocks_for((long long)n_land, 1ll << 20)), dim3(256), 0, s, D);
        TUBECHK(what, hipGetLastError());
        st->land_gen = v.gen;
    }
    hipLaunchKernelGGL(k_tube_fill, dim3(blocks_for(n_words, 1ll << 20)), dim3(256), 0, s, (unsigned long long*)st->layers, n_mc, n_mfc, n_words);
    if(n_items > 0){
        const unsigned n_blk = blocks_for(n_items * 4, 1ll << 18);       // (one wave of 64 items per block)
        hipLaunchKernelGGL(k_tube_args, dim3(1), dim3(64), 0, s, D, (TubeDev*)st->args);
        hipLaunchKernelGGL(k_tube_raster<0>, dim3(n_blk), dim3(64), 0, s, (const TubeDev*)st->args, n_items);
        hipLaunchKernelGGL(k_tube_raster<1>, dim3(n_blk), dim3(64), 0, s, (const TubeDev*)st->args, n_items);
    }
    hipLaunchKernelGGL(k_tube_finish, dim3(blocks_for(n_mfc, 1ll << 20)), dim3(256), 0, s, D);
    if(st->detect) hipLaunchKernelGGL(k_tube_detect, dim3(blocks_for(st->cells * v.F, 1ll << 20)), dim3(256), 0, s, D);
    TUBECHK(what, hipGetLastError());
    TUBECHK(what, hipEventRecord(st->e1, s));
    st->tube_gen = v.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_tubemap_shape(geoac_ctx* ctx, int* n_members, int* n_freq, int* n0, int* n1){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_shape", &b);
    if(rc) return rc;
    if(n_members) *n_members = b.st->M;
    if(n_freq) *n_freq = b.st->F;
    if(n0) *n0 = b.st->spec.n[0];
    if(n1) *n1 = b.st->spec.n[1];
    return GEOAC_OK;
}

extern "C" int geoac_fan_tubemap_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_dev", &b);
    if(rc) return rc;
    if(layer < 0 || layer >= GEOAC_TUBE_LAYERS) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_tubemap_dev: unknown layer");
    size_t off, n;
    layer_span(b.st, layer, &off, &n);
    if(dev_ptr) *dev_ptr = (char*)b.st->layers + off;
    if(bytes) *bytes = n;
    return GEOAC_OK;
}

extern "C" int geoac_fan_tubemap_fetch(geoac_ctx* ctx, int layer, void* host){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_fetch", &b);
    if(rc) return rc;
    if(layer < 0 || layer >= GEOAC_TUBE_LAYERS || !host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_tubemap_fetch: unknown layer / NULL buffer");
    size_t off, n;
    layer_span(b.st, layer, &off, &n);
    return fetch(b, "fan_tubemap_fetch", host, off, n);
}

extern "C" int geoac_fan_tubemap_fetch_detect(geoac_ctx* ctx, uint32_t* detect_host){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_fetch_detect", &b);
    if(rc) return rc;
    if(!detect_host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_tubemap_fetch_detect: NULL buffer");
    if(!b.st->detect) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_tubemap_fetch_detect: the tube map was made without a detection threshold (detect_db = NaN)");
    return fetch(b, "fan_tubemap_fetch_detect", detect_host, detect_off(b.st), detect_bytes(b.st));
}

extern "C" int geoac_fan_tubemap_stats(geoac_ctx* ctx, uint64_t* stats4){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_stats", &b);
    if(rc) return rc;
    if(!stats4) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_tubemap_stats: NULL buffer");
    return fetch(b, "fan_tubemap_stats", stats4, stats_off(b.st), 4 * 8);
}

extern "C" int geoac_fan_tubemap_timing(geoac_ctx* ctx, double* ms){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_tubemap_timing: NULL argument");
    TUBECHK("fan_tubemap_timing", hipEventSynchronize(b.st->e1));
    float t = 0;
    TUBECHK("fan_tubemap_timing", hipEventElapsedTime(&t, b.st->e0, b.st->e1));
    *ms = t;
    return GEOAC_OK;
}
