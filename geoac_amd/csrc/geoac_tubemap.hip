// geoac_tubemap.hip - tube maps (include/geoac_tubemap.h): the landing triangles of the last completed launch rasterised on a regular grid,
// on the device.
//
// Reads the record table, the level table of geoac_map.hip, the landing table of geoac_stations.hip (land[M][legs][n_rays] of (c0, c1, turn,
// valid), 32 B per corner, in the map's coordinates) and the lattice axes of the launch angles; writes only buffers of its own.  No kernel of
// the launch plan is involved.  The layers are a GeoacLayers of geoac_map.hip, which fills and finishes them; the tail holds the work counters.
//
// Kernels:
//   k_tube_raster   <0>: one lane per (member, leg, lattice cell), the cell's two triangles one after the other.  A triangle that passes the
//                   filters that do not depend on the cell centre proposes a box of centres: the bounding box of its corners in cell-index
//                   space, widened by one cell on every side, clipped to the grid; on the spherical sets the longitudes are first brought within
//                   180 degrees of corner 0 and the box is mapped to the grid's columns modulo 360 (up to three disjoint runs of columns).
//                   The box only proposes: at every proposed centre the exact filters and sign rule of geoac_stations.h decide, so the box has
//                   to be conservative and nothing more.  A box of at most coop_min centres is walked by its lane; the lanes with larger
//                   boxes are balloted, and the wave takes them one at a time: corners and box broadcast, 64 centres per trip.  A hit adds 1
//                   to COUNT and takes part in the key minima / maxima.
//                   <1>: the same walk again; hits whose level equals their cell's LEVEL_MAX compete for BEST with leg * n_tri + tri.
// Every reduction is an integer atomic (u64 add; u64 min / max on the order-preserving key of a double; u64 min on the hit's key), so the
// layers do not depend on the order the hits are seen in.
//
// The arithmetic of the test and of the interpolated values is fixed by the headers and restated in tests/station_reference.py and
// tests/tubemap_reference.py: every product is rounded before it is added, so this file is compiled with contraction off (the pragma below; the
// Makefile gives the same flag).  The rule at a centre is that of geoac_tri_rule.h, which geoac_stations.hip uses at a station.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "../../include/geoac_tubemap.h"
#include "geoac_launch_int.h"
#include "geoac_stations_int.h"
#include "geoac_tubemap_int.h"
#include "geoac_tri_rule.h"

#pragma clang fp contract(off)

namespace {

const double kTubePi = 3.141592653589793238462643;
const double kTubeSlack = 1.0 / 1099511627776.0;      // 2^-40: slack of the station-independent side test, relative to the coordinates' size

struct TubeDev {
    const double* rec; const double* level;       // the launch's tables
    const double4* land;                          // [M][legs][n_rays]: c0, c1, turn, valid
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
    const Tri R = tri_rule(x0, y0, x1, y1, x2, y2, D.edge2);
    if(!R.hit) return;
    const double W0 = R.w0 / R.s, W1 = R.w1 / R.s, W2 = R.w2 / R.s;
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
        atomicMin(&D.count[mc + b], geoac_key(tt));
        atomicMax(&D.count[2 * mc + b], geoac_key(rg / tt));
    }
    const unsigned long long key = (unsigned long long)((long long)T.leg * (2ll * D.n_cells) + T.tri);
    for(int f = 0; f < D.F; f++){
        const double* L = D.level + ((long long)T.m * D.F + f) * per_m;
        const double lv = interp(W0, W1, W2, L[q0], L[q1], L[q2]);
        if(!isfinite(lv)) continue;
        const long long b = ((long long)T.m * D.F + f) * D.cells + cell;
        if(PASS == 0) atomicMax(&D.lvl[b], geoac_key(lv));
        else if(D.lvl[b] == geoac_key(lv)) atomicMin(&D.lvl[(long long)D.M * D.F * D.cells + b], key);
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

static_assert(sizeof(TubeDev) <= 512, "TubeState::args holds one TubeDev");

static_assert(GEOAC_TUBE_COUNT == GEOAC_MAP_COUNT && GEOAC_TUBE_TTIME_MIN == GEOAC_MAP_TTIME_MIN && GEOAC_TUBE_CEL_MAX == GEOAC_MAP_CEL_MAX &&
              GEOAC_TUBE_LEVEL_MAX == GEOAC_MAP_LEVEL_MAX && GEOAC_TUBE_BEST == GEOAC_MAP_BEST && GEOAC_TUBE_LAYERS == GEOAC_MAP_LAYERS, "GeoacLayers numbers the layers as geoac_map.h does");

struct TubeState {
    GeoacLayers L{};                                      // tail: the four work counters
    void* args = nullptr; size_t args_cap = 0;           // the walk's arguments (k_tube_args)
    unsigned long long tube_gen = 0;                      // the context's invalidation counter the map was made at (0: never)
    geoac_tube_spec spec{};
    EventPair ev;
};

// the first thing wrong with a spec, or NULL; *code the status it earns
const char* spec_fault(int eqset, const geoac_tube_spec* s, int n_rays, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){
        *code = GEOAC_E_UNSUPPORTED;
        return "not implemented for the 2-D set: a fan on one axis has no landing triangles (geoac_fan_map bins its arrivals)";
    }
    if(!s) return "spec is NULL";
    if(const char* f = geoac_grid_fault(eqset, s->origin, s->step, s->n, s->wrap_lon, s->turn_min, s->turn_max)) return f;
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

struct Bound { geoac_ctx* ctx; GeoacLaunchView v; TubeState* st; };

int bind(geoac_ctx* ctx, const char* what, bool create, Bound* b){
    int rc = bind_launch(ctx, what, GEOAC_SLOT_TUBE, &b->v);
    if(rc) return rc;
    b->ctx = ctx;
    if(!*b->v.state && create) *b->v.state = new TubeState();
    b->st = (TubeState*)*b->v.state;
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

}  // namespace

extern "C" void geoac_tube_release(void* state){
    TubeState* st = (TubeState*)state;
    if(!st) return;
    if(st->L.base) hipFree(st->L.base);
    if(st->args) hipFree(st->args);
    st->ev.release();
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
    const std::string lattice = geoac_lattice_fault(b.v, nt, np);
    if(!lattice.empty()) return geoac_map_fail(ctx, GEOAC_E_INVALID, ("fan_tubemap: " + lattice).c_str());
    TubeState* st = b.st;
    hipStream_t s = (hipStream_t)v.stream;
    st->tube_gen = 0;                                  // (no current tube map until this one is complete)
    GEOAC_CHK(what, st->ev.start(s));
    void* level = nullptr; size_t level_bytes = 0; const void* land = nullptr;
    if((rc = geoac_fan_level_dev(ctx, &level, &level_bytes))) return rc;         // (formed on first use after a launch, geoac_map.hip)
    if((rc = geoac_sta_land_dev(ctx, what, &land))) return rc;                   // (the same, geoac_stations.hip)
    st->spec = *spec;
    GeoacLayers& L = st->L;
    L.M = v.M; L.F = v.F; L.cells = (long long)spec->n[0] * spec->n[1]; L.tail_words = 4; L.detect = !std::isnan(spec->detect_db);
    if(geoac_layers_grow(&L) || grow(&st->args, &st->args_cap, 512))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_tubemap: no device memory for the layers (" + std::to_string(geoac_layers_bytes(&L) >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(v.F) + " frequencies x " + std::to_string(L.cells) + " cells)").c_str());
    TubeDev D{};
    D.rec = v.rec; D.level = (const double*)level; D.land = (const double4*)land;
    char* base = (char*)L.base;
    size_t off, bytes;
    geoac_layers_span(&L, GEOAC_TUBE_COUNT, &off, &bytes);     D.count = (unsigned long long*)(base + off);
    geoac_layers_span(&L, GEOAC_TUBE_LEVEL_MAX, &off, &bytes); D.lvl = (unsigned long long*)(base + off);
    geoac_layers_tail_span(&L, &off, &bytes);                  D.stats = (unsigned long long*)(base + off);
    geoac_layers_detect_span(&L, &off, &bytes);                D.detect = (unsigned*)(base + off);
    D.o0 = spec->origin[0]; D.o1 = spec->origin[1]; D.s0 = spec->step[0]; D.s1 = spec->step[1]; D.n0 = spec->n[0]; D.n1 = spec->n[1];
    D.turn_tol = spec->turn_tol; D.edge2 = spec->edge_max * spec->edge_max;
    const double mag = (fabs(spec->origin[0]) + spec->n[0] * spec->step[0]) + (fabs(spec->origin[1]) + spec->n[1] * spec->step[1]) + (spherical(v.eqset) ? 720.0 : 0.0);
    const double pre = 2.0 * spec->edge_max + kTubeSlack * (mag + spec->edge_max);
    D.pre2 = pre * pre;
    D.turn_min = spec->turn_min; D.turn_max = spec->turn_max; D.detect_db = spec->detect_db;
    D.spherical = spherical(v.eqset) ? 1 : 0;
    D.M = v.M; D.F = v.F; D.n_rays = v.n_rays; D.legs = v.legs; D.n_theta = nt; D.n_phi = np;
    geoac_lattice_extent(spec->leg_min, spec->leg_max, v.legs, nt, np, spec->phi_periodic, &D.leg0, &D.n_legs, &D.n_cells);
    D.cells = L.cells;
    // GEOAC_TUBE_COOP (diagnostic, tools/perf_tubemap.py): another threshold for the cooperative walk; the layers do not depend on it
    D.coop_min = GEOAC_TUBE_COOP_MIN;
    if(const char* e = getenv("GEOAC_TUBE_COOP")){ const long t = strtol(e, nullptr, 10); if(t >= 0 && t <= 0x7fffffffl) D.coop_min = (int)t; }
    const long long n_items = (long long)v.M * D.n_legs * D.n_cells;
    geoac_layers_fill(&L, s);
    if(n_items > 0){
        const unsigned n_blk = blocks_for(n_items * 4, 256, 1ll << 18);  // (one wave of 64 items per block)
        hipLaunchKernelGGL(k_tube_args, dim3(1), dim3(64), 0, s, D, (TubeDev*)st->args);
        hipLaunchKernelGGL(k_tube_raster<0>, dim3(n_blk), dim3(64), 0, s, (const TubeDev*)st->args, n_items);
        hipLaunchKernelGGL(k_tube_raster<1>, dim3(n_blk), dim3(64), 0, s, (const TubeDev*)st->args, n_items);
    }
    geoac_layers_finish(&L, s);
    if(L.detect) geoac_layers_detect(&L, spec->detect_db, s);
    GEOAC_CHK(what, hipGetLastError());
    GEOAC_CHK(what, st->ev.stop(s));
    st->tube_gen = v.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_tubemap_shape(geoac_ctx* ctx, int* n_members, int* n_freq, int* n0, int* n1){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_shape", &b);
    if(rc) return rc;
    if(n_members) *n_members = b.st->L.M;
    if(n_freq) *n_freq = b.st->L.F;
    if(n0) *n0 = b.st->spec.n[0];
    if(n1) *n1 = b.st->spec.n[1];
    return GEOAC_OK;
}

extern "C" int geoac_fan_tubemap_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_dev", &b);
    return rc ? rc : geoac_layers_dev(ctx, "fan_tubemap_dev", &b.st->L, layer, dev_ptr, bytes);
}

extern "C" int geoac_fan_tubemap_fetch(geoac_ctx* ctx, int layer, void* host){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_fetch", &b);
    return rc ? rc : geoac_layers_fetch(ctx, "fan_tubemap_fetch", &b.st->L, b.v.map.stream, layer, host);
}

extern "C" int geoac_fan_tubemap_fetch_detect(geoac_ctx* ctx, uint32_t* detect_host){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_fetch_detect", &b);
    return rc ? rc : geoac_layers_fetch_detect(ctx, "fan_tubemap_fetch_detect", "tube map", &b.st->L, b.v.map.stream, detect_host);
}

extern "C" int geoac_fan_tubemap_stats(geoac_ctx* ctx, uint64_t* stats4){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_stats", &b);
    return rc ? rc : geoac_layers_fetch_tail(ctx, "fan_tubemap_stats", &b.st->L, b.v.map.stream, stats4);
}

extern "C" int geoac_fan_tubemap_timing(geoac_ctx* ctx, double* ms){
    Bound b;
    int rc = bind_map(ctx, "fan_tubemap_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_tubemap_timing: NULL argument");
    GEOAC_CHK("fan_tubemap_timing", b.st->ev.ms(ms));
    return GEOAC_OK;
}
