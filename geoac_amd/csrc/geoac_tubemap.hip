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
// Makefile gives the same flag).  The rule at a centre is that of geoac_tri_rule.h, which geoac_stations.hip uses at a station.  The box, the
// enumeration of its candidates and the wave's walk are geoac_tube_walk.h, which geoac_ltubemap.hip runs over crossing triangles; what is this
// file's own is where a corner comes from (the landing table), its two filters, and what a hit reduces (tube_test).
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
#include "geoac_tube_walk.h"

#pragma clang fp contract(off)

namespace {

struct TubeDev {
    WalkGrid G;                                   // the grid, the square of the bound of walk_box's side test, the cooperative threshold
    const double* rec; const double* level;       // the launch's tables
    const double4* land;                          // [M][legs][n_rays]: c0, c1, turn, valid
    unsigned long long *count, *lvl, *stats;      // COUNT | TTIME_MIN | CEL_MAX follow one another, M * cells words each; LEVEL_MAX | BEST, M * F * cells each
    unsigned* detect;
    double turn_tol, edge2;                       // edge2 = edge_max * edge_max
    double turn_min, turn_max, detect_db;
    int M, F, n_rays, legs, n_theta, n_phi;
    int leg0, n_legs, n_cells;                    // legs leg0 .. leg0 + n_legs - 1 take part; cells of the lattice
    long long cells;                              // n0 * n1
};

// the filters that do not depend on the centre (all three corners valid, the turning heights within turn_tol), then the box of geoac_tube_walk.h
__device__ inline bool tube_box(const TubeDev& D, const double4& a, const double4& b, const double4& c, WalkTri* T){
    if(!(a.w != 0.0 && b.w != 0.0 && c.w != 0.0)) return false;
    const double tmx = dmax(dmax(a.z, b.z), c.z), tmn = dmin(dmin(a.z, b.z), c.z);
    if(!(tmx - tmn <= D.turn_tol)) return false;
    return walk_box(D.G, a, b, c, T);
}

// the exact test of geoac_stations.h at the centre of cell (i0, i1), the turning band, and the reductions of a hit
template <int PASS>
__device__ inline void tube_test(const TubeDev& D, const WalkTri& T, int i0, int i1){
    const double s0 = D.G.o0 + ((double)i0 + 0.5) * D.G.s0, s1 = D.G.o1 + ((double)i1 + 0.5) * D.G.s1;
    const double x0 = T.x0 - s0, x1 = T.x1 - s0, x2 = T.x2 - s0;
    double y0 = T.y0 - s1, y1 = T.y1 - s1, y2 = T.y2 - s1;
    if(D.G.spherical){ y0 = wrap180(y0); y1 = wrap180(y1); y2 = wrap180(y2); }
    const Tri R = tri_rule(x0, y0, x1, y1, x2, y2, D.edge2);
    if(!R.hit) return;
    const double W0 = R.w0 / R.s, W1 = R.w1 / R.s, W2 = R.w2 / R.s;
    const double turn = interp(W0, W1, W2, T.z0, T.z1, T.z2);
    if(!(turn >= D.turn_min && turn < D.turn_max)) return;
    const long long per_m = (long long)D.n_rays * D.legs;
    const long long q0 = (long long)T.r0 * D.legs + T.plane, q1 = (long long)T.r1 * D.legs + T.plane, q2 = (long long)T.r2 * D.legs + T.plane;
    const long long cell = (long long)i0 * D.G.n1 + i1;
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
    const unsigned long long key = (unsigned long long)((long long)T.plane * (2ll * D.n_cells) + T.tri);
    for(int f = 0; f < D.F; f++){
        const double* L = D.level + ((long long)T.m * D.F + f) * per_m;
        const double lv = interp(W0, W1, W2, L[q0], L[q1], L[q2]);
        if(!isfinite(lv)) continue;
        const long long b = ((long long)T.m * D.F + f) * D.cells + cell;
        if(PASS == 0) atomicMax(&D.lvl[b], geoac_key(lv));
        else if(D.lvl[b] == geoac_key(lv)) atomicMin(&D.lvl[(long long)D.M * D.F * D.cells + b], key);
    }
}

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
    WalkCount C;
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
            WalkTri T;
            bool ok = false;
            if(ac){
                const double4 co = land[t == 0 ? rb : rd];
                ok = t == 0 ? tube_box(D, ca, co, cc, &T) : tube_box(D, ca, cc, co, &T);
                T.r0 = ra; T.r1 = t == 0 ? rb : rc; T.r2 = t == 0 ? rc : rd;
                T.tri = 2 * cell + t; T.plane = leg; T.m = m;
            }
            walk_wave(D.G, ok, T, lane, &C, [&D](const WalkTri& U, int i0, int i1){ tube_test<PASS>(D, U, i0, i1); });
        }
    }
    if(PASS == 0) walk_totals(C, lane, D.stats);
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
    D.G.o0 = spec->origin[0]; D.G.o1 = spec->origin[1]; D.G.s0 = spec->step[0]; D.G.s1 = spec->step[1]; D.G.n0 = spec->n[0]; D.G.n1 = spec->n[1];
    D.turn_tol = spec->turn_tol; D.edge2 = spec->edge_max * spec->edge_max;
    D.G.pre2 = walk_pre2(spec->origin, spec->step, spec->n, spec->edge_max, spherical(v.eqset));
    D.turn_min = spec->turn_min; D.turn_max = spec->turn_max; D.detect_db = spec->detect_db;
    D.G.spherical = spherical(v.eqset) ? 1 : 0;
    D.M = v.M; D.F = v.F; D.n_rays = v.n_rays; D.legs = v.legs; D.n_theta = nt; D.n_phi = np;
    geoac_lattice_extent(spec->leg_min, spec->leg_max, v.legs, nt, np, spec->phi_periodic, &D.leg0, &D.n_legs, &D.n_cells);
    D.cells = L.cells;
    // GEOAC_TUBE_COOP (diagnostic, tools/perf_tubemap.py): another threshold for the cooperative walk; the layers do not depend on it
    D.G.coop_min = GEOAC_TUBE_COOP_MIN;
    if(const char* e = getenv("GEOAC_TUBE_COOP")){ const long t = strtol(e, nullptr, 10); if(t >= 0 && t <= 0x7fffffffl) D.G.coop_min = (int)t; }
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
