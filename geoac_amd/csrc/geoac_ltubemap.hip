// geoac_ltubemap.hip - level tube maps (include/geoac_ltubemap.h): the crossing triangles of the last completed launch rasterised per selected
// level on a regular grid, on the device.
//
// Reads the crossing records (geoac_fan_levels_dev), the branch table of geoac_lstations.hip (geoac_lsta_xland_dev: xland[M][L][B][n_rays] of
// (c0, c1, slot k, present), 32 B per corner, in the map's coordinates) and the lattice shape of the launch angles; writes only buffers of its
// own.  No kernel of the launch plan is involved.
//
// Kernels:
//   k_ltube_args    the walk's arguments into device memory (as kernel arguments they would all be held in scalar registers at once).
//   k_ltube_raster  <0>: one lane per (member, selected level, selected branch, lattice cell), the cell's two triangles one after the other.
//                   A triangle whose three corners hold the branch proposes the candidate box of geoac_tube_walk.h; at every proposed centre
//                   the exact rule of geoac_lstations.h decides (tri_rule of geoac_tri_rule.h on corners relative to the centre).  A hit adds
//                   1 to COUNT and, when its interpolated TTIME and ATTEN are both finite, takes part in the two key minima; the two values
//                   are read from the three corners' crossing records through slot k.
//                   <1>: the same walk again; hits whose TTIME equals their cell's TTIME_MIN compete for FIRST with b * n_tri + tri.
//   k_ltube_finish  one thread per (selected level, cell): keys back to doubles, the empty markers, REACH.
// Every reduction is an integer atomic (u64 add; u64 min on the order-preserving key of a double; u64 min on the hit's key), so the layers do
// not depend on the order the hits are seen in.
//
// The arithmetic is fixed by the headers and restated in tests/lstation_reference.py and tests/ltubemap_reference.py: every product is rounded
// before it is added, so this file is compiled with contraction off (the pragma below; the Makefile gives the same flag).
//
// Index bounds, stated again at each load and store:
//   item < M * Ls * n_br * n_cells, so cell < n_cells, bi < n_br, ls < Ls, m < M;  b < B (branch_of);  l = sel[ls] < L (host: level_mask has no
//   bit at or above L);  corner rays < n_theta * n_phi = n_rays (host check);  record slot k < capL (written by k_lsta_prep);  a proposed centre
//   has i0 < n0, i1 < n1 (walk_box clips), so word < M * Ls * cells = W, and the four layers are W words each.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "../../include/geoac_ltubemap.h"
#include "geoac_launch_int.h"
#include "geoac_lstations_int.h"
#include "geoac_ltubemap_int.h"
#include "geoac_tube_walk.h"

#pragma clang fp contract(off)

namespace {

struct LTubeDev {
    WalkGrid G;
    const double* lrec;                           // [M][n_rays][L][capL][GEOAC_LVL_STRIDE]
    const double4* xland;                         // [M][L][B][n_rays]: c0, c1, slot k, present
    unsigned long long *layers, *stats;           // COUNT | TTIME_MIN | ATTEN_MIN | FIRST, W words each; the three work counters
    double edge2;                                 // edge_max * edge_max
    int M, L, capL, n_rays, n_theta, n_phi;
    int B, ord_max, n_dir, dir_mask;              // branches of the table; directions selected
    int Ls, n_br, n_cells;                        // selected levels; selected branches = n_legs * n_dir * ord_max; cells of the lattice
    int sel[GEOAC_MAX_LEVELS];                    // sel[ls] < L: the selected levels in ascending order
    long long cells, W;                           // n0 * n1; M * Ls * cells
};

// selected branch bi < n_br -> the table's branch b < B
__device__ inline int branch_of(const LTubeDev& D, int bi){
    const int per_leg = D.n_dir * D.ord_max;
    const int li = bi / per_leg, rem = bi - li * per_leg;          // li < n_legs
    const int ds = rem / D.ord_max, o = rem - ds * D.ord_max;      // ds < n_dir, o < ord_max
    const int d = D.dir_mask == 2 ? 1 : ds;
    return (li * 2 + d) * D.ord_max + o;
}

// the exact rule of geoac_lstations.h at the centre of cell (i0, i1), and the reductions of a hit
template <int PASS>
__device__ inline void ltube_test(const LTubeDev& D, const WalkTri& T, int i0, int i1){
    const double s0 = D.G.o0 + ((double)i0 + 0.5) * D.G.s0, s1 = D.G.o1 + ((double)i1 + 0.5) * D.G.s1;
    const double x0 = T.x0 - s0, x1 = T.x1 - s0, x2 = T.x2 - s0;
    double y0 = T.y0 - s1, y1 = T.y1 - s1, y2 = T.y2 - s1;
    if(D.G.spherical){ y0 = wrap180(y0); y1 = wrap180(y1); y2 = wrap180(y2); }
    const Tri R = tri_rule(x0, y0, x1, y1, x2, y2, D.edge2);
    if(!R.hit) return;
    const double W0 = R.w0 / R.s, W1 = R.w1 / R.s, W2 = R.w2 / R.s;
    const int ls = T.plane / D.B, b = T.plane - ls * D.B;          // plane = ls * B + b: ls < Ls, b < B
    const long long l = D.sel[ls];                                 // < L
    // a corner's record: ray r < n_rays, slot k < capL
    const double* R0 = D.lrec + ((((long long)T.m * D.n_rays + T.r0) * D.L + l) * D.capL + (int)T.z0) * GEOAC_LVL_STRIDE;
    const double* R1 = D.lrec + ((((long long)T.m * D.n_rays + T.r1) * D.L + l) * D.capL + (int)T.z1) * GEOAC_LVL_STRIDE;
    const double* R2 = D.lrec + ((((long long)T.m * D.n_rays + T.r2) * D.L + l) * D.capL + (int)T.z2) * GEOAC_LVL_STRIDE;
    const double tt = interp(W0, W1, W2, R0[GEOAC_LVL_TTIME], R1[GEOAC_LVL_TTIME], R2[GEOAC_LVL_TTIME]);
    const double at = interp(W0, W1, W2, R0[GEOAC_LVL_ATTEN], R1[GEOAC_LVL_ATTEN], R2[GEOAC_LVL_ATTEN]);
    const long long word = ((long long)T.m * D.Ls + ls) * D.cells + ((long long)i0 * D.G.n1 + i1);          // < W
    const bool fin = isfinite(tt) && isfinite(at);
    if(PASS == 0){
        atomicAdd(&D.layers[word], 1ull);
        if(fin){
            atomicMin(&D.layers[D.W + word], geoac_key(tt));
            atomicMin(&D.layers[2 * D.W + word], geoac_key(at));
        }
    } else if(fin && D.layers[D.W + word] == geoac_key(tt)){
        const unsigned long long key = (unsigned long long)((long long)b * (2ll * D.n_cells) + T.tri);
        atomicMin(&D.layers[3 * D.W + word], key);
    }
}

__global__ void k_ltube_args(LTubeDev D, LTubeDev* out){
    if(blockIdx.x == 0 && threadIdx.x == 0) *out = D;
}

// one lane per (member, selected level, selected branch, lattice cell); every lane of a wave makes the same number of trips, so that the
// ballots of walk_wave see whole waves.  Blocks of one wave: the waves' cost is uneven, so they are spread over the CUs one by one.
template <int PASS>
__global__ void __launch_bounds__(64) k_ltube_raster(const LTubeDev* __restrict__ Dp, long long n_items){
    const LTubeDev& D = *Dp;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    const int nt1 = D.n_theta - 1;
    WalkCount C;
    for(long long base = wave * 64; base < n_items; base += n_waves * 64){
        const long long item = base + lane;
        const bool live = item < n_items;
        int cell = 0, bi = 0, ls = 0, m = 0;
        if(live){
            cell = (int)(item % D.n_cells); long long q = item / D.n_cells;          // cell < n_cells
            bi = (int)(q % D.n_br); q /= D.n_br;                                     // bi < n_br
            ls = (int)(q % D.Ls); m = (int)(q / D.Ls);                               // ls < Ls, m < M
        }
        const int b = branch_of(D, bi);                                              // < B
        const int i = cell % nt1, j = cell / nt1;
        const int jn = (j + 1 == D.n_phi) ? 0 : j + 1;       // (only a periodic lattice has a cell in its last column)
        const int ra = j * D.n_theta + i, rb = ra + 1, rd = jn * D.n_theta + i, rc = rd + 1;          // every one < n_theta * n_phi = n_rays
        // plane (m, l, b) of [M][L][B], l = sel[ls] < L
        const double4* plane = D.xland + (((long long)m * D.L + D.sel[ls]) * D.B + b) * (long long)D.n_rays;
        double4 ca = make_double4(0.0, 0.0, 0.0, 0.0), cc = ca;
        if(live){ ca = plane[ra]; cc = plane[rc]; }
        const bool ac = live && ca.w != 0.0 && cc.w != 0.0;   // (both triangles hold corners a and c)
#pragma unroll 1
        for(int t = 0; t < 2; t++){
            WalkTri T;
            bool ok = false;
            if(ac){
                const double4 co = plane[t == 0 ? rb : rd];
                if(co.w != 0.0) ok = t == 0 ? walk_box(D.G, ca, co, cc, &T) : walk_box(D.G, ca, cc, co, &T);
                T.r0 = ra; T.r1 = t == 0 ? rb : rc; T.r2 = t == 0 ? rc : rd;
                T.tri = 2 * cell + t; T.plane = ls * D.B + b; T.m = m;
            }
            walk_wave(D.G, ok, T, lane, &C, [&D](const WalkTri& U, int i0, int i1){ ltube_test<PASS>(D, U, i0, i1); });
        }
    }
    if(PASS == 0) walk_totals(C, lane, D.stats);
}

// one thread per (selected level, cell): idx < Ls * cells; member m's word is m * Ls * cells + idx < W
__global__ void __launch_bounds__(256) k_ltube_finish(unsigned long long* layers, unsigned* reach, int M, long long ls_cells, long long W){
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < ls_cells; idx += stride){
        unsigned n = 0;
        for(int m = 0; m < M; m++){
            const long long word = (long long)m * ls_cells + idx;
            if(layers[word] > 0ull) n++;
            for(int q = 1; q <= 2; q++){
                const unsigned long long k = layers[q * W + word];
                // (no hit writes the key of a NaN: all ones still means "no finite hit")
                const double v = k == ~0ull ? (double)INFINITY : geoac_unkey(k);
                layers[q * W + word] = (unsigned long long)__double_as_longlong(v);
            }
            // (FIRST: all ones is -1 as a signed word already)
        }
        reach[idx] = n;                                      // [Ls][n0][n1]
    }
}

static_assert(sizeof(LTubeDev) <= 512, "LTubeState::args holds one LTubeDev");

struct LTubeState {
    void* base = nullptr; size_t cap = 0;                // COUNT | TTIME_MIN | ATTEN_MIN | FIRST | three work counters and a spare | REACH
    void* args = nullptr; size_t args_cap = 0;           // the walk's arguments (k_ltube_args)
    unsigned long long gen = 0;                           // the context's invalidation counter the map was made at (0: never)
    geoac_ltube_spec spec{};
    int M = 0, Ls = 0, formed = 0;
    long long cells = 0;
    EventPair ev;
    size_t words() const { return (size_t)M * Ls * (size_t)cells; }
    size_t layer_bytes() const { return 8 * words(); }
    size_t stats_off() const { return GEOAC_LTUBE_LAYERS * layer_bytes(); }
    size_t reach_off() const { return stats_off() + 4 * 8; }
    size_t reach_bytes() const { return 4 * (size_t)Ls * (size_t)cells; }
    size_t bytes() const { return reach_off() + reach_bytes(); }
};

int popcount8(int mask){ int n = 0; for(int l = 0; l < 31; l++) n += (mask >> l) & 1; return n; }

// the first thing wrong with a spec, or NULL; *code the status it earns
const char* spec_fault(int eqset, const geoac_ltube_spec* s, int n_rays, int n_levels, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){
        *code = GEOAC_E_UNSUPPORTED;
        return "not implemented for the 2-D set: it has neither level crossings nor a lattice of launch angles";
    }
    if(!s) return "spec is NULL";
    if(const char* f = geoac_grid_fault(eqset, s->origin, s->step, s->n, s->wrap_lon, -INFINITY, INFINITY)) return f;
    // the lattice, the legs, the ordinals and the edge filter: geoac_lstation_check's own verdict on the shared fields
    geoac_lstation_spec ls;
    ls.n_theta = s->n_theta; ls.n_phi = s->n_phi; ls.phi_periodic = s->phi_periodic; ls.leg_min = s->leg_min; ls.leg_max = s->leg_max;
    ls.ord_max = s->ord_max; ls.edge_max = s->edge_max; ls.cap = 1;
    const int32_t level0 = 0;
    if(const char* f = geoac_lstation_fault(eqset, &ls, n_rays, n_levels, 1, &level0)) return f;
    if(!std::isfinite(s->edge_max)) return "edge_max must be finite: it bounds the cells a crossing triangle can cover";
    if(spherical(eqset)){
        if(!(s->edge_max < 180.0)) return "edge_max must be below 180 degrees on the spherical sets";
        if(!((double)s->n[1] * s->step[1] <= 360.0)) return "n[1] * step[1] must not exceed 360 degrees on the spherical sets";
    }
    const double span = (2.0 * s->edge_max / s->step[0] + 3.0) * (2.0 * s->edge_max / s->step[1] + 3.0);
    if(!(span <= (double)GEOAC_TUBE_MAX_SPAN)) return "candidate span (2 edge_max / step[0] + 3) * (2 edge_max / step[1] + 3) exceeds GEOAC_TUBE_MAX_SPAN (2^20): lower edge_max or coarsen the grid";
    if(s->dir_mask < 1 || s->dir_mask > 3) return "dir_mask must be 1 (upward), 2 (downward) or 3 (both)";
    if(s->level_mask == 0) return "level_mask selects no level";
    if(s->level_mask < 0 || (s->level_mask >> n_levels) != 0) return "level_mask has a bit at or above the number of levels of the launch";
    return nullptr;
}

struct Bound { geoac_ctx* ctx; GeoacLaunchView v; LTubeState* st; };

int bind(geoac_ctx* ctx, const char* what, bool create, Bound* b){
    int rc = bind_launch(ctx, what, GEOAC_SLOT_LTUBE, &b->v);
    if(rc) return rc;
    b->ctx = ctx;
    if(!*b->v.state && create) *b->v.state = new LTubeState();
    b->st = (LTubeState*)*b->v.state;
    return GEOAC_OK;
}

// a current level tube map, or GEOAC_E_INVALID
int bind_map(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = bind(ctx, what, false, b);
    if(rc) return rc;
    if(!b->st || b->st->gen != b->v.map.gen)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no level tube map of the last completed launch (call geoac_fan_level_tubemap after geoac_fan_launch)").c_str());
    // ... and the level list it was made of is still the launch's (geoac_set_levels does not move the invalidation counter)
    if((rc = geoac_fan_levels_dev(ctx, nullptr, nullptr, nullptr, nullptr)))
        return geoac_map_fail(ctx, rc, (std::string(what) + ": " + geoac_last_error(ctx)).c_str());
    return GEOAC_OK;
}

}  // namespace

extern "C" void geoac_ltube_release(void* state){
    LTubeState* st = (LTubeState*)state;
    if(!st) return;
    if(st->base) hipFree(st->base);
    if(st->args) hipFree(st->args);
    st->ev.release();
    delete st;
}

extern "C" const char* geoac_ltube_fault(int eqset, const geoac_ltube_spec* spec, int n_rays, int n_levels){
    int code;
    return spec_fault(eqset, spec, n_rays, n_levels, &code);
}

extern "C" int geoac_ltube_check(int eqset, const geoac_ltube_spec* spec, int n_rays, int n_levels, int64_t* cells, int* n_selected){
    int code;
    if(spec_fault(eqset, spec, n_rays, n_levels, &code)) return code;
    if(cells) *cells = (int64_t)spec->n[0] * spec->n[1];
    if(n_selected) *n_selected = popcount8(spec->level_mask);
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_tubemap(geoac_ctx* ctx, const geoac_ltube_spec* spec){
    const char* what = "fan_level_tubemap";
    Bound b;
    int rc = bind(ctx, what, false, &b);
    if(rc) return rc;
    const GeoacMapView& v = b.v.map;
    int code;
    if(v.eqset == GEOAC_EQ_2D) return geoac_map_fail(ctx, GEOAC_E_UNSUPPORTED, (std::string("fan_level_tubemap: ") + spec_fault(v.eqset, spec, v.n_rays, 0, &code)).c_str());
    // the crossings of that launch: the last completed launch had levels, and the level list has not changed since
    void* lrec = nullptr; void* lcount = nullptr; size_t lrec_bytes = 0, lcount_bytes = 0;
    if((rc = geoac_fan_levels_dev(ctx, &lrec, &lrec_bytes, &lcount, &lcount_bytes)))
        return geoac_map_fail(ctx, rc, (std::string("fan_level_tubemap: ") + geoac_last_error(ctx)).c_str());
    int L = 0, capL = 0;
    if((rc = geoac_get_levels(ctx, &L, nullptr, &capL))) return rc;
    if(const char* fault = spec_fault(v.eqset, spec, v.n_rays, L, &code)) return geoac_map_fail(ctx, code, (std::string("fan_level_tubemap: ") + fault).c_str());
    if(capL < 1 || lrec_bytes != sizeof(double) * GEOAC_LVL_STRIDE * (size_t)v.M * v.n_rays * L * capL || lcount_bytes != sizeof(int) * (size_t)v.M * v.n_rays * L)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_tubemap: the crossing records do not have the shape of the launch ([M][n_rays][L][cap])");
    const int nt = spec->n_theta, np = spec->n_phi;
    const std::string lattice = geoac_lattice_fault(b.v, nt, np);
    if(!lattice.empty()) return geoac_map_fail(ctx, GEOAC_E_INVALID, ("fan_level_tubemap: " + lattice).c_str());
    if((rc = bind(ctx, what, true, &b))) return rc;      // (the state is created only now: a call refused above allocates nothing)
    LTubeState* st = b.st;
    hipStream_t s = (hipStream_t)v.stream;
    st->gen = 0;                                       // (no current map until this one is complete)
    st->spec = *spec;
    st->M = v.M; st->Ls = popcount8(spec->level_mask); st->cells = (long long)spec->n[0] * spec->n[1];
    // the layers before anything goes to the stream: a call refused for memory here has started no event (it keeps the state, with no current map)
    if(grow(&st->base, &st->cap, st->bytes()) || grow(&st->args, &st->args_cap, 512))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_level_tubemap: no device memory for the layers (" + std::to_string(st->bytes() >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(st->Ls) + " levels x " + std::to_string(st->cells) + " cells)").c_str());
    GEOAC_CHK(what, st->ev.start(s));
    const void* xland = nullptr;
    int B = 0, leg0 = 0, n_legs = 0, formed = 0;
    if((rc = geoac_lsta_xland_dev(ctx, what, spec->leg_min, spec->leg_max, spec->ord_max, &xland, &B, &leg0, &n_legs, &formed))){
        (void)st->ev.stop(s);                          // (the pair stays whole; the accessor's message stands)
        return rc;
    }
    st->formed = formed;
    LTubeDev D{};
    D.G.o0 = spec->origin[0]; D.G.o1 = spec->origin[1]; D.G.s0 = spec->step[0]; D.G.s1 = spec->step[1]; D.G.n0 = spec->n[0]; D.G.n1 = spec->n[1];
    D.G.spherical = spherical(v.eqset) ? 1 : 0;
    D.G.pre2 = walk_pre2(spec->origin, spec->step, spec->n, spec->edge_max, spherical(v.eqset));
    // GEOAC_LTUBE_COOP (diagnostic, tools/perf_ltubemap.py): another threshold for the cooperative walk; the layers do not depend on it
    D.G.coop_min = GEOAC_TUBE_COOP_MIN;
    if(const char* e = getenv("GEOAC_LTUBE_COOP")){ const long t = strtol(e, nullptr, 10); if(t >= 0 && t <= 0x7fffffffl) D.G.coop_min = (int)t; }
    D.lrec = (const double*)lrec; D.xland = (const double4*)xland;
    D.layers = (unsigned long long*)st->base; D.stats = (unsigned long long*)((char*)st->base + st->stats_off());
    D.edge2 = spec->edge_max * spec->edge_max;
    D.M = v.M; D.L = L; D.capL = capL; D.n_rays = v.n_rays; D.n_theta = nt; D.n_phi = np;
    D.B = B; D.ord_max = spec->ord_max; D.dir_mask = spec->dir_mask; D.n_dir = spec->dir_mask == 3 ? 2 : 1;
    D.Ls = 0;
    for(int l = 0; l < L; l++) if((spec->level_mask >> l) & 1) D.sel[D.Ls++] = l;
    D.n_br = n_legs * D.n_dir * D.ord_max;
    int leg0_, n_legs_;
    geoac_lattice_extent(spec->leg_min, spec->leg_max, v.legs, nt, np, spec->phi_periodic, &leg0_, &n_legs_, &D.n_cells);
    D.cells = st->cells; D.W = (long long)st->words();
    const long long n_items = (long long)v.M * D.Ls * D.n_br * D.n_cells;
    // COUNT and the counters 0, the three key layers all ones: the largest key, and -1 as FIRST's signed word
    GEOAC_CHK(what, hipMemsetAsync(st->base, 0, st->layer_bytes(), s));
    GEOAC_CHK(what, hipMemsetAsync((char*)st->base + st->layer_bytes(), 0xff, 3 * st->layer_bytes(), s));
    GEOAC_CHK(what, hipMemsetAsync((char*)st->base + st->stats_off(), 0, 4 * 8, s));
    if(n_items > 0){
        const unsigned n_blk = blocks_for(n_items * 4, 256, 1ll << 18);  // (one wave of 64 items per block)
        hipLaunchKernelGGL(k_ltube_args, dim3(1), dim3(64), 0, s, D, (LTubeDev*)st->args);
        hipLaunchKernelGGL(k_ltube_raster<0>, dim3(n_blk), dim3(64), 0, s, (const LTubeDev*)st->args, n_items);
        hipLaunchKernelGGL(k_ltube_raster<1>, dim3(n_blk), dim3(64), 0, s, (const LTubeDev*)st->args, n_items);
    }
    const long long ls_cells = (long long)D.Ls * D.cells;
    hipLaunchKernelGGL(k_ltube_finish, dim3(blocks_for(ls_cells, 256, 1ll << 16)), dim3(256), 0, s, D.layers, (unsigned*)((char*)st->base + st->reach_off()), v.M, ls_cells, D.W);
    GEOAC_CHK(what, hipGetLastError());
    GEOAC_CHK(what, st->ev.stop(s));
    st->gen = v.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_tubemap_shape(geoac_ctx* ctx, int* n_members, int* n_selected, int* n0, int* n1){
    Bound b;
    int rc = bind_map(ctx, "fan_level_tubemap_shape", &b);
    if(rc) return rc;
    if(n_members) *n_members = b.st->M;
    if(n_selected) *n_selected = b.st->Ls;
    if(n0) *n0 = b.st->spec.n[0];
    if(n1) *n1 = b.st->spec.n[1];
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_tubemap_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_map(ctx, "fan_level_tubemap_dev", &b);
    if(rc) return rc;
    if(layer < 0 || layer >= GEOAC_LTUBE_LAYERS) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_tubemap_dev: layer must be one of GEOAC_LTUBE_COUNT .. GEOAC_LTUBE_FIRST");
    if(dev_ptr) *dev_ptr = (char*)b.st->base + (size_t)layer * b.st->layer_bytes();
    if(bytes) *bytes = b.st->layer_bytes();
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_tubemap_fetch(geoac_ctx* ctx, int layer, void* host){
    const char* what = "fan_level_tubemap_fetch";
    Bound b;
    int rc = bind_map(ctx, what, &b);
    if(rc) return rc;
    if(layer < 0 || layer >= GEOAC_LTUBE_LAYERS) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_tubemap_fetch: layer must be one of GEOAC_LTUBE_COUNT .. GEOAC_LTUBE_FIRST");
    if(!host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_tubemap_fetch: NULL argument");
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, hipMemcpyAsync(host, (char*)b.st->base + (size_t)layer * b.st->layer_bytes(), b.st->layer_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_tubemap_fetch_reach(geoac_ctx* ctx, uint32_t* reach_host){
    const char* what = "fan_level_tubemap_fetch_reach";
    Bound b;
    int rc = bind_map(ctx, what, &b);
    if(rc) return rc;
    if(!reach_host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_tubemap_fetch_reach: NULL argument");
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, hipMemcpyAsync(reach_host, (char*)b.st->base + b.st->reach_off(), b.st->reach_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_tubemap_stats(geoac_ctx* ctx, uint64_t* stats4){
    const char* what = "fan_level_tubemap_stats";
    Bound b;
    int rc = bind_map(ctx, what, &b);
    if(rc) return rc;
    if(!stats4) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_tubemap_stats: NULL argument");
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, hipMemcpyAsync(stats4, (char*)b.st->base + b.st->stats_off(), 4 * 8, hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    stats4[3] = (uint64_t)b.st->formed;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_tubemap_timing(geoac_ctx* ctx, double* ms){
    Bound b;
    int rc = bind_map(ctx, "fan_level_tubemap_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_tubemap_timing: NULL argument");
    GEOAC_CHK("fan_level_tubemap_timing", b.st->ev.ms(ms));
    return GEOAC_OK;
}
