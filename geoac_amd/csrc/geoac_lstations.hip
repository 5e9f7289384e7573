// geoac_lstations.hip - level stations (include/geoac_lstations.h): first-order eigenray estimates at R receivers above the ground from the
// crossing records of the last completed launch (geoac_levels.h), on the device.
//
// Reads the crossing records and their counts (geoac_fan_levels_dev) and the lattice axes of the launch angles; writes only buffers of its
// own.  No kernel of the launch plan is involved.  The search is the one of station arrivals (geoac_stations.hip), on other corners: the walk
// is geoac_lattice_list.h, the lattice proof and extent are geoac_stations_int.h's.
//
// Three kernels:
//   k_lsta_prep    branch table xland[M][L][B][n_rays] of (c0, c1, slot k, present).  One thread per (member, ray, level) walks the kept
//                  crossings once, in path order, with two ordinal counters (upward, downward) that reset when the leg changes, and files
//                  crossing k under its branch b = ((leg - leg0) * 2 + d) * ord_max + o.  The table is cleared first: an absent branch
//                  reads present = 0.  The ray index is the fastest axis, so the corner loads of neighbouring lanes coalesce as they do on
//                  the landing table of k_sta_count.  It depends on the launch, leg0, n_legs and ord_max, and is kept while those hold
//                  (geoac_lsta_xland_dev, which geoac_ltubemap.hip calls too: one table serves the lists and the level tube map).
//   k_lsta_count, k_lsta_rows    the two passes of geoac_lattice_list.h over the list segments (member, station, branch, chunk of lattice
//                  cells): a plane is (m, level_of[s], b) of the table, the rows come out sorted by b * n_tri + tri.  What is this file's
//                  own is LstaDev below: which plane, no filter, and a row that reads the three corners' crossing records through slot k.
//
// The arithmetic is fixed by the header and restated in tests/lstation_reference.py: every product is rounded before it is added, so this
// file is compiled with contraction off (the pragma below; the Makefile gives the same flag).  Divisions and floor are IEEE.
//
// Index bounds, stated again at each load and store (those of the walk: geoac_lattice_list.h, with n_planes = B):
//   t < M * n_rays * L in k_lsta_prep, so ray < n_rays, l < L, m < M;  record slot k < min(count, capL) <= capL;  branch b < B (tested:
//   leg in leg0 .. leg0 + n_legs - 1, o < ord_max);  level_of[s] in 0 .. L - 1 (checked on the host before the copy).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/geoac_lstations.h"
#include "geoac_lattice_list.h"
#include "geoac_lstations_int.h"

#pragma clang fp contract(off)

namespace {

const double kLstaPi = 3.141592653589793238462643;

struct LstaDev : ListDev {                        // n_planes = B = n_legs * 2 * ord_max: legs leg0 .. leg0 + n_legs - 1 take part
    const double* lrec; const int* lcount;        // the launch's crossings: [M][n_rays][L][capL][GEOAC_LVL_STRIDE], [M][n_rays][L]
    const int* level_of;                          // [n_sta], each in 0 .. L - 1
    double4* xland;                               // [M][L][B][n_rays]: c0, c1, slot k, present
    int L, capL, leg0, n_legs, ord_max;

    // plane (m, l, b) of [M][L][B]: s < n_sta; l = level_of[s] in 0 .. L - 1 (host check); b = S.p < B
    __device__ const double4* plane(const Seg& S) const { return xland + ((S.m * L + level_of[S.s]) * n_planes + S.p) * (long long)n_rays; }
    __device__ bool admit(const double4&, const double4&, const double4&) const { return true; }
    // the row of a hit; r0, r1, r2 the ray indices of its corners (< n_rays), their record slots in the corners' .z (< capL, written by
    // k_lsta_prep), r the row's index in the lists (< M * n_sta * cap)
    __device__ void write_row(const Seg& S, int tri, const Tri& T, int r0, int r1, int r2, const double4& c0, const double4& c1, const double4& c2, long long r) const {
        const long long m = S.m;
        const int l = level_of[S.s], b = S.p;
        const int k0 = (int)c0.z, k1 = (int)c1.z, k2 = (int)c2.z;
        double* row = rows + r * GEOAC_LSTA_STRIDE;
        const double W0 = T.w0 / T.s, W1 = T.w1 / T.s, W2 = T.w2 / T.s;
        const double* R0 = lrec + ((((m * n_rays + r0) * L + l) * capL) + k0) * GEOAC_LVL_STRIDE;
        const double* R1 = lrec + ((((m * n_rays + r1) * L + l) * capL) + k1) * GEOAC_LVL_STRIDE;
        const double* R2 = lrec + ((((m * n_rays + r2) * L + l) * capL) + k2) * GEOAC_LVL_STRIDE;
        const double p0 = phi_ax[r0 / n_theta];              // r / n_theta < n_phi
        double p1 = phi_ax[r1 / n_theta], p2 = phi_ax[r2 / n_theta];
        if(periodic){ p1 = near(p0, p1); p2 = near(p0, p2); }
        const int o = b % ord_max, ld = b / ord_max;
        row[GEOAC_LSTA_LEG] = (double)(leg0 + ld / 2);
        row[GEOAC_LSTA_DIR] = (ld & 1) ? -1.0 : 1.0;
        row[GEOAC_LSTA_ORD] = (double)o;
        row[GEOAC_LSTA_TRI] = (double)tri;
        row[GEOAC_LSTA_RAY0] = (double)r0;
        row[GEOAC_LSTA_ORIENT] = T.s > 0.0 ? 1.0 : -1.0;
        row[GEOAC_LSTA_W0] = W0; row[GEOAC_LSTA_W1] = W1; row[GEOAC_LSTA_W2] = W2;
        row[GEOAC_LSTA_THETA] = interp(W0, W1, W2, theta_ax[r0 % n_theta], theta_ax[r1 % n_theta], theta_ax[r2 % n_theta]);
        row[GEOAC_LSTA_PHI] = interp(W0, W1, W2, p0, p1, p2);
        row[GEOAC_LSTA_TTIME] = interp(W0, W1, W2, R0[GEOAC_LVL_TTIME], R1[GEOAC_LVL_TTIME], R2[GEOAC_LVL_TTIME]);
        row[GEOAC_LSTA_ATTEN] = interp(W0, W1, W2, R0[GEOAC_LVL_ATTEN], R1[GEOAC_LVL_ATTEN], R2[GEOAC_LVL_ATTEN]);
        row[GEOAC_LSTA_N0 + 0] = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 3], R1[GEOAC_LVL_P0 + 3], R2[GEOAC_LVL_P0 + 3]);
        row[GEOAC_LSTA_N0 + 1] = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 4], R1[GEOAC_LVL_P0 + 4], R2[GEOAC_LVL_P0 + 4]);
        row[GEOAC_LSTA_N0 + 2] = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 5], R1[GEOAC_LVL_P0 + 5], R2[GEOAC_LVL_P0 + 5]);
    }
};

// one thread per (m, ray, l): the ray's kept crossings of the level, filed by branch
__global__ void __launch_bounds__(256) k_lsta_prep(LstaDev D){
    const long long n = (long long)D.M * D.n_rays * D.L;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride){        // t < M * L * n_rays
        const int ray = (int)(t % D.n_rays);                     // ray < n_rays
        const long long ml = t / D.n_rays;
        const int l = (int)(ml % D.L);                           // l < L
        const long long m = ml / D.L;                            // m < M
        const long long rl = (m * D.n_rays + ray) * D.L + l;     // < M * n_rays * L: the (member, ray, level) of both crossing tables
        const int seen = D.lcount[rl];
        const int kept = seen < D.capL ? seen : D.capL;          // only the first min(count, capL) crossings exist
        const double* R = D.lrec + rl * D.capL * GEOAC_LVL_STRIDE;
        double4* plane = D.xland + (m * D.L + l) * D.n_planes * (long long)D.n_rays + ray;          // branch b of this ray: plane[b * n_rays], b < B
        int leg_now = -1, o_up = 0, o_down = 0;
        for(int k = 0; k < kept; k++, R += GEOAC_LVL_STRIDE){    // record slot k < kept <= capL
            const int leg = (int)R[GEOAC_LVL_LEG];
            if(leg != leg_now){ leg_now = leg; o_up = 0; o_down = 0; }
            const int d = R[GEOAC_LVL_DIR] > 0.0 ? 0 : 1;
            const int o = d ? o_down++ : o_up++;
            const int li = leg - D.leg0;
            if(li < 0 || li >= D.n_legs || o >= D.ord_max) continue;
            const int b = (li * 2 + d) * D.ord_max + o;          // b < n_legs * 2 * ord_max = B
            double4 c;
            if(D.spherical){
                c.x = R[GEOAC_LVL_P0 + 1] * 180.0 / kLstaPi;
                c.y = R[GEOAC_LVL_P0 + 2] * 180.0 / kLstaPi;
            } else {
                c.x = R[GEOAC_LVL_P0 + 0];
                c.y = R[GEOAC_LVL_P0 + 1];
            }
            c.z = (double)k;
            c.w = 1.0;
            plane[(long long)b * D.n_rays] = c;
        }
    }
}

__global__ void __launch_bounds__(256) k_lsta_count(LstaDev D, long long n_seg_all){ list_count(D, n_seg_all); }
__global__ void __launch_bounds__(256) k_lsta_rows(LstaDev D, long long n_seg_all){ list_rows(D, n_seg_all); }

struct LstaState {
    void* xland = nullptr; size_t xland_cap = 0;
    ListBufs lb;                                          // axes: theta_ax | phi_ax | sta | level_of; out: rows | hits
    unsigned long long lsta_gen = 0, xland_gen = 0;       // the context's invalidation counter they were made at (0: never)
    int x_leg0 = -1, x_n_legs = -1, x_ord_max = -1;       // what the branch table was formed with
    std::vector<int32_t> h_level_of;                      // host copy of the tail of `axes` (alive while the copy runs)
    int M = 0, n_sta = 0, cap = 0;
    size_t rows_bytes() const { return sizeof(double) * (size_t)M * n_sta * cap * GEOAC_LSTA_STRIDE; }
    size_t hits_bytes() const { return sizeof(uint32_t) * (size_t)M * n_sta; }
};

// the first thing wrong with a spec or a level list, or NULL; *code the status it earns
const char* lspec_fault(int eqset, const geoac_lstation_spec* s, int n_rays, int n_levels, int n_sta, const int32_t* level_of, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){
        *code = GEOAC_E_UNSUPPORTED;
        return "not implemented for the 2-D set: it has neither level crossings nor a lattice of launch angles";
    }
    if(!s) return "spec is NULL";
    if(s->n_theta < 2 || s->n_phi < 2) return "n_theta and n_phi must both be at least 2";
    if((long long)s->n_theta * s->n_phi != (long long)n_rays) return "n_theta * n_phi must equal the number of rays of the launch";
    if(s->phi_periodic != 0 && s->phi_periodic != 1) return "phi_periodic must be 0 or 1";
    if(s->leg_min < 0 || s->leg_max < s->leg_min) return "legs: need 0 <= leg_min <= leg_max";
    if(s->ord_max < 1 || s->ord_max > GEOAC_LVL_MAX_CAP) return "ord_max must be in 1 .. 64";
    if(std::isnan(s->edge_max) || !(s->edge_max > 0.0)) return "edge_max must be > 0 and not NaN (+inf: no bound)";
    if(s->cap < 1 || s->cap > GEOAC_STA_MAX_CAP) return "cap must be in 1 .. 256";
    if(n_levels < 1 || n_levels > GEOAC_MAX_LEVELS) return "n_levels must be in 1 .. 8";
    if(n_sta < 1 || n_sta > GEOAC_STA_MAX_STATIONS) return "n_sta must be in 1 .. 2^24";
    if(!level_of) return "level_of is NULL";
    for(int k = 0; k < n_sta; k++)
        if(level_of[k] < 0 || level_of[k] >= n_levels) return "level_of: every entry must be in 0 .. n_levels - 1, an index into the level list of the launch";
    return nullptr;
}

struct LBound { geoac_ctx* ctx; GeoacLaunchView v; LstaState* st; };

int lbind(geoac_ctx* ctx, const char* what, bool create, LBound* b){
    int rc = bind_launch(ctx, what, GEOAC_SLOT_LSTA, &b->v);
    if(rc) return rc;
    b->ctx = ctx;
    if(!*b->v.state && create) *b->v.state = new LstaState();
    b->st = (LstaState*)*b->v.state;
    return GEOAC_OK;
}

// current lists, or GEOAC_E_INVALID
int lbind_lists(geoac_ctx* ctx, const char* what, LBound* b){
    int rc = lbind(ctx, what, false, b);
    if(rc) return rc;
    if(!b->st || b->st->lsta_gen != b->v.map.gen)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no level-station lists of the last completed launch (call geoac_fan_level_stations after geoac_fan_launch)").c_str());
    return GEOAC_OK;
}

}  // namespace

extern "C" void geoac_lsta_release(void* state){
    LstaState* st = (LstaState*)state;
    if(!st) return;
    if(st->xland) hipFree(st->xland);
    st->lb.release();
    delete st;
}

// the branch table of the last completed launch under (leg_min, leg_max, ord_max): formed on first use after a launch or when the three give
// another (leg0, n_legs, ord_max), and kept until then.  The level-station state is created if the context has none.
extern "C" int geoac_lsta_xland_dev(geoac_ctx* ctx, const char* what, int leg_min, int leg_max, int ord_max, const void** xland_dev, int* n_branches, int* leg0,
                                    int* n_legs, int* formed){
    LBound b;
    int rc = lbind(ctx, what, true, &b);
    if(rc) return rc;
    const GeoacMapView& v = b.v.map;
    void* lrec = nullptr; void* lcount = nullptr; size_t lrec_bytes = 0, lcount_bytes = 0;
    if((rc = geoac_fan_levels_dev(ctx, &lrec, &lrec_bytes, &lcount, &lcount_bytes)))
        return geoac_map_fail(ctx, rc, (std::string(what) + ": " + geoac_last_error(ctx)).c_str());
    int L = 0, capL = 0;
    if((rc = geoac_get_levels(ctx, &L, nullptr, &capL))) return rc;
    if(leg_min < 0 || leg_max < leg_min || ord_max < 1 || ord_max > GEOAC_LVL_MAX_CAP || L < 1 || capL < 1 ||
       lrec_bytes != sizeof(double) * GEOAC_LVL_STRIDE * (size_t)v.M * v.n_rays * L * capL || lcount_bytes != sizeof(int) * (size_t)v.M * v.n_rays * L)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": the branch table needs 0 <= leg_min <= leg_max, ord_max in 1 .. 64 and crossing records of the launch's shape").c_str());
    LstaState* st = b.st;
    hipStream_t s = (hipStream_t)v.stream;
    LstaDev D{};
    D.lrec = (const double*)lrec; D.lcount = (const int*)lcount;
    D.spherical = spherical(v.eqset) ? 1 : 0;
    D.M = v.M; D.L = L; D.capL = capL; D.n_rays = v.n_rays;
    int n_cells = 0;
    geoac_lattice_extent(leg_min, leg_max, v.legs, 2, 2, 0, &D.leg0, &D.n_legs, &n_cells);       // (the legs do not depend on the lattice)
    D.ord_max = ord_max;
    D.n_planes = D.n_legs * 2 * D.ord_max;
    const size_t n_xland = (size_t)v.M * L * D.n_planes * v.n_rays;
    const bool form = n_xland > 0 && (st->xland_gen != v.gen || st->x_leg0 != D.leg0 || st->x_n_legs != D.n_legs || st->x_ord_max != D.ord_max);
    if(form){
        st->xland_gen = 0;
        if(grow(&st->xland, &st->xland_cap, sizeof(double4) * n_xland))
            return geoac_map_fail(ctx, GEOAC_E_NOMEM, (std::string(what) + ": no device memory for the branch table (" + std::to_string((sizeof(double4) * n_xland) >> 20) + " MiB)").c_str());
        D.xland = (double4*)st->xland;
        // cleared first: an absent branch reads present = 0
        GEOAC_CHK(what, hipMemsetAsync(st->xland, 0, sizeof(double4) * n_xland, s));
        hipLaunchKernelGGL(k_lsta_prep, dim3(blocks_for((long long)v.M * v.n_rays * L, 256)), dim3(256), 0, s, D);
        GEOAC_CHK(what, hipGetLastError());
        st->xland_gen = v.gen; st->x_leg0 = D.leg0; st->x_n_legs = D.n_legs; st->x_ord_max = D.ord_max;
    }
    if(xland_dev) *xland_dev = st->xland;
    if(n_branches) *n_branches = D.n_planes;
    if(leg0) *leg0 = D.leg0;
    if(n_legs) *n_legs = D.n_legs;
    if(formed) *formed = form ? 1 : 0;
    return GEOAC_OK;
}

extern "C" const char* geoac_lstation_fault(int eqset, const geoac_lstation_spec* spec, int n_rays, int n_levels, int n_sta, const int32_t* level_of){
    int code;
    return lspec_fault(eqset, spec, n_rays, n_levels, n_sta, level_of, &code);
}

extern "C" int geoac_lstation_check(int eqset, const geoac_lstation_spec* spec, int n_rays, int n_levels, int n_sta, const int32_t* level_of){
    int code;
    return lspec_fault(eqset, spec, n_rays, n_levels, n_sta, level_of, &code) ? code : GEOAC_OK;
}

extern "C" int geoac_fan_level_stations(geoac_ctx* ctx, const geoac_lstation_spec* spec, int n_sta, const double* sta, const int32_t* level_of){
    const char* what = "fan_level_stations";
    LBound b;
    int rc = lbind(ctx, what, false, &b);
    if(rc) return rc;
    const GeoacMapView& v = b.v.map;
    int code;
    if(v.eqset == GEOAC_EQ_2D) return geoac_map_fail(ctx, GEOAC_E_UNSUPPORTED, (std::string("fan_level_stations: ") + lspec_fault(v.eqset, spec, v.n_rays, 0, n_sta, level_of, &code)).c_str());
    // the crossings of that launch: the last completed launch had levels, and the level list has not changed since
    void* lrec = nullptr; void* lcount = nullptr; size_t lrec_bytes = 0, lcount_bytes = 0;
    if((rc = geoac_fan_levels_dev(ctx, &lrec, &lrec_bytes, &lcount, &lcount_bytes)))
        return geoac_map_fail(ctx, rc, (std::string("fan_level_stations: ") + geoac_last_error(ctx)).c_str());
    int L = 0, capL = 0;
    if((rc = geoac_get_levels(ctx, &L, nullptr, &capL))) return rc;
    if(const char* fault = lspec_fault(v.eqset, spec, v.n_rays, L, n_sta, level_of, &code)) return geoac_map_fail(ctx, code, (std::string("fan_level_stations: ") + fault).c_str());
    if(!sta) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_stations: sta is NULL");
    if(capL < 1 || lrec_bytes != sizeof(double) * GEOAC_LVL_STRIDE * (size_t)v.M * v.n_rays * L * capL || lcount_bytes != sizeof(int) * (size_t)v.M * v.n_rays * L)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_stations: the crossing records do not have the shape of the launch ([M][n_rays][L][cap])");
    const int nt = spec->n_theta, np = spec->n_phi;
    const std::string lattice = geoac_lattice_fault(b.v, nt, np);
    if(!lattice.empty()) return geoac_map_fail(ctx, GEOAC_E_INVALID, ("fan_level_stations: " + lattice).c_str());
    if((rc = lbind(ctx, what, true, &b))) return rc;     // (the state is created only now: a refused call allocates nothing)
    LstaState* st = b.st;
    hipStream_t s = (hipStream_t)v.stream;
    st->lsta_gen = 0;                                  // (no current lists until these are complete)
    GEOAC_CHK(what, st->lb.ev.start(s));
    st->M = v.M; st->n_sta = n_sta; st->cap = spec->cap;

    LstaDev D{};
    D.lrec = (const double*)lrec; D.lcount = (const int*)lcount;
    D.edge2 = spec->edge_max * spec->edge_max;
    D.spherical = spherical(v.eqset) ? 1 : 0; D.periodic = spec->phi_periodic;
    D.M = v.M; D.L = L; D.capL = capL; D.n_rays = v.n_rays; D.n_theta = nt; D.n_phi = np; D.n_sta = n_sta; D.cap = spec->cap;
    geoac_lattice_extent(spec->leg_min, spec->leg_max, v.legs, nt, np, spec->phi_periodic, &D.leg0, &D.n_legs, &D.n_cells);
    D.ord_max = spec->ord_max;
    const long long n_seg_all = list_segments(&D, D.n_legs * 2 * D.ord_max);

    const size_t n_axes = (size_t)nt + np + 2 * (size_t)n_sta;
    const size_t out_need = st->rows_bytes() + st->hits_bytes();
    const void* xland = nullptr;
    if((rc = geoac_lsta_xland_dev(ctx, what, spec->leg_min, spec->leg_max, spec->ord_max, &xland, nullptr, nullptr, nullptr, nullptr))) return rc;
    if(list_grow(&st->lb, D, sizeof(int32_t) * (size_t)n_sta, n_seg_all, out_need))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_level_stations: no device memory for the lists (" + std::to_string(out_need >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(n_sta) + " stations x " + std::to_string(spec->cap) + " rows)").c_str());
    D.xland = (double4*)xland;
    // lattice axes and stations, and behind them the stations' levels: a second host block, a second copy (list_fill left the stream idle:
    // no earlier call's copy still reads the block)
    GEOAC_CHK(what, list_fill(&st->lb, &D, b.v, sta, s));
    st->h_level_of.assign(level_of, level_of + n_sta);
    D.level_of = (const int*)((const char*)st->lb.axes + sizeof(double) * n_axes);
    GEOAC_CHK(what, hipMemcpyAsync((void*)D.level_of, st->h_level_of.data(), sizeof(int32_t) * (size_t)n_sta, hipMemcpyHostToDevice, s));
    D.hits = (unsigned*)((char*)st->lb.out + st->rows_bytes());
    GEOAC_CHK(what, list_launch(k_lsta_count, k_lsta_rows, D, st->lb.out, out_need, n_seg_all, s));
    GEOAC_CHK(what, st->lb.ev.stop(s));
    st->lsta_gen = v.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_stations_shape(geoac_ctx* ctx, int* n_members, int* n_sta, int* cap){
    LBound b;
    int rc = lbind_lists(ctx, "fan_level_stations_shape", &b);
    if(rc) return rc;
    if(n_members) *n_members = b.st->M;
    if(n_sta) *n_sta = b.st->n_sta;
    if(cap) *cap = b.st->cap;
    return GEOAC_OK;
}

extern "C" int geoac_lsta_coords_dev(geoac_ctx* ctx, const double** sta_dev, const int** level_of_dev, int* n_sta){
    LBound b;
    int rc = lbind_lists(ctx, "fan_level_refine", &b);
    if(rc) return rc;
    const double* tail = (const double*)b.st->lb.axes + b.st->lb.h_axes.size();          // axes: theta_ax | phi_ax | sta | level_of
    if(sta_dev) *sta_dev = tail - 2 * (size_t)b.st->n_sta;
    if(level_of_dev) *level_of_dev = (const int*)tail;
    if(n_sta) *n_sta = b.st->n_sta;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_stations_dev(geoac_ctx* ctx, int which, void** dev_ptr, size_t* bytes){
    LBound b;
    int rc = lbind_lists(ctx, "fan_level_stations_dev", &b);
    if(rc) return rc;
    if(which < 0 || which > 1) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_stations_dev: which must be 0 (hits) or 1 (rows)");
    const LstaState* st = b.st;
    if(dev_ptr) *dev_ptr = (char*)st->lb.out + (which == 1 ? 0 : st->rows_bytes());
    if(bytes) *bytes = which == 1 ? st->rows_bytes() : st->hits_bytes();
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_stations_fetch(geoac_ctx* ctx, uint32_t* hits, double* rows){
    const char* what = "fan_level_stations_fetch";
    LBound b;
    int rc = lbind_lists(ctx, what, &b);
    if(rc) return rc;
    const LstaState* st = b.st;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    const char* base = (const char*)st->lb.out;
    if(rows) GEOAC_CHK(what, hipMemcpyAsync(rows, base, st->rows_bytes(), hipMemcpyDeviceToHost, s));
    if(hits) GEOAC_CHK(what, hipMemcpyAsync(hits, base + st->rows_bytes(), st->hits_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_stations_timing(geoac_ctx* ctx, double* ms){
    const char* what = "fan_level_stations_timing";
    LBound b;
    int rc = lbind_lists(ctx, what, &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_stations_timing: NULL argument");
    GEOAC_CHK(what, b.st->lb.ev.ms(ms));
    return GEOAC_OK;
}
