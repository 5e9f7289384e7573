// geoac_stations.hip - station arrivals (include/geoac_stations.h): first-order eigenray estimates at R stations from the record table of the
// last completed launch, on the device.
//
// Reads the record table, the level table of geoac_map.hip and the lattice axes of the launch angles; writes only buffers of its own.  No
// kernel of the launch plan is involved.
//
// Three kernels:
//   k_sta_prep    landing table land[M][legs][n_rays] of (c0, c1, turn, valid), 32 B per corner instead of the 256 B of a record, in the map's
//                 coordinates.  It depends on the launch alone and is kept until the next launch.
//   k_sta_count, k_sta_rows    the two passes of geoac_lattice_list.h, which level stations (geoac_lstations.hip) run too, over the list
//                 segments (member, station, leg, chunk of lattice cells): a plane is a leg of the landing table, the rows come out sorted
//                 by leg * n_tri + tri.  What is this file's own is StaDev below: which plane, the turning-height filter, the row.
//
// The arithmetic is fixed by the header and restated in tests/station_reference.py: every product is rounded before it is added, so this
// file is compiled with contraction off (the pragma below; the Makefile gives the same flag).  Divisions and floor are IEEE.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/geoac_stations.h"
#include "geoac_lattice_list.h"
#include "geoac_stations_int.h"

#pragma clang fp contract(off)

namespace {

const double kStaPi = 3.141592653589793238462643;

struct StaDev : ListDev {                         // n_planes = n_legs: legs leg0 .. leg0 + n_legs - 1 take part
    const double* rec; const double* level;       // the launch's tables
    double4* land;                                // [M][legs][n_rays]: c0, c1, turn, valid
    double* lvl;                                  // the lists' level rows, beside ListDev's rows
    double turn_tol;
    int F, legs, leg0;

    // leg0 + p < legs (geoac_lattice_extent), m < M
    __device__ const double4* plane(const Seg& S) const { return land + (S.m * legs + (leg0 + S.p)) * n_rays; }
    // the turning heights of the corners within turn_tol of each other (a NaN refuses)
    __device__ bool admit(const double4& c0, const double4& c1, const double4& c2) const {
        const double tmx = dmax(dmax(c0.z, c1.z), c2.z), tmn = dmin(dmin(c0.z, c1.z), c2.z);
        return tmx - tmn <= turn_tol;
    }
    // the row of a hit; r0, r1, r2 the ray indices of its corners (< n_rays), r the row's index in the lists (< M * n_sta * cap)
    __device__ void write_row(const Seg& S, int tri, const Tri& T, int r0, int r1, int r2, const double4&, const double4&, const double4&, long long r) const {
        const long long m = S.m;
        const int leg = leg0 + S.p;
        double* row = rows + r * GEOAC_STA_STRIDE;
        double* lv = lvl + r * F;
        const double W0 = T.w0 / T.s, W1 = T.w1 / T.s, W2 = T.w2 / T.s;
        const long long per_m = (long long)n_rays * legs;
        const double* R0 = rec + (m * per_m + (long long)r0 * legs + leg) * GEOAC_REC_STRIDE;
        const double* R1 = rec + (m * per_m + (long long)r1 * legs + leg) * GEOAC_REC_STRIDE;
        const double* R2 = rec + (m * per_m + (long long)r2 * legs + leg) * GEOAC_REC_STRIDE;
        const double p0 = phi_ax[r0 / n_theta];               // r / n_theta < n_phi
        double p1 = phi_ax[r1 / n_theta], p2 = phi_ax[r2 / n_theta];
        if(periodic){ p1 = near(p0, p1); p2 = near(p0, p2); }
        const double b0 = R0[GEOAC_REC_BACKAZ];
        const double b1 = near(b0, R1[GEOAC_REC_BACKAZ]), b2 = near(b0, R2[GEOAC_REC_BACKAZ]);
        const double tt = interp(W0, W1, W2, R0[GEOAC_REC_TTIME], R1[GEOAC_REC_TTIME], R2[GEOAC_REC_TTIME]);
        const double rg = interp(W0, W1, W2, R0[GEOAC_REC_RANGE], R1[GEOAC_REC_RANGE], R2[GEOAC_REC_RANGE]);
        row[GEOAC_STA_LEG] = (double)leg;
        row[GEOAC_STA_TRI] = (double)tri;
        row[GEOAC_STA_RAY0] = (double)r0;
        row[GEOAC_STA_ORIENT] = T.s > 0.0 ? 1.0 : -1.0;
        row[GEOAC_STA_W0] = W0; row[GEOAC_STA_W1] = W1; row[GEOAC_STA_W2] = W2;
        row[GEOAC_STA_THETA] = interp(W0, W1, W2, theta_ax[r0 % n_theta], theta_ax[r1 % n_theta], theta_ax[r2 % n_theta]);
        row[GEOAC_STA_PHI] = interp(W0, W1, W2, p0, p1, p2);
        row[GEOAC_STA_TTIME] = tt;
        row[GEOAC_STA_CELERITY] = rg / tt;
        row[GEOAC_STA_TURN] = interp(W0, W1, W2, R0[GEOAC_REC_TURN], R1[GEOAC_REC_TURN], R2[GEOAC_REC_TURN]);
        row[GEOAC_STA_INCL] = interp(W0, W1, W2, R0[GEOAC_REC_INCL], R1[GEOAC_REC_INCL], R2[GEOAC_REC_INCL]);
        row[GEOAC_STA_BACKAZ] = interp(W0, W1, W2, b0, b1, b2);
        row[14] = 0.0; row[15] = 0.0;
        for(int f = 0; f < F; f++){
            const double* L = level + (m * F + f) * per_m;
            lv[f] = interp(W0, W1, W2, L[(long long)r0 * legs + leg], L[(long long)r1 * legs + leg], L[(long long)r2 * legs + leg]);
        }
    }
};

// one thread per (m, leg, ray): the landing point in the map's coordinates
__global__ void k_sta_prep(StaDev D){
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
            o.x = R[GEOAC_REC_STATE + 1] * 180.0 / kStaPi;
            o.y = R[GEOAC_REC_STATE + 2] * 180.0 / kStaPi;
        } else {
            o.x = R[GEOAC_REC_STATE + 0];
            o.y = R[GEOAC_REC_STATE + 1];
        }
        o.z = R[GEOAC_REC_TURN];
        o.w = R[GEOAC_REC_VALID];
        D.land[t] = o;
    }
}

__global__ void k_sta_count(StaDev D, long long n_seg_all){ list_count(D, n_seg_all); }
__global__ void k_sta_rows(StaDev D, long long n_seg_all){ list_rows(D, n_seg_all); }

struct StaState {
    void* land = nullptr; size_t land_cap = 0;
    ListBufs lb;                                          // axes: theta_ax | phi_ax | sta; out: rows | level | hits
    unsigned long long sta_gen = 0, land_gen = 0;         // the context's invalidation counter they were made at (0: never)
    int M = 0, F = 0, n_sta = 0, cap = 0;
    size_t rows_bytes() const { return sizeof(double) * (size_t)M * n_sta * cap * GEOAC_STA_STRIDE; }
    size_t level_bytes() const { return sizeof(double) * (size_t)M * n_sta * cap * F; }
    size_t hits_bytes() const { return sizeof(uint32_t) * (size_t)M * n_sta; }
};

// the first thing wrong with a spec, or NULL; *code the status it earns
const char* spec_fault(int eqset, const geoac_station_spec* s, int n_rays, int n_sta, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){
        *code = GEOAC_E_UNSUPPORTED;
        return "not implemented for the 2-D set: on one axis the search is for the interval between two neighbouring rays that holds the station's range, a different (1-D) routine";
    }
    if(!s) return "spec is NULL";
    if(s->n_theta < 2 || s->n_phi < 2) return "n_theta and n_phi must both be at least 2";
    if((long long)s->n_theta * s->n_phi != (long long)n_rays) return "n_theta * n_phi must equal the number of rays of the launch";
    if(s->phi_periodic != 0 && s->phi_periodic != 1) return "phi_periodic must be 0 or 1";
    if(s->leg_min < 0 || s->leg_max < s->leg_min) return "legs: need 0 <= leg_min <= leg_max";
    if(std::isnan(s->turn_tol) || !(s->turn_tol >= 0.0)) return "turn_tol must be >= 0 and not NaN (+inf: no bound)";
    if(std::isnan(s->edge_max) || !(s->edge_max > 0.0)) return "edge_max must be > 0 and not NaN (+inf: no bound)";
    if(s->cap < 1 || s->cap > GEOAC_STA_MAX_CAP) return "cap must be in 1 .. 256";
    if(n_sta < 1 || n_sta > GEOAC_STA_MAX_STATIONS) return "n_sta must be in 1 .. 2^24";
    return nullptr;
}

bool same_bits(double a, double b){ uint64_t x, y; memcpy(&x, &a, 8); memcpy(&y, &b, 8); return x == y; }

struct Bound { geoac_ctx* ctx; GeoacLaunchView v; StaState* st; };

int bind(geoac_ctx* ctx, const char* what, bool create, Bound* b){
    int rc = bind_launch(ctx, what, GEOAC_SLOT_STA, &b->v);
    if(rc) return rc;
    b->ctx = ctx;
    if(!*b->v.state && create) *b->v.state = new StaState();
    b->st = (StaState*)*b->v.state;
    return GEOAC_OK;
}

// current lists, or GEOAC_E_INVALID
int bind_lists(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = bind(ctx, what, false, b);
    if(rc) return rc;
    if(!b->st || b->st->sta_gen != b->v.map.gen)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no station lists of the last completed launch (call geoac_fan_stations after geoac_fan_launch)").c_str());
    return GEOAC_OK;
}

}  // namespace

extern "C" void geoac_sta_release(void* state){
    StaState* st = (StaState*)state;
    if(!st) return;
    if(st->land) hipFree(st->land);
    st->lb.release();
    delete st;
}

extern "C" const char* geoac_station_fault(int eqset, const geoac_station_spec* spec, int n_rays, int n_sta){
    int code;
    return spec_fault(eqset, spec, n_rays, n_sta, &code);
}

std::string geoac_lattice_fault(const GeoacLaunchView& v, int nt, int np){
    if(v.n_ang != v.map.n_rays || !v.theta_deg || !v.phi_deg) return "the context holds no launch angles for the records";
    for(int j = 0; j < np; j++)
        for(int i = 0; i < nt; i++)
            if(!same_bits(v.theta_deg[(size_t)j * nt + i], v.theta_deg[i]) || !same_bits(v.phi_deg[(size_t)j * nt + i], v.phi_deg[(size_t)j * nt]))
                return "the launch angles are not an n_theta x n_phi lattice (ray " + std::to_string((size_t)j * nt + i) +
                       " differs from its row's theta or its column's phi; ray = j * n_theta + i, the order of geoac_fan_enumerate)";
    return std::string();
}

void geoac_lattice_extent(int leg_min, int leg_max, int legs, int nt, int np, int phi_periodic, int* leg0, int* n_legs, int* n_cells){
    const int leg_last = leg_max < legs - 1 ? leg_max : legs - 1;
    *leg0 = leg_min;
    *n_legs = leg_last >= leg_min ? leg_last - leg_min + 1 : 0;
    *n_cells = (nt - 1) * (phi_periodic ? np : np - 1);
}

extern "C" int geoac_sta_land_dev(geoac_ctx* ctx, const char* what, const void** land_dev){
    Bound b;
    int rc = bind(ctx, what, true, &b);
    if(rc) return rc;
    StaState* st = b.st; const GeoacMapView& v = b.v.map;
    if(st->land_gen != v.gen){
        const size_t n_land = (size_t)v.M * v.legs * v.n_rays;
        if(grow(&st->land, &st->land_cap, sizeof(double4) * n_land))
            return geoac_map_fail(ctx, GEOAC_E_NOMEM, (std::string(what) + ": no device memory for the landing table (" + std::to_string((sizeof(double4) * n_land) >> 20) + " MiB)").c_str());
        StaDev D{};
        D.rec = v.rec; D.land = (double4*)st->land; D.spherical = spherical(v.eqset) ? 1 : 0;
        D.M = v.M; D.n_rays = v.n_rays; D.legs = v.legs;
        hipLaunchKernelGGL(k_sta_prep, dim3(blocks_for((long long)n_land, 256)), dim3(256), 0, (hipStream_t)v.stream, D);
        GEOAC_CHK(what, hipGetLastError());
        st->land_gen = v.gen;
    }
    if(land_dev) *land_dev = st->land;
    return GEOAC_OK;
}

extern "C" int geoac_station_check(int eqset, const geoac_station_spec* spec, int n_rays, int n_sta){
    int code;
    return spec_fault(eqset, spec, n_rays, n_sta, &code) ? code : GEOAC_OK;
}

extern "C" int geoac_fan_stations(geoac_ctx* ctx, const geoac_station_spec* spec, int n_sta, const double* sta){
    const char* what = "fan_stations";
    Bound b;
    int rc = bind(ctx, what, true, &b);
    if(rc) return rc;
    const GeoacMapView& v = b.v.map;
    int code;
    if(const char* fault = spec_fault(v.eqset, spec, v.n_rays, n_sta, &code)) return geoac_map_fail(ctx, code, (std::string("fan_stations: ") + fault).c_str());
    if(!sta) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_stations: sta is NULL");
    const int nt = spec->n_theta, np = spec->n_phi;
    const std::string lattice = geoac_lattice_fault(b.v, nt, np);
    if(!lattice.empty()) return geoac_map_fail(ctx, GEOAC_E_INVALID, ("fan_stations: " + lattice).c_str());
    StaState* st = b.st;
    hipStream_t s = (hipStream_t)v.stream;
    st->sta_gen = 0;                                   // (no current lists until these are complete)
    GEOAC_CHK(what, st->lb.ev.start(s));
    void* level = nullptr; size_t level_bytes = 0; const void* land = nullptr;
    if((rc = geoac_fan_level_dev(ctx, &level, &level_bytes))) return rc;         // (formed on first use after a launch, geoac_map.hip)
    if((rc = geoac_sta_land_dev(ctx, what, &land))) return rc;                   // (the same, below)
    st->M = v.M; st->F = v.F; st->n_sta = n_sta; st->cap = spec->cap;

    StaDev D{};
    D.rec = v.rec; D.level = (const double*)level; D.land = (double4*)land;
    D.turn_tol = spec->turn_tol; D.edge2 = spec->edge_max * spec->edge_max;
    D.spherical = spherical(v.eqset) ? 1 : 0; D.periodic = spec->phi_periodic;
    D.M = v.M; D.F = v.F; D.n_rays = v.n_rays; D.legs = v.legs; D.n_theta = nt; D.n_phi = np; D.n_sta = n_sta; D.cap = spec->cap;
    int n_legs;
    geoac_lattice_extent(spec->leg_min, spec->leg_max, v.legs, nt, np, spec->phi_periodic, &D.leg0, &n_legs, &D.n_cells);
    const long long n_seg_all = list_segments(&D, n_legs);

    const size_t out_need = st->rows_bytes() + st->level_bytes() + st->hits_bytes();
    if(list_grow(&st->lb, D, 0, n_seg_all, out_need))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_stations: no device memory for the lists (" + std::to_string(out_need >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(n_sta) + " stations x " + std::to_string(spec->cap) + " rows)").c_str());
    GEOAC_CHK(what, list_fill(&st->lb, &D, b.v, sta, s));
    D.lvl = (double*)((char*)st->lb.out + st->rows_bytes()); D.hits = (unsigned*)((char*)st->lb.out + st->rows_bytes() + st->level_bytes());
    GEOAC_CHK(what, list_launch(k_sta_count, k_sta_rows, D, st->lb.out, out_need, n_seg_all, s));
    GEOAC_CHK(what, st->lb.ev.stop(s));
    st->sta_gen = v.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_stations_shape(geoac_ctx* ctx, int* n_members, int* n_freq, int* n_sta, int* cap){
    Bound b;
    int rc = bind_lists(ctx, "fan_stations_shape", &b);
    if(rc) return rc;
    if(n_members) *n_members = b.st->M;
    if(n_freq) *n_freq = b.st->F;
    if(n_sta) *n_sta = b.st->n_sta;
    if(cap) *cap = b.st->cap;
    return GEOAC_OK;
}

// for geoac_refine.hip: the stations of the current lists as the kernels read them (the tail of `axes`)
extern "C" int geoac_sta_coords_dev(geoac_ctx* ctx, const double** sta_dev, int* n_sta){
    Bound b;
    int rc = bind_lists(ctx, "fan_refine", &b);
    if(rc) return rc;
    if(sta_dev) *sta_dev = (const double*)b.st->lb.axes + (b.st->lb.h_axes.size() - 2 * (size_t)b.st->n_sta);
    if(n_sta) *n_sta = b.st->n_sta;
    return GEOAC_OK;
}

extern "C" int geoac_fan_stations_dev(geoac_ctx* ctx, int which, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_lists(ctx, "fan_stations_dev", &b);
    if(rc) return rc;
    if(which < 0 || which > 2) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_stations_dev: which must be 0 (hits), 1 (rows) or 2 (level)");
    const StaState* st = b.st;
    const size_t off = which == 1 ? 0 : (which == 2 ? st->rows_bytes() : st->rows_bytes() + st->level_bytes());
    if(dev_ptr) *dev_ptr = (char*)st->lb.out + off;
    if(bytes) *bytes = which == 1 ? st->rows_bytes() : (which == 2 ? st->level_bytes() : st->hits_bytes());
    return GEOAC_OK;
}

extern "C" int geoac_fan_stations_fetch(geoac_ctx* ctx, uint32_t* hits, double* rows, double* level){
    const char* what = "fan_stations_fetch";
    Bound b;
    int rc = bind_lists(ctx, what, &b);
    if(rc) return rc;
    const StaState* st = b.st;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    const char* base = (const char*)st->lb.out;
    if(rows) GEOAC_CHK(what, hipMemcpyAsync(rows, base, st->rows_bytes(), hipMemcpyDeviceToHost, s));
    if(level) GEOAC_CHK(what, hipMemcpyAsync(level, base + st->rows_bytes(), st->level_bytes(), hipMemcpyDeviceToHost, s));
    if(hits) GEOAC_CHK(what, hipMemcpyAsync(hits, base + st->rows_bytes() + st->level_bytes(), st->hits_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_stations_timing(geoac_ctx* ctx, double* ms){
    const char* what = "fan_stations_timing";
    Bound b;
    int rc = bind_lists(ctx, what, &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_stations_timing: NULL argument");
    GEOAC_CHK(what, b.st->lb.ev.ms(ms));
    return GEOAC_OK;
}
