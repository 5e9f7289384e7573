// geoac_stations.hip - station arrivals (include/geoac_stations.h): first-order eigenray estimates at R stations from the record table of the
// last completed launch, on the device.
//
// Reads the record table, the level table of geoac_map.hip and the lattice axes of the launch angles; writes only buffers of its own.  No
// kernel of the launch plan is involved.
//
// Three kernels:
//   k_sta_prep    landing table land[M][legs][n_rays] of (c0, c1, turn, valid), 32 B per corner instead of the 256 B of a record, in the map's
//                 coordinates.  It depends on the launch alone and is kept until the next launch.
//   k_sta_count   one wave per list segment (member, station, leg, chunk of STA_CHUNK lattice cells): the hits of the segment.
//   k_sta_rows    the same segments again.  A wave sums the counts of the segments before its own in the (member, station) list - its base in
//                 the list - and, when it has hits and the base is below cap, walks its chunk once more and writes the rows: per trip of 64
//                 cells a ballot per triangle of the cell and a prefix count give every hit its place.  Segments and triangles are walked
//                 in key order, so the rows come out sorted by leg * n_tri + tri with no sort, no atomic and no floating-point reduction
//                 across threads: a list is the same bits on every run.  Most segments have no hit and end after reading one count.
// One lane tests both triangles of a lattice cell (they share two of the cell's four corners).  There is no bounding-box reject in front
// of the cross products: in floating point it is not equivalent to the sign rule (a product difference can round to zero), and the three
// 32-byte corner loads it would need are the cost of the test anyway.
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
#include "geoac_launch_int.h"
#include "geoac_stations_int.h"
#include "geoac_tri_rule.h"

#pragma clang fp contract(off)

namespace {

const double kStaPi = 3.141592653589793238462643;
const int STA_CHUNK = 2048;                      // lattice cells per list segment: 32 trips of a wave

struct StaDev {
    const double* rec; const double* level;       // the launch's tables
    const double* theta_ax; const double* phi_ax; // [n_theta], [n_phi] lattice axes [deg]
    const double* sta;                            // [n_sta][2]
    double4* land;                                // [M][legs][n_rays]: c0, c1, turn, valid
    unsigned* cnt;                                // [M][n_sta][nseg]: hits per list segment
    unsigned* hits; double* rows; double* lvl;    // the lists
    double turn_tol, edge2;                       // edge2 = edge_max * edge_max
    int spherical, periodic;
    int M, F, n_rays, legs, n_theta, n_phi, n_sta, cap;
    int leg0, n_legs;                             // legs leg0 .. leg0 + n_legs - 1 take part
    int n_cells, n_chunks, nseg;                  // cells of the lattice, chunks per leg, segments per list = n_legs * n_chunks
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

// the triangle of three landing-table corners against a station: the filters on the corners, then the rule of geoac_tri_rule.h
__device__ inline Tri tri_test(const StaDev& D, const double4& c0, const double4& c1, const double4& c2, double s0, double s1){
    Tri T;
    T.w0 = T.w1 = T.w2 = T.s = 0.0; T.hit = false;
    if(!(c0.w != 0.0 && c1.w != 0.0 && c2.w != 0.0)) return T;
    const double tmx = dmax(dmax(c0.z, c1.z), c2.z), tmn = dmin(dmin(c0.z, c1.z), c2.z);
    if(!(tmx - tmn <= D.turn_tol)) return T;
    const double x0 = c0.x - s0, x1 = c1.x - s0, x2 = c2.x - s0;
    double y0 = c0.y - s1, y1 = c1.y - s1, y2 = c2.y - s1;
    if(D.spherical){ y0 = wrap180(y0); y1 = wrap180(y1); y2 = wrap180(y2); }
    return tri_rule(x0, y0, x1, y1, x2, y2, D.edge2);
}

// ray indices of the corners a, b, c, d of a cell
__device__ inline void cell_rays(const StaDev& D, int cell, int* a, int* b, int* c, int* d){
    const int nt1 = D.n_theta - 1;
    const int i = cell % nt1, j = cell / nt1;
    const int jn = (j + 1 == D.n_phi) ? 0 : j + 1;       // (only a periodic lattice has a cell in its last column)
    *a = j * D.n_theta + i; *b = *a + 1; *d = jn * D.n_theta + i; *c = *d + 1;
}

__device__ inline double near(double v0, double vk){ return v0 + wrap180(vk - v0); }

// the row of a hit; r0, r1, r2 the ray indices of its corners
__device__ void write_row(const StaDev& D, long long m, int leg, int tri, const Tri& T, int r0, int r1, int r2, double* row, double* lv){
    const double W0 = T.w0 / T.s, W1 = T.w1 / T.s, W2 = T.w2 / T.s;
    const long long per_m = (long long)D.n_rays * D.legs;
    const double* R0 = D.rec + (m * per_m + (long long)r0 * D.legs + leg) * GEOAC_REC_STRIDE;
    const double* R1 = D.rec + (m * per_m + (long long)r1 * D.legs + leg) * GEOAC_REC_STRIDE;
    const double* R2 = D.rec + (m * per_m + (long long)r2 * D.legs + leg) * GEOAC_REC_STRIDE;
    const double p0 = D.phi_ax[r0 / D.n_theta];
    double p1 = D.phi_ax[r1 / D.n_theta], p2 = D.phi_ax[r2 / D.n_theta];
    if(D.periodic){ p1 = near(p0, p1); p2 = near(p0, p2); }
    const double b0 = R0[GEOAC_REC_BACKAZ];
    const double b1 = near(b0, R1[GEOAC_REC_BACKAZ]), b2 = near(b0, R2[GEOAC_REC_BACKAZ]);
    const double tt = interp(W0, W1, W2, R0[GEOAC_REC_TTIME], R1[GEOAC_REC_TTIME], R2[GEOAC_REC_TTIME]);
    const double rg = interp(W0, W1, W2, R0[GEOAC_REC_RANGE], R1[GEOAC_REC_RANGE], R2[GEOAC_REC_RANGE]);
    row[GEOAC_STA_LEG] = (double)leg;
    row[GEOAC_STA_TRI] = (double)tri;
    row[GEOAC_STA_RAY0] = (double)r0;
    row[GEOAC_STA_ORIENT] = T.s > 0.0 ? 1.0 : -1.0;
    row[GEOAC_STA_W0] = W0; row[GEOAC_STA_W1] = W1; row[GEOAC_STA_W2] = W2;
    row[GEOAC_STA_THETA] = interp(W0, W1, W2, D.theta_ax[r0 % D.n_theta], D.theta_ax[r1 % D.n_theta], D.theta_ax[r2 % D.n_theta]);
    row[GEOAC_STA_PHI] = interp(W0, W1, W2, p0, p1, p2);
    row[GEOAC_STA_TTIME] = tt;
    row[GEOAC_STA_CELERITY] = rg / tt;
    row[GEOAC_STA_TURN] = interp(W0, W1, W2, R0[GEOAC_REC_TURN], R1[GEOAC_REC_TURN], R2[GEOAC_REC_TURN]);
    row[GEOAC_STA_INCL] = interp(W0, W1, W2, R0[GEOAC_REC_INCL], R1[GEOAC_REC_INCL], R2[GEOAC_REC_INCL]);
    row[GEOAC_STA_BACKAZ] = interp(W0, W1, W2, b0, b1, b2);
    row[14] = 0.0; row[15] = 0.0;
    for(int f = 0; f < D.F; f++){
        const double* L = D.level + (m * D.F + f) * per_m;
        lv[f] = interp(W0, W1, W2, L[(long long)r0 * D.legs + leg], L[(long long)r1 * D.legs + leg], L[(long long)r2 * D.legs + leg]);
    }
}

// a list segment, decoded from its index: seg = ((m * n_sta + s) * n_legs + li) * n_chunks + chunk
struct Seg { long long m; int s, li, chunk; long long list; };
__device__ inline Seg seg_of(const StaDev& D, long long seg){
    Seg S;
    S.chunk = (int)(seg % D.n_chunks); seg /= D.n_chunks;
    S.li = (int)(seg % D.n_legs); seg /= D.n_legs;
    S.list = seg;
    S.s = (int)(seg % D.n_sta); S.m = seg / D.n_sta;
    return S;
}

// both triangles of the lane's cell on a leg (cell >= n_cells: no hit)
__device__ inline void cell_test(const StaDev& D, const double4* land, int cell, int cell_end, double s0, double s1, Tri* A, Tri* B, int* a, int* b, int* c, int* d){
    A->hit = false; B->hit = false;
    if(cell >= cell_end) return;
    cell_rays(D, cell, a, b, c, d);
    const double4 ca = land[*a], cc = land[*c];
    if(!(ca.w != 0.0 && cc.w != 0.0)) return;             // (both triangles hold corners a and c)
    const double4 cb = land[*b], cd = land[*d];
    *A = tri_test(D, ca, cb, cc, s0, s1);
    *B = tri_test(D, ca, cc, cd, s0, s1);
}

// one wave per list segment: its hits
__global__ void k_sta_count(StaDev D, long long n_seg_all){
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    for(long long seg = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); seg < n_seg_all; seg += n_waves){
        const Seg S = seg_of(D, seg);
        const int leg = D.leg0 + S.li;
        const double4* land = D.land + (S.m * D.legs + leg) * D.n_rays;
        const double s0 = D.sta[2 * S.s], s1 = D.sta[2 * S.s + 1];
        const int c_begin = S.chunk * STA_CHUNK;
        const int c_end = c_begin + STA_CHUNK < D.n_cells ? c_begin + STA_CHUNK : D.n_cells;
        unsigned n = 0;
        for(int base = c_begin; base < c_end; base += 64){
            Tri A, B; int a, b, c, d;
            cell_test(D, land, base + lane, c_end, s0, s1, &A, &B, &a, &b, &c, &d);
            n += (unsigned)__popcll(__ballot(A.hit)) + (unsigned)__popcll(__ballot(B.hit));
        }
        if(lane == 0) D.cnt[S.list * D.nseg + S.li * D.n_chunks + S.chunk] = n;
    }
}

// one wave per list segment: its base in the list, and its rows
__global__ void k_sta_rows(StaDev D, long long n_seg_all){
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    for(long long seg = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); seg < n_seg_all; seg += n_waves){
        const Seg S = seg_of(D, seg);
        const int mine = S.li * D.n_chunks + S.chunk;
        const unsigned* cnt = D.cnt + S.list * D.nseg;
        unsigned before = 0, total = 0;
        for(int k = lane; k < D.nseg; k += 64){
            const unsigned v = cnt[k];
            total += v;
            before += k < mine ? v : 0u;
        }
        for(int off = 32; off > 0; off >>= 1){
            total += (unsigned)__shfl_xor((int)total, off, 64);
            before += (unsigned)__shfl_xor((int)before, off, 64);
        }
        if(mine == 0 && lane == 0) D.hits[S.list] = total;
        if(cnt[mine] == 0u || before >= (unsigned)D.cap) continue;
        const int leg = D.leg0 + S.li;
        const double4* land = D.land + (S.m * D.legs + leg) * D.n_rays;
        const double s0 = D.sta[2 * S.s], s1 = D.sta[2 * S.s + 1];
        const int c_begin = S.chunk * STA_CHUNK;
        const int c_end = c_begin + STA_CHUNK < D.n_cells ? c_begin + STA_CHUNK : D.n_cells;
        const unsigned long long below = (1ull << lane) - 1ull;
        unsigned at = before;
        for(int base = c_begin; base < c_end && at < (unsigned)D.cap; base += 64){
            Tri A, B; int a = 0, b = 0, c = 0, d = 0;
            const int cell = base + lane;
            cell_test(D, land, cell, c_end, s0, s1, &A, &B, &a, &b, &c, &d);
            const unsigned long long ma = __ballot(A.hit), mb = __ballot(B.hit);
            const unsigned posA = at + (unsigned)__popcll(ma & below) + (unsigned)__popcll(mb & below);
            const unsigned posB = posA + (A.hit ? 1u : 0u);
            if(A.hit && posA < (unsigned)D.cap){
                const long long r = S.list * D.cap + posA;
                write_row(D, S.m, leg, 2 * cell, A, a, b, c, D.rows + r * GEOAC_STA_STRIDE, D.lvl + r * D.F);
            }
            if(B.hit && posB < (unsigned)D.cap){
                const long long r = S.list * D.cap + posB;
                write_row(D, S.m, leg, 2 * cell + 1, B, a, c, d, D.rows + r * GEOAC_STA_STRIDE, D.lvl + r * D.F);
            }
            at += (unsigned)__popcll(ma) + (unsigned)__popcll(mb);
        }
    }
}

struct StaState {
    void* land = nullptr; size_t land_cap = 0;
    void* axes = nullptr; size_t axes_cap = 0;            // theta_ax | phi_ax | sta
    void* cnt = nullptr; size_t cnt_cap = 0;
    void* out = nullptr; size_t out_cap = 0;              // rows | level | hits
    unsigned long long sta_gen = 0, land_gen = 0;         // the context's invalidation counter they were made at (0: never)
    std::vector<double> h_axes;                           // host copy of what `axes` is filled from (alive while the copy runs)
    int M = 0, F = 0, n_sta = 0, cap = 0;
    EventPair ev;
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
    if(st->axes) hipFree(st->axes);
    if(st->cnt) hipFree(st->cnt);
    if(st->out) hipFree(st->out);
    st->ev.release();
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
    GEOAC_CHK(what, st->ev.start(s));
    void* level = nullptr; size_t level_bytes = 0; const void* land = nullptr;
    if((rc = geoac_fan_level_dev(ctx, &level, &level_bytes))) return rc;         // (formed on first use after a launch, geoac_map.hip)
    if((rc = geoac_sta_land_dev(ctx, what, &land))) return rc;                   // (the same, below)
    st->M = v.M; st->F = v.F; st->n_sta = n_sta; st->cap = spec->cap;

    StaDev D{};
    D.rec = v.rec; D.level = (const double*)level;
    D.turn_tol = spec->turn_tol; D.edge2 = spec->edge_max * spec->edge_max;
    D.spherical = spherical(v.eqset) ? 1 : 0; D.periodic = spec->phi_periodic;
    D.M = v.M; D.F = v.F; D.n_rays = v.n_rays; D.legs = v.legs; D.n_theta = nt; D.n_phi = np; D.n_sta = n_sta; D.cap = spec->cap;
    geoac_lattice_extent(spec->leg_min, spec->leg_max, v.legs, nt, np, spec->phi_periodic, &D.leg0, &D.n_legs, &D.n_cells);
    D.n_chunks = (D.n_cells + STA_CHUNK - 1) / STA_CHUNK;
    D.nseg = D.n_legs * D.n_chunks;
    const long long n_lists = (long long)v.M * n_sta, n_seg_all = n_lists * D.nseg;

    const size_t n_axes = (size_t)nt + np + 2 * (size_t)n_sta;
    const size_t out_need = st->rows_bytes() + st->level_bytes() + st->hits_bytes();
    if(grow(&st->axes, &st->axes_cap, sizeof(double) * n_axes) ||
       grow(&st->cnt, &st->cnt_cap, sizeof(unsigned) * (size_t)n_seg_all) || grow(&st->out, &st->out_cap, out_need))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_stations: no device memory for the lists (" + std::to_string(out_need >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(n_sta) + " stations x " + std::to_string(spec->cap) + " rows)").c_str());
    // lattice axes and stations: one host block, one copy (the block lives in the state until the next call)
    GEOAC_CHK(what, hipStreamSynchronize(s));             // (an earlier call's copy may still read h_axes)
    st->h_axes.resize(n_axes);
    for(int i = 0; i < nt; i++) st->h_axes[i] = b.v.theta_deg[i];
    for(int j = 0; j < np; j++) st->h_axes[nt + j] = b.v.phi_deg[(size_t)j * nt];
    for(size_t k = 0; k < 2 * (size_t)n_sta; k++) st->h_axes[nt + np + k] = sta[k];
    GEOAC_CHK(what, hipMemcpyAsync(st->axes, st->h_axes.data(), sizeof(double) * n_axes, hipMemcpyHostToDevice, s));
    D.theta_ax = (const double*)st->axes; D.phi_ax = D.theta_ax + nt; D.sta = D.phi_ax + np;
    D.land = (double4*)land; D.cnt = (unsigned*)st->cnt;
    D.rows = (double*)st->out; D.lvl = (double*)((char*)st->out + st->rows_bytes()); D.hits = (unsigned*)((char*)st->out + st->rows_bytes() + st->level_bytes());
    GEOAC_CHK(what, hipMemsetAsync(st->out, 0, out_need, s));
    if(n_seg_all > 0){
        hipLaunchKernelGGL(k_sta_count, dim3(blocks_for(n_seg_all, 4)), dim3(256), 0, s, D, n_seg_all);
        hipLaunchKernelGGL(k_sta_rows, dim3(blocks_for(n_seg_all, 4)), dim3(256), 0, s, D, n_seg_all);
        GEOAC_CHK(what, hipGetLastError());
    }
    GEOAC_CHK(what, st->ev.stop(s));
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
    if(sta_dev) *sta_dev = (const double*)b.st->axes + (b.st->h_axes.size() - 2 * (size_t)b.st->n_sta);
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
    if(dev_ptr) *dev_ptr = (char*)st->out + off;
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
    const char* base = (const char*)st->out;
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
    GEOAC_CHK(what, b.st->ev.ms(ms));
    return GEOAC_OK;
}
