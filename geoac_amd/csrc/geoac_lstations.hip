// geoac_lstations.hip - level stations (include/geoac_lstations.h): first-order eigenray estimates at R receivers above the ground from the
// crossing records of the last completed launch (geoac_levels.h), on the device.
//
// Reads the crossing records and their counts (geoac_fan_levels_dev) and the lattice axes of the launch angles; writes only buffers of its
// own.  No kernel of the launch plan is involved, and geoac_stations.hip is not touched: what is shared is included (geoac_tri_rule.h,
// geoac_lattice_fault, geoac_lattice_extent), the rest is written here.
//
// Three kernels:
//   k_lsta_prep    branch table xland[M][L][B][n_rays] of (c0, c1, slot k, present).  One thread per (member, ray, level) walks the kept
//                  crossings once, in path order, with two ordinal counters (upward, downward) that reset when the leg changes, and files
//                  crossing k under its branch b = ((leg - leg0) * 2 + d) * ord_max + o.  The table is cleared first: an absent branch
//                  reads present = 0.  The ray index is the fastest axis, so the corner loads of neighbouring lanes coalesce as they do on
//                  the landing table of k_sta_count.  It depends on the launch, leg0, n_legs and ord_max, and is kept while those hold.
//   k_lsta_count   one wave per list segment (member, station, branch, chunk of LSTA_CHUNK lattice cells): the hits of the segment, on the
//                  plane (m, level_of[s], b) of the table.
//   k_lsta_rows    the same segments again.  A wave sums the integer counts of the segments before its own in the (member, station) list -
//                  its base - and, when it has hits and the base is below cap, walks its chunk once more: per trip of 64 cells a ballot
//                  per triangle of the cell and a prefix count give every hit its place.  Segments and triangles are walked in key order,
//                  so the rows come out sorted by b * n_tri + tri with no sort, no atomic and no floating-point reduction across threads:
//                  a list is the same bits on every run.  A row reads the three corners' crossing records through slot k.
// One lane tests both triangles of a lattice cell (they share two of the cell's four corners).
//
// The arithmetic is fixed by the header and restated in tests/lstation_reference.py: every product is rounded before it is added, so this
// file is compiled with contraction off (the pragma below; the Makefile gives the same flag).  Divisions and floor are IEEE.
//
// Index bounds, stated again at each load and store:
//   t < M * n_rays * L in k_lsta_prep, so ray < n_rays, l < L, m < M;  record slot k < min(count, capL) <= capL;  branch b < B (tested:
//   leg in leg0 .. leg0 + n_legs - 1, o < ord_max);  seg < M * n_sta * B * n_chunks, so s < n_sta, b < B, chunk < n_chunks, m < M;
//   level_of[s] in 0 .. L - 1 (checked on the host before the copy);  cell < n_cells, so the corner rays a, b, c, d < n_theta * n_phi = n_rays
//   (cell_rays; checked on the host: n_theta * n_phi == n_rays);  list row pos < cap (tested at the store).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/geoac_lstations.h"
#include "geoac_launch_int.h"
#include "geoac_lstations_int.h"
#include "geoac_tri_rule.h"

#pragma clang fp contract(off)

namespace {

const double kLstaPi = 3.141592653589793238462643;
const int LSTA_CHUNK = 2048;                     // lattice cells per list segment: 32 trips of a wave

struct LstaDev {
    const double* lrec; const int* lcount;        // the launch's crossings: [M][n_rays][L][capL][GEOAC_LVL_STRIDE], [M][n_rays][L]
    const double* theta_ax; const double* phi_ax; // [n_theta], [n_phi] lattice axes [deg]
    const double* sta;                            // [n_sta][2]
    const int* level_of;                          // [n_sta], each in 0 .. L - 1
    double4* xland;                               // [M][L][B][n_rays]: c0, c1, slot k, present
    unsigned* cnt;                                // [M][n_sta][nseg]: hits per list segment
    unsigned* hits; double* rows;                 // the lists
    double edge2;                                 // edge_max * edge_max
    int spherical, periodic;
    int M, L, capL, n_rays, n_theta, n_phi, n_sta, cap;
    int leg0, n_legs, ord_max, B;                 // legs leg0 .. leg0 + n_legs - 1 take part; B = n_legs * 2 * ord_max
    int n_cells, n_chunks, nseg;                  // cells of the lattice, chunks per branch, segments per list = B * n_chunks
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
        double4* plane = D.xland + (m * D.L + l) * D.B * (long long)D.n_rays + ray;      // branch b of this ray: plane[b * n_rays], b < B
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

// the triangle of three branch-table corners against a station: all three present, then the rule of geoac_tri_rule.h
__device__ inline Tri ltri_test(const LstaDev& D, const double4& c0, const double4& c1, const double4& c2, double s0, double s1){
    Tri T;
    T.w0 = T.w1 = T.w2 = T.s = 0.0; T.hit = false;
    if(!(c0.w != 0.0 && c1.w != 0.0 && c2.w != 0.0)) return T;
    const double x0 = c0.x - s0, x1 = c1.x - s0, x2 = c2.x - s0;
    double y0 = c0.y - s1, y1 = c1.y - s1, y2 = c2.y - s1;
    if(D.spherical){ y0 = wrap180(y0); y1 = wrap180(y1); y2 = wrap180(y2); }
    return tri_rule(x0, y0, x1, y1, x2, y2, D.edge2);
}

// ray indices of the corners a, b, c, d of a cell, cell < n_cells: every one < n_theta * n_phi
__device__ inline void lcell_rays(const LstaDev& D, int cell, int* a, int* b, int* c, int* d){
    const int nt1 = D.n_theta - 1;
    const int i = cell % nt1, j = cell / nt1;            // i <= n_theta - 2; j <= n_phi - 1 under phi_periodic, else <= n_phi - 2
    const int jn = (j + 1 == D.n_phi) ? 0 : j + 1;       // (only a periodic lattice has a cell in its last column)
    *a = j * D.n_theta + i; *b = *a + 1; *d = jn * D.n_theta + i; *c = *d + 1;
}

__device__ inline double lnear(double v0, double vk){ return v0 + wrap180(vk - v0); }

// the row of a hit; r0, r1, r2 the ray indices of its corners (< n_rays), k0, k1, k2 their record slots (< capL, written by k_lsta_prep)
__device__ void lwrite_row(const LstaDev& D, long long m, int l, int b, int tri, const Tri& T, int r0, int r1, int r2, int k0, int k1, int k2, double* row){
    const double W0 = T.w0 / T.s, W1 = T.w1 / T.s, W2 = T.w2 / T.s;
    const double* R0 = D.lrec + ((((m * D.n_rays + r0) * D.L + l) * D.capL) + k0) * GEOAC_LVL_STRIDE;
    const double* R1 = D.lrec + ((((m * D.n_rays + r1) * D.L + l) * D.capL) + k1) * GEOAC_LVL_STRIDE;
    const double* R2 = D.lrec + ((((m * D.n_rays + r2) * D.L + l) * D.capL) + k2) * GEOAC_LVL_STRIDE;
    const double p0 = D.phi_ax[r0 / D.n_theta];          // r / n_theta < n_phi
    double p1 = D.phi_ax[r1 / D.n_theta], p2 = D.phi_ax[r2 / D.n_theta];
    if(D.periodic){ p1 = lnear(p0, p1); p2 = lnear(p0, p2); }
    const int o = b % D.ord_max, ld = b / D.ord_max;
    row[GEOAC_LSTA_LEG] = (double)(D.leg0 + ld / 2);
    row[GEOAC_LSTA_DIR] = (ld & 1) ? -1.0 : 1.0;
    row[GEOAC_LSTA_ORD] = (double)o;
    row[GEOAC_LSTA_TRI] = (double)tri;
    row[GEOAC_LSTA_RAY0] = (double)r0;
    row[GEOAC_LSTA_ORIENT] = T.s > 0.0 ? 1.0 : -1.0;
    row[GEOAC_LSTA_W0] = W0; row[GEOAC_LSTA_W1] = W1; row[GEOAC_LSTA_W2] = W2;
    row[GEOAC_LSTA_THETA] = interp(W0, W1, W2, D.theta_ax[r0 % D.n_theta], D.theta_ax[r1 % D.n_theta], D.theta_ax[r2 % D.n_theta]);
    row[GEOAC_LSTA_PHI] = interp(W0, W1, W2, p0, p1, p2);
    row[GEOAC_LSTA_TTIME] = interp(W0, W1, W2, R0[GEOAC_LVL_TTIME], R1[GEOAC_LVL_TTIME], R2[GEOAC_LVL_TTIME]);
    row[GEOAC_LSTA_ATTEN] = interp(W0, W1, W2, R0[GEOAC_LVL_ATTEN], R1[GEOAC_LVL_ATTEN], R2[GEOAC_LVL_ATTEN]);
    row[GEOAC_LSTA_N0 + 0] = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 3], R1[GEOAC_LVL_P0 + 3], R2[GEOAC_LVL_P0 + 3]);
    row[GEOAC_LSTA_N0 + 1] = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 4], R1[GEOAC_LVL_P0 + 4], R2[GEOAC_LVL_P0 + 4]);
    row[GEOAC_LSTA_N0 + 2] = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 5], R1[GEOAC_LVL_P0 + 5], R2[GEOAC_LVL_P0 + 5]);
}

// a list segment, decoded from its index: seg = ((m * n_sta + s) * B + b) * n_chunks + chunk, seg < M * n_sta * B * n_chunks
struct LSeg { long long m; int s, b, chunk; long long list; };
__device__ inline LSeg lseg_of(const LstaDev& D, long long seg){
    LSeg S;
    S.chunk = (int)(seg % D.n_chunks); seg /= D.n_chunks;
    S.b = (int)(seg % D.B); seg /= D.B;
    S.list = seg;                                        // < M * n_sta
    S.s = (int)(seg % D.n_sta); S.m = seg / D.n_sta;
    return S;
}

// both triangles of the lane's cell on a plane of the table (cell >= cell_end: no hit); plane[r], r < n_rays
__device__ inline void lcell_test(const LstaDev& D, const double4* plane, int cell, int cell_end, double s0, double s1, Tri* A, Tri* Bt, double4* ca, double4* cb,
                                  double4* cc, double4* cd, int* a, int* b, int* c, int* d){
    A->hit = false; Bt->hit = false;
    if(cell >= cell_end) return;                         // cell < cell_end <= n_cells from here on
    lcell_rays(D, cell, a, b, c, d);
    *ca = plane[*a]; *cc = plane[*c];
    if(!(ca->w != 0.0 && cc->w != 0.0)) return;          // (both triangles hold corners a and c)
    *cb = plane[*b]; *cd = plane[*d];
    *A = ltri_test(D, *ca, *cb, *cc, s0, s1);
    *Bt = ltri_test(D, *ca, *cc, *cd, s0, s1);
}

// one wave per list segment: its hits
__global__ void __launch_bounds__(256) k_lsta_count(LstaDev D, long long n_seg_all){
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    for(long long seg = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); seg < n_seg_all; seg += n_waves){
        const LSeg S = lseg_of(D, seg);
        const int l = D.level_of[S.s];                   // s < n_sta; l in 0 .. L - 1 (host check)
        const double4* plane = D.xland + ((S.m * D.L + l) * D.B + S.b) * (long long)D.n_rays;       // plane (m, l, b) of [M][L][B]
        const double s0 = D.sta[2 * S.s], s1 = D.sta[2 * S.s + 1];
        const int c_begin = S.chunk * LSTA_CHUNK;
        const int c_end = c_begin + LSTA_CHUNK < D.n_cells ? c_begin + LSTA_CHUNK : D.n_cells;
        unsigned n = 0;
        for(int base = c_begin; base < c_end; base += 64){
            Tri A, Bt; double4 ca, cb, cc, cd; int a, b, c, d;
            lcell_test(D, plane, base + lane, c_end, s0, s1, &A, &Bt, &ca, &cb, &cc, &cd, &a, &b, &c, &d);
            n += (unsigned)__popcll(__ballot(A.hit)) + (unsigned)__popcll(__ballot(Bt.hit));
        }
        if(lane == 0) D.cnt[S.list * D.nseg + S.b * D.n_chunks + S.chunk] = n;          // [M n_sta][nseg], b * n_chunks + chunk < nseg
    }
}

// one wave per list segment: its base in the list, and its rows
__global__ void __launch_bounds__(256) k_lsta_rows(LstaDev D, long long n_seg_all){
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    for(long long seg = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); seg < n_seg_all; seg += n_waves){
        const LSeg S = lseg_of(D, seg);
        const int mine = S.b * D.n_chunks + S.chunk;     // < nseg
        const unsigned* cnt = D.cnt + S.list * D.nseg;
        unsigned before = 0, total = 0;
        for(int k = lane; k < D.nseg; k += 64){          // k < nseg
            const unsigned v = cnt[k];
            total += v;
            before += k < mine ? v : 0u;
        }
        for(int off = 32; off > 0; off >>= 1){
            total += (unsigned)__shfl_xor((int)total, off, 64);
            before += (unsigned)__shfl_xor((int)before, off, 64);
        }
        if(mine == 0 && lane == 0) D.hits[S.list] = total;          // list < M * n_sta
        if(cnt[mine] == 0u || before >= (unsigned)D.cap) continue;
        const int l = D.level_of[S.s];                   // s < n_sta; l in 0 .. L - 1 (host check)
        const double4* plane = D.xland + ((S.m * D.L + l) * D.B + S.b) * (long long)D.n_rays;
        const double s0 = D.sta[2 * S.s], s1 = D.sta[2 * S.s + 1];
        const int c_begin = S.chunk * LSTA_CHUNK;
        const int c_end = c_begin + LSTA_CHUNK < D.n_cells ? c_begin + LSTA_CHUNK : D.n_cells;
        const unsigned long long below = (1ull << lane) - 1ull;
        unsigned at = before;
        for(int base = c_begin; base < c_end && at < (unsigned)D.cap; base += 64){
            Tri A, Bt; double4 ca, cb, cc, cd; int a = 0, b = 0, c = 0, d = 0;
            ca.z = cb.z = cc.z = cd.z = 0.0;
            const int cell = base + lane;
            lcell_test(D, plane, cell, c_end, s0, s1, &A, &Bt, &ca, &cb, &cc, &cd, &a, &b, &c, &d);
            const unsigned long long ma = __ballot(A.hit), mb = __ballot(Bt.hit);
            const unsigned posA = at + (unsigned)__popcll(ma & below) + (unsigned)__popcll(mb & below);
            const unsigned posB = posA + (A.hit ? 1u : 0u);
            if(A.hit && posA < (unsigned)D.cap)          // row posA < cap of list < M * n_sta
                lwrite_row(D, S.m, l, S.b, 2 * cell, A, a, b, c, (int)ca.z, (int)cb.z, (int)cc.z, D.rows + (S.list * D.cap + posA) * GEOAC_LSTA_STRIDE);
            if(Bt.hit && posB < (unsigned)D.cap)
                lwrite_row(D, S.m, l, S.b, 2 * cell + 1, Bt, a, c, d, (int)ca.z, (int)cc.z, (int)cd.z, D.rows + (S.list * D.cap + posB) * GEOAC_LSTA_STRIDE);
            at += (unsigned)__popcll(ma) + (unsigned)__popcll(mb);
        }
    }
}

struct LstaState {
    void* xland = nullptr; size_t xland_cap = 0;
    void* axes = nullptr; size_t axes_cap = 0;            // theta_ax | phi_ax | sta | level_of
    void* cnt = nullptr; size_t cnt_cap = 0;
    void* out = nullptr; size_t out_cap = 0;              // rows | hits
    unsigned long long lsta_gen = 0, xland_gen = 0;       // the context's invalidation counter they were made at (0: never)
    int x_leg0 = -1, x_n_legs = -1, x_ord_max = -1;       // what the branch table was formed with
    std::vector<double> h_axes;                           // host copies of what `axes` is filled from (alive while the copies run)
    std::vector<int32_t> h_level_of;
    int M = 0, n_sta = 0, cap = 0;
    EventPair ev;
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
    if(st->axes) hipFree(st->axes);
    if(st->cnt) hipFree(st->cnt);
    if(st->out) hipFree(st->out);
    st->ev.release();
    delete st;
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
    GEOAC_CHK(what, st->ev.start(s));
    st->M = v.M; st->n_sta = n_sta; st->cap = spec->cap;

    LstaDev D{};
    D.lrec = (const double*)lrec; D.lcount = (const int*)lcount;
    D.edge2 = spec->edge_max * spec->edge_max;
    D.spherical = spherical(v.eqset) ? 1 : 0; D.periodic = spec->phi_periodic;
    D.M = v.M; D.L = L; D.capL = capL; D.n_rays = v.n_rays; D.n_theta = nt; D.n_phi = np; D.n_sta = n_sta; D.cap = spec->cap;
    geoac_lattice_extent(spec->leg_min, spec->leg_max, v.legs, nt, np, spec->phi_periodic, &D.leg0, &D.n_legs, &D.n_cells);
    D.ord_max = spec->ord_max;
    D.B = D.n_legs * 2 * D.ord_max;
    D.n_chunks = (D.n_cells + LSTA_CHUNK - 1) / LSTA_CHUNK;
    D.nseg = D.B * D.n_chunks;
    const long long n_lists = (long long)v.M * n_sta, n_seg_all = n_lists * D.nseg;
    const size_t n_xland = (size_t)v.M * L * D.B * v.n_rays;

    const size_t n_axes = (size_t)nt + np + 2 * (size_t)n_sta;
    const size_t axes_need = sizeof(double) * n_axes + sizeof(int32_t) * (size_t)n_sta;
    const size_t out_need = st->rows_bytes() + st->hits_bytes();
    const bool form = n_xland > 0 && (st->xland_gen != v.gen || st->x_leg0 != D.leg0 || st->x_n_legs != D.n_legs || st->x_ord_max != D.ord_max);
    if(form){
        st->xland_gen = 0;
        if(grow(&st->xland, &st->xland_cap, sizeof(double4) * n_xland))
            return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_level_stations: no device memory for the branch table (" + std::to_string((sizeof(double4) * n_xland) >> 20) + " MiB)").c_str());
    }
    if(grow(&st->axes, &st->axes_cap, axes_need) || grow(&st->cnt, &st->cnt_cap, sizeof(unsigned) * (size_t)n_seg_all) || grow(&st->out, &st->out_cap, out_need))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_level_stations: no device memory for the lists (" + std::to_string(out_need >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(n_sta) + " stations x " + std::to_string(spec->cap) + " rows)").c_str());
    D.xland = (double4*)st->xland;
    if(form){
        // cleared first: an absent branch reads present = 0
        GEOAC_CHK(what, hipMemsetAsync(st->xland, 0, sizeof(double4) * n_xland, s));
        hipLaunchKernelGGL(k_lsta_prep, dim3(blocks_for((long long)v.M * v.n_rays * L, 256)), dim3(256), 0, s, D);
        GEOAC_CHK(what, hipGetLastError());
        st->xland_gen = v.gen; st->x_leg0 = D.leg0; st->x_n_legs = D.n_legs; st->x_ord_max = D.ord_max;
    }
    // lattice axes, stations and their levels: two host blocks, two copies (the blocks live in the state until the next call)
    GEOAC_CHK(what, hipStreamSynchronize(s));             // (an earlier call's copies may still read the host blocks)
    st->h_axes.resize(n_axes);
    for(int i = 0; i < nt; i++) st->h_axes[i] = b.v.theta_deg[i];
    for(int j = 0; j < np; j++) st->h_axes[nt + j] = b.v.phi_deg[(size_t)j * nt];
    for(size_t k = 0; k < 2 * (size_t)n_sta; k++) st->h_axes[nt + np + k] = sta[k];
    st->h_level_of.assign(level_of, level_of + n_sta);
    GEOAC_CHK(what, hipMemcpyAsync(st->axes, st->h_axes.data(), sizeof(double) * n_axes, hipMemcpyHostToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync((char*)st->axes + sizeof(double) * n_axes, st->h_level_of.data(), sizeof(int32_t) * (size_t)n_sta, hipMemcpyHostToDevice, s));
    D.theta_ax = (const double*)st->axes; D.phi_ax = D.theta_ax + nt; D.sta = D.phi_ax + np;
    D.level_of = (const int*)((const char*)st->axes + sizeof(double) * n_axes);
    D.cnt = (unsigned*)st->cnt;
    D.rows = (double*)st->out; D.hits = (unsigned*)((char*)st->out + st->rows_bytes());
    GEOAC_CHK(what, hipMemsetAsync(st->out, 0, out_need, s));
    if(n_seg_all > 0){
        hipLaunchKernelGGL(k_lsta_count, dim3(blocks_for(n_seg_all, 4)), dim3(256), 0, s, D, n_seg_all);
        hipLaunchKernelGGL(k_lsta_rows, dim3(blocks_for(n_seg_all, 4)), dim3(256), 0, s, D, n_seg_all);
        GEOAC_CHK(what, hipGetLastError());
    }
    GEOAC_CHK(what, st->ev.stop(s));
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

extern "C" int geoac_fan_level_stations_dev(geoac_ctx* ctx, int which, void** dev_ptr, size_t* bytes){
    LBound b;
    int rc = lbind_lists(ctx, "fan_level_stations_dev", &b);
    if(rc) return rc;
    if(which < 0 || which > 1) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_stations_dev: which must be 0 (hits) or 1 (rows)");
    const LstaState* st = b.st;
    if(dev_ptr) *dev_ptr = (char*)st->out + (which == 1 ? 0 : st->rows_bytes());
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
    const char* base = (const char*)st->out;
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
    GEOAC_CHK(what, b.st->ev.ms(ms));
    return GEOAC_OK;
}
