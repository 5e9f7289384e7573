// geoac_lampmap.hip - level loudness maps (include/geoac_lampmap.h): the crossing triangles of the last completed launch rasterised per selected
// level on a regular grid as ray tubes - geometric and received amplitude per (member, level, cell) - on the device.
//
// Reads the crossing records (geoac_fan_levels_dev), the branch table of geoac_lstations.hip (geoac_lsta_xland_dev), the lattice axes of the launch
// angles, the members' source points and the launch's parameter block (geoac_lamp_view); writes only buffers of its own.  No kernel of the launch
// plan is involved, and no probe kernel is changed: the medium comes from geoac_launch_probe_atmo1d / geoac_launch_probe_grid (coop = 0), called
// once per profile on a host copy of the parameter block whose table pointers are advanced to that profile, as member_view / member_view_grid of
// geoac_kernels.hip advance them on the device.
//
// Kernels:
//   k_lampmap_points  the probe's abscissae: per profile the same Pk points - the selected levels (stratified sets: Ls heights or radii; grid set:
//                     Ls * cells cell centres at the level's height), then the n_src source points as the launch placed them.
//   k_lampmap_raster  <0>: the walk of k_ltube_raster - one lane per (member, selected level, selected branch, lattice cell), blocks of one 64-lane
//                     wave, the cooperative walk above coop_min (geoac_tube_walk.h), the arguments in a block of device memory.  At a proposed
//                     centre only the triangle rule runs (tri_rule); a hit is parked in the lane's registers and its amplitude chain - two SINCOSD,
//                     an EXP, some twenty f64 divisions and eight square roots - runs where the lanes meet again after the triangle's candidates
//                     (or when the lane finds a second hit), so that the lanes that miss do not wait for it candidate by candidate.  A usable
//                     hit adds 1 to COUNT and takes part in the key maxima of AMP_MAX and RAMP_MAX; any other adds 1 to WEAK.
//                     AX, AA and DET of header steps 1 and 2 depend on the triangle alone.  They are formed once per parked hit from the
//                     triangle's own corners, not per candidate centre: the cooperative walk broadcasts a WalkTri and nothing else, and the bits
//                     are the same wherever they are formed.
//                     <1>: the same walk again; usable hits whose RAMP key equals their cell's compete for LOUDEST with b * n_tri + tri.
//   k_lampmap_finish  one thread per (selected level, cell): keys back to doubles, the empty markers, DETECT.
// Every reduction is an integer atomic (u64 add; u64 max on the order-preserving key of a double; u64 min on the hit's key).  No LDS, no
// floating-point atomics.
//
// The arithmetic is fixed by the header and restated in tests/lampmap_reference.py: every product is rounded before it is added, so this file is
// compiled with contraction off (the pragma below; the Makefile gives the same flag).
//
// Index bounds, stated again at each load and store:
//   item < M * Ls * n_br * n_cells, so cell < n_cells, bi < n_br, ls < Ls, m < M;  b < B (branch_of);  l = sel[ls] < L (host: level_mask has no
//   bit at or above L);  corner rays < n_theta * n_phi = n_rays (host check), so ray % n_theta < n_theta and ray / n_theta < n_phi index the axes;
//   record slot k < capL (written by k_lsta_prep);  a proposed centre has i0 < n0, i1 < n1 (walk_box clips), so word < M * Ls * cells = W, and the
//   five layers are W words each;  probe point p < Pk of profile k < K: k * Pk + p < K * Pk, the extent of the probe's output.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/geoac_lampmap.h"
#include "geoac_device.h"
#include "geoac_launch_int.h"
#include "geoac_lstations_int.h"
#include "geoac_level_amp_int.h"
#include "geoac_lampmap_int.h"
#include "geoac_tube_walk.h"
#include "geoac_lamp_tube.h"

#pragma clang fp contract(off)

namespace {

const double kLampLn10 = 2.302585092994045684;
const long long kProbeChunk = 1ll << 16;          // points per geoac_launch_probe_grid call: 30 doubles of scratch each

struct LAmpDev {
    WalkGrid G;
    const double* lrec;                           // [M][n_rays][L][capL][GEOAC_LVL_STRIDE]
    const double4* xland;                         // [M][L][B][n_rays]: c0, c1, slot k, present
    const double* theta_ax; const double* phi_ax; // [n_theta], [n_phi]: the lattice axes of the launch angles [deg]
    const double* src3;                           // [M][3]: the members' source points in the layout of geoac_params.src
    double* pts;                                  // [1 or 3][Pk]: the probe's abscissae
    const double* med;                            // the probe's output: out9 [K Pk][9] | rho [K Pk] (1-D), api7 [K Pk][7] (grid)
    unsigned long long *layers, *stats;           // COUNT | WEAK | AMP_MAX | RAMP_MAX | LOUDEST, W words each; the three work counters
    double edge2, det_floor, r_earth, z_grnd;
    double z_level[GEOAC_MAX_LEVELS], r_level[GEOAC_MAX_LEVELS];          // z_km[l]; r_earth + z_km[l]
    int M, K, n_src, L, capL, n_rays, n_theta, n_phi, periodic;
    int B, ord_max, n_dir, dir_mask;              // branches of the table; directions selected
    int Ls, n_br, n_cells;                        // selected levels; selected branches = n_legs * n_dir * ord_max; cells of the lattice
    int eqset, grid;
    int sel[GEOAC_MAX_LEVELS];                    // sel[ls] < L: the selected levels in ascending order
    long long cells, W, Pk;                       // n0 * n1; M * Ls * cells; probe points per profile
};

// selected branch bi < n_br -> the table's branch b < B
__device__ inline int branch_of(const LAmpDev& D, int bi){
    const int per_leg = D.n_dir * D.ord_max;
    const int li = bi / per_leg, rem = bi - li * per_leg;          // li < n_legs
    const int ds = rem / D.ord_max, o = rem - ds * D.ord_max;      // ds < n_dir, o < ord_max
    const int d = D.dir_mask == 2 ? 1 : ds;
    return (li * 2 + d) * D.ord_max + o;
}

// probe point p (< Pk): its abscissae - the height coordinate alone, or (x, y, z)
__device__ inline void lampmap_put(const LAmpDev& D, long long p, double a, double b, double hc){
    if(!D.grid) D.pts[p] = hc;
    else { D.pts[p] = a; D.pts[D.Pk + p] = b; D.pts[2 * D.Pk + p] = hc; }
}

// one thread per probe point p < Pk: level points first (Ls, or Ls * cells cell centres), then the n_src sources as the launch placed them
__global__ void __launch_bounds__(256) k_lampmap_points(const LAmpDev* __restrict__ Dp){
    const LAmpDev& D = *Dp;
    const long long n_lvl = D.grid ? (long long)D.Ls * D.cells : (long long)D.Ls;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < D.Pk; p += stride){       // p < Pk = n_lvl + n_src
        if(p < n_lvl){
            const int ls = D.grid ? (int)(p / D.cells) : (int)p;                                       // < Ls
            const int l = D.sel[ls];                                                                  // < L
            if(D.grid){
                const long long c = p - (long long)ls * D.cells;                                      // < cells
                const int i0 = (int)(c / D.G.n1), i1 = (int)(c - (long long)i0 * D.G.n1);
                lampmap_put(D, p, D.G.o0 + ((double)i0 + 0.5) * D.G.s0, D.G.o1 + ((double)i1 + 0.5) * D.G.s1, D.z_level[l]);
            } else lampmap_put(D, p, 0.0, 0.0, D.eqset == GEOAC_EQ_GLOBAL ? D.r_level[l] : D.z_level[l]);
        } else {
            const double* s = D.src3 + 3 * ((p - n_lvl) * D.K);                                       // source p - n_lvl < n_src: member (p - n_lvl) * K < M
            if(D.eqset == GEOAC_EQ_GLOBAL){
                const double z = s[0] < D.z_grnd ? D.z_grnd : s[0];
                lampmap_put(D, p, 0.0, 0.0, z + D.r_earth);
            } else {
                const double z = D.z_grnd < s[2] ? s[2] : D.z_grnd;
                lampmap_put(D, p, s[0], s[1], z);
            }
        }
    }
}

// the probe's values at point g (< K * Pk)
__device__ inline LampMedium lampmap_medium(const LAmpDev& D, long long g){
    LampMedium m;
    if(D.grid){ const double* a = D.med + 7 * g; m.c = a[0]; m.rho = a[1]; m.u = a[2]; m.v = a[3]; }
    else { const double* o = D.med + 9 * g; m.c = o[0]; m.u = o[3]; m.v = o[6]; m.rho = D.med[9 * ((long long)D.K * D.Pk) + g]; }
    return m;
}

// a hit on its way from the candidate loop to its amplitude chain
struct LampHit {
    WalkTri T;
    double w0, w1, w2, s;
    int i0, i1, have;
};

// header steps 1 to 6 for a parked hit, and its reductions
template <int PASS>
__device__ inline void lampmap_flush(const LAmpDev& D, LampHit& H){
    H.have = 0;
    const WalkTri& T = H.T;
    const double W0 = H.w0 / H.s, W1 = H.w1 / H.s, W2 = H.w2 / H.s;
    const int ls = T.plane / D.B, b = T.plane - ls * D.B;          // plane = ls * B + b: ls < Ls, b < B
    const long long l = D.sel[ls];                                 // < L
    // 1. the crossing area, 2. the launch-angle area: the triangle's own
    const double ex1 = T.x1 - T.x0, ex2 = T.x2 - T.x0;
    double ey1 = T.y1 - T.y0, ey2 = T.y2 - T.y0;
    if(D.G.spherical){ ey1 = wrap180(ey1); ey2 = wrap180(ey2); }
    const double AX = ex1 * ey2 - ex2 * ey1;
    // corner rays r < n_rays = n_theta * n_phi: r % n_theta < n_theta, r / n_theta < n_phi
    const double th0 = D.theta_ax[T.r0 % D.n_theta], th1 = D.theta_ax[T.r1 % D.n_theta], th2 = D.theta_ax[T.r2 % D.n_theta];
    const double ph0 = D.phi_ax[T.r0 / D.n_theta], ph1 = D.phi_ax[T.r1 / D.n_theta], ph2 = D.phi_ax[T.r2 / D.n_theta];
    const double at1 = th1 - th0, at2 = th2 - th0, ap1 = wrap180(ph1 - ph0), ap2 = wrap180(ph2 - ph0);
    const double AA = at1 * ap2 - at2 * ap1;
    const double det = AX / AA;
    // 3. the level-station row's values; a corner's record: ray r < n_rays, slot k < capL
    const double* R0 = D.lrec + ((((long long)T.m * D.n_rays + T.r0) * D.L + l) * D.capL + (int)T.z0) * GEOAC_LVL_STRIDE;
    const double* R1 = D.lrec + ((((long long)T.m * D.n_rays + T.r1) * D.L + l) * D.capL + (int)T.z1) * GEOAC_LVL_STRIDE;
    const double* R2 = D.lrec + ((((long long)T.m * D.n_rays + T.r2) * D.L + l) * D.capL + (int)T.z2) * GEOAC_LVL_STRIDE;
    double p1 = ph1, p2 = ph2;
    if(D.periodic){ p1 = ph0 + wrap180(ph1 - ph0); p2 = ph0 + wrap180(ph2 - ph0); }
    const double theta = interp(W0, W1, W2, th0, th1, th2), phi = interp(W0, W1, W2, ph0, p1, p2);
    const double tt = interp(W0, W1, W2, R0[GEOAC_LVL_TTIME], R1[GEOAC_LVL_TTIME], R2[GEOAC_LVL_TTIME]);
    const double at = interp(W0, W1, W2, R0[GEOAC_LVL_ATTEN], R1[GEOAC_LVL_ATTEN], R2[GEOAC_LVL_ATTEN]);
    const double n0 = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 3], R1[GEOAC_LVL_P0 + 3], R2[GEOAC_LVL_P0 + 3]);
    const double n1 = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 4], R1[GEOAC_LVL_P0 + 4], R2[GEOAC_LVL_P0 + 4]);
    const double n2 = interp(W0, W1, W2, R0[GEOAC_LVL_P0 + 5], R1[GEOAC_LVL_P0 + 5], R2[GEOAC_LVL_P0 + 5]);
    // 4. the medium in profile k = m % K < K: the level point (the cell centre's on the grid set) and source m / K < n_src of the profile's Pk points
    const long long cell = (long long)H.i0 * D.G.n1 + H.i1;                                    // < cells
    const int k = T.m % D.K;
    const long long n_lvl = D.grid ? (long long)D.Ls * D.cells : (long long)D.Ls;
    const LampMedium med = lampmap_medium(D, k * D.Pk + (D.grid ? (long long)ls * D.cells + cell : (long long)ls));
    const LampMedium src = lampmap_medium(D, k * D.Pk + n_lvl + T.m / D.K);
    // 5. the amplitude, 6. the received amplitude
    const double s0 = D.G.o0 + ((double)H.i0 + 0.5) * D.G.s0;
    double tz, dd, amp;
    lamp_tube(D.eqset, med, src, theta, phi, n0, n1, n2, det, s0, D.r_level[l], &tz, &dd, &amp);
    const double ramp = amp * rfn_exp(-(at * (kLampLn10 / 20.0)));
    const bool usable = AA != 0.0 && fabs(det) > D.det_floor && rfn_finite(det) && det != 0.0 && rfn_finite(dd) && dd != 0.0 && rfn_finite(amp) && amp != 0.0 &&
                        rfn_finite(tt) && rfn_finite(at) && rfn_finite(ramp);
    const long long word = ((long long)T.m * D.Ls + ls) * D.cells + cell;                      // < W
    if(PASS == 0){
        if(usable){
            atomicAdd(&D.layers[word], 1ull);
            atomicMax(&D.layers[2 * D.W + word], geoac_key(amp));
            atomicMax(&D.layers[3 * D.W + word], geoac_key(ramp));
        } else atomicAdd(&D.layers[D.W + word], 1ull);
    } else if(usable && D.layers[3 * D.W + word] == geoac_key(ramp)){
        const unsigned long long key = (unsigned long long)((long long)b * (2ll * D.n_cells) + T.tri);
        atomicMin(&D.layers[4 * D.W + word], key);
    }
}

// the exact rule of geoac_lstations.h at the centre of cell (i0, i1); a hit is parked (the one parked before it goes through its chain first)
template <int PASS>
__device__ inline void lampmap_test(const LAmpDev& D, LampHit& H, const WalkTri& T, int i0, int i1){
    const double s0 = D.G.o0 + ((double)i0 + 0.5) * D.G.s0, s1 = D.G.o1 + ((double)i1 + 0.5) * D.G.s1;
    const double x0 = T.x0 - s0, x1 = T.x1 - s0, x2 = T.x2 - s0;
    double y0 = T.y0 - s1, y1 = T.y1 - s1, y2 = T.y2 - s1;
    if(D.G.spherical){ y0 = wrap180(y0); y1 = wrap180(y1); y2 = wrap180(y2); }
    const Tri R = tri_rule(x0, y0, x1, y1, x2, y2, D.edge2);
    if(!R.hit) return;
    if(H.have) lampmap_flush<PASS>(D, H);
    H.T = T; H.w0 = R.w0; H.w1 = R.w1; H.w2 = R.w2; H.s = R.s; H.i0 = i0; H.i1 = i1; H.have = 1;
}

__global__ void k_lampmap_args(LAmpDev D, LAmpDev* out){
    if(blockIdx.x == 0 && threadIdx.x == 0) *out = D;
}

// one lane per (member, selected level, selected branch, lattice cell); every lane of a wave makes the same number of trips, so that the
// ballots of walk_wave see whole waves.  Blocks of one wave: the waves' cost is uneven, so they are spread over the CUs one by one.
template <int PASS>
__global__ void __launch_bounds__(64) k_lampmap_raster(const LAmpDev* __restrict__ Dp, long long n_items){
    const LAmpDev& D = *Dp;
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long n_waves = (long long)gridDim.x * (blockDim.x >> 6);
    const int nt1 = D.n_theta - 1;
    WalkCount C;
    LampHit H;
    H.have = 0;
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
            walk_wave(D.G, ok, T, lane, &C, [&D, &H](const WalkTri& U, int i0, int i1){ lampmap_test<PASS>(D, H, U, i0, i1); });
            // the lanes meet again here: the hits parked on the way go through their chains together
            if(H.have) lampmap_flush<PASS>(D, H);
        }
    }
    if(PASS == 0) walk_totals(C, lane, D.stats);
}

// one thread per (selected level, cell): idx < Ls * cells; member m's word is m * Ls * cells + idx < W
__global__ void __launch_bounds__(256) k_lampmap_finish(unsigned long long* layers, unsigned* detect, int M, long long ls_cells, long long W, double detect_amp){
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < ls_cells; idx += stride){
        unsigned n = 0;
        for(int m = 0; m < M; m++){
            const long long word = (long long)m * ls_cells + idx;
            double ramp = 0.0;
            for(int q = 2; q <= 3; q++){
                const unsigned long long k = layers[q * W + word];
                // (no usable hit writes key 0, the key of a NaN with every bit set: 0 still means "no usable hit")
                const double v = k == 0ull ? -(double)INFINITY : geoac_unkey(k);
                layers[q * W + word] = (unsigned long long)__double_as_longlong(v);
                ramp = v;
            }
            if(ramp >= detect_amp) n++;                      // (false for every cell when detect_amp is NaN)
            // (LOUDEST: all ones is -1 as a signed word already)
        }
        if(detect) detect[idx] = n;                          // [Ls][n0][n1]
    }
}

// offsets of the parts of one device block, each on a 256-byte boundary
struct Carve {
    size_t off = 0;
    size_t operator()(size_t n){ const size_t at = off; off += (n + 255) / 256 * 256; return at; }
};

static_assert(sizeof(LAmpDev) <= 1024, "LAmpState::args holds one LAmpDev");

struct LAmpState {
    void* base = nullptr; size_t cap = 0;                // COUNT | WEAK | AMP_MAX | RAMP_MAX | LOUDEST | three work counters and a spare | DETECT
    void* args = nullptr; size_t args_cap = 0;           // the walk's arguments (k_lampmap_args)
    void* aux = nullptr; size_t aux_cap = 0;             // theta_ax | phi_ax | src3 | pts | med | out30 scratch (grid set)
    std::vector<double> h_aux;                           // host copy of theta_ax | phi_ax | src3 (alive while its copy runs)
    unsigned long long gen = 0;                          // the context's invalidation counter the map was made at (0: never)
    geoac_lampmap_spec spec{};
    int M = 0, Ls = 0, formed = 0, detect = 0;
    long long cells = 0;
    EventPair ev;
    size_t words() const { return (size_t)M * Ls * (size_t)cells; }
    size_t layer_bytes() const { return 8 * words(); }
    size_t stats_off() const { return GEOAC_LAMPMAP_LAYERS * layer_bytes(); }
    size_t detect_off() const { return stats_off() + 4 * 8; }
    size_t detect_bytes() const { return 4 * (size_t)Ls * (size_t)cells; }
    size_t bytes() const { return detect_off() + detect_bytes(); }
};

int popcount31(int mask){ int n = 0; for(int l = 0; l < 31; l++) n += (mask >> l) & 1; return n; }

const char* const kNoGlobalRngDep = "not available for GEOAC_EQ_GLOBAL_RNGDEP: on a range-dependent spherical grid the probe tube of geoac_level_amp.h is not converged behind a turning point, "
                                    "and a coarse lattice tube is no better conditioned (DESIGN 8p, 8q)";

// the first thing wrong with a spec, or NULL; *code the status it earns
const char* spec_fault(int eqset, const geoac_lampmap_spec* s, int n_rays, int n_levels, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset == GEOAC_EQ_GLOBAL_RNGDEP){ *code = GEOAC_E_UNSUPPORTED; return kNoGlobalRngDep; }
    // the grid, the lattice, the legs, the ordinals, the edge filter, the directions and the levels: geoac_ltube_check's own verdict on the shared
    // fields (and on an unknown set, the 2-D set and a NULL spec)
    geoac_ltube_spec t{};
    if(s){
        t.origin[0] = s->origin[0]; t.origin[1] = s->origin[1]; t.step[0] = s->step[0]; t.step[1] = s->step[1]; t.n[0] = s->n[0]; t.n[1] = s->n[1];
        t.wrap_lon = s->wrap_lon; t.n_theta = s->n_theta; t.n_phi = s->n_phi; t.phi_periodic = s->phi_periodic; t.leg_min = s->leg_min; t.leg_max = s->leg_max;
        t.ord_max = s->ord_max; t.edge_max = s->edge_max; t.dir_mask = s->dir_mask; t.level_mask = s->level_mask;
    }
    if(const char* f = geoac_ltube_fault(eqset, s ? &t : nullptr, n_rays, n_levels)){
        if(eqset == GEOAC_EQ_2D) *code = GEOAC_E_UNSUPPORTED;
        return f;
    }
    if(!std::isfinite(s->det_floor) || s->det_floor < 0.0) return "det_floor must be finite and >= 0";
    if(!std::isnan(s->detect_amp) && !(std::isfinite(s->detect_amp) && s->detect_amp > 0.0)) return "detect_amp must be NaN (no DETECT layer) or finite and > 0";
    return nullptr;
}

struct Bound { geoac_ctx* ctx; GeoacLaunchView v; LAmpState* st; };

int bind(geoac_ctx* ctx, const char* what, bool create, Bound* b){
    int rc = bind_launch(ctx, what, GEOAC_SLOT_LAMPMAP, &b->v);
    if(rc) return rc;
    b->ctx = ctx;
    if(!*b->v.state && create) *b->v.state = new LAmpState();
    b->st = (LAmpState*)*b->v.state;
    return GEOAC_OK;
}

// a current loudness map, or GEOAC_E_INVALID
int bind_map(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = bind(ctx, what, false, b);
    if(rc) return rc;
    if(!b->st || b->st->gen != b->v.map.gen)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no level loudness map of the last completed launch (call geoac_fan_level_ampmap after geoac_fan_launch)").c_str());
    // ... and the level list it was made of is still the launch's (geoac_set_levels does not move the invalidation counter)
    if((rc = geoac_fan_levels_dev(ctx, nullptr, nullptr, nullptr, nullptr)))
        return geoac_map_fail(ctx, rc, (std::string(what) + ": " + geoac_last_error(ctx)).c_str());
    return GEOAC_OK;
}

}  // namespace

extern "C" void geoac_lampmap_release(void* state){
    LAmpState* st = (LAmpState*)state;
    if(!st) return;
    if(st->base) hipFree(st->base);
    if(st->args) hipFree(st->args);
    if(st->aux) hipFree(st->aux);
    st->ev.release();
    delete st;
}

extern "C" const char* geoac_lampmap_fault(int eqset, const geoac_lampmap_spec* spec, int n_rays, int n_levels){
    int code;
    return spec_fault(eqset, spec, n_rays, n_levels, &code);
}

extern "C" int geoac_lampmap_check(int eqset, const geoac_lampmap_spec* spec, int n_rays, int n_levels, int64_t* cells, int* n_selected){
    int code;
    if(spec_fault(eqset, spec, n_rays, n_levels, &code)) return code;
    if(cells) *cells = (int64_t)spec->n[0] * spec->n[1];
    if(n_selected) *n_selected = popcount31(spec->level_mask);
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_ampmap(geoac_ctx* ctx, const geoac_lampmap_spec* spec){
    const char* what = "fan_level_ampmap";
    const std::string pre = "fan_level_ampmap: ";
    Bound b;
    int rc = bind(ctx, what, false, &b);
    if(rc) return rc;
    const GeoacMapView& v = b.v.map;
    int code;
    if(v.eqset == GEOAC_EQ_2D || v.eqset == GEOAC_EQ_GLOBAL_RNGDEP)
        return geoac_map_fail(ctx, GEOAC_E_UNSUPPORTED, (pre + spec_fault(v.eqset, spec, v.n_rays, 0, &code)).c_str());
    GeoacLampView lv;
    if((rc = geoac_lamp_view(ctx, &lv))) return rc;
    if(lv.mode & (GEOAC_MODE_WRITE_RAYS | GEOAC_MODE_WRITE_CAUSTICS))
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (pre + "not available with sample capture (WriteRays / WriteCaustics)").c_str());
    // the crossings of that launch: the last completed launch had levels, and the level list has not changed since
    void* lrec = nullptr; void* lcount = nullptr; size_t lrec_bytes = 0, lcount_bytes = 0;
    if((rc = geoac_fan_levels_dev(ctx, &lrec, &lrec_bytes, &lcount, &lcount_bytes)))
        return geoac_map_fail(ctx, rc, (pre + geoac_last_error(ctx)).c_str());
    int L = 0, capL = 0;
    double z_km[GEOAC_MAX_LEVELS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if((rc = geoac_get_levels(ctx, &L, z_km, &capL))) return rc;
    if(const char* fault = spec_fault(v.eqset, spec, v.n_rays, L, &code)) return geoac_map_fail(ctx, code, (pre + fault).c_str());
    if(capL < 1 || L > GEOAC_MAX_LEVELS || lrec_bytes != sizeof(double) * GEOAC_LVL_STRIDE * (size_t)v.M * v.n_rays * L * capL || lcount_bytes != sizeof(int) * (size_t)v.M * v.n_rays * L)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (pre + "the crossing records do not have the shape of the launch ([M][n_rays][L][cap])").c_str());
    const int nt = spec->n_theta, np = spec->n_phi;
    const std::string lattice = geoac_lattice_fault(b.v, nt, np);
    if(!lattice.empty()) return geoac_map_fail(ctx, GEOAC_E_INVALID, (pre + lattice).c_str());
    const int K = lv.n_profiles < 1 ? 1 : lv.n_profiles;
    if(!lv.dev_params || lv.n_members != v.M || v.M % K != 0 || (v.eqset == GEOAC_EQ_3D_RNGDEP) != (lv.grid != 0))
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (pre + "the members, profiles or tables of the context are not those of the last completed launch").c_str());
    if((rc = bind(ctx, what, true, &b))) return rc;      // (the state is created only now: a call refused above allocates nothing)
    LAmpState* st = b.st;
    hipStream_t s = (hipStream_t)v.stream;
    st->gen = 0;                                       // (no current map until this one is complete)
    st->spec = *spec;
    st->M = v.M; st->Ls = popcount31(spec->level_mask); st->cells = (long long)spec->n[0] * spec->n[1];
    st->detect = std::isnan(spec->detect_amp) ? 0 : 1;
    const int grid = lv.grid ? 1 : 0, n_src = v.M / K;
    const size_t Pk = (grid ? (size_t)st->Ls * (size_t)st->cells : (size_t)st->Ls) + (size_t)n_src, Pall = Pk * (size_t)K;
    if(Pk > 0x7fffffffull) return geoac_map_fail(ctx, GEOAC_E_INVALID, (pre + "more than 2^31 medium points per profile: select fewer levels or coarsen the grid").c_str());
    const size_t chunk = Pk < (size_t)kProbeChunk ? Pk : (size_t)kProbeChunk;
    Carve carve;
    const size_t n_host = (size_t)nt + np + 3 * (size_t)v.M;
    const size_t o_host = carve(sizeof(double) * n_host), o_pts = carve(sizeof(double) * (grid ? 3 : 1) * Pk), o_med = carve(sizeof(double) * (grid ? 7 : 10) * Pall),
                 o_out30 = carve(grid ? sizeof(double) * 30 * chunk : 0);
    // the layers before anything goes to the stream: a call refused for memory here has started no event (it keeps the state, with no current map)
    if(grow(&st->base, &st->cap, st->bytes()) || grow(&st->args, &st->args_cap, 1024) || grow(&st->aux, &st->aux_cap, carve.off))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, (pre + "no device memory for the layers and the medium (" + std::to_string((st->bytes() + carve.off) >> 20) + " MiB for " + std::to_string(v.M) +
                                                   " members x " + std::to_string(st->Ls) + " levels x " + std::to_string(st->cells) + " cells and " + std::to_string(Pall) + " medium points)").c_str());
    GEOAC_CHK(what, hipStreamSynchronize(s));          // (an earlier call's copy may still read h_aux)
    GEOAC_CHK(what, st->ev.start(s));
    const void* xland = nullptr;
    int B = 0, leg0 = 0, n_legs = 0, formed = 0;
    if((rc = geoac_lsta_xland_dev(ctx, what, spec->leg_min, spec->leg_max, spec->ord_max, &xland, &B, &leg0, &n_legs, &formed))){
        (void)st->ev.stop(s);                          // (the pair stays whole; the accessor's message stands)
        return rc;
    }
    st->formed = formed;
    char* aux = (char*)st->aux;
    // lattice axes as geoac_lstations.hip takes them, and the members' source points: one host block, one copy
    st->h_aux.resize(n_host);
    for(int i = 0; i < nt; i++) st->h_aux[i] = b.v.theta_deg[i];
    for(int j = 0; j < np; j++) st->h_aux[nt + j] = b.v.phi_deg[(size_t)j * nt];
    for(size_t q = 0; q < 3 * (size_t)v.M; q++) st->h_aux[(size_t)nt + np + q] = lv.src3[q];
    GEOAC_CHK(what, hipMemcpyAsync(aux + o_host, st->h_aux.data(), sizeof(double) * n_host, hipMemcpyHostToDevice, s));
    LAmpDev D{};
    D.G.o0 = spec->origin[0]; D.G.o1 = spec->origin[1]; D.G.s0 = spec->step[0]; D.G.s1 = spec->step[1]; D.G.n0 = spec->n[0]; D.G.n1 = spec->n[1];
    D.G.spherical = spherical(v.eqset) ? 1 : 0;
    D.G.pre2 = walk_pre2(spec->origin, spec->step, spec->n, spec->edge_max, spherical(v.eqset));
    // GEOAC_LTUBE_COOP (diagnostic, tools/perf_lampmap.py): another threshold for the cooperative walk; the layers do not depend on it
    D.G.coop_min = GEOAC_TUBE_COOP_MIN;
    if(const char* e = getenv("GEOAC_LTUBE_COOP")){ const long t = strtol(e, nullptr, 10); if(t >= 0 && t <= 0x7fffffffl) D.G.coop_min = (int)t; }
    D.lrec = (const double*)lrec; D.xland = (const double4*)xland;
    D.theta_ax = (const double*)(aux + o_host); D.phi_ax = D.theta_ax + nt; D.src3 = D.phi_ax + np;
    D.pts = (double*)(aux + o_pts); D.med = (const double*)(aux + o_med);
    D.layers = (unsigned long long*)st->base; D.stats = (unsigned long long*)((char*)st->base + st->stats_off());
    D.edge2 = spec->edge_max * spec->edge_max; D.det_floor = spec->det_floor; D.r_earth = lv.r_earth; D.z_grnd = lv.z_grnd;
    for(int l = 0; l < GEOAC_MAX_LEVELS; l++){ D.z_level[l] = l < L ? z_km[l] : 0.0; D.r_level[l] = l < L ? lv.r_earth + z_km[l] : 0.0; }
    D.M = v.M; D.K = K; D.n_src = n_src; D.L = L; D.capL = capL; D.n_rays = v.n_rays; D.n_theta = nt; D.n_phi = np; D.periodic = spec->phi_periodic;
    D.B = B; D.ord_max = spec->ord_max; D.dir_mask = spec->dir_mask; D.n_dir = spec->dir_mask == 3 ? 2 : 1;
    D.eqset = v.eqset; D.grid = grid;
    D.Ls = 0;
    for(int l = 0; l < L; l++) if((spec->level_mask >> l) & 1) D.sel[D.Ls++] = l;
    D.n_br = n_legs * D.n_dir * D.ord_max;
    int leg0_, n_legs_;
    geoac_lattice_extent(spec->leg_min, spec->leg_max, v.legs, nt, np, spec->phi_periodic, &leg0_, &n_legs_, &D.n_cells);
    D.cells = st->cells; D.W = (long long)st->words(); D.Pk = (long long)Pk;
    const long long n_items = (long long)v.M * D.Ls * D.n_br * D.n_cells;
    // COUNT, WEAK, the two key layers and the counters 0 (key 0: below every key a hit writes), LOUDEST all ones: -1 as a signed word
    GEOAC_CHK(what, hipMemsetAsync(st->base, 0, 4 * st->layer_bytes(), s));
    GEOAC_CHK(what, hipMemsetAsync((char*)st->base + 4 * st->layer_bytes(), 0xff, st->layer_bytes(), s));
    GEOAC_CHK(what, hipMemsetAsync((char*)st->base + st->stats_off(), 0, 4 * 8, s));
    hipLaunchKernelGGL(k_lampmap_args, dim3(1), dim3(64), 0, s, D, (LAmpDev*)st->args);
    const LAmpDev* args = (const LAmpDev*)st->args;
    hipLaunchKernelGGL(k_lampmap_points, dim3(blocks_for((long long)Pk, 256, 1ll << 16)), dim3(256), 0, s, args);
    GEOAC_CHK(what, hipGetLastError());
    // the medium, profile by profile: a host copy of the launch's parameter block with its tables advanced to profile k
    for(int k = 0; k < K; k++){
        GeoacDevParams P = *lv.dev_params;
        double* med = (double*)(aux + o_med);
        if(grid){
            if(K > 1){ P.gtab += (long long)k * P.gtab_stride; P.dev_consts += 3 * k; }
            for(size_t at = 0; at < Pk; at += chunk){      // points at .. at + n - 1 < Pk of profile k: api7 row k * Pk + at
                const int n = (int)(Pk - at < chunk ? Pk - at : chunk);
                GEOAC_CHK(what, geoac_launch_probe_grid(&P, n, D.pts + at, D.pts + Pk + at, D.pts + 2 * Pk + at, 0, (double*)(aux + o_out30), med + 7 * ((size_t)k * Pk + at), s));
            }
        } else {
            if(K > 1){
                P.seg += (size_t)k * P.nseg * GEOAC_SEGW; P.rho += (size_t)k * P.nseg * 4;
                if(P.atab) P.atab += (size_t)k * (P.nseg + 2) * GEOAC_ATABW;
            }
            GEOAC_CHK(what, geoac_launch_probe_atmo1d(&P, (int)Pk, D.pts, med + 9 * (size_t)k * Pk, med + 9 * Pall + (size_t)k * Pk, s));
        }
    }
    if(n_items > 0){
        const unsigned n_blk = blocks_for(n_items * 4, 256, 1ll << 18);  // (one wave of 64 items per block)
        hipLaunchKernelGGL(k_lampmap_raster<0>, dim3(n_blk), dim3(64), 0, s, args, n_items);
        hipLaunchKernelGGL(k_lampmap_raster<1>, dim3(n_blk), dim3(64), 0, s, args, n_items);
    }
    const long long ls_cells = (long long)D.Ls * D.cells;
    hipLaunchKernelGGL(k_lampmap_finish, dim3(blocks_for(ls_cells, 256, 1ll << 16)), dim3(256), 0, s, D.layers, st->detect ? (unsigned*)((char*)st->base + st->detect_off()) : (unsigned*)nullptr,
                       v.M, ls_cells, D.W, spec->detect_amp);
    GEOAC_CHK(what, hipGetLastError());
    GEOAC_CHK(what, st->ev.stop(s));
    st->gen = v.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_ampmap_shape(geoac_ctx* ctx, int* n_members, int* n_selected, int* n0, int* n1, int* has_detect){
    Bound b;
    int rc = bind_map(ctx, "fan_level_ampmap_shape", &b);
    if(rc) return rc;
    if(n_members) *n_members = b.st->M;
    if(n_selected) *n_selected = b.st->Ls;
    if(n0) *n0 = b.st->spec.n[0];
    if(n1) *n1 = b.st->spec.n[1];
    if(has_detect) *has_detect = b.st->detect;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_ampmap_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_map(ctx, "fan_level_ampmap_dev", &b);
    if(rc) return rc;
    if(layer < 0 || layer >= GEOAC_LAMPMAP_LAYERS) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_ampmap_dev: layer must be one of GEOAC_LAMPMAP_COUNT .. GEOAC_LAMPMAP_LOUDEST");
    if(dev_ptr) *dev_ptr = (char*)b.st->base + (size_t)layer * b.st->layer_bytes();
    if(bytes) *bytes = b.st->layer_bytes();
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_ampmap_fetch(geoac_ctx* ctx, int layer, void* host){
    const char* what = "fan_level_ampmap_fetch";
    Bound b;
    int rc = bind_map(ctx, what, &b);
    if(rc) return rc;
    if(layer < 0 || layer >= GEOAC_LAMPMAP_LAYERS) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_ampmap_fetch: layer must be one of GEOAC_LAMPMAP_COUNT .. GEOAC_LAMPMAP_LOUDEST");
    if(!host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_ampmap_fetch: NULL argument");
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, hipMemcpyAsync(host, (char*)b.st->base + (size_t)layer * b.st->layer_bytes(), b.st->layer_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_ampmap_fetch_detect(geoac_ctx* ctx, uint32_t* detect_host){
    const char* what = "fan_level_ampmap_fetch_detect";
    Bound b;
    int rc = bind_map(ctx, what, &b);
    if(rc) return rc;
    if(!b.st->detect) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_ampmap_fetch_detect: the map was made without a DETECT layer (detect_amp = NaN)");
    if(!detect_host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_ampmap_fetch_detect: NULL argument");
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, hipMemcpyAsync(detect_host, (char*)b.st->base + b.st->detect_off(), b.st->detect_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_ampmap_stats(geoac_ctx* ctx, uint64_t* stats4){
    const char* what = "fan_level_ampmap_stats";
    Bound b;
    int rc = bind_map(ctx, what, &b);
    if(rc) return rc;
    if(!stats4) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_ampmap_stats: NULL argument");
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, hipMemcpyAsync(stats4, (char*)b.st->base + b.st->stats_off(), 4 * 8, hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    stats4[3] = (uint64_t)b.st->formed;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_ampmap_timing(geoac_ctx* ctx, double* ms){
    Bound b;
    int rc = bind_map(ctx, "fan_level_ampmap_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_ampmap_timing: NULL argument");
    GEOAC_CHK("fan_level_ampmap_timing", b.st->ev.ms(ms));
    return GEOAC_OK;
}
