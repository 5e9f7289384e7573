// geoac_level_refine.hip - level refinement (include/geoac_level_refine.h): Newton eigenrays for every estimate of the level-station lists.
//
// A round is one fan of three rays per seed - the trial and two probes, one launch angle each moved by h - through the existing launch path
// (geoac_fan_set_angles, geoac_fan_launch with the level list still set: nothing of the launch plan is touched or known here) and one kernel
// that applies the header's step rule to every seed from its own member's crossing records (geoac_fan_levels_dev).  Every member integrates
// every ray; a seed reads one member's crossings, the other M - 1 are discarded (header, "Cost").
//
// Three kernels:
//   k_lrf_seed   one thread per (list, row): the kept rows of the level-station lists become the dense seed list, each at its list's prefix
//                count plus its place in the list - list order, no atomics (k_rfn_seed's scheme).  The prefix counts are integers summed on
//                the host from hits[M][n_sta].
//   k_lrf_step   one thread per seed, after a round's launch: the branch walk of the three rays, miss, accept / reject, Newton step, the next
//                trial and its probes; counts the seeds still active (the one integer the host reads per round).
//   k_lrf_rows   one thread per seed, after the last launch: the row.
// The kernels' arguments live in a block of device memory (LrfDev), as RfnDev does.  No LDS; the walk's state is a handful of registers.
//
// The arithmetic is fixed by the header and restated in tests/level_refine_reference.py; the elementary functions are geoac_rfn_series.h's.
// Every product is rounded before it is added, so this file is compiled with contraction off (the pragma below; the Makefile gives the same
// flag).
//
// Index bounds, stated again at each load and store.  N = n_seeds, the round's fan has 3 * N rays.
//   seed i < N;  list < n_lists = M * n_sta, so member m = list / n_sta < M and station s = list % n_sta < n_sta;  level l = level_of[s] in
//   0 .. L - 1 (checked on the host by geoac_fan_level_stations before its copy; L is that launch's, the level list has not changed);
//   ray = j * N + i < 3 * N, j in 0 .. 2;  (m, ray, l) < M * 3 * N * L, the extent of both crossing tables of the round (checked on the host
//   against the byte counts of geoac_fan_levels_dev after every launch);  record slot k < min(count, capL) <= capL.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/geoac_level_refine.h"
#include "geoac_launch_int.h"
#include "geoac_lstations_int.h"
#include "geoac_level_refine_int.h"
#include "geoac_rfn_series.h"

#pragma clang fp contract(off)

namespace {

enum { LRF_META = 6 };                            // ints per seed in LrfDev::meta

struct LrfDev {
    const double* lsta_rows; const unsigned* hits; // the level-station lists (read by k_lrf_seed only)
    const unsigned* offs;                         // [n_lists]: seeds before the list
    const double* sta; const int* level_of;       // [n_sta][2], [n_sta]: copies of this call's own
    const double* src;                            // [M][2]: the members' source points in the stations' axes
    int* meta;                                    // [n_seeds][LRF_META]: member, station, level, leg, direction (0 up, 1 down), ordinal
    double* trial;                                // [2][3 * n_seeds]: theta | phi of the next launch, ray j * n_seeds + i
    double* best;                                 // [5][n_seeds]: b_th | b_ph | b_miss | d_th | d_ph
    int* state;                                   // [3][n_seeds]: status (0: active) | shrink counter | rounds used
    unsigned* active;
    double* rows;
    double tol, step_max, h, r_earth;
    double r_level[GEOAC_MAX_LEVELS];             // r_earth + z_km[l]
    int spherical, max_shrink;
    int M, n_sta, cap, n_seeds, L, capL;
    long long n_lists;
};

// the three rays of seed i (< N) in the next launch: ray j * N + i < 3 * N; theta at trial[ray], phi at trial[3 * N + ray]
__device__ inline void lrf_set_trial(const LrfDev& D, long long i, double th, double ph){
    const long long N = D.n_seeds;
    D.trial[i] = th;              D.trial[3 * N + i] = ph;
    D.trial[N + i] = th + D.h;    D.trial[4 * N + i] = ph;
    D.trial[2 * N + i] = th;      D.trial[5 * N + i] = ph + D.h;
}

__global__ void k_lrf_seed(const LrfDev* __restrict__ Dp){
    const LrfDev& D = *Dp;
    const long long n = D.n_lists * D.cap;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for(long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride){        // t < n_lists * cap: a row of the lists
        const long long list = t / D.cap;                        // < n_lists
        const unsigned k = (unsigned)(t % D.cap);
        const unsigned h = D.hits[list];
        if(k >= (h < (unsigned)D.cap ? h : (unsigned)D.cap)) continue;
        const long long i = (long long)D.offs[list] + k;         // < n_seeds: offs[list] + min(hits, cap) <= the prefix count of the next list
        const double* row = D.lsta_rows + t * GEOAC_LSTA_STRIDE;
        const int s = (int)(list % D.n_sta);                     // < n_sta
        int* me = D.meta + LRF_META * i;
        me[0] = (int)(list / D.n_sta); me[1] = s; me[2] = D.level_of[s];
        me[3] = (int)row[GEOAC_LSTA_LEG]; me[4] = row[GEOAC_LSTA_DIR] > 0.0 ? 0 : 1; me[5] = (int)row[GEOAC_LSTA_ORD];
        const long long N = D.n_seeds;
        lrf_set_trial(D, i, row[GEOAC_LSTA_THETA], row[GEOAC_LSTA_PHI]);
        D.best[i] = 0.0; D.best[N + i] = 0.0; D.best[2 * N + i] = inf; D.best[3 * N + i] = 0.0; D.best[4 * N + i] = 0.0;
        D.state[i] = 0; D.state[N + i] = 0; D.state[2 * N + i] = 0;
    }
}

// BRANCH(ray) of the header: the crossing record of the seed's (leg, direction, ordinal) among the kept crossings of (m, ray, l), or NULL.
// ray < 3 * N, so rl < M * 3 * N * L, the extent of lcount and (times capL records) of lrec.
__device__ inline const double* lrf_branch(const LrfDev& D, const double* lrec, const int* lcount, const int* me, long long ray){
    const long long rl = ((long long)me[0] * (3ll * D.n_seeds) + ray) * D.L + me[2];
    const int seen = lcount[rl];
    const int kept = seen < D.capL ? seen : D.capL;              // only the first min(count, capL) crossings exist
    const double* R = lrec + rl * D.capL * GEOAC_LVL_STRIDE;
    int leg_now = -1, o_up = 0, o_down = 0;
    for(int k = 0; k < kept; k++, R += GEOAC_LVL_STRIDE){        // record slot k < kept <= capL
        const int leg = (int)R[GEOAC_LVL_LEG];
        if(leg != leg_now){ leg_now = leg; o_up = 0; o_down = 0; }
        const int d = R[GEOAC_LVL_DIR] > 0.0 ? 0 : 1;
        const int o = d ? o_down++ : o_up++;
        if(leg == me[3] && d == me[4] && o == me[5]) return R;
    }
    return nullptr;
}

// crossing point of a record in the stations' axes (geoac_lstations.h)
__device__ inline void lrf_point(const LrfDev& D, const double* R, double* c0, double* c1){
    if(D.spherical){ *c0 = R[GEOAC_LVL_P0 + 1] * 180.0 / kRfnPi; *c1 = R[GEOAC_LVL_P0 + 2] * 180.0 / kRfnPi; }
    else { *c0 = R[GEOAC_LVL_P0 + 0]; *c1 = R[GEOAC_LVL_P0 + 1]; }
}

// Newton step from the base crossing point and the two probes' records; false: SINGULAR
__device__ inline bool lrf_newton(const LrfDev& D, double c0, double c1, const double* Rt, const double* Rp, double s0, double s1, double* d_th, double* d_ph){
    if(!Rt || !Rp) return false;
    double ct0, ct1, cp0, cp1;
    lrf_point(D, Rt, &ct0, &ct1);
    lrf_point(D, Rp, &cp0, &cp1);
    const double e0 = s0 - c0, a00 = (ct0 - c0) / D.h, a01 = (cp0 - c0) / D.h;
    double e1, a10, a11;
    if(D.spherical){ e1 = wrap180(s1 - c1); a10 = wrap180(ct1 - c1) / D.h; a11 = wrap180(cp1 - c1) / D.h; }
    else { e1 = s1 - c1; a10 = (ct1 - c1) / D.h; a11 = (cp1 - c1) / D.h; }
    const double det = a00 * a11 - a01 * a10;
    double dt = (a11 * e0 - a01 * e1) / det;
    double dp = (a00 * e1 - a10 * e0) / det;
    if(det == 0.0 || !rfn_finite(det) || !rfn_finite(dt) || !rfn_finite(dp)) return false;
    if(dt > D.step_max) dt = D.step_max;
    if(dt < -D.step_max) dt = -D.step_max;
    if(dp > D.step_max) dp = D.step_max;
    if(dp < -D.step_max) dp = -D.step_max;
    *d_th = dt; *d_ph = dp;
    return true;
}

__global__ void k_lrf_step(const LrfDev* __restrict__ Dp, const double* __restrict__ lrec, const int* __restrict__ lcount, int round){
    const LrfDev& D = *Dp;
    const long long N = D.n_seeds;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= N || D.state[i] != 0) return;                        // i < N from here on
    const int* me = D.meta + LRF_META * i;
    const double s0 = D.sta[2 * me[1]], s1 = D.sta[2 * me[1] + 1];          // station me[1] < n_sta
    const double th = D.trial[i], ph = D.trial[3 * N + i];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double* R = lrf_branch(D, lrec, lcount, me, i);        // ray i: the trial itself
    double c0 = 0.0, c1 = 0.0, miss = inf;
    if(R){
        lrf_point(D, R, &c0, &c1);
        if(D.spherical) miss = rfn_dist(c0, c1, s0, s1, D.r_level[me[2]]);          // level me[2] < L <= GEOAC_MAX_LEVELS
        else { const double dx = s0 - c0, dy = s1 - c1; miss = sqrt(dx * dx + dy * dy); }
        if(!(miss == miss)) miss = inf;
    }
    int status = 0;
    D.state[2 * N + i] = round;
    if(miss <= D.tol){
        status = GEOAC_RFN_CONVERGED;
        D.best[i] = th; D.best[N + i] = ph; D.best[2 * N + i] = miss;
    } else if(round == 1 && miss == inf){
        status = GEOAC_RFN_LOST;
        D.best[i] = th; D.best[N + i] = ph;
    } else if(round == 1 || miss < D.best[2 * N + i]){
        double d_th = 0.0, d_ph = 0.0;
        D.best[i] = th; D.best[N + i] = ph; D.best[2 * N + i] = miss;
        D.state[N + i] = 0;
        // (miss < inf here unless round == 1, and then miss == inf was LOST: the base ray holds its branch)
        if(!lrf_newton(D, c0, c1, lrf_branch(D, lrec, lcount, me, N + i), lrf_branch(D, lrec, lcount, me, 2 * N + i), s0, s1, &d_th, &d_ph)) status = GEOAC_RFN_SINGULAR;
        D.best[3 * N + i] = d_th; D.best[4 * N + i] = d_ph;
    } else {
        D.best[3 * N + i] = D.best[3 * N + i] / 2.0;
        D.best[4 * N + i] = D.best[4 * N + i] / 2.0;
        const int n = D.state[N + i] + 1;
        D.state[N + i] = n;
        if(n > D.max_shrink) status = GEOAC_RFN_STALLED;
    }
    D.state[i] = status;
    if(status == 0){
        lrf_set_trial(D, i, D.best[i] + D.best[3 * N + i], D.best[N + i] + D.best[4 * N + i]);
        atomicAdd(D.active, 1u);
    } else lrf_set_trial(D, i, D.best[i], D.best[N + i]);
}

__global__ void k_lrf_rows(const LrfDev* __restrict__ Dp, const double* __restrict__ lrec, const int* __restrict__ lcount){
    const LrfDev& D = *Dp;
    const long long N = D.n_seeds;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= N) return;                                           // i < N from here on
    const int* me = D.meta + LRF_META * i;
    int status = D.state[i];
    if(status == 0){ status = GEOAC_RFN_ITER_LIMIT; D.state[i] = status; }
    double* row = D.rows + i * GEOAC_LRF_STRIDE;
    row[GEOAC_LRF_MEMBER] = (double)me[0]; row[GEOAC_LRF_STATION] = (double)me[1]; row[GEOAC_LRF_LEG] = (double)me[3];
    row[GEOAC_LRF_DIR] = me[4] ? -1.0 : 1.0; row[GEOAC_LRF_ORD] = (double)me[5];
    row[GEOAC_LRF_STATUS] = (double)status; row[GEOAC_LRF_ITER] = (double)D.state[2 * N + i];
    row[GEOAC_LRF_THETA] = D.best[i]; row[GEOAC_LRF_PHI] = D.best[N + i];
    row[GEOAC_LRF_MISS] = status == GEOAC_RFN_LOST ? -1.0 : D.best[2 * N + i];
    double tt = 0.0, cel = 0.0, att = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
    // a CONVERGED seed was integrated again at its best angles in the final launch: ray i holds the branch there (no record: the zeros stay)
    const double* R = status == GEOAC_RFN_CONVERGED ? lrf_branch(D, lrec, lcount, me, i) : nullptr;
    if(R){
        const double s0 = D.sta[2 * me[1]], s1 = D.sta[2 * me[1] + 1];      // station me[1] < n_sta
        const double* src = D.src + 2 * me[0];                              // member me[0] < M
        double range;
        if(D.spherical) range = rfn_dist(src[0], src[1], s0, s1, D.r_earth);
        else { const double dx = s0 - src[0], dy = s1 - src[1]; range = sqrt(dx * dx + dy * dy); }
        tt = R[GEOAC_LVL_TTIME]; cel = range / tt; att = R[GEOAC_LVL_ATTEN];
        n0 = R[GEOAC_LVL_P0 + 3]; n1 = R[GEOAC_LVL_P0 + 4]; n2 = R[GEOAC_LVL_P0 + 5];
    }
    row[GEOAC_LRF_TTIME] = tt; row[GEOAC_LRF_CELERITY] = cel; row[GEOAC_LRF_ATTEN] = att;
    row[GEOAC_LRF_N0 + 0] = n0; row[GEOAC_LRF_N0 + 1] = n1; row[GEOAC_LRF_N0 + 2] = n2;
}

struct LrfState {
    void* buf = nullptr; size_t buf_cap = 0;              // every device array of a call, carved below
    LrfDev h{};                                           // host copy of the argument block (alive while its copy runs)
    LrfDev* args = nullptr;
    std::vector<unsigned> h_offs;
    std::vector<double> h_src, h_trial;
    unsigned long long gen = 0;                           // the context's invalidation counter the result was made at (0: none)
    int n_seeds = 0, launches = 0;
    double ms_launch = 0.0, ms_kernels = 0.0;
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    EventPair ev;
    size_t rows_bytes() const { return sizeof(double) * (size_t)n_seeds * GEOAC_LRF_STRIDE; }
};

const char* spec_fault(int eqset, const geoac_level_refine_spec* s, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){
        *code = GEOAC_E_UNSUPPORTED;
        return "not implemented for the 2-D set: it has neither level crossings nor level-station lists to refine (geoac_lstations.h)";
    }
    if(!s) return "spec is NULL";
    if(s->max_iter < 1 || s->max_iter > GEOAC_RFN_MAX_ITER) return "max_iter must be in 1 .. 32";
    if(s->max_shrink < 0 || s->max_shrink > GEOAC_RFN_MAX_SHRINK) return "max_shrink must be in 0 .. 16";
    if(!std::isfinite(s->tol) || !(s->tol > 0.0)) return "tol must be finite and > 0";
    if(!std::isfinite(s->step_max_deg) || !(s->step_max_deg > 0.0)) return "step_max_deg must be finite and > 0";
    if(!std::isfinite(s->probe_deg) || !(s->probe_deg > 0.0) || s->probe_deg > 1.0) return "probe_deg must be finite, > 0 and <= 1";
    return nullptr;
}

struct Bound { geoac_ctx* ctx; GeoacLrfView v; LrfState* st; };

// (not bind_launch: geoac_fan_level_refine has its own message for a context without current lists, and the fetches ask for a current result)
int bind(geoac_ctx* ctx, const char* what, Bound* b){
    if(!ctx) return GEOAC_E_INVALID;
    b->ctx = ctx;
    int rc = geoac_lrf_view(ctx, &b->v);
    if(rc) return rc;
    b->st = (LrfState*)*b->v.state;
    if(hipSetDevice(b->v.map.device) != hipSuccess) return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": hipSetDevice failed").c_str());
    return GEOAC_OK;
}

// a current result, or GEOAC_E_INVALID.  (geoac_set_levels does not move the invalidation counter: the crossing tables answer for it.)
int bind_result(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = bind(ctx, what, b);
    if(rc) return rc;
    if(!b->st || b->st->gen == 0 || b->st->gen != b->v.map.gen || geoac_fan_levels_dev(ctx, nullptr, nullptr, nullptr, nullptr) != GEOAC_OK)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no level refinement result, or a launch, new angles, an atmosphere upload, geoac_set_sources, "
                                                     "geoac_set_frequencies or geoac_set_levels have come since it (call geoac_fan_level_refine again)").c_str());
    return GEOAC_OK;
}

size_t up256(size_t n){ return (n + 255) / 256 * 256; }

}  // namespace

extern "C" void geoac_lrf_release(void* state){
    LrfState* st = (LrfState*)state;
    if(!st) return;
    if(st->buf) hipFree(st->buf);
    st->ev.release();
    delete st;
}

extern "C" const char* geoac_level_refine_fault(int eqset, const geoac_level_refine_spec* spec){
    int code;
    return spec_fault(eqset, spec, &code);
}

extern "C" int geoac_level_refine_check(int eqset, const geoac_level_refine_spec* spec){
    int code;
    return spec_fault(eqset, spec, &code) ? code : GEOAC_OK;
}

extern "C" int geoac_fan_level_refine(geoac_ctx* ctx, const geoac_level_refine_spec* spec){
    const char* what = "fan_level_refine";
    Bound b;
    int rc = bind(ctx, what, &b);
    if(rc) return rc;
    int code;
    if(const char* fault = spec_fault(b.v.map.eqset, spec, &code)) return geoac_map_fail(ctx, code, (std::string("fan_level_refine: ") + fault).c_str());
    int M = 0, n_sta = 0, cap = 0;
    if(!b.v.map.fresh || geoac_fan_level_stations_shape(ctx, &M, &n_sta, &cap) != GEOAC_OK)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_refine: no level-station lists of the last completed launch (call geoac_fan_level_stations after a geoac_fan_launch with levels; "
                                                    "a launch, new angles, an atmosphere upload, geoac_set_sources and geoac_set_frequencies invalidate them)");
    void* lrec = nullptr; void* lcount = nullptr; size_t lrec_bytes = 0, lcount_bytes = 0;
    if((rc = geoac_fan_levels_dev(ctx, &lrec, &lrec_bytes, &lcount, &lcount_bytes)))
        return geoac_map_fail(ctx, rc, (std::string("fan_level_refine: ") + geoac_last_error(ctx)).c_str());
    if(b.v.mode & (GEOAC_MODE_WRITE_RAYS | GEOAC_MODE_WRITE_CAUSTICS))
        return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_refine: not available with sample capture (WriteRays / WriteCaustics)");
    if(M != b.v.n_members) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_refine: the members of the context are not those of the level-station lists");
    int L = 0, capL = 0;
    double z_km[GEOAC_MAX_LEVELS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if((rc = geoac_get_levels(ctx, &L, z_km, &capL))) return rc;
    if(L < 1 || L > GEOAC_MAX_LEVELS || capL < 1) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_refine: the context has no level list");
    hipStream_t s = (hipStream_t)b.v.map.stream;
    void* d_hits = nullptr; void* d_rows = nullptr; const double* d_sta = nullptr; const int* d_level_of = nullptr; size_t bytes = 0;
    if((rc = geoac_fan_level_stations_dev(ctx, 0, &d_hits, &bytes)) || (rc = geoac_fan_level_stations_dev(ctx, 1, &d_rows, &bytes)) ||
       (rc = geoac_lsta_coords_dev(ctx, &d_sta, &d_level_of, nullptr))) return rc;
    // seeds before every list: integer prefix counts of min(hits, cap), on the host
    const long long n_lists = (long long)M * n_sta;
    std::vector<unsigned> hits((size_t)n_lists);
    GEOAC_CHK(what, hipMemcpyAsync(hits.data(), d_hits, sizeof(unsigned) * (size_t)n_lists, hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    std::vector<unsigned> offs((size_t)n_lists);
    long long n_seeds = 0;
    for(long long l = 0; l < n_lists; l++){
        offs[(size_t)l] = (unsigned)n_seeds;
        n_seeds += hits[(size_t)l] < (unsigned)cap ? hits[(size_t)l] : (unsigned)cap;
        if(3 * n_seeds * M > GEOAC_RFN_MAX_RAY_MEMBERS)
            return geoac_map_fail(ctx, GEOAC_E_CAPACITY, ("fan_level_refine: more than " + std::to_string(GEOAC_RFN_MAX_RAY_MEMBERS) + " ray-members per round (3 rays x seeds x " + std::to_string(M) +
                                                          " members: every member integrates every seed and its two probes); refine fewer stations or members at a time").c_str());
    }
    if(!*b.v.state) *b.v.state = new LrfState();       // (the state is created only now: a refused call allocates nothing)
    LrfState* st = b.st = (LrfState*)*b.v.state;
    st->gen = 0;                                       // (no current result until this one is complete)
    st->h_offs.swap(offs);
    const size_t N = (size_t)n_seeds;
    st->n_seeds = (int)n_seeds; st->launches = 0; st->ms_launch = 0.0; st->ms_kernels = 0.0;
    for(int k = 0; k < 6; k++) st->stats[k] = 0;
    st->stats[2] = (uint64_t)n_seeds;
    if(n_seeds == 0){ st->gen = b.v.map.gen; return GEOAC_OK; }       // (an empty result; nothing was launched, the lists stay)

    // one device block: args | offs | sta | level_of | src | meta | trial | best | state | active | rows
    size_t off = 0;
    auto carve = [&](size_t n){ const size_t at = off; off += up256(n); return at; };
    const size_t o_args = carve(sizeof(LrfDev)), o_offs = carve(sizeof(unsigned) * (size_t)n_lists), o_sta = carve(sizeof(double) * 2 * (size_t)n_sta),
                 o_lof = carve(sizeof(int) * (size_t)n_sta), o_src = carve(sizeof(double) * 2 * (size_t)M), o_meta = carve(sizeof(int) * LRF_META * N),
                 o_trial = carve(sizeof(double) * 6 * N), o_best = carve(sizeof(double) * 5 * N), o_state = carve(sizeof(int) * 3 * N), o_active = carve(sizeof(unsigned)),
                 o_rows = carve(sizeof(double) * GEOAC_LRF_STRIDE * N);
    if(grow(&st->buf, &st->buf_cap, off)) return geoac_map_fail(ctx, GEOAC_E_NOMEM, "fan_level_refine: no device memory for the seeds");
    char* base = (char*)st->buf;
    st->args = (LrfDev*)(base + o_args);
    LrfDev& D = st->h;
    D = LrfDev{};
    D.lsta_rows = (const double*)d_rows; D.hits = (const unsigned*)d_hits; D.offs = (const unsigned*)(base + o_offs);
    D.sta = (const double*)(base + o_sta); D.level_of = (const int*)(base + o_lof); D.src = (const double*)(base + o_src);
    D.meta = (int*)(base + o_meta); D.trial = (double*)(base + o_trial); D.best = (double*)(base + o_best); D.state = (int*)(base + o_state);
    D.active = (unsigned*)(base + o_active); D.rows = (double*)(base + o_rows);
    D.tol = spec->tol; D.step_max = spec->step_max_deg; D.h = spec->probe_deg; D.r_earth = b.v.r_earth;
    for(int l = 0; l < GEOAC_MAX_LEVELS; l++) D.r_level[l] = l < L ? b.v.r_earth + z_km[l] : 0.0;
    D.spherical = spherical(b.v.map.eqset) ? 1 : 0; D.max_shrink = spec->max_shrink;
    D.M = M; D.n_sta = n_sta; D.cap = cap; D.n_seeds = (int)n_seeds; D.L = L; D.capL = capL; D.n_lists = n_lists;
    st->h_src.assign(b.v.src, b.v.src + 2 * (size_t)M);
    st->h_trial.resize(6 * N);
    GEOAC_CHK(what, hipMemcpyAsync(st->args, &D, sizeof(LrfDev), hipMemcpyHostToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_offs, st->h_offs.data(), sizeof(unsigned) * (size_t)n_lists, hipMemcpyHostToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_sta, d_sta, sizeof(double) * 2 * (size_t)n_sta, hipMemcpyDeviceToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_lof, d_level_of, sizeof(int) * (size_t)n_sta, hipMemcpyDeviceToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_src, st->h_src.data(), sizeof(double) * st->h_src.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_lrf_seed, dim3(blocks_for(n_lists * cap, 256)), dim3(256), 0, s, (const LrfDev*)st->args);
    GEOAC_CHK(what, hipGetLastError());

    const unsigned n_blk = blocks_for(n_seeds, 64);
    const int n_rays = 3 * (int)n_seeds;
    const size_t n_rl = (size_t)M * n_rays * L;          // (member, ray, level) of a round's crossing tables
    GeoacMapView mv{};
    unsigned active = 1;
    for(int round = 1; round <= spec->max_iter && active > 0; round++){
        // the trial angles and their probes: device -> host -> geoac_fan_set_angles (48 bytes per seed).  The sync also ends the seed kernel's
        // reads of the lists, which the launch invalidates.
        GEOAC_CHK(what, hipMemcpyAsync(st->h_trial.data(), D.trial, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, s));
        GEOAC_CHK(what, hipStreamSynchronize(s));
        if((rc = geoac_fan_set_angles(ctx, n_rays, st->h_trial.data(), st->h_trial.data() + 3 * N))) return rc;
        if((rc = geoac_fan_launch(ctx))) return rc;
        st->launches = round;
        st->stats[0] = (uint64_t)round; st->stats[1] += (uint64_t)n_rays * (uint64_t)M;
        double ms3[3] = {0, 0, 0}; uint64_t st3[3] = {0, 0, 0};
        if(geoac_last_timing(ctx, ms3, st3) == GEOAC_OK) st->ms_launch += ms3[0];
        if((rc = geoac_map_view(ctx, &mv))) return rc;
        if((rc = geoac_fan_levels_dev(ctx, &lrec, &lrec_bytes, &lcount, &lcount_bytes))) return rc;
        if(mv.M != M || mv.n_rays != n_rays || lcount_bytes != sizeof(int) * n_rl || lrec_bytes != sizeof(double) * GEOAC_LVL_STRIDE * n_rl * capL)
            return geoac_map_fail(ctx, GEOAC_E_HIP, "fan_level_refine: the round's crossing tables do not have the shape of the seeds ([M][3 * n_seeds][L][cap])");
        GEOAC_CHK(what, st->ev.start(s));
        GEOAC_CHK(what, hipMemsetAsync(D.active, 0, sizeof(unsigned), s));
        hipLaunchKernelGGL(k_lrf_step, dim3(n_blk), dim3(64), 0, s, (const LrfDev*)st->args, (const double*)lrec, (const int*)lcount, round);
        GEOAC_CHK(what, hipGetLastError());
        GEOAC_CHK(what, st->ev.stop(s));
        GEOAC_CHK(what, hipMemcpyAsync(&active, D.active, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        GEOAC_CHK(what, hipStreamSynchronize(s));
        double t = 0; GEOAC_CHK(what, st->ev.ms(&t));
        st->ms_kernels += t;
    }
    GEOAC_CHK(what, st->ev.start(s));
    hipLaunchKernelGGL(k_lrf_rows, dim3(n_blk), dim3(64), 0, s, (const LrfDev*)st->args, (const double*)lrec, (const int*)lcount);
    GEOAC_CHK(what, hipGetLastError());
    GEOAC_CHK(what, st->ev.stop(s));
    std::vector<int> status(N);
    GEOAC_CHK(what, hipMemcpyAsync(status.data(), D.state, sizeof(int) * N, hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    double t = 0; GEOAC_CHK(what, st->ev.ms(&t));
    st->ms_kernels += t;
    for(size_t i = 0; i < N; i++){
        const int c = status[i];
        st->stats[c == GEOAC_RFN_CONVERGED ? 3 : (c == GEOAC_RFN_STALLED || c == GEOAC_RFN_ITER_LIMIT ? 4 : 5)]++;
    }
    st->gen = mv.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_refine_shape(geoac_ctx* ctx, int* n_seeds, int* launches){
    Bound b;
    int rc = bind_result(ctx, "fan_level_refine_shape", &b);
    if(rc) return rc;
    if(n_seeds) *n_seeds = b.st->n_seeds;
    if(launches) *launches = b.st->launches;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_refine_dev(geoac_ctx* ctx, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_result(ctx, "fan_level_refine_dev", &b);
    if(rc) return rc;
    if(dev_ptr) *dev_ptr = b.st->n_seeds ? (void*)b.st->h.rows : nullptr;
    if(bytes) *bytes = b.st->rows_bytes();
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_refine_fetch(geoac_ctx* ctx, double* rows){
    const char* what = "fan_level_refine_fetch";
    Bound b;
    int rc = bind_result(ctx, what, &b);
    if(rc) return rc;
    if(b.st->n_seeds == 0 || !rows) return GEOAC_OK;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, hipMemcpyAsync(rows, b.st->h.rows, b.st->rows_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_refine_timing(geoac_ctx* ctx, double ms[2]){
    Bound b;
    int rc = bind_result(ctx, "fan_level_refine_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_refine_timing: NULL argument");
    ms[0] = b.st->ms_launch; ms[1] = b.st->ms_kernels;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_refine_stats(geoac_ctx* ctx, uint64_t stats[6]){
    Bound b;
    int rc = bind_result(ctx, "fan_level_refine_stats", &b);
    if(rc) return rc;
    if(!stats) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_refine_stats: NULL argument");
    for(int k = 0; k < 6; k++) stats[k] = b.st->stats[k];
    return GEOAC_OK;
}
