// geoac_level_refine.hip - level refinement (include/geoac_level_refine.h): Newton eigenrays for every estimate of the level-station lists.
//
// A round is one fan of three rays per seed - the trial and two probes, one launch angle each moved by h - through the existing launch path
// (geoac_fan_set_angles, geoac_fan_launch with the level list still set: nothing of the launch plan is touched or known here) and one kernel
// that applies the header's step rule to every seed from its own member's crossing records (geoac_fan_levels_dev).  Every member integrates
// every ray; a seed reads one member's crossings, the other M - 1 are discarded (header, "Cost").  The seed list, the rounds and the step
// rule are geoac_newton_rounds.h's, shared with geoac_refine.hip; this file's own are where a seed comes from (a level-station row), its
// miss and Jacobian (finite differences of two probe rays' crossing points) and what a finished row holds.
//
// Three kernels:
//   k_lrf_seed   one thread per (list, row): the kept rows of the level-station lists become the dense seed list, each at its list's prefix
//                count (integers summed on the host from hits[M][n_sta]) plus its place in the list - list order, no atomics.
//   k_lrf_step   one thread per seed, after a round's launch: the branch walk of the three rays, miss, the step rule, the next trial and its
//                probes; counts the seeds still active (the one integer the host reads per round).
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
#include <string>
#include <vector>

#include "../../include/geoac_level_refine.h"
#include "geoac_launch_int.h"
#include "geoac_lstations_int.h"
#include "geoac_level_refine_int.h"
#include "geoac_newton_rounds.h"

#pragma clang fp contract(off)

namespace {

enum { LRF_META = 6 };                            // ints per seed in LrfDev::meta

struct LrfDev : RoundsDev {
    enum { RAYS = 3 };
    const double* lsta_rows;                      // the level-station lists' rows (read by k_lrf_seed only)
    const int* level_of;                          // [n_sta]: a copy of this call's own
    const double* src;                            // [M][2]: the members' source points in the stations' axes
    int* meta;                                    // [n_seeds][LRF_META]: member, station, level, leg, direction (0 up, 1 down), ordinal
    double* rows;
    double h, r_earth;
    double r_level[GEOAC_MAX_LEVELS];             // r_earth + z_km[l]
    int L, capL;

    struct Seed { const int* me; double s0, s1, c0, c1; };               // the seed's meta row, its station, the trial ray's crossing point
    // the three rays of seed i (< N) in the next launch: ray j * N + i < 3 * N; theta at trial[ray], phi at trial[3 * N + ray]
    __device__ void set_trial(long long i, double th, double ph) const {
        const long long N = n_seeds;
        trial[i] = th;              trial[3 * N + i] = ph;
        trial[N + i] = th + h;      trial[4 * N + i] = ph;
        trial[2 * N + i] = th;      trial[5 * N + i] = ph + h;
    }
    __device__ double miss(long long i, const double* lrec, const int* lcount, Seed* S) const;
    __device__ bool newton(long long i, const Seed& S, double th, double ph, const double* lrec, const int* lcount, double* d_th, double* d_ph) const;
};

__global__ void k_lrf_seed(const LrfDev* __restrict__ Dp){
    const LrfDev& D = *Dp;
    const long long n = D.n_lists * D.cap;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride){        // t < n_lists * cap: a row of the lists
        const long long list = t / D.cap, i = seed_slot(D, list, (unsigned)(t % D.cap));          // list < n_lists
        if(i < 0) continue;                                      // i < n_seeds from here on
        const double* row = D.lsta_rows + t * GEOAC_LSTA_STRIDE;
        const int s = (int)(list % D.n_sta);                     // < n_sta
        int* me = D.meta + LRF_META * i;
        me[0] = (int)(list / D.n_sta); me[1] = s; me[2] = D.level_of[s];
        me[3] = (int)row[GEOAC_LSTA_LEG]; me[4] = row[GEOAC_LSTA_DIR] > 0.0 ? 0 : 1; me[5] = (int)row[GEOAC_LSTA_ORD];
        D.set_trial(i, row[GEOAC_LSTA_THETA], row[GEOAC_LSTA_PHI]);
        seed_init(D, i);
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

// miss of the trial's crossing point: ray i is the trial itself
__device__ inline double LrfDev::miss(long long i, const double* lrec, const int* lcount, Seed* S) const {
    const int* me = meta + LRF_META * i;
    const double s0 = sta[2 * me[1]], s1 = sta[2 * me[1] + 1];              // station me[1] < n_sta
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double* R = lrf_branch(*this, lrec, lcount, me, i);
    double c0 = 0.0, c1 = 0.0, miss = inf;
    if(R){
        lrf_point(*this, R, &c0, &c1);
        if(spherical) miss = rfn_dist(c0, c1, s0, s1, r_level[me[2]]);      // level me[2] < L <= GEOAC_MAX_LEVELS
        else { const double dx = s0 - c0, dy = s1 - c1; miss = sqrt(dx * dx + dy * dy); }
        if(!(miss == miss)) miss = inf;
    }
    S->me = me; S->s0 = s0; S->s1 = s1; S->c0 = c0; S->c1 = c1;
    return miss;
}

// Newton step from the base crossing point and the two probes' records (rays N + i and 2 * N + i); false: SINGULAR
__device__ inline bool LrfDev::newton(long long i, const Seed& S, double, double, const double* lrec, const int* lcount, double* d_th, double* d_ph) const {
    const double* Rt = lrf_branch(*this, lrec, lcount, S.me, n_seeds + i);
    const double* Rp = lrf_branch(*this, lrec, lcount, S.me, 2ll * n_seeds + i);
    if(!Rt || !Rp) return false;
    const double c0 = S.c0, c1 = S.c1, s0 = S.s0, s1 = S.s1;
    double ct0, ct1, cp0, cp1;
    lrf_point(*this, Rt, &ct0, &ct1);
    lrf_point(*this, Rp, &cp0, &cp1);
    const double e0 = s0 - c0, a00 = (ct0 - c0) / h, a01 = (cp0 - c0) / h;
    double e1, a10, a11;
    if(spherical){ e1 = wrap180(s1 - c1); a10 = wrap180(ct1 - c1) / h; a11 = wrap180(cp1 - c1) / h; }
    else { e1 = s1 - c1; a10 = (ct1 - c1) / h; a11 = (cp1 - c1) / h; }
    double det, dt, dp;
    solve(a00, a01, a10, a11, e0, e1, &det, &dt, &dp);
    if(!cut(det, &dt, &dp, step_max)) return false;
    *d_th = dt; *d_ph = dp;
    return true;
}

__global__ void k_lrf_step(const LrfDev* __restrict__ Dp, const double* __restrict__ lrec, const int* __restrict__ lcount, int round){
    rounds_step(*Dp, round, lrec, lcount);
}

__global__ void k_lrf_rows(const LrfDev* __restrict__ Dp, const double* __restrict__ lrec, const int* __restrict__ lcount){
    const LrfDev& D = *Dp;
    const long long N = D.n_seeds;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= N) return;                                           // i < N from here on
    const int* me = D.meta + LRF_META * i;
    double* row = D.rows + i * GEOAC_LRF_STRIDE;
    const int status = row_head(D, i, row, GEOAC_LRF_STATUS, GEOAC_LRF_ITER, GEOAC_LRF_THETA, GEOAC_LRF_PHI, GEOAC_LRF_MISS);
    row[GEOAC_LRF_MEMBER] = (double)me[0]; row[GEOAC_LRF_STATION] = (double)me[1]; row[GEOAC_LRF_LEG] = (double)me[3];
    row[GEOAC_LRF_DIR] = me[4] ? -1.0 : 1.0; row[GEOAC_LRF_ORD] = (double)me[5];
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

struct LrfState : RoundsState {
    LrfDev h{};                                           // host copy of the argument block (alive while its copy runs)
    LrfDev* args = nullptr;
    std::vector<double> h_src;
    size_t rows_bytes() const { return sizeof(double) * (size_t)n_seeds * GEOAC_LRF_STRIDE; }
};

const char* spec_fault(int eqset, const geoac_level_refine_spec* s, int* code){
    if(const char* fault = rounds_spec_fault(eqset, s, "not implemented for the 2-D set: it has neither level crossings nor level-station lists to refine (geoac_lstations.h)", code))
        return fault;
    if(!std::isfinite(s->probe_deg) || !(s->probe_deg > 0.0) || s->probe_deg > 1.0) return "probe_deg must be finite, > 0 and <= 1";
    return nullptr;
}

using Bound = RoundsBound<GeoacLrfView, LrfState>;

// a current result, or GEOAC_E_INVALID.  (geoac_set_levels does not move the invalidation counter: the crossing tables answer for it.)
int bind_result(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = rounds_bind(ctx, what, geoac_lrf_view, b);
    if(rc) return rc;
    if(!b->st || b->st->gen == 0 || b->st->gen != b->v.map.gen || geoac_fan_levels_dev(ctx, nullptr, nullptr, nullptr, nullptr) != GEOAC_OK)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no level refinement result, or a launch, new angles, an atmosphere upload, geoac_set_sources, "
                                                     "geoac_set_frequencies or geoac_set_levels have come since it (call geoac_fan_level_refine again)").c_str());
    return GEOAC_OK;
}

}  // namespace

extern "C" void geoac_lrf_release(void* state){ rounds_release<LrfState>(state); }

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
    int rc = rounds_bind(ctx, what, geoac_lrf_view, &b);
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
    const long long n_lists = (long long)M * n_sta;
    std::vector<unsigned> offs;
    long long n_seeds = 0;
    GEOAC_CHK(what, count_seeds(d_hits, n_lists, cap, M, 3, s, &offs, &n_seeds));
    if(n_seeds < 0)
        return geoac_map_fail(ctx, GEOAC_E_CAPACITY, ("fan_level_refine: more than " + std::to_string(GEOAC_RFN_MAX_RAY_MEMBERS) + " ray-members per round (3 rays x seeds x " + std::to_string(M) +
                                                      " members: every member integrates every seed and its two probes); refine fewer stations or members at a time").c_str());
    LrfState* st = b.begin(&offs, n_seeds);
    if(n_seeds == 0){ st->gen = b.v.map.gen; return GEOAC_OK; }       // (an empty result; nothing was launched, the lists stay)

    // one device block: args | offs | sta | level_of | src | meta | trial | best | state | active | rows
    const size_t N = (size_t)n_seeds;
    Carve carve;
    const size_t o_args = carve(sizeof(LrfDev)), o_offs = carve(sizeof(unsigned) * (size_t)n_lists), o_sta = carve(sizeof(double) * 2 * (size_t)n_sta),
                 o_lof = carve(sizeof(int) * (size_t)n_sta), o_src = carve(sizeof(double) * 2 * (size_t)M), o_meta = carve(sizeof(int) * LRF_META * N),
                 o_trial = carve(sizeof(double) * 6 * N), o_best = carve(sizeof(double) * 5 * N), o_state = carve(sizeof(int) * 3 * N), o_active = carve(sizeof(unsigned)),
                 o_rows = carve(sizeof(double) * GEOAC_LRF_STRIDE * N);
    if(grow(&st->buf, &st->buf_cap, carve.off)) return geoac_map_fail(ctx, GEOAC_E_NOMEM, "fan_level_refine: no device memory for the seeds");
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
    rc = run_rounds(b, what, D, 3, spec->max_iter, [&](int round, const GeoacMapView& v){
        if(int e = geoac_fan_levels_dev(ctx, &lrec, &lrec_bytes, &lcount, &lcount_bytes)) return e;
        if(v.M != M || v.n_rays != n_rays || lcount_bytes != sizeof(int) * n_rl || lrec_bytes != sizeof(double) * GEOAC_LVL_STRIDE * n_rl * capL)
            return geoac_map_fail(ctx, GEOAC_E_HIP, "fan_level_refine: the round's crossing tables do not have the shape of the seeds ([M][3 * n_seeds][L][cap])");
        hipLaunchKernelGGL(k_lrf_step, dim3(n_blk), dim3(64), 0, s, (const LrfDev*)st->args, (const double*)lrec, (const int*)lcount, round);
        return (int)GEOAC_OK;
    });
    if(rc) return rc;
    return finish_rounds(b, what, D, [&]{ hipLaunchKernelGGL(k_lrf_rows, dim3(n_blk), dim3(64), 0, s, (const LrfDev*)st->args, (const double*)lrec, (const int*)lcount); });
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
    return rc ? rc : rounds_timing(ctx, "fan_level_refine_timing", *b.st, ms);
}

extern "C" int geoac_fan_level_refine_stats(geoac_ctx* ctx, uint64_t stats[6]){
    Bound b;
    int rc = bind_result(ctx, "fan_level_refine_stats", &b);
    return rc ? rc : rounds_stats(ctx, "fan_level_refine_stats", *b.st, stats);
}

// (geoac_level_refine_int.h: for geoac_level_amp.hip)
extern "C" int geoac_lrf_seeds(geoac_ctx* ctx, const char* what, GeoacLrfSeeds* out){
    Bound b;
    int rc = bind_result(ctx, what, &b);
    if(rc) return rc;
    const LrfDev& D = b.st->h;
    const long long N = b.st->n_seeds;
    *out = GeoacLrfSeeds{};
    out->n_seeds = b.st->n_seeds;
    if(N == 0) return GEOAC_OK;                                   // (no block was carved: h is the last call's)
    out->M = D.M; out->L = D.L; out->capL = D.capL; out->probe_deg = D.h;
    out->meta = D.meta; out->status = D.state; out->theta = D.best; out->phi = D.best + N;
    return GEOAC_OK;
}
