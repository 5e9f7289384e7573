// geoac_newton_rounds.h - the Newton rounds that geoac_refine.hip (station refinement) and geoac_level_refine.hip (level refinement) share: the
// dense seed list of the (member, station) lists, a round's fan of RAYS rays per seed through geoac_fan_set_angles and geoac_fan_launch, and the
// step rule of include/geoac_refine.h applied to every seed after each launch.  The caller derives its kernel argument block from RoundsDev and
// gives it a constant, a type (Seed) and three members, and nothing else - its miss, its Jacobian, its row tail, its view, its state's own
// fields, its entry points and its messages stay its own:
//   RAYS                                        rays per seed: trial is [2][RAYS * n_seeds], theta | phi, the seeds' own rays first
//   double miss(i, tables..., Seed*)            the miss of seed i's own ray in the round's tables, inf for "no record" and for NaN; Seed, the
//                                               caller's own type, is what it leaves for newton (the seed's record, its station)
//   bool newton(i, const Seed&, th, ph, tables..., &d_th, &d_ph)       the Newton step, through solve and cut below; false: SINGULAR
//   void set_trial(i, th, ph)                   the rays of seed i in the next launch
//
// The arithmetic is restated in tests/refine_reference.py (step_rule): contraction is off from here on.  Index bounds stand at each load and store.
#ifndef GEOAC_NEWTON_ROUNDS_H_
#define GEOAC_NEWTON_ROUNDS_H_

#include <cmath>
#include <vector>

#include "../../include/geoac_refine.h"
#include "geoac_launch_int.h"
#include "geoac_rfn_series.h"

#pragma clang fp contract(off)

namespace {

struct RoundsDev {
    const unsigned* hits;                         // [n_lists]: the lists' hit counts (read by the seed kernel only)
    const unsigned* offs;                         // [n_lists]: seeds before the list
    const double* sta;                            // [n_sta][2]: a copy of this call's own
    double* trial;                                // [2][RAYS * n_seeds]: theta | phi of the next launch
    double* best;                                 // [5][n_seeds]: b_th | b_ph | b_miss | d_th | d_ph
    int* state;                                   // [3][n_seeds]: status (0: active) | shrink counter | rounds used
    unsigned* active;
    double tol, step_max;
    int spherical, max_shrink;
    int M, n_sta, cap, n_seeds;
    long long n_lists;
};

// row k < cap of list < n_lists = M * n_sta: its seed index i < n_seeds, or -1 when the list keeps no such row (k >= min(hits, cap))
__device__ inline long long seed_slot(const RoundsDev& D, long long list, unsigned k){
    const unsigned h = D.hits[list];
    if(k >= (h < (unsigned)D.cap ? h : (unsigned)D.cap)) return -1;
    return (long long)D.offs[list] + k;                      // < n_seeds: offs are the prefix counts of exactly these minima (count_seeds)
}
// a seed before its first round: nothing accepted yet
__device__ inline void seed_init(const RoundsDev& D, long long i){
    const long long N = D.n_seeds;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    D.best[i] = 0.0; D.best[N + i] = 0.0; D.best[2 * N + i] = inf; D.best[3 * N + i] = 0.0; D.best[4 * N + i] = 0.0;
    D.state[i] = 0; D.state[N + i] = 0; D.state[2 * N + i] = 0;
}
// the 2 x 2 system a * (dt, dp) = e, then the test and cut of its solution; false: SINGULAR.  (The ground rule scales between the two.)
__device__ inline void solve(double a00, double a01, double a10, double a11, double e0, double e1, double* det, double* dt, double* dp){
    *det = a00 * a11 - a01 * a10;
    *dt = (a11 * e0 - a01 * e1) / *det;
    *dp = (a00 * e1 - a10 * e0) / *det;
}
__device__ inline bool cut(double det, double* dt, double* dp, double step_max){
    if(det == 0.0 || !rfn_finite(det) || !rfn_finite(*dt) || !rfn_finite(*dp)) return false;
    if(*dt > step_max) *dt = step_max;
    if(*dt < -step_max) *dt = -step_max;
    if(*dp > step_max) *dp = step_max;
    if(*dp < -step_max) *dp = -step_max;
    return true;
}
// one thread per seed, after a round's launch: miss, accept / reject, Newton step, next trial; counts the seeds still active
template<class Dev, class... Tab>
__device__ inline void rounds_step(const Dev& D, int round, Tab... tab){
    const long long N = D.n_seeds;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= N || D.state[i] != 0) return;                    // i < N from here on
    const double th = D.trial[i], ph = D.trial[Dev::RAYS * N + i];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    typename Dev::Seed S;
    const double miss = D.miss(i, tab..., &S);
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
        // (miss < inf here unless round == 1, and then miss == inf was LOST: the trial ray holds its record)
        if(!D.newton(i, S, th, ph, tab..., &d_th, &d_ph)) status = GEOAC_RFN_SINGULAR;
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
        D.set_trial(i, D.best[i] + D.best[3 * N + i], D.best[N + i] + D.best[4 * N + i]);
        atomicAdd(D.active, 1u);
    } else D.set_trial(i, D.best[i], D.best[N + i]);
}

// the head of seed i's finished row, at the caller's columns: a seed still active ends as ITER_LIMIT.  Returns the status.
__device__ inline int row_head(const RoundsDev& D, long long i, double* row, int c_status, int c_iter, int c_theta, int c_phi, int c_miss){
    const long long N = D.n_seeds;
    int status = D.state[i];
    if(status == 0){ status = GEOAC_RFN_ITER_LIMIT; D.state[i] = status; }
    row[c_status] = (double)status; row[c_iter] = (double)D.state[2 * N + i];
    row[c_theta] = D.best[i]; row[c_phi] = D.best[N + i];
    row[c_miss] = status == GEOAC_RFN_LOST ? -1.0 : D.best[2 * N + i];
    return status;
}

// host half: what both callers keep for a result, and the steps of a call that they do alike
struct RoundsState {
    void* buf = nullptr; size_t buf_cap = 0;              // every device array of a call, carved by the caller
    std::vector<unsigned> h_offs;
    std::vector<double> h_trial;
    unsigned long long gen = 0;                           // the context's invalidation counter the result was made at (0: none)
    GeoacMapView last{};                                  // the view of the last round's launch
    int n_seeds = 0, launches = 0;
    double ms_launch = 0.0, ms_kernels = 0.0;
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    EventPair ev;
    // a call begins: no current result until this one is complete
    void begin(std::vector<unsigned>* offs, long long n){
        gen = 0; h_offs.swap(*offs);
        n_seeds = (int)n; launches = 0; ms_launch = 0.0; ms_kernels = 0.0;
        for(int k = 0; k < 6; k++) stats[k] = 0;
        stats[2] = (uint64_t)n;
    }
};

// an entry point's context, the caller's view of it with the state's slot, and the state in the slot (NULL until a call has created it)
template<class View, class State>
struct RoundsBound {
    geoac_ctx* ctx; View v; State* st;
    // a call begins: the state is created only now, when nothing can refuse the call any more (a refused call allocates nothing)
    State* begin(std::vector<unsigned>* offs, long long n){
        if(!*v.state) *v.state = new State();
        st = (State*)*v.state;
        st->begin(offs, n);
        return st;
    }
};
// (not bind_launch: the callers have their own messages for a context without current lists)
template<class View, class State>
int rounds_bind(geoac_ctx* ctx, const char* what, int (*view)(geoac_ctx*, View*), RoundsBound<View, State>* b){
    if(!ctx) return GEOAC_E_INVALID;
    b->ctx = ctx;
    int rc = view(ctx, &b->v);
    if(rc) return rc;
    b->st = (State*)*b->v.state;
    if(hipSetDevice(b->v.map.device) != hipSuccess) return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": hipSetDevice failed").c_str());
    return GEOAC_OK;
}
template<class State>
void rounds_release(void* state){
    State* st = (State*)state;
    if(!st) return;
    if(st->buf) hipFree(st->buf);
    st->ev.release();
    delete st;
}
// the arrays of one device block, each at a multiple of 256 bytes: carve(n) is the offset of the next n bytes, off the block's size
struct Carve {
    size_t off = 0;
    size_t operator()(size_t n){ const size_t at = off; off += (n + 255) / 256 * 256; return at; }
};

// the checks that both specs share, in the callers' order; no_2d is the caller's own refusal of the 2-D set.  NULL: none failed
template<class Spec>
const char* rounds_spec_fault(int eqset, const Spec* s, const char* no_2d, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){ *code = GEOAC_E_UNSUPPORTED; return no_2d; }
    if(!s) return "spec is NULL";
    if(s->max_iter < 1 || s->max_iter > GEOAC_RFN_MAX_ITER) return "max_iter must be in 1 .. 32";
    if(s->max_shrink < 0 || s->max_shrink > GEOAC_RFN_MAX_SHRINK) return "max_shrink must be in 0 .. 16";
    if(!std::isfinite(s->tol) || !(s->tol > 0.0)) return "tol must be finite and > 0";
    if(!std::isfinite(s->step_max_deg) || !(s->step_max_deg > 0.0)) return "step_max_deg must be finite and > 0";
    return nullptr;
}
// seeds before every list: integer prefix counts of min(hits, cap), on the host.  *n_seeds < 0: more than GEOAC_RFN_MAX_RAY_MEMBERS
// ray-members per round (rays_per_seed x seeds x M); the refusal's message is the caller's.
hipError_t count_seeds(const void* d_hits, long long n_lists, int cap, int M, int rays_per_seed, hipStream_t s, std::vector<unsigned>* offs, long long* n_seeds){
    std::vector<unsigned> hits((size_t)n_lists);
    hipError_t e = hipMemcpyAsync(hits.data(), d_hits, sizeof(unsigned) * (size_t)n_lists, hipMemcpyDeviceToHost, s);
    if(e == hipSuccess) e = hipStreamSynchronize(s);
    if(e != hipSuccess) return e;
    offs->resize((size_t)n_lists);
    long long n = 0;
    for(long long l = 0; l < n_lists && n >= 0; l++){
        (*offs)[(size_t)l] = (unsigned)n;
        n += hits[(size_t)l] < (unsigned)cap ? hits[(size_t)l] : (unsigned)cap;
        if(rays_per_seed * n * M > GEOAC_RFN_MAX_RAY_MEMBERS) n = -1;
    }
    *n_seeds = n;
    return hipSuccess;
}
// the rounds, behind the seed kernel: while seeds are active and rounds are left, the trial angles to the host, one fan of rays_per_seed *
// n_seeds rays, and step(round, view): the caller's check of the launch's tables against the seeds' shape (a status ends the call) and its kernel
template<class Bound, class Step>
int run_rounds(const Bound& b, const char* what, const RoundsDev& D, int rays_per_seed, int max_iter, Step step){
    RoundsState* st = b.st;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    const int n_rays = rays_per_seed * D.n_seeds;
    int rc = GEOAC_OK;
    unsigned active = 1;
    st->h_trial.resize(2 * (size_t)n_rays);
    for(int round = 1; round <= max_iter && active > 0; round++){
        // (16 bytes per ray.  The sync also ends the seed kernel's reads of the lists, which the launch invalidates.)
        GEOAC_CHK(what, hipMemcpyAsync(st->h_trial.data(), D.trial, sizeof(double) * 2 * (size_t)n_rays, hipMemcpyDeviceToHost, s));
        GEOAC_CHK(what, hipStreamSynchronize(s));
        if((rc = geoac_fan_set_angles(b.ctx, n_rays, st->h_trial.data(), st->h_trial.data() + n_rays))) return rc;
        if((rc = geoac_fan_launch(b.ctx))) return rc;
        st->launches = round;
        st->stats[0] = (uint64_t)round; st->stats[1] += (uint64_t)n_rays * (uint64_t)D.M;
        double ms3[3] = {0, 0, 0}; uint64_t st3[3] = {0, 0, 0};
        if(geoac_last_timing(b.ctx, ms3, st3) == GEOAC_OK) st->ms_launch += ms3[0];
        if((rc = geoac_map_view(b.ctx, &st->last))) return rc;
        GEOAC_CHK(what, st->ev.start(s));
        GEOAC_CHK(what, hipMemsetAsync(D.active, 0, sizeof(unsigned), s));
        if((rc = step(round, st->last))) return rc;
        GEOAC_CHK(what, hipGetLastError());
        GEOAC_CHK(what, st->ev.stop(s));
        GEOAC_CHK(what, hipMemcpyAsync(&active, D.active, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        GEOAC_CHK(what, hipStreamSynchronize(s));
        double t = 0; GEOAC_CHK(what, st->ev.ms(&t));
        st->ms_kernels += t;
    }
    return GEOAC_OK;
}

// after the last round: rows() launches the caller's rows kernel; the statuses into stats[3 .. 5]; the result is current, at the last round's counter
template<class Bound, class Rows>
int finish_rounds(const Bound& b, const char* what, const RoundsDev& D, Rows rows){
    RoundsState* st = b.st;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, st->ev.start(s));
    rows();
    GEOAC_CHK(what, hipGetLastError());
    GEOAC_CHK(what, st->ev.stop(s));
    std::vector<int> status((size_t)D.n_seeds);
    GEOAC_CHK(what, hipMemcpyAsync(status.data(), D.state, sizeof(int) * status.size(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    double t = 0; GEOAC_CHK(what, st->ev.ms(&t));
    st->ms_kernels += t;
    for(const int c : status)
        st->stats[c == GEOAC_RFN_CONVERGED ? 3 : (c == GEOAC_RFN_STALLED || c == GEOAC_RFN_ITER_LIMIT ? 4 : 5)]++;
    st->gen = st->last.gen;
    return GEOAC_OK;
}

// the bodies of *_timing and *_stats behind the caller's bind_result
int rounds_timing(geoac_ctx* ctx, const char* what, const RoundsState& st, double ms[2]){
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": NULL argument").c_str());
    ms[0] = st.ms_launch; ms[1] = st.ms_kernels;
    return GEOAC_OK;
}
int rounds_stats(geoac_ctx* ctx, const char* what, const RoundsState& st, uint64_t stats[6]){
    if(!stats) return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": NULL argument").c_str());
    for(int k = 0; k < 6; k++) stats[k] = st.stats[k];
    return GEOAC_OK;
}

}  // namespace

#endif
