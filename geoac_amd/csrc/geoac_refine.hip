// geoac_refine.hip - station refinement (include/geoac_refine.h): Newton eigenrays for every estimate of the station lists.
//
// A round is one fan of all seeds through the existing launch path (geoac_fan_set_angles, geoac_fan_launch: nothing of the launch plan is
// touched or known here) and one kernel that applies the header's step rule to every seed from its own member's record.  Every member
// integrates every seed; a seed reads one member's record, the other M - 1 are discarded (header, "Cost").
//
// Three kernels:
//   k_rfn_seed   one thread per (list, row): the kept rows of the station lists become the dense seed list, each at its list's prefix count
//                plus its place in the list - list order, no atomics.  The prefix counts are integers summed on the host from hits[M][n_sta].
//   k_rfn_step   one thread per seed, after a round's launch: miss, accept / reject, Newton step, next trial; counts the seeds still active
//                (the one integer the host reads per round, as the epoch loop reads its live count).
//   k_rfn_rows   one thread per seed, after the last launch: the row and the seed's levels.
// The kernels' arguments live in a block of device memory (RfnDev): passed by value they would sit in scalar registers beside the loop state.
//
// The arithmetic is fixed by the header and restated in tests/refine_reference.py, elementary functions included (geoac_rfn_series.h, which
// geoac_level_refine.hip includes too): every product is rounded before it is added, so this file is compiled with contraction off (the pragma
// below; the Makefile gives the same flag).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/geoac_refine.h"
#include "geoac_launch_int.h"
#include "geoac_stations_int.h"
#include "geoac_refine_int.h"
#include "geoac_tri_rule.h"
#include "geoac_rfn_series.h"

#pragma clang fp contract(off)

namespace {

struct RfnDev {
    const double* sta_rows; const unsigned* hits; // the station lists (read by k_rfn_seed only)
    const unsigned* offs;                         // [n_lists]: seeds before the list
    const double* sta; const double* mem;         // [n_sta][2], [M][GEOAC_RFN_MEMW]: copies of this call's own
    int* meta;                                    // [n_seeds][4]: member, station, leg, triangle
    double* trial;                                // [2][n_seeds]: theta | phi of the next launch
    double* best;                                 // [5][n_seeds]: b_th | b_ph | b_miss | d_th | d_ph
    int* state;                                   // [3][n_seeds]: status (0: active) | shrink counter | rounds used
    unsigned* active;
    double* rows; double* lvl;
    double tol, step_max, rg, r_earth;
    int eqset, spherical, max_shrink;
    int M, F, n_sta, cap, n_seeds, legs;
    long long n_lists;
};

__global__ void k_rfn_seed(const RfnDev* __restrict__ Dp){
    const RfnDev& D = *Dp;
    const long long n = D.n_lists * D.cap;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for(long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride){
        const long long list = t / D.cap;
        const unsigned k = (unsigned)(t % D.cap);
        const unsigned h = D.hits[list];
        if(k >= (h < (unsigned)D.cap ? h : (unsigned)D.cap)) continue;
        const long long i = (long long)D.offs[list] + k;
        const double* row = D.sta_rows + t * GEOAC_STA_STRIDE;
        int* me = D.meta + 4 * i;
        me[0] = (int)(list / D.n_sta); me[1] = (int)(list % D.n_sta); me[2] = (int)row[GEOAC_STA_LEG]; me[3] = (int)row[GEOAC_STA_TRI];
        const long long N = D.n_seeds;
        D.trial[i] = row[GEOAC_STA_THETA]; D.trial[N + i] = row[GEOAC_STA_PHI];
        D.best[i] = 0.0; D.best[N + i] = 0.0; D.best[2 * N + i] = inf; D.best[3 * N + i] = 0.0; D.best[4 * N + i] = 0.0;
        D.state[i] = 0; D.state[N + i] = 0; D.state[2 * N + i] = 0;
    }
}

// miss of a record on the seed's leg (header, "The record")
__device__ inline double rfn_miss(const RfnDev& D, const double* R, double s0, double s1){
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    if(R[GEOAC_REC_VALID] == 0.0) return inf;
    const double* S = R + GEOAC_REC_STATE;
    double miss;
    if(D.spherical) miss = rfn_dist(S[1] * 180.0 / kRfnPi, S[2] * 180.0 / kRfnPi, s0, s1, D.rg);
    else { const double dx = s0 - S[0], dy = s1 - S[1]; miss = sqrt(dx * dx + dy * dy); }
    return miss == miss ? miss : inf;
}

// Newton step of a record in launch angles; false: SINGULAR
__device__ inline bool rfn_newton(const RfnDev& D, const double* R, double s0, double s1, double th, double ph, const double* mem, double* d_th, double* d_ph){
    const double* S = R + GEOAC_REC_STATE;
    double e0, e1, a00, a01, a10, a11;
    if(D.spherical){
        e0 = s0 * kRfnPi / 180.0 - S[1];
        e1 = wrap180(s1 - S[2] * 180.0 / kRfnPi) * kRfnPi / 180.0;
        const double q = 1.0 / D.rg, qc = 1.0 / (D.rg * rfn_cos(S[1]));
        a00 = S[7] - ((q * S[4]) / S[3]) * S[6];    a01 = S[13] - ((q * S[4]) / S[3]) * S[12];
        a10 = S[8] - ((qc * S[5]) / S[3]) * S[6];   a11 = S[14] - ((qc * S[5]) / S[3]) * S[12];
    } else if(D.eqset == GEOAC_EQ_3D){
        e0 = s0 - S[0]; e1 = s1 - S[1];
        double st, ct, sp, cp;
        rfn_sincosd(th, &st, &ct);
        rfn_sincosd(90.0 - ph, &sp, &cp);
        const double n0 = ct * cp, n1 = ct * sp;
        const double m = 1.0 + (n0 * mem[2] + n1 * mem[3]);
        const double g0 = (n0 / m) / S[3], g1 = (n1 / m) / S[3];
        a00 = S[4] - g0 * S[6];  a01 = S[8] - g0 * S[10];  a10 = S[5] - g1 * S[6];  a11 = S[9] - g1 * S[10];
    } else {
        e0 = s0 - S[0]; e1 = s1 - S[1];
        const double g0 = S[3] / S[5], g1 = S[4] / S[5];
        a00 = S[6] - g0 * S[8];  a01 = S[12] - g0 * S[14];  a10 = S[7] - g1 * S[8];  a11 = S[13] - g1 * S[14];
    }
    const double det = a00 * a11 - a01 * a10;
    double dlt = (((a11 * e0 - a01 * e1) / det) * 180.0) / kRfnPi;
    double dlp = (((a00 * e1 - a10 * e0) / det) * 180.0) / kRfnPi;
    if(det == 0.0 || !rfn_finite(det) || !rfn_finite(dlt) || !rfn_finite(dlp)) return false;
    if(dlt > D.step_max) dlt = D.step_max;
    if(dlt < -D.step_max) dlt = -D.step_max;
    if(dlp > D.step_max) dlp = D.step_max;
    if(dlp < -D.step_max) dlp = -D.step_max;
    *d_th = dlt; *d_ph = -dlp;
    return true;
}

__global__ void k_rfn_step(const RfnDev* __restrict__ Dp, const double* __restrict__ rec, int round){
    const RfnDev& D = *Dp;
    const long long N = D.n_seeds;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= N || D.state[i] != 0) return;
    const int* me = D.meta + 4 * i;
    const int m = me[0], leg = me[2];
    const double s0 = D.sta[2 * me[1]], s1 = D.sta[2 * me[1] + 1];
    const double* R = rec + (((long long)m * N + i) * D.legs + leg) * GEOAC_REC_STRIDE;
    const double th = D.trial[i], ph = D.trial[N + i];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double miss = rfn_miss(D, R, s0, s1);
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
        if(!rfn_newton(D, R, s0, s1, th, ph, D.mem + (long long)m * GEOAC_RFN_MEMW, &d_th, &d_ph)) status = GEOAC_RFN_SINGULAR;
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
        D.trial[i] = D.best[i] + D.best[3 * N + i];
        D.trial[N + i] = D.best[N + i] + D.best[4 * N + i];
        atomicAdd(D.active, 1u);
    } else {
        D.trial[i] = D.best[i];
        D.trial[N + i] = D.best[N + i];
    }
}

__global__ void k_rfn_rows(const RfnDev* __restrict__ Dp, const double* __restrict__ rec, const double* __restrict__ level){
    const RfnDev& D = *Dp;
    const long long N = D.n_seeds;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= N) return;
    const int* me = D.meta + 4 * i;
    const int m = me[0], leg = me[2];
    int status = D.state[i];
    if(status == 0){ status = GEOAC_RFN_ITER_LIMIT; D.state[i] = status; }
    double* row = D.rows + i * GEOAC_RFN_STRIDE;
    row[GEOAC_RFN_MEMBER] = (double)m; row[GEOAC_RFN_STATION] = (double)me[1]; row[GEOAC_RFN_LEG] = (double)leg; row[GEOAC_RFN_TRI] = (double)me[3];
    row[GEOAC_RFN_STATUS] = (double)status; row[GEOAC_RFN_ITER] = (double)D.state[2 * N + i];
    row[GEOAC_RFN_THETA] = D.best[i]; row[GEOAC_RFN_PHI] = D.best[N + i];
    row[GEOAC_RFN_MISS] = status == GEOAC_RFN_LOST ? -1.0 : D.best[2 * N + i];
    const bool conv = status == GEOAC_RFN_CONVERGED;
    double tt = 0.0, cel = 0.0, turn = 0.0, incl = 0.0, baz = 0.0, amp = 0.0, jac = 0.0;
    if(conv){
        const double* R = rec + (((long long)m * N + i) * D.legs + leg) * GEOAC_REC_STRIDE;
        const double s0 = D.sta[2 * me[1]], s1 = D.sta[2 * me[1] + 1];
        const double* mem = D.mem + (long long)m * GEOAC_RFN_MEMW;
        const double range = D.spherical ? rfn_dist(mem[0], mem[1], s0, s1, D.r_earth) : sqrt(s0 * s0 + s1 * s1);
        tt = R[GEOAC_REC_TTIME]; cel = range / tt; turn = R[GEOAC_REC_TURN]; incl = R[GEOAC_REC_INCL]; baz = R[GEOAC_REC_BACKAZ];
        amp = R[GEOAC_REC_AMP]; jac = R[GEOAC_REC_JACOB];
    }
    row[GEOAC_RFN_TTIME] = tt; row[GEOAC_RFN_CELERITY] = cel; row[GEOAC_RFN_TURN] = turn; row[GEOAC_RFN_INCL] = incl; row[GEOAC_RFN_BACKAZ] = baz;
    row[GEOAC_RFN_AMP] = amp; row[GEOAC_RFN_JACOB] = jac;
    for(int f = 0; f < D.F; f++)
        D.lvl[i * D.F + f] = conv ? level[(((long long)m * D.F + f) * N + i) * D.legs + leg] : 0.0;
}

struct RfnState {
    void* buf = nullptr; size_t buf_cap = 0;              // every device array of a call, carved below
    RfnDev h{};                                           // host copy of the argument block (alive while its copy runs)
    RfnDev* args = nullptr;
    std::vector<unsigned> h_offs;
    std::vector<double> h_mem, h_trial;
    unsigned long long gen = 0;                           // the context's invalidation counter the result was made at (0: none)
    int n_seeds = 0, F = 0, launches = 0;
    double ms_launch = 0.0, ms_kernels = 0.0;
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    EventPair ev;
    size_t rows_bytes() const { return sizeof(double) * (size_t)n_seeds * GEOAC_RFN_STRIDE; }
    size_t level_bytes() const { return sizeof(double) * (size_t)n_seeds * F; }
};

const char* spec_fault(int eqset, const geoac_refine_spec* s, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){
        *code = GEOAC_E_UNSUPPORTED;
        return "not implemented for the 2-D set: it has no station lists to refine (geoac_stations.h)";
    }
    if(!s) return "spec is NULL";
    if(s->max_iter < 1 || s->max_iter > GEOAC_RFN_MAX_ITER) return "max_iter must be in 1 .. 32";
    if(s->max_shrink < 0 || s->max_shrink > GEOAC_RFN_MAX_SHRINK) return "max_shrink must be in 0 .. 16";
    if(!std::isfinite(s->tol) || !(s->tol > 0.0)) return "tol must be finite and > 0";
    if(!std::isfinite(s->step_max_deg) || !(s->step_max_deg > 0.0)) return "step_max_deg must be finite and > 0";
    return nullptr;
}

struct Bound { geoac_ctx* ctx; GeoacRfnView v; RfnState* st; };

// (not bind_launch: geoac_fan_refine has its own message for a context without a current launch, and the fetches ask for a current result)
int bind(geoac_ctx* ctx, const char* what, bool create, Bound* b){
    if(!ctx) return GEOAC_E_INVALID;
    b->ctx = ctx;
    int rc = geoac_rfn_view(ctx, &b->v);
    if(rc) return rc;
    if(!*b->v.state && create) *b->v.state = new RfnState();
    b->st = (RfnState*)*b->v.state;
    if(hipSetDevice(b->v.map.device) != hipSuccess) return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": hipSetDevice failed").c_str());
    return GEOAC_OK;
}

// a current result, or GEOAC_E_INVALID
int bind_result(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = bind(ctx, what, false, b);
    if(rc) return rc;
    if(!b->st || b->st->gen == 0 || b->st->gen != b->v.map.gen)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no refinement result, or a launch, new angles, an atmosphere upload, geoac_set_sources or "
                                                     "geoac_set_frequencies have come since it (call geoac_fan_refine again)").c_str());
    return GEOAC_OK;
}

size_t up256(size_t n){ return (n + 255) / 256 * 256; }

}  // namespace

extern "C" void geoac_rfn_release(void* state){
    RfnState* st = (RfnState*)state;
    if(!st) return;
    if(st->buf) hipFree(st->buf);
    st->ev.release();
    delete st;
}

extern "C" const char* geoac_refine_fault(int eqset, const geoac_refine_spec* spec){
    int code;
    return spec_fault(eqset, spec, &code);
}

extern "C" int geoac_refine_check(int eqset, const geoac_refine_spec* spec){
    int code;
    return spec_fault(eqset, spec, &code) ? code : GEOAC_OK;
}

extern "C" int geoac_fan_refine(geoac_ctx* ctx, const geoac_refine_spec* spec){
    const char* what = "fan_refine";
    Bound b;
    int rc = bind(ctx, what, true, &b);
    if(rc) return rc;
    int code;
    if(const char* fault = spec_fault(b.v.map.eqset, spec, &code)) return geoac_map_fail(ctx, code, (std::string("fan_refine: ") + fault).c_str());
    int M = 0, F = 0, n_sta = 0, cap = 0;
    if(!b.v.map.fresh || geoac_fan_stations_shape(ctx, &M, &F, &n_sta, &cap) != GEOAC_OK)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_refine: no station lists of the last completed launch (call geoac_fan_stations after geoac_fan_launch; a launch, new angles, "
                                                    "an atmosphere upload, geoac_set_sources and geoac_set_frequencies invalidate them)");
    if(!b.v.map.calc_amp || !b.v.calc_amp)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_refine: needs calc_amp = 1, for the lattice launch and now (the Newton step reads the launch-angle derivatives of the landing state)");
    if(b.v.mode & (GEOAC_MODE_WRITE_RAYS | GEOAC_MODE_WRITE_CAUSTICS))
        return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_refine: not available with sample capture (WriteRays / WriteCaustics)");
    if(M != b.v.n_members) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_refine: the members of the context are not those of the station lists");
    RfnState* st = b.st;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    void* d_hits = nullptr; void* d_rows = nullptr; const double* d_sta = nullptr; size_t bytes = 0;
    if((rc = geoac_fan_stations_dev(ctx, 0, &d_hits, &bytes)) || (rc = geoac_fan_stations_dev(ctx, 1, &d_rows, &bytes)) || (rc = geoac_sta_coords_dev(ctx, &d_sta, nullptr))) return rc;
    // seeds before every list: integer prefix counts of min(hits, cap), on the host
    const long long n_lists = (long long)M * n_sta;
    std::vector<unsigned> hits((size_t)n_lists);
    GEOAC_CHK(what, hipMemcpyAsync(hits.data(), d_hits, sizeof(unsigned) * (size_t)n_lists, hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    st->h_offs.resize((size_t)n_lists);
    long long n_seeds = 0;
    for(long long l = 0; l < n_lists; l++){
        st->h_offs[(size_t)l] = (unsigned)n_seeds;
        n_seeds += hits[(size_t)l] < (unsigned)cap ? hits[(size_t)l] : (unsigned)cap;
        if(n_seeds * M > GEOAC_RFN_MAX_RAY_MEMBERS)
            return geoac_map_fail(ctx, GEOAC_E_CAPACITY, ("fan_refine: more than " + std::to_string(GEOAC_RFN_MAX_RAY_MEMBERS) + " ray-members per round (seeds x " + std::to_string(M) +
                                                          " members: every member integrates every seed); refine fewer stations or members at a time").c_str());
    }
    st->gen = 0;                                       // (no current result until this one is complete)
    const size_t N = (size_t)n_seeds;
    st->n_seeds = (int)n_seeds; st->F = F; st->launches = 0; st->ms_launch = 0.0; st->ms_kernels = 0.0;
    for(int k = 0; k < 6; k++) st->stats[k] = 0;
    st->stats[2] = (uint64_t)n_seeds;
    if(n_seeds == 0){ st->gen = b.v.map.gen; return GEOAC_OK; }       // (an empty result; nothing was launched, the lists stay)

    // one device block: args | offs | sta | mem | meta | trial | best | state | active | rows | level
    size_t off = 0;
    auto carve = [&](size_t n){ const size_t at = off; off += up256(n); return at; };
    const size_t o_args = carve(sizeof(RfnDev)), o_offs = carve(sizeof(unsigned) * (size_t)n_lists), o_sta = carve(sizeof(double) * 2 * (size_t)n_sta),
                 o_mem = carve(sizeof(double) * GEOAC_RFN_MEMW * (size_t)M), o_meta = carve(sizeof(int) * 4 * N), o_trial = carve(sizeof(double) * 2 * N),
                 o_best = carve(sizeof(double) * 5 * N), o_state = carve(sizeof(int) * 3 * N), o_active = carve(sizeof(unsigned)),
                 o_rows = carve(sizeof(double) * GEOAC_RFN_STRIDE * N), o_level = carve(sizeof(double) * (size_t)F * N);
    if(grow(&st->buf, &st->buf_cap, off)) return geoac_map_fail(ctx, GEOAC_E_NOMEM, "fan_refine: no device memory for the seeds");
    char* base = (char*)st->buf;
    st->args = (RfnDev*)(base + o_args);
    RfnDev& D = st->h;
    D = RfnDev{};
    D.sta_rows = (const double*)d_rows; D.hits = (const unsigned*)d_hits; D.offs = (const unsigned*)(base + o_offs);
    D.sta = (const double*)(base + o_sta); D.mem = (const double*)(base + o_mem);
    D.meta = (int*)(base + o_meta); D.trial = (double*)(base + o_trial); D.best = (double*)(base + o_best); D.state = (int*)(base + o_state);
    D.active = (unsigned*)(base + o_active); D.rows = (double*)(base + o_rows); D.lvl = (double*)(base + o_level);
    D.tol = spec->tol; D.step_max = spec->step_max_deg; D.rg = b.v.r_earth + b.v.z_grnd; D.r_earth = b.v.r_earth;
    D.eqset = b.v.map.eqset; D.spherical = spherical(b.v.map.eqset) ? 1 : 0; D.max_shrink = spec->max_shrink;
    D.M = M; D.F = F; D.n_sta = n_sta; D.cap = cap; D.n_seeds = (int)n_seeds; D.legs = b.v.map.legs; D.n_lists = n_lists;
    st->h_mem.assign(b.v.mem, b.v.mem + (size_t)M * GEOAC_RFN_MEMW);
    st->h_trial.resize(2 * N);
    GEOAC_CHK(what, hipMemcpyAsync(st->args, &D, sizeof(RfnDev), hipMemcpyHostToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_offs, st->h_offs.data(), sizeof(unsigned) * (size_t)n_lists, hipMemcpyHostToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_sta, d_sta, sizeof(double) * 2 * (size_t)n_sta, hipMemcpyDeviceToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_mem, st->h_mem.data(), sizeof(double) * st->h_mem.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rfn_seed, dim3(blocks_for(n_lists * cap, 256)), dim3(256), 0, s, (const RfnDev*)st->args);
    GEOAC_CHK(what, hipGetLastError());

    const unsigned n_blk = blocks_for(n_seeds, 64);
    GeoacMapView mv{};
    unsigned active = 1;
    for(int round = 1; round <= spec->max_iter && active > 0; round++){
        // the trial angles: device -> host -> geoac_fan_set_angles (16 bytes per seed)
        GEOAC_CHK(what, hipMemcpyAsync(st->h_trial.data(), D.trial, sizeof(double) * 2 * N, hipMemcpyDeviceToHost, s));
        GEOAC_CHK(what, hipStreamSynchronize(s));
        if((rc = geoac_fan_set_angles(ctx, (int)n_seeds, st->h_trial.data(), st->h_trial.data() + N))) return rc;
        if((rc = geoac_fan_launch(ctx))) return rc;
        st->launches = round;
        st->stats[0] = (uint64_t)round; st->stats[1] += (uint64_t)n_seeds * (uint64_t)M;
        double ms3[3] = {0, 0, 0}; uint64_t st3[3] = {0, 0, 0};
        if(geoac_last_timing(ctx, ms3, st3) == GEOAC_OK) st->ms_launch += ms3[0];
        if((rc = geoac_map_view(ctx, &mv))) return rc;
        if(mv.M != M || mv.n_rays != (int)n_seeds || mv.legs != D.legs) return geoac_map_fail(ctx, GEOAC_E_HIP, "fan_refine: the round's launch does not have the shape of the seeds");
        GEOAC_CHK(what, st->ev.start(s));
        GEOAC_CHK(what, hipMemsetAsync(D.active, 0, sizeof(unsigned), s));
        hipLaunchKernelGGL(k_rfn_step, dim3(n_blk), dim3(64), 0, s, (const RfnDev*)st->args, mv.rec, round);
        GEOAC_CHK(what, hipGetLastError());
        GEOAC_CHK(what, st->ev.stop(s));
        GEOAC_CHK(what, hipMemcpyAsync(&active, D.active, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        GEOAC_CHK(what, hipStreamSynchronize(s));
        double t = 0; GEOAC_CHK(what, st->ev.ms(&t));
        st->ms_kernels += t;
    }
    void* level = nullptr; size_t level_bytes = 0;
    if((rc = geoac_fan_level_dev(ctx, &level, &level_bytes))) return rc;         // (formed on first use after a launch, geoac_map.hip)
    GEOAC_CHK(what, st->ev.start(s));
    hipLaunchKernelGGL(k_rfn_rows, dim3(n_blk), dim3(64), 0, s, (const RfnDev*)st->args, mv.rec, (const double*)level);
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
    if((rc = geoac_map_view(ctx, &mv))) return rc;
    st->gen = mv.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_refine_shape(geoac_ctx* ctx, int* n_seeds, int* n_freq, int* iterations){
    Bound b;
    int rc = bind_result(ctx, "fan_refine_shape", &b);
    if(rc) return rc;
    if(n_seeds) *n_seeds = b.st->n_seeds;
    if(n_freq) *n_freq = b.st->F;
    if(iterations) *iterations = b.st->launches;
    return GEOAC_OK;
}

extern "C" int geoac_fan_refine_dev(geoac_ctx* ctx, int which, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_result(ctx, "fan_refine_dev", &b);
    if(rc) return rc;
    if(which < 0 || which > 1) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_refine_dev: which must be 0 (rows) or 1 (level)");
    const RfnState* st = b.st;
    if(dev_ptr) *dev_ptr = st->n_seeds ? (which == 0 ? (void*)st->h.rows : (void*)st->h.lvl) : nullptr;
    if(bytes) *bytes = which == 0 ? st->rows_bytes() : st->level_bytes();
    return GEOAC_OK;
}

extern "C" int geoac_fan_refine_fetch(geoac_ctx* ctx, double* rows, double* level){
    const char* what = "fan_refine_fetch";
    Bound b;
    int rc = bind_result(ctx, what, &b);
    if(rc) return rc;
    const RfnState* st = b.st;
    if(st->n_seeds == 0) return GEOAC_OK;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    if(rows) GEOAC_CHK(what, hipMemcpyAsync(rows, st->h.rows, st->rows_bytes(), hipMemcpyDeviceToHost, s));
    if(level) GEOAC_CHK(what, hipMemcpyAsync(level, st->h.lvl, st->level_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_refine_timing(geoac_ctx* ctx, double ms[2]){
    Bound b;
    int rc = bind_result(ctx, "fan_refine_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_refine_timing: NULL argument");
    ms[0] = b.st->ms_launch; ms[1] = b.st->ms_kernels;
    return GEOAC_OK;
}

extern "C" int geoac_fan_refine_stats(geoac_ctx* ctx, uint64_t stats[6]){
    Bound b;
    int rc = bind_result(ctx, "fan_refine_stats", &b);
    if(rc) return rc;
    if(!stats) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_refine_stats: NULL argument");
    for(int k = 0; k < 6; k++) stats[k] = b.st->stats[k];
    return GEOAC_OK;
}
