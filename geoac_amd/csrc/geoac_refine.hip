// geoac_refine.hip - station refinement (include/geoac_refine.h): Newton eigenrays for every estimate of the station lists.
//
// A round is one fan of all seeds through the existing launch path (geoac_fan_set_angles, geoac_fan_launch: nothing of the launch plan is
// touched or known here) and one kernel that applies the header's step rule to every seed from its own member's record.  Every member
// integrates every seed; a seed reads one member's record, the other M - 1 are discarded (header, "Cost").  The seed list, the rounds and the
// step rule are geoac_newton_rounds.h's, shared with geoac_level_refine.hip; this file's own are where a seed comes from (a station-list
// row), its miss and Jacobian (the landing record's launch-angle derivatives) and what a finished row holds.
//
// Three kernels:
//   k_rfn_seed   one thread per (list, row): the kept rows of the station lists become the dense seed list, each at its list's prefix count
//                plus its place in the list - list order, no atomics.  The prefix counts are integers summed on the host from hits[M][n_sta].
//   k_rfn_step   one thread per seed, after a round's launch: miss, the step rule, next trial; counts the seeds still active (the host's one read).
//   k_rfn_rows   one thread per seed, after the last launch: the row and the seed's levels.
// The kernels' arguments live in a block of device memory (RfnDev): passed by value they would sit in scalar registers beside the loop state.
//
// The arithmetic is fixed by the header and restated in tests/refine_reference.py, elementary functions included (geoac_rfn_series.h):
// every product is rounded before it is added, so this file is compiled with contraction off (the pragma below; the Makefile gives the
// same flag).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string>
#include <vector>

#include "../../include/geoac_refine.h"
#include "geoac_launch_int.h"
#include "geoac_stations_int.h"
#include "geoac_refine_int.h"
#include "geoac_tri_rule.h"
#include "geoac_newton_rounds.h"

#pragma clang fp contract(off)

namespace {

struct RfnDev : RoundsDev {
    enum { RAYS = 1 };
    const double* sta_rows;                       // the station lists' rows (read by k_rfn_seed only)
    const double* mem;                            // [M][GEOAC_RFN_MEMW]: a copy of this call's own
    int* meta;                                    // [n_seeds][4]: member, station, leg, triangle
    double* rows; double* lvl;
    double rg, r_earth;
    int eqset, F, legs;

    struct Seed { const double* R; double s0, s1; int m; };             // the seed's record of the round, its station, its member
    __device__ void set_trial(long long i, double th, double ph) const { trial[i] = th; trial[n_seeds + i] = ph; }

    // miss of the seed's record on its leg (header, "The record")
    __device__ double miss(long long i, const double* rec, Seed* Sd) const {
        const int* me = meta + 4 * i;
        const double s0 = sta[2 * me[1]], s1 = sta[2 * me[1] + 1];
        const double* R = rec + (((long long)me[0] * n_seeds + i) * legs + me[2]) * GEOAC_REC_STRIDE;
        Sd->R = R; Sd->s0 = s0; Sd->s1 = s1; Sd->m = me[0];
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        if(R[GEOAC_REC_VALID] == 0.0) return inf;
        const double* S = R + GEOAC_REC_STATE;
        double miss;
        if(spherical) miss = rfn_dist(S[1] * 180.0 / kRfnPi, S[2] * 180.0 / kRfnPi, s0, s1, rg);
        else { const double dx = s0 - S[0], dy = s1 - S[1]; miss = sqrt(dx * dx + dy * dy); }
        return miss == miss ? miss : inf;
    }

    // Newton step of the seed's record in launch angles; false: SINGULAR
    __device__ bool newton(long long, const Seed& Sd, double th, double ph, const double*, double* d_th, double* d_ph) const {
        const double* S = Sd.R + GEOAC_REC_STATE;
        const double s0 = Sd.s0, s1 = Sd.s1;
        double e0, e1, a00, a01, a10, a11;
        if(spherical){
            e0 = s0 * kRfnPi / 180.0 - S[1];
            e1 = wrap180(s1 - S[2] * 180.0 / kRfnPi) * kRfnPi / 180.0;
            const double q = 1.0 / rg, qc = 1.0 / (rg * rfn_cos(S[1]));
            a00 = S[7] - ((q * S[4]) / S[3]) * S[6];    a01 = S[13] - ((q * S[4]) / S[3]) * S[12];
            a10 = S[8] - ((qc * S[5]) / S[3]) * S[6];   a11 = S[14] - ((qc * S[5]) / S[3]) * S[12];
        } else if(eqset == GEOAC_EQ_3D){
            e0 = s0 - S[0]; e1 = s1 - S[1];
            const double* mm = mem + (long long)Sd.m * GEOAC_RFN_MEMW;
            double st, ct, sp, cp;
            rfn_sincosd(th, &st, &ct);
            rfn_sincosd(90.0 - ph, &sp, &cp);
            const double n0 = ct * cp, n1 = ct * sp;
            const double m = 1.0 + (n0 * mm[2] + n1 * mm[3]);
            const double g0 = (n0 / m) / S[3], g1 = (n1 / m) / S[3];
            a00 = S[4] - g0 * S[6];  a01 = S[8] - g0 * S[10];  a10 = S[5] - g1 * S[6];  a11 = S[9] - g1 * S[10];
        } else {
            e0 = s0 - S[0]; e1 = s1 - S[1];
            const double g0 = S[3] / S[5], g1 = S[4] / S[5];
            a00 = S[6] - g0 * S[8];  a01 = S[12] - g0 * S[14];  a10 = S[7] - g1 * S[8];  a11 = S[13] - g1 * S[14];
        }
        double det, dlt, dlp;
        solve(a00, a01, a10, a11, e0, e1, &det, &dlt, &dlp);
        dlt = (dlt * 180.0) / kRfnPi; dlp = (dlp * 180.0) / kRfnPi;          // (the derivatives are per radian; azimuth runs against phi)
        if(!cut(det, &dlt, &dlp, step_max)) return false;
        *d_th = dlt; *d_ph = -dlp;
        return true;
    }
};

__global__ void k_rfn_seed(const RfnDev* __restrict__ Dp){
    const RfnDev& D = *Dp;
    const long long n = D.n_lists * D.cap;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride){
        const long long list = t / D.cap, i = seed_slot(D, list, (unsigned)(t % D.cap));
        if(i < 0) continue;
        const double* row = D.sta_rows + t * GEOAC_STA_STRIDE;
        int* me = D.meta + 4 * i;
        me[0] = (int)(list / D.n_sta); me[1] = (int)(list % D.n_sta); me[2] = (int)row[GEOAC_STA_LEG]; me[3] = (int)row[GEOAC_STA_TRI];
        D.trial[i] = row[GEOAC_STA_THETA]; D.trial[D.n_seeds + i] = row[GEOAC_STA_PHI];
        seed_init(D, i);
    }
}

__global__ void k_rfn_step(const RfnDev* __restrict__ Dp, const double* __restrict__ rec, int round){ rounds_step(*Dp, round, rec); }

__global__ void k_rfn_rows(const RfnDev* __restrict__ Dp, const double* __restrict__ rec, const double* __restrict__ level){
    const RfnDev& D = *Dp;
    const long long N = D.n_seeds;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= N) return;
    const int* me = D.meta + 4 * i;
    const int m = me[0], leg = me[2];
    double* row = D.rows + i * GEOAC_RFN_STRIDE;
    const bool conv = row_head(D, i, row, GEOAC_RFN_STATUS, GEOAC_RFN_ITER, GEOAC_RFN_THETA, GEOAC_RFN_PHI, GEOAC_RFN_MISS) == GEOAC_RFN_CONVERGED;
    row[GEOAC_RFN_MEMBER] = (double)m; row[GEOAC_RFN_STATION] = (double)me[1]; row[GEOAC_RFN_LEG] = (double)leg; row[GEOAC_RFN_TRI] = (double)me[3];
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

struct RfnState : RoundsState {
    RfnDev h{};                                           // host copy of the argument block (alive while its copy runs)
    RfnDev* args = nullptr;
    std::vector<double> h_mem;
    int F = 0;
    size_t rows_bytes() const { return sizeof(double) * (size_t)n_seeds * GEOAC_RFN_STRIDE; }
    size_t level_bytes() const { return sizeof(double) * (size_t)n_seeds * F; }
};

const char* spec_fault(int eqset, const geoac_refine_spec* s, int* code){
    return rounds_spec_fault(eqset, s, "not implemented for the 2-D set: it has no station lists to refine (geoac_stations.h)", code);
}

using Bound = RoundsBound<GeoacRfnView, RfnState>;

// a current result, or GEOAC_E_INVALID
int bind_result(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = rounds_bind(ctx, what, geoac_rfn_view, b);
    if(rc) return rc;
    if(!b->st || b->st->gen == 0 || b->st->gen != b->v.map.gen)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no refinement result, or a launch, new angles, an atmosphere upload, geoac_set_sources or "
                                                     "geoac_set_frequencies have come since it (call geoac_fan_refine again)").c_str());
    return GEOAC_OK;
}

}  // namespace

extern "C" void geoac_rfn_release(void* state){ rounds_release<RfnState>(state); }

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
    int rc = rounds_bind(ctx, what, geoac_rfn_view, &b);
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
    hipStream_t s = (hipStream_t)b.v.map.stream;
    void* d_hits = nullptr; void* d_rows = nullptr; const double* d_sta = nullptr; size_t bytes = 0;
    if((rc = geoac_fan_stations_dev(ctx, 0, &d_hits, &bytes)) || (rc = geoac_fan_stations_dev(ctx, 1, &d_rows, &bytes)) || (rc = geoac_sta_coords_dev(ctx, &d_sta, nullptr))) return rc;
    const long long n_lists = (long long)M * n_sta;
    std::vector<unsigned> offs;
    long long n_seeds = 0;
    GEOAC_CHK(what, count_seeds(d_hits, n_lists, cap, M, 1, s, &offs, &n_seeds));
    if(n_seeds < 0)
        return geoac_map_fail(ctx, GEOAC_E_CAPACITY, ("fan_refine: more than " + std::to_string(GEOAC_RFN_MAX_RAY_MEMBERS) + " ray-members per round (seeds x " + std::to_string(M) +
                                                      " members: every member integrates every seed); refine fewer stations or members at a time").c_str());
    RfnState* st = b.begin(&offs, n_seeds);
    st->F = F;
    if(n_seeds == 0){ st->gen = b.v.map.gen; return GEOAC_OK; }       // (an empty result; nothing was launched, the lists stay)

    // one device block: args | offs | sta | mem | meta | trial | best | state | active | rows | level
    const size_t N = (size_t)n_seeds;
    Carve carve;
    const size_t o_args = carve(sizeof(RfnDev)), o_offs = carve(sizeof(unsigned) * (size_t)n_lists), o_sta = carve(sizeof(double) * 2 * (size_t)n_sta),
                 o_mem = carve(sizeof(double) * GEOAC_RFN_MEMW * (size_t)M), o_meta = carve(sizeof(int) * 4 * N), o_trial = carve(sizeof(double) * 2 * N),
                 o_best = carve(sizeof(double) * 5 * N), o_state = carve(sizeof(int) * 3 * N), o_active = carve(sizeof(unsigned)),
                 o_rows = carve(sizeof(double) * GEOAC_RFN_STRIDE * N), o_level = carve(sizeof(double) * (size_t)F * N);
    if(grow(&st->buf, &st->buf_cap, carve.off)) return geoac_map_fail(ctx, GEOAC_E_NOMEM, "fan_refine: no device memory for the seeds");
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
    GEOAC_CHK(what, hipMemcpyAsync(st->args, &D, sizeof(RfnDev), hipMemcpyHostToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_offs, st->h_offs.data(), sizeof(unsigned) * (size_t)n_lists, hipMemcpyHostToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_sta, d_sta, sizeof(double) * 2 * (size_t)n_sta, hipMemcpyDeviceToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_mem, st->h_mem.data(), sizeof(double) * st->h_mem.size(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_rfn_seed, dim3(blocks_for(n_lists * cap, 256)), dim3(256), 0, s, (const RfnDev*)st->args);
    GEOAC_CHK(what, hipGetLastError());

    const unsigned n_blk = blocks_for(n_seeds, 64);
    rc = run_rounds(b, what, D, 1, spec->max_iter, [&](int round, const GeoacMapView& v){
        if(v.M != M || v.n_rays != (int)n_seeds || v.legs != D.legs) return geoac_map_fail(ctx, GEOAC_E_HIP, "fan_refine: the round's launch does not have the shape of the seeds");
        hipLaunchKernelGGL(k_rfn_step, dim3(n_blk), dim3(64), 0, s, (const RfnDev*)st->args, v.rec, round);
        return (int)GEOAC_OK;
    });
    if(rc) return rc;
    void* level = nullptr; size_t level_bytes = 0;
    if((rc = geoac_fan_level_dev(ctx, &level, &level_bytes))) return rc;         // (formed on first use after a launch, geoac_map.hip; the counter stays)
    return finish_rounds(b, what, D, [&]{ hipLaunchKernelGGL(k_rfn_rows, dim3(n_blk), dim3(64), 0, s, (const RfnDev*)st->args, st->last.rec, (const double*)level); });
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
    return rc ? rc : rounds_timing(ctx, "fan_refine_timing", *b.st, ms);
}

extern "C" int geoac_fan_refine_stats(geoac_ctx* ctx, uint64_t stats[6]){
    Bound b;
    int rc = bind_result(ctx, "fan_refine_stats", &b);
    return rc ? rc : rounds_stats(ctx, "fan_refine_stats", *b.st, stats);
}
