// geoac_level_amp.hip - level amplitudes (include/geoac_level_amp.h): the ray-tube spreading at a receiver altitude from the three crossing
// records per row - base ray, theta probe, phi probe - that a round of three rays per row leaves in the crossing tables (geoac_fan_levels_dev).
//
// Two ways in.  geoac_fan_level_amp_at makes the round itself: 3 n launch angles through geoac_fan_set_angles and geoac_fan_launch (unchanged, the
// level list still set: nothing of the launch plan is touched or known here), rows [M][n].  geoac_fan_level_amp launches nothing: it reads the final
// round of a current geoac_fan_level_refine, whose seeds (member, level, branch, status, best angles) stay in the refinement's own block
// (geoac_lrf_seeds of geoac_level_refine_int.h), rows [n_seeds].  Both end in the same three launches on the context's stream:
//   k_lamp_gather  one thread per row: BRANCH of the three rays, the record slots, and the abscissae of the crossing point for the medium probe;
//                  the members' source points behind them.
//   the probe      geoac_launch_probe_atmo1d / geoac_launch_probe_grid (coop = 0) of geoac_kernels.hip on those abscissae: the kernels behind
//                  geoac_probe_atmo_1d / geoac_probe_grid, so a host restatement takes the same bits from the public probe calls.
//   k_lamp_rows    one thread per row: the header's steps 1 .. 5.
// The kernels' arguments live in a block of device memory (LampDev).  No LDS, no atomics; a thread owns its row.
//
// The arithmetic is fixed by the header and restated in tests/level_amp_reference.py; the elementary functions are geoac_rfn_series.h's.  Every
// product is rounded before it is added, so this file is compiled with contraction off (the pragma below; the Makefile gives the same flag).
// BRANCH is the walk of geoac_level_refine.hip (lrf_branch), restated here over this file's own argument block.
//
// Index bounds, stated again at each load and store.  R = n_rows rows, N rays per block of the round's fan (3 * N rays), M members, L levels.
//   row t < R;  its ray index i = t % N < N (geoac_fan_level_amp: R = N, i = t; _at: R = M * N, rows [M][N]);  meta row t: member m < M and level
//   l < L (checked on the host before the copy / by the refinement's seed kernel), branch;  ray = j * N + i < 3 * N, j in 0 .. 2;
//   (m, ray, l) < M * 3 * N * L, the extent of both crossing tables (checked on the host against the byte counts of geoac_fan_levels_dev);
//   record slot k < min(count, capL) <= capL;  probe point p < R + M: p = t the crossing of row t, p = R + m the source of member m.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/geoac_level_amp.h"
#include "geoac_launch_int.h"
#include "geoac_level_refine_int.h"
#include "geoac_level_amp_int.h"
#include "geoac_newton_rounds.h"                  // (Carve; the series of geoac_rfn_series.h come with it)
#include "geoac_lamp_tube.h"                      // (steps 3 to 5, shared with geoac_lampmap.hip)

#pragma clang fp contract(off)

namespace {

enum { LAMP_META = 6 };                           // ints per row in LampDev::meta, the layout of the refinement's seeds (geoac_level_refine_int.h)

struct LampDev {
    const int* meta;                              // [R][LAMP_META]: member, (station), level, leg, direction (0 up, 1 down), ordinal
    const int* rstatus;                           // [R]: the refinement's statuses (geoac_fan_level_amp), or NULL
    const double* th;                             // [N]: the base rays' launch angles [deg]
    const double* ph;
    const double* src3;                           // [M][3]: the members' source points in the layout of geoac_params.src
    int* slots;                                   // [R][3]: record slot of BRANCH(base, theta probe, phi probe), -1 absent, -2 the row is SKIPPED
    double* pts;                                  // [1 or 3][R + M]: the probe's abscissae
    const double* med;                            // the probe's output: out9 [R + M][9] | rho [R + M] (1-D), api7 [R + M][7] (grid)
    double* rows;                                 // [R][GEOAC_LAMP_STRIDE]
    double h, r_earth, z_grnd;
    double r_level[GEOAC_MAX_LEVELS];             // r_earth + z_km[l]
    long long R, N;
    int M, L, capL, eqset, spherical, grid;
};

// BRANCH(ray) of geoac_level_refine.h: the slot of the crossing record of (leg, direction, ordinal) among the kept crossings of (m, ray, l), or -1.
// ray < 3 * N, so rl < M * 3 * N * L, the extent of lcount and (times capL records) of lrec.
__device__ inline int lamp_branch(const LampDev& D, const double* lrec, const int* lcount, const int* me, long long ray){
    const long long rl = ((long long)me[0] * (3ll * D.N) + ray) * D.L + me[2];
    const int seen = lcount[rl];
    const int kept = seen < D.capL ? seen : D.capL;              // only the first min(count, capL) crossings exist
    const double* Q = lrec + rl * D.capL * GEOAC_LVL_STRIDE;
    int leg_now = -1, o_up = 0, o_down = 0;
    for(int k = 0; k < kept; k++, Q += GEOAC_LVL_STRIDE){        // record slot k < kept <= capL
        const int leg = (int)Q[GEOAC_LVL_LEG];
        if(leg != leg_now){ leg_now = leg; o_up = 0; o_down = 0; }
        const int d = Q[GEOAC_LVL_DIR] > 0.0 ? 0 : 1;
        const int o = d ? o_down++ : o_up++;
        if(leg == me[3] && d == me[4] && o == me[5]) return k;
    }
    return -1;
}
// record slot k (< capL) of (m, ray, l): the same rl as above
__device__ inline const double* lamp_record(const LampDev& D, const double* lrec, const int* me, long long ray, int k){
    const long long rl = ((long long)me[0] * (3ll * D.N) + ray) * D.L + me[2];
    return lrec + (rl * D.capL + k) * GEOAC_LVL_STRIDE;
}
// crossing point of a record in the stations' axes (geoac_lstations.h)
__device__ inline void lamp_point(const LampDev& D, const double* Q, double* c0, double* c1){
    if(D.spherical){ *c0 = Q[GEOAC_LVL_P0 + 1] * 180.0 / kRfnPi; *c1 = Q[GEOAC_LVL_P0 + 2] * 180.0 / kRfnPi; }
    else { *c0 = Q[GEOAC_LVL_P0 + 0]; *c1 = Q[GEOAC_LVL_P0 + 1]; }
}
// probe point p (< R + M): its abscissae (header, step 2) - the height coordinate hc alone, or (a, b, hc) in table order: (x, y, z) / (lat, lon, r)
__device__ inline void lamp_put(const LampDev& D, long long p, double a, double b, double hc){
    const long long P = D.R + D.M;
    if(!D.grid) D.pts[p] = hc;                                   // p < R + M, the extent of a plane of pts
    else { D.pts[p] = a; D.pts[P + p] = b; D.pts[2 * P + p] = hc; }
}
// the source point of member m (< M) as the launch places it
__device__ inline void lamp_source(const LampDev& D, int m){
    const double* s = D.src3 + 3 * m;
    if(D.spherical){
        const double z = s[0] < D.z_grnd ? D.z_grnd : s[0];
        lamp_put(D, D.R + m, s[1] * kRfnPi / 180.0, s[2] * kRfnPi / 180.0, z + D.r_earth);
    } else {
        const double z = D.z_grnd < s[2] ? s[2] : D.z_grnd;
        lamp_put(D, D.R + m, s[0], s[1], z);
    }
}

__global__ void __launch_bounds__(64) k_lamp_gather(const LampDev* __restrict__ Dp, const double* __restrict__ lrec, const int* __restrict__ lcount){
    const LampDev& D = *Dp;
    const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for(long long m = t0; m < D.M; m += stride) lamp_source(D, (int)m);                 // m < M
    for(long long t = t0; t < D.R; t += stride){                                          // t < R
        const int* me = D.meta + LAMP_META * t;
        const long long i = t % D.N;                                                      // < N
        int* sl = D.slots + 3 * t;
        int k0 = -2, k1 = -2, k2 = -2;
        if(!D.rstatus || D.rstatus[t] == GEOAC_RFN_CONVERGED){
            k0 = lamp_branch(D, lrec, lcount, me, i);
            k1 = lamp_branch(D, lrec, lcount, me, D.N + i);
            k2 = lamp_branch(D, lrec, lcount, me, 2 * D.N + i);
        }
        sl[0] = k0; sl[1] = k1; sl[2] = k2;
        if(k0 >= 0){
            const double* Q = lamp_record(D, lrec, me, i, k0) + GEOAC_LVL_P0;
            if(D.spherical) lamp_put(D, t, Q[1], Q[2], Q[0]); else lamp_put(D, t, Q[0], Q[1], Q[2]);
        } else {                                                                          // (a point the probe can evaluate; its values are not read)
            const double* s = D.src3 + 3 * me[0];                                         // member me[0] < M
            if(D.spherical) lamp_put(D, t, s[1] * kRfnPi / 180.0, s[2] * kRfnPi / 180.0, D.r_level[me[2]]); else lamp_put(D, t, s[0], s[1], D.z_grnd);
        }
    }
}

// the probe's values at point p (< R + M)
__device__ inline LampMedium lamp_medium(const LampDev& D, long long p){
    LampMedium m;
    if(D.grid){ const double* a = D.med + 7 * p; m.c = a[0]; m.rho = a[1]; m.u = a[2]; m.v = a[3]; }
    else { const double* o = D.med + 9 * p; m.c = o[0]; m.u = o[3]; m.v = o[6]; m.rho = D.med[9 * (D.R + D.M) + p]; }
    return m;
}

__global__ void __launch_bounds__(64) k_lamp_rows(const LampDev* __restrict__ Dp, const double* __restrict__ lrec){
    const LampDev& D = *Dp;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < D.R; t += stride){      // t < R
        const int* me = D.meta + LAMP_META * t;
        const long long i = t % D.N;                                                      // < N
        const int* sl = D.slots + 3 * t;
        double* row = D.rows + t * GEOAC_LAMP_STRIDE;
        const double th = D.th[i], ph = D.ph[i];
        int status = GEOAC_LAMP_OK;
        if(sl[0] == -2) status = GEOAC_LAMP_SKIPPED;
        else if(sl[0] < 0) status = GEOAC_LAMP_ABSENT;
        else if(sl[1] < 0 || sl[2] < 0) status = GEOAC_LAMP_NO_PROBE;
        double det = 0.0, tz = 0.0, dd = 0.0, amp = 0.0, c_out = 0.0, rho_out = 0.0, tt = 0.0, att = 0.0;
        if(status == GEOAC_LAMP_OK){
            const double* Q = lamp_record(D, lrec, me, i, sl[0]);
            const double* Qt = lamp_record(D, lrec, me, D.N + i, sl[1]);
            const double* Qp = lamp_record(D, lrec, me, 2 * D.N + i, sl[2]);
            const double h = D.h;
            double c0, c1, ct0, ct1, cp0, cp1;
            lamp_point(D, Q, &c0, &c1); lamp_point(D, Qt, &ct0, &ct1); lamp_point(D, Qp, &cp0, &cp1);
            const double a00 = (ct0 - c0) / h, a01 = (cp0 - c0) / h;
            double a10, a11;
            if(D.spherical){ a10 = wrap180(ct1 - c1) / h; a11 = wrap180(cp1 - c1) / h; }
            else { a10 = (ct1 - c1) / h; a11 = (cp1 - c1) / h; }
            det = a00 * a11 - a01 * a10;
            const LampMedium m = lamp_medium(D, t), s = lamp_medium(D, D.R + me[0]);      // member me[0] < M
            // steps 3 to 5 (geoac_lamp_tube.h); level me[2] < L <= GEOAC_MAX_LEVELS
            lamp_tube(D.eqset, m, s, th, ph, Q[GEOAC_LVL_P0 + 3], Q[GEOAC_LVL_P0 + 4], Q[GEOAC_LVL_P0 + 5], det, c0, D.r_level[me[2]], &tz, &dd, &amp);
            if(det == 0.0 || !rfn_finite(det) || dd == 0.0 || !rfn_finite(dd) || amp == 0.0 || !rfn_finite(amp)){
                status = GEOAC_LAMP_SINGULAR;
                det = 0.0; tz = 0.0; dd = 0.0; amp = 0.0;
            } else { c_out = m.c; rho_out = m.rho; tt = Q[GEOAC_LVL_TTIME]; att = Q[GEOAC_LVL_ATTEN]; }
        }
        row[GEOAC_LAMP_MEMBER] = (double)me[0]; row[GEOAC_LAMP_INDEX] = (double)i; row[GEOAC_LAMP_LEG] = (double)me[3];
        row[GEOAC_LAMP_DIR] = me[4] ? -1.0 : 1.0; row[GEOAC_LAMP_ORD] = (double)me[5]; row[GEOAC_LAMP_STATUS] = (double)status;
        row[GEOAC_LAMP_THETA] = th; row[GEOAC_LAMP_PHI] = ph;
        row[GEOAC_LAMP_DET] = det; row[GEOAC_LAMP_TZ] = tz; row[GEOAC_LAMP_D] = dd; row[GEOAC_LAMP_AMP] = amp;
        row[GEOAC_LAMP_C] = c_out; row[GEOAC_LAMP_RHO] = rho_out; row[GEOAC_LAMP_TTIME] = tt; row[GEOAC_LAMP_ATTEN] = att;
    }
}

struct LampState {
    void* buf = nullptr; size_t buf_cap = 0;              // every device array of a call
    LampDev h{};                                          // host copy of the argument block (alive while its copy runs)
    std::vector<int> h_meta;
    std::vector<double> h_ang, h_src;
    unsigned long long gen = 0;                           // the context's invalidation counter the result was made at (0: none)
    long long n_rows = 0;
    int M = 0;
    double ms_launch = 0.0, ms_kernels = 0.0;
    EventPair ev;
    size_t rows_bytes() const { return sizeof(double) * (size_t)n_rows * GEOAC_LAMP_STRIDE; }
};

struct Bound { geoac_ctx* ctx; GeoacLampView v; LampState* st; };

int bind(geoac_ctx* ctx, const char* what, Bound* b){
    if(!ctx) return GEOAC_E_INVALID;
    b->ctx = ctx;
    int rc = geoac_lamp_view(ctx, &b->v);
    if(rc) return rc;
    b->st = (LampState*)*b->v.state;
    if(hipSetDevice(b->v.map.device) != hipSuccess) return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": hipSetDevice failed").c_str());
    return GEOAC_OK;
}

// a current result, or GEOAC_E_INVALID.  (geoac_set_levels does not move the invalidation counter: the crossing tables answer for it.)
int bind_result(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = bind(ctx, what, b);
    if(rc) return rc;
    if(!b->st || b->st->gen == 0 || b->st->gen != b->v.map.gen || geoac_fan_levels_dev(ctx, nullptr, nullptr, nullptr, nullptr) != GEOAC_OK)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no level amplitude rows, or a launch, new angles, an atmosphere upload, geoac_set_sources, "
                                                     "geoac_set_frequencies or geoac_set_levels have come since them (call geoac_fan_level_amp_at or geoac_fan_level_amp again)").c_str());
    return GEOAC_OK;
}

const char* const kNoGlobalRngDep = "not available for GEOAC_EQ_GLOBAL_RNGDEP: on a range-dependent spherical grid the forward-difference tube is not converged in probe_deg behind a turning point, and a row could not say so (DESIGN 8p)";

const char* probe_fault(int eqset, double probe_deg, int* code){
    *code = GEOAC_E_INVALID;
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(eqset == GEOAC_EQ_2D){ *code = GEOAC_E_UNSUPPORTED; return "not implemented for the 2-D set: it has no level crossings (geoac_levels.h)"; }
    if(eqset == GEOAC_EQ_GLOBAL_RNGDEP){ *code = GEOAC_E_UNSUPPORTED; return kNoGlobalRngDep; }
    if(!std::isfinite(probe_deg) || !(probe_deg > 0.0) || probe_deg > 1.0) return "probe_deg must be finite, > 0 and <= 1";
    return nullptr;
}

// what both entry points refuse of a context, whatever their arguments
int context_fault(const Bound& b, const std::string& what){
    if(b.v.map.eqset == GEOAC_EQ_2D) return geoac_map_fail(b.ctx, GEOAC_E_UNSUPPORTED, (what + ": not implemented for the 2-D set: it has no level crossings (geoac_levels.h)").c_str());
    if(b.v.map.eqset == GEOAC_EQ_GLOBAL_RNGDEP) return geoac_map_fail(b.ctx, GEOAC_E_UNSUPPORTED, (what + ": " + kNoGlobalRngDep).c_str());
    if(b.v.n_profiles > 1)
        return geoac_map_fail(b.ctx, GEOAC_E_UNSUPPORTED, (what + ": not available for an ensemble or a grid ensemble (K > 1): the medium probes evaluate member 0's atmosphere only; "
                                                          "take the member's amplitudes on a context of its own").c_str());
    if(b.v.mode & (GEOAC_MODE_WRITE_RAYS | GEOAC_MODE_WRITE_CAUSTICS))
        return geoac_map_fail(b.ctx, GEOAC_E_INVALID, (what + ": not available with sample capture (WriteRays / WriteCaustics)").c_str());
    return GEOAC_OK;
}

// the three launches behind either entry point.  D holds everything but the pointers into this call's block; meta / angles come from the host
// vectors of the state (h_meta, h_ang non-empty) or are the refinement's device arrays already in D.  The round's tables must have N rays per block.
int make_rows(Bound& b, const char* what, LampDev& D){
    LampState* st = b.st;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    const size_t R = (size_t)D.R, N = (size_t)D.N, M = (size_t)D.M, P = R + M;
    void* lrec = nullptr; void* lcount = nullptr; size_t lrec_bytes = 0, lcount_bytes = 0;
    int rc = geoac_fan_levels_dev(b.ctx, &lrec, &lrec_bytes, &lcount, &lcount_bytes);
    if(rc) return geoac_map_fail(b.ctx, rc, (std::string(what) + ": " + geoac_last_error(b.ctx)).c_str());
    GeoacMapView now{};
    if((rc = geoac_map_view(b.ctx, &now))) return rc;
    const size_t n_rl = M * 3 * N * (size_t)D.L;                      // (member, ray, level) of the round's crossing tables
    if(!now.fresh || (size_t)now.M != M || (size_t)now.n_rays != 3 * N || lcount_bytes != sizeof(int) * n_rl || lrec_bytes != sizeof(double) * GEOAC_LVL_STRIDE * n_rl * (size_t)D.capL)
        return geoac_map_fail(b.ctx, GEOAC_E_HIP, (std::string(what) + ": the crossing tables do not have the shape of the rows ([M][3 * n][L][cap])").c_str());
    if(!b.v.dev_params) return geoac_map_fail(b.ctx, GEOAC_E_INVALID, (std::string(what) + ": no parameter block of a completed launch").c_str());

    // one device block: args | meta | th | ph | src3 | slots | pts | med (| out30) | rows
    const size_t planes = D.grid ? 3 : 1, med_w = D.grid ? 7 : 10;
    Carve carve;
    const size_t o_args = carve(sizeof(LampDev)), o_meta = carve(sizeof(int) * LAMP_META * R), o_ang = carve(sizeof(double) * 2 * N), o_src = carve(sizeof(double) * 3 * M),
                 o_slots = carve(sizeof(int) * 3 * R), o_pts = carve(sizeof(double) * planes * P), o_med = carve(sizeof(double) * med_w * P),
                 o_out30 = carve(D.grid ? sizeof(double) * 30 * P : 0), o_rows = carve(sizeof(double) * GEOAC_LAMP_STRIDE * R);
    if(grow(&st->buf, &st->buf_cap, carve.off)) return geoac_map_fail(b.ctx, GEOAC_E_NOMEM, (std::string(what) + ": no device memory for the rows").c_str());
    char* base = (char*)st->buf;
    if(!st->h_meta.empty()){
        D.meta = (const int*)(base + o_meta); D.th = (const double*)(base + o_ang); D.ph = D.th + N;
        GEOAC_CHK(what, hipMemcpyAsync(base + o_meta, st->h_meta.data(), sizeof(int) * LAMP_META * R, hipMemcpyHostToDevice, s));
        GEOAC_CHK(what, hipMemcpyAsync(base + o_ang, st->h_ang.data(), sizeof(double) * 2 * N, hipMemcpyHostToDevice, s));
    }
    D.src3 = (const double*)(base + o_src); D.slots = (int*)(base + o_slots); D.pts = (double*)(base + o_pts); D.med = (const double*)(base + o_med);
    D.rows = (double*)(base + o_rows);
    st->h_src.assign(b.v.src3, b.v.src3 + 3 * M);
    st->h = D;
    GEOAC_CHK(what, hipMemcpyAsync(base + o_args, &st->h, sizeof(LampDev), hipMemcpyHostToDevice, s));
    GEOAC_CHK(what, hipMemcpyAsync(base + o_src, st->h_src.data(), sizeof(double) * 3 * M, hipMemcpyHostToDevice, s));
    const LampDev* args = (const LampDev*)(base + o_args);
    const unsigned n_blk = blocks_for((long long)R, 64);
    GEOAC_CHK(what, st->ev.start(s));
    hipLaunchKernelGGL(k_lamp_gather, dim3(n_blk), dim3(64), 0, s, args, (const double*)lrec, (const int*)lcount);
    GEOAC_CHK(what, hipGetLastError());
    double* pts = (double*)(base + o_pts); double* med = (double*)(base + o_med);
    if(D.grid) GEOAC_CHK(what, geoac_launch_probe_grid(b.v.dev_params, (int)P, pts, pts + P, pts + 2 * P, 0, (double*)(base + o_out30), med, s));
    else       GEOAC_CHK(what, geoac_launch_probe_atmo1d(b.v.dev_params, (int)P, pts, med, med + 9 * P, s));
    hipLaunchKernelGGL(k_lamp_rows, dim3(n_blk), dim3(64), 0, s, args, (const double*)lrec);
    GEOAC_CHK(what, hipGetLastError());
    GEOAC_CHK(what, st->ev.stop(s));
    GEOAC_CHK(what, hipStreamSynchronize(s));                          // (the host vectors and st->h may change from here on)
    GEOAC_CHK(what, st->ev.ms(&st->ms_kernels));
    st->n_rows = (long long)R; st->M = (int)M;
    st->gen = now.gen;
    return GEOAC_OK;
}

// the level list of the context into D; GEOAC_E_INVALID without one
int level_list(const Bound& b, const std::string& what, LampDev* D){
    int L = 0, capL = 0;
    double z_km[GEOAC_MAX_LEVELS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc = geoac_get_levels(b.ctx, &L, z_km, &capL);
    if(rc) return rc;
    if(L < 1 || L > GEOAC_MAX_LEVELS || capL < 1) return geoac_map_fail(b.ctx, GEOAC_E_INVALID, (what + ": the context has no level list (geoac_set_levels)").c_str());
    D->L = L; D->capL = capL;
    for(int l = 0; l < GEOAC_MAX_LEVELS; l++) D->r_level[l] = l < L ? b.v.r_earth + z_km[l] : 0.0;
    return GEOAC_OK;
}

void fill_common(const Bound& b, LampDev* D){
    D->r_earth = b.v.r_earth; D->z_grnd = b.v.z_grnd;
    D->eqset = b.v.map.eqset; D->spherical = spherical(b.v.map.eqset) ? 1 : 0; D->grid = b.v.grid ? 1 : 0;
}

LampState* begin(Bound& b){
    if(!*b.v.state) *b.v.state = new LampState();
    b.st = (LampState*)*b.v.state;
    b.st->gen = 0; b.st->n_rows = 0; b.st->M = 0; b.st->ms_launch = 0.0; b.st->ms_kernels = 0.0;
    b.st->h_meta.clear(); b.st->h_ang.clear();
    return b.st;
}

}  // namespace

extern "C" void geoac_lamp_release(void* state){
    LampState* st = (LampState*)state;
    if(!st) return;
    if(st->buf) hipFree(st->buf);
    st->ev.release();
    delete st;
}

extern "C" int geoac_level_amp_check(int eqset, double probe_deg, const char** fault){
    int code;
    const char* f = probe_fault(eqset, probe_deg, &code);
    if(fault) *fault = f;
    return f ? code : GEOAC_OK;
}

extern "C" int geoac_fan_level_amp_at(geoac_ctx* ctx, int n, const double* theta_deg, const double* phi_deg, const int* level_of, const int* leg, const int* dir,
                                      const int* ord, double probe_deg){
    const char* what = "fan_level_amp_at";
    Bound b;
    int rc = bind(ctx, what, &b);
    if(rc) return rc;
    if((rc = context_fault(b, what))) return rc;
    int code;
    if(const char* fault = probe_fault(b.v.map.eqset, probe_deg, &code)) return geoac_map_fail(ctx, code, (std::string("fan_level_amp_at: ") + fault).c_str());
    if(n <= 0 || !theta_deg || !phi_deg || !level_of || !leg || !dir || !ord) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_amp_at: n must be > 0 and no array NULL");
    LampDev D{};
    if((rc = level_list(b, what, &D))) return rc;
    for(int i = 0; i < n; i++){
        if(level_of[i] < 0 || level_of[i] >= D.L) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_amp_at: level_of outside the context's level list");
        if(dir[i] != 1 && dir[i] != -1) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_amp_at: dir must be +1 (upward) or -1 (downward)");
        if(leg[i] < 0 || ord[i] < 0) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_amp_at: leg and ord must be >= 0");
    }
    const int M = b.v.n_members;
    if(3ll * n * M > GEOAC_RFN_MAX_RAY_MEMBERS)
        return geoac_map_fail(ctx, GEOAC_E_CAPACITY, ("fan_level_amp_at: more than " + std::to_string(GEOAC_RFN_MAX_RAY_MEMBERS) + " ray-members (3 rays x n x " + std::to_string(M) +
                                                      " members: every member integrates every ray and its two probes); ask for fewer rays or members at a time").c_str());
    LampState* st = begin(b);
    // the round's fan: ray j * n + i is ray i at the trial (j = 0), at theta + h (1), at phi + h (2)
    std::vector<double> fan(6 * (size_t)n);
    for(int i = 0; i < n; i++){
        fan[i] = theta_deg[i];                          fan[3 * (size_t)n + i] = phi_deg[i];
        fan[(size_t)n + i] = theta_deg[i] + probe_deg;  fan[4 * (size_t)n + i] = phi_deg[i];
        fan[2 * (size_t)n + i] = theta_deg[i];          fan[5 * (size_t)n + i] = phi_deg[i] + probe_deg;
    }
    if((rc = geoac_fan_set_angles(ctx, 3 * n, fan.data(), fan.data() + 3 * (size_t)n))) return rc;
    if((rc = geoac_fan_launch(ctx))) return rc;
    double ms3[3] = {0, 0, 0}; uint64_t st3[3] = {0, 0, 0};
    if(geoac_last_timing(ctx, ms3, st3) == GEOAC_OK) st->ms_launch = ms3[0];
    if((rc = geoac_lamp_view(ctx, &b.v))) return rc;                    // (the launch's parameter block, its source point and ground, the counter after it)
    if((rc = level_list(b, what, &D))) return rc;                       // (the level radii with the launch's r_earth)
    st->h_meta.resize((size_t)LAMP_META * M * n);
    for(int m = 0; m < M; m++)
        for(int i = 0; i < n; i++){
            int* me = &st->h_meta[(size_t)LAMP_META * ((size_t)m * n + i)];
            me[0] = m; me[1] = 0; me[2] = level_of[i]; me[3] = leg[i]; me[4] = dir[i] > 0 ? 0 : 1; me[5] = ord[i];
        }
    st->h_ang.assign(theta_deg, theta_deg + n);
    st->h_ang.insert(st->h_ang.end(), phi_deg, phi_deg + n);
    fill_common(b, &D);
    D.h = probe_deg; D.R = (long long)M * n; D.N = n; D.M = M;
    return make_rows(b, what, D);
}

extern "C" int geoac_fan_level_amp(geoac_ctx* ctx){
    const char* what = "fan_level_amp";
    Bound b;
    int rc = bind(ctx, what, &b);
    if(rc) return rc;
    if((rc = context_fault(b, what))) return rc;
    GeoacLrfSeeds S;
    if((rc = geoac_lrf_seeds(ctx, what, &S))) return rc;
    LampState* st = begin(b);
    if(S.n_seeds == 0){ st->gen = b.v.map.gen; st->M = b.v.n_members; return GEOAC_OK; }      // (an empty result)
    LampDev D{};
    if((rc = level_list(b, what, &D))) return rc;
    if(D.L != S.L || D.capL != S.capL || b.v.n_members != S.M)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_amp: the level list or the members of the context are not those of the refinement");
    fill_common(b, &D);
    D.meta = S.meta; D.rstatus = S.status; D.th = S.theta; D.ph = S.phi;
    D.h = S.probe_deg; D.R = S.n_seeds; D.N = S.n_seeds; D.M = S.M;
    return make_rows(b, what, D);
}

extern "C" int geoac_fan_level_amp_shape(geoac_ctx* ctx, int* n_rows, int* members){
    Bound b;
    int rc = bind_result(ctx, "fan_level_amp_shape", &b);
    if(rc) return rc;
    if(n_rows) *n_rows = (int)b.st->n_rows;
    if(members) *members = b.st->M;
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_amp_dev(geoac_ctx* ctx, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_result(ctx, "fan_level_amp_dev", &b);
    if(rc) return rc;
    if(dev_ptr) *dev_ptr = b.st->n_rows ? (void*)b.st->h.rows : nullptr;
    if(bytes) *bytes = b.st->rows_bytes();
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_amp_fetch(geoac_ctx* ctx, double* rows){
    const char* what = "fan_level_amp_fetch";
    Bound b;
    int rc = bind_result(ctx, what, &b);
    if(rc) return rc;
    if(b.st->n_rows == 0 || !rows) return GEOAC_OK;
    hipStream_t s = (hipStream_t)b.v.map.stream;
    GEOAC_CHK(what, hipMemcpyAsync(rows, b.st->h.rows, b.st->rows_bytes(), hipMemcpyDeviceToHost, s));
    GEOAC_CHK(what, hipStreamSynchronize(s));
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_amp_timing(geoac_ctx* ctx, double ms[2]){
    Bound b;
    int rc = bind_result(ctx, "fan_level_amp_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_level_amp_timing: NULL argument");
    ms[0] = b.st->ms_launch; ms[1] = b.st->ms_kernels;
    return GEOAC_OK;
}
