// geoac_levels.hip - level crossings (include/geoac_levels.h): k_levels, its launcher, and the host-only check of a level list.
//
// k_levels is a second consumer of what k_accum consumes: one thread per column of an epoch's chunk walks the column's rows in order, with
// k_accum's bookkeeping (colmap / n_cols / nrows / legend / nlegend; chunk row 0 is the carry row; the pair i == cur_end - a leg-end row
// followed by the next leg's start row - is no segment).  It keeps running sums of its own (tt, at, ltt, lat, leg in Q.state, zeroed per
// launch), formed with k_accum's arrivals-only arithmetic in k_accum's order: one add per row and sum, the per-leg partial sum folded into
// the cumulative one at the leg end.  They are therefore k_accum's sums bit for bit, and k_accum's state is not touched.
//
// The thread owns its ray's [L][cap] record slots and [L] counts (caller's ray order through perm): no atomics, no lists, no sorting - the
// output is the same bits on every run and under every launch plan.
//
// This file is compiled with -ffp-contract=off (csrc/Makefile): FRAC, TTIME, ATTEN and the interpolated components are a subtract, a
// divide, a multiply and an add each, rounded one by one, as tests/levels_reference.py restates them.
//
// Index bounds - every one is a bound k_accum already relies on:
//   col < n_cols <= n_pad (the first test);  chunk rows i and i + 1 with i + 1 < nrows[col] <= s_rows + 1 - the rows k_rk4 wrote and the
//   post-pass read; contrib row i of the same range;  slot = colmap[col] < n_pad (k_compact lists slots);  ray = perm[slot] in
//   [0, n_rays) for a slot with rows (tested all the same);  level l < L, a template constant;  record slot k < cap (tested at the store).
#include <hip/hip_runtime.h>
#include <cmath>

#include "geoac_levels_int.h"

namespace {

__device__ inline bool lvl_up(double ha, double hb, double lev){ return ha < lev && lev <= hb; }
__device__ inline bool lvl_down(double ha, double hb, double lev){ return ha >= lev && lev > hb; }

template <int L>
__global__ void __launch_bounds__(256) k_levels(GeoacDevParams P, GeoacLevelParams Q){
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if(col >= (P.colmap ? *P.n_cols : P.n_pad)) return;         // col < n_cols <= n_pad from here on
    const size_t np = (size_t)P.n_pad;
    const int nr = P.nrows[col];                                // [n_pad]; 0 for slots without a ray
    if(nr < 2) return;
    const int slot = P.colmap ? P.colmap[col] : col;            // colmap[col], col < n_cols: a slot, < n_pad
    const int ray = P.perm ? P.perm[slot] : slot;               // perm [n_pad]; the caller's ray index, member-major: m n_rays + ray
    if(ray < 0 || ray >= P.n_rays) return;                      // (a slot with rows has a ray; P.n_rays = M x the fan's rays)
    double* st = Q.state + slot;                                // [GEOAC_LVL_NSTATE][n_pad]
    double tt = st[0], at = st[np], ltt = st[2 * np], lat = st[3 * np];
    int leg = (int)st[4 * np];
    const int ne = P.nlegend[col];                              // <= GEOAC_MAXLEGS (k_rk4)
    int e = 0;
    int next_end = (e < ne) ? P.legend[(size_t)e * np + col] : 0x7fffffff;
    int cur_end = -1;
    const int pw = P.pathw, cap = Q.cap;
    int* const cnt = Q.count + (size_t)ray * L;                 // [M n_rays][L]
    double* const rec = Q.rec + (size_t)ray * L * cap * GEOAC_LVL_STRIDE;      // [M n_rays][L][cap][GEOAC_LVL_STRIDE]
    int n[L];                                                   // (constant indices only: registers)
    #pragma unroll
    for(int l = 0; l < L; l++) n[l] = cnt[l];
    const double* const hcol = P.path + (size_t)Q.hidx * np + col;            // height component of row r: hcol[r pw np], hidx < pw
    const size_t rs = (size_t)pw * np;

    // the sums of segment (i, i + 1), as k_accum forms them (arrivals-only form)
    auto add_segment = [&](int i, double c_tt, double c_at){
        ltt += c_tt; lat += c_at;
        if(i + 1 == next_end){
            tt += ltt; at += lat; ltt = 0.0; lat = 0.0;
            leg++; cur_end = i + 1; e++;
            next_end = (e < ne) ? P.legend[(size_t)e * np + col] : 0x7fffffff;      // e < ne: an entry k_rk4 wrote
        }
    };
    // a crossing of level l in segment (i, i + 1), i + 1 < nr: before the segment's contribution goes into the sums
    auto emit = [&](int l, int k, int i, double dir, double ha, double hb, double lev, double c_tt, double c_at){
        if(k >= cap) return;                                    // record slot k < cap; the count runs on
        double* R = rec + ((size_t)l * cap + k) * GEOAC_LVL_STRIDE;
        const double f = (lev - ha) / (hb - ha);
        const double* a = P.path + (size_t)i * rs + col;        // rows i and i + 1 < nr
        const double* b = a + rs;
        R[GEOAC_LVL_LEG] = (double)leg; R[GEOAC_LVL_DIR] = dir; R[GEOAC_LVL_FRAC] = f;
        R[GEOAC_LVL_TTIME] = (tt + ltt) + f * c_tt;
        R[GEOAC_LVL_ATTEN] = (at + lat) + f * c_at;
        #pragma unroll
        for(int q = 0; q < 6; q++){
            double v = 0.0;
            if(q < pw){ const double pa = a[(size_t)q * np], pb = b[(size_t)q * np]; v = pa + f * (pb - pa); }       // component q < pathw
            R[GEOAC_LVL_P0 + q] = v;
        }
        R[GEOAC_LVL_RSVD] = 0.0;
    };

    double h_cur = hcol[0];                                     // row 0, the carry row (nr >= 2)
    for(int i0 = 0; i0 + 1 < nr; i0 += 8){
        // eight segments' heights and contributions fetched together (a trip to memory per row otherwise, as in k_accum's eight-row form); a
        // row beyond the column's last one is replaced by row 0 and not used
        double hn[8], c0[8], c1[8];
        #pragma unroll
        for(int j = 0; j < 8; j++){
            const int i = i0 + j;
            const bool ok = i + 1 < nr;
            hn[j] = hcol[(size_t)(ok ? i + 1 : 0) * rs];        // row i + 1 < nr
            const double* cpt = P.contrib + ((size_t)(ok ? i : 0) * 2) * np + col;      // contrib row i, i + 1 < nr
            c0[j] = cpt[0]; c1[j] = cpt[np];
        }
        // does any of them cross a level?  (The pair i == cur_end is not excluded here: the plain loop below decides.)
        bool hit = false;
        #pragma unroll
        for(int j = 0; j < 8; j++){
            const double ha = j == 0 ? h_cur : hn[j > 0 ? j - 1 : 0], hb = hn[j];
            if(i0 + j + 1 < nr){
                #pragma unroll
                for(int l = 0; l < L; l++) hit = hit || lvl_up(ha, hb, Q.lev[l]) || lvl_down(ha, hb, Q.lev[l]);
            }
        }
        if(!hit){
            #pragma unroll
            for(int j = 0; j < 8; j++){
                const int i = i0 + j;
                if(i + 1 >= nr || i == cur_end) continue;
                add_segment(i, c0[j], c1[j]);
            }
        } else {
            // the rare batch: row by row from memory, so that the record code exists once per level
            for(int i = i0; i < i0 + 8 && i + 1 < nr; i++){
                if(i == cur_end) continue;                      // (leg-end row -> next leg's start row): not a segment
                const double ha = hcol[(size_t)i * rs], hb = hcol[(size_t)(i + 1) * rs];      // rows i, i + 1 < nr
                const double* cpt = P.contrib + ((size_t)i * 2) * np + col;                   // contrib row i, i + 1 < nr
                const double c_tt = cpt[0], c_at = cpt[np];
                #pragma unroll
                for(int l = 0; l < L; l++){                     // level l < L
                    const double lev = Q.lev[l];
                    const bool up = lvl_up(ha, hb, lev), down = lvl_down(ha, hb, lev);
                    if(up || down){
                        emit(l, n[l], i, up ? 1.0 : -1.0, ha, hb, lev, c_tt, c_at);
                        n[l]++;
                    }
                }
                add_segment(i, c_tt, c_at);
            }
        }
        h_cur = hn[7];                                          // row i0 + 8 where the column has it (the loop ends otherwise)
    }
    #pragma unroll
    for(int l = 0; l < L; l++) cnt[l] = n[l];
    st[0] = tt; st[np] = at; st[2 * np] = ltt; st[3 * np] = lat; st[4 * np] = (double)leg;
}

}  // namespace

extern "C" hipError_t geoac_launch_levels(const GeoacDevParams* P, const GeoacLevelParams* Q, hipStream_t s){
    if(Q->n_levels < 1 || Q->n_levels > GEOAC_MAX_LEVELS || Q->cap < 1 || Q->cap > GEOAC_LVL_MAX_CAP || Q->hidx < 0 || Q->hidx >= P->pathw || P->pathw > 6 ||
       P->rays_form || !Q->state || !Q->rec || !Q->count) return hipErrorInvalidValue;
    dim3 b(256), g((unsigned)((P->n_cols_bound + 255) / 256));
    switch(Q->n_levels){
        case 1: hipLaunchKernelGGL(k_levels<1>, g, b, 0, s, *P, *Q); break;
        case 2: hipLaunchKernelGGL(k_levels<2>, g, b, 0, s, *P, *Q); break;
        case 3: hipLaunchKernelGGL(k_levels<3>, g, b, 0, s, *P, *Q); break;
        case 4: hipLaunchKernelGGL(k_levels<4>, g, b, 0, s, *P, *Q); break;
        case 5: hipLaunchKernelGGL(k_levels<5>, g, b, 0, s, *P, *Q); break;
        case 6: hipLaunchKernelGGL(k_levels<6>, g, b, 0, s, *P, *Q); break;
        case 7: hipLaunchKernelGGL(k_levels<7>, g, b, 0, s, *P, *Q); break;
        default: hipLaunchKernelGGL(k_levels<8>, g, b, 0, s, *P, *Q); break;
    }
    return hipGetLastError();
}

// ---- the host-only check of a level list ----
static const char* levels_fault(int eqset, const geoac_params* p, int n_levels, const double* z_km, int cap){
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(!p) return "params is NULL";
    if(n_levels < 0 || n_levels > GEOAC_MAX_LEVELS) return "n_levels must be in 0 .. 8";
    if(cap < 0 || cap > GEOAC_LVL_MAX_CAP) return "cap must be in 1 .. 64 (0: the default of 8)";
    if(n_levels > 0 && !z_km) return "z_km is NULL";
    const bool sph = (eqset == GEOAC_EQ_GLOBAL || eqset == GEOAC_EQ_GLOBAL_RNGDEP);
    const double top = sph ? p->vert_limit - p->r_earth : p->vert_limit;      // (NaN: the top node of an atmosphere not uploaded yet - no bound)
    for(int l = 0; l < n_levels; l++){
        if(!std::isfinite(z_km[l])) return "every level must be finite";
        if(l > 0 && !(z_km[l] > z_km[l - 1])) return "levels must be strictly ascending";
        if(!(z_km[l] > p->z_grnd)) return "every level must lie strictly above z_grnd";
        if(top == top && !(z_km[l] < top)) return "every level must lie below the vertical limit (spherical sets: vert_limit - r_earth)";
    }
    return nullptr;
}

extern "C" int geoac_levels_check(int eqset, const geoac_params* params, int n_levels, const double* z_km, int cap, const char** fault){
    if(fault) *fault = nullptr;
    if(eqset == GEOAC_EQ_2D){
        if(fault) *fault = "level crossings are not available for the 2-D set (its sums always take the sample-capture form)";
        return GEOAC_E_UNSUPPORTED;
    }
    const char* f = levels_fault(eqset, params, n_levels, z_km, cap);
    if(fault) *fault = f;
    return f ? GEOAC_E_INVALID : GEOAC_OK;
}
