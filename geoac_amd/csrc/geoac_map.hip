// geoac_map.hip - arrival maps (include/geoac_map.h): the record table of the last completed launch binned on a regular grid, on the device.
//
// Reads the record table and, with a frequency set, the attenuation table; writes only buffers of its own.  No kernel of the launch plan is
// involved, so every equation set is served alike.  Every reduction is an integer atomic - u64 adds for the counts, u64 min / max on the
// order-preserving key of a double for the extrema, u64 min on the arrival index for BEST - so the result does not depend on the order the
// arrivals are seen in: a map is the same bits on every run and equals a host restatement that reduces by the same keys (tests/map_reference.py).
// No floating-point value is ever added to another here.
//
// The cell arithmetic is fixed: degrees = rad * 180.0 / Pi (one multiply, one divide), q = floor((c - origin) / step) (one subtract, one
// divide).  None of it is a multiply-add, so contraction cannot alter it.  The longitude wrap lon - 360.0 * floor((lon - origin) / 360.0) has a
// product, but of 360 and a small integer: it is exact, and a fused form rounds the same value once, as the separate subtraction does.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <string>

#include "../../include/geoac_map.h"
#include "geoac_launch_int.h"

namespace {

const double kMapPi = 3.141592653589793238462643;

struct MapDev {
    const double* rec; const double* atten;       // the launch's tables (atten: NULL at F == 1)
    double* level; int* cell;                     // [M][F][n_rays][legs]; [M][n_rays][legs]: cell of the arrival, -1 filtered out or outside
    unsigned long long *count, *ttime, *cel, *lvl, *best, *outside;
    unsigned* detect;
    double o0, o1, s0, s1, turn_min, turn_max, detect_db;
    int n0, n1, wrap, leg_min, leg_max;
    int kind;                                     // 0 spherical (lat, lon in degrees), 1 Cartesian 3-D (x, y), 2 the 2-D set (range)
    int M, F, n_rays, legs, calc_amp;
    long long cells;
};

// a layer allocation (GeoacLayers) as k_map_finish and k_map_detect read it
struct LayersDev {
    unsigned long long *count, *ttime, *cel, *lvl, *best;
    unsigned* detect;
    double detect_db;
    long long cells;
    int M, F;
};

// initial values of the layers, which lie back to back in one allocation: COUNT 0 | TTIME key ~0 | CEL key 0 | LEVEL key 0 | BEST max | tail 0 | DETECT 0
__global__ void k_map_fill(unsigned long long* w, long long n_mc, long long n_mfc, long long n_words){
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride){
        unsigned long long v = 0;
        if(i >= n_mc && i < 2 * n_mc) v = ~0ull;
        else if(i >= 3 * n_mc + n_mfc && i < 3 * n_mc + 2 * n_mfc) v = 0x7fffffffffffffffull;
        w[i] = v;
    }
}

// one thread per (m, f, ray, leg): the level of the arrival, NaN where the leg wrote no row
__global__ void k_map_level(MapDev D){
    const long long per_m = (long long)D.n_rays * D.legs, n = per_m * D.M * D.F;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride){
        const long long rl = i % per_m, mf = i / per_m;
        const int f = (int)(mf % D.F);
        const long long m = mf / D.F;
        const double* R = D.rec + (m * per_m + rl) * GEOAC_REC_STRIDE;
        double lv = __longlong_as_double(0x7ff8000000000000ll);
        if(R[GEOAC_REC_VALID] != 0.0){
            const double att = D.atten ? D.atten[f * per_m + rl] : R[GEOAC_REC_ATTEN];
            const double amp_db = D.calc_amp ? 20.0 * log10(R[GEOAC_REC_AMP]) : 0.0;
            lv = amp_db - att;
        }
        D.level[i] = lv;
    }
}

// one thread per (m, ray, leg): filters, cell, and every reduction of the arrival
__global__ void k_map_bin(MapDev D){
    const long long per_m = (long long)D.n_rays * D.legs, n = per_m * D.M;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride){
        const double* R = D.rec + r * GEOAC_REC_STRIDE;
        const long long m = r / per_m, rl = r % per_m;
        const int leg = (int)(rl % D.legs);
        int cell = -1;
        const double turn = R[GEOAC_REC_TURN];
        if(R[GEOAC_REC_VALID] != 0.0 && leg >= D.leg_min && leg <= D.leg_max && turn >= D.turn_min && turn < D.turn_max){
            double c0, c1 = 0.0;
            if(D.kind == 0){
                c0 = R[GEOAC_REC_STATE + 1] * 180.0 / kMapPi;
                c1 = R[GEOAC_REC_STATE + 2] * 180.0 / kMapPi;
                if(D.wrap) c1 = c1 - 360.0 * floor((c1 - D.o1) / 360.0);
            } else {
                c0 = R[GEOAC_REC_STATE + 0];
                if(D.kind == 1) c1 = R[GEOAC_REC_STATE + 1];
            }
            const double q0 = floor((c0 - D.o0) / D.s0);
            const double q1 = D.kind == 2 ? 0.0 : floor((c1 - D.o1) / D.s1);
            if(q0 >= 0.0 && q0 < (double)D.n0 && q1 >= 0.0 && q1 < (double)D.n1){
                cell = (int)q0 * D.n1 + (int)q1;
                const long long b = m * D.cells + cell;
                const double tt = R[GEOAC_REC_TTIME];
                atomicAdd(&D.count[b], 1ull);
                atomicMin(&D.ttime[b], geoac_key(tt));
                atomicMax(&D.cel[b], geoac_key(R[GEOAC_REC_RANGE] / tt));
                for(int f = 0; f < D.F; f++){
                    const double lv = D.level[(m * D.F + f) * per_m + rl];
                    if(isfinite(lv)) atomicMax(&D.lvl[(m * D.F + f) * D.cells + cell], geoac_key(lv));
                }
            } else atomicAdd(&D.outside[m], 1ull);
        }
        D.cell[r] = cell;
    }
}

// one thread per (m, f, ray, leg): the arrivals that hold their cell's LEVEL_MAX compete for BEST with their index, the smallest wins
__global__ void k_map_best(MapDev D){
    const long long per_m = (long long)D.n_rays * D.legs, n = per_m * D.M * D.F;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride){
        const long long rl = i % per_m, mf = i / per_m, m = mf / D.F;
        const int cell = D.cell[m * per_m + rl];
        if(cell < 0) continue;
        const double lv = D.level[i];
        if(!isfinite(lv)) continue;
        const long long b = mf * D.cells + cell;
        if(D.lvl[b] == geoac_key(lv)) atomicMin(&D.best[b], (unsigned long long)rl);
    }
}

// one thread per (m, f, cell): keys back to doubles in place, empty-cell markers
__global__ void k_map_finish(LayersDev D){
    const long long n = D.cells * D.M * D.F;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const unsigned long long p_inf = 0x7ff0000000000000ull, m_inf = 0xfff0000000000000ull;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride){
        const unsigned long long k = D.lvl[i];
        if(k == 0ull){ D.lvl[i] = m_inf; D.best[i] = ~0ull; }
        else D.lvl[i] = (unsigned long long)__double_as_longlong(geoac_unkey(k));
        const long long c = i % D.cells, mf = i / D.cells;
        if(mf % D.F == 0){
            const long long b = (mf / D.F) * D.cells + c;
            const bool any = D.count[b] != 0ull;
            D.ttime[b] = any ? (unsigned long long)__double_as_longlong(geoac_unkey(D.ttime[b])) : p_inf;
            D.cel[b] = any ? (unsigned long long)__double_as_longlong(geoac_unkey(D.cel[b])) : m_inf;
        }
    }
}

// one thread per (f, cell): members whose LEVEL_MAX reaches detect_db
__global__ void k_map_detect(LayersDev D){
    const long long n = D.cells * D.F;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride){
        const long long c = i % D.cells, f = i / D.cells;
        unsigned hits = 0;
        for(int m = 0; m < D.M; m++){
            const double lv = __longlong_as_double((long long)D.lvl[((long long)m * D.F + f) * D.cells + c]);
            hits += lv >= D.detect_db ? 1u : 0u;
        }
        D.detect[i] = hits;
    }
}

struct MapState {
    GeoacLayers L{};                                     // tail: outside[M]
    double* level = nullptr; size_t level_cap = 0;
    int* cell = nullptr; size_t cell_cap = 0;
    unsigned long long map_gen = 0, level_gen = 0;       // the context's invalidation counter they were made at (0: never)
    geoac_map_spec spec{};
    EventPair ev;
};

// the first thing wrong with a spec, or NULL
const char* spec_fault(int eqset, const geoac_map_spec* s){
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(!s) return "spec is NULL";
    if(const char* f = geoac_grid_fault(eqset, s->origin, s->step, s->n, s->wrap_lon, s->turn_min, s->turn_max)) return f;
    if(eqset == GEOAC_EQ_2D && s->n[1] != 1) return "the 2-D set has one axis (range): n[1] must be 1";
    if(s->leg_min < 0 || s->leg_max < s->leg_min) return "legs: need 0 <= leg_min <= leg_max";
    return nullptr;
}

struct Bound { geoac_ctx* ctx; GeoacMapView v; MapState* st; };

// view of the context + its map state (created on first use); `what` names the caller in messages
int bind(geoac_ctx* ctx, const char* what, bool create, Bound* b){
    GeoacLaunchView lv;
    int rc = bind_launch(ctx, what, GEOAC_SLOT_MAP, &lv);
    if(rc) return rc;
    b->ctx = ctx; b->v = lv.map;
    if(!*lv.state && create) *lv.state = new MapState();
    b->st = (MapState*)*lv.state;
    return GEOAC_OK;
}

void fill_dev(const Bound& b, MapDev* D){
    const GeoacMapView& v = b.v; MapState* st = b.st;
    *D = MapDev{};
    D->rec = v.rec; D->atten = v.atten; D->level = st->level; D->cell = st->cell;
    D->M = v.M; D->F = v.F; D->n_rays = v.n_rays; D->legs = v.legs; D->calc_amp = v.calc_amp;
    D->kind = spherical(v.eqset) ? 0 : (v.eqset == GEOAC_EQ_2D ? 2 : 1);
}

// the level table of the launch, formed once per launch
int ensure_level(Bound& b, const char* what){
    MapState* st = b.st; const GeoacMapView& v = b.v;
    if(st->level_gen == v.gen) return GEOAC_OK;
    const long long n = (long long)v.M * v.F * v.n_rays * v.legs;
    if(grow((void**)&st->level, &st->level_cap, sizeof(double) * (size_t)n))
        return geoac_map_fail(b.ctx, GEOAC_E_NOMEM, (std::string(what) + ": no device memory for the level table").c_str());
    MapDev D; fill_dev(b, &D);
    hipLaunchKernelGGL(k_map_level, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)v.stream, D);
    GEOAC_CHK(what, hipGetLastError());
    st->level_gen = v.gen;
    return GEOAC_OK;
}

// a current map, or GEOAC_E_INVALID
int bind_map(geoac_ctx* ctx, const char* what, Bound* b){
    int rc = bind(ctx, what, false, b);
    if(rc) return rc;
    if(!b->st || b->st->map_gen != b->v.gen)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no map of the last completed launch (call geoac_fan_map after geoac_fan_launch)").c_str());
    return GEOAC_OK;
}

LayersDev layers_dev(const GeoacLayers* L, double detect_db){
    LayersDev D{};
    char* base = (char*)L->base;
    size_t off, bytes;
    geoac_layers_span(L, GEOAC_MAP_COUNT, &off, &bytes);     D.count = (unsigned long long*)(base + off);
    geoac_layers_span(L, GEOAC_MAP_TTIME_MIN, &off, &bytes); D.ttime = (unsigned long long*)(base + off);
    geoac_layers_span(L, GEOAC_MAP_CEL_MAX, &off, &bytes);   D.cel = (unsigned long long*)(base + off);
    geoac_layers_span(L, GEOAC_MAP_LEVEL_MAX, &off, &bytes); D.lvl = (unsigned long long*)(base + off);
    geoac_layers_span(L, GEOAC_MAP_BEST, &off, &bytes);      D.best = (unsigned long long*)(base + off);
    geoac_layers_detect_span(L, &off, &bytes);               D.detect = (unsigned*)(base + off);
    D.detect_db = detect_db; D.cells = L->cells; D.M = L->M; D.F = L->F;
    return D;
}

}  // namespace

// ---- the layer allocation (geoac_map_int.h), for geoac_tubemap.hip as well ----
void geoac_layers_span(const GeoacLayers* L, int layer, size_t* off, size_t* bytes){
    const size_t mc = (size_t)L->M * (size_t)L->cells * 8, mfc = mc * (size_t)L->F;
    switch(layer){
    case GEOAC_MAP_COUNT:     *off = 0;            *bytes = mc;  break;
    case GEOAC_MAP_TTIME_MIN: *off = mc;           *bytes = mc;  break;
    case GEOAC_MAP_CEL_MAX:   *off = 2 * mc;       *bytes = mc;  break;
    case GEOAC_MAP_LEVEL_MAX: *off = 3 * mc;       *bytes = mfc; break;
    default:                  *off = 3 * mc + mfc; *bytes = mfc; break;
    }
}
void geoac_layers_tail_span(const GeoacLayers* L, size_t* off, size_t* bytes){
    size_t o, n;
    geoac_layers_span(L, GEOAC_MAP_BEST, &o, &n);
    *off = o + n; *bytes = (size_t)L->tail_words * 8;
}
void geoac_layers_detect_span(const GeoacLayers* L, size_t* off, size_t* bytes){
    size_t o, n;
    geoac_layers_tail_span(L, &o, &n);
    *off = o + n; *bytes = (size_t)L->F * (size_t)L->cells * 4;
}
size_t geoac_layers_bytes(const GeoacLayers* L){
    size_t off, n;
    geoac_layers_detect_span(L, &off, &n);
    return off + ((n + 7) & ~(size_t)7);
}
int geoac_layers_grow(GeoacLayers* L){ return grow(&L->base, &L->cap, geoac_layers_bytes(L)); }

void geoac_layers_fill(const GeoacLayers* L, void* stream){
    const long long n_mc = (long long)L->M * L->cells, n_mfc = n_mc * L->F, n_words = (long long)(geoac_layers_bytes(L) / 8);
    hipLaunchKernelGGL(k_map_fill, dim3(blocks_for(n_words, 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)L->base, n_mc, n_mfc, n_words);
}
void geoac_layers_finish(const GeoacLayers* L, void* stream){
    hipLaunchKernelGGL(k_map_finish, dim3(blocks_for((long long)L->M * L->F * L->cells, 256)), dim3(256), 0, (hipStream_t)stream, layers_dev(L, 0.0));
}
void geoac_layers_detect(const GeoacLayers* L, double detect_db, void* stream){
    hipLaunchKernelGGL(k_map_detect, dim3(blocks_for(L->cells * L->F, 256)), dim3(256), 0, (hipStream_t)stream, layers_dev(L, detect_db));
}

static int fetch_span(geoac_ctx* ctx, const char* what, const GeoacLayers* L, void* stream, void* host, size_t off, size_t bytes){
    hipError_t e = hipMemcpyAsync(host, (const char*)L->base + off, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if(e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? GEOAC_OK : hip_fail(ctx, what, e);
}

int geoac_layers_dev(geoac_ctx* ctx, const char* what, const GeoacLayers* L, int layer, void** dev_ptr, size_t* bytes){
    if(layer < 0 || layer >= GEOAC_MAP_LAYERS) return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": unknown layer").c_str());
    size_t off, n;
    geoac_layers_span(L, layer, &off, &n);
    if(dev_ptr) *dev_ptr = (char*)L->base + off;
    if(bytes) *bytes = n;
    return GEOAC_OK;
}
int geoac_layers_fetch(geoac_ctx* ctx, const char* what, const GeoacLayers* L, void* stream, int layer, void* host){
    if(layer < 0 || layer >= GEOAC_MAP_LAYERS || !host) return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": unknown layer / NULL buffer").c_str());
    size_t off, n;
    geoac_layers_span(L, layer, &off, &n);
    return fetch_span(ctx, what, L, stream, host, off, n);
}
int geoac_layers_fetch_detect(geoac_ctx* ctx, const char* what, const char* noun, const GeoacLayers* L, void* stream, uint32_t* host){
    if(!host) return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": NULL buffer").c_str());
    if(!L->detect) return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": the " + noun + " was made without a detection threshold (detect_db = NaN)").c_str());
    size_t off, n;
    geoac_layers_detect_span(L, &off, &n);
    return fetch_span(ctx, what, L, stream, host, off, n);
}
int geoac_layers_fetch_tail(geoac_ctx* ctx, const char* what, const GeoacLayers* L, void* stream, void* host){
    if(!host) return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": NULL buffer").c_str());
    size_t off, n;
    geoac_layers_tail_span(L, &off, &n);
    return fetch_span(ctx, what, L, stream, host, off, n);
}

// ---- the grid and the turning-height band of a spec, for geoac_tubemap.hip as well ----
const char* geoac_grid_fault(int eqset, const double origin[2], const double step[2], const int n[2], int wrap_lon, double turn_min, double turn_max){
    for(int a = 0; a < 2; a++){
        if(!std::isfinite(origin[a])) return "origin must be finite";
        if(!std::isfinite(step[a]) || !(step[a] > 0.0)) return "step must be finite and greater than 0";
        if(n[a] < 1) return "n must be at least 1 per axis";
    }
    if((long long)n[0] * n[1] > (long long)GEOAC_MAP_MAX_CELLS) return "n[0] * n[1] exceeds GEOAC_MAP_MAX_CELLS (2^24)";
    if(wrap_lon != 0 && wrap_lon != 1) return "wrap_lon must be 0 or 1";
    if(wrap_lon && !spherical(eqset)) return "wrap_lon is for the spherical sets only (a Cartesian set has no longitude)";
    if(std::isnan(turn_min) || std::isnan(turn_max) || !(turn_min < turn_max)) return "turning-height band: need turn_min < turn_max, neither NaN (-inf / +inf: no bound)";
    return nullptr;
}

extern "C" void geoac_map_release(void* state){
    MapState* st = (MapState*)state;
    if(!st) return;
    if(st->L.base) hipFree(st->L.base);
    if(st->level) hipFree(st->level);
    if(st->cell) hipFree(st->cell);
    st->ev.release();
    delete st;
}

extern "C" int geoac_map_check(int eqset, const geoac_map_spec* spec, int64_t* cells){
    if(spec_fault(eqset, spec)) return GEOAC_E_INVALID;
    if(cells) *cells = (int64_t)spec->n[0] * spec->n[1];
    return GEOAC_OK;
}

extern "C" int geoac_fan_map(geoac_ctx* ctx, const geoac_map_spec* spec){
    const char* what = "fan_map";
    Bound b;
    int rc = bind(ctx, what, true, &b);
    if(rc) return rc;
    if(const char* fault = spec_fault(b.v.eqset, spec)) return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string("fan_map: ") + fault).c_str());
    MapState* st = b.st; const GeoacMapView& v = b.v;
    hipStream_t s = (hipStream_t)v.stream;
    st->map_gen = 0;                                   // (no current map until this one is complete)
    GEOAC_CHK(what, st->ev.start(s));
    if((rc = ensure_level(b, what))) return rc;
    st->spec = *spec;
    GeoacLayers& L = st->L;
    L.M = v.M; L.F = v.F; L.cells = (long long)spec->n[0] * spec->n[1]; L.tail_words = v.M; L.detect = !std::isnan(spec->detect_db);
    const long long n_rec = (long long)v.M * v.n_rays * v.legs;
    if(geoac_layers_grow(&L) || grow((void**)&st->cell, &st->cell_cap, sizeof(int) * (size_t)n_rec))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_map: no device memory for the layers (" + std::to_string(geoac_layers_bytes(&L) >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(v.F) + " frequencies x " + std::to_string(L.cells) + " cells)").c_str());
    MapDev D; fill_dev(b, &D);
    const LayersDev P = layers_dev(&L, spec->detect_db);
    D.count = P.count; D.ttime = P.ttime; D.cel = P.cel; D.lvl = P.lvl; D.best = P.best; D.detect = P.detect;
    size_t off, bytes;
    geoac_layers_tail_span(&L, &off, &bytes);          D.outside = (unsigned long long*)((char*)L.base + off);
    D.o0 = spec->origin[0]; D.o1 = spec->origin[1]; D.s0 = spec->step[0]; D.s1 = spec->step[1]; D.n0 = spec->n[0]; D.n1 = spec->n[1];
    D.wrap = spec->wrap_lon; D.leg_min = spec->leg_min; D.leg_max = spec->leg_max; D.turn_min = spec->turn_min; D.turn_max = spec->turn_max;
    D.detect_db = spec->detect_db; D.cells = L.cells;
    geoac_layers_fill(&L, s);
    hipLaunchKernelGGL(k_map_bin, dim3(blocks_for(n_rec, 256)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(k_map_best, dim3(blocks_for(n_rec * v.F, 256)), dim3(256), 0, s, D);
    geoac_layers_finish(&L, s);
    if(L.detect) geoac_layers_detect(&L, spec->detect_db, s);
    GEOAC_CHK(what, hipGetLastError());
    GEOAC_CHK(what, st->ev.stop(s));
    st->map_gen = v.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_map_shape(geoac_ctx* ctx, int* n_members, int* n_freq, int* n0, int* n1){
    Bound b;
    int rc = bind_map(ctx, "fan_map_shape", &b);
    if(rc) return rc;
    if(n_members) *n_members = b.st->L.M;
    if(n_freq) *n_freq = b.st->L.F;
    if(n0) *n0 = b.st->spec.n[0];
    if(n1) *n1 = b.st->spec.n[1];
    return GEOAC_OK;
}

extern "C" int geoac_fan_map_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_map(ctx, "fan_map_dev", &b);
    return rc ? rc : geoac_layers_dev(ctx, "fan_map_dev", &b.st->L, layer, dev_ptr, bytes);
}

extern "C" int geoac_fan_map_fetch(geoac_ctx* ctx, int layer, void* host){
    Bound b;
    int rc = bind_map(ctx, "fan_map_fetch", &b);
    return rc ? rc : geoac_layers_fetch(ctx, "fan_map_fetch", &b.st->L, b.v.stream, layer, host);
}

extern "C" int geoac_fan_map_fetch_detect(geoac_ctx* ctx, uint32_t* detect_host){
    Bound b;
    int rc = bind_map(ctx, "fan_map_fetch_detect", &b);
    return rc ? rc : geoac_layers_fetch_detect(ctx, "fan_map_fetch_detect", "map", &b.st->L, b.v.stream, detect_host);
}

extern "C" int geoac_fan_map_outside(geoac_ctx* ctx, uint64_t* outside_host){
    Bound b;
    int rc = bind_map(ctx, "fan_map_outside", &b);
    return rc ? rc : geoac_layers_fetch_tail(ctx, "fan_map_outside", &b.st->L, b.v.stream, outside_host);
}

extern "C" int geoac_fan_map_timing(geoac_ctx* ctx, double* ms){
    Bound b;
    int rc = bind_map(ctx, "fan_map_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_map_timing: NULL argument");
    GEOAC_CHK("fan_map_timing", b.st->ev.ms(ms));
    return GEOAC_OK;
}

extern "C" int geoac_fan_level_dev(geoac_ctx* ctx, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind(ctx, "fan_level_dev", true, &b);
    if(rc) return rc;
    if((rc = ensure_level(b, "fan_level_dev"))) return rc;
    if(dev_ptr) *dev_ptr = b.st->level;
    if(bytes) *bytes = sizeof(double) * (size_t)b.v.M * b.v.F * b.v.n_rays * b.v.legs;
    return GEOAC_OK;
}

extern "C" int geoac_fan_fetch_level(geoac_ctx* ctx, double* level_host){
    Bound b;
    int rc = bind(ctx, "fan_fetch_level", true, &b);
    if(rc) return rc;
    if(!level_host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_fetch_level: NULL buffer");
    if((rc = ensure_level(b, "fan_fetch_level"))) return rc;
    const size_t n = sizeof(double) * (size_t)b.v.M * b.v.F * b.v.n_rays * b.v.legs;
    GEOAC_CHK("fan_fetch_level", hipMemcpyAsync(level_host, b.st->level, n, hipMemcpyDeviceToHost, (hipStream_t)b.v.stream));
    GEOAC_CHK("fan_fetch_level", hipStreamSynchronize((hipStream_t)b.v.stream));
    return GEOAC_OK;
}
