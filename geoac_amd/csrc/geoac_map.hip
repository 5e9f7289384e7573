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
#include "geoac_map_int.h"

namespace {

const double kMapPi = 3.141592653589793238462643;
const unsigned long long kSign = 0x8000000000000000ull;

// order-preserving key of a double: a < b as doubles (and -0 < +0) <=> key(a) < key(b) as unsigned integers
__device__ inline unsigned long long map_key(double v){
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | kSign);
}
__device__ inline double map_unkey(unsigned long long k){
    return __longlong_as_double((long long)((k >> 63) ? (k & ~kSign) : ~k));
}

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

// initial values of the layers, which lie back to back in one allocation: COUNT 0 | TTIME key ~0 | CEL key 0 | LEVEL key 0 | BEST max | outside 0 | DETECT 0
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
                atomicMin(&D.ttime[b], map_key(tt));
                atomicMax(&D.cel[b], map_key(R[GEOAC_REC_RANGE] / tt));
                for(int f = 0; f < D.F; f++){
                    const double lv = D.level[(m * D.F + f) * per_m + rl];
                    if(isfinite(lv)) atomicMax(&D.lvl[(m * D.F + f) * D.cells + cell], map_key(lv));
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
        if(D.lvl[b] == map_key(lv)) atomicMin(&D.best[b], (unsigned long long)rl);
    }
}

// one thread per (m, f, cell): keys back to doubles in place, empty-cell markers
__global__ void k_map_finish(MapDev D){
    const long long n = D.cells * D.M * D.F;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const unsigned long long p_inf = 0x7ff0000000000000ull, m_inf = 0xfff0000000000000ull;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride){
        const unsigned long long k = D.lvl[i];
        if(k == 0ull){ D.lvl[i] = m_inf; D.best[i] = ~0ull; }
        else D.lvl[i] = (unsigned long long)__double_as_longlong(map_unkey(k));
        const long long c = i % D.cells, mf = i / D.cells;
        if(mf % D.F == 0){
            const long long b = (mf / D.F) * D.cells + c;
            const bool any = D.count[b] != 0ull;
            D.ttime[b] = any ? (unsigned long long)__double_as_longlong(map_unkey(D.ttime[b])) : p_inf;
            D.cel[b] = any ? (unsigned long long)__double_as_longlong(map_unkey(D.cel[b])) : m_inf;
        }
    }
}

// one thread per (f, cell): members whose LEVEL_MAX reaches detect_db
__global__ void k_map_detect(MapDev D){
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
    void* layers = nullptr; size_t layers_cap = 0;
    double* level = nullptr; size_t level_cap = 0;
    int* cell = nullptr; size_t cell_cap = 0;
    unsigned long long map_gen = 0, level_gen = 0;       // the context's invalidation counter they were made at (0: never)
    geoac_map_spec spec{};
    int M = 0, F = 0, n_rays = 0, legs = 0;
    long long cells = 0;
    bool detect = false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    size_t mc() const { return (size_t)M * (size_t)cells; }
    size_t mfc() const { return mc() * (size_t)F; }
};

unsigned blocks_for(long long n){ long long b = (n + 255) / 256; if(b < 1) b = 1; if(b > (1ll << 20)) b = 1ll << 20; return (unsigned)b; }

int grow(void** p, size_t* cap, size_t need){
    if(*p && *cap >= need) return GEOAC_OK;
    if(*p){ hipFree(*p); *p = nullptr; *cap = 0; }                  // (hipFree waits for the work that may still read it)
    if(hipMalloc(p, need) != hipSuccess){ (void)hipGetLastError(); *p = nullptr; return GEOAC_E_NOMEM; }
    *cap = need;
    return GEOAC_OK;
}

bool spherical(int eqset){ return eqset == GEOAC_EQ_GLOBAL || eqset == GEOAC_EQ_GLOBAL_RNGDEP; }

// the first thing wrong with a spec, or NULL
const char* spec_fault(int eqset, const geoac_map_spec* s){
    if(eqset < GEOAC_EQ_2D || eqset > GEOAC_EQ_GLOBAL_RNGDEP) return "unknown equation set";
    if(!s) return "spec is NULL";
    for(int a = 0; a < 2; a++){
        if(!std::isfinite(s->origin[a])) return "origin must be finite";
        if(!std::isfinite(s->step[a]) || !(s->step[a] > 0.0)) return "step must be finite and greater than 0";
        if(s->n[a] < 1) return "n must be at least 1 per axis";
    }
    if((long long)s->n[0] * s->n[1] > (long long)GEOAC_MAP_MAX_CELLS) return "n[0] * n[1] exceeds GEOAC_MAP_MAX_CELLS (2^24)";
    if(eqset == GEOAC_EQ_2D && s->n[1] != 1) return "the 2-D set has one axis (range): n[1] must be 1";
    if(s->wrap_lon != 0 && s->wrap_lon != 1) return "wrap_lon must be 0 or 1";
    if(s->wrap_lon && !spherical(eqset)) return "wrap_lon is for the spherical sets only (a Cartesian set has no longitude)";
    if(s->leg_min < 0 || s->leg_max < s->leg_min) return "legs: need 0 <= leg_min <= leg_max";
    if(std::isnan(s->turn_min) || std::isnan(s->turn_max) || !(s->turn_min < s->turn_max)) return "turning-height band: need turn_min < turn_max, neither NaN (-inf / +inf: no bound)";
    return nullptr;
}

struct Bound { geoac_ctx* ctx; GeoacMapView v; MapState* st; };

// view of the context + its map state (created on first use); `what` names the caller in messages
int bind(geoac_ctx* ctx, const char* what, bool create, Bound* b){
    if(!ctx) return GEOAC_E_INVALID;
    b->ctx = ctx;
    int rc = geoac_map_view(ctx, &b->v);
    if(rc) return rc;
    if(!b->v.fresh)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no completed launch, or new angles, an atmosphere upload, geoac_set_sources or "
                                                     "geoac_set_frequencies have come since it (launch again)").c_str());
    if(!*b->v.state && create) *b->v.state = new MapState();
    b->st = (MapState*)*b->v.state;
    if(hipSetDevice(b->v.device) != hipSuccess) return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": hipSetDevice failed").c_str());
    return GEOAC_OK;
}

int hip_fail(geoac_ctx* ctx, const char* what, hipError_t e){
    return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}
#define MAPCHK(what, call) do { hipError_t e_ = (call); if(e_ != hipSuccess) return hip_fail(b.ctx, what, e_); } while(0)

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
    hipLaunchKernelGGL(k_map_level, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)v.stream, D);
    MAPCHK(what, hipGetLastError());
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

// byte offset and size of a layer inside the allocation
void layer_span(const MapState* st, int layer, size_t* off, size_t* bytes){
    const size_t mc = st->mc() * 8, mfc = st->mfc() * 8;
    switch(layer){
    case GEOAC_MAP_COUNT:     *off = 0;            *bytes = mc;  break;
    case GEOAC_MAP_TTIME_MIN: *off = mc;           *bytes = mc;  break;
    case GEOAC_MAP_CEL_MAX:   *off = 2 * mc;       *bytes = mc;  break;
    case GEOAC_MAP_LEVEL_MAX: *off = 3 * mc;       *bytes = mfc; break;
    default:                  *off = 3 * mc + mfc; *bytes = mfc; break;
    }
}
size_t outside_off(const MapState* st){ return 3 * st->mc() * 8 + 2 * st->mfc() * 8; }
size_t detect_off(const MapState* st){ return outside_off(st) + (size_t)st->M * 8; }
size_t detect_bytes(const MapState* st){ return (size_t)st->F * (size_t)st->cells * 4; }

int fetch(Bound& b, const char* what, void* host, size_t off, size_t bytes){
    MAPCHK(what, hipMemcpyAsync(host, (const char*)b.st->layers + off, bytes, hipMemcpyDeviceToHost, (hipStream_t)b.v.stream));
    MAPCHK(what, hipStreamSynchronize((hipStream_t)b.v.stream));
    return GEOAC_OK;
}

}  // namespace

extern "C" void geoac_map_release(void* state){
    MapState* st = (MapState*)state;
    if(!st) return;
    if(st->layers) hipFree(st->layers);
    if(st->level) hipFree(st->level);
    if(st->cell) hipFree(st->cell);
    if(st->e0) hipEventDestroy(st->e0);
    if(st->e1) hipEventDestroy(st->e1);
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
    if(!st->e0){ MAPCHK(what, hipEventCreate(&st->e0)); MAPCHK(what, hipEventCreate(&st->e1)); }
    MAPCHK(what, hipEventRecord(st->e0, s));
    if((rc = ensure_level(b, what))) return rc;
    st->spec = *spec; st->M = v.M; st->F = v.F; st->n_rays = v.n_rays; st->legs = v.legs;
    st->cells = (long long)spec->n[0] * spec->n[1];
    st->detect = !std::isnan(spec->detect_db);
    const long long n_rec = (long long)v.M * v.n_rays * v.legs;
    const size_t need = detect_off(st) + ((detect_bytes(st) + 7) & ~(size_t)7);
    if(grow(&st->layers, &st->layers_cap, need) || grow((void**)&st->cell, &st->cell_cap, sizeof(int) * (size_t)n_rec))
        return geoac_map_fail(ctx, GEOAC_E_NOMEM, ("fan_map: no device memory for the layers (" + std::to_string(need >> 20) + " MiB for " + std::to_string(v.M) + " members x " +
                                                   std::to_string(v.F) + " frequencies x " + std::to_string(st->cells) + " cells)").c_str());
    MapDev D; fill_dev(b, &D);
    char* base = (char*)st->layers;
    size_t off, bytes;
    layer_span(st, GEOAC_MAP_COUNT, &off, &bytes);     D.count = (unsigned long long*)(base + off);
    layer_span(st, GEOAC_MAP_TTIME_MIN, &off, &bytes); D.ttime = (unsigned long long*)(base + off);
    layer_span(st, GEOAC_MAP_CEL_MAX, &off, &bytes);   D.cel = (unsigned long long*)(base + off);
    layer_span(st, GEOAC_MAP_LEVEL_MAX, &off, &bytes); D.lvl = (unsigned long long*)(base + off);
    layer_span(st, GEOAC_MAP_BEST, &off, &bytes);      D.best = (unsigned long long*)(base + off);
    D.outside = (unsigned long long*)(base + outside_off(st));
    D.detect = (unsigned*)(base + detect_off(st));
    D.o0 = spec->origin[0]; D.o1 = spec->origin[1]; D.s0 = spec->step[0]; D.s1 = spec->step[1]; D.n0 = spec->n[0]; D.n1 = spec->n[1];
    D.wrap = spec->wrap_lon; D.leg_min = spec->leg_min; D.leg_max = spec->leg_max; D.turn_min = spec->turn_min; D.turn_max = spec->turn_max;
    D.detect_db = spec->detect_db; D.cells = st->cells;
    const long long n_mc = (long long)st->mc(), n_mfc = (long long)st->mfc(), n_words = (long long)(need / 8);
    hipLaunchKernelGGL(k_map_fill, dim3(blocks_for(n_words)), dim3(256), 0, s, (unsigned long long*)st->layers, n_mc, n_mfc, n_words);
    hipLaunchKernelGGL(k_map_bin, dim3(blocks_for(n_rec)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(k_map_best, dim3(blocks_for(n_rec * v.F)), dim3(256), 0, s, D);
    hipLaunchKernelGGL(k_map_finish, dim3(blocks_for(n_mfc)), dim3(256), 0, s, D);
    if(st->detect) hipLaunchKernelGGL(k_map_detect, dim3(blocks_for(st->cells * v.F)), dim3(256), 0, s, D);
    MAPCHK(what, hipGetLastError());
    MAPCHK(what, hipEventRecord(st->e1, s));
    st->map_gen = v.gen;
    return GEOAC_OK;
}

extern "C" int geoac_fan_map_shape(geoac_ctx* ctx, int* n_members, int* n_freq, int* n0, int* n1){
    Bound b;
    int rc = bind_map(ctx, "fan_map_shape", &b);
    if(rc) return rc;
    if(n_members) *n_members = b.st->M;
    if(n_freq) *n_freq = b.st->F;
    if(n0) *n0 = b.st->spec.n[0];
    if(n1) *n1 = b.st->spec.n[1];
    return GEOAC_OK;
}

extern "C" int geoac_fan_map_dev(geoac_ctx* ctx, int layer, void** dev_ptr, size_t* bytes){
    Bound b;
    int rc = bind_map(ctx, "fan_map_dev", &b);
    if(rc) return rc;
    if(layer < 0 || layer >= GEOAC_MAP_LAYERS) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_map_dev: unknown layer");
    size_t off, n;
    layer_span(b.st, layer, &off, &n);
    if(dev_ptr) *dev_ptr = (char*)b.st->layers + off;
    if(bytes) *bytes = n;
    return GEOAC_OK;
}

extern "C" int geoac_fan_map_fetch(geoac_ctx* ctx, int layer, void* host){
    Bound b;
    int rc = bind_map(ctx, "fan_map_fetch", &b);
    if(rc) return rc;
    if(layer < 0 || layer >= GEOAC_MAP_LAYERS || !host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_map_fetch: unknown layer / NULL buffer");
    size_t off, n;
    layer_span(b.st, layer, &off, &n);
    return fetch(b, "fan_map_fetch", host, off, n);
}

extern "C" int geoac_fan_map_fetch_detect(geoac_ctx* ctx, uint32_t* detect_host){
    Bound b;
    int rc = bind_map(ctx, "fan_map_fetch_detect", &b);
    if(rc) return rc;
    if(!detect_host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_map_fetch_detect: NULL buffer");
    if(!b.st->detect) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_map_fetch_detect: the map was made without a detection threshold (detect_db = NaN)");
    return fetch(b, "fan_map_fetch_detect", detect_host, detect_off(b.st), detect_bytes(b.st));
}

extern "C" int geoac_fan_map_outside(geoac_ctx* ctx, uint64_t* outside_host){
    Bound b;
    int rc = bind_map(ctx, "fan_map_outside", &b);
    if(rc) return rc;
    if(!outside_host) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_map_outside: NULL buffer");
    return fetch(b, "fan_map_outside", outside_host, outside_off(b.st), (size_t)b.st->M * 8);
}

extern "C" int geoac_fan_map_timing(geoac_ctx* ctx, double* ms){
    Bound b;
    int rc = bind_map(ctx, "fan_map_timing", &b);
    if(rc) return rc;
    if(!ms) return geoac_map_fail(ctx, GEOAC_E_INVALID, "fan_map_timing: NULL argument");
    MAPCHK("fan_map_timing", hipEventSynchronize(b.st->e1));
    float t = 0;
    MAPCHK("fan_map_timing", hipEventElapsedTime(&t, b.st->e0, b.st->e1));
    *ms = t;
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
    MAPCHK("fan_fetch_level", hipMemcpyAsync(level_host, b.st->level, n, hipMemcpyDeviceToHost, (hipStream_t)b.v.stream));
    MAPCHK("fan_fetch_level", hipStreamSynchronize((hipStream_t)b.v.stream));
    return GEOAC_OK;
}
