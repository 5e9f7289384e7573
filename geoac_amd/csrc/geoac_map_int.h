// geoac_map_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_map.hip (arrival maps, include/geoac_map.h), and what
// geoac_map.hip owns for the other post-launch files: the layer allocation of a map and the checks of a map grid.
// The map code sees a context only through this view: the record and attenuation tables of the last completed launch, their shapes, the
// stream, and one pointer slot for its own state.  It never touches the launch plan.
#ifndef GEOAC_MAP_INT_H_
#define GEOAC_MAP_INT_H_

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct geoac_ctx;

struct GeoacMapView {
    int eqset, device;
    void* stream;                  // hipStream_t of the context
    int fresh;                     // 1: a launch has completed and nothing has invalidated its tables since
    unsigned long long gen;        // the context's invalidation counter now (a map is current while it carries this value)
    const double* rec;             // [M][n_rays][legs][GEOAC_REC_STRIDE]
    const double* atten;           // [F][n_rays][legs] while F > 1 (then M == 1); NULL at F == 1: the records' GEOAC_REC_ATTEN column serves
    int M, F, n_rays, legs, calc_amp;
    void** state;                  // slot in the context for the map state (NULL until the first use)
};

// the same view, the caller's launch angles as the context keeps them on the host (ray order, not the slot order of the device arrays), and
// the pointer slot of the file that asked: arrival maps, station arrivals, tube maps, level stations, level tube maps or level loudness maps
enum { GEOAC_SLOT_MAP = 0, GEOAC_SLOT_STA = 1, GEOAC_SLOT_TUBE = 2, GEOAC_SLOT_LSTA = 3, GEOAC_SLOT_LTUBE = 4, GEOAC_SLOT_LAMPMAP = 5 };
struct GeoacLaunchView {
    GeoacMapView map;              // (its `state` is always the map's slot)
    const double* theta_deg;       // [n_ang] host, the angles of geoac_fan_set_angles
    const double* phi_deg;
    int n_ang;
    void** state;                  // slot in the context for the asking file's state (NULL until the first use)
};

extern "C" int  geoac_map_view(geoac_ctx* ctx, GeoacMapView* v);
extern "C" int  geoac_launch_view(geoac_ctx* ctx, int slot, GeoacLaunchView* v);
extern "C" int  geoac_map_fail(geoac_ctx* ctx, int code, const char* msg);      // sets geoac_last_error, returns code
extern "C" void geoac_map_release(void* state);                                 // geoac_destroy: frees the map state (device current, stream idle)

// One layer allocation: COUNT | TTIME_MIN | CEL_MAX (M * cells words of 8 bytes each) | LEVEL_MAX | BEST (M * F * cells each) | tail words |
// DETECT (F * cells u32).  The layer numbers are those of geoac_map.h (geoac_tubemap.h has the same).  The tail is outside[M] for the arrival
// map and the four work counters for the tube map.  While a map is formed the extrema hold the order-preserving key of a double;
// geoac_layers_finish turns them into doubles and writes the empty-cell markers.
struct GeoacLayers {
    void* base; size_t cap;        // the allocation (geoac_layers_grow) and its size
    int M, F;
    long long cells;
    int tail_words;
    int detect;                    // 1: the DETECT layer is formed
};

// order-preserving key of a double: a < b as doubles (and -0 < +0) <=> key(a) < key(b) as unsigned integers
__device__ inline unsigned long long geoac_key(double v){
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double geoac_unkey(unsigned long long k){
    return __longlong_as_double((long long)((k >> 63) ? (k & ~0x8000000000000000ull) : ~k));
}

size_t geoac_layers_bytes(const GeoacLayers* L);
int    geoac_layers_grow(GeoacLayers* L);                                                       // GEOAC_OK / GEOAC_E_NOMEM
void   geoac_layers_span(const GeoacLayers* L, int layer, size_t* off, size_t* bytes);          // byte offset and size of a layer
void   geoac_layers_tail_span(const GeoacLayers* L, size_t* off, size_t* bytes);
void   geoac_layers_detect_span(const GeoacLayers* L, size_t* off, size_t* bytes);
// launches on `stream` (no status: the caller checks hipGetLastError after its own launches)
void   geoac_layers_fill(const GeoacLayers* L, void* stream);                                   // initial values of every word
void   geoac_layers_finish(const GeoacLayers* L, void* stream);                                 // keys back to doubles, empty-cell markers
void   geoac_layers_detect(const GeoacLayers* L, double detect_db, void* stream);               // members with LEVEL_MAX >= detect_db
// the bodies of <what>_dev, <what>_fetch, <what>_fetch_detect and of the tail's fetch; `noun` names the map in the message ("map", "tube map")
int    geoac_layers_dev(geoac_ctx* ctx, const char* what, const GeoacLayers* L, int layer, void** dev_ptr, size_t* bytes);
int    geoac_layers_fetch(geoac_ctx* ctx, const char* what, const GeoacLayers* L, void* stream, int layer, void* host);
int    geoac_layers_fetch_detect(geoac_ctx* ctx, const char* what, const char* noun, const GeoacLayers* L, void* stream, uint32_t* host);
int    geoac_layers_fetch_tail(geoac_ctx* ctx, const char* what, const GeoacLayers* L, void* stream, void* host);

// the first thing wrong with a map grid or a turning-height band, or NULL (the 2-D set's one-axis rule is geoac_map_check's own)
const char* geoac_grid_fault(int eqset, const double origin[2], const double step[2], const int n[2], int wrap_lon, double turn_min, double turn_max);

#endif
