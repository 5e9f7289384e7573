// geoac_map_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_map.hip (arrival maps, include/geoac_map.h).
// The map code sees a context only through this view: the record and attenuation tables of the last completed launch, their shapes, the
// stream, and one pointer slot for its own state.  It never touches the launch plan.
#ifndef GEOAC_MAP_INT_H_
#define GEOAC_MAP_INT_H_

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

extern "C" int  geoac_map_view(geoac_ctx* ctx, GeoacMapView* v);
extern "C" int  geoac_map_fail(geoac_ctx* ctx, int code, const char* msg);      // sets geoac_last_error, returns code
extern "C" void geoac_map_release(void* state);                                 // geoac_destroy: frees the map state (device current, stream idle)

#endif
