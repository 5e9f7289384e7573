// geoac_tubemap_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_tubemap.hip (tube maps, include/geoac_tubemap.h):
// the map's view of the last completed launch (geoac_map_int.h), the caller's launch angles as the context keeps them on the host (ray order),
// and one pointer slot for the tube-map state.
#ifndef GEOAC_TUBEMAP_INT_H_
#define GEOAC_TUBEMAP_INT_H_

#include "geoac_map_int.h"

struct GeoacTubeView {
    GeoacMapView map;              // (its `state` is the map's slot: not used here)
    const double* theta_deg;       // [n_ang] host, the angles of geoac_fan_set_angles
    const double* phi_deg;
    int n_ang;
    void** state;                  // slot in the context for the tube-map state (NULL until the first use)
};

extern "C" int  geoac_tube_view(geoac_ctx* ctx, GeoacTubeView* v);
extern "C" void geoac_tube_release(void* state);                                 // geoac_destroy: frees the tube-map state (device current, stream idle)

#endif
