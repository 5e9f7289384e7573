// geoac_stations_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_stations.hip (station arrivals,
// include/geoac_stations.h): the map's view of the last completed launch (geoac_map_int.h), the caller's launch angles as the context keeps
// them on the host (ray order, not the slot order of the device arrays), and one pointer slot for the station state.
#ifndef GEOAC_STATIONS_INT_H_
#define GEOAC_STATIONS_INT_H_

#include "geoac_map_int.h"

struct GeoacStaView {
    GeoacMapView map;              // (its `state` is the map's slot: not used here)
    const double* theta_deg;       // [n_ang] host, the angles of geoac_fan_set_angles
    const double* phi_deg;
    int n_ang;
    void** state;                  // slot in the context for the station state (NULL until the first use)
};

extern "C" int  geoac_sta_view(geoac_ctx* ctx, GeoacStaView* v);
extern "C" void geoac_sta_release(void* state);                                  // geoac_destroy: frees the station state (device current, stream idle)

#endif
