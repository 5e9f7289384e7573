// geoac_refine_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_refine.hip (station refinement, include/geoac_refine.h):
// the map's view of the last completed launch (geoac_map_int.h), what the step rule needs of the members (source point, wind Mach numbers
// at the source) and of the parameters, and one pointer slot for the refinement state.
#ifndef GEOAC_REFINE_INT_H_
#define GEOAC_REFINE_INT_H_

#include "geoac_map_int.h"

#define GEOAC_RFN_MEMW 4           // doubles per member in GeoacRfnView::mem

struct GeoacRfnView {
    GeoacMapView map;              // (its `state` is the map's slot: not used here)
    int n_members;                 // M = n_src * K of the context now
    const double* mem;             // [M][GEOAC_RFN_MEMW] host: the member's source in the map's axes (lat, lon [deg] / x, y [km]), then u / c, v / c of its
                                   // profile at max(z_src, z_grnd) (GEOAC_EQ_3D; 0 for the other sets)
    double r_earth, z_grnd;
    int calc_amp, mode;            // of the parameters now (the next launch's)
    void** state;                  // slot in the context for the refinement state (NULL until the first use)
};

extern "C" int  geoac_rfn_view(geoac_ctx* ctx, GeoacRfnView* v);
extern "C" void geoac_rfn_release(void* state);                                  // geoac_destroy: frees the refinement state (device current, stream idle)

#endif
