// geoac_level_refine_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_level_refine.hip (level refinement,
// include/geoac_level_refine.h): the map's view of the last completed launch (geoac_map_int.h), the members' source points in the stations'
// axes, what the rule needs of the parameters, and one pointer slot for the refinement state.  Nothing of a member's medium: the step is taken
// from crossing points alone, so the view serves grid ensembles too.
#ifndef GEOAC_LEVEL_REFINE_INT_H_
#define GEOAC_LEVEL_REFINE_INT_H_

#include "geoac_map_int.h"

struct GeoacLrfView {
    GeoacMapView map;              // (its `state` is the map's slot: not used here)
    int n_members;                 // M = n_src * K of the context now
    const double* src;             // [M][2] host: the member's source in the stations' axes (lat, lon [deg] / x, y [km])
    double r_earth;
    int mode;                      // of the parameters now (the next launch's)
    void** state;                  // slot in the context for the refinement state (NULL until the first use)
};

extern "C" int  geoac_lrf_view(geoac_ctx* ctx, GeoacLrfView* v);
extern "C" void geoac_lrf_release(void* state);                                  // geoac_destroy: frees the refinement state (device current, stream idle)

// what geoac_level_amp.hip reads of a current refinement result: the seeds' device arrays in the refinement's own block (valid until the next
// geoac_fan_level_refine) and the shape of its final launch, whose crossing tables geoac_fan_levels_dev still holds.  GEOAC_E_INVALID (with the
// message of the *_fetch calls, `what` in front) when there is no current result.
struct GeoacLrfSeeds {
    int n_seeds, M, L, capL;
    double probe_deg;
    const int* meta;               // [n_seeds][6]: member, station, level, leg, direction (0 up, 1 down), ordinal
    const int* status;             // [n_seeds]: GEOAC_RFN_CONVERGED ..
    const double* theta;           // [n_seeds]: the best point, = the base ray's launch angles in the final launch
    const double* phi;
};
extern "C" int  geoac_lrf_seeds(geoac_ctx* ctx, const char* what, GeoacLrfSeeds* out);

#endif
