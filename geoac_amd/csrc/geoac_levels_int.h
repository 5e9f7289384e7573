// geoac_levels_int.h - the seam between geoac_api.cpp (which owns geoac_ctx and the epoch pipeline) and geoac_levels.hip (level crossings,
// include/geoac_levels.h): the second argument block of k_levels and its launcher.  GeoacDevParams stays as it is; k_levels takes
// GeoacLevelParams beside it, as the kernels of a frequency set take GeoacFreqParams.
#ifndef GEOAC_LEVELS_INT_H_
#define GEOAC_LEVELS_INT_H_

#include <hip/hip_runtime.h>

#include "../../include/geoac_levels.h"
#include "geoac_device.h"

#define GEOAC_LVL_NSTATE 5      // rows of the state block: tt, at, ltt, lat, leg (as ST_TT, ST_AT, ST_LTT, ST_LAT, ST_PLEG of the ray state, which k_accum owns)

struct GeoacLevelParams {
    int     n_levels;                   // L, 1 .. GEOAC_MAX_LEVELS
    int     cap;                        // crossings kept per (ray, level), 1 .. GEOAC_LVL_MAX_CAP
    int     hidx;                       // height component of a path row (EQ::HIDX): 2 for the Cartesian sets, 0 for the spherical sets
    int     pad_;
    double  lev[GEOAC_MAX_LEVELS];      // the levels in the units of that component: z_km, or r_earth + z_km (added once on the host, as P.ground is)
    double* state;                      // [GEOAC_LVL_NSTATE][n_pad], zeroed per launch
    double* rec;                        // [M n_rays][L][cap][GEOAC_LVL_STRIDE], zeroed per launch
    int*    count;                      // [M n_rays][L], zeroed per launch
};

// k_levels of one epoch: behind k_accum (and k_accum_freq) of that epoch on their stream, with the parameter block they were given
extern "C" hipError_t geoac_launch_levels(const GeoacDevParams* P, const GeoacLevelParams* Q, hipStream_t s);

#endif
