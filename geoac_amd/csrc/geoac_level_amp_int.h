// geoac_level_amp_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_level_amp.hip (level amplitudes,
// include/geoac_level_amp.h): the map's view of the last completed launch (geoac_map_int.h), the members' source points as the parameters hold
// them, the parameter block of the last completed launch for the probe launchers of geoac_kernels.hip (which evaluate member 0's medium: K is
// here so that the file can refuse K > 1), and one pointer slot for the state.
#ifndef GEOAC_LEVEL_AMP_INT_H_
#define GEOAC_LEVEL_AMP_INT_H_

#include "geoac_map_int.h"

struct GeoacDevParams;

struct GeoacLampView {
    GeoacMapView map;              // (its `state` is the map's slot: not used here)
    int n_members;                 // M = n_src * K of the context now
    int n_profiles;                // K
    int grid;                      // 1: a range-dependent set with its grid uploaded (geoac_launch_probe_grid serves), 0: geoac_launch_probe_atmo1d
    const double* src3;            // [M][3] host: the member's source in the layout of geoac_params.src (x, y, z / z, lat, lon)
    double r_earth, z_grnd;
    int mode;                      // of the parameters now (the next launch's)
    const GeoacDevParams* dev_params;   // host copy of the last completed launch's parameter block (valid while map.fresh)
    void** state;                  // slot in the context for the state (NULL until the first use)
};

extern "C" int  geoac_lamp_view(geoac_ctx* ctx, GeoacLampView* v);
extern "C" void geoac_lamp_release(void* state);                                 // geoac_destroy: frees the state (device current, stream idle)

// the probe launchers of geoac_kernels.hip, as geoac_api.cpp declares them (geoac_probe.h: the same kernels, the same bits)
extern "C" hipError_t geoac_launch_probe_atmo1d(const GeoacDevParams* P, int n, const double* x, double* out9, double* rho, hipStream_t s);
extern "C" hipError_t geoac_launch_probe_grid(const GeoacDevParams* P, int n, const double* a0, const double* a1, const double* a2, int coop,
                                              double* out30, double* api7, hipStream_t s);

#endif
