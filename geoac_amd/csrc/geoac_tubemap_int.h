// geoac_tubemap_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_tubemap.hip (tube maps, include/geoac_tubemap.h).
// The tube map reads a context through the GeoacLaunchView of geoac_map_int.h, with its own slot.
#ifndef GEOAC_TUBEMAP_INT_H_
#define GEOAC_TUBEMAP_INT_H_

extern "C" void geoac_tube_release(void* state);                                 // geoac_destroy: frees the tube-map state (device current, stream idle)

#endif
