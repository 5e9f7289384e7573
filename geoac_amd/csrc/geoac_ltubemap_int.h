// geoac_ltubemap_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_ltubemap.hip (level tube maps,
// include/geoac_ltubemap.h).  The file reads a context through the GeoacLaunchView of geoac_map_int.h, with its own slot (GEOAC_SLOT_LTUBE),
// the crossing records through the public geoac_fan_levels_dev / geoac_get_levels, and the branch table through geoac_lstations_int.h.
#ifndef GEOAC_LTUBEMAP_INT_H_
#define GEOAC_LTUBEMAP_INT_H_

extern "C" void geoac_ltube_release(void* state);                                // geoac_destroy: frees the level-tube-map state (device current, stream idle)

#endif
