// geoac_lampmap_int.h - the seam between geoac_api.cpp (which owns geoac_ctx) and geoac_lampmap.hip (level loudness maps,
// include/geoac_lampmap.h).  The file reads a context through the GeoacLaunchView of geoac_map_int.h, with its own slot (GEOAC_SLOT_LAMPMAP),
// the crossing records through the public geoac_fan_levels_dev / geoac_get_levels, the branch table through geoac_lstations_int.h, and the
// members' source points, the launch's parameter block and the probe launchers through geoac_level_amp_int.h (geoac_lamp_view).
#ifndef GEOAC_LAMPMAP_INT_H_
#define GEOAC_LAMPMAP_INT_H_

extern "C" void geoac_lampmap_release(void* state);                              // geoac_destroy: frees the loudness-map state (device current, stream idle)

#endif
