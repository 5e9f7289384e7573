// geoac_launch_int.h - what geoac_map.hip, geoac_stations.hip, geoac_tubemap.hip, geoac_refine.hip, geoac_lstations.hip and
// geoac_level_refine.hip do alike with a
// context and with the HIP runtime: device buffers that grow, the status of a failed HIP call, grid sizes, the event pair behind a *_timing
// function, and the first steps of every entry point that reads the last completed launch.  Plain functions; each file keeps its own state and
// its own entry points.  (What a pair of files alone shares has a header of its own: geoac_lattice_list.h for the two list searches, geoac_stations.hip
// and geoac_lstations.hip, geoac_tube_walk.h for the two tube maps, geoac_tubemap.hip and geoac_ltubemap.hip, and geoac_newton_rounds.h for the two refinements, geoac_refine.hip and geoac_level_refine.hip.)
#ifndef GEOAC_LAUNCH_INT_H_
#define GEOAC_LAUNCH_INT_H_

#include <hip/hip_runtime.h>
#include <string>

#include "../../include/geoac_hip.h"
#include "geoac_map_int.h"

namespace {

// a device buffer of at least `need` bytes, its content lost when it has to grow
int grow(void** p, size_t* cap, size_t need){
    if(*p && *cap >= need) return GEOAC_OK;
    if(*p){ hipFree(*p); *p = nullptr; *cap = 0; }                  // (hipFree waits for the work that may still read it)
    if(hipMalloc(p, need ? need : 8) != hipSuccess){ (void)hipGetLastError(); *p = nullptr; return GEOAC_E_NOMEM; }
    *cap = need;
    return GEOAC_OK;
}

int hip_fail(geoac_ctx* ctx, const char* what, hipError_t e){
    return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}
// (in a function that returns a status and has the context at hand as b.ctx)
#define GEOAC_CHK(what, call) do { hipError_t e_ = (call); if(e_ != hipSuccess) return hip_fail(b.ctx, what, e_); } while(0)

bool spherical(int eqset){ return eqset == GEOAC_EQ_GLOBAL || eqset == GEOAC_EQ_GLOBAL_RNGDEP; }

// blocks for n items at per_block items each: at least 1, at most cap
unsigned blocks_for(long long n, int per_block, long long cap = 1ll << 20){
    long long b = (n + per_block - 1) / per_block;
    if(b < 1) b = 1;
    if(b > cap) b = cap;
    return (unsigned)b;
}

// the two events around a call's work on the stream (created on first use)
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t start(hipStream_t s){
        if(!e0){
            hipError_t e = hipEventCreate(&e0);
            if(e == hipSuccess) e = hipEventCreate(&e1);
            if(e != hipSuccess) return e;
        }
        return hipEventRecord(e0, s);
    }
    hipError_t stop(hipStream_t s){ return hipEventRecord(e1, s); }
    hipError_t ms(double* out){
        hipError_t e = hipEventSynchronize(e1);
        float t = 0;
        if(e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        *out = t;
        return e;
    }
    void release(){
        if(e0) hipEventDestroy(e0);
        if(e1) hipEventDestroy(e1);
    }
};

// the first steps of an entry point that reads the last completed launch: the view with the asking file's slot, the refusal when there is no
// such launch, the context's device made current.  `what` names the entry point in messages.  (The state in the slot is the caller's to create.)
int bind_launch(geoac_ctx* ctx, const char* what, int slot, GeoacLaunchView* v){
    if(!ctx) return GEOAC_E_INVALID;
    int rc = geoac_launch_view(ctx, slot, v);
    if(rc) return rc;
    if(!v->map.fresh)
        return geoac_map_fail(ctx, GEOAC_E_INVALID, (std::string(what) + ": no completed launch, or new angles, an atmosphere upload, geoac_set_sources or "
                                                     "geoac_set_frequencies have come since it (launch again)").c_str());
    if(hipSetDevice(v->map.device) != hipSuccess) return geoac_map_fail(ctx, GEOAC_E_HIP, (std::string(what) + ": hipSetDevice failed").c_str());
    return GEOAC_OK;
}

}  // namespace

#endif
