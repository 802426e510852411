// What the ra_api*.cpp files share: the argument-check macro, the lifecycle of the handles a context owns, the chunk counters and those
// hot-path passes of ra_api.cpp that the thin entry points (ra_api_ops.cpp, ra_api_mcubes.cpp) and the test hooks (ra_api_debug.cpp)
// call; hdq_pass, fine_level and forward_pass have no caller outside ra_api.cpp and stay private to it.
#pragma once
#include "ra_ctx.hpp"

#define RA_CHECK(cond, msg)          \
    do {                             \
        if (!(cond)) {               \
            ra_set_error(msg);       \
            return 1;                \
        }                            \
    } while (0)

// the handles of a context (ra_ctx::meshes, topos, cloths): p if v owns it, else null
template <typename T> static T* owned(const std::vector<std::unique_ptr<T>>& v, const T* p) {
    for (auto& u : v) if (u.get() == p) return u.get();
    return nullptr;
}
// ... and its end: the device current and idle first (launches that read the handle may still be queued), then out of v
template <typename T> static void release_owned(ra_ctx* c, std::vector<std::unique_ptr<T>>& v, const T* p) {
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    for (auto it = v.begin(); it != v.end(); ++it) if (it->get() == p) { v.erase(it); break; }
}

// weights finalized, a frame set, the context's device current; who: the entry point, for the message
int check_ready(ra_ctx* c, const char* who);

inline DevCounters* dcnt(ra_ctx* c) { return c->dcounters.as<DevCounters>(); }
inline int* icnt(ra_ctx* c, int k) { return reinterpret_cast<int*>(c->dcounters.as<char>() + 128) + k; }   // small int counters
enum { CNT_HIT = 1, CNT_RAYS = 2, CNT_SAMP = 3, CNT_FC0 = 8, CNT_FC_SLOTS = 96, CNT_ALL = CNT_FC0 + CNT_FC_SLOTS };
int* next_fine_counter(ra_ctx* c, hipStream_t s);

inline int raw_channels(const ra_ctx* c) { return c->cfg.relight ? 17 : 16; }
// the fields of a full query that come from the context's configuration and weights; the caller adds its lists and outputs
FullIO full_io(ra_ctx* c);
void k4_fwd_launch(ra_ctx* c, const FullIO& io, char* tape, hipStream_t s);
int full_query(ra_ctx* c, FullIO io, int n, hipStream_t s);
// the decoders of ra_sdf_volume (ra_api.cpp): mode 0 canonical sdf(x), 1 sdf(x + resd(x)), 2 the hierarchical query of world points; compensated tier
int sdf_points_precise(ra_ctx* c, int mode, const float* pts, int n, float dist_th, float* sdf, hipStream_t s);
