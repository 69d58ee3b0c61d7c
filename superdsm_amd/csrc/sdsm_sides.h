// The side streams of a launch (sdsm_sides.hip): one pool per device, shared by all plans, and per caller stream the choice of pool streams
// that run side by side with it.
#pragma once
#include <mutex>

#include "sdsm_plan.h"

// Side streams / fork-join events of the solve classes.  A plan borrows a set at its first launch and gives it back when it is
// destroyed: creating and destroying HIP streams costs milliseconds (hipStreamDestroy synchronises), a reference-style caller
// builds a plan per batch.  A set carries no state between users (events are recorded before they are waited for).
// The set holds a POOL of side streams, created on demand, and for every caller stream it has seen the pool streams that run side by side
// with that stream and with each other (choose_sides): which hardware queue a stream lands on depends on every stream the process
// created before it, so no fixed set of streams is clear of every caller's queue.
// state of a choice: 1 the caller's stream and the sides run side by side, 0 fewer than three clean sides (classes share a queue), -1 a probe stayed undecided
struct SideChoice { hipStream_t caller = nullptr; int idx[4] = {-1, -1, -1, -1}; int want = 0, clean = 0, state = 0, reprobes = 0; uint64_t born = 0; bool valid = false; };
struct SideSet {
    hipStream_t pool[SDSM_SIDE_POOL]; int n_pool = 0; hipEvent_t fj[5]; int device; std::mutex enqueue;
    int32_t *probe_words = nullptr;                 // SDSM_PROBE_BYTES, allocated once
    SideChoice cache[SDSM_SIDE_CACHE]; uint64_t tick = 0; int probes = 0, unknowns = 0; bool warned = false;
};

// The device's set for the plan (borrowed at its first launch; created at the first launch on the device that needs one).
SDSM_INTERNAL hipError_t acquire_sides(const sdsm_plan *p, hipStream_t caller);
// The side streams for launches from `caller`, under the set's mutex: from the cache, or found by probing (synchronises the caller's stream and the pool).
SDSM_INTERNAL hipError_t choose_sides(SideSet *q, hipStream_t caller, int want, SideChoice *out);
