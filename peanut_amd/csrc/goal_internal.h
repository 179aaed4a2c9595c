// What csrc/goal.hip offers to the other translation units of the library and to nobody outside it: the batched geodesic field on
// given masks, which the batched short-term goal (csrc/stg.hip, peanut_stg_plan_batch) is built around.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "peanut_hip.h"

namespace peanut {

// Why these E solver handles cannot share a solve (E outside 1..PEANUT_GOAL_MAX_BATCH, a null or repeated handle, handles that differ
// in map size or in the solver options), or null.  Touches no device.
const char* fmm_masks_batch_bad(int E, peanut_goal_t* const* g);

// Once per call, before the first solve: the lead handle's batch scratch exists (made on first use, kept with the handle) and work
// begun on any of the handles has run out.  After it fmm_distance_masks_batch allocates nothing and creates no stream.
int fmm_masks_batch_prepare(int E, peanut_goal_t* const* g);

// peanut_fmm_distance(g[e], trav[e], seed_mask[e], -1, -1, fill_mode = 1, out[e], s) for every episode e whose bit in `skip` is
// clear, in the launches and host synchronisations of one solve; every episode gets the bits of its own single call.  g[0] leads
// (its batch scratch is used) whether or not it is skipped, and the slots are the episodes' indices, so a caller that drops episodes
// from one solve to the next passes the same arrays with another `skip`.  Entries of skipped episodes are not looked at.  All arrays
// are HOST arrays of E device pointers.  Synchronises inside (the solver polls its counters); the fill is enqueued, not waited for.
int fmm_distance_masks_batch(int E, peanut_goal_t* const* g, const unsigned char* const* trav, const unsigned char* const* seed_mask,
                             double* const* out, unsigned int skip, hipStream_t s);

}  // namespace peanut
