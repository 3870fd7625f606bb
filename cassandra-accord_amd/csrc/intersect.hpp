// intersect.hpp — launch interface of the Deps.intersecting kernels (intersect.hip; ad_deps_intersect).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace adx {

// One group per (destination d, owned request r, map m): row = d * n_owned + r of the result, group
// g = 3 * row + m. The input is an ad_merged (device CSR per map), the scope a set of destination range lists
// and one route per request.
struct IntersectArgs {
    uint64_t n_owned;
    uint32_t n_dest;
    bool rank_ids;                                // ids are uint32 ranks (4 bytes), else {msb, lsb, node} (24 bytes)
    bool start_inclusive;                         // ranges are [s, e), else (s, e]
    const uint64_t* keys_off[3]; const int64_t* keys[3];
    const uint64_t* txn_off[3];  const int64_t* txns[3];
    const uint64_t* k2t_off[3];  const int32_t* k2t[3];
    const uint64_t* dest_off;                     // [n_dest + 1] ranges of destination d
    const int64_t* dest_start; const int64_t* dest_end;
    const uint8_t* domain;                        // [n_owned] 0: key route, 1: range route (null: all key routes)
    const uint64_t* route_off;                    // [n_owned + 1] words of request r's route
    const int64_t* route;                         // key route: ascending keys; range route: {start, end} pairs
    uint32_t* gsz;                                // [3 k + m][n_dest * n_owned]: keys (ranges), ids, k2t ints of a group
    const uint64_t* goff;                         // [3 k + m][n_dest * n_owned + 1] their scan, each map from 0
    uint32_t* heavy; uint32_t* n_heavy;           // groups beyond the one-wave kernel (listed by the size pass)
    uint32_t* error;                              // IS_E_* bits
    int64_t* o_keys[3]; void* o_ids[3]; int32_t* o_k2t[3];
};

constexpr uint32_t IS_E_ROUTE = 1;     // route_off does not start at 0, or descends
constexpr uint32_t IS_E_INPUT = 2;     // the input's keysToTxnIds is malformed (offsets or id indices out of range)
constexpr uint32_t IS_E_IDS = 4;       // a map of more than IS_MAX_IDS ids
constexpr uint32_t IS_MAX_IDS = 131072;

hipError_t run_intersect_size(const IntersectArgs& a, hipStream_t st);
// the 9 totals of goff, the error word and the heavy count into tot[11]
hipError_t run_intersect_totals(const IntersectArgs& a, uint64_t* tot, hipStream_t st);
hipError_t run_intersect_emit(const IntersectArgs& a, uint32_t n_heavy, hipStream_t st);

}  // namespace adx
