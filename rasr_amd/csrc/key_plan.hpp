// key_plan.hpp -- the plan of a call's segments by key that cmllr.hip and mllr.hip share: the checks of the segment tables and every
// key's segments in ascending order.  Host arithmetic only, no device call: tests/host_keyplan_test.cc compiles it into a program of its
// own.
#pragma once
#include <vector>

#include "common.hpp"

namespace amx {

struct KeySeg {
    long long begin, end;   // frames [begin, end) of one segment
};

// key_base[k]: the frames of the keys before k
struct KeyPlan {
    long long           t0 = 0, n = 0;   // the call's frames [t0, t0 + n); n == 0: nothing to do
    std::vector<int>    key_tab;         // key_seg [n_keys + 1] into segs, then (on request) key_base [n_keys]
    std::vector<KeySeg> segs;            // every key's segments that hold frames, in ascending order
};

// The checks of a call's segment tables and the plan (a counting sort by key keeps every key's segments in ascending order).
// n_seg >= 0 is the caller's check: its message names the caller's dimension.
inline int plan_keys(const char* who, int n_seg, const long* frame_offsets, const int* seg_key, int n_keys, bool with_base, KeyPlan* out) {
    *out = KeyPlan{};
    if (n_seg <= 0)
        return AMX_OK;
    AMX_REQUIRE(frame_offsets && seg_key, AMX_ERR_INVALID, "%s: NULL frame_offsets or seg_key", who);
    AMX_REQUIRE(frame_offsets[0] >= 0, AMX_ERR_INVALID, "%s: frame_offsets[0] = %ld is negative", who, frame_offsets[0]);
    for (int s = 0; s < n_seg; ++s) {
        AMX_REQUIRE(frame_offsets[s + 1] >= frame_offsets[s], AMX_ERR_INVALID, "%s: frame_offsets decrease at segment %d (%ld after %ld)", who, s,
                    frame_offsets[s + 1], frame_offsets[s]);
        AMX_REQUIRE(seg_key[s] >= 0 && seg_key[s] < n_keys, AMX_ERR_INVALID, "%s: segment %d: key %d is outside [0, %d)", who, s, seg_key[s], n_keys);
    }
    const long long n = frame_offsets[n_seg] - frame_offsets[0];
    if (n == 0)
        return AMX_OK;
    AMX_REQUIRE(n < (1ll << 30), AMX_ERR_INVALID, "%s: %lld frames are more than one call takes", who, n);
    out->t0 = frame_offsets[0], out->n = n;
    out->key_tab.assign((size_t)n_keys + 1 + (with_base ? n_keys : 0), 0);
    int*                   key_seg = out->key_tab.data();
    std::vector<long long> key_frames((size_t)n_keys, 0);
    for (int s = 0; s < n_seg; ++s)
        if (frame_offsets[s + 1] > frame_offsets[s]) {
            ++key_seg[seg_key[s] + 1];
            key_frames[(size_t)seg_key[s]] += frame_offsets[s + 1] - frame_offsets[s];
        }
    long long run = 0;
    for (int k = 0; k < n_keys; ++k) {
        key_seg[k + 1] += key_seg[k];
        if (with_base)
            key_seg[n_keys + 1 + k] = (int)run;
        run += key_frames[(size_t)k];
    }
    out->segs.resize((size_t)key_seg[n_keys]);
    std::vector<int> cursor(key_seg, key_seg + n_keys);
    for (int s = 0; s < n_seg; ++s)
        if (frame_offsets[s + 1] > frame_offsets[s])
            out->segs[(size_t)cursor[(size_t)seg_key[s]]++] = KeySeg{frame_offsets[s], frame_offsets[s + 1]};
    return AMX_OK;
}

}  // namespace amx
