// The anchor vote of a listed read, shared by place_kernel (mf_place.hip) and align_kernel (mf_align.hip): one statement of the rule that
// places a read.
#pragma once
#include "mf_place.h"
#include "mf_tally_dev.h"

namespace mf {

// The whole wave votes for read `src` (begun: np windows).  Lanes take the windows 64 at a time: canonical key and the read's orientation
// together, slot, anchor entry -- one 8-byte gather --, candidate (record, strand, start) as a 64-bit key; WaveTally counts the votes,
// in repeated sweeps where a read has more than 64 candidates.  best_cnt 0: no window voted; tie: the most votes are shared; best_key:
// (record << 1 | strand) << 32 | start of the winner; windows: the windows that voted.
template <int KW>
__device__ __forceinline__ void place_vote(const ReadsView &R, const KmerSetView &S, const Anchor *__restrict__ anchor, const NucWindows<KW> &src, uint64_t np,
                                           int lane, uint32_t &best_cnt, uint64_t &best_key, bool &tie, uint32_t &windows)
{
    best_cnt = 0; windows = 0; best_key = 0; tie = false;
    uint64_t lo_bound = 0;                               // the candidates this sweep counts: lo_bound and above
    for (;;) {
        WaveTally<uint64_t> tally;
        for (uint64_t p0 = 0; p0 < np; p0 += 64) {
            const uint64_t p = p0 + (uint64_t)lane;
            uint64_t id = WaveTally<uint64_t>::NONE;
            bool voted = false;
            if (p < np && src.valid_at(p)) {
                uint32_t rev;
                const uint64_t slot = table_find(S, oriented_at<KW>(R.words, src.b0 + p, S.k, rev));
                if (slot != ~0ULL) {
                    const Anchor a = anchor[slot];
                    if (a.pos != ANCHOR_NONE) {            // (a window that is its own reverse complement finds no anchor: the build drops them)
                        const uint32_t rs = a.rb ^ (rev & 1u);   // record << 1 | strand
                        const uint32_t off = (uint32_t)((rs & 1u) ? np - 1 - p : p);
                        const uint64_t cand = ((uint64_t)rs << 32) | (uint32_t)((int32_t)a.pos - (int32_t)off);
                        voted = true;
                        if (cand >= lo_bound) id = cand;
                    }
                }
            }
            if (lo_bound == 0) windows += (uint32_t)__popcll(__ballot(voted));
            tally.add(id, lane);
        }
        tally.fold(best_cnt, best_key, tie);
        if (!tally.overflow) break;
        lo_bound = tally.next_bound();
    }
}

} // namespace mf
