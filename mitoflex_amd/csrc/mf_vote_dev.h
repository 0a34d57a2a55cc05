// What place_kernel (mf_place.hip) and align_kernel (mf_align.hip) share, each stated once: the anchor vote that places a listed read
// (place_vote), its winner decoded (Winner), a read's letter (read_letter), the bases it piles (pile_bases, which rescue_kernel of mf_pairs.hip calls too), what lane 0 commits for the read
// (commit_read), and the
// launchers' choice of an instantiation (dispatch_kw_flag).
#pragma once
#include "mf_place.h"
#include "mf_tally_dev.h"
#include <type_traits>

namespace mf {

// The letter of base g of the packed read stream, 0 .. 3, or READ_LETTER_NONE for an N (hasn: the read holds one; the invalid-position
// index is searched only then).
constexpr uint32_t READ_LETTER_NONE = 4;
__device__ __forceinline__ uint32_t read_letter(const ReadsView &R, uint64_t g, bool hasn)
{
    if (hasn) { const uint64_t ni = npos_lower_bound(R, g); if (ni < R.n_npos && R.npos[ni] == g) return READ_LETTER_NONE; }
    return (R.words[g >> 4] >> (2 * ((uint32_t)g & 15u))) & 3u;
}

// last record that starts at or before p (rec_start: n_rec + 1 ascending offsets)
__device__ __forceinline__ uint32_t record_of(const uint64_t *__restrict__ rec_start, uint32_t n_rec, uint64_t p)
{
    uint32_t a = 0, b = n_rec;
    while (b - a > 1) { const uint32_t m = (a + b) >> 1; if (rec_start[m] <= p) a = m; else b = m; }
    return a;
}

// The winner of a placed read's vote: record << 1 | strand, the leftmost base's record coordinate, the record's first position on the
// bait and its length.  winner_of decodes best_key wave-uniform (into scalar registers); winner_at is the decode itself.
struct Winner {
    uint32_t rs; int64_t start; uint64_t s0; int64_t len;
    __device__ __forceinline__ uint32_t record() const { return rs >> 1; }
    __device__ __forceinline__ uint32_t strand() const { return rs & 1u; }
};
__device__ __forceinline__ Winner winner_at(uint32_t rs, int32_t start, const uint64_t *__restrict__ rec_start)
{
    Winner w;
    w.rs = rs;
    w.start = start;
    w.s0 = rec_start[rs >> 1];
    w.len = (int64_t)(rec_start[(rs >> 1) + 1] - w.s0);
    return w;
}
__device__ __forceinline__ Winner winner_of(uint64_t best_key, const uint64_t *__restrict__ rec_start)
{
    return winner_at(__builtin_amdgcn_readfirstlane((uint32_t)(best_key >> 32)), (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)best_key), rec_start);
}

// The bases of a read of L bases at b0, placed as W says, into pile: [position][letter].  The whole wave calls it; lane l takes bases
// l, l + 64, ..  Consecutive lanes add to consecutive positions: no two lanes of an instruction share a counter.
__device__ __forceinline__ void pile_bases(const ReadsView &R, uint64_t b0, bool hasn, uint64_t L, const Winner &W, unsigned long long *__restrict__ pile, int lane)
{
    for (uint64_t i = (uint64_t)lane; i < L; i += 64) {
        uint32_t letter = read_letter(R, b0 + i, hasn);
        if (letter == READ_LETTER_NONE) continue;                                                                       // an N counts nowhere
        int64_t c = W.start + (int64_t)i;
        if (W.strand()) { c = W.start + (int64_t)(L - 1 - i); letter ^= 3u; }
        if (c < 0 || c >= W.len) continue;                                                                              // an overhang counts nowhere
        atomicAdd(&pile[4 * (W.s0 + (uint64_t)c) + letter], 1ull);
    }
}

// What lane 0 commits for listed read r of L bases once the vote (and, in a cutting launch, the cut) is known.  placed: the vote has a
// strict winner W; accept: the cut accepts it (true in a launch without one).  [begin, end): the unclipped footprint on W's record --
// the placement's in place_kernel, the alignment's in align_kernel; an accepted read adds +1 / -1 into diff at its clipped ends and bumps
// forward or reverse, over_begin, over_end of its record in cnt.  gather: the launch holds `rejected` and the SCORE_BINS bins of every
// record behind the 4 * n_rec + 1 counters; bin: the placed read's mismatches or edits.  A read that is not placed bumps "not placed".
// place (optional): place[r].  keep_bits (optional): the read's bit is cleared where keep_clears says so -- the bitmap's words are shared
// by the waves of 32 reads, hence the atomic.
__device__ __forceinline__ void commit_read(bool placed, bool accept, const Winner &W, uint64_t L, int64_t begin, int64_t end, bool gather, uint32_t bin,
                                            uint32_t votes, uint32_t windows, uint32_t r, uint32_t n_rec, PlaceOut *__restrict__ place,
                                            unsigned long long *__restrict__ diff, GatheredCounts &cnt, uint32_t *__restrict__ keep_bits, int keep)
{
    PlaceOut out{PLACE_AMBIGUOUS, 0u, 0, 0, 0u, windows};
    if (placed) {
        const uint32_t j = W.record();
        out = PlaceOut{j, W.strand(), (int32_t)W.start, (int32_t)(W.start + (int64_t)L), votes, windows};
        if (accept) {
            // the winning anchor's window lies inside the record (band < k: on diagonal 0 of an alignment): the clipped footprint is not empty
            const int64_t lo = begin < 0 ? 0 : begin < W.len ? begin : W.len;
            const int64_t hi = end < 0 ? 0 : end < W.len ? end : W.len;
            atomicAdd(&diff[W.s0 + (uint64_t)lo], 1ull);
            atomicAdd(&diff[W.s0 + (uint64_t)hi], ~0ull);
            cnt.bump(4 * j + W.strand());
            if (begin < 0) cnt.add(4 * j + 2, 1);
            if (end > W.len) cnt.add(4 * j + 3, 1);
        }
        if (gather) {
            const uint32_t g0 = 4 * n_rec + 1 + SCORE_GATHERED * j;
            if (!accept) cnt.add(g0, 1);
            cnt.add(g0 + 1 + (bin < SCORE_BINS - 1 ? bin : SCORE_BINS - 1), 1);
        }
    } else cnt.bump(4 * n_rec);
    if (place) place[r] = out;
    if (keep_bits && keep_clears(placed, accept, keep)) atomicAnd(&keep_bits[r >> 5], ~(1u << (r & 31u)));
}

// the key width and one flag of a launch as template arguments: f(integral_constant<int, KW>, bool_constant<FLAG>)
template <class F>
static inline void dispatch_kw_flag(int kw, bool flag, F &&f)
{
    if (kw == 1) { if (flag) f(std::integral_constant<int, 1>{}, std::true_type{}); else f(std::integral_constant<int, 1>{}, std::false_type{}); }
    else { if (flag) f(std::integral_constant<int, 2>{}, std::true_type{}); else f(std::integral_constant<int, 2>{}, std::false_type{}); }
}

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
