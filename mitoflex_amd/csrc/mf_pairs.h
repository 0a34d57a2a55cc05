// Launchers of mf_pairs.hip: what two placed and scored mate sets say pair by pair, and the rescue of an unplaced mate from the window
// its settled mate implies (include/mitofilter.h, "pairs"; internal to libmitofilter_hip).
#pragma once
#include "mf_place.h"
#include "mf_rescue.h"
#include "mf_align_launch.h"

namespace mf {

struct PairOut { uint32_t kind; int32_t insert; };      // mf_pair_t
constexpr uint32_t PAIR_NONE = 0, PAIR_PROPER = 1, PAIR_DISCORDANT = 2, PAIR_RESCUED_1 = 3, PAIR_RESCUED_2 = 4, PAIR_SINGLE_1 = 5, PAIR_SINGLE_2 = 6;     // MF_PAIR_*

// The pair counters of a paired call, 64-bit words: proper, discordant, cross, rescued, single, insert_sum of every record (the fields
// of mf_pair_record_t), then the pairs without a settled mate, the rescue targets listed, and the rescued mates that did not pass.
constexpr uint32_t PAIR_RECORD_COUNTERS = 6;
struct PairLayout {
    size_t n_rec;
    constexpr explicit PairLayout(size_t n_rec_) : n_rec(n_rec_) {}
    constexpr size_t none() const { return PAIR_RECORD_COUNTERS * n_rec; }
    constexpr size_t listed() const { return none() + 1; }
    constexpr size_t rescued_not_passing() const { return none() + 2; }
    constexpr size_t words() const { return none() + 3; }
};

struct PairWindow { uint32_t min_insert, max_insert, rescue_permille; };

// One thread per pair, grid-stride, over both sets' pass bits (bits1, bits2: n bits each, the filter pass's bitmaps), the placements of the mates that
// pass (place1, place2: n entries each, of which only those need to hold anything) and, where the cut can reject (max_permille < 1000),
// their scores (score1, score2: null otherwise is fine): kind and insert of every pair that needs no scan into pairs[i], the pair
// counters bumped, and -- with list non-null -- the pairs of exactly one settled mate whose other mate is not placed into list (any order; counters[listed()] counts them, zeroed by
// the caller).  Without a list those pairs are settled as single at once.
hipError_t launch_pair_list(const uint32_t *bits1, const uint32_t *bits2, const PlaceOut *place1, const PlaceOut *place2, const ScoreOut *score1,
                            const ScoreOut *score2, uint64_t n, uint32_t max_permille, PairWindow win, uint32_t n_rec, PairOut *pairs, uint32_t *list, unsigned long long *counters, int n_cu, hipStream_t st);

// One wave per listed pair, grid-stride: the unplaced mate's candidates on its settled mate's record scored, the winner committed into
// the counters of a verifying placement (diff, counts: its record counters with the gathered score section behind them, sums: its
// compared / mismatches sums, pile: optional) as an accepted placed read of votes 0 (score1 / score2: optional), and the pair's kind and
// insert written.  A rescued mate that passed leaves counts[4 * n_rec]; one that did not is counted in counters[rescued_not_passing()].
hipError_t launch_rescue(const ReadsView &R1, const ReadsView &R2, const uint32_t *bits1, const uint32_t *bits2, PlaceOut *place1, PlaceOut *place2,
                         ScoreOut *score1, ScoreOut *score2, const uint32_t *list, uint64_t n_pairs, PairWindow win, int k, const ScoreBait &bait, const uint64_t *rec_start, uint32_t n_rec, PairOut *pairs,
                         unsigned long long *counters, unsigned long long *diff, unsigned long long *counts, unsigned long long *sums,
                         unsigned long long *pile, int n_cu, hipStream_t st);

// The aligning forms (include/mitofilter.h, "pairs with a band").  launch_pair_list_aligned is launch_pair_list over the sets' alignments:
// a placed mate is settled when align_accepts accepts its alignment (read only where max_permille < 1000).
hipError_t launch_pair_list_aligned(const uint32_t *bits1, const uint32_t *bits2, const PlaceOut *place1, const PlaceOut *place2, const AlignOut *align1,
                                    const AlignOut *align2, uint64_t n, uint32_t max_permille, PairWindow win, uint32_t n_rec, PairOut *pairs, uint32_t *list, unsigned long long *counters, int n_cu, hipStream_t st);

// What the aligning rescue takes beside launch_rescue's arguments: the counters of an aligning layout (sums: ALIGN_SUMS a record; indel;
// ins_pile and ext_pile / extend as PlaceAlign holds them), the sets' alignments (optional), the band, and the work memory: work holds
// align_work_words(max_len) words for each of rescue_align_waves(n_pairs, max_len, n_cu) waves; max_len: no read of EITHER set is longer
// (a rescue target need not pass, so it is on no list).
struct RescueAlign {
    uint32_t band; AlignOut *align1, *align2; unsigned long long *sums, *indel, *ins_pile, *ext_pile; uint32_t extend;
    unsigned long long *work; uint64_t max_len;
};
// the waves of the aligning rescue: align_waves' rule, so never more than the bound on the work memory allows
uint64_t rescue_align_waves(uint64_t n_pairs, uint64_t max_len, int n_cu);
// launch_rescue with the seed scored ungapped as there, and the winner then aligned inside the band around the seed's start: committed
// with the alignment's footprint, edits and sums, and added wherever an accepted aligned read adds.
hipError_t launch_rescue_aligned(const ReadsView &R1, const ReadsView &R2, const uint32_t *bits1, const uint32_t *bits2, PlaceOut *place1, PlaceOut *place2,
                                 const uint32_t *list, uint64_t n_pairs, PairWindow win, int k, const ScoreBait &bait, const uint64_t *rec_start,
                                 uint32_t n_rec, PairOut *pairs, unsigned long long *counters, unsigned long long *diff, unsigned long long *counts,
                                 unsigned long long *pile, const RescueAlign &A, int n_cu, hipStream_t st);

} // namespace mf
