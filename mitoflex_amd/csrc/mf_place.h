// Launchers of mf_place.hip: where on the bait, and on which strand, the reads that pass lie, and which bases they put on every bait
// position (internal to libmitofilter_hip).
#pragma once
#include <hip/hip_runtime.h>
#include "mf_common.h"
#include "mf_kernels.h"
#include "mf_placelayout.h"          // SCORE_BINS, SCORE_GATHERED, PILE_SUMS: what the kernels share with the host's layout
#include "mf_score.h"                // ScoreBait, keep_clears
#include "mf_call.h"                 // PLACE_CLAMP and the call rules

namespace mf {

constexpr uint32_t ANCHOR_NONE = 0xFFFFFFFFu;        // position of a slot whose key is no anchor
constexpr uint32_t PLACE_AMBIGUOUS = 0xFFFFFFFEu;    // MF_PLACE_AMBIGUOUS
constexpr uint32_t PLACE_NONE = 0xFFFFFFFFu;         // MF_PLACE_NONE
struct alignas(8) Anchor { uint32_t pos, rb; };          // position inside the record (ANCHOR_NONE: no anchor), record << 1 | b
struct PlaceOut { uint32_t record, strand; int32_t start, end; uint32_t votes, windows; };       // mf_place_t
struct ScoreOut { uint32_t compared, mismatches; };      // mf_score_t
// What a cutting launch (a verifying or an aligning one) takes beside a placing one.  bait: the bait's packed letters and its validity,
// one bit a position, with the index of each array's last word (the 16-base compare clamps to it).  sums: counters of every record,
// summed over the ACCEPTED reads.  keep_bits (optional): n_reads bits laid out like the pass bitmap and holding a copy of it; a listed
// read loses its bit there where keep_clears(placed, accepted, keep) of mf_score.h says so (keep: MF_KEEP_ACCEPTED or MF_KEEP_PLACED).
// Nothing else is written for it.
struct PlaceCut { ScoreBait bait; uint32_t max_permille; unsigned long long *sums; uint32_t *keep_bits; int keep; };
// The verifying launch.  score (optional): n_reads entries, zeroed.  cut.sums: compared, mismatches, 2 counters a record.
struct PlaceVerify { PlaceCut cut; ScoreOut *score; };

// Anchor table, indexed by the slot of the key table: anchor[slot] = { the window's position inside its record, record << 1 | b } when
// exactly one valid bait window holds the key and that window is not its own reverse complement (b: 1 when the bait's reverse
// complement is the canonical form); { ANCHOR_NONE, 0 } otherwise.  rec_start: n_rec + 1 ascending base offsets on the device.
// lo / hi: `slots` words of scratch each.  The result does not depend on the order the windows arrive in.  Positions below 2^31 - 1.
hipError_t launch_build_anchor(const BaitView &B, const uint64_t *rec_start, uint32_t n_rec, const KmerSetView &S, Anchor *anchor, uint32_t *lo,
                               uint32_t *hi, hipStream_t st);
// { PLACE_NONE, 0, 0, 0, 0, 0 } into every entry
hipError_t launch_place_init(PlaceOut *place, uint64_t n_reads, hipStream_t st);
// the longest read of a ragged read set into *max_len (zeroed by the caller)
hipError_t launch_max_read_len(const uint64_t *offsets, uint64_t n_reads, unsigned long long *max_len, hipStream_t st);
// One wave per listed read: every window whose key is an anchor votes for (record, strand, start); the strict winner places the read.
// place (optional, n_reads entries, initialised): place[read].  diff: B.total + 1 counters that receive +1 at the first and -1 behind
// the last covered position of every placed read (global positions, two's complement).  counts: 4 * n_rec + 1 counters -- forward,
// reverse, over_begin, over_end of every record, then the listed reads that are not placed.
// pile (optional): 4 * B.total counters, [position][A, C, G, T] -- the pile-up.  Every valid base of a placed read that lies inside its
// record adds 1 to the counter of its position and letter, complemented on strand 1 (the bait's forward letters); the other outputs
// are the same with and without it.
// verify (optional): every placed read is scored against the bait along its placement before anything of it is counted (mf_score.h), and
// one whose mismatches * 1000 exceed max_permille * compared is REJECTED: it adds to no counter above, only to its record's `rejected`.
// counts then holds SCORE_GATHERED * n_rec counters more behind the 4 * n_rec + 1: rejected and the SCORE_BINS bins of min(mismatches, 31)
// of every record's placed reads, accepted or not.
hipError_t launch_place(const ReadsView &R, const KmerSetView &S, const Anchor *anchor, const uint64_t *rec_start, const uint32_t *list,
                        const unsigned long long *n_list, uint32_t n_rec, PlaceOut *place, unsigned long long *diff, unsigned long long *counts,
                        unsigned long long *pile, const PlaceVerify *verify, int n_cu, hipStream_t st);
// Base depth from the difference counters: depth[p] = diff[0] + .. + diff[p] for p < total, clamped into `depth` (optional); rec_sums
// (optional, zeroed by the caller): covered and base_sum of every record, 2 counters each.  partial: place_scan_tiles(total) + 1 words.
uint64_t place_scan_tiles(uint64_t total);
hipError_t launch_place_profile(const unsigned long long *diff, uint64_t total, const uint64_t *rec_start, uint32_t n_rec, unsigned long long *partial,
                                uint32_t *depth, unsigned long long *rec_sums, hipStream_t st);

// The pile-up called, per position p < B.total: out[p] (optional) = the four counters of pile clamped at PLACE_CLAMP; consensus[p]
// (optional) = the letter with strictly the most bases in upper case when at least min_depth bases lie there, 'N' when the most is tied,
// else the bait's own letter in lower case ('n' for an invalid one: B.runlen[p] == 0).  rec_sums (optional, zeroed by the caller): bases,
// matches, mismatches, called, ambiguous, variants of every record, PILE_SUMS counters each.
struct PileOut { uint32_t a, c, g, t; };                 // mf_pileup_t
hipError_t launch_pileup_call(const unsigned long long *pile, const BaitView &B, const uint64_t *rec_start, uint32_t n_rec, uint32_t min_depth,
                              PileOut *out, uint8_t *consensus, unsigned long long *rec_sums, hipStream_t st);

// The gapped consensus called (include/mitofilter.h, "gapped consensus") from the counters of an aligning placement: diff (total + 1, as
// launch_place_profile takes them; partial: place_scan_tiles(total) + 1 words, the scan is made here), indel (ALIGN_POSITION_COUNTERS a
// position), ins_pile (4 * span counters a position; null only when span is 0) and the called consensus bytes.  Per position p: ins_out
// (optional) = its span entries of ins_pile clamped at PLACE_CLAMP; count[p] = the bytes it emits, 0 .. 1 + span; bytes[p * (1 + span) ..]
// = those bytes.  rec_sums (optional, zeroed by the caller): length, deleted, insertions, inserted_bases of every record (GAPPED_SUMS).
hipError_t launch_gapped_call(const unsigned long long *diff, uint64_t total, const unsigned long long *indel, const unsigned long long *ins_pile, uint32_t span,
                              const uint8_t *consensus, const uint64_t *rec_start, uint32_t n_rec, uint32_t min_depth, unsigned long long *partial,
                              PileOut *ins_out, uint8_t *count, uint8_t *bytes, unsigned long long *rec_sums, hipStream_t st);

// The ends of the records called (include/mitofilter.h, "extended records") from the extension pile of an extending placement: ext_pile,
// 4 * extend counters an end, [record][begin, end][offset][A, C, G, T].  Per end (2 * n_rec of them, `extend` columns each): ext_out
// (optional) = its columns clamped at PLACE_CLAMP; bytes[end * extend ..] = the bytes of the columns it emits, by offset; sums
// [EXTEND_END_SUMS * end] = how many it emits, then the unclamped sum of all its counts.
hipError_t launch_extend_call(const unsigned long long *ext_pile, uint32_t extend, uint32_t n_rec, uint32_t min_depth, PileOut *ext_out, uint8_t *bytes,
                              unsigned long long *sums, hipStream_t st);

} // namespace mf
