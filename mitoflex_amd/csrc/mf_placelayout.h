// Where a placement-family call (mf_place, mf_pileup, mf_verify and their file-level calls) keeps what on the device: the counters its
// kernels add into (PlaceLayout) and what its report works in (ReportScratch), as pure functions of plain values.  Host-only (no HIP
// include): tests/test_placelayout.py holds every offset here to a restatement of its own without a device.
#pragma once
#include "../../include/mitofilter.h"
#include <stddef.h>
#include <algorithm>
namespace mf {
constexpr uint32_t SCORE_BINS = 32;                      // MF_SCORE_BINS
constexpr uint32_t SCORE_GATHERED = 1 + SCORE_BINS;      // counters a record that a verifying launch gathers behind placement's: rejected, the bins
constexpr uint32_t PILE_SUMS = 6;                        // counters a record of the call kernel's sums: the fields of mf_pileup_record_t
constexpr uint32_t ALIGN_RECORD_SUMS = 5;                // an aligning placement's sums a record: compared, mismatches, insertions, deletions, gapped
constexpr uint32_t ALIGN_POSITION_COUNTERS = 3;          // ... and its counters a position: del, ins, ins_bases (mf_indel_t)

// The counters of a placement, one array of 64-bit words: [pile-up counters | difference counters | record counters].  The four pile-up
// counters a position (only with a pile-up) come FIRST because the call kernel reads them 16 bytes at a time: at the front of an
// allocation they are aligned whatever the other two counts are (and a base that a faulty clip let through would still land inside the
// array).  Then the difference counters (positions + 1), then forward / reverse / over_begin / over_end of every record and the passing
// reads that are not placed (4 R + 1).  A verifying placement keeps a fourth section behind them: rejected and the MF_SCORE_BINS bins of
// every record (what the kernel gathers with the record counters, SCORE_GATHERED R), then compared and mismatches of every record (2 R).
// An ALIGNING placement (mf_align; it is a verifying one) keeps the wider sums there -- compared, mismatches, insertions, deletions, gapped
// of every record (ALIGN_RECORD_SUMS R) -- and a fifth section behind them: del, ins, ins_bases of every position.
// A GAPPED aligning placement (mf_align_gapped with the insertion pile or the gapped consensus asked for) keeps a sixth section behind
// the indel counters: the insertion pile, 4 * span words a position (span = 2 * band), [position][run offset][A, C, G, T].
// An EXTENDING placement (mf_align_extended with extend > 0 and an extension output asked for; it is a gapped one) keeps a seventh section
// behind the insertion pile: the extension pile, 4 * 2 * extend words a record, [record][begin, end][offset][A, C, G, T].
// Every offset into the array is computed here.
struct PlaceLayout {
    size_t n_pile, n_diff, n_cnt, n_rec; bool verify; uint32_t max_permille; bool align; uint32_t band; size_t n_indel, n_ins; uint32_t extend; size_t n_ext;
    PlaceLayout(uint64_t positions, size_t n_rec_, bool pileup, bool verify_, uint32_t max_permille_, bool align_ = false, uint32_t band_ = 0, bool gapped = false,
                uint32_t extend_ = 0)
        : n_pile(pileup ? 4 * (size_t)positions : 0), n_diff((size_t)positions + 1), n_cnt(4 * n_rec_ + 1), n_rec(n_rec_), verify(verify_), max_permille(max_permille_),
          align(align_), band(band_), n_indel(align_ ? ALIGN_POSITION_COUNTERS * (size_t)positions : 0),
          n_ins(align_ && gapped ? 4 * (size_t)(2 * band_) * (size_t)positions : 0), extend(align_ && gapped ? extend_ : 0),
          n_ext(4 * 2 * (size_t)extend * n_rec_) {}
    size_t n_sums() const { return align ? ALIGN_RECORD_SUMS : 2; }
    size_t n_score() const { return verify ? ((size_t)SCORE_GATHERED + n_sums()) * n_rec : 0; }
    size_t words() const { return n_pile + n_diff + n_cnt + n_score() + n_indel + n_ins + n_ext; }
    unsigned long long *ext(unsigned long long *base) const { return n_ext ? cnt(base) + n_cnt + n_score() + n_indel + n_ins : nullptr; }
    uint32_t span() const { return 2 * band; }
    unsigned long long *ins(unsigned long long *base) const { return n_ins ? cnt(base) + n_cnt + n_score() + n_indel : nullptr; }
    unsigned long long *indel(unsigned long long *base) const { return n_indel ? cnt(base) + n_cnt + n_score() : nullptr; }
    unsigned long long *pile(unsigned long long *base) const { return n_pile ? base : nullptr; }
    unsigned long long *diff(unsigned long long *base) const { return base + n_pile; }
    unsigned long long *cnt(unsigned long long *base) const { return base + n_pile + n_diff; }
    unsigned long long *score_sums(unsigned long long *base) const { return cnt(base) + n_cnt + (size_t)SCORE_GATHERED * n_rec; }
    // the score section as it is downloaded (n_score() words from cnt(base) + n_cnt) into the records; accepted from the placement counters
    void score_records(const unsigned long long *h_cnt, mf_score_record_t *out) const
    {
        const unsigned long long *g = h_cnt + n_cnt, *sums = g + (size_t)SCORE_GATHERED * n_rec;
        for (size_t j = 0; j < n_rec; j++) {
            out[j].accepted = h_cnt[4 * j] + h_cnt[4 * j + 1]; out[j].rejected = g[SCORE_GATHERED * j];
            out[j].compared = sums[2 * j]; out[j].mismatches = sums[2 * j + 1];
            for (uint32_t b = 0; b < SCORE_BINS; b++) out[j].hist[b] = g[SCORE_GATHERED * j + 1 + b];
        }
    }
    // the same section of an aligning placement into its records
    void align_records(const unsigned long long *h_cnt, mf_align_record_t *out) const
    {
        const unsigned long long *g = h_cnt + n_cnt, *sums = g + (size_t)SCORE_GATHERED * n_rec;
        for (size_t j = 0; j < n_rec; j++) {
            const unsigned long long *s = sums + ALIGN_RECORD_SUMS * j;
            out[j].accepted = h_cnt[4 * j] + h_cnt[4 * j + 1]; out[j].rejected = g[SCORE_GATHERED * j];
            out[j].compared = s[0]; out[j].mismatches = s[1]; out[j].insertions = s[2]; out[j].deletions = s[3]; out[j].gapped = s[4];
            for (uint32_t b = 0; b < SCORE_BINS; b++) out[j].hist[b] = g[SCORE_GATHERED * j + 1 + b];
        }
    }
};

// What the report of a placement works in, two device buffers cut into sections (byte offset and size; an absent section has size 0).
// The "sums" buffer (64-bit words): placement's work words -- covered and base_sum of every record (2 R), then the scan's partials
// (scan_tiles + 1, scan_tiles being place_scan_tiles(positions)) -- then the pile-up's record sums (PILE_SUMS a record).  The
// "positions" buffer: the called pile-up FIRST, because the call kernel writes it 16 bytes an entry, then the base depth (u32), then the
// consensus (bytes), then 16 spare bytes behind it.  place: base depth or placement records are asked for; pile: the layout holds a
// pile-up.  A resident call cuts the sections out of the read set's cached buffers (d_rsum, d_rpos), a file-level call out of two
// temporaries of its own.  A gapped call (gapped_span >= 0, the span of its insertion pile) has three sections more behind the spare
// bytes of the positions buffer, the first at a multiple of 16 -- the clamped insertion pile (span entries a position), the number of
// bytes every position emits, those bytes (1 + span a position) -- and its record sums (GAPPED_SUMS a record) at the end of the sums
// buffer.  An extending call (extend > 0; it is a gapped one) has two sections more behind those, the first at a multiple of 16 -- the
// clamped extension pile (extend entries an end, two ends a record), the bytes every end emits (extend an end) -- and its sums
// (EXTEND_END_SUMS an end) at the end of the sums buffer.  Every offset is computed here.
constexpr uint32_t EXTEND_END_SUMS = 2;                  // counters an end of the extension call: emitted columns, piled bases
constexpr uint32_t GAPPED_SUMS = 4;                      // counters a record of the gapped call: the fields of mf_gapped_record_t
struct ReportScratch {
    struct Section {
        size_t off = 0, bytes = 0;
        template <class T> T *in(void *buf) const { return bytes ? reinterpret_cast<T *>(static_cast<uint8_t *>(buf) + off) : nullptr; }
    };
    Section work, pile_sums;                           // of the sums buffer
    Section pile_out, depth, consensus, spare;         // of the positions buffer
    Section gap_sums;                                  // of the sums buffer, a gapped call
    Section ins_out, gap_count, gap_bytes;             // of the positions buffer, a gapped call
    Section ext_sums;                                  // of the sums buffer, an extending call
    Section ext_out, ext_bytes;                        // of the positions buffer, an extending call
    size_t sums_bytes, pos_bytes;
    ReportScratch(uint64_t positions, size_t n_rec, uint64_t scan_tiles, bool place, bool pile, int gapped_span = -1, uint32_t extend = 0)
    {
        const size_t P = (size_t)std::max<uint64_t>(positions, 1), R = std::max<size_t>(n_rec, 1);
        size_t at = 0;
        auto put = [&at](Section &s, size_t bytes) { s.off = at; s.bytes = bytes; at += bytes; };
        put(work, place ? (2 * n_rec + (size_t)scan_tiles + 1) * 8 : 0);
        put(pile_sums, pile ? PILE_SUMS * R * 8 : 0);
        put(gap_sums, gapped_span >= 0 ? GAPPED_SUMS * R * 8 : 0);
        put(ext_sums, gapped_span >= 0 && extend ? EXTEND_END_SUMS * 2 * R * 8 : 0);
        sums_bytes = at; at = 0;
        put(pile_out, pile ? P * sizeof(mf_pileup_t) : 0);
        put(depth, place ? P * 4 : 0);
        put(consensus, pile ? P : 0);
        put(spare, pile ? 16 : 0);
        if (gapped_span >= 0) {
            const size_t span = (size_t)gapped_span;
            at = (at + 15) / 16 * 16;
            put(ins_out, P * span * sizeof(mf_pileup_t));
            put(gap_count, P);
            put(gap_bytes, P * (1 + span));
            if (extend) {
                at = (at + 15) / 16 * 16;
                put(ext_out, 2 * R * (size_t)extend * sizeof(mf_pileup_t));
                put(ext_bytes, 2 * R * (size_t)extend);
            }
        }
        pos_bytes = at;
    }
};
} // namespace mf
