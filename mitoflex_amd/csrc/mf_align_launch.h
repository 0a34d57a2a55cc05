// Launcher of mf_align.hip: placement as launch_place does it, then every placed read aligned to its record inside a band of diagonals
// (mf_align.h); the cut, the counters and the pile-up follow the alignment (internal to libmitofilter_hip).
#pragma once
#include "mf_place.h"

namespace mf {

struct AlignOut { uint32_t compared, mismatches, insertions, deletions; int32_t ref_begin, ref_end; };       // mf_align_t
constexpr uint32_t ALIGN_SUMS = 5;             // counters a record: compared, mismatches, insertions, deletions, gapped of its accepted reads
constexpr uint32_t ALIGN_INDEL = 3;            // counters a position: del, ins, ins_bases

// The aligning launch: a cutting launch (PlaceCut; cut.sums: ALIGN_SUMS counters a record) and  band: 0 .. 31.  align (optional): n_reads
// entries, zeroed.  indel: ALIGN_INDEL counters a position, [position][del, ins, ins_bases].  work: align_work_words(max_len) words for
// each of align_waves(..) waves -- the direction bits of a read's band and what the traceback leaves per read base; max_len: no listed
// read is longer.  ins_pile (optional; the gapped launch): 4 * 2 * band counters a position, [position][run offset][A, C, G, T], zeroed --
// the letters of the inserted bases of the accepted reads; everything else is the plain launch's.
// ext_pile, extend (optional; the extending launch, a gapped one): 4 * 2 * extend counters a record, [record][begin, end][offset][A, C, G, T],
// zeroed -- the bases of the accepted reads' diagonal steps outside their record, below `extend` columns from it.
struct PlaceAlign {
    PlaceCut cut; uint32_t band; AlignOut *align; unsigned long long *indel;
    unsigned long long *work; uint64_t max_len;
    unsigned long long *ins_pile;
    unsigned long long *ext_pile = nullptr; uint32_t extend = 0;
};
// 64-bit words of work memory a wave needs for reads of up to max_len bases: two direction bits a cell (64 lanes x 32 rows a block of
// 64 words), then one word a read base
uint64_t align_work_words(uint64_t max_len);
// the waves of the launch: launch_place's shape, fewer where their work memory would pass ALIGN_WORK_BYTES (never fewer than one
// workgroup's): the memory is bounded whatever the number of reads
uint64_t align_waves(uint64_t n_reads, uint64_t max_len, int n_cu);
// The arguments of launch_place; counts holds what a verifying launch's holds (the bins are those of min(edits, 31)).
hipError_t launch_align(const ReadsView &R, const KmerSetView &S, const Anchor *anchor, const uint64_t *rec_start, const uint32_t *list,
                        const unsigned long long *n_list, uint32_t n_rec, PlaceOut *place, unsigned long long *diff, unsigned long long *counts,
                        unsigned long long *pile, const PlaceAlign &align, int n_cu, hipStream_t st);

} // namespace mf
