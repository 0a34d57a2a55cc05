// Launchers of mf_assign.hip: which bait record the reads that pass come from (internal to libmitofilter_hip).
#pragma once
#include <hip/hip_runtime.h>
#include "mf_common.h"
#include "mf_kernels.h"

namespace mf {

// owner of a key that more than one record holds (and of an empty slot)
constexpr uint32_t OWNER_SHARED = 0xFFFFFFFFu;
// what a read is assigned when it passes but no record wins (MF_ASSIGN_AMBIGUOUS)
constexpr uint32_t ASSIGN_AMBIGUOUS = 0xFFFFFFFEu;

// Record-owner table, indexed by the slot of the key table: owner[slot] = the one record whose valid windows hold the key, else
// OWNER_SHARED.  rec_start: n_rec + 1 ascending base offsets (record j holds bases [rec_start[j], rec_start[j + 1])).
// rec_group (optional, n_rec words): the group of every record -- the table then holds the one GROUP whose records' valid windows hold
// the key (nullptr: each record is its own group).  hi_scratch: `slots` words.  owner is filled completely; the result does not depend
// on the order the windows arrive in.
hipError_t launch_build_owner(const BaitView &B, const uint64_t *rec_start, uint32_t n_rec, const uint32_t *rec_group, const KmerSetView &S,
                              uint32_t *owner, uint32_t *hi_scratch, hipStream_t st);
// The same for a protein set (S.prot): aa / runlen / total as ProtBaitHost holds them, rec_start in residues.
hipError_t launch_build_powner(const uint8_t *aa, const uint8_t *runlen, uint64_t total, const uint64_t *rec_start, uint32_t n_rec,
                               const uint32_t *rec_group, const KmerSetView &S, uint32_t *owner, uint32_t *hi_scratch, hipStream_t st);
// The passing reads of a pass bitmap as a list of read numbers (any order); *n_list (zeroed by the caller) receives their number.
hipError_t launch_pass_list(const uint32_t *bits, uint64_t n_reads, uint32_t *list, unsigned long long *n_list, hipStream_t st);
// One wave per listed read: u_j over the read's windows, the record with the strictly largest u_j (ASSIGN_AMBIGUOUS: none, or a tie).
// The windows are the valid k-windows of a nucleotide set, or the valid (strand, start) peptide windows of a protein set (S.prot);
// owner may be a group-owner table, n_rec then being the number of groups.
// assign (optional, n_reads words): assign[read]; pairs (optional, one per list entry): (read << 32) | record;
// counts: n_rec + 1 counters (records, then ambiguous), zeroed by the caller.
hipError_t launch_assign(const ReadsView &R, const KmerSetView &S, const uint32_t *owner, const uint32_t *list, const unsigned long long *n_list,
                         uint32_t n_rec, uint32_t *assign, uint64_t *pairs, unsigned long long *counts, int n_cu, hipStream_t st);

// ---- k-mer depth (mf_depth)
constexpr uint32_t DEPTH_NONE = 0xFFFFFFFFu;        // no valid window starts at a position (MF_DEPTH_NONE)
constexpr uint32_t DEPTH_CLAMP = 0xFFFFFFFEu;       // the profile's largest depth
constexpr uint32_t DEPTH_ITEM = 256;                // positions of one work item of the profile kernel at most
struct DepthItem { uint64_t begin; uint32_t len, rec; };       // positions [begin, begin + len) of record `rec`

// Representative table (slot-indexed): rep[slot] = the smallest bait position whose valid window holds the key; pos_rep[p] = rep of the
// window that starts at p, DEPTH_NONE where no valid window does.  Nucleotide sets: B as the table builder takes it (aa unused); protein
// sets (S.prot): aa / B.runlen / B.total as ProtBaitHost holds them (B.words unused).  pos_rep: B.total words (positions below 2^32 - 1).
// by_slot: rep[slot] = slot instead (counters per slot: the scattered form, for measurement; the counters then number `slots`).
hipError_t launch_build_depth(const BaitView &B, const uint8_t *aa, const KmerSetView &S, uint32_t *rep, uint32_t *pos_rep, bool by_slot,
                              hipStream_t st);
// One wave per listed read: atomicAdd of 1 into cnt[rep[slot]] for every window of the read whose key the set holds (the windows of
// launch_assign).  Exactly one of cnt32 / cnt64 is given (the latter when the windows of the read set could reach 2^32).
hipError_t launch_depth_count(const ReadsView &R, const KmerSetView &S, const uint32_t *rep, const uint32_t *list, const unsigned long long *n_list,
                              uint32_t *cnt32, unsigned long long *cnt64, int n_cu, hipStream_t st);
// tot[i] += cnt32[i] for i < n (atomic: several lanes of a device share tot)
hipError_t launch_depth_fold(const uint32_t *cnt32, uint64_t n, unsigned long long *tot, hipStream_t st);
// profile (optional; B.total words) and the per-record sums (optional; 4 words a record: windows, covered, depth_sum, depth_max; zeroed by
// the caller) from the totals; items cover every position of every non-empty record
hipError_t launch_depth_profile(const DepthItem *items, uint32_t n_items, const uint32_t *pos_rep, const unsigned long long *tot, uint32_t *profile,
                                unsigned long long *rec, hipStream_t st);

} // namespace mf
