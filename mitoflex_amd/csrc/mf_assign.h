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

} // namespace mf
