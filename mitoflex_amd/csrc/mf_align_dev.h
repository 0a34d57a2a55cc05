// Device-side pieces of the banded alignment that the kernels of mf_align.hip and mf_pairs.hip both build on: the alignment of one placed
// read by a whole wave (align_read, the rule of mf_align.h -- rows, moves, end, traceback and counts as mf_align.hip's head describes
// them) and what an accepted aligned read adds per position (align_adds).  align_kernel aligns a read on the diagonal its vote won;
// rescue_align_kernel of mf_pairs.hip aligns a rescued mate on the diagonal of its winning candidate.
#pragma once
#include "mf_align_launch.h"
#include "mf_vote_dev.h"
#include "mf_align.h"

namespace mf {

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) { return ~wave_max_u64(~v); }

// base i of the read oriented to the bait's forward strand: 0 .. 3, or ALIGN_X_NONE for an N
static_assert(ALIGN_X_NONE == READ_LETTER_NONE, "an N is the same value in both");
__device__ __forceinline__ uint32_t oriented_base(const ReadsView &R, uint64_t b0, bool hasn, uint64_t L, uint32_t strand, uint64_t i)
{
    const uint32_t letter = read_letter(R, b0 + (strand ? L - 1 - i : i), hasn);
    return strand && letter != READ_LETTER_NONE ? letter ^ 3u : letter;
}

struct AlignResult { uint32_t compared, mismatches, insertions, deletions; int64_t ref_begin, ref_end; };

// what the traceback leaves for a read base: the column (low word), inserted (bit 32), deleted positions behind it (from bit 33)
__device__ __forceinline__ int64_t ent_column(unsigned long long e) { return (int64_t)(int32_t)(uint32_t)e; }
__device__ __forceinline__ bool ent_inserted(unsigned long long e) { return (e >> 32) & 1u; }
__device__ __forceinline__ uint32_t ent_deleted(unsigned long long e) { return (uint32_t)(e >> 33); }

// The whole wave aligns one placed read; every lane returns the same result.  dirs, ent: the wave's work memory.
__device__ __forceinline__ AlignResult align_read(const ReadsView &R, uint64_t b0, bool hasn, uint64_t L, uint32_t strand, int64_t start, uint64_t s0,
                                                  int64_t len, const ScoreBait &B, int W, unsigned long long *dirs, unsigned long long *ent, int lane)
{
    const int d = lane - W;
    const bool active = lane <= 2 * W;
    uint32_t prev = 0, xv = ALIGN_X_NONE;
    unsigned long long bits = 0;
    for (uint64_t i = 1; i <= L; i++) {
        const uint64_t b = i - 1;                                   // the read base this row consumes
        if ((b & 63) == 0) xv = b + (uint64_t)lane < L ? oriented_base(R, b0, hasn, L, strand, b + (uint64_t)lane) : ALIGN_X_NONE;
        const uint32_t x = __shfl(xv, (int)(b & 63));
        bool cmp;
        const uint32_t diag = prev + (active ? align_sub(x, start + (int64_t)b + d, len, B, s0, cmp) : 0u);
        const uint32_t up = __shfl_down(prev, 1);                   // D(i - 1, c): the lane above's
        uint32_t t = diag;
        if (lane < 2 * W && up + 1u < t) t = up + 1u;
        uint32_t key = t + (uint32_t)(63 - lane);
        for (int o = 1; o <= 2 * W; o <<= 1) { const uint32_t v = __shfl_up(key, o); if (lane >= o && v < key) key = v; }
        const uint32_t D = key - (uint32_t)(63 - lane);
        const uint32_t left = __shfl_up(D, 1);                      // D(i, c - 1)
        bits |= (unsigned long long)align_move(D, diag, lane > 0, left) << (2 * ((uint32_t)b & 31u));
        if (((uint32_t)b & 31u) == 31u || i == L) { dirs[(b >> 5) * 64 + (uint64_t)lane] = bits; bits = 0; }
        prev = D;
    }
    int dd = align_end_diagonal(wave_min_u64(active ? align_end_key(prev, d) : ~0ull));
    AlignResult a{0, 0, 0, 0, 0, start + (int64_t)L + dd};
    __threadfence_block();                                          // (the wave's own stores, read back below)
    uint64_t i = L;
    uint32_t pend = 0;                                              // deletions of the current row seen so far
    for (uint64_t blk = (L - 1) >> 5;; blk--) {
        const unsigned long long w = dirs[blk * 64 + (uint64_t)lane];
        unsigned long long mine = 0;
        while (i > blk * 32) {
            const uint32_t bi = (uint32_t)(i - 1) & 31u;
            const unsigned long long wd = __shfl(w, dd + W);
            const uint32_t mv = __builtin_amdgcn_readfirstlane((uint32_t)(wd >> (2 * bi)) & 3u);
            if (mv == ALIGN_DEL && dd > -W) { a.deletions++; pend++; dd--; continue; }
            const bool ins = mv == ALIGN_INS && dd < W;
            if ((uint32_t)lane == bi)
                mine = ((unsigned long long)pend << 33) | ((unsigned long long)ins << 32) | (uint32_t)(int32_t)(start + (int64_t)i + dd);
            pend = 0;
            if (ins) { a.insertions++; dd++; }
            i--;
        }
        if (lane < 32 && blk * 32 + (uint64_t)lane < L) ent[blk * 32 + (uint64_t)lane] = mine;
        if (blk == 0) break;
    }
    a.ref_begin = start + dd;
    __threadfence_block();
    unsigned long long acc = 0;
    for (uint64_t b = (uint64_t)lane; b < L; b += 64) {
        const unsigned long long e = ent[b];
        if (ent_inserted(e)) continue;
        bool cmp;
        const uint32_t s = align_sub(oriented_base(R, b0, hasn, L, strand, b), ent_column(e) - 1, len, B, s0, cmp);
        acc += ((unsigned long long)s << 32) | (cmp ? 1u : 0u);
    }
    acc = wave_sum_u64(acc);
    a.compared = __builtin_amdgcn_readfirstlane((uint32_t)acc); a.mismatches = __builtin_amdgcn_readfirstlane((uint32_t)(acc >> 32));
    return a;
}

// What an accepted read adds per position, lane l taking bases l, l + 64, ..: the base of a diagonal step into pile (optional), the
// positions its row deletes into indel[.][0], an inserted base into indel[.][2] and, where it begins a run, indel[.][1].
// GAPPED: the t-th base of an insertion run also into ins_pile[(position) * span + t][letter], span = 2 W; t < span holds the store
// inside the position's own entries whatever the walk counted.
// EXTEND: the base of a diagonal step outside the record, at offset e of an end of record j (extend_offset, mf_call.h), into
// ext_pile[(2 j + side) * E + e][letter] when e < E -- which holds the store inside that end's own entries; it adds nowhere otherwise.
template <bool GAPPED, bool EXTEND>
__device__ __forceinline__ void align_adds(const ReadsView &R, uint64_t b0, bool hasn, uint64_t L, uint32_t strand, uint64_t s0, int64_t len,
                                           const unsigned long long *ent, unsigned long long *__restrict__ pile, unsigned long long *__restrict__ indel,
                                           unsigned long long *__restrict__ ins_pile, uint32_t span, unsigned long long *__restrict__ ext_pile, uint32_t E,
                                           uint32_t j, int lane)
{
    for (uint64_t b = (uint64_t)lane; b < L; b += 64) {
        const unsigned long long e = ent[b];
        const int64_t c = ent_column(e);
        for (uint32_t q = 0; q < ent_deleted(e); q++) {
            const int64_t p = c + (int64_t)q;
            if (p >= 0 && p < len) atomicAdd(&indel[ALIGN_INDEL * (s0 + (uint64_t)p)], 1ull);
        }
        const int64_t p = c - 1;
        if (p < 0 || p >= len) {
            if constexpr (EXTEND) {
                if (ent_inserted(e)) continue;
                uint32_t side;
                const uint64_t off = extend_offset(p, len, side);
                if (off >= (uint64_t)E) continue;
                const uint32_t x = oriented_base(R, b0, hasn, L, strand, b);
                if (x < ALIGN_X_NONE) atomicAdd(&ext_pile[4 * extend_entry(j, side, E, off) + x], 1ull);
            }
            continue;
        }
        if (!ent_inserted(e)) {
            if (!pile) continue;
            const uint32_t x = oriented_base(R, b0, hasn, L, strand, b);
            if (x < ALIGN_X_NONE) atomicAdd(&pile[4 * (s0 + (uint64_t)p) + x], 1ull);
        } else {
            atomicAdd(&indel[ALIGN_INDEL * (s0 + (uint64_t)p) + 2], 1ull);
            // the base before it is of the same run when it was inserted too and its row deleted nothing
            if (!(b > 0 && (ent[b - 1] >> 32) == 1ull)) atomicAdd(&indel[ALIGN_INDEL * (s0 + (uint64_t)p) + 1], 1ull);
            if (GAPPED) {
                const uint32_t t = align_run_offset(ent, b, span);
                const uint32_t x = oriented_base(R, b0, hasn, L, strand, b);
                if (t < span && x < ALIGN_X_NONE) atomicAdd(&ins_pile[4 * ((s0 + (uint64_t)p) * span + t) + x], 1ull);
            }
        }
    }
}

} // namespace mf
