// The banded alignment of a placed read against its record (include/mitofilter.h, "banded alignment"): the scalar pieces of the rule.
// Plain integer code that the alignment kernel (mf_align.hip) and the CPU model check (tests/native/align_model_check.cpp) both compile,
// as mf_score.h is: nothing here needs a HIP include on the host side.
//
// A read of L bases, oriented to the bait's forward strand (x[0 .. L)), is placed at `start` on the record that begins at position s0 of
// the bait and has len positions.  Cell (i, c), 0 <= i <= L, lies on diagonal d = c - (start + i); the band holds |d| <= W.
//   D(0, c) = 0;   D(i, c) = min( D(i-1, c-1) + sub(i-1, c-1),   D(i-1, c) + 1 [insertion],   D(i, c-1) + 1 [deletion] )
// Every cell of the band is reached by its own diagonal, so D(i, c) <= i: only the neighbours outside the band are infinite.
#pragma once
#include "mf_score.h"
#include "mf_call.h"          // gapped_call_position: the gapped consensus' other scalar piece, beside align_run_offset here

namespace mf {

constexpr uint32_t ALIGN_MAX_BAND = 31;        // 2 W + 1 diagonals fit a 64-wide wave
constexpr uint32_t ALIGN_X_NONE = 4;           // an oriented read letter that is no letter (N)
enum : uint32_t { ALIGN_DIAG = 0, ALIGN_DEL = 1, ALIGN_INS = 2 };          // the move INTO a cell, two bits a cell

// band: 0 .. min(31, k - 1)
MF_SCORE_HD bool align_band_ok(uint32_t band, int k) { return band <= ALIGN_MAX_BAND && (int)band < k; }

// sub(x, c) and whether the column is compared: not compared (and free) outside [0, len), for a read N and on an invalid bait letter.
// No address is formed for a coordinate outside the record, whatever lies beside it in the bait.
MF_SCORE_HD uint32_t align_sub(uint32_t x, int64_t c, int64_t len, const ScoreBait &B, uint64_t s0, bool &compared)
{
    compared = false;
    if (x >= ALIGN_X_NONE || c < 0 || c >= len) return 0;
    const uint64_t g = s0 + (uint64_t)c;
    if (!((B.valid[g >> 5] >> ((uint32_t)g & 31u)) & 1u)) return 0;
    compared = true;
    return ((B.words[g >> 4] >> (2u * ((uint32_t)g & 15u))) & 3u) != x;
}

// The move that a cell of value D is entered by: the first that reproduces D of diagonal (its candidate value `diag`), deletion (from the
// cell to its left in the row, of value `left`, where the band has one) and insertion.
MF_SCORE_HD uint32_t align_move(uint32_t D, uint32_t diag, bool has_left, uint32_t left)
{
    return D == diag ? ALIGN_DIAG : has_left && D == left + 1u ? ALIGN_DEL : ALIGN_INS;
}

// What the traceback leaves for read base b, one word: the column the path enters row b + 1 at (low 32 bits), whether base b was inserted
// (bit 32), how many bait positions row b + 1 deletes behind it (from bit 33).  So (ent >> 32) == 1: inserted, and its row deleted nothing.
// The offset of the inserted base b inside its run of insertions (the gapped consensus, include/mitofilter.h): the number of directly
// preceding bases that were inserted and whose rows deleted nothing.  A run stays in one column and moves one diagonal a step, so the
// band holds it below span = 2 W; the walk stops at span whatever the words say, and a result that is not below span is stored nowhere.
MF_SCORE_HD uint32_t align_run_offset(const unsigned long long *ent, uint64_t b, uint32_t span)
{
    uint32_t t = 0;
    while (t < span && (uint64_t)t < b && (ent[b - 1 - t] >> 32) == 1ull) t++;
    return t;
}

// The end cell is the cell of row L with the least key: least D, then least |d| (d = c - (start + L)), then the smaller c.
MF_SCORE_HD uint64_t align_end_key(uint32_t D, int d)
{
    return ((uint64_t)D << 8) | ((uint64_t)(d < 0 ? -d : d) << 1) | (d > 0 ? 1u : 0u);
}
MF_SCORE_HD int align_end_diagonal(uint64_t key)
{
    const int a = (int)((key >> 1) & 127u);
    return (key & 1u) ? a : -a;
}

// the cut: edits over the columns of the alignment
MF_SCORE_HD bool align_accepts(uint32_t compared, uint32_t mismatches, uint32_t insertions, uint32_t deletions, uint32_t max_permille)
{
    return ((uint64_t)mismatches + insertions + deletions) * 1000u <= (uint64_t)max_permille * ((uint64_t)compared + insertions + deletions);
}

} // namespace mf
