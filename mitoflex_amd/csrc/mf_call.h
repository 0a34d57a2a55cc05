// The call rules of the placement family, position by position (include/mitofilter.h, "pile-up" and "gapped consensus").  Plain integer
// code that the call kernels (mf_place.hip), the host report (mf_report.cpp) and the CPU model checks (tests/native/pileup_model_check.cpp,
// gapped_model_check.cpp) all compile, as mf_score.h is: nothing here needs a HIP include on the host side.
#pragma once
#include "mf_score.h"          // MF_SCORE_HD

namespace mf {

constexpr uint32_t PLACE_CLAMP = 0xFFFFFFFEu;        // the largest depth or count reported
constexpr uint32_t CALL_LETTERS = 0x54474341u;       // "ACGT", letter l in byte l

// a 64-bit counter as it is reported; every call below goes by the UNCLAMPED counters
MF_SCORE_HD uint32_t clamp_count(unsigned long long c) { return c < PLACE_CLAMP ? (uint32_t)c : PLACE_CLAMP; }

// the letter with strictly the most bases: best = the first letter that holds the maximum, tied = another letter holds it too
MF_SCORE_HD void strict_most4(unsigned long long c0, unsigned long long c1, unsigned long long c2, unsigned long long c3, uint32_t &best, bool &tied)
{
    unsigned long long m = c0;
    best = 0; tied = false;
    if (c1 > m) { m = c1; best = 1; tied = false; } else if (c1 == m) tied = true;
    if (c2 > m) { m = c2; best = 2; tied = false; } else if (c2 == m) tied = true;
    if (c3 > m) { m = c3; best = 3; tied = false; } else if (c3 == m) tied = true;
}

// The call of the pile-up at one position: c0 .. c3 its bases by letter, b the bait's letter there (0 .. 3; means nothing unless valid).
// consensus: the letter with strictly the most bases in upper case when at least min_depth bases lie there, 'N' when the most is tied,
// else the bait's own letter in lower case ('n' for an invalid one).  depth and own (the bases that show the bait's letter) are what the
// record sums add; a variant is a called position whose letter is not the bait's valid one.
struct PileCall { uint8_t consensus; bool called, ambiguous, variant; unsigned long long depth, own; };
MF_SCORE_HD PileCall pileup_call_position(unsigned long long c0, unsigned long long c1, unsigned long long c2, unsigned long long c3, uint32_t b, bool valid,
                                          uint32_t min_depth)
{
    uint32_t best; bool tied;
    strict_most4(c0, c1, c2, c3, best, tied);
    PileCall r;
    r.depth = c0 + c1 + c2 + c3;
    const bool deep = r.depth >= (unsigned long long)min_depth;
    r.consensus = (uint8_t)(deep ? (tied ? (uint32_t)'N' : (CALL_LETTERS >> (8 * best)) & 255u)
                                 : (valid ? ((CALL_LETTERS >> (8 * b)) & 255u) | 0x20u : (uint32_t)'n'));
    r.own = b == 0 ? c0 : b == 1 ? c1 : b == 2 ? c2 : c3;
    r.called = deep && !tied;
    r.ambiguous = deep && tied;
    r.variant = deep && !tied && valid && best != b;
    return r;
}

// The call of the gapped consensus at one position, from unclamped sums: D the base depth, del the position's deletion counter, ins its
// 4 * span insertion counters [offset][A, C, G, T] (not read when span is 0), cons its consensus byte.  Writes the emitted bytes to out
// (room for 1 + span) and returns how many; deleted: the position emits no byte of its own.  Both majorities are strict.
MF_SCORE_HD uint32_t gapped_call_position(unsigned long long D, unsigned long long del, const unsigned long long *ins, uint32_t span, uint32_t min_depth,
                                          uint8_t cons, uint8_t *out, bool &deleted)
{
    const bool deep = D >= (unsigned long long)min_depth;
    deleted = span != 0 && deep && 2 * del > D;          // (band 0: nothing is deleted)
    uint32_t m = 0;
    if (!deleted) out[m++] = cons;
    for (uint32_t q = 0; deep && q < span; q++) {          // the columns are emitted up to the first that is not
        const unsigned long long c0 = ins[4 * q], c1 = ins[4 * q + 1], c2 = ins[4 * q + 2], c3 = ins[4 * q + 3];
        if (!(2 * (c0 + c1 + c2 + c3) > D)) break;
        uint32_t best; bool tied;
        strict_most4(c0, c1, c2, c3, best, tied);
        out[m++] = (uint8_t)(tied ? 'N' : (CALL_LETTERS >> (8 * best)) & 255u);
    }
    return m;
}

// The extension of a record's ends (include/mitofilter.h, "extended records").  A record coordinate c outside [0, len) lies at offset
// -1 - c of the begin (side 0) or c - len of the end (side 1); offset 0 is the column next to the record.
MF_SCORE_HD uint64_t extend_offset(int64_t c, int64_t len, uint32_t &side)
{
    side = c < 0 ? 0u : 1u;
    return c < 0 ? (uint64_t)(-1 - c) : (uint64_t)(c - len);
}
// the entry of (record j, side, offset e < E) in a table of E columns an end, two ends a record
MF_SCORE_HD uint64_t extend_entry(uint64_t j, uint32_t side, uint32_t E, uint64_t e) { return (2 * j + side) * (uint64_t)E + e; }
// The call at one column, from unclamped counts: emitted iff at least min_depth bases lie there and exactly one letter has the most;
// byte: that letter in upper case.  An end emits its columns up to the first that is not.
MF_SCORE_HD bool extend_call_column(unsigned long long c0, unsigned long long c1, unsigned long long c2, unsigned long long c3, uint32_t min_depth, uint8_t &byte)
{
    uint32_t best; bool tied;
    strict_most4(c0, c1, c2, c3, best, tied);
    byte = (uint8_t)((CALL_LETTERS >> (8 * best)) & 255u);
    return c0 + c1 + c2 + c3 >= (unsigned long long)min_depth && !tied;
}

} // namespace mf
