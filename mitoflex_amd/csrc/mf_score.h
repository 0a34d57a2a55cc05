// The score of a placed read against the bait, sixteen bases at a time (include/mitofilter.h, "verification").  Plain integer code that
// the placement kernel (mf_place.hip) and the CPU model check (tests/native/score_model_check.cpp) both compile: nothing here needs a
// HIP include on the host side.
//
// A read of L bases whose first base is base b0 of the packed read stream lies on strand `strand` with its leftmost base at record
// coordinate `start` of the record that begins at position s0 of the bait and has len positions.  Its footprint clipped to the record is
// [lo, hi) = [max(start, 0), min(start + L, len)): never empty for a placed read.  Chunk t of the footprint holds the record
// coordinates lo + 16 t .. lo + 16 t + 15 below hi; score_chunk16 compares them in one go:
//   y   the bait's sixteen letters from s0 + c0, funnel-shifted out of two words of the packed bait;
//   x   the read's sixteen letters that lie on them.  Strand 0: read offsets c0 - start upwards, funnel-shifted out of two words of the
//       stream.  Strand 1: read offsets start + L - 1 - c0 DOWNWARDS, complemented -- the window that ends there, mirrored and
//       complemented (not, bit reverse, pair swap).  Where that window would begin before the read (the footprint's last, partial chunk)
//       it is taken from the read's first base and the mirrored word shifted down by what is missing: no address before b0 is formed.
//   m   one bit a base, at the even bit of its pair: base below hi AND the bait letter valid (the packed validity mask, one bit a
//       position, funnel-shifted and spread).
// mismatches = popcount(((x ^ y) | ((x ^ y) >> 1)) & m), compared = popcount(m).  Read Ns are NOT looked at here: a read with an invalid
// base goes base by base (score_base).
//
// Memory safety: the second word of each funnel read may lie behind the last word that holds data.  Every index is clamped to the last
// word of its array (r_last, b_last, v_last); a clamped word only ever supplies bits that the mask drops.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MF_SCORE_HD __host__ __device__ inline
#else
#define MF_SCORE_HD inline
#endif

namespace mf {

struct ScoreBait {
    const uint32_t *words;      // the bait's letters, 16 a word
    uint64_t b_last;            // index of the last word of `words`
    const uint32_t *valid;      // bit p & 31 of word p >> 5: the bait letter at p is valid
    uint64_t v_last;            // index of the last word of `valid`
};

MF_SCORE_HD uint32_t score_popc(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}
MF_SCORE_HD uint32_t score_brev(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    return (v >> 16) | (v << 16);
#endif
}
// the reverse complement of sixteen packed bases
MF_SCORE_HD uint32_t score_revcomp16(uint32_t x)
{
    const uint32_t y = score_brev(~x);
    return (0xAAAAAAAAu & (y << 1)) | (0x55555555u & (y >> 1));
}
// 32 bits of the stream w from bit `bit` of word `word` on; the second word's index clamped to `last`
MF_SCORE_HD uint32_t score_funnel(const uint32_t *w, uint64_t word, uint32_t bit, uint64_t last)
{
    const uint64_t i0 = word < last ? word : last, i1 = word + 1 < last ? word + 1 : last;
    return (uint32_t)((((uint64_t)w[i1] << 32) | w[i0]) >> bit);
}
// the low sixteen bits, each moved to the even bit of a pair
MF_SCORE_HD uint32_t score_spread16(uint32_t v)
{
    v &= 0xFFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    return (v | (v << 1)) & 0x55555555u;
}

// the clipped footprint [lo, hi) of a read of L bases at `start` on a record of len positions
MF_SCORE_HD void score_footprint(uint64_t L, int64_t start, int64_t len, int64_t &lo, int64_t &hi)
{
    lo = start > 0 ? start : 0;
    hi = start + (int64_t)L < len ? start + (int64_t)L : len;
}

// Chunk t of the footprint (16 t < hi - lo): compared in the low half, mismatches in the high half of the result.
// rwords: the read stream, r_last the index of its last word.
MF_SCORE_HD uint64_t score_chunk16(const uint32_t *rwords, uint64_t r_last, uint64_t b0, uint64_t L, uint32_t strand, int64_t start, const ScoreBait &B,
                                   uint64_t s0, int64_t lo, int64_t hi, uint64_t t)
{
    const int64_t c0 = lo + 16 * (int64_t)t;
    const int64_t left = hi - c0;
    const uint32_t n = left < 16 ? (uint32_t)left : 16u;
    const uint64_t g = s0 + (uint64_t)c0;                                       // (c0 >= 0: the clip came first)
    const uint32_t y = score_funnel(B.words, g >> 4, 2u * ((uint32_t)g & 15u), B.b_last);
    const uint32_t v = score_funnel(B.valid, g >> 5, (uint32_t)g & 31u, B.v_last);
    uint32_t x;
    if (!strand) {
        const uint64_t rg = b0 + (uint64_t)(c0 - start);
        x = score_funnel(rwords, rg >> 4, 2u * ((uint32_t)rg & 15u), r_last);
    } else {
        const int64_t a = start + (int64_t)L - 1 - c0 - 15;                     // the read offset the mirrored window begins at
        const uint32_t miss = a < 0 ? (uint32_t)(-a) : 0u;                      // (only in the footprint's last chunk: miss <= 15)
        const uint64_t rg = b0 + (uint64_t)(a < 0 ? 0 : a);
        x = score_revcomp16(score_funnel(rwords, rg >> 4, 2u * ((uint32_t)rg & 15u), r_last)) >> (2u * miss);
    }
    const uint32_t m = score_spread16(v) & (n < 16 ? (1u << (2u * n)) - 1u : 0xFFFFFFFFu);
    const uint32_t d = x ^ y;
    return ((uint64_t)score_popc((d | (d >> 1)) & m) << 32) | score_popc(m);
}

// One base, for reads that hold an invalid base: read offset i (a valid base) -> the same packed pair, or 0 where it is not compared.
MF_SCORE_HD uint64_t score_base(const uint32_t *rwords, uint64_t b0, uint64_t L, uint32_t strand, int64_t start, const ScoreBait &B, uint64_t s0, int64_t len,
                                uint64_t i)
{
    const uint64_t rg = b0 + i;
    uint32_t letter = (rwords[rg >> 4] >> (2u * ((uint32_t)rg & 15u))) & 3u;
    int64_t c = start + (int64_t)i;
    if (strand) { c = start + (int64_t)(L - 1 - i); letter ^= 3u; }
    if (c < 0 || c >= len) return 0;
    const uint64_t g = s0 + (uint64_t)c;
    if (!((B.valid[g >> 5] >> ((uint32_t)g & 31u)) & 1u)) return 0;
    const uint32_t bl = (B.words[g >> 4] >> (2u * ((uint32_t)g & 15u))) & 3u;
    return ((uint64_t)(letter != bl) << 32) | 1u;
}

// the cut: a placed read with these counts is accepted
MF_SCORE_HD bool score_accepts(uint32_t compared, uint32_t mismatches, uint32_t max_permille)
{
    return (uint64_t)mismatches * 1000u <= (uint64_t)max_permille * compared;
}

// The keep rule (include/mitofilter.h, "which mates are written"): a PASSING read loses its bit in the keep bitmap when this is true.
// keep 0 (MF_KEEP_PASSING): never.  1 (MF_KEEP_ACCEPTED): placed and rejected by the cut.  2 (MF_KEEP_PLACED): that, or not placed
// (ambiguous, no anchor).  `accepted` means nothing for a read that is not placed.
MF_SCORE_HD bool keep_clears(bool placed, bool accepted, int keep)
{
    return keep == 1 ? placed && !accepted : keep == 2 ? !placed || !accepted : false;
}

} // namespace mf
