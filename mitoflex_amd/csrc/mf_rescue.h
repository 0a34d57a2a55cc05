// Mate rescue (include/mitofilter.h, "pairs"): where the candidates of an unplaced mate lie, which of them are admissible, and which one
// wins.  Plain integer code in the manner of mf_score.h, which the rescue kernel (mf_pairs.hip) and the CPU model check
// (tests/native/pair_model_check.cpp) both compile: nothing but these functions decides a rescue.
//
// The settled mate A lies on record j, strand s, at [a, e).  Its mate B of L bases is looked for on record j and on strand 1 - s, one
// candidate per insert d in [min_insert, max_insert]: the pair would then span d positions, from the strand-0 mate's start to the
// strand-1 mate's end.  A candidate is scored by the verification rule (mf_score.h) and is admissible when compared >= k and
// mismatches * 1000 <= rescue_permille * compared.  B is rescued when exactly one admissible candidate has the fewest mismatches.
//
// A lane of the kernel keeps a RescueFold over the candidates it scores (rescue_fold_add), the wave combines its 64 folds pairwise
// (rescue_fold_merge: commutative and associative, so any order of combination gives the same fold) and rescue_wins reads the result.
#pragma once
#include "mf_score.h"

namespace mf {

constexpr uint32_t RESCUE_MAX = 4096;                    // MF_RESCUE_MAX: the most candidates a window holds
constexpr uint32_t RESCUE_NO_CANDIDATE = 0xFFFFFFFFu;    // `mismatches` of a fold that holds no admissible candidate

// the record coordinate of the leftmost base of B's candidate for insert d: B ends where the pair ends when A lies forward, B starts
// where the pair starts when A lies reverse
MF_SCORE_HD int64_t rescue_start(uint32_t s, int64_t a, int64_t e, uint64_t L, uint64_t d)
{
    return s ? e - (int64_t)d : a + (int64_t)d - (int64_t)L;
}

MF_SCORE_HD bool rescue_admissible(uint32_t compared, uint32_t mismatches, uint32_t k, uint32_t rescue_permille)
{
    return compared >= k && score_accepts(compared, mismatches, rescue_permille);
}

// the fewest mismatches among the admissible candidates seen, the smallest insert that reached them, and how many candidates reached
// them (saturating: only 1 and "more than 1" are told apart)
struct RescueFold { uint32_t mismatches, d, n; };

MF_SCORE_HD RescueFold rescue_fold_empty() { return RescueFold{RESCUE_NO_CANDIDATE, 0u, 0u}; }

MF_SCORE_HD RescueFold rescue_fold_merge(const RescueFold &x, const RescueFold &y)
{
    if (x.mismatches != y.mismatches) return x.mismatches < y.mismatches ? x : y;
    if (x.mismatches == RESCUE_NO_CANDIDATE) return x;
    const uint32_t n = x.n + y.n;
    return RescueFold{x.mismatches, x.d < y.d ? x.d : y.d, n < x.n ? 0xFFFFFFFFu : n};
}

// the candidate of insert d with this score, folded into f
MF_SCORE_HD void rescue_fold_add(RescueFold &f, uint32_t compared, uint32_t mismatches, uint32_t d, uint32_t k, uint32_t rescue_permille)
{
    if (rescue_admissible(compared, mismatches, k, rescue_permille)) f = rescue_fold_merge(f, RescueFold{mismatches, d, 1u});
}

MF_SCORE_HD bool rescue_wins(const RescueFold &f) { return f.mismatches != RESCUE_NO_CANDIDATE && f.n == 1u; }

// The score of the candidate at `start` for a read WITHOUT an invalid base: its clipped footprint sixteen bases at a time.  rwords / r_last
// / b0 name the read as score_chunk16 takes it (the stream itself, or a copy of the read's words with b0 reduced to its offset in the
// first of them).  A candidate that misses the record altogether compares nothing.
MF_SCORE_HD uint64_t rescue_score_chunks(const uint32_t *rwords, uint64_t r_last, uint64_t b0, uint64_t L, uint32_t strand, int64_t start, const ScoreBait &B,
                                         uint64_t s0, int64_t len)
{
    int64_t lo, hi;
    score_footprint(L, start, len, lo, hi);
    uint64_t acc = 0;
    if (hi <= lo) return acc;
    const uint64_t chunks = (uint64_t)(hi - lo + 15) >> 4;
    for (uint64_t t = 0; t < chunks; t++) acc += score_chunk16(rwords, r_last, b0, L, strand, start, B, s0, lo, hi, t);
    return acc;
}

// ... and for a read WITH invalid bases, base by base.  nmask: bit i & 31 of word i >> 5 is set when read offset i is invalid.
MF_SCORE_HD uint64_t rescue_score_bases(const uint32_t *rwords, uint64_t b0, uint64_t L, uint32_t strand, int64_t start, const ScoreBait &B, uint64_t s0,
                                        int64_t len, const uint32_t *nmask)
{
    uint64_t acc = 0;
    for (uint64_t i = 0; i < L; i++) {
        if ((nmask[i >> 5] >> ((uint32_t)i & 31u)) & 1u) continue;                  // an N is not compared
        acc += score_base(rwords, b0, L, strand, start, B, s0, len, i);
    }
    return acc;
}

} // namespace mf
