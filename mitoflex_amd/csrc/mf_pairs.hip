// Pair-aware placement (gfx950, 64-wide waves): what two placed and scored mate sets say pair by pair, and the rescue of an unplaced
// mate from the window its settled mate implies (include/mitofilter.h, "pairs").
//
//   pair_list_kernel   one thread per pair over both sets' pass bits, the placements of the mates that pass (and their scores where the
//                      cut can reject): a mate is settled when it is placed and accepted.  Both settled: proper, discordant or cross,
//                      with the insert.  None: none.  One: single -- or, in a rescuing call and with the other mate not placed at all, a
//                      rescue target: those are compacted into a list with a ballot and one atomic a wave.  Grid-stride; the records'
//                      counters gather in LDS where they fit.
//   rescue_kernel      one wave per listed pair, grid-stride.  The unplaced mate's packed words are staged once in the wave's slice of
//                      LDS (and, for a read with an N, one bit a base that says where); lanes then take the candidates 64 at a time and
//                      each scores its own with the verification rule of mf_score.h -- sixteen bases at a time over the clipped
//                      footprint, base by base for a read with an N -- and keeps the fold of mf_rescue.h.  One butterfly combines the 64
//                      folds.  A strict winner is committed by lane 0 as an accepted placed read of votes 0 (commit_read, the score sums,
//                      the bin), the wave piles its bases (pile_bases), and lane 0 writes the pair's kind and insert.  A read too long for
//                      the slice is scored from global memory.  Rescued reads are few: plain global atomics.
// The aligning forms (include/mitofilter.h, "pairs with a band") are instantiations of the same two kernels:
//   pair_list_kernel<true>   reads the sets' alignments where the plain one reads their scores: settled is align_accepts.
//   rescue_kernel<true, ..>  staging, scan, fold and butterfly are the plain kernel's -- the seed is ungapped.  The winner is then aligned
//                      by the whole wave inside the band around the candidate's start (align_read, mf_align_dev.h) in the wave's own
//                      slice of work memory; lane 0 writes the alignment, commits the read with the alignment's footprint and its edits
//                      as the bin, and adds the five align sums; the wave adds what an accepted aligned read adds (align_adds<GAPPED,
//                      EXTEND>, the instantiations launch_align picks).
#include "mf_pairs.h"
#include "mf_align_dev.h"
#include <algorithm>
#include <type_traits>

namespace mf {

constexpr int PAIR_BLOCK = 256;
constexpr uint32_t PAIR_LDS = 1024;                      // pair counters up to this gather in LDS first

__device__ __forceinline__ bool pass_bit(const uint32_t *__restrict__ bits, uint64_t i) { return (bits[i >> 5] >> ((uint32_t)i & 31u)) & 1u; }

// what a set's cut went by: its scores, or (ALIGN) its alignments
template <bool ALIGN> using CutOut = std::conditional_t<ALIGN, AlignOut, ScoreOut>;
__device__ __forceinline__ bool cut_accepts(const ScoreOut &s, uint32_t max_permille) { return score_accepts(s.compared, s.mismatches, max_permille); }
__device__ __forceinline__ bool cut_accepts(const AlignOut &a, uint32_t max_permille) { return align_accepts(a.compared, a.mismatches, a.insertions, a.deletions, max_permille); }

template <bool ALIGN>
__global__ void __launch_bounds__(PAIR_BLOCK)
pair_list_kernel(const uint32_t *__restrict__ bits1, const uint32_t *__restrict__ bits2, const PlaceOut *__restrict__ place1, const PlaceOut *__restrict__ place2,
                 const CutOut<ALIGN> *__restrict__ score1, const CutOut<ALIGN> *__restrict__ score2, uint64_t n, uint32_t max_permille, PairWindow win, uint32_t n_rec,
                 PairOut *__restrict__ pairs, uint32_t *__restrict__ list, unsigned long long *__restrict__ counters)
{
    __shared__ unsigned long long s_cnt[PAIR_LDS];
    const PairLayout P(n_rec);
    const uint32_t n_cnt = (uint32_t)P.none() + 1;
    const bool lds = n_cnt <= PAIR_LDS;
    if (lds) for (uint32_t j = threadIdx.x; j < n_cnt; j += blockDim.x) s_cnt[j] = 0;
    __syncthreads();
    auto add = [&](size_t idx, unsigned long long v) { if (lds) atomicAdd(&s_cnt[idx], v); else atomicAdd(&counters[idx], v); };
    // grid-stride, 256 pairs a turn: with one workgroup a turn, 65 k workgroups each flushed into the one counter of the pairs without a
    // settled mate, and a call on 16.7 M pairs took 3.15 ms where it now takes 2.41
    unsigned long long n_none = 0;                       // (lane 0 of every wave)
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = i0 + threadIdx.x;
        bool target = false, none_pair = false;
        if (i < n) {
            // a read that does not pass has no placement: its entry is not read (and, unless the caller asked for the array, never written)
            const PlaceOut none{PLACE_NONE, 0u, 0, 0, 0u, 0u};
            const PlaceOut a = pass_bit(bits1, i) ? place1[i] : none, b = pass_bit(bits2, i) ? place2[i] : none;
            bool set1 = a.record < PLACE_AMBIGUOUS, set2 = b.record < PLACE_AMBIGUOUS;
            if (max_permille < 1000) {                       // (at 1000 every placed read is accepted: the scores are not read)
                if (set1) { const CutOut<ALIGN> s = score1[i]; set1 = cut_accepts(s, max_permille); }
                if (set2) { const CutOut<ALIGN> s = score2[i]; set2 = cut_accepts(s, max_permille); }
            }
            PairOut out{PAIR_NONE, -1};
            if (set1 && set2) {
                if (a.record != b.record) { out.kind = PAIR_DISCORDANT; add(PAIR_RECORD_COUNTERS * (size_t)a.record + 2, 1); }
                else {
                    if (a.strand != b.strand) {
                        const int64_t ins = a.strand ? (int64_t)a.end - b.start : (int64_t)b.end - a.start;
                        if (ins > 0) out.insert = (int32_t)ins;
                    }
                    const bool proper = out.insert > 0 && (uint32_t)out.insert >= win.min_insert && (uint32_t)out.insert <= win.max_insert;
                    out.kind = proper ? PAIR_PROPER : PAIR_DISCORDANT;
                    add(PAIR_RECORD_COUNTERS * (size_t)a.record + (proper ? 0 : 1), 1);
                    if (proper) add(PAIR_RECORD_COUNTERS * (size_t)a.record + 5, (unsigned long long)out.insert);
                }
                pairs[i] = out;
            } else if (set1 || set2) {
                // the mate that is not settled: not passing or ambiguous -> a target; placed and rejected -> never rescued
                target = list && (set1 ? b.record : a.record) >= PLACE_AMBIGUOUS;
                if (!target) {
                    pairs[i] = PairOut{set1 ? PAIR_SINGLE_1 : PAIR_SINGLE_2, -1};
                    add(PAIR_RECORD_COUNTERS * (size_t)(set1 ? a.record : b.record) + 4, 1);
                }
            } else { pairs[i] = out; none_pair = true; }
        }
        // most pairs of a raw read set have no settled mate: counted by ballot, added once a wave at the end
        n_none += (unsigned long long)__popcll(__ballot(none_pair));
        const unsigned long long votes = __ballot(target);
        if (votes) {                                         // (wave-uniform)
            const int lane = threadIdx.x & 63;
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(&counters[P.listed()], (unsigned long long)__popcll(votes));
            base = wave_pick((uint64_t)base, 0);
            if (target) list[base + (uint64_t)__popcll(votes & ((1ull << lane) - 1ull))] = (uint32_t)i;
        }
    }
    if (n_none && (threadIdx.x & 63) == 0) add(P.none(), n_none);
    __syncthreads();
    if (lds) for (uint32_t j = threadIdx.x; j < n_cnt; j += blockDim.x) if (s_cnt[j]) atomicAdd(&counters[j], s_cnt[j]);
}

constexpr int RESCUE_BLOCK = 256;
constexpr uint32_t RESCUE_WORDS = 64, RESCUE_NMASK = 32;             // a wave's slice of LDS: the read's words, its invalid bases one bit each
constexpr uint64_t RESCUE_STAGE_MAX = 16 * RESCUE_WORDS - 30;        // the longest read whose words fit the slice wherever it begins in its first word
static_assert(RESCUE_STAGE_MAX <= 32 * RESCUE_NMASK, "one bit a base of a staged read");

// what one lane of a wave wrote to LDS is read by the others
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ RescueFold wave_fold(RescueFold f)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f = rescue_fold_merge(f, RescueFold{__shfl_xor(f.mismatches, o), __shfl_xor(f.d, o), __shfl_xor(f.n, o)});
    return f;
}

// What the aligning rescue takes beside the plain one (nothing otherwise, as GapArgs of mf_align.hip): the sets' alignments (optional),
// the band, the indel table, the insertion pile (GAPPED) and the extension pile with its columns an end (EXTEND), and the work memory:
// work_words words a wave, the direction bits in the first dir_words of them.
template <bool ALIGN> struct RescueAlignArgs {};
template <> struct RescueAlignArgs<true> {
    AlignOut *__restrict__ align1, *__restrict__ align2; int band;
    unsigned long long *__restrict__ indel, *__restrict__ ins_pile, *__restrict__ ext_pile; uint32_t extend;
    unsigned long long *work; uint64_t dir_words, work_words;
};

template <bool ALIGN, bool GAPPED, bool EXTEND>
__global__ void __launch_bounds__(RESCUE_BLOCK)
rescue_kernel(ReadsView R1, ReadsView R2, const uint32_t *__restrict__ bits1, const uint32_t *__restrict__ bits2, PlaceOut *__restrict__ place1,
              PlaceOut *__restrict__ place2, ScoreOut *__restrict__ score1, ScoreOut *__restrict__ score2,
              const uint32_t *__restrict__ list, PairWindow win, uint32_t k, ScoreBait bait, const uint64_t *__restrict__ rec_start, uint32_t n_rec,
              PairOut *__restrict__ pairs, unsigned long long *__restrict__ counters, unsigned long long *__restrict__ diff, unsigned long long *__restrict__ counts,
              unsigned long long *__restrict__ sums, unsigned long long *__restrict__ pile, RescueAlignArgs<ALIGN> G)
{
    __shared__ uint32_t s_words[RESCUE_BLOCK / 64][RESCUE_WORDS];
    __shared__ uint32_t s_nmask[RESCUE_BLOCK / 64][RESCUE_NMASK];
    const PairLayout P(n_rec);
    GatheredCounts cnt(nullptr, counts, 0xFFFFFFFFu);    // (more counters than LDS gathers: every add goes to global memory)
    cnt.hist_begin();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t *const words = s_words[w], *const nmask = s_nmask[w];
    const uint64_t n_list = counters[P.listed()];
    const uint64_t n_waves = (uint64_t)gridDim.x * (RESCUE_BLOCK / 64);
    const uint32_t width = win.max_insert - win.min_insert + 1;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n_list; i += n_waves) {
        const uint32_t r = list[i];
        // (a listed pair: exactly one mate is settled, the other passes and is ambiguous or does not pass and has no entry)
        const PlaceOut none{PLACE_NONE, 0u, 0, 0, 0u, 0u};
        const PlaceOut p1 = pass_bit(bits1, r) ? place1[r] : none, p2 = pass_bit(bits2, r) ? place2[r] : none;
        const bool b_is_2 = p1.record < PLACE_AMBIGUOUS;                   // mate 1 is the settled one: mate 2 is looked for
        const PlaceOut A = b_is_2 ? p1 : p2, B = b_is_2 ? p2 : p1;
        const ReadsView &R = b_is_2 ? R2 : R1;
        uint64_t b0, L;
        if (R.uniform_len) { b0 = (uint64_t)r * R.uniform_len; L = R.uniform_len; }
        else { b0 = R.offsets[r]; L = R.offsets[r + 1] - b0; }
        const bool hasn = (R.has_n[r >> 5] >> (r & 31)) & 1u;
        const uint32_t j = A.record, strand = A.strand ^ 1u;
        const uint64_t s0 = rec_start[j];
        const int64_t len = (int64_t)(rec_start[j + 1] - s0);
        const bool staged = L <= RESCUE_STAGE_MAX;
        const uint64_t r_last = R.n_words ? R.n_words - 1 : 0;
        const uint32_t nw = (uint32_t)((((uint32_t)b0 & 15u) + L + 15) >> 4);          // (staged: at most RESCUE_WORDS)
        if (staged) {
            for (uint32_t t = (uint32_t)lane; t < nw; t += 64) { const uint64_t g = (b0 >> 4) + t; words[t] = R.words[g < r_last ? g : r_last]; }
            if (hasn)
                for (uint64_t base = 0; base < L; base += 64) {
                    const uint64_t o = base + (uint64_t)lane;
                    const unsigned long long m = __ballot(o < L && read_letter(R, b0 + o, true) == READ_LETTER_NONE);
                    if (lane == 0) { nmask[base >> 5] = (uint32_t)m; nmask[(base >> 5) + 1] = (uint32_t)(m >> 32); }
                }
            wave_lds_sync();
        }
        // the candidate at `start` scored: (mismatches << 32) | compared
        auto score_at = [&](int64_t start) -> uint64_t {
            if (staged) {
                const uint64_t rb0 = b0 & 15u;
                return hasn ? rescue_score_bases(words, rb0, L, strand, start, bait, s0, len, nmask)
                            : rescue_score_chunks(words, nw ? nw - 1 : 0, rb0, L, strand, start, bait, s0, len);
            }
            if (!hasn) return rescue_score_chunks(R.words, r_last, b0, L, strand, start, bait, s0, len);
            uint64_t acc = 0;
            for (uint64_t o = 0; o < L; o++)
                if (read_letter(R, b0 + o, true) != READ_LETTER_NONE) acc += score_base(R.words, b0, L, strand, start, bait, s0, len, o);
            return acc;
        };
        RescueFold f = rescue_fold_empty();
        for (uint32_t c0 = 0; c0 < width; c0 += 64) {
            const uint32_t c = c0 + (uint32_t)lane;
            if (c >= width) continue;
            const uint32_t d = win.min_insert + c;
            const uint64_t sc = score_at(rescue_start(A.strand, A.start, A.end, L, d));
            rescue_fold_add(f, (uint32_t)sc, (uint32_t)(sc >> 32), d, k, win.rescue_permille);
        }
        f = wave_fold(f);
        const bool won = __builtin_amdgcn_readfirstlane((uint32_t)rescue_wins(f)) != 0;
        const uint32_t d = __builtin_amdgcn_readfirstlane(f.d);
        if (won) {
            const int64_t start = rescue_start(A.strand, A.start, A.end, L, d);
            const Winner W = winner_at((j << 1) | strand, (int32_t)start, rec_start);
            // ALIGN: the seed's diagonal is the band's middle; the wave's slice holds a read of either set (max_len is over both)
            AlignResult a{0, 0, 0, 0, 0, 0};
            unsigned long long *ent = nullptr;
            if constexpr (ALIGN) {
                unsigned long long *const dirs = G.work + (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * G.work_words;
                ent = dirs + G.dir_words;
                a = align_read(R, b0, hasn, L, strand, start, s0, len, bait, G.band, dirs, ent, lane);
            }
            if (lane == 0) {
                PlaceOut *const place = b_is_2 ? place2 : place1;
                if constexpr (ALIGN) {
                    AlignOut *const align = b_is_2 ? G.align2 : G.align1;
                    if (align) align[r] = AlignOut{a.compared, a.mismatches, a.insertions, a.deletions, (int32_t)a.ref_begin, (int32_t)a.ref_end};
                    commit_read(true, true, W, L, a.ref_begin, a.ref_end, true, a.mismatches + a.insertions + a.deletions, 0u, B.windows, r, n_rec, place, diff, cnt, nullptr, 0);
                    const unsigned long long v[ALIGN_SUMS] = {a.compared, a.mismatches, a.insertions, a.deletions, (a.insertions | a.deletions) != 0};
#pragma unroll
                    for (uint32_t q = 0; q < ALIGN_SUMS; q++) if (v[q]) atomicAdd(&sums[ALIGN_SUMS * (size_t)j + q], v[q]);
                } else {
                    const uint64_t sc = score_at(start);
                    const uint32_t compared = (uint32_t)sc, mismatches = (uint32_t)(sc >> 32);
                    ScoreOut *const score = b_is_2 ? score2 : score1;
                    commit_read(true, true, W, L, start, start + (int64_t)L, true, mismatches, 0u, B.windows, r, n_rec, place, diff, cnt, nullptr, 0);
                    atomicAdd(&sums[2 * (size_t)j], (unsigned long long)compared);
                    atomicAdd(&sums[2 * (size_t)j + 1], (unsigned long long)mismatches);
                    if (score) score[r] = ScoreOut{compared, mismatches};
                }
                // it is no longer among the passing reads that are not placed -- or among the reads that do not pass
                if (B.record == PLACE_AMBIGUOUS) atomicAdd(&counts[4 * (size_t)n_rec], ~0ull);
                else atomicAdd(&counters[P.rescued_not_passing()], 1ull);
                pairs[r] = PairOut{b_is_2 ? PAIR_RESCUED_2 : PAIR_RESCUED_1, (int32_t)d};
                atomicAdd(&counters[PAIR_RECORD_COUNTERS * (size_t)j + 3], 1ull);
                atomicAdd(&counters[PAIR_RECORD_COUNTERS * (size_t)j + 5], (unsigned long long)d);
            }
            if constexpr (ALIGN)
                align_adds<GAPPED, EXTEND>(R, b0, hasn, L, strand, s0, len, ent, pile, G.indel, G.ins_pile, 2u * (uint32_t)G.band, G.ext_pile, G.extend, j, lane);
            else if (pile) pile_bases(R, b0, hasn, L, W, pile, lane);
        } else if (lane == 0) {
            pairs[r] = PairOut{b_is_2 ? PAIR_SINGLE_1 : PAIR_SINGLE_2, -1};
            atomicAdd(&counters[PAIR_RECORD_COUNTERS * (size_t)j + 4], 1ull);
        }
        if (ALIGN || staged) wave_lds_sync();            // (the next pair's words overwrite these, and an aligning wave's next read its work slice)
    }
    cnt.hist_end(lane);
}

template <bool ALIGN>
static hipError_t pair_list_launch(const uint32_t *bits1, const uint32_t *bits2, const PlaceOut *place1, const PlaceOut *place2, const CutOut<ALIGN> *score1,
                                   const CutOut<ALIGN> *score2, uint64_t n, uint32_t max_permille,
                                   PairWindow win, uint32_t n_rec, PairOut *pairs, uint32_t *list, unsigned long long *counters, int n_cu, hipStream_t st)
{
    if (!n) return hipSuccess;
    // eight workgroups a CU at most, each over its share of the pairs
    const unsigned grid = std::min<unsigned>(grid_of(n, PAIR_BLOCK), (unsigned)(n_cu > 0 ? n_cu : 1) * 8u);
    hipLaunchKernelGGL(pair_list_kernel<ALIGN>, dim3(grid), dim3(PAIR_BLOCK), 0, st, bits1, bits2, place1, place2, score1, score2, n, max_permille, win, n_rec,
                       pairs, list, counters);
    return hipGetLastError();
}

hipError_t launch_pair_list(const uint32_t *bits1, const uint32_t *bits2, const PlaceOut *place1, const PlaceOut *place2, const ScoreOut *score1,
                            const ScoreOut *score2, uint64_t n, uint32_t max_permille,
                            PairWindow win, uint32_t n_rec, PairOut *pairs, uint32_t *list, unsigned long long *counters, int n_cu, hipStream_t st)
{
    return pair_list_launch<false>(bits1, bits2, place1, place2, score1, score2, n, max_permille, win, n_rec, pairs, list, counters, n_cu, st);
}

hipError_t launch_pair_list_aligned(const uint32_t *bits1, const uint32_t *bits2, const PlaceOut *place1, const PlaceOut *place2, const AlignOut *align1,
                                    const AlignOut *align2, uint64_t n, uint32_t max_permille,
                                    PairWindow win, uint32_t n_rec, PairOut *pairs, uint32_t *list, unsigned long long *counters, int n_cu, hipStream_t st)
{
    return pair_list_launch<true>(bits1, bits2, place1, place2, align1, align2, n, max_permille, win, n_rec, pairs, list, counters, n_cu, st);
}

hipError_t launch_rescue(const ReadsView &R1, const ReadsView &R2, const uint32_t *bits1, const uint32_t *bits2, PlaceOut *place1, PlaceOut *place2,
                         ScoreOut *score1, ScoreOut *score2, const uint32_t *list,
                         uint64_t n_pairs, PairWindow win, int k, const ScoreBait &bait, const uint64_t *rec_start, uint32_t n_rec, PairOut *pairs,
                         unsigned long long *counters, unsigned long long *diff, unsigned long long *counts, unsigned long long *sums,
                         unsigned long long *pile, int n_cu, hipStream_t st)
{
    if (!n_pairs) return hipSuccess;
    // the launch shape of launch_place: 32 waves a CU at most, never more waves than pairs
    const uint64_t waves = std::min<uint64_t>((uint64_t)(n_cu > 0 ? n_cu : 1) * 32, n_pairs);
    hipLaunchKernelGGL((rescue_kernel<false, false, false>), dim3(grid_of(waves, RESCUE_BLOCK / 64)), dim3(RESCUE_BLOCK), 0, st, R1, R2, bits1, bits2, place1, place2, score1, score2, list, win,
                       (uint32_t)k, bait, rec_start, n_rec, pairs, counters, diff, counts, sums, pile, RescueAlignArgs<false>{});
    return hipGetLastError();
}

static_assert(ASSIGN_BLOCK % RESCUE_BLOCK == 0, "align_waves counts whole workgroups of align_kernel: whole workgroups of this kernel too");

uint64_t rescue_align_waves(uint64_t n_pairs, uint64_t max_len, int n_cu) { return align_waves(n_pairs, max_len, n_cu); }

hipError_t launch_rescue_aligned(const ReadsView &R1, const ReadsView &R2, const uint32_t *bits1, const uint32_t *bits2, PlaceOut *place1, PlaceOut *place2,
                                 const uint32_t *list, uint64_t n_pairs, PairWindow win, int k, const ScoreBait &bait, const uint64_t *rec_start,
                                 uint32_t n_rec, PairOut *pairs, unsigned long long *counters, unsigned long long *diff, unsigned long long *counts,
                                 unsigned long long *pile, const RescueAlign &A, int n_cu, hipStream_t st)
{
    if (!n_pairs) return hipSuccess;
    // launch_align's shape and its bound on the work memory: whole workgroups, each wave with a slice of its own
    const unsigned grid = (unsigned)(rescue_align_waves(n_pairs, A.max_len, n_cu) / (RESCUE_BLOCK / 64));
    const uint64_t n = std::max<uint64_t>(A.max_len, 1);
    const RescueAlignArgs<true> G{A.align1, A.align2, (int)A.band, A.indel, A.ins_pile, A.ext_pile, A.extend, A.work, 64 * ((n + 31) / 32), align_work_words(A.max_len)};
    const auto launch = [&](auto GAPPED, auto EXTEND) {
        hipLaunchKernelGGL((rescue_kernel<true, decltype(GAPPED)::value, decltype(EXTEND)::value>), dim3(grid), dim3(RESCUE_BLOCK), 0, st, R1, R2, bits1, bits2, place1,
                           place2, (ScoreOut *)nullptr, (ScoreOut *)nullptr, list, win, (uint32_t)k, bait, rec_start, n_rec, pairs, counters, diff, counts, A.sums, pile, G);
    };
    // (the instantiations launch_align picks: an extending launch is a gapped one whatever the band; at band 0 the insertion pile has no entry)
    if (A.ext_pile && A.extend) launch(std::true_type{}, std::true_type{});
    else if (A.ins_pile && A.band) launch(std::true_type{}, std::false_type{});
    else launch(std::false_type{}, std::false_type{});
    return hipGetLastError();
}

} // namespace mf
