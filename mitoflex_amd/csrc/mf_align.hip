// Banded alignment of the placed reads (gfx950, 64-wide waves): the verifying placement with indels.
//
//   align_kernel   one wave per listed read, grid-stride.  The vote, its winner and lane 0's commit are place_kernel's (place_vote, Winner,
//                  commit_read: mf_vote_dev.h).  A placed read is aligned to its record inside the band of 2 W + 1 diagonals around
//                  the winning one (align_read, the rule of mf_align.h):
//                    rows      lane l <= 2 W owns diagonal d = l - W and holds D(i, start + i + d) of the row in one register.  Per row
//                              t[d] = min(prev[d] + sub, prev[d + 1] + 1) -- prev[d + 1] is the lane above's --, then the deletions
//                              inside the row: D[d] = min over e <= d of t[e] + (d - e), an inclusive prefix minimum over the lanes of
//                              t[e] + (63 - lane) in log2 steps that stop at the band's width (none at W == 0).  Every cell of the band
//                              is finite (D <= i), so only the two lanes at the band's edges need a predicate in place of infinity.
//                              The read's oriented letters are fetched 64 rows at a time, one a lane (an N through the npos index),
//                              and handed round by a shuffle; a lane reads the bait letter of its own column.
//                    moves     two bits a cell (align_move), 32 rows to a 64-bit word a lane, stored [row block][lane] -- 512 bytes a
//                              block, coalesced -- into the wave's slice of work memory.
//                    end       wave minimum of align_end_key over the last row.
//                    traceback wave-uniform, a row block at a time: the block's words are loaded once, a lane each, and the move of the
//                              current cell is picked out of the owning lane's register.  For read base b it leaves one word: the column
//                              the path enters row b + 1 at, whether base b was inserted, and how many bait positions row b + 1 deletes
//                              behind it -- 32 a block, stored coalesced behind the direction bits.
//                    counts    lanes take the read bases 64 at a time: compared and mismatches of the diagonal steps, one reduction.
//                  Lane 0 then commits the read with the alignment's footprint and its edits as the bin value, and keeps the five
//                  sums of a run of accepted reads on one record; for an accepted read the wave walks the base words once more
//                  (align_adds): the pile-up of the diagonal steps, the deleted positions, the insertion runs.  The GAPPED
//                  instantiations (the gapped consensus, include/mitofilter.h) also add the letter of every inserted base into the
//                  insertion pile, at its offset inside its run (align_run_offset, mf_align.h); the plain ones take an empty
//                  argument more and are otherwise the code they were.  The EXTEND instantiations (extended records, include/
//                  mitofilter.h; they are GAPPED ones, with a span of 0 at band 0) add the base of a diagonal step that lies outside
//                  the record into the extension pile of that end of the record instead of nowhere.
// Work memory: align_work_words(max_len) words a wave, as many waves as the launch has: bounded whatever the number of reads.
#include "mf_align_dev.h"          // align_read, align_adds: shared with the aligning rescue of mf_pairs.hip
#include <algorithm>

namespace mf {

constexpr uint64_t ALIGN_WORK_BYTES = 256ull << 20;
constexpr uint64_t ALIGN_WAVES_PER_BLOCK = ASSIGN_BLOCK / 64;

struct AlignArgs {
    ScoreBait bait; uint32_t max_permille; int band;
    AlignOut *__restrict__ align; unsigned long long *__restrict__ sums, *__restrict__ indel;
    uint32_t *__restrict__ keep_bits; int keep;
    unsigned long long *work; uint64_t max_len, dir_words, work_words;
};

// What the gapped launch takes beside the plain one (nothing otherwise: the plain instantiations take no argument they would read).
// The extending launch is a gapped one that takes the extension pile and its columns an end as well.
template <bool GAPPED, bool EXTEND = false> struct GapArgs {};
template <> struct GapArgs<true, false> { unsigned long long *__restrict__ ins_pile; };
template <> struct GapArgs<true, true> { unsigned long long *__restrict__ ins_pile, *__restrict__ ext_pile; uint32_t extend; };

template <int KW, bool GAPPED, bool EXTEND>
__global__ void __launch_bounds__(ASSIGN_BLOCK)
align_kernel(ReadsView R, KmerSetView S, const Anchor *__restrict__ anchor, const uint64_t *__restrict__ rec_start, const uint32_t *__restrict__ list,
             const unsigned long long *__restrict__ n_list_p, uint32_t n_rec, PlaceOut *__restrict__ place, unsigned long long *__restrict__ diff,
             unsigned long long *__restrict__ counts, unsigned long long *__restrict__ pile, AlignArgs A, GapArgs<GAPPED, EXTEND> G)
{
    __shared__ uint32_t s_hist[HIST_MAX];
    // forward, reverse, over_begin, over_end of every record; not placed; behind them rejected and the 32 bins of every record
    GatheredCounts cnt(s_hist, counts, 4 * n_rec + 1 + SCORE_GATHERED * n_rec);
    cnt.hist_begin();
    NucWindows<KW> src(R, S, nullptr);
    const int lane = threadIdx.x & 63;
    const uint64_t n_list = *n_list_p;
    const uint64_t n_waves = (uint64_t)gridDim.x * (ASSIGN_BLOCK / 64);
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    unsigned long long *const dirs = A.work + wave * A.work_words, *const ent = dirs + A.dir_words;
    uint32_t sum_j = 0; bool sum_any = false;                // (lane 0) the sums of a run of accepted reads on one record
    unsigned long long sum_v[ALIGN_SUMS] = {0, 0, 0, 0, 0};
    auto flush = [&]() {
#pragma unroll
        for (uint32_t q = 0; q < ALIGN_SUMS; q++) { if (sum_v[q]) atomicAdd(&A.sums[ALIGN_SUMS * sum_j + q], sum_v[q]); sum_v[q] = 0; }
        sum_any = false;
    };
    for (uint64_t i = wave; i < n_list; i += n_waves) {
        const uint32_t r = list[i];
        const uint64_t np = src.begin(r);                    // windows; the read has np + k - 1 bases when np > 0
        uint32_t best_cnt, windows; uint64_t best_key; bool tie;
        place_vote<KW>(R, S, anchor, src, np, lane, best_cnt, best_key, tie, windows);
        const uint64_t L = np + (uint64_t)S.k - 1;
        const bool placed = best_cnt && !tie && L <= A.max_len;          // (no listed read is longer than max_len: the work memory's bound)
        AlignResult a{0, 0, 0, 0, 0, 0};
        bool accept = true;
        Winner W{};
        if (placed) {
            W = winner_of(best_key, rec_start);
            a = align_read(R, src.b0, src.hasn, L, W.strand(), W.start, W.s0, W.len, A.bait, A.band, dirs, ent, lane);
            accept = align_accepts(a.compared, a.mismatches, a.insertions, a.deletions, A.max_permille);
        }
        if (lane == 0) {
            // (the alignment is written before the commit: in this order the kernel has the registers it had with its own block)
            if (placed && A.align) A.align[r] = AlignOut{a.compared, a.mismatches, a.insertions, a.deletions, (int32_t)a.ref_begin, (int32_t)a.ref_end};
            commit_read(placed, accept, W, L, a.ref_begin, a.ref_end, true, a.mismatches + a.insertions + a.deletions, best_cnt, windows, r, n_rec, place, diff, cnt,
                        A.keep_bits, A.keep);
            if (placed && accept) {
                if (sum_any && sum_j != W.record()) flush();
                sum_j = W.record(); sum_any = true;
                sum_v[0] += a.compared; sum_v[1] += a.mismatches; sum_v[2] += a.insertions; sum_v[3] += a.deletions;
                sum_v[4] += (a.insertions | a.deletions) != 0;
            }
        }
        if (placed && accept) {
            unsigned long long *ins_pile = nullptr, *ext_pile = nullptr; uint32_t extend = 0;
            if constexpr (GAPPED) ins_pile = G.ins_pile;
            if constexpr (EXTEND) { ext_pile = G.ext_pile; extend = G.extend; }
            align_adds<GAPPED, EXTEND>(R, src.b0, src.hasn, L, W.strand(), W.s0, W.len, ent, pile, A.indel, ins_pile, 2u * (uint32_t)A.band, ext_pile, extend,
                                       W.record(), lane);
        }
    }
    if (lane == 0 && sum_any) flush();
    cnt.hist_end(lane);
}

uint64_t align_work_words(uint64_t max_len)
{
    const uint64_t n = std::max<uint64_t>(max_len, 1);
    return 64 * ((n + 31) / 32) + n;
}

uint64_t align_waves(uint64_t n_reads, uint64_t max_len, int n_cu)
{
    uint64_t waves = std::min<uint64_t>((uint64_t)(n_cu > 0 ? n_cu : 1) * 32, std::max<uint64_t>(n_reads, 1));
    waves = std::min(waves, ALIGN_WORK_BYTES / (align_work_words(max_len) * 8));
    return std::max<uint64_t>((waves + ALIGN_WAVES_PER_BLOCK - 1) / ALIGN_WAVES_PER_BLOCK, 1) * ALIGN_WAVES_PER_BLOCK;
}

hipError_t launch_align(const ReadsView &R, const KmerSetView &S, const Anchor *anchor, const uint64_t *rec_start, const uint32_t *list,
                        const unsigned long long *n_list, uint32_t n_rec, PlaceOut *place, unsigned long long *diff, unsigned long long *counts,
                        unsigned long long *pile, const PlaceAlign &P, int n_cu, hipStream_t st)
{
    if (!R.n_reads) return hipSuccess;
    const unsigned grid = (unsigned)(align_waves(R.n_reads, P.max_len, n_cu) / ALIGN_WAVES_PER_BLOCK);
    const uint64_t n = std::max<uint64_t>(P.max_len, 1);
    const AlignArgs A{P.cut.bait, P.cut.max_permille, (int)P.band, P.align, P.cut.sums, P.indel, P.cut.keep_bits, P.cut.keep, P.work, P.max_len, 64 * ((n + 31) / 32),
                      align_work_words(P.max_len)};
    const auto launch = [&](auto KW, auto GAPPED, auto EXTEND) {
        GapArgs<decltype(GAPPED)::value, decltype(EXTEND)::value> G;
        if constexpr (decltype(GAPPED)::value) G.ins_pile = P.ins_pile;
        if constexpr (decltype(EXTEND)::value) { G.ext_pile = P.ext_pile; G.extend = P.extend; }
        hipLaunchKernelGGL((align_kernel<decltype(KW)::value, decltype(GAPPED)::value, decltype(EXTEND)::value>), dim3(grid), dim3(ASSIGN_BLOCK), 0, st, R, S, anchor,
                           rec_start, list, n_list, n_rec, place, diff, counts, pile, A, G);
    };
    // (an extending launch is a gapped one whatever the band: at band 0 the span is 0 and the insertion pile, which has no entry, is not touched)
    if (P.ext_pile && P.extend) {
        if (S.kw == 1) launch(std::integral_constant<int, 1>{}, std::true_type{}, std::true_type{});
        else launch(std::integral_constant<int, 2>{}, std::true_type{}, std::true_type{});
    } else dispatch_kw_flag(S.kw, P.ins_pile && P.band, [&](auto KW, auto GAPPED) { launch(KW, GAPPED, std::false_type{}); });          // (band 0: the insertion pile has no entry)
    return hipGetLastError();
}

} // namespace mf
