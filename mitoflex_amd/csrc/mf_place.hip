// Placement of baited reads on the bait (gfx950, 64-wide waves): position, strand and base depth; the pile-up of their bases.
// What place_kernel shares with align_kernel (mf_align.hip) is stated once in mf_vote_dev.h -- the vote, the winner, a read's letter,
// lane 0's commit --, the call rules once in mf_call.h.
//
//   anchor_span_kernel     one thread per bait window: atomicMin / atomicMax of its position into two slot-indexed arrays;
//   anchor_finish_kernel   one thread per slot keeps the key as an anchor where both agree (exactly one window holds it, whatever order the
//                          windows came in) and that window is not its own reverse complement: its position inside its record, its
//                          record (record_of) and the bait's orientation go into one 8-byte entry.
//   place_kernel           one wave per listed read, grid-stride.  place_vote: every window whose key is an anchor votes for (record,
//                          strand, start); a strict winner places the read (Winner: decoded wave-uniform once for score_read and once
//                          more for pile_bases, and by lane 0 for its own block).  With VERIFY the wave then scores the winner against the bait (score_read, mf_score.h): lanes take the clipped footprint
//                          sixteen bases at a time -- the read's word funnel-shifted (mirrored and complemented on strand 1) against the
//                          bait's, masked by length, clip and the bait's validity bits --, a read with an N base by base (read_letter);
//                          one wave reduction, then the cut.  Lane 0 commits the read (commit_read): its placement, +1 / -1 into the
//                          difference counters at the clipped ends of its footprint, its record's counters through the per-wave run and
//                          the workgroup's LDS histogram; a rejected read keeps its placement and its score and bumps only `rejected`
//                          and its bin.  Given a keep bitmap (KEEP) the read's bit there is cleared where the keep rule says so; those
//                          instantiations keep a commit block of their own, which holds their registers.  Lane 0 also keeps the
//                          packed sums of a run of accepted reads on one record (VERIFY, run_add).  With PILE the wave last walks an
//                          accepted read's bases 64 at a time (pile_bases): read_letter, complement on strand 1, clip to the record, one
//                          64-bit add into [position][letter].
//   place_scan_reduce_kernel, place_scan_partials_kernel, place_profile_kernel
//                          base depth = inclusive scan of the difference counters (a -1 that lands on the next record's first position
//                          is right under a global scan: no segmentation): tile sums, their exclusive scan (launch_tile_partials), then
//                          per tile the scan (tile_scan_begin), the clamp and the records' covered / base_sum through RecordWalk
//                          (reduced over the wave where a wave lies inside one record).
//   pileup_call_kernel     per position, tiled like place_profile_kernel: the four counters clamped, pileup_call_position (mf_call.h) for
//                          the consensus byte and what the records' six sums add, through the same record walk.
//   gapped_call_kernel     per position, tiled the same way and behind the same scan: the gapped consensus of an aligning placement --
//                          the insertion pile clamped, gapped_call_position (mf_call.h) for the bytes the position emits and how many,
//                          the records' four sums.
#include "mf_place.h"
#include "mf_vote_dev.h"
#include <algorithm>

namespace mf {

template <int KW>
__global__ void __launch_bounds__(256)
anchor_span_kernel(BaitView B, KmerSetView S, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B.total || B.runlen[p] < (uint32_t)S.k) return;          // (runlen: valid bases from p inside its record, capped at 255 >= k)
    const uint64_t slot = table_find(S, canonical_at<KW>(B.words, p, S.k));
    if (slot == ~0ULL) return;                                          // (cannot happen: every valid window's key is in the set)
    atomicMin(&lo[slot], (uint32_t)p);
    atomicMax(&hi[slot], (uint32_t)p);
}

template <int KW>
__global__ void __launch_bounds__(256)
anchor_finish_kernel(BaitView B, const uint64_t *__restrict__ rec_start, uint32_t n_rec, int k, const uint32_t *__restrict__ lo,
                     const uint32_t *__restrict__ hi, Anchor *__restrict__ anchor, uint64_t slots)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    Anchor out{ANCHOR_NONE, 0u};
    const uint32_t p = lo[s];
    if (p != ANCHOR_NONE && p == hi[s]) {                               // (an empty slot: lo all ones, hi 0)
        uint32_t rev;
        (void)oriented_at<KW>(B.words, p, k, rev);
        if (rev != 2u) {
            const uint32_t a = record_of(rec_start, n_rec, p);
            out = Anchor{p - (uint32_t)rec_start[a], (a << 1) | rev};
        }
    }
    anchor[s] = out;
}

__global__ void __launch_bounds__(256) place_init_kernel(PlaceOut *__restrict__ place, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) place[i] = PlaceOut{PLACE_NONE, 0u, 0, 0, 0u, 0u};
}

__global__ void __launch_bounds__(256) max_read_len_kernel(const uint64_t *__restrict__ offsets, uint64_t n, unsigned long long *__restrict__ max_len)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long len = i < n ? offsets[i + 1] - offsets[i] : 0;
    len = wave_max_u64(len);
    if ((threadIdx.x & 63) == 0 && len) atomicMax(max_len, len);
}

// What a verifying launch is given beside a placing one (nothing otherwise: the plain instantiations take no argument more than before).
// KEEP: a verifying launch that is also given a keep bitmap; the verifying launches without one keep their code and their registers.
template <bool VERIFY, bool KEEP> struct VerifyArgs { static constexpr bool verify = false, keep_rule = false; };
template <> struct VerifyArgs<true, false> {
    static constexpr bool verify = true, keep_rule = false;
    ScoreBait bait; uint32_t max_permille;
    ScoreOut *__restrict__ score;                  // optional, n_reads entries, zeroed
    unsigned long long *__restrict__ sums;         // compared, mismatches of every record's accepted reads
};
template <> struct VerifyArgs<true, true> : VerifyArgs<true, false> {
    static constexpr bool keep_rule = true;
    uint32_t *__restrict__ keep_bits; int keep;    // the pass bitmap's copy that loses the bits keep_clears names (mf_score.h)
};

// The score of the placed read (mf_score.h): lanes take the clipped footprint sixteen bases at a time, a read with an invalid base goes
// base by base; one wave reduction of the packed pair.  Every lane returns the read's (mismatches << 32) | compared.
__device__ __forceinline__ unsigned long long score_read(const ReadsView &R, uint64_t b0, bool hasn, uint64_t L, const Winner &W, const ScoreBait &B, int lane)
{
    unsigned long long acc = 0;
    if (!hasn) {
        int64_t lo, hi;
        score_footprint(L, W.start, W.len, lo, hi);
        const uint64_t chunks = (uint64_t)(hi - lo + 15) >> 4;
        const uint64_t r_last = R.n_words ? R.n_words - 1 : 0;
        for (uint64_t t = (uint64_t)lane; t < chunks; t += 64) acc += score_chunk16(R.words, r_last, b0, L, W.strand(), W.start, B, W.s0, lo, hi, t);
    } else {
        for (uint64_t i = (uint64_t)lane; i < L; i += 64) {
            if (read_letter(R, b0 + i, true) == READ_LETTER_NONE) continue;                                             // an N is not compared
            acc += score_base(R.words, b0, L, W.strand(), W.start, B, W.s0, W.len, i);
        }
    }
    return wave_sum_u64(acc);
}

template <int KW, bool PILE, bool VERIFY, bool KEEP>
__global__ void __launch_bounds__(ASSIGN_BLOCK)
place_kernel(ReadsView R, KmerSetView S, const Anchor *__restrict__ anchor, const uint64_t *__restrict__ rec_start, const uint32_t *__restrict__ list,
             const unsigned long long *__restrict__ n_list_p, uint32_t n_rec, PlaceOut *__restrict__ place, unsigned long long *__restrict__ diff,
             unsigned long long *__restrict__ counts, unsigned long long *__restrict__ pile, VerifyArgs<VERIFY, KEEP> V)
{
    __shared__ uint32_t s_hist[HIST_MAX];
    // forward, reverse, over_begin, over_end of every record; not placed; with VERIFY behind them rejected and the 32 bins of every record
    GatheredCounts cnt(s_hist, counts, 4 * n_rec + 1 + (VERIFY ? SCORE_GATHERED * n_rec : 0u));
    cnt.hist_begin();
    NucWindows<KW> src(R, S, nullptr);
    const int lane = threadIdx.x & 63;
    const uint64_t n_list = *n_list_p;
    const uint64_t n_waves = (uint64_t)gridDim.x * (ASSIGN_BLOCK / 64);
    uint32_t sum_j = 0; unsigned long long sum_v = 0;        // (lane 0, VERIFY) the packed sums of a run of accepted reads on one record
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n_list; i += n_waves) {
        const uint32_t r = list[i];
        const uint64_t np = src.begin(r);                    // windows; the read has np + k - 1 bases when np > 0
        uint32_t best_cnt, windows; uint64_t best_key; bool tie;
        place_vote<KW>(R, S, anchor, src, np, lane, best_cnt, best_key, tie, windows);
        const uint64_t L = np + S.k - 1;
        const bool placed = best_cnt && !tie;
        // VERIFY: the read is scored before anything of it is counted; a rejected read then counts nowhere but in rejected and its bin
        uint32_t compared = 0, mismatches = 0; bool accept = true;
        if constexpr (VERIFY) {
            if (placed) {
                const unsigned long long sc = score_read(R, src.b0, src.hasn, L, winner_of(best_key, rec_start), V.bait, lane);
                compared = __builtin_amdgcn_readfirstlane((uint32_t)sc); mismatches = __builtin_amdgcn_readfirstlane((uint32_t)(sc >> 32));
                accept = score_accepts(compared, mismatches, V.max_permille);
            }
        }
        // (lane 0, VERIFY) an accepted read on record j into the run of packed sums
        auto run_add = [&](uint32_t j) {
            if constexpr (VERIFY) {
                if (sum_v && sum_j != j) { atomicAdd(&V.sums[2 * sum_j], sum_v & 0xFFFFFFFFull); atomicAdd(&V.sums[2 * sum_j + 1], sum_v >> 32); sum_v = 0; }
                // (a run's packed halves stay below 2^32: flushed before either could carry)
                if ((sum_v & 0xFFFFFFFFull) + compared > 0xFFFFFFFFull || (sum_v >> 32) + mismatches > 0xFFFFFFFFull) {
                    atomicAdd(&V.sums[2 * sum_j], sum_v & 0xFFFFFFFFull); atomicAdd(&V.sums[2 * sum_j + 1], sum_v >> 32); sum_v = 0;
                }
                sum_j = j; sum_v += ((unsigned long long)mismatches << 32) | compared;
            }
        };
        if (lane == 0) {
            // lane 0 decodes the winner for itself, as it always did: behind one wave-uniform decode in front of this block a pass over
            // reads stacked on one start took 0.5 % longer; align_kernel shares its one decode
            Winner W{};
            if (placed) W = winner_at((uint32_t)(best_key >> 32), (int32_t)(uint32_t)best_key, rec_start);
            if constexpr (KEEP) {
                // the keep-rule instantiations keep their own block: through commit_read the one without the pile lost a register, went from
                // five to six waves a SIMD and took 1.3 to 4.9 % longer
                PlaceOut out{PLACE_AMBIGUOUS, 0u, 0, 0, 0u, windows};
                if (placed) {
                    const uint32_t j = W.record();
                    const int64_t start = W.start, end = start + (int64_t)L;
                    out = PlaceOut{j, W.strand(), (int32_t)start, (int32_t)end, best_cnt, windows};
                    if (accept) {
                        // the winning anchor's window lies inside the record and inside the read: 0 <= begin < last <= len
                        atomicAdd(&diff[W.s0 + (uint64_t)(start > 0 ? start : 0)], 1ull);
                        atomicAdd(&diff[W.s0 + (uint64_t)(end < W.len ? end : W.len)], ~0ull);
                        cnt.bump(4 * j + W.strand());
                        if (start < 0) cnt.add(4 * j + 2, 1);
                        if (end > W.len) cnt.add(4 * j + 3, 1);
                    }
                    const uint32_t g0 = 4 * n_rec + 1 + SCORE_GATHERED * j;
                    if (!accept) cnt.add(g0, 1);
                    cnt.add(g0 + 1 + (mismatches < SCORE_BINS - 1 ? mismatches : SCORE_BINS - 1), 1);
                    if (accept) run_add(j);
                    if (V.score) V.score[r] = ScoreOut{compared, mismatches};
                } else cnt.bump(4 * n_rec);
                if (place) place[r] = out;
                // the keep rule: the words of the bitmap are shared by the waves of 32 reads, hence the atomic; nothing else is written for it
                if (keep_clears(placed, accept, V.keep)) atomicAnd(&V.keep_bits[r >> 5], ~(1u << (r & 31u)));
            } else {
                commit_read(placed, accept, W, L, W.start, W.start + (int64_t)L, VERIFY, mismatches, best_cnt, windows, r, n_rec, place, diff, cnt, nullptr, 0);
                if constexpr (VERIFY) {
                    if (placed && accept) run_add(W.record());
                    if (placed && V.score) V.score[r] = ScoreOut{compared, mismatches};
                }
            }
        }
        if (PILE && placed && accept) pile_bases(R, src.b0, src.hasn, L, winner_of(best_key, rec_start), pile, lane);
    }
    if constexpr (VERIFY)
        if (lane == 0 && sum_v) { atomicAdd(&V.sums[2 * sum_j], sum_v & 0xFFFFFFFFull); atomicAdd(&V.sums[2 * sum_j + 1], sum_v >> 32); }
    cnt.hist_end(lane);
}

// ------------------------------------------------------------------------------------------------------------------ base depth
constexpr uint32_t PS_BLOCK = 256, PS_ITEMS = 16, PS_TILE = PS_BLOCK * PS_ITEMS;

// exclusive prefix of v over the workgroup in thread order; *total = the workgroup's sum
__device__ __forceinline__ unsigned long long block_exclusive_u64(unsigned long long v, unsigned long long *lds, unsigned long long *total)
{
    unsigned long long inc = v;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long t = __shfl_up(inc, d); if (lane >= (uint32_t)d) inc += t; }
    __syncthreads();
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    unsigned long long base = 0, sum = 0;
    for (uint32_t i = 0; i < nw; i++) { if (i < w) base += lds[i]; sum += lds[i]; }
    if (total) *total = sum;
    return base + inc - v;
}

__global__ void __launch_bounds__(PS_BLOCK)
place_scan_reduce_kernel(const unsigned long long *__restrict__ diff, uint64_t n, unsigned long long *__restrict__ partial)
{
    __shared__ unsigned long long lds[PS_BLOCK / 64];
    const uint64_t t0 = (uint64_t)blockIdx.x * PS_TILE;
    unsigned long long s = 0;
    for (uint32_t k = 0; k < PS_ITEMS; k++) { const uint64_t i = t0 + (uint64_t)k * PS_BLOCK + threadIdx.x; if (i < n) s += diff[i]; }
    unsigned long long tot;
    (void)block_exclusive_u64(s, lds, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(PS_BLOCK)
place_scan_partials_kernel(unsigned long long *__restrict__ partial, uint64_t nb)        // in place, exclusive
{
    __shared__ unsigned long long lds[PS_BLOCK / 64];
    unsigned long long carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += PS_BLOCK) {
        const uint64_t i = b0 + threadIdx.x;
        const unsigned long long v = i < nb ? partial[i] : 0;
        unsigned long long tot;
        const unsigned long long ex = block_exclusive_u64(v, lds, &tot);
        if (i < nb) partial[i] = carry + ex;
        carry += tot;
        __syncthreads();
    }
}

// The record of a thread's run of ascending positions, and the sums it keeps for that record: begin() finds the record of the first
// position, next(p) flushes the sums and moves on when p lies behind the record, finish() adds what is left -- one add a wave where all
// its lanes are in the same record (same-address atomics serialise).  rec_sums: N counters a record.
template <int N>
struct RecordWalk {
    const uint64_t *__restrict__ rec_start; unsigned long long *__restrict__ rec_sums;
    uint32_t j = ~0u; uint64_t j_end = 0;
    unsigned long long v[N];
    __device__ __forceinline__ RecordWalk(const uint64_t *rec_start_, unsigned long long *rec_sums_) : rec_start(rec_start_), rec_sums(rec_sums_)
    {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = 0;
    }
    __device__ __forceinline__ void begin(uint32_t n_rec, uint64_t i0) { j = record_of(rec_start, n_rec, i0); j_end = rec_start[j + 1]; }
    __device__ __forceinline__ void flush()
    {
#pragma unroll
        for (int k = 0; k < N; k++) { if (v[k]) atomicAdd(&rec_sums[N * (uint64_t)j + k], v[k]); v[k] = 0; }
    }
    __device__ __forceinline__ void next(uint64_t p)
    {
        if (p < j_end) return;
        flush();
        do { j++; j_end = rec_start[j + 1]; } while (p >= j_end);
    }
    __device__ __forceinline__ void finish()
    {
        const uint32_t j0 = __builtin_amdgcn_readfirstlane(j);
        if (__ballot(j != j0) == 0) {
#pragma unroll
            for (int k = 0; k < N; k++) v[k] = wave_sum_u64(v[k]);
            if ((threadIdx.x & 63) == 0 && j != ~0u) flush();
        } else flush();
    }
};

// The scan of the difference counters inside a tile: v = the thread's PS_ITEMS counters from position i0 on (0 behind n); returns the sum
// of every counter before i0 -- the tile's partial and the workgroup's exclusive prefix.  The whole workgroup calls it.
__device__ __forceinline__ unsigned long long tile_scan_begin(const unsigned long long *__restrict__ diff, uint64_t n, const unsigned long long *__restrict__ partial,
                                                              uint64_t i0, unsigned long long *lds, unsigned long long (&v)[PS_ITEMS])
{
    unsigned long long s = 0;
#pragma unroll
    for (uint32_t k = 0; k < PS_ITEMS; k++) { v[k] = i0 + k < n ? diff[i0 + k] : 0; s += v[k]; }
    return partial[blockIdx.x] + block_exclusive_u64(s, lds, nullptr);
}

// the four counters of a position as they are reported
__device__ __forceinline__ PileOut pile_clamped(unsigned long long c0, unsigned long long c1, unsigned long long c2, unsigned long long c3)
{
    return PileOut{clamp_count(c0), clamp_count(c1), clamp_count(c2), clamp_count(c3)};
}

__global__ void __launch_bounds__(PS_BLOCK)
place_profile_kernel(const unsigned long long *__restrict__ diff, uint64_t n, const unsigned long long *__restrict__ partial,
                     const uint64_t *__restrict__ rec_start, uint32_t n_rec, uint32_t *__restrict__ depth, unsigned long long *__restrict__ rec_sums)
{
    __shared__ unsigned long long lds[PS_BLOCK / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * PS_TILE + (uint64_t)threadIdx.x * PS_ITEMS;
    unsigned long long v[PS_ITEMS];
    unsigned long long run = tile_scan_begin(diff, n, partial, i0, lds, v);
    // the thread's positions lie in one record and the records behind it: covered and base_sum per record, added when the record changes
    RecordWalk<2> walk(rec_start, rec_sums);
    if (rec_sums && i0 < n) walk.begin(n_rec, i0);
#pragma unroll
    for (uint32_t k = 0; k < PS_ITEMS; k++) {
        const uint64_t p = i0 + k;
        run += v[k];
        if (p >= n) continue;
        if (depth) depth[p] = clamp_count(run);
        if (!rec_sums) continue;
        walk.next(p);
        walk.v[0] += run != 0; walk.v[1] += run;
    }
    if (rec_sums) walk.finish();
}

// The pile-up called.  A thread takes PS_ITEMS positions in a row -- one word of the bait --, a workgroup PS_TILE.
__global__ void __launch_bounds__(PS_BLOCK)
pileup_call_kernel(const unsigned long long *__restrict__ pile, BaitView B, const uint64_t *__restrict__ rec_start, uint32_t n_rec, uint32_t min_depth,
                   PileOut *__restrict__ out, uint8_t *__restrict__ consensus, unsigned long long *__restrict__ rec_sums)
{
    static_assert(PS_ITEMS == 16, "a thread's positions are one packed word");
    const uint64_t n = B.total;
    const uint64_t i0 = (uint64_t)blockIdx.x * PS_TILE + (uint64_t)threadIdx.x * PS_ITEMS;
    RecordWalk<(int)PILE_SUMS> walk(rec_start, rec_sums);          // bases, matches, mismatches, called, ambiguous, variants
    if (rec_sums && i0 < n) walk.begin(n_rec, i0);
    const uint32_t word = i0 < n ? B.words[i0 >> 4] : 0u;
#pragma unroll 4
    for (uint32_t k = 0; k < PS_ITEMS; k++) {
        const uint64_t p = i0 + k;
        if (p >= n) break;
        const ulonglong2 lo = reinterpret_cast<const ulonglong2 *>(pile)[2 * p], hi = reinterpret_cast<const ulonglong2 *>(pile)[2 * p + 1];
        const bool valid = B.runlen[p] != 0;
        const PileCall c = pileup_call_position(lo.x, lo.y, hi.x, hi.y, (word >> (2 * k)) & 3u, valid, min_depth);          // (mf_call.h)
        if (out) out[p] = pile_clamped(lo.x, lo.y, hi.x, hi.y);
        if (consensus) consensus[p] = c.consensus;
        if (!rec_sums) continue;
        walk.next(p);
        walk.v[0] += c.depth;
        if (valid) { walk.v[1] += c.own; walk.v[2] += c.depth - c.own; }
        walk.v[3] += c.called;
        walk.v[4] += c.ambiguous;
        walk.v[5] += c.variant;
    }
    if (rec_sums) walk.finish();
}

// The gapped consensus called (include/mitofilter.h, "gapped consensus"), tiled like place_profile_kernel, whose scan of the difference
// counters it shares (tile_scan_begin): the call goes by the UNCLAMPED base depth D, position by position (gapped_call_position,
// mf_call.h, which the CPU model check compiles too).  Per position: the clamped counters into ins_out (optional), the
// number of emitted bytes into count[p] (0 .. 1 + span) and the bytes into bytes[p * (1 + span) ..]; per record (rec_sums, optional,
// zeroed): length, deleted, insertions, inserted_bases.
__global__ void __launch_bounds__(PS_BLOCK)
gapped_call_kernel(const unsigned long long *__restrict__ diff, uint64_t n, const unsigned long long *__restrict__ partial,
                   const unsigned long long *__restrict__ indel, const unsigned long long *__restrict__ ins_pile, uint32_t span,
                   const uint8_t *__restrict__ consensus, const uint64_t *__restrict__ rec_start, uint32_t n_rec, uint32_t min_depth,
                   PileOut *__restrict__ ins_out, uint8_t *__restrict__ count, uint8_t *__restrict__ bytes, unsigned long long *__restrict__ rec_sums)
{
    __shared__ unsigned long long lds[PS_BLOCK / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * PS_TILE + (uint64_t)threadIdx.x * PS_ITEMS;
    unsigned long long v[PS_ITEMS];
    unsigned long long run = tile_scan_begin(diff, n, partial, i0, lds, v);
    RecordWalk<(int)GAPPED_SUMS> walk(rec_start, rec_sums);          // length, deleted, insertions, inserted_bases
    if (rec_sums && i0 < n) walk.begin(n_rec, i0);
    for (uint32_t k = 0; k < PS_ITEMS; k++) {
        const uint64_t p = i0 + k;
        run += v[k];
        if (p >= n) break;
        const unsigned long long *const ins = span ? ins_pile + 4 * p * (uint64_t)span : nullptr;
        if (ins_out)
            for (uint32_t q = 0; q < span; q++) ins_out[p * (uint64_t)span + q] = pile_clamped(ins[4 * q], ins[4 * q + 1], ins[4 * q + 2], ins[4 * q + 3]);
        bool deleted;
        const uint32_t m = gapped_call_position(run, span ? indel[ALIGN_POSITION_COUNTERS * p] : 0ull, ins, span, min_depth, consensus[p],
                                                bytes + p * (uint64_t)(1 + span), deleted);
        count[p] = (uint8_t)m;
        if (!rec_sums) continue;
        walk.next(p);
        const uint32_t inserted = m - (deleted ? 0u : 1u);
        walk.v[0] += m; walk.v[1] += deleted; walk.v[2] += inserted != 0; walk.v[3] += inserted;
    }
    if (rec_sums) walk.finish();
}

// The ends of the records called (include/mitofilter.h, "extended records"): one wave per (record, side), n_ends = 2 R of them, each over
// its E columns of ext_pile, lanes taking the offsets lane, lane + 64, ..  Every column: the clamped counters into ext_out (optional) and
// extend_call_column (mf_call.h) from the unclamped ones; a ballot finds the first column that is not emitted, the bytes of the columns
// before it go to bytes[end * E ..] in the order of the offsets.  sums[EXTEND_END_SUMS * end]: the emitted columns, then the unclamped
// sum of all counts of the end's table.
__global__ void __launch_bounds__(PS_BLOCK)
extend_call_kernel(const unsigned long long *__restrict__ ext_pile, uint32_t E, uint32_t n_ends, uint32_t min_depth, PileOut *__restrict__ ext_out,
                   uint8_t *__restrict__ bytes, unsigned long long *__restrict__ sums)
{
    const uint32_t end = (blockIdx.x * PS_BLOCK + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (end >= n_ends) return;                                      // (wave-uniform)
    const unsigned long long *const t = ext_pile + 4 * (uint64_t)end * E;
    unsigned long long piled = 0;
    uint32_t emitted = E;                                           // the first column that is not emitted
    bool open = true;
    for (uint32_t base = 0; base < E; base += 64) {
        const uint32_t e = base + lane;
        const bool in = e < E;
        unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        if (in) { c0 = t[4 * (uint64_t)e]; c1 = t[4 * (uint64_t)e + 1]; c2 = t[4 * (uint64_t)e + 2]; c3 = t[4 * (uint64_t)e + 3]; }
        piled += c0 + c1 + c2 + c3;
        if (in && ext_out) ext_out[(uint64_t)end * E + e] = pile_clamped(c0, c1, c2, c3);
        if (!open) continue;
        uint8_t byte;
        const bool emit = extend_call_column(c0, c1, c2, c3, min_depth, byte) && in;
        const unsigned long long stop = __ballot(!emit);
        const uint32_t first = stop ? (uint32_t)__ffsll((long long)stop) - 1u : 64u;
        if (lane < first) bytes[(uint64_t)end * E + e] = byte;      // (emit holds for these lanes: e < E)
        if (stop) { emitted = base + first; open = false; }
    }
    piled = wave_sum_u64(piled);
    if (lane == 0) { sums[EXTEND_END_SUMS * end] = emitted; sums[EXTEND_END_SUMS * end + 1] = piled; }
}

hipError_t launch_build_anchor(const BaitView &B, const uint64_t *rec_start, uint32_t n_rec, const KmerSetView &S, Anchor *anchor, uint32_t *lo,
                               uint32_t *hi, hipStream_t st)
{
    const uint64_t slots = S.slot_mask + 1;
    hipError_t e = hipMemsetAsync(lo, 0xFF, slots * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(hi, 0, slots * 4, st);
    if (e != hipSuccess) return e;
    if (B.total && n_rec) {
        if (S.kw == 1) hipLaunchKernelGGL(anchor_span_kernel<1>, dim3(grid_of(B.total, 256)), dim3(256), 0, st, B, S, lo, hi);
        else hipLaunchKernelGGL(anchor_span_kernel<2>, dim3(grid_of(B.total, 256)), dim3(256), 0, st, B, S, lo, hi);
    }
    if (S.kw == 1) hipLaunchKernelGGL(anchor_finish_kernel<1>, dim3(grid_of(slots, 256)), dim3(256), 0, st, B, rec_start, n_rec, S.k, lo, hi, anchor, slots);
    else hipLaunchKernelGGL(anchor_finish_kernel<2>, dim3(grid_of(slots, 256)), dim3(256), 0, st, B, rec_start, n_rec, S.k, lo, hi, anchor, slots);
    return hipGetLastError();
}

hipError_t launch_place_init(PlaceOut *place, uint64_t n_reads, hipStream_t st)
{
    if (!n_reads) return hipSuccess;
    hipLaunchKernelGGL(place_init_kernel, dim3(grid_of(n_reads, 256)), dim3(256), 0, st, place, n_reads);
    return hipGetLastError();
}

hipError_t launch_max_read_len(const uint64_t *offsets, uint64_t n_reads, unsigned long long *max_len, hipStream_t st)
{
    if (!n_reads) return hipSuccess;
    hipLaunchKernelGGL(max_read_len_kernel, dim3(grid_of(n_reads, 256)), dim3(256), 0, st, offsets, n_reads, max_len);
    return hipGetLastError();
}

hipError_t launch_place(const ReadsView &R, const KmerSetView &S, const Anchor *anchor, const uint64_t *rec_start, const uint32_t *list,
                        const unsigned long long *n_list, uint32_t n_rec, PlaceOut *place, unsigned long long *diff, unsigned long long *counts,
                        unsigned long long *pile, const PlaceVerify *verify, int n_cu, hipStream_t st)
{
    if (!R.n_reads) return hipSuccess;
    // the launch shape of launch_assign: four workgroups (32 waves) a CU at most, never more waves than reads
    const uint64_t waves = std::min<uint64_t>((uint64_t)(n_cu > 0 ? n_cu : 1) * 32, R.n_reads);
    const unsigned grid = grid_of(waves, ASSIGN_BLOCK / 64);
    const auto launch = [&](auto V) {                        // the instantiation that V's type, the key width and the pile-up name
        dispatch_kw_flag(S.kw, pile != nullptr, [&](auto KW, auto PILE) {
            hipLaunchKernelGGL((place_kernel<decltype(KW)::value, decltype(PILE)::value, decltype(V)::verify, decltype(V)::keep_rule>), dim3(grid),
                               dim3(ASSIGN_BLOCK), 0, st, R, S, anchor, rec_start, list, n_list, n_rec, place, diff, counts, pile, V);
        });
    };
    if (verify) {
        const PlaceCut &C = verify->cut;
        VerifyArgs<true, true> K;
        K.bait = C.bait; K.max_permille = C.max_permille; K.score = verify->score; K.sums = C.sums;
        K.keep_bits = C.keep_bits; K.keep = C.keep;
        if (K.keep_bits) launch(K); else launch(static_cast<const VerifyArgs<true, false> &>(K));
    } else launch(VerifyArgs<false, false>{});
    return hipGetLastError();
}

uint64_t place_scan_tiles(uint64_t total) { return (total + PS_TILE - 1) / PS_TILE; }

// the tiles' exclusive prefixes of the difference counters into partial: what tile_scan_begin starts from
static void launch_tile_partials(const unsigned long long *diff, uint64_t total, unsigned long long *partial, uint64_t nb, hipStream_t st)
{
    hipLaunchKernelGGL(place_scan_reduce_kernel, dim3((unsigned)nb), dim3(PS_BLOCK), 0, st, diff, total, partial);
    hipLaunchKernelGGL(place_scan_partials_kernel, dim3(1), dim3(PS_BLOCK), 0, st, partial, nb);
}

hipError_t launch_place_profile(const unsigned long long *diff, uint64_t total, const uint64_t *rec_start, uint32_t n_rec, unsigned long long *partial,
                                uint32_t *depth, unsigned long long *rec_sums, hipStream_t st)
{
    const uint64_t nb = place_scan_tiles(total);
    if (!nb || !n_rec) return hipSuccess;
    launch_tile_partials(diff, total, partial, nb, st);
    hipLaunchKernelGGL(place_profile_kernel, dim3((unsigned)nb), dim3(PS_BLOCK), 0, st, diff, total, partial, rec_start, n_rec, depth, rec_sums);
    return hipGetLastError();
}

hipError_t launch_pileup_call(const unsigned long long *pile, const BaitView &B, const uint64_t *rec_start, uint32_t n_rec, uint32_t min_depth,
                              PileOut *out, uint8_t *consensus, unsigned long long *rec_sums, hipStream_t st)
{
    const uint64_t nb = place_scan_tiles(B.total);
    if (!nb || !n_rec) return hipSuccess;
    hipLaunchKernelGGL(pileup_call_kernel, dim3((unsigned)nb), dim3(PS_BLOCK), 0, st, pile, B, rec_start, n_rec, min_depth, out, consensus, rec_sums);
    return hipGetLastError();
}

hipError_t launch_gapped_call(const unsigned long long *diff, uint64_t total, const unsigned long long *indel, const unsigned long long *ins_pile, uint32_t span,
                              const uint8_t *consensus, const uint64_t *rec_start, uint32_t n_rec, uint32_t min_depth, unsigned long long *partial,
                              PileOut *ins_out, uint8_t *count, uint8_t *bytes, unsigned long long *rec_sums, hipStream_t st)
{
    const uint64_t nb = place_scan_tiles(total);
    if (!nb || !n_rec) return hipSuccess;
    launch_tile_partials(diff, total, partial, nb, st);
    hipLaunchKernelGGL(gapped_call_kernel, dim3((unsigned)nb), dim3(PS_BLOCK), 0, st, diff, total, partial, indel, ins_pile, span, consensus, rec_start, n_rec,
                       min_depth, ins_out, count, bytes, rec_sums);
    return hipGetLastError();
}

hipError_t launch_extend_call(const unsigned long long *ext_pile, uint32_t extend, uint32_t n_rec, uint32_t min_depth, PileOut *ext_out, uint8_t *bytes,
                              unsigned long long *sums, hipStream_t st)
{
    if (!extend || !n_rec) return hipSuccess;
    const uint32_t n_ends = 2 * n_rec;
    hipLaunchKernelGGL(extend_call_kernel, dim3(grid_of(n_ends, PS_BLOCK / 64)), dim3(PS_BLOCK), 0, st, ext_pile, extend, n_ends, min_depth, ext_out, bytes, sums);
    return hipGetLastError();
}

} // namespace mf
