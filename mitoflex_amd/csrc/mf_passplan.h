// What one filter pass runs and where its launches go, as one pure function of plain values, and the one definition of the tally block a pass
// writes.  Host-only (no HIP include): tests/test_passplan.py holds every rule here to a restatement of its own without a device.
#pragma once
#include "../../include/mitofilter.h"
#include "mf_kernels_cfg.h"
namespace mf {
// A pass's tally block: three regions -- phase 0 and phase 1 of the finish kernels, the exact kernel behind finish -- of EXACT_MAX_GRID (pass,
// candidate) pairs, two 64-bit words a pair.  Every other kind of pass tallies into region 0 alone.  Nothing clears a block between passes: a
// kernel overwrites its workgroups' pairs of the region it tallies into (the exact and protein kernels zero the rest of theirs) and leaves the
// other regions as an earlier pass -- of another set, perhaps -- left them.  So a pass is summed over the regions it wrote, PassPlan::tally_regions.
struct TallyLayout {
    static constexpr int REGIONS = 3;
    static constexpr size_t region(int i) { return (size_t)i * EXACT_MAX_GRID * 2; }          // word offset of region i
    static constexpr size_t words() { return region(REGIONS); }
    static constexpr size_t bytes() { return words() * sizeof(unsigned long long); }
    struct Totals { unsigned long long pass = 0, cand = 0; };
    static Totals sum(const unsigned long long *block, int regions) { Totals t; for (size_t i = 0; i < region(regions); i += 2) { t.pass += block[i]; t.cand += block[i + 1]; } return t; }
};
struct PassKnobs { int pass, finish_streams, screen_streams, split_pipe, exact_co, s8_finish; };          // the per-pass options (mf_api.cpp PassOptions), read once a pass
// Bait-rich input (more than a few per cent of the reads are bait reads -- what the `bim` loop enriches towards) is better
// served by the candidate-bitmap pass: one thread per stage-1 record means several records per bait read, and the screen
// writes them all.  The choice follows the work the last call of this read set (the last batch of this device) saw (adapt_after_call).
// finish_two: the finish kernels of consecutive passes go to two streams; split_serial: very many candidates (> 5 % of the reads), the candidate-bitmap pass on one stream
struct PassFeedback { bool prefer_split = false, finish_two = false, split_serial = false; };
struct PassInputs {
    int prot, s, stride, kw, k, s8_finish;                       // the set (KmerSetView)
    unsigned thr; int mode; bool count_all, overlap, more;       // the call; overlap: it has several passes (the streams exist), more: another pass of it follows
    PassFeedback fb; int flip, cur, nsets;                       // the read set; flip: parity of the pipelined passes so far, cur: the buffer set of the latest result
};
enum class PassKind { PROTEIN, FINISH, SPLIT_PIPELINED, ONE_STREAM };
enum class PassStream { MAIN, FINISH_A, SCREEN_ALT, FINISH_B };          // DevCtx: stream, stream2, stream3, stream4
struct PassPlan {
    PassKind kind = PassKind::ONE_STREAM; int q = 0, q_out = 0;          // q: the buffer set of the records and candidates; q_out: of the result bits and the tally
    PassStream screen_on = PassStream::MAIN, later_on = PassStream::MAIN;          // two_streams: not the same, ev_screen[q] orders them; screen: one runs (and, but in a FINISH pass, a mark kernel)
    bool two_streams = false, wait_prev_finish = false, screen = false, screen_clears_bits = false, needs_cand = false, exact_behind_finish = false, exact_coresident = false;
    int flip = 0, cur = 0; bool sample_pass = false;          // what the read set holds after the pass
    int tally_regions = 1;          // the leading regions of the tally block this pass writes: what its totals are summed over (TallyLayout::sum)
};
inline PassPlan plan_pass(const PassKnobs &kn, const PassInputs &in)
{
    PassPlan p; p.flip = in.flip; p.cur = p.q_out = in.cur;
    if (in.prot) { p.kind = PassKind::PROTEIN; return p; }          // protein-space set: one kernel translates and probes every read (no screen exists in residue space)
    const bool screened = in.mode == MF_MODE_SCREENED && in.s > 0;
    // (stride-8 geometries, k < 28: twice the samples, several times the records -- measured faster through the candidate bitmap for a bait the LDS table
    // screens well, 16.5 kbp: k = 21 0.314 against 0.319 ms a pass, k = 25 / 27 0.292 against 0.298.  Beyond ~20 kbp the candidate bitmap's exact kernel is
    // what a pass waits for -- its LDS k-mer table fills up -- and screen + finish is faster: k = 21 33 kbp 0.50 -> 0.45, 50 kbp 0.74 -> 0.55, 100 kbp
    // 1.88 -> 1.51, 350 kbp 3.03 -> 1.98, k = 25 100 kbp 1.68 -> 1.21: KmerSetView::s8_finish, profiles/r06/o_stride8_finish.txt)
    // (round 3, after the stage-1 fields were fixed for 14-base samples: still the faster pass for stride 8 -- k = 21 0.299 vs 0.302-0.309 ms, k = 25 0.278-0.280 vs 0.281-0.283)
    const bool s8 = kn.s8_finish < 0 ? in.s8_finish != 0 : kn.s8_finish == 1;
    const bool finish = screened && kn.pass != 1 && !in.fb.prefer_split && in.thr == 1 && !in.count_all && (in.stride == 16 || kn.pass == 2 || s8);
    const bool split = !finish && screened && !in.count_all && in.overlap && kn.split_pipe && kn.pass != 2 && !in.fb.split_serial;
    // ONE_STREAM (hit counts wanted, the exhaustive mode, MF_PASS=serial): records and candidates of set 0.  split / exhaustive: no per-pass memsets --
    // the exact kernel clears the candidate words it consumes, writes every result word and zeroes unused tally slots
    if (!finish && !split) { p.screen = p.needs_cand = screened; return p; }
    // FINISH: the screen records its stage-1 positives (and clears this pass's result bitmap on the side), the finish kernels settle them and set
    // the pass bits with atomics.  SPLIT_PIPELINED: the three-kernel pass.  Either way pass i works on buffer set i mod 2 (records, candidate bitmap,
    // result bitmap, tallies) and its later kernels go to the second stream and run beside the screen of pass i + 1, which uses the other set.
    // (three buffer sets for pipelined passes: the screen of pass i + 3 waits for the finish kernels of pass i, not of pass i + 1 -- with two sets a
    // finish chain that outlasts the next screen, as the two-word keys' does, held the screen after that: k = 41 0.243 -> 0.234 ms a pass, k = 63 0.257 -> 0.250 (k = 31
    // 0.224 -> 0.222, 33 kbp 0.243 -> 0.237), profiles/r06/n_three_sets.txt.  A call of one pass -- a file-level call's batches -- keeps to two.)
    // (Kept to the two-word keys: for k <= 32 it is worth 1-2 %, and with three sets two or three screens are in flight at a time, so that a launch
    // lasts twice what a pass takes -- the per-launch figure bench.py's `roofline` reports for the headline would no longer say what the pass does.)
    const bool two = split || (in.overlap && kn.pass == 0);
    const int odd = (p.flip ^= 1);
    p.kind = finish ? PassKind::FINISH : PassKind::SPLIT_PIPELINED;
    p.screen = true; p.two_streams = p.wait_prev_finish = two;          // (waits: the later kernels of nsets passes ago worked on this set)
    p.q = p.q_out = p.cur = (in.cur + 1) % (two && in.kw == 2 ? in.nsets : 2);
    // consecutive screens go to two streams in turn: nothing orders them against each other (different buffer sets), so the
    // workgroups of the next screen take over the CUs as the last ones of this screen drain (MF_SCREEN_STREAMS=1: one stream)
    p.screen_on = two && kn.screen_streams == 2 && odd ? PassStream::SCREEN_ALT : PassStream::MAIN;
    // The finish kernels are chains of memory latencies.  With few records (the benchmark's 0.5 % bait reads) they are over long
    // before the next screen is and one stream carries them all; when they are what a pass waits for (bait-rich input: 2 % bait
    // reads and more, seen in the last call's tallies) those of consecutive passes go to two streams and run side by side --
    // 2 %: 0.303 -> 0.280 ms per pass, 10 %: 0.666 -> 0.596; at 0.5 % the same costs 2 % (0.208 -> 0.213).  MF_FINISH_STREAMS=1 / 2 forces.
    // (two-word keys, k >= 33: a finish kernel's probes are twice as long, and one stream's worth of them is not over when the next screen is --
    // k = 41 0.2369 -> 0.2331 ms a pass, k = 63 0.2960 -> 0.2817: profiles/r05/c_k41_finish_streams_probe.txt)
    const bool fin2 = finish && (kn.finish_streams == 2 || (kn.finish_streams == 0 && (in.fb.finish_two || in.kw == 2)));
    p.later_on = !two ? PassStream::MAIN : fin2 && odd ? PassStream::FINISH_B : PassStream::FINISH_A;
    p.screen_clears_bits = p.sample_pass = finish;
    // For k >= 48 (runs of four and more samples: fewer reads are settled by a run) phase 1 hands the reads that hold a bait s-mer outside
    // any run to an exact kernel behind it, which deals a read's windows to eight lanes, instead of counting them on the one lane that met
    // the s-mer: k = 63 0.283 -> 0.257 ms a pass.  Below that the third launch costs more than the tail it removes (k = 31 0.219 -> 0.226,
    // k = 41 0.235 -> 0.248, 33 kbp bait 0.228 -> 0.262: profiles/r06/j_finish_exact_ab.txt).  (An experiment build overrides it: an expression of `in`.)
#ifndef MF_FINISH_EXACT
#define MF_FINISH_EXACT (in.k >= 48)
#endif
    p.exact_behind_finish = finish && MF_FINISH_EXACT;          // (merges into the finish kernels' bits, tallies into region 2)
    p.tally_regions = !finish ? 1 : p.exact_behind_finish ? 3 : 2;          // (a finish pass without it leaves region 2 as a pass of another set wrote it)
    p.needs_cand = split || p.exact_behind_finish;
    // the exact kernel takes its co-resident form when a screen follows (a screen workgroup holds 128 KiB of every CU's LDS for the whole pass), its
    // full form behind the last screen of the call (exact_co, tests: the co-resident form behind every screen)
    p.exact_coresident = finish ? p.exact_behind_finish && in.more : in.more || kn.exact_co;
    return p;
}
// After a call, from its last pass's candidate total: work items per read of a screen + finish pass -- ~0.025 at 0.5 % bait reads, 0.4 at
// 10 %, 0.8 at 20 % -- or candidate reads per read of a candidate-bitmap pass.  (Since a run start is left to the first lane that holds one,
// the two kinds of pass are within 5 % of each other from 2 % to 100 % bait reads; the switch stays for inputs that are nearly all bait.)
inline PassFeedback adapt_after_call(PassFeedback f, bool sample_pass, unsigned long long cand, unsigned long long n_reads)
{
    if (n_reads < 100000) return f;
    if (sample_pass) { if (cand > n_reads) f.prefer_split = true; f.finish_two = cand > n_reads / 20; return f; }
    if (f.prefer_split && cand < n_reads / 8) f.prefer_split = false;
    if (cand > n_reads / 20) f.split_serial = true; else if (cand < n_reads / 40) f.split_serial = false;
    return f;
}
} // namespace mf
