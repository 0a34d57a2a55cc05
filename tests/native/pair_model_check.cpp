// The rescue of an unplaced mate (mitoflex_amd/csrc/mf_rescue.h over mf_score.h) on the CPU, as rescue_kernel of mf_pairs.hip runs it,
// against a per-base loop over strings.  Built by tests/test_pair_model.py with -fsanitize=address,undefined: every array is on the heap
// and holds exactly the words the contract names -- the read stream's words, the copy of the read's words a wave stages (nw words, the
// read's offset reduced to its place in the first), one bit a base for a read with an N, the bait's packed letters and validity bits
// padded by one word -- so an index one word too far stops the program.
//
// The model: candidate c of the window goes to lane c mod 64, which folds it (rescue_fold_add); the 64 folds are combined in the
// butterfly's order (rescue_fold_merge); rescue_wins and the fold's d decide.  The reference: every candidate scored base by base over
// strings, the admissible ones with the fewest mismatches counted.
// The long read's path: a read beyond the 994 bases a wave stages is scored from the stream itself with its full b0 -- sixteen bases at a
// time without an N, and with one base by base over every offset that holds none, as the kernel's loop over read_letter and score_base
// does; both are held to the staged copy's score (and so to the per-base loop), at every candidate for the lengths around the limit.
// The sweep: window widths 1, 63, 64, 65 and 4096 (the reads beyond 151 bases: 1 and 65, no ties) with the true insert first, last and inside; L = k, 47, 48, 49,
// 150, 151, 993, 994, 995, 1200 (994 with b0 mod 16 = 15 fills the slice's 64 words); every b0 mod 16; both strands; the mate over both ends of the FIRST and of the LAST record of the set (exactly k bases inside, and k - 1),
// at either end and inside; a bait N and a read N in the footprint; ties planted through a stretch of period 7.
// Prints "pair model ok: <cases> cases <rescued> rescued <ties> ties <short> short <candidates of reads with an N scored from the stream>
// streamed_n" and exits 0, or the first difference and exits 1.
#include "../../mitoflex_amd/csrc/mf_rescue.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
static char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
static uint32_t code(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }

struct Words {
    uint32_t *w; size_t n;
    explicit Words(size_t n_) : w((uint32_t *)calloc(n_ ? n_ : 1, 4)), n(n_) {}
    ~Words() { free(w); }
    Words(const Words &) = delete;
};

struct Case { uint32_t compared, mismatches; };
static Case per_base(const std::string &rec, const std::string &read, uint32_t strand, int64_t start)
{
    Case out{0, 0};
    const int64_t L = (int64_t)read.size(), len = (int64_t)rec.size();
    for (int64_t i = 0; i < L; i++) {
        const int64_t c = strand ? start + (L - 1 - i) : start + i;
        const char r = strand ? comp(read[(size_t)i]) : read[(size_t)i];
        if (c < 0 || c >= len || r == 'N' || rec[(size_t)c] == 'N') continue;
        out.compared++;
        out.mismatches += r != rec[(size_t)c];
    }
    return out;
}

int main()
{
    const uint32_t k = 21, permille = 100;
    const int lengths[] = {(int)k, 47, 48, 49, 150, 151, 993, 994, 995, 1200};
    const uint32_t widths[] = {1, 63, 64, 65, 4096};
    unsigned long long cases = 0, rescued = 0, ties = 0, shorts = 0, streamed_n = 0;
    for (int L : lengths)
        for (int which_rec = 0; which_rec < 2; which_rec++)                     // the record under test: the set's first, its last
            for (int with_n = 0; with_n < 2; with_n++)
                for (int tie = 0; tie < 2; tie++) {
                    const int64_t len = 2 * L + 75, other = 83;
                    const uint64_t s0 = which_rec ? (uint64_t)other : 0, total = (uint64_t)(len + other);
                    std::string bait(total, 'A');
                    for (auto &c : bait) c = "ACGT"[rnd() & 3u];
                    Words bw((total + 15) / 16 + 1), bv((total + 31) / 32 + 1);
                    // the true positions of the mate: k - 1 and k bases inside at either end, the ends themselves, the middle
                    const int64_t trues[] = {-(int64_t)L + (int64_t)k - 1, -(int64_t)L + (int64_t)k, 0, (len - L) / 2, len - L, len - (int64_t)k, len - (int64_t)k + 1};
                    for (int64_t tstart : trues) {
                        std::string b = bait;
                        if (tie) for (int64_t c = 7; c < len; c++) b[s0 + (size_t)c] = b[s0 + (size_t)c - 7];          // the whole record has period 7
                        if (with_n) { const int64_t c = tstart + L / 2; if (c >= 0 && c < len) b[s0 + (size_t)c] = 'N'; b[s0] = 'N'; b[s0 + (size_t)len - 1] = 'N'; }
                        for (size_t i = 0; i < bw.n; i++) bw.w[i] = 0;
                        for (size_t i = 0; i < bv.n; i++) bv.w[i] = 0;
                        for (uint64_t p = 0; p < total; p++)
                            if (b[p] != 'N') { bw.w[p >> 4] |= code(b[p]) << (2 * (p & 15)); bv.w[p >> 5] |= 1u << (p & 31); }
                        const mf::ScoreBait SB{bw.w, bw.n - 1, bv.w, bv.n - 1};
                        const std::string rec = b.substr(s0, (size_t)len);
                        for (uint32_t width : widths)
                            for (int where = 0; where < 3; where++)              // the true insert first, last, inside
                                for (uint32_t strand_a = 0; strand_a < 2; strand_a++)
                                    for (uint32_t bmod = 0; bmod < 16; bmod++) {
                                        if (width == 4096 && (bmod % 8 != 3 || where == 2)) continue;
                                        if (L > 151 && (tie || (width != 1 && width != 65) || where == 2)) continue;          // (the long reads: fewer windows)
                                        if (width == 1 && where) continue;
                                        const int read_n = (int)(rnd() & 1u);
                                        const uint32_t strand = strand_a ^ 1u;                 // the looked-for mate's
                                        // the mate as the record reads at tstart on its strand, a substitution every 20 bases, an N for some
                                        std::string fwd((size_t)L, 'A');
                                        for (int64_t i = 0; i < L; i++) {
                                            const int64_t c = tstart + i;
                                            fwd[(size_t)i] = (c >= 0 && c < len && rec[(size_t)c] != 'N') ? rec[(size_t)c] : "ACGT"[rnd() & 3u];
                                            if (i % 20 == 11 && !tie) fwd[(size_t)i] = "CGTA"[code(fwd[(size_t)i])];
                                        }
                                        std::string read = fwd;
                                        if (strand) for (int64_t i = 0; i < L; i++) read[(size_t)i] = comp(fwd[(size_t)(L - 1 - i)]);
                                        if (read_n) read[(size_t)(L / 3)] = 'N';
                                        // the window and the settled mate that imply it
                                        const uint32_t d_true = 5000 + (rnd() & 63u);
                                        const uint32_t off = where == 0 ? 0 : where == 1 ? width - 1 : width / 2;
                                        const uint32_t min_insert = d_true - off, max_insert = min_insert + width - 1;
                                        const int64_t a = tstart + L - (int64_t)d_true, e = tstart + (int64_t)d_true;          // (each used on its strand)
                                        if (mf::rescue_start(strand_a, a, e, (uint64_t)L, d_true) != tstart) { printf("DIFFERS: rescue_start\n"); return 1; }
                                        // the stream: three filler words, bmod filler bases, the read as its LAST bases
                                        const uint64_t b0 = 48 + bmod, nb = b0 + (uint64_t)L;
                                        Words rw((nb + 15) / 16);
                                        for (uint64_t g = 0; g < nb; g++) rw.w[g >> 4] |= (g < b0 ? rnd() & 3u : code(read[g - b0] == 'N' ? 'T' : read[g - b0])) << (2 * (g & 15));
                                        // what a wave stages
                                        const uint32_t nw = (uint32_t)(((b0 & 15u) + (uint64_t)L + 15) >> 4);
                                        if (L <= 994 && nw > 64) { printf("DIFFERS: %u words of a staged read of %d bases\n", nw, L); return 1; }
                                        Words staged(nw), nmask(2 * (((size_t)L + 63) / 64));
                                        for (uint32_t t = 0; t < nw; t++) { const uint64_t g = (b0 >> 4) + t; staged.w[t] = rw.w[g < rw.n - 1 ? g : rw.n - 1]; }
                                        for (int64_t i = 0; i < L; i++) if (read[(size_t)i] == 'N') nmask.w[i >> 5] |= 1u << (i & 31);
                                        const uint64_t rb0 = b0 & 15u;
                                        mf::RescueFold lanes[64];
                                        for (auto &f : lanes) f = mf::rescue_fold_empty();
                                        // the reference beside it
                                        uint32_t best = 0xFFFFFFFFu, best_d = 0, n_best = 0; bool reached = false;
                                        for (uint32_t c = 0; c < width; c++) {
                                            const uint32_t d = min_insert + c;
                                            const int64_t start = mf::rescue_start(strand_a, a, e, (uint64_t)L, d);
                                            const uint64_t sc = read_n ? mf::rescue_score_bases(staged.w, rb0, (uint64_t)L, strand, start, SB, s0, len, nmask.w)
                                                                       : mf::rescue_score_chunks(staged.w, nw - 1, rb0, (uint64_t)L, strand, start, SB, s0, len);
                                            mf::rescue_fold_add(lanes[c & 63u], (uint32_t)sc, (uint32_t)(sc >> 32), d, k, permille);
                                            const Case want = per_base(rec, read, strand, start);
                                            if ((uint32_t)sc != want.compared || (uint32_t)(sc >> 32) != want.mismatches) {
                                                printf("DIFFERS: L %d rec %d N %d/%d start %lld strand %u b0 %u: model %u/%u per-base loop %u/%u\n", L, which_rec, with_n, read_n,
                                                       (long long)start, strand, bmod, (uint32_t)sc, (uint32_t)(sc >> 32), want.compared, want.mismatches);
                                                return 1;
                                            }
                                            if (c == 0 || c == off || L > 151) {          // the long read's path: the stream itself, the read's first base at b0
                                                uint64_t sg = 0;
                                                if (!read_n) sg = mf::rescue_score_chunks(rw.w, rw.n - 1, b0, (uint64_t)L, strand, start, SB, s0, len);
                                                else {
                                                    for (uint64_t o = 0; o < (uint64_t)L; o++)
                                                        if (read[(size_t)o] != 'N') sg += mf::score_base(rw.w, b0, (uint64_t)L, strand, start, SB, s0, len, o);
                                                    streamed_n++;
                                                }
                                                if (sg != sc) {
                                                    printf("DIFFERS: the stream and its staged copy: L %d N %d start %lld strand %u b0 %u: %u/%u against %u/%u\n", L, read_n,
                                                           (long long)start, strand, bmod, (uint32_t)sg, (uint32_t)(sg >> 32), (uint32_t)sc, (uint32_t)(sc >> 32));
                                                    return 1;
                                                }
                                            }
                                            if (want.compared < k) continue;
                                            reached = true;
                                            if ((uint64_t)want.mismatches * 1000u > (uint64_t)permille * want.compared) continue;
                                            if (want.mismatches < best) { best = want.mismatches; best_d = d; n_best = 1; }
                                            else if (want.mismatches == best) n_best++;
                                        }
                                        for (int o = 32; o > 0; o >>= 1) {                  // the butterfly: every lane ends with the same fold
                                            mf::RescueFold next[64];
                                            for (int l = 0; l < 64; l++) next[l] = mf::rescue_fold_merge(lanes[l], lanes[l ^ o]);
                                            for (int l = 0; l < 64; l++) lanes[l] = next[l];
                                        }
                                        for (int l = 1; l < 64; l++)
                                            if (lanes[l].mismatches != lanes[0].mismatches || lanes[l].d != lanes[0].d || lanes[l].n != lanes[0].n) { printf("DIFFERS: lanes disagree\n"); return 1; }
                                        const mf::RescueFold f = lanes[0];
                                        const bool won = mf::rescue_wins(f);
                                        cases++;
                                        if (won != (n_best == 1) || f.mismatches != best || (won && f.d != best_d) || (n_best > 1) != (f.n > 1 && f.mismatches != 0xFFFFFFFFu)) {
                                            printf("DIFFERS: L %d rec %d N %d/%d tie %d true %lld window %u..%u strand %u b0 %u: fold %u d %u n %u, reference %u d %u n %u\n", L, which_rec,
                                                   with_n, read_n, tie, (long long)tstart, min_insert, max_insert, strand, bmod, f.mismatches, f.d, f.n, best, best_d, n_best);
                                            return 1;
                                        }
                                        rescued += won; ties += n_best > 1; shorts += !reached;
                                    }
                    }
                }
    printf("pair model ok: %llu cases %llu rescued %llu ties %llu short %llu streamed_n\n", cases, rescued, ties, shorts, streamed_n);
    return 0;
}
