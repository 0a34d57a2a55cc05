// The 16-base compare of the verifying placement (mitoflex_amd/csrc/mf_score.h) on the CPU, against a per-base loop over strings.
// Built by tests/test_score_model.py with -fsanitize=address,undefined: every array is on the heap and holds exactly the words the
// contract names (the read stream's words; the bait's packed letters and validity bits padded by one word), so a funnel read that goes
// one word too far, or a clamp that is missing, stops the program.
//
// The sweep: every (b0 mod 16) x (start mod 16) x strand; lengths 21, 32, 33, 47, 48, 49, 150, 1500; start from -16 to +16 around 0
// and around len - L; the read on the LAST record of the set and as the LAST read of the stream; a bait N inside the footprint;
// mismatches planted at read offsets 0, L - 1, 15, 16, 17.  Prints "score model ok: <cases> cases" and exits 0, or the first
// difference and exits 1.
#include "../../mitoflex_amd/csrc/mf_score.h"

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
static uint32_t code(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }          // (N packs as T's code: any letter would do)

// exactly-sized heap array of n words
struct Words {
    uint32_t *w; size_t n;
    explicit Words(size_t n_) : w((uint32_t *)calloc(n_ ? n_ : 1, 4)), n(n_) {}
    ~Words() { free(w); }
    Words(const Words &) = delete;
};

struct Case { uint64_t compared, mismatches; };

// the header's text, base by base over strings: bait record `rec` (letters, N invalid), read text as it lies in the stream
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
    const int lengths[] = {21, 32, 33, 47, 48, 49, 150, 1500};
    unsigned long long cases = 0;
    for (int L : lengths) {
        // the set: a first record of 37 positions, then the record under test as the LAST one; its length is no multiple of 16 or 32 in
        // one pass and a multiple in the other, so that the word behind the end both is and is not the padding word
        for (int len_kind = 0; len_kind < 2; len_kind++) {
            const int64_t len = len_kind ? (int64_t)((L + 37 + 64 + 31) / 32 * 32 - 37) : (int64_t)L + 41;
            const uint64_t s0 = 37, total = s0 + (uint64_t)len;
            std::string bait(total, 'A');
            for (auto &c : bait) c = "ACGT"[rnd() & 3u];
            for (int with_n = 0; with_n < 2; with_n++) {
                std::string b = bait;
                if (with_n) { b[s0 + (size_t)len / 2] = 'N'; b[s0] = 'N'; b[total - 1] = 'N'; }
                Words bw((total + 15) / 16 + 1), bv((total + 31) / 32 + 1);
                for (uint64_t p = 0; p < total; p++) {
                    if (b[p] != 'N') { bw.w[p >> 4] |= code(b[p]) << (2 * (p & 15)); bv.w[p >> 5] |= 1u << (p & 31); }
                }
                const mf::ScoreBait SB{bw.w, bw.n - 1, bv.w, bv.n - 1};
                const std::string rec = b.substr(s0);
                std::vector<int64_t> starts;
                for (int64_t d = -16; d <= 16; d++) { starts.push_back(d); starts.push_back(len - L + d); }
                for (int64_t start : starts)
                    for (uint32_t strand = 0; strand < 2; strand++)
                        for (uint32_t bmod = 0; bmod < 16; bmod++) {
                            // the read as the bait's footprint reads on its strand (random where it hangs over), mismatches planted
                            std::string fwd((size_t)L, 'A');
                            for (int64_t i = 0; i < L; i++) {
                                const int64_t c = start + i;
                                fwd[(size_t)i] = (c >= 0 && c < len && rec[(size_t)c] != 'N') ? rec[(size_t)c] : "ACGT"[rnd() & 3u];
                            }
                            std::string read = fwd;
                            if (strand) for (int64_t i = 0; i < L; i++) read[(size_t)i] = comp(fwd[(size_t)(L - 1 - i)]);
                            const int planted[] = {0, L - 1, 15, 16, 17};
                            const uint32_t which = rnd();
                            for (int q = 0; q < 5; q++)
                                if ((which >> q) & 1u) { char &c = read[(size_t)planted[q]]; c = "CGTA"[code(c)]; }
                            // the stream: bmod filler bases, then the read as its LAST bases; exactly the words that hold them
                            const uint64_t b0 = bmod, nb = b0 + (uint64_t)L;
                            Words rw((nb + 15) / 16);
                            for (uint64_t g = 0; g < nb; g++) rw.w[g >> 4] |= (g < b0 ? rnd() & 3u : code(read[g - b0])) << (2 * (g & 15));
                            int64_t lo, hi;
                            mf::score_footprint((uint64_t)L, start, len, lo, hi);
                            uint64_t acc = 0, acc_base = 0;
                            for (uint64_t t = 0; 16 * (int64_t)t < hi - lo; t++) acc += mf::score_chunk16(rw.w, rw.n - 1, b0, (uint64_t)L, strand, start, SB, s0, lo, hi, t);
                            for (uint64_t i = 0; i < (uint64_t)L; i++) acc_base += mf::score_base(rw.w, b0, (uint64_t)L, strand, start, SB, s0, len, i);
                            const Case want = per_base(rec, read, strand, start);
                            cases++;
                            if ((uint32_t)acc != want.compared || (acc >> 32) != want.mismatches || acc_base != acc) {
                                printf("DIFFERS: L %d len %lld N %d start %lld strand %u b0 %u: chunks %u/%u bases %u/%u per-base loop %llu/%llu\n", L, (long long)len, with_n,
                                       (long long)start, strand, bmod, (uint32_t)acc, (uint32_t)(acc >> 32), (uint32_t)acc_base, (uint32_t)(acc_base >> 32),
                                       (unsigned long long)want.compared, (unsigned long long)want.mismatches);
                                return 1;
                            }
                            if (mf::score_accepts((uint32_t)want.compared, (uint32_t)want.mismatches, 1000) != true
                                || mf::score_accepts((uint32_t)want.compared, (uint32_t)want.mismatches, 0) != (want.mismatches == 0)) { printf("DIFFERS: the cut\n"); return 1; }
                        }
            }
        }
    }
    printf("score model ok: %llu cases\n", cases);
    return 0;
}
