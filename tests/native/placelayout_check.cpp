// Stand-alone check of mitoflex_amd/csrc/mf_placelayout.h (tests/test_placelayout.py builds it with ASan + UBSan): every offset of
// PlaceLayout and every section of ReportScratch against the formulas restated here, from the comments above the two structs and
// the sizes the three report calls reserved before they shared one layout.
#include "../../mitoflex_amd/csrc/mf_placelayout.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s  [P=%llu R=%llu pileup=%d verify=%d place=%d pile=%d tiles=%llu]\n", __FILE__, __LINE__, #c, \
    (unsigned long long)P, (unsigned long long)R, pileup, verify, place, pile, (unsigned long long)tiles); exit(1); } } while (0)

using W = unsigned long long;
static uint64_t P, R, tiles; static int pileup, verify, place, pile;
static size_t max1(uint64_t v) { return (size_t)(v ? v : 1); }

static void check_layout()
{
    const mf::PlaceLayout L(P, (size_t)R, pileup, verify, 777);
    // [4 P pile-up counters, only with a pile-up | P + 1 difference counters | 4 R + 1 record counters | verifying: 33 R gathered, 2 R sums]
    const size_t n_pile = pileup ? 4 * P : 0, n_diff = P + 1, n_cnt = 4 * R + 1, n_score = verify ? (33 + 2) * R : 0;
    CHECK(L.n_pile == n_pile && L.n_diff == n_diff && L.n_cnt == n_cnt && L.n_rec == R && L.n_score() == n_score);
    CHECK(L.verify == (bool)verify && L.max_permille == 777);
    CHECK(L.words() == n_pile + n_diff + n_cnt + n_score);
    W *const base = reinterpret_cast<W *>((uintptr_t)1 << 20);          // (never dereferenced)
    const uintptr_t b = (uintptr_t)base;
    CHECK(L.pile(base) == (n_pile ? base : nullptr));
    CHECK((uintptr_t)L.diff(base) == b + 8 * n_pile);
    CHECK((uintptr_t)L.cnt(base) == b + 8 * (n_pile + n_diff));
    CHECK((uintptr_t)L.score_sums(base) == b + 8 * (n_pile + n_diff + n_cnt + 33 * R));
}

static void check_score_records()
{
    const mf::PlaceLayout L(P, (size_t)R, pileup, true, 1000);
    std::vector<W> h(L.n_cnt + L.n_score());
    for (size_t i = 0; i < h.size(); i++) h[i] = 1000 + i;          // distinct: a field says which word it came from
    std::vector<mf_score_record_t> out(R);
    L.score_records(h.data(), out.data());
    const size_t g = 4 * R + 1, sums = g + 33 * R;
    for (size_t j = 0; j < R; j++) {
        CHECK(out[j].accepted == h[4 * j] + h[4 * j + 1] && out[j].rejected == h[g + 33 * j]);
        CHECK(out[j].compared == h[sums + 2 * j] && out[j].mismatches == h[sums + 2 * j + 1]);
        for (size_t bin = 0; bin < MF_SCORE_BINS; bin++) CHECK(out[j].hist[bin] == h[g + 33 * j + 1 + bin]);
    }
}

static void check_scratch()
{
    using S = mf::ReportScratch;
    const S s(P, (size_t)R, tiles, place, pile);
    // what the calls reserved before: placement's work words and base depth; the pile-up's sums, called pile-up and consensus
    const size_t work = (2 * R + tiles + 1) * 8, depth = max1(P) * 4, psums = max1(R) * 6 * 8, pout = max1(P) * 16, cons = max1(P);
    const S::Section *in_sums[] = {&s.work, &s.pile_sums}, *in_pos[] = {&s.pile_out, &s.depth, &s.consensus, &s.spare};
    size_t at = 0;
    for (const S::Section *x : in_sums) { CHECK(x->off >= at && x->off + x->bytes <= s.sums_bytes); at = x->off + x->bytes; }          // inside, in order: none overlaps
    at = 0;
    for (const S::Section *x : in_pos) { CHECK(x->off >= at && x->off + x->bytes <= s.pos_bytes); at = x->off + x->bytes; }
    CHECK(s.work.bytes == (place ? work : 0) && s.depth.bytes == (place ? depth : 0));
    CHECK(s.pile_sums.bytes == (pile ? psums : 0) && s.pile_out.bytes == (pile ? pout : 0) && s.consensus.bytes == (pile ? cons : 0) && s.spare.bytes == (pile ? 16u : 0u));
    CHECK(s.pile_out.off == 0 && s.depth.off % 4 == 0 && s.pile_sums.off % 8 == 0);
    if (place && !pile) CHECK(s.sums_bytes == work && s.pos_bytes == depth);                       // mf_place
    if (pile && !place) CHECK(s.sums_bytes == psums && s.pos_bytes == pout + cons + 16);           // mf_pileup
    CHECK(s.sums_bytes <= work + psums && s.pos_bytes <= pout + depth + cons + 16);                 // mf_verify, whatever it asks for
    uint8_t *const buf = reinterpret_cast<uint8_t *>((uintptr_t)1 << 20);          // (never dereferenced)
    CHECK((uintptr_t)s.depth.in<uint32_t>(buf) == (place ? (uintptr_t)buf + s.depth.off : 0));
    CHECK((uintptr_t)s.pile_sums.in<W>(buf) == (pile ? (uintptr_t)buf + s.pile_sums.off : 0));
}

int main()
{
    const uint64_t positions[] = {0, 1, 15, 16, 17, 1000, (1ull << 31) - 2}, records[] = {0, 1, 2, 1000};
    unsigned long long cases = 0;
    for (uint64_t p : positions)
        for (uint64_t r : records) {
            P = p; R = r;
            for (pileup = 0; pileup < 2; pileup++)
                for (verify = 0; verify < 2; verify++) {
                    check_layout();
                    check_score_records();
                    for (place = 0; place < 2; place++)
                        for (pile = 0; pile < 2; pile++)
                            for (uint64_t t : {(P + 1023) / 1024, (P + 255) / 256}) { tiles = t; check_scratch(); cases++; }
                }
        }
    printf("place layout ok: %llu cases\n", cases);
    return 0;
}
