// Stand-alone check of the gapped sections of mitoflex_amd/csrc/mf_placelayout.h (tests/test_gapped_layout.py builds it with ASan +
// UBSan): the sixth section of PlaceLayout -- the insertion pile behind the indel counters -- and the gapped sections of ReportScratch
// against the formulas restated here; and that a layout that is not gapped is what it was.
#include "../../mitoflex_amd/csrc/mf_placelayout.h"
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s  [P=%llu R=%llu pileup=%d band=%u gapped=%d place=%d]\n", __FILE__, __LINE__, #c, \
    (unsigned long long)P, (unsigned long long)R, pileup, band, gapped, place); exit(1); } } while (0)

using W = unsigned long long;
static uint64_t P, R; static int pileup, gapped, place; static uint32_t band;

static void check_layout()
{
    const mf::PlaceLayout L(P, (size_t)R, pileup, true, 40, true, band, gapped);
    const mf::PlaceLayout old(P, (size_t)R, pileup, true, 40, true, band);
    // [4 P pile-up | P + 1 difference | 4 R + 1 record | 33 R gathered, 5 R sums | 3 P indel | gapped: 4 * 2 * band * P insertion pile]
    const size_t n_pile = pileup ? 4 * P : 0, before = n_pile + (P + 1) + (4 * R + 1) + (33 + 5) * R + 3 * P, n_ins = gapped ? 4 * (size_t)(2 * band) * P : 0;
    CHECK(old.words() == before && old.n_ins == 0 && old.ins(nullptr) == nullptr);
    CHECK(L.n_ins == n_ins && L.words() == before + n_ins && L.span() == 2 * band);
    CHECK(L.n_pile == old.n_pile && L.n_diff == old.n_diff && L.n_cnt == old.n_cnt && L.n_score() == old.n_score() && L.n_indel == old.n_indel);
    W *const base = reinterpret_cast<W *>((uintptr_t)1 << 20);          // (never dereferenced)
    CHECK(L.pile(base) == old.pile(base) && L.diff(base) == old.diff(base) && L.cnt(base) == old.cnt(base) && L.score_sums(base) == old.score_sums(base));
    CHECK(L.indel(base) == old.indel(base));
    CHECK(L.ins(base) == (n_ins ? base + before : nullptr));
    if (n_ins) CHECK(L.ins(base) == L.indel(base) + 3 * P);
    // a placement that does not align has no such section, whatever it is told
    CHECK(mf::PlaceLayout(P, (size_t)R, pileup, true, 40, false, band, gapped).n_ins == 0);
}

static void check_scratch()
{
    using S = mf::ReportScratch;
    const uint64_t tiles = (P + 4095) / 4096;
    const S old(P, (size_t)R, tiles, place, pileup), plain(P, (size_t)R, tiles, place, pileup, -1);
    CHECK(old.sums_bytes == plain.sums_bytes && old.pos_bytes == plain.pos_bytes && plain.gap_sums.bytes == 0 && plain.ins_out.bytes == 0 && plain.gap_count.bytes == 0
          && plain.gap_bytes.bytes == 0);
    const size_t span = 2 * band, P1 = (size_t)(P ? P : 1), R1 = (size_t)(R ? R : 1);
    const S s(P, (size_t)R, tiles, place, pileup, (int)span);
    CHECK(s.work.off == old.work.off && s.work.bytes == old.work.bytes && s.pile_sums.off == old.pile_sums.off && s.pile_sums.bytes == old.pile_sums.bytes);
    CHECK(s.pile_out.off == old.pile_out.off && s.depth.off == old.depth.off && s.consensus.off == old.consensus.off && s.spare.off == old.spare.off);
    CHECK(s.gap_sums.off == old.sums_bytes && s.gap_sums.bytes == 4 * R1 * 8 && s.sums_bytes == old.sums_bytes + 4 * R1 * 8 && s.gap_sums.off % 8 == 0);
    const size_t at = (old.pos_bytes + 15) / 16 * 16;
    CHECK(s.ins_out.off == at && s.ins_out.bytes == P1 * span * 16 && s.ins_out.off % 16 == 0);
    CHECK(s.gap_count.off == at + P1 * span * 16 && s.gap_count.bytes == P1);
    CHECK(s.gap_bytes.off == s.gap_count.off + P1 && s.gap_bytes.bytes == P1 * (1 + span));
    CHECK(s.pos_bytes == s.gap_bytes.off + s.gap_bytes.bytes);
}

int main()
{
    const uint64_t positions[] = {0, 1, 15, 16, 17, 1000, 16569, (1ull << 31) - 2}, records[] = {0, 1, 8, 1000};
    unsigned long long cases = 0;
    for (uint64_t p : positions)
        for (uint64_t r : records)
            for (uint32_t b : {0u, 1u, 8u, 31u})
                for (pileup = 0; pileup < 2; pileup++)
                    for (gapped = 0; gapped < 2; gapped++)
                        for (place = 0; place < 2; place++) { P = p; R = r; band = b; check_layout(); check_scratch(); cases++; }
    // the sizes the header states: 512 bytes a position at band 8, 8.4 MB for a bait of 16 569 positions
    if (mf::PlaceLayout(16569, 1, true, true, 1000, true, 8, true).n_ins * 8 != 16569ull * 512) { fprintf(stderr, "the band-8 size\n"); return 1; }
    printf("gapped layout ok: %llu cases\n", cases);
    return 0;
}
