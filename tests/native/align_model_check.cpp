// The banded alignment's rule (mitoflex_amd/csrc/mf_align.h) on the CPU, against cases that the plain-Python oracle
// (tests/align_oracle.py) dumps.  Built by tests/test_align_model.py, once plain and once with -fsanitize=address,undefined: the bait's
// packed letters and validity bits are exactly-sized heap arrays, so an address formed for a coordinate outside the record's words stops
// the program.
//
// Two models, both over the shared header's pieces (align_sub, align_move, align_end_key, align_accepts):
//   scalar   the full table of the band's cells, cell by cell, and the traceback over it;
//   lanes    what the kernel does: 64 lanes, one diagonal each; per row t = min(prev + sub, the lane above's + 1), an inclusive prefix
//            minimum of t + (63 - lane) in log2 steps up to the band's width, two direction bits a cell packed 32 rows to a word
//            [row block][lane]; the traceback a row block at a time leaving one word a read base (column, inserted, deleted behind it);
//            counts and the per-position adds from those words.
// Each must give the oracle's compared, mismatches, insertions, deletions, ref_begin, ref_end, deleted positions and insertion runs.
//
// A case is one line:  W start x rec compared mismatches insertions deletions ref_begin ref_end  n_del p ..  n_runs c n ..
// Prints "align model ok: <cases> cases" and exits 0, or the first difference and exits 1.
#include "../../mitoflex_amd/csrc/mf_align.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace mf;

struct Words {
    uint32_t *w; size_t n;
    explicit Words(size_t n_) : w((uint32_t *)calloc(n_ ? n_ : 1, 4)), n(n_) {}
    ~Words() { free(w); }
    Words(const Words &) = delete;
};

struct Result {
    long long compared = 0, mismatches = 0, insertions = 0, deletions = 0, ref_begin = 0, ref_end = 0;
    std::vector<long long> deleted;                       // record coordinates, ascending
    std::map<long long, long long> runs, run_bases;       // insertion runs that begin at column c; their bases
    bool operator==(const Result &o) const
    {
        return compared == o.compared && mismatches == o.mismatches && insertions == o.insertions && deletions == o.deletions && ref_begin == o.ref_begin
               && ref_end == o.ref_end && deleted == o.deleted && runs == o.runs && run_bases == o.run_bases;
    }
    void print(const char *name) const
    {
        printf("  %s: %lld %lld %lld %lld %lld %lld del", name, compared, mismatches, insertions, deletions, ref_begin, ref_end);
        for (long long p : deleted) printf(" %lld", p);
        printf(" runs");
        for (auto &kv : runs) printf(" %lld x%lld (%lld)", kv.first, kv.second, run_bases.at(kv.first));
        printf("\n");
    }
};

struct Problem {
    int W; int64_t start, len; uint64_t s0; std::vector<uint32_t> x; const ScoreBait *B;
    uint64_t L() const { return x.size(); }
};

static Result scalar_model(const Problem &P)
{
    const int W = P.W, n = 2 * W + 1;
    const uint64_t L = P.L();
    const uint32_t INF = 0xFFFFFFFFu;
    std::vector<uint32_t> D((L + 1) * n, 0);
    auto at = [&](uint64_t i, int d) -> uint32_t { return d < -W || d > W ? INF : D[i * n + (d + W)]; };
    auto plus = [&](uint32_t v, uint32_t c) { return v == INF ? INF : v + c; };
    bool cmp;
    for (uint64_t i = 1; i <= L; i++)
        for (int d = -W; d <= W; d++) {
            const int64_t c = P.start + (int64_t)i + d;
            const uint32_t diag = at(i - 1, d) + align_sub(P.x[i - 1], c - 1, P.len, *P.B, P.s0, cmp);
            D[i * n + (d + W)] = std::min(diag, std::min(plus(at(i - 1, d + 1), 1), plus(at(i, d - 1), 1)));
        }
    uint64_t best = ~0ull;
    for (int d = -W; d <= W; d++) best = std::min(best, align_end_key(at(L, d), d));
    int d = align_end_diagonal(best);
    Result r;
    r.ref_end = P.start + (int64_t)L + d;
    uint64_t i = L;
    long long run_col = 0; bool in_run = false;           // walking backwards: a run ends where the move before it is no insertion at its column
    while (i > 0) {
        const int64_t c = P.start + (int64_t)i + d;
        const uint32_t s = align_sub(P.x[i - 1], c - 1, P.len, *P.B, P.s0, cmp);
        const uint32_t mv = align_move(at(i, d), at(i - 1, d) + s, d > -W, at(i, d - 1));
        if (mv == ALIGN_DIAG) { r.compared += cmp; r.mismatches += s; i--; in_run = false; }
        else if (mv == ALIGN_DEL) { r.deletions++; if (c - 1 >= 0 && c - 1 < P.len) r.deleted.push_back(c - 1); d--; in_run = false; }
        else {
            r.insertions++;
            if (c - 1 >= 0 && c - 1 < P.len) {
                if (!(in_run && run_col == c)) r.runs[c]++;
                r.run_bases[c]++;
            }
            in_run = true; run_col = c;
            i--; d++;
        }
    }
    r.ref_begin = P.start + d;
    std::sort(r.deleted.begin(), r.deleted.end());
    return r;
}

// ---- the kernel's formulation, lane by lane
static const int LANES = 64;
template <class T> static std::vector<T> shfl_up(const std::vector<T> &v, int o) { std::vector<T> r(v); for (int l = o; l < LANES; l++) r[l] = v[l - o]; return r; }
template <class T> static std::vector<T> shfl_down(const std::vector<T> &v, int o) { std::vector<T> r(v); for (int l = 0; l + o < LANES; l++) r[l] = v[l + o]; return r; }

static Result lane_model(const Problem &P)
{
    const int W = P.W;
    const uint64_t L = P.L();
    std::vector<unsigned long long> dirs(64 * ((L + 31) / 32)), ent(L);
    std::vector<uint32_t> prev(LANES, 0);
    std::vector<unsigned long long> bits(LANES, 0);
    bool cmp;
    for (uint64_t i = 1; i <= L; i++) {
        const uint64_t b = i - 1;
        const uint32_t x = P.x[b];
        const std::vector<uint32_t> up = shfl_down(prev, 1);
        std::vector<uint32_t> diag(LANES), key(LANES), D(LANES);
        for (int lane = 0; lane < LANES; lane++) {
            const int d = lane - W;
            diag[lane] = prev[lane] + (lane <= 2 * W ? align_sub(x, P.start + (int64_t)b + d, P.len, *P.B, P.s0, cmp) : 0u);
            uint32_t t = diag[lane];
            if (lane < 2 * W && up[lane] + 1u < t) t = up[lane] + 1u;
            key[lane] = t + (uint32_t)(63 - lane);
        }
        for (int o = 1; o <= 2 * W; o <<= 1) {
            const std::vector<uint32_t> v = shfl_up(key, o);
            for (int lane = 0; lane < LANES; lane++) if (lane >= o && v[lane] < key[lane]) key[lane] = v[lane];
        }
        for (int lane = 0; lane < LANES; lane++) D[lane] = key[lane] - (uint32_t)(63 - lane);
        const std::vector<uint32_t> left = shfl_up(D, 1);
        for (int lane = 0; lane < LANES; lane++) {
            bits[lane] |= (unsigned long long)align_move(D[lane], diag[lane], lane > 0, left[lane]) << (2 * ((uint32_t)b & 31u));
            if (((uint32_t)b & 31u) == 31u || i == L) { dirs.at((b >> 5) * 64 + lane) = bits[lane]; bits[lane] = 0; }
        }
        prev = D;
    }
    uint64_t best = ~0ull;
    for (int lane = 0; lane <= 2 * W; lane++) best = std::min(best, align_end_key(prev[lane], lane - W));
    int dd = align_end_diagonal(best);
    Result r;
    r.ref_end = P.start + (int64_t)L + dd;
    uint64_t i = L;
    uint32_t pend = 0;
    for (uint64_t blk = (L - 1) >> 5;; blk--) {
        while (i > blk * 32) {
            const uint32_t bi = (uint32_t)(i - 1) & 31u;
            const uint32_t mv = (uint32_t)(dirs.at(blk * 64 + (dd + W)) >> (2 * bi)) & 3u;
            if (mv == ALIGN_DEL && dd > -W) { r.deletions++; pend++; dd--; continue; }
            const bool ins = mv == ALIGN_INS && dd < W;
            ent.at(blk * 32 + bi) = ((unsigned long long)pend << 33) | ((unsigned long long)ins << 32) | (uint32_t)(int32_t)(P.start + (int64_t)i + dd);
            pend = 0;
            if (ins) { r.insertions++; dd++; }
            i--;
        }
        if (blk == 0) break;
    }
    r.ref_begin = P.start + dd;
    for (uint64_t b = 0; b < L; b++) {                      // the counts and the adds, a read base at a time as the lanes take them
        const unsigned long long e = ent[b];
        const int64_t c = (int64_t)(int32_t)(uint32_t)e;
        for (uint32_t q = 0; q < (uint32_t)(e >> 33); q++) if (c + q >= 0 && c + q < P.len) r.deleted.push_back(c + q);
        if (!((e >> 32) & 1u)) { const uint32_t s = align_sub(P.x[b], c - 1, P.len, *P.B, P.s0, cmp); r.compared += cmp; r.mismatches += s; continue; }
        if (c - 1 < 0 || c - 1 >= P.len) continue;
        r.run_bases[c]++;
        if (!(b > 0 && (ent[b - 1] >> 32) == 1ull)) r.runs[c]++;
    }
    std::sort(r.deleted.begin(), r.deleted.end());
    return r;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: align_model_check CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    unsigned long long cases = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ss(line);
        int W; long long start; std::string x, rec;
        Result want;
        size_t n_del, n_runs;
        ss >> W >> start >> x >> rec >> want.compared >> want.mismatches >> want.insertions >> want.deletions >> want.ref_begin >> want.ref_end >> n_del;
        for (size_t q = 0; q < n_del; q++) { long long p; ss >> p; want.deleted.push_back(p); }
        ss >> n_runs;
        for (size_t q = 0; q < n_runs; q++) { long long c, n; ss >> c >> n; want.runs[c]++; want.run_bases[c] += n; }
        if (!ss) { printf("case %llu: cannot be read\n", cases); return 1; }
        std::sort(want.deleted.begin(), want.deleted.end());
        // the record as the LAST one of a set, behind 37 positions of another: exactly the words that hold them, padded by one
        const uint64_t s0 = 37, total = s0 + rec.size();
        Words bw((total + 15) / 16 + 1), bv((total + 31) / 32 + 1);
        for (uint64_t p = 0; p < total; p++) {
            const char ch = p < s0 ? "ACGT"[p & 3] : rec[p - s0];
            const char *f = ch == 'N' ? nullptr : strchr("ACGT", ch);
            if (f) { bw.w[p >> 4] |= (uint32_t)(f - "ACGT") << (2 * (p & 15)); bv.w[p >> 5] |= 1u << (p & 31); }
        }
        const ScoreBait SB{bw.w, bw.n - 1, bv.w, bv.n - 1};
        Problem P{W, start, (int64_t)rec.size(), s0, {}, &SB};
        for (char ch : x) { const char *f = ch == 'N' ? nullptr : strchr("ACGT", ch); P.x.push_back(f ? (uint32_t)(f - "ACGT") : ALIGN_X_NONE); }
        if (!align_band_ok((uint32_t)W, W + 1) || align_band_ok(32, 64) || align_band_ok((uint32_t)W, W)) { printf("the band check\n"); return 1; }
        const Result a = scalar_model(P), b = lane_model(P);
        cases++;
        if (!(a == want) || !(b == want)) {
            printf("DIFFERS: case %llu (W %d start %lld L %zu len %zu)\n", cases, W, start, x.size(), rec.size());
            want.print("oracle"); a.print("scalar"); b.print("lanes ");
            return 1;
        }
        const uint32_t c = (uint32_t)want.compared, m = (uint32_t)want.mismatches, ni = (uint32_t)want.insertions, nd = (uint32_t)want.deletions;
        if (!align_accepts(c, m, ni, nd, 1000) || align_accepts(c, m, ni, nd, 0) != (m + ni + nd == 0)
            || align_accepts(c, m, ni, nd, 60) != ((unsigned long long)(m + ni + nd) * 1000 <= 60ull * (c + ni + nd))) { printf("DIFFERS: the cut\n"); return 1; }
    }
    printf("align model ok: %llu cases\n", cases);
    return 0;
}
