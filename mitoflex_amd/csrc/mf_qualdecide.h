// The quality filter's rules (filter/filter_bin/src/main.rs:214-321) as plain functions over records and counts: no thread, channel, timer
// or device.  run_qualfilter_pipeline's decision thread is a sequence of calls to these; tests/test_qualdecide.py calls them directly.
#pragma once
#include "mf_pipeline.h"

namespace mf {
// The cut (main.rs:222-233, 291-299) of records [lo, hi) of one or two mates, up to the first record at which the reference would panic:
// a line that is not valid UTF-8, or `drain(..start)` past the end of a string.  Returns that record's index (it and the records
// behind it are left as they were), or hi.
inline uint64_t qual_check_cut(FqRec *const mrec[2], int nm, uint64_t lo, uint64_t hi, const QualParams &P)
{
    const uint64_t L = P.end - P.start;
    for (uint64_t i = lo; i < hi; i++) {
        bool bad = false;
        for (int m = 0; m < nm && !bad; m++) {
            const FqRec &r = mrec[m][i];
            // header, sequence and quality are unwrapped (main.rs:214-216, 287-289) and panic on invalid UTF-8; the
            // '+' line is bound to `_` and never unwrapped: lines() yields an Err for it and carries on
            bad = !utf8_valid(r.h, r.hl) || !utf8_valid(r.s, r.sl) || !utf8_valid(r.q, r.ql);
        }
        if (!bad && P.start) {
            for (int m = 0; m < nm; m++) bad = bad || P.start > mrec[m][i].sl;      // seq1, seq2 first
            for (int m = 0; m < nm; m++) bad = bad || P.start > mrec[m][i].ql;      // then qua1, qua2
        }
        if (bad) return i;
        for (int m = 0; m < nm; m++) {
            FqRec &r = mrec[m][i];
            if (P.start) { r.s += P.start; r.sl -= (uint32_t)P.start; r.q += P.start; r.ql -= (uint32_t)P.start; }
            if (P.end) { if (r.sl > L) r.sl = (uint32_t)L; if (r.ql > L) r.ql = (uint32_t)L; }
        }
    }
    return hi;
}

// What does not depend on other records: too many N (main.rs:236, 302), too many low qualities.  n_count / bad_count: of mate 1 and,
// for pairs, mate 2; r1: mate 1's record after the cut.  PE: both mates against a cutoff from seq1's length (main.rs:239-243);
// SE: from the quality string's (:305).
inline bool qual_drop(int nm, const FqRec &r1, const uint32_t n_count[2], const uint32_t bad_count[2], uint64_t ns, float limit)
{
    if (n_count[0] > ns || (nm == 2 && n_count[1] > ns)) return true;
    const float cf = (float)(nm == 2 ? r1.sl : r1.ql) * limit;      // `(len as f32 * limit) as usize`: the product in f32, the conversion saturating, NaN -> 0
    const uint64_t cutoff = !(cf > 0.0f) ? 0 : (cf >= 18446744073709551616.0f ? ~0ull : (uint64_t)cf);
    return bad_count[0] >= cutoff || (nm == 2 && bad_count[1] >= cutoff);
}

// The take (main.rs:254-259) over a batch's n checked records: a record that is alive (null: all are) and no duplicate (null: none is)
// adds mate 1's sequence length to the budget when there is one (trim != 0) and is kept -- unless it overflows the budget: the
// reference stops there, and that record is not kept.
struct QualTake { uint64_t kept = 0; bool stop = false; };
inline QualTake qual_take(const uint8_t *alive, const uint8_t *dup, const FqRec *mate1, uint64_t n, uint64_t trim, uint64_t &budget, uint8_t *keep)
{
    QualTake t;
    for (uint64_t i = 0; i < n; i++) {
        if ((alive && !alive[i]) || (dup && dup[i])) continue;
        if (trim) { budget += mate1[i].sl; if (budget > trim) { t.stop = true; break; } }
        keep[i] = 1; t.kept++;
    }
    return t;
}

} // namespace mf
