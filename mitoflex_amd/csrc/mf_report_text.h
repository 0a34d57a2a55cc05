// The text of the report files `fastfilter bait` writes: one pure function per format, from the arrays of the file-level calls
// (include/mitofilter.h) to an open FILE.  names: the records' (or groups') names; starts: names.size() + 1 offsets, record j holds
// positions [starts[j], starts[j + 1]) of the per-position arrays.  Each returns false when f is null or a write failed.  Host code with no
// dependency beyond the C ABI header, so that tests/native/report_text_check.cpp holds every format to its bytes without a device.
#pragma once
#include "../../include/mitofilter.h"

#include <cstdio>
#include <string>
#include <vector>

namespace mf_text {

using Names = std::vector<std::string>;
using Starts = std::vector<uint64_t>;
typedef unsigned long long ull;

inline bool written(FILE *f) { return fflush(f) == 0 && !ferror(f); }
inline ull pile_depth(const mf_pileup_t &c) { return (ull)c.a + c.c + c.g + c.t; }

// --report / --group-report: counts holds names.size() + 2 entries, the last two the ambiguous and the unassigned reads
inline bool write_reads(FILE *f, bool grouped, const Names &names, const uint64_t *counts)
{
    if (!f) return false;
    const size_t n = names.size();
    fputs(grouped ? "group\tname\treads\n" : "record\tname\treads\n", f);
    for (size_t i = 0; i < n; i++) fprintf(f, "%zu\t%s\t%llu\n", i, names[i].c_str(), (ull)counts[i]);
    fprintf(f, "-\t*ambiguous*\t%llu\n-\t*unassigned*\t%llu\n", (ull)counts[n], (ull)counts[n + 1]);
    return written(f);
}

// --depth-report
inline bool write_depth_report(FILE *f, const Names &names, const Starts &starts, const mf_depth_record_t *recs)
{
    if (!f) return false;
    fputs("record\tname\tlength\twindows\tcovered\tmean\tmax\n", f);
    for (size_t i = 0; i < names.size(); i++) {
        const mf_depth_record_t &d = recs[i];
        fprintf(f, "%zu\t%s\t%llu\t%llu\t%llu\t%.3f\t%llu\n", i, names[i].c_str(), (ull)(starts[i + 1] - starts[i]), (ull)d.windows, (ull)d.covered,
                d.windows ? (double)d.depth_sum / (double)d.windows : 0.0, (ull)d.depth_max);
    }
    return written(f);
}

// name, 1-based position, depth of every position (skip_none: but those whose depth is MF_DEPTH_NONE)
inline bool write_positions(FILE *f, const Names &names, const Starts &starts, const uint32_t *depth, bool skip_none)
{
    if (!f) return false;
    for (size_t i = 0; i < names.size(); i++)
        for (uint64_t p = starts[i]; p < starts[i + 1]; p++)
            if (!skip_none || depth[p] != MF_DEPTH_NONE) fprintf(f, "%s\t%llu\t%u\n", names[i].c_str(), (ull)(p - starts[i] + 1), depth[p]);
    return written(f);
}
// --depth-profile: the valid windows; --base-depth: every position
inline bool write_depth_profile(FILE *f, const Names &names, const Starts &starts, const uint32_t *profile) { return write_positions(f, names, starts, profile, true); }
inline bool write_base_depth(FILE *f, const Names &names, const Starts &starts, const uint32_t *depth) { return write_positions(f, names, starts, depth, false); }

// --place-report: the max column is taken over the record's base depth; not_placed: the passing mates that are not placed
inline bool write_place_report(FILE *f, const Names &names, const Starts &starts, const mf_place_record_t *recs, const uint32_t *base_depth, uint64_t not_placed)
{
    if (!f) return false;
    fputs("record\tname\tlength\tforward\treverse\tover_begin\tover_end\tcovered\tmean\tmax\n", f);
    for (size_t i = 0; i < names.size(); i++) {
        const mf_place_record_t &d = recs[i];
        const uint64_t len = starts[i + 1] - starts[i];
        uint32_t mx = 0;
        for (uint64_t p = starts[i]; p < starts[i + 1]; p++) if (base_depth[p] > mx) mx = base_depth[p];
        fprintf(f, "%zu\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.3f\t%u\n", i, names[i].c_str(), (ull)len, (ull)d.forward, (ull)d.reverse, (ull)d.over_begin,
                (ull)d.over_end, (ull)d.covered, len ? (double)d.base_sum / (double)len : 0.0, mx);
    }
    fprintf(f, "-\t*unplaced*\t%llu\n", (ull)not_placed);
    return written(f);
}

// --pileup: name, 1-based position, bait letter, depth = A + C + G + T, A, C, G, T
inline bool write_pileup(FILE *f, const Names &names, const Starts &starts, const uint8_t *letters, const mf_pileup_t *pile)
{
    if (!f) return false;
    for (size_t i = 0; i < names.size(); i++)
        for (uint64_t p = starts[i]; p < starts[i + 1]; p++) {
            const mf_pileup_t &c = pile[p];
            fprintf(f, "%s\t%llu\t%c\t%llu\t%u\t%u\t%u\t%u\n", names[i].c_str(), (ull)(p - starts[i] + 1), (char)letters[p], pile_depth(c), c.a, c.c, c.g, c.t);
        }
    return written(f);
}

// --consensus: FASTA, 60 letters a line; an empty record has a header and no sequence line
inline bool write_consensus(FILE *f, const Names &names, const Starts &starts, const uint8_t *consensus)
{
    if (!f) return false;
    for (size_t i = 0; i < names.size(); i++) {
        fprintf(f, ">%s\n", names[i].c_str());
        for (uint64_t p = starts[i]; p < starts[i + 1]; p += 60) {
            const uint64_t left = starts[i + 1] - p;
            fwrite(consensus + p, 1, (size_t)(left < 60 ? left : 60), f);
            fputc('\n', f);
        }
    }
    return written(f);
}

// --variants: the called positions (an upper-case letter) whose bait letter is valid and differs: name, 1-based position, ref, alt, depth, alt count
inline bool write_variants(FILE *f, const Names &names, const Starts &starts, const uint8_t *letters, const mf_pileup_t *pile, const uint8_t *consensus)
{
    if (!f) return false;
    for (size_t i = 0; i < names.size(); i++)
        for (uint64_t p = starts[i]; p < starts[i + 1]; p++) {
            const uint8_t alt = consensus[p], ref = letters[p];
            if (!(alt == 'A' || alt == 'C' || alt == 'G' || alt == 'T') || ref == 'N' || alt == ref) continue;
            const mf_pileup_t &c = pile[p];
            fprintf(f, "%s\t%llu\t%c\t%c\t%llu\t%u\n", names[i].c_str(), (ull)(p - starts[i] + 1), (char)ref, (char)alt, pile_depth(c),
                    alt == 'A' ? c.a : alt == 'C' ? c.c : alt == 'G' ? c.g : c.t);
        }
    return written(f);
}

// --score-report: per record the placed reads on either side of the cut, the compared and mismatching bases of the accepted ones, their
// mismatches per thousand compared bases (0.000 when nothing was compared), then the MF_SCORE_BINS bins of min(mismatches, 31) over ALL
// placed reads
inline bool write_score_report(FILE *f, const Names &names, const Starts &starts, const mf_score_record_t *recs)
{
    if (!f) return false;
    fputs("record\tname\tlength\taccepted\trejected\tcompared\tmismatches\tpermille", f);
    for (int b = 0; b < MF_SCORE_BINS; b++) fprintf(f, b == MF_SCORE_BINS - 1 ? "\tmm%d+" : "\tmm%d", b);
    fputc('\n', f);
    for (size_t i = 0; i < names.size(); i++) {
        const mf_score_record_t &d = recs[i];
        fprintf(f, "%zu\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%.3f", i, names[i].c_str(), (ull)(starts[i + 1] - starts[i]), (ull)d.accepted, (ull)d.rejected,
                (ull)d.compared, (ull)d.mismatches, d.compared ? 1000.0 * (double)d.mismatches / (double)d.compared : 0.0);
        for (int b = 0; b < MF_SCORE_BINS; b++) fprintf(f, "\t%llu", (ull)d.hist[b]);
        fputc('\n', f);
    }
    return written(f);
}

// --score-report with --band: the same behind a banded alignment -- insertions, deletions and gapped behind mismatches, edits (mismatches
// + insertions + deletions) per thousand alignment columns (compared + insertions + deletions), the bins of min(edits, 31)
inline bool write_align_report(FILE *f, const Names &names, const Starts &starts, const mf_align_record_t *recs)
{
    if (!f) return false;
    fputs("record\tname\tlength\taccepted\trejected\tcompared\tmismatches\tinsertions\tdeletions\tgapped\tpermille", f);
    for (int b = 0; b < MF_SCORE_BINS; b++) fprintf(f, b == MF_SCORE_BINS - 1 ? "\ted%d+" : "\ted%d", b);
    fputc('\n', f);
    for (size_t i = 0; i < names.size(); i++) {
        const mf_align_record_t &d = recs[i];
        const uint64_t gaps = d.insertions + d.deletions, columns = d.compared + gaps;
        fprintf(f, "%zu\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.3f", i, names[i].c_str(), (ull)(starts[i + 1] - starts[i]), (ull)d.accepted, (ull)d.rejected,
                (ull)d.compared, (ull)d.mismatches, (ull)d.insertions, (ull)d.deletions, (ull)d.gapped, columns ? 1000.0 * (double)(d.mismatches + gaps) / (double)columns : 0.0);
        for (int b = 0; b < MF_SCORE_BINS; b++) fprintf(f, "\t%llu", (ull)d.hist[b]);
        fputc('\n', f);
    }
    return written(f);
}

// --indels: name, 1-based position, base depth, del, ins, ins_bases of the positions where any of the three is not zero (an insertion lies
// behind its position)
inline bool write_indels(FILE *f, const Names &names, const Starts &starts, const uint32_t *base_depth, const mf_indel_t *indels)
{
    if (!f) return false;
    fputs("name\tpos\tdepth\tdel\tins\tins_bases\n", f);
    for (size_t i = 0; i < names.size(); i++)
        for (uint64_t p = starts[i]; p < starts[i + 1]; p++)
            if (indels[p].del || indels[p].ins || indels[p].ins_bases)
                fprintf(f, "%s\t%llu\t%u\t%u\t%u\t%u\n", names[i].c_str(), (ull)(p - starts[i] + 1), base_depth[p], indels[p].del, indels[p].ins, indels[p].ins_bases);
    return written(f);
}

// --gapped-consensus: FASTA like --consensus, the records cut out of the gapped consensus by its own R + 1 offsets
inline bool write_gapped_consensus(FILE *f, const Names &names, const uint64_t *gapped_starts, const uint8_t *gapped)
{
    return write_consensus(f, names, Starts(gapped_starts, gapped_starts + names.size() + 1), gapped);
}

// --insertions: name, 1-based position, 0-based offset inside the insertion behind it, base depth, A, C, G, T of every (position, offset)
// of the insertion pile (span entries a position) with a count that is not zero
inline bool write_insertions(FILE *f, const Names &names, const Starts &starts, const uint32_t *base_depth, const mf_pileup_t *ins_pile, uint32_t span)
{
    if (!f) return false;
    fputs("name\tpos\toffset\tdepth\tA\tC\tG\tT\n", f);
    for (size_t i = 0; i < names.size(); i++)
        for (uint64_t p = starts[i]; p < starts[i + 1]; p++)
            for (uint32_t q = 0; q < span; q++) {
                const mf_pileup_t &c = ins_pile[p * span + q];
                if (c.a || c.c || c.g || c.t)
                    fprintf(f, "%s\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\n", names[i].c_str(), (ull)(p - starts[i] + 1), q, base_depth[p], c.a, c.c, c.g, c.t);
            }
    return written(f);
}

// --extension-report: name, end (begin or end), 1-based distance from the record, depth (the bases of the column), A, C, G, T of every
// (record, end, offset) of the extension pile (extend entries an end, begin then end of every record) with a count that is not zero
inline bool write_extension_report(FILE *f, const Names &names, const mf_pileup_t *ext_pile, uint32_t extend)
{
    if (!f) return false;
    fputs("name\tend\toffset\tdepth\tA\tC\tG\tT\n", f);
    for (size_t i = 0; i < names.size(); i++)
        for (uint32_t side = 0; side < 2; side++)
            for (uint32_t e = 0; e < extend; e++) {
                const mf_pileup_t &c = ext_pile[(2 * i + side) * (size_t)extend + e];
                if (c.a || c.c || c.g || c.t)
                    fprintf(f, "%s\t%s\t%u\t%llu\t%u\t%u\t%u\t%u\n", names[i].c_str(), side ? "end" : "begin", e + 1, (ull)c.a + c.c + c.g + c.t, c.a, c.c, c.g, c.t);
            }
    return written(f);
}

// --pair-report (`fastfilter pairs`): per record the pairs by kind (include/mitofilter.h, pairs) and the mean insert of the proper and
// the rescued ones (0.000 when there are none), then a last line for the pairs without a settled mate
inline bool write_pair_report(FILE *f, const Names &names, const Starts &starts, const mf_pair_record_t *recs, uint64_t pairs_none)
{
    if (!f) return false;
    fputs("record\tname\tlength\tproper\tdiscordant\tcross\trescued\tsingle\tmean_insert\n", f);
    for (size_t i = 0; i < names.size(); i++) {
        const mf_pair_record_t &d = recs[i];
        const uint64_t with_insert = d.proper + d.rescued;
        fprintf(f, "%zu\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.3f\n", i, names[i].c_str(), (ull)(starts[i + 1] - starts[i]), (ull)d.proper, (ull)d.discordant,
                (ull)d.cross, (ull)d.rescued, (ull)d.single, with_insert ? (double)d.insert_sum / (double)with_insert : 0.0);
    }
    fprintf(f, "-\t*none*\t%llu\n", (ull)pairs_none);
    return written(f);
}

} // namespace mf_text
