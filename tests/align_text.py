"""The two text formats of `fastfilter bait --band W` restated in Python from their description (README, mf_report_text.h): the score
report behind a banded alignment and the indel table.  tests/test_align_abi.py holds the C++ writers to them without a device,
tests/test_gpu_align.py the files the CLI writes."""
BINS = 32


def align_report_text(names, starts, recs):
    """recs: rows of accepted, rejected, compared, mismatches, insertions, deletions, gapped and BINS bins"""
    out = ["record\tname\tlength\taccepted\trejected\tcompared\tmismatches\tinsertions\tdeletions\tgapped\tpermille\t"
           + "\t".join("ed%d" % b + ("+" if b == BINS - 1 else "") for b in range(BINS)) + "\n"]
    for j, (name, row) in enumerate(zip(names, recs)):
        row = [int(v) for v in row]
        acc, rej, cmpd, mm, ni, nd, gapped = row[:7]
        columns = cmpd + ni + nd
        permille = 1000.0 * (mm + ni + nd) / columns if columns else 0.0
        out.append("\t".join([str(j), name, str(int(starts[j + 1]) - int(starts[j]))] + [str(v) for v in row[:7]] + ["%.3f" % permille]
                             + [str(v) for v in row[7:7 + BINS]]) + "\n")
    return "".join(out)


def indels_text(names, starts, depth, indels):
    """indels: rows of del, ins, ins_bases a position"""
    out = ["name\tpos\tdepth\tdel\tins\tins_bases\n"]
    for j, name in enumerate(names):
        for p in range(int(starts[j]), int(starts[j + 1])):
            d, i, b = (int(v) for v in indels[p])
            if d or i or b:
                out.append("%s\t%d\t%d\t%d\t%d\t%d\n" % (name, p - int(starts[j]) + 1, int(depth[p]), d, i, b))
    return "".join(out)
