"""The two text formats of `fastfilter bait --band W --extend E --extended-consensus / --extension-report` restated in Python from
their description (README, mf_report_text.h).  tests/test_extend_text.py holds the C++ writers to them without a device,
tests/test_gpu_extend.py the files the CLI writes."""


def extended_fasta(names, extended_starts, extended, width=60):
    """FASTA under the records' names, 60 letters a line; an empty record has a header and no sequence line"""
    out = []
    for j, name in enumerate(names):
        seq = bytes(extended[int(extended_starts[j]):int(extended_starts[j + 1])]).decode("ascii")
        out.append(">%s\n" % name)
        out.extend(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
    return "".join(out)


def extension_text(names, ext_pile):
    """ext_pile: [R][begin, end][E][A, C, G, T]; a row for every (record, end, offset) with a count that is not zero: the name, begin or
    end, the 1-based distance from the record, the bases of the column, and the four counts"""
    out = ["name\tend\toffset\tdepth\tA\tC\tG\tT\n"]
    for j, name in enumerate(names):
        for side, word in enumerate(("begin", "end")):
            for e, row in enumerate(ext_pile[j][side]):
                a, c, g, t = (int(v) for v in row)
                if a or c or g or t:
                    out.append("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, word, e + 1, a + c + g + t, a, c, g, t))
    return "".join(out)
