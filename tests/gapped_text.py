"""The two text formats of `fastfilter bait --band W --gapped-consensus / --insertions` restated in Python from their description
(README, mf_report_text.h).  tests/test_gapped_abi.py holds the C++ writers to them without a device, tests/test_gpu_gapped.py the files
the CLI writes."""


def gapped_fasta(names, gapped_starts, gapped, width=60):
    """FASTA under the records' names, 60 letters a line; an empty record has a header and no sequence line"""
    out = []
    for j, name in enumerate(names):
        seq = bytes(gapped[int(gapped_starts[j]):int(gapped_starts[j + 1])]).decode("ascii")
        out.append(">%s\n" % name)
        out.extend(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
    return "".join(out)


def insertions_text(names, starts, depth, ins_pile):
    """ins_pile: [positions][span][A, C, G, T]; a row for every (position, offset) with a count that is not zero"""
    out = ["name\tpos\toffset\tdepth\tA\tC\tG\tT\n"]
    for j, name in enumerate(names):
        for p in range(int(starts[j]), int(starts[j + 1])):
            for q, row in enumerate(ins_pile[p]):
                a, c, g, t = (int(v) for v in row)
                if a or c or g or t:
                    out.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, p - int(starts[j]) + 1, q, int(depth[p]), a, c, g, t))
    return "".join(out)
