// The quality filter's host pipeline (readers, MateZip, the decision thread, the writers) as one program, linked with
// tests/native/qualfilter_stub.cpp -- which stands in for the GPU counting and hashing -- and the four host sources, so that
// it runs under sanitizers and without a GPU.  MF_BATCH_READS sets the batch size.
//   qualpipe_check FQ1|- FQ2|- OUT1 OUT2|- START END NS QUALITY LIMIT DEDUP TRIM TRUNCATE     ("-": stdin, single end, stdout)
// prints "kept total panicked", or "error CODE: text", on standard error (standard output may be the second output file)
#include "../../include/mitofilter.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv)
{
    if (argc < 13) return 2;
    auto path = [&](int i) { return strcmp(argv[i], "-") ? argv[i] : nullptr; };
    uint64_t kept = 0, total = 0; int panicked = 0;
    const int rc = mf_qualfilter_files(path(1), path(2), path(3), path(4), strtoull(argv[5], nullptr, 10), strtoull(argv[6], nullptr, 10),
                                       strtoull(argv[7], nullptr, 10), (uint32_t)atoi(argv[8]), strtof(argv[9], nullptr), atoi(argv[10]),
                                       strtoull(argv[11], nullptr, 10), atoi(argv[12]), 0, &kept, &total, &panicked);
    if (rc) { fprintf(stderr, "error %d: %s\n", rc, mf_last_error()); return 1; }
    fprintf(stderr, "%llu %llu %d\n", (unsigned long long)kept, (unsigned long long)total, panicked);
    return 0;
}
