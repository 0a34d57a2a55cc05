/* libmitofilter_hip.so -- C ABI of the MI355X-native MitoFlex read pre-filter.
 *
 * What this boundary replaces.  The reference has NO FFI on this path: its
 * only interface is the subprocess CLI `assemble/fastfilter` invoked through
 * `shell_call` (assemble/assemble_wrapper.py:317-345, utility/helper.py:35-86).
 * That CLI contract is kept by mitoflex_amd/assemble/fastfilter (built from
 * mitoflex_amd/csrc/fastfilter_main.cpp).  The functions below are the
 * additional in-process boundary BASELINE.json's north_star asks for
 * ("libmitofilter_hip.so + ctypes wrapper"), following the export set
 * recommended in SURVEY.md section 8b.  Each entry point cites the reference
 * site whose role it takes over; where the reference has none it says so.
 *
 * Conventions: plain C, caller-allocated buffers, opaque handles created and
 * destroyed by the library, return 0 on success / negative MF_E_* on failure,
 * never throws; mf_last_error() returns a thread-local message.  Safe for
 * concurrent calls on different devices; one host thread per device.
 *
 * There is no CPU fallback in this library: every compute entry point runs
 * HIP kernels on a gfx950 device and fails with MF_E_NO_DEVICE without one.
 */
#ifndef MITOFILTER_H
#define MITOFILTER_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MF_ABI_VERSION 5

enum {
    MF_OK = 0,
    MF_E_ARG = -1,        /* bad argument */
    MF_E_IO = -2,         /* cannot open / read / write a file */
    MF_E_NOMEM = -3,
    MF_E_HIP = -4,        /* a HIP call failed; see mf_last_error() */
    MF_E_NO_DEVICE = -5,  /* no usable gfx950 device */
    MF_E_FORMAT = -6      /* malformed input */
};

/* mf_filter modes */
enum {
    MF_MODE_SCREENED = 0,   /* s-mer screen kernel + exact kernel on candidates (default) */
    MF_MODE_EXHAUSTIVE = 1  /* exact kernel on every read (no screen) */
};

/* what a mf_kmerset holds */
enum {
    MF_KIND_NUCLEOTIDE = 0, /* canonical nucleotide k-mers (the north-star path) */
    MF_KIND_PROTEIN = 1     /* peptide k-mers of a protein database; reads are translated in six frames */
};

/* pair rule for mf_filter_fastq_files */
enum { MF_PAIR_EITHER = 0, MF_PAIR_BOTH = 1 };

typedef struct mf_kmerset mf_kmerset; /* bait k-mer table (+ screen structures), replicated per device */
typedef struct mf_reads mf_reads;     /* one packed read set resident in one device's HBM */

typedef struct {
    int32_t  k;            /* k-mer length, 11..63 */
    int32_t  key_words;    /* 1 (k<=32) or 2 u64 per key */
    uint64_t slots;        /* open-address table slots (pow2) */
    uint64_t n_keys;       /* distinct canonical k-mers */
    uint64_t n_windows;    /* sum over records of max(0, len-k+1) */
    int32_t  screen_s;     /* s-mer length used by the screen, 0 = screen disabled */
    int32_t  screen_stride;/* sample stride in bases */
    uint32_t bloom_words;  /* nucleotide sets: the screen's LDS bit table in u32 words; protein sets: the key bit table in u32
                              words, staged in LDS when <= 16384 and read through L2 when larger */
    uint32_t smer_slots;   /* exact s-mer table slots */
    uint64_t n_smers;      /* distinct s-mers (both strands) */
    int32_t  kind;         /* MF_KIND_*; for MF_KIND_PROTEIN k is the peptide k-mer length (ABI 2) */
    int32_t  genetic_code; /* NCBI translation table of a protein set, else 0 (ABI 2) */
    /* ABI 5: which screen a set of this size takes (the bait-size axis) */
    uint32_t front_mode;         /* 0 LDS table only | 1 LDS table, positives looked up in front2 turn by turn | 2 every sample through
                                    front2 (+ front3), no LDS table | 3 LDS table, lone positives through front2 sixty-four at a time |
                                    4 a one-bit LDS table in front of mode 2's look-ups */
    uint32_t front2_log2_blocks; /* log2 of front2's 128-bit blocks (0: none) */
    uint32_t front3_log2_blocks; /* log2 of front3's 128-bit blocks (0: none) */
    uint32_t canonical_screen;      /* 1: the screen's tables hold one canonical key per bait s-mer (larger baits) instead of one per strand */
} mf_kmerset_info_t;

typedef struct {
    uint64_t n_reads;
    uint64_t total_bases;
    uint64_t n_invalid;    /* invalid (non-ACGT) bases */
    uint32_t uniform_len;  /* >0 when every read has this length */
    int32_t  device;
} mf_reads_info_t;

typedef struct {
    uint64_t n_reads;
    uint64_t n_pass;
    uint64_t n_candidates;   /* screened mode: reads handed to the exact kernel -- or, for threshold 1 without hit counts (the
                                finish-kernel pass), stage-1 positives that were looked up (work items, not reads) */
    float    ms_total;       /* hipEvent time per pass, first launch -> last kernel end, averaged over the passes of the call
                                (consecutive threshold-1 passes overlap: finish kernels run under the next screen kernel) */
    float    ms_screen;      /* screen kernel only (streams every packed byte once); the kernel times come from
                                events attached to the dispatches themselves (hipExtLaunchKernelGGL start/stop) */
    float    ms_mark;        /* mark kernel: finishes the screen's positives, sets candidate bits (0 in the finish-kernel pass) */
    float    ms_exact;       /* exact kernel -- or the first (run) phase of the finish kernel */
    uint64_t algorithmic_bytes; /* ceil(2*bases/8) + ceil(n_reads/8): SURVEY.md 8d byte model */
} mf_filter_stats_t;

/* ---- library ---------------------------------------------------------- */
int         mf_abi_version(void);
const char *mf_last_error(void);
/* number of visible gfx950 devices (>=0) or MF_E_HIP */
int         mf_device_count(void);
int         mf_device_name(int device, char *buf, size_t buflen);
/* hipDeviceSynchronize on `device` (bench.py's barrier bracket) */
int         mf_device_synchronize(int device);

/* ---- bait k-mer set (no reference counterpart:
 * profile/MT_database is protein, findmitoscaf/findmitoscaf.py:57) --------
 * Parses a NUCLEOTIDE FASTA on the host, then builds the canonical-k-mer
 * open-address table and the screen structures with device kernels.  The
 * table is byte-identical to the CPU oracle's (history-independent layout). */
int mf_kmerset_build_from_fasta(const char *fasta_path, int k, int device, mf_kmerset **out);
int mf_kmerset_build_from_text(const char *fasta_text, size_t len, int k, int device, mf_kmerset **out);
/* Protein-space bait set (SURVEY.md 8f "next" #4): the peptide k-mers (kp residues, 4..12; 5 bits per
 * residue, first residue least significant) of a PROTEIN FASTA such as the reference's
 * profile/MT_database/<clade>.fa, which the reference itself only hands to tblastn
 * (findmitoscaf/findmitoscaf.py:57, annotation/annotation_tookit.py:55-97 `-db_gencode`).
 * genetic_code is the NCBI translation table the reads are translated with -- the reference's
 * --genetic-code / profile/codes.json value (arguments.py:449-453): 1, 2, 3, 4, 5, 9, 11, 13, 14, 21.
 * The handle goes to the same mf_filter* entry points: every read is translated in six frames,
 * hits = number of (frame, window) pairs whose kp codons are all sense codons free of invalid
 * bases and whose peptide k-mer is in the set; `mode` is ignored (there is no screen). */
int mf_kmerset_build_protein_from_fasta(const char *protein_fasta_path, int kp, int genetic_code, int device, mf_kmerset **out);
int mf_kmerset_build_protein_from_text(const char *protein_fasta_text, size_t len, int kp, int genetic_code, int device,
                                       mf_kmerset **out);
int mf_kmerset_info(const mf_kmerset *ks, mf_kmerset_info_t *info);
/* copy the device table back: keys_out must hold slots*key_words u64 */
int mf_kmerset_export(const mf_kmerset *ks, int device, uint64_t *keys_out, size_t n_u64);
int mf_kmerset_free(mf_kmerset *ks);

/* ---- packed reads (row B1).  Layout: dense little-endian 2-bit stream,
 * base i in words[i>>4] bits [2*(i&15), +1]; invalid bases stored as 0 and
 * listed ascending in npos (global base indices); offsets has n_reads+1 base
 * offsets.  The FASTQ conventions (4-line records, CR stripped, partial tail
 * dropped, .gz by extension) are the reference's: filter/filter_bin/src/
 * main.rs:287-321, filter/filter_bin/src/helper.rs:14-31. ------------------ */
int mf_reads_from_packed(const uint32_t *words, const uint64_t *offsets, uint64_t n_reads,
                         const uint64_t *npos, uint64_t n_npos, int device, mf_reads **out);
int mf_reads_from_fastq(const char *fastq_path, int device, mf_reads **out);
/* Deterministic synthetic PE150-shaped read set generated straight into the
 * packed layout (bench / large parity properties): n_reads
 * reads of read_len bases, iid uniform background; a fraction mito_ppm/1e6 of
 * reads is sampled from bait_text (random strand, sub_ppm/1e6 substitution
 * error); n_read_ppm/1e6 of reads get invalid bases at rate n_base_ppm/1e6.
 * host_words_out/host_npos_out (optional) receive malloc'd host copies that
 * the caller frees with mf_free_host(). */
int mf_reads_synth(uint64_t n_reads, uint32_t read_len, uint64_t seed,
                   const char *bait_fasta_text, size_t bait_len,
                   uint32_t mito_ppm, uint32_t sub_ppm, uint32_t n_read_ppm, uint32_t n_base_ppm,
                   int device, mf_reads **out,
                   uint32_t **host_words_out, uint64_t *host_n_words_out,
                   uint64_t **host_npos_out, uint64_t *host_n_npos_out);
/* ABI 5: the same with "real-data-shaped" extras for the low-complexity leg of bench.py: msat_ppm / 1e6 of the reads are
 * microsatellites (a random motif of 1..6 bases repeated: poly-A, (TA)n, ...), numt_ppm / 1e6 are NUMT-like reads (sampled from
 * the bait, numt_div_ppm / 1e6 substitutions per base). */
int mf_reads_synth_ex(uint64_t n_reads, uint32_t read_len, uint64_t seed,
                      const char *bait_fasta_text, size_t bait_len,
                      uint32_t mito_ppm, uint32_t sub_ppm, uint32_t n_read_ppm, uint32_t n_base_ppm,
                      uint32_t msat_ppm, uint32_t numt_ppm, uint32_t numt_div_ppm,
                      int device, mf_reads **out,
                      uint32_t **host_words_out, uint64_t *host_n_words_out,
                      uint64_t **host_npos_out, uint64_t *host_n_npos_out);
void mf_free_host(void *p);
int mf_reads_info(const mf_reads *r, mf_reads_info_t *info);
int mf_reads_free(mf_reads *r);

/* ---- the hot path (rows B2, B3, B4): k-mer extract -> canonicalise ->
 * open-address probe -> hit threshold.  Inputs already resident in HBM.
 * out_bits: host buffer of ceil(n_reads/32) u32, bit r set = read r passes
 * (hits >= threshold, threshold >= 1).  hits_out: optional host buffer of
 * n_reads u32 receiving the full hit count of every read (disables the
 * early exit; parity/debug).  stats optional. */
int mf_filter(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode,
              uint32_t *out_bits, uint32_t *hits_out, mf_filter_stats_t *stats);

/* Same, result left on the device (no D2H); for timing loops.  Runs `steps`
 * passes back to back on the library's stream.  ms_total is the whole loop
 * (one event pair around it) divided by steps; the per-kernel times are
 * averages over the passes whose dispatches carry start/stop events --
 * every pass up to 8 steps, every 8th pass beyond (a profiled dispatch costs
 * a few microseconds of command-processor work). */
int mf_filter_resident(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode,
                       int steps, mf_filter_stats_t *stats);

/* Same as mf_filter_resident, and the number of passing reads of EVERY one of the `steps` passes in n_pass_per_step[0 .. steps)
 * (each pass tallies into a block of its own): consecutive passes of a call overlap on two buffer sets, and a fault that
 * touched only the middle passes would not show in the tally of the last one.  No reference counterpart (test support for
 * the pipelined pass). */
int mf_filter_resident_passes(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode,
                              int steps, uint64_t *n_pass_per_step, mf_filter_stats_t *stats);

/* Same as mf_filter_resident_passes, and the result bitmap of EVERY one of the `steps` passes in bits_per_step: steps rows of
 * ceil(n_reads/32) u32, pass s at s * ceil(n_reads/32), bit r of a row set = read r passed in that pass.  n_pass_per_step is
 * optional here.  A row is what the pass left in the result bitmap of its own buffer set: behind the pass's last kernel, on the
 * stream that carries it, the bitmap is copied into a device log (n_reads/8 bytes a pass), and where an event orders that
 * kernel against the screen that next clears the bitmap, the event is recorded again behind the copy.  The plans, kernels,
 * arguments, streams and events of the passes are those of mf_filter_resident_passes, and the host does not synchronise
 * between passes.  The copy is one short node more per pass, so the overlap of consecutive passes is not timed exactly as in
 * mf_filter_resident.  What it catches: a pass that wrote to the wrong buffer set, a bitmap cleared wrongly or not at all, a
 * stale buffer, a wait that the plan left out -- faults of the plan and the kernels.  It is no race detector.  No reference
 * counterpart (test support for the pipelined pass).  MF_E_ARG: bits_per_step NULL, steps < 1. */
int mf_filter_resident_bits(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, int steps,
                            uint32_t *bits_per_step, uint64_t *n_pass_per_step, mf_filter_stats_t *stats);

/* One-shot over host buffers (SURVEY.md 8b name): H2D, filter, D2H. */
int mf_filter_packed(const mf_kmerset *ks, int device,
                     const uint32_t *words, const uint64_t *offsets, uint64_t n_reads,
                     const uint64_t *npos, uint64_t n_npos,
                     uint32_t threshold, uint32_t *out_bits);

/* ---- file level: what a MitoFlex stage calls.  Takes the place
 * `bim.bwa_map` has in the reference (bim/bim.py:43-58: reads in, baited
 * reads out as FASTQ) and is hooked ahead of `megahit_core buildlib`
 * (assemble/assemble_wrapper.py:162-193).  fq2/out2 NULL = single end.
 * Records are zipped like the reference's PE reader (filter/filter_bin/src/
 * main.rs:214); survivors keep input order and are written header/seq/+/qual
 * (main.rs:261-268).  Chunks of whole pairs are dealt to n_devices GPUs (one
 * host thread each, no collective); ".gz" inputs/outputs by extension. */
int mf_filter_fastq_files(mf_kmerset *ks, const char *fq1, const char *fq2,
                          const char *out1, const char *out2,
                          uint32_t threshold, int pair_mode, int n_devices,
                          uint64_t *kept, uint64_t *total);
/* The same on a chosen list of devices (ABI 3): devices[0 .. n_devices) are device indices below
 * mf_device_count(), each at most once.  A ".gz" FILE takes the device ingest path: its bytes are
 * copied up as they are, the slabs of the stream are dealt to the listed devices round robin and
 * inflate, line index, 2-bit pack, filter and the copy of the survivors run there, with a bounded
 * amount of device memory whatever the file's size (the reference's readers stream too:
 * filter/filter_bin/src/helper.rs:14-31).  Plain files, pipes and BGZF take the host pipeline,
 * which wants the list to be a run of consecutive devices.  mf_filter_fastq_files(.., n, ..) is
 * this call with devices 0 .. n - 1. */
int mf_filter_fastq_files_on(mf_kmerset *ks, const char *fq1, const char *fq2,
                             const char *out1, const char *out2,
                             uint32_t threshold, int pair_mode,
                             const int *devices, int n_devices,
                             uint64_t *kept, uint64_t *total);

/* ---- record assignment: which bait record the baited reads come from.  No reference counterpart.
 * A record is what the bait parser calls one ('>' at a line start opens it; sequence before any header is an anonymous leading
 * record), numbered 0 .. R-1 in file order; its name is the header text after '>' up to the first space, tab or CR ("" for the
 * anonymous one).  Empty records, records shorter than k and duplicate names are all kept and numbered.  A canonical k-mer of the
 * set is UNIQUE to record j when j is the only record with a valid window holding it, else SHARED.  A read that passes
 * (hits >= threshold) is assigned the record with the strictly largest number of its windows whose k-mer is unique to that record;
 * MF_ASSIGN_AMBIGUOUS when that number is 0 for every record or the largest is tied; a read that does not pass: MF_ASSIGN_NONE.
 * The per-slot record-owner table is built on the device by the first call that needs it.  Protein sets: MF_E_ARG. */
#define MF_ASSIGN_AMBIGUOUS 0xFFFFFFFEu
#define MF_ASSIGN_NONE      0xFFFFFFFFu
int mf_kmerset_record_count(const mf_kmerset *ks, uint64_t *n_records);
/* copies the NUL-terminated name; returns MF_E_ARG if buflen is too small and sets *needed (may be NULL) */
int mf_kmerset_record_name(const mf_kmerset *ks, uint64_t i, char *buf, size_t buflen, size_t *needed);
/* one pass like mf_filter, then assignment; out_bits (ceil(n_reads/32) u32) / assign_out (n_reads u32) / record_reads (R + 2 u64:
 * reads assigned to each record, then ambiguous, then unassigned reads; they sum to n_reads) / stats (of the filter pass) each optional */
int mf_assign(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode,
              uint32_t *out_bits, uint32_t *assign_out, uint64_t *record_reads, mf_filter_stats_t *stats);
/* mf_filter_fastq_files_on plus the per-record counts of the kept reads (R + 2 u64, mates counted one by one: a kept mate that
 * did not pass its own threshold is unassigned; they sum to kept * (2 if paired else 1)); the same ingest path and output files
 * byte-identical to it */
int mf_filter_fastq_files_by_record(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                    uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                    uint64_t *record_reads, uint64_t *kept, uint64_t *total);

/* ---- group assignment: which GROUP of bait records the baited reads come from, for nucleotide and protein sets.  No reference
 * counterpart.  The calls above keep their behaviour (protein sets included: MF_E_ARG).
 * Records: protein sets follow the same record rules as nucleotide sets ('>' at a line start opens a record; its name is the header
 * text up to the first space, tab or CR).
 * Grouping: every record belongs to one group; groups are numbered 0 .. G-1 in order of first appearance.  By default, and after
 * mf_kmerset_group_records(ks, NULL, 0), the grouping is the IDENTITY: each record is its own group, named after it (G = R; duplicate
 * names are not merged).  mf_kmerset_group_records(ks, sep, f) (f >= 1) names a record's group by the f-th sep-separated token of its
 * name, counting from 1; a name with fewer than f fields is its own group name.  (MT_database headers, gi_NC_<acc>_<GENE>_<Genus>_
 * <species>_<len>_aa: sep "_", f = 4 groups by gene.)
 * Windows of a read: nucleotide sets, its valid k-windows (as mf_assign); protein sets, the (frame, window) pairs that count as hits
 * (six frames, kp codons, all sense codons, no invalid base): 2 * max(0, L - 3kp + 1) of them for a read of length L.
 * A key is UNIQUE to group g when every record with a valid window holding it belongs to g.  A read that passes (hits >= threshold)
 * is assigned the group with the strictly largest number of its windows whose key is unique to that group; MF_ASSIGN_AMBIGUOUS when
 * there is none or the largest is tied; a read that does not pass: MF_ASSIGN_NONE.  Under the identity grouping a nucleotide set's
 * grouped calls return exactly what mf_assign / mf_filter_fastq_files_by_record return.
 * The per-slot group-owner table is built on each device by the first grouped call there; it is separate from the record-owner
 * table, so mf_assign is unaffected by the grouping. */
/* sep NULL or field 0: identity.  Frees the set's group-owner tables on every device: it must not run while another call uses the set. */
int mf_kmerset_group_records(mf_kmerset *ks, const char *sep, int field);
int mf_kmerset_group_count(const mf_kmerset *ks, uint64_t *n_groups);
/* copies the NUL-terminated name; returns MF_E_ARG if buflen is too small and sets *needed (may be NULL) */
int mf_kmerset_group_name(const mf_kmerset *ks, uint64_t i, char *buf, size_t buflen, size_t *needed);
/* mf_assign by group: group_reads has G + 2 entries (each group, then ambiguous, then unassigned reads) */
int mf_assign_groups(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode,
                     uint32_t *out_bits, uint32_t *assign_out, uint64_t *group_reads, mf_filter_stats_t *stats);
/* mf_filter_fastq_files_by_record by group (G + 2 u64); the same ingest path and output files byte-identical to
 * mf_filter_fastq_files_on */
int mf_filter_fastq_files_by_group(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                   uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                   uint64_t *group_reads, uint64_t *kept, uint64_t *total);

/* ---- k-mer depth along the bait records: how deep, and how evenly, the baited reads cover each record.  No reference counterpart: the
 * reference gets a per-contig mean depth from `bwa mem | samtools depth -aa | avgdep` (findmitoscaf/findmitoscaf.py:439-467).
 * Positions: a set's positions are the letters of its records, concatenated in file order, invalid letters included -- bases of a
 * nucleotide set, residues of a protein set (mf_kmerset_info's n_windows does not count them; mf_kmerset_record_starts does).  Record j
 * covers [starts[j], starts[j+1]).
 * Valid window: position p starts a valid window when the k bases (nucleotide set) or kp residues (protein set) from p lie inside one
 * record and none of them is invalid (the rule the table builders use).
 * Counted reads: only the reads that pass (hits >= threshold), as mf_filter decides.
 * Windows of a read: those of mf_assign_groups -- nucleotide sets, the valid k-windows, canonical keys; protein sets, the (frame, window)
 * pairs that count as hits.
 * Depth of a window: the depth of the valid window at p is the number of windows, over all counted reads, whose key equals the key of the
 * window at p.  Nucleotide keys are canonical, so both strands count.  A key that several bait windows hold (a repeat, a k-mer shared
 * between records) gives its full count to each of them, like a multi-mapping read; a read that holds a key twice counts twice.
 * Profile: one uint32_t per position -- the depth of the window that starts there, clamped at 0xFFFFFFFE; MF_DEPTH_NONE where no valid
 * window starts.
 * Per-record summary: windows = the record's valid windows, covered = those of depth >= 1, depth_sum / depth_max = the sum and the
 * maximum of their unclamped depths.  The mean k-mer depth is depth_sum / windows; for reads of length L it is about base depth *
 * (L - k + 1) / L.  No base-level depth is computed here: mf_place below does.
 * File level: every mate that passes its own threshold is counted, whether or not the pair rule keeps its pair; the pair rule decides
 * only what is written.  A file-level profile therefore equals the sum of the in-memory profiles of the mate-1 and mate-2 read sets,
 * before clamping.
 * The per-slot representative table (smallest position whose valid window holds the key) and the per-position table behind it are built
 * on each device by the first depth call there.  Sets of 2^32 - 1 positions or more: MF_E_ARG. */
#define MF_DEPTH_NONE 0xFFFFFFFFu
typedef struct { uint64_t windows, covered, depth_sum, depth_max; } mf_depth_record_t;
/* R + 1 position offsets, nucleotide and protein sets alike; MF_E_ARG and *needed (may be NULL) when n is too small */
int mf_kmerset_record_starts(const mf_kmerset *ks, uint64_t *starts, size_t n, size_t *needed);
/* one pass like mf_filter, then depth; out_bits / profile (starts[R] u32) / records (R entries) / stats each optional */
int mf_depth(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode,
             uint32_t *out_bits, uint32_t *profile, mf_depth_record_t *records, mf_filter_stats_t *stats);
/* mf_filter_fastq_files_on plus depth over the whole input; the same ingest path, output files byte-identical to it; profile / records
 * each optional */
int mf_filter_fastq_files_depth(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                uint32_t *profile, mf_depth_record_t *records, uint64_t *kept, uint64_t *total);

/* ---- placement: where on the bait, and on which strand, a baited read lies, and the BASE depth that follows.  Nucleotide sets only:
 * every call below returns MF_E_ARG for a protein set.  No reference counterpart: the reference places reads with `bwa mem` and gets base
 * depth from `samtools depth -aa` (findmitoscaf/findmitoscaf.py:439-467).
 * Positions, records and valid windows are those of the depth section (mf_kmerset_record_starts).
 * Anchor: a canonical key of the set is an ANCHOR when exactly one valid bait window, over all records, holds it, and that window is not
 * its own reverse complement.  An anchor has the position p of that window, the record j of that window, and a bait orientation b: 0 when
 * the bait's forward text of the window is the canonical form, 1 when its reverse complement is.
 * Votes of a read of length L: every valid k-window at offset o (0 <= o <= L - k) whose canonical key is an anchor casts one vote.  r is 0
 * when the read's forward text of the window is the canonical form, else 1; strand = b xor r (0: the read lies as the bait's forward
 * strand, 1: its reverse complement does); start = p - starts[j] - o for strand 0 and p - starts[j] - (L - k - o) for strand 1: the
 * record coordinate of the leftmost base of the read's footprint, which may be negative.  The vote goes to the candidate (j, strand,
 * start); two anchors in different records are different candidates even when their global diagonals coincide.
 * Placement: defined for the reads that pass (hits >= threshold, as mf_filter decides).  The winner is the candidate with strictly the
 * most votes: record = j, strand, start, end = start + L (exclusive, unclipped), votes = the winner's votes, windows = the read's anchor
 * windows over all candidates.  record = MF_PLACE_AMBIGUOUS when the read passes but has no anchor window or the largest vote count is
 * tied; the other fields are then 0, except windows.  record = MF_PLACE_NONE and every other field 0 when the read does not pass.
 * There is NO handling of indels or clipping: the whole read counts on its winning diagonal.
 * Base depth: a placed read covers the record positions [max(start, 0), min(end, len_j)) -- never empty, because the winning anchor's
 * window lies inside the record.  Base depth is one uint32_t per position of the set, invalid letters included (there is no "none"
 * marker): the number of placed reads that cover it, clamped at 0xFFFFFFFE.
 * Per record (mf_place_record_t): forward / reverse = the reads placed on the record, by strand; over_begin = those with start < 0;
 * over_end = those with end > len_j; covered = positions of depth >= 1; base_sum = the sum of the unclamped depths (the mean base depth
 * is base_sum / len_j).
 * unplaced: two uint64_t -- the passing reads that are not placed, then the reads that do not pass.  Sum(forward + reverse) + unplaced[0]
 * + unplaced[1] = n_reads.
 * File level: as for depth, every mate that passes its own threshold is placed and counted, whether or not the pair rule keeps its pair.
 * A file-level base depth therefore equals the sum, before clamping, of the in-memory base depths of the mate-1 and mate-2 read sets; the
 * record summaries add likewise, except covered; unplaced[1] counts mates.  The output files are byte-identical to
 * mf_filter_fastq_files_on's.
 * Rejected with MF_E_ARG: sets of 2^31 - 1 positions or more; sets of 2^30 records or more (record and strand share one 32-bit word on
 * the device, and a record has four counters); read sets holding a read of 2^31 - positions bases or more, positions being the set's
 * (start and end are 32-bit: no read may end at 2^31 or beyond wherever it lies, which also refuses every read of 2^31 bases or more).
 * The per-slot anchor table is built on each device by the first placement call there. */
#define MF_PLACE_AMBIGUOUS 0xFFFFFFFEu
#define MF_PLACE_NONE      0xFFFFFFFFu
typedef struct { uint32_t record, strand; int32_t start, end; uint32_t votes, windows; } mf_place_t;
typedef struct { uint64_t forward, reverse, over_begin, over_end, covered, base_sum; } mf_place_record_t;
/* one pass like mf_filter, then placement; out_bits / place_out (n_reads entries) / base_depth (starts[R] u32) / records (R entries) /
 * unplaced (2 u64) / stats each optional */
int mf_place(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode,
             uint32_t *out_bits, mf_place_t *place_out, uint32_t *base_depth,
             mf_place_record_t *records, uint64_t *unplaced, mf_filter_stats_t *stats);
/* mf_filter_fastq_files_on plus placement over the whole input; the same ingest path; base_depth / records / unplaced each optional */
int mf_filter_fastq_files_placed(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                 uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                 uint32_t *base_depth, mf_place_record_t *records, uint64_t *unplaced,
                                 uint64_t *kept, uint64_t *total);

/* ---- pile-up: which bases the placed reads put on every bait position, the consensus they give and where it differs from the bait.
 * Nucleotide sets only: every call below returns MF_E_ARG for a protein set.  No reference counterpart: the reference gets this from
 * `bwa mem` + `samtools mpileup`.
 * Positions, records and placement are exactly those of the placement section: a pile-up call places the passing reads as mf_place does.
 * Pile-up: take a placed read of length L with (record j, strand, start).  Its base at read offset i (0 <= i < L) lies at record
 * coordinate c = start + i for strand 0 and c = start + (L - 1 - i) for strand 1; on strand 1 the letter is complemented, so counts are
 * always in the bait's forward letters.  The base is counted when 0 <= c < len_j and it is a valid letter: an invalid read base (N)
 * counts nowhere, and a base that hangs over either end of the record counts nowhere -- in particular NOT in the neighbouring record,
 * although global positions are contiguous (only the extended calls below pile such bases, in a table of their own).  Reads that are
 * ambiguous, unplaced or not passing contribute nothing.  Invalid bait
 * positions still receive counts.  There is no handling of indels or clipping: behind an insertion the shifted bases pile up as
 * mismatches.  The result is four uint32_t per position of the set, mf_pileup_t { a, c, g, t }, each clamped at 0xFFFFFFFE.
 * a + c + g + t at a position is at most the position's base depth (mf_place); the two are equal where no covering read has an N there.
 * Consensus: take min_depth >= 1 (0 is MF_E_ARG).  Per position let d be the unclamped sum of the four counts and m the largest count.
 * If d >= min_depth and exactly one letter has count m, the position is CALLED and the byte is that letter in upper case; if
 * d >= min_depth and the maximum is tied, the position is AMBIGUOUS and the byte is 'N'; if d < min_depth the byte is the bait's own
 * letter in lower case ('n' for an invalid bait letter).  One byte per position: a record's consensus has the record's length and can
 * be baited with again.
 * Per record (mf_pileup_record_t): bases = sum of d; matches = sum of the count of the bait's letter, over valid bait positions;
 * mismatches = sum of d minus that count, over valid bait positions; called = the called positions; ambiguous = the ambiguous
 * positions; variants = called positions whose bait letter is valid and differs from the call.  bases - matches - mismatches is what
 * fell on invalid bait letters.
 * unplaced: as in mf_place.
 * File level: every mate that passes its own threshold is piled, as for placement.  Counts, bases, matches and mismatches add over mates
 * and devices before clamping; the consensus, called, ambiguous and variants are computed once from the summed counts.  The output
 * files are byte-identical to mf_filter_fastq_files_on's.
 * Limits: placement's limits apply.  The counters take 32 bytes a position on the device: when they cannot be allocated the call
 * returns MF_E_NOMEM with a message that names the size.
 * The bait's packed letters are kept on each device, beside the anchor table, by the first pile-up call there. */
typedef struct { uint32_t a, c, g, t; } mf_pileup_t;
typedef struct { uint64_t bases, matches, mismatches, called, ambiguous, variants; } mf_pileup_record_t;
/* one of 'A' 'C' 'G' 'T' 'N' per position (starts[R] bytes), 'N' for an invalid bait letter; MF_E_ARG and *needed (may be NULL) when n
 * is too small */
int mf_kmerset_bait_letters(const mf_kmerset *ks, uint8_t *letters, size_t n, size_t *needed);
/* one pass like mf_filter, then placement and pile-up; out_bits / pileup (starts[R] entries) / consensus (starts[R] bytes) / records
 * (R entries) / unplaced (2 u64) / stats each optional */
int mf_pileup(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth,
              uint32_t *out_bits, mf_pileup_t *pileup, uint8_t *consensus,
              mf_pileup_record_t *records, uint64_t *unplaced, mf_filter_stats_t *stats);
/* mf_filter_fastq_files_on plus the pile-up over the whole input; the same ingest path; pileup / consensus / records / unplaced each
 * optional */
int mf_filter_fastq_files_pileup(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
                                 uint32_t threshold, int pair_mode, const int *devices, int n_devices,
                                 uint32_t min_depth, mf_pileup_t *pileup, uint8_t *consensus,
                                 mf_pileup_record_t *records, uint64_t *unplaced, uint64_t *kept, uint64_t *total);

/* ---- verification: how well every placed read agrees with the bait along its placement, and an identity cut on that score.
 * Nucleotide sets only: every call below returns MF_E_ARG for a protein set.  No reference counterpart: the reference reads this off
 * the NM tag and the CIGAR of `bwa mem`.
 * Positions, records and placement are exactly those of the placement section, the coordinates of a read's bases those of the pile-up
 * section.
 * Score of a placed read: take a read of length L placed at (record j, strand, start).  Its base at read offset i lies at record
 * coordinate c = start + i for strand 0 and c = start + (L - 1 - i) for strand 1; on strand 1 the letter is complemented.  The base is
 * COMPARED when 0 <= c < len_j, the read base is a valid letter and the bait letter at c is valid.  A compared base is a MISMATCH when
 * the oriented read letter differs from the bait letter.  compared and mismatches are the two counts.  The winning anchor's window lies
 * inside both the read and the record and matches exactly, so compared >= k and mismatches <= compared - k: nothing ever divides by
 * zero.  Overhangs, read Ns and invalid bait letters are not compared.  This score handles no indels: behind an insertion the
 * shifted bases are mismatches, which is what the score is there to show (the banded alignment below handles them).
 * Cut: max_permille in 0 .. 1000 (more is MF_E_ARG).  A placed read is ACCEPTED iff
 * (uint64_t)mismatches * 1000 <= (uint64_t)max_permille * compared, otherwise REJECTED.  A rejected read contributes NOTHING to base
 * depth, to forward / reverse / over_begin / over_end, or to the pile-up counters.  It is not "unplaced": its mf_place_t keeps the real
 * placement, and its mf_score_t says why it was cut.  At max_permille = 1000 every placed read is accepted, and every placement and
 * pile-up output equals mf_place's and mf_pileup's bit for bit.
 * Per read (mf_score_t): compared, mismatches; { 0, 0 } for a read that is not placed.
 * Per record (mf_score_record_t): accepted / rejected = the placed reads of the record on either side of the cut; compared and
 * mismatches are summed over the ACCEPTED reads; hist[b] counts ALL placed reads of the record, accepted and rejected, with
 * min(mismatches, MF_SCORE_BINS - 1) == b -- read at 1000 permille, the histogram is what a cut is picked from.
 * accepted == forward + reverse of the placement record; sum(hist) == accepted + rejected; sum(forward + reverse + rejected) +
 * unplaced[0] + unplaced[1] == n_reads; compared == matches + mismatches and mismatches == mismatches of the pile-up record.
 * File level: as for placement, every mate that passes its own threshold is scored, whether or not the pair rule keeps its pair; all
 * counts add over mates and devices; the consensus is called once from the summed counts.  The output files are byte-identical to
 * mf_filter_fastq_files_on's: a rejected read is still written.
 * Limits: placement's limits apply; min_depth == 0 is MF_E_ARG as for the pile-up.  When pileup, consensus and pileup_records are all
 * NULL a call allocates no pile-up counters and piles nothing.
 * The bait's validity, one bit a position, is kept on each device beside its packed letters by the first verifying or pile-up call. */
#define MF_SCORE_BINS 32
typedef struct { uint32_t compared, mismatches; } mf_score_t;
typedef struct { uint64_t accepted, rejected, compared, mismatches, hist[MF_SCORE_BINS]; } mf_score_record_t;
/* one pass like mf_filter, then placement, score, cut and (when asked for) pile-up; out_bits / place_out / score_out (n_reads entries
 * each) / base_depth (starts[R] u32) / place_records / pileup (starts[R] entries) / consensus (starts[R] bytes) / pileup_records /
 * score_records (R entries each) / unplaced (2 u64) / stats each optional */
int mf_verify(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille,
              uint32_t *out_bits, mf_place_t *place_out, mf_score_t *score_out, uint32_t *base_depth, mf_place_record_t *place_records,
              mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records, mf_score_record_t *score_records,
              uint64_t *unplaced, mf_filter_stats_t *stats);
/* mf_filter_fastq_files_on plus verified placement and pile-up over the whole input; the same ingest path; every output optional */
int mf_filter_fastq_files_verified(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
              uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille,
              uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
              mf_pileup_record_t *pileup_records, mf_score_record_t *score_records, uint64_t *unplaced, uint64_t *kept, uint64_t *total);

/* ---- which mates are written: the keep rule.  The verifying calls above cut the reports only; the two calls below also let the cut
 * decide what is written.  Every mate has a PASS bit (it passes its own threshold); the keep mode turns it into a KEEP bit:
 *   MF_KEEP_PASSING   the keep bit is the pass bit: everything is what mf_verify / mf_filter_fastq_files_verified give.
 *   MF_KEEP_ACCEPTED  a mate that is placed and REJECTED by the cut loses its bit.
 *   MF_KEEP_PLACED    additionally a passing mate that is NOT PLACED (ambiguous, or no anchor window) loses its bit: only mates that are
 *                     placed and accepted keep it.
 * Any other keep is MF_E_ARG.  The keep bit takes the pass bit's place in the pair rule, and the pair rule itself is as it was:
 * MF_PAIR_EITHER writes a pair when either mate still has its bit, MF_PAIR_BOTH when both have; single-end input writes a read that
 * keeps its bit.  *kept counts what is written.  What the reports count does NOT depend on the keep mode: base depth, the records,
 * the pile-up, the scores and unplaced are those of every mate that passes its own threshold, cut at max_permille as above.
 * Two identities for single-end input, score_records summed over the records:
 *   MF_KEEP_ACCEPTED:  kept == passing reads - sum(rejected)      (passing reads = total - unplaced[1])
 *   MF_KEEP_PLACED:    kept == sum(accepted)
 * Resident: keep_bits (optional, n_reads bits laid out like out_bits, tail bits 0) receives the keep bits; out_bits stays the pass
 * bits.  With MF_KEEP_PASSING keep_bits equals out_bits.  This scoring knows no indels: under a tight cut a read with a true indel
 * against the bait is rejected and, with a keep mode, not written -- read the histogram at max_permille 1000 before picking a cut, or
 * use the aligning calls below. */
enum { MF_KEEP_PASSING = 0, MF_KEEP_ACCEPTED = 1, MF_KEEP_PLACED = 2 };
/* mf_verify with a keep mode: keep behind max_permille, keep_bits behind out_bits; every output optional */
int mf_verify_keep(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille,
              int keep, uint32_t *out_bits, uint32_t *keep_bits, mf_place_t *place_out, mf_score_t *score_out, uint32_t *base_depth,
              mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records,
              mf_score_record_t *score_records, uint64_t *unplaced, mf_filter_stats_t *stats);
/* mf_filter_fastq_files_verified with a keep mode (behind max_permille): the output files hold the pairs the keep bits select */
int mf_filter_fastq_files_verified_keep(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
              uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille, int keep,
              uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
              mf_pileup_record_t *pileup_records, mf_score_record_t *score_records, uint64_t *unplaced, uint64_t *kept, uint64_t *total);

/* ---- banded alignment: the verifying calls with indels.  mf_align is mf_verify_keep with one more parameter, band (W); placement --
 * the anchor vote, the strict winner, mf_place_t -- is exactly as above.  Every placed read is then aligned to its record inside the
 * band of 2 W + 1 diagonals around the winning one, and the cut, the histogram, the keep rule, the base-depth footprint, over_begin /
 * over_end and the pile-up coordinates follow the alignment; a per-position indel table is new.  Nucleotide sets only.
 * The rule.  A read of L bases is placed at (record j of len positions, strand, start).  x[0 .. L) is the read oriented to the bait's
 * forward strand (on strand 1 its reverse complement); i indexes x; c is a record coordinate.  Cells D(i, c), 0 <= i <= L,
 * |c - (start + i)| <= W; everything outside the band is +inf.
 *   D(0, c) = 0 for every c of the band (the begin on the bait is free; row 0 has no step inside the row).
 *   D(i, c), i >= 1, is the least of   diagonal   D(i-1, c-1) + sub(i-1, c-1)
 *                                      insertion  D(i-1, c) + 1      (read base i-1 against nothing)
 *                                      deletion   D(i, c-1) + 1      (bait position c-1 against nothing)
 *   sub(i, c) = 0 and the column is NOT COMPARED when c < 0, c >= len, x[i] is an N or the bait letter at c is invalid; otherwise the
 *   column is COMPARED and sub is 1 iff the letters differ (mf_verify's compared and mismatch).  A coordinate outside [0, len) is a
 *   wildcard even where a neighbouring record lies there.
 *   End cell: the c of row L with the least D(L, c); ties go to the least |c - (start + L)|, then to the smaller c.  That c is ref_end.
 *   Traceback from (L, ref_end): at a cell the first move that reproduces its value, in the order diagonal, deletion, insertion; it
 *   stops at i == 0, and the c there is ref_begin.
 *   compared and mismatches are counted over the diagonal steps; insertions = insertion steps (read bases), deletions = deletion steps
 *   (bait positions); edits = mismatches + insertions + deletions.
 *   Cut: accepted iff (uint64_t)edits * 1000 <= (uint64_t)max_permille * (compared + insertions + deletions).
 * band is 0 .. min(31, k - 1); anything else is MF_E_ARG.  With band < k the footprint clipped to the record is never empty.  At
 * band == 0 the rule is mf_verify_keep's, and every output equals that call's bit for bit (mf_align_t's compared / mismatches are
 * mf_score_t's, its ref_begin / ref_end are start / end).
 * What an ACCEPTED read adds: base depth over [max(ref_begin, 0), min(ref_end, len)) -- deleted positions inside count as covered --;
 * forward or reverse; over_begin iff ref_begin < 0, over_end iff ref_end > len; to the pile-up, for every diagonal step whose read base
 * is valid and whose c lies in [0, len), 1 at [c][oriented letter] (inserted bases add nowhere); to the indel table (mf_indel_t, one
 * entry a bait position, clamped like the depth): a deletion step over c in [0, len) adds 1 to del[c]; a maximal run of n insertion
 * steps at column c (between positions c-1 and c) adds 1 to ins[c-1] and n to ins_bases[c-1] when 0 <= c-1 < len.  A REJECTED read adds
 * to `rejected` and its histogram bin only.
 * Per read (mf_align_t): all zero for a read that is not placed.  Per record (mf_align_record_t): sums over the accepted reads; gapped =
 * accepted reads with at least one gap; hist[min(edits, 31)] over all placed reads.
 * accepted == forward + reverse; sum(hist) == accepted + rejected; base_sum == the sum of the clipped footprints of the accepted reads;
 * sum(del) over a record <= deletions; mismatches of the pile-up record == mismatches of the align record.
 * The consensus rule is unchanged and calls substitutions only: the indel table is the report on indels (the gapped consensus below
 * calls them).
 * Device memory: the traceback's direction bits and per-base columns live in a slice per resident wave (24 bytes a base of the longest
 * read), bounded whatever the number of reads; there is no read-length limit below placement's. */
typedef struct { uint32_t compared, mismatches, insertions, deletions; int32_t ref_begin, ref_end; } mf_align_t;
typedef struct { uint32_t del, ins, ins_bases; } mf_indel_t;
typedef struct { uint64_t accepted, rejected, compared, mismatches, insertions, deletions, gapped, hist[MF_SCORE_BINS]; } mf_align_record_t;
/* mf_verify_keep with band behind keep, align_out for score_out, indels (starts[R] entries) behind pileup_records and align_records for
 * score_records; every output optional */
int mf_align(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille,
              int keep, uint32_t band, uint32_t *out_bits, uint32_t *keep_bits, mf_place_t *place_out, mf_align_t *align_out, uint32_t *base_depth,
              mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records,
              mf_indel_t *indels, mf_align_record_t *align_records, uint64_t *unplaced, mf_filter_stats_t *stats);
/* mf_filter_fastq_files_verified_keep likewise: the output files hold the pairs the keep bits of the aligned cut select */
int mf_filter_fastq_files_aligned(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
              uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille, int keep,
              uint32_t band, uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
              mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records, uint64_t *unplaced,
              uint64_t *kept, uint64_t *total);

/* ---- gapped consensus: the aligning calls with the letters of the inserted bases, and a consensus that calls indels.  mf_align_gapped
 * and mf_filter_fastq_files_gapped are mf_align and mf_filter_fastq_files_aligned with four outputs behind align_records, each optional.
 * With all four NULL they ARE the older calls: nothing more is allocated, the same kernels run, the same bits come back.  Asking for any
 * of them implies the pile-up counters.  Nucleotide sets only; band as above.  ABI 5 still.
 * The rule.  span = 2 * band: a run of insertion steps stays in one column and moves one diagonal a step, so no run is longer.
 *   Insertion pile.  An accepted read's maximal run of n insertion steps at column c (between record positions c-1 and c; the run that
 *   adds 1 to ins[c-1] and n to ins_bases[c-1]), when 0 <= c-1 < len: the t-th base of the run, t from 0 in the order of the oriented read
 *   x (so in the bait's forward letters), adds 1 at ins_pile[(s0 + c-1) * span + t][letter].  An inserted N adds nowhere and still takes
 *   its offset t.  Rejected, ambiguous, unplaced and non-passing reads add nothing.  For every position the sum over t and the four
 *   letters is <= ins_bases, equal when no inserted base is an N.  Output: mf_pileup_t[positions * span], clamped at 0xFFFFFFFE like the
 *   pile-up.  The call below goes by the unclamped sums.
 *   Call.  For each position p of a record, in order.  D: the unclamped base depth of the aligning call (deleted positions count as
 *   covered).  min_depth: the pile-up's (0 is MF_E_ARG).
 *     p is DELETED iff D >= min_depth and 2 * del[p] > D; a deleted position emits no byte.  Otherwise it emits the byte the unchanged
 *     consensus rule gives for p.
 *     Then the insertion columns behind p, q = 0, 1, .., span - 1, n_q being the sum of the four counts at (p, q): column q is emitted iff
 *     D >= min_depth and 2 * n_q > D, and emission stops at the first q that is not.  An emitted column's byte is the letter with
 *     strictly the largest count, in upper case; a tie gives 'N'.
 *     Both majorities are strict: support from exactly half of the covering reads calls nothing.
 *   Result.  gapped: the emitted bytes of all records, concatenated; the caller's buffer holds positions * (1 + span) bytes, which is
 *   always enough.  gapped_starts: R + 1 offsets into gapped.  mf_gapped_record_t per record: insertions counts the positions with at
 *   least one emitted column.
 *   length == len_j - deleted + inserted_bases.  At band == 0 the span is 0 and nothing is deleted: gapped is consensus byte for byte and
 *   gapped_starts is the record starts.
 * File level: the insertion counters add over mates, batches and devices before they are clamped, like the pile-up's; the call is made
 * once, from the sums.
 * Device memory: 4 * span 64-bit counters a position behind the indel counters (512 bytes a position at band 8, about 2 KB at band 31);
 * where they cannot be allocated the call returns MF_E_NOMEM and names the size. */
typedef struct { uint64_t length, deleted, insertions, inserted_bases; } mf_gapped_record_t;
int mf_align_gapped(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille,
              int keep, uint32_t band, uint32_t *out_bits, uint32_t *keep_bits, mf_place_t *place_out, mf_align_t *align_out, uint32_t *base_depth,
              mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records,
              mf_indel_t *indels, mf_align_record_t *align_records, mf_pileup_t *ins_pile, uint8_t *gapped, uint64_t *gapped_starts,
              mf_gapped_record_t *gapped_records, uint64_t *unplaced, mf_filter_stats_t *stats);
int mf_filter_fastq_files_gapped(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
              uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille, int keep,
              uint32_t band, uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
              mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records, mf_pileup_t *ins_pile, uint8_t *gapped,
              uint64_t *gapped_starts, mf_gapped_record_t *gapped_records, uint64_t *unplaced, uint64_t *kept, uint64_t *total);

/* ---- extended records: the gapped calls with the bases that hang over a record's ends piled up, and both ends called.
 * mf_align_extended and mf_filter_fastq_files_extended are mf_align_gapped and mf_filter_fastq_files_gapped with `extend` behind `band`
 * and four outputs behind gapped_records, each optional.  extend is E, 0 <= E <= MF_EXTEND_MAX; more is MF_E_ARG.  With extend == 0 the
 * four must be NULL (else MF_E_ARG) and the calls ARE the gapped ones: nothing more is allocated, the same kernels run, the same bits
 * come back.  Asking for any of the four implies the pile-up counters and the gapped consensus, asked for or not.  Band, cut, keep rule
 * and placement are exactly the gapped calls'; band 0 is allowed (the path is then the placement's diagonal).  Nucleotide sets only.
 * ABI 5 still.  Nothing above changes: base depth, pile-up and over_begin / over_end count what they counted.
 * The rule.
 *   Extension pile.  An ACCEPTED read's DIAGONAL step that puts oriented read base x[i] on record coordinate c with c < 0 or c >= len_j
 *   has the offset e = -1 - c at the begin (side 0) and e = c - len_j at the end (side 1); e = 0 is the column next to the record.  When
 *   e < E and x[i] is a valid letter the step adds 1 at ext_pile[(2 j + side) * E + e][letter], in the bait's forward letters as
 *   everywhere.  An N adds nowhere and its column is not shifted; insertion and deletion steps outside [0, len) add nowhere; steps with
 *   e >= E add nowhere; rejected, ambiguous, unplaced and non-passing reads add nothing.  A base beyond record j's end goes to j's end
 *   table, never to the neighbouring record, although global positions are contiguous.  Output: mf_pileup_t[R * 2 * E], clamped at
 *   0xFFFFFFFE; the call below goes by the unclamped sums.
 *   For every record and e, the four counts at end offset e sum to at most the number of the record's accepted reads with
 *   ref_end - len_j > e (begin: -ref_begin > e), and to exactly that where no overhanging base is an N.
 *   Call.  Per record and side, for e = 0, 1, ..: n_e is the sum of the four counts at offset e; column e is emitted iff
 *   n_e >= min_depth and exactly one letter has the largest count, and emission stops at the first e that is not emitted.  A tie emits
 *   nothing and stops the end: an N at a growing end would only break the next generation's k-mers.  The byte is that letter in upper case.
 *   Result.  extended holds, for every record in order: the emitted begin columns from the farthest to e = 0, then the record's bytes
 *   of the gapped consensus of the same call (at band 0 the plain consensus), then the emitted end columns from e = 0 up.
 *   extended_starts: R + 1 offsets into extended.  mf_extend_record_t per record: begin_bases and end_bases are the emitted columns,
 *   begin_piled and end_piled the unclamped sum of all counts of that end's table, length == gapped length + begin_bases + end_bases.
 *   The caller's buffer of positions * (1 + 2 * band) + 2 * R * E bytes is always enough.
 * File level: the counters add over mates, batches and devices before they are clamped; the call is made once, from the sums.
 * Device memory: 2 * E * 4 64-bit counters a record behind the insertion pile (256 KB a record at E = 4096); where they cannot be
 * allocated the call returns MF_E_NOMEM and names the size. */
#define MF_EXTEND_MAX 4096
typedef struct { uint64_t length, begin_bases, end_bases, begin_piled, end_piled; } mf_extend_record_t;
int mf_align_extended(const mf_kmerset *ks, const mf_reads *reads, uint32_t threshold, int mode, uint32_t min_depth, uint32_t max_permille,
              int keep, uint32_t band, uint32_t extend, uint32_t *out_bits, uint32_t *keep_bits, mf_place_t *place_out, mf_align_t *align_out,
              uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus, mf_pileup_record_t *pileup_records,
              mf_indel_t *indels, mf_align_record_t *align_records, mf_pileup_t *ins_pile, uint8_t *gapped, uint64_t *gapped_starts,
              mf_gapped_record_t *gapped_records, mf_pileup_t *ext_pile, uint8_t *extended, uint64_t *extended_starts,
              mf_extend_record_t *extend_records, uint64_t *unplaced, mf_filter_stats_t *stats);
int mf_filter_fastq_files_extended(mf_kmerset *ks, const char *fq1, const char *fq2, const char *out1, const char *out2,
              uint32_t threshold, int pair_mode, const int *devices, int n_devices, uint32_t min_depth, uint32_t max_permille, int keep,
              uint32_t band, uint32_t extend, uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
              mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records, mf_pileup_t *ins_pile, uint8_t *gapped,
              uint64_t *gapped_starts, mf_gapped_record_t *gapped_records, mf_pileup_t *ext_pile, uint8_t *extended, uint64_t *extended_starts,
              mf_extend_record_t *extend_records, uint64_t *unplaced, uint64_t *kept, uint64_t *total);

/* ---- pairs: the two mates of a pair seen together -- the insert they span, and the RESCUE of a mate the vote cannot place from the
 * window its placed mate implies.  Every call above treats a mate as a lone read: a read in a diverged stretch of the bait (no k-mer
 * in common with it) draws no vote, a read inside a repeat or inside a stretch two records share has no anchor window, and neither adds
 * to base depth, the pile-up or the consensus -- although its mate a few hundred bases away is placed without trouble.  Aligners call
 * this mate rescue (`bwa mem` does it; the reference gets its pile-up from `bwa mem`, see the placement section).  Nucleotide sets only.
 * ABI 5 still.  Nothing above changes.
 * A paired call takes two read sets of equal n_reads on one device: read i of the first set and read i of the second are mates.  It
 * takes min_insert >= 1, max_insert >= min_insert with max_insert - min_insert + 1 <= MF_RESCUE_MAX and max_insert < 2^31, rescue (0 or
 * 1), rescue_permille (0 .. 1000) and the verifying call's threshold, mode, min_depth, max_permille.
 * The rule.
 *   1. Each set is verified as today: filtered, placed by vote, scored and cut at max_permille exactly as mf_verify does it.  Both sets
 *      add into ONE set of counters, as the file-level calls already sum mates.  A mate is SETTLED when it is placed by vote and accepted.
 *   2. Insert.  The insert of two settled mates on one record and on opposite strands is `end` of the strand-1 mate minus `start` of the
 *      strand-0 mate; it is reported when it is above 0, else as -1.  The pair is PROPER when min_insert <= insert <= max_insert.
 *   3. Rescue target.  With rescue = 1, a pair with exactly one settled mate A (record j, strand s, start a, end e) is looked at when the
 *      other mate B, of L bases, has record >= MF_PLACE_AMBIGUOUS: B did not pass, or passed but is ambiguous.  A mate that was placed and
 *      rejected is never rescued.
 *   4. Candidates.  B's candidates lie on record j and on strand 1 - s.  For s = 0 the candidate starts are a + d - L for every d in
 *      [min_insert, max_insert]; for s = 1 they are e - d.  Either way the pair's insert would be d.  Each candidate is scored by the
 *      verification rule, unchanged: only bases inside record j are compared -- bases in a neighbouring record never, although global
 *      positions are contiguous --, and only valid read bases on valid bait letters.  A candidate is ADMISSIBLE when compared >= k and
 *      mismatches * 1000 <= rescue_permille * compared.
 *   5. Winner.  B is rescued when exactly one admissible candidate has the fewest mismatches.  Two candidates that share the fewest
 *      mismatches, whatever their compared, leave B as it was: a shifted copy in a homopolymer or a tandem repeat does not rescue.
 *   6. What a rescued mate changes.  Its mf_place_t becomes { j, 1 - s, start, start + L, votes = 0, windows as the vote left them }:
 *      votes == 0 on a placed row is what marks a rescue.  Its mf_score_t is the winning candidate's.  From there on it counts
 *      everywhere an accepted placed read counts -- base depth, forward / reverse / over_begin / over_end, the score sums and its
 *      histogram bin, the pile-up -- whatever max_permille says: rescue_permille is its cut.  It leaves unplaced[0] if it passed, else
 *      unplaced[1].  The identities of the verification section keep holding with n_reads being both sets' reads.  The pass bits are not
 *      touched, and the paired call has no keep mode.
 *   7. Per pair: mf_pair_t { kind, insert }.  MF_PAIR_NONE: no mate is settled.  MF_PAIR_PROPER.  MF_PAIR_DISCORDANT: both are settled
 *      and the pair is not proper.  MF_PAIR_RESCUED_1 / _2: mate 1 / mate 2 was rescued.  MF_PAIR_SINGLE_1 / _2: mate 1 / mate 2 is
 *      settled and the other is neither settled nor rescued.  insert is -1 for NONE and SINGLE_*, and for a discordant pair without one;
 *      a rescued pair's insert is the winning d.
 *   8. Per record: mf_pair_record_t.  cross counts the pairs whose settled mates lie on different records, at mate 1's record;
 *      discordant counts the other discordant pairs, on their common record; proper likewise.  rescued and single are counted at the
 *      settled mate's record.  insert_sum runs over the proper and the rescued pairs.  pairs_none: one uint64_t, the pairs of kind NONE.
 *      Sum(proper + discordant + cross + rescued + single) + pairs_none == n_reads of one set.
 *   9. With rescue = 0 every output except the pair outputs equals what two mf_verify calls give, added up.
 * Outputs: bits1 / bits2, place1 / place2, score1 / score2 (per read of either set), pairs (n_reads entries), base_depth, place_records,
 * pileup, consensus, pileup_records, score_records as mf_verify gives them, pair_records (R entries), pairs_none, unplaced (2 u64, over
 * both sets), stats (both passes: counts and times added).  Every output is optional; the pile-up counters are allocated only when
 * pileup, consensus or pileup_records is asked for.
 * MF_E_ARG before any device work: a NULL handle; a protein set; unequal n_reads; sets on different devices; the insert and permille
 * ranges above; rescue other than 0 or 1; min_depth == 0.  Placement's limits apply. */
#define MF_RESCUE_MAX 4096
enum { MF_PAIR_NONE = 0, MF_PAIR_PROPER = 1, MF_PAIR_DISCORDANT = 2, MF_PAIR_RESCUED_1 = 3, MF_PAIR_RESCUED_2 = 4, MF_PAIR_SINGLE_1 = 5,
       MF_PAIR_SINGLE_2 = 6 };
typedef struct { uint32_t kind; int32_t insert; } mf_pair_t;
typedef struct { uint64_t proper, discordant, cross, rescued, single, insert_sum; } mf_pair_record_t;
int mf_place_pairs(const mf_kmerset *ks, const mf_reads *reads1, const mf_reads *reads2, uint32_t threshold, int mode, uint32_t min_depth,
              uint32_t max_permille, uint32_t min_insert, uint32_t max_insert, int rescue, uint32_t rescue_permille, uint32_t *bits1,
              uint32_t *bits2, mf_place_t *place1, mf_place_t *place2, mf_score_t *score1, mf_score_t *score2, mf_pair_t *pairs,
              uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup, uint8_t *consensus,
              mf_pileup_record_t *pileup_records, mf_score_record_t *score_records, mf_pair_record_t *pair_records, uint64_t *pairs_none,
              uint64_t *unplaced, mf_filter_stats_t *stats);

/* ---- pairs with a band: mf_align_pairs is mf_place_pairs with `band` and `extend` behind max_permille, and with the aligning family's
 * outputs in place of the scores: both mate sets aligned, and a rescued mate aligned around its seed.  So one consensus has both the
 * rescued mates -- the only reads over a diverged stretch -- and the indels and the growing ends the banded alignment calls there.
 * Nucleotide sets only.  ABI 5 still.  Nothing above changes; there is no keep mode, as in mf_place_pairs.
 * The rule.
 *   1. Each set is aligned exactly as mf_align_extended does it: filtered, placed by vote, aligned inside the band, cut at max_permille
 *      on edits per thousand columns.  Both sets add into ONE set of counters: base depth, the place counters, the pile-up, the indel
 *      table, the insertion pile, the extension pile, the align sums and the histogram.  A mate is SETTLED when it is placed by vote and
 *      the aligned cut accepts it.
 *   2. Insert, PROPER, rescue target, candidates and winner are rules 2 - 5 of the pairs section, word for word.  All of them go by the
 *      mf_place_t rows (start, end: the vote's diagonal), not by ref_begin / ref_end.  The candidates are scored UNGAPPED by the
 *      verification rule; rescue_permille and compared >= k apply to the ungapped candidate; a tie rescues nothing.  The seed is
 *      ungapped: a mate with an indel well inside it is found only through the matches of its longer side, the other side lying shifted
 *      on the seed's diagonal, so it needs a looser rescue_permille than a mate without one.  The value is a policy choice, not measured.
 *   3. A rescued mate is then aligned as any placed read is: inside the 2 * band + 1 diagonals around the winning candidate's start, on
 *      record j and strand 1 - s, by the banded-alignment rule unchanged.  It is ACCEPTED whatever the alignment's permille:
 *      rescue_permille on the seed is its cut.  Its mf_place_t is { j, 1 - s, start, start + L, votes = 0, windows as the vote left
 *      them }; its mf_align_t is the alignment's.  From there on it adds everywhere an accepted aligned read adds: base depth over the
 *      clipped [ref_begin, ref_end); forward / reverse; over_begin / over_end by ref_begin / ref_end; the five align sums, `gapped` and
 *      the bin min(edits, 31); the pile-up of its diagonal steps; del / ins / ins_bases; the insertion pile in a gapped call; the
 *      extension pile in an extending call.  It leaves unplaced[0] if it passed, else unplaced[1].  The pair's insert is the winning d.
 *      Its clipped footprint is not empty: the seed compares at least k > band columns inside the record on diagonal 0 of the band, the
 *      path is monotone and ends within band columns of the seed's diagonal, so [ref_begin, ref_end) holds a column of the record; and
 *      whatever an alignment did, the two depth adds are clamped into [0, len] of the record.
 *   4. Identities.  At band == 0 (extend == 0, the gapped outputs NULL) every output mf_place_pairs also has equals that call's bit for
 *      bit; mf_align_t's compared / mismatches are mf_score_t's, its ref_begin / ref_end are start / end.  At rescue == 0 every output
 *      except the pair outputs equals two mf_align_extended calls added up.  The aligning section's identities hold with n_reads being
 *      both sets' reads (accepted == forward + reverse; sum(hist) == accepted + rejected; base_sum == the sum of the clipped footprints;
 *      the pile-up record's mismatches == the align record's), and the pair section's sum identity holds.
 * Outputs: mf_place_pairs's with align1 / align2 for score1 / score2, then indels, align_records, the four gapped and the four extended
 * outputs as mf_align_extended gives them, each over both sets; every output optional.  Which counters are allocated follows the
 * single-set calls: the pile-up counters with any pile-up, gapped or extended output, the insertion pile with a gapped or extended one,
 * the extension pile with extend > 0 and an extended one.
 * MF_E_ARG before any device work: everything mf_place_pairs refuses; band above 31 or not below k; extend above MF_EXTEND_MAX;
 * extension outputs with extend == 0.  MF_E_NOMEM names the size, as the gapped and extended calls give it.
 * Device memory: beside the single-set calls', one work slice per resident wave of the rescue (24 bytes a base of the longer set's
 * longest read: a rescue target need not pass), bounded whatever the number of pairs. */
int mf_align_pairs(const mf_kmerset *ks, const mf_reads *reads1, const mf_reads *reads2, uint32_t threshold, int mode, uint32_t min_depth,
              uint32_t max_permille, uint32_t band, uint32_t extend, uint32_t min_insert, uint32_t max_insert, int rescue,
              uint32_t rescue_permille, uint32_t *bits1, uint32_t *bits2, mf_place_t *place1, mf_place_t *place2, mf_align_t *align1,
              mf_align_t *align2, mf_pair_t *pairs, uint32_t *base_depth, mf_place_record_t *place_records, mf_pileup_t *pileup,
              uint8_t *consensus, mf_pileup_record_t *pileup_records, mf_indel_t *indels, mf_align_record_t *align_records,
              mf_pileup_t *ins_pile, uint8_t *gapped, uint64_t *gapped_starts, mf_gapped_record_t *gapped_records, mf_pileup_t *ext_pile,
              uint8_t *extended, uint64_t *extended_starts, mf_extend_record_t *extend_records, mf_pair_record_t *pair_records,
              uint64_t *pairs_none, uint64_t *unplaced, mf_filter_stats_t *stats);

/* Options that select which kernels a filter pass runs (process-wide; every variant gives the same bits and is parity-tested):
 *   pass=default|split|serial   adapt=0|1   finish_streams=0|1|2   screen_streams=1|2   split_pipe=0|1   exact_co=0|1
 * and, read when a k-mer set is BUILT (ABI 5; every form gives the same bits -- tests force them on small baits):
 *   front=-1|0|1|2|3|4 (which screen; -1: by the bait's size)   canon=-1|0|1 (one canonical key per bait s-mer in the screen's tables)
 *   s8_finish=-1|0|1 (k < 28: threshold-1 passes through screen + finish)   front2_log2b=0|6..24   front3_log2b=-1|0|6..27
 *   (MF_FRONT, MF_CANON, MF_S8_FINISH, MF_FRONT2_LOG2B, MF_FRONT3_LOG2B under MF_ENV_KNOBS=1); expect_files=0|1, short_lived=0|1 (ABI 4);
 *   depth_index=0|1, read when a set's depth tables are built (MF_DEPTH_INDEX): 1 counts depth per table slot instead of per
 *   representative position -- the same results, kept to measure the scattered atomics against.
 * The library does NOT take these from the environment in a production process: the MF_PASS, MF_ADAPT, MF_FINISH_STREAMS,
 * MF_SCREEN_STREAMS, MF_SPLIT_PIPE and MF_EXACT_CO variables only count when MF_ENV_KNOBS=1 is set beside them (tests, bench.py,
 * profiling scripts).  ABI 3. */
int mf_set_option(const char *name, const char *value);

/* What the calling thread's last successful mf_filter_fastq_files / _on call did (ABI 3).  path: which
 * of the library's two ingest paths took the input. */
enum { MF_INGEST_PATH_HOST = 0, MF_INGEST_PATH_DEVICE = 1 };
typedef struct {
    int32_t  path, n_devices, consumers, reserved;
    uint64_t input_bytes;          /* bytes of the input files as they lie (compressed, if .gz) -- device path only */
    uint64_t text_bytes;           /* bytes of FASTQ text they hold -- device path only */
    uint64_t records;              /* FASTQ records cut from it, both mates */
    double   seconds;              /* wall time of the call */
    double   decode_busy_seconds;  /* time with at least one inflate kernel running, summed over devices and mates (0: no .gz) */
    uint64_t pool_bytes_peak;      /* this call's device buffers at most, on any one device */
    uint64_t device_bytes_peak;    /* everything in use on a device at most (hipMemGetInfo after each piece) */
    uint64_t chunks, chunks_linked, gaps, gap_bytes;   /* speculative chunks; those the link step took; stretches (bytes of text) the host bridged */
} mf_ingest_stats_t;
int mf_last_ingest_stats(mf_ingest_stats_t *out);

/* The device ingest path keeps device buffers, pinned staging buffers and the consumers' read sets of a call for the process's next
 * call (allocating them anew costs a call a tenth of a second and more).  mf_release_cached() gives all of it back to the runtime;
 * *bytes (may be NULL) receives the device bytes released.  Call it between calls, not during one.  The library calls the same code by
 * itself whenever one of its own allocations finds a device full.  ABI 4. */
int mf_release_cached(uint64_t *bytes);

/* Host-to-device copy rate of this box in GB/s (pinned memory, `bytes` per copy, best of `reps`): the
 * roof of the device ingest path, whose input goes up over PCIe as it lies on disk. */
int mf_h2d_bandwidth(int device, size_t bytes, int reps, double *gb_per_s);

/* ---- FASTQ quality filter: the reference's `filter/filter_v2` (filter/filter_bin/src/main.rs:14-329),
 * the stage that runs on the raw reads before this path (SURVEY.md 8f "next" #2).  Same rules, same
 * output bytes: cut [start, end), drop reads with more than `ns` 'N' or with at least
 * (len * limit) quality bytes <= `quality`, optional de-duplication on mate 1 (first occurrence
 * kept; SipHash-1-3 like Rust's DefaultHasher), stop once `trim` bases have been kept,
 * `truncate_only` skips the tests.  fq1 NULL = standard input; out2 NULL with fq2 set = standard
 * output.  Counting and hashing run on the GPU over the raw FASTQ text; the order-dependent rules
 * are applied on the host.  Regular .gz input files take the device ingest path (inflate, line index,
 * counting, hashing, the de-duplication set, the decisions and the formatting of the kept records on
 * the GPU; mf_last_ingest_stats tells), everything else the host pipeline; MF_QUAL_INGEST=device|host
 * forces either for what both can take.  Same bytes either way.  *panicked is set when the reference would have aborted mid-file (cut
 * start beyond a string, invalid UTF-8): output up to that record is written, as the reference's
 * BufWriter flushes on unwind, and the CLI then exits 101. */
int mf_qualfilter_files(const char *fq1, const char *fq2, const char *out1, const char *out2,
                        uint64_t start, uint64_t end, uint64_t ns, uint32_t quality, float limit,
                        int dedup, uint64_t trim, int truncate_only, int device,
                        uint64_t *kept, uint64_t *total, int *panicked);

#ifdef __cplusplus
}
#endif
#endif /* MITOFILTER_H */
