/*
 * mdx.h — C ABI of libmdx.so, the MI355X-native damage-tabulation engine.
 *
 * The reference (ginolhac/mapDamage) has no FFI/plugin interface for this path; its seam is
 * the set of accumulator objects created in mapdamage/main.py:147-155 and the loop body
 * main.py:165-217 that feeds them.  Each entry point below names the reference interface it
 * replaces.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * Threading: one host thread drives one context; contexts are independent (one per GPU).
 * All work is enqueued on the context's HIP stream (mdx_set_stream lets the caller share a
 * stream with e.g. PyTorch); calls return after enqueueing unless stated otherwise.
 * Ownership: the caller owns every buffer it passes in; device memory allocated by the
 * library is released by mdx_destroy / mdx_batch_free.
 * Errors: functions return 0 (MDX_OK) or a negative code; mdx_last_error() gives text.
 */
#ifndef MDX_H
#define MDX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDX_ABI_VERSION 6   /* 6: mdx_stats_loglik, mdx_stats_run, mdx_stats_pmat (additions again: the number stays); mdx_set_strata, mdx_strata_groups, mdx_strata_kept, mdx_finish_merged, mdx_finish_merged_host, mdx_merged_words, mdx_lgd_copies (additions only: no structure and no existing call changed, so the number stays); mdx_fasta_index, mdx_set_reference_fasta, mdx_reference_fetch, mdx_host_threads, mdx_warm, mdx_*_patches_device, mdx_rescale_expand_device, mdx_mr_round, mdx_batch_fold, mdx_bgzf_deflate, mdx_gbam_rescale_slab / _write_rescaled / _record_name; 2: mdx_batch::seq_format, mdx_pack_seq, mdx_gbam_set_seq_format; 3: mdx_gbam_tell / _fixups, mdx_bam_seek; 4: mdx_batch::lowq (the struct grew by one pointer); 5: mdx_batch::libsort (another one), mdx_libsorts, mdx_gbam_view_flags / _set_flags */

#define MDX_OK 0
#define MDX_ERR_ARG (-1)          /* bad argument / unsupported configuration */
#define MDX_ERR_HIP (-2)          /* HIP runtime failure */
#define MDX_ERR_STATE (-3)        /* call order violated (e.g. tabulate before set_reference) */
#define MDX_ERR_MASK_INDEX (-4)   /* reserved, never returned: the IndexError of align.py:69-71 (a masked column beyond
                                     the gapped reference) needs a reference slice cut short by its contig end, and
                                     such a record is MDX_ERR_BAD_READ already (the reference raises at align.py:33) */
#define MDX_ERR_LGD_OVERFLOW (-5) /* more out-of-range fragment lengths than lgd_over_cap */
#define MDX_ERR_BAD_READ (-6)     /* record the reference cannot process: alignment past the
                                     contig end (pysam ValueError from align.py:33 / main.py:180),
                                     tid/library out of range, CIGAR/SEQ length mismatch */

#define MDX_ERR_UNSUPPORTED (-8)  /* mdx_gbam_* / mdx_gsam_*: something the GPU decode path does not take (use the host decoder, from mdx_gbam_tell / mdx_gsam_tell on) */
#define MDX_ERR_COMM (-7)         /* RCCL failure, or another rank of the communicator reported an error */

/* Optional hint in the `flag` column (a bit SAM does not define): every base quality of the record is at least
 * --min-basequal, so nothing of it can be masked (align.py:65-71 masks only qualities below the threshold).  The
 * kernel then skips the record's quality window loads.  The caller vouches for it (mdx_bam_qmin gives the lowest
 * quality of each record; mapdamage_amd.batch.mark_unmaskable sets the bit); without the bit nothing changes.
 * SAM defines FLAG bits 0..11 only, but a file may carry anything in its 16 bits: the decoders of this library
 * (mdx_bam_*, mdx_gbam_*, the SAM text parser) clear bits 14 and 15 (see MDX_FLAG_HAS_QUAL) of what they read, and a caller that packs its own flag
 * column must do the same unless it vouches for the record. */
#define MDX_FLAG_QUAL_ABOVE_MIN 0x8000
/* A second hint, bit 14 (round 6): the record HAS base qualities — it holds at least one base and the first byte of its
 * quality string is not 0xFF (what `not read.qual` tests at main.py:185 and rescale.py:306).  The rescaling kernels then do
 * not fetch that byte to route the record (a scattered load per record: a tenth of the fused launch's time when no second
 * quality column is written, mdx_tabulate_rescale_patches_device); without the bit they look.  Set by the library where it
 * sees the qualities anyway: mdx_batch_upload (a batch with a quality column) and the device decoder; the decoders clear
 * bits 14 and 15 of what a file carries, and a caller that packs its own flag column does the same unless it vouches. */
#define MDX_FLAG_HAS_QUAL 0x4000

#define MDX_N_MIS_COLS 25         /* mapdamage/seq.py:6-30 without the derived "Total" */

typedef struct mdx_ctx mdx_ctx;

/* Per-run options: --length/--around/--min-basequal (mapdamage/config.py:143-166) and the
 * number of libraries (mapdamage/reader.py:47-50; 1 with --merge-libraries, reader.py:44-46). */
typedef struct {
    int32_t length;        /* L >= 1 */
    int32_t around;        /* A >= 0 */
    int32_t minqual;       /* 0..93; 0 disables masking */
    int32_t nlib;          /* >= 1 */
    int32_t lgd_max;       /* dense fragment-length histogram covers [0, lgd_max) */
    int32_t device;        /* HIP device ordinal */
    int64_t lgd_over_cap;  /* capacity (records) of the out-of-range length list */
} mdx_config;

/* The two forms of the `seq` column ("seq:u8[] (ASCII or 4-bit)").
 *   MDX_SEQ_ASCII  one byte per base, the characters pysam's read.query holds.
 *   MDX_SEQ_4BIT   two bases per byte, base i of the column in bits [4 (i & 1), 4 (i & 1) + 4) of byte i / 2 (the
 *                  low nibble first — BAM stores the high nibble first), code 1 = 'A', 2 = 'C', 4 = 'T', 8 = 'G' and 0 for
 *                  every other symbol.  Nothing is lost: the reference counts a read symbol only when it is exactly one
 *                  of "ACGT" (statistics.py:27, 101; rescale.py:228-246), every other one behaves alike.  seq_off and
 *                  n_bases keep counting bases; the column holds (n_bases + 1) / 2 bytes.  mdx_pack_seq converts;
 *                  mdx_gbam_set_seq_format makes the device decode path write this form straight from BAM's nibbles.
 *                  Such a batch runs through the packed kernels (half the SEQ and reference bytes, no LDS update per
 *                  plain match): the plain tabulation, --min-basequal (mdx_batch::lowq) and, with one library,
 *                  mdx_tabulate_rescale_device — tables in the LDS, reference below 4 Gbases; for anything else the
 *                  library unpacks it into a scratch column first and the results are the same bytes. */
#define MDX_SEQ_ASCII 0
#define MDX_SEQ_4BIT 1
/*   MDX_SEQ_4BITQ  MDX_SEQ_4BIT with --min-basequal folded in (align.py:53-73: a read column whose quality is below the
 *                  threshold turns into N / N — it counts its read base in the composition table, statistics.py:100-103, and
 *                  nothing else): a symbol whose quality is below the CONTEXT's threshold is stored as the complement of its
 *                  code (14, 13, 11, 7 for A, C, T, G; 15 for a symbol that is no base), every other nibble as in MDX_SEQ_4BIT.  The packed masked kernel reads
 *                  nothing but this column — no quality byte, no bitmap.  Made by the library: mdx_batch_upload and the device
 *                  decoder (mdx_gbam_set_min_basequal) hand such a column over when the context has a --min-basequal,
 *                  mdx_tabulate_host folds on the copy stream; a MDX_SEQ_4BIT batch with qualities (or a bitmap, `lowq`) is
 *                  folded into a scratch column in front of every launch.  The column belongs to the context whose threshold
 *                  made it (a context without one refuses it). */
#define MDX_SEQ_4BITQ 2

/* One batch of alignment records as SoA columns: exactly what main.py:165-217 reads from each
 * pysam.AlignedSegment.  `seq` is the full SEQ (soft clips included); `qual`
 * raw Phred (BAM convention, first byte 0xFF = absent) or NULL; `cigar` BAM-encoded len<<4|op.
 * Limits of one batch: fewer than 2^30 records, at most 4 GiB of bases (32-bit seq_off); larger inputs are
 * fed as several batches (the context accumulates).  n_bases must be exact: it bounds the 8/12-byte window
 * loads of the kernels (no byte outside [seq, seq + n_bases) is read). */
typedef struct {
    int64_t n_reads;
    int64_t n_cigar;       /* == cigar_off[n_reads] */
    int64_t n_bases;       /* == seq_off[n_reads]   */
    const uint16_t *flag;
    const uint16_t *lib;
    const int32_t *tid;
    const int32_t *pos;
    const int32_t *tlen;
    const uint32_t *cigar_off; /* n_reads + 1 */
    const uint32_t *cigar;
    const uint32_t *seq_off;   /* n_reads + 1 */
    const uint8_t *seq;
    const uint8_t *qual;       /* may be NULL */
    int32_t seq_format;        /* MDX_SEQ_ASCII (0), MDX_SEQ_4BIT or MDX_SEQ_4BITQ */
    int32_t reserved;          /* 0 */
    /* Optional, device batches only, used with --min-basequal and a MDX_SEQ_4BIT column: bit i & 31 of 32-bit word i / 32 =
     * qual[i] is below the context's --min-basequal (align.py:65-71; 0xFF — no qualities — is not); (n_bases + 31) / 32 words.
     * A caller that has the bits spares the library the pass over the quality column when it folds the mask into a scratch
     * copy of the column in front of the launch (MDX_SEQ_4BITQ).  NULL: folded from `qual`.  The library's own batches
     * (mdx_batch_upload, the device decoder) are MDX_SEQ_4BITQ already and leave this NULL. */
    const uint8_t *lowq;
    /* Optional, device batches only, used when the context has several libraries and the seq column is 4-bit: the
     * per-record columns bucketed by library (reader.py:47-50, statistics.py:12-20 — the tables are keyed by library, a file
     * interleaves them): an opaque device blob.  The packed kernel then counts all libraries in ONE launch, one after the
     * other, each over its own records.  NULL: the library sorts in front of every launch (mdx_libsorts counts those).
     * mdx_batch_upload fills it in, mdx_batch_free releases it; a caller that builds mdx_batch itself leaves it NULL. */
    const uint8_t *libsort;
} mdx_batch;

/* ASCII SEQ bytes -> the MDX_SEQ_4BIT column (host buffers; `packed` holds (n_bases + 1) / 2 bytes; `threads` host
 * threads, 0 = all).  What main.py:180-205 and statistics.py:22-35 do with a read symbol depends only on which of
 * "ACGT" it is, if any. */
int mdx_pack_seq(const uint8_t *ascii, int64_t n_bases, uint8_t *packed, int32_t threads);

int mdx_abi_version(void);
const char *mdx_strerror(int code);

/* Replaces the construction of MisincorporationRates / DNAComposition / FragmentLengths
 * (mapdamage/main.py:147-155, statistics.py:10-20,59-73,107-115): zeroed device accumulators. */
int mdx_create(const mdx_config *cfg, mdx_ctx **out);
void mdx_destroy(mdx_ctx *ctx);
const char *mdx_last_error(const mdx_ctx *ctx);

/* Use `hip_stream` (a hipStream_t) for all subsequent work; NULL = the context's own stream. */
int mdx_set_stream(mdx_ctx *ctx, void *hip_stream);

/* Replaces pysam.FastaFile(options.ref) + the per-read ref.fetch(...).upper() calls
 * (main.py:115,180; align.py:32-33): uploads the contigs (original FASTA bytes, BAM tid order,
 * contig i = bases[contig_off[i] .. contig_off[i+1])) once and keeps them resident in HBM,
 * case-folded and symbol-classified by a device kernel.  Host pointers. */
int mdx_set_reference(mdx_ctx *ctx, const uint8_t *bases, const int64_t *contig_off, int32_t n_contig);

/* The same from the FASTA file itself: replaces pysam.FastaFile(options.ref) (main.py:115 — htslib's faidx, which reads
 * `<fasta>.fai` and builds it when the file has none) and the fetches behind it (main.py:180, align.py:32-33).
 * mdx_fasta_index: makes sure `<fasta_path>.fai` exists (name, length, offset, linebases, linewidth per sequence, htslib's
 * format; lines of unequal length within a sequence are an error, as they are to faidx); err (may be NULL) receives the text.
 * mdx_set_reference_fasta: the sequences `names[0 .. n_contig)` (the BAM header's, in tid order: chrom lookup is by name,
 * main.py:175-180) become the resident reference.  The file's bytes go to HBM as they lie on disk, a piece at a time, and a
 * kernel takes the line ends out by the index's arithmetic — no pass over the bases on the host; pieces of the file that
 * hold none of the wanted sequences are not read.  lengths (may be NULL) receives the length of each; a name the index
 * lacks is MDX_ERR_ARG, or with missing_ok an empty contig (a record mapped to it is MDX_ERR_BAD_READ when it is met: the
 * reference fails in fetch at that read, not before).  A byte of the file belongs to one sequence: an index whose rows for two
 * wanted sequences share bytes (a hand-edited or foreign .fai) is MDX_ERR_ARG, the message naming both; rows that merely
 * touch are served.  Synchronous.
 * The file may be uncompressed or bgzip-compressed (BGZF; told by its first bytes, not by its name).  A BGZF file's index
 * holds offsets into the inflated text, as htslib writes them, and it has a second one, `<fasta_path>.gzi` (bgzip's block
 * index).  mdx_fasta_index makes sure both exist: a missing .fai is built from the text inflated on the host's threads — once —
 * and written together with the .gzi; a .gzi that exists is left alone.  mdx_set_reference_fasta sends the BGZF blocks that
 * hold bytes of the wanted sequences — no others — to HBM compressed and inflates, CRC-checks and strips them there; the block
 * table comes from the .gzi, or from a walk over the block headers when there is none or it does not fit the file.  A block
 * that does not inflate, whose ISIZE disagrees or whose CRC32 is wrong is MDX_ERR_ARG, the message naming the block's offset
 * in the file.  A plain (single-member) gzip file is neither: its text begins with 0x1f, not with '>'.
 * mdx_fasta_load_stats (introspection for tests and tools): what the calling thread's last mdx_set_reference_fasta read —
 * out[0] BGZF blocks of the file, out[1] blocks inflated on the device, out[2] slabs (BGZF) or pieces (uncompressed) uploaded,
 * out[3] bytes of the file uploaded. */
int mdx_fasta_index(const char *fasta_path, char *err, int32_t err_cap);
int mdx_set_reference_fasta(mdx_ctx *ctx, const char *fasta_path, int32_t n_contig, const char *const *names, int32_t missing_ok,
                            int64_t *lengths);
int mdx_fasta_load_stats(int64_t *out);
/* Introspection for tests: bases [start, end) of contig tid of the resident reference as the kernels see them — the letter
 * where ref.fetch(chrom, start, end).upper() (main.py:180) holds one of "ACGT", '-' for '-', 'N' for anything else.  Host
 * buffer of end - start bytes; synchronous. */
int mdx_reference_fetch(mdx_ctx *ctx, int32_t tid, int64_t start, int64_t end, uint8_t *out);

/* Copies a host batch into device memory owned by the library (for resident/benchmark use).
 * `dev` receives device pointers; release with mdx_batch_free. */
int mdx_batch_upload(mdx_ctx *ctx, const mdx_batch *host, mdx_batch *dev);
int mdx_batch_free(mdx_ctx *ctx, mdx_batch *dev);
/* A caller's own device batch under --min-basequal (align.py:53-73): a MDX_SEQ_4BIT column with qualities (or the bitmap
 * `lowq`) is folded into a scratch column in front of EVERY launch that counts it — a pass over column and qualities each
 * time (2.2 x the unmasked launch against 1.3 x).  mdx_batch_fold does it ONCE, in place: the batch's seq column takes the
 * mask into its nibbles and *dev_batch becomes MDX_SEQ_4BITQ — from then on it belongs to this context's threshold (another
 * context with another threshold must not be handed it: check_batch cannot tell).  Enqueued on the context's stream.  The
 * library's own batches (mdx_batch_upload, the device decoder) are folded when they are made. */
int mdx_batch_fold(mdx_ctx *ctx, mdx_batch *dev_batch);

/* Replaces the loop body main.py:165-217 for every record of the batch: flag filter
 * (reader.py:121-132), coordinates/flanks (align.py:14-35), CIGAR gapping with optional
 * quality masking (align.py:38-88), strand step (main.py:200-205), and the accumulator
 * updates (statistics.py:22-51,75-93,117-126).  Accumulates; may be called repeatedly.
 * _host: columns in (pageable) host memory, copied through two pinned bounce buffers of the context, the call
 * returns when the last column has left the caller's buffers; _device: columns already in HBM.
 * Several libraries: a 4-bit seq column is counted by one launch over the records bucketed by library (mdx_batch::libsort);
 * an ASCII one by one launch per group of libraries that fits the LDS, each over all records.  Transparently. */
int mdx_tabulate_host(mdx_ctx *ctx, const mdx_batch *batch);
int mdx_tabulate_device(mdx_ctx *ctx, const mdx_batch *batch);

/* The index mdx_sync reports for a bad record is its index within its batch plus this base (default 0): a caller
 * that enqueues several batches before it synchronises (mdx_tabulate_host returns as soon as the host columns are
 * staged; copies and kernels of consecutive batches overlap) sets the base to the number of records in front of each
 * batch and gets back an index in its own numbering.  The lowest such index of all batches since the last
 * mdx_sync / mdx_reset is reported. */
int mdx_set_record_base(mdx_ctx *ctx, int64_t base);

/* Waits for the stream and reports deferred per-read errors (MDX_ERR_BAD_READ ...);
 * *bad_read (may be NULL) receives the index of the first offending record of its batch. */
int mdx_sync(mdx_ctx *ctx, int64_t *bad_read);

/* Number of uint64 words of the packed canonical table block written by mdx_finish_device:
 * [ mis nlib*2*2*L*25 | comp nlib*2*2*(L+A)*4 | lgd nlib*2*2*lgd_max | n_kept | n_lgd_over ]. */
int64_t mdx_table_words(const mdx_ctx *ctx);

/* Writes the canonical tables (layout: mapdamage_amd/layout.py) into a *device* buffer of
 * mdx_table_words() uint64 — this context's own counts; mdx_finish_allreduce sums them across GPUs
 * (or the caller all-reduces the buffer itself, e.g. with torch.distributed). */
int mdx_finish_device(mdx_ctx *ctx, uint64_t *d_tables);

/* Replaces reading the `.data` dicts before `.write()` (main.py:229-231): synchronises and
 * copies the canonical tables to host memory.  lgd_over receives (lib, kind, strand, length)
 * quadruples for lengths >= lgd_max (at most lgd_over_cap); any pointer may be NULL.
 * With a communicator attached (mdx_comm_init / mdx_comm_adopt) the call is collective and returns the
 * totals over all ranks on every rank; lgd_over then receives the lists of all ranks in rank order (every rank is
 * bounded by the context's lgd_over_cap, so mdx_comm_size() x that many entries always suffice) and a buffer too
 * small for them is MDX_ERR_LGD_OVERFLOW, never a shortened list. */
int mdx_finish(mdx_ctx *ctx, uint64_t *mis, uint64_t *comp, uint64_t *lgd, int64_t *lgd_over,
               int64_t lgd_over_cap, int64_t *n_lgd_over, int64_t *n_kept);

/* Cross-device reduction (SURVEY.md §8b "finish() performs cross-device reduction", §8e).  The reference has no
 * counterpart (it is a single process); what makes the reduction legal is that every accumulator update is a
 * `+= 1` (statistics.py:30,35,40,103,124,126).  One context per GPU / per process; records are sharded over
 * the contexts with no data-path exchange, and the tables are summed with one ncclAllReduce(ncclUint64, ncclSum)
 * over xGMI on the context's stream.  librccl.so.1 is resolved at run time (dlopen) by the first of these calls;
 * a process that never calls them does not need RCCL.
 *   mdx_comm_unique_id  rank 0 obtains the 128-byte rendezvous id (ncclGetUniqueId) and hands it to the other
 *                       ranks by any means (MPI, a file, torch.distributed's store);
 *   mdx_comm_init       every rank: ncclCommInitRank on the context's device (collective, blocks until all joined);
 *   mdx_comm_adopt      alternatively use an ncclComm_t the caller already owns (not destroyed by mdx_destroy);
 *   mdx_finish_allreduce  mdx_finish_device + in-place all-reduce of the packed block: every rank ends up with
 *                       the totals in its device buffer.  Enqueued on the context's stream; collective.
 * With a communicator attached, mdx_finish itself performs the reduction: an error flag is agreed on first (a rank
 * whose mdx_sync fails makes every rank return — MDX_ERR_COMM on the healthy ones — instead of leaving them in
 * the collective), then the tables are all-reduced and the out-of-range length lists all-gathered in rank order. */
#define MDX_COMM_ID_BYTES 128
int mdx_comm_unique_id(uint8_t *id /* MDX_COMM_ID_BYTES */);
int mdx_comm_init(mdx_ctx *ctx, const uint8_t *id, int32_t nranks, int32_t rank);
int mdx_comm_adopt(mdx_ctx *ctx, void *rccl_comm, int32_t nranks, int32_t rank);
int mdx_comm_size(const mdx_ctx *ctx);   /* 0 = no communicator attached */
/* The ranks RCCL itself counts in the attached communicator (ncclCommCount; 0 = none attached, < 0 = error): what a
 * benchmark line quotes as proof that the collective ran over that many ranks. */
int mdx_comm_count(mdx_ctx *ctx);
int mdx_finish_allreduce(mdx_ctx *ctx, uint64_t *d_tables);

/* Strata: the tables per (library, group of reference sequences) in one pass.  mapDamage 2.0 keyed its tables by reference
 * sequence as well (the `Chr` column of its misincorporation.txt); the reference snapshot merges the sequences (the hidden
 * --merge-reference-sequences of mapdamage/config.py is all that is left of the choice), so a user who wants mitochondrion
 * against nuclear genome, or every contig of an assembly, filters the file once per sequence.  Here a stratified context is
 * an ordinary one created with nlib = libraries x n_groups; the table of a record is lib * n_groups + group_of_tid[tid].
 *   mdx_set_strata     after mdx_create, before the first tabulation (MDX_ERR_STATE once records were counted; mdx_reset
 *                      lifts that).  group_of_tid: host, n_contig entries in [0, n_groups) — n_contig the reference's number
 *                      of sequences (checked at the first tabulation).  cfg.nlib no multiple of n_groups: MDX_ERR_ARG.
 *                      The key is made on the device, in front of every launch, into a scratch column of the context (8 bytes
 *                      per record); the batch's lib column — which keeps naming the LIBRARY, below cfg.nlib / n_groups — is
 *                      not written.  A record whose library is 0xFFFF or not below the number of libraries keeps 0xFFFF:
 *                      MDX_ERR_BAD_READ at mdx_sync if the flag filter keeps it, as in any context.  mdx_batch_upload on a
 *                      stratified context buckets the resident batch by stratum (mdx_batch::libsort), so set the strata first.
 *                      The fused calls (mdx_tabulate_rescale_*) count one library and refuse such a context (MDX_ERR_ARG).
 *   mdx_set_strata_regions  the group from a set of genomic regions (a BED file) instead of the sequence alone: on-target
 *                      against off-target of a capture panel, without a `samtools view -L` in front.  A record occupies
 *                      [pos, pos + max(1, reference bases of its CIGAR)) — M D N = X consume, clips and insertions do not
 *                      (htslib's bam_endpos) — and takes the group of the first interval of its sequence it shares a base
 *                      with (start < rec_end && end > rec_pos); rest_group where there is none, or where tid is outside
 *                      [0, n_contig).  The intervals of sequence t are iv_off[t] .. iv_off[t + 1] of the parallel arrays
 *                      iv_start, iv_end, iv_group (host; 0-based, half-open), sorted and disjoint within a sequence
 *                      (iv_end[k] <= iv_start[k + 1]): the key kernel binary-searches the slice.  MDX_ERR_ARG, with a
 *                      message naming the first offending interval, for offsets that decrease, an interval that is not
 *                      0 <= start < end, one that begins before its predecessor ends, a group or rest_group outside
 *                      [0, n_groups).  State rules, cfg.nlib, n_contig, mdx_batch_upload and the fused calls as for
 *                      mdx_set_strata.  A context has tid strata or region strata: calling the other kind is
 *                      MDX_ERR_STATE.  The arrays are copied to the device and stay there for the context's life.  The
 *                      flag filter is unchanged: a record it drops gets a key and is not counted in mdx_strata_kept.
 *   mdx_set_strata_damage  the group from what the record itself shows, for the conditional substitution analysis that tells
 *                      endogenous molecules from modern contamination (is damage at one end of a molecule associated with
 *                      damage at its other end?): four groups, 0 none, 1 5p, 2 3p, 3 both.  A record is 5p-damaged if
 *                      MisincorporationRates.update(read, seq, refseq, "5p", library) (statistics.py:22-35, as called from
 *                      main.py:185-212) would add to C>T at an index below `positions`, 3p-damaged if the "3p" call would add
 *                      to G>A there — C>T with single_stranded != 0.  Everything that shapes those calls shapes the rule:
 *                      terminal soft clips are no part of the query, hard clips are ignored, the gap columns of insertions
 *                      and deletions are positions, a reverse-strand record is reverse-complemented first, an N operation
 *                      misaligns the columns behind it as align.py:76-88 does, under --min-basequal a column below the
 *                      threshold is N / N (a record without qualities is not masked), and only the exact symbols match.  The
 *                      key kernel reads the record's CIGAR, a few SEQ symbols per end (all three forms of `seq`; qual or lowq
 *                      only where a column shows the substitution) and the resident reference: mdx_set_reference must have
 *                      been called before the first tabulation and before mdx_batch_upload (MDX_ERR_STATE).  A tid outside
 *                      the reference or a window beyond its sequence: group none, reported by the tabulation if kept.
 *                      cfg.nlib no multiple of 4, positions outside [1, cfg.length]: MDX_ERR_ARG.  State rules, the flag
 *                      filter, the fused calls and "one kind per context" as above.
 *   mdx_set_strata_pmd  the group from the record's post-mortem damage score (PMDS; Skoglund et al. 2014, PNAS 111:2229): the
 *                      log-likelihood ratio, over the whole alignment and with the base qualities, that the read carries
 *                      deamination damage.  n_thresholds + 1 groups: a record's group is the number of thresholds its score
 *                      reaches.  The rule, per record in its TRUE alignment (an N operation does not shift the columns behind
 *                      it): the query is SEQ without its terminal soft clips, nq bases q = 0 .. nq - 1; z5 = q + 1 and
 *                      z3 = nq - q for a forward record, the other way round for a reverse one; only the columns of M = X add
 *                      terms — in the molecule's orientation (a reverse record complemented) a 5p term at z5 where the
 *                      reference holds C and the read C (match) or T (mismatch), a 3p term at z3 where the reference holds G
 *                      and the read G or A (single_stranded: C and C or T again: a C column then adds both); exact symbols only.
 *                      terms[mismatch][min(z, 256) - 1][quality column] is the caller's table of the terms, 2^24 to the unit
 *                      (mapdamage_amd/pmd.py term_table builds it from D_z = p (1-p)^(z-1) + C and eps_q = 10^(-q/10) / 3);
 *                      the quality column is min(quality, 93), or 94 (eps = 0) for a record without qualities (no qual
 *                      column, or 0xFF as the record's first quality).  The score is the int64 sum of the record's terms —
 *                      exact, whatever the order —, thresholds_fx the thresholds in the same unit (ceil(t 2^24)), strictly
 *                      increasing, 1 to 15 of them.  A tid outside the reference, a pos < 0 or a window beyond its sequence:
 *                      score 0, nothing read, reported by the tabulation if kept.  The key kernel reads every aligned base
 *                      (ASCII and MDX_SEQ_4BIT forms of `seq`), its quality and its reference base — some 250 bytes per
 *                      record, a group of 16 lanes per record: mdx_set_reference comes before the first tabulation and before
 *                      mdx_batch_upload (MDX_ERR_STATE), and a batch brings its qual column if the qualities are to count.
 *                      cfg.nlib no multiple of n_thresholds + 1, thresholds not increasing or not 1 to 15, a null pointer, or
 *                      a context with cfg.minqual > 0 (the decoders fold the mask into SEQ and may drop the quality column:
 *                      the score together with --min-basequal is not defined here): MDX_ERR_ARG.  State rules, the flag
 *                      filter, the fused calls and "one kind per context" as above.  The arrays are copied.
 *   mdx_strata_pmd_histogram  hist[cfg.nlib / n_groups][82] (host): the kept records of each library by their score, bin
 *                      clamp((S >> 23) + 41, 0, 81) — half units over [-20, 20), bin 0 what lies below, bin 81 what lies at
 *                      or above 20 — of this context's batches since mdx_create / mdx_reset.  Counted by the kernel that makes
 *                      the key (a resident batch that brings its buckets: by a launch of it for the histogram alone), so a
 *                      library's bins sum to its strata's mdx_strata_kept; synchronous.  MDX_ERR_STATE without PMD strata.
 *   mdx_strata_pmd_unqualified  *n (host): how many of those records were scored without qualities (eps = 0); synchronous.
 *   mdx_strata_pmd_keep_scores  on != 0: from the next keyed batch on the key kernel also leaves every record's score, as the
 *                      float32 a score tag holds (mdx_gbam_write_kept_tagged: the nearest float32 to the fixed-point S, ties to
 *                      even, times 2^-24; a record outside the reference 0.0) — a column of the context, of the batch keyed
 *                      last.  Off (the default): no column, no store.  MDX_ERR_STATE without PMD strata.
 *   mdx_strata_pmd_scores  out[n] (host): that column, n = the records of the batch keyed last (else MDX_ERR_ARG); synchronous.
 *                      MDX_ERR_STATE without PMD strata, with the switch off, or when the batch tabulated last was not keyed
 *                      (none since the switch; a resident batch that brought its buckets).
 *   mdx_strata_groups  n_groups, 0 for a context without strata
 *   mdx_strata_kept    kept[cfg.nlib] (host): the records the flag filter (reader.py:121-132) kept, per stratum, of this
 *                      context's batches since mdx_create / mdx_reset — the block's n_kept is one word for the whole run.
 *                      Counted by the kernel that makes the key; synchronous.  The strata sum to n_kept.
 * mdx_finish, mdx_finish_device and mdx_finish_allreduce need nothing new: the block holds cfg.nlib tables in stratum order.
 *   mdx_finish_merged  d_tables (device: a block of mdx_table_words(), from mdx_finish_device or all-reduced) -> d_merged
 *                      (device, mdx_merged_words() words, another buffer): the block of cfg.nlib / n_groups tables, the groups
 *                      of each library summed, the two tail words copied — what the run without strata would have counted.
 *                      Enqueued on the context's stream.  Without strata: a copy.
 *   mdx_finish_merged_host  the same of this context's own counts into host memory (mdx_merged_words() words), for a
 *                      caller without device buffers of its own: synchronises (deferred errors as mdx_sync), finalises and
 *                      sums in HBM, copies the sum.
 * Many tables: the launches take MDX_ML_MAX_LIBS (64) tables at a time, fewer on a device with fewer pools of blocks.  The
 * dense fragment-length histogram is kept in several copies to spread its atomics (32 for a context of few tables); their
 * number halves while the copies together would pass 1 GiB, down to one: 1 000 tables at the default lgd_max of 65 536 are
 * 2.1 GB.  mdx_lgd_copies: how many this context has (introspection).  More than 65 535 tables: MDX_ERR_ARG from mdx_create,
 * with a context to read the message from (the 16-bit library column names no more). */
int mdx_set_strata(mdx_ctx *ctx, int32_t n_groups, const int32_t *group_of_tid, int32_t n_contig);
int mdx_set_strata_regions(mdx_ctx *ctx, int32_t n_groups, int32_t n_contig, const int64_t *iv_off /* n_contig+1 */,
                           const int32_t *iv_start, const int32_t *iv_end, const int32_t *iv_group, int32_t rest_group);
int mdx_set_strata_damage(mdx_ctx *ctx, int32_t positions, int32_t single_stranded);
int mdx_set_strata_pmd(mdx_ctx *ctx, int32_t n_thresholds, const int64_t *thresholds_fx, const int32_t *terms /* [2][256][95] */,
                       int32_t single_stranded);
int mdx_strata_pmd_histogram(mdx_ctx *ctx, uint64_t *hist /* n_libraries x 82 */);
int mdx_strata_pmd_unqualified(mdx_ctx *ctx, uint64_t *n);
int mdx_strata_pmd_keep_scores(mdx_ctx *ctx, int32_t on);
int mdx_strata_pmd_scores(mdx_ctx *ctx, float *out, int64_t n);
int mdx_strata_groups(const mdx_ctx *ctx);
int mdx_strata_kept(mdx_ctx *ctx, uint64_t *kept);
int64_t mdx_merged_words(const mdx_ctx *ctx);
int mdx_finish_merged(mdx_ctx *ctx, const uint64_t *d_tables, uint64_t *d_merged);
int mdx_finish_merged_host(mdx_ctx *ctx, uint64_t *merged);
int mdx_lgd_copies(const mdx_ctx *ctx);

/* ---- Duplicate removal: later copies of a molecule get 0x400 in the flag column before the batch is counted, and the flag
 * filter (0xF04) of every launch, count and written file drops them.
 *
 * A record is EXAMINED if (FLAG & 0xF04) == 0 on the column as it stands, its library is below the context's libraries (on a
 * stratified context: cfg.nlib / n_groups — the batch's lib column, not the key), FLAG & 0x1 is clear, tid >= 0, pos >= 0 and
 * its CIGAR consumes a reference base.  Its ends are the unclipped ones: left = pos - the leading run of S and H, right = pos +
 * the reference span - 1 + the trailing run of S and H; a left below -2^31 or a right above 2^32 - 1 leaves the record
 * unexamined.  Two examined records are copies of one molecule if they agree in (library, tid, FLAG & 0x10, left, right)
 * (ends = 0, both) or in (library, tid, FLAG & 0x10, the 5' coordinate: left forwards, right on the reverse strand) (ends = 1);
 * nothing else is compared, and nothing is hashed in place of a field.  The first in the order of the marked batches' records
 * represents the molecule, every later one is marked — whatever the batches' sizes, the lanes' schedule or the table's size.
 *
 *   mdx_dedup_begin    after mdx_create, before the first mdx_dedup_mark: the set of signatures in HBM — 16 bytes per examined
 *                      record in a store that grows, and a table of 64-bit slots with a 32-bit count each, at most half full,
 *                      doubled (a rehash launch on the stream, no readback) when the records marked so far and the coming
 *                      batch's could pass that.  expected_records sizes the first table (0: a small one).  A second call
 *                      empties the set and takes the new `ends`.
 *   mdx_dedup_mark     enqueued on the context's stream: the batch's flag column — device memory the caller grants as
 *                      writable — gets 0x400 where the record is a later copy.  The batches marked are consecutive stretches
 *                      of one stream of records.  MDX_ERR_STATE without mdx_dedup_begin.
 *   mdx_dedup_counts   synchronous: per library the records examined, marked, left unexamined because paired, and left
 *                      unexamined for another reason (no position, no reference base, ends beyond their fields).  Records
 *                      the flag filter drops or whose library the context does not know are in none of them.
 *   mdx_dedup_histogram  synchronous: per library the molecules seen c times, bin c - 1 for c = 1..1023, bin 1023 for c >= 1024.
 *   mdx_dedup_info     synchronous: info[0] slots of the table, [1] times it has grown, [2] the longest walk of an insert (slots
 *                      looked at), [3] all walks summed, [4] the store's entries (the examined records), [5] bytes of HBM the
 *                      store and the table hold, [6] the records (or slots) a block of the stage's kernels takes, [7] the
 *                      records a round of its one-block prefix sum takes (tests: the sizes at which the kernels turn).
 * mdx_reset empties the set and the counters (the setting stays), mdx_destroy frees them.  MDX_TEST_DUP_SLOTS=<n> in the
 * environment: the first table's slots, for tests of growth and long walks.
 *
 * Limits: a batch of fewer than 2^30 records, as everywhere, and at most 2^30 records marked between mdx_dedup_begin (or
 * mdx_reset) and the end of the stream, whether examined or not: the table is sized by the records marked, never more than
 * half full, and has at most 2^31 slots (a record keeps its slot's index in 32 bits).  The mdx_dedup_mark that would pass
 * either returns MDX_ERR_ARG and marks nothing; the batches before it stand. */
int mdx_dedup_begin(mdx_ctx *ctx, int32_t ends, int64_t expected_records);
int mdx_dedup_mark(mdx_ctx *ctx, mdx_batch *device_batch);
int mdx_dedup_counts(mdx_ctx *ctx, uint64_t *out /* [n_libraries][4] */);
int mdx_dedup_histogram(mdx_ctx *ctx, uint64_t *out /* [n_libraries][1024] */);
int mdx_dedup_info(mdx_ctx *ctx, uint64_t *info /* [8] */);

/* ---- Depth of coverage of the counted records, gathered beside the tabulation: how much of the resident reference they
 * cover, how deep, and where (the rule: csrc/mdx_depth_key.h).
 *
 * A record is COUNTED if (FLAG & 0xF04) == 0 on the flag column as it stands (behind the record filters,
 * mdx_gbam_view_set_flags and mdx_dedup_mark), its library is below the context's libraries (on a stratified context:
 * cfg.nlib / n_groups), 0 <= tid < n_contig, pos >= 0, its CIGAR consumes a reference base and pos + refspan does not pass
 * the end of sequence tid.  A record that passes the first two checks and fails a later one is OUTSIDE: counted as such, it
 * adds nothing.  M, = and X cover their bases; D and N advance without covering (samtools depth without -J); I, S, H and P
 * neither advance nor break a covered stretch.
 *
 * The accumulator is a difference array in HBM: one int32 per base of the reference in its concatenated order and one more,
 * allocated in whole tiles — 4 bytes per base, 12.4 GB for a genome of 3.1 Gb.  An interval [s, e) of sequence t adds +1 at
 * off[t] + s and -1 at off[t] + e; the depth of a base is the prefix sum up to it.
 *
 *   mdx_depth_begin   after the reference is resident (else MDX_ERR_STATE): the zeroed accumulator; a second call zeroes it.
 *                     An allocation that fails is MDX_ERR_HIP with the size in the message.  A new reference releases the
 *                     accumulator: begin again.
 *   mdx_depth_add     enqueued on the context's stream: the intervals of a device batch's counted records, two atomics each,
 *                     and the counters.  Reads flag, lib, tid, pos and the CIGAR; writes nothing of the batch.  MDX_ERR_STATE
 *                     without mdx_depth_begin.
 *   mdx_depth_finish  synchronous; three launches (tile sums, a one-block scan of them, a pass that rebuilds the depths and
 *                     consumes them) that leave the accumulator as it is: it may be called again, and more batches added
 *                     behind it.  per_contig [n_contig][4]: counted records, covered bases (depth >= 1), aligned bases (the
 *                     sum of depths), the largest depth.  hist [1024]: bases at depth d in bin d for d <= 1022, bin 1023 for
 *                     d >= 1023; it sums to the reference's length.  counts [4]: counted records, outside records, intervals,
 *                     maximal runs of depth > 0.  Any pointer may be NULL.
 *   mdx_depth_runs    synchronous: the maximal runs of equal depth > 0 in reference order, end exclusive — the lines of
 *                     `bedtools genomecov -bg`.  *n = their number; cap too small: MDX_ERR_ARG, *n still set, nothing written.
 *   mdx_depth_fetch   introspection for tests, as mdx_reference_fetch: the depths of bases [start, end) of sequence tid.  The
 *                     sums in front of the tile that holds the sequence's first element come from the finish's first two
 *                     launches; the elements from there to `end` are copied and summed on the host.  (The sequence's own
 *                     elements alone would not do: its first one also holds the -1s of the reads that end with the sequence
 *                     in front.)
 *   mdx_depth_info    info[0] records a block of the add kernel takes, [1] elements of a tile, [2] tiles a round of the
 *                     one-block scan takes, [3] bytes of HBM held.
 * mdx_reset zeroes the accumulator and the counters, mdx_destroy frees them.  MDX_TEST_DEPTH_ROUND=<tiles> in the
 * environment, read at the mdx_depth_begin that allocates: a smaller info[2], for tests of the scan's round boundary.
 *
 * Limit: an element is an int32, so fewer than 2^31 records are added between mdx_depth_begin (or mdx_reset) and the end —
 * added, whether counted or not, which the host knows without a readback.  The mdx_depth_add that would pass it returns
 * MDX_ERR_ARG and adds nothing; the batches before it stand. */
int mdx_depth_begin(mdx_ctx *ctx);
int mdx_depth_add(mdx_ctx *ctx, const mdx_batch *device_batch);
int mdx_depth_finish(mdx_ctx *ctx, uint64_t *per_contig /* [n_contig][4] */, uint64_t *hist /* [1024] */, uint64_t *counts /* [4] */);
int mdx_depth_runs(mdx_ctx *ctx, int32_t *tid, int64_t *start, int64_t *end, uint32_t *depth, int64_t cap, int64_t *n);
int mdx_depth_fetch(mdx_ctx *ctx, int32_t tid, int64_t start, int64_t end, uint32_t *out);
int mdx_depth_info(mdx_ctx *ctx, uint64_t *info /* [4] */);

/* Depth on target: the depths of mdx_depth_* parted by the region strata of the context (mdx_set_strata_regions), without a
 * second pass over the records.  The rule of what counts and covers is unchanged; only the attribution of BASES is new: base
 * p of sequence t belongs to interval k of t iff iv_start[k] <= p < iv_end[k], and to the rest otherwise — every base of a
 * sequence without intervals too.  (The tables part RECORDS, by the first interval a record overlaps: a read that hangs over
 * an interval's edge adds its outside bases to the rest here.)  The intervals are the strata's as they stand, abutting
 * intervals of different groups apart.
 *
 * Synchronous: the tile sums and their scan as for mdx_depth_finish, then one pass (depth_regions_kernel) that rebuilds the
 * depths as the third launch of the finish does and consumes them as runs that also end where the interval changes.  The
 * accumulator stays as it is: the call may be repeated, and made between adds.
 *   per_interval [n_iv][4]       covered bases, aligned bases, smallest depth, largest depth of each interval, in the order of
 *                                the strata's columns
 *   per_group [n_groups][4]      bases, covered, aligned, largest depth: a group's row is the sum (the max) over its
 *                                intervals; the row of rest_group also holds the bases no interval covers and their numbers
 *   group_hist [n_groups][1024]  bases of the group at depth d, binned as mdx_depth_finish bins; the rest's bases in the row
 *                                of rest_group.  The rows sum to the histogram of mdx_depth_finish.
 * Any pointer may be NULL.  n_iv == 0 is valid: everything is the rest.
 * MDX_ERR_STATE without mdx_depth_begin or without region strata.  MDX_ERR_ARG, naming the interval, if one ends beyond its
 * sequence's length (mdx_set_strata_regions does not know the lengths), or if the strata name another number of sequences
 * than the reference has: nothing is launched.
 * The first call reads the intervals back, builds their columns in the accumulator's element coordinates (16 bytes per
 * interval) and allocates the words the pass writes (32 bytes per interval, 8 KiB per group); mdx_depth_info's bytes include
 * them from then on.  mdx_reset, mdx_destroy, a new reference and a new mdx_set_strata_regions release them. */
int mdx_depth_regions(mdx_ctx *ctx, uint64_t *per_interval /* [n_iv][4] */, uint64_t *per_group /* [n_groups][4] */,
                      uint64_t *group_hist /* [n_groups][1024] */);

/* ---- Allele counts and pseudo-haploid calls at listed sites, gathered beside the tabulation: what `samtools mpileup -l panel |
 * pileupCaller` makes of the file the run would otherwise have to write first (the rule: csrc/mdx_pileup_key.h).
 *
 * A record is COUNTED, OUTSIDE or ignored exactly as for mdx_depth_add.  The sites of a counted record are those of its tid with
 * 0-based position in [pos, pos + refspan); one walk of the CIGAR finds the operation that holds the site.  Under M, = or X the
 * site has a query base, which goes to the first of: Masked (inside the first mask5 query bases of the molecule's 5' end or the
 * last mask3 of its 3' end — the windows of mdx_gbam_set_kept_mask in mode MDX_MASK_ALL), Other (not exactly A, C, G or T; the
 * complemented nibbles of MDX_SEQ_4BITQ too), LowQual (the record has qualities and the base's is below min_basequal), or one
 * of eight base x strand counters, the base as stored and the strand by FLAG & 0x10.  Under D the site adds to Deletions, under
 * N nothing.  Twelve uint32 counters per site: A+ C+ G+ T+ A- C- G- T- Deletions LowQual Other Masked.  Libraries and groups
 * are summed.
 *
 * The call is a function of a site's counters, seed, tid and position alone — the same in one batch and in many, under any
 * schedule: the eligible counts are the two strands summed, with alleles only those of ref and alt, with single_strand only the
 * - strand's at a {C, T} site and only the + strand's at a {G, A} site (pileupCaller --singleStrandMode); fewer than min_depth
 * eligible bases: N.  z = the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * ((tid << 32 | position) + 1).  RANDOM: the
 * first base in A C G T order whose cumulative eligible count exceeds z % total.  MAJORITY: the base with the most eligible
 * bases, among k tied ones number z % k of them in A C G T order.
 *
 *   mdx_pileup_begin   after the reference is resident (else MDX_ERR_STATE): site_pos [site_off[n_contig]] 0-based, strictly
 *                      increasing inside a sequence's slice [site_off[t], site_off[t + 1]) and below that sequence's length;
 *                      alleles [n_sites][2] (ref, alt as 0 .. 3 for A C G T, different) or NULL.  MDX_ERR_ARG, naming the
 *                      site, for an unsorted, repeated or out-of-range one; for n_contig other than the reference's, no site,
 *                      2^31 sites or more, or a config outside its ranges (single_strand needs alleles).  Uploads the sites
 *                      and allocates the zeroed counters, 48 bytes per site (58 MB for a panel of 1.2 M sites); an allocation
 *                      that fails is MDX_ERR_HIP with the size.  A second call releases the first one's sites and counters: it
 *                      starts from zero.  A new reference releases them too: begin again.
 *   mdx_pileup_add     enqueued on the context's stream: the (record, site) pairs of a device batch's counted records, one
 *                      atomic each.  Reads flag, lib, tid, pos, the CIGAR and SEQ (all three forms) and, with min_basequal
 *                      above 0, the quality column if the batch brings one; writes nothing of the batch.  MDX_ERR_STATE
 *                      without mdx_pileup_begin.
 *   mdx_pileup_finish  synchronous; one launch (a lane per site) that leaves the counters as they are: it may be called again,
 *                      and more batches added behind it.  counters [n_sites][12]; refbase [n_sites]: the resident reference's
 *                      letter at the site, N for one that is not A, C, G or T; call [n_sites]: A C G T N ('.' under
 *                      MDX_PILEUP_CALL_NONE); depth [n_sites]: the sum of the eight base counters; counts [4]: counted records,
 *                      outside records, records over at least one site, pairs.  Any pointer may be NULL.
 *   mdx_pileup_info    info[0] pairs the add kernel's LDS list holds in a round, [1] records a block of it takes, [2] bytes
 *                      of HBM held, [3] sites.
 * mdx_reset zeroes the counters, mdx_destroy frees them.  MDX_TEST_PILEUP_LIST=<pairs> in the environment, read at
 * mdx_pileup_begin: a smaller info[0], for tests of the list's round boundary.
 *
 * Limit: a counter is a uint32 and a record adds at most one to it, so fewer than 2^31 records are added between
 * mdx_pileup_begin (or mdx_reset) and the end — added, whether counted or not, which the host knows without a readback.  The
 * mdx_pileup_add that would pass it returns MDX_ERR_ARG and adds nothing; the batches before it stand. */
#define MDX_PILEUP_CALL_NONE 0
#define MDX_PILEUP_CALL_RANDOM 1
#define MDX_PILEUP_CALL_MAJORITY 2
typedef struct {
    int32_t min_basequal;  /* 0..93 */
    int32_t mask5, mask3;  /* 0..255 query bases at the molecule's 5' and 3' end */
    int32_t call;          /* MDX_PILEUP_CALL_* */
    int32_t min_depth;     /* >= 1 */
    int32_t single_strand; /* 0 or 1; 1 needs alleles */
    uint64_t seed;
} mdx_pileup_config;
int mdx_pileup_begin(mdx_ctx *ctx, const mdx_pileup_config *config, const int32_t *site_pos, const int64_t *site_off /* [n_contig + 1] */,
                     int32_t n_contig, const uint8_t *alleles /* [n_sites][2] or NULL */);
int mdx_pileup_add(mdx_ctx *ctx, const mdx_batch *device_batch);
int mdx_pileup_finish(mdx_ctx *ctx, uint32_t *counters /* [n_sites][12] */, uint8_t *refbase, uint8_t *call, uint32_t *depth /* [n_sites] each */,
                      uint64_t *counts /* [4] */);
int mdx_pileup_info(mdx_ctx *ctx, uint64_t *info /* [4] */);

/* ---- Genotype likelihoods at the same sites, gathered by the same adds: what `angsd -GL 2 -doGlf 2 -sites panel` makes of the
 * file (GATK's model; the rule: csrc/mdx_pileup_key.h).
 *
 * A (record, site) pair adds exactly when it adds to one of the eight base x strand counters — Masked, Other, LowQual, Deletions
 * and N add nothing, so mask5 / mask3 and min_basequal shape the likelihoods as they shape the counts.  Its quality is
 * min(qual[q], 93), for a record without qualities noqual_quality.  table [94][3] holds, per quality, round(2^24 * x) for x =
 * log(1 - e), log((1 - e) / 2 + e / 6), log(e / 3) with e = min(0.75, 10^(-q / 10)): the term of an observed base b under a
 * genotype bb, under a heterozygous one that holds b, under any other.  A site's sums are int64 [2 strands][4 bases][3], row c
 * of them beside counter c, 192 bytes a site; the device only adds integers, so they are the same in one batch and in many,
 * under any schedule.  At the finish the eligible strands are those of the call (single_strand of mdx_pileup_config); for the
 * ten genotypes AA AC AG AT CC CG CT GG GT TT, logL = the sum over the four bases of the eligible strands' sums of the term
 * that the genotype gives the base, whatever the site's alleles.
 *
 *   mdx_pileup_likelihoods_begin   behind mdx_pileup_begin and in front of the first mdx_pileup_add (else MDX_ERR_STATE):
 *                      allocates and zeroes the sums; an allocation that fails is MDX_ERR_HIP with the size.  noqual_quality
 *                      1..93.  A later mdx_pileup_begin or a new reference releases them, mdx_reset zeroes them, mdx_destroy
 *                      frees them; mdx_pileup_info's bytes include them.  Called again it zeroes them and takes the new table.
 *   mdx_pileup_add     launches the add kernel's variant while the sums exist: three 64-bit atomics beside the counter's.  It
 *                      then reads the quality column, if the batch brings one, for the records that have qualities.
 *   mdx_pileup_likelihoods_finish  synchronous; one launch (a lane per site) that leaves the sums as they are.  sums
 *                      [n_sites][24]; gl [n_sites][10]: logL minus the site's largest, <= 0, in units of 2^-24 (natural
 *                      logarithm); best [n_sites]: the index of the first genotype at 0; bases [n_sites]: the eligible
 *                      strands' base counters summed — 0: ten zeros, best 0; counts [2]: pairs that added, those of them from
 *                      records without qualities.  Any pointer may be NULL.  MDX_ERR_STATE without the sums.
 *
 * Limit: the largest magnitude of the table, below 2^29, times the 2^31 records of the stage's limit is below 2^63: no sum
 * leaves its int64. */
int mdx_pileup_likelihoods_begin(mdx_ctx *ctx, const int64_t *table /* [94][3] */, int32_t noqual_quality);
int mdx_pileup_likelihoods_finish(mdx_ctx *ctx, int64_t *sums /* [n_sites][24] or NULL */, int64_t *gl /* [n_sites][10] */, uint8_t *best,
                                  uint32_t *bases /* [n_sites] each */, uint64_t *counts /* [2] */);

/* ---- The same likelihoods under a damage profile: the position-specific deamination rates of a misincorporation.txt inside
 * the error model (as ATLAS and snpAD have them), instead of mask5 / mask3 (the rule: csrc/mdx_pileup_key.h).
 *
 * A pair adds exactly when it adds above, with the same quality.  Its base has two distances in query bases of the stored query
 * without terminal soft clips, [qs, qe) — insertions count, D and N columns do not; the windows of mask5 / mask3, not the
 * alignment columns of misincorporation.txt —: z5 = q - qs + 1 and z3 = qe - q for a forward record, exchanged for a reverse
 * one; a distance below 1 (a CIGAR that disagrees with its SEQ) is taken as 1.  Each indexes row min(z, n_rows) - 1 of its end;
 * the last row is the pooled tail.  In stored orientation a forward record has ct = d5[z5], ga = d3[z3], a reverse record ct =
 * d3[z3], ga = d5[z5].  An observed C or T is the source s or the product t of the channel C>T with r = ct, an observed G or A of
 * G>A with r = ga; with Pss = (1 - r)(1 - e) + r e / 3 and Pst = r (1 - e) + (1 - r) e / 3 the table holds, per end, row and
 * quality, round(2^24 * x) for the nine x
 *   observed s:  log Pss (genotype ss), log(Pss / 2 + e / 6) (s and another), log(e / 3) (no s)
 *   observed t:  log(1 - e) (tt), log(Pst / 2 + (1 - e) / 2) (st), log Pst (ss), log((1 - e) / 2 + e / 6) (t and another, not s),
 *                log(Pst / 2 + e / 6) (s and another, not t), log(e / 3) (neither)
 * end 0 with the 5' C>T rates, end 1 with the 3' G>A rates.  A site's sums are int64 [2 strands][10 genotypes AA AC AG AT CC CG
 * CT GG GT TT], 160 bytes a site; a pair adds ten terms to its strand's row.  At the finish logL is the eligible strands' rows
 * summed.
 *
 *   mdx_pileup_likelihoods_damage_begin   behind mdx_pileup_begin and in front of the first mdx_pileup_add, as
 *                      mdx_pileup_likelihoods_begin, which it excludes within the same pileup: whichever of the two is called
 *                      second is MDX_ERR_STATE.  table [2][n_rows][94][9]; n_rows = K + 1, 2..255; noqual_quality 1..93.
 *                      Allocates and zeroes the sums and copies the table (n_rows * 13 536 bytes) to the device.  A later
 *                      mdx_pileup_begin or a new reference releases both, mdx_reset zeroes the sums, mdx_destroy frees them;
 *                      mdx_pileup_info's bytes include them.  Called again it zeroes the sums and takes the new table.
 *   mdx_pileup_add     launches the add kernel's third variant while these sums exist: ten 64-bit atomics beside the
 *                      counter's, the nine terms read from the table in device memory.
 *   mdx_pileup_likelihoods_finish   serves both models; in this one sums is [n_sites][20], everything else as above.
 *
 * Limit: every probability is at least e / 3, so no entry is larger in magnitude than the plain table's: the same bound. */
int mdx_pileup_likelihoods_damage_begin(mdx_ctx *ctx, const int64_t *table /* [2][n_rows][94][9] */, int32_t n_rows /* K + 1 */,
                                        int32_t noqual_quality);

/* Zero all accumulators (new run with the same options and reference). */
int mdx_reset(mdx_ctx *ctx);

/* Kernel timing with HIP events recorded on the launch stream around the tabulation kernel.
 * mdx_timing_read synchronises, returns the number of timed launches and their summed
 * duration since the last call, and clears the record. */
int mdx_timing_enable(mdx_ctx *ctx, int enable);
int mdx_timing_read(mdx_ctx *ctx, int64_t *n_launches, double *total_ms);

/* Replaces seqtk.comp() of the reference's native extension (mapdamage/seqtk/seqtk.c:55-143) as
 * used by composition.write_base_comp (mapdamage/composition.py:6-25): per-contig counts of
 * A, C, G, T (upper and lower case folded) of the resident reference.
 * counts: host buffer of n_contig * 4 uint64, order A, C, G, T.  Synchronous. */
int mdx_genome_composition(mdx_ctx *ctx, uint64_t *counts);

/* Quality rescaling, mapdamage/rescale.py (BASELINE configs[4]).
 * mdx_rescale_set_model replaces _get_corr_prob + the per-column floating-point work of
 * _rescale_qual_read (rescale.py:23-46, 228-246): `lut` [2][1+len5p+len3p][94] maps (substitution
 * 0 = C>T / 1 = G>A, position key, old Phred) to the new Phred; `term` [2][1+len5p+len3p] is the
 * per-column contribution to the MR tag.  Position key 0 = no correction, 1..len5p = position from
 * the 5' end, len5p+k = position -k from the 3' end (mapdamage_amd/rescale.py builds both with the
 * reference's own expressions).
 * mdx_rescale_host replaces _rescale_qual_core's loop (rescale.py:300-344) for a batch: record
 * routing, _rescale_qual_read, soft-clip re-attachment.  Host pointers; synchronous.  qual_out has
 * the layout of batch->qual; mr_raw[i] is the MR sum before its "%.5f" truncation (NaN when record i
 * is written unchanged); status[i]: 0 unmapped, 1 no qualities, 2 rescaled from both ends,
 * 3 rescaled from the 5' end only (inward-facing pair), 4 improperly paired (unchanged). */
int mdx_rescale_set_model(mdx_ctx *ctx, const uint8_t *lut, const double *term, int32_t len5p, int32_t len3p);
int mdx_rescale_host(mdx_ctx *ctx, const mdx_batch *batch, const int32_t *mtid, const int32_t *mpos,
                     uint8_t *qual_out, double *mr_raw, uint8_t *status);
/* The same for a batch resident in HBM (device pointers throughout, enqueued on the context's stream; errors surface
 * at mdx_sync), and — BASELINE configs[4], "rescaling fused into the same pass" — both results of one resident
 * batch in one call: the count tables (main.py:165-217) and the rescaled qualities (rescale.py:300-344) from the
 * same columns, uploaded once.  d_qual_out is a column of its own (n_bases bytes; it must not be the batch's quality
 * column: MDX_ERR_ARG), filled completely — the qualities of records written back unchanged included.
 * mdx_tabulate_rescale_device is one fused launch when the tabulation runs as the plain fast kernel (tables in the LDS,
 * all libraries in one launch, no --min-basequal, reference below 4 GiB) and the model has at most 31 window positions:
 * the tabulation kernel rescales the [S] M [S] records of at most 2 x --length aligned bases while it counts them and
 * lists the others for the rescale kernels behind it; otherwise — and with MDX_NO_FUSE=1 in the environment — it is
 * mdx_tabulate_device followed by mdx_rescale_device.  Either way the results are the same bytes.  A NaN in mr_raw
 * (record written back unchanged) is any NaN.
 * mdx_rescale_timing_read: time of the rescale launches (the rescale kernels with the copy of the quality column
 * they contain — after a fused launch: of the kernels that take the records it has listed; HIP events, like
 * mdx_timing_read for the tabulation kernel, which then times the fused kernel; enabled by mdx_timing_enable). */
int mdx_rescale_device(mdx_ctx *ctx, const mdx_batch *dev_batch, const int32_t *d_mtid, const int32_t *d_mpos,
                       uint8_t *d_qual_out, double *d_mr_raw, uint8_t *d_status);
int mdx_tabulate_rescale_device(mdx_ctx *ctx, const mdx_batch *dev_batch, const int32_t *d_mtid, const int32_t *d_mpos,
                                uint8_t *d_qual_out, double *d_mr_raw, uint8_t *d_status);
/* The same two calls with the rescaled qualities as a LIST instead of a second column (round 6): _rescale_qual_read changes a
 * few quality bytes of a read — the C>T / G>A columns near its ends (rescale.py:228-246) — and a caller that writes the
 * records back (rescale.py:266-273, 344) needs those bytes, not a copy of the hundred it leaves alone.  One entry per quality
 * byte whose value changes: index of the byte in the batch's quality column | new Phred << 32, in no particular order.  The
 * list comes in n_parts parts (a power of two; 256 and more for a launch of millions of records: thousands of wavefronts
 * appending to one list queue at one address): part p = d_patch[p * patch_cap ..], d_n_patch[p] (device; zeroed by the call)
 * its number of entries — which may pass patch_cap: the entries beyond are lost and the caller repeats the call with longer
 * parts (n_reads x (len5p + len3p) entries in all always suffice; the parts fill evenly).  Nothing else is written: of a
 * record that is written back unchanged no quality byte is read but its first (rescale.py:306).  mr_raw, status, the
 * summary, errors: as above.  mdx_rescale_expand_device: d_qual_out = the batch's quality column with a list applied (for
 * callers that want the column after all, and the tests; d_qual_out may be the column itself). */
int mdx_rescale_patches_device(mdx_ctx *ctx, const mdx_batch *dev_batch, const int32_t *d_mtid, const int32_t *d_mpos,
                               uint64_t *d_patch, int64_t patch_cap, int32_t n_parts, uint64_t *d_n_patch, double *d_mr_raw,
                               uint8_t *d_status);
int mdx_tabulate_rescale_patches_device(mdx_ctx *ctx, const mdx_batch *dev_batch, const int32_t *d_mtid, const int32_t *d_mpos,
                                        uint64_t *d_patch, int64_t patch_cap, int32_t n_parts, uint64_t *d_n_patch, double *d_mr_raw,
                                        uint8_t *d_status);
int mdx_rescale_expand_device(mdx_ctx *ctx, const mdx_batch *dev_batch, const uint64_t *d_patch, int64_t patch_cap, int32_t n_parts,
                              const uint64_t *d_n_patch, uint8_t *d_qual_out);
int mdx_rescale_timing_read(mdx_ctx *ctx, int64_t *n_launches, double *total_ms);
/* Calls of mdx_tabulate_rescale_device so far that ran as the fused launch (the others: two kernels). */
int64_t mdx_fused_launches(const mdx_ctx *ctx);
/* Kernel launches so far that ran as the packed kernel (a MDX_SEQ_4BIT batch in a plain tabulation or with --min-basequal:
 * one per call whatever the number of libraries — up to 64 libraries per launch, MDX_ML_MAX_LIBS, and as many as the
 * launch has pools of two blocks). */
int64_t mdx_packed_launches(const mdx_ctx *ctx);
/* ... and those of them that ran the packed kernel compiled for the default geometry: --length 70 --around 10, one library,
 * no --min-basequal (MDX_NO_GEO_SPEC=1 in the environment: none — the kernel that takes its geometry from its arguments). */
int64_t mdx_geo_spec_launches(const mdx_ctx *ctx);
/* Calls so far that bucketed their batch by library themselves (several libraries, a batch without mdx_batch::libsort). */
int64_t mdx_libsorts(const mdx_ctx *ctx);
/* The geometry of the context's last tabulation launch (introspection for tests; all zero before the first): out[0] blocks of
 * the grid, out[1] wavefronts per block, out[2] tiles of the call's whole batch, out[3] pools of blocks that share a tile
 * counter.  (A launch of the packed kernels over several libraries hands out the tiles of its own libraries' kept records, a
 * library's to the pools of that library; the split is made on the device and not reported: out[2] bounds it from above.)  MDX_TEST_CUS=n in the environment when the context is created sizes its launches as on a device
 * of n compute units (never more than the device has): few wavefronts then take many tiles each of a small batch. */
int mdx_last_launch_geometry(const mdx_ctx *ctx, int32_t out[4]);
/* The integer content of the `subs` dictionary that _rescale_qual_read fills through _record_subs
 * (rescale.py:82-143) and _print_subs logs (:159-192), accumulated over every mdx_rescale_host call
 * since mdx_rescale_set_model.  words (uint64), npos = 1 + len5p + len3p:
 *   [0, 4)                  subs["A"], ["C"], ["G"], ["T"]: reference bases of the rescaled reads' columns
 *   [4, 4 + 4*2*94)         [transition 0=CT,1=TC,2=GA,3=AG][0=before,1=after][Phred]: subs["CT-before"] ...
 *   [756, 756 + 2*npos*94)  [0=C>T,1=G>A][position key][old Phred]: occurrences of each rescaled column kind,
 *                           from which the host sums the "-pvals" terms (each is a function of that triple)
 * mdx_rescale_summary_words returns the number of words (0 before a model is set). */
int64_t mdx_rescale_summary_words(const mdx_ctx *ctx);
int mdx_rescale_summary(mdx_ctx *ctx, uint64_t *words);

/* Input sources (additions of ABI 6; every entry point that takes a path opens one of its own).  A source is the compressed
 * input opened once: a regular file — and "-" when fd 0 is one (`< x.bam`), from fd 0's current offset — is mapped as
 * before; anything else — a pipe, FIFO, character device or socket: "-", /dev/stdin, /dev/fd/N, a named pipe — is a stream,
 * read front to back, once, by a thread of the source's own into a window.  The window holds the bytes from the release
 * point on: a stream's consumer gives back what it will not read again (mdx_bam_next: the blocks it has inflated;
 * mdx_gbam_next: everything in front of mdx_gbam_tell's position, where a host decoder can take the stream up with
 * mdx_bam_seek), and the reader stops when it is 16 MiB ahead of that point, or as far ahead as a consumer has asked for if
 * that is farther (the device decoder: three slabs) — memory stays bounded however long the stream is.  Reading or seeking
 * in front of the release point is MDX_ERR_ARG with a message, never a wait.  A pipe's buffer is raised to what this
 * process may set (F_SETPIPE_SZ on the source's own descriptor).  The one-piece decode (mdx_bam_read_source) reads a stream
 * to its end: memory in proportion to the stream.  A stream that ends inside a block, a damaged block, an empty stream: the
 * same codes and texts as the same bytes in a file.
 *   mdx_source_open    *out is set even on failure (mdx_source_error says why; close it)
 *   mdx_source_peek    the first n bytes (fewer: the input is shorter), e.g. to tell SAM from BAM; a stream waits for them
 *   mdx_source_read    the next bytes in order (SAM text), the peeked ones included: how many, 0 at the end, -1 on error
 *   mdx_*_open_source  the handles take a reference of their own: the source may be closed behind them, and lives until the
 *                      last of them is closed (mdx_source_close, mdx_bam_close, mdx_gbam_close)
 * A caller that holds a descriptor opens "/dev/fd/N". */
typedef struct mdx_source mdx_source;
int mdx_source_open(const char *path, mdx_source **out);
const char *mdx_source_error(const mdx_source *source);
int mdx_source_is_stream(const mdx_source *source);
int mdx_source_peek(mdx_source *source, uint8_t *buf, int32_t n, int32_t *got);
int64_t mdx_source_read(mdx_source *source, uint8_t *buf, int64_t cap);
/* mdx_source_seek: the next mdx_source_read starts at byte `offset` of the input (MDX_ERR_ARG in front of a stream's release
 * point) — where a host SAM parser takes a stream up behind the device decoder (mdx_gsam_tell). */
int mdx_source_seek(mdx_source *source, int64_t offset);
void mdx_source_close(mdx_source *source);

/* Native BAM decoding (host side, no GPU involved).  Replaces opening and iterating a
 * pysam.AlignmentFile (mapdamage/reader.py:38, 83-96; pysam is not needed): the BGZF blocks are
 * inflated on `threads` host threads and every record is unpacked into the SoA columns of mdx_batch.
 * The handle owns all memory; mdx_bam_batch returns host views valid until mdx_bam_free.
 * `lib` is zero-filled (the caller maps read groups to libraries, reader.py:63-81, from rg_index:
 * per-record index into mdx_bam_rg_name(), -1 = no RG tag).  mtid/mpos are the mate fields used by
 * the rescale routing; has_mr flags records that already carry an MR tag (rescale.py:277). */
typedef struct mdx_bam mdx_bam;
int mdx_bam_read(const char *path, int threads, mdx_bam **out);
int mdx_bam_read_source(mdx_source *source, int threads, mdx_bam **out);
void mdx_bam_free(mdx_bam *bam);
const char *mdx_bam_error(const mdx_bam *bam);
const char *mdx_bam_header_text(const mdx_bam *bam);
int32_t mdx_bam_n_ref(const mdx_bam *bam);
const char *mdx_bam_ref_name(const mdx_bam *bam, int32_t i);
int64_t mdx_bam_ref_length(const mdx_bam *bam, int32_t i);
int mdx_bam_batch(const mdx_bam *bam, mdx_batch *view, const int32_t **mtid, const int32_t **mpos,
                  const int32_t **rg_index, const uint8_t **has_mr);
const uint8_t *mdx_bam_qmin(const mdx_bam *bam);     /* lowest quality per record (0xFF: none) */

/* Record filters (--min-mapq, --require-flags, --exclude-flags, --min-read-length, --max-read-length; none is a reference
 * option).  A record is dropped when (FLAG & require_flags) != require_flags, when (FLAG & exclude_flags) != 0, when
 * MAPQ < min_mapq (numeric: 255 passes any threshold), when l_seq < min_length, or when max_length > 0 and l_seq > max_length
 * — evaluated in that order, on the 16 flag bits as the file carries them; l_seq is the length of the SEQ field (0 for a
 * SAM '*'), not the CIGAR's query length.  A dropped record keeps its place in the batch and gets 0x200 OR-ed into its
 * entry of the flag column by the decoder, which the flag filter of every kernel (0xF04) drops: nothing downstream takes a
 * filter argument.  counts[6] = records read, then the records dropped by each of the five reasons (a record counts under
 * the first that drops it; every record of the input is evaluated, also those the flag filter drops anyway).
 * mdx_bam_apply_record_filter marks the flag column of a decoded mdx_bam (mdx_bam_read, every chunk of mdx_bam_next) and
 * ADDS to counts (may be NULL); NULL or all-zero filter: nothing is marked, counts[0] += the records.  It tests the flag
 * bits the decoder read from the file, not the column — marks made since (its own, --downsample's 0x200) are not looked at —;
 * every call counts the batch again, so one call per decoded batch. */
typedef struct mdx_record_filter {
    int32_t min_mapq;
    uint32_t require_flags, exclude_flags;
    int32_t min_length, max_length;
} mdx_record_filter;
int mdx_bam_apply_record_filter(mdx_bam *bam, const mdx_record_filter *filter, uint64_t counts[6]);
int32_t mdx_bam_n_rg(const mdx_bam *bam);
const char *mdx_bam_rg_name(const mdx_bam *bam, int32_t i);
const char *mdx_bam_qnames(const mdx_bam *bam, const uint32_t **offsets);

/* Streaming form of the same decoder, for files larger than host memory and to overlap decoding with
 * tabulation (the reference iterates its AlignmentFile record by record, mapdamage/main.py:165; here the
 * unit is a chunk of records).  mdx_bam_open parses the header (mdx_bam_stream_header: a record-less
 * mdx_bam for the accessors above, owned by the stream, whose mdx_bam_error also carries stream errors).
 * mdx_bam_next returns the complete records within the next chunk_bytes of uncompressed BAM data as a new
 * mdx_bam (caller frees with mdx_bam_free; independent of the stream), *out = NULL at end of file.  Records
 * come in file order; rg_index of a chunk indexes that chunk's own mdx_bam_rg_name().  One thread per
 * stream; chunks may be consumed on other threads. */
typedef struct mdx_bam_stream mdx_bam_stream;
int mdx_bam_open(const char *path, int threads, mdx_bam_stream **out);
int mdx_bam_open_source(mdx_source *source, int threads, mdx_bam_stream **out);
const mdx_bam *mdx_bam_stream_header(const mdx_bam_stream *stream);
int mdx_bam_next(mdx_bam_stream *stream, int64_t chunk_bytes, mdx_bam **out);
/* Points the stream at the BGZF block at compressed offset comp_off; the next chunk starts with the record `phase`
 * inflated bytes into that block (the pair mdx_gbam_tell hands out; 0, 0 of a file's first record block rewinds). */
int mdx_bam_seek(mdx_bam_stream *stream, int64_t comp_off, int64_t phase);
void mdx_bam_close(mdx_bam_stream *stream);
/* Rewriting a BAM (the `--rescale-only` output of mapdamage/rescale.py:285-365, which writes every record back
 * through pysam): with mdx_bam_stream_keep_raw(stream, 1) each chunk keeps its encoded records as they stood in
 * the file; mdx_bam_raw returns them (rec_off[i] = offset of record i's block_size field, rec_off[n] = end);
 * mdx_bam_patch_rescaled writes the chunk's records to `out` (capacity out_cap bytes: raw size + 7 per rescaled
 * record suffices), those with rescaled[i] != 0 with their QUAL replaced by qual_out[seq_off[i] ...] and an `MR:f`
 * tag (mr[i]) appended, every other byte unchanged. */
/* The BGZF writer on the device (round 6): replaces zlib's deflate behind pysam's AlignmentFile(..., "wb") for the output of the
 * rescaling pass (rescale.py:290-291, :344 — every record is written back; on sixteen host threads the output's blocks were
 * 2.1 of the pass's 3.5 seconds).  `data` (host, n bytes of encoded BAM: header or records, any cut) is cut into blocks of
 * 0xFF00 bytes, every block becomes one BGZF member — in four pieces, a lane per piece: LZ77 with one hash candidate that may
 * reach back into the piece in front, a dynamic Huffman code of the piece's own counts, a stored block where that is not
 * smaller, the pieces joined the way zlib's Z_SYNC_FLUSH joins blocks (csrc/mdx_deflate.h, held against zlib's inflate by
 * tests/test_inflate_core.py) —, and the members are written side by side to `out` (host; n + (n / 0xFF00 + 1) * 64 bytes
 * always suffice), *out_len their bytes.  No end-of-file marker.  Any inflater reads the result; it is not zlib's output bit
 * for bit (3 % larger than its level 6 on BAM records with qualities, smaller than its level 1).  2.9 GB/s of records in, host
 * buffer to host buffer (sixteen host threads at level 6: 0.63 GB/s).  Synchronous, on the context's stream. */
int mdx_bgzf_deflate(mdx_ctx *ctx, const uint8_t *data, int64_t n, uint8_t *out, int64_t out_cap, int64_t *out_len);
/* --rescale-only with the records never on the host (round 6; rescale.py:285-365).  The handle is configured with qualities
 * and mate columns and hands out ASCII seq columns (mdx_gbam_configure(.., want_qual = 1, want_mate = 1)); after every
 * mdx_gbam_next:
 *   mdx_gbam_rescale_slab   the slab's records through the context's rescale kernels (mdx_rescale_set_model first; the list
 *                           form, mdx_rescale_patches_device), the new quality bytes into the QUAL fields of the inflated
 *                           records in HBM, MR rounded as rescale.py:275-276 does, every record — rescaled ones with an MR:f tag
 *                           appended — laid out as the output stream in HBM and compressed there (mdx_bgzf_deflate's kernels): `out`
 *                           (host; the slab's inflated size + 7 bytes per record + 64 per member always suffice) receives BGZF
 *                           members only.  counts[0..5) += records by routing status (rescale.py:300-342).  A rescaled record
 *                           that has an MR tag already: MDX_ERR_BAD_READ, *mr_clash = its index in the slab (rescale.py:277-278;
 *                           mdx_gbam_record_name gives its name); a record the kernels cannot process: *mr_clash = -2 - index.
 *   mdx_gbam_write_rescaled the second half on its own, for a caller that ran the rescale kernels itself: patch list (device),
 *                           mr / rescaled per record (host).
 * The file's header is the caller's to write (mdx_bgzf_deflate takes any bytes), and the end-of-file marker. */
int mdx_gbam_rescale_slab(struct mdx_gbam *g, uint8_t *out, int64_t out_cap, int64_t *out_len, int64_t *counts, int64_t *mr_clash);
int mdx_gbam_write_rescaled(struct mdx_gbam *g, const uint64_t *d_patch, int64_t patch_cap, int32_t n_parts, const uint64_t *d_n_patch,
                            const float *mr, const uint8_t *rescaled, uint8_t *out, int64_t out_cap, int64_t *out_len, int64_t *mr_clash);
int mdx_gbam_record_name(struct mdx_gbam *g, int64_t index, char *buf, int32_t cap);
/* --write-kept: the records a run counted, handed on as BAM in the pass that counts them (not a reference option; what
 * `samtools view -q/-F/-L` or `pmdtools --threshold` behind the run would have written).  After every mdx_gbam_next, and behind the
 * tabulation launch of its view (mdx_tabulate_device):
 *   mdx_gbam_kept_bound     *bytes = an `out_cap` that always suffices for mdx_gbam_write_kept on the view handed out last: the
 *                           inflated bytes of the view's records (exact, from the chain of record offsets), 64 more per 0xFF00 of
 *                           them, and 64.
 *   mdx_gbam_write_kept     the view's records with (flag & 0xF04) == 0 in the flag column as it stands now (after the record
 *                           filter's 0x200 and whatever mdx_gbam_view_set_flags marked), in the file's order, each copied byte for
 *                           byte from its block_size field to its last tag byte, as BGZF members to `out` (host): no header, no
 *                           end-of-file marker, nothing at all for a view without such a record.  *n_written = the records,
 *                           *raw_bytes = their bytes before compression, *out_len = the members' bytes.
 *                           group_selected (host, one byte per group; NULL: every such record): only the records whose group is
 *                           listed — the context must be stratified (mdx_set_strata*) with n_groups groups, else MDX_ERR_ARG, and
 *                           its key column must be that of this very view: the view tabulated, and no other batch since, else
 *                           MDX_ERR_STATE.  A record without a library (key 0xFFFF) is never written with a selection.  The rule
 *                           is csrc/mdx_kept.h.
 * Sizes, their prefix sum (64-bit offsets) and the gather run on the device; sixteen bytes come back before the members do.  The
 * handle owns the scratch (sizes, offsets, tile sums, the stream, the selection), grown when a slab needs more and released by
 * mdx_gbam_close: no allocation per slab.  Synchronous, on the context's stream.  The header (mdx_bgzf_deflate takes any bytes)
 * and the end-of-file marker are the caller's to write. */
int mdx_gbam_kept_bound(struct mdx_gbam *g, int64_t *bytes);
int mdx_gbam_write_kept(struct mdx_gbam *g, const uint8_t *group_selected, int32_t n_groups, uint8_t *out, int64_t out_cap, int64_t *out_len,
                        int64_t *n_written, int64_t *raw_bytes);
/* ... with what the run computed per record appended to every written record as tags (--tag-group, --tag-pmd-score; the rule
 * is csrc/mdx_kept_tags.h):
 *   mdx_gbam_write_kept_tagged  mdx_gbam_write_kept, and behind the last tag byte of every written record first
 *                           group_tag 'S' <uint16>: its group, key % n_groups, the index of groups.tsv — then score_tag 'f'
 *                           <float32>: its PMD score, the fixed-point score rounded to the nearest float32 (ties to even) times
 *                           2^-24; block_size grows by 5, 7 or 12 and no other byte changes.  group_tag / score_tag: two
 *                           characters [A-Za-z][A-Za-z0-9] each (no terminator is read), different from one another, or NULL:
 *                           no such tag — both NULL is mdx_gbam_write_kept.  Either tag takes the context's key column as a
 *                           selection does: a stratified context of n_groups groups (MDX_ERR_ARG), the key column of this very
 *                           view (MDX_ERR_STATE), and no record with key 0xFFFF is written.  The score tag needs the score
 *                           column of the same keyed batch too: PMD strata with mdx_strata_pmd_keep_scores (MDX_ERR_STATE).
 *                           A written record that has a tag of one of the two names already: MDX_ERR_BAD_READ, *clash = the lowest
 *                           such index of the slab (mdx_gbam_record_name gives its name), nothing of the slab is written; else
 *                           *clash = -1 (clash may be NULL).  A tag region that cannot be followed (an unknown type, a B array
 *                           past the record's end) ends the search without a clash; dropped records are not searched.
 *   mdx_gbam_kept_bound_tagged  mdx_gbam_kept_bound with tag_bytes (0, 5, 7 or 12) more for every record of the view. */
int mdx_gbam_kept_bound_tagged(struct mdx_gbam *g, int32_t tag_bytes, int64_t *bytes);
int mdx_gbam_write_kept_tagged(struct mdx_gbam *g, const uint8_t *group_selected, int32_t n_groups, const char *group_tag, const char *score_tag,
                               uint8_t *out, int64_t out_cap, int64_t *out_len, int64_t *n_written, int64_t *raw_bytes, int64_t *clash);
/* --write-index: the BAI index (SAM specification 5.2) of the file those members make, from what the run has on the device — no
 * second inflate of the output.  The rule is csrc/mdx_kept_index.h: extents by the CIGAR, reg2bin, one chunk per maximal run
 * of consecutive written records with the same (tid, bin), the linear index's minima; nothing is merged, so the index is a
 * function of the written file alone.
 *   mdx_gbam_kept_index     right behind mdx_gbam_write_kept / _tagged of the view handed out last (anything else:
 *                           MDX_ERR_STATE; a call that failed does not count).  stream_base = the uncompressed bytes all
 *                           earlier slabs wrote (the sum of their *raw_bytes): every offset that comes back is stream_base + the
 *                           record's offset in this slab's stream, and the caller turns the few of them into virtual file
 *                           offsets with the members' compressed sizes (BSIZE).  *prev_tid / *prev_pos: the last written
 *                           record in front of this slab (-1, -1: none), updated to this slab's last one.  runs (host, runs_cap
 *                           entries; *n_written of the write always suffice, fewer than the slab has: MDX_ERR_ARG) receives
 *                           *n_runs entries in file order: records [first, last) of the slab's written ones, bytes
 *                           [ustart, uend) of the stream.  A slab's first run may continue the last run of the slab in
 *                           front (equal tid and bin): joining them is the caller's.  The linear index is kept on the device
 *                           across the calls.  A written record out of coordinate order against the written record before
 *                           it (reason MDX_INDEX_UNSORTED), or one outside [0, min(LN, 2^29)] of a header sequence
 *                           (MDX_INDEX_UNPLACEABLE): MDX_ERR_BAD_READ, *bad = the lowest such index of the slab
 *                           (mdx_gbam_record_name gives its name), *reason says which; nothing comes back.  Dropped records are
 *                           not looked at.  Nothing is launched for a slab without written records.
 *   mdx_gbam_kept_index_linear  out[n] (host): one word per 16 KiB window of every header sequence in turn, n = the sum of
 *                           ceil(LN / 16384) (*n_words, may be NULL; out NULL with n 0 asks for it alone): the lowest ustart
 *                           of a written record that touches the window, all ones for an untouched one.  Once, behind the
 *                           last slab.
 * The handle owns the scratch and the linear index (190 k words for a 3 Gb genome); mdx_gbam_close releases them. */
#define MDX_INDEX_UNSORTED 1
#define MDX_INDEX_UNPLACEABLE 2
typedef struct mdx_index_run {
    int32_t tid;
    uint32_t bin;
    uint64_t ustart, uend;
    uint32_t first, last;
} mdx_index_run;
int mdx_gbam_kept_index(struct mdx_gbam *g, int64_t stream_base, int32_t *prev_tid, int32_t *prev_pos, mdx_index_run *runs, int64_t runs_cap,
                        int64_t *n_runs, int64_t *bad, int32_t *reason);
int mdx_gbam_kept_index_linear(struct mdx_gbam *g, uint64_t *out, int64_t n, int64_t *n_words);
/* --mask-ends: the written records handed on with the damaged ends of their molecules masked — base N, quality 0 — in the
 * same pass (not a reference option; what `bam trimBam` or `pmdtools --adjustbaseq` behind the run would have done).  The rule
 * is csrc/mdx_kept_mask.h: windows of k5 / k3 query bases (SEQ without its terminal soft clips, gaps not counted) at the
 * molecule's 5' and 3' ends — a reverse-strand record's 5' end is its stored right end —, and what a window selects:
 *   MDX_MASK_ALL          every base of it;
 *   MDX_MASK_TRANSITIONS  the 5' window a stored T (reverse strand: A), the 3' window a stored A (reverse strand: T), with
 *                         single_stranded what the 5' window selects;
 *   MDX_MASK_MISMATCHES   those of them under which the resident reference (mdx_set_reference*) has the partner, C under T
 *                         and G under A.
 * No record changes its length, no tag (NM, MD) is touched: sizes, offsets, tags and index are what they are without.
 *   mdx_gbam_set_kept_mask     the mask of every later mdx_gbam_write_kept / _tagged call of the handle: one kernel between
 *                           the gather and the BGZF writer, in place on the handle's stream buffer — the slab's inflated
 *                           records, which the tabulation and the index read, stay as the file has them.  k5, k3: 0..255;
 *                           both 0 clears the mask (what and single_stranded are not looked at then).  Setting or clearing
 *                           zeroes the counts.  MDX_ERR_ARG for a value out of range or an unknown `what`.  A write with
 *                           MDX_MASK_MISMATCHES on a context without a resident reference: MDX_ERR_STATE, nothing launched.
 *   mdx_gbam_kept_mask_counts  *records = the written records with at least one masked base, *bases = the masked bases
 *                           (whatever they held before), summed over the writes since the mask was set; synchronous.
 * Without a mask a write launches, copies and allocates nothing more than before. */
#define MDX_MASK_ALL 0
#define MDX_MASK_TRANSITIONS 1
#define MDX_MASK_MISMATCHES 2
int mdx_gbam_set_kept_mask(struct mdx_gbam *g, int32_t k5, int32_t k3, int32_t what, int32_t single_stranded);
int mdx_gbam_kept_mask_counts(struct mdx_gbam *g, uint64_t *records, uint64_t *bases);
/* --calmd: every written record leaves with NM and MD recomputed against the resident reference (not a reference option;
 * what `samtools calmd` behind the run would have done, by inflating, rewriting and deflating the file again).  The rule is
 * csrc/mdx_kept_md.h: one walk over the record's operations gives the edit count and the MD string; the record keeps its fields
 * and its tags in their order without every field named NM or MD, then NM (C, S or I: the smallest that holds it) and MD:Z
 * follow, and block_size is the new length — a record may grow or shrink.  Computed from the bytes the file will hold: behind
 * the mask of mdx_gbam_set_kept_mask, with the tags of mdx_gbam_write_kept_tagged in place.  A record the rule cannot follow
 * (its CIGAR does not fill SEQ, it lies outside its sequence, its tags cannot be walked to its end, it has a CG:B tag, its MD
 * would pass 2 * l_seq + 64 characters) is skipped: written byte for byte as it is.  The resident reference keeps no IUPAC
 * letters: an ambiguity code of the FASTA appears in MD as N, and no base of a read matches it.
 *   mdx_gbam_set_kept_md     on != 0: every later mdx_gbam_write_kept / _tagged call of the handle runs the stage — the new
 *                           sizes, their scan, sixteen bytes back and a rewrite into a second stream buffer of the handle,
 *                           which is what gets compressed; *raw_bytes is the new total, and mdx_gbam_kept_index behind the
 *                           write describes the new stream.  0 switches it off.  Either way the counts start again at 0.  A
 *                           write on a context without a resident reference (mdx_set_reference*): MDX_ERR_STATE, nothing
 *                           launched.
 *   mdx_gbam_kept_md_counts  out[0] = the written records recomputed, out[1] = those skipped, out[2] = those that had an NM or
 *                           MD field (in tags that can be walked), summed over the writes since the stage was switched;
 *                           synchronous.
 *   mdx_gbam_kept_bound_md   mdx_gbam_kept_bound_tagged, and with md != 0 what the stage can add: a record grows by at most
 *                           7 (NM:I) + 3 + (2 * l_seq + 64) + 1 bytes, and a recomputed record holds its SEQ and QUAL, so
 *                           2 * l_seq <= 4 * block_size / 3 — 75 bytes per record of the view and four thirds of its bytes.
 * Without the stage a write launches, copies and allocates nothing more than before. */
int mdx_gbam_set_kept_md(struct mdx_gbam *g, int32_t on);
int mdx_gbam_kept_md_counts(struct mdx_gbam *g, uint64_t out[3]);
int mdx_gbam_kept_bound_md(struct mdx_gbam *g, int32_t tag_bytes, int32_t md, int64_t *bytes);
/* mdx_mr_round: float("%.5f" % x) of rescale.py:275-276 for n MR sums (mr_raw of the rescale calls) on `threads` host threads —
 * the value printed with five decimals, read back, and narrowed to the 32 bits of an MR:f tag; NaN (a record written back
 * unchanged) gives 0. */
int mdx_mr_round(const double *mr_raw, int64_t n, float *out, int32_t threads);
int mdx_bam_stream_keep_raw(mdx_bam_stream *stream, int on);
int mdx_bam_raw(const mdx_bam *bam, const uint8_t **data, const uint64_t **rec_off);
int mdx_bam_patch_rescaled(const mdx_bam *bam, const uint8_t *qual_out, const float *mr, const uint8_t *rescaled,
                           uint8_t *out, int64_t out_cap, int64_t *out_len);

/* Introspection for tests/benchmarks: 0 = LDS-privatised path, 1 = global-atomic fallback. */
int mdx_table_mode(const mdx_ctx *ctx);

/* ---- GPU-side BAM decode.  The device counterpart of mdx_bam_open / mdx_bam_next — and with them of
 * pysam.AlignmentFile behind mapdamage/reader.py:20-46: the compressed file goes to HBM a slab of BGZF blocks at a
 * time, is inflated there (one wavefront per block; RFC 1951, mapdamage_amd/csrc/mdx_inflate.h) and unpacked there
 * into the columns of an mdx_batch that never exist on the host; the view mdx_gbam_next fills holds DEVICE pointers,
 * ready for mdx_tabulate_device / mdx_rescale_device, valid until the next mdx_gbam_next / mdx_gbam_close (which
 * wait for the context's stream first).  The header is parsed on the host (mdx_gbam_header: for the mdx_bam_*
 * accessors).  mdx_gbam_configure: the header's read-group ids with the library of each, the library of a record
 * without RG tag (-1: none — such a record gets library 0xFFFF, MDX_ERR_BAD_READ at mdx_sync if it is one the kernel
 * counts, as is a read group the header does not list), and whether the quality and mate columns are wanted.
 * Any BGZF layout is taken: htslib starts every block at a record and flushes the header into blocks of its own
 * (bgzf_flush_try in bam_write1); htsjdk / Picard, sambamba and biobambam fill their blocks whatever the record
 * boundaries.  The inflated blocks of a slab lie back to back in HBM, every block guesses where its first record
 * starts, and a guess counts only if the chain of records in front of it ends there (a block whose guess was wrong is
 * scanned again: mdx_gbam_fixups); a slab's batch holds the records that START in it — the blocks behind it are inflated
 * as far as its last record reaches.  MDX_ERR_UNSUPPORTED is what is left: a record longer than a gigabyte, and (see
 * mdx_gbam_skip) a sharded run over a file whose record boundaries cannot be told without the slab in front.  The
 * CRC32 of every block is checked on the device, like its ISIZE (MDX_ERR_ARG, as in the host decoder).
 * chunk_bytes: compressed bytes per slab.  mdx_gbam_next at the end of the file: MDX_OK, n_reads 0,
 * mdx_gbam_at_end 1.  mdx_ctx_stream: the HIP stream (hipStream_t) and device the context works on. */
typedef struct mdx_gbam mdx_gbam;
int mdx_ctx_stream(mdx_ctx *ctx, void **stream, int *device);
int mdx_gbam_open(mdx_ctx *ctx, const char *path, mdx_gbam **out);
int mdx_gbam_open_source(mdx_ctx *ctx, mdx_source *source, mdx_gbam **out);
const mdx_bam *mdx_gbam_header(const mdx_gbam *g);
const char *mdx_gbam_error(const mdx_gbam *g);
int mdx_gbam_configure(mdx_gbam *g, int32_t n_rg, const char *const *rg_ids, const int32_t *lib_of_rg, int32_t lib_default,
                       int want_qual, int want_mate);
int mdx_gbam_next(mdx_gbam *g, int64_t chunk_bytes, mdx_batch *dev_view, const int32_t **d_mtid, const int32_t **d_mpos);
/* --min-basequal on the device path (needs want_qual): records none of whose qualities is below the threshold get
 * MDX_FLAG_QUAL_ABOVE_MIN in the flag column, a 4-bit SEQ column takes the mask into its nibbles (the views are
 * MDX_SEQ_4BITQ), a slab without a single maskable record is handed over without its quality column (the unmasked
 * kernel), and mdx_gbam_missing_qualities says whether a record the kernel counts has come by without qualities so far
 * (what main.py:185-192 warns about).  minqual must be the threshold of the context the file was opened on (or 0): the
 * views carry it in their nibbles (MDX_ERR_ARG otherwise). */
int mdx_gbam_set_min_basequal(mdx_gbam *g, int32_t minqual);
/* MDX_SEQ_4BIT: the unpack kernel keeps BAM's nibbles (recoded, low nibble first) instead of expanding them to ASCII;
 * the views of mdx_gbam_next then carry seq_format = MDX_SEQ_4BIT.  Default MDX_SEQ_ASCII. */
int mdx_gbam_set_seq_format(mdx_gbam *g, int32_t seq_format);
int mdx_gbam_missing_qualities(const mdx_gbam *g);
/* The record filter of the device path (mdx_record_filter above): set any time before the first mdx_gbam_next (MDX_ERR_STATE
 * behind it; NULL or all zero: off).  The unpack kernel evaluates it on the record's fixed fields and ORs 0x200 into the flag
 * column and sums the reasons on the device: no copy and no wait per slab.  mdx_gbam_filter_counts: the six counts,
 * cumulative over the slabs decoded so far (skipped slabs are not read); it waits for the context's stream.  The records
 * read count the slabs handed out; a slab whose mdx_gbam_next FAILED behind its unpack launch (a block that fails its CRC32,
 * a HIP error) may have added to the five reasons already — such a file ends in the host decoder's error for the same
 * block, and a caller that goes on regardless should take the counts before the call, not after. */
int mdx_gbam_set_record_filter(mdx_gbam *g, const mdx_record_filter *filter);
int mdx_gbam_filter_counts(const mdx_gbam *g, uint64_t out[6]);
int mdx_gbam_at_end(const mdx_gbam *g);
/* Steps over the slab mdx_gbam_next would decode next (same chunk_bytes, same borders) without touching the device: in a
 * run over several GPUs (one process and one mdx_gbam per GPU) rank r decodes the slabs r, r + N, ... and skips
 * the others — the loop of mapdamage/main.py:165-217 sharded by record with no exchange until the tables are summed. */
int mdx_gbam_skip(mdx_gbam *g, int64_t chunk_bytes);
/* Where the next slab begins: compressed offset of its first BGZF block and the inflated bytes in front of its first
 * record (a record may straddle BGZF blocks and slabs; a slab holds the records that start in it).  mdx_bam_seek takes the
 * pair: when mdx_gbam_next fails, the tables hold the slabs in front and the host decoder can go on from here.
 * MDX_ERR_STATE behind mdx_gbam_skip (the offset is the device scan's guess then). */
int mdx_gbam_tell(const mdx_gbam *g, int64_t *comp_off, int64_t *phase);
/* BGZF blocks whose guessed first record was not where the chain of records in front of it ended; such a block is scanned
 * again from the right offset (the batch is exact either way; 0 for a file laid out the way htslib does). */
int mdx_gbam_fixups(const mdx_gbam *g);
/* --downsample on the device path (mapdamage/reader.py:134-146: a record the flag filter keeps stays with probability p,
 * one draw of Python's random.Random per kept record in file order — the generator stays with the caller).
 * mdx_gbam_view_flags copies the flag column of the view mdx_gbam_next handed out last to the host (n = its n_reads;
 * 2 bytes per record), mdx_gbam_view_set_flags writes it back: the caller draws, marks the records that leave with a bit
 * the flag filter drops (0x200) and tabulates the view.  Both synchronous. */
int mdx_gbam_view_flags(mdx_gbam *g, uint16_t *flags, int64_t n);
int mdx_gbam_view_set_flags(mdx_gbam *g, const uint16_t *flags, int64_t n);
void mdx_gbam_close(mdx_gbam *g);
/* The host beside the device.  mdx_host_threads: the threads this process inflates BGZF blocks on (the host's share of a slab,
 * mdx_gbam_next; the pool starts with the first such slab and keeps its size) — half of the hardware threads, at most 128 and
 * at most what the control group's cpu.max grants less two, divided by LOCAL_WORLD_SIZE (the ranks of this node, one per GPU,
 * SURVEY 8e, inflate at the same time); MDX_GBAM_HOST_THREADS overrides, MDX_CPU_MAX_FILE names a stand-in for
 * /sys/fs/cgroup/cpu.max.  mdx_host_pool_threads: starts the pool if need be and returns its size.
 * mdx_warm: what a process pays once whichever file comes first — the device's context, the decode kernels' code object, the
 * pool, a pinned buffer of pinned_bytes for the host's share — for a helper thread at the start of a run (the command line
 * warms up beside its header and index reads).  The reference has no counterpart (pysam opens a file in microseconds). */
int mdx_host_threads(void);
int mdx_host_pool_threads(void);
int mdx_warm(int32_t device, int64_t pinned_bytes);
/* Introspection for tests: the device inflate and CRC32 stages of the decode path alone, on BGZF payloads the caller
 * supplies (host buffers).  blk holds four words per block — payload offset in comp, payload bytes, offset in out,
 * bytes out (ISIZE, at most 65536) — and want_crc the CRC32 of each block's inflated bytes (may be NULL: no check).
 * status[b] = bytes produced, or a negative inflate code (-4: ISIZE disagrees); crc_ok[b] = 1 when the check passed.
 * tests/test_gpu_decode.py feeds it every deflate block type, window distances across the LDS ring and damaged
 * streams, against zlib. */
int mdx_gbam_inflate_blocks(mdx_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, const uint32_t *blk, int32_t n_blocks,
                            uint8_t *out, int64_t out_bytes, int32_t *status, const uint32_t *want_crc, uint8_t *crc_ok);

/* ---- GPU-side SAM text decode (additions of ABI 6).  The counterpart of mdx_gbam_* for SAM text, and with it of sam.read_sam
 * (the parser behind mapdamage/reader.py:34-38 when the input is not BGZF): the text goes to HBM a slab of whole lines at a
 * time and is parsed there — a bitmap of the slab's newlines and tabs, the line ends compacted out of it, eight lanes per
 * line for the fields — into the columns of an mdx_batch that never exist on the host.  The view of mdx_gsam_next follows
 * the rules of mdx_gbam_next: device pointers valid until the next mdx_gsam_next / mdx_gsam_close, MDX_SEQ_4BIT nibbles
 * recoded as the BAM unpack recodes them (MDX_SEQ_4BITQ under mdx_gsam_set_min_basequal), flag bits 14 and 15 cleared and
 * then MDX_FLAG_HAS_QUAL / MDX_FLAG_QUAL_ABOVE_MIN set, library 0xFFFF for a missing or unlisted read group (MDX_ERR_BAD_READ
 * only if the kernel counts the record), a slab without a maskable record handed over without its quality column.
 *   mdx_gsam_open        the header — the leading run of lines that start with '@' — is parsed on the host (mdx_gsam_header:
 *                        a record-less mdx_bam for the mdx_bam_* accessors).  Two @SQ lines with one SN: MDX_ERR_UNSUPPORTED
 *                        (read_sam keeps the last index of a name)
 *   mdx_gsam_next        the complete lines within the next chunk_bytes of text (a slab ends at its last '\n'; a last line
 *                        without one is a record too).  Two slabs in a pipeline: the next one is copied to HBM under the
 *                        kernels of this one.  At the end: MDX_OK, n_reads 0, mdx_gsam_at_end 1.
 *   mdx_gsam_tell        byte offset of the first line of the slab mdx_gsam_next would decode.  A stream is never released
 *                        past it: a host parser can take the stream up there (mdx_source_seek) when a call fails — and the
 *                        slab handed out last stays readable until the next call.
 * bgzip-compressed text (BGZF: the input's first gzip member carries the 'BC' extra subfield; what inflates from it does not
 * start with "BAM\1") is taken by the same calls: mdx_gsam_open inflates the blocks the header lies in on the host, and a slab
 * of mdx_gsam_next is then a run of whole BGZF blocks — chunk_bytes counts COMPRESSED bytes, as for mdx_gbam_next — whose
 * compressed bytes go to HBM, where the BGZF kernels of the BAM path inflate and CRC-check them into the slab's text: the
 * text never exists on the host.  Any BGZF layout (empty blocks, end-of-file blocks anywhere or missing, stored blocks, other
 * extra subfields).  The last '\n' of a slab's text is found on the device; the bytes behind it — the start of a line that
 * ends in a later block — are copied in front of the next slab's text, which is inflated at a fixed gap (up to the 32-byte
 * boundary in front of the carried bytes the gap holds '\n': empty lines, which are no records and which the line number of
 * mdx_gsam_error does not count).  A line may span any number of blocks and slabs.  A block that does not inflate, whose ISIZE
 * disagrees or whose CRC32 is wrong: MDX_ERR_ARG; a later member that is not BGZF: MDX_ERR_UNSUPPORTED.
 *   mdx_gsam_is_bgzf     1: the input is bgzip-compressed text (mdx_gsam_tell_bgzf tells its position), 0: plain text
 *   mdx_gsam_tell_bgzf   (compressed offset of a BGZF block, inflated bytes in front of the line within it) of the first line
 *                        of the slab mdx_gsam_next would decode — where the carried bytes START, which may be several blocks
 *                        back —, modelled on mdx_gbam_tell.  A stream is never released past that block: a host inflater
 *                        takes it up there (mdx_source_seek).  MDX_ERR_ARG for plain text (mdx_gsam_tell, which in turn
 *                        refuses compressed text).
 * Lines are parsed as read_sam parses them: fewer than 11 fields (an empty line too) is no record; FLAG & 0x3FFF; RNAME the
 * header's index or -1; POS - 1; TLEN; CIGAR '*' no operations; SEQ '*' empty, upper-cased, every other symbol N; QUAL '*'
 * 0xFF per base; the last RG:Z: tag wins.  Where Python's int(), str.upper(), text decoding or ReadBatch.validate() could
 * differ from that, the slab is given up with MDX_ERR_UNSUPPORTED and none of it is counted: a byte >= 0x80 or a '\r', a
 * line starting with '@' behind the first record, FLAG not 1-5 digits or above 65535, POS / TLEN not -?[0-9]+ or outside
 * int32, a CIGAR byte outside [0-9MIDNSHP=X], an operation of 2^28 bases or more, digits without an operation, QUAL not '*'
 * and not as long as SEQ or with a byte below 33, SEQ '*' with QUAL not '*'.  mdx_gsam_error says which line and why. */
typedef struct mdx_gsam mdx_gsam;
int mdx_gsam_open(mdx_ctx *ctx, const char *path, mdx_gsam **out);
int mdx_gsam_open_source(mdx_ctx *ctx, mdx_source *source, mdx_gsam **out);
const mdx_bam *mdx_gsam_header(const mdx_gsam *g);
const char *mdx_gsam_error(const mdx_gsam *g);
/* the read groups with the library of each, the library of a record without RG tag (-1: none), the quality column wanted —
 * as mdx_gbam_configure (no mate columns: SAM's RNEXT / PNEXT are not parsed) */
int mdx_gsam_configure(mdx_gsam *g, int32_t n_rg, const char *const *rg_ids, const int32_t *lib_of_rg, int32_t lib_default, int want_qual);
/* MDX_SEQ_ASCII (default) or MDX_SEQ_4BIT, as mdx_gbam_set_seq_format */
int mdx_gsam_set_seq_format(mdx_gsam *g, int32_t seq_format);
/* --min-basequal on the device path, as mdx_gbam_set_min_basequal (the context's threshold; needs want_qual) */
int mdx_gsam_set_min_basequal(mdx_gsam *g, int32_t minqual);
int mdx_gsam_next(mdx_gsam *g, int64_t chunk_bytes, mdx_batch *dev_view);
int mdx_gsam_at_end(const mdx_gsam *g);
int mdx_gsam_tell(const mdx_gsam *g, int64_t *offset);
int mdx_gsam_is_bgzf(const mdx_gsam *g);
int mdx_gsam_tell_bgzf(const mdx_gsam *g, int64_t *comp_off, int64_t *phase);
/* the flag column of the view handed out last, to the host and back (--downsample), as mdx_gbam_view_flags / _set_flags */
int mdx_gsam_view_flags(mdx_gsam *g, uint16_t *flags, int64_t n);
int mdx_gsam_view_set_flags(mdx_gsam *g, const uint16_t *flags, int64_t n);
/* a record the kernel counts has come by without qualities so far (under mdx_gsam_set_min_basequal; main.py:185-192) */
int mdx_gsam_missing_qualities(const mdx_gsam *g);
/* The record filter, as mdx_gbam_set_record_filter / mdx_gbam_filter_counts.  With a MAPQ threshold the field pass parses
 * field 5: anything but 1 to 3 digits with a value of 255 or less gives the slab up to the host parser (MDX_ERR_UNSUPPORTED).
 * A slab that is given up adds nothing to the counts. */
int mdx_gsam_set_record_filter(mdx_gsam *g, const mdx_record_filter *filter);
int mdx_gsam_filter_counts(const mdx_gsam *g, uint64_t out[6]);
void mdx_gsam_close(mdx_gsam *g);

/* ---- The Bayesian estimate of the damage parameters on the device (additions of ABI 6): mapdamage/r/stats/ — the model of
 * function.r, the priors and proposals of priorPropose.r, the seven Metropolis updates of postConditonal.r in the order of
 * runGibbs, adjustPropVar between the burn-in rounds, the correcting probabilities of postPredCheck.  One wavefront per
 * chain, any number of chains in a launch, everything in double; a chain's result depends on its own inputs alone.
 * A table is the m x 16 matrix of readMapDamData (data.r), row-major, columns A C G T A.C A.G A.T C.A C.G C.T G.A G.C G.T
 * T.A T.C T.G, as doubles; with it go the constant of its likelihood (the sum over rows and reference bases of
 * lnfact(N) - sum lnfact(S), function.r:124-128, which no parameter moves), its nick vector nuVec [m] (main.r:98-148) and
 * its base frequencies acgt [4].  A parameter vector is Theta, Rho, DeltaD, DeltaS, Lambda, LambdaRight, LambdaDisp; a trace
 * row is that vector and LogLik.
 * Random numbers: Philox4x32-10 with key (seed, chain id) and counter (phase, iteration, update index, draw index); words 0-1
 * and 2-3 of a block make two uniforms ((x >> 11) + 0.5) * 2^-53, a normal is Box–Muller of the two.  Phase 0 is the start
 * search (iteration = start, draws 0..3: the uniforms of Theta, DeltaD, DeltaS, Lambda, LambdaRight, the picks of LambdaDisp
 * and Rho), phases 1..R the burn-in rounds (R = max(n_adjust, 1)), R + 1 the kept iterations — update index = the
 * parameter's index, draw 0 its proposal's normal, draw 1 the uniform of the accept step —, R + 2 the correcting
 * probabilities (iteration = draw of the posterior, draws 0..3: the row picked from the trace for Lambda, LambdaDisp,
 * LambdaRight, LambdaDisp again, DeltaS, DeltaD, Theta, Rho).
 *   mdx_stats_loglik   n log-likelihoods: evaluation e takes table table_of[e] and params[e][7].  -inf outside the
 *                      parameters' ranges, logLikAll (function.r:142-161) inside, with the overhang vector of
 *                      logLikAllOptimize (start.r:28-44).  What the start search evaluates, and the tests' window onto it.
 *   mdx_stats_run      n_chains chains from the start search to the correcting probabilities.  trace [chain][n_iter][8],
 *                      prop_sd [chain][7] (the proposal SDs after the last adjustment), acc [chain][8] (distinct
 *                      consecutive values of each column / n_iter), corr [chain][m][2] (C.T, G.A of row i), start
 *                      [chain][8] (the start the chain took and its log-likelihood; may be NULL).  Synchronous.
 *   mdx_stats_pmat     n substitution matrices [n][16] (row = from) for in[n][6] = Theta, Rho, acgt: getPmat
 *                      (function.r:8-64), HKY85 in closed form or (jukes_cantor != 0) Jukes–Cantor. */
#define MDX_STATS_MAX_M 256
typedef struct {
    int32_t m;               /* rows of a table: 2 x --seq-length with both termini (even), else --seq-length */
    int32_t termini;         /* 0 both, 1 5p, 2 3p */
    int32_t fix_ti_tv;       /* --jukes-cantor */
    int32_t same_overhangs;  /* 0 with --diff-hangs (both termini only) */
    int32_t fix_disp;        /* 0 with --var-disp */
    int32_t n_rand;          /* --rand (0: the start values of runGeneral.r) */
    int32_t n_adjust;        /* --adjust */
    int32_t n_burn;          /* --burn, >= 1 */
    int32_t n_iter;          /* --iter, >= 1 */
    int32_t n_pred;          /* draws behind a correcting probability (10000 in postPredCheck) */
    uint32_t seed;           /* --stats-seed */
    int32_t reserved;
} mdx_stats_config;
int mdx_stats_loglik(int32_t device, const mdx_stats_config *cfg, int32_t n_tables, const double *tables, const double *lnfact,
                     const double *nu, const double *acgt, int64_t n, const int32_t *table_of, const double *params, double *loglik);
int mdx_stats_run(int32_t device, const mdx_stats_config *cfg, int32_t n_chains, const double *tables, const double *lnfact,
                  const double *nu, const double *acgt, const uint32_t *chain_id, double *trace, double *prop_sd, double *acc,
                  double *corr, double *start);
int mdx_stats_pmat(int32_t device, int64_t n, const double *theta_rho_acgt, int32_t jukes_cantor, double *out);

#ifdef __cplusplus
}
#endif
#endif /* MDX_H */
