/*
 * nprealign.h -- C ABI of libnprealign.so: batched banded five-state pair-HMM realignment of
 * nanopore reads on MI355X (gfx950), the drop-in for the reference's per-read `cactus_realign`
 * subprocess.
 *
 * What it replaces.  The reference has no FFI for this path: it has a PROCESS boundary.  One
 * `cactus_realign` process is forked per SAM record by sonLib's system() at
 *     nanopore/analyses/utils.py:587            (realign; fan-out loop utils.py:565-570,
 *                                                gather/splice utils.py:591-609)
 *     nanopore/analyses/alignmentUncertainty.py:41        (rescore the original alignment)
 *     nanopore/analyses/marginAlignSnpCaller.py:136-146   (dump all posterior match probabilities)
 * with inputs "reference FASTA, read FASTA, exonerate cigar on stdin, --diagonalExpansion,
 * --splitMatrixBiggerThanThis, --gapGamma, --matchGamma, --loadHmm" and outputs "one cigar line
 * on stdout (+ score), optional `refPos readPos prob` TSV".  Each entry point below cites the
 * piece of that contract it stands for.  INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions: plain pointers and sizes only; the caller owns every input buffer (borrowed for the
 * duration of the call); every function returns NPR_OK (0) or a negative NPR_ERR_* code and, where an
 * `err` buffer is given, writes a message into it; no exceptions, no globals, no stdout.  One
 * npr_ctx per (thread, device); calls on one ctx must be serialised by the caller.  There is NO CPU
 * fallback: npr_create fails with NPR_ERR_NO_DEVICE when no gfx950 GPU / HIP runtime is usable.
 *
 * Coordinates: X = reference, Y = read; cigar ops are (op,len) int32 pairs with SAM op codes
 * 0 = M, 1 = I (read only), 2 = D (reference only) -- the mapping realignSamFile3TargetFn relies on
 * (utils.py:602) and getExonerateCigarFormatString emits (utils.py:173).
 */
#ifndef NPREALIGN_H
#define NPREALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPR_ABI_VERSION 1

/* error codes */
#define NPR_OK 0
#define NPR_ERR_INVALID (-1)       /* bad argument / guide cigar is not a global alignment (utils.py:381-382) */
#define NPR_ERR_ZERO_PROB (-2)     /* total probability of the banded model is zero */
#define NPR_ERR_CAPACITY (-3)      /* an output buffer (ops / posterior pairs) was too small */
#define NPR_ERR_MODEL (-4)         /* HMM has a transition outside the five-state cell update */
#define NPR_ERR_NO_DEVICE (-5)     /* no usable gfx950 device: there is no CPU fallback */
#define NPR_ERR_HIP (-6)           /* HIP runtime error (message in err / npr_last_error) */
#define NPR_ERR_BAND_TOO_WIDE (-7) /* an anti-diagonal has more in-band cells than the kernels support */
#define NPR_ERR_NOMEM (-8)
#define NPR_ERR_STATE (-9)         /* call sequence violated (e.g. finish before run) */

/* cigar op codes (SAM numbering) */
#define NPR_OP_M 0
#define NPR_OP_I 1
#define NPR_OP_D 2

/* band construction */
#define NPR_BAND_ANCHOR 0 /* cactus_realign's: anchors from the guide's M columns +- diagonalExpansion,
                             rectangles between distant anchors, split above splitMatrixBiggerThanThis^2 */
#define NPR_BAND_FIXED 1  /* fixed width W around the guide path (BASELINE.json "band=100/200") */

/* what to return per read: the three call sites of cactus_realign */
#define NPR_MODE_REALIGN 0          /* utils.py:587: new MEA cigar + score */
#define NPR_MODE_RESCORE_ORIGINAL 1 /* alignmentUncertainty.py:41: --rescoreOriginalAlignment
                                       --rescoreByPosteriorProbIgnoringGaps: guide ops kept, score = mean
                                       posterior of its M columns */
#define NPR_MODE_ALL_POSTERIORS 2   /* marginAlignSnpCaller.py:136-146: --outputAllPosteriorProbs; the MEA
                                       cigar is produced as well (stdout of that call) */
#define NPR_MODE_EXPECTATIONS 3     /* utils.py:509-528: the batch is staged for npr_batch_expectations (the E-step of
                                       cactus_expectationMaximisation); npr_batch_run / finish behave as NPR_MODE_REALIGN.
                                       A batch staged in another mode may be laid out for realignment only (scratch regions
                                       of their own size, long reads on two wavefronts): npr_batch_expectations then
                                       returns NPR_ERR_STATE */

#define NPR_MAX_MODELS 8

typedef struct npr_ctx npr_ctx;
typedef struct npr_batch npr_batch;
typedef struct npr_plan npr_plan;

/* The command-line options of cactus_realign used by the reference's three call strings. */
typedef struct {
    int32_t band_mode;           /* NPR_BAND_* */
    int32_t diagonal_expansion;  /* --diagonalExpansion=10 (utils.py:587) */
    int32_t constraint_trim;     /* anchors trimmed at both ends of each gapless block (cPecan default 14) */
    int64_t split_threshold;     /* --splitMatrixBiggerThanThis: 3000 realign (utils.py:587), 100 analyses
                                    (alignmentUncertainty.py:41, marginAlignSnpCaller.py:136) */
    int32_t fixed_width;         /* W for NPR_BAND_FIXED, >= 2 (narrower: NPR_ERR_INVALID for the read) */
    double gap_gamma;            /* --gapGamma  (abstractMapper.py:25 default 0.5); in [0, 1], else npr_batch_create returns NPR_ERR_INVALID */
    double match_gamma;          /* --matchGamma (abstractMapper.py:25 default 0.0); in [-1, 1], else NPR_ERR_INVALID (the device MEA stage keeps
                                    its weights, quantum - gapGamma * gap mass in units of 1e-7, in 32 bits; npr_mea_cigar takes any value) */
    double posterior_threshold;  /* 0.01 */
    int32_t mode;                /* NPR_MODE_* */
    int32_t max_pairs_per_base;  /* capacity of the sparse posterior list per read base (0 -> 6) */
} npr_params;

typedef struct {
    int32_t status;    /* NPR_OK or NPR_ERR_* for this read only: one bad read does not fail the batch */
    int32_t n_segments;
    int64_t cells;     /* in-band lattice cells processed (forward + backward + posterior test each) */
    double loglik;     /* natural-log total probability summed over segments */
    double loglik_bwd; /* same from the backward pass (consistency check) */
    double score;      /* REALIGN / ALL_POSTERIORS: mean posterior of the MEA pairs; RESCORE: mean posterior of
                          the guide's M columns -- what the reference reads back as pA.score
                          (alignmentUncertainty.py:48) */
    int64_t n_ops;     /* number of (op,len) pairs of the output cigar */
    int64_t n_pairs;   /* number of posterior pairs >= threshold */
} npr_read_result;

typedef struct {
    int64_t n_reads, n_tasks;
    int64_t cells;          /* total in-band cells of the batch */
    int64_t diagonals;      /* total anti-diagonals */
    int64_t max_width;      /* widest anti-diagonal (cells) */
    int64_t device_bytes;   /* device memory held by the batch */
    int64_t slots;          /* resident wavefront slots used by the DP launch */
    int32_t kernel_variant; /* kernel that carries most cells: 0 = generic LDS-ring kernel, 1 = register kernel on a frame
                               that follows the anti-diagonal (k_dp_stair / k_dp_wide), 2 = register kernel on column
                               stripes (k_dp_tile) */
} npr_batch_stats;

/* ---- library / context ---- */
int32_t npr_abi_version(void);
const char *npr_strerror(int32_t code);

/* device_id >= 0.  Fails with NPR_ERR_NO_DEVICE if HIP or the device is unavailable. */
int32_t npr_create(int32_t device_id, npr_ctx **out, char *err, size_t errlen);
void npr_destroy(npr_ctx *ctx);
const char *npr_last_error(npr_ctx *ctx);
/* Context options.  NPR_OPT_OVERLAP (value 0 / 1 / 2, default 0): the context is one of several on its device whose batches are
 * in flight together -- a pipelined job stages batch k+1 and finishes batch k-1 while batch k is in its DP pass
 * (nanopore_amd/job.py; the reference's analogue is jobTree running several cactus_realign processes at once,
 * /root/reference/Makefile:1 maxThreads).  The contexts of a device share its forward scratch and take turns in it; with this
 * option the device MEA stage keeps its tables in buffers of the context's own instead (so npr_batch_finish need not wait for
 * another batch's DP pass), and the DP launches of narrow bands take four wavefronts per SIMD instead of seven, so that the staging
 * and MEA kernels of the other batches find slots and registers beside them (a persistent launch that fills the chip leaves room for
 * nothing; nanopore_amd/job.py's default since the end of round 5).  Value 2: the tables of its own only -- the next batch's DP pass
 * starts when it is staged, not when this batch's MEA stage has given the shared scratch back; the MEA kernels take the slots the
 * DP pass leaves as its wavefronts run out.  Results do not change. */
#define NPR_OPT_OVERLAP 1
/* NPR_OPT_RELEASE_SCRATCH (an action; value 2: only the context's cache of released device buffers, the scratch stays): the device's forward scratch (shared by the contexts of the device; the
 * next batch that needs it allocates it again) and this context's cache of released device buffers go back to the driver.  For
 * a process that stays alive after a big batch (the parent of a pipeline, a test session) next to others that need the HBM. */
#define NPR_OPT_RELEASE_SCRATCH 2
/* TEST AND BRING-UP SWITCHES (all 0 by default; none changes a result -- every kernel class computes the same bits or is checked
 * against the same oracle -- only which kernel runs or where a table lives).  They select the code paths the parity tests
 * compare with each other; a caller of the drop-in path never sets them.  Since round 4 these are context options, not
 * environment variables: what the library runs does not depend on the caller's environment.  (Still read from the environment,
 * and changing no choice of kernel: NPR_TIMING=1 stage times on stderr, NPR_POISON=<byte> device buffers filled when handed
 * out, NPR_HOST_THREADS=<n> host worker threads.) */
#define NPR_OPT_KERNEL 3           /* 1: the any-band kernel (k_dp_generic) for every task */
#define NPR_OPT_ARITH 4            /* 1: one exponent per cell (k_dp_stair) instead of one per row (k_dp_rs / k_dp_mid_rs) */
#define NPR_OPT_PAIR 5             /* a read's two sweeps on two wavefronts: 0 the default rule (row-scaled arithmetic: every task of 64+ anti-diagonals), 1 never, 2 the tasks longer than a fair share, 3 always */
#define NPR_OPT_NO_TILE 6          /* 1: no stripe kernel (wide bands take k_dp_wide / k_dp_generic) */
#define NPR_OPT_NO_WIDE 7          /* 1: no multi-wavefront frame kernel */
#define NPR_OPT_TILE_RS 8          /* the stripe kernel: 0 / 1 column-scaled arithmetic (k_dp_tile_cs, the default), 2 one exponent per cell (k_dp_tile) */
#define NPR_OPT_TILE_WAVES 9       /* wavefronts per stripe task (1 .. 8; 0: default 4) */
/* 10, 11, 12, 16, 18 and 19 are retired bring-up switches: npr_ctx_option refuses them as unknown */
#define NPR_OPT_HOST_MEA 13        /* 1: chain + cigar on the host in realign mode too */
#define NPR_OPT_MEA_RING_ONLY 14   /* 1: every read through the LDS-ring chain kernel */
#define NPR_OPT_MEA_GLOBAL_SORT 15 /* 1: the sort's tables in HBM whatever the span */
#define NPR_OPT_EM_GENERIC 17      /* 1: the E-step on the any-band kernel */
#define NPR_OPT_MEA_WIDE_OPS 20    /* 1: the packed cigars cross PCIe as whole words even when every run fits 14 bits */
#define NPR_OPT_EM_TILE 21         /* the E-step of stripe tasks: 0 column-scaled arithmetic first (k_dp_tile_cs's E-step instance; what its certificate refuses goes to k_em_tile), 1 k_em_tile only, 2 (tests) as 0 with every other task refused */
/* NPR_OPT_FINISH_TEXT (not a bring-up switch; 0 by default, value 1): npr_batch_finish's device MEA stage formats the cigars as SAM text on the
 * device (csrc/npr_cigtext.hip) right after it has gathered them, and the TEXT and its offsets cross PCIe through the pinned staging
 * instead of the packed words; npr_batch_cigar_text then copies from the host.  npr_batch_ops / npr_batch_ops_packed (and the batch
 * statistics, k-mer and pileup entry points) on such a batch fetch the words from the device on demand while the stage's tables are still
 * there, and return NPR_ERR_STATE with a message once another batch's finish has overwritten them.  Results do not change; batches that take the
 * host stage are not affected. */
#define NPR_OPT_FINISH_TEXT 22
#define NPR_OPT_COUNT 23
int32_t npr_ctx_option(npr_ctx *ctx, int32_t option, int64_t value);

/* --loadHmm=<file> (utils.py:586-587): the 25 transition and 80 emission PROBABILITIES exactly as they
 * stand in the two-line model file (nanopore/mappers/blasr_hmm_0.txt).  slot in [0, NPR_MAX_MODELS): reads
 * pick a slot through `model_slot` (per-read-type models, scripts/modifyHmm.py).  T == NULL installs the
 * stock model used when the reference passes no --loadHmm (abstractMapper.py:36-37). */
int32_t npr_set_hmm(npr_ctx *ctx, int32_t slot, const double *T25, const double *E80);

/* ---- batch: replaces the per-read fan-out / gather of utils.py:557-609 ---- */
/* Stage 1 (host + H2D): band construction, packing, upload.  Sequences are ASCII (ACGT, any case; anything
 * else is N).  The reference side is a table of n_refs sequences, ref[ref_off[k] .. ref_off[k+1]) -- the
 * contigs of the reference FASTA (argv[1] of cactus_realign) -- and read i is aligned against sequence
 * ref_index[i] (the cigar's target name, utils.py:570); ref_index == NULL means n_refs == n_reads and read i
 * uses sequence i (per-read slices).  read i = read[read_off[i] .. read_off[i+1]) (aR.query, utils.py:570);
 * guide i = (op,len) pairs guide_ops[2*guide_off[i] .. 2*guide_off[i+1]) and must be GLOBAL over both
 * sequences (the chained records of utils.py:313-386).  Only the parts of a reference sequence that a read's
 * band touches are uploaded, so a 4.6 Mb contig shared by 50 k reads costs nothing extra.
 * model_slot may be NULL (all 0). */
int32_t npr_batch_create(npr_ctx *ctx, const npr_params *params, int64_t n_reads, int64_t n_refs,
                         const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                         const uint8_t *read, const int64_t *read_off, const int32_t *guide_ops,
                         const int64_t *guide_off, const int32_t *model_slot, npr_batch **out);
/* The same with guides that carry coordinates, like the exonerate cigar line the reference pipes into cactus_realign
 * (`cigar: query qstart qend + target tstart tend + score ops`, getExonerateCigarFormatString at
 * nanopore/analyses/utils.py:173-186, consumed at utils.py:587): guide i starts at reference position
 * guide_start[2*i] and read position guide_start[2*i+1] (0-based) and spans what its ops consume; the realignment is
 * confined to that window, exactly as cactus_realign realigns only the sub-sequences a cigar covers.  Output cigars
 * cover the window; posterior coordinates stay absolute in the sequences.  guide_start == NULL: every guide starts
 * at (0, 0) and must be global, i.e. npr_batch_create. */
int32_t npr_batch_create_at(npr_ctx *ctx, const npr_params *params, int64_t n_reads, int64_t n_refs,
                            const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                            const uint8_t *read, const int64_t *read_off, const int32_t *guide_ops,
                            const int64_t *guide_off, const int64_t *guide_start, const int32_t *model_slot,
                            npr_batch **out);
/* Stage 2 (device): forward + backward + posterior extraction for every read of the batch; inputs are
 * resident in HBM.  Blocks until done; kernel_ms (nullable) receives the HIP-event time of the DP launch
 * measured on the context's stream.  May be called repeatedly (benchmarks). */
int32_t npr_batch_run(npr_batch *b, float *kernel_ms);
/* Stage 3: MEA chain / rescore, cigars.  In NPR_MODE_REALIGN and NPR_MODE_ALL_POSTERIORS the chain and the cigar are computed on
 * the device from the posterior pairs where they lie (integer arithmetic: the same ops and scores as the host stage, npr_mea_cigar)
 * and only the run-length ops come back.  In NPR_MODE_RESCORE_ORIGINAL the guide's M columns -- spread into a table on the device
 * when the batch was staged -- are looked up where the pairs lie and summed in fixed point (the host stage's double exactly, npr_rescore);
 * eight bytes per read come back, and the cigars are the guide's (made when npr_batch_ops / npr_batch_ops_packed ask).  No mode moves
 * the pairs over PCIe unless npr_batch_pairs asks for them.  Batches whose tables do not fit the device, a rescore sum that could not be
 * exact (a threshold below 2^-20, a guide of 2^23 M columns) and NPR_OPT_HOST_MEA copy the pairs to the host and finish there. */
int32_t npr_batch_finish(npr_batch *b);
void npr_batch_destroy(npr_batch *b);

int32_t npr_batch_get_stats(const npr_batch *b, npr_batch_stats *st);
/* Diagnostics: how the batch's DP problems (segments) were spread over the kernel classes.  tasks[c] / cells[c] for
 * class c (either may be NULL), capacity `cap` entries; returns the number of classes (19):
 *   0-2  register kernel, one wavefront per task, 64 / 128 / 256 slots (k_dp_stair<1|2|4>)
 *   3-6  register kernel, 4 / 8 / 8 / 12 wavefronts per task, 512 / 1024 / 2048 / 3072 slots (k_dp_wide)
 *   7-9  generic kernel, LDS ring for at most 512 / 1024 / 2270 cells per anti-diagonal;  10  generic kernel, HBM ring
 *   11   register kernel on column stripes, any width (k_dp_tile; k_em_tile for npr_batch_expectations); takes what 3-10
 *        would take unless NPR_OPT_NO_TILE is set
 *   12-14  classes 15-17 with the forward and the backward sweep of a task on two wavefronts at once, k_dp_mid_rs<1|2|4> (round 5): the
 *        sweeps start at the two ends and MEET IN THE MIDDLE, each going on past the cut against the rows the other one stored -- a task's
 *        serial chain halves, no more bytes or instructions than k_dp_rs, the same bits; the default for every row-scaled task of 64+
 *        anti-diagonals (shorter ones stay in 15-17).  NPR_OPT_PAIR 1: never, 2: only the tasks longer than a wavefront's fair share of
 *        their class as far as second wavefronts are free
 *   15-17  classes 0-2 in row-scaled arithmetic (k_dp_rs<1|2|4>: one exponent per anti-diagonal row of the wavefront instead of
 *        one per cell, about 1.4 times the cells per second): every task of 0-2 unless NPR_OPT_ARITH = 1 is set or a loaded model's
 *        values can grow from one anti-diagonal to the next.  A task for which one exponent per row was not enough (a stretch of
 *        its alignment ~110 binary orders below the row's largest values: an indel of 70+ bases) is run again by npr_batch_run
 *        with the kernel of 0-2; npr_batch_segment_arith says which arithmetic a segment's results come from.
 *   18   class 11's column stripes in column-scaled arithmetic (k_dp_tile_cs: one exponent per lane of a stripe; the default for the stripe
 *        tasks since round 6, same bits as class 11; a task without its per-lane range certificate runs again in class 11's kernel) */
int32_t npr_batch_class_stats(const npr_batch *b, int64_t *tasks, int64_t *cells, int32_t cap);
/* Which device arithmetic each segment (matrix split) of each read ran in, in read order: seg_off[n_reads + 1], arith[seg_off
 * [n_reads]] (pass arith == NULL for the offsets alone).  0: one exponent per cell (npr_cell.h: k_dp_tile, k_dp_generic, k_dp_wide
 * k_dp_stair); 1: one exponent per anti-diagonal row (npr_rs.h: k_dp_rs, k_dp_mid_rs; classes 15-17, 12-14).  Both are fp32 evaluations of the same recurrences (cactus_realign's forward / backward pass, reference call
 * site nanopore/analyses/utils.py:587) within the stated 1e-4 of the fp64 oracle; the parity tests ask so that they can
 * compare bit for bit with the matching CPU restatement (oracle/realign_oracle_f32.c / realign_oracle_rs.c). */
int32_t npr_batch_segment_arith(const npr_batch *b, int64_t *seg_off, int32_t *arith, int64_t cap);
/* results, valid after npr_batch_finish */
int32_t npr_batch_results(const npr_batch *b, npr_read_result *out /* [n_reads] */);
/* output cigars, CSR: ops_off[n_reads+1] (in op pairs), ops[2*ops_off[n_reads]].  Pass ops == NULL to get
 * only the offsets (two-pass sizing). */
int32_t npr_batch_ops(const npr_batch *b, int64_t *ops_off, int32_t *ops, int64_t cap_pairs);
/* the same cigars, one 32-bit word per operation: length << 2 | op (the form the device MEA stage produces and a sharded
 * job ships between ranks); words[ops_off[n_reads]].  Pass words == NULL for the offsets only. */
int32_t npr_batch_ops_packed(const npr_batch *b, int64_t *ops_off, uint32_t *words, int64_t cap_words);
/* sparse posteriors (>= threshold), CSR by read, sorted by (x, y); x is the 0-based reference coordinate in
 * the read's slice, y the 0-based read coordinate: the `refPos readPos prob` TSV of
 * --outputAllPosteriorProbs (marginAlignSnpCaller.py:149).  After a device-side npr_batch_finish the pairs are
 * still in HBM: the first call with x != NULL copies and sorts them (pair_off alone costs nothing). */
int32_t npr_batch_pairs(const npr_batch *b, int64_t *pair_off, int32_t *x, int32_t *y, float *p, int64_t cap);
/* TEST HOOK (tests/test_gpu_parity.py: the finish stages against malformed input).  Replaces, on the device, the posterior pairs the DP pass left for
 * `read` -- which must have a single segment -- by the n given ones (window coordinates; n at most the list's capacity), as if the DP kernel had
 * written them with status `task_status` (NPR_OK, or e.g. NPR_ERR_CAPACITY for a list that overflowed).  Between npr_batch_run and npr_batch_finish.
 * Nothing in the product calls it. */
int32_t npr_batch_debug_set_pairs(npr_batch *b, int64_t read, const int32_t *x, const int32_t *y, const float *p, int64_t n, int32_t task_status);
/* TEST HOOK (tests/test_gpu_mea_cases.py).  Which stage the last npr_batch_finish of the batch took: 0 the device stage (the MEA chain of
 * csrc/npr_mea.hip; in NPR_MODE_RESCORE_ORIGINAL the device's fixed-point sum), 1 the host stage (NPR_OPT_HOST_MEA, tables that found no room,
 * or a read the device chain gave up on -- more than 64 pairs on a reference position, a pair 8192 read positions below the chain's top: the
 * WHOLE batch is finished on the host then, with the same results).  NPR_ERR_STATE before npr_batch_finish.  Read-only. */
int32_t npr_batch_debug_finish_stage(const npr_batch *b);
/* TEST HOOK (tests/test_gpu_second_pass.py: the second pass of npr_batch_run on every scaled class).  mark[n_segments]: one byte per segment, in
 * the order npr_batch_segment_arith reports them (n_segments must be its seg_off[n_reads], else NPR_ERR_INVALID).  In the next npr_batch_run
 * every task of a row- / column-scaled launch (classes 12-18) whose segment is marked counts as refused by its range certificate: its first-pass
 * result gets the status such a task leaves (on the host and on the device; its pairs and totals are written, as a refused task's are) before
 * the run looks for the tasks to run again, and everything from there on is the path of a task refused by itself.  Marks on tasks of other
 * classes are ignored.  That run clears the marks.  Nothing in the product calls it. */
int32_t npr_batch_debug_refuse(npr_batch *b, const uint8_t *mark, int64_t n_segments);

/* ---- post-alignment statistics on the device ----
 * The per-read integer reductions the reference's analyses make by walking every aligned pair in Python:
 * nanopore/analyses/coverage.py:10-95 (ReadAlignmentCoverageCounter), substitutions.py:9-56, indels.py:9-45.
 * One record of NPR_STATS_WORDS int32 per read:
 *   [0] matches (same base, reference base in ACGT)   [1] mismatches (both in ACGT, different)   [2] aligned pairs against N
 *   [3] aligned pairs (M columns)
 *   [4] read insertions between aligned pairs, [5] their total length; [6] read deletions, [7] their total length
 *       (coverage.py:36-41 / indels.py:22-25: runs between two consecutive aligned pairs)
 *   [8] read bases / [9] reference bases the cigar consumes before its first aligned pair, [10] / [11] after its last one
 *       (what a global alignment adds, coverage.py:42-58)
 *   [12] reference bases, [13] read bases the cigar consumes; [14] 0 or NPR_ERR_INVALID (cigar runs out of its sequences)
 *   [15 + 5 * r + q] aligned pairs of reference base r against read base q, A C G T N (substitutions.py:13-19)
 * npr_batch_align_stats: the alignments npr_batch_finish just produced, where they lie (packed cigars and base codes are
 * still in HBM after the device MEA stage; otherwise the cigars are uploaded).  npr_align_stats: any alignments, e.g. the
 * records of a mapper's SAM file: read i = read[read_off[i] ..) against reference sequence ref_index[i] (NULL: i), cigar
 * i = (op, length) pairs ops[2 * ops_off[i] ..) starting at reference position start[2 * i] and read position
 * start[2 * i + 1] (start == NULL: 0, 0).  Sequences are ASCII as in npr_batch_create. */
#define NPR_STATS_WORDS 40
int32_t npr_batch_align_stats(npr_batch *b, int32_t *stats /* [n_reads][NPR_STATS_WORDS] */);
int32_t npr_align_stats(npr_ctx *ctx, int64_t n_reads, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off,
                        const int32_t *ref_index, const uint8_t *read, const int64_t *read_off, const int32_t *ops,
                        const int64_t *ops_off, const int64_t *start, int32_t *stats /* [n_reads][NPR_STATS_WORDS] */);

/* ---- k-mer tables on the device (the reference's KmerAnalysis and IndelKmerAnalysis) ----
 * Base codes are npr_encode_bases': A C G T -> 0..3 in either letter case, anything else -> 4.  A k-mer's bin is its base-4
 * number, first base most significant; bin 4^k takes the k-mers that hold a code 4.  1 <= k <= 6 (NPR_ERR_INVALID otherwise);
 * a table has 4^k + 1 int64 counters and is overwritten. */

/* All windows of n_seqs ASCII sequences (sequence i = seq[seq_off[i] .. seq_off[i + 1])), forward strand:
 * nanopore/analyses/kmerAnalysis.py:16-17 and :24-25 -- s[i - k : i] for i in k .. len(s) - 1, so the last window of a
 * sequence is left out, as `xrange(kmerSize, len(seq))` leaves it out.  The reverse complements the reference adds
 * (:20, :28) are a permutation of the bins and are the caller's. */
int32_t npr_kmer_counts(npr_ctx *ctx, int32_t k, int64_t n_seqs, const uint8_t *seq, const int64_t *seq_off,
                        int64_t *counts /* [4^k + 1] */);
/* The same windows, bins and letter rules, into one table per group in one pass: what the unmapped-read meta-analyses count
 * (nanopore/metaAnalyses/unmappedKmerAnalysis.py:12-27: read type x mapped / unmapped).  Sequence i is
 * text[seq_begin[i] .. seq_end[i]), a span inside a larger text as npr_batch_create_spans takes reads (columns 2-3 of
 * npr_fastq_index fit directly); group[i] in [0, n_groups) picks its table, -1 leaves it out.  1 <= n_groups <= 64.  A group
 * outside that range, a span that ends before it begins, a bad k or n_groups: NPR_ERR_INVALID, nothing counted, no table
 * touched.  Empty sequences, sequences shorter than k + 1 and n_seqs == 0 are legal and add nothing.  Counts are exact and
 * the same from run to run. */
int32_t npr_kmer_counts_groups(npr_ctx *ctx, int32_t k, int64_t n_seqs, const uint8_t *text, const int64_t *seq_begin,
                               const int64_t *seq_end, const int32_t *group, int32_t n_groups,
                               int64_t *counts /* [n_groups][4^k + 1] */);
/* The k-mers that straddle a gap of an alignment, of the read (read_counts) and of the reference (ref_counts):
 * nanopore/analyses/indelKmerAnalysis.py:11-19 (indelKmerFinder) over the read side and the reference side of
 * record.aligned_pairs (:32-40: s = readSeq[start : end + 1], s = refSeq[start : end + 1]); the reversed k-mers the
 * reference adds (:36, :40) are a permutation of the bins and are the caller's.  Alignments as for npr_align_stats.
 * Positions are window coordinates: they count from the first base the cigar consumes, where the reference indexes
 * record.query from the start of SEQ -- the same thing for a record without soft clips.  A record whose cigar runs
 * past its sequences adds nothing and makes the call return NPR_ERR_INVALID (the tables hold the other records). */
int32_t npr_align_indel_kmers(npr_ctx *ctx, int32_t k, int64_t n_reads, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off,
                              const int32_t *ref_index, const uint8_t *read, const int64_t *read_off, const int32_t *ops,
                              const int64_t *ops_off, const int64_t *start, int64_t *read_counts, int64_t *ref_counts /* [4^k + 1] each */);
/* ... of the alignments npr_batch_finish just produced, where they lie (indelKmerAnalysis.py:29-40 over the realigned SAM
 * without writing it first): to npr_align_indel_kmers what npr_batch_align_stats is to npr_align_stats.  Reads that
 * failed add nothing. */
int32_t npr_batch_indel_kmers(npr_batch *b, int32_t k, int64_t *read_counts, int64_t *ref_counts /* [4^k + 1] each */);

/* ---- read-quality tables on the device (the reference's FastQC analysis, nanopore/analyses/fastqc.py) ----
 * The reference shells out to the Java FastQC; here the statistics are defined in exact integer terms and counted in one
 * pass over the reads' base and quality bytes.  Read i has the bases text[seq_begin[i] .. seq_end[i]) and the quality
 * bytes text[qual_begin[i] .. qual_end[i]).
 *
 * Spans and groups.  Spans are positions inside a larger text, as npr_kmer_counts_groups takes them (columns 2-3 of
 * npr_fastq_index and the pairs of npr_fastq_qual_index fit directly); they may come in any order.  group[i] in
 * [0, n_groups) picks the tables, -1 leaves the read out.  1 <= n_groups <= NPR_RQ_MAX_GROUPS (8).
 *
 * Invalid input.  NPR_ERR_INVALID for any of: a group outside the range, a span that ends before it begins,
 * qual_end - qual_begin != seq_end - seq_begin for a read whose group is not -1, a bad n_groups.  Nothing is counted and
 * no table is touched then; this is checked on the host before any launch.
 *
 * Legal input that adds nothing.  n_reads == 0 is legal: the tables are written as for empty groups.  Empty reads are legal.
 *
 * Position bin, NPR_RQ_POS_BINS = 336.  bin(p) = p for p < 16; otherwise, with e = floor(log2 p),
 * bin(p) = 16 * (e - 3) + ((p >> (e - 4)) & 15): sixteen bins per octave, width 1 below 32, width 2 below 64, and so on.
 * Any p >= 2^24 goes to bin 335.  The inverse: bin b >= 16 starts at (16 + b % 16) << (b / 16 - 1) and is
 * 1 << (b / 16 - 1) wide.  The device computes bin(p) from a count-leading-zeros, without table or search.
 *
 * Quality column, NPR_RQ_QUAL_COLS = 95.  A byte c with 33 <= c <= 126 goes to column c - 33, any other byte to column 94.
 *
 * Base column.  npr_encode_bases' codes: A C G T -> 0..3 in either letter case, anything else -> 4.
 *
 * pos_qual and pos_base.  Every position p of every counted read adds one at [bin(p)][column].
 *
 * len_hist.  One count per read at bin(length); an empty read lands in bin 0.
 *
 * meanq_hist.  One count per non-empty read, in column floor(sum of (c - 33) / length) when every quality byte is in
 * 33..126, else in column 94.
 *
 * gc_hist.  One count per non-empty read.  With n the read's A + C + G + T count and gc its G + C count, the column is
 * (200 * gc + n) / (2 * n), integer division -- the percentage rounded half up, 0..100 -- and 101 when n == 0.
 *
 * totals, NPR_RQ_TOTALS = 8.  reads, bases, shortest length, longest length, smallest quality byte, largest quality byte,
 * empty reads, reads with a quality byte outside 33..126.  Shortest and longest length are -1 when the group has no read,
 * smallest and largest quality byte are -1 when the group has no base.
 *
 * All counts are exact and the same from run to run; the tables are overwritten. */
#define NPR_RQ_POS_BINS 336
#define NPR_RQ_QUAL_COLS 95
#define NPR_RQ_GC_COLS 102
#define NPR_RQ_TOTALS 8
#define NPR_RQ_MAX_GROUPS 8
#define NPR_RQ_TILE 2048 /* positions of one read a workgroup takes per step */
int32_t npr_read_quality(npr_ctx *ctx, int64_t n_reads, const uint8_t *text, const int64_t *seq_begin, const int64_t *seq_end,
                         const int64_t *qual_begin, const int64_t *qual_end, const int32_t *group, int32_t n_groups,
                         int64_t *pos_qual /* [n_groups][NPR_RQ_POS_BINS][NPR_RQ_QUAL_COLS] */,
                         int64_t *pos_base /* [n_groups][NPR_RQ_POS_BINS][5] */, int64_t *len_hist /* [n_groups][NPR_RQ_POS_BINS] */,
                         int64_t *meanq_hist /* [n_groups][NPR_RQ_QUAL_COLS] */, int64_t *gc_hist /* [n_groups][102] */,
                         int64_t *totals /* [n_groups][NPR_RQ_TOTALS] */);

/* ---- the device pileup: per-position depth and base counts of a set of alignments ----
 * What the reference gets from samtools after writing the realigned SAM, converting it to BAM, sorting and indexing it:
 * `samtools depth` (nanopore/metaAnalyses/coverageDepth.py:49-65) and `samtools mpileup` (analyses/consensus.py).  A table of
 * NPR_PILEUP_WORDS int32 counters per reference position, rows in the order of the n_refs reference sequences given to
 * npr_pileup_create (first row of a sequence + position, as for npr_batch_base_expectations), over the selected records:
 *   [0..3] aligned (M) columns whose READ base is A, C, G, T (either letter case)     [4] M columns with any other read base
 *   [5] deletion columns: the position lies inside a D run of the record
 *   [6] insertion runs attached to the position: an I run is attached to the last reference column (M or D) the record consumed
 *       before it; an I run before the record's first column is attached to nothing; I runs not separated by a column count once
 *       (mpileup's `+<n>` marker: a leading 2I is dropped, 2I3I shows one marker, a trailing I is shown)
 *   [7] records whose first reference column (M or D) is the position (mpileup's `^`)
 * `samtools depth` prints the sum of words 0-4 and gives a line to every position where the sum of words 0-5 is not zero.
 * Counts are integers: the table is the same from run to run.  A record costs its cigar runs and its M columns, not its
 * reference span: the D runs of a global alignment (a chained or realigned record spans its whole contig) go through a
 * difference array that is summed up when the counts are read.
 * NOT reproduced: samtools 0.1.19 admits at most 8000 records to a position's pileup (bam_pileup.c, maxcnt), which depends on
 * the order of the file; this table has no cap.
 * A pileup is an object because it outlives a batch: a file is realigned in several chunks and the table accumulates.  It
 * belongs to its context and must be destroyed before it; calls on it count as calls on the context. */
#define NPR_PILEUP_WORDS 8
typedef struct npr_pileup npr_pileup;
/* a zeroed table on the device for n_refs reference sequences of ref_len[k] positions */
int32_t npr_pileup_create(npr_ctx *ctx, int64_t n_refs, const int64_t *ref_len, npr_pileup **out);
void npr_pileup_destroy(npr_pileup *pl);
/* Adds the alignments npr_batch_finish just produced, where they lie (the packed cigars and the base codes are still in HBM
 * after the device MEA stage; otherwise the cigars are uploaded): read i against the reference sequence and from the window
 * start it was staged with.  use[i] != 0 selects read i (NULL: all); reads that failed add nothing.  The batch must be of the
 * pileup's context.  A selected read whose window does not fit its reference sequence in the pileup's table, or whose cigar
 * runs past its window, adds nothing and makes the call return NPR_ERR_INVALID (the other reads are counted). */
int32_t npr_pileup_add_batch(npr_pileup *pl, npr_batch *b, const uint8_t *use /* [n_reads] or NULL */);
/* Adds any alignments, e.g. the records of a mapper's SAM file; arguments as for npr_align_stats, without reference bases:
 * record i = cigar ops[2 * ops_off[i] ..) of read bases read[read_begin[i] .. read_end[i]) against reference sequence
 * ref_index[i], starting at reference position start[2 * i] and read position start[2 * i + 1] (start == NULL: 0, 0).
 * read_end == NULL: read_begin has n_reads + 1 entries and read i ends where read i + 1 begins.  use as above.  A selected
 * record that is malformed (an operation outside M I D, a negative length, a reference index or start outside its sequences)
 * or whose cigar runs past its read or its reference sequence adds NOTHING -- every cigar is checked before its first add --
 * and makes the call return NPR_ERR_INVALID; the other records are counted. */
int32_t npr_pileup_add(npr_pileup *pl, int64_t n_reads, const int32_t *ref_index, const uint8_t *read, const int64_t *read_begin,
                       const int64_t *read_end, const int32_t *ops, const int64_t *ops_off, const int64_t *start, const uint8_t *use);
/* The table so far (the difference array summed on the device, then copied); more records may be added afterwards. */
int32_t npr_pileup_counts(npr_pileup *pl, int32_t *counts /* [sum ref_len][NPR_PILEUP_WORDS] */);
/* ... or only depth[r] = words 0-4 summed and covered[r] = (words 0-5 summed != 0), made on the device: 5 bytes per position
 * cross PCIe instead of 32. */
int32_t npr_pileup_depth(npr_pileup *pl, int32_t *depth /* [sum ref_len] */, uint8_t *covered /* [sum ref_len] */);

/* ---- alignment-quality tables on the device (the reference's QualiMap analysis, nanopore/analyses/qualimap.py) ----
 * The reference converts the SAM file to BAM, sorts it and shells out to the Java `qualimap bamqc`.  Here the statistics are
 * defined in exact integer terms and counted where the data already lies: npr_pileup_coverage reduces a pileup's table,
 * npr_align_quality makes one pass over the records with the reference bases beside them.
 *
 * Rows.  Reference positions are rows of the concatenated sequences, as for npr_pileup_create; T is the sum of ref_len.
 *
 * Windows.  W = n_windows, 1 <= W <= NPR_AQ_MAX_WINDOWS (65536).  Window w holds the rows [w * T / W, (w + 1) * T / W),
 * integer division; equivalently row r lies in window ((r + 1) * W - 1) / T.  Windows ignore sequence boundaries, as
 * QualiMap's do.  When W > T some windows are empty; T == 0 is legal (every window is empty).
 *
 * Bins.  bin(v) is the position bin of npr_read_quality (NPR_RQ_POS_BINS = 336: exact below 16, then sixteen per octave,
 * everything from 2^24 on in bin 335).
 *
 * Base codes.  npr_encode_bases': A C G T -> 0..3 in either letter case, anything else -> 4.
 *
 * Output.  Every table is int64, exact, overwritten, and the same from run to run.
 *
 * npr_pileup_coverage runs over the table of `pl` as npr_pileup_counts would return it (the difference array summed).
 * ref / ref_off are the ASCII reference sequences in the pileup's order: sequence k = ref[ref_off[k] .. ref_off[k + 1]),
 * and ref_off[k + 1] - ref_off[k] must be the pileup's ref_len[k].  With depth = words 0-4 of a row summed:
 *   win[w][NPR_AQ_WIN_WORDS = 8] over the rows of window w:  [0] rows  [1] sum of depth  [2] sum of depth^2
 *     [3] rows with depth >= 1  [4] reference G + C  [5] reference A + C + G + T  [6] record starts (word 7 of the table)
 *     [7] deletion columns (word 5)
 *   depth_hist[336]: one count per row at bin(depth), depth 0 included.
 *   start_hist[336]: one count per row at bin(word 7) -- the duplication table: how many positions begin k records.
 *   totals[NPR_AQ_TOTALS = 8]: rows, depth sum, largest depth, rows with depth >= 1, largest start count, records (sum of
 *     word 7), deletion columns (sum of word 5), insertion markers (sum of word 6).  The two largest values are 0 when T == 0.
 * The largest depth is reduced first: when largest depth^2 x rows of the longest window >= 2^63 the call returns
 * NPR_ERR_CAPACITY and writes nothing (word 2 of a window is the first sum that could leave int64).  A bad n_windows, a null
 * pointer or a length that is not the pileup's: NPR_ERR_INVALID, checked on the host before any launch, nothing written.
 *
 * npr_align_quality takes the records exactly as npr_pileup_add takes them (ref_index .. use), and with them mapq[i], an
 * int32 in 0..255, and clip[2 * i], clip[2 * i + 1] in [0, 2^42), the soft-clipped bases before and after
 * read[read_begin[i] .. read_end[i]).  ref / ref_off are the n_refs reference sequences as ASCII (ref_off[0] may be any
 * position of `ref`; ref_off never decreases); they give the rows.  A record's position in its read counts from the start
 * of SEQ: p = clip[2 * i] + start[2 * i + 1] + offset, offset = the read bases its cigar has consumed.  A run is a cigar
 * operation of length >= 1; every run is taken alone (2I3I is two I runs).  Over the counted records:
 *   mapq_hist[256]: one count per record.
 *   win_mapq[W][2]: [0] the M columns in the window, [1] the sum of the record's MAPQ over those columns; an M run adds
 *     overlap and overlap x mapq to each window it overlaps.
 *   pos_base[336][5]: every read base an M or I run consumes, at [bin(p)][code].
 *   clip_hist[336]: every soft-clipped read position at bin(p): the positions [0, clip[2 * i]) and the clip[2 * i + 1]
 *     positions from clip[2 * i] + (read_end[i] - read_begin[i]) on.
 *   gc_hist[102]: one count per record whose read[read_begin[i] .. read_end[i]) is not empty, over those bases, by the
 *     column rule of npr_read_quality's gc_hist.
 *   indel[2][5]: kind (0 an I run, 1 a D run) by class, below.      indel_len[2][336]: kind by bin(run length).
 *   totals[NPR_AQ_TOTALS = 8]: records counted, M columns, I runs, inserted bases, D runs, deleted bases, soft-clipped
 *     bases, records with a clip.
 * Classes (NPR_AQ_HOMOPOLYMER = 3): 0..3 = inside a homopolymer of A C G T, 4 = everything else.  x = the reference row of
 * the next column at the run (for an I run before the record's first column: the record's start).  For a code b < 4,
 * l = how many of the rows x - 1, x - 2, ... in a row hold code b, r = how many rows in a row hold b to the right, from x
 * for an I run and from x + length for a D run; both are counted inside the record's own sequence only and stop at
 * NPR_AQ_HOMOPOLYMER.  An I run whose inserted read bases all have one code b < 4 is class b when l + r >= 3; a D run whose
 * deleted reference bases all have one code b < 4 is class b when l + length + r >= 3; every other run is class 4.
 * Invalid records, the rule of npr_pileup_add: a selected record that is malformed (as there; also a MAPQ outside 0..255 or
 * a clip outside its range) or whose cigar runs past its read or its reference sequence adds NOTHING -- it is checked before its
 * first add -- and makes the call return NPR_ERR_INVALID; the other records are counted and every table is written.
 * Checked on the host, nothing written: a bad n_windows, n_refs < 0 or ref_off that decreases, a null pointer the call
 * needs, operation offsets that decrease.  n_reads == 0 is legal (zero tables). */
#define NPR_AQ_MAX_WINDOWS 65536
#define NPR_AQ_WIN_WORDS 8
#define NPR_AQ_TOTALS 8
#define NPR_AQ_HOMOPOLYMER 3
#define NPR_AQ_TILE 2048 /* consecutive rows a workgroup of the coverage kernel takes */
int32_t npr_pileup_coverage(npr_pileup *pl, const uint8_t *ref, const int64_t *ref_off, int32_t n_windows,
                            int64_t *win /* [n_windows][NPR_AQ_WIN_WORDS] */, int64_t *depth_hist /* [NPR_RQ_POS_BINS] */,
                            int64_t *start_hist /* [NPR_RQ_POS_BINS] */, int64_t *totals /* [NPR_AQ_TOTALS] */);
int32_t npr_align_quality(npr_ctx *ctx, int64_t n_reads, const int32_t *ref_index, const uint8_t *read, const int64_t *read_begin,
                          const int64_t *read_end, const int32_t *ops, const int64_t *ops_off, const int64_t *start, const uint8_t *use,
                          const int32_t *mapq, const int64_t *clip /* [n_reads][2] */, int64_t n_refs, const uint8_t *ref,
                          const int64_t *ref_off, int32_t n_windows, int64_t *mapq_hist /* [256] */,
                          int64_t *win_mapq /* [n_windows][2] */, int64_t *pos_base /* [NPR_RQ_POS_BINS][5] */,
                          int64_t *clip_hist /* [NPR_RQ_POS_BINS] */, int64_t *gc_hist /* [NPR_RQ_GC_COLS] */, int64_t *indel /* [2][5] */,
                          int64_t *indel_len /* [2][NPR_RQ_POS_BINS] */, int64_t *totals /* [NPR_AQ_TOTALS] */);

/* ---- exact-match seeding on the device: the local hits a base mapper hands to chainSamFile ----
 * The reference's base mappers (last, bwa, lastz, blasr) are external binaries and not part of this build; this is the build's own
 * mapper (nanopore_amd/mappers/seedMapper.py), behind the C ABI like every other stage.  Base codes are npr_encode_bases': A C G T ->
 * 0..3 in either letter case, anything else -> 4, and a code 4 matches NOTHING, not even another code 4.  For a reference sequence X, a
 * read Y in one orientation and parameters k <= min_len, a MATCH is (a, b, L) with X[a + t] == Y[b + t] (both codes < 4) for
 * 0 <= t < L, L >= min_len, that cannot be extended: a == 0 or b == 0 or X[a - 1], Y[b - 1] do not match, and likewise at a + L, b + L.
 * Matches never cross from one reference sequence into the next.  The forward strand is the read as given, the reverse strand its
 * reverse complement, and b counts in that orientation (what a FLAG 16 record holds).  The result for a read is the SET of all its
 * matches against every reference sequence on the strands asked for, as rows of four int32 -- reference index, a, b | strand << 31
 * (strand 1 = reverse), L -- sorted by (strand, reference index, a, b): the same from run to run.  8 <= k <= 32 and
 * k <= min_len < 2^31, NPR_ERR_INVALID otherwise.  k decides what the index holds (the positions whose next k bases are all A C G T,
 * bucketed by the first min(k, 12) of them); which matches exist is decided by min_len alone.  A repeat of the reference is never
 * masked: a read position inside a homopolymer run meets every position of the run. */
typedef struct npr_seed_index npr_seed_index;
/* The index of n_refs ASCII sequences (sequence i = ref[ref_off[i] .. ref_off[i + 1]), as for npr_kmer_counts), built on the device
 * and kept there until it is destroyed.  It belongs to its context and must be destroyed before it; calls on it count as calls on the
 * context.  n_refs == 0 and sequences shorter than k are legal and never match.  Fewer than 2^31 - 64 bases and sequences together. */
int32_t npr_seed_index_create(npr_ctx *ctx, int32_t k, int64_t n_refs, const uint8_t *ref, const int64_t *ref_off, npr_seed_index **out);
void npr_seed_index_destroy(npr_seed_index *index);
/* The matches of n_reads reads: read i = text[begin[i] .. end[i]), a span inside a larger text as npr_kmer_counts_groups takes them.
 * strands: 1 forward, 2 reverse, 3 both.  hit_off[n_reads + 1] is always filled: the rows of read i are hits[4 * hit_off[i] ..
 * 4 * hit_off[i + 1]).  hits (cap rows of four int32; may be NULL with cap 0) is written only when all rows fit: returns the number of
 * rows (>= 0), or NPR_ERR_CAPACITY when there are more than cap -- hit_off[n_reads] then says how many, and hits is not touched.
 * n_reads == 0, empty reads and reads shorter than k are legal and have no rows.  NPR_ERR_INVALID (nothing written): a bad min_len or
 * strands, a span that ends before it begins, 2^31 - 64 read bases and reads together or more in one call. */
int64_t npr_seed_matches(npr_seed_index *index, int64_t min_len, int32_t strands, int64_t n_reads, const uint8_t *text, const int64_t *begin,
                         const int64_t *end, int64_t *hit_off, int32_t *hits, int64_t cap);
/* The rows npr_seed_matches returned as the SAM records of a base mapper, one per match, in row order: QNAME \t FLAG \t RNAME \t POS \t 255
 * \t CIGAR \t * \t 0 \t 0 \t SEQ \t * \n with QNAME = text[name_span[2 * i] .. name_span[2 * i + 1]) of the row's read i, FLAG 0 or 16,
 * RNAME = entry `reference index` of the rnames list (CSR), POS = a + 1, CIGAR = <b>H<L>M<rest>H with rest = read length - b - L and
 * clips of length 0 left out, SEQ = the L matched bases in the strand's orientation, letters as they stand in the text and
 * complemented for the reverse strand.  Hard clips keep a record at tens of bytes where soft clips would repeat the whole read in
 * every one.  Record q lands at out[rec_off[q] .. rec_off[q + 1]), rec_off[hit_off[n_reads] + 1]; out == NULL: only the offsets.
 * Returns the total length, NPR_ERR_CAPACITY when cap is smaller, NPR_ERR_INVALID for a row outside its read or the reference list.
 * Threaded host code, no GPU needed. */
int64_t npr_seed_sam_text(int64_t n_reads, const uint8_t *text, const int64_t *name_span, const int64_t *begin, const int64_t *end,
                          const char *rnames, const int64_t *rname_off, int64_t n_refs, const int64_t *hit_off, const int32_t *hits,
                          int64_t *rec_off, char *out, int64_t cap);

/* ---- chaining of seed rows on the device: the guide alignments chainSamFile makes of a base mapper's local hits ----
 * The co-linear chains of the rows npr_seed_matches returned (csrc/npr_seedchain.hip), one per (read, reference) that has rows, all reads
 * of a call at once; npr_chain_hits + npr_chain_merge below state the same rule for one (read, reference) on the host.
 * ROWS.  A row is (reference index r, a, b | strand << 31, L): the block of reference positions [a, a + L) against read positions
 * [b, b + L) in that strand's orientation, of score L.  Rows need not be maximal matches; any rows are legal that satisfy, for read i:
 * sorted by (strand, r, a, b) (equal neighbours allowed), 0 <= r < n_refs, L >= 1, a >= 0, a + L <= ref_len[r], b + L <= read_len[i];
 * lengths below 2^31; hit_off starts at 0 and never decreases; max_gap >= 0.  Anything else: NPR_ERR_INVALID, decided on the host in one
 * pass over the rows before any output is written and before any kernel indexes with them.
 * RULE (the reference's chainFn, nanopore/analyses/utils.py:388-426).  Within one (read, reference) order the rows by (a, strand, b),
 * row order among equals -- the stable sort by first reference position of the SAM order.  Row j may precede row i when j sorts before
 * i, both lie on one strand, a_i > a_j + L_j - 1, b_i > b_j + L_j - 1 and (a_i - (a_j + L_j - 1)) + (b_i - (b_j + L_j - 1)) <= max_gap.
 * best_i = L_i + the largest best_j of such j (none: L_i); among equally good j the one that sorts first.  The chain ends at the row of
 * largest best, among equals -- across both strands -- the one that sorts last, and is followed back from there.  The reference compares
 * SIGNED read coordinates (utils.py _blockCoordinates): on the reverse strand those are b minus the constant read length - 1, so b in
 * the strand's orientation compares identically and is what is used here.
 * GUIDE.  What npr_chain_merge gives for the chain's blocks over ref_len[r] x read_len[i]: before every block, between blocks and after
 * the last one a D for the reference bases and then an I for the read bases not covered, lengths of 0 left out, neighbours of one kind
 * merged (two blocks adjacent on one diagonal are one M).  It spans exactly ref_len[r] x read_len[i]; a chain of m rows has at most
 * 3 m + 2 op pairs.
 * OUTPUT.  The chains of read i are chains[4 * chain_off[i] .. 4 * chain_off[i + 1]) in ascending reference index, each (r, strand,
 * score, rows in the chain); chain c's guide is the (op, length) pairs ops[2 * ops_off[c] .. 2 * ops_off[c + 1]) with NPR_OP_M / I / D:
 * the layout npr_batch_create* takes as guide_off / guide_ops.  Returns the number of chains (>= 0).
 * CAPACITY, as npr_seed_matches: chain_off[n_reads + 1] is filled whenever the rows are valid; chains (cap_chains rows of four), ops_off
 * [cap_chains + 1] and ops (cap_ops pairs) are written only when everything fits.  More chains than cap_chains (or chains / ops_off
 * NULL): NPR_ERR_CAPACITY, chain_off[n_reads] says how many, nothing else is written and nothing runs on the device.  The chains fit
 * but not the op pairs: NPR_ERR_CAPACITY and ops_off[0] alone receives the number of pairs needed (it is 0 in every successful result,
 * so the two cannot be confused).  n_reads == 0 and reads without rows are legal; without any chain the result is 0 and ops_off[0] = 0
 * when ops_off is given. */
int64_t npr_seed_chains(npr_ctx *ctx, int64_t max_gap, int64_t n_reads, const int64_t *read_len, int64_t n_refs, const int64_t *ref_len,
                        const int64_t *hit_off, const int32_t *hits, int64_t *chain_off, int32_t *chains, int64_t cap_chains,
                        int64_t *ops_off, int32_t *ops, int64_t cap_ops);
/* The chains as the records chainSamFile writes, one per chain: QNAME \t FLAG \t RNAME \t 1 \t 255 \t CIGAR \t * \t 0 \t 0 \t SEQ \t * \n
 * with QNAME, RNAME as npr_seed_sam_text takes them, FLAG 0 or 16 by the chain's strand, CIGAR the text of its op pairs (operations 0..8
 * = MIDNSHP=X; "*" without any), SEQ the whole read text[begin[i] .. end[i]) as it stands, reversed and complemented (A <-> T, C <-> G
 * in either case, everything else kept) for strand 1.  Records come in the file order of chainSamFile: by (reference index, QNAME as
 * bytes), NOT in chain order: record k lands at out[rec_off[k] .. rec_off[k + 1]), rec_off[chain_off[n_reads] + 1]; out == NULL: only
 * the offsets.  Returns the total length, NPR_ERR_CAPACITY when cap is smaller, NPR_ERR_INVALID for offsets that decrease, a chain
 * outside the reference list, a strand other than 0 / 1, an operation outside 0..8, a negative length -- and for two reads of one name:
 * their order would be undefined, and the pipeline makes names unique before it maps.  Threaded host code, no GPU needed. */
int64_t npr_seed_chain_sam_text(int64_t n_reads, const uint8_t *text, const int64_t *name_span, const int64_t *begin, const int64_t *end,
                                const char *rnames, const int64_t *rname_off, int64_t n_refs, const int64_t *chain_off, const int32_t *chains,
                                const int64_t *ops_off, const int32_t *ops, int64_t *rec_off, char *out, int64_t cap);

/* ---- reads to rows, chains and guides in one call, the rows never leaving the device ----
 * npr_seed_matches followed by npr_seed_chains, as one object that owns its device buffers: the reads are encoded and matched as
 * npr_seed_matches does, and what that call and npr_seed_chains do on the host between the kernels happens on the device
 * (csrc/npr_seedmap.hip): the reads' row counts are scanned into hit_off, every read's rows are sorted by (strand, reference index, a, b)
 * where the match kernel wrote them -- a read of at most NPR_SEED_MAP_LDS_ROWS rows in the LDS of one workgroup, a longer one by the same
 * workgroup in global memory; no read length and no row count is refused -- and the (read, reference) chain spans are found in the
 * sorted rows; then the chain kernels run on the rows where they lie.  The host reads back three totals (rows, chains, op pairs).
 * The arrays are DEFINED by the two calls: hit_off, hits are what npr_seed_matches returns for the same index, min_len, strands and
 * reads; chain_off, chains, ops_off, ops are what npr_seed_chains returns for those rows with read_len[i] = end[i] - begin[i], the
 * index's own sequence lengths as ref_len, and max_gap.  The rows are valid by construction and are not looked at again.
 * Errors are those of the two calls (a bad min_len, strands or max_gap, a span that ends before it begins, 2^31 - 64 read bases and
 * reads together or more): NPR_ERR_INVALID, *out = NULL, nothing launched.  n_reads == 0, empty reads, reads shorter than k and reads
 * without a match are legal: the result then has chain_off all zero and ops_off[0] == 0.
 * The map belongs to the index's context (not to the index) and must be destroyed before it; calls on it count as calls on the
 * context.  npr_seed_map_counts: counts[0..2] = rows, chains, guide op pairs.  npr_seed_map_fetch copies what is asked for to the host
 * -- hit_off [n_reads + 1], hits [rows][4], chain_off [n_reads + 1], chains [chains][4], ops_off [chains + 1], ops [pairs][2]; a NULL
 * pointer is not fetched -- any number of times. */
#define NPR_SEED_MAP_LDS_ROWS 4096 /* 16 bytes a row: 64 KB of LDS */
typedef struct npr_seed_map npr_seed_map;
int32_t npr_seed_map_create(npr_seed_index *index, int64_t min_len, int32_t strands, int64_t max_gap, int64_t n_reads, const uint8_t *text,
                            const int64_t *begin, const int64_t *end, npr_seed_map **out);
int32_t npr_seed_map_counts(const npr_seed_map *m, int64_t counts[3]);
int32_t npr_seed_map_fetch(npr_seed_map *m, int64_t *hit_off, int32_t *hits, int64_t *chain_off, int32_t *chains, int64_t *ops_off,
                           int32_t *ops);
void npr_seed_map_destroy(npr_seed_map *m);

/* Expected base counts per reference position from the posterior pairs of a finished batch, on the device (SURVEY.md 8f
 * next #4): what marginAlignSnpCaller.py:150-155 collates from the --outputAllPosteriorProbs files, one text line at a time:
 * every pair (refPos, readPos, p) of a selected read adds p to expect[(first row of its reference + refPos) * 4 + base] for
 * the read's base at readPos (A C G T; other bases add nothing) and sets seen[...].  use[i] != 0 selects read i (NULL: all) --
 * the caller's coverage sampling; the reference table is n_refs sequences of ref_len[k] positions, rows in that order.
 * Accumulated in 64-bit fixed point (units of 2^-40): a sum is the exact sum of its fp32 terms whatever the order, so the
 * table is the same from run to run and equals a sequential double-precision sum of the same pairs. */
int32_t npr_batch_base_expectations(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, double *expect,
                                    uint8_t *seen);

/* ---- SNP calls on the device: the calling step of MarginAlignSnpCaller (marginAlignSnpCaller.py:18-23, :163-197) ----
 * A table has one row per reference position (rows laid out as for npr_batch_base_expectations and npr_pileup_create) with four
 * non-negative base weights w[A C G T], a `seen` flag, the reference base code and the true base code (npr_encode_bases' codes,
 * 4 = not A/C/G/T).  Per row and error model m:
 *   not seen                     -> not_called += 1, nothing else
 *   total = ((w0+w1)+w2)+w3 == 0, or the reference base is not A/C/G/T -> nothing
 *   otherwise  log p[c] = log evolution[ref][c] + sum_o (w[o] / total) log error_m[c][o], normalised over the four candidates c
 *              (fp64), and every candidate c != ref is one call with bin = rint(100 p[c]) (round half to even, 0..100):
 *              true_pos[bin] += 1 when true != ref and true == c, else false_pos[bin] += 1;  rows_called += 1.
 * What leaves the device is this structure per model: the cumulative sums of the two histograms from the top are the
 * curves the reference computes from its lists of calls.  Counts are integers: the same from run to run.
 * evolution16 ([reference][candidate]) and error16 ([model][candidate][observed]) are PROBABILITIES; the library takes the
 * logs.  A zero in evolution16 makes that candidate impossible (p = 0).  NPR_ERR_INVALID, with `out` untouched: n_models
 * outside 1..NPR_SNP_MAX_MODELS, an error16 entry that is not a finite number above zero (the host path's 0 * log 0 is a
 * NaN), an evolution16 entry that is negative or not finite, or a row of evolution16 that is all zero.
 * true_code == NULL: the truth is the reference, every call is a false positive. */
#define NPR_SNP_BINS 101
#define NPR_SNP_MAX_MODELS 4
typedef struct npr_snp_calls {
    int64_t true_pos[NPR_SNP_BINS];   /* calls with rint(100 p) == bin that name the held-out base */
    int64_t false_pos[NPR_SNP_BINS];  /* every other call */
    int64_t not_called;               /* rows never seen */
    int64_t rows_called;              /* rows that produced their three calls */
} npr_snp_calls;
/* any table given on the host: rows x 4 weights (finite, >= 0: NPR_ERR_INVALID otherwise), seen, ref / true codes */
int32_t npr_snp_calls_table(npr_ctx *ctx, int64_t rows, const double *weights, const uint8_t *seen, const uint8_t *ref_code,
                            const uint8_t *true_code, int32_t n_models, const double *evolution16,
                            const double *error16 /* [n_models][16] */, npr_snp_calls *out /* [n_models] */);
/* the posterior expectations of a finished all-posteriors batch, selected by use[] (arguments, state and validity rules as for
 * npr_batch_base_expectations), read where k_base_expectations left them: the table never leaves the device.
 * ref_code / true_code: [sum ref_len]. */
int32_t npr_batch_snp_calls(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const uint8_t *ref_code,
                            const uint8_t *true_code, int32_t n_models, const double *evolution16, const double *error16,
                            npr_snp_calls *out);
/* the aligned-base frequencies of a pileup: w = words 0-3, seen = (words 0-4 summed != 0).  ref_code / true_code: one per row
 * of the pileup's table. */
int32_t npr_pileup_snp_calls(npr_pileup *pl, const uint8_t *ref_code, const uint8_t *true_code, int32_t n_models,
                             const double *evolution16, const double *error16, npr_snp_calls *out);

/* ---- SNP variants on the device: the calls themselves and a consensus, from the same posteriors ----
 * The tables, the row layout, evolution16 and the posterior are those of the npr_*_snp_calls block above, for ONE error model
 * (error16 [candidate][observed], 16 entries) and without a truth.  Instead of histograms two things leave the device
 * (csrc/npr_snpcall.hip: k_snp_variants_count, a scan, k_snp_variants_emit): a best base and its quality per row, and the list of calls.
 * A row is CALLABLE when it is seen, total = ((w0+w1)+w2)+w3 != 0 and its reference base is A/C/G/T.  For a callable row, in fp64:
 *   lp[c]  = log evolution[ref][c] + sum_o (w[o] / total) log error[c][o]     (o = 0..3 added in that order, starting from 0)
 *   e[c]   = exp(lp[c] - max_c lp[c]),   sum = ((e0+e1)+e2)+e3,   p[c] = e[c] / sum
 * BEST.  best[row] = the candidate of largest lp; among candidates whose lp are exactly equal, the reference base if it is one of
 * them, else the one of lowest code.  qual[row] = min(93, floor(-10 log10(q))) with q = (the e of the three other candidates, added
 * in ascending code) / sum; q == 0 gives 93.  A row that is not callable has best = 4 and qual = 0.
 * CALLS.  Every candidate c != ref of a callable row with p[c] >= threshold is one call (row, c, p[c]).  The calls come in ascending
 * (row, candidate code) order in call_row / call_alt / call_p; the arrays are the same from run to run.  threshold is a finite number
 * in [0, 1].  A zero in evolution16 makes p[c] = 0: such a candidate is no call at any threshold above 0 and IS a call at threshold
 * 0, where every callable row has its three calls.
 * OUTPUT AND CAPACITY, as npr_seed_matches.  best and qual ([rows] each) may be NULL and are then not copied.  The return value is the
 * number of calls (>= 0), which *n_calls receives too; the call arrays hold cap entries (they may be NULL with cap 0).  More calls
 * than cap: NPR_ERR_CAPACITY, *n_calls says how many, the call arrays are not touched -- best and qual are filled in both cases.
 * rows == 0 is legal (no calls).  NPR_ERR_INVALID, with EVERY output untouched: a threshold outside [0, 1] or not a number, cap < 0,
 * n_calls NULL, an error16 entry that is not a finite number above zero, an evolution16 entry that is negative or not finite or a row
 * of it that is all zero -- and whatever the npr_*_snp_calls call on the same table refuses (a weight that is negative or not finite,
 * missing base codes; npr_batch_snp_variants before npr_batch_finish: NPR_ERR_STATE). */
int64_t npr_snp_variants_table(npr_ctx *ctx, int64_t rows, const double *weights, const uint8_t *seen, const uint8_t *ref_code,
                               const double *evolution16, const double *error16 /* [16] */, double threshold, uint8_t *best, uint8_t *qual,
                               int64_t *call_row, uint8_t *call_alt, double *call_p, int64_t cap, int64_t *n_calls);
/* the posterior expectations of a finished all-posteriors batch (table and arguments as for npr_batch_snp_calls) */
int64_t npr_batch_snp_variants(npr_batch *b, const uint8_t *use, int64_t n_refs, const int64_t *ref_len, const uint8_t *ref_code,
                               const double *evolution16, const double *error16, double threshold, uint8_t *best, uint8_t *qual,
                               int64_t *call_row, uint8_t *call_alt, double *call_p, int64_t cap, int64_t *n_calls);
/* the aligned-base frequencies of a pileup (table as for npr_pileup_snp_calls) */
int64_t npr_pileup_snp_variants(npr_pileup *pl, const uint8_t *ref_code, const double *evolution16, const double *error16,
                                double threshold, uint8_t *best, uint8_t *qual, int64_t *call_row, uint8_t *call_alt, double *call_p,
                                int64_t cap, int64_t *n_calls);

/* Baum-Welch E-step over the staged batch with the models currently installed: what
 * `cactus_realign --outputExpectations` produces per alignment and cactus_expectationMaximisation sums over all of
 * them in every EM iteration (nanopore/analyses/utils.py:509-528).  T_exp[slot*25 + from*5 + to] and
 * E_exp[slot*80 + state*16 + x*4 + y] receive the expected transition / emission counts of the reads that use model
 * `slot` (gap states: a base's count is spread evenly over the other index), loglik[slot] the summed natural-log
 * likelihood.  Arrays are NPR_MAX_MODELS slots long and are overwritten.  The band / split plan of the batch is
 * unaffected, so the call can be repeated after npr_set_hmm for the next iteration. */
int32_t npr_batch_expectations(npr_batch *b, double *T_exp, double *E_exp, double *loglik, float *kernel_ms);

/* debugging / parity aid: dense per-cell match-state forward and backward values of read i, task-major,
 * band order, as (mantissa, exponent) block-floating-point pairs (value = mant * 2^exp).  Runs the read
 * again on the device.  Buffers sized npr_read_result.cells. */
int32_t npr_batch_dense(npr_batch *b, int64_t read_index, float *Fm_v, int32_t *Fm_e, float *Bm_v,
                        int32_t *Bm_e, int64_t cap);

/* debugging / parity aid for the north-star kernel: the forward match values k_dp_rs (row-scaled arithmetic: one exponent per
 * anti-diagonal row, renormalised every 16 rows) leaves in its scratch for the backward sweep, read i, task-major, band order,
 * as (value, exponent of the cell's row): F = value * 2^exponent.  A cell more than ~211 binary orders below its rows' maximum
 * is 0 (flushed) -- the range certificate (npr_batch_segment_arith reports the tasks that ran again without it) bounds the
 * posterior mass such cells can carry by 2^-60.  Runs the read's tasks again, one at a time; NPR_ERR_STATE when a segment of
 * the read is not in a class k_dp_rs runs.  Buffers sized npr_read_result.cells. */
int32_t npr_batch_rs_forward(npr_batch *b, int64_t read_index, float *Fm_v, int32_t *Fm_e, int64_t cap);

/* Test aid: npr_batch_create expands band rows, frame schedules, stripe tables and row offsets on the device; this
 * recomputes every task of the batch with the host planner (the npr_plan_* functions below, the ones the tests pin
 * against the oracle) and compares entry by entry.  Returns the number of tasks that differ (0 = identical) or NPR_ERR_*. */
int64_t npr_batch_plan_check(npr_batch *b, const int32_t *guide_ops /* as given to npr_batch_create: a batch keeps no copy */);

/* One call = create + run + finish + copy-out + destroy, for callers that do not need staging. */
int32_t npr_realign_batch(npr_ctx *ctx, const npr_params *params, int64_t n_reads, int64_t n_refs,
                          const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                          const uint8_t *read, const int64_t *read_off, const int32_t *guide_ops,
                          const int64_t *guide_off, const int32_t *model_slot, npr_read_result *results,
                          int64_t *ops_off, int32_t *ops, int64_t cap_op_pairs);

/* ---- host logic, callable without a GPU (unit tests of the boundary) ---- */
/* band / segmentation of one read (cactus_realign stages a5.1-a5.2 of SURVEY.md 8a) */
int32_t npr_plan_create(const npr_params *params, int64_t lX, int64_t lY, const int32_t *guide_ops,
                        int64_t n_guide_ops, npr_plan **out);
void npr_plan_destroy(npr_plan *pl);
int32_t npr_plan_segments(const npr_plan *pl);
/* info8 = xs, ys, xe, ye, ragged_start, ragged_end, D, cells */
int32_t npr_plan_segment_info(const npr_plan *pl, int32_t seg, int64_t *info8);
/* lattice-clipped band: lo[D+1], n[D+1] */
int32_t npr_plan_segment_band(const npr_plan *pl, int32_t seg, int32_t *lo, int32_t *n);
/* Frame schedule of the register kernels for one segment (host logic, for inspection and tests): the kernels hold a
 * frame of `slots` lattice points of the current anti-diagonal, slot j = (x0 + j, y0 - j), which takes an X-step
 * (x0 += 1) into every odd anti-diagonal and a Y-step (y0 += 1) into every even one and may be rebased by one slot
 * before a step.  Per anti-diagonal d (arrays of D+1): jlo[d] = slot of the first band cell, rebase[d] in {-1,0,+1} =
 * rebase applied before the step into d (+1, towards higher x-y, only before X-steps; -1 only before Y-steps),
 * row_off[d] = offset (cells) of its row in the forward scratch, rows holding whole lanes of `slots_per_lane` slots;
 * *cells = scratch cells of the segment.  slots = 64 * slots_per_lane for k_dp_stair (slots_per_lane 1, 2, 4);
 * 512, 1024 (slots_per_lane 2), 2048 or 3072 (4) for k_dp_wide.  NPR_ERR_BAND_TOO_WIDE when the band cannot be
 * followed with that frame. */
int32_t npr_plan_frame_schedule(const npr_plan *pl, int32_t seg, int32_t slots, int32_t slots_per_lane, int32_t *jlo,
                                int32_t *rebase, uint32_t *row_off, int64_t *cells);
/* Stripe table of the wide-band kernel (k_dp_tile) for one segment (host logic, for inspection and tests): the lattice
 * columns 0..lX are cut into stripes of at most 64 * slots_per_lane columns, one wavefront sweeps a stripe anti-diagonal
 * by anti-diagonal.  stripes5[5 * k ..] = first column, columns, first / last anti-diagonal with band cells in the
 * stripe, index of its first row in the task's forward scratch (one row per anti-diagonal of a stripe); *rows = rows of
 * the segment.  Returns the number of stripes (stripes5 == NULL: only that), NPR_ERR_CAPACITY when cap is smaller. */
int32_t npr_plan_stripes(const npr_plan *pl, int32_t seg, int32_t slots_per_lane, int32_t *stripes5, int32_t cap, int64_t *rows);
/* MEA chain + cigar from sparse posteriors (stage a5.6).  Returns number of op pairs or NPR_ERR_*. */
int64_t npr_mea_cigar(int64_t lX, int64_t lY, const int32_t *x, const int32_t *y, const float *p, int64_t n,
                      double gap_gamma, double match_gamma, int32_t *ops, int64_t cap_pairs, double *score);
/* mean posterior over the M columns of a cigar (stage a5.7) */
int32_t npr_rescore(const int32_t *guide_ops, int64_t n_guide_ops, const int32_t *x, const int32_t *y,
                    const float *p, int64_t n, double *score);
/* Chaining of local hits (stage before the realigner, nanopore/analyses/utils.py:388-426 chainFn): hit k spans reference
 * [ref_start, ref_end] and signed read positions [read_start, read_end] (last aligned pair inclusive, reverse-strand
 * positions negated as AlignedPair.getSignedReadPos does), scores `score` (aligned pairs).  Writes the indices of the
 * highest-scoring co-linear chain, in chain order, to chain[0 .. return value); same chain as the reference's quadratic
 * scan, ties included, found with a sort and a windowed scan.  Host code. */
int64_t npr_chain_hits(int64_t n, const int64_t *ref_start, const int64_t *read_start, const int64_t *ref_end,
                       const int64_t *read_end, const uint8_t *reverse, const int64_t *score, int64_t max_gap, int64_t *chain);
/* The global alignment a chain stands for (mergeChainedAlignedReads, nanopore/analyses/utils.py:295-386): block k = a local
 * alignment whose first aligned pair is at reference position ref_pos[k] and position read_pos[k] of SEQ (its leading hard +
 * soft clips; the same on either strand), M / I / D operations ops[2 * ops_off[k] ..).  Unaligned reference / read bases
 * between, before and after the blocks become D / I operations, neighbours of one kind are merged; the result spans
 * ref_len x read_len (the asserts of utils.py:381-382).  Returns the number of (op, length) pairs written to out_ops,
 * NPR_ERR_INVALID when the blocks are out of order, overlap or run past the sequences (the reference's asserts),
 * NPR_ERR_CAPACITY when cap_pairs is too small (ops + 2 per block + 2 always suffices).  Host code. */
int64_t npr_chain_merge(int64_t n_blocks, const int64_t *ref_pos, const int64_t *read_pos, const int64_t *ops_off, const int32_t *ops,
                        int64_t ref_len, int64_t read_len, int32_t *out_ops, int64_t cap_pairs);
/* SAM CIGAR text of n op lists (CSR as returned by npr_batch_ops): what realignSamFile3TargetFn assigns to aR.cigar
 * and pysam prints (nanopore/analyses/utils.py:597-605), for a writer that splices 50 k records at once.  String i is
 * out[str_off[i] .. str_off[i+1]) (no terminator; "*" for an empty list).  out == NULL: only the offsets; returns the
 * total length, NPR_ERR_CAPACITY when cap is smaller, NPR_ERR_INVALID for an op outside M/I/D.  Threaded. */
int64_t npr_format_cigars(int64_t n, const int64_t *ops_off, const int32_t *ops, int64_t *str_off, char *out, int64_t cap);
/* The same from packed cigars, one 32-bit word per operation (length << 2 | op -- the form the ranks of a sharded job send
 * to rank 0, nanopore_amd/dist.py): list i = words[word_off[i] .. word_off[i] + n_ops[i]), the lists in any order and
 * anywhere in `words`, so the gathered payloads need no merge copy before the SAM is written. */
int64_t npr_format_cigars_packed(int64_t n, const int64_t *word_off, const int64_t *n_ops, const uint32_t *words, int64_t *str_off,
                                 char *out, int64_t cap);
/* The same text made ON THE DEVICE (csrc/npr_cigtext.hip): host arrays in, host arrays out, the words uploaded, counted, scanned and
 * formatted by kernels in between.  The contract of npr_format_cigars_packed word for word -- out == NULL: only the offsets; returns the
 * total length; NPR_ERR_CAPACITY when cap is smaller (the offsets are written); NPR_ERR_INVALID for an op outside M/I/D or a negative
 * n_ops, and then neither out nor str_off is written.  It exists so that the kernels can be tested on lists no batch produces; a caller
 * with cigars on the host wants npr_format_cigars_packed. */
int64_t npr_cigar_text_packed(npr_ctx *ctx, int64_t n, const int64_t *word_off, const int64_t *n_ops, const uint32_t *words, int64_t *str_off,
                              char *out, int64_t cap);
/* The cigars npr_batch_ops_packed would return, as that text: string i = cigar of read i ("*" for a read that failed), str_off[n_reads + 1];
 * out == NULL: only the offsets; returns the total length, NPR_ERR_CAPACITY when cap is smaller, NPR_ERR_STATE before npr_batch_finish.
 * After npr_batch_finish in every mode.  The packed words are formatted where they lie while the copy the device MEA stage left on the
 * device is still valid (no other batch finished on the device since) and uploaded from the batch's host form otherwise (the host stage,
 * NPR_MODE_RESCORE_ORIGINAL, a later finish in between); under NPR_OPT_FINISH_TEXT the text is on the host already.  The first call makes
 * the text and keeps it with the batch: the sizing call and the fetching call cost one formatting. */
int64_t npr_batch_cigar_text(npr_batch *b, int64_t *str_off, char *out, int64_t cap);
/* The realigned SAM records themselves, as text: what realignSamFile3TargetFn's writer puts out for every record after
 * assigning the new cigar (nanopore/analyses/utils.py:591-609; pysam's AlignmentFile.write there), for a job that writes
 * 50 k records per rank at once.  Record i = QNAME \t FLAG \t RNAME \t POS \t MAPQ \t CIGAR \t * \t 0 \t 0 \t SEQ \t * \n with
 * QNAME = qnames[qname_off[i] .. qname_off[i+1]), RNAME = entry ref_index[i] of the rnames list, POS = pos[i] (1-based, as
 * printed), FLAG = flag[i] (NULL: 0), MAPQ = mapq[i] (NULL: 255), CIGAR = the packed list i as in npr_format_cigars_packed
 * ("*" when empty), SEQ = seq[seq_off[i] .. seq_off[i+1]) ("*" when empty).  Record i lands at out[rec_off[i] .. rec_off[i+1]).  out == NULL:
 * only the offsets; returns the total length, NPR_ERR_CAPACITY when cap is smaller, NPR_ERR_INVALID for a negative
 * number or an op outside M/I/D.  Threaded host code. */
int64_t npr_format_sam_records(int64_t n, const char *qnames, const int64_t *qname_off, const int32_t *flag, const char *rnames,
                               const int64_t *rname_off, const int32_t *ref_index, const int64_t *pos, const int32_t *mapq,
                               const int64_t *word_off, const int64_t *n_ops, const uint32_t *words, const char *seq, const int64_t *seq_off,
                               int64_t *rec_off, char *out, int64_t cap);
/* ASCII -> base codes 0..4 (A,C,G,T,N) */
void npr_encode_bases(const uint8_t *ascii, int64_t n, uint8_t *codes);

/* ---- bulk text ingest / splice: the file side of realignSamFile2TargetFn / realignSamFile3TargetFn ----
 * The reference walks the SAM file record by record in Python (pysam iterator + samIterator, nanopore/analyses/utils.py:287-293,
 * :563-570), builds one exonerate cigar per record (utils.py:168-180), and afterwards copies every record to the output with
 * only its CIGAR replaced (utils.py:591-609).  At 50 k records of 8 kb that loop is longer than the DP; these entry points do
 * the same over the whole text of the file (the caller maps or reads it), threaded, so that the records of a rank's shard go
 * from file bytes to the C ABI's batch arrays -- and the realigned cigars back into file bytes -- without a Python object
 * per record.  Host code; no GPU needed. */

/* Alignment lines of a SAM text: *header_end = offset of the first byte after the @-header lines; returns the number of
 * alignment lines (non-empty lines after the header).  span[2 * i], span[2 * i + 1] = [start, end) of line i without its
 * "\n" / "\r\n"; span == NULL: only count.  NPR_ERR_CAPACITY when cap (lines) is smaller. */
int64_t npr_sam_index(const char *text, int64_t len, int64_t *header_end, int64_t *span, int64_t cap);

/* Fields of n alignment lines (span as from npr_sam_index, possibly a sub-range: a rank's shard).  fields[i * NPR_SAM_COLS + c]:
 *   0 end of QNAME (it starts at span[2 * i])      1, 2  RNAME [start, end)       3, 4  CIGAR [start, end)
 *   5, 6 SEQ [start, end)                          7 FLAG     8 POS - 1 (0-based, pysam's aR.pos)     9 MAPQ
 *   10 tid = index of RNAME in the given name table (the @SQ order), -1 for "*" or a name not in it (column 15 says which)
 *   11, 12 [start, end) of the aligned part of SEQ in the text (soft clips cut off: aR.query, the sequence handed to
 *      cactus_realign, utils.py:570); empty for SEQ "*"
 *   13 operations M / I / D of the cigar (the guide: clips carry no operation, utils.py:173)
 *   14 reference bases the cigar consumes (aR.aend - aR.pos)
 *   15 NPR_OK; NPR_ERR_INVALID: fewer than 11 columns, a malformed number or cigar, or an operation outside M I D S H
 *      (the reference asserts `op in (0, 1, 2, 4, 5)`, utils.py:171; pysam's iterator raises on a line it cannot parse);
 *      NPR_SAM_NO_REFERENCE: RNAME is "*" -- the only records samIterator drops (utils.py:287-293);
 *      NPR_SAM_UNKNOWN_REFERENCE: RNAME names a sequence the table (the header's @SQ lines) does not have -- an error of
 *      the file (a SAM without its @SQ lines, a truncated header), never a record to drop silently
 * rnames / rname_off: the n_refs reference names, CSR.  Threaded. */
#define NPR_SAM_COLS 16
#define NPR_SAM_NO_REFERENCE 1
#define NPR_SAM_UNKNOWN_REFERENCE 2
int32_t npr_sam_parse(const char *text, const int64_t *span, int64_t n, const char *rnames, const int64_t *rname_off, int64_t n_refs,
                      int64_t *fields);
/* The guides of n parsed lines as the batch entry points take them: (op, length) pairs of the M / I / D operations of line i
 * at guide_ops[2 * guide_off[i] ..), guide_off = exclusive prefix sum of fields column 13 (made by the caller, n + 1 entries).
 * Lines whose column 15 is not NPR_OK are skipped. */
int32_t npr_sam_guides(const char *text, const int64_t *fields, int64_t n, const int64_t *guide_off, int32_t *guide_ops);
/* Output records: line i of the input with its CIGAR field replaced by the packed cigar i (one 32-bit word per operation,
 * length << 2 | op, list i = words[word_off[i] .. word_off[i] + n_ops[i]); "*" when empty), every other byte copied --
 * QNAME, FLAG, RNAME, POS, MAPQ, the mate fields, SEQ, QUAL and the tags exactly as the mapper wrote them, which is what
 * realignSamFile3TargetFn's `aR.cigar = ...; outputSam.write(aR)` produces (utils.py:597-605).  Each record ends in "\n".
 * Record i lands at out[rec_off[i] .. rec_off[i + 1]); out == NULL: only the offsets.  Returns the total length,
 * NPR_ERR_CAPACITY when cap is smaller, NPR_ERR_INVALID for an operation outside M / I / D.  Threaded. */
int64_t npr_sam_splice(const char *text, const int64_t *span, const int64_t *fields, int64_t n, const int64_t *word_off,
                       const int64_t *n_ops, const uint32_t *words, int64_t *rec_off, char *out, int64_t cap);

/* npr_sam_splice for cigars that are text already (npr_batch_cigar_text, npr_cigar_text_packed, npr_format_cigars_packed): line i with its
 * CIGAR field replaced by cigar_text[str_off[i] .. str_off[i + 1]), every other byte copied, each record ending in "\n".  Same return and
 * errors as npr_sam_splice, without the check of the operations (NPR_ERR_INVALID: offsets that decrease).  Threaded host code. */
int64_t npr_sam_splice_text(const char *text, const int64_t *span, const int64_t *fields, int64_t n, const int64_t *str_off,
                            const char *cigar_text, int64_t *rec_off, char *out, int64_t cap);

/* FASTA text (getFastaDictionary, utils.py:233-238): returns the number of records; rec[4 * k ..] = [start, end) of the
 * record's name (first word of the header line) and [start, end) of its sequence lines in the text, seq_len[k] = bases
 * (line ends and blanks not counted).  rec == NULL: only count.  NPR_ERR_CAPACITY when cap (records) is smaller. */
int64_t npr_fasta_index(const char *text, int64_t len, int64_t *rec, int64_t *seq_len, int64_t cap);
/* ... and the sequences themselves, contiguous: record k at out[seq_off[k] .. seq_off[k + 1]) (seq_off = prefix sum of
 * seq_len), line ends and blanks removed -- the reference table npr_batch_create takes.  Threaded over records. */
int32_t npr_fasta_pack(const char *text, const int64_t *rec, int64_t n, const int64_t *seq_off, uint8_t *out);
/* FASTQ text (getFastqDictionary, utils.py:240-245), four-line records: rec[4 * k ..] = [start, end) of the name (first
 * word after '@') and [start, end) of the sequence line.  rec == NULL: only count.  NPR_ERR_INVALID for a record that does
 * not start with '@' or whose third line does not start with '+'. */
int64_t npr_fastq_index(const char *text, int64_t len, int64_t *rec, int64_t cap);
/* ... and where the quality lines are: for the n records npr_fastq_index found (rec as it filled it), qual[2 * k ..] =
 * [start, end) of record k's fourth line, by the same line rules (the line ends at '\n' or at the end of the text, '\r' before
 * it left out).  A last record whose fourth line is missing gets an empty span at the end of the text.  NPR_ERR_INVALID when a
 * record's sequence span lies outside the text or its third line does not start with '+'. */
int32_t npr_fastq_qual_index(const char *text, int64_t len, const int64_t *rec, int64_t n, int64_t *qual /* [2 n] */);
/* Which of n names a SAM file maps (abstractUnmappedAnalysis.py:39-43: samIterator, then `not record.is_unmapped`): name i is
 * names_text[name_span[2 * i] .. name_span[2 * i + 1]); span / fields are the m alignment lines as npr_sam_index and
 * npr_sam_parse give them.  mark[i] is set to 1 when some line has QNAME bytes equal to name i (case-sensitive), column 15
 * NPR_OK and FLAG & 4 == 0; every name equal to the QNAME is marked, and nothing is ever cleared: marks of several files OR
 * together.  Returns the number of such lines whose QNAME is none of the names, or NPR_ERR_INVALID (nothing marked) when a
 * line's column 15 is NPR_ERR_INVALID or NPR_SAM_UNKNOWN_REFERENCE.  Host code, threaded over the lines. */
int64_t npr_names_mark(const char *names_text, const int64_t *name_span /* [2 n] */, int64_t n, const char *sam_text,
                       const int64_t *span, const int64_t *fields, int64_t m, uint8_t *mark /* [n], OR-ed into */);

/* ---- coordinate-sorted BAM and its BAI index from a SAM text (SAMv1 section 4 BAM, 4.1 BGZF, 5 indexing) ----
 * What the reference gets from samToBamFile, pysam.sort and pysam.index (nanopore/metaAnalyses/customTrackAssemblyHub.py:56-62).  The
 * BAM is BGZF with STORED deflate blocks by default (the file is about the size of the uncompressed stream); npr_bgzf_deflate and
 * npr_sam_bam_deflate write the same stream with every block COMPRESSED on the device (csrc/npr_deflate.hip).  The host parts
 * (npr_sam_parse_tail, npr_bam_tags, npr_bam_header, npr_bai_write: csrc/npr_bam_host.cpp, threaded, no GPU needed) read what
 * npr_sam_parse leaves aside and write the two small tables; the device parts (csrc/npr_bam.hip) order, measure, encode, frame and index.
 *
 * npr_sam_parse_tail: for the same n lines, tail[i * NPR_SAM_TAIL_COLS + c]:
 *   0 RNEXT as a tid: "=" gives the record's own tid (column 10 of `fields`), "*" or a name not in the table gives -1
 *   1 PNEXT - 1          2 TLEN          3, 4 QUAL [start, end)          5, 6 the optional fields [start, end): from the byte after the
 *   tab that ends QUAL to the end of the line (a "\r" before the line end is not part of it: the span is npr_sam_index's); empty (both
 *   the end of the line) when the line has 11 columns
 *   7 NPR_OK; NPR_ERR_INVALID: fewer than 11 columns; FLAG, POS, MAPQ, PNEXT or TLEN is not a decimal number; FLAG outside 0..65535,
 *     MAPQ outside 0..255, POS or PNEXT outside 0..2^29, TLEN outside -2^31+1..2^31-1; a QNAME of 0 or more than 254 bytes; a QUAL that
 *     is neither "*" nor as long as SEQ (a QUAL beside SEQ "*" must be "*").
 *   `fields` are the lines' rows as npr_sam_parse filled them (columns 5, 6 and 10 are read).  The cigar is not looked at here.
 *
 * npr_bam_tags: the optional fields of n lines as BAM auxiliary bytes; record i lands at out[tag_off[i] .. tag_off[i + 1]), tag_off[n + 1];
 *   out == NULL: only the offsets.  Returns the total length, NPR_ERR_CAPACITY when cap is smaller, NPR_ERR_INVALID for a malformed field.
 *   A line whose tail status is not NPR_OK has no bytes.  A field is TAG:TYPE:VALUE, TAG two bytes, fields separated by one tab; an empty
 *   field (two tabs in a row, a tab at the end) is malformed.  Output per field: the two TAG bytes, a type byte, the value:
 *   A one printable byte -> 'A' and the byte.    f a number strtof accepts whole -> 'f' and its 4 bytes.
 *   i a decimal integer in -2^31 .. 2^32 - 1 -> the SMALLEST of the types c C s S i I that holds it, and for a value >= 0 the unsigned
 *     type of a width before the signed one: 0..255 'C', 256..65535 'S', 65536..2^32-1 'I', -128..-1 'c', -32768..-129 's', below 'i'.
 *   Z the bytes as they are (spaces allowed, no tab) and a NUL.    H an even number of hex digits, stored like Z.
 *   B a subtype byte of c C s S i I f, then "," and a number for every element (none: an empty array): 'B', the subtype, the count as
 *     uint32, the elements in the subtype's width, little endian; an integer element outside its subtype's range is malformed.
 *
 * npr_bam_header: the bytes before the first record: "BAM\1", l_text, the header text, n_ref, and per @SQ line l_name (with its NUL),
 *   the name and its NUL, l_ref.  The text is the SAM header (`len` bytes, the @-lines as they stand in the file) with its @HD line
 *   changed: the value of its SO: field becomes "coordinate" (sorted != 0) or "unsorted" (SO: is appended when @HD has none); without an
 *   @HD line "@HD\tVN:1.0\tSO:coordinate\n" ("SO:unsorted") is put in front.  Names come from SN:, lengths from LN: (a decimal number
 *   in 1 .. 2^31 - 1).  out == NULL: only the length; ref_len (cap_refs entries, may be NULL) receives the lengths.  Returns the length;
 *   *n_refs the number of @SQ lines.  NPR_ERR_INVALID: no @SQ line, or one without SN: or a valid LN:; NPR_ERR_CAPACITY: cap or cap_refs.
 *
 * npr_bam_sort_order: the permutation that sorts n records by (tid, pos + 1, FLAG & 16 != 0): order[j] = the record at place j.  tid -1
 *   sorts after every other tid; pos -1 (POS 0) first within its tid; equal keys keep their input order (the sort is STABLE).  An LSD
 *   radix sort of 64-bit keys (tid' << 33 | (pos + 1) << 1 | reverse, tid' = largest tid + 1 for tid -1) with the record number as
 *   payload, 8 bits a pass, only as many passes as the largest possible key has bits: per pass the digit histograms of every workgroup,
 *   one prefix sum, one stable scatter whose ranks come from wavefront ballots and per-wavefront counts, never from the order in which
 *   atomics land.  n < 2^31, tid in -1 .. 2^30 - 1, pos in -1 .. 2^31 - 2: NPR_ERR_INVALID otherwise, nothing written.
 *
 * npr_bgzf_frame: `len` bytes as a BGZF stream.  Block b holds the payload data[b * P .. min(len, (b + 1) * P)), P = NPR_BGZF_PAYLOAD;
 *   a block of L payload bytes is, in order: 1f 8b 08 04, MTIME 0 (4 bytes), XFL 0, OS ff, XLEN 6 0, 'B' 'C' 2 0, BSIZE = L + 30 as
 *   uint16 (the block's length - 1); 01, LEN = L, ~LEN (uint16 each: one stored deflate block, final); the payload; CRC-32 of the payload
 *   (polynomial 0xEDB88320 reflected, initial value and final xor 0xFFFFFFFF) and ISIZE = L as uint32.  All little endian.  After the
 *   last block the 28-byte end-of-file block: 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00.
 *   len == 0 gives that block alone.  Returns the stream's length = len + 31 * ceil(len / P) + 28; out == NULL: only that;
 *   NPR_ERR_CAPACITY when cap is smaller, and then nothing is written.  The VIRTUAL OFFSET of byte u of the data is therefore
 *   ((u / P) * (P + 31)) << 16 | (u % P), in closed form; nothing below walks the blocks.
 *
 * npr_bgzf_deflate: the same stream in the same blocks (block b still holds data[b * P .. min(len, (b + 1) * P)), so the block of byte u is
 *   still u / P), every block's deflate data compressed by one workgroup, independently of every other block.  A block of L payload bytes is
 *   the 18 header bytes above with BSIZE = the block's length - 1; ONE FINAL BLOCK of raw DEFLATE (RFC 1951), the last byte filled with
 *   zero bits; CRC-32 and ISIZE = L as above.  After the last block the same end-of-file block.
 *   MATCHES are 3 .. 258 bytes long, 1 .. 32768 back, and never reach before the block's first byte.  The positions are taken in rounds of
 *   256 consecutive ones; a position p with 3 bytes left has two candidates: p - 1, and the largest position of an earlier round whose three
 *   bytes hash ((b0 | b1 << 8 | b2 << 16) * 0x9E3779B1 >> 20, 4096 entries) as p's do.  The longer match wins, the nearer on a tie.  The PARSE
 *   is greedy from position 0: the match of a position that has one of 3 or more bytes, else a literal.
 *   CODES.  The lengths of a Huffman code over the counts (literal/length: 286 symbols, distance: 30, code lengths: 19), ties broken by
 *   symbol number (the used symbols are ordered by (count, symbol); of two the earlier never has the shorter code).  When a length would
 *   exceed 15 bits (7 for the code-length alphabet), the codes per length are folded to the limit and, while the Kraft sum exceeds one, a
 *   code of the largest shorter length moves one bit down: a complete prefix code again.  No distance symbol: HDIST = 0 and one code of
 *   length zero; exactly one: one code of one bit.  The code lengths are sent one by one (symbols 16 / 17 / 18 are not used).
 *   CHOICE.  From the counts, before anything is emitted, the exact bits of (a) one dynamic-Huffman block over the parse, (b) one over the
 *   literals alone, (c) one stored block (8 L + 40).  The smallest is emitted; on a tie the later of a, b, c.  So no block exceeds L + 31
 *   bytes, and the stream never exceeds what npr_bgzf_frame returns.  The output is the same bytes from run to run.
 *   block_off (may be NULL) receives the file offset of every block and, last, of the end-of-file block: ceil(len / P) + 1 entries.  The
 *   VIRTUAL OFFSET of byte u is block_off[u / P] << 16 | (u % P); for u == len on a full last block that is the end-of-file block's offset,
 *   as in the stored layout.  out == NULL: returns an upper bound, the stored length (what npr_bgzf_frame returns).  NPR_ERR_CAPACITY when
 *   cap is below that bound, and then nothing is written.  Else returns the stream's actual length; no byte at or after it is touched.
 *
 * npr_deflate_last: of the last stream this context compressed (npr_bgzf_deflate or npr_sam_bam_deflate that returned a length), out[0 .. 3]
 *   = the blocks emitted as (a), (b), (c) and out[3] = the uncompressed stream's length; all 0 before the first.  NPR_ERR_INVALID for a
 *   NULL argument.
 *
 * npr_sam_bam_deflate: npr_sam_bam (below; one body, the same checks and refusals) with the stream framed as npr_bgzf_deflate does and
 *   every virtual offset of the index taken from its block table.  bam_out == NULL: the upper bound npr_sam_bam returns; cap is checked
 *   against that bound; returns the file's actual length.
 *
 * npr_sam_bam: the whole conversion in one call; the text, the two parse tables and the tag bytes go up once, the BAM file image and the
 *   index tables come back.  Record i is line i (span, fields, tail as the parsers filled them; tags / tag_off as npr_bam_tags did).
 *   FAILS, with nothing written: a line whose tail status is not NPR_OK or whose `fields` status is NPR_SAM_UNKNOWN_REFERENCE; a tid
 *   outside -1 .. n_refs - 1; a CIGAR that is neither "*" nor a list of <number><letter> with letters of MIDNSHP=X and numbers below 2^28
 *   (NPR_ERR_INVALID).  Nothing is dropped: a record with RNAME "*" is kept with tid -1.  (That the cigar's read bases equal l_seq is not checked.)
 *   MEASURE.  n_ops = the cigar's operations ("*": 0), consumed = the sum of its M D N = X lengths, end = pos + consumed, or pos + 1 when
 *   consumed is 0 or FLAG has 4 set; bin = reg2bin(pos, end) of the specification (pos -1 is taken as 0; tid -1: 4680).  l_seq = the
 *   length of SEQ, 0 for "*".  Nothing here looks at ref_len, and no record is refused for where it ends: a record that ends past 2^29
 *   (POS is at most 2^29, so it never begins there) fits no level and gets reg2bin's last answer, bin 0; a record that begins at or past
 *   its reference's end keeps the bin of its position.
 *   ORDER.  sorted != 0: npr_bam_sort_order on (tid, pos, FLAG); else the file's order.
 *   RECORD.  block_size, refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen (36 bytes); QNAME and a
 *   NUL; the cigar, one uint32 per operation = length << 4 | op with MIDNSHP=X = 0..8; SEQ two bases a byte, first base in the high
 *   nibble, through "=ACMGRSVTWYHKDBN" = 0..15 in either letter case, any other byte 15, an odd last nibble 0; QUAL bytes - 33, or l_seq
 *   bytes 0xFF for "*"; the tag bytes.  A cigar of more than 65535 operations: n_cigar_op = 2, the cigar <l_seq>S<consumed>N, and after
 *   the record's other tags 'C' 'G' 'B' 'I', n_ops as uint32 and the real operations.
 *   The records follow the header in order; the stream is framed as npr_bgzf_frame does.  Returns the file's length; bam_out == NULL:
 *   only that (the index is not made); NPR_ERR_CAPACITY when cap is smaller.
 *   INDEX (sorted != 0 and bam_out != NULL; else the index arguments are not touched and may be NULL), over the records in sorted order,
 *   with v(u) the virtual offset of stream byte u and [u0, u1) a record's bytes:
 *   chunks: a maximal run of consecutive records of one (tid, bin) is one chunk [v(u0 of its first), v(u1 of its last)); the runs come
 *     back ordered by (tid, bin), tid -1 last, file order among equals, as run_tid / run_bin / run_beg / run_end (room for n each);
 *     *n_runs says how many.
 *   linear: reference k has ((ref_len[k] - 1) >> 14) + 1 windows of 16384 positions (ref_len[k] >= 1), the references' windows back to
 *     back; linear[w] = the smallest v(u0) of the records of tid k with max(pos, 0) >> 14 <= w' <= (end - 1) >> 14 (w' beyond the last
 *     window counts as the last: a record past its reference's end, or past 2^29 on a reference of 2^29 bases, lies in the last window),
 *     or all ones when there is none.  (The backfill and the cut are npr_bai_write's.)  A ref_len above 2^29 is accepted, because the
 *     parser keeps POS at or below 2^29: every record begins where a BAI can address it.  Such a reference has windows from the 32 768th
 *     on; they hold the records that reach past 2^29 (which lie in bin 0), npr_bai_write writes them like the others, and no query
 *     consults them (npr_bai_chunks takes regions up to 2^29): positions past 2^29 are covered by no index.
 *   meta[k][4]: the smallest v(u0) and the largest v(u1) of the records of tid k (all ones and 0 without one), the number of those
 *     with FLAG & 4 clear, and with it set.  *n_no_coor = the records of tid -1.
 *
 * npr_bai_write: the BAI file from those arrays: "BAI\1", n_ref; per reference n_bin, per bin: bin, n_chunk, the chunks' (beg, end) --
 *   the runs of one (tid, bin) are the bin's chunks, in the order given; a reference with a record gets the pseudo-bin 37450 last, with
 *   the two chunks (meta[k][0], meta[k][1]) and (meta[k][2], meta[k][3]) --; n_intv = the reference's windows up to the last one that
 *   has a record (0 without one), and their values, a window without a record taking the value of the next one that has one; after the
 *   last reference n_no_coor as uint64.  Runs of tid -1 are not written.  out == NULL: only the length.  NPR_ERR_INVALID for runs that
 *   are not ordered by (tid, bin) or a tid outside -1 .. n_refs - 1; NPR_ERR_CAPACITY when cap is smaller. */
#define NPR_SAM_TAIL_COLS 8
#define NPR_BGZF_PAYLOAD 65280
#define NPR_BAM_TILE 4096 /* bases of one record a workgroup of the encode kernel takes */
int32_t npr_sam_parse_tail(const char *text, const int64_t *span, const int64_t *fields, int64_t n, const char *rnames,
                           const int64_t *rname_off, int64_t n_refs, int64_t *tail);
int64_t npr_bam_tags(const char *text, const int64_t *tail, int64_t n, int64_t *tag_off, uint8_t *out, int64_t cap);
int64_t npr_bam_header(const char *sam_header, int64_t len, int32_t sorted, uint8_t *out, int64_t cap, int64_t *n_refs,
                       int64_t *ref_len, int64_t cap_refs);
int32_t npr_bam_sort_order(npr_ctx *ctx, int64_t n, const int32_t *tid, const int64_t *pos, const int32_t *flag, int32_t *order);
int64_t npr_bgzf_frame(npr_ctx *ctx, const uint8_t *data, int64_t len, uint8_t *out, int64_t cap);
int64_t npr_sam_bam(npr_ctx *ctx, const uint8_t *text, int64_t text_len, const int64_t *span, const int64_t *fields, const int64_t *tail,
                    int64_t n, const int64_t *tag_off, const uint8_t *tags, const uint8_t *header, int64_t header_len, int64_t n_refs,
                    const int64_t *ref_len, int32_t sorted, uint8_t *bam_out, int64_t cap, int64_t *n_runs, int32_t *run_tid,
                    uint32_t *run_bin, uint64_t *run_beg, uint64_t *run_end, uint64_t *linear, uint64_t *meta, int64_t *n_no_coor);
int64_t npr_bgzf_deflate(npr_ctx *ctx, const uint8_t *data, int64_t len, uint8_t *out, int64_t cap,
                         int64_t *block_off /* [ceil(len / NPR_BGZF_PAYLOAD) + 1] or NULL */);
int32_t npr_deflate_last(npr_ctx *ctx, int64_t *out /* [4] */);
int64_t npr_sam_bam_deflate(npr_ctx *ctx, const uint8_t *text, int64_t text_len, const int64_t *span, const int64_t *fields,
                            const int64_t *tail, int64_t n, const int64_t *tag_off, const uint8_t *tags, const uint8_t *header,
                            int64_t header_len, int64_t n_refs, const int64_t *ref_len, int32_t sorted, uint8_t *bam_out, int64_t cap,
                            int64_t *n_runs, int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg, uint64_t *run_end,
                            uint64_t *linear, uint64_t *meta, int64_t *n_no_coor);
int64_t npr_bai_write(int64_t n_refs, const int64_t *ref_len, int64_t n_runs, const int32_t *run_tid, const uint32_t *run_bin,
                      const uint64_t *run_beg, const uint64_t *run_end, const uint64_t *linear, const uint64_t *meta, int64_t n_no_coor,
                      uint8_t *out, int64_t cap);

/* ---- reading BGZF: the blocks of a file inflated on the device (SAMv1 section 4.1, RFC 1951, RFC 1952) ----
 * The inverse of npr_bgzf_frame / npr_bgzf_deflate, for the files of any writer (htslib, zlib): csrc/npr_inflate.h is the decoder, one body
 * for host and device, csrc/npr_inflate.hip the kernel, one workgroup a block.
 *
 * npr_bgzf_scan (host, no GPU): walks the blocks of file[0, len).  A block is: 1f 8b 08, FLG with FEXTRA (bit 2) set, MTIME, XFL, OS, XLEN,
 *   the extra subfields (SI1, SI2, SLEN, data), among them -- anywhere, not only first -- 'B' 'C' of SLEN 2 whose value is BSIZE = the
 *   block's length - 1; the deflate data; CRC-32 and ISIZE (uint32 each).  The block must lie inside the file, hold its extra field and its
 *   trailer, and ISIZE must be at most 65536.  A block of ISIZE 0 is a block like any other.  The file must end with the 28-byte end-of-file
 *   block of npr_bgzf_frame and the blocks before it must fill the file exactly: otherwise it is truncated, NPR_ERR_INVALID.
 *   *n_blocks = the blocks before that last end-of-file block.  block_off / stream_off (either may be NULL; cap_blocks entries each): the
 *   file offset of every block and the stream offset of its first payload byte (the sum of the ISIZEs before it), and at index *n_blocks
 *   the end-of-file block's offset and the stream's length; NPR_ERR_CAPACITY when cap_blocks < *n_blocks + 1 (*n_blocks is set).  Returns
 *   the stream's length.  The deflate data is not looked at.
 *
 * npr_bgzf_inflate: the payloads of all blocks of the file, in order, in out[0, returned length).  out == NULL: only the stream's length
 *   (the scan alone).  NPR_ERR_CAPACITY when cap is smaller.  Every block's deflate data is decoded by one workgroup, independently of
 *   every other block, as RFC 1951 in full: any number of deflate blocks up to the one with BFINAL, stored, fixed and dynamic ones, code
 *   length symbols 16 / 17 / 18, lengths 3 .. 258, distances 1 .. 32768, matches that overlap their own output.  A block is ACCEPTED
 *   exactly when a fresh raw inflater of zlib (no history) accepts its deflate data and ends on its last byte, the output has ISIZE bytes
 *   and their CRC-32 is the trailer's.  The refusals, a status per block (csrc/npr_inflate.h INF_*): 1 BTYPE 3; 2 a stored block's LEN is
 *   not ~NLEN; 3 over-subscribed code lengths; 4 incomplete code lengths (zlib's rule: a literal/length or distance code whose longest
 *   code has one bit may be incomplete, and there may be no distance code at all; the code-length code must be complete); 5 a repeat code
 *   with no length before it or running past HLIT + HDIST; 6 no code for symbol 256; 7 HLIT above 286, HDIST above 30, literal/length
 *   symbols 286 / 287, distance symbols 30 / 31, bits that are no code; 8 a distance that reaches before the block's first byte; 9 output
 *   past ISIZE; 10 input past the deflate data's end; 11 bytes of deflate data left after the final block; 12 a produced length that is
 *   not ISIZE; 13 a CRC-32 that is not the trailer's; 14 the decoder's step bound (unreachable).  When any block is refused the call
 *   returns NPR_ERR_INVALID and NO byte of out is touched.  A refused block costs bounded time: every read is checked against the block,
 *   every write against ISIZE, and every loop of the decoder is bounded.
 *
 * npr_inflate_last: of the last file this context inflated (a call that reached the device), out[0 .. 3] = the blocks, the first refused
 *   block (-1: none), its status (above; 0: none), the stream's length.  Before the first: 0, -1, 0, 0.  NPR_ERR_INVALID for a NULL argument. */
int64_t npr_bgzf_scan(const uint8_t *file, int64_t len, int64_t *block_off, int64_t *stream_off, int64_t cap_blocks, int64_t *n_blocks);
int64_t npr_bgzf_inflate(npr_ctx *ctx, const uint8_t *file, int64_t len, uint8_t *out, int64_t cap);
int32_t npr_inflate_last(npr_ctx *ctx, int64_t *out /* [4] */);

/* ---- reading BAM: a BAM file as SAM text (SAMv1 section 4.2), the records walked and written on the device (csrc/npr_bamread.hip) ----
 * npr_bam_aux_text (host, threaded, no GPU): the inverse of npr_bam_tags.  The auxiliary bytes of n records, record i =
 *   aux[aux_off[i] .. aux_off[i + 1]), as text, record i at out[text_off[i] .. text_off[i + 1]), text_off[n + 1]: its fields as
 *   TAG:TYPE:VALUE separated by one tab (no tab before the first or after the last).  A one byte; c C s S i I all print as type i, in
 *   decimal; f as C's %g; Z and H the bytes up to their NUL; B the subtype letter, then "," and a value per element (integers in decimal, f
 *   as %g).  placeholder (may be NULL): where placeholder[i] is not 0, the first CG:B:I field of record i is left out of the text and
 *   cg[2 i], cg[2 i + 1] receive the offset of its elements from the record's first auxiliary byte and their number (cg[2 n], both -1
 *   for a record without one); an element whose low four bits exceed 8 is malformed.  out == NULL: only the offsets and cg.  Returns the
 *   total length; NPR_ERR_CAPACITY when cap is smaller; NPR_ERR_INVALID, with nothing written to out, for an unknown type, a field cut by the
 *   record's end, a Z or H without NUL, or an array that runs past the record.
 *
 * npr_bam_sam: file[0, len), a BAM file image, as SAM text in sam_out: the header text (l_text bytes as they stand), then one line per
 *   record in the file's order.  The blocks are inflated as npr_bgzf_inflate does (the same refusals; npr_inflate_last tells).  One
 *   wavefront checks the header (magic "BAM\1", l_text, n_ref, every l_name with its NUL and l_ref inside the stream); one wavefront
 *   follows the block_size chain, in rounds into a table of fixed size, and checks per record: block_size at least 33, the record inside
 *   the stream (the last one ends with it), l_read_name at least 1 with a NUL at its end, the 32 fixed bytes, name, cigar, SEQ and QUAL
 *   inside block_size, refID and next_refID in -1 .. n_ref - 1, pos and next_pos at most 2^31 - 2 (walk status 6: POS and PNEXT, one more,
 *   end at 2^31 - 1 in SAM); a cigar operation above 8 is refused too.  THE LINE, columns separated by
 *   one tab: QNAME; FLAG; RNAME, "*" for refID -1; POS + 1; MAPQ; CIGAR: "*" for no operation, else <length><MIDNSHP=X> per operation --
 *   when the stored cigar is <l_seq>S<n>N and the record has a CG:B:I field, that field's operations, and the field is dropped --; RNEXT:
 *   "*" for next_refID -1, "=" when it equals refID, else the name; PNEXT + 1; TLEN; SEQ through "=ACMGRSVTWYHKDBN", "*" for l_seq 0; QUAL
 *   + 33, "*" when l_seq is 0 or the first byte is 0xFF; the auxiliary fields as npr_bam_aux_text writes them, each after a tab; "\n".
 *   Returns the text's length and sets *n_records (may be NULL); sam_out == NULL: only that.  NPR_ERR_CAPACITY when cap is smaller (cap may
 *   be a generous bound: only the returned length is written).  NPR_ERR_INVALID for every refusal above.  Nothing is written to sam_out
 *   unless the call succeeds. */
int64_t npr_bam_aux_text(const uint8_t *aux, const int64_t *aux_off /* [n + 1] */, int64_t n, const uint8_t *placeholder /* [n] or NULL */,
                         int64_t *text_off /* [n + 1] */, int64_t *cg /* [2 n] */, uint8_t *out, int64_t cap);
int64_t npr_bam_sam(npr_ctx *ctx, const uint8_t *file, int64_t len, uint8_t *sam_out, int64_t cap, int64_t *n_records);

/* ---- a BAM file into a pileup without SAM text: the records added where they lie on the device (csrc/npr_bampile.hip, csrc/npr_bamrec.h) ----
 * What the reference runs on a sorted BAM file -- `samtools depth x.bam` (nanopore/metaAnalyses/coverageDepth.py:49-65), `samtools mpileup`
 * (analyses/consensus.py:56-64) -- without turning the file into SAM text, parsing it on the host and uploading cigars and bases again.
 *
 * npr_bam_open: file[0, len), a BAM file image, as an object on the device: the blocks are inflated as npr_bgzf_inflate does (the same
 *   refusals; npr_inflate_last tells), the header is checked and the block_size chain followed by the kernels of npr_bam_sam (the same
 *   refusals, NPR_ERR_INVALID; a cigar operation above 8 is a matter of npr_pileup_add_bam).  The stream and the table of record offsets stay
 *   on the device; the header's names and lengths are kept on the host.  No object is returned unless the call succeeds.  The object belongs
 *   to its context and must be closed before it; calls on it count as calls on the context.
 * npr_bam_stream_info: out[0 .. 3] = the records, n_ref, l_text, the stream's length; returns the number of records.
 * npr_bam_stream_refs: ref_len[k] = l_ref of sequence k, its name = names[name_off[k] .. name_off[k + 1]) (back to back, without NULs).
 *   Returns the names' total length; names == NULL: only that, nothing is written; NPR_ERR_CAPACITY when cap is smaller.  ref_len and name_off
 *   may be NULL.
 *
 * npr_pileup_add_bam: the records of `bs` into the table of `pl`.  First the header: n_ref must be the pileup's n_refs, every l_ref its
 *   ref_len[k], and both objects of one context -- else NPR_ERR_INVALID, nothing is added and counts is all zero.
 *   SELECTED is a record with refID >= 0, (flag & flag_mask) == 0, l_seq > 0 and a cigar of at least one operation.  THE CIGAR, by the rule
 *   of npr_bam_sam: the stored operations -- unless they are exactly <l_seq>S<n>N: then the record's auxiliary fields are walked on the device
 *   (types A c C s S i I f Z H B, every step checked against the record's end) and the elements of the first CG:B:I field, when there is one,
 *   are the operations (of no element: the record is not selected).
 *   COLUMNS.  M, = and X runs are columns: word 0-3 of the row by the read's nibble 1, 2, 4, 8 (A, C, G, T), word 4 for every other code
 *   ("=" and N among them).  D runs are deletion columns (word 5, through the difference array).  Words 6 and 7 by the rules of
 *   npr_pileup_add: an I run is attached to the last column (M = X or D) the record consumed before it, however many N, S, H, P runs or runs
 *   of length 0 lie between; I runs not separated by a column count once; an I run before the first column counts not at all; word 7 is
 *   set at the record's first column.  N advances the reference and counts nothing, S advances the read and counts nothing, H and P do
 *   nothing, a run of length 0 does nothing.
 *   REFUSED is a selected record with pos < 0, with pos + the reference bases its cigar consumes (M D N = X) above l_ref, with read bases
 *   consumed (M I S = X) other than l_seq, with an operation code above 8, or -- under a placeholder cigar -- with malformed auxiliary fields
 *   (a field cut by the record's end, an unknown type or array subtype, a Z or H without NUL, an array past the record's end).  Sums are
 *   taken in 64 bits.  A refused record adds NOTHING -- every cigar is checked before the first add --, the other records are counted, and
 *   the call returns NPR_ERR_INVALID.
 *   counts[0 .. 3] = the records, the selected ones, the added ones, the refused ones (selected = added + refused); written whenever the
 *   kernels ran.  Counts are integers: the table does not depend on the order.  Nothing but the counts crosses to the host. */
typedef struct npr_bam_stream npr_bam_stream;
int32_t npr_bam_open(npr_ctx *ctx, const uint8_t *file, int64_t len, npr_bam_stream **out);
void npr_bam_close(npr_bam_stream *bs);
int64_t npr_bam_stream_info(npr_bam_stream *bs, int64_t *out /* [4] */);
int64_t npr_bam_stream_refs(npr_bam_stream *bs, int64_t *ref_len /* [n_ref] */, int64_t *name_off /* [n_ref + 1] */, uint8_t *names, int64_t cap);
int32_t npr_pileup_add_bam(npr_pileup *pl, npr_bam_stream *bs, int32_t flag_mask, int64_t *counts /* [4] */);

/* ---- region queries on an indexed BAM file: the BAI read, only the blocks it names inflated (SAMv1 section 5; csrc/npr_bamregion.hip) ----
 * What the reference's users get from pysam.index: `samtools view x.bam chr:a-b`, `samtools depth -r`, `mpileup -r`.  A region is
 * [beg, end) of reference sequence tid, 0-based and half-open.  A record's interval is [rb, re): rb = max(pos, 0), re = max(pos + the
 * reference bases of its cigar (M D N = X), rb + 1); with FLAG 4 set or without a cigar re = rb + 1 (the MEASURE rule of npr_sam_bam); under
 * the placeholder cigar <l_seq>S<n>N the operations are those of the first CG:B:I field, when there is one.  A record OVERLAPS the region
 * when its refID is tid and rb < end && re > beg.
 *
 * npr_bai_chunks (host, no GPU): the chunks a reader has to visit for the region, from bai[0, bai_len), the BAI file image of any writer
 *   ("BAI\1", n_ref; per reference n_bin, per bin: bin, n_chunk, the chunks' (beg, end); n_intv, ioffset[n_intv]; optionally n_no_coor).
 *   The bins are those of the specification's reg2bins(beg, end): bin 0 and, for the shifts 26, 23, 20, 17, 14 with first bins 1, 9, 73,
 *   585, 4681, first + (beg >> shift) .. first + ((end - 1) >> shift); the pseudo-bin 37450 is never one of them.  The lower bound is
 *   low = ioffset[min(beg >> 14, n_intv - 1)], 0 when n_intv is 0 (htslib's rule: safe for every writer).  A chunk with end <= low is
 *   dropped; the rest are sorted by beg and a chunk whose beg is less than or equal to the running end is merged into its predecessor:
 *   the result is disjoint, ascending chunks, chunk_beg[i] / chunk_end[i] (virtual offsets).  Returns their number; chunk_beg == NULL:
 *   only that; NPR_ERR_CAPACITY when cap is smaller.  *n_ref is set once the header has been read.  NPR_ERR_INVALID, with nothing written
 *   to the chunks, for a wrong magic, a count (n_ref, n_bin, n_chunk, n_intv) that is negative or runs past bai_len -- every read is checked
 *   against bai_len first, so a malformed image costs bounded time --, a chunk with end < beg (in any bin but the pseudo-bin, of any
 *   reference), a tid outside 0 .. n_ref - 1, a region that does not satisfy 0 <= beg < end <= 2^29, or bytes after the last reference
 *   that are not the 8 of n_no_coor (which is optional).
 *
 * npr_bam_open_region: npr_bam_open for the records that overlap the region, found through the index.  The block headers are scanned
 *   (npr_bgzf_scan); the blocks that hold the BAM header are inflated (block 0, and more while the header runs on) and the header is
 *   checked as npr_bam_open checks it; the index's n_ref must be the file's.  A chunk [vb, ve) of npr_bai_chunks needs the blocks whose
 *   file offset lies in [vb >> 16, ve >> 16], the last one only when ve & 0xffff > 0; vb >> 16 and ve >> 16 must be block offsets of the
 *   scan (ve >> 16 may be the end-of-file block's) and the low 16 bits may not exceed that block's ISIZE.  The union of the header's and
 *   the chunks' blocks, in file order, is inflated into ONE COMPACT STREAM (the same decoder, statuses and refusals; npr_inflate_last
 *   reports the blocks and the length of this stream: how a caller sees that the file was not inflated whole).  Every chunk is walked by
 *   one wavefront with the per-record checks of npr_bam_sam, from its first byte until the record offset reaches its end; a chunk that
 *   does not end on a record boundary is refused with walk status 7.  The records of all chunks, in file order, are then filtered: a
 *   record is kept when it overlaps the region.  A kept candidate (refID tid, FLAG 4 clear) under a placeholder cigar whose auxiliary
 *   fields are malformed (npr_pileup_add_bam states when) is not kept and makes the call fail.  NPR_ERR_INVALID for every refusal above
 *   and of npr_bai_chunks; no object is returned unless the call succeeds.  The object is an ordinary npr_bam_stream: its records are the
 *   overlapping ones in file order, its header fields the file's, npr_bam_stream_info out[3] the compact stream's length; whole records
 *   are kept, so npr_pileup_add_bam on it gives a table that is complete inside [beg, end) and partial outside.
 * npr_bam_stream_restrict: narrows the object's record table in place to the records that overlap the region, order preserved, by the same
 *   filter; needs no index and works on a file in any order; restricting twice gives the intersection.  Returns the number of records
 *   left.  NPR_ERR_INVALID (the table stays as it was) for a tid outside 0 .. n_ref - 1, a region that does not satisfy 0 <= beg < end,
 *   or malformed auxiliary fields as above.
 * npr_bam_stream_sam: the header text and one line per record of the object, exactly the lines npr_bam_sam writes (one body); arguments,
 *   return value and refusals as npr_bam_sam.  After npr_bam_open_region or npr_bam_stream_restrict: `samtools view -h x.bam region`. */
int64_t npr_bai_chunks(const uint8_t *bai, int64_t bai_len, int32_t tid, int64_t beg, int64_t end, uint64_t *chunk_beg, uint64_t *chunk_end,
                       int64_t cap, int64_t *n_ref);
int32_t npr_bam_open_region(npr_ctx *ctx, const uint8_t *file, int64_t len, const uint8_t *bai, int64_t bai_len, int32_t tid, int64_t beg,
                            int64_t end, npr_bam_stream **out);
int64_t npr_bam_stream_restrict(npr_bam_stream *bs, int32_t tid, int64_t beg, int64_t end);
int64_t npr_bam_stream_sam(npr_bam_stream *bs, uint8_t *sam_out, int64_t cap, int64_t *n_records);

/* ---- BAM streams to BAM files: sorted, merged and region files without SAM text, the index of any sorted file (csrc/npr_bammerge.hip) ----
 * What the reference's users get from `samtools sort`, `samtools merge` / `cat`, `samtools view -b x.bam chr:a-b` and `samtools index`
 * (the reference joins its mappers' files with combineSamFiles): the records are measured, ordered and moved where they lie on the device;
 * only the file image and the index arrays cross to the host.  Every record's bytes pass as they stand, whatever wrote them.
 *
 * npr_bam_streams_bam: the records of streams[0 .. n_streams) -- as their record tables stand now, that is after any npr_bam_open_region or
 *   npr_bam_stream_restrict -- as ONE BAM file image.  n_streams >= 1; all streams belong to ctx and have the same n_ref, the same l_ref values
 *   and the same names in the same order (reference ids are not remapped), else NPR_ERR_INVALID.  A stream may appear twice, and may have no
 *   record; the total must be below 2^31; the streams are not changed.  header[0, header_len) is the complete BAM header of the output as
 *   npr_bam_header writes it (magic, l_text, the text, n_ref, the names and lengths), ending exactly at header_len, with the streams' n_ref
 *   and l_ref values, else NPR_ERR_INVALID.
 *   MEASURE, per record from its bytes (csrc/npr_bamrec.h bamrec_measure, one body with the region queries' interval): the MEASURE rule of
 *   npr_sam_bam restated on BAM fields.  The operations are the stored ones, or under the placeholder cigar <l_seq>S<n>N those of the first
 *   CG:B:I field when there is one; consumed = the sum of their M D N = X lengths (64 bits); end = pos + consumed, or pos + 1 when consumed
 *   is 0 or FLAG has 4 set; bin = reg2bin(max(pos, 0), max(end, max(pos, 0) + 1)), 4680 for refID -1: the bin of the interval [rb, re) of
 *   "region queries".  A record with an operation code above 8 among those operations makes the call fail with NPR_ERR_INVALID, and so does
 *   a record with refID >= 0 and FLAG 4 clear whose auxiliary fields under a placeholder cigar are malformed (npr_pileup_add_bam states
 *   when); nothing is written then.  (With refID -1 or FLAG 4 such fields are not needed: the stored operations count.)
 *   ORDER.  The records are concatenated in argument order, each stream's in its table's order.  sorted != 0: the stable order of
 *   npr_bam_sort_order on (refID, pos, FLAG) -- ties keep the concatenation's order; a pos below -1 sorts as -1 --; else the concatenation
 *   as it stands (`samtools cat`).
 *   BYTES.  Every record is copied as it stands, block_size through its last auxiliary byte, with exactly one change: the two bytes of
 *   `bin` are the measured bin.  The stream is header, then the records; compress == 0 frames it as npr_bgzf_frame does, else as
 *   npr_bgzf_deflate does (npr_deflate_last tells).
 *   INDEX (sorted != 0 and bam_out != NULL; else the index arguments are not touched and may be NULL): exactly the INDEX paragraph of
 *   npr_sam_bam -- the same arrays with room for the total record count, the same order of runs, the same linear (the windows of the
 *   streams' l_ref values, each at least 1) and meta.
 *   Returns the file's length and sets *n_records (may be NULL) to the total; bam_out == NULL: the length with stored blocks, an upper
 *   bound of the compressed one, and nothing else is made.  NPR_ERR_CAPACITY when cap is smaller than that bound, as npr_sam_bam_deflate.
 *   Nothing is written to bam_out unless the call succeeds.
 * npr_bam_merge_last: of the last image npr_bam_streams_bam wrote on this context, out[0 .. 3] = the records, the stream's length, the
 *   bytes the gather kernel moved (the stream without its header; it reads and writes each once) and that kernel's time in nanoseconds
 *   between two events.  Before the first: zeros.
 *
 * npr_bam_index: the index of file[0, len), a BAM file image of any writer, as it stands.  The file is opened as npr_bam_open opens it (the
 *   same refusals).  The records must be in coordinate order already: (refID, pos) never decreases from a record to the next, refID -1
 *   counting as last; FLAG is not looked at (writers break ties differently).  A file out of order is NPR_ERR_INVALID and no array is
 *   touched.  MEASURE and its refusals as above.  The arrays are those of the INDEX paragraph of npr_sam_bam, with v(u) taken from THIS
 *   file's blocks (npr_bgzf_scan's tables): the block that holds stream byte u is the last one whose first byte lies at or before u -- a
 *   block of ISIZE 0 holds no byte and is passed over --, v(u) = block_off << 16 | (u - stream_off); u == the stream's length is one past
 *   the payload of a short last block (block_off << 16 | ISIZE), and the end-of-file block's offset << 16 after a last block of 65 280
 *   bytes.  *n_refs = the header's n_ref and ref_len[k] its l_ref values (each at least 1, else NPR_ERR_INVALID), what npr_bai_write needs;
 *   meta has room for cap_refs x 4, linear for cap_linear windows, the run arrays for cap_runs each (there are at most as many runs as
 *   records).  A count above its cap is NPR_ERR_CAPACITY: *n_refs and *n_runs are set and no array is written.  Returns the number of
 *   records. */
int64_t npr_bam_streams_bam(npr_ctx *ctx, npr_bam_stream *const *streams, int64_t n_streams, const uint8_t *header, int64_t header_len,
                            int32_t sorted, int32_t compress, uint8_t *bam_out, int64_t cap, int64_t *n_records, int64_t *n_runs,
                            int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg, uint64_t *run_end, uint64_t *linear, uint64_t *meta,
                            int64_t *n_no_coor);
int32_t npr_bam_merge_last(npr_ctx *ctx, int64_t *out /* [4] */);
int64_t npr_bam_index(npr_ctx *ctx, const uint8_t *file, int64_t len, int64_t *n_refs, int64_t *ref_len, int64_t cap_refs, int64_t *n_runs,
                      int32_t *run_tid, uint32_t *run_bin, uint64_t *run_beg, uint64_t *run_end, int64_t cap_runs, uint64_t *linear,
                      int64_t cap_linear, uint64_t *meta, int64_t *n_no_coor);

/* npr_batch_create_at for reads that are NOT contiguous in memory: read i = read[read_begin[i] .. read_end[i]) -- e.g. the
 * aligned part of each record's SEQ inside the mapped SAM text (columns 11, 12 of npr_sam_parse), so the sequences go from
 * the file's bytes to the pinned staging buffer in one copy.  Everything else as npr_batch_create_at. */
int32_t npr_batch_create_spans(npr_ctx *ctx, const npr_params *params, int64_t n_reads, int64_t n_refs,
                               const uint8_t *ref, const int64_t *ref_off, const int32_t *ref_index,
                               const uint8_t *read, const int64_t *read_begin, const int64_t *read_end,
                               const int32_t *guide_ops, const int64_t *guide_off, const int64_t *guide_start,
                               const int32_t *model_slot, npr_batch **out);

#ifdef __cplusplus
}
#endif
#endif
