// npr_device.h -- structures shared between the host API and the HIP kernels of libnprealign.
#pragma once
#include <cstdint>

#include "npr_internal.h"
#include "npr_band.h"

namespace npr {

// One banded DP problem on the device (a Segment of a read).
struct Task {
    int64_t x_off;     // first reference base code of the segment in d_seq
    int64_t y_off;     // first read base code of the segment in d_seq
    int64_t band_off;  // first anti-diagonal entry in d_lo / d_n / d_coff
    int64_t pair_off;  // first slot of this task in the posterior pair buffers
    int32_t lX, lY;    // segment spans
    int32_t D;         // lX + lY
    int32_t pair_cap;  // slots available at pair_off
    int32_t flags;     // bit0 ragged start, bit1 ragged end
    int32_t model;     // model slot
    int32_t xs, ys;    // offset of the segment inside the read's slice (added to emitted coordinates)
    int32_t read;      // owning read
    int32_t cells_pad; // padded cell count (scratch use)
    int64_t ctl_off;   // register-kernel tasks: first anti-diagonal entry in d_ctl (pairs of words), else -1
    int64_t tile_off;  // stripe-kernel tasks: index of the task's header in d_stripes (Stripe units), else -1
    int64_t rowmask_off;  // stripe-kernel tasks: first row of the task in d_rowmask (one word per row of a stripe), else -1
};

// k_dp_tile cuts a task's lattice columns into stripes of at most 64*R columns; one wavefront sweeps a stripe
// anti-diagonal by anti-diagonal, one row of the forward scratch per anti-diagonal.  A task's table is a header
// {X = number of stripes, K = rows of the whole task} followed by its stripes in column order.
struct Stripe {
    int32_t X;      // first lattice column of the stripe
    int32_t K;      // lattice columns (a multiple of the slots per lane; the last stripe may reach past lX)
    int32_t df, dl; // first / last anti-diagonal on which the band has cells in the stripe (dl < df: none)
    uint32_t row0;  // row index of anti-diagonal df in the task's scratch; anti-diagonal d is row row0 + d - df
    int32_t pad[3];
};

struct TaskOut {
    float tot_m;      // total probability = tot_m * 2^tot_e (forward)
    int32_t tot_e;
    float btot_m;     // same from the backward pass
    int32_t btot_e;
    int32_t npairs;   // pairs >= threshold found (may exceed pair_cap -> status NPR_ERR_CAPACITY)
    int32_t status;
};

struct KernelArgs {
    const Task *tasks;
    TaskOut *outs;
    int32_t *queue;  // work-queue head
    int32_t ntasks;
    const DevModel *models;
    const uint8_t *seq;
    const int32_t *lo;
    const int32_t *n;
    const uint32_t *coff;  // per anti-diagonal: offset of its first cell inside the task (cells padded to x4)
    const Stripe *stripes;  // k_dp_tile: stripe tables (Task::tile_off)
    const uint32_t *rowmask;  // k_dp_tile: lane masks of every row, packed (npr_sched.h tile_row_word; Task::rowmask_off)
    unsigned long long *prof;  // unused (kept so the fields after it keep their kernarg offsets)
    const int64_t *region;  // k_dp_tile: first scratch cell of each workgroup (regions sized by the workgroup's first task)
    const uint32_t *ctl;   // register kernel: two control words per anti-diagonal (row offset; jlo | n << 13 | (rebase + 1) << 26)
    char *F;               // forward match-state scratch: one region of 8*slot_stride bytes per resident wave.  The
                           // register kernel keeps (mantissa, exponent) interleaved per cell; the generic kernel
                           // keeps a mantissa plane followed by an exponent plane.
    int64_t slot_stride;
    int32_t slot_base;     // first scratch region of this launch (concurrent launches own disjoint regions)
    int32_t *px;  // sparse posterior output
    int32_t *py;
    float *pp;
    float threshold;
    int32_t wcap;  // ring capacity (cells per anti-diagonal) of the generic kernel
    float *Bv;     // dense dump of the backward match state (debug launches only)
    int32_t *Be;
    float *ring;   // generic kernel, global-ring variant: 18*wcap floats per resident wave (bands too wide for LDS)
    // Baum-Welch E-step launches only (k_dp_generic<.., EM = true>)
    float *Fx;       // forward sx, sy, lx, ly planes: 4 * slot_stride floats per resident wave
    double *em_T;    // [NPR_MAX_MODELS][25] expected transition counts, accumulated with atomics
    double *em_E;    // [NPR_MAX_MODELS][EM_BINS] expected emission counts (compact bins, see EM_BINS)
};

// compact emission bins of the E-step: 16 match [x*4+y], 4 shortGapX [x], 4 longGapX [x], 4 shortGapY [y], 4 longGapY [y]
constexpr int EM_BINS = 32;

struct CompactArgs {
    const Task *tasks;
    const TaskOut *outs;
    const int64_t *dst_off;
    int32_t ntasks;
    const int32_t *px;
    const int32_t *py;
    const float *pp;
    int32_t *cx;
    int32_t *cy;
    float *cp;
};

// launchers (npr_kernels.hip)
int launch_generic(const KernelArgs &a, int grid, int threads, size_t lds_bytes, bool dense, bool global_ring, void *stream);
int launch_em(const KernelArgs &a, int grid, size_t lds_bytes, bool global_ring, void *stream);
size_t em_extra_lds_bytes();
int launch_compact(const CompactArgs &a, void *stream);
int launch_stair(const KernelArgs &a, int R, int grid, void *stream);
int launch_wide(const KernelArgs &a, int R, int NW, int grid, void *stream);
int launch_em_stair(const KernelArgs &a, int R, int grid, void *stream);
size_t em_stair_lds_bytes();
// device MEA stage (npr_mea.hip); offsets are per read, prefix sums with n_reads + 1 entries
// k_mea_sort_lds takes a read whose spans (lX + 1 and lY) both stay within this: its two tables, lX + 1 + lY ints, then fit the LDS of a CU
constexpr int kMeaSortLdsSpan = 16 * 1024;
struct MeaArgs {
    const Task *tasks;
    const TaskOut *outs;
    int32_t ntasks, n_reads;
    const int32_t *px, *py;  // posterior pairs as the DP kernels left them (per task at Task::pair_off)
    const float *pp;
    const int64_t *rx_off;   // reference positions: lX + 1 entries per read in cnt / start
    const int64_t *ry_off;   // read positions: lY entries per read in colsum
    const int64_t *rp_off;   // pairs: the read's slice of sx / sy / sq / back
    int32_t *cnt, *start, *colsum;
    int32_t *sx, *sy, *sq, *back;
    int32_t *sw;             // weight of every sorted pair (the sort writes it, k_mea_weigh reads it)
    // the kept pairs (weight above matchGamma) of every read, at the read's slice too: by id = in (x, y) order (kx, ky, kq and
    // the chain's back pointers kback), and in the order the chain visits them (vrec: read position, weight, id, 0)
    int32_t *kx, *ky, *kq, *kback;
    int4 *vrec;
    int32_t *kept;           // per read: kept pairs; -1: the ring kernel took the read (back pointers over the sorted pairs)
    // the pieces a read's chain problem is cut into (k_mea_cuts): np[r] planned pieces, boundaries pb[pboff[r] + 0 .. np[r]] among
    // the kept pairs, the last pair of each piece's heaviest chain pbest[poff[r] + j]; lane s of k_mea_chain_lanes takes piece
    // lane_piece[s] of read lane_read[s]
    const int32_t *np, *poff, *pboff, *lane_read, *lane_piece;
    int32_t *pb, *pbest;
    int32_t n_pieces;
    int32_t *best_who;       // last pair of the heaviest chain, -1 if none
    int32_t *read_flag;      // 0 or an NPR_ERR_* raised by this stage
    double gap_gamma, match_gamma;
    int32_t ring;            // entries of the prefix-maximum ring (power of two)
    const int32_t *order;    // reads by decreasing pair count: the per-read kernels take them in this order (no long read last)
    const int32_t *read_first, *read_ntasks, *task_of;  // the tasks of a read: task_of[read_first[r] + s]
    int32_t sort_lds_bytes;  // > 0: k_mea_sort_lds with this much LDS for the reads whose tables fit it
    int32_t sort_threads;    // threads of its workgroups (0: 1024)
    int32_t any_global_sort; // some read's tables do not: the global-memory kernels for those
    const int64_t *cnt_off;  // per read: its slice of cnt / start (lX + 1 entries), -1 for a read sorted in LDS
    int32_t ring_only;       // tests: every read through the LDS-ring kernel
    int32_t *ops_tmp;        // (op, length) pairs, each read's written backwards from the end of its slice
    const int64_t *ot_off;
    int32_t *n_ops, *chain_len;
    int64_t *chain_mass;
    uint32_t *ops_dense;     // one word per op: length << 2 | op
    const int64_t *od_off;
    int32_t *max_run;        // per read: its longest run (k_mea_trace) ...
    uint16_t *ops_dense16;   // ... when none of the batch exceeds 14 bits: the words' low halves, the form that crosses PCIe (else null)
};
int launch_tile(const KernelArgs &a, int R, int NW, int grid, void *stream, bool flat = false);
size_t tile_lds_bytes(int nw);
int64_t tile_scratch_cells(int64_t rows, int R);  // forward scratch (8-byte cells) of a task with that many stripe rows
// ---- device planner (npr_plan.hip): band rows, frame schedules, stripe tables and generic row offsets of a batch,
// expanded on the device from the segments' plan points (npr_band.h) ----
struct PlanSeg {
    int64_t point_first;  // first of the segment's pieces + 1 points
    int64_t band_off;     // first entry of its rows in lo / n (/ coff)
    int32_t pieces, lX, lY, pad;
};
struct SegSummary {
    int64_t cells;          // in-band lattice cells
    int64_t generic_cells;  // scratch cells of the generic kernel (rows padded to 4)
    int32_t max_width;
    int32_t bad;            // anti-diagonals without cells
    int32_t rough;          // anti-diagonals on which a band edge does not move by exactly one cell
    int32_t pad;
};
// the register classes with a frame schedule: (slots per lane, wavefronts) of kernel classes 0..6
constexpr int kSchedClasses = 7;
constexpr int kSchedR[kSchedClasses] = {1, 2, 4, 2, 2, 4, 4};
constexpr int kSchedNW[kSchedClasses] = {1, 1, 1, 4, 8, 8, 12};
struct PlanArgs {
    int32_t n_segs, fixed_mode, width;
    const PlanPoint *points;
    const PlanSeg *segs;
    int32_t *lo, *n;
    SegSummary *summary;
};
struct SchedArgs {
    int32_t n_segs;
    const PlanSeg *segs;
    const SegSummary *summary;
    const int32_t *lo, *n;
    const int64_t *ctl_off;    // per segment: first entry of its control words (pairs), -1: no candidate class
    const uint32_t *cand;      // per segment: bit c set = class c may take it
    uint32_t *ctl;
    int32_t *cls;              // out: the first candidate class whose frame can follow the band, -1: none
    int64_t *cells;            // out: forward scratch cells of that schedule
};
struct StripeArgs {
    int32_t count, R;
    const int32_t *seg_index;  // the segments that go to k_dp_tile
    const PlanSeg *segs;
    const SegSummary *summary;
    const int32_t *lo, *n;
    const int64_t *tile_off;   // per listed segment: its header in `stripes`
    Stripe *stripes;
    int64_t *rows;             // out, per listed segment
};
struct CoffArgs {
    int32_t n_segs;
    const PlanSeg *segs;
    const int32_t *n;
    uint32_t *coff;
};
int launch_plan_bands(const PlanArgs &a, void *stream);
// k_dp_stair addresses a row of a task's forward scratch as (descriptor of the task's region - row_bias) + a 32-bit byte
// offset of where lane 0 of the row would land; the bias keeps that offset non-negative for rows whose first lane is not
// lane 0 (8 * R * 63 bytes at most).  A task therefore needs 8 * cells + bias < 2^32: see stair_fits().
template <int R>
NPR_HD constexpr uint32_t row_bias() { return R == 4 ? 2048u : 1024u; }
NPR_HD constexpr bool stair_fits(int64_t rows, int slots) { return rows * slots < (int64_t(1) << 29) - 512; }
struct RowMaskArgs {
    int32_t count;              // stripe-kernel tasks
    const int32_t *seg_index;   // their segments
    const PlanSeg *segs;
    const int32_t *lo, *n;
    const int64_t *tile_off;    // per task: header of its stripe table
    const Stripe *stripes;
    const int64_t *mask_off;    // per task: first row in `out`
    uint32_t *out;
};
int launch_plan_rowmask(const RowMaskArgs &a, void *stream);
// the frame schedules in chunks (npr_plan.hip): chunk_off = prefix sum of plan_sched_chunks_of(D) over the segments (device, n_segs + 1
// entries), `chunks` = plan_sched_chunk_bytes(n_chunks) of scratch, cur = n_segs + kSchedClasses ints of scratch, cand_union = OR of the segments' candidate masks
size_t plan_sched_chunk_bytes(int64_t n_chunks);
int64_t plan_sched_chunks_of(int64_t D);
int launch_plan_sched(const SchedArgs &a, const int64_t *chunk_off, int64_t n_chunks, void *chunks, int32_t *cur, uint32_t cand_union, void *stream);
int launch_plan_stripes(const StripeArgs &a, void *stream);
int launch_plan_coff(const CoffArgs &a, void *stream);
int launch_encode(uint8_t *seq, int64_t n, void *stream);

// k_align_stats (npr_stats.hip): per-read reductions over aligned pairs
struct StatsSeg {  // a piece of a read's window whose base codes lie in `seq`: reference [xs, xe) at x_off, read [ys, ye) at y_off
    int32_t xs, xe, ys, ye;
    int64_t x_off, y_off;
};
struct StatsArgs {
    int32_t n_reads;
    const int64_t *ops_off;  // [n_reads + 1]
    const uint32_t *ops;     // one word per cigar op: length << 2 | op
    const int32_t *seg_off;  // [n_reads + 1]
    const StatsSeg *segs;
    const uint8_t *seq;      // base codes 0..4
    int32_t *out;            // [n_reads][NPR_STATS_WORDS]
};
int launch_align_stats(const StatsArgs &a, void *stream);
// k-mer tables (npr_kmer.hip).  A k-mer's bin is its base-4 number, first base most significant; bin 4^k takes the k-mers with a code 4.
constexpr int NPR_KMER_MAX_K = 6;
constexpr int NPR_KMER_PAD = 64;  // bytes readable past the last base of KmerArgs::seq (a lane loads its run and the halo in 16-byte pieces)
NPR_HD constexpr int kmer_bins(int k) { return (1 << (2 * k)) + 1; }
struct KmerArgs {  // k_kmer_spectrum
    const uint8_t *seq;      // ASCII, the sequences back to back, 16-byte aligned
    int64_t n;               // bases
    const int64_t *seq_off;  // [n_seqs + 1], seq_off[0] = 0, seq_off[n_seqs] = n
    int64_t n_seqs;
    int32_t k;
    unsigned long long *counts;  // [kmer_bins(k)], added to
};
int launch_kmer_spectrum(const KmerArgs &a, void *stream);
constexpr int NPR_KMER_TILE = 8192;  // bases per workgroup and step of the two k_kmer_spectrum kernels
constexpr int NPR_KMER_MAX_GROUPS = 64;
struct KmerGroupArgs {  // k_kmer_spectrum_groups: the sequences ordered by group, group g's bases back to back from seq[tile0[g] * NPR_KMER_TILE] on
    const uint8_t *seq;        // ASCII, NPR_KMER_PAD readable bytes past the last tile
    const int64_t *tile0;      // [n_groups + 1] first tile of every group (a group without bases has none)
    const int64_t *seq_first;  // [n_groups + 1] group g's offsets are seq_off[seq_first[g] .. seq_first[g + 1]): one per sequence and the group's end
    const int64_t *seq_off;    // positions in seq; a group's first = tile0[g] * NPR_KMER_TILE
    int32_t n_groups;
    int32_t k;
    unsigned long long *counts;  // [n_groups][kmer_bins(k)], added to
};
int launch_kmer_spectrum_groups(const KmerGroupArgs &a, int64_t tiles, void *stream);
struct IndelKmerArgs {  // k_indel_kmers: `s` as for k_align_stats, but every record has ONE piece, its whole window (none: the record is skipped); s.out unused
    StatsArgs s;
    int32_t k;
    unsigned long long *read_counts, *ref_counts;  // [kmer_bins(k)] each, added to
    int32_t *bad;            // set to 1 when a record's cigar runs past its piece (the record adds nothing)
};
int launch_indel_kmers(const IndelKmerArgs &a, void *stream);
// read-quality tables (npr_readqual.hip; the definitions: include/nprealign.h, npr_read_quality)
constexpr int RQ_POS_BINS = 336, RQ_QUAL_COLS = 95, RQ_BASE_COLS = 5, RQ_GC_COLS = 102, RQ_TOTALS = 8, RQ_MAX_GROUPS = 8;
constexpr int RQ_TILE = 2048;     // positions of one read per work item
constexpr int RQ_ALIGN = 16;      // a staged read starts on a multiple of it and RQ_ALIGN bytes past the last read are readable: a lane loads 8 bytes at a time
constexpr int RQ_ROW = 6;         // per-read scratch row: quality sum, G + C, A + C + G + T, bad quality bytes, 255 - smallest quality byte, largest quality byte
constexpr int RQ_TILE_CLASSES = (1 << 24) / RQ_TILE + 1;  // tiles from position 2^24 on all count into bin 335: one class
constexpr unsigned long long RQ_LEN_TOP = 1ull << 62;     // the shortest length is kept as the largest RQ_LEN_TOP - length
constexpr size_t RQ_GROUP_WORDS = static_cast<size_t>(RQ_POS_BINS) * (RQ_QUAL_COLS + RQ_BASE_COLS + 1) + RQ_QUAL_COLS + RQ_GC_COLS + RQ_TOTALS;
struct ReadQualArgs {
    const uint8_t *seq, *qual;    // the counted reads' bytes: read r's at [start[r], start[r] + len[r])
    const int64_t *start, *len;   // [n]
    const int32_t *group;         // [n], 0 .. n_groups - 1
    const unsigned long long *items;  // [n_items] (read << 32 | tile), ordered by (group, min(tile, RQ_TILE_CLASSES - 1))
    int64_t n, n_items;
    int32_t n_groups;
    unsigned long long *rows;     // [n][RQ_ROW], zeroed
    // zeroed, added to; totals as the device keeps them: reads, bases, largest RQ_LEN_TOP - length, largest length, largest 255 - quality byte,
    // largest quality byte, empty reads, reads with a bad quality byte
    unsigned long long *pos_qual, *pos_base, *len_hist, *meanq_hist, *gc_hist, *totals;
};
int launch_read_quality(const ReadQualArgs &a, void *stream);
// the integer exclusive prefix sum the analysis units share (the contract and the kernels: npr_scan.h; compiled in npr_scan.hip): out[i] = in[0] + ...
// + in[i - 1] for i in 0 .. n, in[n] is never read, in == out is allowed for types of one width.  _group: one workgroup, one launch; _tiled: three
// launches over tiles, `tile` is scratch of scan_tiles(n) entries
int64_t scan_tiles(int64_t n);
template <typename In, typename Out>
int launch_scan_group(const In *in, Out *out, int64_t n, void *stream);
template <typename In, typename Out>
int launch_scan_tiled(const In *in, Out *out, int64_t n, Out *tile, void *stream);
// the device pileup (npr_pileup.hip): NPR_PILEUP_WORDS int32 per reference position, a difference array for the deletion columns
struct PileupRec {
    int64_t row0;    // table row of the record's first reference position
    int64_t d0;      // slot of that position in the difference array (row0 + index of the reference sequence)
    int64_t y_off;   // the record's first read base in PileupArgs::seq
    int32_t xlen;    // reference positions from there to the end of what the record may cover; < 0: the record is not selected
    int32_t ylen;    // read bases there
};
struct PileupArgs {  // k_pileup_add
    int64_t n;
    const int64_t *ops_off;  // [n + 1]
    const uint32_t *ops;     // one word per cigar op: length << 2 | op
    const PileupRec *recs;
    const uint8_t *seq;      // read bases: ASCII (ascii != 0) or base codes 0..4
    int32_t ascii;
    int32_t *tab;            // [rows][NPR_PILEUP_WORDS], added to
    int32_t *diff;           // [rows + n_refs], added to
    int32_t *bad;            // set to 1 when a record's cigar runs past what it has (the record adds nothing)
};
struct PileupScanArgs {  // the running sum of diff into word 5 of tab
    int64_t n_slots, n_refs;  // n_slots = rows + n_refs
    const int64_t *dbase;    // [n_refs + 1]: first slot of every sequence (first row + index)
    const int32_t *diff;
    int32_t *tile;           // [scan_tiles(n_slots)] scratch
    int32_t *tab;
};
int launch_pileup_add(const PileupArgs &a, void *stream);
int launch_pileup_scan(const PileupScanArgs &a, void *stream);
int launch_pileup_depth(const int32_t *tab, int64_t rows, int32_t *depth, uint8_t *covered, void *stream);
// alignment-quality tables (npr_alnqual.hip; the definitions: include/nprealign.h, npr_pileup_coverage and npr_align_quality)
constexpr int AQ_WIN_WORDS = 8, AQ_TOTALS = 8, AQ_HOMOPOLYMER = 3, AQ_MAX_WINDOWS = 65536, AQ_MAPQ_COLS = 256, AQ_CLASSES = 5;
constexpr int AQ_TILE = 2048;  // consecutive rows of the pileup's table one workgroup of k_pileup_coverage takes
struct CoverageArgs {  // k_coverage_max, then k_pileup_coverage
    const int32_t *tab;      // [rows][NPR_PILEUP_WORDS], word 5 summed
    const uint8_t *ref;      // [rows] ASCII, the sequences back to back
    int64_t rows;            // T
    int32_t n_windows;       // W
    unsigned long long *max_depth;  // one word, zeroed: k_coverage_max
    // zeroed, added to: win [W][AQ_WIN_WORDS], depth_hist / start_hist [RQ_POS_BINS], totals [AQ_TOTALS] (word 2 is left to the host)
    unsigned long long *win, *depth_hist, *start_hist, *totals;
};
int launch_coverage_max(const CoverageArgs &a, void *stream);
int launch_pileup_coverage(const CoverageArgs &a, void *stream);
struct AlnQualRec {
    int64_t row0;      // table row of the record's first reference position
    int64_t s0, s1;    // rows of the record's reference sequence: [s0, s1)
    int64_t y_off;     // read[read_begin] of the record in AlnQualArgs::seq
    int64_t clip0, clip1;
    int32_t xlen;      // reference positions from row0 to the end of the sequence; < 0: the record is not selected
    int32_t span;      // read_end - read_begin
    int32_t sy;        // read position the cigar starts at (<= span)
    int32_t mapq;
};
constexpr size_t AQ_TABLE_WORDS = AQ_MAPQ_COLS + static_cast<size_t>(RQ_POS_BINS) * RQ_BASE_COLS + RQ_POS_BINS + RQ_GC_COLS + 2 * AQ_CLASSES + 2 * RQ_POS_BINS + AQ_TOTALS;
struct AlnQualArgs {  // k_align_quality
    int64_t n;
    const int64_t *ops_off;  // [n + 1]
    const uint32_t *ops;     // one word per cigar op: length << 2 | op
    const AlnQualRec *recs;
    const uint8_t *seq;      // read bases, ASCII
    const uint8_t *ref;      // [rows] ASCII, the sequences back to back
    int64_t rows;            // T
    int32_t n_windows;       // W
    unsigned long long *tab; // [AQ_TABLE_WORDS] zeroed, added to: mapq_hist, pos_base, clip_hist, gc_hist, indel, indel_len, totals in this order
    unsigned long long *win_mapq;  // [W][2] zeroed, added to
    int32_t *bad;            // set to 1 when a record's cigar runs past what it has (the record adds nothing)
};
int launch_align_quality(const AlnQualArgs &a, void *stream);
// exact-match seeding (npr_seed.hip).  A set of sequences lies in a CODE BUFFER: one separator byte, then every sequence followed by one
// separator, then NPR_SEED_PAD more separators; sequence s of ASCII offsets off[] starts at off[s] + s + 1.  Bases A C G T are 0..3; every
// other byte of the two buffers that meet has a value of its own side (reference: other base 4, separator 6; read: 5 and 7), so that
// "bytes equal" is "bases match" and a match ends at a separator at the latest.
constexpr int NPR_SEED_MIN_K = 8, NPR_SEED_MAX_K = 32, NPR_SEED_MAX_KB = 12;
constexpr int NPR_SEED_PAD = 48;  // a lane loads 32 bytes from its position, an extension step 8 bytes past a separator; rounded so that the buffer ends on 16 bytes
constexpr uint8_t NPR_SEED_REF_OTHER = 4, NPR_SEED_READ_OTHER = 5, NPR_SEED_REF_SEP = 6, NPR_SEED_READ_SEP = 7;
NPR_HD constexpr int64_t seed_code_bytes(int64_t bases, int64_t n_seqs) { return (bases + n_seqs + 1 + NPR_SEED_PAD + 15) / 16 * 16; }
constexpr int NPR_SEED_SCAN_TILE = 4096;  // table entries a workgroup of the seed unit's own scan takes; the table is allocated in whole tiles (no bounds check: npr_seed.hip)
NPR_HD constexpr int64_t seed_table_entries(int kb) { return ((int64_t(1) << (2 * kb)) + 1 + NPR_SEED_SCAN_TILE - 1) / NPR_SEED_SCAN_TILE * NPR_SEED_SCAN_TILE; }
struct SeedEncodeArgs {  // k_seed_encode: ASCII sequences lying back to back -> a code buffer, and (rc != nullptr) the buffer of their reverse complements
    const uint8_t *ascii;
    const int64_t *off;      // [n_seqs + 1], off[0] = 0
    int64_t n_seqs;
    int64_t bytes;           // seed_code_bytes(off[n_seqs], n_seqs)
    uint8_t other, sep;
    uint8_t *codes, *rc;
};
int launch_seed_encode(const SeedEncodeArgs &a, void *stream);
struct SeedIndexArgs {  // k_seed_bucket_count / the scan / k_seed_bucket_fill: the window starts of the reference by their first kb bases
    const uint8_t *codes;
    int64_t bytes;
    int32_t k, kb;
    int32_t *table;          // [seed_table_entries(kb)], zeroed; afterwards table[key] = END of bucket `key` in pos (it begins where bucket key - 1 ends)
    int32_t *tile;           // [table entries / NPR_SEED_SCAN_TILE] scratch of the scan
    int32_t *pos;            // [window starts]: positions in codes
};
int launch_seed_index(const SeedIndexArgs &a, void *stream);
struct SeedMatchArgs {  // k_seed_match<false> counts every read's matches into count[], k_seed_match<true> writes them
    const uint8_t *ref;      // the index's code buffer, table and positions
    const int32_t *table, *pos;
    const int64_t *ref_off;  // [n_refs + 1] ASCII offsets of the reference sequences
    int64_t n_refs;
    int32_t k, kb;
    int32_t min_len;
    const uint8_t *read;     // code buffer of the reads in one orientation
    int64_t bytes;
    const int64_t *read_off; // [n_reads + 1]
    int64_t n_reads;
    uint32_t strand;         // 0 forward, 1 reverse complement
    uint32_t *count;         // [n_reads], zeroed: matches per read (emitting: the next free row of the read's range)
    const int64_t *hit_off;  // [n_reads + 1] (emitting)
    int32_t *hits;           // [hit_off[n_reads]][4] = reference index, a, b | strand << 31, L (emitting)
};
int launch_seed_match(const SeedMatchArgs &a, bool emit, void *stream);
// chaining of seed rows on the device (npr_seedchain.hip).  A CHAIN SPAN is one (read, reference) that has rows: its forward-strand run
// and its reverse-strand run of rows (either may be empty), each contiguous in the rows and in (a, b) order.
struct SeedChainSpan {
    int64_t first[2];        // first row of the run on strand 0 / 1
    int32_t n[2];            // rows of the run (0: the strand has none)
    int32_t read, ref;
};
struct SeedChainArgs {
    const int32_t *hits;     // [rows][4] = reference index, a, b | strand << 31, L: validated on the host
    const SeedChainSpan *span;
    int64_t n_chains;
    uint32_t max_gap;        // (clamped: a gap sum is below 2^32)
    const int32_t *ref_len, *read_len;
    int32_t *node;           // [rows][4] scratch: a row's last reference position, last read position, best chain score ending in it, and the
                             // largest last reference position of its run's rows up to it
    int32_t *back;           // [rows] scratch: the predecessor as an index into the run, -1 none
    int32_t *run_end;        // [2 * n_chains][2] scratch: the row (index into the run) the best chain of a run ends in, and its score
    int32_t *chains;         // [n_chains][4] = reference index, strand, score, rows in the chain
    int64_t *n_ops;          // [n_chains + 1]: op pairs per chain, then (launch_scan_group) their exclusive prefix
    int32_t *ops;            // [n_ops[n_chains]][2]
};
int launch_seed_chain_dp(const SeedChainArgs &a, void *stream);     // k_chain_dp, k_chain_trace<false>, the scan of n_ops
int launch_seed_chain_write(const SeedChainArgs &a, void *stream);  // k_chain_trace<true>
// from the rows k_seed_match emitted to the chain spans k_chain_dp takes, on the device (npr_seedmap.hip)
// (the tier boundary of k_map_sort is NPR_SEED_MAP_LDS_ROWS of include/nprealign.h: a read of at most so many rows is sorted in LDS, one of more in global memory)
struct SeedMapArgs {
    int64_t n_reads;
    const uint32_t *count;   // [n_reads] what k_seed_match<false> counted
    int64_t *hit_off;        // [n_reads + 1]: the exclusive prefix of count
    int32_t *hits;           // [hit_off[n_reads]][4]: k_map_sort sorts every read's rows by (strand, reference index, a, b) in place
    int64_t *chain_off;      // [n_reads + 1]: k_map_spans<false> writes every read's number of chains, the scan turns them into offsets in place
    SeedChainSpan *span;     // [chain_off[n_reads]]: k_map_spans<true>
};
int launch_seedmap_offsets(const SeedMapArgs &a, void *stream);  // launch_scan_group: hit_off of count
int launch_seedmap_chains(const SeedMapArgs &a, void *stream);   // k_map_sort, k_map_spans<false>, the scan of chain_off
int launch_seedmap_spans(const SeedMapArgs &a, void *stream);    // k_map_spans<true>
// SAM CIGAR text of packed cigars on the device (npr_cigtext.hip): list i = words[word_off[i] .. word_off[i] + n_ops[i])
struct CigTextArgs {
    int64_t n;
    const int64_t *word_off;  // [n], or [n + 1] when n_ops is null
    const int64_t *n_ops;     // [n]; null: list i ends where list i + 1 begins
    const uint32_t *words;    // one word per cigar op: length << 2 | op
    int64_t *str_off;         // [n + 1]: the lengths pass writes every string's length, the scan turns them into offsets in place
    int64_t *tile;            // [scan_tiles(n)] scratch of the scan
    int32_t *bad;             // set to 1 when a list holds an operation outside M I D
    char *out;                // the write pass: string i at out[str_off[i] .. str_off[i + 1])
};
int launch_cigtext_offsets(const CigTextArgs &a, void *stream);  // lengths + exclusive scan: str_off, *bad
int launch_cigtext_write(const CigTextArgs &a, void *stream);
// SAM -> sorted BAM + BAI on the device (npr_bam.hip; the definitions: include/nprealign.h, "coordinate-sorted BAM")
constexpr int BAM_SORT_BITS = 8, BAM_SORT_DIGITS = 1 << BAM_SORT_BITS;
constexpr int BAM_SORT_ROUNDS = 8;                    // a workgroup of 256 threads takes this many rounds of 256 consecutive keys
constexpr int BAM_SORT_TILE = 256 * BAM_SORT_ROUNDS;
inline int64_t bam_sort_blocks(int64_t n) { return (n + BAM_SORT_TILE - 1) / BAM_SORT_TILE; }
struct BamSortArgs {  // one pass: k_sort_hist, the scan of hist, k_sort_scatter
    int64_t n;
    int32_t shift;               // the pass's digit = (key >> shift) & 255
    const unsigned long long *keys_in;
    const uint32_t *vals_in;     // null: the values are the indices (the first pass)
    unsigned long long *keys_out;
    uint32_t *vals_out;
    uint32_t *hist;              // [256][blocks] digit-major, then its exclusive scan in place (int32)
    int32_t *tile;               // [scan_tiles(256 * blocks)] scratch of the scan
};
int launch_bam_sort_pass(const BamSortArgs &a, void *stream);
int launch_bam_sort_keys(int64_t n, const int32_t *tid, const int64_t *pos, const int32_t *flag, int32_t no_tid, unsigned long long *keys, void *stream);
constexpr int BGZF_PAYLOAD = 65280, BGZF_SLICE = 255, BGZF_OVERHEAD = 31, BGZF_EOF = 28;
struct BgzfArgs {  // k_bgzf_frame: one workgroup of 256 threads per block, slices of BGZF_SLICE bytes
    const uint8_t *data;
    int64_t len;
    uint8_t *out;
    uint32_t x2n[32];            // x^(2^k) modulo the polynomial, reflected
    uint32_t level[8];           // x^(8 * BGZF_SLICE * 2^k): the multiplier of level k of the combining tree when the right half is full
};
int launch_bgzf_frame(const BgzfArgs &a, void *stream);
// BGZF blocks of compressed deflate data (npr_deflate.hip; the block layout and the choice rule: include/nprealign.h, npr_bgzf_deflate)
constexpr int DEFLATE_SLOT = BGZF_PAYLOAD + BGZF_OVERHEAD;   // stride of the slots the blocks are compressed into
constexpr int DEFLATE_MAX_GROUPS = 512;                      // workgroups of k_bgzf_deflate: each takes every DEFLATE_MAX_GROUPS-th block
inline int64_t deflate_groups(int64_t blocks) { return blocks < DEFLATE_MAX_GROUPS ? blocks : DEFLATE_MAX_GROUPS; }
struct DeflateArgs {
    BgzfArgs z;                  // data, len, the CRC constants; out = the slots: [blocks * DEFLATE_SLOT + 8]
    uint16_t *dist;              // [deflate_groups(blocks)][BGZF_PAYLOAD] scratch: distance - 1 of the match found at a position
    int64_t *block_len;          // [blocks + 1]: every block's length, then their exclusive scan in place: block_off
    int64_t *tile;               // [scan_tiles(blocks)] scratch of the scan
    uint32_t *chosen;            // [4] zeroed, added to: blocks emitted as (a) matches and literals, (b) literals, (c) stored; [3] stays 0 unless the
                                 // emitted bits disagree with the measured ones (a defect: the block is then stored and the call fails)
    uint8_t *packed;             // the file image: block b at block_off[b], the end-of-file block at block_off[blocks]
};
int launch_bgzf_deflate(const DeflateArgs &a, void *stream);  // k_bgzf_deflate, the scan, k_bgzf_pack
// BGZF blocks inflated (npr_inflate.hip; the decoder and its statuses: npr_inflate.h)
constexpr int INFLATE_MAX_GROUPS = 1024;                     // workgroups of k_bgzf_inflate: each takes every INFLATE_MAX_GROUPS-th block
struct InflateArgs {
    BgzfArgs z;                  // the CRC constants (data, len, out are not used)
    const uint8_t *file;         // the file image
    const int64_t *block_off;    // [blocks + 1] file offset of every block, then of the end-of-file block (npr_bgzf_scan)
    const int64_t *stream_off;   // [blocks + 1] stream offset of every block's payload, then the stream's length
    int64_t blocks;
    uint8_t *stream;             // [stream_off[blocks]] the payloads; a block that is refused leaves its bytes as they were
    int32_t *status;             // [blocks] INF_OK or why a block was refused
};
int launch_bgzf_inflate(const InflateArgs &a, void *stream);
// BAM records as SAM lines (npr_bamread.hip; the line format: its head and include/nprealign.h, npr_bam_sam)
struct BamReadRec {  // what k_bam_measure finds
    int64_t aux_off;             // first auxiliary byte in the stream
    int32_t aux_len, l_seq;
    int32_t fixed_len;           // text bytes of the eleven mandatory columns with their ten tabs, the CIGAR as the record stores it
    int32_t cig_len;             // ... of which the CIGAR
    int32_t placeholder;         // the stored cigar is <l_seq>S<n>N: a CG:B:I tag, when there is one, holds the real operations
    int32_t pad;
};
struct BamReadArgs {
    const uint8_t *stream;       // the uncompressed BAM stream
    int64_t len;
    int32_t n_ref;
    const uint8_t *names;        // the reference names back to back, name k = names[name_off[k] .. name_off[k + 1])
    const int64_t *name_off;
    int64_t n;                   // records
    const int64_t *rec_off;      // [n] stream offset of every record's block_size
    BamReadRec *meas;            // [n]
    int32_t *bad;                // set to 1 by a cigar operation above 8
    const int64_t *aux_pack_off; // [n + 1] where a record's auxiliary bytes go in aux_pack (k_bam_gather_aux)
    uint8_t *aux_pack;
    const int64_t *cg;           // [2 n] the real operations of a folded cigar: byte offset within the record's auxiliary bytes and count; -1: none
    const uint8_t *aux_text;     // the auxiliary fields as text (npr_bam_aux_text), record i = [aux_text_off[i], aux_text_off[i + 1])
    const int64_t *aux_text_off;
    const int64_t *line_off;     // [n + 1] first byte of every line in out
    const unsigned long long *items;  // [n_items] record << 32 | tile of SEQ / QUAL
    int64_t n_items;
    uint8_t *out;                // the lines
};
int launch_bam_head(const uint8_t *stream, int64_t len, int64_t *out4, void *hip_stream);  // out: status (0 ok), the header's end, l_text, n_ref
// up to cap record offsets from `start` on into table; out: how many, where the next record begins (len: the stream is done), status (0 ok)
int launch_bam_walk(const uint8_t *stream, int64_t len, int64_t start, int32_t n_ref, int64_t *table, int64_t cap, int64_t *out3, void *hip_stream);
int launch_bam_read_measure(const BamReadArgs &a, void *stream);
int launch_bam_gather_aux(const BamReadArgs &a, void *stream);
int launch_bam_emit(const BamReadArgs &a, void *stream);
// the records of a BAM stream into a pileup where they lie (npr_bampile.hip; the rules: npr_bamrec.h and include/nprealign.h, npr_pileup_add_bam)
struct BamPileRec {  // what k_bampile_check finds
    int64_t ops_at;              // first cigar word in the stream (the stored ones or a CG:B:I field's; any alignment)
    int64_t n_ops;
    int64_t seq_at;              // first byte of the packed bases in the stream
    int64_t row0;                // table row of POS
    int64_t d0;                  // slot of POS in the difference array (row0 + refID)
    int32_t verdict;             // BR_SKIP, BR_ADD, BR_REFUSED
    int32_t pad;
};
struct BamPileArgs {
    const uint8_t *stream;       // the uncompressed BAM stream
    int64_t len;
    int64_t n;                   // records
    const int64_t *rec_off;      // [n] stream offset of every record's block_size
    int64_t n_ref;
    const int64_t *ref_len;      // [n_ref]
    const int64_t *dbase;        // [n_ref + 1] first slot of every sequence in the difference array (first row + index)
    int32_t flag_mask;
    BamPileRec *recs;            // [n]
    unsigned long long *counts;  // [4], added to: (unused), selected, added, refused
    int32_t *tab;                // [rows][NPR_PILEUP_WORDS], added to
    int32_t *diff;               // [rows + n_ref], added to
};
int launch_bampile_check(const BamPileArgs &a, void *stream);
int launch_bampile_add(const BamPileArgs &a, void *stream);
// the records of the chunks of an index, and the records that overlap a region (npr_bamregion.hip; the rules: include/nprealign.h, "region queries")
struct BamChunkArgs {
    const uint8_t *stream;       // the compact stream: the payloads of the inflated blocks back to back
    int64_t len;
    int32_t n_ref;
    int64_t n_chunks;
    const int64_t *chunk_beg;    // [n_chunks] first byte of every chunk in the stream
    const int64_t *chunk_end;    // [n_chunks] one past its last record
    int64_t *count;              // [n_chunks + 1] the count pass: records of every chunk; the write pass: their exclusive scan
    int64_t *stop;               // [n_chunks] the count pass: where the walk of the chunk ended
    int32_t *status;             // [n_chunks] the count pass: WALK_OK or why it ended there (npr_bamrec.h)
    int64_t *table;              // the write pass: [count[n_chunks]] the record offsets, chunk after chunk
};
int launch_bam_chunk_count(const BamChunkArgs &a, void *stream);
int launch_bam_chunk_write(const BamChunkArgs &a, void *stream);
struct BamOverlapArgs {
    const uint8_t *stream;
    int64_t n;                   // records
    const int64_t *rec_off;      // [n]
    int32_t tid;
    int64_t beg, end;            // the region
    int64_t *keep;               // [n + 1] the flag pass: 1 for a record that overlaps; the gather pass: their exclusive scan
    int32_t *bad;                // set to 1 by malformed auxiliary fields under a placeholder cigar
    int64_t *kept;               // the gather pass: [keep[n]] the offsets of the kept records, order preserved
};
int launch_bam_overlap_flags(const BamOverlapArgs &a, void *stream);
int launch_bam_overlap_gather(const BamOverlapArgs &a, void *stream);
struct BamRec {  // one SAM line as the host's parsers found it
    int64_t name, cigar_lo, cigar_hi, seq, qual;  // offsets in the text; qual < 0: "*"
    int64_t tag_off;
    int32_t l_name, l_seq, tag_len;
    int32_t tid, pos, flag, mapq, next_tid, next_pos, tlen;
};
struct BamMeasure {  // what k_bam_measure finds
    int64_t size;       // bytes of the record in the stream, block_size included
    uint32_t n_ops, consumed;
    int32_t end;
    uint32_t bin;
};
constexpr int BAM_TILE = 4096;
struct BamArgs {
    int64_t n, n_items, header_len;
    const uint8_t *text;
    const BamRec *recs;
    const uint8_t *tags;
    BamMeasure *meas;
    int32_t *bad;                // set to 1 by a malformed cigar
    const uint32_t *order;       // [n] record at place j
    int64_t *size_sorted;        // [n + 1]: the sizes in output order, then their exclusive scan in place
    int64_t *tile;               // scratch of that scan
    int64_t *rec_off;            // [n]: first stream byte of record i
    const unsigned long long *items;  // [n_items] record << 32 | tile of SEQ / QUAL
    uint8_t *raw;                // the uncompressed stream
    // the index, over the places j
    int64_t n_refs;
    const int64_t *lin_off;      // [n_refs + 1] first window of every reference
    uint32_t *head;              // [n + 1]: 1 where a run of one (tid, bin) begins, then its exclusive scan in place (int32)
    int32_t *head_tile;
    unsigned long long *run_key; // [runs] tid' << 16 | bin in file order
    unsigned long long *run_beg, *run_end;  // [runs] in file order
    unsigned long long *linear, *meta, *no_coor;
    const int64_t *block_off;    // file offset of every BGZF block of a compressed file, [blocks + 1]; null: stored blocks, the closed form
    const int64_t *stream_off;   // null: blocks of BGZF_PAYLOAD bytes.  Else the blocks of any writer: stream offset of every block's payload, [n_blocks + 1],
    int64_t n_blocks;            // beside block_off [n_blocks + 1] (npr_bgzf_scan's tables); a virtual offset is then searched for (npr_bamrec.h)
};
int launch_bam_measure(const BamArgs &a, void *stream);
int launch_bam_offsets(const BamArgs &a, void *stream);   // sizes in output order, their scan, rec_off
int launch_bam_encode(const BamArgs &a, void *stream);    // the cigars, then the (record, tile) items
int launch_bam_index_heads(const BamArgs &a, void *stream);  // head flags + scan, linear, meta
int launch_bam_index_runs(const BamArgs &a, void *stream);   // the runs in file order
struct BamGatherArgs {
    int64_t n_runs;
    const uint32_t *perm;
    const unsigned long long *key, *beg, *end;
    int32_t no_tid;
    int32_t *run_tid;
    uint32_t *run_bin;
    unsigned long long *out_beg, *out_end;
};
int launch_bam_gather_runs(const BamGatherArgs &a, void *stream);
// BAM records to a BAM stream where they lie on the device (npr_bammerge.hip; the rules: include/nprealign.h, "BAM streams to BAM files")
constexpr int MERGE_PIECE = 4096;  // bytes of the output stream one wavefront of k_merge_gather writes: 64 lanes x 16 bytes x 4 rounds
struct MergeArgs {
    int64_t n;                   // records, the streams' tables back to back
    const uint8_t *const *src;   // [n] where record i's block_size lies (k_merge_sources: its stream + its table entry)
    BamRec *recs;                // [n] k_merge_measure: tid, pos, flag (what the index kernels of npr_bam.hip read; the rest stays 0)
    BamMeasure *meas;            // [n] k_merge_measure: size, end, bin
    int32_t *tid, *flag;         // [n] the sort key's parts
    int64_t *pos;
    int32_t *bad;                // set to BR_WHY_OP / BR_WHY_AUX by a refused record, to -1 by a pair of records out of coordinate order (k_merge_ordered)
    const uint32_t *order;       // [n] record at place j; null: the identity
    int64_t *size_sorted;        // [n + 1] k_merge_place: the sizes in output order; then their exclusive scan in place
    const uint8_t **place_src;   // [n] k_merge_place: src of the record at place j
    uint32_t *place_bin;         // [n] ... and its measured bin
    int64_t header_len, stream_len;  // the output stream: header_len bytes of header, then the records
    uint8_t *raw;                // [stream_len], 16-byte aligned
};
int launch_merge_sources(const uint8_t *stream, const int64_t *rec_off, int64_t n, const uint8_t **src, void *hip_stream);
int launch_merge_measure(const MergeArgs &a, void *stream);
int launch_merge_ordered(const MergeArgs &a, void *stream);
int launch_merge_place(const MergeArgs &a, void *stream);
int launch_merge_gather(const MergeArgs &a, void *stream);
constexpr float EXPECT_FIXED_ONE = 1099511627776.0f;  // 2^40
struct ExpectArgs {
    const Task *tasks;
    const TaskOut *outs;
    int32_t ntasks;
    const int32_t *px, *py;
    const float *pp;
    const uint8_t *seq;
    const uint8_t *use;     // per read: 0 = skip (NULL: all reads)
    const int64_t *target;  // per read: table row of reference position 0 of its window
    unsigned long long *expect;  // [positions][4], fixed point: units of 1 / EXPECT_FIXED_ONE
    uint8_t *seen;          // [positions]
};
int launch_base_expectations(const ExpectArgs &a, void *stream);
// SNP calls from a table of four base weights per reference position (npr_snpcall.hip; include/nprealign.h: npr_*_snp_calls).  The table is
// read where it lies, in the form it has: `source` says which.
enum { SNP_SRC_FIXED = 0, SNP_SRC_PILEUP = 1, SNP_SRC_DOUBLE = 2 };
constexpr int SNP_BINS = 101;                 // NPR_SNP_BINS
constexpr int SNP_OUT_WORDS = 2 * SNP_BINS + 2;  // one model's output: true_pos[101], false_pos[101], not_called, rows_called (an npr_snp_calls)
struct SnpCallArgs {
    int64_t rows;
    int32_t source;
    int32_t n_models;           // 1 .. 4
    const void *table;          // SNP_SRC_FIXED: unsigned long long [rows][4] in units of 1 / EXPECT_FIXED_ONE; SNP_SRC_PILEUP: int32 [rows][NPR_PILEUP_WORDS];
                                // SNP_SRC_DOUBLE: double [rows][4]
    const uint8_t *seen;        // [rows]; SNP_SRC_PILEUP: unused (seen = words 0-4 summed != 0)
    const uint8_t *ref_code;    // [rows] base codes 0..4
    const uint8_t *true_code;   // [rows], or NULL: the truth is the reference
    double log_evolution[16];   // [reference][candidate]
    double log_error[4][16];    // [model][candidate][observed]
    unsigned long long *out;    // [n_models][SNP_OUT_WORDS], added to
    // The variant kernels alone (include/nprealign.h: npr_*_snp_variants): error model 0, no true_code, no `out`.
    double threshold;           // a candidate c != ref of a callable row is a call when p[c] >= threshold
    uint8_t *best, *qual;       // [rows]: the most probable base (4: the row is not callable) and its quality 0..93
    uint8_t *mask;              // [rows] scratch: bit j = the j-th candidate other than the reference base, in ascending code, is a call
    uint32_t *tile_calls;       // [tiles]: the set mask bits of SNP_VARIANT_TILE consecutive rows
    int64_t *tile_off;          // [tiles + 1]: their exclusive scan; the last entry is the number of calls
    int64_t n_calls;            // emit: what tile_off[tiles] said, the length of the three arrays below
    int64_t *call_row;          // [n_calls] ascending (row, candidate code)
    uint8_t *call_alt;
    double *call_p;
};
int launch_snp_calls(const SnpCallArgs &a, void *stream);
constexpr int SNP_VARIANT_TILE = 256;  // rows of one workgroup of the variant kernels, one per thread
constexpr int64_t snp_variant_tiles(int64_t rows) { return (rows + SNP_VARIANT_TILE - 1) / SNP_VARIANT_TILE; }
int launch_snp_variants_count(const SnpCallArgs &a, void *stream);  // best, qual, mask, tile_calls, then the scan: tile_off
int launch_snp_variants_emit(const SnpCallArgs &a, void *stream);   // the calls of a.n_calls = tile_off[tiles] <= the arrays' length
// NPR_MODE_RESCORE_ORIGINAL on the device (npr_stats.hip; cactus_realign --rescoreOriginalAlignment, nanopore/analyses/alignmentUncertainty.py:41):
// the mean posterior over the M columns of the guide.  k_rescore_table spreads the guide's M runs into a table of one entry per reference
// position of the read's window (the read position the guide aligns it to, -1: none); k_rescore_sum looks every posterior pair up in it where the
// DP kernels left the pairs and adds the hits in FIXED POINT: p * 2^shift is an integer for an fp32 p at or above the posterior threshold, so a
// read's sum is the exact sum of its terms whatever order the atomics land in -- and equal to npr_host.cpp's `rescore`, whose double sum over
// the sorted pair list is exact too as long as columns * 2^shift stays below 2^53.
struct RescoreArgs {
    int32_t n_reads, ntasks;
    const int64_t *run_off;  // [n_reads + 1]: the M runs of each read's guide in `runs`
    const int32_t *runs;     // (x0, y0, length) per run, window coordinates
    const int64_t *gx_off;   // [n_reads + 1]: the read's slice of `gy` (reference span of its window + 1 entries)
    int32_t *gy;
    const Task *tasks;
    const TaskOut *outs;
    const int32_t *px, *py;
    const float *pp;
    unsigned long long *sum;  // [n_reads]
    int32_t shift;
};
int launch_rescore_table(const RescoreArgs &a, void *stream);
int launch_rescore_sum(const RescoreArgs &a, void *stream);
size_t mea_chain_lds_bytes(int ring);
int launch_mea_sort(const MeaArgs &a, void *stream);
int launch_mea_chain(const MeaArgs &a, void *stream);
int launch_mea_gather(const MeaArgs &a, void *stream);
int launch_em_wide(const KernelArgs &a, int R, int NW, int grid, void *stream);
int launch_em_tile(const KernelArgs &a, int R, int grid, void *stream);  // k_em_tile: the E-step on column stripes
size_t em_tile_lds_bytes(int nw);
// k_dp_rs<R> (npr_kernel_rs.hip): the one-wavefront frame kernel in row-scaled arithmetic (npr_rs.h) -- one exponent per
// anti-diagonal row instead of one per cell.  A task's scratch region (8 bytes per cell of its frame schedule, as for
// k_dp_stair) holds the forward rows at 4 bytes per cell in its first half and the row exponents, one word per NPR_RS_K
// anti-diagonals, from byte 4 * rs_half_cells(cells) on.
constexpr int NPR_RS_K = 16;
constexpr int NPR_RS_TOP = 85;  // the renormalised maximum of a row pair lies in [2^84, 2^85)
// The certificate that one exponent per row was enough.  s = eF + eB - eTot of an anti-diagonal turns a
// forward-backward product into a posterior; the rows' maxima stay below 2^(NPR_RS_TOP + 6), so no F * 2^s or B * 2^s of that
// row exceeds 2^(NPR_RS_TOP + 6 + s), and a cell whose other factor fell below fp32's normal range (2^-126 in row units: flushed,
// or a denormal that lost bits) carries a true posterior mass below 2^(NPR_RS_TOP + 6 + s - 126 + 1).  While every s stays below
// NPR_RS_S_LIMIT that is 2^-60 per cell, and all the path mass the sweeps can have lost -- every lost path passes through a
// flushed cell on the anti-diagonal where it was flushed -- is below cells x 2^-60: nothing a posterior, a total or a cigar can
// see.  A task with a row at or above the limit (its alignment runs ~90 binary orders further below the product of the row's
// largest forward and backward values than usual: the stretch between a long deletion and a long insertion, say) reports
// TASK_RERUN instead of NPR_OK and npr_batch_run runs it again with the per-cell-exponent kernel (k_dp_stair), which has no
// such limit.  So does a task whose forward sweep arrives at the end corner with nothing: whether that band really carries
// no probability (NPR_ERR_ZERO_PROB) is for the kernel without a range limit to say.
constexpr int NPR_RS_S_LIMIT = 126 - 60 - (NPR_RS_TOP + 6) - 1;
constexpr int32_t TASK_RERUN = 1;  // TaskOut::status of such a task between the two launches (never leaves npr_batch_run)
NPR_HD constexpr int64_t rs_half_cells(int64_t cells_pad) { return (cells_pad + 63) & ~int64_t(63); }
int launch_rs(const KernelArgs &a, int R, int grid, void *stream, bool sw, bool flat);  // sw: a loaded model has short-gap switches; flat: all gap emissions are 2^-2 (npr_rs.h)
// k_dp_mid_rs (npr_kernel_mid.hip): k_dp_rs's sweeps on two wavefronts that meet in the middle -- the forward one from row 0, the backward one from
// row D, each going on past the cut against the other's stored rows.  Tasks of fewer than MID_MIN_D anti-diagonals stay with k_dp_rs.
constexpr int32_t MID_MIN_D = 4 * NPR_RS_K;
constexpr int MID_WAVES2 = 7;  // wavefronts per SIMD k_dp_mid_rs<2> is compiled for
// resident wavefronts per CU of k_dp_mid_rs<R> (80 / .. / 124 registers)
inline int mid_waves_per_cu(int R) { return R == 1 ? 24 : (R == 2 ? 4 * MID_WAVES2 : 16); }
int launch_mid_rs(const KernelArgs &a, int R, int grid, void *stream, bool sw, bool flat);
// k_dp_tile_cs (npr_kernel_tile_cs.hip): k_dp_tile's stripes in column-scaled arithmetic -- one exponent per lane (pair of lattice columns);
// sw / flat as for launch_rs
int launch_tile_cs(const KernelArgs &a, int NW, int grid, void *stream, bool sw, bool flat);
size_t tile_cs_lds_bytes(int nw);
// ... and its E-step instance (k_dp_tile_cs<.., EM>): k_em_tile's job in that arithmetic; a task whose certificate fails comes back TASK_RERUN, uncounted
int launch_em_tile_cs(const KernelArgs &a, int NW, int grid, void *stream, bool sw, bool flat);
int em_tile_cs_waves();
int em_tile_cs_waves_per_cu();
size_t rs_lds_bytes();
int em_tile_waves();
int em_tile_waves_per_cu();
size_t em_wide_lds_bytes(int nw);
size_t wide_lds_bytes(int nw);
size_t stair_lds_bytes();
size_t generic_lds_bytes(int wcap);
int generic_max_wcap();

}  // namespace npr
