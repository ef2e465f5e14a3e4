/*
 * portello_liftover.h -- C ABI of the MI355X-native liftover engine.
 *
 * This is the drop-in boundary for portello's per-read CIGAR-composition hot path.  The reference has no FFI:
 * the path is three `pub fn`s called synchronously, one (read segment x contig segment) pair at a time, from
 *   get_liftover_alignment_for_read_and_contig_segment        src/read_alignment_scanner.rs:136-288
 * inside scan_chromosome_segment (src/read_alignment_scanner.rs:369-492).  A Rust caller binds the functions
 * below with `extern "C"`, keeps one `plo_ctx` per BamReaderWorkerThreadData
 * (src/worker_thread_data.rs:8-18) and turns the per-record loop into: collect window -> one batch call ->
 * finish records.
 *
 * Conventions
 *   - every function returns a plo_status (0 = ok) and never unwinds; plo_last_error() gives a message;
 *   - a plo_index is immutable after creation and may be shared by any number of contexts/threads;
 *   - a plo_ctx is single-threaded (one per worker thread), owns one HIP stream, its workspaces and its
 *     output buffers; output pointers stay valid until the next call on the same context;
 *   - one *item* = one call of get_liftover_alignment_for_read_and_contig_segment, i.e. one
 *     (read split segment x contig split segment) pair;
 *   - CIGAR ops use the BAM encoding `len << 4 | op`, op in M0 I1 D2 N3 S4 H5 P6 =7 X8 (rust-htslib `Cigar`);
 *   - all positions are 0-based; coordinates must fit the BAM 31-bit range (else PLO_ERR_RANGE);
 *   - there is NO CPU fallback: without a usable HIP device every entry point fails with PLO_ERR_NO_DEVICE.
 */
#ifndef PORTELLO_LIFTOVER_H
#define PORTELLO_LIFTOVER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLO_API_VERSION 20 /* 4: plo_timing starts with struct_size (the callee fills no more than the caller's struct holds); 5: plo_gather_*, plo_ctx_set_stats (plo_timing::algo_bytes / lane_utilisation of light items only on request), plo_ctx_stream / plo_ctx_device; 6: plo_ctx_set_phase_events; 7: plo_records_build_dev, plo_bam_window_batch_raw; 8: plo_bgzf_compress_dev, plo_bam_write_blocks; 9: plo_batch_build_dev, plo_bam_window_raw; 10: plo_bgzf_inflate_dev, plo_window_cut_dev; 11: plo_bgzf_inflate_part_dev, plo_window_cut_part_dev, plo_part_start_dev; 12: plo_nm_dev (NM:i on the records of plo_records_build_dev); 13: plo_md_dev (MD:Z on them, the source's MD cut); 14: plo_records_sort_dev (the window's records in coordinate order), plo_bam_output_header_so, plo_bam_merge_runs; 15: plo_records_index_dev (what a BAM index needs of every record of a sorted buffer), plo_bam_writer_index_enable / _index_add, plo_bam_merge_runs_indexed; 16: plo_eqx_dev (= / X CIGARs on the records of plo_records_build_dev); 17: plo_fasta_* (the reference FASTA loaded on the device), plo_fasta_load_file; 18: plo_runs_merge_plan_dev / plo_runs_merge_emit_dev (sorted windows merged into large runs on the device); 19: plo_depth_* (the depth of the records: difference array, scan, windows, runs) */

typedef enum plo_status {
    PLO_OK = 0,
    PLO_ERR_INVALID_ARG = 1,
    PLO_ERR_NO_DEVICE = 2,
    PLO_ERR_HIP = 3,
    PLO_ERR_OUT_OF_MEMORY = 4,
    PLO_ERR_RANGE = 5,    /* coordinate outside the 31-bit BAM range or invalid CIGAR op code            */
    PLO_ERR_INTERNAL = 6, /* device-side capacity exceeded even in the large-item path                  */
    PLO_ERR_IO = 7,       /* portello_bam.h: file cannot be opened / read / written, truncated or corrupt BGZF   */
    PLO_ERR_DATA = 8      /* input the reference aborts on: an item ended LEN_MISMATCH / PANIC when records are
                             finished (src/read_alignment_scanner.rs:207-229), or a record whose SA tag it would
                             panic on (portello_bam.h)                                                  */
} plo_status;

/* Per-item result status.  The reference expresses these as Option::None / panic!:
 *   LIFTED        Some(record)                                   src/read_alignment_scanner.rs:185,284
 *   NO_LIFTOVER   liftover_read_alignment returned None           src/liftover_read_alignment.rs:218
 *   LEN_MISMATCH  read length of lifted CIGAR != seq_len; the reference aborts   src/read_alignment_scanner.rs:204-229
 *   PANIC         a sequence index would be out of bounds (Rust slice-index panic in
 *                 simplify_alignment_indels.rs:58-60,74-77 / indel_breakend_homology.rs:38-39)
 *   NEED_BASES    no counterpart in the reference: the batch came with PLO_SEQ_BAM4_SPARSE bases, a sequence comparison
 *                 of this item reached bases the batch does not carry, and no `seq_full` was given to look them up in.
 *                 The item has no result; lift it again from a batch that holds the read's complete bases.       */
enum {
    PLO_ITEM_LIFTED = 0,
    PLO_ITEM_NO_LIFTOVER = 1,
    PLO_ITEM_LEN_MISMATCH = 2,
    PLO_ITEM_PANIC = 3,
    PLO_ITEM_NEED_BASES = 4
};

/* Read-sequence encodings accepted at the boundary */
enum {
    PLO_SEQ_BAM4 = 0, /* BAM 4-bit packing, 2 bases per byte, high nibble first, code table "=ACMGRSVTWYHKDBN"
                         (what bam::Record::seq() holds; decoded by as_bytes() at read_alignment_scanner.rs:170,238) */
    PLO_SEQ_ASCII = 1, /* one byte per base */
    PLO_SEQ_BAM4_SPARSE = 2
    /* BAM 4-bit packing, but only the bases the kernels are likely to look at travel to the device (the sequence
       comparisons of left_shift_indels / simplify_alignment_indels touch a few dozen bases around each indel, the other
       ~97 % of a HiFi read never leave the host).  A read's bases are cut into granules of 32 bases (16 bytes).  At
       read_seq_off[r] (a multiple of 16): a header of ceil(seq_len / 1024) pairs {uint32 mask, uint32 rank} -- mask bit k of
       pair b set = granule 32 b + k is present, rank = number of present granules before granule 32 b -- padded to a
       multiple of 16 bytes, followed by the present granules in ascending order, each the 16 bytes of the dense BAM4
       encoding (the last one zero-padded).  plo_sparse_seq_pack (portello_bam.h) writes this form from records / dense
       bases and CIGARs.  A comparison that reaches an absent granule is detected on the device and the item is lifted
       again from the read's complete bases (plo_batch_in::seq_full), so results never depend on which granules were sent. */
};

/* Where the sequence / batch buffers of a descriptor live */
enum {
    PLO_MEM_HOST = 0,  /* host memory: the library copies to the device */
    PLO_MEM_DEVICE = 1 /* device memory on the index's device: borrowed, caller keeps it alive */
};

/* Pipeline stages (bit mask).  PLO_STAGES_ALL reproduces get_liftover_alignment_for_read_and_contig_segment;
 * subsets expose the individual reference functions so that they can be pinned against the reference's own
 * known-answer tests. */
enum {
    PLO_STAGE_STRAND = 1u << 0,   /* caller glue src/read_alignment_scanner.rs:149-176: need_flipped, and for
                                     reverse-mapped contig segments rev_pos + reversed CIGAR                     */
    PLO_STAGE_LSHIFT = 1u << 1,   /* left_shift_indels (lib/rust-vc-utils/.../shift_indels/left_shift_indels.rs:17-39);
                                     with STRAND: only items on reverse-mapped contig segments (as the reference),
                                     without STRAND: every item, CIGAR/pos used as given, ref_seq = the contig's
                                     rev_contig_seq                                                              */
    PLO_STAGE_LIFTOVER = 1u << 2, /* liftover_read_alignment  src/liftover_read_alignment.rs:137-223            */
    PLO_STAGE_LENCHECK = 1u << 3, /* seq_len == get_cigar_read_offset(cigar,false)  read_alignment_scanner.rs:204-229 */
    PLO_STAGE_SIMPLIFY = 1u << 4, /* simplify_alignment_indels src/simplify_alignment_indels.rs:119-156,
                                     ref_seq = reference[chrom_index of the contig segment]                      */
    PLO_STAGES_ALL = 0x1f
};

/* ------------------------------------------------------------------------------------------------------------
 * Index: the contig->reference mapping consumed by phase 2, i.e. AllContigMappingInfo
 * (src/contig_alignment_scanner/mod.rs:25-47,76) + the reference sequences (src/main.rs:24-62) + contig lengths
 * (ChromList of the read->contig BAM, src/read_alignment_scanner.rs:163-164).
 * plo_index_create builds, per contig segment, the block map of get_read_segment_to_ref_pos_tree_map
 * (lib/rust-vc-utils/src/bam_utils/read_to_ref_map.rs:101-137, ignore_hard_clip = false as at
 * contig_alignment_scanner/mod.rs:98-102) on the device and packs everything into HBM once.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct plo_index_desc {
    /* contigs (index = tid in the read->contig BAM) */
    uint32_t n_contigs;
    const int64_t *contig_len;      /* [n_contigs] */
    const uint32_t *contig_seg_off; /* [n_contigs+1] CSR into the segment arrays = ordered_contig_segment_info */

    /* contig split segments, sequencing order within each contig (SeqOrderSplitReadSegment,
       lib/rust-vc-utils/src/bam_utils/split_read.rs:15-32) */
    uint32_t n_segments;
    const uint32_t *seg_chrom_index;      /* reference chromosome the segment maps to            */
    const int64_t *seg_pos;               /* 0-based reference start of the segment alignment    */
    const uint8_t *seg_is_fwd_strand;     /* 1 = contig segment maps to the forward strand       */
    const uint8_t *seg_mapq;
    const int64_t *seg_seq_order_start;   /* seq_order_read_start (contig coordinates)           */
    const int64_t *seg_seq_order_end;     /* seq_order_read_end                                  */
    const uint32_t *seg_cigar_off;        /* [n_segments+1] CSR into seg_cigar                   */
    const uint32_t *seg_cigar;            /* contig->reference CIGARs, BAM-encoded ops           */

    /* reference chromosomes: `reference: &[Vec<u8>]` (upper-cased ASCII, src/main.rs:24-62) */
    uint32_t n_chroms;
    const int64_t *chrom_len;             /* [n_chroms] */
    const uint8_t *const *chrom_seq;      /* [n_chroms] pointers (see seq_mem) */

    /* ContigMappingInfo::rev_contig_seq (contig_alignment_scanner/mod.rs:113-125): ASCII, length contig_len,
       NULL where the contig has no reverse-mapped segment */
    const uint8_t *const *rev_contig_seq; /* [n_contigs] pointers or NULL array */

    int32_t seq_mem;                      /* PLO_MEM_HOST or PLO_MEM_DEVICE for chrom_seq / rev_contig_seq */
} plo_index_desc;

typedef struct plo_index plo_index;
typedef struct plo_ctx plo_ctx;

/* ------------------------------------------------------------------------------------------------------------
 * Batch input: a window of primary read records with their sequencing-order split segments
 * (get_seq_order_read_split_segments output, read_alignment_scanner.rs:421).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct plo_batch_in {
    /* reads = primary bam::Record's */
    uint32_t n_reads;
    const uint8_t *read_is_reverse;  /* [n_reads] record.is_reverse()                          */
    const uint32_t *read_seq_len;    /* [n_reads] record.seq_len()                             */
    const uint64_t *read_seq_off;    /* [n_reads] byte offset of the read's bases inside `seq` */
    const uint8_t *seq;              /* all read bases, encoding `seq_fmt`                      */
    uint64_t seq_bytes;              /* size of `seq` in bytes                                  */
    int32_t seq_fmt;                 /* PLO_SEQ_BAM4 / PLO_SEQ_ASCII / PLO_SEQ_BAM4_SPARSE      */

    /* read split segments (SeqOrderSplitReadSegment) */
    uint32_t n_segs;
    const uint32_t *seg_read;        /* [n_segs] index of the owning read                      */
    const uint32_t *seg_contig;      /* [n_segs] chrom_index = contig the segment is aligned to */
    const int64_t *seg_pos;          /* [n_segs] 0-based position on the forward contig         */
    const uint8_t *seg_is_fwd_strand;/* [n_segs]                                                */
    const uint32_t *seg_cigar_off;   /* [n_segs+1] CSR into `cigar`                             */
    const uint32_t *cigar;           /* read->contig CIGARs                                     */

    /* Optional explicit item list.  NULL: the engine enumerates items itself with the overlap rule of
       get_contig_split_segments_from_read_mapping (read_alignment_scanner.rs:80-103).  Non-NULL: item i pairs
       read segment item_seg[i] with contig segment item_cseg[i] (index *within the contig's segment list*). */
    uint32_t n_items;
    const uint32_t *item_seg;
    const uint32_t *item_cseg;

    /* PLO_SEQ_BAM4_SPARSE only, optional (NULL: items that reach absent bases end PLO_ITEM_NEED_BASES).  HOST memory in both
       entry points: the dense BAM4 bases of read r start at seq_full + read_seq_full_off[r] (e.g. inside the BAM record the
       read came from).  Read only for the reads of such items, after the first pass over the batch. */
    const uint8_t *seq_full;
    const uint64_t *read_seq_full_off; /* [n_reads] */
} plo_batch_in;

/* Batch output (SoA, one entry per item, ordered by (read segment, contig segment index)).
 * plo_liftover_batch: pointers are host (pinned) memory owned by the context.
 * plo_liftover_batch_dev: pointers are device memory owned by the context. */
typedef struct plo_batch_out {
    uint32_t n_items;
    const uint32_t *item_seg;          /* read segment index                                                  */
    const uint32_t *item_cseg;         /* contig_segment_index (as used in the PS tag, :257-262)              */
    const uint8_t *item_status;        /* PLO_ITEM_*                                                          */
    const uint8_t *item_need_flipped;  /* need_flipped_read_alignment (:153-157)                              */
    const uint8_t *item_mapq;          /* contig segment MAPQ adopted by the record (:250-252)                */
    const uint32_t *item_chrom_index;  /* tid of the lifted record (:232-247)                                 */
    const int64_t *item_ref_pos;       /* lifted 0-based position (valid when LIFTED/LEN_MISMATCH)            */
    const uint64_t *item_cigar_off;    /* offset of the item's CIGAR inside `cigar`                           */
    const uint32_t *item_cigar_len;    /* number of ops                                                       */
    const uint32_t *cigar;             /* lifted CIGARs                                                       */
    uint64_t n_cigar;                  /* extent of `cigar` in ops (items index it through item_cigar_off; the
                                          buffer is slab-allocated on the device and may contain unused gaps)  */
} plo_batch_out;

/* Per-call device timing measured with HIP events on the context's stream.
   `struct_size`: set by the CALLER to sizeof(plo_timing) of the header it was built against before plo_ctx_timing;
   the library writes at most that many bytes (fields are only ever appended), and stores the size it filled. */
typedef struct plo_timing {
    uint32_t struct_size;
    float total_ms;      /* first kernel start -> last kernel end                                   */
    float enumerate_ms;  /* item enumeration + scans                                                */
    float lift_ms;       /* the wave-cooperative tile kernels of the scan formulation (k_lift_tiles*: light items of batches the lane
                            kernel does not take)                                                      */
    float big_ms;        /* one-wave-per-item kernel in global scratch (0 if not launched)          */
    uint32_t n_items;
    uint32_t n_big_items; /* items of that kernel */
    uint64_t n_in_ops;   /* input CIGAR ops over all items                                          */
    uint64_t n_out_ops;  /* output CIGAR ops                                                        */
    uint64_t algo_bytes; /* algorithmic bytes of the call, SURVEY.md 8(d) formula, counted on device.  The light-item kernel
                            (k_lift_lanes) counts them only on a context with plo_ctx_set_stats(ctx, 1): its production
                            instantiation is compiled without the counters (0 from its items otherwise)              */
    float lanes_ms;      /* the lane-per-item kernel (k_lift_lanes: items whose working region fits an LDS share)  */
    float retry_ms;      /* items of tiles that overflowed their LDS slice, re-run one per wave       */
    uint32_t n_lane_items;
    uint32_t n_retry_items;
    float mid_ms;        /* workgroup-per-item kernel (items too heavy for a shared tile)             */
    uint32_t n_mid_items;
    uint32_t n_miss_items; /* PLO_SEQ_BAM4_SPARSE: items that reached absent bases (lifted again from seq_full) */
    float miss_ms;         /* that second pass: list download, host gather, upload, kernel (wall clock)         */
    uint32_t tile_cap;     /* geometry of the tile kernel for this batch: elements per LDS slice (256: the variant with the
                              capacity compiled in, k_lift_tiles_c256) and window of item weights per tile        */
    uint32_t tile_window;
    float heavy_lanes_ms;        /* the heavy items' lane-per-item kernel, `heavy_kernel` says which (k_lift_lanes_g / _w3: regions in
                                    global scratch behind LDS windows; k_lift_stream: teams of waves); lift_ms / mid_ms are 0 then */
    uint32_t n_heavy_lane_items;
    float lane_utilisation;      /* lane-per-item kernels: lanes at work / (64 x loop trips), summed over the liftover loop and the
                                    shift stage's event rounds of all waves (0 when no such kernel ran; the light-item kernel
                                    counts only under plo_ctx_set_stats, as for algo_bytes)                                   */
    uint32_t heavy_kernel;       /* which kernel `heavy_lanes_ms` is the time of: 0 none, 1 k_lift_lanes_g, 2 k_lift_lanes_g_w3,
                                    3 k_lift_stream (teams of waves, stages chained through LDS rings)                       */
    uint32_t host_syncs;         /* host round trips of the call (stream synchronisations that returned counts to the host)  */
} plo_timing;

plo_status plo_index_create(const plo_index_desc *desc, int device, plo_index **out);
void plo_index_destroy(plo_index *index);
/* number of block-map entries of contig segment `global_seg` (= contig_seg_off[contig] + i), and a copy of them
   (keys = contig positions, vals = reference positions, INT64_MIN for None), downloaded from the device, for
   inspection/tests */
plo_status plo_index_segment_map(const plo_index *index, uint32_t global_seg, uint32_t cap, int64_t *keys,
                                 int64_t *vals, uint32_t *n_entries);

/* `hip_stream`: a hipStream_t to run on (e.g. torch's current stream) or NULL to create a private one */
plo_status plo_ctx_create(const plo_index *index, void *hip_stream, plo_ctx **out);
void plo_ctx_destroy(plo_ctx *ctx);
/* on != 0: the light-item kernel of this context's later calls counts plo_timing::algo_bytes and lane_utilisation (an instantiation with
   the counters in its loops, a few per cent slower); default: off, or what the environment's PLO_LANE_STATS says at plo_ctx_create */
plo_status plo_ctx_set_stats(plo_ctx *ctx, int on);
/* on == 0: the one-round-trip calls of this context (plo_liftover_batch_dev on a context whose last batch had light items only) record no
   HIP events between their phases -- every record is a bubble of ~6 us on the stream, 5 % of a reference-sized window's call -- and
   plo_ctx_timing then reports the counts of such a call but no times (enumerate_ms, lanes_ms, total_ms = 0).  A production caller that
   never asks for the times switches them off; default: on (or what the environment's PLO_PHASE_EVENTS says at plo_ctx_create). */
plo_status plo_ctx_set_phase_events(plo_ctx *ctx, int on);

/* Host buffers in, host (pinned, context-owned) buffers out; synchronous. */
plo_status plo_liftover_batch(plo_ctx *ctx, const plo_batch_in *in, uint32_t stages, plo_batch_out *out);
/* Device buffers in, device (context-owned) buffers out; returns after the result sizes are known, output is
   complete on the context's stream (call plo_ctx_sync or synchronise the stream before reading it).
   The batch is checked on the device before any lift kernel runs.
   PLO_ERR_INVALID_ARG: an index outside its array -- a seg_cigar_off entry below its predecessor or above
   seg_cigar_off[n_segs] among them.
   PLO_ERR_RANGE: a coordinate outside the 31-bit BAM range (seg_pos below 0 or above 0x7ffffff0); an op code above 8; a CIGAR
   spanning 2^30 bases or more (the last span accepted is 2^30 - 1); a read segment that ends behind its contig's end and
   meets a reverse-strand contig segment (rev_pos, src/read_alignment_scanner.rs:164-166, would be negative: the reference
   panics there); more than 2^31 - 1 ops / item weights in the batch.
   A batch with faults of both kinds, in whichever segments, gets PLO_ERR_INVALID_ARG. */
plo_status plo_liftover_batch_dev(plo_ctx *ctx, const plo_batch_in *in, uint32_t stages, plo_batch_out *out);

/* ------------------------------------------------------------------------------------------------------------
 * Record finishing (the part of src/read_alignment_scanner.rs:245-284 and :310-346 that is arithmetic on the
 * record, not htslib bookkeeping): for the result of the LAST plo_liftover_batch_dev call on this context
 *   - per lifted item: flags (BAM_FREVERSE toggled when need_flipped :274-276,:126; supplementary set :282, cleared
 *     on the primary :346), reference end (get_alignment_end, lib/rust-vc-utils/src/bam_utils/bam_record_utils.rs:21-27)
 *     and bin (bam_reg2bin, lib/rust-vc-utils/src/bam_utils/util.rs:10-35, :278-279);
 *   - per read: number of lifted records, the primary one (max MAPQ, first wins :338-346), and for reads without any
 *     lifted record the flags of the unmapped copy (:317-335);
 *   - reverse_alignment_seq_and_qual (:125-133) for every record that needs it (lifted items with need_flipped,
 *     unmapped copies of reverse-strand reads): 4-bit reverse complement (decode, comp_base, re-encode) + reversed
 *     qualities, written into two context-owned buffers.
 * Requires seg_read to be non-decreasing (segments grouped by read, as get_seq_order_read_split_segments yields them).
 * All pointers are device pointers.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct plo_finish_in {
    const uint16_t *read_flags;    /* [n_reads] record.flags() of the primary read->contig records   */
    const uint8_t *qual;           /* base qualities of all reads (1 byte per base)                  */
    const uint64_t *read_qual_off; /* [n_reads] byte offset of the read's qualities inside `qual`     */
    uint64_t qual_bytes;           /* size of `qual`                                                  */
} plo_finish_in;

#define PLO_NO_FLIP UINT64_MAX

typedef struct plo_finish_out {
    /* per item (same order as plo_batch_out) */
    const uint16_t *item_flag;     /* flags of the lifted record (valid for LIFTED items)             */
    const uint16_t *item_bin;
    const int64_t *item_ref_end;
    const uint8_t *item_is_primary;
    const uint64_t *item_seq_off;  /* byte offset of the flipped bases inside rev_seq, PLO_NO_FLIP if the record keeps
                                      the read's original seq/qual                                    */
    const uint64_t *item_qual_off; /* same for rev_qual                                                */
    /* per read */
    const uint32_t *read_n_lifted;
    const uint32_t *read_primary_item; /* item index of the primary record (UINT32_MAX if none)       */
    const uint16_t *read_unmapped_flag; /* flags of the unmapped copy (valid when read_n_lifted == 0)  */
    const uint64_t *read_seq_off;  /* flipped bases of the unmapped copy, PLO_NO_FLIP if not needed    */
    const uint64_t *read_qual_off;
    /* flipped sequences */
    const uint8_t *rev_seq;        /* same encoding as the batch's seq_fmt, every record 16-byte aligned */
    const uint8_t *rev_qual;
    uint64_t rev_seq_bytes, rev_qual_bytes;
    float finish_ms, revcomp_ms;   /* HIP-event times of the two kernels groups                        */
    uint32_t n_items, n_reads;     /* extents of the per-item / per-read arrays: the batch they were made for (API version 4;
                                      plo_records_build_finished refuses arrays of another batch before indexing them) */
} plo_finish_out;

plo_status plo_finish_batch_dev(plo_ctx *ctx, const plo_batch_in *in, const plo_finish_in *fin, plo_finish_out *out);

/* ---- SA tag text (device-resident) ----------------------------------------------------------------------------
 * Consumes the results of the preceding plo_liftover_batch_dev + plo_finish_batch_dev on the same context and writes,
 * for every LIFTED item of a read that has at least two lifted records, the text of get_sa_tag_segment
 * (src/read_alignment_scanner.rs:292-301): "{chrom},{pos+1},{strand},{cigar},{mapq},0;".  The SA:Z value of record j is
 * the concatenation of the segments of the read's other lifted items in item order (:352-364, done by the caller:
 * items of a read are consecutive).  Chromosome labels are ChromList labels (the reference BAM header's @SQ names).
 * All pointers are device pointers; outputs are owned by the context and valid until its next call. */
typedef struct plo_sa_in {
    uint32_t n_chroms;
    const uint32_t *chrom_name_off; /* [n_chroms + 1] byte offsets into chrom_names                    */
    const uint8_t *chrom_names;     /* concatenated labels, no terminators                             */
} plo_sa_in;

typedef struct plo_sa_out {
    uint32_t n_items;
    const uint32_t *item_sa_off;    /* [n_items + 1] byte offsets into sa_text; empty range = no segment */
    const uint8_t *sa_text;
    uint64_t sa_bytes;
    float sa_ms;
} plo_sa_out;

plo_status plo_sa_segments_dev(plo_ctx *ctx, const plo_sa_in *in, plo_sa_out *out);

/* ---- Output records (device-resident) ---------------------------------------------------------------------------
 * Consumes the results of the preceding plo_liftover_batch_dev (+ plo_compact_output_dev), plo_finish_batch_dev and
 * plo_sa_segments_dev on the same context and writes the window's output BAM records -- for every read, in order, its lifted
 * records (item order) or, when nothing lifted and !is_target_region, the unmapped copy -- byte for byte what
 * plo_records_build (portello_bam.h) writes from host copies: clone_record with NM / SA / PS / ZM removed
 * (src/read_alignment_scanner.rs:105-118), PS / ZM :254-268, pos / CIGAR / flags / bin :270-282, reversed bases and qualities
 * :125-133, unmapped copy :317-335, SA :348-364, serialised as bam_write1 does (CG:B,I beyond 65535 CIGAR ops).
 * `records` holds the window's stretch of the BAM stream as it stands (plo_bam_window_batch_raw, portello_bam.h: the batch's `seq` and
 * the finishing's `qual` may be views into the same buffer).  PS:Z labels are the @SQ names of the read->contig BAM; the strand suffix
 * comes from the context's index, the SA labels are already inside the SA text.  The label table is trusted as plo_sa_in's is
 * (contig_name_off non-decreasing and inside contig_names): the caller makes it from the BAM header, it is not data of the stream.
 * Every record is checked on the device before a byte is written: a read_rec_off or a record's block_size / l_qname / n_cigar /
 * l_seq that points outside `records`, or an l_seq that differs from the batch's read_seq_len -> PLO_ERR_INVALID_ARG, nothing written.
 * Called out of order (no finish / SA result on the context), or after a batch with sparse or ASCII bases -> PLO_ERR_INVALID_ARG.
 * The stream is waited for twice: once for the sizes and once behind the emit kernel, for the event times -- like
 * plo_finish_batch_dev and plo_sa_segments_dev the call returns when its kernels are through, so a caller cannot put the download
 * of one window under the emit kernel of the same context.  All pointers are device pointers; outputs are owned by the context, valid until its next call. */
typedef struct plo_records_in {
    const uint8_t *records;          /* the window's records as they stand: block_size word + block_size bytes each   */
    uint64_t records_bytes;
    const uint64_t *read_rec_off;    /* [n_reads] offset of primary record r's block_size word inside `records`       */
    uint32_t n_contigs;              /* at least the index's contigs                                                   */
    const uint32_t *contig_name_off; /* [n_contigs + 1] byte offsets into contig_names                                 */
    const uint8_t *contig_names;     /* concatenated labels, no terminators                                            */
    int32_t is_target_region;        /* src/read_alignment_scanner.rs:318-320: no unmapped copy                        */
} plo_records_in;

typedef struct plo_records_out {
    const uint8_t *bytes;            /* records, each prefixed by its block_size: what plo_bam_write takes             */
    uint64_t n_bytes;
    uint32_t n_records;
    const uint64_t *record_off;      /* [n_records + 1]                                                                */
    uint32_t n_lifted, n_unmapped_copies;
    float records_ms;                /* HIP-event time of this call's work on the stream: plan + scans + the 40 bytes of sizes
                                        copied back, then (behind the host's look at them) emit + 8 bytes up for record_off's end */
} plo_records_out;

plo_status plo_records_build_dev(plo_ctx *ctx, const plo_batch_in *in, const plo_records_in *rin, plo_records_out *out);

/* ---- NM:i of the lifted records (device-resident, opt-in) ---------------------------------------------------------
 * clone_record cuts NM (src/read_alignment_scanner.rs:105-118): the edit distance against the contig is wrong on the reference, and
 * nothing puts the right one back -- the reference's answer is a samtools calmd pass over the sorted output.  plo_nm_dev counts it for
 * every item with status PLO_ITEM_LIFTED from what the context holds already: the item's output CIGAR (as plo_records_build_dev writes
 * it), the record's bases in the orientation the record carries them (plo_finish_out::rev_seq when item_seq_off != PLO_NO_FLIP, the
 * batch's `seq` otherwise; BAM 4-bit, high nibble first) and the index's chrom_seq from item_ref_pos on.  The rule is calmd's
 * (bam_md.c): M / = / X compare base by base -- with c1 the read's code and c2 the reference byte's code in "=ACMGRSVTWYHKDBN" (any other
 * byte: 15) a pair matches iff c1 == 0, or c1 == c2 and c1 != 15 (N against N is a mismatch, R against R a match, a read '=' matches
 * anything); I and D add their lengths; N, S, H, P add nothing.
 * Call it after plo_liftover_batch_dev (+ plo_compact_output_dev) and plo_finish_batch_dev on the same context and batch.  Called out of
 * order, after a batch with PLO_SEQ_BAM4_SPARSE or PLO_SEQ_ASCII bases, or on an index without chrom_seq -> PLO_ERR_INVALID_ARG.  A CIGAR
 * that consumes more reference than the chromosome has behind item_ref_pos, or more bases than read_seq_len, is refused by a check on the
 * device before any such base is read -> PLO_ERR_RANGE, err_item is the LOWEST such item, no result is handed out.
 * While the context holds a result, plo_records_build_dev writes NM:i (always type i: 'N','M','i' + u32 LE, 7 bytes, the form calmd
 * appends) into every lifted record, directly behind ZM:C and in front of SA:Z / CG:B,I; the unmapped copy gets none.  Without a result
 * its bytes are the host builder's, as before.  The result is dropped by the context's next plo_liftover_batch* (and plo_finish_batch_dev)
 * call, so a caller who does not ask for NM never sees it.  NM exists on this route only: plo_records_build and
 * plo_records_build_finished (portello_bam.h) write no NM.  One launch, one wait.  Outputs are owned by the context, valid until its
 * next plo_liftover_batch* call. */
typedef struct plo_nm_out {
    uint32_t n_items;
    const uint32_t *item_nm;     /* [n_items] device; 0 for items that are not LIFTED */
    uint64_t n_cmp_bases;        /* bases compared (M / = / X), whole batch */
    uint32_t err_item;           /* PLO_ERR_RANGE: lowest offending item, UINT32_MAX otherwise */
    float nm_ms;                 /* HIP-event time of the call's kernels */
} plo_nm_out;

plo_status plo_nm_dev(plo_ctx *ctx, const plo_batch_in *in, plo_nm_out *out);

/* ---- MD:Z of the lifted records (device-resident, opt-in) ---------------------------------------------------------
 * calmd's second output.  clone_record does not cut MD: a source record that carries one (against the contig) leaves with it unchanged,
 * and it is wrong on the reference.  plo_md_dev writes the text for every item with status PLO_ITEM_LIFTED from the same inputs as
 * plo_nm_dev.  The rule is bam_fillmd1_core's (bam_md.c): a counter u of matched bases starts at 0; M / = / X go base by base, a pair
 * matches exactly as for plo_nm_dev; a match does ++u, a mismatch writes u in decimal (also 0), the reference letter, u = 0.  A D of
 * length > 0 writes u (also 0), '^', its reference letters, u = 0 (two in a row: ...^AC0^GTT...).  I, S, N, H, P write nothing and keep u.
 * At the end u is written, so the text of a LIFTED item is never empty ("0" without compared bases and deletions).  Ops of length 0 are
 * skipped: calmd would write an empty '^' for 0D, the lift never emits one.  The reference letter is the chrom_seq byte: A..Z as it
 * is, a..z upper-cased (calmd's toupper), any other byte 'N', which keeps the text inside [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*.  The letters
 * of the text (those behind '^' too) plus the I lengths are plo_nm_dev's NM of the item.
 * Call order and refusals are plo_nm_dev's: after plo_liftover_batch_dev (+ plo_compact_output_dev) and plo_finish_batch_dev on the same
 * context and batch; out of order, sparse or ASCII bases, an index without chrom_seq -> PLO_ERR_INVALID_ARG; a CIGAR past the chromosome
 * or the read -> PLO_ERR_RANGE by the same check on the device, err_item the LOWEST such item, no result handed out.  The call is
 * independent of plo_nm_dev: either alone, both in either order, neither drops the other's result.
 * While the context holds a result, plo_records_build_dev writes 'M','D','Z' + text + NUL into every lifted record, behind ZM:C, behind
 * NM:i when that is written too (calmd appends NM, then MD), in front of SA:Z / CG:B,I, and cuts the FIRST field tagged MD of the source
 * record, whatever its type, from the lifted records.  The unmapped copy gets no MD and keeps its source aux bytes.  Without a result every
 * byte is as before, a stale source MD included.  The result is dropped by the context's next plo_liftover_batch* (and
 * plo_finish_batch_dev) call.  Host builders write no MD.  Two passes over the same bytes (lengths, then text) with the 64-bit scan of the
 * lengths between them; TWO waits: one for the total size, one behind the emit.  Outputs are owned by the context, valid until its next
 * plo_liftover_batch* call. */
typedef struct plo_md_out {
    uint32_t n_items;
    const uint64_t *item_md_off;  /* [n_items + 1] device; an item that is not LIFTED has length 0 */
    const uint8_t *md_text;       /* device; the values side by side, no tag, no NUL */
    uint64_t md_bytes;
    uint32_t err_item;            /* PLO_ERR_RANGE: lowest offending item, UINT32_MAX otherwise */
    float md_ms;                  /* HIP-event time of the call's kernels */
} plo_md_out;

plo_status plo_md_dev(plo_ctx *ctx, const plo_batch_in *in, plo_md_out *out);

/* ---- = / X CIGARs of the lifted records (device-resident, opt-in) ------------------------------------------------
 * The reads that go in are pbmm2 alignments with '=' and 'X' ops; liftover_read_alignment maps every compared op to M
 * (src/liftover_read_alignment.rs:103-107) and simplify_alignment_indels pushes M only, so the records that come out carry M alone, and
 * the reference tool offers no way to put the ops back.  plo_eqx_dev rewrites the CIGAR of every item with status PLO_ITEM_LIFTED from the
 * same inputs as plo_nm_dev and plo_md_dev.  The rule: walk the item's output CIGAR (the ops plo_records_build_dev writes without this call).
 * An op with code M, = or X and length L is COMPARED: its L base pairs are classified by plo_nm_dev's pair rule -- c1 the read's 4-bit
 * code, c2 the reference byte's code in "=ACMGRSVTWYHKDBN" (any other byte 15); a pair matches iff c1 == 0, or c1 == c2 and c1 != 15 (N
 * against N is X, R against R is =, a read '=' is =, a reference byte outside the table is X unless the read has '=') -- and the op is
 * replaced by its maximal runs, '=' for a run of matching and 'X' for a run of mismatching pairs, in order.  Runs do not cross op
 * boundaries (5M5= over ten matching pairs gives 5=5=), so every output op is no longer than the op it came from and its length fits 28
 * bits; the output has no two adjacent alike ops wherever the input has none, which compress_cigar guarantees for the lift's CIGARs.  A
 * compared op of length 0 yields nothing.  Every other op (I, D, N, S, H, P, codes 9-15) is copied as it stands, in its place.  Reference
 * length, read length, pos, bin and item_ref_end therefore do not change.  The bases under X plus the I and D lengths are the item's
 * plo_nm_dev value; the X positions are the mismatch letters of its plo_md_dev text that do not stand behind '^'.  Example: reference
 * ACGTACGT from pos, read ACGAACGT, 8M -> 3=1X4=; 2S4M1I3M rewrites only the 4M and the 3M.
 * Call order and refusals are plo_md_dev's: after plo_liftover_batch_dev (+ plo_compact_output_dev) and plo_finish_batch_dev on the same
 * context and batch; out of order, sparse or ASCII bases, an index without chrom_seq -> PLO_ERR_INVALID_ARG; a CIGAR past the chromosome
 * or the read -> PLO_ERR_RANGE by the same check on the device before a base of the step is touched, err_item the LOWEST such item, no
 * result handed out.  The call is independent of plo_nm_dev and plo_md_dev: alone or with either or both, in any order, none of the three
 * drops another's result; plo_nm_dev and plo_md_dev go on reading the lift's M CIGAR, so their results are the same either way.
 * While the context holds a result, plo_records_build_dev takes every lifted record's CIGAR from it: n_cigar_op, the ops in the record,
 * and bam_write1's rule by the NEW count -- an item whose = / X CIGAR has more than 65535 ops gets the <l_seq>S<ref_len>N placeholder and
 * its real ops in CG:B,I even where its M CIGAR had fewer.  Everything else in a record is byte for byte what it is without the call.
 * SA:Z is NOT changed: it keeps the M CIGARs plo_sa_segments_dev wrote (minimap2's and pbmm2's SA fields are summaries in M as well).
 * Without a result every byte is as before.  The result is dropped by the context's next plo_liftover_batch* (and plo_finish_batch_dev)
 * call.  Host builders write no = / X.  Two passes over the same bytes (op counts, then ops) with the 64-bit scan of the counts between
 * them; TWO waits: one for the total that sizes eqx_ops, one behind the emit.  Outputs are owned by the context, valid until its next
 * plo_liftover_batch* call. */
typedef struct plo_eqx_out {
    uint32_t n_items;
    const uint64_t *item_eqx_off;  /* [n_items + 1] device, in ops; an item that is not LIFTED has length 0 */
    const uint32_t *eqx_ops;       /* device; BAM-encoded ops (len << 4 | code), the items side by side */
    uint64_t n_ops;
    uint32_t err_item;             /* PLO_ERR_RANGE: lowest offending item, UINT32_MAX otherwise */
    float eqx_ms;                  /* HIP-event time of the call's kernels */
} plo_eqx_out;

plo_status plo_eqx_dev(plo_ctx *ctx, const plo_batch_in *in, plo_eqx_out *out);

/* ---- BGZF blocks (device-resident) ------------------------------------------------------------------------------
 * Cuts the n_bytes at `bytes` -- any device buffer, typically plo_records_out::bytes -- into payloads of 0xff00 bytes (htslib's
 * BGZF_BLOCK_SIZE), the last one short, and writes each as a complete BGZF block: the 18-byte gzip header with the `BC` subfield and
 * BSIZE, deflate data ending in a BFINAL block, CRC-32, ISIZE.  One wavefront per block (deflate.hpp).
 *   level 0: a stored block; the bytes are exactly those plo_bam_write writes for the same payload at level 0.
 *   level 1: LZ77 within the block and a dynamic Huffman code; a block whose deflate form is not smaller than 5 + len bytes is written
 *            stored, so level 1 is never larger than level 0 and no block exceeds 18 + 5 + 0xff00 + 8 bytes.  The bytes of a block depend
 *            on its payload alone.  This is the device's one deflate level; it is not byte-identical with zlib or htslib at any level.
 *   any other level: PLO_ERR_INVALID_ARG.  n_bytes == 0: PLO_OK with zero blocks.  bytes == NULL with n_bytes > 0: PLO_ERR_INVALID_ARG.
 * The blocks are packed densely, without the EOF block: plo_bam_write_blocks (portello_bam.h) appends them to a writer as they are.
 * The call uses buffers of its own: the output of the preceding plo_records_build_dev (and of every other call) on the context stays
 * valid and unchanged.  Like its neighbours the call returns when its kernels are through.  All pointers are device pointers; outputs
 * are owned by the context, valid until its next plo_bgzf_compress_dev.
 * Device memory the context keeps for it (grown to the largest call, freed with the context): the fixed-stride slots and the dense
 * output, each n_blocks x (18 + 5 + 0xff00 + 8) bytes, i.e. two buffers of about the input's size each (2.4 GB for a 1.19 GB window),
 * plus, at level 1, 130 560 bytes of token buffer per resident wave (at most 3 workgroups of 4 waves per CU: 401 MB on 256 CUs). */
typedef struct plo_bgzf_out {
    const uint8_t *blocks;      /* n_blocks complete BGZF blocks, densely packed, no EOF block                          */
    uint64_t n_bytes;
    uint32_t n_blocks;
    const uint64_t *block_off;  /* [n_blocks + 1]                                                                        */
    uint64_t n_in;              /* payload bytes consumed                                                                */
    float bgzf_ms;              /* HIP-event time of this call's kernels                                                 */
} plo_bgzf_out;

plo_status plo_bgzf_compress_dev(plo_ctx *ctx, const uint8_t *bytes, uint64_t n_bytes, int level, plo_bgzf_out *out);

/* ---- Coordinate-sorted records (device-resident, opt-in; API version 14) --------------------------------------------
 * The records at `bytes` -- each prefixed by its block_size, typically plo_records_out::bytes / record_off -- copied in coordinate order
 * into a buffer of the call's own.  The key of a record is
 *     (uint64)(refID < 0 ? n_ref : refID) << 32 | (uint64)(pos + 1) << 1 | ((flag >> 4) & 1)
 * with refID at +4, pos at +8 and flag at +18 from the block_size word, little-endian, and the records are ordered by the pair (key, input
 * index): references in header order, then position, forward before reverse, refID -1 last, ties in input order.  The pair is unique, so
 * the result is fully determined.
 * Checked on the device before any byte is moved: record_off[0] == 0, record_off does not decrease and ends at n_bytes; every record is
 * at least 36 bytes long and block_size + 4 is its length; refID lies in [-1, n_ref), pos in [-1, 2^31 - 2].  A record that breaks one of
 * these -> PLO_ERR_INVALID_ARG, err_record the LOWEST such record, no result handed out, plo_last_error names the record and the field.
 * n_records == 0 -> PLO_OK with empty outputs (record_off[0] == 0); NULL bytes or record_off with n_records > 0 -> PLO_ERR_INVALID_ARG.
 * Buffers: the call's own, grown to the largest call and freed with the context: one copy of the window's bytes (n_bytes), two arrays of
 * keys (2 x 8 n), two of indices (2 x 4 n), the lengths in input and in sorted order (2 x 8 n) and the offsets (8 (n + 1)): n_bytes +
 * 48 n_records in all.  The input, the outputs of plo_records_build_dev and of every other call on the context stay valid and unchanged;
 * the call's own outputs are valid until the context's next plo_records_sort_dev.  plo_bgzf_compress_dev takes out->bytes as it takes
 * plo_records_out::bytes.  The call runs on the context's stream and returns when its kernels are through: ONE wait. */
typedef struct plo_sort_in {
    const uint8_t *bytes;         /* device: records, each prefixed by its block_size (plo_records_out::bytes, or any such buffer) */
    uint64_t n_bytes;
    uint32_t n_records;
    const uint64_t *record_off;   /* device [n_records + 1] */
    uint32_t n_ref;               /* @SQ count of the output header: refID must lie in [-1, n_ref) */
} plo_sort_in;

typedef struct plo_sort_out {
    const uint8_t *bytes;         /* device: the same records in sorted order, densely packed */
    uint64_t n_bytes;             /* == in->n_bytes */
    uint32_t n_records;
    const uint64_t *record_off;   /* device [n_records + 1], of the sorted buffer */
    const uint32_t *perm;         /* device [n_records]: sorted position j holds input record perm[j] */
    const uint64_t *key;          /* device [n_records]: the sorted keys */
    uint32_t n_mapped;            /* records with refID >= 0; the refID -1 tail begins at this sorted position */
    uint32_t err_record;          /* PLO_ERR_INVALID_ARG from the device check: lowest offending input record, else UINT32_MAX */
    float sort_ms;                /* HIP-event time of the call's kernels */
} plo_sort_out;

plo_status plo_records_sort_dev(plo_ctx *ctx, const plo_sort_in *in, plo_sort_out *out);

/* ---- Index entries of coordinate-sorted records (device-resident, opt-in; API version 15) -----------------------------
 * What a BAM index (BAI, SAMv1 5.2) needs of every record at `bytes` -- typically plo_sort_out::bytes / record_off --, 24 bytes a record,
 * so that the host can write <run>.bai without holding an uncompressed record (plo_bam_writer_index_add, portello_bam.h).
 *   refID >= 0   beg = max(pos, 0); rlen = the summed lengths of the ops M, D, N, =, X (codes 0, 2, 3, 7, 8) of the in-record CIGAR (64-bit;
 *                the placeholder <l_seq>S<ref_len>N of a record with more than 65 535 ops needs no special case, codes 9-15 consume
 *                nothing); end = beg + rlen, or beg + 1 when FLAG & 4 is set or rlen == 0
 *   refID == -1  beg = -1, end = 0, bin 4680
 * Checked on the device before a byte of a record is trusted, kinds in err_kind:
 *   1 .. 5  what plo_records_sort_dev checks, in its order: record_off, the 36 bytes, block_size, refID in [-1, n_ref), pos
 *   6       36 + l_read_name + 4 n_cigar_op > 4 + block_size: the CIGAR leaves the record
 *   7       end > 2^29: BAI cannot address it
 *   8       the pair (refID < 0 ? n_ref : refID, pos) is lower than the previous record's: the buffer is not coordinate sorted (the strand
 *           bit of plo_records_sort_dev's key is no part of the test)
 * A record reports the first kind it breaks in this order.  Any -> PLO_ERR_INVALID_ARG, err_record the LOWEST such record, err_kind what it
 * broke, no entries handed out, plo_last_error names both.  n_records == 0 -> PLO_OK; NULL bytes or record_off with n_records > 0 ->
 * PLO_ERR_INVALID_ARG; more than 2^27 - 1 records -> PLO_ERR_RANGE.
 * A wave takes a record: the ops are read a lane each, coalesced, and summed across the lanes.  One kernel, no LDS, ONE wait.  The input
 * and every other result on the context stay untouched; `entry` (24 n_records bytes, grown to the largest call) is valid until the
 * context's next plo_records_index_dev. */
typedef struct plo_index_entry {
    uint64_t off;                 /* record_off[i]: where the record's block_size stands in the buffer */
    int32_t ref_id;               /* -1: unplaced */
    int32_t beg, end;             /* 0-based half-open */
    uint32_t flags;               /* bit 0: FLAG & 4 (unmapped); bits 16..31: reg2bin(beg, end) */
} plo_index_entry;

typedef struct plo_index_in {
    const uint8_t *bytes;         /* device: coordinate-sorted records, each prefixed by its block_size (plo_sort_out::bytes) */
    uint64_t n_bytes;
    uint32_t n_records;
    const uint64_t *record_off;   /* device [n_records + 1] */
    uint32_t n_ref;               /* @SQ count of the output header */
} plo_index_in;

typedef struct plo_index_out {
    const plo_index_entry *entry; /* device [n_records], owned by the context until its next plo_records_index_dev */
    uint32_t n_records;
    uint32_t n_placed;            /* records with refID >= 0 */
    uint32_t err_record;          /* PLO_ERR_INVALID_ARG from the device check: lowest offending record, else UINT32_MAX */
    uint32_t err_kind;            /* what it broke (1 .. 8 above), else 0 */
    float index_ms;               /* HIP-event time of the call's kernel */
} plo_index_out;

plo_status plo_records_index_dev(plo_ctx *ctx, const plo_index_in *in, plo_index_out *out);

/* ---- Depth of the records (device-resident, opt-in; API version 19) ---------------------------------------------------------
 * How many records cover every reference base, taken from the records while they lie on the device (plo_records_out, plo_sort_out, a
 * merged chunk: any buffer of records with offsets) -- what `samtools depth` or `mosdepth` compute by reading the written file back.
 * The input need not be sorted.
 * THE OBJECT.  A depth object holds ONE int32 array for a list of chromosomes (n_ref, ref_len[], the output header's @SQ order).
 *   Chromosome r owns a slot of ref_len[r] + 1 entries; the last one takes the -1 of an interval that ends at the chromosome's end.
 *   Slots start at multiples of 64 entries: slot_off[0] = 0, slot_off[r + 1] = slot_off[r] + (ref_len[r] + 1 rounded up to 64).  The
 *   entries between the slots stay zero.  The array has slot_off[n_ref] entries: 4 x the sum of (ref_len + 1), rounded up per slot -- about
 *   12.4 GB for a human genome of 3.1 Gb -- plus the sums of the scan, 4 bytes per PLO_DEPTH_TILE (1024) entries.  plo_depth_info_get reports
 *   the bytes the object holds.
 * THE RULE.  A record is COUNTED iff refID >= 0, pos >= 0 and (FLAG & exclude_flags) == 0.  exclude_flags defaults to 0x704, the mask of
 * mosdepth and samtools depth: unmapped, secondary, QC-fail, duplicate.  Supplementary records count.
 *   Its ops are the record's REAL CIGAR: the in-record ops, or the ops of the record's first CG field when that is a B,I array and the
 *   in-record CIGAR is the placeholder <l_seq>S<n>N (what plo_batch_build_dev takes as a read's CIGAR).  A placeholder without such a
 *   field is taken as it stands, as htslib takes it: its N covers nothing.
 *   Walking the ops from pos: M, =, X cover their reference bases; D covers them iff count_deletions is set (set: mosdepth and
 *   `samtools depth -J`; clear, the default: `samtools depth`); N covers nothing and consumes reference; I, S, H, P and the codes 9-15
 *   consume nothing; ops of length 0 are ignored.  The depth at a base is the number of counted records that cover it.
 * CHECKED for every record of an add, counted or not, on the device, before a byte of it is trusted and before anything is added;
 * kinds in err_kind, a record reports the first kind it breaks in this order:
 *   1 .. 5  what plo_records_sort_dev checks, in its order: record_off, the 36 bytes, block_size, refID in [-1, n_ref), pos
 *   6       36 + l_read_name + 4 n_cigar_op > 4 + block_size: the in-record CIGAR leaves the record (the index call's rule)
 *   7       a record in placeholder form whose aux fields would begin behind its end, with a malformed aux field in front of its first
 *           CG, or whose first CG is an array that leaves the record
 *   8       a counted record whose reference end -- pos + the lengths of its M, D, N, =, X ops -- lies beyond ref_len[refID]
 * Any -> PLO_ERR_INVALID_ARG, err_record the LOWEST such record, err_kind what it broke, plo_last_error names both, and A REFUSED CALL ADDS
 * NOTHING: the add kernel reads the check's word first.
 * plo_depth_create allocates and zeroes the array on ctx's device (ctx only names the device and takes the error text).  opts NULL: the
 * defaults.  n_ref == 0 is allowed (an empty array); a negative ref_len -> PLO_ERR_INVALID_ARG.
 * plo_depth_add_dev runs on the CALLING context's stream with that context's scratch (8 bytes a record) and returns when its kernels are
 * through: a check (a wave per record) and the add (a wave per record: the ops a lane each, 64 a trip; a wave prefix sum of the reference
 * lengths gives every op its start, ballots find the ends of every maximal covered stretch, ONE int32 atomic add of device scope per end:
 * two a record for an = / X CIGAR without deletions).  The adds commute, so the array does not depend on the order of records, calls or
 * contexts, and adds from several contexts of the same device may overlap in time.  A context of another device -> PLO_ERR_INVALID_ARG;
 * more than 2^27 - 1 records in one call -> PLO_ERR_RANGE.
 * plo_depth_finish_dev turns the differences into depths in place: ONE inclusive 32-bit scan over the whole array (every slot's
 * differences sum to zero, so it equals a scan per chromosome) as tile sums, a scan of the sums, apply -- five launches, none of which
 * waits on another workgroup.
 * plo_depth_windows_dev: for a window size w >= 1 chromosome r has ceil(ref_len[r] / w) windows, the last one short; the uint64 sum of
 * depths of every window and the table win_first[n_ref + 1] come down in the call's one wait, as HOST arrays owned by the object until its
 * next windows call.  One launch.
 * plo_depth_runs_dev: the per-base bedGraph.  A run is a maximal stretch of equal depth within a chromosome, zero-depth runs included; runs
 * never cross a chromosome, a chromosome of length 0 has none; they are ordered by (ref_id, beg).  The runs stay on the DEVICE, owned by the
 * object until its next runs call (16 bytes a run).
 * plo_depth_reset zeroes the array and reopens the object.
 * ORDER.  The object is open (adds, then one finish) or finished (windows, runs).  An add or a finish on a finished object, windows or runs
 * on an open one -> PLO_ERR_INVALID_ARG.  finish, windows, runs, reset and destroy MUST NOT OVERLAP AN ADD on any context: that is the
 * caller's duty (join the adding threads first); the object does not lock.
 * plo_depth_info_get hands out the array and its entry count, so that a caller with several devices can sum the difference arrays of their
 * objects before the finish (the summing itself is the caller's). */
#define PLO_DEPTH_EXCLUDE_DEFAULT 0x704u

typedef struct plo_depth plo_depth;

typedef struct plo_depth_opts {
    uint32_t exclude_flags;       /* a record with any of these FLAG bits is not counted */
    int32_t count_deletions;      /* != 0: D covers its bases */
} plo_depth_opts;

typedef struct plo_depth_info {
    int32_t *array;               /* device [n_entries]: differences while the object is open, depths once it is finished */
    uint64_t n_entries;           /* slot_off[n_ref] */
    const uint64_t *slot_off;     /* HOST [n_ref + 1], owned by the object */
    uint64_t bytes_allocated;     /* device bytes the object holds now: the array, the scan's sums, its tables, windows and runs */
    uint32_t n_ref;
    uint32_t exclude_flags;
    int32_t count_deletions;
    int32_t finished;
} plo_depth_info;

typedef struct plo_depth_in {
    const uint8_t *bytes;         /* device: records, each prefixed by its block_size, in any order */
    uint64_t n_bytes;
    uint32_t n_records;
    const uint64_t *record_off;   /* device [n_records + 1] */
} plo_depth_in;

typedef struct plo_depth_add_out {
    uint32_t n_records;
    uint32_t n_counted;           /* records the rule counts */
    uint32_t err_record;          /* PLO_ERR_INVALID_ARG from the device check: lowest offending record, else UINT32_MAX */
    uint32_t err_kind;            /* what it broke (1 .. 8 above), else 0 */
    float add_ms;                 /* HIP-event time of the call's two kernels */
} plo_depth_add_out;

typedef struct plo_depth_windows_out {
    const uint64_t *sum;          /* HOST [n_windows]: the sum of the depths of every window */
    const uint64_t *win_first;    /* HOST [n_ref + 1]: the first window of every chromosome; [n_ref] = n_windows */
    uint64_t n_windows;
    float windows_ms;
} plo_depth_windows_out;

typedef struct plo_depth_run {
    int32_t ref_id;
    int32_t beg, end;             /* 0-based half-open */
    int32_t depth;
} plo_depth_run;

typedef struct plo_depth_runs_out {
    const plo_depth_run *run;     /* device [n_runs], ordered by (ref_id, beg) */
    uint64_t n_runs;
    float runs_ms;
} plo_depth_runs_out;

plo_status plo_depth_create(plo_ctx *ctx, uint32_t n_ref, const int32_t *ref_len, const plo_depth_opts *opts, plo_depth **out);
void plo_depth_destroy(plo_depth *depth);
plo_status plo_depth_info_get(const plo_depth *depth, plo_depth_info *info);
plo_status plo_depth_add_dev(plo_ctx *ctx, plo_depth *depth, const plo_depth_in *in, plo_depth_add_out *out);
plo_status plo_depth_finish_dev(plo_ctx *ctx, plo_depth *depth, float *finish_ms);
plo_status plo_depth_windows_dev(plo_ctx *ctx, plo_depth *depth, uint32_t window, plo_depth_windows_out *out);
plo_status plo_depth_runs_dev(plo_ctx *ctx, plo_depth *depth, plo_depth_runs_out *out);
plo_status plo_depth_reset(plo_ctx *ctx, plo_depth *depth);

/* ---- Allele pileup and candidate sites (device-resident, opt-in; API version 20) -------------------------------------------
 * Which reference bases carry non-reference evidence, taken from the records while they lie on the device (the inputs of plo_depth_add_dev)
 * against the calling context's reference -- the front of a small-variant caller, and the check that a lift put its reads in the right
 * place.  Only EVENTS are counted; the reference-matching count at a base is depth - (A + C + G + T + N).
 * THE OBJECT.  A pileup object holds ONE int32 array with PLO_PILEUP_CHANNELS = 8 counters per reference base; a base's 32 bytes are
 *   contiguous and 32-byte aligned:
 *     0 A, 1 C, 2 G, 3 T   a mismatching read base A, C, G, T          5 DEL   deletions that begin at this base
 *     4 N                  a mismatching read base of any other code   6 INS   insertions anchored at this base
 *                                                                      7 CLIP  soft clips anchored at this base
 *   It is created over a list of chromosomes (n_ref, ref_len[], the output header's @SQ order), like plo_depth_create, optionally with at
 *   most ONE region [beg, end) per chromosome.  No regions: every chromosome is covered whole.  With regions a chromosome without one has
 *   no bases in the object.  Chromosome r's slot holds slot_end[r] - slot_beg[r] bases and begins at base slot_off[r] of the array
 *   (slot_off counts in BASES; the counter of channel ch of base b is array[(slot_off[r] + b - slot_beg[r]) * 8 + ch]).  An event outside
 *   its chromosome's region is dropped silently: no error.  MEMORY: 32 bytes a base -- about 2 GB for chr20, about 99 GB for a whole genome
 *   of 3.1 Gb; the regions exist for this reason.
 *   plo_pileup_create -> PLO_ERR_INVALID_ARG for a negative ref_len, a region with ref_id outside [0, n_ref), with beg < 0, beg > end or
 *   end > ref_len[ref_id], and for two regions on one chromosome.  n_ref == 0 is allowed.  opts NULL: the defaults.
 * COUNTED RECORDS.  A record is counted iff refID >= 0, pos >= 0 and (FLAG & exclude_flags) == 0; exclude_flags defaults to 0x704, as for
 *   depth.  Its ops are the record's REAL CIGAR as defined for depth.  A counted record whose real CIGAR consumes no reference adds nothing.
 * WALKING THE OPS from pos, rf the reference position reached, rd the read position; ops of length 0 are ignored:
 *   M, =, X   every one of the L base pairs is classified by plo_nm_dev's pair rule: c1 the read's 4-bit code, c2 the reference byte's code
 *             in "=ACMGRSVTWYHKDBN" (any other byte: 15); the pair MATCHES iff c1 == 0, or c1 == c2 and c1 != 15.  The op's own code is
 *             not trusted: X over matching bases adds nothing, = over a mismatch adds.  A mismatching pair at reference base b adds 1 to
 *             [b][ch], ch = A, C, G, T for c1 = 1, 2, 4, 8 and N for every other c1.
 *   D         adds 1 to [rf][DEL]: only the first deleted base.
 *   I         adds 1 to [max(rf - 1, pos)][INS]: the VCF anchor -- the base in front, or the record's first base when none is in front.
 *   S         adds 1 to [max(rf - 1, pos)][CLIP]: a leading clip lands on the first aligned base, a trailing one on the last.
 *   N, H, P and the codes 9-15 add nothing.
 * CHECKED for every record of an add, on the device, before anything is added; a record reports the first kind it breaks:
 *   1 .. 8   exactly the kinds of plo_depth_add_dev, in its order
 *   9        the bases and qualities leave the record: 36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq > 4 + block_size
 *   10       a counted record whose real CIGAR's read length (M I S = X) differs from l_seq
 * Any -> PLO_ERR_INVALID_ARG, err_record the LOWEST such record, err_kind what it broke, and A REFUSED CALL ADDS NOTHING.
 * CONTEXT.  The reference is the CALLING context's index: refID r is chromosome r of its chrom_seq (what plo_records_build_dev writes).
 *   PLO_ERR_INVALID_ARG for an index without chrom_seq, an index whose chromosome count or lengths differ from the object's, and a context
 *   of another device; more than 2^27 - 1 records in a call -> PLO_ERR_RANGE.
 * plo_pileup_add_dev runs on the calling context's stream: a check and the add, a wave per record each.  The add takes the ops 64 a step,
 *   cuts the M / = / X ops at the 16-byte lines of the reference and issues ONE int32 atomic add of device scope per event.  n_events is the
 *   number of adds issued inside the regions.
 * plo_pileup_sites_dev lists the candidate sites.  With m the maximum of count[ch] over the channels in channel_mask, base b is a site iff
 *   m >= min_count, and depth == NULL or frac_num == 0 or m * frac_den >= frac_num * depth[b] (64-bit products; a depth of 0 passes).
 *   `depth` is a FINISHED depth object over the same n_ref / ref_len, or NULL (then every site's depth is -1).  opts NULL: the defaults
 *   (channel_mask 0x6F: A C G T DEL INS; min_count 1; frac_num 0).  PLO_ERR_INVALID_ARG for frac_den == 0 while frac_num != 0,
 *   min_count < 1, an open depth object, a depth object with another chromosome list.  The sites are ordered by (ref_id, pos) and stay on
 *   the DEVICE, owned by the object until its next sites call or reset (48 bytes a site); ref_base is the chrom_seq byte.
 * NO STATES: there is no finish step; the sum of n_events since the last reset equals the sum of the array.  Adds commute, and adds from
 *   several contexts of one device may overlap in time.  Sites, reset and destroy MUST NOT OVERLAP AN ADD: the caller's duty. */
#define PLO_PILEUP_CHANNELS 8
#define PLO_PILEUP_MASK_DEFAULT 0x6Fu

typedef struct plo_pileup plo_pileup;

typedef struct plo_pileup_region {
    int32_t ref_id;
    int32_t beg, end;             /* 0-based half-open */
} plo_pileup_region;

typedef struct plo_pileup_opts {
    uint32_t exclude_flags;       /* a record with any of these FLAG bits is not counted */
    uint32_t n_regions;           /* 0: every chromosome whole */
    const plo_pileup_region *regions;
} plo_pileup_opts;

typedef struct plo_pileup_info {
    int32_t *array;               /* device [n_bases * 8] */
    uint64_t n_bases;             /* slot_off[n_ref] */
    const uint64_t *slot_off;     /* HOST [n_ref + 1], in bases, owned by the object */
    const int32_t *slot_beg;      /* HOST [n_ref] */
    const int32_t *slot_end;      /* HOST [n_ref] */
    uint64_t bytes_allocated;     /* device bytes the object holds now: the array, its tables, the sites and their scan */
    uint32_t n_ref;
    uint32_t exclude_flags;
} plo_pileup_info;

typedef struct plo_pileup_add_out {
    uint32_t n_records;
    uint32_t n_counted;           /* records the rule counts */
    uint32_t err_record;          /* PLO_ERR_INVALID_ARG from the device check: lowest offending record, else UINT32_MAX */
    uint32_t err_kind;            /* what it broke (1 .. 10 above), else 0 */
    uint64_t n_events;            /* adds issued inside the regions */
    float add_ms;                 /* HIP-event time of the call's two kernels */
} plo_pileup_add_out;

typedef struct plo_pileup_sites_opts {
    uint32_t channel_mask;        /* bit ch: channel ch takes part in the maximum */
    int32_t min_count;            /* >= 1 */
    uint32_t frac_num, frac_den;  /* frac_num == 0: no fraction test */
} plo_pileup_sites_opts;

typedef struct plo_pileup_site {
    int32_t ref_id;
    int32_t pos;                  /* 0-based */
    int32_t depth;                /* -1 without a depth object */
    uint8_t ref_base;
    uint8_t pad[3];
    int32_t count[PLO_PILEUP_CHANNELS];
} plo_pileup_site;

typedef struct plo_pileup_sites_out {
    const plo_pileup_site *site;  /* device [n_sites], ordered by (ref_id, pos) */
    uint64_t n_sites;
    float sites_ms;
} plo_pileup_sites_out;

plo_status plo_pileup_create(plo_ctx *ctx, uint32_t n_ref, const int32_t *ref_len, const plo_pileup_opts *opts, plo_pileup **out);
void plo_pileup_destroy(plo_pileup *pileup);
plo_status plo_pileup_info_get(const plo_pileup *pileup, plo_pileup_info *info);
plo_status plo_pileup_reset(plo_ctx *ctx, plo_pileup *pileup);
/* in: plo_depth_in's shape and meaning */
plo_status plo_pileup_add_dev(plo_ctx *ctx, plo_pileup *pileup, const plo_depth_in *in, plo_pileup_add_out *out);
plo_status plo_pileup_sites_dev(plo_ctx *ctx, plo_pileup *pileup, const plo_depth *depth, const plo_pileup_sites_opts *opts, plo_pileup_sites_out *out);

/* ---- Sorted windows merged into large runs (device-resident, opt-in; API version 18) --------------------------------------
 * A k-way merge of coordinate-sorted record buffers -- typically copies of plo_sort_out::bytes / record_off of several windows -- that each
 * lie in an allocation of their own: a plan, then an emit per chunk of the merged stream, on one context.
 * The order is plo_records_sort_dev's.  Number the records run-major, g = run_first[r] + place; the merged order is the pair (key, g) with
 * that call's key.  The pair is unique, so the result is fully determined; it is what plo_records_sort_dev gives over the runs'
 * concatenation, byte for byte, and what plo_bam_merge_runs gives over the same runs as files, record for record.
 * plo_runs_merge_plan_dev.  Checked on the device before a byte of a record is trusted, per run, kinds in err_kind:
 *   1 .. 5  what plo_records_sort_dev checks, in its order, against the run's own record_off and n_bytes: record_off[0] == 0, not
 *           decreasing, ends at n_bytes; the 36 bytes; block_size; refID in [-1, n_ref); pos
 *   6       the record's key is lower than the key of the record before it in the same run: the run is not sorted
 * Any -> PLO_ERR_INVALID_ARG: err_run / err_record (the place in that run) name the LOWEST g that breaks something, err_kind the first kind
 * it breaks; no result is handed out, plo_last_error names all three.  n_runs == 0 or no record at all -> PLO_OK with empty outputs
 * (record_off[0] == 0, n_chunks == 0).  n_runs > PLO_MERGE_MAX_RUNS, chunk_bytes == 0, a NULL `runs` with n_runs > 0, a run with records
 * and a NULL pointer, or a run without records and n_bytes != 0 -> PLO_ERR_INVALID_ARG; more than 2^32 - 2 records in all -> PLO_ERR_RANGE.
 * A run may be empty, and its pointers may then be NULL.
 * Chunks: chunk c begins at merged record chunk_first[c] and holds as many following records as keep its bytes <= chunk_bytes, but never
 * fewer than one.  The table is made on the device and copied down in the call's ONE wait; chunk_first and chunk_off are HOST arrays.
 * Kernels: keys (a thread per record), a rank launch per doubling of the groups of runs (ceil(log2(n_runs)) of them), gather, the 64-bit
 * scan (3), chunks (one lane).  Buffers, the call's own, grown to the largest plan and freed with the context: 50 n_records + 8 bytes,
 * the descriptor table and the chunk table; no record byte is moved.
 * plo_runs_merge_emit_dev copies the records of chunk `chunk` of the context's current plan, in merged order, into a buffer of the call's own
 * (grown to the largest chunk) and hands out record_off rebased to the chunk: the shapes plo_records_index_dev and plo_bgzf_compress_dev
 * take.  One launch, one wait: a wave per 16 KB of the chunk finds the records that reach into its piece and reads each from
 * runs[r].bytes + runs[r].record_off[place]; every output byte is stored exactly once.  PLO_ERR_INVALID_ARG without a plan (none yet, the
 * last one refused) or for chunk >= n_chunks.
 * Two rules.  The runs -- bytes and record_off -- must stay valid and unchanged from the plan to the last emit.  A chunk is valid until the
 * context's next emit; the plan's outputs until the context's next plan.  The inputs and every other result on the context stay untouched. */
#define PLO_MERGE_MAX_RUNS 4096

typedef struct plo_merge_run {
    const uint8_t *bytes;         /* device: the run's records in coordinate order, each prefixed by its block_size */
    uint64_t n_bytes;
    uint32_t n_records;
    const uint64_t *record_off;   /* device [n_records + 1], counted from the run's own `bytes` */
} plo_merge_run;

typedef struct plo_merge_in {
    const plo_merge_run *runs;    /* HOST [n_runs] */
    uint32_t n_runs;
    uint32_t n_ref;               /* @SQ count of the output header */
    uint64_t chunk_bytes;         /* the most bytes of a chunk that holds more than one record */
} plo_merge_in;

typedef struct plo_merge_out {
    uint32_t n_records;
    uint32_t n_mapped;            /* records with refID >= 0; the refID -1 tail begins at this merged position */
    uint64_t n_bytes;
    const uint32_t *src;          /* device [n_records]: merged position j holds record g = src[j] */
    const uint64_t *key;          /* device [n_records]: the merged keys */
    const uint64_t *record_off;   /* device [n_records + 1], of the merged stream */
    uint32_t n_chunks;
    const uint32_t *chunk_first;  /* HOST [n_chunks + 1]: chunk c is the merged records [chunk_first[c], chunk_first[c + 1]) */
    const uint64_t *chunk_off;    /* HOST [n_chunks + 1]: record_off[chunk_first[c]] */
    uint32_t err_run;             /* PLO_ERR_INVALID_ARG from the device check: the run of the lowest offending g, else UINT32_MAX */
    uint32_t err_record;          /* its place in that run, else UINT32_MAX */
    uint32_t err_kind;            /* what it broke (1 .. 6 above), else 0 */
    float plan_ms;                /* HIP-event time of the call's kernels */
} plo_merge_out;

typedef struct plo_merge_chunk_out {
    const uint8_t *bytes;         /* device: the chunk's records in merged order, densely packed */
    uint64_t n_bytes;
    uint32_t n_records;
    uint32_t first_record;        /* chunk_first[chunk] */
    const uint64_t *record_off;   /* device [n_records + 1], counted from the chunk's first byte */
    float emit_ms;                /* HIP-event time of the call's kernel */
} plo_merge_chunk_out;

plo_status plo_runs_merge_plan_dev(plo_ctx *ctx, const plo_merge_in *in, plo_merge_out *out);
plo_status plo_runs_merge_emit_dev(plo_ctx *ctx, uint32_t chunk, plo_merge_chunk_out *out);

/* ---- The liftover batch (device-resident) ------------------------------------------------------------------------
 * Builds the plo_batch_in / plo_finish_in of a window from its records as they stand in device memory: what plo_bam_window_batch_raw
 * (portello_bam.h) builds on the host, array for array -- the sequencing-order split segments of every primary record
 * (get_seq_order_read_split_segments, split_read.rs:56-155): the CG:B,I restore of a long CIGAR, the first SA:Z field cut at ';' and ','
 * with split_terminator's rules (sa_tag_parser.rs:26-59), the clip positions, the stable sort by sequencing-order start, the labels looked
 * up in the @SQ names given here (a hash table built on the device on every call).  batch.seq = fin.qual = records; read_seq_off /
 * read_qual_off are byte offsets into it; seq_fmt = PLO_SEQ_BAM4; n_items = 0 (the engine enumerates).
 * Every record is checked before any of its bytes is trusted: a read_rec_off, block_size, l_qname / n_cigar / l_seq that points outside
 * `records` -> PLO_ERR_INVALID_ARG.  Input the host batcher refuses -> PLO_ERR_DATA: err_read is the LOWEST failing read, err_kind its
 * first failure in the host's order (segments in text order; per segment field count, field parse, no aligned op, read size, unknown label;
 * then an empty split segment), and plo_last_error names both.  More than 2^31 - 1 CIGAR ops in the window -> PLO_ERR_RANGE.  A failing
 * call leaves nothing the caller may use.  n_reads == 0: PLO_OK with empty arrays.
 * The stream is waited for once for the totals and the error word, and once behind the emit kernel for the event times.  The call uses
 * buffers of its own, grown to the largest call and freed with the context: its outputs stay valid across the following lift / compact /
 * finish / SA / records / bgzf calls on the context, until its next plo_batch_build_dev.  All pointers are device pointers. */
typedef enum plo_bb_err {
    PLO_BB_ERR_NONE = 0,
    PLO_BB_ERR_SA_NOT_Z = 1,       /* the SA aux field is not a string                                        */
    PLO_BB_ERR_FIELD_COUNT = 2,    /* an SA segment without exactly six fields (an empty one included)        */
    PLO_BB_ERR_MALFORMED = 3,      /* pos / CIGAR / MAPQ / NM of an SA segment does not parse                 */
    PLO_BB_ERR_UNALIGNED = 4,      /* an SA segment whose CIGAR has no M, = or X op                           */
    PLO_BB_ERR_READ_SIZE = 5,      /* an SA segment's read length differs from the primary record's           */
    PLO_BB_ERR_UNKNOWN_CONTIG = 6, /* an SA segment on a contig the header does not name                      */
    PLO_BB_ERR_EMPTY_SEGMENT = 7   /* a segment that covers no read base in sequencing order                  */
} plo_bb_err;

typedef struct plo_batch_build_in {
    const uint8_t *records;          /* the window's stretch of the BAM stream                                          */
    uint64_t records_bytes;
    const uint64_t *read_rec_off;    /* [n_reads] offset of primary record r's block_size word inside `records`         */
    uint32_t n_reads;
    uint32_t n_contigs;              /* @SQ names of the read->contig BAM                                               */
    const uint32_t *contig_name_off; /* [n_contigs + 1] byte offsets into contig_names                                  */
    const uint8_t *contig_names;     /* concatenated labels, no terminators                                             */
} plo_batch_build_in;

typedef struct plo_batch_build_out {
    plo_batch_in batch;  /* device pointers owned by the context; seq = records, seq_fmt = PLO_SEQ_BAM4, n_items = 0 */
    plo_finish_in fin;   /* qual = records                                                                           */
    uint32_t err_read;   /* lowest failing read, UINT32_MAX if none                                                  */
    uint32_t err_kind;   /* PLO_BB_ERR_*                                                                             */
    float batch_ms;      /* HIP-event time of the call's kernels                                                     */
} plo_batch_build_out;

plo_status plo_batch_build_dev(plo_ctx *ctx, const plo_batch_build_in *in, plo_batch_build_out *out);

/* ---- The input BAM stream (device-resident) ------------------------------------------------------------------------
 * plo_bgzf_inflate_dev: the public, device-resident form of the reader's device inflate.  `bgzf` (HOST memory, pageable or page-locked)
 * holds BGZF blocks from a block boundary on.  The headers are walked on the host with the reader's rules (gzip magic with FEXTRA, the
 * `BC` subfield, BSIZE, the ISIZE trailer; ISIZE above 65536 is refused); every WHOLE block whose inflated bytes still fit in `dst` is
 * taken, uploaded, inflated (k_bgzf_inflate) and checked against its CRC-32 (k_bgzf_crc) on the context's stream, and the inflated
 * bytes are left packed at dst[0, n_bytes).  Nothing inflated is copied to the host.  A trailing partial block (fewer than 28 bytes
 * left, or fewer than BSIZE) and the blocks from the first one that no longer fits are not consumed: bgzf_consumed says where to go on.
 * A block with ISIZE 0 (the EOF block, wherever it stands) is consumed and adds nothing.  Bytes at a block boundary that are no BGZF
 * header -> PLO_ERR_IO; a block that does not decode or fails its CRC -> PLO_ERR_IO, plo_last_error names the block's offset inside
 * `bgzf` (the contents of dst are undefined then).  bgzf_bytes == 0: PLO_OK with nothing consumed.  The call returns when its kernels are
 * through.  `dst` is a device buffer of the caller's; the compressed bytes are staged in a buffer the context owns. */
typedef struct plo_bgzf_inflate_in {
    const uint8_t *bgzf; /* host */
    uint64_t bgzf_bytes;
    uint8_t *dst;        /* device */
    uint64_t dst_cap;
} plo_bgzf_inflate_in;

typedef struct plo_bgzf_inflate_out {
    uint32_t n_blocks;      /* blocks consumed (those with ISIZE 0 included)            */
    uint64_t bgzf_consumed; /* compressed bytes consumed: the next call's `bgzf` starts there */
    uint64_t n_bytes;       /* inflated bytes at dst                                     */
    float inflate_ms;       /* HIP-event time: upload, both kernels, the status download */
} plo_bgzf_inflate_out;

plo_status plo_bgzf_inflate_dev(plo_ctx *ctx, const plo_bgzf_inflate_in *in, plo_bgzf_inflate_out *out);

/* plo_window_cut_dev: the record walk and the window cut of plo_bam_read_window (portello_bam.h) over stream[0, stream_bytes), a stretch of
 * the inflated BAM stream in device memory that begins at a record boundary.  Record by record in stream order, exactly the host's loop:
 *   - in front of every record, in this order: n_reads == max_records -> the window ends (PLO_CUT_MAX_RECORDS); n_unmapped >= max_unmapped
 *     -> PLO_CUT_MAX_UNMAPPED; the record's offset >= max_bytes and at least one primary or unmapped record taken -> PLO_CUT_MAX_BYTES;
 *   - then the record: no byte left -> PLO_CUT_EOF with final != 0, PLO_CUT_END_OF_BYTES otherwise; fewer than 4 bytes left or fewer than
 *     4 + block_size -> with final == 0 the window ends IN FRONT of it with PLO_CUT_END_OF_BYTES (add bytes and cut again from the same
 *     start), with final != 0 PLO_ERR_IO ("truncated BAM record"); block_size < 32 -> PLO_ERR_IO (this test comes before the one against
 *     the bytes left, as on the host); fixed fields + name + CIGAR + bases + qualities beyond block_size -> PLO_ERR_IO; flag 0x4 with
 *     tid >= 0 -> PLO_ERR_DATA; flag 0x4 -> an unmapped record; flag 0x800 -> skipped; anything else -> a primary read.
 * On an error err_off is the offset of the FIRST offending record and nothing else of `out` may be used.  A bad record behind the point
 * where the window ends does not fail this window: it fails the window it belongs to.
 * max_unmapped / max_bytes == 0: the host's rule, 4 x max_records + 1024 and max(1 GB, min(8 GB, max_records << 16)).  max_records == 0 ->
 * PLO_ERR_INVALID_ARG.  stream_bytes == 0: PLO_OK with zero records, PLO_CUT_EOF when final != 0, PLO_CUT_END_OF_BYTES otherwise.
 * Every block_size is checked against stream_bytes before a byte behind it is read: nothing outside [stream, stream + stream_bytes) is read.
 * The stretch is walked in segments of PLO_CUT_SEG_BYTES from guessed record boundaries (window_core.hpp); the guesses are hints, the
 * result is the serial walk's whatever they are.  The stream is waited for once for the counts that size the outputs and once behind the
 * emit kernels.  All pointers are device pointers; outputs are owned by the context and valid until its next plo_window_cut_dev. */
#define PLO_CUT_SEG_BYTES 32768u
typedef enum plo_cut_end {
    PLO_CUT_MAX_RECORDS = 0,
    PLO_CUT_MAX_UNMAPPED = 1,
    PLO_CUT_MAX_BYTES = 2,
    PLO_CUT_END_OF_BYTES = 3, /* final == 0: the bytes ended (in front of a record, or inside the one at window_bytes) */
    PLO_CUT_EOF = 4,          /* final != 0 and the walk ended exactly at stream_bytes                                  */
    PLO_CUT_PART_END = 5      /* plo_window_cut_part_dev: the record at window_bytes starts at or behind own_bytes      */
} plo_cut_end;

typedef struct plo_window_cut_in {
    const uint8_t *stream;
    uint64_t stream_bytes;
    uint32_t max_records;
    uint64_t max_unmapped; /* 0: 4 x max_records + 1024                         */
    uint64_t max_bytes;    /* 0: max(1 GB, min(8 GB, max_records << 16))         */
    int32_t final;         /* nothing follows these bytes                        */
} plo_window_cut_in;

typedef struct plo_window_cut_out {
    uint32_t n_reads;
    const uint64_t *read_rec_off; /* [n_reads] offsets of the primary records' block_size words: what plo_batch_build_in / plo_records_in take */
    uint32_t n_unmapped;
    const uint64_t *unmapped_off; /* [n_unmapped + 1] offsets inside `unmapped`                                                */
    const uint8_t *unmapped;      /* the unmapped records side by side in stream order, each with its block_size word: the bytes
                                     plo_bam_window_unmapped returns                                                            */
    uint64_t unmapped_bytes;
    uint64_t window_bytes;        /* the stretch the window consumes; the next window starts there                              */
    int32_t ended_by;             /* plo_cut_end                                                                                */
    uint64_t err_off;             /* PLO_ERR_IO / PLO_ERR_DATA: offset of the first offending record, UINT64_MAX otherwise       */
    float cut_ms;                 /* HIP-event time of the call's kernels                                                       */
    uint32_t n_rewalks;           /* segments walked again because their guessed start was not the true one (a diagnostic)      */
} plo_window_cut_out;

plo_status plo_window_cut_dev(plo_ctx *ctx, const plo_window_cut_in *in, plo_window_cut_out *out);

/* ---- One PART of a BAM file on the device (API version 11) ----------------------------------------------------------
 * The rule is plo_bam_open_range's (portello_bam.h): the compressed file is cut at size x part / n_parts, a part owns the records whose
 * first byte lies in a BGZF block that STARTS inside its stretch [lo, hi), and reads on past hi to finish the last of them.
 *
 * plo_bgzf_inflate_part_dev: plo_bgzf_inflate_dev for a reader that knows where `bgzf` lies in its file (bgzf_file_off: the file offset
 * of bgzf[0]) and where its part ends (range_end: the part's hi, UINT64_MAX = no end).  Same blocks, same bytes, same errors; in addition
 * own_bytes: the offset inside dst of the first consumed block whose file offset is >= range_end, n_bytes when there is none.  (A block
 * with ISIZE 0 holds no byte: a byte belongs to the last block that starts at or before it, so an empty block at the border changes
 * nothing.)  Host arithmetic in the header walk; the kernels are plo_bgzf_inflate_dev's. */
typedef struct plo_bgzf_inflate_part_in {
    const uint8_t *bgzf; /* host */
    uint64_t bgzf_bytes;
    uint8_t *dst;        /* device */
    uint64_t dst_cap;
    uint64_t bgzf_file_off;
    uint64_t range_end;
} plo_bgzf_inflate_part_in;

typedef struct plo_bgzf_inflate_part_out {
    uint32_t n_blocks;
    uint64_t bgzf_consumed;
    uint64_t n_bytes;
    float inflate_ms;
    uint64_t own_bytes; /* records that start at dst + own_bytes or behind it are the next part's */
} plo_bgzf_inflate_part_out;

plo_status plo_bgzf_inflate_part_dev(plo_ctx *ctx, const plo_bgzf_inflate_part_in *in, plo_bgzf_inflate_part_out *out);

/* plo_window_cut_part_dev: plo_window_cut_dev with the host's range test in front of every record, where plo_bam_read_window has it:
 * behind the three stop tests and the tests for "no byte left" and "fewer than 4 bytes left", in front of block_size < 32.  A record whose
 * offset is >= own_bytes ends the window in front of it with PLO_CUT_PART_END (the host's eof of a part): whatever stands there or behind
 * it, a refused record included, never fails this call.  own_bytes == UINT64_MAX: plo_window_cut_dev.  own_bytes counts from `stream`:
 * a reader that cuts window after window moves it with the stream. */
typedef struct plo_window_cut_part_in {
    const uint8_t *stream;
    uint64_t stream_bytes;
    uint32_t max_records;
    uint64_t max_unmapped;
    uint64_t max_bytes;
    int32_t final;
    uint64_t own_bytes;
} plo_window_cut_part_in;

plo_status plo_window_cut_part_dev(plo_ctx *ctx, const plo_window_cut_part_in *in, plo_window_cut_out *out);

/* plo_part_start_dev: where the first record of a part behind the first starts.  stream[0, stream_bytes) (device memory) begins at the
 * first inflated byte of the part's first BGZF block, usually inside a record; n_ref is the header's reference count; final != 0 says that
 * nothing follows these bytes.  The result is the host's (plo_bam_open_range) over the same bytes.  Every offset p with
 * p + 36 <= stream_bytes is one of
 *   accept: eight records follow each other from p, each of them plausible (block_size >= 32 and within the bytes, reference ids in
 *           [-1, n_ref), a NUL-terminated name of at least one byte, fixed fields + name + CIGAR + bases + qualities within block_size,
 *           CIGAR op codes 0 .. 8) -- or at least one does and the chain ends exactly at stream_bytes with final != 0;
 *   cut:    at least one plausible record, then the bytes end inside a record or in front of one, with final == 0;
 *   reject: anything else.
 * The lowest p that is no reject decides: accept -> PLO_PART_FOUND with first_off = p; cut -> PLO_PART_NEED_MORE (call again from the
 * same start with more bytes); none -> PLO_PART_NONE (with final != 0 and little data the stretch is the tail of one record: the part is
 * empty; otherwise the host reports PLO_ERR_DATA).  Every block_size is compared with the bytes left before anything behind it is read. */
typedef enum plo_part_kind { PLO_PART_FOUND = 0, PLO_PART_NEED_MORE = 1, PLO_PART_NONE = 2 } plo_part_kind;

typedef struct plo_part_start_in {
    const uint8_t *stream;
    uint64_t stream_bytes;
    uint32_t n_ref;
    int32_t final;
} plo_part_start_in;

typedef struct plo_part_start_out {
    int32_t kind;       /* plo_part_kind                                  */
    uint64_t first_off; /* PLO_PART_FOUND: the first record's offset, UINT64_MAX otherwise */
    float start_ms;     /* HIP-event time of the kernel                    */
} plo_part_start_out;

plo_status plo_part_start_dev(plo_ctx *ctx, const plo_part_start_in *in, plo_part_start_out *out);

/* (plo_finish_batch_dev returns PLO_ERR_DATA when an item of the batch ended LEN_MISMATCH or PANIC -- the reference aborts
   there, :207-229 -- and leaves is_target_region handling (:318-320: no unmapped copy) to the caller.)

   Packs the output CIGARs of the last plo_liftover_batch_dev result densely (items in order, no gaps): the kernels
   allocate them in per-wave slabs, so plo_batch_out.cigar spans up to 16 Ki unused ops per resident wave.  Rewrites
   item_cigar_off, cigar and n_cigar of `out` (and what plo_finish_batch_dev / plo_sa_segments_dev will read).  Worth it
   before the arrays leave the device (plo_liftover_batch does it itself before its device-to-host copy). */
/* Like the kernels of plo_liftover_batch_dev it completes on the context's stream, not at return: order consumers on that
   stream (or call plo_ctx_sync). */
plo_status plo_compact_output_dev(plo_ctx *ctx, plo_batch_out *out);

/* ------------------------------------------------------------------------------------------------------------
 * The record gather of several GPUs (one process per GPU; SURVEY.md 8(e), INTEGRATION.md section 6 route (b)): the reference's sink is
 * one locked writer behind all workers (src/read_alignment_scanner.rs:24, :483) -- here rank `root` receives every rank's result
 * arrays over RCCL: a 16-byte size all-gather, then ONE group of ncclSend (peers) / ncclRecv (root) per array, device memory to device
 * memory (xGMI is point to point: every peer's link runs into the root at once).  RCCL is bound by name at the first call.
 *   rank 0:      plo_gather_unique_id(id); hand `id` to the other ranks (a file, a socket, MPI, torch.distributed ...)
 *   every rank:  plo_gather_create(id, rank, world, device, &g);
 *   per batch:   plo_liftover_batch_dev(ctx, ..., &out); plo_compact_output_dev(ctx, &out);
 *                plo_gather_records(g, ctx, &out, root, gathered = an array of `world` structs on root, NULL elsewhere); ... plo_gather_wait(g);
 * plo_gather_records returns when the exchange is posted on the context's stream (behind the compaction); the sizes in `gathered` are
 * valid at once, the arrays after plo_gather_wait (or any synchronisation of that stream).  gathered[root] points at the rank's own
 * arrays, the others at buffers the gather object owns until its next call.  A context must not start its next batch before the
 * exchange that reads its buffers is through (two contexts taking turns hide the exchange under the next batch's kernels).
 * ---------------------------------------------------------------------------------------------------------- */
#define PLO_GATHER_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */
typedef struct plo_gather plo_gather;
plo_status plo_gather_unique_id(uint8_t id[PLO_GATHER_ID_BYTES]);
plo_status plo_gather_create(const uint8_t id[PLO_GATHER_ID_BYTES], int rank, int world, int device, plo_gather **out);
void plo_gather_destroy(plo_gather *g);
plo_status plo_gather_records(plo_gather *g, plo_ctx *ctx, const plo_batch_out *out, int root, plo_batch_out *gathered);
plo_status plo_gather_wait(plo_gather *g);
const char *plo_gather_last_error(const plo_gather *g); /* g == NULL: the calling thread's last plo_gather_unique_id / _create failure */
/* the HIP stream and device ordinal a context runs on (what a caller orders its own work behind / selects before its own HIP calls) */
void *plo_ctx_stream(plo_ctx *ctx);
int plo_ctx_device(plo_ctx *ctx);

/* Page-locked host memory for the arrays handed to plo_liftover_batch: copies from such buffers are direct DMA transfers
   (measured on MI355X, chr20 batch of 50 k reads / 385 MB: pageable 14 GB/s, page-locked see DESIGN.md).  The caller fills
   them in place (e.g. one set per worker thread, reused from batch to batch) and releases them with plo_host_free. */
plo_status plo_host_alloc(size_t bytes, void **out);
void plo_host_free(void *p);

plo_status plo_ctx_sync(plo_ctx *ctx);
/* Copies `bytes` from device memory (e.g. a plo_liftover_batch_dev output array) to host memory on the context's
   stream and waits for it. */
plo_status plo_ctx_download(plo_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
plo_status plo_ctx_timing(plo_ctx *ctx, plo_timing *out);
const char *plo_last_error(const plo_ctx *ctx);
const char *plo_version(void);
/* PLO_API_VERSION the library was built with */
uint32_t plo_api_version(void);
/* Device self-test of the wavefront primitives (DPP scans, cross-lane reads): 0 = ok. */
int plo_selftest(int device);

/* ------------------------------------------------------------------------------------------------------------
 * The reference FASTA on the device (API 17): what get_chrom_array (src/main.rs:24-62) and get_genome_ref_from_fasta
 * (lib/rust-vc-utils/src/genome_ref.rs:43-80) do on the host -- one upper-cased ASCII array per chromosome, in the order of the
 * assembly->reference header, checked against its lengths -- as a stream compaction in HBM.  Plain text only, as the reference.
 *
 * THE RULE (this project's own: the FASTA crate the reference parses with is not pinned here; for well-formed files the rule gives
 * what the crate documents -- a record per '>' line, id = first white-space-delimited token, sequence lines joined without their
 * trailing white space, then to_ascii_uppercase):
 *   Lines end at '\n'; the last line may lack it.
 *   A line whose first byte is '>' is a header line.  Its id is the bytes behind '>' up to the first space, tab, '\r' or the line end; an
 *   id may be empty; the rest of the line is ignored, whatever it holds.
 *   Every other line is a sequence line of the record the last header line opened: '\n', '\r', space and tab are dropped, A-Z is kept,
 *   a-z is stored upper-cased, and EVERY other byte is refused -- a '>' that is not the first byte of its line, a digit, '*', '-', a
 *   control byte, a byte >= 0x80.  A base in front of the first header line is refused; dropped bytes there are allowed.  An empty file
 *   gives zero records; a header line directly followed by another gives a record of length 0.
 *   Wanted chromosomes: names and lengths in the order the caller wants them (plo_phase1_info's ref_names / ref_lens).  Records whose id
 *   is not wanted are skipped and never stored (their bytes are still checked).  Without a list every record is kept, in file order.
 * REFUSALS: PLO_ERR_DATA from plo_fasta_finish, which reports the first of the following (a refused byte also from the feed call that
 *   meets it and from every feed call behind it):
 *   1. the lowest refused byte of the text: PLO_FA_ERR_BAD_BYTE or PLO_FA_ERR_NO_HEADER, err_offset = its file offset (found on the
 *      device by an atomic min, so it does not depend on which wave saw which byte);
 *   2. else PLO_FA_ERR_DUPLICATE: a wanted id on a second header line -- err_offset = the offset of the lowest such line, err_chrom = its
 *      place in the list, err_len = the first copy's length.  A DELIBERATE DIFFERENCE: the reference's HashMap::insert
 *      (genome_ref.rs:51-53) silently keeps the last copy; samtools faidx refuses, and so does this loader;
 *   3. else the lowest place in the list that is PLO_FA_ERR_MISSING (never seen) or PLO_FA_ERR_LENGTH (err_len = the length found,
 *      err_offset = its header line; a record longer than wanted stores nothing outside its slot and is counted to its end).
 *   A refused load hands out no sequence: n_chroms = 0, chrom_seq = NULL.
 * OUTPUT: one device allocation the object owns.  Chromosome c starts at a 256-byte-aligned offset of it (plo_index_create gives its own
 *   copies a hipMalloc each), a slot has at least 16 bytes, the gaps and the tail are zero.
 * The result depends on the bytes alone: not on where the pieces are cut, nor on any launch geometry.
 * The loader exists before any index does, so it is an object of its own on a device with a private stream and its own workspaces.  An
 * index created from its pointers (seq_mem = PLO_MEM_DEVICE) BORROWS them: destroy the index first, the plo_fasta after it.
 * ---------------------------------------------------------------------------------------------------------- */
enum { PLO_FA_ERR_NONE = 0, PLO_FA_ERR_BAD_BYTE = 1, PLO_FA_ERR_NO_HEADER = 2, PLO_FA_ERR_MISSING = 3, PLO_FA_ERR_LENGTH = 4, PLO_FA_ERR_DUPLICATE = 5 };

typedef struct plo_fasta plo_fasta;

typedef struct plo_fasta_want {
    uint32_t n;
    const char *const *names; /* [n] NUL-terminated, no name twice */
    const int64_t *lens;      /* [n] */
} plo_fasta_want;

typedef struct plo_fasta_out {
    uint32_t n_chroms;               /* the wanted list's, or without one the records seen                                   */
    const int64_t *chrom_len;        /* [n_chroms] host memory of the object                                                  */
    const uint8_t *const *chrom_seq; /* [n_chroms] host array of DEVICE pointers: plo_index_desc::chrom_seq with PLO_MEM_DEVICE */
    uint64_t n_records_seen;         /* header lines of the text, wanted or not                                               */
    uint64_t n_bases;                /* bases of the text, stored or not                                                      */
    uint64_t text_bytes;
    float fasta_ms;                  /* HIP-event time of the kernels of all pieces, summed                                   */
    int32_t err_kind;                /* PLO_FA_ERR_*                                                                          */
    uint64_t err_offset;
    uint32_t err_chrom;
    int64_t err_len;
} plo_fasta_out;

/* want == NULL: keep every record.  text_bytes_hint: the size of the text when known (sizes the first output allocation of a load
   without a list, which grows when it has to), 0 otherwise. */
plo_status plo_fasta_create(const plo_fasta_want *want, uint64_t text_bytes_hint, int device, plo_fasta **out);
/* The text as consecutive pieces of any size, 0 included, in host memory (page-locked memory is copied by DMA).  Returns once `text` has
   been read; kernels of the piece may still run on the object's stream. */
plo_status plo_fasta_feed(plo_fasta *f, const uint8_t *text, uint64_t n_bytes);
/* The end of the text.  Waits for the stream.  The pointers in `out` stay valid until plo_fasta_destroy. */
plo_status plo_fasta_finish(plo_fasta *f, plo_fasta_out *out);
/* Record i of the text in file order (i < n_records_seen, valid after plo_fasta_finish, refused loads included): its id (owned by the
   object), its length, and its place in the wanted list (-1: not wanted; without a list: i). */
plo_status plo_fasta_record(const plo_fasta *f, uint64_t i, const char **id, int64_t *len, int32_t *want_index);
/* Copies n host sequences into device memory the object owns; host_seq[i] == NULL stays NULL.  For plo_index_desc::rev_contig_seq, which
   seq_mem covers together with chrom_seq: with device chromosomes the reverse contigs have to be device pointers too. */
plo_status plo_fasta_adopt(plo_fasta *f, uint32_t n, const uint8_t *const *host_seq, const int64_t *len, const uint8_t **dev_out);
/* Copies `bytes` from device memory of the object (a chromosome, an adopted sequence) to host memory on its stream and waits. */
plo_status plo_fasta_download(plo_fasta *f, void *host_dst, const void *dev_src, size_t bytes);
void plo_fasta_destroy(plo_fasta *f);
const char *plo_fasta_last_error(const plo_fasta *f); /* f == NULL: the calling thread's last plo_fasta_create failure */

#ifdef __cplusplus
}
#endif
#endif /* PORTELLO_LIFTOVER_H */
