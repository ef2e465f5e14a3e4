// engine.hip -- gfx950 kernels + the C ABI of include/portello_liftover.h.
//
// Kernel pipeline of one batch (all on the context's stream):
//   k_seg_count          two lanes per read split segment, 16 ops per lane and step: batch validation, reference span, read length, op count
//                        with match runs merged, how many contig segments it touches (a8)
//   scan                 item offsets, n_items (host sync: buffer sizes)
//   k_item_emit          thread per segment: resolved item descriptors (strand glue a9, block-map window a3), item class + weight
//   k_cls_hist / k_cls_scan / k_permute2   class order (strand x light / heavy): groups and tiles are strand-homogeneous; the host reads
//                        the class counts and the weight sum / maximum while k_permute2 runs
//   k_chunk_sort         light items by weight inside windows of 128 positions of the class order (groups of similar length)
//   k_lift_lanes         DOMINANT KERNEL on HiFi batches (lane_core.hpp): persistent waves, 64 light items per wave (32 / 16 / 8 when the
//                        batch has few), one LANE per item, the whole shift / liftover / length check / simplify pipeline in place in a
//                        ~180-byte LDS region per item; the shift stage of items whose ops alternate match / lone indel (nearly all of
//                        HiFi data) runs as a lockstep loop over the clusters, lengths changed in place (PLO_LANE_LOCKSTEP=0: every
//                        item through the event-aligned walk)
//   k_lift_lanes_g       heavy items of batches with many of them (dominant on the stress workload): the same lane-per-item code, the
//                        regions in wave-private global scratch behind per-lane LDS windows (lane_core.hpp, LaneWin)
//   (heavy items of smaller batches)   scan of the weights, k_max_u32 (weight histogram -> tile geometry, host sync), k_tile_bounds,
//   k_lift_tiles         persistent waves, one wave per tile of items, the pipeline as wave scans over a flattened op stream in LDS
//   k_lift_retry         items whose LDS region / slice overflowed (lanes or tiles): one item per wave, larger slice
//   k_lift_mid           items heavier than the routing threshold: one WORKGROUP per item (8 or 16 waves share the item's op
//                        stream in LDS, scan carries cross the waves through LDS: Coop<NW>, lift_core.hpp)
//   k_lift_big           items too heavy even for that: one wave per item, wave-private global scratch
//   k_sum_stats          per-wave statistic slots -> batch counters (after the lift kernels)
//   k_compact_cigar      dense re-packing of the slab-allocated output CIGARs (plo_compact_output_dev)
//   k_finish_* / k_revcomp / k_sa_*   record finishing and SA text (plo_finish_batch_dev, plo_sa_segments_dev)
//   k_map_build          block maps of the contig segments, once per index (plo_index_create)
// There is no CPU path: every entry point fails with PLO_ERR_NO_DEVICE / PLO_ERR_HIP when the device is unusable.
#include <hip/hip_runtime.h>

#include <plo_wave.hpp>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "enumerate.hpp"
#include "finish_core.hpp"
#include "records_core.hpp"
#include "batch_core.hpp"
#include "nm_core.hpp"
#include "md_core.hpp"
#include "eqx_core.hpp"
#include "sort_core.hpp"
#include "merge_core.hpp"
#include "index_core.hpp"
#include "depth_core.hpp"
#include "pileup_core.hpp"
#define PLO_FA_HOST 1
#include "fasta_core.hpp"
#include "window_core.hpp"
#include "bgzf_walk.hpp"
#include "index_pack.hpp"
#include "inflate.hpp"
#include "deflate.hpp"
#include "lift_core.hpp"
#include "lane_core.hpp"
#include "lane_stream.hpp"

using namespace plo;

// ---------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------

// SEG_LANES lanes per read segment: the reference span (get_cigar_ref_offset) is a strided partial sum per lane + an
// xor-shuffle reduction, so that one load instruction covers SEG_LANES * 4 contiguous bytes of every segment's CIGAR;
// lane 0 of the group then does the overlap test against the contig's segments.
#ifndef PLO_SEG_LANES
#define PLO_SEG_LANES 2  // measured on MI355X (wgs30x enumerate pass): round 1, strided dword loads: 8 lanes 0.64 ms, 16 lanes 1.52 ms, 32 lanes 0.99 ms;
                         // round 2: 8 lanes 0.539 ms, 4 lanes 0.485 ms, 2 lanes 0.486 ms; round 3, every lane 32 / SEG_LANES consecutive ops per step
                         // with 16-byte loads: 8 lanes 0.497 ms, 4 lanes 0.432 ms, 2 lanes 0.402 ms, 1 lane 0.411 ms
#endif
constexpr uint32_t SEG_LANES = PLO_SEG_LANES, SEG_UNROLL = 32 / SEG_LANES < 2 ? 2 : 32 / SEG_LANES;
// It is also the boundary check of the device path (the kernels index with what the batch says): bit 0 of *err = an index
// outside its array (PLO_ERR_INVALID_ARG), bit 1 = a coordinate outside the 31-bit BAM range, an op code above 8, a CIGAR
// spanning 2^30 bases or more, or (raised by the descriptor kernels) a negative rev_pos (PLO_ERR_RANGE) -- what the
// reference's types rule out by construction.
enum { VERR_INDEX = 1u, VERR_RANGE = 2u, VERR_CAP = 4u };
__global__ __launch_bounds__(256) void k_seg_count(DevIndex ix, DevBatch bt, uint32_t *seg_cnt, int *seg_reflen, uint32_t *seg_readlen,
                                                   uint32_t *seg_nm, uint32_t *err) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s = t / SEG_LANES, sub = t % SEG_LANES;
    const bool live = s < bt.n_segs;
    uint32_t bad = 0;
    // Two dependent chains, issued side by side so that the kernel is three memory round trips deep instead of five:
    //   CIGAR offsets -> ops (reference span)   and   contig -> its segment range -> segment intervals (overlap test,
    //   one contig segment per lane of the group)
    uint32_t c0 = 0, c1 = 0, contig = 0, rd = 0;
    long long r_start = 0;
    if (live) {  // level 0: the segment's own fields
        c0 = bt.seg_cigar_off[s];
        c1 = bt.seg_cigar_off[s + 1];
        contig = bt.seg_contig[s];
        r_start = (long long)bt.seg_pos[s];
        rd = bt.seg_read[s];
        if (c1 < c0 || c1 > 0x7fffffffu) {  // (ops are indexed with int: more than 2^31 - 1 of them cannot be addressed)
            bad |= c1 < c0 ? VERR_INDEX : VERR_RANGE;
            c1 = c0;
        }
        if (r_start < 0 || r_start > 0x7ffffff0LL) bad |= VERR_RANGE;
        if (contig >= ix.n_contigs) bad |= VERR_INDEX;
        if (rd >= bt.n_reads) bad |= VERR_INDEX;
    }
    // level 1, all of it unconditional (lanes without a valid index read plo_safe_words): the read's length and offset, the contig's segment
    // range -- and, in the loop below, the ops
    const bool rd_ok = live && sub == 0 && rd < bt.n_reads, ct_ok = live && contig < ix.n_contigs;
    const unsigned long long len = *(rd_ok ? bt.read_seq_len + rd : (const uint32_t *)plo_safe_words);
    const unsigned long long off = *(rd_ok ? bt.read_seq_off + rd : (const uint64_t *)plo_safe_words);
    const uint32_t *const gp = ct_ok ? ix.contig_seg_off + contig : (const uint32_t *)plo_safe_words;
    const uint32_t g0 = gp[0], g1 = gp[1];  // g0 == g1: contig never seen in the asm->ref BAM (contig_alignment_scanner/mod.rs:364-367), or no contig
    long long part = 0;
    unsigned long long rpart = 0;  // read bases the CIGAR consumes (M I S H = X): what the length check compares with seq_len
    // Every lane of the group takes eight CONSECUTIVE ops per step (two 16-byte loads; the group's four lanes 128 contiguous bytes), so
    // that "is the previous op an alignment match too" -- the merged op count the lane-per-item kernel sizes its LDS regions by --
    // needs one shuffle per step: the last op of the lane below, or of the group's last lane in the previous step.
    uint32_t pairs = 0, carry = 0;
    constexpr uint32_t OPL = 32 / SEG_LANES;  // (a multiple of 4: 16-byte loads)
    const uint32_t n_ops_all = bt.n_segs ? bt.seg_cigar_off[bt.n_segs] : 0u;
    if (c1 > n_ops_all) {  // (offsets that are not monotone further on: the segment's ops would end behind the batch's -- none are read)
        bad |= VERR_INDEX;
        c1 = c0;
    }
    for (uint32_t base = c0; base < c1; base += SEG_LANES * OPL) {
        const uint32_t my = base + OPL * sub;
        uint32_t c[OPL];
        if (my < c1 && my + OPL <= n_ops_all) {  // (ops behind the segment's end belong to the next segment: masked by `have` below)
#pragma unroll
            for (uint32_t q = 0; q < OPL / 4; ++q) {
                const Ops4 a = *(const Ops4 *)(bt.cigar + my + 4 * q);
                c[4 * q] = a.x, c[4 * q + 1] = a.y, c[4 * q + 2] = a.z, c[4 * q + 3] = a.w;
            }
        } else {
#pragma unroll
            for (uint32_t u = 0; u < OPL; ++u) c[u] = (my + u < c1) ? bt.cigar[my + u] : 0xfu;  // (15: no op code, counted nowhere below)
        }
        uint32_t mprev = 0, mfirst = 0;
#pragma unroll
        for (uint32_t u = 0; u < OPL; ++u) {
            const uint32_t t = c[u] & 15u;
            const bool have = my + u < c1;
            if (have && ((0x18D >> t) & 1)) part += (long long)(c[u] >> 4);
            if (have && ((0x1B3 >> t) & 1)) rpart += (unsigned long long)(c[u] >> 4);
            if (have && t > 8u) bad |= VERR_RANGE;
            const uint32_t m = (have && ((0x181u >> t) & 1u)) ? 1u : 0u;
            if (u == 0) mfirst = m;
            else pairs += m & mprev;
            mprev = m;
        }
        const uint32_t below = (uint32_t)__shfl_up((int)mprev, 1, 64);
        pairs += mfirst & (sub ? below : carry);
        carry = (uint32_t)__shfl((int)mprev, (int)((threadIdx.x & 63u) | (SEG_LANES - 1)), 64);
    }
    // the first interval of every lane is fetched before the reduction needs the ops
    const uint32_t gl = g0 + sub;
    long long cs = 0, ce = 0;
    if (gl < g1) {
        cs = (long long)ix.cs_start[gl];
        ce = (long long)ix.cs_end[gl];
    }
#pragma unroll
    for (uint32_t d = 1; d < SEG_LANES; d <<= 1) {
        part += __shfl_xor(part, (int)d, 64);
        rpart += (unsigned long long)__shfl_xor((long long)rpart, (int)d, 64);
        pairs += (uint32_t)__shfl_xor((int)pairs, (int)d, 64);
    }
    if (part > 0x3fffffffLL) bad |= VERR_RANGE;
    if (rd_ok) {
        // (sparse bases: the header must lie inside the buffer; where it points is checked by every probe)
        const unsigned long long need = bt.seq_fmt == PLO_SEQ_BAM4          ? (len + 1) / 2
                                        : bt.seq_fmt == PLO_SEQ_BAM4_SPARSE ? (unsigned long long)sparse_header_bytes((uint32_t)len)
                                                                            : len;
        if (off > bt.seq_bytes || need > bt.seq_bytes - off) bad |= VERR_INDEX;
        if (bt.seq_fmt == PLO_SEQ_BAM4_SPARSE && (off & 15ull)) bad |= VERR_INDEX;
    }
    if (bad) atomicOr(err, bad);
    const long long r_end = r_start + part;
    // segment_range.intersect_range(&read_range): other.end >= self.start && other.start < self.end (int_range.rs:56-58)
    uint32_t n = (gl < g1 && r_end >= cs && r_start < ce) ? 1u : 0u;
    for (uint32_t g = gl + SEG_LANES; g < g1; g += SEG_LANES)  // contigs with more segments than lanes
        if (r_end >= (long long)ix.cs_start[g] && r_start < (long long)ix.cs_end[g]) ++n;
#pragma unroll
    for (uint32_t d = 1; d < SEG_LANES; d <<= 1) {
        n += (uint32_t)__shfl_xor((int)n, (int)d, 64);
        bad |= (uint32_t)__shfl_xor((int)bad, (int)d, 64);
    }
    if (!live || sub != 0) return;
    if (bad) n = 0;  // (a segment that fails the checks has no items: the one-round-trip path launches the lift kernels before the host sees the flag)
    seg_reflen[s] = (int)part;
    seg_readlen[s] = rpart > 0xfffffffeull ? 0xffffffffu : (uint32_t)rpart;
    seg_nm[s] = (c1 - c0) - pairs;
    seg_cnt[s] = n;
}

// thread per read segment: resolve the descriptors of its items (build_item_desc) at their scanned offsets
// `item_cap` (the one-round-trip path, liftover_fast): the item arrays hold that many items; a batch with more raises VERR_CAP and writes
// none beyond them (the host then takes the path that asks for the count first)
__global__ void k_item_emit(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, const uint32_t *seg_off, int *seg_reflen, uint32_t item_cap, uint32_t *err) {
    uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= bt.n_segs) return;
    // (level 0 of the descriptor loads goes out with the offsets: enumerate.hpp)
    const uint32_t o0 = seg_off[s], o1 = seg_off[s + 1];
    if (o1 > item_cap) {
        if (o1 > o0) atomicOr(err, (uint32_t)VERR_CAP);
        return;
    }
    const int ref_len = seg_reflen[s];
    SegInfo si;
    seg_info_level0(si, bt, wk, stages, s);
    if (o0 == o1) return;  // (no items -- among them the segments whose contig the index does not know: nothing below is indexed by it)
    seg_info_level1(si, ix, bt, wk, stages, s);
    bool neg = false;
    emit_segment_items(ix, wk, stages, s, o0, (long long)ref_len, si, &neg);
    if (neg) atomicOr(err, (uint32_t)VERR_RANGE);  // (a read segment behind its contig's end on a reverse-strand contig segment: enumerate.hpp)
}

// Block maps of the contig segments, built on the device at index creation: ONE WAVE per contig split segment walks its contig->reference
// CIGAR 64 ops at a time (build_segment_map_wave, enumerate.hpp: prefix sums for the positions, a max-scan for the start of every match
// run, a prefix sum of 1 or 2 entries per flush); count pass, host prefix sum (a few thousand segments), emit pass.  (Round 4: one THREAD
// per segment, 1 806 threads walking ~50 k ops each -- 37.8 ms per pass on wgs30x.)
__global__ __launch_bounds__(64) void k_map_build(const uint32_t *seg_cigar, const uint32_t *seg_cigar_off, const int64_t *seg_pos, uint32_t n_segments,
                                                  const uint32_t *kv_off, KV *kv, int *counts) {
    for (uint32_t g = blockIdx.x; g < n_segments; g += gridDim.x) {
        const uint32_t c0 = seg_cigar_off[g], c1 = seg_cigar_off[g + 1];
        const int cnt = build_segment_map_wave(seg_cigar + c0, c1 - c0, (long long)seg_pos[g], kv ? kv + kv_off[g] : nullptr);
        if (counts && threadIdx.x == 0) counts[g] = cnt;
    }
}

// explicit item list: thread per item
__global__ void k_item_desc(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, const uint32_t *in_seg, const uint32_t *in_cseg,
                            uint32_t *err) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= wk.n_items) return;
    uint32_t seg = in_seg[i];
    {   // the pair must exist: a read segment of the batch and a contig segment of ITS contig
        bool ok = seg < bt.n_segs;
        if (ok) {
            uint32_t contig = bt.seg_contig[seg];
            ok = contig < ix.n_contigs && in_cseg[i] < ix.contig_seg_off[contig + 1] - ix.contig_seg_off[contig];
        }
        if (!ok) {  // the host discards the batch before any lift kernel runs; the scans in between only need a class and a weight
            atomicOr(err, (uint32_t)VERR_INDEX);
            wk.item_cls[i] = 2u;
            wk.item_nin[i] = 0u;
            return;
        }
    }
    if (!build_item_desc(ix, bt, wk, stages, i, seg, in_cseg[i], segment_ref_len(bt, seg))) atomicOr(err, (uint32_t)VERR_RANGE);
}

// ---- device-wide exclusive scan of uint32 (three launches; out has n+1 entries, out[n] = total) -------------------
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_PER_THREAD = 8;
constexpr int SCAN_BLOCK = SCAN_THREADS * SCAN_PER_THREAD;

__device__ __forceinline__ unsigned block_scan_incl(unsigned v, unsigned *wave_tot /*[4]*/, unsigned &block_total) {
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = (unsigned)wv::scan_add((int)v);
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int k = 0; k < w; ++k) base += wave_tot[k];
    block_total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
    return inc + base;
}

// Class order (lift_types.hpp DevWork) in three launches: per block of CLS_BLOCK items the counts of classes 0, 1, 2 (k_cls_hist,
// which also reduces the weights the host sizes buffers by), an exclusive scan of the block counts (k_cls_scan, one workgroup),
// and the permutation itself from block offset + rank inside the block (k_permute2).
constexpr uint32_t CLS_THREADS = 256, CLS_PER = 8, CLS_BLOCK = CLS_THREADS * CLS_PER;
// partial: [6][nb] per block: items of class 0 / 1 / 2, heaviest item, sum of the weights (exact, 64 bits as two words: the batch-size
// guard and the output sizing rest on it); totals (k_cls_scan): [0..2] class counts, [3] heaviest item, [4..5] 64-bit sum of the weights
// the CLS_PER = 8 consecutive values of a thread: two 16-byte loads (the arrays come from hipMalloc and base is a multiple of 8), element by element
// with `fill` behind the end only in the array's last block
__device__ __forceinline__ void load8(const uint32_t *a, uint32_t base, uint32_t n, uint32_t fill, uint32_t (&v)[8]) {
    if (base + 8u <= n) {
        const uint4 x = *(const uint4 *)(a + base), y = *(const uint4 *)(a + base + 4);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w, v[4] = y.x, v[5] = y.y, v[6] = y.z, v[7] = y.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) v[k] = base + k < n ? a[base + k] : fill;
    }
}
// (`n_dev` != NULL: the item count is read from device memory -- the one-round-trip path launches with the arrays' capacity `n`; a count above
// it means k_item_emit raised VERR_CAP and the arrays hold a mixture of this batch's and the last one's descriptors: the class totals then
// come out zero, so that k_permute2, k_chunk_sort_w and the lift kernels touch nothing before the host sees the flag and takes the other path)
__global__ __launch_bounds__(CLS_THREADS) void k_cls_hist(const uint32_t *item_cls, const uint32_t *item_w, uint32_t n, uint32_t nb, uint32_t *partial, const uint32_t *n_dev) {
    __shared__ uint32_t acc[6];
    if (n_dev) n = *n_dev <= n ? *n_dev : 0u;  // (more items than the arrays hold, VERR_CAP: k_item_emit left stale descriptors -- nothing is classified, nothing lifted)
    if (threadIdx.x < 6) acc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * CLS_BLOCK + threadIdx.x * CLS_PER;
    uint32_t c0 = 0, c1 = 0, c2 = 0, mw = 0, sl = 0, sh = 0;  // sl / sh: sums of the weights' low / high 16 bits (a block's fit 32 bits each)
    uint32_t cv[CLS_PER], wv_[CLS_PER];
    load8(item_cls, base, n, 3u, cv);
    load8(item_w, base, n, 0u, wv_);
#pragma unroll
    for (uint32_t k = 0; k < CLS_PER; ++k) {
        const uint32_t c = cv[k], w = wv_[k];  // (behind the end: class 3 counted nowhere, weight 0)
        c0 += c == 0;
        c1 += c == 1;
        c2 += c == 2;
        mw = w > mw ? w : mw;
        sl += w & 0xffffu;
        sh += w >> 16;
    }
    // (counts of a wave fit 16 bits: 64 threads x 8 items)
    const int p01 = wv::reduce_add((int)(c0 | (c1 << 16))), p2 = wv::reduce_add((int)c2), pm = wv::reduce_max((int)(mw & 0x7fffffffu));
    const int psl = wv::reduce_add((int)sl), psh = wv::reduce_add((int)sh);
    if ((threadIdx.x & 63u) == 0) {
        atomicAdd(&acc[0], (uint32_t)p01 & 0xffffu);
        atomicAdd(&acc[1], (uint32_t)p01 >> 16);
        atomicAdd(&acc[2], (uint32_t)p2);
        atomicMax(&acc[3], (uint32_t)pm);
        atomicAdd(&acc[4], (uint32_t)psl);
        atomicAdd(&acc[5], (uint32_t)psh);
    }
    __syncthreads();
    if (threadIdx.x < 6) partial[threadIdx.x * nb + blockIdx.x] = acc[threadIdx.x];
}
__global__ __launch_bounds__(SCAN_THREADS) void k_cls_scan(uint32_t *partial, uint32_t nb, uint32_t *totals) {
    __shared__ unsigned wt[4];
    // one pass over the blocks, SCAN_THREADS at a time: the six rows of a step are loaded together (one round trip per step, not one per
    // row and step), the three class rows scanned, the other three reduced
    unsigned carry[3] = {0, 0, 0};
    unsigned mx = 0;
    unsigned long long sum = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += SCAN_THREADS) {
        const uint32_t i = b0 + threadIdx.x;
        const bool ok = i < nb;
        const uint32_t j = ok ? i : 0u;  // (nb > 0: the kernel is launched for batches with items)
        unsigned v[6];
#pragma unroll
        for (uint32_t c = 0; c < 6; ++c) v[c] = partial[c * nb + j];
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            const unsigned x = ok ? v[c] : 0u;
            unsigned tot;
            const unsigned inc = block_scan_incl(x, wt, tot);
            if (ok) partial[c * nb + i] = carry[c] + inc - x;
            carry[c] += tot;
        }
        if (ok) {
            mx = v[3] > mx ? v[3] : mx;
            sum += (unsigned long long)v[4] + ((unsigned long long)v[5] << 16);
        }
    }
    // heaviest item and the sum of the weights
    __shared__ unsigned long long ssum;
    __shared__ unsigned smax;
    if (threadIdx.x == 0) {
        ssum = 0;
        smax = 0;
    }
    __syncthreads();
    mx = (unsigned)wv::reduce_max((int)(mx & 0x7fffffffu));  // (weights are below 2^31: checked sums of CIGAR ops and block-map entries)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) sum += (unsigned long long)__shfl_xor((long long)sum, d, 64);
    if ((threadIdx.x & 63u) == 0) {
        atomicMax(&smax, mx);
        atomicAdd(&ssum, sum);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        totals[0] = carry[0];
        totals[1] = carry[1];
        totals[2] = carry[2];
        totals[3] = smax;
        totals[4] = (uint32_t)(ssum & 0xffffffffull);
        totals[5] = (uint32_t)(ssum >> 32);
    }
}
__global__ __launch_bounds__(CLS_THREADS) void k_permute2(const uint32_t *item_cls, const uint32_t *item_nin, const uint32_t *partial, const uint32_t *totals,
                                                          uint32_t n, uint32_t nb, uint32_t *perm, uint32_t *nin_p, uint32_t huge_w, const uint32_t *n_dev) {
    __shared__ unsigned wt[4];
    if (n_dev) n = *n_dev <= n ? *n_dev : 0u;
    const uint32_t base = blockIdx.x * CLS_BLOCK + threadIdx.x * CLS_PER;
    // every load in front of the scans and of the stores (a load behind a store waits for the store: the memory counter is in order)
    uint32_t cls[CLS_PER], wgt[CLS_PER];
    load8(item_cls, base, n, 3u, cls);
    load8(item_nin, base, n, 0u, wgt);
    const uint32_t p0 = partial[0 * nb + blockIdx.x], p1 = partial[1 * nb + blockIdx.x], p2 = partial[2 * nb + blockIdx.x];
    const uint32_t n0 = totals[0], n1 = totals[1], n2 = totals[2];
    uint32_t c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
    for (uint32_t k = 0; k < CLS_PER; ++k) {
        c0 += cls[k] == 0;
        c1 += cls[k] == 1;
        c2 += cls[k] == 2;
    }
    unsigned tot;
    const unsigned i01 = block_scan_incl(c0 | (c1 << 16), wt, tot);  // (a block holds 2 048 items: each count fits 16 bits)
    const unsigned i2 = block_scan_incl(c2, wt, tot);
    uint32_t r0 = p0 + (i01 & 0xffffu) - c0;
    uint32_t r1 = p1 + (i01 >> 16) - c1;
    uint32_t r2 = p2 + i2 - c2;
#pragma unroll
    for (uint32_t k = 0; k < CLS_PER; ++k) {
        const uint32_t i = base + k;
        if (i >= n) break;
        const uint32_t c = cls[k];
        const uint32_t j = class_order_pos(i, c, r0, r1, r2, n0, n1, n2);
        perm[j] = i;
        // only the large items are tiled; items no geometry can hold (heavier than huge_w) take no room in the weight stream: they
        // ride along in their neighbours' tiles, 64 per pass, and are handed to the large-item kernel there
        const uint32_t w = wgt[k];
        nin_p[j] = (c >= 2 && w <= huge_w) ? w : 0u;
        r0 += c == 0;
        r1 += c == 1;
        r2 += c == 2;
    }
}

// k_cls_scan and k_permute2 in one launch (the one-round-trip path: every launch of an enumerate pass costs ~5 us of dispatch latency, as
// much as these kernels' work on a 50 k-read window): every block adds up k_cls_hist's raw rows itself -- the blocks in front of it for its
// offsets, all of them for the class totals -- and block 0 leaves the totals ([0..5] as k_cls_scan, [6] = the item count as the scan left it).
__global__ __launch_bounds__(CLS_THREADS) void k_permute2_s(const uint32_t *item_cls, const uint32_t *item_nin, const uint32_t *partial, uint32_t *totals, uint32_t n,
                                                            uint32_t nb, uint32_t *perm, uint32_t *nin_p, uint32_t huge_w, const uint32_t *n_dev) {
    __shared__ unsigned wt[4];
    __shared__ uint32_t red[6];
    __shared__ unsigned long long rsum;
    __shared__ unsigned rmax;
    const uint32_t n_raw = *n_dev;
    n = n_raw <= n ? n_raw : 0u;
    const uint32_t base = blockIdx.x * CLS_BLOCK + threadIdx.x * CLS_PER;
    uint32_t cls[CLS_PER], wgt[CLS_PER];
    load8(item_cls, base, n, 3u, cls);
    load8(item_nin, base, n, 0u, wgt);
    if (threadIdx.x < 6) red[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        rsum = 0;
        rmax = 0;
    }
    __syncthreads();
    {
        uint32_t t0 = 0, t1 = 0, t2 = 0, q0 = 0, q1 = 0, q2 = 0;
        unsigned mx = 0;
        unsigned long long sum = 0;
        for (uint32_t b = threadIdx.x; b < nb; b += CLS_THREADS) {
            const uint32_t v0 = partial[b], v1 = partial[nb + b], v2 = partial[2 * nb + b];
            t0 += v0, t1 += v1, t2 += v2;
            if (b < blockIdx.x) q0 += v0, q1 += v1, q2 += v2;
            if (blockIdx.x == 0) {
                const unsigned m = partial[3 * nb + b];
                mx = m > mx ? m : mx;
                sum += (unsigned long long)partial[4 * nb + b] + ((unsigned long long)partial[5 * nb + b] << 16);
            }
        }
        const uint32_t r[6] = {(uint32_t)wv::reduce_add((int)t0), (uint32_t)wv::reduce_add((int)t1), (uint32_t)wv::reduce_add((int)t2),
                               (uint32_t)wv::reduce_add((int)q0), (uint32_t)wv::reduce_add((int)q1), (uint32_t)wv::reduce_add((int)q2)};
        if (blockIdx.x == 0) {
            mx = (unsigned)wv::reduce_max((int)(mx & 0x7fffffffu));
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) sum += (unsigned long long)__shfl_xor((long long)sum, d, 64);
        }
        if ((threadIdx.x & 63u) == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (r[k]) atomicAdd(&red[k], r[k]);
            if (blockIdx.x == 0) {
                atomicMax(&rmax, mx);
                atomicAdd(&rsum, sum);
            }
        }
    }
    __syncthreads();
    const uint32_t n0 = red[0], n1 = red[1], n2 = red[2], p0 = red[3], p1 = red[4], p2 = red[5];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        totals[0] = n0;
        totals[1] = n1;
        totals[2] = n2;
        totals[3] = rmax;
        totals[4] = (uint32_t)(rsum & 0xffffffffull);
        totals[5] = (uint32_t)(rsum >> 32);
        totals[6] = n_raw;
    }
    uint32_t c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
    for (uint32_t k = 0; k < CLS_PER; ++k) {
        c0 += cls[k] == 0;
        c1 += cls[k] == 1;
        c2 += cls[k] == 2;
    }
    unsigned tot;
    const unsigned i01 = block_scan_incl(c0 | (c1 << 16), wt, tot);
    const unsigned i2 = block_scan_incl(c2, wt, tot);
    uint32_t r0 = p0 + (i01 & 0xffffu) - c0;
    uint32_t r1 = p1 + (i01 >> 16) - c1;
    uint32_t r2 = p2 + i2 - c2;
#pragma unroll
    for (uint32_t k = 0; k < CLS_PER; ++k) {
        const uint32_t i = base + k;
        if (i >= n) break;
        const uint32_t c = cls[k];
        const uint32_t j = class_order_pos(i, c, r0, r1, r2, n0, n1, n2);
        perm[j] = i;
        const uint32_t w = wgt[k];
        nin_p[j] = (c >= 2 && w <= huge_w) ? w : 0u;
        r0 += c == 0;
        r1 += c == 1;
        r2 += c == 2;
    }
}

// The lane-per-item kernel runs a group of 64 items for as long as its longest item takes -- in batch order about twice the average.
// Inside windows of LANE_SORT_WINDOW consecutive positions of the class order (two groups: the reads of a window still share their
// descriptor / CIGAR / block-map cache lines) the items are therefore sorted by weight: a group of the longer and a group of the
// shorter ones.  One workgroup per window, counting sort in LDS.
constexpr uint32_t LANE_SORT_WINDOW = 128;
constexpr uint32_t LANE_SORT_MAX_CHUNK = 2048, LANE_SORT_THREADS = 256, LANE_SORT_PER = LANE_SORT_MAX_CHUNK / LANE_SORT_THREADS;
// `glist` != NULL: the sorted window is also cut into the lane kernel's groups by LDS budget (lane_groups_cut, enumerate.hpp: consecutive
// items while there are fewer than 64 and their regions fit `cap` dwords) and the groups are appended to the list ({first position, count};
// *n_groups zeroed by the host).  A window sorted by weight has its long items together; as fixed groups of 64 those need more LDS than a
// wave's slice and run in several rounds -- which is what made windows larger than 128 slower although they level the lanes better.
// Sort key: what the group's loops run for -- the merged op count n_m (= / X ops, which the tiling weight counts, are merged away before any
// loop sees them) plus the block-map entries of the item's window (the liftover loop's extra pieces); in the class with the shift stage n_m
// counts twice (its rounds and scans follow the indel clusters, half of n_m, and cost twice a liftover iteration).  Off line, windows of 128,
// against the tiling weight: shift rounds per group 1.67 -> 1.52 x the mean, liftover iterations 1.59 -> 1.49 (forward class) / 1.56.
__global__ __launch_bounds__(LANE_SORT_THREADS) void k_chunk_sort(uint32_t *perm, const uint32_t *n_m, const uint32_t *w0, const uint32_t *w1, uint32_t n0, uint32_t n1,
                                                                  uint32_t chunk, const uint32_t *region, uint32_t cap, uint32_t *glist, uint32_t *n_groups, uint32_t glist_cap) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[4];
    __shared__ uint16_t reg[LANE_SORT_MAX_CHUNK], nxt[LANE_SORT_MAX_CHUNK];
    __shared__ uint32_t pre[LANE_SORT_MAX_CHUNK + 1];
    __shared__ uint32_t starts[LANE_SORT_MAX_CHUNK + 1], g_base, g_cnt;
    const uint32_t c0 = (n0 + chunk - 1) / chunk;
    uint32_t lo, hi;
    if (blockIdx.x < c0) {  // chunks do not straddle the two lane classes
        lo = blockIdx.x * chunk;
        hi = lo + chunk < n0 ? lo + chunk : n0;
    } else {
        lo = n0 + (blockIdx.x - c0) * chunk;
        hi = lo + chunk < n0 + n1 ? lo + chunk : n0 + n1;
    }
    hist[threadIdx.x] = 0;
    __syncthreads();
    uint32_t g[LANE_SORT_PER], k[LANE_SORT_PER];
#pragma unroll
    for (uint32_t j = 0; j < LANE_SORT_PER; ++j) {
        const uint32_t p = lo + j * LANE_SORT_THREADS + threadIdx.x;
        g[j] = p < hi ? perm[p] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < LANE_SORT_PER; ++j) {
        const uint32_t p = lo + j * LANE_SORT_THREADS + threadIdx.x;
        uint32_t w = 0u;
        if (p < hi) w = (blockIdx.x < c0 ? n_m[g[j]] : 2u * n_m[g[j]]) + (w1[g[j]] - w0[g[j]]);
        k[j] = w < 255u ? w : 255u;
        if (p < hi) atomicAdd(&hist[k[j]], 1u);
    }
    __syncthreads();
    // exclusive prefix of the 256 bins: thread t owns bin t
    const uint32_t mine = hist[threadIdx.x];
    const uint32_t inc = (uint32_t)wv::scan_add((int)mine);
    if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) before += wsum[w];
    hist[threadIdx.x] = before + inc - mine;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < LANE_SORT_PER; ++j) {
        const uint32_t p = lo + j * LANE_SORT_THREADS + threadIdx.x;
        if (p < hi) {
            const uint32_t pos = atomicAdd(&hist[k[j]], 1u);
            perm[lo + pos] = g[j];
            if (glist) reg[pos] = (uint16_t)(region[g[j]] < 0xffffu ? region[g[j]] : 0xffffu);
        }
    }
    if (!glist) return;
    const uint32_t n = hi - lo;
    __syncthreads();
    {   // exclusive prefix of the regions in sorted order: thread t owns positions [t * PER, t * PER + PER)
        uint32_t loc[LANE_SORT_PER], tot = 0;
#pragma unroll
        for (uint32_t j = 0; j < LANE_SORT_PER; ++j) {
            const uint32_t i = threadIdx.x * LANE_SORT_PER + j;
            loc[j] = tot;
            tot += i < n ? (uint32_t)reg[i] : 0u;
        }
        const uint32_t inc2 = (uint32_t)wv::scan_add((int)tot);
        __syncthreads();  // (wsum is reused)
        if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = inc2;
        __syncthreads();
        uint32_t base = inc2 - tot;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) base += wsum[w];
#pragma unroll
        for (uint32_t j = 0; j < LANE_SORT_PER; ++j) {
            const uint32_t i = threadIdx.x * LANE_SORT_PER + j;
            if (i < n) pre[i] = base + loc[j];
        }
        if (threadIdx.x == LANE_SORT_THREADS - 1) pre[n] = base + tot;  // (positions beyond n add nothing)
    }
    __syncthreads();
    // the group that starts at position i ends at the largest j <= i + 64 with pre[j] - pre[i] <= cap (at least one item)
#pragma unroll
    for (uint32_t jj = 0; jj < LANE_SORT_PER; ++jj) {
        const uint32_t i = jj * LANE_SORT_THREADS + threadIdx.x;
        if (i < n) {
            uint32_t a = i, b = i + 64u < n ? i + 64u : n;  // invariant: a fits, everything above b does not (or is out of range)
            while (a < b) {
                const uint32_t m = (a + b + 1u) >> 1;
                if (pre[m] - pre[i] <= cap) a = m;
                else b = m - 1u;
            }
            nxt[i] = (uint16_t)(a > i ? a : i + 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ng = 0;
        for (uint32_t i = 0; i < n; i = nxt[i]) starts[ng++] = i;
        starts[ng] = n;
        g_cnt = ng;
        g_base = atomicAdd(n_groups, ng);
    }
    __syncthreads();
    // (the host sizes the list for the most groups the windows can have, a group being cut at 64 items or at the slice's capacity; a
    // group beyond it would be a sizing bug -- it is not written, and the batch's count then exceeds the capacity, which the host checks)
    for (uint32_t q = threadIdx.x; q < g_cnt; q += LANE_SORT_THREADS) {
        if (g_base + q >= glist_cap) continue;
        glist[2 * (g_base + q)] = lo + starts[q];
        glist[2 * (g_base + q) + 1] = starts[q + 1] - starts[q];
    }
}

// The same sort for the default geometry -- windows of at most 128 positions, fixed groups: one WAVE per window (two items per lane, four bins
// per lane), four windows per workgroup, no workgroup barrier and 4 KB of LDS (k_chunk_sort: a workgroup and 25 KB per window).
__global__ __launch_bounds__(256) void k_chunk_sort_w(uint32_t *perm, const uint32_t *n_m, const uint32_t *w0, const uint32_t *w1, uint32_t n0, uint32_t n1,
                                                      uint32_t chunk, const uint32_t *totals_dev) {
    __shared__ uint32_t hist_all[4][256];
    if (totals_dev) {  // (the class counts from device memory: k_cls_scan's totals)
        n0 = totals_dev[0];
        n1 = totals_dev[1];
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t *const hist = hist_all[wave];
    const uint32_t c0 = (n0 + chunk - 1) / chunk, c1 = (n1 + chunk - 1) / chunk;
    const uint32_t win = blockIdx.x * 4u + wave;
    if (win >= c0 + c1) return;
    uint32_t lo, hi;
    if (win < c0) {  // windows do not straddle the two lane classes
        lo = win * chunk;
        hi = lo + chunk < n0 ? lo + chunk : n0;
    } else {
        lo = n0 + (win - c0) * chunk;
        hi = lo + chunk < n0 + n1 ? lo + chunk : n0 + n1;
    }
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) hist[lane + 64u * q] = 0;
    uint32_t g[2], k[2];
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
        const uint32_t p = lo + j * 64u + lane;
        g[j] = p < hi ? perm[p] : 0u;
    }
    uint32_t a[2], b0[2], b1[2];
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {  // (six gathers in flight)
        a[j] = n_m[g[j]];
        b0[j] = w0[g[j]];
        b1[j] = w1[g[j]];
    }
    wv::sync();
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
        const uint32_t p = lo + j * 64u + lane;
        const uint32_t w = (win < c0 ? a[j] : 2u * a[j]) + (b1[j] - b0[j]);
        k[j] = w < 255u ? w : 255u;
        if (p < hi) atomicAdd(&hist[k[j]], 1u);
    }
    wv::sync();
    {   // exclusive prefix of the 256 bins: lane t owns bins 4 t .. 4 t + 3
        uint32_t h[4], tot = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            h[q] = hist[4u * lane + q];
            tot += h[q];
        }
        uint32_t base = (uint32_t)wv::scan_add((int)tot) - tot;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            hist[4u * lane + q] = base;
            base += h[q];
        }
    }
    wv::sync();
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
        const uint32_t p = lo + j * 64u + lane;
        if (p < hi) perm[lo + atomicAdd(&hist[k[j]], 1u)] = g[j];
    }
}

// thread per tile: first class-order position (>= n_small) whose exclusive op prefix reaches the tile's window
__global__ void k_tile_bounds(const uint32_t *op_prefix, uint32_t n_items, uint32_t n_tiles, int window, uint32_t n_small, uint32_t *tile_lo) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tiles) return;
    uint32_t lo = prefix_lower_bound(op_prefix, n_items, (unsigned long long)t * (unsigned)window);
    tile_lo[t] = lo > n_small ? lo : n_small;
}

// maximum (out[0]) and 64-bit sum (out[2..3]) of a uint32 array, one atomic pair per wave, plus a histogram of the values
// in bins of WHIST_STEP (out[WHIST_AT + b], last bin = everything above); out must be zeroed
constexpr int WHIST_STEP = 32, WHIST_BINS = 40, WHIST_AT = 8;
// out[4..6] = *t0, *t1, *t2 (scan totals the host wants in the same copy)
__global__ __launch_bounds__(256) void k_max_u32(const uint32_t *in, uint32_t n, uint32_t *out, const uint32_t *t0, const uint32_t *t1,
                                                 const uint32_t *t2) {
    __shared__ uint32_t hist[WHIST_BINS];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[4] = *t0;
        out[5] = *t1;
        out[6] = *t2;
    }
    if (threadIdx.x < WHIST_BINS) hist[threadIdx.x] = 0;
    __syncthreads();
    uint32_t m = 0;
    unsigned long long sum = 0;
    // (the weights of a batch crowd into a few bins: one LDS atomic per distinct bin of a wave's 64 items, not one per item)
    const uint32_t n_up = (n + 63u) & ~63u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += gridDim.x * blockDim.x) {
        const bool live = i < n;
        uint32_t v = live ? in[i] : 0u;
        m = v > m ? v : m;
        sum += v;
        uint32_t b = v / WHIST_STEP;
        b = b < WHIST_BINS - 1 ? b : WHIST_BINS - 1;
        unsigned long long todo = __ballot(live);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t lb = (uint32_t)__shfl((int)b, leader, 64);
            const unsigned long long same = __ballot(live && b == lb);
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
    __syncthreads();
    if (threadIdx.x < WHIST_BINS && hist[threadIdx.x]) atomicAdd(out + WHIST_AT + threadIdx.x, hist[threadIdx.x]);
    int r = wv::reduce_max((int)(m & 0x7fffffffu));
    unsigned lo = (unsigned)wv::reduce_add((int)(unsigned)(sum & 0xffffffull));
    unsigned hi = (unsigned)wv::reduce_add((int)(unsigned)(sum >> 24));
    // one global atomic per block and counter (a hot address takes ~88 atomics per microsecond)
    __shared__ unsigned long long bsum;
    __shared__ unsigned bmax;
    if (threadIdx.x == 0) {
        bsum = 0;
        bmax = 0;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        if (r > 0) atomicMax(&bmax, (unsigned)r);
        atomicAdd(&bsum, (unsigned long long)lo + ((unsigned long long)hi << 24));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (bmax) atomicMax(out, bmax);
        atomicAdd((unsigned long long *)(out + 2), bsum);
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_sums(const uint32_t *in, uint32_t n, uint32_t *partial) {
    __shared__ unsigned wt[4];
    uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER_THREAD;
    static_assert(SCAN_PER_THREAD == 8, "load8");
    uint32_t v[SCAN_PER_THREAD];
    load8(in, base, n, 0u, v);
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) s += v[k];
    unsigned tot;
    block_scan_incl(s, wt, tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_partials(uint32_t *partial, uint32_t nb, uint32_t *out, uint32_t n) {
    __shared__ unsigned wt[4];
    unsigned carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += SCAN_THREADS) {
        uint32_t i = b0 + threadIdx.x;
        unsigned v = i < nb ? partial[i] : 0;
        unsigned tot;
        unsigned inc = block_scan_incl(v, wt, tot);
        if (i < nb) partial[i] = carry + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_apply(const uint32_t *in, uint32_t n, const uint32_t *partial,
                                                             uint32_t *out) {
    __shared__ unsigned wt[4];
    uint32_t base = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER_THREAD;
    uint32_t v[SCAN_PER_THREAD];
    load8(in, base, n, 0u, v);
    const unsigned before = partial[blockIdx.x];
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) s += v[k];
    unsigned tot;
    unsigned inc = block_scan_incl(s, wt, tot);
    unsigned run = before + inc - s;
    if (base + SCAN_PER_THREAD <= n) {  // (two 16-byte stores; out comes from hipMalloc and base is a multiple of 8)
        uint4 x, y;
        x.x = run, x.y = x.x + v[0], x.z = x.y + v[1], x.w = x.z + v[2];
        y.x = x.w + v[3], y.y = y.x + v[4], y.z = y.y + v[5], y.w = y.z + v[6];
        *(uint4 *)(out + base) = x;
        *(uint4 *)(out + base + 4) = y;
    } else {
        for (int k = 0; k < SCAN_PER_THREAD; ++k) {
            if (base + k < n) out[base + k] = run;
            run += v[k];
        }
    }
}

// (Round 6 also tried ONE WORKGROUP for a window's ~52 k values -- 16 waves, every wave its stretch as coalesced rows, one exchange through LDS:
// 0.239-0.242 ms per 50 k-read call against 0.236-0.239 with the three launches, EXPERIMENTS 6.12; removed.  Back-to-back launches of small
// kernels overlap their dispatch; a command is only dear where the stream has to drain: event records, the copy back.)
// The exclusive scan in ONE launch (decoupled look-back), an experiment of the one-round-trip path that stays switched off (PLO_SCAN_CHAIN=1):
// two launches fewer, but the chain of look-backs costs more than their ~5 us each -- wgs30x 2 M reads (1 006 tiles): enumerate pass 0.273 ms
// against 0.261, step 1.512 against 1.490 ms; 50 k-read window (25 tiles): 0.249-0.258 against 0.250 ms (tools/exp_scan.sh).
// How it works: tiles of SCAN_BLOCK values take their number from a ticket, so a tile only ever waits for tiles that started before
// it; a tile publishes {1, its sum}, looks back over the words of the tiles in front of it -- 64 at a time, one per lane of its first wave,
// adding sums until a word {2, inclusive prefix} turns up -- and publishes {2, its inclusive prefix}.  State and value travel in one 64-bit
// word (no ordering between two stores to rely on).  `state` (a word per tile) and `ticket` are zero at launch.  out[n] = the total.
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_chain(const uint32_t *in, uint32_t n, uint32_t *out, unsigned long long *state, uint32_t *ticket) {
    __shared__ unsigned wt[4];
    __shared__ uint32_t sh_tile, sh_before;
    if (threadIdx.x == 0) sh_tile = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t tile = sh_tile;
    const uint32_t base = tile * SCAN_BLOCK + threadIdx.x * SCAN_PER_THREAD;
    uint32_t v[SCAN_PER_THREAD];
    load8(in, base, n, 0u, v);
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER_THREAD; ++k) s += v[k];
    unsigned tot;
    const unsigned inc = block_scan_incl(s, wt, tot);
    if (threadIdx.x < 64u) {
        const int lane = (int)threadIdx.x;
        if (lane == 0) __hip_atomic_store(state + tile, ((tile ? 1ull : 2ull) << 32) | (unsigned long long)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned before = 0;
        if (tile) {
            int j0 = (int)tile - 1;
            for (;;) {
                const int j = j0 - lane;
                unsigned long long w = 2ull << 32;  // (in front of tile 0: a prefix of zero)
                if (j >= 0) {
                    for (;;) {
                        w = __hip_atomic_load(state + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((w >> 32) != 0) break;
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                const unsigned long long pm = __ballot((w >> 32) == 2ull);
                const int first = pm ? __builtin_ctzll(pm) : 63;
                before += (unsigned)wv::reduce_add((int)(lane <= first ? (unsigned)w : 0u));
                if (pm) break;
                j0 -= 64;
            }
            if (lane == 0) __hip_atomic_store(state + tile, (2ull << 32) | (unsigned long long)(before + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            sh_before = before;
            if (tile + 1u == gridDim.x) out[n] = before + tot;
        }
    }
    __syncthreads();
    unsigned run = sh_before + inc - s;
    if (base + SCAN_PER_THREAD <= n) {
        uint4 x, y;
        x.x = run, x.y = x.x + v[0], x.z = x.y + v[1], x.w = x.z + v[2];
        y.x = x.w + v[3], y.y = y.x + v[4], y.z = y.y + v[5], y.w = y.z + v[6];
        *(uint4 *)(out + base) = x;
        *(uint4 *)(out + base + 4) = y;
    } else {
        for (int k = 0; k < SCAN_PER_THREAD; ++k) {
            if (base + k < n) out[base + k] = run;
            run += v[k];
        }
    }
}

// ---- the dominant kernel: one wave per tile ---------------------------------------------------------------------
constexpr uint32_t STAT_SLOTS = 1u << 16;  // >= waves of any lift launch (CUs x 16 blocks x 4 waves at most)
constexpr int TILE_WAVES = 4;  // waves per workgroup; every wave works on its own tile with its own LDS slice

// Persistent: the grid is sized to the resident capacity of the chip and every wave strides over the tiles, keeping its
// output slab and statistics in registers (WaveCtx).
// Register budget: 3 waves per SIMD (<= 168 VGPRs) is what the LDS slices allow as well (12 waves per CU); without the
// attribute the allocator may drift past 168 and the resident waves drop to 2 per SIMD.
#ifndef PLO_TILE_WPE
#define PLO_TILE_WPE 3
#endif
#define PLO_TILE_OCC __attribute__((amdgpu_waves_per_eu(PLO_TILE_WPE, PLO_TILE_WPE)))
// (every lift kernel exists twice: for dense read bases and, `_sp`, for PLO_SEQ_BAM4_SPARSE batches, whose probes look granules up)
// CAPC > 0: the slice capacity as a compile-time constant.  The arrays of the slice then sit at constant offsets from one base and
// the LDS instructions carry them as immediates (one address register per element instead of one per array and access): 166 -> 137
// VGPRs at cap 320, and with cap 256 the kernel fits 128 VGPRs, i.e. 16 waves per CU -- which is also exactly what 16 slices of
// tile_mem_bytes(256) = 10 240 B leave of the 160 KB of LDS.
template <bool SP, int CAPC>
PLO_DEV void lift_tiles_kernel(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t n_tiles, int window,
                               int big_thresh, int cap, uint32_t lds_per_wave) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int w = threadIdx.x >> 6;
    // XCD-aware placement: workgroup b runs on XCD b % 8 (observed dispatch order); consecutive wave ids -- hence
    // neighbouring tiles, i.e. reads of the same contig region with the same block-map / reference lines -- share an L2.
    uint32_t nb = gridDim.x;
    uint32_t per = nb >> 3;
    uint32_t b = blockIdx.x;
    uint32_t tb = (per > 0 && (nb & 7u) == 0) ? (b & 7u) * per + (b >> 3) : b;
    const uint32_t tw = blockDim.x >> 6;
    const uint32_t wave = tb * tw + (uint32_t)w, n_waves = nb * tw;
    if constexpr (CAPC > 0) {
        cap = CAPC;
        lds_per_wave = (uint32_t)((tile_mem_bytes(CAPC) + 15) & ~(size_t)15);
    }
    TileMem m = carve_tile_mem(smem + (size_t)w * lds_per_wave, cap);
    WaveCtx ctx;
    (void)window;
    if (wk.slab_pre) {  // first slab by wave id: 3 072 waves reserving theirs at the same moment would serialise on one counter
        ctx.slab_base = (unsigned long long)wave * SLAB_OPS;
        ctx.slab_left = SLAB_OPS;
    }
    lift_tiles_persistent<SP>(ix, bt, wk, stages, wave, n_waves, n_tiles, big_thresh, m, ctx);
    wave_ctx_flush(wk, ctx, wave);
}
__global__ __launch_bounds__(TILE_WAVES * 64) PLO_TILE_OCC void k_lift_tiles(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages,
                                                               uint32_t n_tiles, int window, int big_thresh, int cap,
                                                               uint32_t lds_per_wave) {
    lift_tiles_kernel<false, 0>(ix, bt, wk, stages, n_tiles, window, big_thresh, cap, lds_per_wave);
}
constexpr int TILE_CAP_SMALL = 256;  // the geometry of batches without heavy items (HiFi reads on a clean assembly): see lift_tiles_kernel
__global__ __launch_bounds__(TILE_WAVES * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_lift_tiles_c256(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages,
                                                               uint32_t n_tiles, int window, int big_thresh, int cap,
                                                               uint32_t lds_per_wave) {
    lift_tiles_kernel<false, TILE_CAP_SMALL>(ix, bt, wk, stages, n_tiles, window, big_thresh, cap, lds_per_wave);
}
__global__ __launch_bounds__(TILE_WAVES * 64) PLO_TILE_OCC void k_lift_tiles_sp(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages,
                                                                  uint32_t n_tiles, int window, int big_thresh, int cap,
                                                                  uint32_t lds_per_wave) {
    lift_tiles_kernel<true, 0>(ix, bt, wk, stages, n_tiles, window, big_thresh, cap, lds_per_wave);
}

// ---- the lane-per-item kernel (lane_core.hpp): DOMINANT on HiFi batches -------------------------------------------------
// Persistent waves over groups of 64 items of the two lane classes (light items without / with the shift stage), one lane per
// item, every wave with its own LDS slice of capw dwords.
constexpr int LANE_WAVES = 4;
#ifndef PLO_LANE_WPE
#define PLO_LANE_WPE 3
#endif
#ifndef PLO_LANE_WPE_MIN
#define PLO_LANE_WPE_MIN PLO_LANE_WPE
#endif
#ifndef PLO_LANE_G_WPE
#define PLO_LANE_G_WPE 2  // k_lift_lanes_g: the windows' bookkeeping on top of 168 registers would spill; 12 KB of LDS per wave anyway
#endif
constexpr int LANE_G_WAVES = 4;
template <bool SP, bool STATS, bool H16>
PLO_DEV void lift_lanes_kernel(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t n0, uint32_t n1, uint32_t gs, int capw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int w = threadIdx.x >> 6;
    // XCD-aware placement as in lift_tiles_kernel: neighbouring groups -- reads over the same stretch of a contig -- share an L2
    const uint32_t nb = gridDim.x, per = nb >> 3, b = blockIdx.x;
    const uint32_t tb = (per > 0 && (nb & 7u) == 0) ? (b & 7u) * per + (b >> 3) : b;
    const uint32_t tw = blockDim.x >> 6;
    const uint32_t wave = tb * tw + (uint32_t)w, n_waves = nb * tw;
    WaveCtx ctx;
    if (wk.slab_pre) {
        ctx.slab_base = (unsigned long long)wave * SLAB_OPS;
        ctx.slab_left = SLAB_OPS;
    }
    // (the ticket counter of the context's next launch: not in use during this one)
    if (wk.lane_ticket_next && b == 0u && threadIdx.x == 0u) *wk.lane_ticket_next = 0u;
    const int kvs_n = wk.lane_kvs ? (int)wk.lane_kvs : LANE_KVS;
    lane_tiles_persistent<SP, false, STATS, H16>(ix, bt, wk, stages, wave, n_waves, n0, n1, gs, (uint32_t *)smem + (size_t)w * (size_t)(capw + 2 * kvs_n), capw, ctx, 0u, kvs_n);
    wave_ctx_flush(wk, ctx, wave);
}
#define PLO_LANE_KERNEL(name, SP_, STATS_, H16_)                                                                                                             \
    __global__ __launch_bounds__(LANE_WAVES * 64) __attribute__((amdgpu_waves_per_eu(PLO_LANE_WPE_MIN, PLO_LANE_WPE))) void name(                             \
        DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t n0, uint32_t n1, uint32_t gs, int capw, const uint32_t *totals_dev) {                   \
        if (totals_dev) { /* (the one-round-trip path: the class counts are on the device only) */                                                             \
            n0 = totals_dev[0];                                                                                                                                 \
            n1 = totals_dev[1];                                                                                                                                 \
        }                                                                                                                                                       \
        lift_lanes_kernel<SP_, STATS_, H16_>(ix, bt, wk, stages, n0, n1, gs, capw);                                                                             \
    }
PLO_LANE_KERNEL(k_lift_lanes, false, false, false)        // production: no statistics counters in the loops
PLO_LANE_KERNEL(k_lift_lanes_stats, false, true, false)   // plo_ctx_set_stats / PLO_LANE_STATS=1: algo_bytes and lane_utilisation counted
PLO_LANE_KERNEL(k_lift_lanes_sp, true, false, false)      // sparse read bases (PLO_SEQ_BAM4_SPARSE)
// 16-bit ops in the regions (lane_core.hpp, H16; PLO_LANE_H16=1, stage sets with the liftover): measured in round 6, 5-10 % slower than the 32-bit
// regions at every geometry tried (EXPERIMENTS 6.4) -- the conversions and the chunk tests cost more instructions than the halved LDS buys
PLO_LANE_KERNEL(k_lift_lanes16, false, false, true)
PLO_LANE_KERNEL(k_lift_lanes16_stats, false, true, true)
#undef PLO_LANE_KERNEL

// The same lane-per-item code for HEAVY items (too heavy for an LDS region: indel-dense or very long CIGARs), every lane's region in
// wave-private global scratch and reached through per-lane LDS windows (lane_core.hpp, LaneWin); `per` items per wave.
// A wave runs as long as its longest item, at the pace of a lone dependent instruction chain (about 3.5 us per op of the item on
// the stress workload, 2.8 us with a SIMD to itself): the kernel's time hardly depends on the number of items until every
// resident wave has its 64, and the workgroup-per-item kernel is the faster one for fewer than some 70 k heavy items
// (lane_heavy_min).  Measured and dropped: the heavy classes sorted by weight (k_chunk_sort's idea without its windows), long
// groups paired with short ones on a SIMD -- 7 % slower at 100 k reads, 11 % at 250 k: neighbours in the batch share reference and
// block-map lines, and a group of items from all over the genome gives that up.  Nor did ordering whole GROUPS by the length of their
// longest item (items left where they are), long ones paired with short ones on a SIMD in workgroups of 8 waves: 9.68 against 9.85 ms
// at 100 k reads, and 8-wave workgroups cost 20 % at 250 k (19.7 against 16.3 ms with two 4-wave workgroups per CU).
template <bool SP>
PLO_DEV void lift_lanes_g_kernel(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t lo, uint32_t mid, uint32_t hi,
                                 uint32_t per, uint32_t *scratch, int stride) {
    const uint32_t k = threadIdx.x >> 6, n_waves = gridDim.x * LANE_G_WAVES;
    const uint32_t wave = blockIdx.x * LANE_G_WAVES + k;
    __shared__ uint32_t windows[LANE_G_WAVES][64 * LANE_WIN_DWORDS + LANE_KVS_DWORDS];
    WaveCtx ctx;
    lane_heavy_persistent<SP>(ix, bt, wk, stages, wave, n_waves, lo, mid, hi, per, windows[k], scratch + (size_t)wave * (size_t)per * (size_t)stride, stride, ctx);
    wave_ctx_flush(wk, ctx, wave);
}
__global__ __launch_bounds__(LANE_G_WAVES * 64) __attribute__((amdgpu_waves_per_eu(PLO_LANE_G_WPE, PLO_LANE_G_WPE))) void k_lift_lanes_g(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t lo,
                                                                                                     uint32_t mid, uint32_t hi, uint32_t per, uint32_t *scratch, int stride) {
    lift_lanes_g_kernel<false>(ix, bt, wk, stages, lo, mid, hi, per, scratch, stride);
}
// The same kernel at three waves per SIMD (168 VGPRs, 144 B of spills per lane; 3 x 53 KB of LDS windows are exactly a CU's): slower for a lone
// wave -- 10.0 against 9.5 ms at 100 k stress reads, where every resident wave has one group and the kernel takes as long as its longest item
// -- and faster once the waves have several groups each and the kernel is bound by issue throughput: 25.7 against 29.3 ms at 500 k reads.
// Chosen by the number of heavy items (liftover_core).
__global__ __launch_bounds__(LANE_G_WAVES * 64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_lift_lanes_g_w3(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t lo,
                                                                                                     uint32_t mid, uint32_t hi, uint32_t per, uint32_t *scratch, int stride) {
    lift_lanes_g_kernel<false>(ix, bt, wk, stages, lo, mid, hi, per, scratch, stride);
}
__global__ __launch_bounds__(LANE_G_WAVES * 64) __attribute__((amdgpu_waves_per_eu(PLO_LANE_G_WPE, PLO_LANE_G_WPE))) void k_lift_lanes_g_sp(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t lo,
                                                                                                        uint32_t mid, uint32_t hi, uint32_t per, uint32_t *scratch, int stride) {
    lift_lanes_g_kernel<true>(ix, bt, wk, stages, lo, mid, hi, per, scratch, stride);
}

// HEAVY items, streamed (lane_stream.hpp): the same stage code as a PIPELINE OF WAVES -- a workgroup is a team of three waves (left shift,
// liftover, simplify; two for the forward class) working on the same 64 item slots, the ops flowing from wave to wave through rings in
// LDS; a lane of the head wave takes the team's next item when it has finished one.  Taken by batches that run all stages.
// Teams [0, t0): the forward class, [t0, t0 + t1): the reverse class; more teams than the chip holds are started as others retire.
#ifndef PLO_PIPE_WPE
#define PLO_PIPE_WPE 4
#endif
#ifndef PLO_PIPE_NI
#define PLO_PIPE_NI 32  // entries of the IN ring per lane (>= refill + 4)
#endif
template <bool SP, int NI, int N1, int N2, int N3>
PLO_DEV void lift_stream_kernel(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t lo, uint32_t mid, uint32_t hi, uint32_t t0, uint32_t t1, uint32_t xcd) {
    __shared__ uint32_t rings[stream_lds_dwords(NI, N1, N2, N3)];
    uint32_t b = 0, e = 0;
    bool has_shift = false;
    // XCD-aware placement (as lift_lanes_kernel): workgroup w runs on XCD w % 8; teams that are neighbours in the class order -- reads over the
    // same stretch of a contig, the same reference and block-map lines -- get workgroups of one XCD, i.e. one L2 (PLO_PIPE_XCD=1; off by default: measured slower)
    uint32_t team = blockIdx.x;
    if (xcd) {
        const uint32_t nb = gridDim.x, per = nb >> 3;
        if (team < 8u * per) team = (team & 7u) * per + (team >> 3);
    }
    pipe_team_span(team, t0, t1, lo, mid, hi, b, e, has_shift);
    WaveCtx ctx;
    pipe_team<SP, NI, N1, N2, N3>(ix, bt, wk, b, e, has_shift, rings, ctx);
    wave_ctx_flush(wk, ctx, blockIdx.x * PIPE_WAVES + (uint32_t)wv::wave_id());
}
__global__ __launch_bounds__(PIPE_WAVES * 64) __attribute__((amdgpu_waves_per_eu(PLO_PIPE_WPE, PLO_PIPE_WPE))) void k_lift_stream(DevIndex ix, DevBatch bt, DevWork wk, uint32_t lo, uint32_t mid, uint32_t hi, uint32_t t0, uint32_t t1, uint32_t xcd) {
    lift_stream_kernel<false, PLO_PIPE_NI, 16, 16, 32>(ix, bt, wk, lo, mid, hi, t0, t1, xcd);
}
__global__ __launch_bounds__(PIPE_WAVES * 64) __attribute__((amdgpu_waves_per_eu(PLO_PIPE_WPE, PLO_PIPE_WPE))) void k_lift_stream_sp(DevIndex ix, DevBatch bt, DevWork wk, uint32_t lo, uint32_t mid, uint32_t hi, uint32_t t0, uint32_t t1, uint32_t xcd) {
    lift_stream_kernel<true, PLO_PIPE_NI, 16, 16, 32>(ix, bt, wk, lo, mid, hi, t0, t1, xcd);
}

// Items of tiles (or of the lane kernel) whose intermediates overflowed the shared capacity: the tile code again, RETRY_PER
// items per wave with a larger LDS slice (retry_cap)
constexpr uint32_t RETRY_PER = 1;
template <bool SP>
PLO_DEV void lift_retry_kernel(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t n_retry, int big_thresh, int cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    TileMem m = carve_tile_mem(smem, cap);
    WaveCtx ctx;
    Coop<1> co;
    if (n_retry == 0xffffffffu) n_retry = (uint32_t)wk.counters[CNT_NRETRY];  // as the tile kernel left it (this kernel hands on to big_list)
    for (uint32_t r = blockIdx.x * RETRY_PER; r < n_retry; r += gridDim.x * RETRY_PER) {
        uint32_t left = n_retry - r;
        lift_tile<1, SP>(co, ix, bt, wk, stages, r, (int)(left < RETRY_PER ? left : RETRY_PER), m, wk.retry_list, LEVEL_RETRY, big_thresh, ctx);
        wv::sync();
    }
    wave_ctx_flush(wk, ctx, blockIdx.x);
}
__global__ __launch_bounds__(64) void k_lift_retry(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t n_retry,
                                                   int big_thresh, int cap) {
    lift_retry_kernel<false>(ix, bt, wk, stages, n_retry, big_thresh, cap);
}
__global__ __launch_bounds__(64) void k_lift_retry_sp(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t n_retry,
                                                      int big_thresh, int cap) {
    lift_retry_kernel<true>(ix, bt, wk, stages, n_retry, big_thresh, cap);
}

// One workgroup of NW waves per item (Coop<NW>): the item's op stream, temporaries and block-map window live in the
// workgroup's LDS (cap elements), every pass walks it NW x 64 elements at a time.  Persistent workgroups over `list`.
constexpr int MID_CAPK = 512;  // staged block-map entries of the one item (4 KB); longer windows are read from global memory
// 128 VGPRs at most: 16 waves per CU, as one workgroup of 16 or two of 8
template <int NW, bool SP>
PLO_DEV void lift_mid_kernel(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t n_list, int mid_thresh, int cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    TileMem m = carve_tile_mem(smem, cap, MID_CAPK);
    Coop<NW> co;
    co.w = wv::wave_id();
    co.xch = (int *)(smem + ((tile_mem_bytes(cap, MID_CAPK) + 15) & ~(size_t)15));
    if (threadIdx.x < (unsigned)Coop<NW>::XCH_INTS) co.xch[threadIdx.x] = 0;
    __syncthreads();
    WaveCtx ctx;
    for (uint32_t i = blockIdx.x; i < n_list; i += gridDim.x) {
        lift_tile<NW, SP>(co, ix, bt, wk, stages, i, 1, m, wk.big_list, LEVEL_MID, mid_thresh, ctx);
        co.sync();
    }
    wave_ctx_flush(wk, ctx, blockIdx.x * NW + (uint32_t)co.w);
}
template <int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_lift_mid(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t n_list,
                                                      int mid_thresh, int cap) {
    lift_mid_kernel<NW, false>(ix, bt, wk, stages, n_list, mid_thresh, cap);
}
template <int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_lift_mid_sp(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t n_list,
                                                         int mid_thresh, int cap) {
    lift_mid_kernel<NW, true>(ix, bt, wk, stages, n_list, mid_thresh, cap);
}
template <int NW>
static size_t mid_lds_bytes(int cap) {
    return ((tile_mem_bytes(cap, MID_CAPK) + 15) & ~(size_t)15) + (size_t)Coop<NW>::XCH_INTS * 4;
}

template <bool SP>
PLO_DEV void lift_big_kernel(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t n_big, const uint32_t *list,
                             unsigned char *scratch, int big_cap, unsigned long long bytes_per_wave) {
    TileMem m = carve_tile_mem(scratch + (unsigned long long)blockIdx.x * bytes_per_wave, big_cap);
    WaveCtx ctx;
    Coop<1> co;
    for (uint32_t i = blockIdx.x; i < n_big; i += gridDim.x) {
        lift_tile<1, SP>(co, ix, bt, wk, stages, i, 1, m, list, LEVEL_LAST, 0, ctx);
        wv::sync();
    }
    wave_ctx_flush(wk, ctx, blockIdx.x);
}
__global__ __launch_bounds__(64) void k_lift_big(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t n_big,
                                                 const uint32_t *list, unsigned char *scratch, int big_cap,
                                                 unsigned long long bytes_per_wave) {
    lift_big_kernel<false>(ix, bt, wk, stages, n_big, list, scratch, big_cap, bytes_per_wave);
}
__global__ __launch_bounds__(64) void k_lift_big_sp(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, uint32_t n_big,
                                                    const uint32_t *list, unsigned char *scratch, int big_cap,
                                                    unsigned long long bytes_per_wave) {
    lift_big_kernel<true>(ix, bt, wk, stages, n_big, list, scratch, big_cap, bytes_per_wave);
}

// Sparse bases (PLO_SEQ_BAM4_SPARSE): the items whose probes reached absent granules are lifted again from the complete bases of
// their reads, which the host gathers from plo_batch_in::seq_full.  k_miss_info tells it which reads; k_miss_patch points the
// items' sequence offsets (a copy of the descriptor column) into the side buffer with those bases.
__global__ void k_miss_info(const uint32_t *list, uint32_t n, DevBatch bt, DevWork wk, uint32_t *out_read, uint32_t *out_len) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t rd = bt.seg_read[wk.item_seg[list[k]]];
    out_read[k] = rd;
    out_len[k] = bt.read_seq_len[rd];
}
__global__ void k_miss_patch(const uint32_t *list, uint32_t n, const uint64_t *vals, uint64_t *seq_off) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) seq_off[list[k]] = vals[k];
}

// sums (and clears) the per-wave statistic slots of the lift kernels that have run since the last call into the batch counters
__global__ __launch_bounds__(256) void k_sum_stats(unsigned long long *ws, uint32_t n_slots, unsigned long long *counters) {
    __shared__ unsigned long long acc[5];
    if (threadIdx.x < 5) acc[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long a[5] = {0, 0, 0, 0, 0};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += gridDim.x * blockDim.x) {
        unsigned long long *w = ws + (size_t)i * STAT_WORDS;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            a[k] += w[k];
            w[k] = 0;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) a[k] += (unsigned long long)__shfl_xor((long long)a[k], d, 64);
        if ((threadIdx.x & 63u) == 0) atomicAdd(&acc[k], a[k]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&counters[CNT_ALGO_BYTES], acc[0]);
        atomicAdd(&counters[CNT_IN_OPS], acc[1]);
        atomicAdd(&counters[CNT_OUT_OPS], acc[2]);
        atomicAdd(&counters[CNT_LANE_ACT], acc[3]);
        atomicAdd(&counters[CNT_LANE_TRIPS], acc[4]);
    }
}

// The one-round-trip path's last launch: k_lift_retry and k_sum_stats in one (a command of any size costs ~5 us on the stream, and a
// reference-sized window's call is made of a dozen of them).  Every wave lifts its share of the retry list as k_lift_retry does, then adds
// what it counted straight into the batch counters (nothing to add for the common wave without a retry item); the first SUM_BLOCKS waves
// also sum (and clear) the statistic slots the light-item kernel's waves left -- complete by stream order, `n_lane_slots` of them from slot 0.
constexpr uint32_t SUM_BLOCKS = 32;
__global__ __launch_bounds__(64) void k_lift_retry_sum(DevIndex ix, DevBatch bt, DevWork wk, uint32_t stages, int big_thresh, int cap, uint32_t n_lane_slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    TileMem m = carve_tile_mem(smem, cap);
    WaveCtx ctx;
    Coop<1> co;
    const uint32_t n_retry = (uint32_t)wk.counters[CNT_NRETRY];
    for (uint32_t r = blockIdx.x * RETRY_PER; r < n_retry; r += gridDim.x * RETRY_PER) {
        uint32_t left = n_retry - r;
        lift_tile<1, false>(co, ix, bt, wk, stages, r, (int)(left < RETRY_PER ? left : RETRY_PER), m, wk.retry_list, LEVEL_RETRY, big_thresh, ctx);
        wv::sync();
    }
    // this wave's own counts, per lane as wave_ctx_flush reads them; the slots of the light-item kernel on top (lane l of wave b: slots
    // b + SUM_BLOCKS (l + 64 j))
    unsigned long long a[5] = {ctx.algo_bytes, ctx.in_ops, ctx.out_ops, 0ull, 0ull};
    const uint32_t lane = (uint32_t)wv::lane();
    if (lane == 0) {
        a[3] = ctx.u_act;
        a[4] = ctx.u_trips;
    }
    if (blockIdx.x < SUM_BLOCKS) {
        for (uint32_t i = blockIdx.x + SUM_BLOCKS * lane; i < n_lane_slots; i += SUM_BLOCKS * 64u) {
            unsigned long long *w = wk.wave_stats + (size_t)i * STAT_WORDS;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                a[k] += w[k];
                w[k] = 0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) a[k] += (unsigned long long)__shfl_xor((long long)a[k], d, 64);
    }
    if (lane == 0) {
        if (a[0]) atomicAdd(&wk.counters[CNT_ALGO_BYTES], a[0]);
        if (a[1]) atomicAdd(&wk.counters[CNT_IN_OPS], a[1]);
        if (a[2]) atomicAdd(&wk.counters[CNT_OUT_OPS], a[2]);
        if (a[3]) atomicAdd(&wk.counters[CNT_LANE_ACT], a[3]);
        if (a[4]) atomicAdd(&wk.counters[CNT_LANE_TRIPS], a[4]);
    }
}

// ---- record finishing (finish_core.hpp) ----------------------------------------------------------------------------------
__global__ void k_finish_items(DevBatch bt, DevWork wk, DevFinish f) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < wk.n_items) finish_item(bt, wk, f, i);
}
__global__ void k_finish_reads(DevBatch bt, DevWork wk, DevFinish f) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < bt.n_reads) finish_read(bt, wk, f, r);
}
__global__ void k_finish_offsets(DevBatch bt, DevWork wk, DevFinish f) {
    uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t n = wk.n_items;
    if (e >= n + bt.n_reads) return;
    uint64_t so = f.su[e] ? (uint64_t)f.soff[e] * 16u : PLO_NO_FLIP;
    uint64_t qo = f.qu[e] ? (uint64_t)f.qoff[e] * 16u : PLO_NO_FLIP;
    if (f.su[e]) f.flist[f.frank[e]] = e;
    if (e < n) {
        f.item_seq_off[e] = so;
        f.item_qual_off[e] = qo;
    } else {
        f.read_seq_off[e - n] = so;
        f.read_qual_off_out[e - n] = qo;
    }
}
// dense re-packing of the slab-allocated output CIGARs: eight lanes per item copy 32 contiguous bytes per step
__global__ __launch_bounds__(256) void k_compact_cigar(const uint32_t *src, uint64_t *cig_off, const uint32_t *cig_len,
                                                       const uint32_t *dense_off, uint32_t n, uint32_t *dst) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t i = t >> 3, sub = t & 7u;
    if (i >= n) return;
    const uint64_t from = cig_off[i];  // read by all eight lanes before lane 0 overwrites it below
    const uint32_t len = cig_len[i], to = dense_off[i];
    for (uint32_t k = sub; k < len; k += 8) dst[to + k] = src[from + k];
    if (sub == 0) cig_off[i] = to;
}

// SA tag text: thread per item (only the few items of reads with several lifted records produce text)
__global__ void k_sa_len(DevWork wk, DevSa sa) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < wk.n_items) sa.len[i] = sa_item_len(wk, sa, i);
}
__global__ void k_sa_emit(DevWork wk, DevSa sa) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < wk.n_items) sa_item_emit(wk, sa, i);
}
// reverse_alignment_seq_and_qual: one workgroup per record that needs it, streaming 16-byte-aligned outputs.
// HBM-bound: per flipped read L/2 + L bytes in, the same out.
__global__ __launch_bounds__(256) void k_revcomp(DevBatch bt, DevWork wk, DevFinish f) {
    uint32_t n = wk.n_items, n_flip = f.frank[n + bt.n_reads];
    for (uint32_t k = blockIdx.x; k < n_flip; k += gridDim.x) {
        uint32_t e = f.flist[k];
        uint32_t read = e < n ? f.item_read[e] : e - n;
        revcomp_record(bt, f, read, f.rev_seq + (uint64_t)f.soff[e] * 16u, f.rev_qual + (uint64_t)f.qoff[e] * 16u, (int)threadIdx.x,
                       (int)blockDim.x);
    }
}

// ---- output records (records_core.hpp) -----------------------------------------------------------------------------------
// plan: a wave per read (the aux walk looks for a string's NUL 64 bytes per step)
__global__ __launch_bounds__(256) void k_rec_plan(DevBatch bt, DevWork wk, DevRecords d) {
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r < bt.n_reads) records_plan_read(bt, wk, d, r);  // (wave-uniform)
}
// the 64-bit exclusive scans of the reads' bytes (blockIdx.y 0), record counts (1) and unmapped copies (2): a wave per 512 values
__global__ __launch_bounds__(64) void k_rec_scan_sums(const unsigned long long *in, uint32_t n, uint32_t nb, unsigned long long *partial) {
    rec_scan_sums(in + (size_t)blockIdx.y * n, n, blockIdx.x, partial + (size_t)blockIdx.y * nb);
}
__global__ __launch_bounds__(64) void k_rec_scan_partials(unsigned long long *partial, uint32_t n, uint32_t nb, unsigned long long *out) {
    rec_scan_partials(partial + (size_t)blockIdx.x * nb, nb, out + (size_t)blockIdx.x * ((size_t)n + 1) + n);
}
__global__ __launch_bounds__(64) void k_rec_scan_apply(const unsigned long long *in, uint32_t n, uint32_t nb, const unsigned long long *partial, unsigned long long *out) {
    rec_scan_apply(in + (size_t)blockIdx.y * n, n, blockIdx.x, partial + (size_t)blockIdx.y * nb, out + (size_t)blockIdx.y * ((size_t)n + 1));
}
// emit: a workgroup per read at a time.  HBM-bound: per 15 kb record ~22.5 kB in, the same out.  VEC false: the plain byte copy (A/B)
template <bool VEC, bool EQX>
__global__ __launch_bounds__(256) void k_rec_emit(DevBatch bt, DevWork wk, DevRecords d) {
    // EQX false: the kernel of a context without a plo_eqx_dev result.  That its CIGARs are the lift's is known when it is compiled, and its
    // code is what it was before the two fields existed (120 VGPRs, 4 waves per SIMD); choosing the CIGAR at run time in the one kernel
    // made it 141 VGPRs and 3 waves, and records_ms without a result 2.05 ms where it had been 1.82 (EXPERIMENTS 16.5)
    if (!EQX) {
        d.item_eqx_off = nullptr;
        d.eqx_ops = nullptr;
    }
    for (uint32_t r = blockIdx.x; r < bt.n_reads; r += gridDim.x) records_emit_read<VEC>(bt, wk, d, r, (int)threadIdx.x, (int)blockDim.x);
}

// ---- NM:i of the lifted records (nm_core.hpp) ------------------------------------------------------------------------------
// persistent waves, items by ticket.  HBM-bound by design: per lifted item l_seq / 2 bytes of bases, ~l_seq bytes of reference, 4 x ops
__global__ __launch_bounds__(256) void k_nm(DevBatch bt, DevWork wk, DevNm d) { nm_items(bt, wk, d); }

// ---- MD:Z of the lifted records (md_core.hpp) ------------------------------------------------------------------------------
// the same persistent waves, twice over the same bytes: the lengths of the items' texts, then (behind the 64-bit scan) the texts
__global__ __launch_bounds__(256) void k_md_count(DevBatch bt, DevWork wk, DevMd d) { md_items<false>(bt, wk, d); }
__global__ __launch_bounds__(256) void k_md_emit(DevBatch bt, DevWork wk, DevMd d) { md_items<true>(bt, wk, d); }

// ---- = / X CIGARs of the lifted records (eqx_core.hpp) ---------------------------------------------------------------------
// the same persistent waves, twice over the same bytes: the op counts of the items' CIGARs, then (behind the 64-bit scan) the ops
__global__ __launch_bounds__(256) void k_eqx_count(DevBatch bt, DevWork wk, DevEqx d) { eqx_items<false>(bt, wk, d); }
__global__ __launch_bounds__(256) void k_eqx_emit(DevBatch bt, DevWork wk, DevEqx d) { eqx_items<true>(bt, wk, d); }

// ---- the window's records in coordinate order (sort_core.hpp) -------------------------------------------------------------
// check + keys + the tile sort in LDS (12 KB), a merge launch per doubling of the runs, the lengths in sorted order, and (behind the
// 64-bit scan) the permuted copy, a wave per 16 KB of output -- the only stage that touches the records' bytes
__global__ __launch_bounds__(256) void k_sort_keys(DevSort d) {
    __shared__ unsigned long long lk[SORT_TILE];
    __shared__ uint32_t li[SORT_TILE];
    sort_tile(d, blockIdx.x, lk, li);
}
__global__ __launch_bounds__(256) void k_sort_merge(const unsigned long long *sk, const uint32_t *si, unsigned long long *dk, uint32_t *di, uint32_t n, uint32_t run) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g < n) sort_merge_pair(sk, si, dk, di, n, run, g);
}
__global__ __launch_bounds__(256) void k_sort_gather(const uint32_t *perm, const unsigned long long *len, unsigned long long *slen, uint32_t n) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < n) slen[j] = len[perm[j]];
}
__global__ __launch_bounds__(256) void k_sort_copy(DevSort d, const uint32_t *perm, unsigned long long n_chunks) {
    if (*d.err != SORT_NO_RECORD) return;  // a refused window: no byte is moved
    const unsigned long long chunk = (unsigned long long)blockIdx.x * 4u + (unsigned long long)wv::wave_id();
    if (chunk < n_chunks) sort_copy_chunk(d, perm, chunk, wv::lane(), 64);  // (wave-uniform)
}

// ---- sorted windows merged into large runs (merge_core.hpp): no LDS anywhere, the runs arrive sorted ---------------------------------------
// check + keys (a thread per record), a rank launch per doubling of the groups of runs, the lengths in merged order, and (behind the 64-bit
// scan) the chunk table by one lane.  The emit -- a wave per 16 KB of the chunk's output -- is the only kernel that touches the records' bytes
__global__ __launch_bounds__(256) void k_merge_keys(DevMerge d) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (g < d.n) merge_key_record(d, (uint32_t)g);
}
__global__ __launch_bounds__(256) void k_merge_rank(DevMerge d, const unsigned long long *sk, const uint32_t *ss, unsigned long long *dk, uint32_t *ds, uint32_t t) {
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p < d.n) merge_rank_pair(d, sk, ss, dk, ds, t, (uint32_t)p);
}
__global__ __launch_bounds__(256) void k_merge_gather(DevMerge d, const uint32_t *src) {
    const unsigned long long j = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (j < d.n) merge_gather(d, src, (uint32_t)j);
}
__global__ __launch_bounds__(64) void k_merge_chunks(DevMerge d, const unsigned long long *key) {
    if (threadIdx.x == 0) merge_chunks(d, key);
}
__global__ __launch_bounds__(256) void k_merge_copy(DevMergeEmit d, unsigned long long n_pieces) {
    const unsigned long long w = (unsigned long long)blockIdx.x * 4u + (unsigned long long)wv::wave_id(), nw = (unsigned long long)gridDim.x * 4u;
    if (w < n_pieces) merge_copy_piece(d, w, wv::lane(), 64);  // (wave-uniform)
    merge_rebase(d, w * 64u + (unsigned long long)wv::lane(), nw * 64u);
}

// ---- index entries of the sorted records (index_core.hpp): a wave per record, the records grid-strided over the waves; no LDS
__global__ __launch_bounds__(256) void k_index(DevBai d) { index_records(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }

// ---- depth of the records (depth_core.hpp): no LDS anywhere, no kernel waits on another workgroup -----------------------------------------
// check and add: a wave per record, the records grid-strided over the waves.  The add is bound by its scattered atomics, one lane a cache line
__global__ __launch_bounds__(256) void k_depth_check(DevDepth d) { depth_check_records(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }
__global__ __launch_bounds__(256) void k_depth_add(DevDepth d) { depth_add_records(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }
// the scan: a wave per tile of PLO_DEPTH_TILE entries.  HBM-bound by design: the array is read by the sums, read and written by the apply
__global__ __launch_bounds__(256) void k_depth_sums(const int32_t *a, unsigned long long n, unsigned long long n_tiles, int32_t *sums) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 4u + (unsigned long long)wv::wave_id();
    if (t < n_tiles) depth_tile_sum(a, n, t, sums);  // (wave-uniform)
}
__global__ __launch_bounds__(256) void k_depth_apply(int32_t *a, unsigned long long n, unsigned long long n_tiles, const int32_t *incl) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 4u + (unsigned long long)wv::wave_id();
    if (t < n_tiles) depth_tile_scan(a, n, t, incl);
}
__global__ __launch_bounds__(64) void k_depth_top(int32_t *a, unsigned long long n) { depth_top_scan(a, n); }
__global__ __launch_bounds__(256) void k_depth_windows(DevDepthWin d) {
    depth_windows(d, (unsigned long long)blockIdx.x * 4u + (unsigned long long)wv::wave_id(), (unsigned long long)gridDim.x * 4u);
}
template <bool EMIT>
__global__ __launch_bounds__(256) void k_depth_runs(DevDepthRuns d, unsigned long long n_tiles) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 4u + (unsigned long long)wv::wave_id();
    if (t < n_tiles) depth_runs_tile<EMIT>(d, t);
}

// ---- allele pileup (pileup_core.hpp): no LDS anywhere, no kernel waits on another workgroup -------------------------------------------------
// a wave per record for the check and the add; the add's cost is its scattered atomics, one per event
__global__ __launch_bounds__(256) void k_pileup_check(DevPileup d) { pileup_check_records(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }
__global__ __launch_bounds__(256) void k_pileup_add(DevPileup d) { pileup_add_records(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }
// a wave per tile of PLO_PILEUP_TILE bases.  HBM-bound by design: the array is read once by the count and once by the emit
template <bool EMIT>
__global__ __launch_bounds__(256) void k_pileup_sites(DevPileupSites d, unsigned long long n_tiles) {
    const unsigned long long t = (unsigned long long)blockIdx.x * 4u + (unsigned long long)wv::wave_id();
    if (t < n_tiles) pileup_sites_tile<EMIT>(d, t);  // (wave-uniform)
}

// ---- the reference FASTA (fasta_core.hpp): a wave per tile of FA_TILE bytes, the tiles grid-strided over the waves; no LDS.  HBM-bound by
// design: the piece is read by k_fa_lines, k_fa_count and k_fa_emit (k_fa_headers leaves the tiles without a header line alone), the bases
// are written once
__global__ __launch_bounds__(256) void k_fa_lines(DevFasta d) { fa_lines_tiles(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }
__global__ __launch_bounds__(64) void k_fa_states(DevFasta d) { fa_states(d); }
__global__ __launch_bounds__(256) void k_fa_count(DevFasta d) { fa_tiles<0, false>(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }
__global__ __launch_bounds__(256) void k_fa_headers(DevFasta d) { fa_tiles<1, false>(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }
template <bool VEC>
__global__ __launch_bounds__(256) void k_fa_emit(DevFasta d) { fa_tiles<2, VEC>(d, blockIdx.x * 4u + (uint32_t)wv::wave_id(), gridDim.x * 4u); }

// ---- the liftover batch (batch_core.hpp) -----------------------------------------------------------------------------------
// the label table: a thread per contig name
__global__ __launch_bounds__(256) void k_bb_table(DevBatchBuild d) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < d.n_contigs) bb_table_insert(d, c);
}
// plan: a wave per read (the SA text is cut 64 bytes per step, a CIGAR text parsed with a lane per op)
__global__ __launch_bounds__(256) void k_bb_plan(DevBatchBuild d) {
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r < d.n_reads) batch_plan_read(d, r);  // (wave-uniform)
}
// emit: a wave per read at a time
__global__ __launch_bounds__(256) void k_bb_emit(DevBatchBuild d) {
    const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = gridDim.x * (blockDim.x >> 6);
    for (uint32_t r = w; r < d.n_reads; r += nw) batch_emit_read(d, r);
}

// ---- the window cut (window_core.hpp) -------------------------------------------------------------------------------------------
// guess: a wave per segment behind the first (segment 0 starts at offset 0)
__global__ __launch_bounds__(256) void k_cut_guess(DevCut d) {
    const uint32_t s = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (s == 0 && wv::lane() == 0) d.guess[0] = 0;
    if (s >= 1 && s < d.n_seg) cut_guess_segment(d, s);  // (wave-uniform)
}
// walk / find / emit: a lane per segment -- 64 independent chains per wave keep 64 loads in flight where one chain has one
__global__ __launch_bounds__(64) void k_cut_walk(DevCut d) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < d.n_seg) (void)cut_walk_segment(d, s, d.guess[s], true);
}
__global__ __launch_bounds__(64) void k_cut_resolve(DevCut d) { cut_resolve(d); }
__global__ __launch_bounds__(64) void k_cut_find(DevCut d) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < d.n_seg) cut_find_segment(d, s);
}
__global__ void k_cut_result(DevCut d) { cut_result(d); }
__global__ __launch_bounds__(64) void k_cut_emit(DevCut d) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < d.n_seg) cut_emit_segment(d, s);
}
// the unmapped records side by side: a workgroup per record at a time, 16-byte stores
// the first record of a part (window_core.hpp): a wave takes tiles of candidates by ticket, in ascending order, until one lies above a find
__global__ __launch_bounds__(256) void k_part_start(DevPart d) {
    for (;;) {
        unsigned long long t = 0;
        if (wv::lane() == 0) t = wv::atomic_add_global(d.res + PS_TICKET, 1ull);
        t = wv::bcast_first(t);
        if (t >= d.n_tiles || !part_start_tile(d, t)) return;  // (wave-uniform)
    }
}
__global__ __launch_bounds__(256) void k_cut_copy(DevCut d) {
    for (unsigned long long u = blockIdx.x; u < d.n_unmapped; u += gridDim.x) cut_copy_unmapped(d, u, (int)threadIdx.x, (int)blockDim.x);
}

// ---- BGZF inflate (inflate.hpp): every block of a chunk of the BAM stream at once, one wave per block ----------------------
struct BgzfBlk {
    unsigned long long coff, uoff;  // offsets of the block's deflate data / inflated bytes inside the chunk buffers
    uint32_t clen, ulen;
};
struct InfWave {  // wave primitives of the decoder's I/O policy (InfWaveIO, inflate.hpp)
    PLO_DEV int lane() const { return wv::lane(); }
    PLO_DEV void sync() const {  // LDS windows / tables and the wave's own global stores (far match sources) are ordered for all its lanes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) expcnt(0) lgkmcnt(0): the write-backs of the ring have reached L2
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    PLO_DEV uint32_t uniform(uint32_t v) const { return wv::bcast_first(v); }
    PLO_DEV uint32_t scalar(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    PLO_DEV uint32_t read_lane(uint32_t v, uint32_t l) const {  // l wave-uniform
        return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane((int)l));
    }
    PLO_DEV int popcount64(unsigned long long v) const { return __builtin_popcountll(v); }
    PLO_DEV uint32_t rank_below(unsigned long long mask) const {  // set bits of mask below this lane
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    }
    PLO_DEV long long clock() const { return wv::clock(); }
    // a byte this wave wrote back earlier: read at device scope (L2), never from a line the CU's vector cache fetched while the
    // line was still being filled
    PLO_DEV uint8_t load_written(const uint8_t *p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
struct InfLds {
    InfWork ws;
    InfWaveMem io;
};
// Four waves per workgroup, each on its own block with its own LDS: the workgroup's waves sit on the four SIMDs of the CU, which
// one-wave workgroups do not (the decoder is bound by instruction issue once a SIMD holds several of them).
constexpr int INF_WAVES = 4;
__global__ __launch_bounds__(INF_WAVES * 64) void k_bgzf_inflate(const uint8_t *comp, const BgzfBlk *blks, uint32_t n, uint8_t *out, int *status) {
    __shared__ InfLds lds_all[INF_WAVES];  // 4 x 15.9 KB: two workgroups, eight blocks in flight per CU
    InfLds &lds = lds_all[wv::wave_id()];
    InfWaveIO<InfWave> io;
    io.m = &lds.io;
    for (uint32_t b = blockIdx.x * INF_WAVES + (uint32_t)wv::wave_id(); b < n; b += gridDim.x * INF_WAVES) {
        const BgzfBlk k = blks[b];
        uint32_t w = 0;
#ifdef PLO_INF_TIMING
        const long long tb = wv::clock();
#endif
        int rc = k.ulen ? inflate_block(io, comp + k.coff, k.clen, out + k.uoff, k.ulen, lds.ws, &w) : 0;
#ifdef PLO_INF_TIMING
        if (b == 7 && wv::lane() == 0)
            printf("[inflate] block %u: %u -> %u bytes, %lld cycles: input chunks %d (%lld), write-backs %d (%lld), matches %d (%lld), far %d (%lld), tables %d (%lld), literals in runs %d (%lld)\n", b, k.clen, k.ulen,
                   wv::clock() - tb, io.n_load, io.t_load, io.n_flush, io.t_flush, io.n_match, io.t_match, io.n_far, io.t_far, io.n_table, io.t_table, io.n_run, io.t_run);
#endif
        if (rc == 0 && w != k.ulen) rc = -9;  // the stream ended before ISIZE bytes
        if (wv::lane() == 0) status[b] = rc;
        io.sync();
    }
}

// The CRC-32 of every inflated block against the one its BGZF trailer carries (crc32_wave, inflate.hpp: a wave per block), behind
// k_bgzf_inflate on the same stream: the host then never reads the inflated bytes to check them (round 4: the CRC pass and the copy of the
// compressed bytes out of the file mapping were 50 of the 63 ms a 470 MB refill took).  status: -10 where the CRC differs.
__global__ __launch_bounds__(INF_WAVES * 64) void k_bgzf_crc(const uint8_t *out, const BgzfBlk *blks, uint32_t n, const uint32_t *crcs, int *status) {
    __shared__ uint32_t tab[256];
    tab[threadIdx.x & 255u] = crc32_table_entry(threadIdx.x & 255u);
    __syncthreads();
    for (uint32_t b = blockIdx.x * INF_WAVES + (uint32_t)wv::wave_id(); b < n; b += gridDim.x * INF_WAVES) {
        const BgzfBlk k = blks[b];
        const uint32_t c = k.ulen ? crc32_wave(out + k.uoff, k.ulen, tab) : 0u;
        if (wv::lane() == 0 && k.ulen && status[b] == 0 && c != crcs[b]) status[b] = -10;
    }
}

// ---- BGZF deflate (deflate.hpp): the output records of a window as finished BGZF blocks, one wave per block ----------------------
struct DefWave {  // what the encoder needs beyond plo_wave.hpp
    PLO_DEV void gsync() const {  // LDS and the wave's own global stores (its tokens) are ordered for all its lanes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    // a token this wave stored earlier: read at device scope (L2), the buffer is reused from block to block
    PLO_DEV uint32_t load_written(const uint16_t *p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// Four waves per workgroup, each on its own block with its own 10.8 KB of LDS (as k_bgzf_inflate: the waves of a workgroup sit on the
// four SIMDs of the CU): 44.2 KB per workgroup, three workgroups = twelve blocks in flight per CU.  Persistent: the waves stride over the
// blocks, so the token buffers are sized by the grid, not by the number of blocks.  size[b] = bytes of block b in its slot (0 on an error).
constexpr int DEF_WAVES = 4;
__global__ __launch_bounds__(DEF_WAVES * 64) void k_bgzf_deflate(const uint8_t *in, unsigned long long n_bytes, uint32_t n, int level, uint8_t *slots,
                                                                 unsigned long long *size, uint16_t *tokens, unsigned *err) {
    __shared__ DefWork ws_all[DEF_WAVES];
    __shared__ uint32_t tab[256];
    tab[threadIdx.x & 255u] = crc32_table_entry(threadIdx.x & 255u);
    __syncthreads();
    DefWork &ws = ws_all[wv::wave_id()];
    const uint32_t wave = blockIdx.x * DEF_WAVES + (uint32_t)wv::wave_id();
    uint16_t *tok = tokens + (size_t)wave * DEF_TOK_UNITS;
    DefWave prim;
    for (uint32_t b = wave; b < n; b += gridDim.x * DEF_WAVES) {
        const unsigned long long at = (unsigned long long)b * DEF_MAX_IN;
        const uint32_t len = (uint32_t)(n_bytes - at < DEF_MAX_IN ? n_bytes - at : DEF_MAX_IN);
        uint32_t sz = 0;
        const int rc = bgzf_deflate_block(prim, ws, tab, in + at, len, slots + (size_t)b * DEF_SLOT, DEF_SLOT, level, tok, &sz);
        if (wv::lane() == 0) {
            size[b] = rc == DEF_OK ? sz : 0;
            if (rc != DEF_OK) wv::atomic_add_global(err, 1u);
        }
        prim.gsync();
    }
}
// the slots' blocks side by side: a workgroup per block at a time, 16-byte stores (copy_span, records_core.hpp)
__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t *slots, const unsigned long long *off, uint32_t n, uint8_t *dense) {
    for (uint32_t b = blockIdx.x; b < n; b += gridDim.x)
        copy_span<true>(dense + off[b], slots + (size_t)b * DEF_SLOT, off[b + 1] - off[b], (int)threadIdx.x, (int)blockDim.x);
}

// ---- self-test of the wave primitives (plo_selftest) -------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_selftest(const int *in, int *out) {
    int lane = wv::lane();
    int x = in[lane];
    out[0 * 64 + lane] = wv::scan_add(x);
    out[1 * 64 + lane] = wv::scan_max(x);
    out[2 * 64 + lane] = wv::shfl_up1(x, -7);
    out[3 * 64 + lane] = wv::shfl(x, (lane * 7 + 3) & 63);
    out[4 * 64 + lane] = wv::bcast_last(x);
    out[5 * 64 + lane] = wv::bcast_first(x);
    wv::MinPlus f;
    f.a = in[64 + lane];
    f.b = in[128 + lane];
    f.s = in[192 + lane];
    wv::MinPlus F = wv::scan_minplus(f);
    out[6 * 64 + lane] = F.a;
    out[7 * 64 + lane] = F.b;
    out[8 * 64 + lane] = F.s;
    unsigned long long bm = wv::ballot((x & 1) != 0);
    out[9 * 64 + lane] = (int)((bm >> lane) & 1ull);
    Coop<1> co;
    AddScan as(co);
    MaxScan ms(co, -1);
    int a0 = as.excl(x & 15), a1 = as.excl((x >> 4) & 15);
    int m0 = ms.incl((x & 3) == 0 ? lane : -1);
    int e0 = ms.excl_of(m0);
    int m1 = ms.incl((x & 3) == 1 ? 64 + lane : -1);
    int e1 = ms.excl_of(m1);
    out[10 * 64 + lane] = a0;
    out[11 * 64 + lane] = a1;
    out[12 * 64 + lane] = e0;
    out[13 * 64 + lane] = e1;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const {
        return (T *)p;
    }
};

struct HostBuf {  // pinned
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const {
        return (T *)p;
    }
};

// what a count / scan / emit pass over the lifted items keeps (plo_md_dev, plo_eqx_dev; aln_pass_run)
struct AlnPass {
    DevBuf len, off, partial;  // [n] the items' lengths, [n + 1] their exclusive scan, the scan's block sums
    DevBuf out;                // what the emit pass writes
    DevBuf blk;                // err_item, the count pass's ticket, the emit pass's ticket
    HostBuf h;                 // blk's words, and the total behind them
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void release() {
        for (DevBuf *b : {&len, &off, &partial, &out, &blk}) b->release();
        h.release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace

struct plo_index {
    int device = 0;
    PackedIndex host;  // host copy of the packed arrays (plo_index_segment_map, validation)
    DevIndex d{};
    std::vector<void *> owned;  // device allocations owned by the index
    uint32_t max_segs_per_contig = 0;
};

// plo_fasta_*: the loader of the reference FASTA (fasta_core.hpp).  An object of its own: it exists before any index does.
struct plo_fasta {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // count pass, header table, emit
    bool emit_timed = false;  // ev[4], ev[5] are recorded and not yet read
    bool byte_stores = false;  // PLO_FASTA_BYTESTORES=1: k_fa_emit<false>, every base a store of its own (the A/B of EXPERIMENTS 17.3)
    std::string err;
    FaHost h;
    DevBuf text, tile_fn, tile_state, cnt, start, partial, blk, hdr, dest;
    HostBuf h_blk, h_hdr, h_dest;
    uint8_t *out = nullptr;
    size_t out_cap = 0;
    float ms = 0.f;
    bool finished = false;
    std::vector<int64_t> o_len;
    std::vector<const uint8_t *> o_ptr;
    std::vector<void *> adopted;
};

// plo_depth_*: the depth array of a list of chromosomes (depth_core.hpp).  An object of its own: several contexts add to it.
struct plo_depth {
    int device = 0;
    uint32_t n_ref = 0;
    uint32_t exclude_flags = PLO_DEPTH_EXCLUDE_DEFAULT;
    int count_del = 0;
    std::atomic<bool> finished{false};
    std::vector<int32_t> ref_len;
    std::vector<uint64_t> slot_off;  // [n_ref + 1]
    unsigned long long n_entries = 0, n1 = 0, n2 = 0;  // entries, their tiles, the tiles of the tiles' sums
    DevBuf arr, d_ref_len, d_slot_off, s1, s2, win_first, win_sum, run_cnt, run_start, run_partial, runs;
    HostBuf h_win;  // win_first [n_ref + 1], then the sums
    size_t bytes() const {
        size_t b = 0;
        for (const DevBuf *x : {&arr, &d_ref_len, &d_slot_off, &s1, &s2, &win_first, &win_sum, &run_cnt, &run_start, &run_partial, &runs}) b += x->cap;
        return b;
    }
};

// plo_pileup_*: the allele counters of a list of chromosomes or of a region of each (pileup_core.hpp).  An object of its own, like plo_depth
struct plo_pileup {
    int device = 0;
    uint32_t n_ref = 0;
    uint32_t exclude_flags = PLO_DEPTH_EXCLUDE_DEFAULT;
    std::vector<int32_t> ref_len, slot_beg, slot_end;
    std::vector<uint64_t> slot_off;  // [n_ref + 1], in bases
    unsigned long long n_bases = 0;
    DevBuf arr, d_ref_len, d_slot_off, d_slot_beg, d_slot_end, site_cnt, site_start, site_partial, sites;
    size_t bytes() const {
        size_t b = 0;
        for (const DevBuf *x : {&arr, &d_ref_len, &d_slot_off, &d_slot_beg, &d_slot_end, &site_cnt, &site_start, &site_partial, &sites}) b += x->cap;
        return b;
    }
};

struct plo_ctx {
    const plo_index *ix = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // workspace
    DevBuf f_flag, f_bin, f_end, f_prim, f_isoff, f_iqoff, f_iread, f_nl, f_pitem, f_uflag, f_rsoff, f_rqoff, f_su, f_qu, f_soff,
        f_qoff, f_rseq, f_rqual, f_fflag, f_frank, f_flist, sa_len, sa_off, sa_text, r_plan, r_size, r_start, r_partial, r_recoff, r_out, r_err;
    DevBuf z_slots, z_size, z_off, z_partial, z_tok, z_out, z_err;  // plo_bgzf_compress_dev: buffers of its own
    // plo_batch_build_dev: buffers of its own (the label table, plan and scans, the segments in text order, the batch's arrays)
    DevBuf bb_table, bb_plan, bb_size, bb_start, bb_partial, bb_kind, bb_err, bb_tkey, bb_tnops, bb_tctext, bb_tclen, bb_tcontig, bb_tdst, bb_tpos, bb_tfwd,
        bb_rev, bb_len, bb_soff, bb_qoff, bb_flags, bb_sread, bb_scontig, bb_spos, bb_sfwd, bb_coff, bb_cigar;
    // plo_window_cut_dev / plo_bgzf_inflate_dev: buffers of their own
    DevBuf wc_guess, wc_land, wc_cnt, wc_start, wc_partial, wc_fire, wc_res, wc_recoff, wc_unmoff, wc_unmsrc, wc_unm, ci_comp, ci_blk, ci_st, ps_res;
    HostBuf h_rec, h_bgzf, h_bb, h_wc, h_ci;
    hipEvent_t wev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t iev[2] = {nullptr, nullptr};
    hipEvent_t zev[2] = {nullptr, nullptr};
    hipEvent_t bev[4] = {nullptr, nullptr, nullptr, nullptr};
    DevWork last_wk{};
    DevBatch last_bt{};
    bool have_last = false, have_finish = false, have_sa = false;
    bool have_nm = false;  // plo_nm_dev's result of the current batch: plo_records_build_dev writes NM:i from it; dropped by the next lift / finish
    DevBuf nm_out, nm_blk;
    HostBuf h_nm;
    hipEvent_t nev[2] = {nullptr, nullptr};
    bool have_md = false;  // plo_md_dev's result of the current batch: plo_records_build_dev writes MD:Z from it and cuts the source's MD; dropped like have_nm
    AlnPass md;            // (out: the text)
    bool have_eqx = false;  // plo_eqx_dev's result of the current batch: plo_records_build_dev writes its = / X CIGARs in place of the lift's; dropped like have_nm
    AlnPass eqx;            // (out: the ops)
    // plo_records_sort_dev: buffers of its own (the sorted copy of the window's bytes, two (key, index) arrays, lengths, offsets)
    DevBuf so_key[2], so_idx[2], so_len, so_slen, so_off, so_partial, so_out, so_blk;
    HostBuf h_so;
    hipEvent_t sev[2] = {nullptr, nullptr};
    // plo_runs_merge_plan_dev / _emit_dev: the plan (two (key, g) arrays, runs, lengths, offsets, the tables) and the current chunk
    DevBuf mg_key[2], mg_src[2], mg_runof, mg_len, mg_mlen, mg_off, mg_partial, mg_runs, mg_first, mg_blk, mg_cfirst, mg_coff, mg_out, mg_ooff;
    HostBuf h_mg, h_mg_tab;
    hipEvent_t gev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool have_plan = false;
    int mg_cur = 0;
    uint32_t mg_n = 0, mg_n_chunks = 0;
    std::vector<uint32_t> mg_chunk_first;
    std::vector<uint64_t> mg_chunk_off;
    // plo_records_index_dev: the entries and its two words (lowest offender << 4 | kind, n_placed)
    DevBuf bai_entry, bai_blk;
    HostBuf h_bai;
    hipEvent_t xev[2] = {nullptr, nullptr};
    // plo_depth_add_dev: the plan word of every record and the call's two words (lowest offender << 4 | kind, n_counted); dpev: every plo_depth_* call.
    // plo_pileup_add_dev and plo_pileup_sites_dev take the same scratch and events (a context runs one call at a time; the add's block holds n_events too)
    DevBuf dp_plan, dp_blk;
    HostBuf h_dp;
    hipEvent_t dpev[2] = {nullptr, nullptr};
    bool rec_bytecopy = false;  // PLO_RECORDS_BYTECOPY=1: plo_records_build_dev moves every byte on its own (k_rec_emit<false>, the A/B of the 16-byte copy)
    hipEvent_t rev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    DevBuf item_region, lane_groups;
    DevBuf misc, whist, cls_partial, lane_scratch, item_cls, retry_list, perm, nin_p, seg_reflen, seg_readlen, seg_nm, seg_cnt, seg_off, scan_partial, item_seg, item_cseg, item_nin, op_prefix, counters, big_list, huge_list, scratch, tile_lo, verr, miss_list, miss_info, miss_vals, miss_seq_off, miss_side;
    DevBuf d_n_m, d_in_off, d_n_in, d_pos1, d_w0, d_w1, d_kv0, d_kv1, d_flags, d_contig, d_seq_len, d_seq_off, d_shift_ref, d_shift_ref_len,
        d_chrom_ref, d_chrom_ref_len, d_read_len;
    // outputs (device)
    DevBuf o_status, o_flip, o_mapq, o_chrom, o_pos, o_coff, o_clen, o_cigar, o_dense_off, o_cigar_dense, wave_stats;
    DevBuf fast_blk;  // liftover_fast: class totals, validation flags and batch counters in one block (one fill, one copy back)
    bool fast_timing = false;  // the last batch took liftover_fast: events 0, 1, 4 only
    bool scan_chain = false;   // liftover_fast: the segments' item offsets by k_scan_chain (PLO_SCAN_CHAIN=1; measured slower than the three scan launches)
    bool fast_fuse = true;     // liftover_fast: the counters' sum inside the retry launch (k_lift_retry_sum; PLO_FAST_FUSE=0: k_lift_retry + k_sum_stats)
    bool phase_events = true;  // liftover_fast records events 0, 1, 4 around its phases (plo_ctx_set_phase_events; every record is a ~5 us bubble on the stream)
    bool fast_no_events = false;  // the last batch took liftover_fast without them: plo_ctx_timing reports no times for it
    // host staging for plo_liftover_batch
    DevBuf i_read_rev, i_read_len, i_read_off, i_seq, i_seg_read, i_seg_contig, i_seg_pos, i_seg_fwd, i_seg_coff, i_cigar,
        i_item_seg, i_item_cseg;
    HostBuf h_item_seg, h_item_cseg, h_status, h_flip, h_mapq, h_chrom, h_pos, h_coff, h_clen, h_cigar, h_counters, h_miss, h_side;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // plo_liftover_batch uploads the read bases on a stream of their own: the enumerate pass does not look at them, so that copy
    // (most of the batch's bytes) runs under it; the first lift kernel waits for ev_seq
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_seq = nullptr;
    hipEvent_t ev_cls = nullptr;  // class totals copied to the host (k_permute2 runs behind it)
    bool seq_pending = false;
    bool ev_big = false, ev_mid = false;
    uint64_t dense_total = 0;
    plo_timing timing{};
    unsigned long long phase_cycles[12] = {0};
    // tuning
    // cap sets the LDS slice of a wave (34 B per element + 1.25 KB): 320 -> 12,160 B -> 3 four-wave blocks = 12 waves per CU,
    // which is also what the kernel's VGPR budget allows; measured on MI355X (wgs30x, 2M reads): cap 512 (8 waves/CU) 8.34 ms,
    // cap 384 (still 2 blocks) 8.33 ms, cap 320 6.26 ms, cap 256 6.27 ms + overflow items.
    int window = 256, big_thresh = 176, cap = 320;
    bool adaptive = true;  // geometry chosen per batch (off when any of PLO_WINDOW / PLO_BIG_THRESH / PLO_CAP is set)
    int n_cus = 256;
    int tile_waves = TILE_WAVES;
    bool small_window_tight = false;  // the 256-element slice re-ran too many items with the wide window: keep 64 elements of allowance
    // lane-per-item kernel (lane_core.hpp): items up to lane_max_w (item_weight) take it, 64 per wave, every wave with an LDS
    // slice of lane_capw dwords; heavier items take the wave-cooperative kernels below.  (Round 1's first attempt at one lane
    // per item -- 36 KB of LDS per wave, synchronous probes -- was a net loss and had been removed; this is a different kernel.)
    int lane_max_w = 192;
    int lane_capw = 3072;
    bool lane_sort = true;  // k_chunk_sort before the lane kernel
    // groups of the lane kernel dealt dynamically (lane_tiles_persistent): two ticket counters used in turn (a launch zeroes the next one's),
    // the rounds every wave takes by fixed slots first (PLO_LANE_STATIC; < 0: fixed slots only)
    DevBuf lane_ticket;
    uint32_t lane_epoch = 0;
    int lane_static_rounds = 0;  // 0: by the launch's rounds (lane_ticket_arm); > 0: that many; < 0: fixed slots only
    int lane_tail_rounds = 1;  // PLO_LANE_TAIL: rounds' worth of cheap groups (no shift stage) dealt last (0: classes one to one)
    int lane_kvs = LANE_KVS;  // block-map entries staged per wave (PLO_LANE_KVS: 64 .. LANE_KVS_MAX)
    bool lane_lockstep = true;  // PLO_LANE_LOCKSTEP=0: the shift stage walks every item event by event (lane_core.hpp; A/B runs of the lockstep loop)
    bool lane_h16 = false;    // PLO_LANE_H16=1: 16-bit regions (k_lift_lanes16; stage sets with the liftover)
    bool lane_stats = false;  // PLO_LANE_STATS=1: the light-item kernel that counts algorithmic bytes and lane utilisation (k_lift_lanes_stats)
    int lane_sort_window = LANE_SORT_WINDOW;
    // groups cut by LDS budget inside larger sort windows (k_chunk_sort, lane_groups_cut): on for batches whose groups are of 64
    bool lane_budget = false;  // (measured, MI355X, wgs30x 2 M reads: 1.42 ms with windows of 512 against 1.29 ms with fixed groups in windows of 128 -- DESIGN.md section 6)
    int lane_budget_window = 512;
    bool lane_stream = true;       // heavy items of all-stage batches through the streaming kernel (lane_stream.hpp)
    // the one-round-trip path (liftover_fast): what the last batch of this context left -- the segments / items its arrays are sized for, its
    // class counts, whether it had heavy items (a context that sees windows of one shape lifts them without asking the device for counts)
    bool fast = true;
    uint32_t fast_ns_cap = 0, fast_item_cap = 0, fast_n0 = 0, fast_n1 = 0;
    uint32_t fast_ref_items = 0, fast_ref_ns = 0;  // items and segments of the last careful batch: the one-round-trip path's launch bound
    bool fast_launch_bound = true;                 // (PLO_FAST_LAUNCH_BOUND=0: grids by the arrays' capacity whatever the batch's size)
    uint32_t item_cap_now = 0;   // items the per-item arrays hold
    uint32_t fast_extra_syncs = 0;  // a fast attempt that fell back: its round trip counts in the call's host_syncs
    bool fast_light_only = false;
    uint32_t lane_groups_cap = 0;  // groups the list of the budget-cut groups has room for (set with the list, attempt 0 of a batch)
    // k_lift_lanes_g (heavy items through the lane-per-item code, regions in global scratch behind LDS windows): lane_heavy_min >= 0 = for
    // batches with at least that many heavy items; < 0 (default) = by lane_heavy_ratio, see the routing in liftover_core (0: never).
    // Stress workload, heavy items -> k_lift_mid / k_lift_lanes_g: 20 k 2.8 / 7.9 ms, 60 k 8.0 / 9.6 ms, 80 k 10.5 / 9.6 ms,
    // 100 k 13.1 / 9.9 ms, 250 k 32.5 / 16-20 ms.
    int lane_heavy_min = -1;
    int lane_heavy_ratio = 50000;
    int lane_stream_ratio = 30000;  // the same for the streaming kernel (PLO_LANE_STREAM_RATIO)
    // workgroup-per-item kernel for the items a shared tile cannot hold (k_lift_mid): waves per workgroup (8 or 16; 0 = off,
    // such items then run one wave each from global scratch) and the largest LDS capacity in elements
    int mid_waves = 16;
    int mid_cap_max = 4096;
};

#define HIP_TRY(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t _e = (call);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(_e);                     \
            return (_e == hipErrorOutOfMemory) ? PLO_ERR_OUT_OF_MEMORY : PLO_ERR_HIP;           \
        }                                                                                       \
    } while (0)

static thread_local std::string g_index_err;

template <class T>
static hipError_t upload(std::vector<void *> &owned, const std::vector<T> &v, const T **out) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    owned.push_back(p);
    if (!v.empty()) {
        e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    }
    *out = (const T *)p;
    return hipSuccess;
}

// ---- plo_nm_dev, plo_md_dev, plo_eqx_dev: the walks of aln_walk.hpp --------------------------------------------------------------

// their entry: `out` cleared, the result of an earlier call dropped, and the checks they share.  fn: the function's name; bases_use: what it
// does with the bases, for the message about their format
template <class Out>
static plo_status aln_enter(plo_ctx *c, const plo_batch_in *in, Out *out, bool plo_ctx::*have, const char *fn, const char *bases_use) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->err_item = UINT32_MAX;
    c->err.clear();
    c->*have = false;
    auto fail = [&](plo_status s, const std::string &text) -> plo_status {
        c->err = std::string(fn) + ": " + text;
        return s;
    };
    if (c->have_last && c->last_bt.seq_fmt != PLO_SEQ_BAM4)
        return fail(PLO_ERR_INVALID_ARG, std::string("the batch came with sparse or ASCII bases; ") + bases_use + " complete BAM 4-bit bases (PLO_SEQ_BAM4)");
    if (!c->have_last || c->last_bt.n_segs != in->n_segs || c->last_bt.n_reads != in->n_reads)
        return fail(PLO_ERR_INVALID_ARG, "no lift result of this batch on the context: call plo_liftover_batch_dev on it first");
    if (!c->have_finish) return fail(PLO_ERR_INVALID_ARG, "no finishing result on the context: call plo_finish_batch_dev on the batch first (the reversed bases are its)");
    const DevIndex &ix = c->ix->d;
    if (!ix.chrom_seq || !ix.chrom_len || !ix.n_chroms) return fail(PLO_ERR_INVALID_ARG, "the index has no chrom_seq");
    if (c->last_wk.n_items > (uint32_t)NM_NO_ITEM) return fail(PLO_ERR_RANGE, "more than 2^31 - 1 items in one batch");
    HIP_TRY(c, hipSetDevice(c->ix->device));
    return PLO_OK;
}

// item `item` was refused by the walk; result: what is not handed out
static plo_status aln_refused(plo_ctx *c, const char *fn, const char *result, uint32_t item, uint32_t *err_item) {
    *err_item = item;
    c->err = std::string(fn) + ": the CIGAR of item " + std::to_string(item) + " consumes more reference than its chromosome has behind item_ref_pos, or more bases than its read has; no " + result + " is handed out";
    return PLO_ERR_RANGE;
}

// the source fields of a DevNm, DevMd or DevEqx from the context
static void aln_src(const plo_ctx *c, AlnSrc &s) {
    const DevIndex &ix = c->ix->d;
    s = AlnSrc{c->f_isoff.as<uint64_t>(), c->f_rseq.as<uint8_t>(), ix.chrom_seq, ix.chrom_len, ix.n_chroms};
}

// as many waves as stay resident (82 to 89 VGPRs: five per SIMD, five workgroups of four per CU), never more than items
static uint32_t aln_grid(const plo_ctx *c, uint32_t n) { return std::min<uint32_t>((n + 3) / 4, (uint32_t)c->n_cus * 5u); }

// count(nblk), the 64-bit scan of the lengths, a wait for the total and the refusal, room(total), emit(nblk), a wait behind it (the event
// time).  Two waits.  d: DevMd or DevEqx with its source filled; count and emit launch their kernel with it, room makes room for `total`
// and points d's emit fields at it.
template <class D, class Count, class Room, class Emit>
static plo_status aln_pass_run(plo_ctx *c, AlnPass &ps, D &d, const char *fn, const char *result, uint32_t *err_item, float *ms, uint64_t *total_out, Count count, Room room, Emit emit) {
    const uint32_t n = c->last_wk.n_items;
    hipStream_t st = c->stream;
    for (int i = 0; i < 4; ++i)
        if (!ps.ev[i]) HIP_TRY(c, hipEventCreate(&ps.ev[i]));
    const uint32_t nb = std::max(1u, (n + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK);
    HIP_TRY(c, ps.len.ensure((size_t)std::max(1u, n) * 8));
    HIP_TRY(c, ps.off.ensure(((size_t)n + 1) * 8));
    HIP_TRY(c, ps.partial.ensure((size_t)nb * 8));
    HIP_TRY(c, ps.blk.ensure(16));
    HIP_TRY(c, ps.h.ensure(32));
    d.item_len = ps.len.as<unsigned long long>();
    d.err_item = ps.blk.as<int>();
    d.ticket = ps.blk.as<unsigned>() + 1;
    unsigned long long *off = ps.off.as<unsigned long long>(), *partial = ps.partial.as<unsigned long long>();
    uint32_t *h = ps.h.as<uint32_t>();
    h[0] = (uint32_t)NM_NO_ITEM;
    h[1] = h[2] = h[3] = 0;
    h[4] = h[5] = 0;
    HIP_TRY(c, hipMemcpyAsync(ps.blk.p, h, 16, hipMemcpyHostToDevice, st));
    const uint32_t nblk = aln_grid(c, n);
    HIP_TRY(c, hipEventRecord(ps.ev[0], st));
    if (n) {
        count(nblk);
        hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.item_len, n, nb, partial);
        hipLaunchKernelGGL(k_rec_scan_partials, dim3(1), dim3(64), 0, st, partial, n, nb, off);
        hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.item_len, n, nb, (const unsigned long long *)partial, off);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h + 4, off + n, 8, hipMemcpyDeviceToHost, st));
    } else {
        HIP_TRY(c, hipMemsetAsync(ps.off.p, 0, 8, st));
    }
    HIP_TRY(c, hipEventRecord(ps.ev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, ps.blk.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h[0] != (uint32_t)NM_NO_ITEM) return aln_refused(c, fn, result, h[0], err_item);
    const uint64_t total = (uint64_t)h[4] | ((uint64_t)h[5] << 32);
    HIP_TRY(c, room(total));
    d.ticket = ps.blk.as<unsigned>() + 2;
    HIP_TRY(c, hipEventRecord(ps.ev[2], st));
    if (n) {
        emit(nblk);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(ps.ev[3], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, ps.ev[0], ps.ev[1]);
    (void)hipEventElapsedTime(&b, ps.ev[2], ps.ev[3]);
    *ms = a + b;
    *total_out = total;
    return PLO_OK;
}

extern "C" {

const char *plo_version(void) { return "portello-liftover-mi355x 0.1 (gfx950)"; }
uint32_t plo_api_version(void) { return PLO_API_VERSION; }

plo_status plo_index_create(const plo_index_desc *desc, int device, plo_index **out) {
    if (!desc || !out) return PLO_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PLO_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return PLO_ERR_NO_DEVICE;
    plo_index *ix = new plo_index();
    ix->device = device;
    std::string err;
    plo_status st = pack_index(desc, ix->host, err, /*build_kv=*/false);
    if (st != PLO_OK) {
        g_index_err = err;
        delete ix;
        return st;
    }
    for (uint32_t c = 0; c < desc->n_contigs; ++c)
        ix->max_segs_per_contig = std::max(ix->max_segs_per_contig, ix->host.contig_seg_off[c + 1] - ix->host.contig_seg_off[c]);
    auto fail = [&](plo_status s) {
        for (void *p : ix->owned) (void)hipFree(p);
        delete ix;
        return s;
    };
    DevIndex &d = ix->d;
    const PackedIndex &h = ix->host;
    {   // block maps: built on the device from the contig->reference CIGARs
        uint32_t ns = desc->n_segments;
        std::vector<uint32_t> cg(desc->seg_cigar, desc->seg_cigar + (ns ? desc->seg_cigar_off[ns] : 0));
        std::vector<uint32_t> cgoff(desc->seg_cigar_off, desc->seg_cigar_off + (ns ? ns + 1 : 0));
        if (!ns) cgoff.assign(1, 0);
        std::vector<int64_t> spos(desc->seg_pos, desc->seg_pos + ns);
        std::vector<void *> tmp;
        const uint32_t *d_cg = nullptr, *d_cgoff = nullptr;
        const int64_t *d_pos = nullptr;
        const int *d_cnt = nullptr;
        std::vector<int> cnt(std::max(1u, ns), 0);
        auto drop_tmp = [&]() {
            for (void *p : tmp) (void)hipFree(p);
        };
        if (upload(tmp, cg, &d_cg) != hipSuccess || upload(tmp, cgoff, &d_cgoff) != hipSuccess || upload(tmp, spos, &d_pos) != hipSuccess ||
            upload(tmp, cnt, &d_cnt) != hipSuccess) {
            drop_tmp();
            return fail(PLO_ERR_HIP);
        }
        if (ns) hipLaunchKernelGGL(k_map_build, dim3(std::min<uint32_t>(ns, 65535u * 16u)), dim3(64), 0, 0, d_cg, d_cgoff, d_pos, ns, (const uint32_t *)nullptr,
                                   (KV *)nullptr, (int *)d_cnt);
        if (hipMemcpy(cnt.data(), d_cnt, cnt.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            drop_tmp();
            return fail(PLO_ERR_HIP);
        }
        ix->host.cs_kv_off.assign(ns + 1, 0);
        for (uint32_t g = 0; g < ns; ++g) {
            if (cnt[g] < 0) {
                g_index_err = "contig segment coordinate outside the 31-bit BAM range or invalid CIGAR op code";
                drop_tmp();
                return fail(PLO_ERR_RANGE);
            }
            ix->host.cs_kv_off[g + 1] = ix->host.cs_kv_off[g] + (uint32_t)cnt[g];
        }
        if (upload(ix->owned, h.cs_kv_off, &d.cs_kv_off) != hipSuccess) {
            drop_tmp();
            return fail(PLO_ERR_HIP);
        }
        void *kvp = nullptr;
        if (hipMalloc(&kvp, std::max<size_t>((size_t)h.cs_kv_off[ns] * sizeof(KV), 16)) != hipSuccess) {
            drop_tmp();
            return fail(PLO_ERR_OUT_OF_MEMORY);
        }
        ix->owned.push_back(kvp);
        d.kv = (const KV *)kvp;
        if (ns) hipLaunchKernelGGL(k_map_build, dim3(std::min<uint32_t>(ns, 65535u * 16u)), dim3(64), 0, 0, d_cg, d_cgoff, d_pos, ns, d.cs_kv_off, (KV *)kvp,
                                   (int *)nullptr);
        hipError_t e = hipDeviceSynchronize();
        drop_tmp();
        if (e != hipSuccess) return fail(PLO_ERR_HIP);
    }
    if (upload(ix->owned, h.cs_chrom, &d.cs_chrom) != hipSuccess) return fail(PLO_ERR_HIP);
    if (upload(ix->owned, h.cs_is_fwd, &d.cs_is_fwd) != hipSuccess) return fail(PLO_ERR_HIP);
    if (upload(ix->owned, h.cs_mapq, &d.cs_mapq) != hipSuccess) return fail(PLO_ERR_HIP);
    if (upload(ix->owned, h.cs_start, &d.cs_start) != hipSuccess) return fail(PLO_ERR_HIP);
    if (upload(ix->owned, h.cs_end, &d.cs_end) != hipSuccess) return fail(PLO_ERR_HIP);
    if (upload(ix->owned, h.contig_seg_off, &d.contig_seg_off) != hipSuccess) return fail(PLO_ERR_HIP);
    if (upload(ix->owned, h.contig_len, &d.contig_len) != hipSuccess) return fail(PLO_ERR_HIP);
    if (upload(ix->owned, h.chrom_len, &d.chrom_len) != hipSuccess) return fail(PLO_ERR_HIP);
    d.n_contigs = desc->n_contigs;
    d.n_segments = desc->n_segments;
    d.n_chroms = desc->n_chroms;
    // sequences: copied from the host or borrowed from the device
    std::vector<const uint8_t *> chrom_ptr(desc->n_chroms, nullptr), rev_ptr(desc->n_contigs, nullptr);
    for (uint32_t c = 0; c < desc->n_chroms; ++c) {
        const uint8_t *src = desc->chrom_seq[c];
        if (!src && desc->chrom_len[c] > 0) return fail(PLO_ERR_INVALID_ARG);
        if (desc->seq_mem == PLO_MEM_DEVICE) {
            chrom_ptr[c] = src;
        } else {
            void *p = nullptr;
            size_t bytes = std::max<size_t>((size_t)desc->chrom_len[c], 16);
            if (hipMalloc(&p, bytes) != hipSuccess) return fail(PLO_ERR_OUT_OF_MEMORY);
            ix->owned.push_back(p);
            if (desc->chrom_len[c] > 0 && hipMemcpy(p, src, (size_t)desc->chrom_len[c], hipMemcpyHostToDevice) != hipSuccess)
                return fail(PLO_ERR_HIP);
            chrom_ptr[c] = (const uint8_t *)p;
        }
    }
    for (uint32_t c = 0; c < desc->n_contigs; ++c) {
        const uint8_t *src = desc->rev_contig_seq ? desc->rev_contig_seq[c] : nullptr;
        if (!src) continue;
        if (desc->seq_mem == PLO_MEM_DEVICE) {
            rev_ptr[c] = src;
        } else {
            void *p = nullptr;
            size_t bytes = std::max<size_t>((size_t)desc->contig_len[c], 16);
            if (hipMalloc(&p, bytes) != hipSuccess) return fail(PLO_ERR_OUT_OF_MEMORY);
            ix->owned.push_back(p);
            if (desc->contig_len[c] > 0 && hipMemcpy(p, src, (size_t)desc->contig_len[c], hipMemcpyHostToDevice) != hipSuccess)
                return fail(PLO_ERR_HIP);
            rev_ptr[c] = (const uint8_t *)p;
        }
    }
    if (upload(ix->owned, chrom_ptr, &d.chrom_seq) != hipSuccess) return fail(PLO_ERR_HIP);
    if (upload(ix->owned, rev_ptr, &d.contig_revseq) != hipSuccess) return fail(PLO_ERR_HIP);
    *out = ix;
    return PLO_OK;
}

void plo_index_destroy(plo_index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->device);
    for (void *p : ix->owned) (void)hipFree(p);
    delete ix;
}

// ---- plo_fasta_*: the reference FASTA (fasta_core.hpp) ---------------------------------------------------------------------------------
static thread_local std::string g_fasta_err;
#define FA_TRY(f, call)                                                                 \
    do {                                                                                \
        hipError_t _e = (call);                                                         \
        if (_e != hipSuccess) {                                                         \
            (f)->err = std::string(#call) + ": " + hipGetErrorString(_e);               \
            return (_e == hipErrorOutOfMemory) ? PLO_ERR_OUT_OF_MEMORY : PLO_ERR_HIP;   \
        }                                                                               \
    } while (0)

static void fasta_release(plo_fasta *f) {
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    for (DevBuf *b : {&f->text, &f->tile_fn, &f->tile_state, &f->cnt, &f->start, &f->partial, &f->blk, &f->hdr, &f->dest}) b->release();
    for (HostBuf *b : {&f->h_blk, &f->h_hdr, &f->h_dest}) b->release();
    if (f->out) (void)hipFree(f->out);
    for (void *p : f->adopted) (void)hipFree(p);
    for (hipEvent_t e : f->ev)
        if (e) (void)hipEventDestroy(e);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}

// the output allocation holds at least `need` bytes: a larger one takes over what the old one holds, the rest of it zero
static plo_status fasta_out_ensure(plo_fasta *f, size_t need) {
    if (need <= f->out_cap) return PLO_OK;
    const size_t cap = ((need + need / 2 + 65536) + 255) & ~(size_t)255;
    uint8_t *p = nullptr;
    FA_TRY(f, hipMalloc((void **)&p, cap));
    hipError_t e = hipMemsetAsync(p, 0, cap, f->stream);
    if (e == hipSuccess && f->out_cap) e = hipMemcpyAsync(p, f->out, f->out_cap, hipMemcpyDeviceToDevice, f->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        f->err = std::string("plo_fasta: growing the output: ") + hipGetErrorString(e);
        return PLO_ERR_HIP;
    }
    if (f->out) (void)hipFree(f->out);
    f->out = p;
    f->out_cap = cap;
    return PLO_OK;
}

static std::string fasta_refusal_text(const plo_fasta *f) {
    const FaHost &h = f->h;
    const std::string name = (h.err_kind >= FA_ERR_MISSING && h.err_chrom < h.want_name.size()) ? h.want_name[h.err_chrom] : std::string();
    switch (h.err_kind) {
    case FA_ERR_BAD_BYTE: return "reference fasta: the byte at offset " + std::to_string(h.err_offset) + " of a sequence line is neither a letter nor white space";
    case FA_ERR_NO_HEADER: return "reference fasta: the base at offset " + std::to_string(h.err_offset) + " stands in front of the first header line";
    case FA_ERR_MISSING: return "Chromosome \"" + name + "\" specified in the assembly-to-ref alignment file, but not in the reference fasta";
    case FA_ERR_LENGTH:
        return "Chromosome \"" + name + "\" specified with inconsistent length: " + std::to_string(h.want_len[h.err_chrom]) + " in the assembly-to-ref alignment file, and " +
               std::to_string(h.err_len) + " in the reference fasta";
    case FA_ERR_DUPLICATE: return "Chromosome \"" + name + "\" has a second header line in the reference fasta, at offset " + std::to_string(h.err_offset) + " (the first copy has length " + std::to_string(h.err_len) + ")";
    }
    return std::string();
}

// one piece of at most FA_MAX_PIECE bytes
static plo_status fasta_piece(plo_fasta *f, const uint8_t *text, uint32_t n) {
    hipStream_t st = f->stream;
    const uint32_t nt = (n + FA_TILE - 1) / FA_TILE, nb = (nt + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK;
    FA_TRY(f, f->text.ensure(((size_t)n + 15) & ~(size_t)15));
    FA_TRY(f, f->tile_fn.ensure((size_t)nt * 4));
    FA_TRY(f, f->tile_state.ensure(((size_t)nt + 1) * 4));
    FA_TRY(f, f->cnt.ensure((size_t)nt * 16));
    FA_TRY(f, f->start.ensure(((size_t)nt + 1) * 16));
    FA_TRY(f, f->partial.ensure((size_t)nb * 16));
    FA_TRY(f, f->blk.ensure(16));
    FA_TRY(f, f->h_blk.ensure(64));
    DevFasta d;
    memset(&d, 0, sizeof(d));
    d.text = f->text.as<uint8_t>();
    d.n = n;
    d.n_tiles = nt;
    d.in_state = f->h.state;
    d.tile_fn = f->tile_fn.as<unsigned>();
    d.tile_state = f->tile_state.as<unsigned>();
    d.cnt = f->cnt.as<unsigned long long>();
    d.start = f->start.as<unsigned long long>();
    d.err = f->blk.as<int>();
    d.want_first_base = f->h.recs.empty() ? 1 : 0;
    d.out = f->out;
    // h_blk: [0, 1] the two offset words up; then [2, 3] their values, [4] the state behind the piece, [6 .. 9] the bases and header lines
    int *hb = f->h_blk.as<int>();
    hb[0] = hb[1] = FA_NONE;
    const dim3 grid(std::min(4096u, (nt + 3u) / 4u));
    FA_TRY(f, hipMemcpyAsync(f->text.p, text, n, hipMemcpyHostToDevice, st));
    FA_TRY(f, hipMemcpyAsync(f->blk.p, hb, 8, hipMemcpyHostToDevice, st));
    FA_TRY(f, hipEventRecord(f->ev[0], st));
    hipLaunchKernelGGL(k_fa_lines, grid, dim3(256), 0, st, d);
    hipLaunchKernelGGL(k_fa_states, dim3(1), dim3(64), 0, st, d);
    hipLaunchKernelGGL(k_fa_count, grid, dim3(256), 0, st, d);
    hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 2), dim3(64), 0, st, (const unsigned long long *)d.cnt, nt, nb, f->partial.as<unsigned long long>());
    hipLaunchKernelGGL(k_rec_scan_partials, dim3(2), dim3(64), 0, st, f->partial.as<unsigned long long>(), nt, nb, d.start);
    hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 2), dim3(64), 0, st, (const unsigned long long *)d.cnt, nt, nb, (const unsigned long long *)f->partial.as<unsigned long long>(), d.start);
    FA_TRY(f, hipGetLastError());
    FA_TRY(f, hipEventRecord(f->ev[1], st));
    FA_TRY(f, hipMemcpyAsync(hb + 2, f->blk.p, 8, hipMemcpyDeviceToHost, st));
    FA_TRY(f, hipMemcpyAsync(hb + 4, d.tile_state + nt, 4, hipMemcpyDeviceToHost, st));
    FA_TRY(f, hipMemcpyAsync(hb + 6, d.start + nt, 8, hipMemcpyDeviceToHost, st));
    FA_TRY(f, hipMemcpyAsync(hb + 8, d.start + (size_t)nt + 1 + nt, 8, hipMemcpyDeviceToHost, st));
    FA_TRY(f, hipStreamSynchronize(st));  // (everything of the pieces in front is through too: their emit, and the copy of their destinations)
    float ms = 0.f;
    if (f->emit_timed && hipEventElapsedTime(&ms, f->ev[4], f->ev[5]) == hipSuccess) f->ms += ms;
    f->emit_timed = false;
    if (hipEventElapsedTime(&ms, f->ev[0], f->ev[1]) == hipSuccess) f->ms += ms;
    unsigned long long n_bases = 0, n_hdr64 = 0;
    memcpy(&n_bases, hb + 6, 8);
    memcpy(&n_hdr64, hb + 8, 8);
    const uint32_t n_hdr = (uint32_t)n_hdr64;
    if (n_hdr) {  // (of a refused piece too: whether its lowest base stands in front of its first header line decides the kind)
        FA_TRY(f, f->hdr.ensure((size_t)n_hdr * sizeof(FaHeader)));
        FA_TRY(f, f->h_hdr.ensure((size_t)n_hdr * sizeof(FaHeader)));
        d.hdr = f->hdr.as<FaHeader>();
        FA_TRY(f, hipEventRecord(f->ev[2], st));
        hipLaunchKernelGGL(k_fa_headers, grid, dim3(256), 0, st, d);
        FA_TRY(f, hipGetLastError());
        FA_TRY(f, hipEventRecord(f->ev[3], st));
        FA_TRY(f, hipMemcpyAsync(f->h_hdr.p, f->hdr.p, (size_t)n_hdr * sizeof(FaHeader), hipMemcpyDeviceToHost, st));
        FA_TRY(f, hipStreamSynchronize(st));
        if (hipEventElapsedTime(&ms, f->ev[2], f->ev[3]) == hipSuccess) f->ms += ms;
    }
    std::vector<FaDest> dest;
    const bool emit = f->h.piece(text, n, f->h_hdr.as<FaHeader>(), n_hdr, n_bases, (unsigned)hb[4], hb[2], hb[3], dest);
    if (f->h.err_kind) {
        f->err = fasta_refusal_text(f);
        return PLO_ERR_DATA;
    }
    if (!emit) return PLO_OK;
    if (plo_status s = fasta_out_ensure(f, (size_t)f->h.out_bytes)) return s;
    FA_TRY(f, f->dest.ensure(dest.size() * sizeof(FaDest)));
    FA_TRY(f, f->h_dest.ensure(dest.size() * sizeof(FaDest)));
    memcpy(f->h_dest.p, dest.data(), dest.size() * sizeof(FaDest));
    d.dest = f->dest.as<FaDest>();
    d.out = f->out;
    FA_TRY(f, hipMemcpyAsync(f->dest.p, f->h_dest.p, dest.size() * sizeof(FaDest), hipMemcpyHostToDevice, st));
    FA_TRY(f, hipEventRecord(f->ev[4], st));
    if (f->byte_stores) hipLaunchKernelGGL(k_fa_emit<false>, grid, dim3(256), 0, st, d);
    else hipLaunchKernelGGL(k_fa_emit<true>, grid, dim3(256), 0, st, d);
    FA_TRY(f, hipGetLastError());
    FA_TRY(f, hipEventRecord(f->ev[5], st));
    f->emit_timed = true;
    return PLO_OK;
}

plo_status plo_fasta_create(const plo_fasta_want *want, uint64_t text_bytes_hint, int device, plo_fasta **out) {
    if (!out) return PLO_ERR_INVALID_ARG;
    *out = nullptr;
    if (want && want->n && (!want->names || !want->lens)) {
        g_fasta_err = "plo_fasta_want: names and lens are required";
        return PLO_ERR_INVALID_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return PLO_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return PLO_ERR_NO_DEVICE;
    plo_fasta *f = new plo_fasta();
    f->device = device;
    if (const char *e = getenv("PLO_FASTA_BYTESTORES")) f->byte_stores = atoi(e) != 0;
    if (want && !f->h.init(want->n, want->names, want->lens)) {
        g_fasta_err = "plo_fasta_want: a name is NULL or stands twice, or a length is negative";
        delete f;
        return PLO_ERR_INVALID_ARG;
    }
    plo_status s = PLO_OK;
    if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess) s = PLO_ERR_HIP;
    for (int i = 0; i < 6 && s == PLO_OK; ++i)
        if (hipEventCreate(&f->ev[i]) != hipSuccess) s = PLO_ERR_HIP;
    // with a list: the slots, once and for all; without: the text's size is an upper bound of the bases, the slots' padding grows it
    if (s == PLO_OK) s = fasta_out_ensure(f, want ? std::max<size_t>((size_t)f->h.out_bytes, 256) : (size_t)text_bytes_hint + 4096);
    if (s != PLO_OK) {
        g_fasta_err = f->err.empty() ? "plo_fasta_create: no stream or event" : f->err;
        fasta_release(f);
        return s;
    }
    *out = f;
    return PLO_OK;
}

plo_status plo_fasta_feed(plo_fasta *f, const uint8_t *text, uint64_t n_bytes) {
    if (!f || (n_bytes && !text)) return PLO_ERR_INVALID_ARG;
    if (f->finished) {
        f->err = "plo_fasta_feed: the load is finished";
        return PLO_ERR_INVALID_ARG;
    }
    if (f->h.err_kind) return PLO_ERR_DATA;
    if (hipSetDevice(f->device) != hipSuccess) return PLO_ERR_NO_DEVICE;
    for (uint64_t at = 0; at < n_bytes;) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(n_bytes - at, FA_MAX_PIECE);
        if (plo_status s = fasta_piece(f, text + at, n)) return s;
        at += n;
    }
    return PLO_OK;
}

plo_status plo_fasta_finish(plo_fasta *f, plo_fasta_out *out) {
    if (!f || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    if (hipSetDevice(f->device) != hipSuccess) return PLO_ERR_NO_DEVICE;
    if (!f->finished) {
        FA_TRY(f, hipStreamSynchronize(f->stream));
        float ms = 0.f;
        if (f->emit_timed && hipEventElapsedTime(&ms, f->ev[4], f->ev[5]) == hipSuccess) f->ms += ms;
        f->emit_timed = false;
        f->finished = true;
        if (f->h.finish()) {
            f->err = fasta_refusal_text(f);
        } else {
            if (plo_status s = fasta_out_ensure(f, (size_t)f->h.out_bytes)) return s;
            if (f->h.has_want) {
                for (size_t w = 0; w < f->h.want_name.size(); ++w) {
                    f->o_len.push_back(f->h.want_len[w]);
                    f->o_ptr.push_back(f->out + f->h.want_dst[w]);
                }
            } else {
                for (const FaRec &r : f->h.recs) {
                    f->o_len.push_back(r.len);
                    f->o_ptr.push_back(f->out + r.dst);
                }
            }
        }
    }
    const FaHost &h = f->h;
    out->n_records_seen = h.recs.size();
    out->n_bases = h.n_bases;
    out->text_bytes = h.file_off;
    out->fasta_ms = f->ms;
    out->err_kind = h.err_kind;
    out->err_offset = h.err_offset;
    out->err_chrom = h.err_chrom;
    out->err_len = h.err_len;
    if (h.err_kind) return PLO_ERR_DATA;
    out->n_chroms = (uint32_t)f->o_len.size();
    out->chrom_len = f->o_len.data();
    out->chrom_seq = f->o_ptr.data();
    return PLO_OK;
}

plo_status plo_fasta_record(const plo_fasta *f, uint64_t i, const char **id, int64_t *len, int32_t *want_index) {
    if (!f || !f->finished || i >= f->h.recs.size()) return PLO_ERR_INVALID_ARG;
    const FaRec &r = f->h.recs[(size_t)i];
    if (id) *id = r.id.c_str();
    if (len) *len = r.len;
    if (want_index) *want_index = r.want;
    return PLO_OK;
}

plo_status plo_fasta_adopt(plo_fasta *f, uint32_t n, const uint8_t *const *host_seq, const int64_t *len, const uint8_t **dev_out) {
    if (!f || (n && (!host_seq || !len || !dev_out))) return PLO_ERR_INVALID_ARG;
    if (hipSetDevice(f->device) != hipSuccess) return PLO_ERR_NO_DEVICE;
    for (uint32_t i = 0; i < n; ++i) {
        dev_out[i] = nullptr;
        if (!host_seq[i]) continue;
        if (len[i] < 0) return PLO_ERR_INVALID_ARG;
        void *p = nullptr;
        FA_TRY(f, hipMalloc(&p, std::max<size_t>((size_t)len[i], 16)));
        f->adopted.push_back(p);
        if (len[i] > 0) FA_TRY(f, hipMemcpy(p, host_seq[i], (size_t)len[i], hipMemcpyHostToDevice));
        dev_out[i] = (const uint8_t *)p;
    }
    return PLO_OK;
}

plo_status plo_fasta_download(plo_fasta *f, void *host_dst, const void *dev_src, size_t bytes) {
    if (!f || (bytes && (!host_dst || !dev_src))) return PLO_ERR_INVALID_ARG;
    if (hipSetDevice(f->device) != hipSuccess) return PLO_ERR_NO_DEVICE;
    if (bytes) FA_TRY(f, hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, f->stream));
    FA_TRY(f, hipStreamSynchronize(f->stream));
    return PLO_OK;
}

void plo_fasta_destroy(plo_fasta *f) {
    if (f) fasta_release(f);
}

const char *plo_fasta_last_error(const plo_fasta *f) { return f ? f->err.c_str() : g_fasta_err.c_str(); }

plo_status plo_index_segment_map(const plo_index *ix, uint32_t g, uint32_t cap, int64_t *keys, int64_t *vals, uint32_t *n) {
    if (!ix || !n || g >= ix->d.n_segments) return PLO_ERR_INVALID_ARG;
    uint32_t k0 = ix->host.cs_kv_off[g], k1 = ix->host.cs_kv_off[g + 1];
    *n = k1 - k0;
    if (keys && vals && k1 > k0) {
        if (hipSetDevice(ix->device) != hipSuccess) return PLO_ERR_NO_DEVICE;
        std::vector<KV> tmp(k1 - k0);  // the maps live on the device only
        if (hipMemcpy(tmp.data(), ix->d.kv + k0, tmp.size() * sizeof(KV), hipMemcpyDeviceToHost) != hipSuccess) return PLO_ERR_HIP;
        for (uint32_t i = 0; i < std::min(cap, k1 - k0); ++i) {
            keys[i] = tmp[i].key;
            vals[i] = tmp[i].val == NONE32 ? INT64_MIN : (int64_t)tmp[i].val;
        }
    }
    return PLO_OK;
}

plo_status plo_ctx_create(const plo_index *ix, void *hip_stream, plo_ctx **out) {
    if (!ix || !out) return PLO_ERR_INVALID_ARG;
    *out = nullptr;
    if (hipSetDevice(ix->device) != hipSuccess) return PLO_ERR_NO_DEVICE;
    plo_ctx *c = new plo_ctx();
    c->ix = ix;
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return PLO_ERR_HIP;
        }
        c->own_stream = true;
    }
    if (hipEventCreateWithFlags(&c->ev_cls, hipEventDisableTiming) != hipSuccess) {
        if (c->own_stream) (void)hipStreamDestroy(c->stream);
        delete c;
        return PLO_ERR_HIP;
    }
    for (int i = 0; i < 7; ++i)
        if (hipEventCreate(&c->ev[i]) != hipSuccess) {
            for (int k = 0; k < i; ++k) (void)hipEventDestroy(c->ev[k]);
            if (c->own_stream) (void)hipStreamDestroy(c->stream);
            delete c;
            return PLO_ERR_HIP;
        }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ix->device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cus = prop.multiProcessorCount;
    }
    (void)hipFuncSetAttribute((const void *)k_lift_tiles, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_tiles_sp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_tiles_c256, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_retry_sp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_mid_sp<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_mid_sp<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (getenv("PLO_DEBUG")) {
        for (int cap : {256, 320, 384, 512}) {
            int nb = -1;
            size_t lds = ((tile_mem_bytes(cap) + 15) & ~(size_t)15) * TILE_WAVES;
            hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_lift_tiles, TILE_WAVES * 64, lds);
            fprintf(stderr, "[plo] cap %d: dynamic LDS %zu B/block -> %d blocks/CU (%s)\n", cap, lds, nb, hipGetErrorString(e));
        }
    }
    (void)hipFuncSetAttribute((const void *)k_lift_mid<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_mid<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (const char *e = getenv("PLO_MID_WAVES")) {
        int v = atoi(e);
        c->mid_waves = v >= 16 ? 16 : (v >= 8 ? 8 : 0);
    }
    if (const char *e = getenv("PLO_MID_CAP")) c->mid_cap_max = std::min(4096, std::max(256, atoi(e) & ~63));
    (void)hipFuncSetAttribute((const void *)k_lift_retry, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_lanes, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_lanes_sp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_lanes_stats, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_lanes16, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)k_lift_lanes16_stats, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (const char *e = getenv("PLO_LANE_MAX_W")) c->lane_max_w = atoi(e);
    if (const char *e = getenv("PLO_LANE_SORT")) c->lane_sort = atoi(e) != 0;
    if (const char *e = getenv("PLO_LANE_STATIC")) c->lane_static_rounds = atoi(e);
    if (const char *e = getenv("PLO_LANE_STATS")) c->lane_stats = atoi(e) != 0;
    if (const char *e = getenv("PLO_LANE_H16")) c->lane_h16 = atoi(e) != 0;
    if (const char *e = getenv("PLO_LANE_TAIL")) c->lane_tail_rounds = std::max(0, atoi(e));
    if (const char *e = getenv("PLO_LANE_KVS")) c->lane_kvs = std::min(LANE_KVS_MAX, std::max(64, atoi(e) & ~63));
    if (!c->lane_h16) c->lane_kvs = std::min(c->lane_kvs, LANE_KVS);
    if (const char *e = getenv("PLO_LANE_LOCKSTEP")) c->lane_lockstep = atoi(e) != 0;
    if (const char *e = getenv("PLO_LANE_SORT_WINDOW")) c->lane_sort_window = c->lane_budget_window = std::min(2048, std::max(64, atoi(e) & ~63));
    if (const char *e = getenv("PLO_LANE_BUDGET")) c->lane_budget = atoi(e) != 0;
    if (const char *e = getenv("PLO_LANE_HEAVY_MIN")) c->lane_heavy_min = atoi(e);
    if (const char *e = getenv("PLO_LANE_HEAVY_RATIO")) c->lane_heavy_ratio = std::max(0, atoi(e));
    if (const char *e = getenv("PLO_LANE_STREAM_RATIO")) c->lane_stream_ratio = std::max(1, atoi(e));
    if (const char *e = getenv("PLO_FAST_PATH")) c->fast = atoi(e) != 0;
    if (const char *e = getenv("PLO_SCAN_CHAIN")) c->scan_chain = atoi(e) != 0;
    if (const char *e = getenv("PLO_FAST_LAUNCH_BOUND")) c->fast_launch_bound = atoi(e) != 0;
    if (const char *e = getenv("PLO_FAST_FUSE")) c->fast_fuse = atoi(e) != 0;
    if (const char *e = getenv("PLO_RECORDS_BYTECOPY")) c->rec_bytecopy = atoi(e) != 0;
    if (const char *e = getenv("PLO_PHASE_EVENTS")) c->phase_events = atoi(e) != 0;
    if (const char *e = getenv("PLO_LANE_CAPW")) c->lane_capw = std::min(40000, std::max(64, atoi(e))) & ~3;
    if (c->lane_max_w + LANE_SLACK > c->lane_capw) c->lane_max_w = c->lane_capw - LANE_SLACK;
    if (const char *e = getenv("PLO_TILE_WAVES")) c->tile_waves = std::min(TILE_WAVES, std::max(1, atoi(e)));
    if (const char *e = getenv("PLO_WINDOW")) c->window = std::max(16, atoi(e)), c->adaptive = false;
    if (const char *e = getenv("PLO_BIG_THRESH")) c->big_thresh = std::max(1, atoi(e)), c->adaptive = false;
    if (const char *e = getenv("PLO_CAP")) c->cap = std::max(64, atoi(e)), c->adaptive = false;
    *out = c;
    return PLO_OK;
}

void plo_ctx_destroy(plo_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->ix->device);
    (void)hipStreamSynchronize(c->stream);
    DevBuf *bufs[] = {&c->f_flag, &c->f_bin, &c->f_end, &c->f_prim, &c->f_isoff, &c->f_iqoff, &c->f_iread, &c->f_nl, &c->f_pitem,
                      &c->f_uflag, &c->f_rsoff, &c->f_rqoff, &c->f_su, &c->f_qu, &c->f_soff, &c->f_qoff, &c->f_rseq, &c->f_rqual, &c->f_fflag, &c->f_frank, &c->f_flist, &c->sa_len, &c->sa_off, &c->sa_text, &c->r_plan, &c->r_size, &c->r_start, &c->r_partial, &c->r_recoff, &c->r_out, &c->r_err, &c->z_slots, &c->z_size, &c->z_off, &c->z_partial, &c->z_tok, &c->z_out, &c->z_err,
                      &c->bb_table, &c->bb_plan, &c->bb_size, &c->bb_start, &c->bb_partial, &c->bb_kind, &c->bb_err, &c->bb_tkey, &c->bb_tnops, &c->bb_tctext, &c->bb_tclen,
                      &c->bb_tcontig, &c->bb_tdst, &c->bb_tpos, &c->bb_tfwd, &c->bb_rev, &c->bb_len, &c->bb_soff, &c->bb_qoff, &c->bb_flags, &c->bb_sread, &c->bb_scontig,
                      &c->bb_spos, &c->bb_sfwd, &c->bb_coff, &c->bb_cigar,
                      &c->wc_guess, &c->wc_land, &c->wc_cnt, &c->wc_start, &c->wc_partial, &c->wc_fire, &c->wc_res, &c->wc_recoff, &c->wc_unmoff, &c->wc_unmsrc, &c->wc_unm, &c->ps_res,
                      &c->ci_comp, &c->ci_blk, &c->ci_st, &c->nm_out, &c->nm_blk,
                      &c->so_key[0], &c->so_key[1], &c->so_idx[0], &c->so_idx[1], &c->so_len, &c->so_slen, &c->so_off, &c->so_partial, &c->so_out, &c->so_blk, &c->bai_entry, &c->bai_blk, &c->dp_plan, &c->dp_blk,
                      &c->mg_key[0], &c->mg_key[1], &c->mg_src[0], &c->mg_src[1], &c->mg_runof, &c->mg_len, &c->mg_mlen, &c->mg_off, &c->mg_partial, &c->mg_runs, &c->mg_first, &c->mg_blk, &c->mg_cfirst,
                      &c->mg_coff, &c->mg_out, &c->mg_ooff,
                      &c->item_region, &c->lane_groups, &c->lane_ticket, &c->misc, &c->whist, &c->cls_partial, &c->lane_scratch, &c->item_cls, &c->retry_list, &c->perm, &c->nin_p, &c->seg_reflen, &c->seg_readlen, &c->seg_nm, &c->seg_cnt, &c->seg_off, &c->scan_partial, &c->item_seg, &c->item_cseg, &c->item_nin, &c->op_prefix,
                      &c->counters, &c->big_list, &c->huge_list, &c->verr, &c->scratch, &c->tile_lo, &c->d_n_m, &c->d_in_off, &c->d_n_in, &c->d_pos1,
                      &c->d_w0, &c->d_w1, &c->d_kv0, &c->d_kv1, &c->d_flags, &c->d_contig, &c->d_seq_len, &c->d_seq_off, &c->d_shift_ref,
                      &c->d_shift_ref_len, &c->d_chrom_ref, &c->d_chrom_ref_len, &c->d_read_len, &c->o_status, &c->o_flip, &c->o_mapq, &c->o_chrom, &c->o_pos,
                      &c->o_coff, &c->o_clen, &c->o_cigar, &c->o_dense_off, &c->o_cigar_dense, &c->wave_stats, &c->fast_blk, &c->i_read_rev, &c->i_read_len, &c->i_read_off, &c->i_seq,
                      &c->i_seg_read, &c->i_seg_contig, &c->i_seg_pos, &c->i_seg_fwd, &c->i_seg_coff, &c->i_cigar,
                      &c->i_item_seg, &c->i_item_cseg, &c->miss_list, &c->miss_info, &c->miss_vals, &c->miss_seq_off, &c->miss_side};
    for (DevBuf *b : bufs) b->release();
    HostBuf *hb[] = {&c->h_item_seg, &c->h_item_cseg, &c->h_status, &c->h_flip, &c->h_mapq, &c->h_chrom, &c->h_pos,
                     &c->h_coff, &c->h_clen, &c->h_cigar, &c->h_counters, &c->h_miss, &c->h_side, &c->h_rec, &c->h_bgzf, &c->h_bb, &c->h_wc, &c->h_ci, &c->h_nm, &c->h_so, &c->h_bai, &c->h_dp, &c->h_mg, &c->h_mg_tab};
    for (HostBuf *b : hb) b->release();
    for (int i = 0; i < 7; ++i)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    for (int i = 0; i < 5; ++i)
        if (c->fev[i]) (void)hipEventDestroy(c->fev[i]);
    for (int i = 0; i < 4; ++i)
        if (c->rev[i]) (void)hipEventDestroy(c->rev[i]);
    for (int i = 0; i < 2; ++i)
        if (c->zev[i]) (void)hipEventDestroy(c->zev[i]);
    for (int i = 0; i < 4; ++i)
        if (c->bev[i]) (void)hipEventDestroy(c->bev[i]);
    for (int i = 0; i < 4; ++i)
        if (c->wev[i]) (void)hipEventDestroy(c->wev[i]);
    for (int i = 0; i < 2; ++i)
        if (c->iev[i]) (void)hipEventDestroy(c->iev[i]);
    for (int i = 0; i < 2; ++i)
        if (c->nev[i]) (void)hipEventDestroy(c->nev[i]);
    c->md.release();
    c->eqx.release();
    for (int i = 0; i < 2; ++i)
        if (c->sev[i]) (void)hipEventDestroy(c->sev[i]);
    for (int i = 0; i < 2; ++i)
        if (c->xev[i]) (void)hipEventDestroy(c->xev[i]);
    for (int i = 0; i < 2; ++i)
        if (c->dpev[i]) (void)hipEventDestroy(c->dpev[i]);
    for (int i = 0; i < 4; ++i)
        if (c->gev[i]) (void)hipEventDestroy(c->gev[i]);
    if (c->ev_seq) (void)hipEventDestroy(c->ev_seq);
    if (c->ev_cls) (void)hipEventDestroy(c->ev_cls);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *plo_last_error(const plo_ctx *c) { return c ? c->err.c_str() : g_index_err.c_str(); }

void *plo_ctx_stream(plo_ctx *c) { return c ? (void *)c->stream : nullptr; }
int plo_ctx_device(plo_ctx *c) { return c ? c->ix->device : -1; }

plo_status plo_ctx_set_stats(plo_ctx *c, int on) {
    if (!c) return PLO_ERR_INVALID_ARG;
    c->lane_stats = on != 0;
    return PLO_OK;
}

plo_status plo_ctx_set_phase_events(plo_ctx *c, int on) {
    if (!c) return PLO_ERR_INVALID_ARG;
    c->phase_events = on != 0;
    return PLO_OK;
}

plo_status plo_ctx_sync(plo_ctx *c) {
    if (!c) return PLO_ERR_INVALID_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PLO_OK;
}

// debugging aid (timing builds, -DPLO_PHASE_TIMING): shader cycles spent per pipeline phase, summed over waves
void plo_ctx_phase_cycles(plo_ctx *c, unsigned long long *out12) {
    for (int k = 0; k < 12; ++k) out12[k] = c ? c->phase_cycles[k] : 0;
}
// debugging aid: the item indices the last batch's lane kernels handed to the retry list (first `max_items` of them); returns how many were copied
unsigned plo_ctx_debug_retry_list(plo_ctx *c, unsigned *out, unsigned max_items) {
    if (!c || !out || !c->retry_list.p) return 0;
    const unsigned n = (unsigned)std::min<size_t>(std::min<size_t>(max_items, c->timing.n_retry_items), c->retry_list.cap / 4);
    if (hipSetDevice(c->ix->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    if (n && hipMemcpy(out, c->retry_list.p, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}
// debugging aid (timing builds): the raw statistic slots of the last batch's lift waves, STAT_WORDS words each -- [5] / [6] the wave's first and
// last tick of the constant 100 MHz clock, [7] its HW_ID | XCC_ID << 16 (tools/wave_timeline.py); returns the slots copied
unsigned plo_ctx_wave_clocks(plo_ctx *c, unsigned long long *out, unsigned max_slots) {
    if (!c || !out || !c->wave_stats.p) return 0;
    const unsigned n = (unsigned)std::min<size_t>(max_slots, c->wave_stats.cap / (STAT_WORDS * 8));
    if (hipSetDevice(c->ix->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    if (hipMemcpy(out, c->wave_stats.p, (size_t)n * STAT_WORDS * 8, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return n;
}

plo_status plo_ctx_download(plo_ctx *c, void *host_dst, const void *dev_src, size_t bytes) {
    if (!c || (bytes && (!host_dst || !dev_src))) return PLO_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->ix->device));
    if (bytes) HIP_TRY(c, hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PLO_OK;
}

static plo_status scan_u32(plo_ctx *c, const uint32_t *in, uint32_t n, uint32_t *out /* n+1 */) {
    uint32_t nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    if (nb == 0) nb = 1;
    if ((((uintptr_t)in) | ((uintptr_t)out)) & 15u) {  // (the kernels move eight values per thread as two 16-byte accesses)
        c->err = "scan_u32: unaligned buffer";
        return PLO_ERR_INVALID_ARG;
    }
    HIP_TRY(c, c->scan_partial.ensure((size_t)nb * 4));
    uint32_t *partial = c->scan_partial.as<uint32_t>();
    hipLaunchKernelGGL(k_scan_sums, dim3(nb), dim3(SCAN_THREADS), 0, c->stream, in, n, partial);
    hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(SCAN_THREADS), 0, c->stream, partial, nb, out, n);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(SCAN_THREADS), 0, c->stream, in, n, (const uint32_t *)partial, out);
    HIP_TRY(c, hipGetLastError());
    return PLO_OK;
}

// which instantiation of the light-item kernel a call takes
typedef void (*lane_kernel_t)(DevIndex, DevBatch, DevWork, uint32_t, uint32_t, uint32_t, uint32_t, int, const uint32_t *);
static lane_kernel_t lane_kernel_of(const plo_ctx *c, uint32_t stages, bool sp) {
    if (sp) return k_lift_lanes_sp;
    const bool h16 = c->lane_h16 && (stages & PLO_STAGE_LIFTOVER) != 0u;  // (16-bit regions need LOAD's merged op codes)
    if (h16) return c->lane_stats ? k_lift_lanes16_stats : k_lift_lanes16;
    return c->lane_stats ? k_lift_lanes_stats : k_lift_lanes;
}

// The lane kernel's ticket counters (lane_tiles_persistent): this launch's -- zero, because the context's previous launch cleared it or the
// allocation did -- and the next launch's, which this one clears.  Without them (PLO_LANE_STATIC < 0, or no memory) the waves keep to fixed slots.
// `groups`, `waves`: the launch's groups (an estimate will do) and waves -- the rounds of fixed slots in front of the tickets follow them unless
// PLO_LANE_STATIC names a number: all but the last two and a half rounds.  Measured on wgs30x (10.5 rounds; EXPERIMENTS 6.2b): 1 / 4 / 8 / 9
// fixed rounds 1.126-1.147 / 1.095-1.103 / 1.085-1.097 / 1.133-1.148 ms -- neighbouring groups on neighbouring waves of one XCD share their
// descriptor, CIGAR and block-map lines in its L2, which the tickets give up; the last rounds are what levels the waves.
static void lane_ticket_arm(plo_ctx *c, DevWork &wk, uint32_t groups, uint32_t waves) {
    wk.lane_kvs = (uint32_t)c->lane_kvs;
    wk.lane_lockstep_off = c->lane_lockstep ? 0u : 1u;
    wk.lane_tail_rounds = (uint32_t)c->lane_tail_rounds;
    wk.lane_ticket = nullptr;
    wk.lane_ticket_next = nullptr;
    wk.lane_static_rounds = 0;
    if (c->lane_static_rounds < 0) return;
    if (!c->lane_ticket.p) {
        if (c->lane_ticket.ensure(256) != hipSuccess) return;
        if (hipMemsetAsync(c->lane_ticket.p, 0, 256, c->stream) != hipSuccess) {
            c->lane_ticket.release();
            return;
        }
    }
    uint32_t *const t = c->lane_ticket.as<uint32_t>();  // (the two counters on lines of their own)
    wk.lane_ticket = t + 32 * (c->lane_epoch & 1u);
    wk.lane_ticket_next = t + 32 * ((c->lane_epoch + 1u) & 1u);
    const uint32_t rounds = waves ? groups / waves : 0u;  // whole rounds of the launch
    wk.lane_static_rounds = c->lane_static_rounds > 0 ? (uint32_t)c->lane_static_rounds : std::max(1u, rounds > 2u ? rounds - 2u : 1u);
    ++c->lane_epoch;
}

// the item work list and the per-item outputs of a batch of `n_items` items in the context's buffers
static void fill_work(plo_ctx *c, DevWork &wk, uint32_t n_items) {
    memset(&wk, 0, sizeof(wk));
    wk.n_items = n_items;
    wk.item_seg = c->item_seg.as<uint32_t>();
    wk.item_cseg = c->item_cseg.as<uint32_t>();
    wk.item_nin = c->item_nin.as<uint32_t>();
    wk.item_cls = c->item_cls.as<uint32_t>();
    wk.perm = c->perm.as<uint32_t>();
    wk.retry_list = c->retry_list.as<uint32_t>();
    wk.lane_max_w = c->lane_max_w;
    wk.item_op_prefix = c->op_prefix.as<uint32_t>();
    wk.d.in_off = c->d_in_off.as<uint32_t>();
    wk.d.n_in = c->d_n_in.as<uint32_t>();
    wk.d.n_m = c->d_n_m.as<uint32_t>();
    wk.d.pos1 = c->d_pos1.as<int>();
    wk.d.w0 = c->d_w0.as<uint32_t>();
    wk.d.w1 = c->d_w1.as<uint32_t>();
    wk.d.kv0 = c->d_kv0.as<uint32_t>();
    wk.d.kv1 = c->d_kv1.as<uint32_t>();
    wk.d.flags = c->d_flags.as<uint32_t>();
    wk.d.contig = c->d_contig.as<uint32_t>();
    wk.d.seq_len = c->d_seq_len.as<uint32_t>();
    wk.d.seq_off = c->d_seq_off.as<uint64_t>();
    wk.d.shift_ref = c->d_shift_ref.as<uint64_t>();
    wk.d.shift_ref_len = c->d_shift_ref_len.as<int>();
    wk.d.chrom_ref = c->d_chrom_ref.as<uint64_t>();
    wk.d.chrom_ref_len = c->d_chrom_ref_len.as<int>();
    wk.d.read_len = c->d_read_len.as<uint32_t>();
    wk.seg_readlen = c->seg_readlen.as<uint32_t>();
    wk.seg_nm = c->seg_nm.as<uint32_t>();
    wk.status = c->o_status.as<uint8_t>();
    wk.flip = c->o_flip.as<uint8_t>();
    wk.mapq = c->o_mapq.as<uint8_t>();
    wk.chrom = c->o_chrom.as<uint32_t>();
    wk.pos = c->o_pos.as<int64_t>();
    wk.cig_off = c->o_coff.as<uint64_t>();
    wk.cig_len = c->o_clen.as<uint32_t>();
    wk.counters = c->counters.as<unsigned long long>();
    wk.big_list = c->big_list.as<uint32_t>();
    wk.miss_list = c->miss_list.as<uint32_t>();
    wk.wave_stats = c->wave_stats.as<unsigned long long>();
}

static plo_status liftover_fast(plo_ctx *c, const plo_batch_in *in, uint32_t stages, plo_batch_out *out, const DevBatch &bt, bool &fallback);

plo_status plo_liftover_batch_dev(plo_ctx *c, const plo_batch_in *in, uint32_t stages, plo_batch_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    c->err.clear();
    c->have_nm = false;
    c->have_md = false;
    c->have_eqx = false;
    HIP_TRY(c, hipSetDevice(c->ix->device));
    if (in->n_segs && (!in->seg_read || !in->seg_contig || !in->seg_pos || !in->seg_is_fwd_strand || !in->seg_cigar_off)) {
        c->err = "plo_batch_in: NULL segment array";
        return PLO_ERR_INVALID_ARG;
    }
    if (in->seq_fmt != PLO_SEQ_BAM4 && in->seq_fmt != PLO_SEQ_ASCII && in->seq_fmt != PLO_SEQ_BAM4_SPARSE) {
        c->err = "plo_batch_in: unknown seq_fmt";
        return PLO_ERR_INVALID_ARG;
    }
    DevBatch bt;
    bt.read_is_reverse = in->read_is_reverse;
    bt.read_seq_len = in->read_seq_len;
    bt.read_seq_off = in->read_seq_off;
    bt.seq = in->seq;
    bt.seq_fmt = in->seq_fmt;
    bt.seq_bytes = in->seq_bytes;
    bt.seg_read = in->seg_read;
    bt.seg_contig = in->seg_contig;
    bt.seg_pos = in->seg_pos;
    bt.seg_is_fwd = in->seg_is_fwd_strand;
    bt.seg_cigar_off = in->seg_cigar_off;
    bt.cigar = in->cigar;
    bt.n_reads = in->n_reads;
    bt.n_segs = in->n_segs;
    const DevIndex &ix = c->ix->d;
    const bool sp = in->seq_fmt == PLO_SEQ_BAM4_SPARSE;  // the `_sp` kernels: probes look granules up
    hipStream_t st = c->stream;
    memset(&c->timing, 0, sizeof(c->timing));
    c->fast_timing = false;
    c->fast_no_events = false;
    uint32_t n_syncs = 0;  // host round trips of the call
    c->ev_big = false;
    c->ev_mid = false;

    // A context that has just lifted a batch of light items only, with arrays that hold this one too: everything is launched with counts
    // read from device memory and the host looks ONCE, at the end (liftover_fast); a batch that turns out not to fit -- more items than
    // the arrays hold, heavy items, an overflow -- is run again on the path below, which asks for the counts first
    if (c->fast && c->fast_light_only && !in->item_seg && !sp && in->n_segs && in->n_segs <= c->fast_ns_cap && c->fast_item_cap && c->lane_max_w >= 0 && c->lane_sort &&
        !c->lane_budget && c->lane_sort_window <= 128 && c->o_cigar.cap) {
        bool fallback = false;
        plo_status fs = liftover_fast(c, in, stages, out, bt, fallback);
        if (!fallback) return fs;
        c->fast_light_only = false;
        c->fast_extra_syncs = 1;
        memset(out, 0, sizeof(*out));
        memset(&c->timing, 0, sizeof(c->timing));
    }
    HIP_TRY(c, hipEventRecord(c->ev[0], st));
    // ---- items: count -> scan -> resolve descriptors -> scan op counts -> tile bounds ----
    uint32_t n_items = 0;
    HIP_TRY(c, c->h_counters.ensure(64 * 8 + CNT_N * 8 + 64));
    uint32_t ns = in->n_segs;
    HIP_TRY(c, c->verr.ensure(16));
    HIP_TRY(c, hipMemsetAsync(c->verr.p, 0, 16, st));
    auto verr_status = [&](uint32_t flags) -> plo_status {
        if (flags & VERR_INDEX) {
            c->err = "plo_batch_in: an index points outside its array (seg_read / seg_contig / seg_cigar_off / read_seq_off / item_seg / item_cseg)";
            return PLO_ERR_INVALID_ARG;
        }
        c->err = "plo_batch_in: coordinate outside the 31-bit BAM range, CIGAR op code above 8, a CIGAR spanning 2^30 bases or more, or a read segment that ends behind its contig's end on a reverse-strand contig segment";
        return PLO_ERR_RANGE;
    };
    {   // k_seg_count always runs: it is the boundary check of the batch (and counts the items unless the caller lists them)
        HIP_TRY(c, c->seg_cnt.ensure((size_t)std::max(1u, ns) * 4));
        HIP_TRY(c, c->seg_off.ensure((size_t)(ns + 1) * 4));
        HIP_TRY(c, c->seg_reflen.ensure((size_t)std::max(1u, ns) * 4));
        HIP_TRY(c, c->seg_readlen.ensure((size_t)std::max(1u, ns) * 4));
        HIP_TRY(c, c->seg_nm.ensure((size_t)std::max(1u, ns) * 4));
        if (ns)
            hipLaunchKernelGGL(k_seg_count, dim3((unsigned)(((unsigned long long)ns * SEG_LANES + 255) / 256)), dim3(256), 0, st, ix, bt,
                               c->seg_cnt.as<uint32_t>(), c->seg_reflen.as<int>(), c->seg_readlen.as<uint32_t>(), c->seg_nm.as<uint32_t>(), c->verr.as<uint32_t>());
        plo_status s = scan_u32(c, c->seg_cnt.as<uint32_t>(), ns, c->seg_off.as<uint32_t>());
        if (s != PLO_OK) return s;
        uint32_t *h = c->h_counters.as<uint32_t>();
        HIP_TRY(c, hipMemcpyAsync(h, c->seg_off.as<uint32_t>() + ns, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h + 1, c->verr.p, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st)); ++n_syncs;
        if (h[1]) return verr_status(h[1]);
        n_items = in->item_seg ? in->n_items : h[0];
    }
    size_t ni = std::max(1u, n_items);
    HIP_TRY(c, c->item_seg.ensure(ni * 4));
    HIP_TRY(c, c->item_cseg.ensure(ni * 4));
    HIP_TRY(c, c->item_nin.ensure(ni * 4));
    HIP_TRY(c, c->item_cls.ensure(ni * 4));
    HIP_TRY(c, c->retry_list.ensure(ni * 4));
    HIP_TRY(c, c->perm.ensure(ni * 4));
    HIP_TRY(c, c->nin_p.ensure(ni * 4));
    HIP_TRY(c, c->op_prefix.ensure((size_t)(n_items + 1) * 4));
    HIP_TRY(c, c->d_in_off.ensure(ni * 4));
    HIP_TRY(c, c->d_n_in.ensure(ni * 4));
    HIP_TRY(c, c->d_n_m.ensure(ni * 4));
    HIP_TRY(c, c->d_pos1.ensure(ni * 4));
    HIP_TRY(c, c->d_w0.ensure(ni * 4));
    HIP_TRY(c, c->d_w1.ensure(ni * 4));
    HIP_TRY(c, c->d_kv0.ensure(ni * 4));
    HIP_TRY(c, c->d_kv1.ensure(ni * 4));
    HIP_TRY(c, c->d_flags.ensure(ni * 4));
    HIP_TRY(c, c->d_contig.ensure(ni * 4));
    HIP_TRY(c, c->d_seq_len.ensure(ni * 4));
    HIP_TRY(c, c->d_seq_off.ensure(ni * 8));
    HIP_TRY(c, c->d_shift_ref.ensure(ni * 8));
    HIP_TRY(c, c->d_shift_ref_len.ensure(ni * 4));
    HIP_TRY(c, c->d_chrom_ref.ensure(ni * 8));
    HIP_TRY(c, c->d_chrom_ref_len.ensure(ni * 4));
    HIP_TRY(c, c->d_read_len.ensure(ni * 4));
    HIP_TRY(c, c->o_status.ensure(ni));
    HIP_TRY(c, c->o_flip.ensure(ni));
    HIP_TRY(c, c->o_mapq.ensure(ni));
    HIP_TRY(c, c->o_chrom.ensure(ni * 4));
    HIP_TRY(c, c->o_pos.ensure(ni * 8));
    HIP_TRY(c, c->o_coff.ensure(ni * 8));
    HIP_TRY(c, c->o_clen.ensure(ni * 4));
    HIP_TRY(c, c->big_list.ensure(ni * 4));
    if (in->seq_fmt == PLO_SEQ_BAM4_SPARSE) HIP_TRY(c, c->miss_list.ensure(ni * 4));
    HIP_TRY(c, c->counters.ensure(CNT_N * 8));
    {   // items the per-item arrays hold (they grow with head-room): the one-round-trip path's capacity (the last batch's item
        // count refused a window with one item more and cost it two passes)
        size_t cap_items = (size_t)0xffffffffu;
        const struct { const DevBuf *b; size_t el; } arrs[] = {
            {&c->item_seg, 4}, {&c->item_cseg, 4}, {&c->item_nin, 4}, {&c->item_cls, 4}, {&c->retry_list, 4}, {&c->perm, 4}, {&c->nin_p, 4},
            {&c->d_in_off, 4}, {&c->d_n_in, 4}, {&c->d_n_m, 4}, {&c->d_pos1, 4}, {&c->d_w0, 4}, {&c->d_w1, 4}, {&c->d_kv0, 4}, {&c->d_kv1, 4},
            {&c->d_flags, 4}, {&c->d_contig, 4}, {&c->d_seq_len, 4}, {&c->d_seq_off, 8}, {&c->d_shift_ref, 8}, {&c->d_shift_ref_len, 4},
            {&c->d_chrom_ref, 8}, {&c->d_chrom_ref_len, 4}, {&c->d_read_len, 4}, {&c->o_status, 1}, {&c->o_flip, 1}, {&c->o_mapq, 1},
            {&c->o_chrom, 4}, {&c->o_pos, 8}, {&c->o_coff, 8}, {&c->o_clen, 4}, {&c->big_list, 4}};
        for (const auto &a : arrs) cap_items = std::min(cap_items, a.b->cap / a.el);
        cap_items = std::min(cap_items, c->op_prefix.cap / 4 ? c->op_prefix.cap / 4 - 1 : 0);
        c->item_cap_now = (uint32_t)std::min<size_t>(cap_items, 0x7fffffffu);
    }
    DevWork wk;
    fill_work(c, wk, n_items);
    {   // statistic slots of the lift kernels' waves: zeroed once, cleared again by every k_sum_stats
        const size_t want = (size_t)STAT_SLOTS * STAT_WORDS * 8;
        if (c->wave_stats.cap < want) {
            HIP_TRY(c, c->wave_stats.ensure(want));
            HIP_TRY(c, hipMemsetAsync(c->wave_stats.p, 0, want, st));
        }
    }
    wk.wave_stats = c->wave_stats.as<unsigned long long>();
    // every lift launch of a batch leaves its waves' statistics in its own range of slots (PLO_STAT_RANGE before the launch); they
    // are added up once before the host reads the counters (PLO_READ_COUNTERS), not after every kernel
    uint32_t stat_used = 0;
#define PLO_STAT_RANGE(n_waves_)     \
    do {                             \
        wk.stat_base = stat_used;    \
        stat_used += (n_waves_);     \
    } while (0)
#define PLO_READ_COUNTERS()                                                                                                          \
    do {                                                                                                                             \
        if (stat_used)                                                                                                               \
            hipLaunchKernelGGL(k_sum_stats, dim3(std::min<uint32_t>((stat_used + 255) / 256, 16u)), dim3(256), 0, st,                 \
                               c->wave_stats.as<unsigned long long>(), stat_used, c->counters.as<unsigned long long>());            \
        stat_used = 0;                                                                                                               \
        HIP_TRY(c, hipMemcpyAsync(hc, c->counters.p, CNT_N * 8, hipMemcpyDeviceToHost, st));                                         \
        HIP_TRY(c, hipStreamSynchronize(st)); ++n_syncs;                                                                                        \
    } while (0)
    wk.big_list = c->big_list.as<uint32_t>();
    if (c->lane_sort && c->lane_budget && c->lane_max_w >= 0) {
        HIP_TRY(c, c->item_region.ensure(ni * 4));
        wk.item_region = c->item_region.as<uint32_t>();
    }
    wk.miss_list = c->miss_list.as<uint32_t>();
    if (n_items) {
        if (in->item_seg)
            hipLaunchKernelGGL(k_item_desc, dim3((n_items + 255) / 256), dim3(256), 0, st, ix, bt, wk, stages, in->item_seg,
                               in->item_cseg, c->verr.as<uint32_t>());
        else
            hipLaunchKernelGGL(k_item_emit, dim3((ns + 255) / 256), dim3(256), 0, st, ix, bt, wk, stages,
                               (const uint32_t *)c->seg_off.as<uint32_t>(), c->seg_reflen.as<int>(), 0xffffffffu, c->verr.as<uint32_t>());
        HIP_TRY(c, hipGetLastError());
    }
    // ---- class order: block counts -> scan -> permutation (three launches); the host learns the class counts and the weights'
    // sum / maximum from one copy, made while k_permute2 runs
    uint32_t total_ops = 0, max_nin = 0, n_small = 0, h_cls[3] = {0, 0, 0};
    unsigned long long all_ops = 0;
    const uint32_t cls_nb = (n_items + CLS_BLOCK - 1) / CLS_BLOCK;
    {
        HIP_TRY(c, c->misc.ensure(256));
        HIP_TRY(c, hipMemsetAsync(c->misc.p, 0, 256, st));
        HIP_TRY(c, c->cls_partial.ensure((size_t)std::max(1u, cls_nb) * 6 * 4));
        uint32_t *m_ = c->h_counters.as<uint32_t>() + 64;  // clear of h[0..47] below
        memset(m_, 0, 8 * 4);
        if (n_items) {
            hipLaunchKernelGGL(k_cls_hist, dim3(cls_nb), dim3(CLS_THREADS), 0, st, (const uint32_t *)c->item_cls.as<uint32_t>(),
                               (const uint32_t *)c->item_nin.as<uint32_t>(), n_items, cls_nb, c->cls_partial.as<uint32_t>(), (const uint32_t *)nullptr);
            hipLaunchKernelGGL(k_cls_scan, dim3(1), dim3(SCAN_THREADS), 0, st, c->cls_partial.as<uint32_t>(), cls_nb, c->misc.as<uint32_t>());
            HIP_TRY(c, hipMemcpyAsync(m_, c->misc.p, 6 * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipMemcpyAsync(m_ + 6, c->verr.p, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipEventRecord(c->ev_cls, st));
            hipLaunchKernelGGL(k_permute2, dim3(cls_nb), dim3(CLS_THREADS), 0, st, (const uint32_t *)c->item_cls.as<uint32_t>(),
                               (const uint32_t *)c->item_nin.as<uint32_t>(), (const uint32_t *)c->cls_partial.as<uint32_t>(),
                               (const uint32_t *)c->misc.as<uint32_t>(), n_items, cls_nb, c->perm.as<uint32_t>(), c->nin_p.as<uint32_t>(),
                               c->adaptive ? (uint32_t)((WHIST_BINS - 1) * WHIST_STEP) : 0xffffffffu, (const uint32_t *)nullptr);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventSynchronize(c->ev_cls)); ++n_syncs;  // (the copies are done; k_permute2 may still be running)
        }
        if (m_[6]) return verr_status(m_[6]);
        h_cls[0] = m_[0];
        h_cls[1] = m_[1];
        h_cls[2] = m_[2];
        n_small = m_[0] + m_[1];
        max_nin = m_[3];
        all_ops = (unsigned long long)m_[4] | ((unsigned long long)m_[5] << 32);
        if (all_ops > 0x7fffffffull) {  // op indices are int: the weights bound the ops of every stage, output included
            c->err = "batch too large: the item weights (CIGAR ops + 2 x block-map entries) sum to more than 2^31; split the batch";
            return PLO_ERR_RANGE;
        }
    }
    // ---- items too heavy for an LDS region.  Many of them: the lane-per-item code again, regions in global scratch (k_lift_lanes_g).
    // A few: tiles of the wave-cooperative kernel (weight prefix, per-batch geometry).
    // The lane kernel takes as long as its longest item takes a wave (about 3.5 us per op), however many items there are; the
    // workgroup-per-item kernel takes about 70 ps per op of the batch.  So: the lanes when the batch's ops (weights) outnumber the
    // longest item's by lane_heavy_ratio -- 50 000, the measured crossing on the stress profile (67 k reads of 2 000 ops, longest
    // 2 800 + 240 block-map allowance).  PLO_LANE_HEAVY_MIN: an item count instead (0: always).
    const uint32_t n_heavy_all = n_items - n_small;
    // The streaming kernel (a team of waves per 64 item slots, lane_stream.hpp; all stages only) has a third of the lane kernel's latency per
    // item -- its stages run side by side -- at about the same instructions per op: measured on the stress profile it is the fastest of the
    // three from ~40 k heavy items (50 k reads: 5.9 ms against 6.65 ms workgroup-per-item and 8.6 ms k_lift_lanes_g) to ~200 k (100 k reads:
    // 9.1 against 9.5 ms; 500 k: 30.6 against 25.9 ms k_lift_lanes_g_w3, whose waves each hold several groups by then).  So: the
    // batch's ops against its longest item's by lane_stream_ratio (30 000) for the lower bound, the three-waves-per-SIMD rule of
    // k_lift_lanes_g_w3 for the upper.  PLO_LANE_STREAM=0 / 1: never / whenever the lane path is taken.
    bool stream_ok = (stages & PLO_STAGES_ALL) == PLO_STAGES_ALL && c->lane_stream && n_items < (1u << 28);
    bool stream_forced = false;
    if (const char *e = getenv("PLO_LANE_STREAM")) {
        stream_ok = stream_ok && atoi(e) != 0;
        stream_forced = stream_ok;
    }
    const bool stream_size = n_heavy_all >= 8192u && n_heavy_all < (uint32_t)c->n_cus * 3u * LANE_G_WAVES * 64u &&
                             all_ops >= (unsigned long long)c->lane_stream_ratio * std::min<unsigned long long>(max_nin, 16384ull);
    const bool heavy_lanes =
        n_heavy_all > 0 && c->lane_max_w >= 0 &&
        (c->lane_heavy_min >= 0 ? n_heavy_all >= (uint32_t)c->lane_heavy_min
                                : ((stream_ok && stream_size) ||
                                   (c->lane_heavy_ratio > 0 && n_heavy_all >= 8192u &&
                                    all_ops >= (unsigned long long)c->lane_heavy_ratio * std::min<unsigned long long>(max_nin, 16384ull))));
    const bool heavy_stream = heavy_lanes && stream_ok && (stream_forced || stream_size || c->lane_heavy_min >= 0);
    if (n_items > n_small && !heavy_lanes) {
        plo_status s = scan_u32(c, c->nin_p.as<uint32_t>(), n_items, c->op_prefix.as<uint32_t>());
        if (s != PLO_OK) return s;
        HIP_TRY(c, c->whist.ensure(256));
        HIP_TRY(c, hipMemsetAsync(c->whist.p, 0, 256, st));
        hipLaunchKernelGGL(k_max_u32, dim3(std::min<uint32_t>((n_items + 255) / 256, 256u)), dim3(256), 0, st,
                           (const uint32_t *)c->item_nin.as<uint32_t>(), n_items, c->whist.as<uint32_t>(),
                           (const uint32_t *)c->op_prefix.as<uint32_t>() + n_items, (const uint32_t *)c->misc.as<uint32_t>(),
                           (const uint32_t *)c->misc.as<uint32_t>() + 1);
        // one copy: [0] max weight, [2..3] weight sum, [4] tiled weight, [8..] weight histogram
        uint32_t *m_ = c->h_counters.as<uint32_t>() + 64;
        HIP_TRY(c, hipMemcpyAsync(m_, c->whist.p, (WHIST_AT + WHIST_BINS) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st)); ++n_syncs;
        uint32_t *h = c->h_counters.as<uint32_t>();
        for (int k = 0; k < WHIST_BINS; ++k) h[8 + k] = m_[WHIST_AT + k];
        total_ops = m_[4];  // weight of the tiled items
        if (c->adaptive) {
            // Tile geometry from the batch's weight distribution: the routing threshold covers all but 0.2 % of the items
            // (those take the large-item kernel), the LDS slice holds one window plus the overhang of its last item.  Dense
            // contig block maps (many blocks per read) thus get larger slices and fewer resident waves instead of a
            // large-item kernel that runs every read alone from global scratch.
            const uint32_t *hist = h + 8;
            // items in the open-ended last bin take the large-item kernel whatever the geometry: the threshold is chosen for the rest
            unsigned long long above = 0, allow = (n_items - std::min<uint32_t>(n_items, hist[WHIST_BINS - 1])) / 500;
            int b = WHIST_BINS - 2;
            for (; b > 0; --b) {  // lowest threshold (b * WHIST_STEP) with at most `allow` items above it
                if (above + hist[b] > allow) break;
                above += hist[b];
            }
            int thresh = std::min(std::max(176, (b + 1) * WHIST_STEP), (WHIST_BINS - 1) * WHIST_STEP);
            c->big_thresh = thresh;
            // up to a threshold of 256 the 320-element slice (12 waves per CU) stays: the few tiles it cannot hold are re-run
            // item by item (k_lift_retry); measured on MI355X, 1 M reads, contig indel rate 1e-3: 4.3 ms against 5.3-7.2 ms
            // with 384-element slices.  Workgroup width per slice size as measured (tools/tune.py --contig-indel).
            // Lowest threshold (no heavy tail at all): the 256-element slice, whose kernel has the capacity compiled in and runs 16
            // waves per CU (wgs30x, 2 M reads: 2.28 ms against 2.43 ms with 320-element slices at 12 waves per CU).
            c->cap = thresh <= 176 && !sp && !getenv("PLO_NO_SMALL_CAP") ? TILE_CAP_SMALL : (thresh <= 256 ? 320 : (thresh + 144 + 63) & ~63);
            // the slice holds one window plus the overhang of its last item; weights count two units per block-map entry, ops only one,
            // so the small slice gets by with half the allowance (measured: window 192 2.27 ms, 208 2.22 ms, 224 2.21 ms with 204 of
            // 2 M items re-run) -- until a batch re-runs more than 0.5 % of its items
            c->window = c->cap - (c->cap == TILE_CAP_SMALL && !c->small_window_tight ? 32 : 64);
            c->tile_waves = c->cap <= 320 ? TILE_WAVES : (c->cap <= 448 ? 2 : 1);
            if (getenv("PLO_DEBUG_GEOMETRY"))
                fprintf(stderr, "[plo] batch geometry: thresh %d cap %d window %d tile_waves %d (max weight %u, %llu items beyond the 0.2 %% cut)\n", thresh, c->cap,
                        c->window, c->tile_waves, max_nin, above);
        }
    }
    const uint32_t n_tiles = total_ops / (uint32_t)c->window + 1;
    if (n_items > n_small && !heavy_lanes) {
        HIP_TRY(c, c->tile_lo.ensure((size_t)(n_tiles + 1) * 4));
        hipLaunchKernelGGL(k_tile_bounds, dim3((n_tiles + 1 + 255) / 256), dim3(256), 0, st, (const uint32_t *)c->op_prefix.as<uint32_t>(),
                           n_items, n_tiles, c->window, n_small, c->tile_lo.as<uint32_t>());
    }
    wk.tile_lo = c->tile_lo.as<uint32_t>();
    wk.n_small = n_small;
    HIP_TRY(c, hipEventRecord(c->ev[1], st));

    // launch geometry of the lane-per-item kernel (light items), needed here already: its waves own one output slab each from the start
    uint32_t lane_gs = 64, lane_nblk = 0;
    const size_t lane_lds = (size_t)(c->lane_capw + 2 * c->lane_kvs) * 4 * LANE_WAVES;  // slices + staged block-map entries
    if (n_small) {
        int occ = 1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, sp ? (const void *)k_lift_lanes_sp : (const void *)k_lift_lanes, LANE_WAVES * 64, lane_lds) != hipSuccess || occ < 1)
            occ = 1;
        // items per group: 64, fewer when that leaves resident waves without a group (small batches; the few light items of an
        // indel-dense batch, whose regions would also take a wave's LDS slice several rounds at 64 a group)
        const uint32_t n0 = h_cls[0], n1 = h_cls[1];
        const uint32_t slots = (uint32_t)(c->n_cus * occ) * LANE_WAVES;
        while (lane_gs > 8u && (n0 + lane_gs / 2 - 1) / (lane_gs / 2) + (n1 + lane_gs / 2 - 1) / (lane_gs / 2) <= slots) lane_gs >>= 1;
        if (const char *e = getenv("PLO_LANE_GROUP")) lane_gs = std::min(64u, std::max(1u, (uint32_t)atoi(e)));
        const uint32_t groups = (n0 + lane_gs - 1) / lane_gs + (n1 + lane_gs - 1) / lane_gs;
        lane_nblk = std::min<uint32_t>((groups + LANE_WAVES - 1) / LANE_WAVES, (uint32_t)(c->n_cus * occ));
        lane_nblk = (lane_nblk + 7u) & ~7u;
    }
    size_t want_cigar = (size_t)all_ops * 2 + (size_t)n_items * 8 + 4096 + (size_t)std::min<uint32_t>(n_tiles + 1024, (uint32_t)c->n_cus * 16) * SLAB_OPS +
                        (size_t)lane_nblk * LANE_WAVES * SLAB_OPS;  // (exactly the slabs the lane kernel's waves pre-own: slab_offset below)
    if (c->o_cigar.cap < want_cigar * 4) HIP_TRY(c, c->o_cigar.ensure(want_cigar * 4));

    if (c->seq_pending) {  // (plo_liftover_batch: the read bases arrive on the copy stream)
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_seq, 0));
        c->seq_pending = false;
    }
    unsigned long long *hc = c->h_counters.as<unsigned long long>();
    uint32_t n_big = 0, n_retry = 0, n_mid = 0, n_huge = 0, n_miss = 0, heavy_kernel = 0;
    float miss_ms = 0.f;
    for (int attempt = 0;; ++attempt) {
        wk.out_cigar = c->o_cigar.as<uint32_t>();
        wk.out_cap = c->o_cigar.cap / 4;
        HIP_TRY(c, hipMemsetAsync(c->counters.p, 0, CNT_N * 8, st));
        if (attempt == 0) HIP_TRY(c, hipEventRecord(c->ev[1], st));
        wk.slab_pre = 0;
        wk.slab_offset = 0;
        if (n_small) {
            const uint32_t n0 = h_cls[0], n1 = h_cls[1];
            // groups cut by LDS budget (wider sort windows without the extra rounds of over-full groups) when the groups are of 64
            const bool budget = c->lane_sort && wk.item_region && lane_gs == 64u;
            uint32_t lane_groups_cap_now = 0;
            if (attempt == 0 && c->lane_sort) {
                const uint32_t ch = (uint32_t)(budget ? c->lane_budget_window : c->lane_sort_window);
                const uint32_t chunks = (n0 + ch - 1) / ch + (n1 + ch - 1) / ch;
                uint32_t *n_groups_dev = c->misc.as<uint32_t>() + 32;  // (misc was cleared before the class kernels)
                if (budget) {
                    // most groups a window can have: every group holds at least cap / (largest region) items
                    // (k_chunk_sort cuts a group at 64 items as well as at the slice's capacity)
                    const uint32_t per_group = std::min<uint32_t>(64u, std::max<uint32_t>(1u, (uint32_t)c->lane_capw / (uint32_t)std::max(1, c->lane_max_w)));
                    const size_t max_groups = (size_t)chunks * (ch / per_group + 2);
                    lane_groups_cap_now = (uint32_t)std::min<size_t>(max_groups, 0xffffffffu);
                    HIP_TRY(c, c->lane_groups.ensure(max_groups * 8));
                    if (getenv("PLO_DEBUG_GEOMETRY"))
                        fprintf(stderr, "[plo] lane groups cut by LDS budget: windows of %u, slices of %d dwords, at most %zu groups\n", ch, c->lane_capw, max_groups);
                }
                if (!budget && ch <= 128u)
                    hipLaunchKernelGGL(k_chunk_sort_w, dim3((chunks + 3u) / 4u), dim3(256), 0, st, c->perm.as<uint32_t>(), (const uint32_t *)c->d_n_m.as<uint32_t>(),
                                       (const uint32_t *)c->d_w0.as<uint32_t>(), (const uint32_t *)c->d_w1.as<uint32_t>(), n0, n1, ch, (const uint32_t *)nullptr);
                else
                    hipLaunchKernelGGL(k_chunk_sort, dim3(chunks), dim3(LANE_SORT_THREADS), 0, st, c->perm.as<uint32_t>(), (const uint32_t *)c->d_n_m.as<uint32_t>(),
                                       (const uint32_t *)c->d_w0.as<uint32_t>(), (const uint32_t *)c->d_w1.as<uint32_t>(), n0, n1, ch,
                                       (const uint32_t *)c->item_region.as<uint32_t>(), (uint32_t)c->lane_capw,
                                       budget ? c->lane_groups.as<uint32_t>() : (uint32_t *)nullptr, n_groups_dev, lane_groups_cap_now);
            }
            wk.lane_groups = budget ? c->lane_groups.as<uint32_t>() : nullptr;
            wk.lane_n_groups = c->misc.as<uint32_t>() + 32;
            if (attempt == 0) c->lane_groups_cap = lane_groups_cap_now;
            wk.lane_groups_cap = c->lane_groups_cap;
            const size_t lds = lane_lds;
            const uint32_t gs = lane_gs, nblk = lane_nblk;
            wk.slab_pre = 1u;  // first slab by wave id
            wk.slab_offset = (unsigned long long)nblk * LANE_WAVES * SLAB_OPS;
            PLO_STAT_RANGE(nblk * LANE_WAVES);
            lane_ticket_arm(c, wk, (n0 + gs - 1) / gs + (n1 + gs - 1) / gs, nblk * LANE_WAVES);
            hipLaunchKernelGGL(lane_kernel_of(c, stages, sp), dim3(nblk), dim3(LANE_WAVES * 64), lds, st, ix, bt, wk, stages, n0, n1, gs, c->lane_capw, (const uint32_t *)nullptr);
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipEventRecord(c->ev[4], st));
        if (heavy_lanes) {
            // as many items per wave as it takes to give every resident wave a group (at least 8, at most 64 lanes at work)
            const uint32_t n_heavy = n_items - n_small, n2 = h_cls[2], n3 = n_heavy - n2;
            // three waves per SIMD once every one of their slots gets a full group (k_lift_lanes_g_w3 above); PLO_LANE_G_W3=0/1 forces
            bool w3 = !sp && n_heavy >= (uint32_t)c->n_cus * 3u * LANE_G_WAVES * 64u;
            if (const char *e = getenv("PLO_LANE_G_W3")) w3 = !sp && atoi(e) != 0;
            const int occ = w3 ? 3 : PLO_LANE_G_WPE;  // (4 waves a workgroup, one per SIMD)
            const uint32_t slots = (uint32_t)(c->n_cus * occ) * LANE_G_WAVES;
            uint32_t per = std::min(64u, std::max(8u, (n_heavy + slots - 1) / slots));
            if (const char *e = getenv("PLO_LANE_HEAVY_PER")) per = std::min(64u, std::max(1u, (uint32_t)atoi(e)));
            const uint32_t groups = (n2 + per - 1) / per + (n3 + per - 1) / per;
            uint32_t nblk = std::min<uint32_t>((groups + LANE_G_WAVES - 1) / LANE_G_WAVES, (uint32_t)(c->n_cus * occ));
            // all stages: the streaming kernel (lane_stream.hpp; PLO_LANE_STREAM=0: the kernel over global regions below, which also
            // takes the stage subsets) -- no scratch, every wave an equal contiguous share of either class
            const bool stream = heavy_stream;
            if (stream) {
                // Items per team: 64, one per lane -- more teams than the chip holds are started as others retire, which levels the load
                // better than lanes taking a second item does (measured, stress profile: 64 / 128 / 256 items per team 9.9 / 11.4 / 20.8 ms
                // at 100 k reads, 30.6 / 32.6 / 41 ms at 500 k: a team is as slow as its last lane, and with 80 items on 64 lanes the second
                // half of its run has a quarter of the lanes at work).  A batch too small to give every CU four teams of 64 is spread over
                // as many teams with fewer lanes each (at least 8).
                const uint32_t full = 64u * (uint32_t)c->n_cus * 4u;
                uint32_t per_team = n_heavy >= full ? 64u : std::min(64u, std::max(8u, (n_heavy + (uint32_t)c->n_cus * 4u - 1) / ((uint32_t)c->n_cus * 4u)));
                int tocc = 0;
                if (getenv("PLO_DEBUG_GEOMETRY") && hipOccupancyMaxActiveBlocksPerMultiprocessor(&tocc, sp ? (const void *)k_lift_stream_sp : (const void *)k_lift_stream, PIPE_WAVES * 64, 0) != hipSuccess) tocc = 0;
                if (const char *e = getenv("PLO_LANE_HEAVY_PER")) per_team = std::min(4096u, std::max(1u, (uint32_t)atoi(e)));
                // (every wave of the launch has a statistics slot)
                while (((unsigned long long)(n2 + per_team - 1) / per_team + (n3 + per_team - 1) / per_team) * PIPE_WAVES + stat_used > STAT_SLOTS) per_team *= 2;
                const uint32_t t0 = (n2 + per_team - 1) / per_team, t1 = (n3 + per_team - 1) / per_team;
                nblk = t0 + t1;
                if (getenv("PLO_DEBUG_GEOMETRY"))
                    fprintf(stderr, "[plo] heavy items through the streaming lane kernel: %u + %u items, %u + %u teams of %d waves (%d teams per CU), %u items per team\n", n2, n3,
                            t0, t1, PIPE_WAVES, tocc, per_team);
                wk.slab_pre = 0u;
                if (!n_small) wk.slab_offset = 0ull;
                PLO_STAT_RANGE(nblk * PIPE_WAVES);
                heavy_kernel = 3u;
                const uint32_t xcd = getenv("PLO_PIPE_XCD") ? (uint32_t)(atoi(getenv("PLO_PIPE_XCD")) != 0) : 0u;  // (measured: 12.05 against 9.21 ms with it, FETCH_SIZE +17 %: more teams than the chip holds are dispatched in order, and the remap sends the early ones to one XCD)
                if (sp) hipLaunchKernelGGL(k_lift_stream_sp, dim3(nblk), dim3(PIPE_WAVES * 64), 0, st, ix, bt, wk, n_small, n_small + n2, n_items, t0, t1, xcd);
                else hipLaunchKernelGGL(k_lift_stream, dim3(nblk), dim3(PIPE_WAVES * 64), 0, st, ix, bt, wk, n_small, n_small + n2, n_items, t0, t1, xcd);
            } else {
                // Regions start on 128-byte lines and hold the heaviest item of the batch (64: room for the liftover's gap, lane_region_gap)
                // -- unless that one is an outlier: the regions of all resident lanes together are kept within 8 GB, an item too long for
                // its region then is handed to the retry list (wave-cooperative code, whatever its size) like any other that outgrows it.
                int stride = (int)((max_nin + LANE_SLACK + 64u + LANE_REGION_PAD + 31u) & ~31u);
                {
                    const unsigned long long fit = (8ull << 30) / (4ull * per * LANE_G_WAVES * std::max(1u, nblk));
                    const int cap_stride = (int)std::max<unsigned long long>(1024ull, std::min<unsigned long long>(fit, 0x7fffffe0ull) & ~31ull);
                    stride = std::min(stride, cap_stride);
                    if (const char *e = getenv("PLO_LANE_HEAVY_STRIDE")) stride = std::max(LANE_REGION_PAD + 64, atoi(e)) & ~31;
                }
                const unsigned long long per_wave = (unsigned long long)per * (unsigned long long)stride * 4ull;
                nblk = (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>(nblk, (16ull << 30) / (per_wave * LANE_G_WAVES)));
                HIP_TRY(c, c->lane_scratch.ensure((size_t)(per_wave * LANE_G_WAVES * nblk)));
                if (getenv("PLO_DEBUG_GEOMETRY"))
                    fprintf(stderr, "[plo] heavy items through the lane-per-item code: %u items, %u per wave, %u workgroups, regions of %d dwords, %.1f MB scratch\n", n_heavy, per,
                            nblk, stride, per_wave * LANE_G_WAVES * nblk / 1e6);
                wk.slab_pre = 0u;  // (a group's output is a slab of its own; the light items' waves own the first slabs, if any)
                if (!n_small) wk.slab_offset = 0ull;
                PLO_STAT_RANGE(nblk * LANE_G_WAVES);
                heavy_kernel = w3 ? 2u : 1u;
                if (sp) hipLaunchKernelGGL(k_lift_lanes_g_sp, dim3(nblk), dim3(LANE_G_WAVES * 64), 0, st, ix, bt, wk, stages, n_small, n_small + n2, n_items, per, c->lane_scratch.as<uint32_t>(), stride);
                else if (w3) hipLaunchKernelGGL(k_lift_lanes_g_w3, dim3(nblk), dim3(LANE_G_WAVES * 64), 0, st, ix, bt, wk, stages, n_small, n_small + n2, n_items, per, c->lane_scratch.as<uint32_t>(), stride);
                else hipLaunchKernelGGL(k_lift_lanes_g, dim3(nblk), dim3(LANE_G_WAVES * 64), 0, st, ix, bt, wk, stages, n_small, n_small + n2, n_items, per, c->lane_scratch.as<uint32_t>(), stride);
            }
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(c->ev[2], st));
        } else if (n_items > n_small) {
            uint32_t lds_per_wave = (uint32_t)((tile_mem_bytes(c->cap) + 15) & ~(size_t)15);
            if (const char *e = getenv("PLO_LDS_PAD")) lds_per_wave += (uint32_t)atoi(e) & ~15u;  // occupancy experiments
            const uint32_t tw = (uint32_t)c->tile_waves;
            uint32_t nblk = (n_tiles + tw - 1) / tw;
            // persistent grid: what the chip keeps resident (CUs x blocks per CU), a multiple of 8 for the XCD mapping
            int occ = 1;
            const bool c256 = !sp && c->cap == TILE_CAP_SMALL && tw == (uint32_t)TILE_WAVES && lds_per_wave == (uint32_t)((tile_mem_bytes(TILE_CAP_SMALL) + 15) & ~(size_t)15);
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, sp ? (const void *)k_lift_tiles_sp : (c256 ? (const void *)k_lift_tiles_c256 : (const void *)k_lift_tiles), (int)tw * 64,
                                                             (size_t)lds_per_wave * tw) != hipSuccess || occ < 1)
                occ = 1;
            nblk = std::min<uint32_t>(nblk, (uint32_t)(c->n_cus * occ));
            nblk = (nblk + 7u) & ~7u;
            wk.slab_pre = n_small == 0 ? 1u : 0u;  // nothing has been reserved yet (the lane kernel did not run)
            if (wk.slab_pre) wk.slab_offset = (unsigned long long)nblk * tw * SLAB_OPS;  // (else: the lane kernel's waves own the first slabs)
            PLO_STAT_RANGE(nblk * tw);
            if (sp)
                hipLaunchKernelGGL(k_lift_tiles_sp, dim3(nblk), dim3(tw * 64), lds_per_wave * tw, st, ix, bt, wk, stages, n_tiles, c->window,
                                   c->big_thresh, c->cap, lds_per_wave);
            else if (c256)
                hipLaunchKernelGGL(k_lift_tiles_c256, dim3(nblk), dim3(tw * 64), lds_per_wave * tw, st, ix, bt, wk, stages, n_tiles, c->window,
                                   c->big_thresh, c->cap, lds_per_wave);
            else
                hipLaunchKernelGGL(k_lift_tiles, dim3(nblk), dim3(tw * 64), lds_per_wave * tw, st, ix, bt, wk, stages, n_tiles, c->window,
                                   c->big_thresh, c->cap, lds_per_wave);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(c->ev[2], st));
        } else {
            HIP_TRY(c, hipEventRecord(c->ev[2], st));
        }
        if (n_items) {
            // Items of tiles whose intermediates overflowed the slice (and items the lane kernel handed on), one per wave with a slice of twice the threshold (the shift /
            // simplify stages at most double an item's ops).  Launched without asking the host how many there are: the kernel reads
            // the count the tile kernel left (mostly zero -- a few microseconds -- and a host round trip less when it is not).
            // Batches without tiles (light items only, or heavy items through the lane code) have computed no tile geometry: the routing
            // threshold then comes from the batch's heaviest item, not from whatever an earlier batch left in the context.
            int r_thresh = c->big_thresh, r_cap = c->cap;
            if (c->adaptive && !(n_items > n_small && !heavy_lanes)) {
                r_thresh = heavy_lanes ? (int)std::min<uint32_t>(std::max<uint32_t>(256u, max_nin), 2016u) : 256;
                r_cap = 320;
            }
            const int retry_cap = std::min(4096, std::max(r_cap, (2 * r_thresh + 64 + 63) & ~63));
            uint32_t lds = (uint32_t)((tile_mem_bytes(retry_cap) + 15) & ~(size_t)15);
            uint32_t nw = (uint32_t)c->n_cus * 2u;
            PLO_STAT_RANGE(nw);
            if (sp) hipLaunchKernelGGL(k_lift_retry_sp, dim3(nw), dim3(64), lds, st, ix, bt, wk, stages, 0xffffffffu, r_thresh, retry_cap);
            else hipLaunchKernelGGL(k_lift_retry, dim3(nw), dim3(64), lds, st, ix, bt, wk, stages, 0xffffffffu, r_thresh, retry_cap);
            HIP_TRY(c, hipGetLastError());
        }
        HIP_TRY(c, hipEventRecord(c->ev[5], st));
        PLO_READ_COUNTERS();
        n_retry = (uint32_t)hc[CNT_NRETRY];
        n_big = (uint32_t)hc[CNT_NBIG];
        n_mid = 0;
        n_huge = n_big;
        const uint32_t *huge_src = c->big_list.as<uint32_t>();
        if (n_big && c->mid_waves) {
            // One workgroup per item.  Capacity from the heaviest item of the batch: the stages at most add a deletion per block
            // (already in the weight) and re-shape indel clusters, so a quarter on top of the weight holds every intermediate of
            // all but pathological items; those, and items beyond the largest slice, go on to the global-scratch kernel.
            int cap = std::min<unsigned long long>((unsigned long long)c->mid_cap_max, (((unsigned long long)max_nin * 5 / 4 + 64 + 63) & ~63ull));
            cap = std::max(cap, 512);
            const int mid_thresh = (cap - 64) * 4 / 5;
            const int nw = c->mid_waves;
            const size_t lds = nw == 16 ? mid_lds_bytes<16>(cap) : mid_lds_bytes<8>(cap);
            const void *fn = sp ? (nw == 16 ? (const void *)k_lift_mid_sp<16> : (const void *)k_lift_mid_sp<8>)
                                : (nw == 16 ? (const void *)k_lift_mid<16> : (const void *)k_lift_mid<8>);
            int occ = 1;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, nw * 64, lds) != hipSuccess || occ < 1) occ = 1;
            uint32_t nblk = std::min<uint32_t>(n_big, (uint32_t)(c->n_cus * occ));
            HIP_TRY(c, c->huge_list.ensure((size_t)n_big * 4));
            wk.huge_list = c->huge_list.as<uint32_t>();
            if (getenv("PLO_DEBUG_GEOMETRY"))
                fprintf(stderr, "[plo] workgroup-per-item kernel: %u items, %d waves, cap %d (threshold %d), %zu B LDS, %d workgroups per CU\n", n_big, nw,
                        cap, mid_thresh, lds, occ);
            PLO_STAT_RANGE(nblk * (uint32_t)nw);
            if (sp && nw == 16)
                hipLaunchKernelGGL(k_lift_mid_sp<16>, dim3(nblk), dim3(16 * 64), lds, st, ix, bt, wk, stages, n_big, mid_thresh, cap);
            else if (sp)
                hipLaunchKernelGGL(k_lift_mid_sp<8>, dim3(nblk), dim3(8 * 64), lds, st, ix, bt, wk, stages, n_big, mid_thresh, cap);
            else if (nw == 16)
                hipLaunchKernelGGL(k_lift_mid<16>, dim3(nblk), dim3(16 * 64), lds, st, ix, bt, wk, stages, n_big, mid_thresh, cap);
            else
                hipLaunchKernelGGL(k_lift_mid<8>, dim3(nblk), dim3(8 * 64), lds, st, ix, bt, wk, stages, n_big, mid_thresh, cap);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(c->ev[6], st));
            c->ev_mid = true;
            PLO_READ_COUNTERS();
            n_huge = (uint32_t)hc[CNT_NHUGE];
            n_mid = n_big - n_huge;
            huge_src = c->huge_list.as<uint32_t>();
        }
        if (n_huge) {
            // size the wave-private scratch from the largest possible intermediate of a single item
            // (pieces <= ops + blocks, raw ops <= 2 x pieces); an item that still overflows is reported (CNT_ERROR)
            int big_cap = 4096;
            while (big_cap < (1 << 22) && (unsigned long long)big_cap < 6ull * max_nin + 2048ull) big_cap <<= 1;
            if (const char *e = getenv("PLO_BIG_CAP")) big_cap = std::max(1024, atoi(e));
            unsigned long long bpw = (tile_mem_bytes(big_cap) + 255) & ~(unsigned long long)255;
            // as many waves as the chip keeps resident (register-limited: 3 per SIMD), bounded by a 4 GiB scratch
            uint32_t nw = std::min<uint32_t>(n_huge, (uint32_t)c->n_cus * 12u);
            nw = (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>(nw, (4ull << 30) / bpw));
            HIP_TRY(c, c->scratch.ensure((size_t)bpw * nw));
            PLO_STAT_RANGE(nw);
            if (sp)
                hipLaunchKernelGGL(k_lift_big_sp, dim3(nw), dim3(64), 0, st, ix, bt, wk, stages, n_huge, huge_src, c->scratch.as<unsigned char>(),
                                   big_cap, bpw);
            else
                hipLaunchKernelGGL(k_lift_big, dim3(nw), dim3(64), 0, st, ix, bt, wk, stages, n_huge, huge_src, c->scratch.as<unsigned char>(),
                                   big_cap, bpw);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(c->ev[3], st));
            c->ev_big = true;
            PLO_READ_COUNTERS();
        }
        n_miss = (uint32_t)hc[CNT_NMISS];
        if (n_miss && in->seq_full && in->read_seq_full_off) {
            // second look at the items that reached bases a sparse batch does not carry: their reads' complete bases go up now
            const auto t0 = std::chrono::steady_clock::now();
            HIP_TRY(c, c->miss_info.ensure((size_t)n_miss * 8));
            HIP_TRY(c, c->h_miss.ensure((size_t)n_miss * 16));
            uint32_t *d_read = c->miss_info.as<uint32_t>(), *d_len = d_read + n_miss;
            hipLaunchKernelGGL(k_miss_info, dim3((n_miss + 255) / 256), dim3(256), 0, st, (const uint32_t *)c->miss_list.as<uint32_t>(), n_miss,
                               bt, wk, d_read, d_len);
            uint32_t *h_read = c->h_miss.as<uint32_t>(), *h_len = h_read + n_miss;
            HIP_TRY(c, hipMemcpyAsync(h_read, d_read, (size_t)n_miss * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st)); ++n_syncs;
            std::vector<uint32_t> order(n_miss);
            for (uint32_t k = 0; k < n_miss; ++k) order[k] = k;
            std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return h_read[a] < h_read[b]; });
            uint64_t *h_vals = (uint64_t *)(h_read + 2 * (size_t)n_miss);
            uint64_t total = 0;
            for (uint32_t k = 0; k < n_miss; ++k) {  // one copy per read, 16-byte aligned, 16 spare bytes for the wide window loads
                const uint32_t a = order[k];
                if (k && h_read[order[k - 1]] == h_read[a]) {
                    h_vals[a] = h_vals[order[k - 1]];
                    continue;
                }
                h_vals[a] = total;
                total += ((((uint64_t)h_len[a] + 1) / 2 + 15) & ~15ull) + 16;
            }
            HIP_TRY(c, c->h_side.ensure((size_t)total));
            HIP_TRY(c, c->miss_side.ensure((size_t)total));
            HIP_TRY(c, c->miss_vals.ensure((size_t)n_miss * 8));
            HIP_TRY(c, c->miss_seq_off.ensure((size_t)std::max(1u, n_items) * 8));
            for (uint32_t k = 0; k < n_miss; ++k) {
                const uint32_t a = order[k];
                if (k && h_read[order[k - 1]] == h_read[a]) continue;
                const size_t nb = ((size_t)h_len[a] + 1) / 2;
                uint8_t *dst = c->h_side.as<uint8_t>() + h_vals[a];
                memcpy(dst, in->seq_full + in->read_seq_full_off[h_read[a]], nb);
                memset(dst + nb, 0, (((nb + 15) & ~(size_t)15) + 16) - nb);
            }
            HIP_TRY(c, hipMemcpyAsync(c->miss_side.p, c->h_side.p, (size_t)total, hipMemcpyHostToDevice, st));
            HIP_TRY(c, hipMemcpyAsync(c->miss_vals.p, h_vals, (size_t)n_miss * 8, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_miss_patch, dim3((n_miss + 255) / 256), dim3(256), 0, st, (const uint32_t *)c->miss_list.as<uint32_t>(), n_miss,
                               (const uint64_t *)c->miss_vals.as<uint64_t>(), c->miss_seq_off.as<uint64_t>());
            DevBatch bt2 = bt;
            bt2.seq = c->miss_side.as<uint8_t>();
            bt2.seq_bytes = total;
            bt2.seq_fmt = PLO_SEQ_BAM4;
            DevWork wk2 = wk;
            wk2.d.seq_off = c->miss_seq_off.as<uint64_t>();
            int big_cap = 4096;
            while (big_cap < (1 << 22) && (unsigned long long)big_cap < 6ull * max_nin + 2048ull) big_cap <<= 1;
            if (const char *e = getenv("PLO_BIG_CAP")) big_cap = std::max(1024, atoi(e));
            unsigned long long bpw = (tile_mem_bytes(big_cap) + 255) & ~(unsigned long long)255;
            uint32_t nw = std::min<uint32_t>(n_miss, (uint32_t)c->n_cus * 12u);
            nw = (uint32_t)std::max<unsigned long long>(1ull, std::min<unsigned long long>(nw, (4ull << 30) / bpw));
            HIP_TRY(c, c->scratch.ensure((size_t)bpw * nw));
            wk2.stat_base = stat_used;
            stat_used += nw;
            hipLaunchKernelGGL(k_lift_big, dim3(nw), dim3(64), 0, st, ix, bt2, wk2, stages, n_miss, (const uint32_t *)c->miss_list.as<uint32_t>(),
                               c->scratch.as<unsigned char>(), big_cap, bpw);
            HIP_TRY(c, hipGetLastError());
            PLO_READ_COUNTERS();
            miss_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        if (hc[CNT_OVERFLOW] == 0) break;
        if (attempt >= 3) {
            c->err = "output CIGAR buffer kept overflowing";
            return PLO_ERR_INTERNAL;
        }
        HIP_TRY(c, c->o_cigar.ensure((size_t)(hc[CNT_CIGAR] + wk.slab_offset + 4096 + (size_t)std::min<uint32_t>(n_tiles + 1024, (uint32_t)c->n_cus * 16) * SLAB_OPS) * 4));
    }
    if (hc[CNT_ERROR]) {
        c->err = "an item exceeded the large-item scratch capacity (raise PLO_BIG_CAP), or the lane kernel's group list its capacity";
        return PLO_ERR_INTERNAL;
    }
    c->timing.n_items = n_items;
    c->timing.n_big_items = n_huge;
    c->timing.n_mid_items = n_mid;
    c->timing.n_miss_items = n_miss;
    c->timing.tile_cap = (uint32_t)c->cap;
    c->timing.tile_window = (uint32_t)c->window;
    c->timing.miss_ms = miss_ms;
    c->timing.n_lane_items = n_small;
    c->timing.n_heavy_lane_items = heavy_lanes ? n_items - n_small : 0u;
    c->timing.heavy_kernel = heavy_kernel;
    c->timing.host_syncs = n_syncs + c->fast_extra_syncs;
    c->fast_extra_syncs = 0;
    c->fast_ns_cap = ns;
    // (PLO_FAST_CAP_EXACT=1, tests: the last batch's item count, so that a window with a few items more exercises the VERR_CAP fallback)
    c->fast_item_cap = getenv("PLO_FAST_CAP_EXACT") ? n_items : std::max(n_items, c->item_cap_now);
    c->fast_ref_items = n_items;
    c->fast_ref_ns = ns;
    c->fast_n0 = h_cls[0];
    c->fast_n1 = h_cls[1];
    // (items the lane kernel handed to the retry kernel are fine: the fast path runs that kernel too; items IT hands on are not)
    c->fast_light_only = n_items > 0 && n_items == n_small && n_big == 0 && n_miss == 0;
    c->timing.n_retry_items = n_retry;
    if (c->adaptive && c->cap == TILE_CAP_SMALL && n_retry > n_items / 200) c->small_window_tight = true;
    c->timing.n_in_ops = hc[CNT_IN_OPS];
    c->timing.n_out_ops = hc[CNT_OUT_OPS];
    c->timing.algo_bytes = hc[CNT_ALGO_BYTES];
    c->timing.lane_utilisation = hc[CNT_LANE_TRIPS] ? (float)((double)hc[CNT_LANE_ACT] / (64.0 * (double)hc[CNT_LANE_TRIPS])) : 0.0f;
    for (int k = 0; k < 12; ++k) c->phase_cycles[k] = hc[CNT_PHASE0 + k];

    out->n_items = n_items;
    out->item_seg = c->item_seg.as<uint32_t>();
    out->item_cseg = c->item_cseg.as<uint32_t>();
    out->item_status = c->o_status.as<uint8_t>();
    out->item_need_flipped = c->o_flip.as<uint8_t>();
    out->item_mapq = c->o_mapq.as<uint8_t>();
    out->item_chrom_index = c->o_chrom.as<uint32_t>();
    out->item_ref_pos = c->o_pos.as<int64_t>();
    out->item_cigar_off = c->o_coff.as<uint64_t>();
    out->item_cigar_len = c->o_clen.as<uint32_t>();
    out->cigar = c->o_cigar.as<uint32_t>();
    out->n_cigar = hc[CNT_CIGAR] + wk.slab_offset;
    c->last_wk = wk;
    c->last_bt = bt;
    c->have_last = true;
    c->have_finish = false;
    c->have_sa = false;
    return PLO_OK;
}

// One host round trip per batch.  The enumerate kernels, the class order, k_lift_lanes and k_lift_retry are launched
// back to back with the item and class counts read from DEVICE memory (k_cls_hist / k_permute2 / k_chunk_sort_w / k_lift_lanes take them by
// pointer; grids are sized by the arrays' capacity, surplus workgroups leave at once); the one copy at the end brings the item count, the
// validation flags, the class counts and the counters.  `fallback`: the batch does not fit what the context's last batch left (more items
// than the arrays hold, heavy items, items handed on by the retry kernel, an output overflow): nothing of it is used.
static plo_status liftover_fast(plo_ctx *c, const plo_batch_in *in, uint32_t stages, plo_batch_out *out, const DevBatch &bt, bool &fallback) {
    fallback = false;
    const DevIndex &ix = c->ix->d;
    hipStream_t st = c->stream;
    const uint32_t ns = in->n_segs;
    // The item capacity the kernels are launched with: what the arrays hold -- but no more than this batch can plausibly need (a quarter more
    // items per segment than the last careful batch had, + 1 024).  A context that has once lifted a 2 M-read batch would otherwise run every
    // 50 k-read window with grids for 2 M items: surplus workgroups leave at once, yet a thousand of them per class kernel and a lane grid of
    // every wave slot cost the call ~20 us (tools/ab_window.py).  A batch with more items raises VERR_CAP like one beyond the arrays.
    uint32_t cap = c->fast_item_cap;
    if (c->fast_launch_bound && c->fast_ref_ns) {
        const unsigned long long per = ((unsigned long long)ns * c->fast_ref_items + c->fast_ref_ns - 1) / c->fast_ref_ns;
        cap = (uint32_t)std::min<unsigned long long>(cap, per + per / 4 + 1024ull);
    }
    // Everything the kernels of this path count in, one block: cleared by ONE fill and read back by ONE copy (a launch of any size costs
    // ~5 us on the stream: three fills and four copies were a quarter of a 50 k-read call's kernels, tools/trace_window.sh)
    //   [0, 256) the class totals ([6] = the item count) and the lane kernel's group counter, [256, 272) the validation flags,
    //   [512, 512 + 8 CNT_N) the batch counters
    constexpr size_t FB_VERR = 256, FB_COUNTERS = 512, FB_BYTES = 1024, FB_BACK = FB_COUNTERS + CNT_N * 8;
    static_assert(FB_BACK <= FB_BYTES, "fast block");
    //   [288, 292) the scan's ticket, [FB_BYTES, ...) the scan's tile words
    constexpr size_t FB_TICKET = 288;
    const bool chain = c->scan_chain;
    const uint32_t scan_nb = std::max(1u, (ns + SCAN_BLOCK - 1) / SCAN_BLOCK);
    const size_t fb_bytes = FB_BYTES + (chain ? (size_t)scan_nb * 8 : 0);
    HIP_TRY(c, c->fast_blk.ensure(fb_bytes));
    HIP_TRY(c, c->h_counters.ensure(FB_BYTES));
    uint8_t *const fb = c->fast_blk.as<uint8_t>();
    uint32_t *const misc_d = (uint32_t *)fb, *const verr_d = (uint32_t *)(fb + FB_VERR);
    unsigned long long *const counters_d = (unsigned long long *)(fb + FB_COUNTERS);
    const bool ev_on = c->phase_events;  // (plo_ctx_set_phase_events(ctx, 0): no event records -- two bubbles of ~6 us fewer on the stream, no phase times)
    if (ev_on) HIP_TRY(c, hipEventRecord(c->ev[0], st));
    HIP_TRY(c, hipMemsetAsync(fb, 0, fb_bytes, st));
    hipLaunchKernelGGL(k_seg_count, dim3((unsigned)(((unsigned long long)ns * SEG_LANES + 255) / 256)), dim3(256), 0, st, ix, bt, c->seg_cnt.as<uint32_t>(),
                       c->seg_reflen.as<int>(), c->seg_readlen.as<uint32_t>(), c->seg_nm.as<uint32_t>(), verr_d);
    if (chain) {
        hipLaunchKernelGGL(k_scan_chain, dim3(scan_nb), dim3(SCAN_THREADS), 0, st, (const uint32_t *)c->seg_cnt.as<uint32_t>(), ns, c->seg_off.as<uint32_t>(),
                           (unsigned long long *)(fb + FB_BYTES), (uint32_t *)(fb + FB_TICKET));
    } else {
        plo_status s = scan_u32(c, c->seg_cnt.as<uint32_t>(), ns, c->seg_off.as<uint32_t>());
        if (s != PLO_OK) return s;
    }
    const uint32_t *n_dev = c->seg_off.as<uint32_t>() + ns, *totals_dev = misc_d;
    DevWork wk;
    fill_work(c, wk, cap);
    wk.counters = counters_d;
    hipLaunchKernelGGL(k_item_emit, dim3((ns + 255) / 256), dim3(256), 0, st, ix, bt, wk, stages, (const uint32_t *)c->seg_off.as<uint32_t>(), c->seg_reflen.as<int>(),
                       cap, verr_d);
    const uint32_t cls_nb = (cap + CLS_BLOCK - 1) / CLS_BLOCK;
    HIP_TRY(c, c->cls_partial.ensure((size_t)std::max(1u, cls_nb) * 6 * 4));
    hipLaunchKernelGGL(k_cls_hist, dim3(cls_nb), dim3(CLS_THREADS), 0, st, (const uint32_t *)c->item_cls.as<uint32_t>(), (const uint32_t *)c->item_nin.as<uint32_t>(), cap,
                       cls_nb, c->cls_partial.as<uint32_t>(), n_dev);
    hipLaunchKernelGGL(k_permute2_s, dim3(cls_nb), dim3(CLS_THREADS), 0, st, (const uint32_t *)c->item_cls.as<uint32_t>(), (const uint32_t *)c->item_nin.as<uint32_t>(),
                       (const uint32_t *)c->cls_partial.as<uint32_t>(), misc_d, cap, cls_nb, c->perm.as<uint32_t>(), c->nin_p.as<uint32_t>(),
                       c->adaptive ? (uint32_t)((WHIST_BINS - 1) * WHIST_STEP) : 0xffffffffu, n_dev);
    if (ev_on) HIP_TRY(c, hipEventRecord(c->ev[1], st));
    // launch geometry from the last batch's class counts (a window of the same shape has the same): group size, persistent grid
    uint32_t lane_gs = 64, lane_nblk = 0;
    const size_t lane_lds = (size_t)(c->lane_capw + 2 * c->lane_kvs) * 4 * LANE_WAVES;
    {
        int occ = 1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)k_lift_lanes, LANE_WAVES * 64, lane_lds) != hipSuccess || occ < 1) occ = 1;
        const uint32_t n0 = c->fast_n0, n1 = c->fast_n1, slots = (uint32_t)(c->n_cus * occ) * LANE_WAVES;
        while (lane_gs > 8u && (n0 + lane_gs / 2 - 1) / (lane_gs / 2) + (n1 + lane_gs / 2 - 1) / (lane_gs / 2) <= slots) lane_gs >>= 1;
        if (const char *e = getenv("PLO_LANE_GROUP")) lane_gs = std::min(64u, std::max(1u, (uint32_t)atoi(e)));
        // (groups of this batch: at most cap / gs + 2 -- one partial group per class)
        const uint32_t groups = cap / lane_gs + 2;
        lane_nblk = std::min<uint32_t>((groups + LANE_WAVES - 1) / LANE_WAVES, (uint32_t)(c->n_cus * occ));
        lane_nblk = (lane_nblk + 7u) & ~7u;
    }
    const uint32_t ch = (uint32_t)c->lane_sort_window;
    hipLaunchKernelGGL(k_chunk_sort_w, dim3((cap / ch + 2u + 3u) / 4u), dim3(256), 0, st, c->perm.as<uint32_t>(), (const uint32_t *)c->d_n_m.as<uint32_t>(),
                       (const uint32_t *)c->d_w0.as<uint32_t>(), (const uint32_t *)c->d_w1.as<uint32_t>(), 0u, 0u, ch, totals_dev);
    wk.out_cigar = c->o_cigar.as<uint32_t>();
    wk.out_cap = c->o_cigar.cap / 4;
    wk.slab_pre = 1u;
    wk.slab_offset = (unsigned long long)lane_nblk * LANE_WAVES * SLAB_OPS;
    wk.n_small = cap;  // (unused by the lane kernel; the retry kernel's tiles take their items from the retry list)
    wk.lane_n_groups = misc_d + 32;
    wk.stat_base = 0;
    uint32_t stat_used = lane_nblk * LANE_WAVES;
    if (wk.slab_offset + SLAB_OPS > wk.out_cap) {  // the output buffer of the last batch does not even hold the waves' first slabs
        fallback = true;
        return PLO_OK;
    }
    if (c->seq_pending) {  // (plo_liftover_batch: the read bases arrive on the copy stream)
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_seq, 0));
        c->seq_pending = false;
    }
    lane_ticket_arm(c, wk, (c->fast_n0 + lane_gs - 1) / lane_gs + (c->fast_n1 + lane_gs - 1) / lane_gs, lane_nblk * LANE_WAVES);  // (the last batch's class counts)
    hipLaunchKernelGGL(lane_kernel_of(c, stages, false), dim3(lane_nblk), dim3(LANE_WAVES * 64), lane_lds, st, ix, bt, wk, stages, 0u, 0u, lane_gs, c->lane_capw, totals_dev);
    HIP_TRY(c, hipGetLastError());
    if (ev_on) HIP_TRY(c, hipEventRecord(c->ev[4], st));  // (the last event of this path: every record is a ~5 us bubble on the stream; retry and counters are not timed)
    {
        const int retry_cap = 320;
        const uint32_t lds = (uint32_t)((tile_mem_bytes(retry_cap) + 15) & ~(size_t)15), nw = (uint32_t)c->n_cus * 2u;
#ifdef PLO_PHASE_TIMING
        const bool fuse = false;  // (timing builds: the waves' clocks travel in their slots, wave_ctx_flush)
#else
        const bool fuse = c->fast_fuse;
#endif
        if (fuse) {  // the counters' sum rides in the retry launch: its waves add their own counts, the first of them the light-item kernel's slots
            hipLaunchKernelGGL(k_lift_retry_sum, dim3(std::max(nw, SUM_BLOCKS)), dim3(64), lds, st, ix, bt, wk, stages, 256, retry_cap, stat_used);
            HIP_TRY(c, hipGetLastError());
        } else {
            wk.stat_base = stat_used;
            stat_used += nw;
            hipLaunchKernelGGL(k_lift_retry, dim3(nw), dim3(64), lds, st, ix, bt, wk, stages, 0xffffffffu, 256, retry_cap);
            HIP_TRY(c, hipGetLastError());
            hipLaunchKernelGGL(k_sum_stats, dim3(std::min<uint32_t>((stat_used + 255) / 256, 16u)), dim3(256), 0, st, c->wave_stats.as<unsigned long long>(), stat_used,
                               counters_d);
        }
    }
    // the one look: class totals and item count, validation flags, counters
    uint8_t *const hb = c->h_counters.as<uint8_t>();
    HIP_TRY(c, hipMemcpyAsync(hb, fb, FB_BACK, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const unsigned long long *hc = (const unsigned long long *)(hb + FB_COUNTERS);
    const uint32_t *const hm = (const uint32_t *)hb;
    const uint32_t hx[8] = {hm[6], *(const uint32_t *)(hb + FB_VERR), hm[0], hm[1], hm[2], hm[3], hm[4], hm[5]};
    const uint32_t n_items = hx[0], verr = hx[1], n0 = hx[2], n1 = hx[3];
    if (verr & (VERR_INDEX | VERR_RANGE)) {
        if (verr & VERR_INDEX) {
            c->err = "plo_batch_in: an index points outside its array (seg_read / seg_contig / seg_cigar_off / read_seq_off / item_seg / item_cseg)";
            return PLO_ERR_INVALID_ARG;
        }
        c->err = "plo_batch_in: coordinate outside the 31-bit BAM range, CIGAR op code above 8, a CIGAR spanning 2^30 bases or more, or a read segment that ends behind its contig's end on a reverse-strand contig segment";
        return PLO_ERR_RANGE;
    }
    const unsigned long long all_ops = (unsigned long long)hx[6] | ((unsigned long long)hx[7] << 32);
    if ((verr & VERR_CAP) || n_items > cap || n0 + n1 != n_items || all_ops > 0x7fffffffull || hc[CNT_OVERFLOW] || hc[CNT_NBIG] || hc[CNT_NMISS] || hc[CNT_ERROR] ||
        (unsigned long long)(n0 / lane_gs + n1 / lane_gs + 2) > (unsigned long long)lane_nblk * LANE_WAVES * 0xffffull) {
        fallback = true;  // more items than the arrays hold / heavy items / handed-on items / output overflow: the careful path runs the batch
        return PLO_OK;
    }
    memset(&c->timing, 0, sizeof(c->timing));
    c->ev_big = false;
    c->ev_mid = false;
    c->timing.n_items = n_items;
    c->timing.tile_cap = (uint32_t)c->cap;
    c->timing.tile_window = (uint32_t)c->window;
    c->timing.n_lane_items = n_items;
    c->timing.n_retry_items = (uint32_t)hc[CNT_NRETRY];
    c->timing.n_in_ops = hc[CNT_IN_OPS];
    c->timing.n_out_ops = hc[CNT_OUT_OPS];
    c->timing.algo_bytes = hc[CNT_ALGO_BYTES];
    c->timing.lane_utilisation = hc[CNT_LANE_TRIPS] ? (float)((double)hc[CNT_LANE_ACT] / (64.0 * (double)hc[CNT_LANE_TRIPS])) : 0.0f;
    c->timing.host_syncs = 1;
    c->fast_timing = true;
    c->fast_no_events = !ev_on;
    for (int k = 0; k < 12; ++k) c->phase_cycles[k] = hc[CNT_PHASE0 + k];
    c->fast_n0 = n0;
    c->fast_n1 = n1;
    out->n_items = n_items;
    out->item_seg = c->item_seg.as<uint32_t>();
    out->item_cseg = c->item_cseg.as<uint32_t>();
    out->item_status = c->o_status.as<uint8_t>();
    out->item_need_flipped = c->o_flip.as<uint8_t>();
    out->item_mapq = c->o_mapq.as<uint8_t>();
    out->item_chrom_index = c->o_chrom.as<uint32_t>();
    out->item_ref_pos = c->o_pos.as<int64_t>();
    out->item_cigar_off = c->o_coff.as<uint64_t>();
    out->item_cigar_len = c->o_clen.as<uint32_t>();
    out->cigar = c->o_cigar.as<uint32_t>();
    out->n_cigar = hc[CNT_CIGAR] + wk.slab_offset;
    wk.n_items = n_items;
    wk.n_small = n_items;
    c->last_wk = wk;
    c->last_bt = bt;
    c->have_last = true;
    c->have_finish = false;
    c->have_sa = false;
    return PLO_OK;
}

plo_status plo_finish_batch_dev(plo_ctx *c, const plo_batch_in *in, const plo_finish_in *fin, plo_finish_out *out) {
    if (!c || !in || !fin || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    c->err.clear();
    if (!c->have_last || c->last_bt.n_segs != in->n_segs || c->last_bt.n_reads != in->n_reads) {
        c->err = "plo_finish_batch_dev: call plo_liftover_batch_dev on the same batch first";
        return PLO_ERR_INVALID_ARG;
    }
    if (c->last_bt.seq_fmt == PLO_SEQ_BAM4_SPARSE) {
        c->err = "plo_finish_batch_dev: the batch came with sparse bases (PLO_SEQ_BAM4_SPARSE); the flipped sequences are written from complete ones";
        return PLO_ERR_INVALID_ARG;
    }
    c->have_finish = false;
    c->have_sa = false;
    c->have_nm = false;
    c->have_md = false;
    c->have_eqx = false;
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 3; ++i)
        if (!c->fev[i]) HIP_TRY(c, hipEventCreate(&c->fev[i]));
    const DevWork &wk = c->last_wk;
    DevBatch bt = c->last_bt;
    uint32_t n = wk.n_items, nr = bt.n_reads, ne = n + nr;
    size_t a = std::max(1u, n), b = std::max(1u, nr), e = std::max(1u, ne);
    HIP_TRY(c, c->f_flag.ensure(a * 2));
    HIP_TRY(c, c->f_bin.ensure(a * 2));
    HIP_TRY(c, c->f_end.ensure(a * 8));
    HIP_TRY(c, c->f_prim.ensure(a));
    HIP_TRY(c, c->f_isoff.ensure(a * 8));
    HIP_TRY(c, c->f_iqoff.ensure(a * 8));
    HIP_TRY(c, c->f_iread.ensure(a * 4));
    HIP_TRY(c, c->f_nl.ensure(b * 4));
    HIP_TRY(c, c->f_pitem.ensure(b * 4));
    HIP_TRY(c, c->f_uflag.ensure(b * 2));
    HIP_TRY(c, c->f_rsoff.ensure(b * 8));
    HIP_TRY(c, c->f_rqoff.ensure(b * 8));
    HIP_TRY(c, c->f_su.ensure(e * 4));
    HIP_TRY(c, c->f_qu.ensure(e * 4));
    HIP_TRY(c, c->f_soff.ensure((e + 1) * 4));
    HIP_TRY(c, c->f_qoff.ensure((e + 1) * 4));
    HIP_TRY(c, c->f_fflag.ensure(e * 4));
    HIP_TRY(c, c->f_frank.ensure((e + 1) * 4));
    HIP_TRY(c, c->f_flist.ensure(e * 4));
    DevFinish f;
    memset(&f, 0, sizeof(f));
    f.read_flags = fin->read_flags;
    f.qual = fin->qual;
    f.read_qual_off = fin->read_qual_off;
    f.qual_bytes = fin->qual_bytes;
    f.seq_bytes = in->seq_bytes;
    f.item_flag = c->f_flag.as<uint16_t>();
    f.item_bin = c->f_bin.as<uint16_t>();
    f.item_ref_end = c->f_end.as<int64_t>();
    f.item_is_primary = c->f_prim.as<uint8_t>();
    f.item_seq_off = c->f_isoff.as<uint64_t>();
    f.item_qual_off = c->f_iqoff.as<uint64_t>();
    f.item_read = c->f_iread.as<uint32_t>();
    f.read_n_lifted = c->f_nl.as<uint32_t>();
    f.read_primary_item = c->f_pitem.as<uint32_t>();
    f.read_unmapped_flag = c->f_uflag.as<uint16_t>();
    f.read_seq_off = c->f_rsoff.as<uint64_t>();
    f.read_qual_off_out = c->f_rqoff.as<uint64_t>();
    f.su = c->f_su.as<uint32_t>();
    f.qu = c->f_qu.as<uint32_t>();
    f.soff = c->f_soff.as<uint32_t>();
    f.qoff = c->f_qoff.as<uint32_t>();
    f.fflag = c->f_fflag.as<uint32_t>();
    f.frank = c->f_frank.as<uint32_t>();
    f.flist = c->f_flist.as<uint32_t>();
    HIP_TRY(c, c->verr.ensure(16));
    HIP_TRY(c, hipMemsetAsync(c->verr.p, 0, 16, st));
    f.n_fault = c->verr.as<unsigned>() + 2;
    HIP_TRY(c, hipEventRecord(c->fev[0], st));
    if (n) hipLaunchKernelGGL(k_finish_items, dim3((n + 255) / 256), dim3(256), 0, st, bt, wk, f);
    if (nr) hipLaunchKernelGGL(k_finish_reads, dim3((nr + 255) / 256), dim3(256), 0, st, bt, wk, f);
    HIP_TRY(c, hipGetLastError());
    plo_status s = scan_u32(c, f.su, ne, c->f_soff.as<uint32_t>());
    if (s != PLO_OK) return s;
    s = scan_u32(c, f.qu, ne, c->f_qoff.as<uint32_t>());
    if (s != PLO_OK) return s;
    s = scan_u32(c, f.fflag, ne, c->f_frank.as<uint32_t>());
    if (s != PLO_OK) return s;
    if (ne) hipLaunchKernelGGL(k_finish_offsets, dim3((ne + 255) / 256), dim3(256), 0, st, bt, wk, f);
    uint32_t *h = c->h_counters.as<uint32_t>();
    HIP_TRY(c, hipMemcpyAsync(h, c->f_soff.as<uint32_t>() + ne, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h + 1, c->f_qoff.as<uint32_t>() + ne, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h + 2, c->verr.as<unsigned>() + 2, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipEventRecord(c->fev[1], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h[2]) {
        c->err = "plo_finish_batch_dev: " + std::to_string(h[2]) + " item(s) ended LEN_MISMATCH / PANIC; the reference aborts here (src/read_alignment_scanner.rs:207-229)";
        return PLO_ERR_DATA;
    }
    uint64_t sb = (uint64_t)h[0] * 16u, qb = (uint64_t)h[1] * 16u;
    HIP_TRY(c, c->f_rseq.ensure(std::max<uint64_t>(sb, 16)));
    HIP_TRY(c, c->f_rqual.ensure(std::max<uint64_t>(qb, 16)));
    f.rev_seq = c->f_rseq.as<uint8_t>();
    f.rev_qual = c->f_rqual.as<uint8_t>();
    if (sb) {
        uint32_t nblk = std::min<uint32_t>(ne, (uint32_t)c->n_cus * 16u);
        hipLaunchKernelGGL(k_revcomp, dim3(nblk), dim3(256), 0, st, bt, wk, f);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->fev[2], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->finish_ms, c->fev[0], c->fev[1]);
    (void)hipEventElapsedTime(&out->revcomp_ms, c->fev[1], c->fev[2]);
    out->item_flag = f.item_flag;
    out->item_bin = f.item_bin;
    out->item_ref_end = f.item_ref_end;
    out->item_is_primary = f.item_is_primary;
    out->item_seq_off = f.item_seq_off;
    out->item_qual_off = f.item_qual_off;
    out->read_n_lifted = f.read_n_lifted;
    out->read_primary_item = f.read_primary_item;
    out->read_unmapped_flag = f.read_unmapped_flag;
    out->read_seq_off = f.read_seq_off;
    out->read_qual_off = f.read_qual_off_out;
    out->rev_seq = f.rev_seq;
    out->rev_qual = f.rev_qual;
    out->rev_seq_bytes = sb;
    out->rev_qual_bytes = qb;
    out->n_items = n;
    out->n_reads = nr;
    c->have_finish = true;
    return PLO_OK;
}

plo_status plo_sa_segments_dev(plo_ctx *c, const plo_sa_in *in, plo_sa_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    c->err.clear();
    if (!c->have_last || !c->have_finish) {
        c->err = "plo_sa_segments_dev: call plo_liftover_batch_dev and plo_finish_batch_dev on the batch first";
        return PLO_ERR_INVALID_ARG;
    }
    if (in->n_chroms < c->ix->d.n_chroms || !in->chrom_name_off || (!in->chrom_names && in->n_chroms)) {
        c->err = "plo_sa_in: one label per chromosome of the index is required";
        return PLO_ERR_INVALID_ARG;
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 3; i < 5; ++i)
        if (!c->fev[i]) HIP_TRY(c, hipEventCreate(&c->fev[i]));
    const DevWork &wk = c->last_wk;
    uint32_t n = wk.n_items;
    HIP_TRY(c, c->sa_len.ensure(((size_t)n + 1) * 4));
    HIP_TRY(c, c->sa_off.ensure(((size_t)n + 1) * 4));
    DevSa sa;
    sa.chrom_name_off = in->chrom_name_off;
    sa.chrom_names = in->chrom_names;
    sa.item_flag = c->f_flag.as<uint16_t>();
    sa.item_read = c->f_iread.as<uint32_t>();
    sa.read_n_lifted = c->f_nl.as<uint32_t>();
    sa.len = c->sa_len.as<uint32_t>();
    sa.off = c->sa_off.as<uint32_t>();
    sa.text = nullptr;
    HIP_TRY(c, hipEventRecord(c->fev[3], st));
    if (n) hipLaunchKernelGGL(k_sa_len, dim3((n + 255) / 256), dim3(256), 0, st, wk, sa);
    HIP_TRY(c, hipGetLastError());
    plo_status s = scan_u32(c, sa.len, n, c->sa_off.as<uint32_t>());
    if (s != PLO_OK) return s;
    uint32_t *h = c->h_counters.as<uint32_t>();
    HIP_TRY(c, hipMemcpyAsync(h, c->sa_off.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    uint64_t bytes = n ? h[0] : 0;
    HIP_TRY(c, c->sa_text.ensure(std::max<uint64_t>(bytes, 16)));
    sa.text = c->sa_text.as<uint8_t>();
    if (bytes) hipLaunchKernelGGL(k_sa_emit, dim3((n + 255) / 256), dim3(256), 0, st, wk, sa);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->fev[4], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->sa_ms, c->fev[3], c->fev[4]);
    out->n_items = n;
    out->item_sa_off = c->sa_off.as<uint32_t>();
    out->sa_text = sa.text;
    out->sa_bytes = bytes;
    c->have_sa = true;
    return PLO_OK;
}

plo_status plo_records_build_dev(plo_ctx *c, const plo_batch_in *in, const plo_records_in *rin, plo_records_out *out) {
    if (!c || !in || !rin || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    c->err.clear();
    if (c->have_last && c->last_bt.seq_fmt != PLO_SEQ_BAM4) {
        c->err = "plo_records_build_dev: the batch came with sparse or ASCII bases; the records are written from complete BAM 4-bit bases (PLO_SEQ_BAM4)";
        return PLO_ERR_INVALID_ARG;
    }
    if (!c->have_last || c->last_bt.n_segs != in->n_segs || c->last_bt.n_reads != in->n_reads) {
        c->err = "plo_records_build_dev: no lift result of this batch on the context: call plo_liftover_batch_dev on it first";
        return PLO_ERR_INVALID_ARG;
    }
    if (!c->have_finish) {
        c->err = "plo_records_build_dev: no finishing result on the context: call plo_finish_batch_dev on the batch first";
        return PLO_ERR_INVALID_ARG;
    }
    if (!c->have_sa) {
        c->err = "plo_records_build_dev: no SA text on the context: call plo_sa_segments_dev behind the finishing first";
        return PLO_ERR_INVALID_ARG;
    }
    if (rin->n_contigs < c->ix->d.n_contigs || !rin->contig_name_off || (!rin->contig_names && rin->n_contigs) ||
        (in->n_reads && (!rin->records || !rin->read_rec_off))) {
        c->err = "plo_records_in: the records, their offsets and one label per contig of the index are required";
        return PLO_ERR_INVALID_ARG;
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 4; ++i)
        if (!c->rev[i]) HIP_TRY(c, hipEventCreate(&c->rev[i]));
    const DevWork &wk = c->last_wk;
    const DevBatch &bt = c->last_bt;
    const uint32_t nr = bt.n_reads, nb = std::max(1u, (nr + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK);
    const size_t b = std::max(1u, nr);
    HIP_TRY(c, c->r_plan.ensure(b * REC_PLAN_WORDS * 4));
    HIP_TRY(c, c->r_size.ensure(3 * b * 8));
    HIP_TRY(c, c->r_start.ensure(3 * (b + 1) * 8));
    HIP_TRY(c, c->r_partial.ensure(3 * (size_t)nb * 8));
    HIP_TRY(c, c->r_err.ensure(REC_ERR_N * 4));
    HIP_TRY(c, c->h_rec.ensure(64));
    DevRecords d;
    memset(&d, 0, sizeof(d));
    d.records = rin->records;
    d.records_bytes = rin->records_bytes;
    d.read_rec_off = rin->read_rec_off;
    d.contig_name_off = rin->contig_name_off;
    d.contig_names = rin->contig_names;
    d.is_target_region = rin->is_target_region;
    d.item_flag = c->f_flag.as<uint16_t>();
    d.item_bin = c->f_bin.as<uint16_t>();
    d.item_ref_end = c->f_end.as<int64_t>();
    d.item_seq_off = c->f_isoff.as<uint64_t>();
    d.item_qual_off = c->f_iqoff.as<uint64_t>();
    d.item_read = c->f_iread.as<uint32_t>();
    d.read_n_lifted = c->f_nl.as<uint32_t>();
    d.read_unmapped_flag = c->f_uflag.as<uint16_t>();
    d.read_seq_off = c->f_rsoff.as<uint64_t>();
    d.read_qual_off = c->f_rqoff.as<uint64_t>();
    d.rev_seq = c->f_rseq.as<uint8_t>();
    d.rev_qual = c->f_rqual.as<uint8_t>();
    d.sa_off = c->sa_off.as<uint32_t>();
    d.sa_text = c->sa_text.as<uint8_t>();
    d.item_nm = c->have_nm ? c->nm_out.as<uint32_t>() : nullptr;
    d.item_md_off = c->have_md ? c->md.off.as<uint64_t>() : nullptr;
    d.md_text = c->have_md ? c->md.out.as<uint8_t>() : nullptr;
    d.item_eqx_off = c->have_eqx ? c->eqx.off.as<uint64_t>() : nullptr;
    d.eqx_ops = c->have_eqx ? c->eqx.out.as<uint32_t>() : nullptr;
    d.cs_is_fwd = c->ix->d.cs_is_fwd;
    d.contig_seg_off = c->ix->d.contig_seg_off;
    d.plan = c->r_plan.as<uint32_t>();
    d.size = c->r_size.as<unsigned long long>();
    d.start = c->r_start.as<unsigned long long>();
    d.err = c->r_err.as<unsigned>();
    unsigned long long *start = c->r_start.as<unsigned long long>();
    unsigned long long *h = c->h_rec.as<unsigned long long>();
    memset(h, 0, 64);
    HIP_TRY(c, hipMemsetAsync(c->r_err.p, 0, REC_ERR_N * 4, st));
    HIP_TRY(c, hipEventRecord(c->rev[0], st));
    if (nr) {
        hipLaunchKernelGGL(k_rec_plan, dim3((nr + 3) / 4), dim3(256), 0, st, bt, wk, d);
        hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 3), dim3(64), 0, st, (const unsigned long long *)d.size, nr, nb, c->r_partial.as<unsigned long long>());
        hipLaunchKernelGGL(k_rec_scan_partials, dim3(3), dim3(64), 0, st, c->r_partial.as<unsigned long long>(), nr, nb, start);
        hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 3), dim3(64), 0, st, (const unsigned long long *)d.size, nr, nb, (const unsigned long long *)c->r_partial.as<unsigned long long>(), start);
        HIP_TRY(c, hipGetLastError());
        // the one round trip: total bytes, records, unmapped copies, and the bounds checks
        HIP_TRY(c, hipMemcpyAsync(h, start + nr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h + 1, start + (size_t)nr + 1 + nr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h + 2, start + 2 * ((size_t)nr + 1) + nr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h + 4, c->r_err.p, REC_ERR_N * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipEventRecord(c->rev[1], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const unsigned *herr = (const unsigned *)(h + 4);
    if (herr[REC_ERR_OFFSET] || herr[REC_ERR_BLOCK] || herr[REC_ERR_LAYOUT] || herr[REC_ERR_SEQLEN]) {
        c->err = "plo_records_build_dev: " + std::to_string(herr[REC_ERR_OFFSET]) + " read_rec_off beyond records_bytes, " + std::to_string(herr[REC_ERR_BLOCK]) +
                 " block_size running past the end of `records`, " + std::to_string(herr[REC_ERR_LAYOUT]) + " l_qname / n_cigar / l_seq pointing outside their record, " +
                 std::to_string(herr[REC_ERR_SEQLEN]) + " l_seq different from the batch's read_seq_len; nothing was written";
        return PLO_ERR_INVALID_ARG;
    }
    const unsigned long long n_bytes = h[0], n_rec = h[1];
    if (n_rec > 0xfffffffeull) {
        c->err = "plo_records_build_dev: more than 2^32 - 2 output records in one window";
        return PLO_ERR_RANGE;
    }
    HIP_TRY(c, c->r_out.ensure(std::max<unsigned long long>(n_bytes, 16)));
    HIP_TRY(c, c->r_recoff.ensure((n_rec + 1) * 8));
    d.out = c->r_out.as<uint8_t>();
    d.record_off = c->r_recoff.as<uint64_t>();
    HIP_TRY(c, hipEventRecord(c->rev[2], st));
    if (n_rec) {
        const uint32_t nblk = std::min<uint32_t>(nr, (uint32_t)c->n_cus * 8u);
        if (c->rec_bytecopy) hipLaunchKernelGGL((k_rec_emit<false, true>), dim3(nblk), dim3(256), 0, st, bt, wk, d);
        else if (d.item_eqx_off) hipLaunchKernelGGL((k_rec_emit<true, true>), dim3(nblk), dim3(256), 0, st, bt, wk, d);
        else hipLaunchKernelGGL((k_rec_emit<true, false>), dim3(nblk), dim3(256), 0, st, bt, wk, d);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(d.record_off + n_rec, &h[0], 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->rev[3], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float a_ms = 0, b_ms = 0;
    (void)hipEventElapsedTime(&a_ms, c->rev[0], c->rev[1]);
    (void)hipEventElapsedTime(&b_ms, c->rev[2], c->rev[3]);
    out->records_ms = a_ms + b_ms;
    out->bytes = d.out;
    out->n_bytes = n_bytes;
    out->n_records = (uint32_t)n_rec;
    out->record_off = d.record_off;
    out->n_unmapped_copies = (uint32_t)h[2];
    out->n_lifted = (uint32_t)(n_rec - h[2]);
    return PLO_OK;
}

// NM:i of every lifted item (nm_core.hpp): one launch of persistent waves and one wait, for the refusal, the count and the event time.
plo_status plo_nm_dev(plo_ctx *c, const plo_batch_in *in, plo_nm_out *out) {
    const plo_status entry = aln_enter(c, in, out, &plo_ctx::have_nm, "plo_nm_dev", "NM is counted over");
    if (entry != PLO_OK) return entry;
    const uint32_t n = c->last_wk.n_items;
    hipStream_t st = c->stream;
    for (int i = 0; i < 2; ++i)
        if (!c->nev[i]) HIP_TRY(c, hipEventCreate(&c->nev[i]));
    HIP_TRY(c, c->nm_out.ensure((size_t)std::max(1u, n) * 4));
    HIP_TRY(c, c->nm_blk.ensure(16));  // n_cmp, err_item, ticket
    HIP_TRY(c, c->h_nm.ensure(16));
    DevNm d;
    memset(&d, 0, sizeof(d));
    aln_src(c, d);
    d.item_nm = c->nm_out.as<uint32_t>();
    d.n_cmp = c->nm_blk.as<unsigned long long>();
    d.err_item = c->nm_blk.as<int>() + 2;
    d.ticket = c->nm_blk.as<unsigned>() + 3;
    uint32_t *h = c->h_nm.as<uint32_t>();
    h[0] = h[1] = h[3] = 0;
    h[2] = (uint32_t)NM_NO_ITEM;
    HIP_TRY(c, hipMemcpyAsync(c->nm_blk.p, h, 16, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->nev[0], st));
    if (n) {
        hipLaunchKernelGGL(k_nm, dim3(aln_grid(c, n)), dim3(256), 0, st, c->last_bt, c->last_wk, d);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->nev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, c->nm_blk.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->nm_ms, c->nev[0], c->nev[1]);
    if (h[2] != (uint32_t)NM_NO_ITEM) return aln_refused(c, "plo_nm_dev", "NM", h[2], &out->err_item);
    out->n_items = n;
    out->item_nm = d.item_nm;
    out->n_cmp_bases = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
    c->have_nm = true;
    return PLO_OK;
}

// MD:Z of every lifted item (md_core.hpp): aln_pass_run with k_md_count and k_md_emit
plo_status plo_md_dev(plo_ctx *c, const plo_batch_in *in, plo_md_out *out) {
    const plo_status entry = aln_enter(c, in, out, &plo_ctx::have_md, "plo_md_dev", "MD is written from");
    if (entry != PLO_OK) return entry;
    hipStream_t st = c->stream;
    DevMd d;
    memset(&d, 0, sizeof(d));
    aln_src(c, d);
    const plo_status run = aln_pass_run(
        c, c->md, d, "plo_md_dev", "MD", &out->err_item, &out->md_ms, &out->md_bytes,
        [&](uint32_t nblk) { hipLaunchKernelGGL(k_md_count, dim3(nblk), dim3(256), 0, st, c->last_bt, c->last_wk, d); },
        [&](uint64_t total) {
            const hipError_t e = c->md.out.ensure((size_t)total + 16);
            d.item_md_off = c->md.off.as<unsigned long long>();
            d.md_text = c->md.out.as<uint8_t>();
            return e;
        },
        [&](uint32_t nblk) { hipLaunchKernelGGL(k_md_emit, dim3(nblk), dim3(256), 0, st, c->last_bt, c->last_wk, d); });
    if (run != PLO_OK) return run;
    out->n_items = c->last_wk.n_items;
    out->item_md_off = c->md.off.as<uint64_t>();
    out->md_text = d.md_text;
    c->have_md = true;
    return PLO_OK;
}

// The = / X CIGAR of every lifted item (eqx_core.hpp): aln_pass_run with k_eqx_count and k_eqx_emit
plo_status plo_eqx_dev(plo_ctx *c, const plo_batch_in *in, plo_eqx_out *out) {
    const plo_status entry = aln_enter(c, in, out, &plo_ctx::have_eqx, "plo_eqx_dev", "the ops are written from");
    if (entry != PLO_OK) return entry;
    hipStream_t st = c->stream;
    DevEqx d;
    memset(&d, 0, sizeof(d));
    aln_src(c, d);
    const plo_status run = aln_pass_run(
        c, c->eqx, d, "plo_eqx_dev", "CIGAR", &out->err_item, &out->eqx_ms, &out->n_ops,
        [&](uint32_t nblk) { hipLaunchKernelGGL(k_eqx_count, dim3(nblk), dim3(256), 0, st, c->last_bt, c->last_wk, d); },
        [&](uint64_t total) {
            const hipError_t e = c->eqx.out.ensure(((size_t)total + 4) * 4);
            d.item_eqx_off = c->eqx.off.as<unsigned long long>();
            d.eqx_ops = c->eqx.out.as<uint32_t>();
            return e;
        },
        [&](uint32_t nblk) { hipLaunchKernelGGL(k_eqx_emit, dim3(nblk), dim3(256), 0, st, c->last_bt, c->last_wk, d); });
    if (run != PLO_OK) return run;
    out->n_items = c->last_wk.n_items;
    out->item_eqx_off = c->eqx.off.as<uint64_t>();
    out->eqx_ops = d.eqx_ops;
    c->have_eqx = true;
    return PLO_OK;
}

// The records at in->bytes in coordinate order (sort_core.hpp): k_sort_keys (check, keys, tiles sorted in LDS), a k_sort_merge per doubling
// of the runs, k_sort_gather, the 64-bit scan of the lengths, k_sort_copy.  6 + ceil(log2(ceil(n / 1024))) launches, one wait behind the
// copy: the copy looks at the check's word itself, so a refused window moves no byte.
plo_status plo_records_sort_dev(plo_ctx *c, const plo_sort_in *in, plo_sort_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->err_record = UINT32_MAX;
    c->err.clear();
    const uint32_t n = in->n_records;
    if (n && (!in->bytes || !in->record_off)) {
        c->err = "plo_sort_in: the records and their offsets are required";
        return PLO_ERR_INVALID_ARG;
    }
    if (n > 0x7ffffffeu || in->n_ref > 0x7fffffffu) {
        c->err = "plo_records_sort_dev: more than 2^31 - 2 records or 2^31 - 1 references";
        return PLO_ERR_RANGE;
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 2; ++i)
        if (!c->sev[i]) HIP_TRY(c, hipEventCreate(&c->sev[i]));
    HIP_TRY(c, c->so_off.ensure(((size_t)n + 1) * 8));
    HIP_TRY(c, c->so_out.ensure((size_t)(n ? in->n_bytes : 0) + 16));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c, c->so_key[i].ensure((size_t)std::max(1u, n) * 8));
        HIP_TRY(c, c->so_idx[i].ensure((size_t)std::max(1u, n) * 4));
    }
    out->bytes = c->so_out.as<uint8_t>();
    out->record_off = c->so_off.as<uint64_t>();
    out->perm = c->so_idx[0].as<uint32_t>();
    out->key = c->so_key[0].as<uint64_t>();
    if (!n) {
        HIP_TRY(c, hipMemsetAsync(c->so_off.p, 0, 8, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        return PLO_OK;
    }
    const uint32_t nb = (n + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK, n_tiles = (n + SORT_TILE - 1) / SORT_TILE, nt = (n + 255u) / 256u;
    HIP_TRY(c, c->so_len.ensure((size_t)n * 8));
    HIP_TRY(c, c->so_slen.ensure((size_t)n * 8));
    HIP_TRY(c, c->so_partial.ensure((size_t)nb * 8));
    HIP_TRY(c, c->so_blk.ensure(16));
    HIP_TRY(c, c->h_so.ensure(32));
    DevSort d;
    memset(&d, 0, sizeof(d));
    d.bytes = in->bytes;
    d.n_bytes = in->n_bytes;
    d.n = n;
    d.record_off = in->record_off;
    d.n_ref = in->n_ref;
    for (int i = 0; i < 2; ++i) {
        d.key[i] = c->so_key[i].as<unsigned long long>();
        d.idx[i] = c->so_idx[i].as<uint32_t>();
    }
    d.len = c->so_len.as<unsigned long long>();
    d.slen = c->so_slen.as<unsigned long long>();
    unsigned long long *off = c->so_off.as<unsigned long long>();
    d.new_off = off;
    d.out = c->so_out.as<uint8_t>();
    d.err = c->so_blk.as<int>();
    d.n_mapped = c->so_blk.as<unsigned>() + 1;
    uint32_t *h = c->h_so.as<uint32_t>();
    h[0] = (uint32_t)SORT_NO_RECORD;
    h[1] = 0;
    h[4] = h[5] = 0;
    HIP_TRY(c, hipMemcpyAsync(c->so_blk.p, h, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->sev[0], st));
    hipLaunchKernelGGL(k_sort_keys, dim3(n_tiles), dim3(SORT_THREADS), 0, st, d);
    int cur = 0;
    for (uint64_t run = SORT_TILE; run < n; run <<= 1, cur ^= 1)
        hipLaunchKernelGGL(k_sort_merge, dim3(nt), dim3(256), 0, st, (const unsigned long long *)d.key[cur], (const uint32_t *)d.idx[cur], d.key[cur ^ 1], d.idx[cur ^ 1], n, (uint32_t)run);
    const uint32_t *perm = d.idx[cur];
    hipLaunchKernelGGL(k_sort_gather, dim3(nt), dim3(256), 0, st, perm, (const unsigned long long *)d.len, d.slen, n);
    hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.slen, n, nb, c->so_partial.as<unsigned long long>());
    hipLaunchKernelGGL(k_rec_scan_partials, dim3(1), dim3(64), 0, st, c->so_partial.as<unsigned long long>(), n, nb, off);
    hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.slen, n, nb, (const unsigned long long *)c->so_partial.as<unsigned long long>(), off);
    const unsigned long long n_chunks = (in->n_bytes + SORT_COPY_CHUNK - 1) / SORT_COPY_CHUNK;
    if (n_chunks) hipLaunchKernelGGL(k_sort_copy, dim3((unsigned)((n_chunks + 3) / 4)), dim3(256), 0, st, d, perm, n_chunks);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->sev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, c->so_blk.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h[0] != (uint32_t)SORT_NO_RECORD) {
        const uint32_t e = h[0];
        HIP_TRY(c, hipMemcpy(h + 4, d.len + e, 8, hipMemcpyDeviceToHost));
        static const char *const what[] = {"", "record_off: it must start at 0, not decrease and end at n_bytes", "its length: fewer than the 36 bytes of block_size and the fixed fields",
                                           "block_size: block_size + 4 differs from the record's length", "refID: outside [-1, n_ref)", "pos: outside [-1, 2^31 - 2]"};
        out->err_record = e;
        out->bytes = nullptr;
        out->record_off = nullptr;
        out->perm = nullptr;
        out->key = nullptr;
        c->err = "plo_records_sort_dev: record " + std::to_string(e) + " is refused for " + (h[4] >= 1 && h[4] <= 5 ? what[h[4]] : "an unknown reason") + "; nothing was sorted";
        return PLO_ERR_INVALID_ARG;
    }
    (void)hipEventElapsedTime(&out->sort_ms, c->sev[0], c->sev[1]);
    out->n_bytes = in->n_bytes;
    out->n_records = n;
    out->perm = perm;
    out->key = (const uint64_t *)d.key[cur];
    out->n_mapped = h[1];
    return PLO_OK;
}

// The merged order of in->runs (merge_core.hpp): k_merge_keys, a k_merge_rank per doubling of the groups of runs, k_merge_gather, the 64-bit
// scan of the lengths, k_merge_chunks.  6 + ceil(log2(n_runs)) launches, one wait: the chunk table comes down with the result words.
plo_status plo_runs_merge_plan_dev(plo_ctx *c, const plo_merge_in *in, plo_merge_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->err_run = out->err_record = UINT32_MAX;
    c->err.clear();
    c->have_plan = false;
    static_assert(sizeof(plo_merge_run) == sizeof(MergeRun) && offsetof(plo_merge_run, record_off) == offsetof(MergeRun, record_off), "plo_merge_run and MergeRun are one layout");
    static_assert(PLO_MERGE_MAX_RUNS == MERGE_MAX_RUNS && MERGE_MAX_RUNS <= 65536, "run_of holds a run in 16 bits");
    if (in->n_runs > PLO_MERGE_MAX_RUNS || in->chunk_bytes == 0 || (in->n_runs && !in->runs) || in->n_ref > 0x7fffffffu) {
        c->err = "plo_merge_in: at most " + std::to_string(PLO_MERGE_MAX_RUNS) + " runs, a chunk_bytes above 0, the run table and at most 2^31 - 1 references are required";
        return PLO_ERR_INVALID_ARG;
    }
    const uint32_t n_runs = in->n_runs;
    uint64_t n64 = 0, n_bytes = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const plo_merge_run &run = in->runs[r];
        if (run.n_records ? (!run.bytes || !run.record_off) : run.n_bytes != 0) {
            c->err = "plo_merge_in: run " + std::to_string(r) + (run.n_records ? ": the records and their offsets are required" : ": bytes without a record");
            return PLO_ERR_INVALID_ARG;
        }
        n64 += run.n_records;
        n_bytes += run.n_bytes;
    }
    if (n64 > 0xfffffffeull) {
        c->err = "plo_runs_merge_plan_dev: more than 2^32 - 2 records in all";
        return PLO_ERR_RANGE;
    }
    const uint32_t n = (uint32_t)n64;
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 4; ++i)
        if (!c->gev[i]) HIP_TRY(c, hipEventCreate(&c->gev[i]));
    HIP_TRY(c, c->mg_off.ensure(((size_t)n + 1) * 8));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c, c->mg_key[i].ensure((size_t)std::max(1u, n) * 8));
        HIP_TRY(c, c->mg_src[i].ensure((size_t)std::max(1u, n) * 4));
    }
    c->mg_chunk_first.assign(1, 0);
    c->mg_chunk_off.assign(1, 0);
    c->mg_n = n;
    c->mg_n_chunks = 0;
    c->mg_cur = 0;
    out->src = c->mg_src[0].as<uint32_t>();
    out->key = c->mg_key[0].as<uint64_t>();
    out->record_off = c->mg_off.as<uint64_t>();
    out->chunk_first = c->mg_chunk_first.data();
    out->chunk_off = c->mg_chunk_off.data();
    if (!n) {
        HIP_TRY(c, hipMemsetAsync(c->mg_off.p, 0, 8, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        c->have_plan = true;
        return PLO_OK;
    }
    // two chunks in a row hold more than chunk_bytes (the second one's first record did not fit the first), and none is empty
    const uint64_t cap64 = std::min<uint64_t>(n, 2 * (n_bytes / in->chunk_bytes) + 2);
    const uint32_t cap = (uint32_t)cap64;
    const uint32_t nb = (n + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK, nt = (uint32_t)(((uint64_t)n + 255u) / 256u);
    const size_t tab_bytes = ((size_t)n_runs + 1) * 4, tab_at = (size_t)n_runs * sizeof(MergeRun);
    HIP_TRY(c, c->mg_len.ensure((size_t)n * 8));
    HIP_TRY(c, c->mg_mlen.ensure((size_t)n * 8));
    HIP_TRY(c, c->mg_runof.ensure((size_t)n * 2));
    HIP_TRY(c, c->mg_partial.ensure((size_t)nb * 8));
    HIP_TRY(c, c->mg_runs.ensure(tab_at));
    HIP_TRY(c, c->mg_first.ensure(tab_bytes));
    HIP_TRY(c, c->mg_blk.ensure(16));
    HIP_TRY(c, c->mg_cfirst.ensure(((size_t)cap + 1) * 4));
    HIP_TRY(c, c->mg_coff.ensure(((size_t)cap + 1) * 8));
    HIP_TRY(c, c->h_mg.ensure(tab_at + tab_bytes + 64));
    HIP_TRY(c, c->h_mg_tab.ensure(((size_t)cap + 1) * 12 + 16));
    uint8_t *hp = c->h_mg.as<uint8_t>();
    memcpy(hp, in->runs, tab_at);
    uint32_t *h_first = (uint32_t *)(hp + tab_at);
    h_first[0] = 0;
    for (uint32_t r = 0; r < n_runs; ++r) h_first[r + 1] = h_first[r] + in->runs[r].n_records;
    uint32_t *h = (uint32_t *)(hp + ((tab_at + tab_bytes + 15) & ~(size_t)15));
    h[0] = (uint32_t)merge_err_word(MERGE_NO_RECORD);
    h[1] = h[2] = h[3] = 0;
    h[4] = h[5] = 0;
    DevMerge d;
    memset(&d, 0, sizeof(d));
    d.runs = c->mg_runs.as<MergeRun>();
    d.run_first = c->mg_first.as<uint32_t>();
    d.n_runs = n_runs;
    d.n = n;
    d.n_ref = in->n_ref;
    d.chunk_bytes = in->chunk_bytes;
    for (int i = 0; i < 2; ++i) {
        d.key[i] = c->mg_key[i].as<unsigned long long>();
        d.src[i] = c->mg_src[i].as<uint32_t>();
    }
    d.run_of = c->mg_runof.as<uint16_t>();
    d.len = c->mg_len.as<unsigned long long>();
    d.mlen = c->mg_mlen.as<unsigned long long>();
    unsigned long long *off = c->mg_off.as<unsigned long long>();
    d.off = off;
    d.err = c->mg_blk.as<int>();
    d.res = c->mg_blk.as<uint32_t>() + 1;
    d.chunk_first = c->mg_cfirst.as<uint32_t>();
    d.chunk_off = c->mg_coff.as<unsigned long long>();
    d.chunk_cap = cap;
    HIP_TRY(c, hipMemcpyAsync(c->mg_runs.p, hp, tab_at, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->mg_first.p, h_first, tab_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->mg_blk.p, h, 12, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->gev[0], st));
    hipLaunchKernelGGL(k_merge_keys, dim3(nt), dim3(256), 0, st, d);
    int cur = 0;
    for (uint32_t t = 0; (1u << t) < n_runs; ++t, cur ^= 1)
        hipLaunchKernelGGL(k_merge_rank, dim3(nt), dim3(256), 0, st, d, (const unsigned long long *)d.key[cur], (const uint32_t *)d.src[cur], d.key[cur ^ 1], d.src[cur ^ 1], t);
    hipLaunchKernelGGL(k_merge_gather, dim3(nt), dim3(256), 0, st, d, (const uint32_t *)d.src[cur]);
    hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.mlen, n, nb, c->mg_partial.as<unsigned long long>());
    hipLaunchKernelGGL(k_rec_scan_partials, dim3(1), dim3(64), 0, st, c->mg_partial.as<unsigned long long>(), n, nb, off);
    hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.mlen, n, nb, (const unsigned long long *)c->mg_partial.as<unsigned long long>(), off);
    hipLaunchKernelGGL(k_merge_chunks, dim3(1), dim3(64), 0, st, d, (const unsigned long long *)d.key[cur]);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->gev[1], st));
    uint8_t *ht = c->h_mg_tab.as<uint8_t>();
    HIP_TRY(c, hipMemcpyAsync(h, c->mg_blk.p, 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(ht, c->mg_coff.p, ((size_t)cap + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(ht + ((size_t)cap + 1) * 8, c->mg_cfirst.p, ((size_t)cap + 1) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h[0] != (uint32_t)merge_err_word(MERGE_NO_RECORD)) {
        const uint32_t g = h[0] ^ 0x80000000u;
        HIP_TRY(c, hipMemcpy(h + 4, d.len + g, 8, hipMemcpyDeviceToHost));
        uint32_t r = 0;
        while (r + 1 < n_runs && h_first[r + 1] <= g) ++r;
        static const char *const what[] = {"", "record_off: it must start at 0, not decrease and end at the run's n_bytes", "its length: fewer than the 36 bytes of block_size and the fixed fields",
                                           "block_size: block_size + 4 differs from the record's length", "refID: outside [-1, n_ref)", "pos: outside [-1, 2^31 - 2]",
                                           "its place: its key is lower than the key of the record before it, the run is not coordinate sorted"};
        out->err_run = r;
        out->err_record = g - h_first[r];
        out->err_kind = h[4];
        out->src = nullptr;
        out->key = nullptr;
        out->record_off = nullptr;
        out->chunk_first = nullptr;
        out->chunk_off = nullptr;
        c->err = "plo_runs_merge_plan_dev: run " + std::to_string(r) + " record " + std::to_string(out->err_record) + " is refused for kind " + std::to_string(h[4]) + ", " +
                 (h[4] >= 1 && h[4] <= 6 ? what[h[4]] : "an unknown reason") + "; nothing was merged";
        return PLO_ERR_INVALID_ARG;
    }
    const uint32_t n_chunks = h[2];
    if (n_chunks == 0 || n_chunks > cap) {
        c->err = "plo_runs_merge_plan_dev: the chunk table outgrew its bound";
        return PLO_ERR_INTERNAL;
    }
    const uint64_t *t_off = (const uint64_t *)ht;
    const uint32_t *t_first = (const uint32_t *)(ht + ((size_t)cap + 1) * 8);
    c->mg_chunk_first.assign(t_first, t_first + n_chunks + 1);
    c->mg_chunk_off.assign(t_off, t_off + n_chunks + 1);
    (void)hipEventElapsedTime(&out->plan_ms, c->gev[0], c->gev[1]);
    c->mg_cur = cur;
    c->mg_n_chunks = n_chunks;
    c->have_plan = true;
    out->n_records = n;
    out->n_mapped = h[1];
    out->n_bytes = c->mg_chunk_off[n_chunks];
    out->src = d.src[cur];
    out->key = (const uint64_t *)d.key[cur];
    out->n_chunks = n_chunks;
    out->chunk_first = c->mg_chunk_first.data();
    out->chunk_off = c->mg_chunk_off.data();
    return PLO_OK;
}

// Chunk `chunk` of the context's current plan (merge_core.hpp): ONE launch of k_merge_copy, a wave per 16 KB of the chunk, one wait.
plo_status plo_runs_merge_emit_dev(plo_ctx *c, uint32_t chunk, plo_merge_chunk_out *out) {
    if (!c || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    c->err.clear();
    if (!c->have_plan) {
        c->err = "plo_runs_merge_emit_dev: the context holds no plan (plo_runs_merge_plan_dev first; a refused plan is none)";
        return PLO_ERR_INVALID_ARG;
    }
    if (chunk >= c->mg_n_chunks) {
        c->err = "plo_runs_merge_emit_dev: chunk " + std::to_string(chunk) + " of a plan of " + std::to_string(c->mg_n_chunks);
        return PLO_ERR_INVALID_ARG;
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    const uint32_t first = c->mg_chunk_first[chunk], nrec = c->mg_chunk_first[chunk + 1] - first;
    const uint64_t nbytes = c->mg_chunk_off[chunk + 1] - c->mg_chunk_off[chunk];
    HIP_TRY(c, c->mg_out.ensure((size_t)nbytes + 16));
    HIP_TRY(c, c->mg_ooff.ensure(((size_t)nrec + 1) * 8));
    DevMergeEmit d;
    memset(&d, 0, sizeof(d));
    d.runs = c->mg_runs.as<MergeRun>();
    d.run_first = c->mg_first.as<uint32_t>();
    d.run_of = c->mg_runof.as<uint16_t>();
    d.src = c->mg_src[c->mg_cur].as<uint32_t>();
    d.off = c->mg_off.as<unsigned long long>();
    d.first = first;
    d.n = nrec;
    d.out = c->mg_out.as<uint8_t>();
    d.out_off = c->mg_ooff.as<unsigned long long>();
    const unsigned long long n_pieces = (nbytes + MERGE_COPY_PIECE - 1) / MERGE_COPY_PIECE;
    HIP_TRY(c, hipEventRecord(c->gev[2], st));
    hipLaunchKernelGGL(k_merge_copy, dim3((unsigned)((n_pieces + 3) / 4)), dim3(256), 0, st, d, n_pieces);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->gev[3], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->emit_ms, c->gev[2], c->gev[3]);
    out->bytes = d.out;
    out->n_bytes = nbytes;
    out->n_records = nrec;
    out->first_record = first;
    out->record_off = (const uint64_t *)d.out_off;
    return PLO_OK;
}

// The index entries of the records at in->bytes (index_core.hpp): ONE launch of k_index, a wave per record, at most 2048 workgroups of four
// waves; the two result words come back behind it, one wait.
plo_status plo_records_index_dev(plo_ctx *c, const plo_index_in *in, plo_index_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->err_record = UINT32_MAX;
    c->err.clear();
    const uint32_t n = in->n_records;
    if (n && (!in->bytes || !in->record_off)) {
        c->err = "plo_index_in: the records and their offsets are required";
        return PLO_ERR_INVALID_ARG;
    }
    if (n > INDEX_MAX_RECORDS || in->n_ref > 0x7fffffffu) {
        c->err = "plo_records_index_dev: more than 2^27 - 1 records or 2^31 - 1 references";
        return PLO_ERR_RANGE;
    }
    static_assert(sizeof(plo_index_entry) == sizeof(IndexEntry) && offsetof(plo_index_entry, flags) == offsetof(IndexEntry, flags), "plo_index_entry and IndexEntry are one layout");
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 2; ++i)
        if (!c->xev[i]) HIP_TRY(c, hipEventCreate(&c->xev[i]));
    HIP_TRY(c, c->bai_entry.ensure((size_t)std::max(1u, n) * sizeof(IndexEntry)));
    out->entry = c->bai_entry.as<plo_index_entry>();
    if (!n) return PLO_OK;
    HIP_TRY(c, c->bai_blk.ensure(16));
    HIP_TRY(c, c->h_bai.ensure(16));
    DevBai d;
    memset(&d, 0, sizeof(d));
    d.s.bytes = in->bytes;
    d.s.n_bytes = in->n_bytes;
    d.s.n = n;
    d.s.record_off = in->record_off;
    d.s.n_ref = in->n_ref;
    d.entry = c->bai_entry.as<IndexEntry>();
    d.err = c->bai_blk.as<int>();
    d.n_placed = c->bai_blk.as<unsigned>() + 1;
    uint32_t *h = c->h_bai.as<uint32_t>();
    h[0] = (uint32_t)INDEX_NO_RECORD;
    h[1] = 0;
    HIP_TRY(c, hipMemcpyAsync(c->bai_blk.p, h, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->xev[0], st));
    hipLaunchKernelGGL(k_index, dim3(std::min(2048u, (n + 3u) / 4u)), dim3(256), 0, st, d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->xev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, c->bai_blk.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h[0] != (uint32_t)INDEX_NO_RECORD) {
        static const char *const what[] = {"", "record_off: it must start at 0, not decrease and end at n_bytes", "its length: fewer than the 36 bytes of block_size and the fixed fields",
                                           "block_size: block_size + 4 differs from the record's length", "refID: outside [-1, n_ref)", "pos: outside [-1, 2^31 - 2]",
                                           "its CIGAR: 36 + l_read_name + 4 n_cigar_op passes the record's end", "its end: behind 2^29, which a BAM index cannot address",
                                           "its place: (reference, pos) is lower than the previous record's, the buffer is not coordinate sorted"};
        out->err_record = h[0] >> 4;
        out->err_kind = h[0] & 15u;
        out->entry = nullptr;
        c->err = "plo_records_index_dev: record " + std::to_string(out->err_record) + " is refused for " + (out->err_kind >= 1 && out->err_kind <= 8 ? what[out->err_kind] : "an unknown reason") +
                 "; no entry is handed out";
        return PLO_ERR_INVALID_ARG;
    }
    (void)hipEventElapsedTime(&out->index_ms, c->xev[0], c->xev[1]);
    out->n_records = n;
    out->n_placed = h[1];
    return PLO_OK;
}

// ---- plo_depth_* (depth_core.hpp) -------------------------------------------------------------------------------------------------------------
// the array, exactly its size (a DevBuf would round 12 GB up by a quarter), zeroed; the tables; the sums of the scan
plo_status plo_depth_create(plo_ctx *c, uint32_t n_ref, const int32_t *ref_len, const plo_depth_opts *opts, plo_depth **out) {
    if (!c || !out || (n_ref && !ref_len)) return PLO_ERR_INVALID_ARG;
    *out = nullptr;
    c->err.clear();
    if (n_ref > 0x7fffffffu) {
        c->err = "plo_depth_create: more than 2^31 - 1 references";
        return PLO_ERR_RANGE;
    }
    for (uint32_t r = 0; r < n_ref; ++r)
        if (ref_len[r] < 0) {
            c->err = "plo_depth_create: ref_len[" + std::to_string(r) + "] is negative";
            return PLO_ERR_INVALID_ARG;
        }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    plo_depth *d = new plo_depth();
    d->device = c->ix->device;
    d->n_ref = n_ref;
    if (opts) {
        d->exclude_flags = opts->exclude_flags;
        d->count_del = opts->count_deletions != 0;
    }
    d->ref_len.assign(ref_len, ref_len + n_ref);
    d->slot_off.resize((size_t)n_ref + 1);
    d->n_entries = depth_layout(n_ref, d->ref_len.data(), d->slot_off.data());
    d->n1 = (d->n_entries + DEPTH_TILE - 1) / DEPTH_TILE;
    d->n2 = (d->n1 + DEPTH_TILE - 1) / DEPTH_TILE;
    const size_t arr_bytes = std::max<size_t>((size_t)d->n_entries * 4, 16);
    hipError_t e = hipMalloc(&d->arr.p, arr_bytes);
    if (e == hipSuccess) d->arr.cap = arr_bytes;
    if (e == hipSuccess) e = d->d_ref_len.ensure(std::max<size_t>((size_t)n_ref * 4, 16));
    if (e == hipSuccess) e = d->d_slot_off.ensure(((size_t)n_ref + 1) * 8);
    if (e == hipSuccess) e = d->s1.ensure(std::max<size_t>((size_t)d->n1 * 4, 16));
    if (e == hipSuccess) e = d->s2.ensure(std::max<size_t>((size_t)d->n2 * 4, 16));
    if (e == hipSuccess) e = hipMemsetAsync(d->arr.p, 0, arr_bytes, c->stream);
    if (e == hipSuccess && n_ref) e = hipMemcpyAsync(d->d_ref_len.p, d->ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d->d_slot_off.p, d->slot_off.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->err = std::string("plo_depth_create: ") + hipGetErrorString(e) + " (" + std::to_string(arr_bytes) + " bytes for " + std::to_string(d->n_entries) + " entries)";
        plo_depth_destroy(d);
        return e == hipErrorOutOfMemory ? PLO_ERR_OUT_OF_MEMORY : PLO_ERR_HIP;
    }
    *out = d;
    return PLO_OK;
}

void plo_depth_destroy(plo_depth *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    for (DevBuf *b : {&d->arr, &d->d_ref_len, &d->d_slot_off, &d->s1, &d->s2, &d->win_first, &d->win_sum, &d->run_cnt, &d->run_start, &d->run_partial, &d->runs}) b->release();
    d->h_win.release();
    delete d;
}

plo_status plo_depth_info_get(const plo_depth *d, plo_depth_info *info) {
    if (!d || !info) return PLO_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    info->array = d->arr.as<int32_t>();
    info->n_entries = d->n_entries;
    info->slot_off = d->slot_off.data();
    info->bytes_allocated = d->bytes();
    info->n_ref = d->n_ref;
    info->exclude_flags = d->exclude_flags;
    info->count_deletions = d->count_del;
    info->finished = d->finished.load() ? 1 : 0;
    return PLO_OK;
}

// what every plo_depth_* call on a context begins with: the object is of the context's device and in a state that admits the call
static plo_status depth_enter(plo_ctx *c, plo_depth *d, int call, const char *name) {
    c->err.clear();
    if (d->device != c->ix->device) {
        c->err = std::string(name) + ": the depth object lives on device " + std::to_string(d->device) + ", the context on device " + std::to_string(c->ix->device);
        return PLO_ERR_INVALID_ARG;
    }
    if (!depth_call_allowed(d->finished.load(), call)) {
        c->err = std::string(name) + (d->finished.load() ? ": the depth object is finished (plo_depth_reset reopens it)" : ": the depth object is not finished (plo_depth_finish_dev)");
        return PLO_ERR_INVALID_ARG;
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    for (int i = 0; i < 2; ++i)
        if (!c->dpev[i]) HIP_TRY(c, hipEventCreate(&c->dpev[i]));
    return PLO_OK;
}

// The check and the add (depth_core.hpp): two launches on the context's stream, a wave per record, at most 2048 workgroups of four waves; the
// call's two words come back behind them, one wait.  The add reads the check's word first.
plo_status plo_depth_add_dev(plo_ctx *c, plo_depth *dp, const plo_depth_in *in, plo_depth_add_out *out) {
    if (!c || !dp || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->err_record = UINT32_MAX;
    plo_status ps = depth_enter(c, dp, DEPTH_CALL_ADD, "plo_depth_add_dev");
    if (ps != PLO_OK) return ps;
    const uint32_t n = in->n_records;
    if (n && (!in->bytes || !in->record_off)) {
        c->err = "plo_depth_in: the records and their offsets are required";
        return PLO_ERR_INVALID_ARG;
    }
    if (n > DEPTH_MAX_RECORDS) {
        c->err = "plo_depth_add_dev: more than 2^27 - 1 records";
        return PLO_ERR_RANGE;
    }
    if (!n) return PLO_OK;
    hipStream_t st = c->stream;
    HIP_TRY(c, c->dp_plan.ensure((size_t)n * 8));
    HIP_TRY(c, c->dp_blk.ensure(16));
    HIP_TRY(c, c->h_dp.ensure(16));
    DevDepth d;
    memset(&d, 0, sizeof(d));
    d.s.bytes = in->bytes;
    d.s.n_bytes = in->n_bytes;
    d.s.n = n;
    d.s.record_off = in->record_off;
    d.s.n_ref = dp->n_ref;
    d.ref_len = dp->d_ref_len.as<int32_t>();
    d.slot_off = dp->d_slot_off.as<uint64_t>();
    d.arr = dp->arr.as<int32_t>();
    d.exclude_flags = dp->exclude_flags;
    d.count_del = dp->count_del;
    d.plan = c->dp_plan.as<uint64_t>();
    d.err = c->dp_blk.as<int>();
    d.n_counted = c->dp_blk.as<unsigned>() + 1;
    uint32_t *h = c->h_dp.as<uint32_t>();
    h[0] = (uint32_t)DEPTH_NO_RECORD;
    h[1] = 0;
    HIP_TRY(c, hipMemcpyAsync(c->dp_blk.p, h, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->dpev[0], st));
    const dim3 grid(std::min(2048u, (n + 3u) / 4u));
    hipLaunchKernelGGL(k_depth_check, grid, dim3(256), 0, st, d);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_depth_add, grid, dim3(256), 0, st, d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->dpev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, c->dp_blk.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h[0] != (uint32_t)DEPTH_NO_RECORD) {
        static const char *const what[] = {"", "record_off: it must start at 0, not decrease and end at n_bytes", "its length: fewer than the 36 bytes of block_size and the fixed fields",
                                           "block_size: block_size + 4 differs from the record's length", "refID: outside [-1, n_ref)", "pos: outside [-1, 2^31 - 2]",
                                           "its CIGAR: 36 + l_read_name + 4 n_cigar_op passes the record's end",
                                           "its aux fields: the CIGAR is the placeholder <l_seq>S<n>N, and the fields begin behind the record's end, one in front of the first CG is malformed, or that CG leaves the record",
                                           "its end: the record is counted and reaches beyond ref_len[refID]"};
        out->err_record = h[0] >> 4;
        out->err_kind = h[0] & 15u;
        c->err = "plo_depth_add_dev: record " + std::to_string(out->err_record) + " is refused for " + (out->err_kind >= 1 && out->err_kind <= 8 ? what[out->err_kind] : "an unknown reason") +
                 "; nothing was added";
        return PLO_ERR_INVALID_ARG;
    }
    (void)hipEventElapsedTime(&out->add_ms, c->dpev[0], c->dpev[1]);
    out->n_records = n;
    out->n_counted = h[1];
    return PLO_OK;
}

// tile sums -> their sums -> one wave scans those -> the tiles of the sums -> the tiles of the array
plo_status plo_depth_finish_dev(plo_ctx *c, plo_depth *dp, float *finish_ms) {
    if (!c || !dp) return PLO_ERR_INVALID_ARG;
    if (finish_ms) *finish_ms = 0.f;
    plo_status ps = depth_enter(c, dp, DEPTH_CALL_FINISH, "plo_depth_finish_dev");
    if (ps != PLO_OK) return ps;
    hipStream_t st = c->stream;
    const unsigned long long n0 = dp->n_entries, n1 = dp->n1, n2 = dp->n2;
    if (n1 + 3 > 0x7fffffffull * 4ull) {
        c->err = "plo_depth_finish_dev: more tiles than a launch has workgroups";
        return PLO_ERR_RANGE;
    }
    int32_t *a = dp->arr.as<int32_t>(), *s1 = dp->s1.as<int32_t>(), *s2 = dp->s2.as<int32_t>();
    HIP_TRY(c, hipEventRecord(c->dpev[0], st));
    if (n0) {
        const dim3 g1((unsigned)((n1 + 3) / 4)), g2((unsigned)((n2 + 3) / 4));
        hipLaunchKernelGGL(k_depth_sums, g1, dim3(256), 0, st, (const int32_t *)a, n0, n1, s1);
        hipLaunchKernelGGL(k_depth_sums, g2, dim3(256), 0, st, (const int32_t *)s1, n1, n2, s2);
        hipLaunchKernelGGL(k_depth_top, dim3(1), dim3(64), 0, st, s2, n2);
        hipLaunchKernelGGL(k_depth_apply, g2, dim3(256), 0, st, s1, n1, n2, (const int32_t *)s2);
        hipLaunchKernelGGL(k_depth_apply, g1, dim3(256), 0, st, a, n0, n1, (const int32_t *)s1);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->dpev[1], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (finish_ms) (void)hipEventElapsedTime(finish_ms, c->dpev[0], c->dpev[1]);
    dp->finished.store(true);
    return PLO_OK;
}

// one launch; the table is the host's (ref_len is), the sums come down behind the kernel, one wait
plo_status plo_depth_windows_dev(plo_ctx *c, plo_depth *dp, uint32_t window, plo_depth_windows_out *out) {
    if (!c || !dp || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    plo_status ps = depth_enter(c, dp, DEPTH_CALL_WINDOWS, "plo_depth_windows_dev");
    if (ps != PLO_OK) return ps;
    if (!window) {
        c->err = "plo_depth_windows_dev: the window size must be 1 or more";
        return PLO_ERR_INVALID_ARG;
    }
    hipStream_t st = c->stream;
    const size_t nt = (size_t)dp->n_ref + 1;
    std::vector<uint64_t> first(nt);
    const unsigned long long n_win = depth_win_layout(dp->n_ref, dp->ref_len.data(), window, first.data());
    HIP_TRY(c, dp->h_win.ensure((nt + (size_t)n_win) * 8));
    HIP_TRY(c, dp->win_first.ensure(nt * 8));
    HIP_TRY(c, dp->win_sum.ensure(std::max<size_t>((size_t)n_win * 8, 16)));
    uint64_t *h = dp->h_win.as<uint64_t>();
    memcpy(h, first.data(), nt * 8);
    HIP_TRY(c, hipMemcpyAsync(dp->win_first.p, h, nt * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->dpev[0], st));
    if (n_win) {
        DevDepthWin d;
        memset(&d, 0, sizeof(d));
        d.arr = dp->arr.as<int32_t>();
        d.ref_len = dp->d_ref_len.as<int32_t>();
        d.slot_off = dp->d_slot_off.as<uint64_t>();
        d.win_first = dp->win_first.as<uint64_t>();
        d.n_ref = dp->n_ref;
        d.w = window;
        d.n_win = n_win;
        d.sum = dp->win_sum.as<uint64_t>();
        const unsigned long long waves = window >= 64 ? n_win : (n_win + 63) / 64;
        hipLaunchKernelGGL(k_depth_windows, dim3((unsigned)std::min<unsigned long long>(16384, (waves + 3) / 4)), dim3(256), 0, st, d);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->dpev[1], st));
    if (n_win) HIP_TRY(c, hipMemcpyAsync(h + nt, dp->win_sum.p, (size_t)n_win * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->windows_ms, c->dpev[0], c->dpev[1]);
    out->sum = h + nt;
    out->win_first = h;
    out->n_windows = n_win;
    return PLO_OK;
}

// run starts per tile, the 64-bit scan (records_core.hpp), the count comes down (the runs are sized by it), emit
plo_status plo_depth_runs_dev(plo_ctx *c, plo_depth *dp, plo_depth_runs_out *out) {
    if (!c || !dp || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    plo_status ps = depth_enter(c, dp, DEPTH_CALL_RUNS, "plo_depth_runs_dev");
    if (ps != PLO_OK) return ps;
    static_assert(sizeof(plo_depth_run) == sizeof(DepthRun) && offsetof(plo_depth_run, depth) == offsetof(DepthRun, depth), "plo_depth_run and DepthRun are one layout");
    hipStream_t st = c->stream;
    const unsigned long long n_tiles = dp->n1;
    if (!n_tiles) return PLO_OK;
    if (n_tiles > 0xffffffffull) {
        c->err = "plo_depth_runs_dev: more than 2^32 - 1 tiles";
        return PLO_ERR_RANGE;
    }
    const uint32_t nt = (uint32_t)n_tiles, nb = (nt + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK;
    HIP_TRY(c, dp->run_cnt.ensure((size_t)nt * 8));
    HIP_TRY(c, dp->run_start.ensure(((size_t)nt + 1) * 8));
    HIP_TRY(c, dp->run_partial.ensure((size_t)nb * 8));
    HIP_TRY(c, c->h_dp.ensure(16));
    DevDepthRuns d;
    memset(&d, 0, sizeof(d));
    d.arr = dp->arr.as<int32_t>();
    d.ref_len = dp->d_ref_len.as<int32_t>();
    d.slot_off = dp->d_slot_off.as<uint64_t>();
    d.n_ref = dp->n_ref;
    d.n_entries = dp->n_entries;
    d.cnt = dp->run_cnt.as<unsigned long long>();
    d.start = dp->run_start.as<unsigned long long>();
    unsigned long long *start = dp->run_start.as<unsigned long long>();
    const dim3 grid((nt + 3u) / 4u);
    HIP_TRY(c, hipEventRecord(c->dpev[0], st));
    hipLaunchKernelGGL(k_depth_runs<false>, grid, dim3(256), 0, st, d, n_tiles);
    hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.cnt, nt, nb, dp->run_partial.as<unsigned long long>());
    hipLaunchKernelGGL(k_rec_scan_partials, dim3(1), dim3(64), 0, st, dp->run_partial.as<unsigned long long>(), nt, nb, start);
    hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.cnt, nt, nb, (const unsigned long long *)dp->run_partial.as<unsigned long long>(), start);
    HIP_TRY(c, hipGetLastError());
    unsigned long long *h = c->h_dp.as<unsigned long long>();
    HIP_TRY(c, hipMemcpyAsync(h, start + nt, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const unsigned long long n_runs = h[0];
    HIP_TRY(c, dp->runs.ensure(std::max<size_t>((size_t)n_runs * sizeof(DepthRun), 16)));
    d.run = dp->runs.as<DepthRun>();
    hipLaunchKernelGGL(k_depth_runs<true>, grid, dim3(256), 0, st, d, n_tiles);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->dpev[1], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->runs_ms, c->dpev[0], c->dpev[1]);
    out->run = dp->runs.as<plo_depth_run>();
    out->n_runs = n_runs;
    return PLO_OK;
}

plo_status plo_depth_reset(plo_ctx *c, plo_depth *dp) {
    if (!c || !dp) return PLO_ERR_INVALID_ARG;
    plo_status ps = depth_enter(c, dp, DEPTH_CALL_RESET, "plo_depth_reset");
    if (ps != PLO_OK) return ps;
    if (dp->n_entries) HIP_TRY(c, hipMemsetAsync(dp->arr.p, 0, (size_t)dp->n_entries * 4, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    dp->finished.store(false);
    return PLO_OK;
}

// ---- plo_pileup_* (pileup_core.hpp) -------------------------------------------------------------------------------------------------------------
// the array, exactly its size, zeroed; the tables of the slots
plo_status plo_pileup_create(plo_ctx *c, uint32_t n_ref, const int32_t *ref_len, const plo_pileup_opts *opts, plo_pileup **out) {
    if (!c || !out || (n_ref && !ref_len) || (opts && opts->n_regions && !opts->regions)) return PLO_ERR_INVALID_ARG;
    *out = nullptr;
    c->err.clear();
    if (n_ref > 0x7fffffffu) {
        c->err = "plo_pileup_create: more than 2^31 - 1 references";
        return PLO_ERR_RANGE;
    }
    static_assert(sizeof(plo_pileup_region) == sizeof(PileupRegion) && offsetof(plo_pileup_region, end) == offsetof(PileupRegion, end), "plo_pileup_region and PileupRegion are one layout");
    plo_pileup *d = new plo_pileup();
    d->device = c->ix->device;
    d->n_ref = n_ref;
    if (opts) d->exclude_flags = opts->exclude_flags;
    d->ref_len.assign(ref_len, ref_len + n_ref);
    d->slot_beg.resize((size_t)n_ref + 1);
    d->slot_end.resize((size_t)n_ref + 1);
    d->slot_off.resize((size_t)n_ref + 1);
    uint32_t which = 0;
    const int bad = pileup_layout(n_ref, d->ref_len.data(), opts ? opts->n_regions : 0u, opts ? (const PileupRegion *)opts->regions : nullptr, d->slot_beg.data(), d->slot_end.data(),
                                  d->slot_off.data(), which);
    if (bad) {
        static const char *const what[] = {"", "is negative", "names a chromosome outside [0, n_ref)", "needs 0 <= beg <= end <= ref_len[ref_id]", "is the second region of its chromosome"};
        c->err = std::string("plo_pileup_create: ") + (bad == 1 ? "ref_len[" : "regions[") + std::to_string(which) + "] " + what[bad];
        delete d;
        return PLO_ERR_INVALID_ARG;
    }
    d->n_bases = d->slot_off[n_ref];
    if (hipSetDevice(c->ix->device) != hipSuccess) {
        delete d;
        c->err = "plo_pileup_create: hipSetDevice failed";
        return PLO_ERR_HIP;
    }
    const size_t arr_bytes = std::max<size_t>((size_t)d->n_bases * 4 * PILEUP_CHANNELS, 32), tab = std::max<size_t>((size_t)n_ref * 4, 16);
    hipError_t e = hipMalloc(&d->arr.p, arr_bytes);
    if (e == hipSuccess) d->arr.cap = arr_bytes;
    if (e == hipSuccess) e = d->d_ref_len.ensure(tab);
    if (e == hipSuccess) e = d->d_slot_beg.ensure(tab);
    if (e == hipSuccess) e = d->d_slot_end.ensure(tab);
    if (e == hipSuccess) e = d->d_slot_off.ensure(((size_t)n_ref + 1) * 8);
    if (e == hipSuccess) e = hipMemsetAsync(d->arr.p, 0, arr_bytes, c->stream);
    if (e == hipSuccess && n_ref) e = hipMemcpyAsync(d->d_ref_len.p, d->ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_ref) e = hipMemcpyAsync(d->d_slot_beg.p, d->slot_beg.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_ref) e = hipMemcpyAsync(d->d_slot_end.p, d->slot_end.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d->d_slot_off.p, d->slot_off.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->err = std::string("plo_pileup_create: ") + hipGetErrorString(e) + " (" + std::to_string(arr_bytes) + " bytes for " + std::to_string(d->n_bases) + " bases)";
        plo_pileup_destroy(d);
        return e == hipErrorOutOfMemory ? PLO_ERR_OUT_OF_MEMORY : PLO_ERR_HIP;
    }
    *out = d;
    return PLO_OK;
}

void plo_pileup_destroy(plo_pileup *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    for (DevBuf *b : {&d->arr, &d->d_ref_len, &d->d_slot_off, &d->d_slot_beg, &d->d_slot_end, &d->site_cnt, &d->site_start, &d->site_partial, &d->sites}) b->release();
    delete d;
}

plo_status plo_pileup_info_get(const plo_pileup *d, plo_pileup_info *info) {
    if (!d || !info) return PLO_ERR_INVALID_ARG;
    memset(info, 0, sizeof(*info));
    info->array = d->arr.as<int32_t>();
    info->n_bases = d->n_bases;
    info->slot_off = d->slot_off.data();
    info->slot_beg = d->slot_beg.data();
    info->slot_end = d->slot_end.data();
    info->bytes_allocated = d->bytes();
    info->n_ref = d->n_ref;
    info->exclude_flags = d->exclude_flags;
    return PLO_OK;
}

// what every plo_pileup_* call on a context begins with: the object is of the context's device; with_ref: the context's index has the
// object's chromosomes, with their bases
static plo_status pileup_enter(plo_ctx *c, plo_pileup *d, bool with_ref, const char *name) {
    c->err.clear();
    if (d->device != c->ix->device) {
        c->err = std::string(name) + ": the pileup object lives on device " + std::to_string(d->device) + ", the context on device " + std::to_string(c->ix->device);
        return PLO_ERR_INVALID_ARG;
    }
    if (with_ref) {
        const DevIndex &ix = c->ix->d;
        const std::vector<int> &cl = c->ix->host.chrom_len;
        if (d->n_ref && (!ix.chrom_seq || !ix.chrom_len)) {
            c->err = std::string(name) + ": the context's index has no chrom_seq";
            return PLO_ERR_INVALID_ARG;
        }
        bool same = ix.n_chroms == d->n_ref && cl.size() == (size_t)d->n_ref;
        for (uint32_t r = 0; same && r < d->n_ref; ++r) same = cl[r] == d->ref_len[r];
        if (!same) {
            c->err = std::string(name) + ": the chromosomes of the context's index (" + std::to_string(ix.n_chroms) + ") differ in number or length from the pileup object's (" + std::to_string(d->n_ref) + ")";
            return PLO_ERR_INVALID_ARG;
        }
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    for (int i = 0; i < 2; ++i)
        if (!c->dpev[i]) HIP_TRY(c, hipEventCreate(&c->dpev[i]));
    return PLO_OK;
}

plo_status plo_pileup_reset(plo_ctx *c, plo_pileup *pu) {
    if (!c || !pu) return PLO_ERR_INVALID_ARG;
    plo_status ps = pileup_enter(c, pu, false, "plo_pileup_reset");
    if (ps != PLO_OK) return ps;
    if (pu->n_bases) HIP_TRY(c, hipMemsetAsync(pu->arr.p, 0, (size_t)pu->n_bases * 4 * PILEUP_CHANNELS, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PLO_OK;
}

// The check and the add (pileup_core.hpp): two launches on the context's stream, a wave per record, at most 2048 workgroups of four waves;
// the call's words come back behind them, one wait.  The add reads the check's word first.
plo_status plo_pileup_add_dev(plo_ctx *c, plo_pileup *pu, const plo_depth_in *in, plo_pileup_add_out *out) {
    if (!c || !pu || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->err_record = UINT32_MAX;
    plo_status ps = pileup_enter(c, pu, true, "plo_pileup_add_dev");
    if (ps != PLO_OK) return ps;
    const uint32_t n = in->n_records;
    if (n && (!in->bytes || !in->record_off)) {
        c->err = "plo_pileup_add_dev: the records and their offsets are required";
        return PLO_ERR_INVALID_ARG;
    }
    if (n > DEPTH_MAX_RECORDS) {
        c->err = "plo_pileup_add_dev: more than 2^27 - 1 records";
        return PLO_ERR_RANGE;
    }
    if (!n) return PLO_OK;
    hipStream_t st = c->stream;
    HIP_TRY(c, c->dp_plan.ensure((size_t)n * 8));
    HIP_TRY(c, c->dp_blk.ensure(16));
    HIP_TRY(c, c->h_dp.ensure(16));
    DevPileup d;
    memset(&d, 0, sizeof(d));
    d.s.bytes = in->bytes;
    d.s.n_bytes = in->n_bytes;
    d.s.n = n;
    d.s.record_off = in->record_off;
    d.s.n_ref = pu->n_ref;
    d.ref_len = pu->d_ref_len.as<int32_t>();
    d.slot_off = pu->d_slot_off.as<uint64_t>();
    d.slot_beg = pu->d_slot_beg.as<int32_t>();
    d.slot_end = pu->d_slot_end.as<int32_t>();
    d.arr = pu->arr.as<int32_t>();
    d.exclude_flags = pu->exclude_flags;
    d.chrom_seq = c->ix->d.chrom_seq;
    d.plan = c->dp_plan.as<uint64_t>();
    d.err = c->dp_blk.as<int>();
    d.n_counted = c->dp_blk.as<unsigned>() + 1;
    d.n_events = c->dp_blk.as<unsigned long long>() + 1;
    uint32_t *h = c->h_dp.as<uint32_t>();
    h[0] = (uint32_t)DEPTH_NO_RECORD;
    h[1] = h[2] = h[3] = 0;
    HIP_TRY(c, hipMemcpyAsync(c->dp_blk.p, h, 16, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(c->dpev[0], st));
    const dim3 grid(std::min(2048u, (n + 3u) / 4u));
    hipLaunchKernelGGL(k_pileup_check, grid, dim3(256), 0, st, d);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(k_pileup_add, grid, dim3(256), 0, st, d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->dpev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, c->dp_blk.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h[0] != (uint32_t)DEPTH_NO_RECORD) {
        static const char *const what[] = {"", "record_off: it must start at 0, not decrease and end at n_bytes", "its length: fewer than the 36 bytes of block_size and the fixed fields",
                                           "block_size: block_size + 4 differs from the record's length", "refID: outside [-1, n_ref)", "pos: outside [-1, 2^31 - 2]",
                                           "its CIGAR: 36 + l_read_name + 4 n_cigar_op passes the record's end",
                                           "its aux fields: the CIGAR is the placeholder <l_seq>S<n>N, and the fields begin behind the record's end, one in front of the first CG is malformed, or that CG leaves the record",
                                           "its end: the record is counted and reaches beyond ref_len[refID]", "its bases and qualities: they pass the record's end",
                                           "its read length: the record is counted and the M, I, S, =, X ops of its real CIGAR do not add up to l_seq"};
        out->err_record = h[0] >> 4;
        out->err_kind = h[0] & 15u;
        c->err = "plo_pileup_add_dev: record " + std::to_string(out->err_record) + " is refused for " + (out->err_kind >= 1 && out->err_kind <= 10 ? what[out->err_kind] : "an unknown reason") +
                 "; nothing was added";
        return PLO_ERR_INVALID_ARG;
    }
    (void)hipEventElapsedTime(&out->add_ms, c->dpev[0], c->dpev[1]);
    out->n_records = n;
    out->n_counted = h[1];
    out->n_events = (uint64_t)h[2] | ((uint64_t)h[3] << 32);
    return PLO_OK;
}

// sites per tile, the 64-bit scan (records_core.hpp), the count comes down (the sites are sized by it), emit
plo_status plo_pileup_sites_dev(plo_ctx *c, plo_pileup *pu, const plo_depth *dp, const plo_pileup_sites_opts *opts, plo_pileup_sites_out *out) {
    if (!c || !pu || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    plo_status ps = pileup_enter(c, pu, true, "plo_pileup_sites_dev");
    if (ps != PLO_OK) return ps;
    static_assert(sizeof(plo_pileup_site) == sizeof(PileupSite) && offsetof(plo_pileup_site, count) == offsetof(PileupSite, count), "plo_pileup_site and PileupSite are one layout");
    plo_pileup_sites_opts o = {PLO_PILEUP_MASK_DEFAULT, 1, 0, 1};
    if (opts) o = *opts;
    if (dp && dp->device != pu->device) {
        c->err = "plo_pileup_sites_dev: the depth object lives on another device";
        return PLO_ERR_INVALID_ARG;
    }
    const int bad = pileup_sites_refused(o.min_count, o.frac_num, o.frac_den, dp != nullptr, dp && dp->finished.load(), dp && dp->n_ref == pu->n_ref && dp->ref_len == pu->ref_len);
    if (bad) {
        static const char *const what[] = {"", "min_count must be 1 or more", "frac_den is 0 while frac_num is not", "the depth object is not finished (plo_depth_finish_dev)",
                                           "the depth object was made over another list of chromosomes"};
        c->err = std::string("plo_pileup_sites_dev: ") + what[bad];
        return PLO_ERR_INVALID_ARG;
    }
    hipStream_t st = c->stream;
    const unsigned long long n_tiles = (pu->n_bases + PILEUP_TILE - 1) / PILEUP_TILE;
    if (!n_tiles) return PLO_OK;
    if (n_tiles > 0xffffffffull) {
        c->err = "plo_pileup_sites_dev: more than 2^32 - 1 tiles";
        return PLO_ERR_RANGE;
    }
    const uint32_t nt = (uint32_t)n_tiles, nb = (nt + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK;
    HIP_TRY(c, pu->site_cnt.ensure((size_t)nt * 8));
    HIP_TRY(c, pu->site_start.ensure(((size_t)nt + 1) * 8));
    HIP_TRY(c, pu->site_partial.ensure((size_t)nb * 8));
    HIP_TRY(c, c->h_dp.ensure(16));
    DevPileupSites d;
    memset(&d, 0, sizeof(d));
    d.arr = pu->arr.as<int32_t>();
    d.slot_off = pu->d_slot_off.as<uint64_t>();
    d.slot_beg = pu->d_slot_beg.as<int32_t>();
    d.n_ref = pu->n_ref;
    d.n_bases = pu->n_bases;
    d.depth = dp ? dp->arr.as<int32_t>() : nullptr;
    d.depth_slot_off = dp ? dp->d_slot_off.as<uint64_t>() : nullptr;
    d.chrom_seq = c->ix->d.chrom_seq;
    d.channel_mask = o.channel_mask;
    d.min_count = o.min_count;
    d.frac_num = o.frac_num;
    d.frac_den = o.frac_den;
    d.cnt = pu->site_cnt.as<unsigned long long>();
    d.start = pu->site_start.as<unsigned long long>();
    unsigned long long *start = pu->site_start.as<unsigned long long>();
    const dim3 grid((nt + 3u) / 4u);
    HIP_TRY(c, hipEventRecord(c->dpev[0], st));
    hipLaunchKernelGGL(k_pileup_sites<false>, grid, dim3(256), 0, st, d, n_tiles);
    hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.cnt, nt, nb, pu->site_partial.as<unsigned long long>());
    hipLaunchKernelGGL(k_rec_scan_partials, dim3(1), dim3(64), 0, st, pu->site_partial.as<unsigned long long>(), nt, nb, start);
    hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)d.cnt, nt, nb, (const unsigned long long *)pu->site_partial.as<unsigned long long>(), start);
    HIP_TRY(c, hipGetLastError());
    unsigned long long *h = c->h_dp.as<unsigned long long>();
    HIP_TRY(c, hipMemcpyAsync(h, start + nt, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const unsigned long long n_sites = h[0];
    HIP_TRY(c, pu->sites.ensure(std::max<size_t>((size_t)n_sites * sizeof(PileupSite), 16)));
    d.site = pu->sites.as<PileupSite>();
    hipLaunchKernelGGL(k_pileup_sites<true>, grid, dim3(256), 0, st, d, n_tiles);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->dpev[1], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->sites_ms, c->dpev[0], c->dpev[1]);
    out->site = pu->sites.as<plo_pileup_site>();
    out->n_sites = n_sites;
    return PLO_OK;
}

// The n_bytes at `bytes` as BGZF blocks (deflate.hpp): k_bgzf_deflate into fixed-stride slots, the 64-bit scan of the blocks' sizes,
// k_bgzf_pack.  One wait, behind the pack: the dense buffer is sized for stored blocks, so no size has to come back first.
plo_status plo_bgzf_compress_dev(plo_ctx *c, const uint8_t *bytes, uint64_t n_bytes, int level, plo_bgzf_out *out) {
    if (!c || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    c->err.clear();
    if (level != 0 && level != 1) {
        c->err = "plo_bgzf_compress_dev: level " + std::to_string(level) + ": the device writes stored blocks (0) or its one deflate level (1)";
        return PLO_ERR_INVALID_ARG;
    }
    if (n_bytes && !bytes) {
        c->err = "plo_bgzf_compress_dev: no bytes";
        return PLO_ERR_INVALID_ARG;
    }
    const uint64_t nblk64 = (n_bytes + DEF_MAX_IN - 1) / DEF_MAX_IN;
    if (nblk64 > 0x7fffffffull) {
        c->err = "plo_bgzf_compress_dev: more than 2^31 blocks in one call";
        return PLO_ERR_RANGE;
    }
    const uint32_t n = (uint32_t)nblk64;
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 2; ++i)
        if (!c->zev[i]) HIP_TRY(c, hipEventCreate(&c->zev[i]));
    HIP_TRY(c, c->z_off.ensure(((size_t)n + 1) * 8));
    HIP_TRY(c, c->h_bgzf.ensure(64));
    unsigned long long *h = c->h_bgzf.as<unsigned long long>();
    memset(h, 0, 64);
    out->block_off = c->z_off.as<uint64_t>();
    if (!n) {
        HIP_TRY(c, hipMemsetAsync(c->z_off.p, 0, 8, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        HIP_TRY(c, c->z_out.ensure(16));
        out->blocks = c->z_out.as<uint8_t>();
        return PLO_OK;
    }
    // resident workgroups: three per CU by LDS (sizeof(DefWork) x 4 + 1 KB each)
    const uint32_t per_cu = (uint32_t)std::max<size_t>(1, (160u << 10) / (sizeof(DefWork) * DEF_WAVES + 1024));
    const uint32_t grid = std::min<uint32_t>((n + DEF_WAVES - 1) / DEF_WAVES, (uint32_t)std::max(1, c->n_cus) * per_cu);
    const uint32_t nb = std::max(1u, (n + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK);
    HIP_TRY(c, c->z_slots.ensure((size_t)n * DEF_SLOT));
    HIP_TRY(c, c->z_size.ensure((size_t)n * 8));
    HIP_TRY(c, c->z_partial.ensure((size_t)nb * 8));
    HIP_TRY(c, c->z_out.ensure((size_t)n * DEF_MAX_BLOCK + 16));
    HIP_TRY(c, c->z_err.ensure(16));
    if (level == 1) HIP_TRY(c, c->z_tok.ensure((size_t)grid * DEF_WAVES * DEF_TOK_UNITS * 2));
    unsigned long long *size = c->z_size.as<unsigned long long>(), *off = c->z_off.as<unsigned long long>();
    HIP_TRY(c, hipMemsetAsync(c->z_err.p, 0, 4, st));
    HIP_TRY(c, hipEventRecord(c->zev[0], st));
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(grid), dim3(DEF_WAVES * 64), 0, st, bytes, (unsigned long long)n_bytes, n, level, c->z_slots.as<uint8_t>(), size,
                       c->z_tok.as<uint16_t>(), c->z_err.as<unsigned>());
    hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)size, n, nb, c->z_partial.as<unsigned long long>());
    hipLaunchKernelGGL(k_rec_scan_partials, dim3(1), dim3(64), 0, st, c->z_partial.as<unsigned long long>(), n, nb, off);
    hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 1), dim3(64), 0, st, (const unsigned long long *)size, n, nb, (const unsigned long long *)c->z_partial.as<unsigned long long>(), off);
    hipLaunchKernelGGL(k_bgzf_pack, dim3(std::min<uint32_t>(n, (uint32_t)c->n_cus * 8u)), dim3(256), 0, st, (const uint8_t *)c->z_slots.as<uint8_t>(),
                       (const unsigned long long *)off, n, c->z_out.as<uint8_t>());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->zev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, off + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h + 1, c->z_err.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if ((unsigned)h[1]) {
        c->err = "plo_bgzf_compress_dev: " + std::to_string((unsigned)h[1]) + " blocks were refused by the encoder";
        return PLO_ERR_INTERNAL;
    }
    (void)hipEventElapsedTime(&out->bgzf_ms, c->zev[0], c->zev[1]);
    out->blocks = c->z_out.as<uint8_t>();
    out->n_bytes = h[0];
    out->n_blocks = n;
    out->n_in = n_bytes;
    return PLO_OK;
}

// The window's plo_batch_in / plo_finish_in from its records in device memory (batch_core.hpp): k_bb_table, k_bb_plan, the 64-bit scans of
// the reads' segment and op counts, one wait for the totals and the error word, k_bb_emit.
plo_status plo_batch_build_dev(plo_ctx *c, const plo_batch_build_in *in, plo_batch_build_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->err_read = UINT32_MAX;
    c->err.clear();
    const uint32_t nr = in->n_reads;
    if ((nr && (!in->records || !in->read_rec_off)) || !in->contig_name_off || (in->n_contigs && !in->contig_names)) {
        c->err = "plo_batch_build_in: the records, their offsets and the contig name table are required";
        return PLO_ERR_INVALID_ARG;
    }
    if (nr > 0x7ffffffeu || in->n_contigs > 0x3fffffffu) {
        c->err = "plo_batch_build_dev: more than 2^31 - 2 reads or 2^30 contigs";
        return PLO_ERR_RANGE;
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 4; ++i)
        if (!c->bev[i]) HIP_TRY(c, hipEventCreate(&c->bev[i]));
    const uint32_t nb = std::max(1u, (nr + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK);
    const size_t b = std::max(1u, nr);
    uint32_t slots = 64;
    while (slots < 2 * in->n_contigs) slots <<= 1;
    HIP_TRY(c, c->bb_table.ensure((size_t)slots * 4));
    HIP_TRY(c, c->bb_plan.ensure(b * BB_PLAN_WORDS * 4));
    HIP_TRY(c, c->bb_size.ensure(2 * b * 8));
    HIP_TRY(c, c->bb_start.ensure(2 * (b + 1) * 8));
    HIP_TRY(c, c->bb_partial.ensure(2 * (size_t)nb * 8));
    HIP_TRY(c, c->bb_kind.ensure(b * 4));
    HIP_TRY(c, c->bb_err.ensure(BB_ERR_WORDS * 4));
    HIP_TRY(c, c->bb_rev.ensure(b));
    HIP_TRY(c, c->bb_len.ensure(b * 4));
    HIP_TRY(c, c->bb_soff.ensure(b * 8));
    HIP_TRY(c, c->bb_qoff.ensure(b * 8));
    HIP_TRY(c, c->bb_flags.ensure(b * 2));
    HIP_TRY(c, c->h_bb.ensure(64));
    DevBatchBuild d;
    memset(&d, 0, sizeof(d));
    d.records = in->records;
    d.records_bytes = in->records_bytes;
    d.read_rec_off = in->read_rec_off;
    d.n_reads = nr;
    d.n_contigs = in->n_contigs;
    d.contig_name_off = in->contig_name_off;
    d.contig_names = in->contig_names;
    d.table = c->bb_table.as<uint32_t>();
    d.table_mask = slots - 1;
    d.plan = c->bb_plan.as<uint32_t>();
    d.size = c->bb_size.as<unsigned long long>();
    d.start = c->bb_start.as<unsigned long long>();
    d.err_kind = c->bb_kind.as<uint32_t>();
    d.err = c->bb_err.as<int>();
    d.read_is_reverse = c->bb_rev.as<uint8_t>();
    d.read_seq_len = c->bb_len.as<uint32_t>();
    d.read_seq_off = c->bb_soff.as<uint64_t>();
    d.read_qual_off = c->bb_qoff.as<uint64_t>();
    d.read_flags = c->bb_flags.as<uint16_t>();
    unsigned long long *start = c->bb_start.as<unsigned long long>();
    unsigned long long *h = c->h_bb.as<unsigned long long>();
    memset(h, 0, 64);
    int *herr = (int *)(h + 2);  // [BB_ERR_WORDS], then the failing read's kind
    herr[0] = BB_NO_READ;
    if (nr) {
        HIP_TRY(c, hipMemsetAsync(c->bb_table.p, 0, (size_t)slots * 4, st));
        HIP_TRY(c, hipMemcpyAsync(c->bb_err.p, herr, BB_ERR_WORDS * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipEventRecord(c->bev[0], st));
        if (in->n_contigs) hipLaunchKernelGGL(k_bb_table, dim3((in->n_contigs + 255) / 256), dim3(256), 0, st, d);
        hipLaunchKernelGGL(k_bb_plan, dim3((nr + 3) / 4), dim3(256), 0, st, d);
        hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 2), dim3(64), 0, st, (const unsigned long long *)d.size, nr, nb, c->bb_partial.as<unsigned long long>());
        hipLaunchKernelGGL(k_rec_scan_partials, dim3(2), dim3(64), 0, st, c->bb_partial.as<unsigned long long>(), nr, nb, start);
        hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 2), dim3(64), 0, st, (const unsigned long long *)d.size, nr, nb, (const unsigned long long *)c->bb_partial.as<unsigned long long>(), start);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->bev[1], st));
        // the one round trip for the sizes: total segments, total ops, the bounds counters and the lowest failing read
        HIP_TRY(c, hipMemcpyAsync(h, start + nr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h + 1, start + (size_t)nr + 1 + nr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(herr, c->bb_err.p, BB_ERR_WORDS * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (herr[1 + REC_ERR_OFFSET] || herr[1 + REC_ERR_BLOCK] || herr[1 + REC_ERR_LAYOUT]) {
            c->err = "plo_batch_build_dev: " + std::to_string(herr[1 + REC_ERR_OFFSET]) + " read_rec_off beyond records_bytes, " + std::to_string(herr[1 + REC_ERR_BLOCK]) +
                     " block_size running past the end of `records`, " + std::to_string(herr[1 + REC_ERR_LAYOUT]) +
                     " l_qname / n_cigar / l_seq pointing outside their record; no batch was built";
            return PLO_ERR_INVALID_ARG;
        }
        if (herr[0] != BB_NO_READ) {
            uint32_t kind = 0;
            HIP_TRY(c, hipMemcpyAsync(&herr[BB_ERR_WORDS], d.err_kind + herr[0], 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            kind = (uint32_t)herr[BB_ERR_WORDS];
            static const char *const what[] = {"no failure", "the SA aux field is not a string", "an SA segment without exactly six fields", "a malformed SA segment",
                                               "an SA segment without an aligned op", "an SA segment whose read length differs from the primary record's",
                                               "an SA segment on a contig the header does not name", "a split segment that covers no read base"};
            out->err_read = (uint32_t)herr[0];
            out->err_kind = kind;
            c->err = "plo_batch_build_dev: read " + std::to_string(herr[0]) + ": " + (kind < 8 ? what[kind] : "?") + " (kind " + std::to_string(kind) + ")";
            return PLO_ERR_DATA;
        }
    }
    const unsigned long long ns = h[0], n_ops = h[1];
    if (n_ops > 0x7fffffffull || ns > 0xfffffffeull) {
        c->err = "plo_batch_build_dev: window carries more than 2^31 - 1 CIGAR ops; read fewer records per window";
        return PLO_ERR_RANGE;
    }
    const size_t sb = std::max<size_t>(ns, 1);
    HIP_TRY(c, c->bb_tkey.ensure(sb * 8));
    HIP_TRY(c, c->bb_tnops.ensure(sb * 4));
    HIP_TRY(c, c->bb_tctext.ensure(sb * 4));
    HIP_TRY(c, c->bb_tclen.ensure(sb * 4));
    HIP_TRY(c, c->bb_tcontig.ensure(sb * 4));
    HIP_TRY(c, c->bb_tdst.ensure(sb * 4));
    HIP_TRY(c, c->bb_tpos.ensure(sb * 8));
    HIP_TRY(c, c->bb_tfwd.ensure(sb));
    HIP_TRY(c, c->bb_sread.ensure(sb * 4));
    HIP_TRY(c, c->bb_scontig.ensure(sb * 4));
    HIP_TRY(c, c->bb_spos.ensure(sb * 8));
    HIP_TRY(c, c->bb_sfwd.ensure(sb));
    HIP_TRY(c, c->bb_coff.ensure((sb + 1) * 4));
    HIP_TRY(c, c->bb_cigar.ensure(std::max<size_t>(n_ops, 1) * 4));
    d.t_key = c->bb_tkey.as<unsigned long long>();
    d.t_nops = c->bb_tnops.as<uint32_t>();
    d.t_ctext = c->bb_tctext.as<uint32_t>();
    d.t_clen = c->bb_tclen.as<uint32_t>();
    d.t_contig = c->bb_tcontig.as<uint32_t>();
    d.t_dst = c->bb_tdst.as<uint32_t>();
    d.t_pos = c->bb_tpos.as<long long>();
    d.t_fwd = c->bb_tfwd.as<uint8_t>();
    d.seg_read = c->bb_sread.as<uint32_t>();
    d.seg_contig = c->bb_scontig.as<uint32_t>();
    d.seg_pos = c->bb_spos.as<int64_t>();
    d.seg_fwd = c->bb_sfwd.as<uint8_t>();
    d.seg_cigar_off = c->bb_coff.as<uint32_t>();
    d.cigar = c->bb_cigar.as<uint32_t>();
    float a_ms = 0, b_ms = 0;
    if (nr) {
        HIP_TRY(c, hipEventRecord(c->bev[2], st));
        hipLaunchKernelGGL(k_bb_emit, dim3(std::min<uint32_t>((nr + 3) / 4, (uint32_t)std::max(1, c->n_cus) * 8u)), dim3(256), 0, st, d);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->bev[3], st));
        HIP_TRY(c, hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&a_ms, c->bev[0], c->bev[1]);
        (void)hipEventElapsedTime(&b_ms, c->bev[2], c->bev[3]);
    } else {
        HIP_TRY(c, hipMemsetAsync(c->bb_coff.p, 0, 4, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    out->batch_ms = a_ms + b_ms;
    plo_batch_in &bi = out->batch;
    bi.n_reads = nr;
    bi.read_is_reverse = d.read_is_reverse;
    bi.read_seq_len = d.read_seq_len;
    bi.read_seq_off = d.read_seq_off;
    bi.seq = in->records;
    bi.seq_bytes = in->records_bytes;
    bi.seq_fmt = PLO_SEQ_BAM4;
    bi.n_segs = (uint32_t)ns;
    bi.seg_read = d.seg_read;
    bi.seg_contig = d.seg_contig;
    bi.seg_pos = d.seg_pos;
    bi.seg_is_fwd_strand = d.seg_fwd;
    bi.seg_cigar_off = d.seg_cigar_off;
    bi.cigar = d.cigar;
    out->fin.read_flags = d.read_flags;
    out->fin.qual = in->records;
    out->fin.read_qual_off = d.read_qual_off;
    out->fin.qual_bytes = in->records_bytes;
    return PLO_OK;
}

plo_status plo_compact_output_dev(plo_ctx *c, plo_batch_out *out) {
    if (!c || !out) return PLO_ERR_INVALID_ARG;
    c->err.clear();
    if (!c->have_last || out->n_items != c->last_wk.n_items) {
        c->err = "plo_compact_output_dev: `out` is not the result of the context's last plo_liftover_batch_dev";
        return PLO_ERR_INVALID_ARG;
    }
    if (c->last_wk.out_cigar == c->o_cigar_dense.as<uint32_t>()) {  // already dense
        out->cigar = c->o_cigar_dense.as<uint32_t>();
        out->n_cigar = c->dense_total;
        return PLO_OK;
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    const uint32_t n = out->n_items;
    HIP_TRY(c, c->o_dense_off.ensure(((size_t)n + 1) * 4));
    plo_status s = scan_u32(c, c->o_clen.as<uint32_t>(), n, c->o_dense_off.as<uint32_t>());
    if (s != PLO_OK) return s;
    uint32_t *h = c->h_counters.as<uint32_t>();
    h[0] = 0;
    if (n) HIP_TRY(c, hipMemcpyAsync(h, c->o_dense_off.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const uint64_t total = h[0];
    HIP_TRY(c, c->o_cigar_dense.ensure(std::max<uint64_t>(total, 4) * 4));
    if (n)
        hipLaunchKernelGGL(k_compact_cigar, dim3((unsigned)(((unsigned long long)n * 8 + 255) / 256)), dim3(256), 0, st,
                           (const uint32_t *)c->o_cigar.as<uint32_t>(), c->o_coff.as<uint64_t>(), (const uint32_t *)c->o_clen.as<uint32_t>(),
                           (const uint32_t *)c->o_dense_off.as<uint32_t>(), n, c->o_cigar_dense.as<uint32_t>());
    HIP_TRY(c, hipGetLastError());
    c->last_wk.out_cigar = c->o_cigar_dense.as<uint32_t>();
    out->cigar = c->o_cigar_dense.as<uint32_t>();
    out->n_cigar = total;
    c->dense_total = total;
    return PLO_OK;
}

// Inflates the n BGZF blocks of one chunk on the device (bam_host.cpp's reader when PLO_BGZF_DEVICE is not 0): `comp` = the
// chunk's compressed bytes (host, pageable or pinned), `blks` = BgzfBlk[n] with offsets inside comp / out, `out` = host
// destination (page-locked for a direct DMA).  Returns 0, or a negative number when the device is unusable / a block is corrupt
// (the caller then inflates on the host, which also produces the diagnostics).  Not part of the public ABI.
static uint32_t bgzf_workgroups() {  // resident workgroups of k_bgzf_inflate on the current device
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return (uint32_t)std::max(1, cus) * (uint32_t)std::max<size_t>(1, (160u << 10) / (sizeof(InfLds) * INF_WAVES));
}
uint32_t plo_internal_bgzf_slots(void) { return bgzf_workgroups() * INF_WAVES; }
// Two slots (stream + device buffers each), so that the caller stages the next group of blocks and checks the CRCs of the previous
// one while the device inflates: begin() enqueues upload, kernel and download of a group, wait() returns when its bytes are in
// `out`.  acquire() / release() bracket a sequence of begin / wait calls (one user at a time).
namespace {
struct InfSlot {
    DevBuf d_comp, d_out, d_blk, d_st;
    HostBuf h_blk, h_st;
    hipStream_t st = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    uint32_t n = 0;
    size_t comp_bytes = 0, out_bytes = 0;
    bool busy = false;
};
struct InfDev {  // one set of slots per device (a reader inflates on the device it was opened for)
    InfSlot slot[2];
    int ok = -1;
};
std::map<int, InfDev> g_inf_devs;
InfDev *g_inf_cur = nullptr;  // the set of the sequence in progress (under g_inf_mu)
int g_inf_prev_dev = -1;      // the calling thread's device before set_device(), restored by release()
std::mutex g_inf_mu;
}  // namespace
void plo_internal_bgzf_acquire(void) {
    g_inf_mu.lock();
    g_inf_cur = nullptr;
    g_inf_prev_dev = -1;
}
int plo_internal_bgzf_set_device(int dev) {  // under acquire(): the sequence runs on `dev` (the calling thread's device until release())
    if (dev < 0) dev = 0;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) return -100;
    if (hipSetDevice(dev) != hipSuccess) return -100;
    g_inf_prev_dev = prev;
    g_inf_cur = &g_inf_devs[dev];
    return 0;
}
void plo_internal_bgzf_release(void) {
    if (g_inf_prev_dev >= 0) (void)hipSetDevice(g_inf_prev_dev);
    g_inf_cur = nullptr;
    g_inf_prev_dev = -1;
    g_inf_mu.unlock();
}
int plo_internal_bgzf_begin(int slot, const uint8_t *comp, size_t comp_bytes, const void *blks, uint32_t n, uint8_t *out, size_t out_bytes, const uint32_t *crcs) {
    if (slot < 0 || slot > 1) return -101;
    if (!g_inf_cur) {  // no set_device(): the calling thread's current device
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return -100;
        g_inf_cur = &g_inf_devs[dev];
    }
    InfDev &D = *g_inf_cur;
    if (D.ok < 0) {
        int nd = 0;
        D.ok = (hipGetDeviceCount(&nd) == hipSuccess && nd > 0 && hipStreamCreateWithFlags(&D.slot[0].st, hipStreamNonBlocking) == hipSuccess &&
                hipStreamCreateWithFlags(&D.slot[1].st, hipStreamNonBlocking) == hipSuccess)
                   ? 1
                   : 0;
    }
    if (!D.ok) return -100;
    InfSlot &q = D.slot[slot];
    q.n = n;
    q.busy = false;
    if (!n) return 0;
    // (the blocks' descriptors and, behind them, their expected CRCs travel as one array)
    const size_t blk_bytes = (size_t)n * sizeof(BgzfBlk), crc_bytes = crcs ? (size_t)n * 4 : 0;
    if (q.d_comp.ensure(comp_bytes + 16) != hipSuccess || q.d_out.ensure(out_bytes + 16) != hipSuccess || q.d_blk.ensure(blk_bytes + crc_bytes) != hipSuccess ||
        q.d_st.ensure((size_t)n * 4) != hipSuccess || q.h_blk.ensure(blk_bytes + crc_bytes) != hipSuccess || q.h_st.ensure((size_t)n * 4) != hipSuccess)
        return -101;
    const bool dbg = getenv("PLO_DEBUG_INFLATE") != nullptr;
    if (dbg && !q.ev[0])
        for (auto &e : q.ev) (void)hipEventCreate(&e);
    memcpy(q.h_blk.p, blks, blk_bytes);  // (the caller's arrays may go away before the copy runs)
    if (crcs) memcpy((uint8_t *)q.h_blk.p + blk_bytes, crcs, crc_bytes);
    hipStream_t st = q.st;
    if (dbg) (void)hipEventRecord(q.ev[0], st);
    if (hipMemcpyAsync(q.d_comp.p, comp, comp_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return -102;
    if (hipMemcpyAsync(q.d_blk.p, q.h_blk.p, blk_bytes + crc_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return -102;
    if (dbg) (void)hipEventRecord(q.ev[1], st);
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(std::min<uint32_t>((n + INF_WAVES - 1) / INF_WAVES, bgzf_workgroups())), dim3(INF_WAVES * 64), 0, st,
                       (const uint8_t *)q.d_comp.p, (const BgzfBlk *)q.d_blk.p, n, (uint8_t *)q.d_out.p, (int *)q.d_st.p);
    if (crcs)
        hipLaunchKernelGGL(k_bgzf_crc, dim3(std::min<uint32_t>((n + INF_WAVES - 1) / INF_WAVES, (uint32_t)bgzf_workgroups() * 4u)), dim3(INF_WAVES * 64), 0, st,
                           (const uint8_t *)q.d_out.p, (const BgzfBlk *)q.d_blk.p, n, (const uint32_t *)((const uint8_t *)q.d_blk.p + blk_bytes), (int *)q.d_st.p);
    if (hipGetLastError() != hipSuccess) return -103;
    if (dbg) (void)hipEventRecord(q.ev[2], st);
    if (hipMemcpyAsync(out, q.d_out.p, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return -104;
    if (hipMemcpyAsync(q.h_st.p, q.d_st.p, (size_t)n * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return -104;
    if (dbg) (void)hipEventRecord(q.ev[3], st);
    q.comp_bytes = comp_bytes;
    q.out_bytes = out_bytes;
    q.busy = true;
    return 0;
}
int plo_internal_bgzf_wait(int slot) {
    if (slot < 0 || slot > 1) return -101;
    if (!g_inf_cur) return 0;  // nothing was begun
    InfSlot &q = g_inf_cur->slot[slot];
    if (!q.busy) return 0;
    q.busy = false;
    if (hipStreamSynchronize(q.st) != hipSuccess) return -105;
    if (getenv("PLO_DEBUG_INFLATE") && q.ev[0]) {
        float a = 0, b = 0, c2 = 0;
        (void)hipEventElapsedTime(&a, q.ev[0], q.ev[1]);
        (void)hipEventElapsedTime(&b, q.ev[1], q.ev[2]);
        (void)hipEventElapsedTime(&c2, q.ev[2], q.ev[3]);
        fprintf(stderr, "[plo] device inflate: %u blocks, %.1f MB -> %.1f MB: H2D %.2f ms, kernel %.2f ms, D2H %.2f ms\n", q.n, q.comp_bytes / 1e6, q.out_bytes / 1e6, a, b, c2);
    }
    const int *stv = q.h_st.as<int>();
    for (uint32_t i = 0; i < q.n; ++i)
        if (stv[i] != 0) return -200;
    return 0;
}
int plo_internal_bgzf_inflate(const uint8_t *comp, size_t comp_bytes, const void *blks, uint32_t n, uint8_t *out, size_t out_bytes) {
    std::lock_guard<std::mutex> g(g_inf_mu);
    g_inf_cur = nullptr;
    int rc = plo_internal_bgzf_begin(0, comp, comp_bytes, blks, n, out, out_bytes, nullptr);
    rc = rc ? rc : plo_internal_bgzf_wait(0);
    g_inf_cur = nullptr;
    return rc;
}

// The inflated BAM stream kept on the device: the header walk on the host (bgzf_walk.hpp), then upload, k_bgzf_inflate and k_bgzf_crc on the
// context's stream straight into the caller's buffer -- plo_internal_bgzf_begin without its copy down.
// (a part of a file, plo_bgzf_inflate_part_dev: where bgzf[0] lies in the file and where the part ends -> *own_bytes, bgzf_walk.hpp)
static plo_status bgzf_inflate(plo_ctx *c, const plo_bgzf_inflate_in *in, plo_bgzf_inflate_out *out, uint64_t file_off, uint64_t range_end, uint64_t *own_bytes) {
    memset(out, 0, sizeof(*out));
    *own_bytes = 0;
    c->err.clear();
    if (!in->bgzf_bytes) return PLO_OK;
    if (!in->bgzf || (in->dst_cap && !in->dst)) {
        c->err = "plo_bgzf_inflate_in: bgzf and dst are required";
        return PLO_ERR_INVALID_ARG;
    }
    std::vector<BgzfWalkBlk> blks;
    uint64_t consumed = 0, n_bytes = 0;
    const int rc = bgzf_walk(in->bgzf, (size_t)in->bgzf_bytes, in->dst_cap, blks, &consumed, &n_bytes, file_off, range_end, own_bytes);
    if (rc != BGZF_WALK_OK) {
        c->err = std::string("plo_bgzf_inflate_dev: ") + (rc == BGZF_WALK_NOT_A_HEADER ? "not a BGZF block" : rc == BGZF_WALK_CORRUPT ? "corrupt BGZF block (no BC subfield, or a BSIZE below the header's own size)" : "BGZF block larger than 64 KiB") +
                 " at offset " + std::to_string(consumed);
        return PLO_ERR_IO;
    }
    out->bgzf_consumed = consumed;
    out->n_bytes = n_bytes;
    out->n_blocks = (uint32_t)blks.size();
    const uint32_t n = (uint32_t)blks.size();
    if (!n || !n_bytes) return PLO_OK;
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 2; ++i)
        if (!c->iev[i]) HIP_TRY(c, hipEventCreate(&c->iev[i]));
    const size_t blk_bytes = (size_t)n * sizeof(BgzfBlk), crc_bytes = (size_t)n * 4;
    HIP_TRY(c, c->ci_comp.ensure((size_t)consumed + 16));
    HIP_TRY(c, c->ci_blk.ensure(blk_bytes + crc_bytes));
    HIP_TRY(c, c->ci_st.ensure((size_t)n * 4));
    HIP_TRY(c, c->h_ci.ensure(blk_bytes + crc_bytes + (size_t)n * 4));
    BgzfBlk *hb = c->h_ci.as<BgzfBlk>();
    uint32_t *hcrc = (uint32_t *)((uint8_t *)c->h_ci.p + blk_bytes);
    int *hst = (int *)((uint8_t *)c->h_ci.p + blk_bytes + crc_bytes);
    for (uint32_t i = 0; i < n; ++i) {
        hb[i] = BgzfBlk{blks[i].coff, blks[i].uoff, (uint32_t)blks[i].clen, (uint32_t)blks[i].ulen};
        hcrc[i] = blks[i].crc;
    }
    HIP_TRY(c, hipEventRecord(c->iev[0], st));
    HIP_TRY(c, hipMemcpyAsync(c->ci_comp.p, in->bgzf, (size_t)consumed, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->ci_blk.p, c->h_ci.p, blk_bytes + crc_bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(std::min<uint32_t>((n + INF_WAVES - 1) / INF_WAVES, bgzf_workgroups())), dim3(INF_WAVES * 64), 0, st,
                       (const uint8_t *)c->ci_comp.p, (const BgzfBlk *)c->ci_blk.p, n, in->dst, c->ci_st.as<int>());
    hipLaunchKernelGGL(k_bgzf_crc, dim3(std::min<uint32_t>((n + INF_WAVES - 1) / INF_WAVES, (uint32_t)bgzf_workgroups() * 4u)), dim3(INF_WAVES * 64), 0, st,
                       (const uint8_t *)in->dst, (const BgzfBlk *)c->ci_blk.p, n, (const uint32_t *)((const uint8_t *)c->ci_blk.p + blk_bytes), c->ci_st.as<int>());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(hst, c->ci_st.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipEventRecord(c->iev[1], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->inflate_ms, c->iev[0], c->iev[1]);
    for (uint32_t i = 0; i < n; ++i)
        if (hst[i] != 0) {
            c->err = "plo_bgzf_inflate_dev: the BGZF block at offset " + std::to_string(blks[i].off) + (hst[i] == -10 ? " fails its CRC-32" : " does not decode (status " + std::to_string(hst[i]) + ")");
            out->n_blocks = 0;
            out->bgzf_consumed = 0;
            out->n_bytes = 0;
            *own_bytes = 0;
            return PLO_ERR_IO;
        }
    return PLO_OK;
}
plo_status plo_bgzf_inflate_dev(plo_ctx *c, const plo_bgzf_inflate_in *in, plo_bgzf_inflate_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    uint64_t own = 0;
    return bgzf_inflate(c, in, out, 0, UINT64_MAX, &own);
}
plo_status plo_bgzf_inflate_part_dev(plo_ctx *c, const plo_bgzf_inflate_part_in *in, plo_bgzf_inflate_part_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    const plo_bgzf_inflate_in pin = {in->bgzf, in->bgzf_bytes, in->dst, in->dst_cap};
    plo_bgzf_inflate_out po;
    uint64_t own = 0;
    const plo_status st = bgzf_inflate(c, &pin, &po, in->bgzf_file_off, in->range_end, &own);
    out->n_blocks = po.n_blocks;
    out->bgzf_consumed = po.bgzf_consumed;
    out->n_bytes = po.n_bytes;
    out->inflate_ms = po.inflate_ms;
    out->own_bytes = own;
    return st;
}

// The windows of plo_bam_read_window cut on the device (window_core.hpp): k_cut_guess, k_cut_walk, k_cut_resolve, the 64-bit scans of the
// segments' counts, k_cut_find, one wait for the result block, then k_cut_emit and k_cut_copy.
static plo_status window_cut(plo_ctx *c, const plo_window_cut_in *in, plo_window_cut_out *out, unsigned long long seg_bytes, uint64_t own_bytes = UINT64_MAX) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->err_off = UINT64_MAX;
    c->err.clear();
    if (!in->max_records || (in->stream_bytes && !in->stream) || seg_bytes < 64) {
        c->err = "plo_window_cut_in: max_records and the stream are required";
        return PLO_ERR_INVALID_ARG;
    }
    const unsigned long long n = in->stream_bytes;
    if (n / seg_bytes + 1 > 0x7ffffffeull) {
        c->err = "plo_window_cut_dev: more than 2^31 - 2 segments";
        return PLO_ERR_RANGE;
    }
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 4; ++i)
        if (!c->wev[i]) HIP_TRY(c, hipEventCreate(&c->wev[i]));
    const uint32_t ns = (uint32_t)(n / seg_bytes + 1);
    const uint32_t nb = (ns + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK;
    HIP_TRY(c, c->wc_guess.ensure((size_t)ns * 8));
    HIP_TRY(c, c->wc_land.ensure((size_t)ns * 8));
    HIP_TRY(c, c->wc_cnt.ensure(3 * (size_t)ns * 8));
    HIP_TRY(c, c->wc_start.ensure(3 * ((size_t)ns + 1) * 8));
    HIP_TRY(c, c->wc_partial.ensure(3 * (size_t)nb * 8));
    HIP_TRY(c, c->wc_fire.ensure(5 * (size_t)ns * 8));
    HIP_TRY(c, c->wc_res.ensure(CR_WORDS * 8));
    HIP_TRY(c, c->h_wc.ensure(CR_WORDS * 8));
    DevCut d;
    memset(&d, 0, sizeof(d));
    d.stream = in->stream;
    d.n = n;
    d.seg_bytes = seg_bytes;
    d.n_seg = ns;
    d.max_records = in->max_records;
    d.max_unmapped = in->max_unmapped ? in->max_unmapped : 4ull * in->max_records + 1024;
    d.max_bytes = in->max_bytes ? in->max_bytes : std::max<unsigned long long>(1ull << 30, std::min<unsigned long long>(8ull << 30, (unsigned long long)in->max_records << 16));
    d.final = in->final ? 1 : 0;
    d.ranged = own_bytes != UINT64_MAX;
    d.own_bytes = own_bytes;
    d.guess = c->wc_guess.as<unsigned long long>();
    d.land = c->wc_land.as<unsigned long long>();
    d.cnt = c->wc_cnt.as<unsigned long long>();
    d.start = c->wc_start.as<unsigned long long>();
    d.fire = c->wc_fire.as<unsigned long long>();
    d.res = c->wc_res.as<unsigned long long>();
    unsigned long long *start = c->wc_start.as<unsigned long long>();
    unsigned long long *h = c->h_wc.as<unsigned long long>();
    HIP_TRY(c, hipEventRecord(c->wev[0], st));
    hipLaunchKernelGGL(k_cut_guess, dim3((ns + 3) / 4), dim3(256), 0, st, d);
    hipLaunchKernelGGL(k_cut_walk, dim3((ns + 63) / 64), dim3(64), 0, st, d);
    hipLaunchKernelGGL(k_cut_resolve, dim3(1), dim3(64), 0, st, d);
    hipLaunchKernelGGL(k_rec_scan_sums, dim3(nb, 3), dim3(64), 0, st, (const unsigned long long *)d.cnt, ns, nb, c->wc_partial.as<unsigned long long>());
    hipLaunchKernelGGL(k_rec_scan_partials, dim3(3), dim3(64), 0, st, c->wc_partial.as<unsigned long long>(), ns, nb, start);
    hipLaunchKernelGGL(k_rec_scan_apply, dim3(nb, 3), dim3(64), 0, st, (const unsigned long long *)d.cnt, ns, nb, (const unsigned long long *)c->wc_partial.as<unsigned long long>(), start);
    hipLaunchKernelGGL(k_cut_find, dim3((ns + 63) / 64), dim3(64), 0, st, d);
    hipLaunchKernelGGL(k_cut_result, dim3(1), dim3(1), 0, st, d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->wev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, d.res, CR_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));  // the one round trip for the counts that size the outputs
    const unsigned long long at = h[CR_AT], why = h[CR_WHY];
    out->n_rewalks = (uint32_t)std::min<unsigned long long>(h[CR_REWALKS], 0xffffffffull);
    if (at > n || why == CUT_NONE) {
        c->err = "plo_window_cut_dev: no end of the window found (internal)";
        return PLO_ERR_INTERNAL;
    }
    if (why >= CUT_WHY_ERR_TRUNC) {
        out->err_off = at;
        const char *what = why == CUT_WHY_ERR_TRUNC ? "truncated BAM record" : why == CUT_WHY_ERR_SHORT ? "BAM record shorter than its fixed fields" : why == CUT_WHY_ERR_LAYOUT ? "BAM record fields exceed its block_size"
                                                                                                                                                                                  : "unmapped record placed on a contig (flag 0x4 with a reference id): the reference aborts on it (read_alignment_scanner.rs:396)";
        c->err = std::string("plo_window_cut_dev: ") + what + " at offset " + std::to_string(at);
        return why == CUT_WHY_ERR_UNM_TID ? PLO_ERR_DATA : PLO_ERR_IO;
    }
    if (h[CR_READS] > 0xfffffffeull || h[CR_UNMAPPED] > 0xfffffffeull) {
        c->err = "plo_window_cut_dev: more than 2^32 - 2 records in the window";
        return PLO_ERR_RANGE;
    }
    const unsigned long long nr = h[CR_READS], nu = h[CR_UNMAPPED], ub = h[CR_UNM_BYTES];
    HIP_TRY(c, c->wc_recoff.ensure(std::max<size_t>(nr, 1) * 8));
    HIP_TRY(c, c->wc_unmoff.ensure(((size_t)nu + 1) * 8));
    HIP_TRY(c, c->wc_unmsrc.ensure(std::max<size_t>(nu, 1) * 8));
    HIP_TRY(c, c->wc_unm.ensure(std::max<size_t>(ub, 16)));
    d.cut_at = at;
    d.read_rec_off = c->wc_recoff.as<uint64_t>();
    d.unm_off = c->wc_unmoff.as<uint64_t>();
    d.unm_src = c->wc_unmsrc.as<uint64_t>();
    d.unmapped = c->wc_unm.as<uint8_t>();
    d.n_unmapped = nu;
    d.unmapped_bytes = ub;
    HIP_TRY(c, hipEventRecord(c->wev[2], st));
    hipLaunchKernelGGL(k_cut_emit, dim3((ns + 63) / 64), dim3(64), 0, st, d);
    if (nu) hipLaunchKernelGGL(k_cut_copy, dim3((uint32_t)std::min<unsigned long long>(nu, (unsigned long long)std::max(1, c->n_cus) * 8ull)), dim3(256), 0, st, d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->wev[3], st));
    HIP_TRY(c, hipStreamSynchronize(st));
    float a_ms = 0, b_ms = 0;
    (void)hipEventElapsedTime(&a_ms, c->wev[0], c->wev[1]);
    (void)hipEventElapsedTime(&b_ms, c->wev[2], c->wev[3]);
    out->cut_ms = a_ms + b_ms;
    out->n_reads = (uint32_t)nr;
    out->read_rec_off = d.read_rec_off;
    out->n_unmapped = (uint32_t)nu;
    out->unmapped_off = d.unm_off;
    out->unmapped = d.unmapped;
    out->unmapped_bytes = ub;
    out->window_bytes = at;
    out->ended_by = (int32_t)why;
    return PLO_OK;
}
plo_status plo_window_cut_dev(plo_ctx *c, const plo_window_cut_in *in, plo_window_cut_out *out) { return window_cut(c, in, out, PLO_CUT_SEG_BYTES); }
plo_status plo_window_cut_part_dev(plo_ctx *c, const plo_window_cut_part_in *in, plo_window_cut_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    const plo_window_cut_in win = {in->stream, in->stream_bytes, in->max_records, in->max_unmapped, in->max_bytes, in->final};
    return window_cut(c, &win, out, PLO_CUT_SEG_BYTES, in->own_bytes);
}
// (tests: the same call with segments of another size; not part of the public ABI)
plo_status plo_internal_window_cut_seg(plo_ctx *c, const plo_window_cut_in *in, plo_window_cut_out *out, uint64_t seg_bytes) { return window_cut(c, in, out, seg_bytes); }

// The first record of a part (window_core.hpp): k_part_start over tiles of PART_TILE candidates, then one wait for the two minima.
static constexpr unsigned long long PART_TILE = 256;
plo_status plo_part_start_dev(plo_ctx *c, const plo_part_start_in *in, plo_part_start_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->kind = PLO_PART_NONE;
    out->first_off = UINT64_MAX;
    c->err.clear();
    if (in->stream_bytes && !in->stream) {
        c->err = "plo_part_start_in: the stream is required";
        return PLO_ERR_INVALID_ARG;
    }
    if (in->stream_bytes < 36) return PLO_OK;  // (no candidate)
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    for (int i = 0; i < 2; ++i)
        if (!c->wev[i]) HIP_TRY(c, hipEventCreate(&c->wev[i]));
    HIP_TRY(c, c->ps_res.ensure(PS_WORDS * 8));
    HIP_TRY(c, c->h_wc.ensure(CR_WORDS * 8));
    DevPart d;
    memset(&d, 0, sizeof(d));
    d.stream = in->stream;
    d.n = in->stream_bytes;
    d.n_cand = d.n - 35;
    d.tile = PART_TILE;
    d.n_tiles = (d.n_cand + d.tile - 1) / d.tile;
    d.n_ref = in->n_ref;
    d.final = in->final ? 1 : 0;
    d.res = c->ps_res.as<unsigned long long>();
    unsigned long long *h = c->h_wc.as<unsigned long long>();
    const uint32_t waves = (uint32_t)std::min<unsigned long long>(d.n_tiles, (unsigned long long)std::max(1, c->n_cus) * 8ull);
    HIP_TRY(c, hipEventRecord(c->wev[0], st));
    HIP_TRY(c, hipMemsetAsync(d.res, 0xff, 2 * 8, st));
    HIP_TRY(c, hipMemsetAsync(d.res + PS_TICKET, 0, 8, st));
    hipLaunchKernelGGL(k_part_start, dim3((waves + 3) / 4), dim3(256), 0, st, d);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->wev[1], st));
    HIP_TRY(c, hipMemcpyAsync(h, d.res, 2 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&out->start_ms, c->wev[0], c->wev[1]);
    const unsigned long long acc = h[PS_ACCEPT], cut = h[PS_CUT];
    if ((acc != CUT_NONE && acc >= d.n_cand) || (cut != CUT_NONE && cut >= d.n_cand)) {
        c->err = "plo_part_start_dev: a candidate outside the stretch (internal)";
        return PLO_ERR_INTERNAL;
    }
    if (acc < cut) {
        out->kind = PLO_PART_FOUND;
        out->first_off = acc;
    } else if (cut != CUT_NONE) {
        out->kind = PLO_PART_NEED_MORE;
    }
    return PLO_OK;
}

plo_status plo_host_alloc(size_t bytes, void **out) {
    if (!out) return PLO_ERR_INVALID_ARG;
    *out = nullptr;
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable);
    if (e == hipErrorNoDevice || e == hipErrorInsufficientDriver) return PLO_ERR_NO_DEVICE;
    if (e != hipSuccess) return e == hipErrorOutOfMemory ? PLO_ERR_OUT_OF_MEMORY : PLO_ERR_HIP;
    *out = p;
    return PLO_OK;
}
void plo_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

plo_status plo_ctx_timing(plo_ctx *c, plo_timing *t) {
    if (!c || !t) return PLO_ERR_INVALID_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float a = 0, l = 0, b = 0, r = 0, g = 0, md = 0;
    if (!c->fast_no_events) {  // (a one-round-trip call on a context with plo_ctx_set_phase_events(ctx, 0) recorded nothing: counts only)
        (void)hipEventElapsedTime(&a, c->ev[0], c->ev[1]);
        (void)hipEventElapsedTime(&l, c->ev[1], c->ev[4]);
    }
    if (!c->fast_timing) {  // (liftover_fast records events 0, 1 and 4 only: its retry launch and the counters' sum are not timed)
        (void)hipEventElapsedTime(&b, c->ev[4], c->ev[2]);
        (void)hipEventElapsedTime(&r, c->ev[2], c->ev[5]);
    }
    if (c->ev_mid) (void)hipEventElapsedTime(&md, c->ev[5], c->ev[6]);
    if (c->ev_big) (void)hipEventElapsedTime(&g, c->ev_mid ? c->ev[6] : c->ev[5], c->ev[3]);
    c->timing.enumerate_ms = a;
    c->timing.lanes_ms = l;
    c->timing.lift_ms = c->timing.n_heavy_lane_items ? 0.0f : b;
    c->timing.heavy_lanes_ms = c->timing.n_heavy_lane_items ? b : 0.0f;
    c->timing.retry_ms = r;
    c->timing.mid_ms = md;
    c->timing.big_ms = g;
    c->timing.total_ms = a + l + b + r + md + g;
    // the caller says how much of the struct it knows (API version 4): never write past that
    const uint32_t have = t->struct_size;
    if (have < 8u || have > (1u << 16)) {
        c->err = "plo_ctx_timing: plo_timing::struct_size must be set to sizeof(plo_timing) by the caller";
        return PLO_ERR_INVALID_ARG;
    }
    const uint32_t n = std::min<uint32_t>(have, (uint32_t)sizeof(plo_timing));
    c->timing.struct_size = n;
    memcpy(t, &c->timing, n);
    return PLO_OK;
}

plo_status plo_liftover_batch(plo_ctx *c, const plo_batch_in *in, uint32_t stages, plo_batch_out *out) {
    if (!c || !in || !out) return PLO_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    c->err.clear();
    HIP_TRY(c, hipSetDevice(c->ix->device));
    hipStream_t st = c->stream;
    uint32_t nr = in->n_reads, ns = in->n_segs;
    // NULL arrays are refused here; everything else about the batch (index ranges, 31-bit coordinates, op codes) is checked on
    // the device by the enumerate kernels of plo_liftover_batch_dev
    if (ns && (!in->seg_read || !in->seg_contig || !in->seg_pos || !in->seg_is_fwd_strand || !in->seg_cigar_off) ) {
        c->err = "plo_batch_in: NULL segment array";
        return PLO_ERR_INVALID_ARG;
    }
    if (nr && (!in->read_is_reverse || !in->read_seq_len || !in->read_seq_off)) {
        c->err = "plo_batch_in: NULL read array";
        return PLO_ERR_INVALID_ARG;
    }
    if (in->item_seg && !in->item_cseg) {
        c->err = "plo_batch_in: item_seg without item_cseg";
        return PLO_ERR_INVALID_ARG;
    }
    uint32_t n_cigar = ns ? in->seg_cigar_off[ns] : 0;
    if ((n_cigar && !in->cigar) || (in->seq_bytes && !in->seq)) {
        c->err = "plo_batch_in: NULL cigar / seq array";
        return PLO_ERR_INVALID_ARG;
    }
    if (n_cigar > 0x7fffffffu) {
        c->err = "plo_batch_in: more than 2^31 - 1 CIGAR ops in one batch; split the batch";
        return PLO_ERR_RANGE;
    }
#define UP(buf, src, bytes)                                                                          \
    do {                                                                                             \
        HIP_TRY(c, (buf).ensure(std::max<size_t>((bytes), 16)));                                     \
        if ((bytes) > 0) HIP_TRY(c, hipMemcpyAsync((buf).p, (src), (bytes), hipMemcpyHostToDevice, st)); \
    } while (0)
    UP(c->i_read_rev, in->read_is_reverse, (size_t)nr);
    UP(c->i_read_len, in->read_seq_len, (size_t)nr * 4);
    UP(c->i_read_off, in->read_seq_off, (size_t)nr * 8);
    UP(c->i_seg_read, in->seg_read, (size_t)ns * 4);
    UP(c->i_seg_contig, in->seg_contig, (size_t)ns * 4);
    UP(c->i_seg_pos, in->seg_pos, (size_t)ns * 8);
    UP(c->i_seg_fwd, in->seg_is_fwd_strand, (size_t)ns);
    HIP_TRY(c, c->i_seg_coff.ensure((size_t)(ns + 1) * 4));
    if (ns) {
        HIP_TRY(c, hipMemcpyAsync(c->i_seg_coff.p, in->seg_cigar_off, (size_t)(ns + 1) * 4, hipMemcpyHostToDevice, st));
    } else {
        HIP_TRY(c, hipMemsetAsync(c->i_seg_coff.p, 0, 4, st));
    }
    UP(c->i_cigar, in->cigar, (size_t)n_cigar * 4);
    {   // the bases last, on the copy stream (the buffers are idle: the previous call on this context has been waited for)
        if (!c->copy_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        if (!c->ev_seq) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_seq, hipEventDisableTiming));
        HIP_TRY(c, c->i_seq.ensure(std::max<size_t>((size_t)in->seq_bytes, 16)));
        if (in->seq_bytes) {
            HIP_TRY(c, hipMemcpyAsync(c->i_seq.p, in->seq, (size_t)in->seq_bytes, hipMemcpyHostToDevice, c->copy_stream));
            HIP_TRY(c, hipEventRecord(c->ev_seq, c->copy_stream));
            c->seq_pending = true;
        }
    }
    plo_batch_in din = *in;
    din.read_is_reverse = c->i_read_rev.as<uint8_t>();
    din.read_seq_len = c->i_read_len.as<uint32_t>();
    din.read_seq_off = c->i_read_off.as<uint64_t>();
    din.seq = c->i_seq.as<uint8_t>();
    din.seg_read = c->i_seg_read.as<uint32_t>();
    din.seg_contig = c->i_seg_contig.as<uint32_t>();
    din.seg_pos = c->i_seg_pos.as<int64_t>();
    din.seg_is_fwd_strand = c->i_seg_fwd.as<uint8_t>();
    din.seg_cigar_off = c->i_seg_coff.as<uint32_t>();
    din.cigar = c->i_cigar.as<uint32_t>();
    if (in->item_seg) {
        UP(c->i_item_seg, in->item_seg, (size_t)in->n_items * 4);
        UP(c->i_item_cseg, in->item_cseg, (size_t)in->n_items * 4);
        din.item_seg = c->i_item_seg.as<uint32_t>();
        din.item_cseg = c->i_item_cseg.as<uint32_t>();
    }
#undef UP
    plo_batch_out dout;
    plo_status s = plo_liftover_batch_dev(c, &din, stages, &dout);
    if (c->seq_pending) {  // no lift kernel waited for the bases (an error, or a batch without items): the caller's buffer is still being read
        (void)hipStreamSynchronize(c->copy_stream);
        c->seq_pending = false;
    }
    if (s != PLO_OK) return s;
    s = plo_compact_output_dev(c, &dout);  // no slab gaps over the bus
    if (s != PLO_OK) return s;
    size_t ni = dout.n_items, nc = (size_t)dout.n_cigar;
#define DOWN(hbuf, src, bytes)                                                                        \
    do {                                                                                              \
        HIP_TRY(c, (hbuf).ensure(std::max<size_t>((bytes), 16)));                                     \
        if ((bytes) > 0) HIP_TRY(c, hipMemcpyAsync((hbuf).p, (src), (bytes), hipMemcpyDeviceToHost, st)); \
    } while (0)
    DOWN(c->h_item_seg, dout.item_seg, ni * 4);
    DOWN(c->h_item_cseg, dout.item_cseg, ni * 4);
    DOWN(c->h_status, dout.item_status, ni);
    DOWN(c->h_flip, dout.item_need_flipped, ni);
    DOWN(c->h_mapq, dout.item_mapq, ni);
    DOWN(c->h_chrom, dout.item_chrom_index, ni * 4);
    DOWN(c->h_pos, dout.item_ref_pos, ni * 8);
    DOWN(c->h_coff, dout.item_cigar_off, ni * 8);
    DOWN(c->h_clen, dout.item_cigar_len, ni * 4);
    DOWN(c->h_cigar, dout.cigar, nc * 4);
#undef DOWN
    HIP_TRY(c, hipStreamSynchronize(st));
    out->n_items = dout.n_items;
    out->item_seg = c->h_item_seg.as<uint32_t>();
    out->item_cseg = c->h_item_cseg.as<uint32_t>();
    out->item_status = c->h_status.as<uint8_t>();
    out->item_need_flipped = c->h_flip.as<uint8_t>();
    out->item_mapq = c->h_mapq.as<uint8_t>();
    out->item_chrom_index = c->h_chrom.as<uint32_t>();
    out->item_ref_pos = c->h_pos.as<int64_t>();
    out->item_cigar_off = c->h_coff.as<uint64_t>();
    out->item_cigar_len = c->h_clen.as<uint32_t>();
    out->cigar = c->h_cigar.as<uint32_t>();
    out->n_cigar = dout.n_cigar;
    return PLO_OK;
}


// Runs the wave primitives on the device and checks them against host-computed expectations.
// 0 = ok, >0 = index of the first failing primitive + 1, <0 = HIP error.
int plo_selftest(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -1;
    if (hipSetDevice(device) != hipSuccess) return -1;
    std::vector<int> in(256), out(14 * 64, 0), exp(14 * 64, 0);
    unsigned rs = 12345u;
    auto rnd = [&]() {
        rs = rs * 1664525u + 1013904223u;
        return (int)(rs >> 8);
    };
    for (int l = 0; l < 64; ++l) {
        in[l] = rnd() % 1000 - 300;
        in[64 + l] = rnd() % 50;
        in[128 + l] = (rnd() % 4 == 0) ? 0x7fffffff : rnd() % 80;
        in[192 + l] = (rnd() % 9 == 0) ? 1 : 0;
    }
    int acc = 0, mx = (int)0x80000000;
    int fa = 0, fb = 0x7fffffff, fs = 0;
    int c0 = 0, c1 = 0, lm = -1;
    for (int l = 0; l < 64; ++l) c1 += in[l] & 15;
    for (int l = 0; l < 64; ++l) {
        int x = in[l];
        acc += x;
        mx = std::max(mx, x);
        exp[0 * 64 + l] = acc;
        exp[1 * 64 + l] = mx;
        exp[2 * 64 + l] = l ? in[l - 1] : -7;
        exp[3 * 64 + l] = in[(l * 7 + 3) & 63];
        exp[4 * 64 + l] = in[63];
        exp[5 * 64 + l] = in[0];
        int a = in[64 + l], b = in[128 + l], sflag = in[192 + l];
        if (sflag) {
            fa = a;
            fb = b;
            fs = 1;
        } else {
            long long na = (long long)fa + a, nb = (long long)fb + a;
            fa = na > 0x7fffffffLL ? 0x7fffffff : (int)na;
            int nbb = nb > 0x7fffffffLL ? 0x7fffffff : (int)nb;
            fb = std::min(nbb, b);
        }
        exp[6 * 64 + l] = fa;
        exp[7 * 64 + l] = fb;
        exp[8 * 64 + l] = fs;
        exp[9 * 64 + l] = x & 1;
        exp[10 * 64 + l] = c0;
        c0 += x & 15;
        exp[11 * 64 + l] = c1;
        c1 += (x >> 4) & 15;
        exp[12 * 64 + l] = lm;
        if ((x & 3) == 0) lm = l;
    }
    int lm2 = lm;
    for (int l = 0; l < 64; ++l) {
        exp[13 * 64 + l] = lm2;
        if ((in[l] & 3) == 1) lm2 = std::max(lm2, 64 + l);
    }
    int *din = nullptr, *dout = nullptr;
    if (hipMalloc(&din, in.size() * 4) != hipSuccess || hipMalloc(&dout, out.size() * 4) != hipSuccess) return -2;
    if (hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return -3;
    hipLaunchKernelGGL(k_selftest, dim3(1), dim3(64), 0, 0, (const int *)din, dout);
    if (hipDeviceSynchronize() != hipSuccess) return -4;
    if (hipMemcpy(out.data(), dout, out.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return -5;
    (void)hipFree(din);
    (void)hipFree(dout);
    for (int k = 0; k < 14; ++k)
        for (int l = 0; l < 64; ++l)
            if (out[k * 64 + l] != exp[k * 64 + l]) {
                fprintf(stderr, "plo_selftest: primitive %d lane %d got %d expected %d\n", k, l, out[k * 64 + l], exp[k * 64 + l]);
                return k + 1;
            }
    return 0;
}

}  // extern "C"
