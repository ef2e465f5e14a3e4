"""A plain restatement of record finishing and of the SA:Z text, in Python and numpy, written from the Rust text and independent of oracle/.

Sources: src/read_alignment_scanner.rs:245-284 (one lifted record: flag, alignment end, bin, supplementary bit), :292-301 (one SA segment),
:310-366 (the read's set: unmapped copy, primary choice, SA values), :125-133 (reverse_alignment_seq_and_qual), hts_reg2bin of
lib/rust-vc-utils/src/bam_utils/util.rs, comp_base of lib/rust-vc-utils/src/seq_util.rs, and the entry layout of
include/portello_liftover.h (plo_finish_out).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from portello_amd import abi

NO_FLIP = abi.NO_FLIP
NO_ITEM = 0xFFFFFFFF
BAM4_DECODE = "=ACMGRSVTWYHKDBN"  # the BAM specification's 4-bit alphabet
CIGAR_LETTERS = "MIDNSHP=XB"      # op codes 0..9; the lift writes no others
REF_OPS = (0, 2, 3, 7, 8)         # M D N = X advance the reference (get_alignment_end)


def comp_base(x: int) -> int:
    """seq_util.rs comp_base on one byte"""
    table = {"A": "T", "T": "A", "C": "G", "G": "C", "N": "N", "a": "t", "t": "a", "c": "g", "g": "c", "n": "n"}
    return ord(table.get(chr(x), "N"))


COMP_ASCII = np.array([comp_base(x) for x in range(256)], np.uint8)
# record.seq().as_bytes() decodes, comp_base complements, record.set() encodes again
COMP_BAM4 = np.array([BAM4_DECODE.index(chr(comp_base(ord(ch)))) for ch in BAM4_DECODE], np.uint8)


def reg2bin(beg: int, end: int) -> int:
    """SAM specification 5.3 (reg2bin) over Python ints.  end == beg is taken as the specification's C code takes it: end - 1 lies in front
    of beg, so the two share a bin only above the 16 kb level, and with beg == 0 (end - 1 == -1) at no level: bin 0"""
    end -= 1
    if beg >> 14 == end >> 14: return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17: return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20: return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23: return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26: return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def ref_end(pos: int, ops) -> int:
    return int(pos) + sum(c >> 4 for c in np.asarray(ops, np.uint32).tolist() if (c & 15) in REF_OPS)


def item_flag(read_flag: int, flipped: bool, primary: bool) -> int:
    f = int(read_flag)
    if flipped:
        f ^= 0x10
    f |= 0x800
    if primary:
        f &= ~0x800
    return f & 0xFFFF


def unmapped_flag(read_flag: int):
    """-> (flag of the unmapped copy, whether its bases and qualities are reversed)"""
    f = (int(read_flag) | 0x4) & ~0x800
    rev = bool(f & 0x10)
    if rev:
        f ^= 0x10
    return f & 0xFFFF, rev


def units16(nbytes: int) -> int:
    return (nbytes + 15) // 16


def seq_bytes_of(seq_fmt: int, L: int) -> int:
    return (L + 1) // 2 if seq_fmt == abi.SEQ_BAM4 else L


def revcomp_bam4(packed: np.ndarray, L: int) -> np.ndarray:
    """(L + 1) // 2 bytes: the reverse complement of the L bases in `packed`; the low nibble behind an odd read is 0 here"""
    p = np.asarray(packed, np.uint8)[:(L + 1) // 2]
    nib = np.empty(2 * len(p), np.uint8)
    nib[0::2] = p >> 4
    nib[1::2] = p & 15
    out = np.zeros(2 * len(p), np.uint8)
    out[:L] = COMP_BAM4[nib[:L]][::-1]
    return ((out[0::2] << 4) | out[1::2]).astype(np.uint8)


def revcomp_ascii(seq: np.ndarray, L: int) -> np.ndarray:
    return COMP_ASCII[np.asarray(seq, np.uint8)[:L]][::-1].copy()


def finish(batch: abi.BatchData, read_flags, qual, read_qual_off, lift: abi.BatchResult) -> dict:
    """every field of a plo_finish_out (the keys of abi.FINISH_ITEM_FIELDS / FINISH_READ_FIELDS), "rev_seq_bytes" / "rev_qual_bytes", "n_fault",
    "item_read" and "entries": for every flipped entry (is_item, index, read, seq_off, qual_off, reversed bases, reversed qualities).
    Fields of an item that is not lifted, and the unmapped flag of a read that has a lifted item, are 0 / NO_FLIP."""
    n, nr = lift.n_items, batch.n_reads
    fmt = batch.seq_fmt
    read_flags = np.asarray(read_flags).astype(np.uint16)
    item_read = np.asarray(batch.seg_read, np.int64)[np.asarray(lift.item_seg, np.int64)] if n else np.zeros(0, np.int64)
    lifted = [int(lift.item_status[i]) == abi.ITEM_LIFTED for i in range(n)]
    res = {name: np.zeros(n, dt) for name, dt in abi.FINISH_ITEM_FIELDS}
    res.update({name: np.zeros(nr, dt) for name, dt in abi.FINISH_READ_FIELDS})
    res["item_read"] = item_read
    res["seq_fmt"] = fmt
    res["n_fault"] = sum(1 for i in range(n) if int(lift.item_status[i]) in (abi.ITEM_LEN_MISMATCH, abi.ITEM_PANIC, abi.ITEM_NEED_BASES))
    by_read = [[] for _ in range(nr)]
    for i in range(n):
        if lifted[i]:
            by_read[int(item_read[i])].append(i)
    primary = [NO_ITEM] * nr
    for r, its in enumerate(by_read):
        res["read_n_lifted"][r] = len(its)
        if its:
            best = its[0]
            for i in its[1:]:
                if int(lift.item_mapq[best]) < int(lift.item_mapq[i]):
                    best = i
            primary[r] = best
        res["read_primary_item"][r] = primary[r]
    flip_entry = [False] * (n + nr)  # items first, then reads
    for i in range(n):
        if not lifted[i]:
            continue
        r = int(item_read[i])
        flipped = bool(lift.item_need_flipped[i])
        res["item_flag"][i] = item_flag(read_flags[r], flipped, primary[r] == i)
        res["item_is_primary"][i] = 1 if primary[r] == i else 0
        pos = int(lift.item_ref_pos[i])
        end = ref_end(pos, lift.item_cigar(i))
        res["item_ref_end"][i] = end
        res["item_bin"][i] = reg2bin(pos, end) & 0xFFFF  # (bam_reg2bin: `as u16`)
        flip_entry[i] = flipped
    for r in range(nr):
        if not by_read[r]:
            res["read_unmapped_flag"][r], flip_entry[n + r] = unmapped_flag(read_flags[r])
    so = qo = 0
    entries = []
    seq, qual = np.asarray(batch.seq, np.uint8), np.asarray(qual, np.uint8)
    for k in range(n + nr):
        is_item = k < n
        idx = k if is_item else k - n
        names = ("item_seq_off", "item_qual_off") if is_item else ("read_seq_off", "read_qual_off")
        if not flip_entry[k]:
            res[names[0]][idx] = res[names[1]][idx] = NO_FLIP
            continue
        r = int(item_read[k]) if is_item else idx
        L = int(batch.read_seq_len[r])
        su, qu = units16(seq_bytes_of(fmt, L)), units16(L)
        if su == 0:  # a read without bases has nothing to reverse: no slot
            res[names[0]][idx] = res[names[1]][idx] = NO_FLIP
            continue
        res[names[0]][idx], res[names[1]][idx] = so * 16, qo * 16
        b0, q0 = int(batch.read_seq_off[r]), int(read_qual_off[r])
        rs = revcomp_bam4(seq[b0:], L) if fmt == abi.SEQ_BAM4 else revcomp_ascii(seq[b0:], L)
        rq = qual[q0:q0 + L][::-1].copy()
        entries.append((is_item, idx, r, so * 16, qo * 16, rs, rq))
        so += su
        qo += qu
    res["rev_seq_bytes"], res["rev_qual_bytes"] = so * 16, qo * 16
    res["entries"] = entries
    return res


def cigar_text(ops) -> bytes:
    return "".join("%d%s" % (int(c) >> 4, CIGAR_LETTERS[int(c) & 15]) for c in ops).encode()


def sa_segment(chrom_name: bytes, pos: int, flag: int, ops, mapq: int) -> bytes:
    """get_sa_tag_segment: the strand is the record's reverse bit, i.e. of the flag behind the flip"""
    return b"%s,%d,%s,%s,%d,0;" % (chrom_name, pos + 1, b"-" if flag & 0x10 else b"+", cigar_text(ops), mapq)


def sa_values(batch: abi.BatchData, lift: abi.BatchResult, item_flags, chrom_names) -> list:
    """the SA:Z value of every item (None: no tag): the segments of the read's other lifted records in record order"""
    n = lift.n_items
    names = [c.encode() if isinstance(c, str) else bytes(c) for c in chrom_names]
    item_read = np.asarray(batch.seg_read, np.int64)[np.asarray(lift.item_seg, np.int64)] if n else []
    seg = {}
    for i in range(n):
        if int(lift.item_status[i]) == abi.ITEM_LIFTED:
            seg[i] = sa_segment(names[int(lift.item_chrom_index[i])], int(lift.item_ref_pos[i]), int(item_flags[i]), lift.item_cigar(i), int(lift.item_mapq[i]))
    out = [None] * n
    for i in seg:
        others = [j for j in seg if j != i and item_read[j] == item_read[i]]
        if others:
            out[i] = b"".join(seg[j] for j in sorted(others))
    return out


def compare(got: dict, exp: dict, who: str = ""):
    """`got` (emu_lib.finish_batch, oracle.finish_batch, a download of plo_finish_out, the sanitizer program) against finish(): every field
    of the lifted items and of all reads, the totals, and the meaningful bytes of every flipped entry -> the number of entries compared"""
    for name, _ in abi.FINISH_ITEM_FIELDS:
        a, e = np.asarray(got[name]), exp[name]
        assert len(a) == len(e), (who, name)
        bad = np.nonzero(a != e)[0]
        assert not len(bad), (who, name, int(bad[0]), a[bad[0]], e[bad[0]])
    for name, _ in abi.FINISH_READ_FIELDS:
        a, e = np.asarray(got[name]), exp[name]
        assert len(a) == len(e), (who, name)
        bad = np.nonzero(a != e)[0]
        assert not len(bad), (who, name, int(bad[0]), a[bad[0]], e[bad[0]])
    assert len(got["rev_seq"]) == exp["rev_seq_bytes"] and len(got["rev_qual"]) == exp["rev_qual_bytes"], (who, len(got["rev_seq"]), len(got["rev_qual"]))
    if "n_fault" in got:
        assert got["n_fault"] == exp["n_fault"], (who, got["n_fault"], exp["n_fault"])
    for is_item, idx, r, so, qo, rs, rq in exp["entries"]:
        L = len(rq)
        gq = got["rev_qual"][qo:qo + L]
        assert np.array_equal(gq, rq), (who, "qual", is_item, idx, r, L, int(np.nonzero(gq != rq)[0][0]))
        gs = np.array(got["rev_seq"][so:so + len(rs)])
        if exp["seq_fmt"] == abi.SEQ_BAM4 and L & 1:  # the low nibble behind the last base of an odd read is not compared
            gs[-1] &= 0xF0
        assert np.array_equal(gs, rs), (who, "seq", is_item, idx, r, L, int(np.nonzero(gs != rs)[0][0]))
    return len(exp["entries"])
