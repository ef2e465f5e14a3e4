"""Output BAM records assembled on the device (plo_records_build_dev, portello_amd/csrc/records_core.hpp).

The yardstick is always plo_records_build on the same window and the same lift result (itself held to oracle/pyrecords.py by
tests/test_bam.py): equality of record_off, of every record's bytes and of the counts.  The CPU tests run records_core.hpp under the
wave emulator (tests/emu/emu_records.cpp) on lift results of the C oracle or hand-made ones; the GPU tests run the C ABI on the device
and the pipeline mode."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import emu_records_lib as erl
from portello_amd import abi, api, bam, bamsynth, synth
from portello_amd import cigar as cg


def _arr(ptr, dtype, count):
    if not count:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype).copy()


class RawWindow:
    """numpy copies of what bam.Window.batch_raw() describes"""

    def __init__(self, win):
        b, f, r = win.batch_raw()
        n, ns = int(b.n_reads), int(b.n_segs)
        self.n = n
        self.raw = _arr(r.raw, np.uint8, int(r.raw_bytes))
        self.rec_off = _arr(r.read_rec_off, np.uint64, n)
        self.seq_off = _arr(b.read_seq_off, np.uint64, n)
        self.qual_off = _arr(f.read_qual_off, np.uint64, n)
        self.flags = _arr(f.read_flags, np.uint16, n)
        assert int(b.seq_bytes) == int(f.qual_bytes) == len(self.raw) and int(b.seq_fmt) == abi.SEQ_BAM4
        assert C.cast(b.seq, C.c_void_p).value == C.cast(r.raw, C.c_void_p).value == C.cast(f.qual, C.c_void_p).value  # views, no copies
        coff = _arr(b.seg_cigar_off, np.uint32, ns + 1) if ns else np.zeros(1, np.uint32)
        self.batch = abi.BatchData(read_is_reverse=_arr(b.read_is_reverse, np.uint8, n), read_seq_len=_arr(b.read_seq_len, np.uint32, n),
                                   read_seq_off=self.seq_off, seq=self.raw, seq_fmt=abi.SEQ_BAM4, seg_read=_arr(b.seg_read, np.uint32, ns),
                                   seg_contig=_arr(b.seg_contig, np.uint32, ns), seg_pos=_arr(b.seg_pos, np.int64, ns),
                                   seg_is_fwd_strand=_arr(b.seg_is_fwd_strand, np.uint8, ns), seg_cigar_off=coff, cigar=_arr(b.cigar, np.uint32, int(coff[-1])))
        # the offsets point at the records' own fields
        for i in range(n):
            o = int(self.rec_off[i]) + 4
            lq, ncg, lseq = int(self.raw[o + 8]), struct.unpack_from("<H", self.raw, o + 12)[0], struct.unpack_from("<I", self.raw, o + 16)[0]
            assert int(self.seq_off[i]) == o + 32 + lq + 4 * ncg and int(self.qual_off[i]) == int(self.seq_off[i]) + (lseq + 1) // 2


def _split(data, off):
    return [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def host_records(win, ix, lift, cn, rn, target):
    o, keep = abi.out_from_result(lift)
    data, off, nl, nu = win.build_records(o, ix.to_desc(), cn, rn, is_target_region=target, n_threads=3)
    return data, np.asarray(off, np.uint64), nl, nu


def check_emulated(win, ix, lift, cn, rn, target, vec=True, nthreads=7, order_seed=0):
    """records_core.hpp under the emulator against plo_records_build: -> (host records, finish arrays)"""
    rw = RawWindow(win)
    st, data, off, nl, nu, err, f, sa_off = erl.records_build(ix, rw.batch, rw.flags, rw.raw, rw.rec_off, rw.seq_off, rw.qual_off, lift, cn, rn, target, vec,
                                                               nthreads, order_seed)
    assert st == 0 and err == [0, 0, 0, 0]
    hdata, hoff, hnl, hnu = host_records(win, ix, lift, cn, rn, target)
    want, got = _split(hdata, hoff), _split(data, off)
    assert len(got) == len(want)
    if len(want):
        assert np.array_equal(off, hoff)
    for i, (a, e) in enumerate(zip(got, want)):
        assert a == e, (i, vec, a[:80], e[:80])
    assert data == hdata and (nl, nu) == (hnl, hnu)
    return want, f, sa_off


def open_window(path, max_records=100_000):
    rd = bam.BamReader(path, 2)
    return rd, rd.read_window(max_records)


# ---- 1. the small_bam recipe of tests/test_bam.py -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("recdev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=411, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


def _aux_tag_order(rec: bytes):
    """tags of a record's aux fields in order (well-formed records only)"""
    lq, ncg, lseq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    a = 36 + lq + 4 * ncg + (lseq + 1) // 2 + lseq
    tags = []
    while a < len(rec):
        tag, t = rec[a:a + 2], chr(rec[a + 2])
        tags.append((tag, t))
        if t in "AcC":
            a += 4
        elif t in "sS":
            a += 5
        elif t in "iIf":
            a += 7
        elif t in "ZH":
            a = rec.index(b"\0", a + 3) + 1
        elif t == "B":
            es = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[chr(rec[a + 3])]
            a += 8 + es * struct.unpack_from("<I", rec, a + 4)[0]
        else:
            raise AssertionError(t)
    return tags


@pytest.mark.parametrize("is_target_region", [False, True])
def test_sample_records_equal_the_host_builder(small_bam, oracle, is_target_region):
    w, path, meta = small_bam
    ix = w.index_data()
    rd, win = open_window(path)
    lift = oracle.liftover_batch(ix, win.batch_data(), abi.STAGES_ALL, 2)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    want, f, sa_off = check_emulated(win, ix, lift, cn, rn, is_target_region)
    check_emulated(win, ix, lift, cn, rn, is_target_region, vec=False, nthreads=3, order_seed=9)  # the byte-copy instantiation, shuffled lanes
    # the sample is not vacuous
    rw = RawWindow(win)
    lifted = lift.item_status == abi.ITEM_LIFTED
    assert (f["item_seq_off"][lifted] != abi.NO_FLIP).any(), "no flipped record"
    assert (f["read_n_lifted"] >= 2).any() and int(sa_off[-1]) > 0, "no read with two lifted records"
    assert (f["read_n_lifted"] == 0).any(), "no read without a lifted record"
    if not is_target_region:
        assert sum(1 for r in want if struct.unpack_from("<H", r, 18)[0] & 4) == int((f["read_n_lifted"] == 0).sum()) > 0
    src = [bytes(rw.raw[int(o):int(o) + 4 + struct.unpack_from("<I", rw.raw, int(o))[0]]) for o in rw.rec_off]
    orders = set()
    for r in src:
        tags = _aux_tag_order(r)
        orders.add(tuple(t for t, _ in tags if t in (b"PS", b"ZM", b"SA", b"NM")))
    assert len(orders) > 1 and any(b"PS" in o for o in orders) and any(b"ZM" in o for o in orders) and any(b"SA" in o for o in orders), orders
    assert any(t == "B" for r in src for _, t in _aux_tag_order(r)), "no B array field"
    win.close()
    rd.close()


# ---- 2. hand-made records ---------------------------------------------------------------------------------------------------------------

CN, RN = ["ctg0"], ["chr1", "chr2"]


def hand_index():
    """one contig with two segments: segment 0 forward on chr1, segment 1 reverse on chr2 (as test_hand_checked_record)"""
    return abi.IndexData(contig_len=np.array([500000]), contig_seg_off=np.array([0, 2], np.uint32), seg_chrom_index=np.array([0, 1], np.uint32),
                         seg_pos=np.array([0, 0]), seg_is_fwd_strand=np.array([1, 0], np.uint8), seg_mapq=np.array([50, 20], np.uint8),
                         seg_seq_order_start=np.array([0, 250000]), seg_seq_order_end=np.array([250000, 500000]), seg_cigar_off=np.array([0, 1, 2], np.uint32),
                         seg_cigar=np.array(list(cg.encode("250000M")) * 2, np.uint32), chrom_seq=[np.zeros(4000, np.uint8)] * 2, rev_contig_seq=[None])


def make_record(k, l_seq, flag=0, qname=None, aux=b"", cigar=None, seed=0):
    rng = np.random.default_rng(1000 + k + seed)
    sp = rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8)
    sp = ((sp & 0x77) | 0x11).astype(np.uint8)  # (a mix of one-hot and other codes)
    if l_seq & 1 and l_seq:
        sp[-1] &= 0xF0
    qual = rng.integers(0, 94, l_seq, dtype=np.uint8).tobytes()
    cigar = np.array(cg.encode(f"{l_seq}M") if l_seq else [], np.uint32) if cigar is None else cigar
    return bamsynth.encode_record(0, 10 + k, 37, flag, qname if qname is not None else b"r%d" % k, cigar, sp.tobytes(), l_seq, qual, aux)


def write_window(tmp_path, recs, name="hand.bam"):
    path = str(tmp_path / name)
    wr = bam.BamWriter(path, "@HD\tVN:1.6\n", CN, [500000], level=1)
    wr.write(b"".join(recs))
    wr.close()
    return open_window(path)


def hand_lift(items):
    """items: (read segment, contig segment, status, flip, mapq, chrom, pos, cigar ops) in item order"""
    cigs = [np.asarray(it[7], np.uint32) for it in items]
    lens = np.array([len(c) for c in cigs], np.uint32)
    off = np.zeros(len(items), np.uint64)
    if len(items):
        off[1:] = np.cumsum(lens[:-1])
    col = lambda j, dt: np.array([it[j] for it in items], dt)
    return abi.BatchResult(item_seg=col(0, np.uint32), item_cseg=col(1, np.uint32), item_status=col(2, np.uint8), item_need_flipped=col(3, np.uint8),
                           item_mapq=col(4, np.uint8), item_chrom_index=col(5, np.uint32), item_ref_pos=col(6, np.int64), item_cigar_off=off,
                           item_cigar_len=lens, cigar=np.concatenate(cigs) if cigs else np.zeros(0, np.uint32))


def simple_items(n_reads, l_seqs, flip=None, second=None):
    """one lifted item per read (contig segment 0), a second one (contig segment 1, flipped) for the reads in `second`"""
    items = []
    for r in range(n_reads):
        c = cg.encode(f"{l_seqs[r]}M") if l_seqs[r] else cg.encode("1D")
        items.append((r, 0, abi.ITEM_LIFTED, 1 if (flip and r in flip) else 0, 50, 0, 1000 + r, c))
        if second and r in second:
            items.append((r, 1, abi.ITEM_LIFTED, 1, 20, 1, 500 + r, c))
    return hand_lift(items)


def long_cigar(n):
    c = np.empty(n, np.uint32)
    c[0::2] = (1 << 4) | 0
    c[1::2] = (1 << 4) | 1
    c[-1] = (1 << 4) | 0
    return c


def test_more_than_65535_cigar_ops(tmp_path):
    """output: placeholder + CG:B,I last; a source record itself stored with the placeholder and a CG tag, which is cut"""
    from oracle import pyrecords as pr

    n = 70_001
    cig = long_cigar(n)
    l_seq = n
    src = pr.Record(0, 10, 60, 0, 0, -1, -1, 0, b"long", [int(x) for x in cig], bytes((l_seq + 1) // 2), l_seq, bytes(l_seq),
                    [(b"rq", b"f" + struct.pack("<f", 1.0)), (b"NM", b"C\x07")])
    rb = src.to_bytes()
    assert struct.unpack_from("<H", rb, 16)[0] == 2 and b"CGBI" in rb  # placeholder and CG tag on disk
    rd, win = write_window(tmp_path, [rb, make_record(1, 33, aux=b"XXZkeep\0")])
    assert win.n_records == 2
    # read 0: the long CIGAR on both of its two records (SA text of 70 001 ops too); read 1: a short record beside it
    lift = hand_lift([(0, 0, 0, 0, 50, 0, 77, cig), (0, 1, 0, 1, 20, 1, 99, cig), (1, 0, 0, 0, 50, 0, 5, cg.encode("33M"))])
    want, f, _ = check_emulated(win, hand_index(), lift, CN, RN, False)
    check_emulated(win, hand_index(), lift, CN, RN, False, vec=False)
    assert struct.unpack_from("<H", want[0], 16)[0] == 2 and want[0].count(b"CGBI") == 1 and want[0].endswith(cig.astype("<u4").tobytes())
    win.close()
    rd.close()


def test_a_tag_that_occurs_twice_keeps_its_second_field(tmp_path):
    aux = b"NMC\x01" + b"XXZa\0" + b"NMC\x02" + b"PSZold\0" + b"ZMC\x09" + b"PSZsecond\0" + b"SAZctg0,100,+,10S11M,60,0;\0" + b"ZMC\x08"
    rd, win = write_window(tmp_path, [make_record(0, 21, aux=aux, cigar=np.array(cg.encode("10M11S"), np.uint32))])
    want, _, _ = check_emulated(win, hand_index(), simple_items(1, [21]), CN, RN, False)
    assert b"NMC\x02" in want[0] and b"NMC\x01" not in want[0] and b"PSZsecond\0" in want[0] and b"ZMC\x08" in want[0] and b"PSZold" not in want[0]
    win.close()
    rd.close()


MALFORMED = [b"XQ?abc", b"XQZno terminator", b"XQBC" + struct.pack("<I", 1000) + b"\x01\x02", b"XQBC" + struct.pack("<I", 0xffffffff), b"XQBz" + struct.pack("<I", 1), b"XQ",
             b"XQi\x01\x02"]


def malformed_records():
    recs = []
    for k, tail in enumerate(MALFORMED):
        # a cut tag and kept fields before the malformed one; the NM behind it must stay (the walk ends at the malformed field)
        aux = b"rqf" + struct.pack("<f", 0.5) + b"ZMC\x07" + b"XXZ" + b"k" * (3 * k) + b"\0" + b"mlBC" + struct.pack("<I", 5) + bytes(5) + tail
        if k % 2 == 0:
            aux = aux[:-len(tail)] + tail + b"NMC\x05"  # (the tail swallows it or not: either way it is not a field any more)
        recs.append(make_record(k, 40 + k, aux=aux))
    return recs


def test_malformed_aux_tail(tmp_path):
    """unknown type letter, Z without NUL, B count past the end, a field cut short: bytes equal to the host's -- lifted records, unmapped
    copies, and the unmapped copies again from the AddressSanitizer + UBSan build of the emulator (CPU), where every input sits in a heap
    block of its exact size: no read outside the record"""
    recs = malformed_records()
    rd, win = write_window(tmp_path, recs)
    n = len(recs)
    want, _, _ = check_emulated(win, hand_index(), simple_items(n, [40 + k for k in range(n)], second={1, 4}), CN, RN, False)
    assert all(b"ZMC\x07" not in r for r in want) and any(b"NMC\x05" in r for r in want)
    none = hand_lift([])
    want_unm, _, _ = check_emulated(win, hand_index(), none, CN, RN, False)
    assert len(want_unm) == n
    # the same window cut off right behind its last record (the last record's malformed tail is the end of the buffer)
    rw = RawWindow(win)
    end = int(rw.rec_off[-1]) + 4 + struct.unpack_from("<I", rw.raw, int(rw.rec_off[-1]))[0]
    rc, err_text, data, nrec = erl.run_asan(rw.raw[:end].tobytes(), rw.rec_off, str(tmp_path))
    assert rc == 0, err_text[-3000:]
    assert nrec == n and data == b"".join(want_unm)
    win.close()
    rd.close()


def test_sequence_lengths_zero_odd_even_flipped(tmp_path):
    lens = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]
    # (a record without bases, SEQ '*', still needs read bases in its CIGAR to be a split segment at all: split_read.rs:112-151)
    recs = [make_record(k, l, cigar=None if l else np.array(cg.encode("3M"), np.uint32)) for k, l in enumerate(lens)]
    rd, win = write_window(tmp_path, recs)
    n = len(lens)
    # every read: a forward record and a flipped one (reversed bases and qualities from finish_core.hpp's buffers)
    want, f, _ = check_emulated(win, hand_index(), simple_items(n, lens, second=set(range(n))), CN, RN, False)
    assert len(want) == 2 * n and (f["item_seq_off"] != abi.NO_FLIP).sum() == n - 1  # (a read without bases has nothing to flip)
    check_emulated(win, hand_index(), simple_items(n, lens, flip=set(range(n))), CN, RN, False, nthreads=64)
    win.close()
    rd.close()


@pytest.mark.parametrize("l_seq", [70, 301])
def test_bulk_copy_meets_every_alignment_residue(tmp_path, l_seq):
    """l_qname and a leading Z tag padded 0..15 bytes each: source and destination of the bulk copy meet in every residue mod 16"""
    recs, k = [], 0
    for qpad in range(16):
        for zpad in range(16):
            recs.append(make_record(k, l_seq, qname=b"q" * (qpad + 1), aux=b"PSZ" + b"z" * zpad + b"\0" + b"rqf" + struct.pack("<f", 0.25) + b"XYZ" + b"y" * 37 + b"\0"))
            k += 1
    rd, win = write_window(tmp_path, recs)
    n = len(recs)
    check_emulated(win, hand_index(), simple_items(n, [l_seq] * n, second=set(range(0, n, 3))), CN, RN, False)
    win.close()
    rd.close()


@pytest.mark.parametrize("is_target_region", [False, True])
def test_reverse_strand_read_without_a_lifted_record(tmp_path, is_target_region):
    """every item NO_LIFTOVER: the unmapped copy with flipped bases and qualities (:317-335) -- and no record under is_target_region"""
    recs = [make_record(0, 45, flag=0x10, aux=b"NMC\x03XXZkeep\0"), make_record(1, 20, aux=b"XXZkeep\0"), make_record(2, 46, flag=0x10)]
    rd, win = write_window(tmp_path, recs)
    lift = hand_lift([(0, 0, abi.ITEM_NO_LIFTOVER, 0, 0, 0, 0, []), (0, 1, abi.ITEM_NO_LIFTOVER, 0, 0, 0, 0, []), (1, 0, abi.ITEM_LIFTED, 0, 50, 0, 10, cg.encode("20M"))])
    want, f, _ = check_emulated(win, hand_index(), lift, CN, RN, is_target_region)
    assert len(want) == (1 if is_target_region else 3)
    if not is_target_region:
        assert f["read_seq_off"][0] != abi.NO_FLIP and struct.unpack_from("<H", want[0], 18)[0] == 4 and want[0][4:8] == b"\xff" * 4
    win.close()
    rd.close()


# ---- 3. the 64-bit scan -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 512, 513, 60_000])
def test_scan_of_sizes_whose_sum_passes_2_32(n):
    rng = np.random.default_rng(n)
    v = rng.integers(0, 1 << 20, n, dtype=np.uint64) + (np.uint64(1 << 17) if n else np.uint64(0))
    if n >= 512:
        v[::7] += np.uint64(3_000_000_000)  # single values beyond 2^31, the sum far beyond 2^32
    want = np.zeros(n + 1, np.uint64)
    want[1:] = np.cumsum(v, dtype=np.uint64)
    assert n < 512 or int(want[-1]) > 1 << 32
    assert np.array_equal(erl.scan64(v, order_seed=n % 3), want)


# ---- 4. refusals: the bounds checks of the core -------------------------------------------------------------------------------------------

def test_records_outside_the_buffer_are_refused_before_anything_is_written(tmp_path):
    recs = [make_record(k, 30 + k, aux=b"XXZkeep\0") for k in range(4)]
    rd, win = write_window(tmp_path, recs)
    rw = RawWindow(win)
    ix, lift = hand_index(), simple_items(4, [30 + k for k in range(4)])
    f = erl.emu_lib.finish_batch(rw.batch, rw.flags, rw.raw, rw.qual_off, lift)
    sa_off, sa_text, _ = erl.emu_lib.sa_segments(rw.batch, lift, f["item_flag"], f["read_n_lifted"], RN)
    run = lambda raw, rec_off, nbytes=None: erl.records_from_finished(ix, rw.batch, raw, rec_off, lift, f, sa_off, sa_text, CN, records_bytes=nbytes)
    assert run(rw.raw, rw.rec_off)[0] == 0
    # a read_rec_off beyond records_bytes
    off = rw.rec_off.copy()
    off[2] = len(rw.raw) - 2
    st, data, _, _, _, err = run(rw.raw, off)
    assert st == 1 and err == [1, 0, 0, 0] and data == b""
    # a block_size running past the end: the buffer cut inside the last record
    st, data, _, _, _, err = run(rw.raw, rw.rec_off, nbytes=int(rw.rec_off[3]) + 20)
    assert st == 1 and err == [0, 1, 0, 0] and data == b""
    # l_qname / n_cigar / l_seq pointing outside the record; an l_seq that is not the batch's
    for field, fmt, val, which in ((8, "<B", 255, 2), (12, "<H", 60000, 2), (16, "<I", 1 << 30, 2), (16, "<I", 2, 3)):
        raw = rw.raw.copy()
        struct.pack_into(fmt, raw, int(rw.rec_off[1]) + 4 + field, val)
        st, data, _, _, _, err = run(raw, rw.rec_off)
        assert st == 1 and err[which] == 1 and sum(err) == 1 and data == b"", (field, err)
    win.close()
    rd.close()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------

class DeviceRun:
    """one window through the C ABI on the device: upload of the records as they stand, lift (or a hand-made lift result is NOT possible
    here: the device lifts itself), compact, finish, SA, records"""

    def __init__(self, win, index, cn, rn, target):
        import torch

        from portello_amd import devbatch
        self.dev = torch.device("cuda", 0)
        self.eng = api.Engine(index)
        b, f, r = win.batch_raw()
        self.up = devbatch.upload_raw_window(b, f, r, self.dev)
        torch.cuda.synchronize()
        self.ddesc = self.up.batch.desc()
        self.out = self.eng.liftover_batch_dev(self.ddesc)
        self.eng.compact_output_dev(self.out)
        self.labels = devbatch.contig_labels(cn, self.dev)
        self.sa_in, self._keep = devbatch.sa_inputs(rn, self.dev)
        self.target = target

    def finish(self):
        self.fo = self.eng.finish_batch_dev(self.ddesc, self.up.finish_in())

    def sa(self):
        self.so = self.eng.sa_segments_dev(self.sa_in)

    def records(self, rin=None):
        from portello_amd import devbatch
        ro = self.eng.records_build_dev(self.ddesc, rin if rin is not None else self.up.records_in(self.labels, self.target))
        return devbatch.DeviceRecords(ro, dev=self.dev, with_offsets=True)

    def lift_result(self):
        from portello_amd import devbatch
        return devbatch.download(self.eng, self.out)


def check_device(win, ixd, index, cn, rn, target):
    run = DeviceRun(win, index, cn, rn, target)
    run.finish()
    run.sa()
    rec = run.records()
    lift = run.lift_result()
    hdata, hoff, hnl, hnu = host_records(win, ixd, lift, cn, rn, target)
    assert rec.n_records == len(hoff) - 1 and (rec.n_lifted, rec.n_unmapped_copies) == (hnl, hnu) and rec.n_bytes == len(hdata)
    if rec.n_records:
        assert np.array_equal(rec.record_off, hoff)
    data = rec.data()
    for i, (a, e) in enumerate(zip(_split(data, rec.record_off), _split(hdata, hoff))):
        assert a == e, (i, a[:80], e[:80])
    assert data == hdata and rec.records_ms > 0
    run.eng.close()
    return lift, rec


@pytest.mark.gpu
@pytest.mark.parametrize("is_target_region", [False, True])
def test_device_records_equal_the_host_builder(small_bam, is_target_region):
    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    rd, win = open_window(path)
    lift, rec = check_device(win, ixd, index, meta["contig_names"], bamsynth.ref_names(w), is_target_region)
    assert (lift.item_status == abi.ITEM_LIFTED).sum() == rec.n_lifted > 0 and (is_target_region or rec.n_unmapped_copies > 0)
    win.close()
    rd.close()
    index.close()


def _device_workload(n_reads=256, seed=5):
    return synth.generate(synth.config("tiny", n_reads=n_reads, seed=seed, split_read_frac=0.3, sorted_reads=True))


@pytest.mark.gpu
def test_device_alignment_residues_and_odd_names(tmp_path):
    """the device's own lift over a workload whose records carry names and leading tags of every length mod 16 (bamsynth's qnames are of
    one length: the records are re-written with padded names and a padded leading Z tag)"""
    w = _device_workload()
    path = str(tmp_path / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=1, n_unmapped=0)
    rd, win = open_window(path)
    rw = RawWindow(win)
    win.close()
    rd.close()
    recs = []
    for i, o in enumerate(rw.rec_off):
        o = int(o)
        body = bytes(rw.raw[o + 4:o + 4 + struct.unpack_from("<I", rw.raw, o)[0]])
        lq, ncg, lseq = body[8], struct.unpack_from("<H", body, 12)[0], struct.unpack_from("<I", body, 16)[0]
        qn = b"n" * (i % 16) + body[32:32 + lq]
        a = 32 + lq + 4 * ncg + (lseq + 1) // 2 + lseq
        nb = body[:8] + bytes([len(qn)]) + body[9:32] + qn + body[32 + lq:a] + b"XPZ" + b"p" * ((i // 16) % 16) + b"\0" + body[a:]
        recs.append(struct.pack("<I", len(nb)) + nb)
    p2 = str(tmp_path / "padded.bam")
    wr = bam.BamWriter(p2, meta["header_text"], meta["contig_names"], [int(x) for x in w.contig_len], level=1)
    wr.write(b"".join(recs))
    wr.close()
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    rd, win = open_window(p2)
    assert win.n_records == w.n_reads
    check_device(win, ixd, index, meta["contig_names"], bamsynth.ref_names(w), False)
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
def test_device_long_cigar(tmp_path):
    """more than 65535 output CIGAR ops on the device: a read of 2= 1I 2= 1I ... against a contig that maps 1:1 keeps its 70 000 ops"""
    cig = np.array(list(cg.encode("2=1I")) * 35_000, np.uint32)
    from oracle import pyrecords as pr

    l_seq = 3 * 35_000
    rng = np.random.default_rng(3)
    sp = ((1 << rng.integers(0, 4, (l_seq + 1) // 2)).astype(np.uint8) << 4 | (1 << rng.integers(0, 4, (l_seq + 1) // 2)).astype(np.uint8)).astype(np.uint8)
    sp[-1] &= 0xF0
    src = pr.Record(0, 100, 60, 0, 0, -1, -1, 0, b"long", [int(x) for x in cig], sp.tobytes(), l_seq, bytes(l_seq), [(b"NM", b"C\x07")])
    rd, win = write_window(tmp_path, [src.to_bytes(), make_record(1, 50)])
    ixd = abi.IndexData(contig_len=np.array([500000]), contig_seg_off=np.array([0, 1], np.uint32), seg_chrom_index=np.zeros(1, np.uint32),
                        seg_pos=np.array([1000]), seg_is_fwd_strand=np.ones(1, np.uint8), seg_mapq=np.array([33], np.uint8),
                        seg_seq_order_start=np.zeros(1), seg_seq_order_end=np.array([500000]), seg_cigar_off=np.array([0, 1], np.uint32),
                        seg_cigar=np.array(cg.encode("500000="), np.uint32), chrom_seq=[np.full(600000, ord("N"), np.uint8)], rev_contig_seq=[None])
    index = api.Index(ixd, 0)
    lift, rec = check_device(win, ixd, index, CN, ["chr1"], False)
    assert int(lift.item_cigar_len.max()) > 65535, "the lifted CIGAR lost its ops: the case does not reach the CG path"
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
def test_device_refusals(small_bam):
    """called before finish / SA on that context, after a sparse batch, with offsets outside the records: PLO_ERR_INVALID_ARG + a message"""
    import torch

    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    rd, win = open_window(path)
    run = DeviceRun(win, index, cn, rn, False)
    with pytest.raises(api.PortelloError, match="no finishing result") as e:
        run.records()
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    run.finish()
    with pytest.raises(api.PortelloError, match="no SA text") as e:
        run.records()
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    run.sa()
    good = run.records()
    assert good.n_records > 0
    # a read_rec_off beyond records_bytes; a block_size running past the end (the buffer declared shorter)
    bad_off = run.up.rec_off.clone()
    bad_off[5] = run.up.raw_bytes + 100
    torch.cuda.synchronize()
    rin = run.up.records_in(run.labels, False)
    rin.read_rec_off = C.cast(C.c_void_p(bad_off.data_ptr()), C.POINTER(C.c_uint64))
    with pytest.raises(api.PortelloError, match="read_rec_off beyond") as e:
        run.records(rin)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    rin = run.up.records_in(run.labels, False)
    rin.records_bytes = int(run.up.rec_off[-1].item()) + 40
    with pytest.raises(api.PortelloError, match="block_size running past") as e:
        run.records(rin)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    assert run.records().data() == good.data()  # (the context is as good as before)
    # after a sparse batch
    from portello_amd import devbatch
    sp = bam.sparse_pack(win.batch_data())
    db = devbatch.DeviceBatch.from_batch_data(sp, run.dev)
    torch.cuda.synchronize()
    sdesc = db.desc()
    run.eng.liftover_batch_dev(sdesc)
    with pytest.raises(api.PortelloError, match="sparse") as e:
        run.eng.records_build_dev(sdesc, run.up.records_in(run.labels, False))
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
def test_bam_to_bam_with_device_records(tmp_path):
    """run_bam_to_bam(device_records=True) as test_bam_to_bam_into_output_shards is set up: every read, every record of the written shards"""
    from oracle import expect
    from portello_amd import pipeline

    w = synth.generate(synth.config("chr20", n_reads=20_000), device="cuda")
    inp, outp, unp = str(tmp_path / "reads.bam"), str(tmp_path / "lifted.bam"), str(tmp_path / "unassembled.bam")
    meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=8)
    ixd = w.index_data()
    index = api.Index(w.index_data_device())
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    st = pipeline.run_bam_to_bam(inp, outp, index, ixd, cn, rn, [int(s.numel()) for s in w.chrom_seq], window_reads=1500, n_workers=2,
                                 io_threads=8, unassembled_path=unp, device_records=True, out_shards=2)
    assert st.reads == w.n_reads and len(st.out_paths) == 2 and all(os.path.exists(p_) and os.path.getsize(p_) > 1000 for p_ in st.out_paths)
    v = expect.verify_lifted_bam(inp, st.out_paths, ixd, cn, rn, window=1000, every=1, threads=8, unassembled_bam=unp)
    assert v["ok"] and v["reads_verified"] == w.n_reads and v["records_verified"] == st.records_out == v["records_in_output"], v
    assert v["unassembled_ok"]
    assert st.records_device_ms > 0
    index.close()
