"""The liftover batch built on the device (plo_batch_build_dev, portello_amd/csrc/batch_core.hpp).

The yardstick is always plo_bam_window_batch_raw on the same window (itself held to the reference's vectors by tests/test_bam.py): every
array equal element for element, and for input the host refuses the same status, the same read and the same kind of failure.  The CPU
tests run batch_core.hpp under the wave emulator (tests/emu/emu_batch.cpp); the GPU tests run the C ABI on the device and the pipeline
mode."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import emu_batch_lib as ebl
from portello_amd import abi, api, bam, bamsynth, synth
from portello_amd import cigar as cg
from test_records_dev import MALFORMED, _aux_tag_order, hand_index, long_cigar, make_record, malformed_records

NAMES = ["ctg0", "ctg1", "c", "ctg10", "a-much-longer-contig-name_with.odd:chars|0123456789"]
HOST_KINDS = (("SA aux tag is not a string", abi.BB_ERR_SA_NOT_Z), ("Unexpected segment in bam SA tag", abi.BB_ERR_FIELD_COUNT),
              ("malformed SA segment", abi.BB_ERR_MALFORMED), ("split segment id unaligned", abi.BB_ERR_UNALIGNED),
              ("SA segment read length differs", abi.BB_ERR_READ_SIZE), ("not found in the input header", abi.BB_ERR_UNKNOWN_CONTIG),
              ("Can't parse consistent split read", abi.BB_ERR_EMPTY_SEGMENT))


def _arr(ptr, dtype, count):
    if not count:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype).copy()


def raw_of(win):
    """(records, read_rec_off) of bam.Window.raw(): no batch is built"""
    r = win.raw()
    return _arr(r.raw, np.uint8, int(r.raw_bytes)), _arr(r.read_rec_off, np.uint64, int(r.n_reads))


def host_batch(win):
    """plo_bam_window_batch_raw: (PLO_OK, arrays by name) or (status, kind of the failure by its message, message)"""
    try:
        b, f, r = win.batch_raw()
    except api.PortelloError as e:
        kinds = [k for text, k in HOST_KINDS if text in str(e)]
        assert len(kinds) == 1, str(e)
        return e.status, kinds[0], str(e)
    n, ns = int(b.n_reads), int(b.n_segs)
    coff = _arr(b.seg_cigar_off, np.uint32, ns + 1)
    cnt = ebl.counts(n, ns, int(coff[-1]))
    return abi.PLO_OK, {name: _arr(getattr(f if name in ("read_flags", "read_qual_off") else b, name), dt, cnt[k]) for name, dt, k in ebl.ARRAYS}, ""


def assert_same_arrays(got, want, what=""):
    for name, _, _ in ebl.ARRAYS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, (what, name, got[name].shape, want[name].shape)
        if not np.array_equal(got[name], want[name]):
            bad = np.flatnonzero(got[name] != want[name])
            raise AssertionError((what, name, int(bad[0]), got[name][bad[:4]], want[name][bad[:4]]))


def check_emulated(win, names, order_seed=0, bad_read=None):
    """batch_core.hpp under the emulator against the host batcher on the same window -> the host's (status, arrays | kind)"""
    raw, rec_off = raw_of(win)
    hst, hres, hmsg = host_batch(win)
    st, arrays, err_read, err_kind, bounds = ebl.batch_build(raw, rec_off, names, order_seed)
    assert bounds == [0, 0, 0, 0]
    assert st == hst, (st, hst, hmsg, err_read, err_kind)
    if st == abi.PLO_OK:
        assert (err_read, err_kind) == (abi.BB_NO_READ, abi.BB_ERR_NONE)
        assert_same_arrays(arrays, hres)
    else:
        assert st == abi.PLO_ERR_DATA and arrays is None
        assert err_kind == hres, (err_kind, hmsg)
        qn = bytes(raw[int(rec_off[err_read]) + 36:]).split(b"\0")[0].decode()
        if "in read" in hmsg or "In read" in hmsg:
            assert qn in hmsg, (err_read, qn, hmsg)  # (the host names the record by its read name)
        if bad_read is not None:
            assert err_read == bad_read, (err_read, bad_read, hmsg)
    return hst, hres


def write_window(tmp_path, recs, names=NAMES, name="hand.bam", max_records=100_000):
    path = str(tmp_path / name)
    wr = bam.BamWriter(path, "@HD\tVN:1.6\n", names, [500000] * len(names), level=1)
    wr.write(b"".join(recs))
    wr.close()
    rd = bam.BamReader(path, 2)
    return rd, rd.read_window(max_records)


def sa_aux(text):
    return b"SAZ" + (text.encode() if isinstance(text, str) else text) + b"\0"


def rec20(k, sa=None, aux=b"", flag=0, cigar="10S5M5S"):
    """a 20-base read (sequencing-order [10, 15) when forward) with an SA text"""
    return make_record(k, 20, flag=flag, aux=aux + (sa_aux(sa) if sa is not None else b""), cigar=np.array(cg.encode(cigar), np.uint32))


# ---- 1. the small_bam recipe of tests/test_records_dev.py ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("batchdev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=411, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


def test_sample_batch_equals_the_host_batcher(small_bam):
    w, path, meta = small_bam
    rd = bam.BamReader(path, 2)
    win = rd.read_window(100_000)
    st, b = check_emulated(win, meta["contig_names"])
    assert st == abi.PLO_OK
    check_emulated(win, meta["contig_names"], order_seed=9)  # shuffled lane order
    # the sample is not vacuous
    raw, rec_off = raw_of(win)
    n = len(rec_off)
    first = np.searchsorted(b["seg_read"], np.arange(n + 1))
    n_seg = np.diff(first)
    assert (n_seg >= 2).sum() > 10, "no reads with two segments"
    src = [bytes(raw[int(o):int(o) + 4 + struct.unpack_from("<I", raw, int(o))[0]]) for o in rec_off]
    sa_texts = [r[r.index(b"SAZ") + 3:].split(b"\0")[0] if (b"SA", "Z") in _aux_tag_order(r) else None for r in src]
    assert any(t is None for t in sa_texts) and all((t is None) == (k == 1) for t, k in zip(sa_texts, n_seg)), "no read without an SA tag"
    assert any(seg.split(b",")[2] == b"-" for t in sa_texts if t for seg in t.split(b";") if seg), "no reverse-strand SA segment"
    moved = 0
    for i in range(n):  # the primary stands first in the text: a read whose first segment is not the primary's was re-ordered by the sort
        tid, pos = struct.unpack_from("<ii", src[i], 4)
        s0 = int(first[i])
        moved += n_seg[i] >= 2 and (int(b["seg_contig"][s0]), int(b["seg_pos"][s0])) != (tid, pos)
    assert moved > 0, "no read whose sorted order differs from its text order"
    win.close()
    rd.close()


# ---- 2. the reference's vectors (as tests/test_bam.py transcribes them) ----------------------------------------------------------------------

SA_VECTOR = ("chr3,10001,+,5535S10=1D39=2X11438S,60,192;chr3,10001,+,3073S15=2D20=2X11=1X5=1I23=1X5=14798S,22,44;"
             "chr4,106872270,-,23=1I226=1I195=1X147=1D1021=7362S,60,19;")  # sa_tag_parser.rs:66-77


def _read_len(text):
    return int(sum(int(c) >> 4 for c in cg.encode(text) if (0x1B3 >> (int(c) & 15)) & 1))


def test_sa_parser_reference_vector(tmp_path):
    """every segment of the vector beside a primary of its own read length, then the whole value in one record: its segments disagree about
    the read's length, which both builders refuse alike"""
    names = ["chr1", "chr2", "chr3", "chr4"]
    recs = []
    for k, seg in enumerate(SA_VECTOR.rstrip(";").split(";")):
        L = _read_len(seg.split(",")[3])
        recs.append(make_record(k, L, aux=sa_aux(seg + ";"), cigar=np.array(cg.encode(f"{L // 2}S{L - L // 2}M"), np.uint32)))
    rd, win = write_window(tmp_path, recs, names)
    st, b = check_emulated(win, names)
    assert st == abi.PLO_OK and list(b["seg_read"]) == [0, 0, 1, 1, 2, 2]
    got = {(int(c), int(p), int(f)) for c, p, f in zip(b["seg_contig"], b["seg_pos"], b["seg_is_fwd_strand"])}
    assert {(2, 10_000, 1), (3, 106_872_269, 0)} <= got
    win.close()
    rd.close()
    L = _read_len(SA_VECTOR.split(";")[0].split(",")[3])
    rd, win = write_window(tmp_path, [make_record(0, L, aux=sa_aux(SA_VECTOR))], names, name="whole.bam")
    st, kind = check_emulated(win, names, bad_read=0)
    assert (st, kind) == (abi.PLO_ERR_DATA, abi.BB_ERR_READ_SIZE)
    win.close()
    rd.close()


def _sam_record(tid, pos1, cigar_text, seq, qual, sa=None, flag=0):
    cig = np.array(cg.encode(cigar_text), dtype=np.uint32)
    lut = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
    n4 = [lut[c] for c in seq] + ([0] if len(seq) & 1 else [])
    sp = bytes((n4[i] << 4) | n4[i + 1] for i in range(0, len(n4), 2))
    aux = (b"SAZ" + sa.encode() + b"\0") if sa else b""
    return bamsynth.encode_record(tid, pos1 - 1, 60, flag, b"qname", cig, sp, len(seq), bytes(ord(c) - 33 for c in qual), aux)


def test_split_segments_reference_vectors(tmp_path):
    """split_read.rs:198-232"""
    names = ["chr0", "chr1", "chr2"]
    seq, qual = "ACGCCGTATCGTCTCGAGGA", "DDDDDEEEEEDDDDDEEEEE"
    r1 = _sam_record(2, 10, "10S5M5S", seq, qual)
    r2 = _sam_record(2, 10, "10S5M5S", seq, qual, sa="chr0,20,-,5M15S,60,0;chr0,100,+,5S5M10S,60,0;chr1,200,-,15S5M,60,0;")
    exp = [(2, 9, True, "10S5M5S"), (1, 199, False, "15S5M"), (0, 99, True, "5S5M10S"), (2, 9, True, "10S5M5S"), (0, 19, False, "5M15S")]
    rd, win = write_window(tmp_path, [r1, r2], names)
    raw, rec_off = raw_of(win)
    st, b, _, _, _ = ebl.batch_build(raw, rec_off, names)
    assert st == abi.PLO_OK and list(b["seg_read"]) == [0, 1, 1, 1, 1]
    assert [(int(c), int(p), bool(f)) for c, p, f in zip(b["seg_contig"], b["seg_pos"], b["seg_is_fwd_strand"])] == [e[:3] for e in exp]
    for s, e in enumerate(exp):
        assert cg.decode(b["cigar"][int(b["seg_cigar_off"][s]):int(b["seg_cigar_off"][s + 1])]) == e[3]
    check_emulated(win, names)
    win.close()
    rd.close()


# ---- 3. hand-made records -----------------------------------------------------------------------------------------------------------------

def _many_segments(k, n_sa, L, seed):
    """a read of L bases whose n_sa SA segments (one aligned base each, either strand) stand in shuffled order"""
    rng = np.random.default_rng(seed)
    segs = []
    for j in rng.permutation(np.arange(1, n_sa + 1)):
        j = int(j)
        fwd = bool(rng.integers(0, 2))
        lead = j if fwd else L - 1 - j
        text = (f"{lead}S" if lead else "") + "1M" + (f"{L - 1 - lead}S" if L - 1 - lead else "")
        segs.append(f"{NAMES[j % len(NAMES)]},{1000 + j},{'+' if fwd else '-'},{text},{j % 61},{j % 7}")
    return make_record(k, L, aux=b"XXZkeep\0" + sa_aux(";".join(segs) + ";"), cigar=np.array(cg.encode(f"1M{L - 1}S"), np.uint32))


def test_hand_made_sa_texts(tmp_path):
    recs = [
        rec20(0, "ctg0,100,+,5S5M10S,60,0"),                                  # no final ';'
        rec20(1, "ctg1,100,+,5S5M10S,60,0,;"),                                # a trailing comma
        rec20(2, "ctg0,+100,+,5S5M10S,60,+3;ctg1,-5,-,5M15S,60,-3;"),         # signed numbers
        rec20(3, "ctg0,100,+,10S5M5S,60,0;ctg1,300,+,10S6M4S,60,0;c,7,+,5S5M10S,1,0;"),  # so_start 10 three times: text order kept
        rec20(4, "ctg10,100,+,5S5M10S,60,0;"),
        rec20(5, "ctg0,9,+,1S5M14S,60,0;", aux=sa_aux("ctg1,100,+,5S5M10S,60,0;")),  # an SA tag twice: the first wins
        rec20(6, "ctg1,100,-,5S5M10S,60,0;", aux=b"mlBC" + struct.pack("<I", 5) + bytes(5) + b"ziBS" + struct.pack("<I", 2) + bytes(4)),  # behind B arrays
        rec20(7, "ctg1,100,-,5S5M10S,60,0;", aux=b"XQ?abc"),                  # behind a malformed field: the walk ends, no SA
        rec20(8, "ctg1,100,-,5S5M10S,60,0;", aux=b"XQZno terminator"),        # (swallowed by a string without its NUL ... which ends at the SA's)
        rec20(9, None, flag=0x10),
        rec20(10, "ctg0,100,+,5S5M10S,60,0;", flag=0x10),                     # a reverse-strand primary
        rec20(11, "a-much-longer-contig-name_with.odd:chars|0123456789,100,+,2S3=1X1I1D2N1P3M10H,255,2147483647;c,1,x,20M,0,-2147483648;"),
        _many_segments(12, 70, 100, 1),
        _many_segments(13, 310, 400, 2),
        _many_segments(14, 64, 65, 3),
        _many_segments(15, 63, 64, 4),
    ]
    rd, win = write_window(tmp_path, recs)
    assert win.n_records == len(recs)
    st, b = check_emulated(win, NAMES)
    assert st == abi.PLO_OK
    check_emulated(win, NAMES, order_seed=5)
    n_seg = np.bincount(b["seg_read"], minlength=len(recs))
    assert list(n_seg[:12]) == [2, 2, 3, 4, 2, 2, 2, 1, 1, 1, 2, 3] and list(n_seg[12:]) == [71, 311, 65, 64]
    s3 = int(np.searchsorted(b["seg_read"], 3))
    assert [int(x) for x in b["seg_contig"][s3:s3 + 4]] == [2, 0, 0, 1]  # so_start 5, then the primary and the two that tie with it, in text order
    s5 = int(np.searchsorted(b["seg_read"], 5))
    assert int(b["seg_contig"][s5]) == 1 and int(b["seg_pos"][s5]) == 99
    win.close()
    rd.close()


def test_cg_placeholder_beside_a_short_record(tmp_path):
    """a source record stored with the <l_seq>S<n>N placeholder and its 70 001 ops in CG:B,I, with an SA segment of the same read length"""
    from oracle import pyrecords as pr

    n = 70_001
    cig = long_cigar(n)
    src = pr.Record(0, 10, 60, 0, 0, -1, -1, 0, b"long", [int(x) for x in cig], bytes((n + 1) // 2), n, bytes(n),
                    [(b"rq", b"f" + struct.pack("<f", 1.0)), (b"SA", b"Zctg1,5,-,%dS%dM,60,0;\0" % (n - 100, 100))])
    rb = src.to_bytes()
    assert struct.unpack_from("<H", rb, 16)[0] == 2 and b"CGBI" in rb
    # a two-op CIGAR that only looks like the placeholder (no CG field) and one whose CG field is not a B,I array stay as they are
    look = make_record(2, 33, cigar=np.array(cg.encode("33S5N"), np.uint32), aux=b"XXZkeep\0")
    other = make_record(3, 33, cigar=np.array(cg.encode("33S5N"), np.uint32), aux=b"CGZtext\0")
    rd, win = write_window(tmp_path, [rb, rec20(1, "ctg0,100,+,5S5M10S,60,0;")], name="cg.bam")
    st, b = check_emulated(win, NAMES)
    assert st == abi.PLO_OK and int(b["seg_cigar_off"][-1]) == n + 2 + 3 + 3
    win.close()
    rd.close()
    for k, rec in enumerate((look, other)):  # (the look-alikes keep their two ops, which align no base: an empty split segment)
        rd, win = write_window(tmp_path, [rec20(0), rec], name=f"look{k}.bam")
        st, kind = check_emulated(win, NAMES, bad_read=1)
        assert (st, kind) == (abi.PLO_ERR_DATA, abi.BB_ERR_EMPTY_SEGMENT)
        win.close()
        rd.close()


def test_sequence_lengths_and_an_empty_window(tmp_path):
    lens = [0, 1, 2, 15, 16, 17]
    recs = [make_record(k, l, cigar=None if l else np.array(cg.encode("3M"), np.uint32)) for k, l in enumerate(lens)]
    rd, win = write_window(tmp_path, recs)
    st, b = check_emulated(win, NAMES)
    assert st == abi.PLO_OK and list(b["read_seq_len"]) == lens
    win.close()
    rd.close()
    # a window with 0 primary records: one unmapped record only
    un = bamsynth.encode_record(-1, -1, 0, 4, b"u0", np.zeros(0, np.uint32), bytes(5), 10, bytes(10), b"")
    rd, win = write_window(tmp_path, [un], name="empty.bam")
    if win is not None:
        assert win.n_records == 0
        st, b = check_emulated(win, NAMES)
        assert st == abi.PLO_OK and all(len(b[name]) == (1 if name == "seg_cigar_off" else 0) for name, _, _ in ebl.ARRAYS)
        win.close()
    st, arrays, err_read, _, _ = ebl.batch_build(np.zeros(0, np.uint8), np.zeros(0, np.uint64), NAMES)
    assert st == abi.PLO_OK and err_read == abi.BB_NO_READ and list(arrays["seg_cigar_off"]) == [0] and len(arrays["seg_read"]) == 0
    rd.close()


# ---- 4. every kind of refused input ---------------------------------------------------------------------------------------------------------

OK_SA = "ctg0,100,+,5S5M10S,60,0;"
BAD = {
    "sa_not_z": (rec20(0, None, aux=b"SAi" + struct.pack("<i", 7)), abi.BB_ERR_SA_NOT_Z),
    "sa_is_h": (rec20(0, None, aux=b"SAH" + OK_SA.encode() + b"\0"), abi.BB_ERR_SA_NOT_Z),
    "five_fields": (rec20(0, "ctg0,100,+,5S5M10S,60;"), abi.BB_ERR_FIELD_COUNT),
    "seven_fields": (rec20(0, "ctg0,100,+,5S5M10S,60,0,1;"), abi.BB_ERR_FIELD_COUNT),
    "six_fields_two_trailing_commas": (rec20(0, "ctg0,100,+,5S5M10S,60,0,,;"), abi.BB_ERR_FIELD_COUNT),
    "empty_segment": (rec20(0, OK_SA + ";" + OK_SA), abi.BB_ERR_FIELD_COUNT),
    "only_a_semicolon": (rec20(0, ";"), abi.BB_ERR_FIELD_COUNT),
    "six_empty_fields": (rec20(0, ",,,,,;"), abi.BB_ERR_FIELD_COUNT),
    "pos_not_a_number": (rec20(0, "ctg0,12x,+,5S5M10S,60,0;"), abi.BB_ERR_MALFORMED),
    "pos_empty": (rec20(0, "ctg0,,+,5S5M10S,60,0;"), abi.BB_ERR_MALFORMED),
    "pos_sign_only": (rec20(0, "ctg0,-,+,5S5M10S,60,0;"), abi.BB_ERR_MALFORMED),
    "pos_past_2_62": (rec20(0, "ctg0,4611686018427387905,+,5S5M10S,60,0;"), abi.BB_ERR_MALFORMED),
    "mapq_256": (rec20(0, "ctg0,100,+,5S5M10S,256,0;"), abi.BB_ERR_MALFORMED),
    "mapq_signed": (rec20(0, "ctg0,100,+,5S5M10S,+6,0;"), abi.BB_ERR_MALFORMED),
    "nm_past_int32": (rec20(0, "ctg0,100,+,5S5M10S,60,2147483648;"), abi.BB_ERR_MALFORMED),
    "nm_below_int32": (rec20(0, "ctg0,100,+,5S5M10S,60,-2147483649;"), abi.BB_ERR_MALFORMED),
    "cigar_trailing_digits": (rec20(0, "ctg0,100,+,5S5M10,60,0;"), abi.BB_ERR_MALFORMED),
    "cigar_op_without_length": (rec20(0, "ctg0,100,+,5SM15S,60,0;"), abi.BB_ERR_MALFORMED),
    "cigar_unknown_op": (rec20(0, "ctg0,100,+,5S5Q10S,60,0;"), abi.BB_ERR_MALFORMED),
    "cigar_lower_case_op": (rec20(0, "ctg0,100,+,5S5m10S,60,0;"), abi.BB_ERR_MALFORMED),
    "cigar_op_length_2_28": (rec20(0, "ctg0,100,+,268435456M,60,0;"), abi.BB_ERR_MALFORMED),
    "cigar_op_length_past_2_62": (rec20(0, "ctg0,100,+,5S4611686018427387905M,60,0;"), abi.BB_ERR_MALFORMED),
    "no_aligned_op": (rec20(0, "ctg0,100,+,5I15S,60,0;"), abi.BB_ERR_UNALIGNED),
    "empty_cigar": (rec20(0, "ctg0,100,+,,60,0;"), abi.BB_ERR_UNALIGNED),
    "read_size": (rec20(0, "ctg0,100,+,5S5M9S,60,0;"), abi.BB_ERR_READ_SIZE),
    "op_length_2_28_less_1_is_taken": (rec20(0, "ctg0,100,+,268435455M,60,0;"), abi.BB_ERR_READ_SIZE),
    "unknown_contig": (rec20(0, "ctg2,100,+,5S5M10S,60,0;"), abi.BB_ERR_UNKNOWN_CONTIG),
    "contig_prefix_of_a_name": (rec20(0, "ctg,100,+,5S5M10S,60,0;"), abi.BB_ERR_UNKNOWN_CONTIG),
    "empty_contig": (rec20(0, ",100,+,5S5M10S,60,0;"), abi.BB_ERR_UNKNOWN_CONTIG),
    "empty_sa_segment": (rec20(0, "ctg0,100,+,5S0M15S,60,0;"), abi.BB_ERR_EMPTY_SEGMENT),
    "empty_primary": (make_record(0, 0), abi.BB_ERR_EMPTY_SEGMENT),
    "primary_of_clips_only": (rec20(0, OK_SA, cigar="20S"), abi.BB_ERR_EMPTY_SEGMENT),
    # one record with two faults: the first in the host's walk order is reported
    "read_size_before_unknown_contig": (rec20(0, "nope,100,+,5S5M9S,60,0;"), abi.BB_ERR_READ_SIZE),
    "malformed_before_unaligned": (rec20(0, "ctg0,x,+,20S,60,0;"), abi.BB_ERR_MALFORMED),
    "first_segment_before_the_second": (rec20(0, "nope,100,+,5S5M10S,60,0;ctg0,100;"), abi.BB_ERR_UNKNOWN_CONTIG),
    "segment_fault_before_the_empty_primary": (rec20(0, "nope,100,+,20M,60,0;", cigar="20S"), abi.BB_ERR_UNKNOWN_CONTIG),
    "sa_not_z_before_the_empty_primary": (rec20(0, None, aux=b"SAC\x01", cigar="20S"), abi.BB_ERR_SA_NOT_Z),
}


def _renamed(rec, k):
    """the record with the read name r<k>"""
    body = rec[4:]
    lq = body[8]
    qn = b"r%d\0" % k
    nb = body[:8] + bytes([len(qn)]) + body[9:32] + qn + body[32 + lq:]
    return struct.pack("<I", len(nb)) + nb


@pytest.mark.parametrize("case", sorted(BAD))
def test_one_bad_record_among_good_ones(tmp_path, case):
    bad, kind = BAD[case]
    recs = [rec20(0, OK_SA), rec20(1), _renamed(bad, 2), rec20(3, OK_SA), _renamed(bad, 4)]
    rd, win = write_window(tmp_path, recs)
    st, got = check_emulated(win, NAMES, order_seed=len(case) % 3, bad_read=2)
    assert (st, got) == (abi.PLO_ERR_DATA, kind)
    win.close()
    rd.close()


def test_parse_uint_wraps_as_the_host_does(tmp_path):
    """20 digits whose value passes 2^64 between two checks of the 2^62 cap: whatever the host makes of them, the device makes too"""
    for k, text in enumerate(("ctg0,100,+,18446744073709551620M,60,0;", "ctg0,100,+,00000000000000000000000020M,60,0;", "ctg0,18446744073709551716,+,20M,60,0;")):
        rd, win = write_window(tmp_path, [rec20(0, OK_SA), rec20(1, text)], name=f"wrap{k}.bam")
        check_emulated(win, NAMES)
        win.close()
        rd.close()


def test_the_lowest_failing_read_is_reported(tmp_path):
    recs = [rec20(0, OK_SA)] + [rec20(k) for k in range(1, 70)]
    recs[66] = _renamed(BAD["five_fields"][0], 66)
    recs[40] = _renamed(BAD["unknown_contig"][0], 40)
    recs[41] = _renamed(BAD["sa_not_z"][0], 41)
    rd, win = write_window(tmp_path, recs)
    st, kind = check_emulated(win, NAMES, bad_read=40)
    assert (st, kind) == (abi.PLO_ERR_DATA, abi.BB_ERR_UNKNOWN_CONTIG)
    win.close()
    rd.close()


def test_records_outside_the_buffer_are_refused(tmp_path):
    recs = [rec20(k, OK_SA, aux=b"XXZkeep\0") for k in range(4)]
    rd, win = write_window(tmp_path, recs)
    raw, rec_off = raw_of(win)
    assert ebl.batch_build(raw, rec_off, NAMES)[0] == abi.PLO_OK
    off = rec_off.copy()
    off[2] = len(raw) - 2
    st, arrays, _, _, bounds = ebl.batch_build(raw, off, NAMES)
    assert st == abi.PLO_ERR_INVALID_ARG and bounds == [1, 0, 0, 0] and arrays is None
    st, arrays, _, _, bounds = ebl.batch_build(raw, rec_off, NAMES, records_bytes=int(rec_off[3]) + 20)
    assert st == abi.PLO_ERR_INVALID_ARG and bounds == [0, 1, 0, 0] and arrays is None
    for field, fmt, val in ((8, "<B", 255), (12, "<H", 60000), (16, "<I", 1 << 30), (0 - 4, "<I", 31)):
        bad = raw.copy()
        struct.pack_into(fmt, bad, int(rec_off[1]) + 4 + field, val)
        st, arrays, _, _, bounds = ebl.batch_build(bad, rec_off, NAMES)
        assert st == abi.PLO_ERR_INVALID_ARG and sum(bounds) == 1 and bounds[1 if field < 0 else 2] == 1 and arrays is None, (field, bounds)
    win.close()
    rd.close()


def test_malformed_aux_under_the_sanitizers(tmp_path):
    """the malformed-aux window of tests/test_records_dev.py, whole and cut off right behind its last record, through the AddressSanitizer +
    UBSan build of the emulator (CPU): every input in a heap block of its exact size, no read outside a record, the host's arrays"""
    names = ["ctg0"]
    recs = malformed_records() + [rec20(len(MALFORMED), OK_SA, aux=b"XQZ" + b"q" * 130 + b"\0"), rec20(len(MALFORMED) + 1, OK_SA[:-1])]
    rd, win = write_window(tmp_path, recs, names)
    raw, rec_off = raw_of(win)
    hst, want, _ = host_batch(win)
    assert hst == abi.PLO_OK
    end = int(rec_off[-1]) + 4 + struct.unpack_from("<I", raw, int(rec_off[-1]))[0]
    for k, data in enumerate((raw.tobytes(), raw[:end].tobytes())):
        rc, err_text, st, arrays = ebl.run_asan(data, rec_off, names, str(tmp_path))
        assert rc == 0, err_text[-3000:]
        assert st == abi.PLO_OK
        assert_same_arrays(arrays, want, k)
    # the last record's malformed tail is the end of the buffer
    tail = [rec20(0, OK_SA)] + malformed_records()
    rd2, win2 = write_window(tmp_path, tail, names, name="tail.bam")
    raw2, off2 = raw_of(win2)
    hst, want2, _ = host_batch(win2)
    end2 = int(off2[-1]) + 4 + struct.unpack_from("<I", raw2, int(off2[-1]))[0]
    rc, err_text, st, arrays = ebl.run_asan(raw2[:end2].tobytes(), off2, names, str(tmp_path))
    assert rc == 0, err_text[-3000:]
    assert st == hst == abi.PLO_OK
    assert_same_arrays(arrays, want2, "tail")
    for h in (win, rd, win2, rd2):
        h.close()


def test_device_batch_needs_device_records():
    from portello_amd import pipeline

    with pytest.raises(ValueError, match="device_records"):
        pipeline.run_bam_to_bam("in.bam", "out.bam", None, None, [], [], [], device_batch=True)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------

class DeviceBuild:
    """one window through plo_batch_build_dev: the records and read_rec_off go up, nothing else"""

    def __init__(self, win, index, names):
        import torch

        from portello_amd import devbatch
        self.dev = torch.device("cuda", 0)
        self.eng = api.Engine(index)
        self.up = devbatch.upload_records(win.raw(), self.dev)
        self.labels = devbatch.contig_labels(names, self.dev)
        torch.cuda.synchronize()

    def build(self, bin_=None):
        from portello_amd import devbatch
        self.built = devbatch.DeviceBuiltWindow(self.up, self.eng.batch_build_dev(bin_ if bin_ is not None else self.up.build_in(self.labels)))
        return self.built

    def arrays(self):
        b, f = self.built.bo.batch, self.built.bo.fin
        n, ns = int(b.n_reads), int(b.n_segs)
        coff = self.eng.download(b.seg_cigar_off, np.uint32, ns + 1)
        cnt = ebl.counts(n, ns, int(coff[-1]))
        return {name: self.eng.download(getattr(f if name in ("read_flags", "read_qual_off") else b, name), dt, cnt[k]) for name, dt, k in ebl.ARRAYS}


def check_device(win, index, names):
    hst, want, _ = host_batch(win)
    assert hst == abi.PLO_OK
    run = DeviceBuild(win, index, names)
    built = run.build()
    b, f = built.bo.batch, built.bo.fin
    assert int(b.seq_fmt) == abi.SEQ_BAM4 and int(b.n_items) == 0 and int(b.seq_bytes) == int(f.qual_bytes) == run.up.raw_bytes
    assert C.cast(b.seq, C.c_void_p).value == C.cast(f.qual, C.c_void_p).value == run.up.raw.data_ptr()
    assert built.batch_ms > 0 and int(built.bo.err_read) == abi.BB_NO_READ
    assert_same_arrays(run.arrays(), want)
    return run


@pytest.mark.gpu
def test_device_batch_equals_the_host_batcher_and_feeds_the_lift(small_bam):
    """plo_batch_build_dev on the small sample: the arrays, then the lift of the device-built batch against the lift of the host-built one
    (bit-identical), then plo_records_build_dev's bytes against plo_records_build"""
    import torch

    from portello_amd import devbatch
    from test_records_dev import host_records
    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    rd = bam.BamReader(path, 2)
    win = rd.read_window(100_000)
    run = check_device(win, index, cn)
    ddesc = run.built.desc()
    out = run.eng.liftover_batch_dev(ddesc)
    run.eng.compact_output_dev(out)
    lift = devbatch.download(run.eng, out)
    # the host-built batch on a context of the same kind
    eng2 = api.Engine(index)
    b, f, r = win.batch_raw()
    up2 = devbatch.upload_raw_window(b, f, r, run.dev)
    torch.cuda.synchronize()
    out2 = eng2.liftover_batch_dev(up2.batch.desc())
    eng2.compact_output_dev(out2)
    lift2 = devbatch.download(eng2, out2)
    for name in ("item_seg", "item_cseg", "item_status", "item_need_flipped", "item_mapq", "item_chrom_index", "item_ref_pos", "item_cigar_off", "item_cigar_len", "cigar"):
        assert np.array_equal(getattr(lift, name), getattr(lift2, name)), name
    assert (lift.item_status == abi.ITEM_LIFTED).sum() > 0
    # the records from the device-built batch; its outputs are still the batch after the calls behind it
    sa_in, _keep = devbatch.sa_inputs(rn, run.dev)
    run.eng.finish_batch_dev(ddesc, run.built.finish_in())
    run.eng.sa_segments_dev(sa_in)
    ro = run.eng.records_build_dev(ddesc, run.built.records_in(run.labels, False))
    rec = devbatch.DeviceRecords(ro, dev=run.dev, with_offsets=True)
    hdata, hoff, hnl, hnu = host_records(win, ixd, lift2, cn, rn, False)
    assert rec.data() == hdata and np.array_equal(rec.record_off, hoff) and (rec.n_lifted, rec.n_unmapped_copies) == (hnl, hnu)
    bo = run.eng.bgzf_compress_dev(ro.bytes, int(ro.n_bytes), 0)
    assert int(bo.n_in) == len(hdata)
    hst, want, _ = host_batch(win)
    assert_same_arrays(run.arrays(), want, "after the calls behind it")
    eng2.close()
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
def test_device_batch_long_cigar_and_many_segments(tmp_path):
    from oracle import pyrecords as pr

    n = 70_001
    cig = long_cigar(n)
    src = pr.Record(0, 10, 60, 0, 0, -1, -1, 0, b"long", [int(x) for x in cig], bytes((n + 1) // 2), n, bytes(n),
                    [(b"rq", b"f" + struct.pack("<f", 1.0)), (b"SA", b"Zctg1,5,-,%dS%dM,60,0;\0" % (n - 100, 100))])
    recs = [src.to_bytes(), rec20(1, "ctg0,100,+,5S5M10S,60,0"), _many_segments(2, 310, 400, 2), _many_segments(3, 64, 65, 3),
            rec20(4, "ctg0,100,+,10S5M5S,60,0;ctg1,300,+,10S6M4S,60,0;c,7,+,5S5M10S,1,0;"), rec20(5, "ctg1,100,-,5S5M10S,60,0;", aux=b"XQ?abc")]
    rd, win = write_window(tmp_path, recs)
    index = api.Index(hand_index(), 0)
    run = check_device(win, index, NAMES)
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
def test_device_batch_chr20_window(tmp_path):
    w = synth.generate(synth.config("chr20", n_reads=20_000), device="cuda")
    inp = str(tmp_path / "reads.bam")
    meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=8)
    index = api.Index(w.index_data_device())
    rd = bam.BamReader(inp, 8)
    win = rd.read_window(20_000)
    assert win.n_records == 20_000
    run = check_device(win, index, meta["contig_names"])
    a = run.arrays()
    assert len(a["seg_read"]) > 20_000, "no split reads in the window"
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sa_not_z", "five_fields", "cigar_unknown_op", "no_aligned_op", "read_size", "unknown_contig", "empty_sa_segment"])
def test_device_refuses_what_the_host_refuses(tmp_path, case):
    """data errors of the input (no fault is provoked on the card): status, err_read, err_kind; an offset outside the buffer; the context works
    afterwards"""
    import torch

    bad, kind = BAD[case]
    recs = [rec20(0, OK_SA), rec20(1), _renamed(bad, 2), rec20(3, OK_SA), _renamed(bad, 4)]
    rd, win = write_window(tmp_path, recs)
    hst, hkind, hmsg = host_batch(win)
    assert (hst, hkind) == (abi.PLO_ERR_DATA, kind)
    index = api.Index(hand_index(), 0)
    run = DeviceBuild(win, index, NAMES)
    with pytest.raises(api.PortelloError, match="read 2") as e:
        run.build()
    assert e.value.status == abi.PLO_ERR_DATA and (e.value.err_read, e.value.err_kind) == (2, kind) and f"kind {kind}" in str(e.value)
    win.close()
    rd.close()
    # a good window on the same context, then offsets outside the buffer, then the good window again
    rd, win = write_window(tmp_path, [rec20(k, OK_SA) for k in range(6)], name="good.bam")
    _, want, _ = host_batch(win)
    good = DeviceBuild(win, index, NAMES)
    good.eng.close()
    good.eng = run.eng
    good.build()
    assert_same_arrays(good.arrays(), want)
    bad_off = good.up.rec_off.clone()
    bad_off[3] = good.up.raw_bytes + 100
    torch.cuda.synchronize()
    bin_ = good.up.build_in(good.labels)
    bin_.read_rec_off = C.cast(C.c_void_p(bad_off.data_ptr()), C.POINTER(C.c_uint64))
    with pytest.raises(api.PortelloError, match="read_rec_off beyond") as e:
        good.build(bin_)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    bin_ = good.up.build_in(good.labels)
    bin_.records_bytes = int(good.up.rec_off[-1].item()) + 40
    with pytest.raises(api.PortelloError, match="block_size running past") as e:
        good.build(bin_)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    good.build()
    assert_same_arrays(good.arrays(), want)
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_bgzf", [False, True])
def test_bam_to_bam_with_device_batch(tmp_path, device_bgzf):
    """run_bam_to_bam(device_records=True, device_batch=True) as test_bam_to_bam_with_device_records is set up: every read, every record"""
    from oracle import expect
    from portello_amd import pipeline

    w = synth.generate(synth.config("chr20", n_reads=20_000), device="cuda")
    inp, outp, unp = str(tmp_path / "reads.bam"), str(tmp_path / "lifted.bam"), str(tmp_path / "unassembled.bam")
    meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=8)
    ixd = w.index_data()
    index = api.Index(w.index_data_device())
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    args = (inp, outp, index, ixd, cn, rn, [int(s.numel()) for s in w.chrom_seq])
    with pytest.raises(ValueError, match="device_records"):
        pipeline.run_bam_to_bam(*args, device_batch=True)
    st = pipeline.run_bam_to_bam(*args, window_reads=1500, n_workers=2, io_threads=8, unassembled_path=unp, device_records=True, device_batch=True,
                                 device_bgzf=device_bgzf, out_shards=2)
    assert st.reads == w.n_reads and len(st.out_paths) == 2 and all(os.path.exists(p_) and os.path.getsize(p_) > 1000 for p_ in st.out_paths)
    v = expect.verify_lifted_bam(inp, st.out_paths, ixd, cn, rn, window=1000, every=1, threads=8, unassembled_bam=unp)
    assert v["ok"] and v["reads_verified"] == w.n_reads and v["records_verified"] == st.records_out == v["records_in_output"], v
    assert v["unassembled_ok"]
    assert st.batch_device_ms > 0 and st.records_device_ms > 0 and "batch" in st.lift_detail_s
    assert (st.bgzf_device_ms > 0) == device_bgzf
    index.close()
