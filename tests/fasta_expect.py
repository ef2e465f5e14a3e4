"""The FASTA rule of include/portello_liftover.h (plo_fasta_*) restated in plain Python, a line at a time, from the header's text and not from
the device code: what the loader must give for any bytes.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from dataclasses import dataclass, field

ERR_NONE, ERR_BAD_BYTE, ERR_NO_HEADER, ERR_MISSING, ERR_LENGTH, ERR_DUPLICATE = 0, 1, 2, 3, 4, 5
ALIGN, MIN_SLOT = 256, 16


@dataclass
class Expect:
    err_kind: int = ERR_NONE
    err_offset: int = 0
    err_chrom: int = 0
    err_len: int = 0
    ids: list = field(default_factory=list)    # every record of the text, file order (bytes)
    lens: list = field(default_factory=list)
    offs: list = field(default_factory=list)   # file offset of every header line
    seqs: list = field(default_factory=list)   # their upper-cased sequences (bytes)
    n_bases: int = 0
    chrom_len: list = field(default_factory=list)  # what is handed out (empty for a refused load)
    chrom_seq: list = field(default_factory=list)


def parse(text: bytes):
    """-> (records [(id, offset of '>', bytearray)], lowest refused byte or None, its kind, bases counted up to the refusal or the end)"""
    recs, at, n_bases = [], 0, 0
    n = len(text)
    while at < n:
        end = text.find(b"\n", at)
        end = n if end < 0 else end  # the last line may lack its '\n'
        line = text[at:end]
        if line[:1] == b">":
            k = 1
            while k < len(line) and line[k] not in b" \t\r":
                k += 1
            recs.append((bytes(line[1:k]), at, bytearray()))
        else:
            for k, b in enumerate(line):
                if b in b"\r \t":
                    continue
                if 65 <= b <= 90 or 97 <= b <= 122:
                    if not recs:
                        return recs, at + k, ERR_NO_HEADER, n_bases
                    recs[-1][2].append(b & 0xDF)
                    n_bases += 1
                else:
                    return recs, at + k, ERR_BAD_BYTE, n_bases
        at = end + 1
    return recs, None, ERR_NONE, n_bases


def slot_bytes(length: int) -> int:
    return (max(length, MIN_SLOT) + ALIGN - 1) // ALIGN * ALIGN


def load(text: bytes, want_names=None, want_lens=None) -> Expect:
    recs, bad, kind, n_bases = parse(text)
    e = Expect()
    if kind:  # 1. the lowest refused byte of the text
        e.err_kind, e.err_offset = kind, bad
        return e
    e.ids = [r[0] for r in recs]
    e.offs = [r[1] for r in recs]
    e.seqs = [bytes(r[2]) for r in recs]
    e.lens = [len(s) for s in e.seqs]
    e.n_bases = n_bases
    if want_names is None:
        e.chrom_len, e.chrom_seq = list(e.lens), list(e.seqs)
        return e
    want = [w if isinstance(w, bytes) else w.encode() for w in want_names]
    first = {}
    for i, rid in enumerate(e.ids):  # 2. a wanted id on a second header line: the lowest such line
        if rid in want:
            if rid in first:
                e.err_kind, e.err_offset, e.err_chrom, e.err_len = ERR_DUPLICATE, e.offs[i], want.index(rid), e.lens[first[rid]]
                return e
            first[rid] = i
    for w, (name, length) in enumerate(zip(want, want_lens)):  # 3. the lowest place in the list that is missing or of another length
        if name not in first:
            e.err_kind, e.err_chrom = ERR_MISSING, w
            return e
        if e.lens[first[name]] != length:
            e.err_kind, e.err_chrom, e.err_len, e.err_offset = ERR_LENGTH, w, e.lens[first[name]], e.offs[first[name]]
            return e
    e.chrom_len = list(want_lens)
    e.chrom_seq = [e.seqs[first[name]] for name in want]
    return e


def want_index(e: Expect, want_names):
    """the place of every record of the text in the wanted list (-1: none; without a list its own number)"""
    if want_names is None:
        return list(range(len(e.ids)))
    want = [w if isinstance(w, bytes) else w.encode() for w in want_names]
    return [want.index(r) if r in want else -1 for r in e.ids]
