"""The encoder of the output BGZF blocks (portello_amd/csrc/deflate.hpp, plo_bgzf_compress_dev) at its own edges.

tests/test_bgzf_dev.py round-trips generic payloads; here every payload is built for one edge of the encoder (tests/deflate_payloads.py)
and the block is taken apart by a tracing decoder (tests/deflate_trace.py), so that a test knows which tokens, code lengths and header
fields the encoder chose: a case that misses its edge fails.  The parts no payload steers freely -- the length limit of the codes at
15 bits, the bit writer at every offset and width, the symbol tables -- are entered directly under the wave emulator.  CPU: emulator,
lane orders, ASan + UBSan.  GPU: every payload through the C ABI against the emulator's bytes, and a call large enough for a persistent
wave to take a second block."""
import functools
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as dc
import deflate_payloads as dp
import deflate_trace as dt
import emu_deflate_lib as edl
from test_bgzf_dev import BLOCK, HDR, _split_blocks, check_block

ORDERS = (0, 1, 4711)
CASES = {c.name: c for c in dp.CASES}


@functools.lru_cache(maxsize=None)
def emu(payload, level, seed=0):
    rc, blk = edl.deflate_block(payload, level, seed)
    assert rc == 0, rc
    return blk


def stored_form(p):
    """the level-0 block of p, written out from RFC 1951 3.2.4 and the BGZF header the host writer emits"""
    return HDR + struct.pack("<HBHH", 18 + 5 + len(p) + 8 - 1, 1, len(p), len(p) ^ 0xFFFF) + p + struct.pack("<II", zlib.crc32(p) & 0xFFFFFFFF, len(p))


def reencode(blocks):
    """the traced blocks written again by the stream builder of the decoder's tests: header fields, code-length sequence, code lengths
    and tokens as traced must give the stream bit for bit"""
    s = dc.Stream()
    for b in blocks:
        toks = [dc.match(*t) if isinstance(t, tuple) else dc.lit(t) for t in b.tokens] + [dc.EOB]
        if b.btype == 0:
            s.stored(b.stored, bool(b.final))
        elif b.btype == 1:
            s.fixed(toks, bool(b.final))
        else:
            s.dynamic(b.ll_lengths, b.d_lengths, toks, bool(b.final), cl_lengths=b.cl_lengths, cl_sequence=b.cl_seq)
    return s.getvalue()


def replay(tokens, out=None):
    """the tokens applied one by one, onto the output so far where a stream has blocks in front"""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


def replay_blocks(blocks):
    out = bytearray()
    for b in blocks:
        if b.btype == 0:
            out += b.stored
        else:
            replay(b.tokens, out)
    return bytes(out)


# ---- the tracer against zlib ---------------------------------------------------------------------------------------------------------------
def _zlib_payloads():
    rng = np.random.default_rng(8)
    text = b"@read/%d/ccs\tACGTTGCA\tRG:Z:x\tnp:i:12\n" * 300
    return [b"", b"a", b"abc" * 5, b"\0" * 70000, text, bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 50000)),
            bytes(rng.integers(0, 4, 9000, dtype=np.uint8)) + text[:9000] + bytes(rng.integers(0, 256, 20000, dtype=np.uint8)), dp.far(32768), dp.counter(6000),
            CASES["all_length_symbols_and_distance_codes"].payload, bytes(rng.integers(32, 96, 30000, dtype=np.uint8)), dp.zero_runs_a()]


@pytest.mark.parametrize("level", [1, 6, 9])
def test_the_tracer_replays_zlib_streams_token_by_token(level):
    kinds = set()
    for p in _zlib_payloads():
        c = zlib.compressobj(level, zlib.DEFLATED, -15)  # (default strategy: fixed blocks where zlib prefers them, never forced)
        data = c.compress(p) + c.flush()
        blocks, out, bits = dt.trace_stream(data)
        assert out == p and (bits + 7) // 8 == len(data)
        assert replay_blocks(blocks) == p
        assert reencode(blocks) == data
        kinds |= {b.btype for b in blocks}
        for b in blocks:
            if b.btype == 2:
                lf, df, cf = b.histograms()
                assert all((f > 0) <= (l > 0) for f, l in zip(lf, b.ll_lengths + [0] * 30)) and all((f > 0) <= (l > 0) for f, l in zip(df, b.d_lengths + [0] * 30))
    assert kinds == {0, 1, 2}


def test_the_yardsticks_of_a_huffman_code():
    assert (dt.unlimited_depth([]), dt.optimal_cost([0, 0])) == (0, 0) and (dt.unlimited_depth([0, 9]), dt.optimal_cost([0, 9])) == (1, 9)
    assert (dt.unlimited_depth([1, 1, 2, 3, 5, 8]), dt.optimal_cost([1, 1, 2, 3, 5, 8])) == (5, 1 * 5 + 1 * 5 + 2 * 4 + 3 * 3 + 5 * 2 + 8)
    assert dt.unlimited_depth([1] * 8) == 3 and dt.unlimited_depth([1, 1, 1, 1, 2, 2]) == 3  # the shallowest of the optimal trees (the deepest: 4)
    assert dt.optimal_cost([5, 0, 5, 5, 5]) == 40


# ---- the crafted payloads under the emulator -------------------------------------------------------------------------------------------------
def check_trace(case, blk):
    """the case's condition on the traced block, the block from its trace, its size against the stored form and the best possible codes"""
    p = case.payload
    tr, out = dt.trace_block(blk[18:-8])
    assert out == p and tr.final == 1
    assert reencode([tr]) == blk[18:-8]
    if case.stored:
        assert tr.btype == 0 and blk == stored_form(p)
        return tr
    if case.cond is not None:
        case.cond(dp.View(tr, case.start, len(case.core)), case.core)
    if tr.btype == 0:
        assert blk == stored_form(p)
        return tr
    assert tr.btype == 2 and len(blk) < 18 + 5 + len(p) + 8 and tr.widest <= 48
    assert replay(tr.tokens) == p
    lf, df, cf = tr.histograms()
    for freq, lengths, limit, what in ((lf, tr.ll_lengths, 15, "literal/length"), (df, tr.d_lengths, 15, "distance"), (cf, tr.cl_lengths, 7, "code-length")):
        lengths = lengths + [0] * (len(freq) - len(lengths))
        assert max(lengths) <= limit and all(l > 0 for f, l in zip(freq, lengths) if f), what
        if dt.unlimited_depth(freq) <= limit:  # no limit in the way: a Huffman code, nothing dearer
            assert dt.cost(freq, lengths) == dt.optimal_cost(freq), (what, dt.cost(freq, lengths), dt.optimal_cost(freq))
        else:  # the limit hit: a PIN of deflate.hpp's halving rule, not a correctness oracle (see check_code below)
            w = list(freq)
            while dt.unlimited_depth(w) > limit:
                w = [(x + 1) >> 1 for x in w]
            assert dt.cost(w, lengths) == dt.optimal_cost(w), what
    return tr


@pytest.mark.parametrize("name", list(CASES))
def test_crafted_payload_under_the_emulator(name):
    case = CASES[name]
    p = case.payload
    blk = emu(p, 1)
    check_block(blk, p)
    for seed in ORDERS[1:]:
        assert emu(p, 1, seed) == blk, seed
    check_trace(case, blk)
    b0 = emu(p, 0)
    assert b0 == stored_form(p) and all(emu(p, 0, seed) == b0 for seed in ORDERS[1:])
    check_block(b0, p)
    assert len(blk) <= len(b0)


def test_the_catalogue_is_complete():
    """every edge of the list has its case, and the cases are as short as their edges allow"""
    for want in ["far_32767", "far_32768", "far_32769", "three_at_4096", "three_at_4097", "four_at_4097", "source_at_0", "source_in_the_last_64_bytes",
                 "match_ends_the_payload", "last_two_unhashed", "last_one_unhashed", "one_byte_x3", "one_byte_x4", "one_byte_x5", "match_at_lane_63_and_lane_0",
                 "match_from_lane_10_skips_a_round", "match_under_an_earlier_match", "acgt_129", "acgt_191", "acgt_192", "bucket_evicted_by_a_collision",
                 "candidate_fails_distance_1_holds", "one_hash_from_64_lanes", "empty", "one_literal", "one_literal_kind_one_distance_code_0",
                 "no_match_in_a_dynamic_block", "one_distance_code_13", "all_length_symbols_and_distance_codes", "hclen_trimmed", "code_length_code_limited_far_32769",
                 "zero_runs_2_3_10_11_138", "zero_run_139", "text_1_stored", "text_2_stored", "text_40_stored", "random_300_stored", "dynamic_wins_by_at_most_8_bytes"] + [
                 f"{k}_{L}" for k in ("run", "repeat") for L in (3, 4, 10, 11, 12, 18, 19, 130, 131, 257, 258, 259, 516, 517)] + [
                 f"code_length_code_limited_seed_{s}" for s in dp.CL_LIMIT_SEEDS]:
        assert want in CASES, want
    assert len(dp.CL_LIMIT_SEEDS) == 2
    assert sum(len(c.payload) < 8192 for c in dp.CASES) >= len(dp.CASES) - 9


# ---- direct entries: def_build_code -------------------------------------------------------------------------------------------------------------
def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _spread(counts, nsym, seed):
    """the counts on symbols picked by a seeded shuffle"""
    freq = [0] * nsym
    for s, c in zip(np.random.default_rng(seed).permutation(nsym)[:len(counts)], counts):
        freq[int(s)] = c
    return freq


def code_tables():
    t = [(f"fibonacci_{k}_of_286", _spread(_fib(k), 286, k), 15) for k in range(16, 25)]
    t.append(("ones_286", [1] * 286, 15))
    for nsym in (286, 30, 19):
        limit = 7 if nsym == 19 else 15
        t += [(f"none_of_{nsym}", [0] * nsym, limit), (f"symbol_0_of_{nsym}", [7] + [0] * (nsym - 1), limit), (f"symbol_5_of_{nsym}", [0] * 5 + [7] + [0] * (nsym - 6), limit),
              (f"symbols_0_7_of_{nsym}", [3] + [0] * 6 + [9] + [0] * (nsym - 8), limit), (f"symbols_3_9_of_{nsym}", [0] * 3 + [1] + [0] * 5 + [1] + [0] * (nsym - 10), limit)]
    t.append(("one_of_65280_beside_ones", [1] * 100 + [65280] + [1] * 185, 15))
    t.append(("powers_of_two_16", _spread([1 << i for i in range(16)], 286, 1), 15))  # depth 15: just fits
    t.append(("powers_of_two_17", _spread([1 << i for i in range(17)], 286, 2), 15))  # depth 16
    t.append(("powers_of_two_22", _spread([1 << i for i in range(22)], 286, 3), 15))
    for k in range(9, 13):
        t += [(f"fibonacci_{k}_of_30_limit_15", _spread(_fib(k), 30, k), 15), (f"fibonacci_{k}_of_30_limit_7", _spread(_fib(k), 30, 50 + k), 7),
              (f"fibonacci_{k}_of_19_limit_7", _spread(_fib(k), 19, k), 7), (f"fibonacci_{k}_of_19_limit_15", _spread(_fib(k), 19, 70 + k), 15)]
    return t


TABLES = {name: (freq, limit) for name, freq, limit in code_tables()}


def check_code(freq, limit, lengths, codes):
    used = [s for s, f in enumerate(freq) if f]
    coded = [s for s, l in enumerate(lengths) if l]
    assert max(lengths) <= limit
    assert sum(1 << (limit - l) for l in lengths if l) == 1 << limit, "Kraft sum"
    if len(used) >= 2:
        assert coded == used
    elif len(used) == 1:  # the added symbol: 0, or 1 where 0 is the one in use
        assert coded == sorted(used + [1 if used[0] == 0 else 0])
    else:
        assert coded == [0, 1]
    for a in used:
        for b in used:
            assert not (freq[a] > freq[b] and lengths[a] > lengths[b]), (a, b)
    assert codes == [dc._reverse(c, l) for c, l in zip(dc.canonical(lengths), lengths)]
    if dt.unlimited_depth(freq) <= limit:
        assert dt.cost(freq, lengths) == dt.optimal_cost(freq)
        return None
    # The limit was hit.  What follows is a PIN of the implementation's rule, not a correctness oracle: it restates deflate.hpp's halving
    # (the counts halved, rounding up, until the tree fits) and asks that the code be a Huffman code of the counts so halved.  Any code
    # within the limit with Kraft sum 1 would be a correct one; the properties above are what correctness needs.  The pin also assumes
    # that the heap tree and the encoder's two-queue tree exceed the limit for the same counts, so that both halve equally often; that
    # holds on every table and payload here and is not proven.  If the encoder's rule changes on purpose, this check changes with it.
    w = list(freq)
    while dt.unlimited_depth(w) > limit:
        w = [(x + 1) >> 1 for x in w]
    assert dt.cost(w, lengths) == dt.optimal_cost(w), "not a Huffman code of the counts halved with rounding up"
    return dt.cost(freq, lengths) / dt.optimal_cost(freq)


@pytest.mark.parametrize("name", list(TABLES))
def test_def_build_code(name):
    freq, limit = TABLES[name]
    lengths, codes = edl.build_code(freq, limit)
    for seed in ORDERS[1:]:
        assert edl.build_code(freq, limit, seed) == (lengths, codes), seed
    ratio = check_code(freq, limit, lengths, codes)
    depth = dt.unlimited_depth(freq)
    if name.startswith("fibonacci") and "_of_286" in name:
        assert depth == int(name.split("_")[1]) - 1 and (ratio is not None) == (depth > 15)  # 17 terms and more: the 15-bit branch that no payload reaches
    if ratio is not None:
        print(f"{name}: unlimited depth {depth}, limit {limit}, cost / optimal cost = {ratio:.4f}")


def test_worst_cost_of_a_limited_code():
    """printed, not asserted: how much dearer than the unlimited Huffman code the halving loop's code is, at worst over the tables"""
    worst = None
    for name, (freq, limit) in TABLES.items():
        if dt.unlimited_depth(freq) > limit:
            lengths, _ = edl.build_code(freq, limit)
            r = dt.cost(freq, lengths) / dt.optimal_cost(freq)
            worst = max(worst or (0, ""), (r, name))
    print(f"worst limited-code cost ratio: {worst[0]:.4f} ({worst[1]})")
    assert worst is not None


# ---- direct entries: def_put ---------------------------------------------------------------------------------------------------------------------
WIDTHS = (0, 1, 31, 32, 33, 47, 48)


def _call(rng, widths):
    return [(int(rng.integers(0, 1 << 62)) & ((1 << w) - 1), int(w)) for w in widths]


def put_sequences():
    rng = np.random.default_rng(12)
    seqs = []
    for start in range(32):  # the open word holds `start` bits when the wide calls come
        first = [(int(rng.integers(0, 1 << 31)) & ((1 << start) - 1), start)] + [(0, 0)] * 63
        seqs.append([first, _call(rng, rng.choice(WIDTHS, 64)), [(0, 0)] * 64, _call(rng, rng.choice(WIDTHS, 64)), _call(rng, [48] * 64), [(0, 0)] * 64,
                     _call(rng, [1] * 64), _call(rng, rng.choice(WIDTHS, 64))])
    seqs.append([[(1, 31)] + [(0, 0)] * 63, [((1 << 48) - 1, 48)] * 64, [(1, 1)] * 64])  # 31 carried bits and 64 x 48: all that DEF_OBUF_WORDS is sized for
    seqs.append([[(0, 0)] * 64] * 3)
    return seqs


def check_put(calls, got, cap_words=None):
    words, bits, open_word = got
    w = dc.BitWriter()
    for call in calls:
        for v, nb in call:
            w.bits(v, nb)
    assert bits == w.bit_length()
    want = w.getvalue() + b"\0" * 4
    nfull = bits // 32
    kept = nfull if cap_words is None else min(nfull, cap_words)
    assert words[:4 * kept] == want[:4 * kept]
    assert words[4 * kept:] == b"\0" * (len(words) - 4 * kept)  # nothing behind the written words (and nothing behind cap_words: emu_deflate_lib.put)
    assert open_word == struct.unpack_from("<I", want, 4 * nfull)[0] & ((1 << (bits & 31)) - 1)


def test_def_put_at_every_offset_and_width():
    for i, calls in enumerate(put_sequences()):
        nwords = sum(nb for call in calls for _, nb in call) // 32
        for seed in ORDERS:
            check_put(calls, edl.put(calls, nwords + 2, seed))
        if nwords:  # a stream one word short: what fits is right, the last word is not written anywhere
            check_put(calls, edl.put(calls, nwords - 1, 1), nwords - 1)


def test_symbol_tables_exhaustively():
    lens, dists, extra = edl.symbols()
    for l in range(3, 259):
        s, ev, eb = dc.length_symbol(l)
        assert tuple(int(x) for x in lens[l - 3]) == (s - 257, eb, ev), l
    want = np.array([(lambda t: (t[0], t[2], t[1]))(dc.dist_symbol(d)) for d in range(1, 32769)], np.uint32)
    assert np.array_equal(dists, want)
    assert [int(x) for x in extra] == dc.LEN_EXTRA + dc.DIST_EXTRA


def test_sanitizer_program_over_the_catalogue(tmp_path):
    """ASan + UBSan (CPU): every crafted payload, slot and token buffer in a heap block of its exact size, then the tables and the put calls"""
    tables, seqs = list(TABLES.values()), put_sequences()
    jobs = b"".join(edl.job_payload(c.payload) for c in dp.CASES) + b"".join(edl.job_table(f, lim) for f, lim in tables)
    caps = [sum(nb for call in calls for _, nb in call) // 32 for calls in seqs]
    jobs += b"".join(edl.job_put(calls, cap) for calls, cap in zip(seqs, caps))
    rc, err, res = edl.run_asan_jobs(jobs, 1, str(tmp_path))
    assert rc == 0, (rc, err[-3000:])
    assert len(res) == len(dp.CASES) + len(tables) + len(seqs)
    for c, r in zip(dp.CASES, res):
        assert r == emu(c.payload, 1), c.name
    for (freq, limit), r in zip(tables, res[len(dp.CASES):]):
        lengths, codes = edl.build_code(freq, limit)
        assert r == bytes(lengths) + struct.pack(f"<{len(codes)}H", *codes)
    for calls, cap, r in zip(seqs, caps, res[len(dp.CASES) + len(tables):]):
        words, bits, open_word = edl.put(calls, cap)
        assert r == words + struct.pack("<II", bits, open_word)


# ---- a wave's second block: the shapes, on the CPU -----------------------------------------------------------------------------------------------
CYCLE = 7


@functools.lru_cache(maxsize=None)
def cycle():
    ps = dp.full_size_cycle()
    assert len(ps) == CYCLE and all(len(p) == BLOCK for p in ps)
    return ps, [emu(p, 1) for p in ps]


def second_block_shape(n_cus):
    # COUPLED to plo_bgzf_compress_dev (engine.hip): resident workgroups per CU by LDS, four waves each; a change there moves the shape at
    # which a wave takes a second block, and this formula has to move with it
    per_cu = (160 << 10) // (edl.lib().emu_bgzf_work_bytes() * 4 + 1024)
    waves = n_cus * per_cu * 4
    return waves, waves + waves // 12 + 5


def test_the_cycle_of_full_size_payloads():
    ps, blocks = cycle()
    for p, b in zip(ps, blocks):
        check_block(b, p, project=False)  # (generic payloads: the project's decoder takes their like in tests/test_bgzf_dev.py)
    units = []
    for b in blocks:
        tr, _ = dt.trace_block(b[18:-8])
        units.append(len(tr.tokens) + len(tr.matches()))
    print("token units of the cycle:", units)
    assert min(units) < 600 and max(units) > 60000  # very different shares of a wave's token buffer
    for n_cus in (256, 304, 64):  # (whatever the device has: the GPU test asserts the same on its own count)
        waves, n = second_block_shape(n_cus)
        assert waves % CYCLE != 0, "a wave's second payload would be its first again"
        off = np.concatenate([[0], np.cumsum([len(blocks[b % CYCLE]) for b in range(n)])])
        assert len(set(int(x) % 16 for x in off[:-1])) >= 8


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------------
class DevCompressor:
    """payloads through Engine.bgzf_compress_dev, the context built as test_index_dev.DevIndexer builds its own"""

    def __init__(self):
        import torch

        import test_records_dev as trd
        from portello_amd import api

        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.index = api.Index(trd.hand_index(), 0)
        self.eng = api.Engine(self.index)

    def upload(self, data):
        t = self.torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(self.dev)
        self.torch.cuda.synchronize()
        return t

    def compress(self, ptr, n, level):
        bo = self.eng.bgzf_compress_dev(ptr, n, level)
        nb = int(bo.n_blocks)
        assert int(bo.n_in) == n and nb == (n + BLOCK - 1) // BLOCK
        off = self.eng.download(bo.block_off, np.uint64, nb + 1).astype(np.int64)
        assert off[0] == 0 and int(off[-1]) == int(bo.n_bytes)
        return off, self.eng.download(bo.blocks, np.uint8, int(bo.n_bytes)).tobytes()

    def close(self):
        self.eng.close()
        self.index.close()


@pytest.fixture(scope="module")
def devc():
    d = DevCompressor()
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1])
def test_crafted_payloads_on_the_device(devc, level):
    """one call per payload; the payloads lie side by side in one device buffer, so their addresses are odd and even as their lengths fall"""
    data = b"\xaa" + b"".join(c.payload for c in dp.CASES) + b"\xbb" * 16
    buf = devc.upload(data)
    at, odd = 1, 0
    for c in dp.CASES:
        n = len(c.payload)
        odd += (buf.data_ptr() + at) & 1
        off, blocks = devc.compress(buf.data_ptr() + at, n, level)
        if n == 0:
            assert len(off) == 1 and blocks == b""
        else:
            assert len(off) == 2 and blocks == emu(c.payload, level), c.name
            check_block(blocks, c.payload, project=False)
        at += n
    assert odd >= 10
    assert buf.cpu().numpy().tobytes() == data  # the input is unchanged


@pytest.mark.gpu
def test_a_waves_second_block_on_the_device(devc):
    """More blocks than resident waves, level 1: every wave of the first twelfth takes a second block into the token buffer its first one
    filled, and reads the tokens back through load_written.  A cycle of seven payloads, the number of waves no multiple of seven."""
    t = devc.torch
    ps, want = cycle()
    waves, n = second_block_shape(t.cuda.get_device_properties(0).multi_processor_count)
    assert waves % CYCLE != 0 and n > waves
    # the shape on the emulator's sizes for this device's own CU count first, so that the device is not what fails it
    emu_off = np.concatenate([[0], np.cumsum([len(want[b % CYCLE]) for b in range(n)])])
    assert len(set(int(x) % 16 for x in emu_off[:-1])) >= 8
    short = ps[2][:12345]
    base = devc.upload(b"".join(ps)).view(CYCLE, BLOCK)
    big = t.cat([base[t.arange(n, device=devc.dev) % CYCLE].reshape(-1), devc.upload(short)])
    t.cuda.synchronize()
    assert big.numel() == n * BLOCK + len(short)
    off, blocks = devc.compress(big.data_ptr(), big.numel(), 1)
    assert len(off) == n + 2 and np.all(np.diff(off) > 0)
    view = memoryview(blocks)
    for b in range(CYCLE):  # the first block of every payload is the emulator's ...
        assert view[off[b]:off[b + 1]] == want[b], b
    for b in range(n):      # ... and every later one equals it
        assert view[off[b]:off[b + 1]] == want[b % CYCLE], (b, b % CYCLE, b >= waves)
    assert view[off[n]:off[n + 1]] == emu(short, 1)
    assert np.array_equal(off[:n + 1], emu_off) and len(set(int(x) % 16 for x in off[:-1])) >= 8  # (behind the bytes: the more telling failure first)
    for b in range(n + 1):
        p = ps[b % CYCLE] if b < n else short
        assert zlib.decompress(view[off[b] + 18:off[b + 1] - 8], -15) == p, b
    del view
    # a small call on the same context, whose buffers have grown: three blocks from an odd address
    off, blocks = devc.compress(big.data_ptr() + 3 * BLOCK + 1, 2 * BLOCK + 77, 1)
    host = ps[3][1:] + ps[4] + ps[5][:78]
    assert _split_blocks(blocks) == [emu(host[k:k + BLOCK], 1) for k in range(0, len(host), BLOCK)]
