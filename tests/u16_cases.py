"""The UTF-16 transcoder (tkz_encode_batch_utf16: k_u16_len / k_u16_write / k_u16_docoffs) and the batch decoder (tkz_decode_batch / _device: k_dec_len /
k_dec_write / k_dec_docoffs) at their tile, lane-group and bitmap-word edges: a plain reference in pure Python, the POSITIONED case generators and the comparisons
the emulated (CPU) and the GPU test modules share.  Every comparison is exact equality of ids, bytes and offsets.

The reference restates the operations one element at a time and knows nothing of tiles:
  get_bytes(units)                   Encoding.UTF8.GetBytes on one document's code units (TikTokenizer.cs:261)
  decode_ids(ids, key_of, specials)  TikTokenizer.Decode (TikTokenizer.cs:586-604)

The constants are the kernels' (tests/test_emu_u16_decode.py::test_constants_are_the_kernels reads them back out of the sources):
  TILE        1024   tkz_kernels.hip: kU16Tile, kDecTile -- code units / ids per wavefront
  GROUP         16   tkz_kernels.hip: kU16Lane, kDecLane -- ... per lane; grp_prefix holds one entry per group, the document-offset kernels walk the rest
  WORD          64   tkz_kernels.hip: tkz_u16_lane reads the document-start bitmap as uint64 words (`p0 >> 6`, `p0 & 63`); a lane at bit 48 takes its 17th bit
                     from the next word
  WG_TILES       4   tkz_kernels.h: kThreads = 256, a wavefront a tile (`simt::bid() * (kThreads / 64) + simt::wave()`): 4096 units a workgroup
  DEC_STAGE  12288   tkz_kernels.hip: kDecStage -- k_dec_write stages a tile of up to this many bytes in LDS and stores a larger one directly
  SCAN_BLOCK  1024   tkz_kernels.h: kScanBlock -- tiles per workgroup of k_scan_partials / k_scan_final

The scan of the tile sums.  Both families call launch_scan (tkz_api.cpp: stage_in, decode_device), and launch_scan ALWAYS runs the three kernels k_scan_partials /
k_scan_top / k_scan_final: the switch to the one-kernel k_scan_small (tkz_kernels.hip: kScanSmallMax = 8192 tiles) is in launch_scan2, which the encode path uses
and these two families never do.  So there is no tile count at which these families change their scan, and no k_scan_small side to cover here.  The edge the
three-kernel form does have is SCAN_BLOCK: from 1025 tiles on a second scan workgroup takes part and k_scan_top's sum over the workgroups matters.  A decode batch
of 1025 tiles is a million ids of one or two bytes -- affordable -- so scan_edge_cases() covers 1023, 1024 and 1025 tiles.
"""
import ctypes as C
import functools
import random

import numpy as np

from tokenizer_amd import _native as N

TILE, GROUP, WORD, WG_TILES, DEC_STAGE, SCAN_BLOCK = 1024, 16, 64, 4, 12288, 1024
WG_UNITS = WG_TILES * TILE
HI, LO = 0xD83D, 0xDE00                       # U+1F600 as a pair
SOUP = [0xD800, 0xDBFF, 0xDC00, 0xDFFF, 0xD83D, 0xDE00, 0x41, 0x4E2D, 0xE9]          # parity.check_utf16_batch's alphabet
# ASCII plus a few 2- and 3-byte units: byte offsets differ from unit offsets everywhere.  43 units: a cycle that shares no factor with 16
FILLER = [ord(c) for c in "the quïck bröwn 中文 fox it's 12 €, naïve →x\n"]
assert len(FILLER) == 43 and not any(0xD800 <= u < 0xE000 for u in FILLER)
assert {1, 2, 3} == {len(chr(u).encode("utf-8")) for u in FILLER}


# ---- the plain reference --------------------------------------------------------------------------------------------------------------------------------

def get_bytes(units):
    """Encoding.UTF8.GetBytes, one unit at a time, on the code units of ONE document."""
    out = bytearray()
    n = len(units)
    i = 0
    while i < n:
        u = int(units[i])
        if u < 0x80:
            out.append(u)
        elif u < 0x800:
            out += bytes((0xC0 | (u >> 6), 0x80 | (u & 0x3F)))
        elif 0xD800 <= u < 0xDC00 and i + 1 < n and 0xDC00 <= int(units[i + 1]) < 0xE000:          # a high half followed by a low half inside the document
            c = 0x10000 + ((u - 0xD800) << 10) + (int(units[i + 1]) - 0xDC00)
            out += bytes((0xF0 | (c >> 18), 0x80 | ((c >> 12) & 0x3F), 0x80 | ((c >> 6) & 0x3F), 0x80 | (c & 0x3F)))
            i += 1
        elif 0xD800 <= u < 0xE000:                                                                 # any other surrogate: one U+FFFD per lone half
            out += b"\xEF\xBF\xBD"
        else:
            out += bytes((0xE0 | (u >> 12), 0x80 | ((u >> 6) & 0x3F), 0x80 | (u & 0x3F)))
        i += 1
    return bytes(out)


def python_codec(units):
    """What Python's own codec makes of the same units: the check that keeps get_bytes from drifting."""
    return np.asarray(units, dtype=np.uint16).tobytes().decode("utf-16-le", "replace").encode("utf-8")


def decode_ids(ids, key_of, specials):
    """TikTokenizer.Decode: the vocabulary key or the special literal of each id, joined; an id found in neither contributes nothing; a vocabulary id is never
    shadowed by a special.  key_of: {id: key bytes}; specials: {literal str: id}."""
    literal_of = {int(i): s.encode("utf-8") for s, i in specials.items()}
    out = []
    for i in ids:
        i = int(i)
        b = key_of.get(i)
        if b is None:
            b = literal_of.get(i)
        if b is not None:
            out.append(b)
    return b"".join(out)


# ---- UTF-16 cases -----------------------------------------------------------------------------------------------------------------------------------------

class Case:
    """One batch: a name that says which edge it is, the documents (lists of code units), and -- computed once, shared by every test -- the reference bytes."""

    def __init__(self, name, docs):
        self.name, self.docs = name, [list(d) for d in docs]
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = [get_bytes(d) for d in self.docs]
        return self._ref

    def total(self):
        return sum(len(d) for d in self.docs)

    def __repr__(self):
        return "Case(%s: %d documents, %d units)" % (self.name, len(self.docs), self.total())


def filler(n, phase=0):
    return [FILLER[(phase + i) % len(FILLER)] for i in range(n)]


def flat_to_docs(flat, starts):
    """flat: the batch's units.  starts: the flat position of every document start BEHIND the first one, in order; a position that repeats is an empty document."""
    cuts = [0] + list(starts) + [len(flat)]
    assert all(a <= b for a, b in zip(cuts, cuts[1:])), cuts
    return [flat[a:b] for a, b in zip(cuts, cuts[1:])]


def pair_positions(step=GROUP):
    """The group edges e at which the pair sweep places D83D at e - 1 and DE00 at e: every multiple of `step` up to a workgroup and a bitmap word beyond it, and
    the tile edges up to the fifth."""
    return sorted(set(range(step, WG_UNITS + WORD + 1, step)) | {1024, 2048, 3072, 4096, 5120})


def pair_case(e, kind):
    """D83D at flat position e - 1, DE00 at e.  kind "inside": one document, a pair.  "boundary": a document boundary exactly at e, both halves lone.
    "empty": an EMPTY document at e between the halves."""
    flat = filler(e + 40, phase=e)
    flat[e - 1], flat[e] = HI, LO
    starts = {"inside": [], "boundary": [e], "empty": [e, e]}[kind]
    return Case("pair_across_%d_%s" % (e, kind), flat_to_docs(flat, starts))


PAIR_KINDS = ("inside", "boundary", "empty")


def bitmap_carry_cases():
    """Document starts at flat positions 64k -- the 17th bit of the lane that ends there, carried in from the next bitmap word --, at 64k +- 1 and at 64k - 16;
    a lone low half as the first unit of the new document and a lone high half as the last unit of the old one: both together, and each alone."""
    ks = (1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65)            # 64k is a multiple of 1024 for k = 16, 32, 48, 64; of 4096 for k = 64
    out = []
    for shift, tag in ((0, "64k"), (1, "64k_plus_1"), (-1, "64k_minus_1"), (-GROUP, "64k_minus_16")):
        for halves in ("both", "high_only", "low_only"):
            def put(flat, p):
                if halves != "low_only": flat[p - 1] = HI
                if halves != "high_only": flat[p] = LO
            # every k in one batch ...
            flat = filler(WORD * ks[-1] + 100, phase=shift + 7)
            starts = [WORD * k + shift for k in ks]
            for p in starts: put(flat, p)
            out.append(Case("bitmap_carry_starts_at_%s_%s" % (tag, halves), flat_to_docs(flat, starts)))
            # ... and one boundary alone in its batch where the word edge is a tile edge too (lane 63 of the tile: its `next` comes from global memory)
            for k in (16, 64):
                p = WORD * k + shift
                flat = filler(p + 70, phase=k)
                put(flat, p)
                out.append(Case("bitmap_carry_single_start_at_%d_%s" % (p, halves), flat_to_docs(flat, [p])))
    return out


def ragged_totals():
    """t mod 16 in {1, 2, 15} and t mod 1024 in {1, 15, 16, 17, 1023}: the residues below cover both sets, odd and even totals, on one, two, three and five tiles."""
    res = (1, 2, 15, 16, 17, 18, 1009, 1010, 1023)
    tot = sorted({base + r for base in (0, TILE, 2 * TILE, WG_UNITS) for r in res})
    assert {t % 16 for t in tot} >= {1, 2, 15} and {t % 1024 for t in tot} >= {1, 15, 16, 17, 1023} and any(t % 2 for t in tot) and any(t % 2 == 0 for t in tot)
    return tot


def ragged_tail_cases():
    out = []
    for t in ragged_totals():
        flat = filler(t, phase=t)
        flat[-1] = HI
        out.append(Case("ragged_tail_%d_lone_high_last" % t, [flat, ] if t % 3 else flat_to_docs(flat, [t // 2])))
        if t >= 2:
            flat = filler(t, phase=t + 1)
            flat[-2], flat[-1] = HI, LO
            out.append(Case("ragged_tail_%d_pair_last" % t, [flat] if t % 3 else flat_to_docs(flat, [t // 2])))
    for t in (TILE + 1, 2 * TILE + 1, 3 * TILE + 1, WG_UNITS + 1):
        flat = filler(t, phase=t + 2)
        flat[-2], flat[-1] = HI, LO
        out.append(Case("ragged_tail_%d_low_half_alone_in_last_tile" % t, [flat]))
        out.append(Case("ragged_tail_%d_low_half_alone_in_last_tile_own_document" % t, flat_to_docs(flat, [t - 1])))
    return out


def mid_group_starts_case():
    """Documents of 1..33 units, cycled until the batch passes two tiles: every residue of a start modulo 16 occurs.  Every third document starts with a lone low
    half, every fourth ends with a lone high half that faces a low half across the boundary; empty documents at the front, in the middle and as the last three."""
    docs, n, total = [], 0, 0
    while total <= 2 * TILE + 100:
        ln = n % 33 + 1
        d = filler(ln, phase=total)
        if n % 3 == 0: d[0] = LO
        if docs and len(docs[-1]) and n % 4 == 1 and docs[-1][-1] == HI: d[0] = LO             # (faces the high half the document before ends with)
        if n % 4 == 0 and ln > 1: d[-1] = HI
        docs.append(d)
        total += ln
        n += 1
    assert {sum(len(x) for x in docs[:i]) % GROUP for i in range(len(docs))} == set(range(GROUP))
    assert any(a and b and a[-1] == HI and b[0] == LO for a, b in zip(docs, docs[1:]))
    mid = len(docs) // 2
    docs = [[], []] + docs[:mid] + [[], [], []] + docs[mid:] + [[], [], []]
    return Case("document_starts_at_every_residue_mod_16", docs)


def soup_at_edges_cases(seed=20240611):
    """The soup alphabet in the 4 units either side of every multiple of 16 of a 3-tile batch, filler elsewhere: as one document, and cut into documents at and
    next to group edges."""
    rng = random.Random(seed)
    n = 3 * TILE
    flat = filler(n, phase=3)
    for e in range(0, n + 1, GROUP):
        for q in range(e - 4, e + 4):
            if 0 <= q < n:
                flat[q] = rng.choice(SOUP)
    starts = sorted(rng.choice([e - 1, e, e, e + 1]) for e in rng.sample(range(GROUP, n, GROUP), 40))
    return [Case("surrogate_soup_at_group_edges_one_document", [flat]), Case("surrogate_soup_at_group_edges_cut_at_the_edges", flat_to_docs(flat, starts))]


def pair_sweep_cases(step=GROUP):
    return [pair_case(e, kind) for e in pair_positions(step) for kind in PAIR_KINDS]


@functools.lru_cache(maxsize=None)
def utf16_case_groups(pair_step=GROUP):
    """name of the group -> its cases.  Built once: the reference bytes of a case are shared by every pattern and comparison."""
    return {"pair_sweep": pair_sweep_cases(pair_step), "bitmap_carry": bitmap_carry_cases(), "ragged_tail": ragged_tail_cases(),
            "mid_group_starts": [mid_group_starts_case()], "soup_at_edges": soup_at_edges_cases()}


def pack_units(docs):
    total = sum(len(d) for d in docs)
    flat = np.asarray([u for d in docs for u in d], dtype=np.uint16) if total else np.zeros(0, np.uint16)
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    return flat, offs


def pack_bytes(ref):
    data = np.frombuffer(b"".join(ref), np.uint8) if sum(map(len, ref)) else np.zeros(0, np.uint8)
    offs = np.cumsum([0] + [len(b) for b in ref]).astype(np.int64)
    return data, offs


def first_diff(got, exp):
    n = min(len(got), len(exp))
    for i in range(n):
        if got[i] != exp[i]:
            return i
    return n


def check_utf16_case(enc, oenc, case):
    """The three comparisons of a UTF-16 case.  Returns the number of ids."""
    flat, offs = pack_units(case.docs)
    ref = case.ref
    ids, ooff = enc.encode_batch_utf16(flat, offs)
    ids, ooff = ids.tolist(), ooff.tolist()
    assert len(ooff) == len(case.docs) + 1 and ooff[0] == 0 and ooff[-1] == len(ids), (case, ooff[:4], ooff[-4:], len(ids))
    # (a) every document against the oracle on the reference bytes
    for d, b in enumerate(ref):
        want = oenc.encode_bytes(b)
        got = ids[ooff[d]:ooff[d + 1]]
        assert got == want, "%r (a) document %d (%d units, flat position %d): ids differ at %d: got %s, expected %s" % (
            case, d, len(case.docs[d]), int(offs[d]), first_diff(got, want), got[:8], want[:8])
    # (b) without the oracle: the ids decode to the reference bytes, the byte offsets are their running sum
    back, boffs = enc.decode_batch(np.asarray(ids, np.int32), np.asarray(ooff, np.int64))
    data, eoffs = pack_bytes(ref)
    assert boffs.tolist() == eoffs.tolist(), "%r (b) byte offsets differ at document %d" % (case, first_diff(boffs.tolist(), eoffs.tolist()))
    assert back.tobytes() == data.tobytes(), "%r (b) bytes differ at %d" % (case, first_diff(back.tobytes(), data.tobytes()))
    # (c) the UTF-8 entry fed the reference bytes
    ids8, ooff8 = enc.encode_batch(data, eoffs)
    assert ids == ids8.tolist() and ooff == ooff8.tolist(), "%r (c) differs from encode_batch on the reference bytes" % (case,)
    return len(ids)


def encode_utf16_raw(enc, flat, offs, cap):
    """tkz_encode_batch_utf16 with room for `cap` ids: (status, needed, ids, offsets)."""
    flat = np.ascontiguousarray(flat, np.uint16)
    offs = np.ascontiguousarray(offs, np.int64)
    ids = np.full(max(1, cap), -7, np.int32)
    ooff = np.empty(len(offs), np.int64)
    needed = C.c_int64(0)
    st = enc.lib.L.tkz_encode_batch_utf16(enc._h, flat.ctypes.data, offs.ctypes.data, len(offs) - 1, ids.ctypes.data, cap, ooff.ctypes.data, C.byref(needed))
    return st, needed.value, ids, ooff


def check_utf16_capacity(enc, oenc):
    """out= arrays one id short: E_CAPACITY, `needed` is the reference count; exactly that many: the ids."""
    case = mid_group_starts_case()
    flat, offs = pack_units(case.docs)
    want, woff = [], [0]
    for b in case.ref:
        want += oenc.encode_bytes(b)
        woff.append(len(want))
    assert len(want) > TILE
    st, needed, _, _ = encode_utf16_raw(enc, flat, offs, len(want) - 1)
    assert (st, needed) == (N.E_CAPACITY, len(want)), (st, needed, len(want))
    out = (np.full(len(want) - 1, -7, np.int32), np.empty(len(offs), np.int64))
    try:
        enc.encode_batch_utf16(flat, offs, out=out)
        raise AssertionError("one id short did not raise")
    except N.TkzError as ex:
        assert ex.code == N.E_CAPACITY
    out = (np.full(len(want), -7, np.int32), np.empty(len(offs), np.int64))
    ids, ooff = enc.encode_batch_utf16(flat, offs, out=out)
    assert ids.tolist() == want and ooff.tolist() == woff
    st, needed, ids, ooff = encode_utf16_raw(enc, flat, offs, len(want))
    assert (st, needed) == (N.OK, len(want)) and ids.tolist() == want and ooff.tolist() == woff


def chunk_cut_case(n_units, nchunks, block_len=4099):
    """A batch whose host chunks are cut (plan_host_batch: at the first document start at or behind total / nchunks * k) BETWEEN a document ending in a high half
    and one starting with a low half, 7k units behind the point the host aims at -- so that the units of a chunk are no multiple of 16.  The documents are whole
    repetitions of one filler block (no multiple of a group or a tile) plus a few units, so the reference bytes are the block's bytes repeated: returns
    (docs as uint16 arrays, reference bytes per document, the flat positions of the cuts)."""
    block = filler(block_len, phase=5)
    bref = get_bytes(block)
    ends = [n_units // nchunks * k + 7 * k for k in range(1, nchunks)] + [n_units]
    docs, ref, pos = [], [], 0

    def add(head, reps, tail):
        docs.append(np.asarray(head + block * reps + tail, np.uint16))
        ref.append(get_bytes(head) + bref * reps + get_bytes(tail))
    for k, end in enumerate(ends):
        first = k > 0
        while pos < end:
            head = [LO] if first else []
            reps = 1 + len(docs) % 5
            if end - pos > (reps + 8) * block_len:
                add(head, reps, [])
            else:                                                     # the last document of the chunk takes what is left, and ends in a high half
                reps, extra = divmod(end - pos - len(head), block_len)
                tail = filler(extra, phase=11)
                if k < nchunks - 1:
                    if not tail: reps, tail = reps - 1, list(block)
                    tail[-1] = HI
                add(head, reps, tail)
            pos += len(docs[-1])
            first = False
        assert pos == end
    return docs, ref, ends[:-1]


def check_chunk_cut(enc, O, ovocab, pattern, n_units, nchunks, block_len=4099, threads=1):
    """The batch of chunk_cut_case through tkz_encode_batch_utf16; the expected ids from the reference bytes through the oracle's batch check; the decoded ids
    against the reference bytes and their running sum."""
    docs, ref, cuts = chunk_cut_case(n_units, nchunks, block_len)
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    assert len(cuts) == nchunks - 1
    for k, c in enumerate(cuts, 1):                 # the cut is a document boundary with a high half in front of it and a low half behind it
        d = int(np.searchsorted(offs[:-1], n_units // nchunks * k, side="left"))          # (std::lower_bound over the document starts)
        assert offs[d] == c and int(docs[d - 1][-1]) == HI and int(docs[d][0]) == LO
    assert all((b - a) % GROUP for a, b in zip([0] + cuts, cuts))
    flat = np.concatenate(docs)
    assert len(flat) == n_units
    ids, ooff = enc.encode_batch_utf16(flat, offs)
    data, boffs = pack_bytes(ref)
    assert boffs[-1] > n_units                                   # (byte offsets are not unit offsets)
    bad, first_bad, ntok = O.check_batch(ovocab, pattern, data, boffs, ids, ooff, threads=threads)
    assert (bad, first_bad, ntok) == (0, -1, len(ids)), "%d of %d documents differ from the oracle on the reference bytes, first %d" % (bad, len(docs), first_bad)
    back, back_offs = enc.decode_batch(ids, ooff)
    assert back_offs.tolist() == boffs.tolist() and back.tobytes() == data.tobytes()
    return len(docs), cuts


# ---- decode cases -------------------------------------------------------------------------------------------------------------------------------------------

class DecodeSetup:
    """A vocabulary as the decode cases see it: key_of, the special tokens registered for it (one of them shadowed by a vocabulary id, as parity.check_decode has
    it), and the ids that are in no table."""

    def __init__(self, entries):
        self.key_of = {int(r): k for k, r in entries}
        self.known = sorted(self.key_of)
        self.max_id = self.known[-1]
        self.specials = {"<|endoftext|>": self.max_id + 1, "<|x|>": self.max_id + 20, "shadow": self.known[5]}
        hole = next((i for i in range(self.known[0], self.max_id) if i not in self.key_of), self.max_id + 7)
        # an id in no table, an id above the largest, a negative one, the largest int32, a special's id
        self.strays = [hole, self.max_id + 1000, -3, 2**31 - 1, self.max_id + 1]
        self.by_len = {}
        for i in self.known:
            self.by_len.setdefault(len(self.key_of[i]), []).append(i)

    def expect(self, ids, offs):
        """(bytes, byte offsets) of the reference, document by document."""
        parts = [decode_ids(ids[int(a):int(b)], self.key_of, self.specials) for a, b in zip(offs, offs[1:])]
        return b"".join(parts), np.cumsum([0] + [len(p) for p in parts]).tolist()

    def ordinary(self, n, seed):
        rng = random.Random(seed)
        return [rng.choice(self.known) for _ in range(n)]


class DecodeCase:
    def __init__(self, name, ids, offs):
        self.name, self.ids, self.offs = name, np.asarray(ids, np.int32), np.asarray(offs, np.int64)
        assert self.offs[0] == 0 and self.offs[-1] == len(self.ids) and (np.diff(self.offs) >= 0).all()

    def __repr__(self):
        return "DecodeCase(%s: %d documents, %d ids)" % (self.name, len(self.offs) - 1, len(self.ids))


def residue_cases(S):
    """Document starts at every residue modulo 16 across two tiles; every fifth id a stray.  Shifted five times, so that every kind of stray lands directly in
    front of a document start in some case."""
    out = []
    for shift in range(5):
        n = 2 * TILE + 37
        ids = S.ordinary(n, seed=shift)
        for i in range(shift, n, 5):
            ids[i] = S.strays[(i // 5) % len(S.strays)]
        offs, p, k = [0], 0, 0
        while True:
            p += k % 33 + 1
            k += 1
            if p >= n: break
            offs.append(p)
        offs.append(n)
        assert {o % GROUP for o in offs[:-1]} == set(range(GROUP))
        out.append(DecodeCase("document_starts_at_every_residue_strays_shifted_%d" % shift, ids, offs))
    # an unknown id directly in front of a document start, mid-group: in some case, for every kind of stray that decodes to nothing
    starts_behind = {}
    for c in out:
        for o in c.offs[1:-1].tolist():
            if o % GROUP and int(c.ids[o - 1]) in S.strays[:4]:
                starts_behind.setdefault(int(c.ids[o - 1]), o)
    assert set(starts_behind) == set(S.strays[:4]), starts_behind
    return out


def stage_keys(S):
    """(a, b, longer, shorter): ids of two keys whose lengths sum to 24 (the same key twice when the vocabulary has one of 12 bytes), a key one byte longer than
    the first and one a byte shorter."""
    for la in (12, 11, 13, 10, 14, 9, 15, 8, 16):
        if all(S.by_len.get(n) for n in (la, 24 - la, la + 1, la - 1)):
            return S.by_len[la][0], S.by_len[24 - la][-1], S.by_len[la + 1][0], S.by_len[la - 1][0]
    raise AssertionError("no keys whose lengths sum to 24")


def stage_limit_cases(S):
    """A tile of 1024 ids that decodes to exactly DEC_STAGE bytes, one byte more, one byte fewer -- as the middle tile of three, so both store paths write at a
    non-zero tile base --, document boundaries inside it."""
    a, b, longer, shorter = stage_keys(S)
    out = []
    for tag, swap in (("exactly_12288", None), ("12289", longer), ("12287", shorter)):
        mid = [a, b] * (TILE // 2)
        if swap is not None: mid[600] = swap                           # (an even position: it held `a`)
        nbytes = sum(len(S.key_of[i]) for i in mid)
        assert nbytes == DEC_STAGE + {"exactly_12288": 0, "12289": 1, "12287": -1}[tag]
        ids = S.ordinary(TILE, 1) + mid + S.ordinary(TILE - 9, 2)
        offs = [0, 700, TILE + 5, TILE + 5, TILE + 517, 2 * TILE - 1, 2 * TILE + 3, len(ids)]
        out.append(DecodeCase("stage_limit_middle_tile_of_%s_bytes" % tag, ids, offs))
    return out


def tile_count_cases(S, counts=(1, 3, 4, 5, 9)):
    """Whole and ragged last tiles at tile counts whose last workgroup is partly empty."""
    out = []
    for n in counts:
        for tag, total in (("full", n * TILE), ("last_tile_of_17", (n - 1) * TILE + 17)):
            ids = S.ordinary(total, seed=n)
            step = max(1, total // 7)
            offs = sorted({0, total} | {min(total, k * step + k) for k in range(1, 7)})
            out.append(DecodeCase("tile_count_%d_%s" % (n, tag), ids, offs))
    return out


def scan_edge_cases(S):
    """SCAN_BLOCK - 1, SCAN_BLOCK and SCAN_BLOCK + 1 tiles: where a second workgroup joins the scan of the tile sums (the module docstring).  A block of ids
    repeated, so the reference stays cheap; a stray every 11th id."""
    block = S.ordinary(1021, seed=77)
    for i in range(0, len(block), 11):
        block[i] = S.strays[(i // 11) % len(S.strays)]
    out = []
    for n in (SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1):
        total = (n - 1) * TILE + 3
        ids = np.resize(np.asarray(block, np.int32), total)
        offs = [0, 5, SCAN_BLOCK * TILE // 2 + 9, total - TILE - 1, total - 2, total]
        out.append(DecodeCase("scan_block_edge_%d_tiles" % n, ids, offs))
    return out


def odd_shape_cases(S):
    unknown = [S.strays[k % 4] for k in range(TILE + 50)]
    one_in_last = S.ordinary(2 * TILE + 1, seed=9)
    return [DecodeCase("only_unknown_ids", unknown, [0, 3, 3, 700, TILE + 1, TILE + 50]),
            DecodeCase("last_document_empty_last_tile_holds_one_id", one_in_last, [0, 11, 2 * TILE, 2 * TILE + 1, 2 * TILE + 1])]


def decode_raw(enc, ids, offs, cap):
    """tkz_decode_batch with room for `cap` bytes: (status, needed, bytes, offsets)."""
    ids = np.ascontiguousarray(ids, np.int32)
    offs = np.ascontiguousarray(offs, np.int64)
    out = np.full(max(1, cap), 0xAA, np.uint8)
    ooff = np.empty(len(offs), np.int64)
    needed = C.c_int64(0)
    st = enc.lib.L.tkz_decode_batch(enc._h, ids.ctypes.data if len(ids) else None, offs.ctypes.data, len(offs) - 1, out.ctypes.data, cap, ooff.ctypes.data, C.byref(needed))
    return st, needed.value, out, ooff


def check_decode_case(enc, S, case, device=None):
    """Bytes and offsets against decode_ids; device(ids, offs, cap) -> (bytes, offsets), when given, is a second entry that must agree (the device entry)."""
    want, woffs = S.expect(case.ids, case.offs)
    st, needed, out, ooff = decode_raw(enc, case.ids, case.offs, len(want))                     # (a capacity of exactly the reference length)
    assert (st, needed) == (N.OK, len(want)), (case, st, needed, len(want))
    assert ooff.tolist() == woffs, "%r: byte offsets differ at document %d" % (case, first_diff(ooff.tolist(), woffs))
    assert out[:needed].tobytes() == want, "%r: bytes differ at %d" % (case, first_diff(out[:needed].tobytes(), want))
    out2, ooff2 = enc.decode_batch(case.ids, case.offs)                                          # (the wrapper's own capacity: a hint larger than the result)
    assert out2.tobytes() == want and ooff2.tolist() == woffs, case
    if device is not None:
        out3, ooff3 = device(case.ids, case.offs, len(want) + 3)
        assert ooff3.tolist() == woffs and out3.tobytes() == want, "%r: the device entry differs" % (case,)
    return len(want)


def check_decode_capacity(enc, S, case):
    """out_cap equal to the reference length succeeds (check_decode_case); one byte short: E_CAPACITY, `needed` the reference length; a capacity that cuts inside
    the FIRST tile of three: the same."""
    want, woffs = S.expect(case.ids, case.offs)
    assert len(case.ids) > 2 * TILE
    first_tile = len(decode_ids(case.ids[:TILE], S.key_of, S.specials))
    for cap in (len(want) - 1, first_tile // 2, 0):
        st, needed, _, _ = decode_raw(enc, case.ids, case.offs, cap)
        assert (st, needed) == (N.E_CAPACITY, len(want)), (case, cap, st, needed, len(want))
    check_decode_case(enc, S, case)                                                              # (and the encoder serves the next call as before)


def sparse_vocab_bytes():
    """the sparse rank table the suite already uses (tests/test_emu_kernels.py::test_decode_sparse_rank_table): the decoder table's sorted, binary-searched form"""
    import parity
    return parity.random_vocab_bytes(random.Random(4), alphabet=b"abc", n_keys=200, rank_step=97_003, rank_base=4_200_000)
