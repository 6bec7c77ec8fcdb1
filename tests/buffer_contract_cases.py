"""The device entries on the CALLER'S buffers (tkz.h: d_bytes is 16-byte aligned and total_bytes long, no padding is asked for; out_cap ids may be written and no
more; on TKZ_E_CAPACITY *total_tokens is the needed size): the cases and comparisons the emulated (CPU) and the GPU test modules share.  Every comparison is exact.

What the other suites hold fixed is varied here: what lies in front of and behind every buffer, the address phase of every pointer, and the capacity.

  Arena      one logical buffer inside a larger allocation of the test's own: at least GUARD = 4 KiB in front of it and behind it, the buffer at a chosen phase of
             its REAL address.  The guards of an output hold a sentinel (-7 as int32, -5 as int64, as the other suites fill their outputs), those of an input the
             case's poison byte (an offset array: the int64 sentinel).  After the call it reports the payload, whether both guards are intact and whether
             [result_end, capacity) still holds the sentinel.  A stray store lands in the test's own memory and is a failed assertion: no case passes a bad pointer.
  TEXTS      the smallest batches (a few sub-tiles of SUB = 1,024 bytes, at most 8 KiB, several documents, an empty one among them) that reach every store path of
             k_place: built by the generators of place_pipeline_cases, count_cases and docmark_cases on place_pipeline_cases' table (the 256 single bytes and three
             words: what a piece costs is known by construction).
  ENTRIES    every *_device entry of tkz.h.  Expected values are the oracle's, through the models of spans_cases.Ctx (ids, offsets, byte and unit starts),
             chunk_cases.Expected, trim_cases.Expect and u8_decode_cases.get_string: computed once per text, shared by the whole matrix.
  the matrix output phase x capacity in full for every entry and text (rows()); poison x input phase in full for the plain entry and the UTF-16 decoder
             (input_rows()); the other axes ride along by PAIRWISE, a fixed table -- nothing is sampled.
  text ends  a text that ends 0..15 bytes into the trailing row a block of k_pretok_rows stages (tkz_pretok_request: `inside`, but tpos + 16 > total), with a
             multi-byte tail across that point: through tkz_pretokenize_utf8 and through tkz_encode_batch_device in the arena.

What no capacity reaches: k_tokspan_write's `o >= S.out_cap` and tkz_chunk_emit's `o >= C.chunk_cap` sit behind the kernels' own `*grand > out_cap` / `nch >
chunk_cap` returns (a call that does not fit leaves those tables alone), and the bytes tkz_pretok_request stages behind the block feed lane 63 only, whose row is
context: a change of either is not visible in any buffer, with whatever poison.

`upload(np_array) -> (owner, pointer)` and `back(owner)` as in count_cases.Ctx: identity for the emulated build, a device tensor on the hardware; store(owner, image)
writes an image into an allocation that exists already (its address is known only then).
"""
import ctypes as C
import functools
import random
import re

import numpy as np

import chunk_cases as CH
import count_cases as CC
import parity
import place_pipeline_cases as PP
import spans_cases as SP
import special_cases as SC
import test_pretok_classify as TPC
import trim_cases as TR
import u8_decode_cases as U8
from tokenizer_amd import _native as N

SUB = PP.SUB
GUARD = 4096
EOT = SC.EOT
EOT_ID = 300                                            # outside the table's 259 ranks
SPECIALS = {EOT: EOT_ID}
ID_SENTINEL, I64_SENTINEL = np.int32(-7), np.int64(-5)
BYTE_SENTINEL, UNIT_SENTINEL = np.uint8(0xA5), np.uint16(0xAAAA)
POISONS = (0x00, ord("a"), ord(" "), ord("7"), ord("\n"), 0x80, 0xE4, 0xFF)
BYTES_PHASES = (0, 16, 32, 48)                          # d_bytes: mod 64 (16-byte aligned, as tkz.h asks)
IDS_IN_PHASES = (0, 4, 8, 12)                           # the decoders' d_ids: mod 16
I64_PHASES = (0, 8)                                     # every int64 array, in or out: mod 16
IDS_OUT_PHASES = (0, 4, 8, 12)                          # d_out_ids (and the span arrays): mod 16
U8_OUT_PHASES = (0, 1, 6, 11)                           # the UTF-8 decoder's bytes: mod 16
U16_OUT_PHASES = (0, 2, 6, 14)                          # the UTF-16 decoder's units: mod 16
CHUNK_MAX = 50                                          # the chunk entry's budget
TRIM_MAX = 40                                           # the trim entries' maximum, for every document


# ---- 1. the arena ------------------------------------------------------------------------------------------------------------------------------------------

class Memory:
    """the transport: count_cases.Ctx's upload / back hooks, and a store into an allocation that exists"""

    def __init__(self, upload=None):
        self.upload = upload or (lambda arr: (arr, arr.ctypes.data))

    back = staticmethod(CC.Ctx.back)

    @staticmethod
    def store(owner, image):
        if hasattr(owner, "copy_"):
            import torch
            owner.copy_(torch.from_numpy(image))
        else:
            owner[:] = image


class Arena:
    """`n` entries of `dtype` at an address that is `phase` mod `mod`, inside an allocation of the test's own; `guard` (a numpy scalar) fills everything around
    them -- and the entries themselves, unless `data` is given (an input).  spill: bytes by which the guard behind is longer than GUARD -- an output whose capacity is
    short gets room for its whole result behind it, so that a kernel that ignored the capacity altogether would still write into this allocation."""

    def __init__(self, mem, dtype, n, phase, mod, guard, data=None, spill=0):
        self.mem, self.dtype, self.n = mem, np.dtype(dtype), int(n)
        self.nbytes = self.n * self.dtype.itemsize
        assert phase % self.dtype.itemsize == 0 and 0 <= phase < mod
        size = GUARD + mod + self.nbytes + GUARD + int(spill)
        self.owner, base = mem.upload(np.zeros(size, np.uint8))
        self.off = GUARD + (phase - (base + GUARD)) % mod            # from the REAL address
        self.ptr = base + self.off
        assert self.ptr % mod == phase and self.off >= GUARD and size - self.off - self.nbytes >= GUARD
        pat = np.frombuffer(np.asarray(guard).tobytes(), np.uint8)
        self.image = pat[(np.arange(size) - self.off) % len(pat)]        # the guard's pattern, lined up with the payload's entries
        self.is_input = data is not None
        if self.is_input:
            data = np.ascontiguousarray(data, self.dtype)
            assert len(data) == self.n
            self.image[self.off:self.off + self.nbytes] = np.frombuffer(data.tobytes(), np.uint8)
        mem.store(self.owner, self.image)
        self.payload = self.front_ok = self.behind_ok = self.now = None

    def read(self):
        """after the call: fetches the allocation.  payload: the n entries; front_ok / behind_ok: the guards are what they were"""
        self.now = np.array(self.mem.back(self.owner), copy=True).view(np.uint8)
        end = self.off + self.nbytes
        self.front_ok = bool((self.now[:self.off] == self.image[:self.off]).all())
        self.behind_ok = bool((self.now[end:] == self.image[end:]).all())
        self.payload = np.frombuffer(self.now[self.off:end].tobytes(), self.dtype)
        return self

    @property
    def guards_ok(self):
        return self.front_ok and self.behind_ok

    def unchanged(self):
        return bool((self.now == self.image).all())

    def tail_ok(self, result_end):
        """[result_end, capacity) still holds the sentinel (outputs)"""
        tail = self.payload[result_end:]
        return bool((np.frombuffer(tail.tobytes(), np.uint8) == self.image[self.off + result_end * self.dtype.itemsize:self.off + self.nbytes]).all())

    def where(self):
        """the first disturbed byte of a guard, relative to the payload's start (negative: in front)"""
        bad = np.nonzero(self.now != self.image)[0]
        bad = bad[(bad < self.off) | (bad >= self.off + self.nbytes)]
        return int(bad[0]) - self.off if len(bad) else None


# ---- 2. the texts ------------------------------------------------------------------------------------------------------------------------------------------

class Text:
    """docs: the batch (bytes); options: the encoder's; fresh: every call gets an encoder that has made no call yet; prepare(enc): run once on a shared encoder"""

    def __init__(self, name, docs, options=(), fresh=False, prepare=None):
        self.name, self.docs, self.options, self.fresh, self.prepare = name, [bytes(d) for d in docs], tuple(options), fresh, prepare
        self.total = sum(map(len, self.docs))
        assert self.total <= 8 * SUB and len(self.docs) >= 3 and b"" in self.docs, (name, self.total)

    def __repr__(self):
        return self.name


def _fast():
    """ordinary words: hits and a few short misses a sub-tile, nothing a lane could not stage -- k_place's fast path"""
    blob = ("".join(PP.crowded(5 + s, 0, seed=s) for s in range(4)) + " abcdefg abcdefg 1").encode()
    return Text("fast", CC.cut(blob, [300, 0, SUB + 700]))


def _dense():
    """a token at every byte (count_cases.many_record_batches): 1,024 records a sub-tile, document starts behind records 256 and 768"""
    docs = CC.many_record_batches()["behind_256_and_768"]
    return Text("dense", docs[:2] + [b""] + docs[2:])


def _lists():
    """the staged and the direct stores of the general path: short misses with inline answers, a token run of 64 (the fast path's limit) and one of 65, missed
    pieces of 18 bytes whose runs exceed kPlaceBig (the whole-wave copy), lists longer than LDS keeps; the memo off, so a merge kernel answers call after call"""
    subs = [PP.crowded(5, 3, long_len=64), PP.crowded(5, 2, long_len=65), PP.crowded(20, 4), PP.ordinary(), PP.crowded(60, 10, seed=3), PP.crowded(100, 28, seed=4)]
    return Text("lists", CC.cut("".join(subs).encode(), [SUB + 500, 0, 2 * SUB + 7, 40]), options=((N.OPT_PIECE_MEMO, 0),))


def _giant():
    """a piece of 1,124 bytes between ordinary sub-tiles (place_pipeline_cases.list_batch's) and one of 1,301 that ends its document"""
    mid = PP.ordinary() + " abcdefg" * 100 + " " + "g" * 223 + "g" * 900 + " zqx" * 31 + PP.ordinary()
    last = " abcdefg" * 90 + " " + "y" * 1300
    return Text("giant", [mid.encode(), b"", last.encode(), b" the abcde"])


def _promoted_words():
    """place_pipeline_cases.check_promoted's generator, run -- not copied -- with its own lexicon"""
    rng = random.Random(61)
    lex = sorted({rng.choice(PP.CONS) + rng.choice("aeiou") + rng.choice(["", "x", "z"]) for _ in range(16)})
    return CC.nested(PP.check_promoted, "words", rng=rng, lex=lex), lex


def _promoted():
    """promoted pieces (TKZ_OPT_PROMOTE 2 after a learning call, as place_pipeline_cases.check_promoted): k_place<..., true>"""
    words, lex = _promoted_words()
    learn = tuple(words(n).encode() for n in (40000, 60000, 50000))
    body = ("".join((words(SUB + 8)[:SUB - 8] + " abcdefg") for _ in range(4)) + PP.ordinary()).encode()

    def prepare(enc):
        data, offs = parity.pack(list(learn))
        enc.encode_batch(data, offs)                                           # the memo fills
        enc.set_option(N.OPT_PROMOTE, 2)
        enc.set_option(N.OPT_PIECE_STATS, 1)
        enc.piece_stats(reset=True)
        enc.encode_batch(data, offs)
        st = enc.piece_stats(reset=True)
        assert st["promoted_pieces_in_tables"] >= len(lex) // 2, st
        enc.set_option(N.OPT_PIECE_STATS, 0)
    return Text("promoted", CC.cut(body, [2 * SUB + 100, 0, SUB]), options=((N.OPT_PROMOTE, 0),), prepare=prepare)


def _redone():
    """docmark_cases.check_thrown_away_attempt's crowded documents: the first call of a fresh encoder with the memo off overflows the miss lists of every
    sub-tile, the attempt is thrown away and redone (inside _end for the two-half form)"""
    gib = CC.generators(47)[1]
    return Text("redone", CC.cut(gib(8000, 2, 2).encode(), [700, 0, 4000]), options=((N.OPT_PIECE_MEMO, 0),), fresh=True)


def _special():
    """the literal at a document's start, at a document's end and across a sub-tile edge (the entries that take no allowed set read it as plain text)"""
    rng = random.Random(17)
    w = lambda n: CC.fill(rng, n)
    lit = EOT.encode()
    a, b = lit + w(400), w(300) + lit
    c = w(2 * SUB - 5 - len(a) - len(b)) + lit + w(50)                          # the literal starts 5 bytes in front of byte 2,048 of the batch
    assert (len(a) + len(b) + c.index(lit)) % SUB == SUB - 5
    return Text("special", [a, b, b"", c, lit, w(30)])


@functools.lru_cache(maxsize=None)
def texts():
    return {t.name: t for t in (_fast(), _dense(), _lists(), _giant(), _promoted(), _redone(), _special())}


TEXT_NAMES = ("fast", "dense", "lists", "giant", "promoted", "redone", "special")


# ---- 3. the expected values: the oracle's, once per text ---------------------------------------------------------------------------------------------------

class Expected:
    """everything an entry may return for `text` with the literal allowed (allowed = [EOT]) or not"""

    def __init__(self, model, trim, text, allowed):
        docs = text.docs
        self.n, self.total = len(docs), text.total
        self.data, self.offs = parity.pack(docs)
        self.ids, self.tok_offs, self.tok_bytes, self.tok_units = model.expected_spans(docs, allowed)
        self.items = [CH.items_of(model, d, allowed) for d in docs]
        self.chunks = CH.Expected(model, docs, CHUNK_MAX, allowed, small=False, items=self.items)
        assert self.chunks.ids == self.ids
        sdocs = [d.decode("utf-8") for d in docs]
        self.trim = {side: TR.expected(trim, sdocs, list(allowed), side, [TRIM_MAX] * self.n) for side in TR.SIDES}
        # the decoders: the ids above, and behind them ids whose bytes are an incomplete sequence at a document's end (u8_decode_cases' single-byte ids)
        one = {k[0]: i for i, k in model.key.items() if len(k) == 1}
        extra = {0: [one[0xE4], one[0xB8]], self.n - 1: [one[0xE4]]}
        self.dec_ids, self.dec_offs, self.dec_docs = [], [0], []
        for d, doc in enumerate(docs):
            more = extra.get(d, [])
            self.dec_ids += self.ids[self.tok_offs[d]:self.tok_offs[d + 1]] + more
            self.dec_offs.append(len(self.dec_ids))
            self.dec_docs.append(doc + bytes(model.key[i][0] for i in more))
        self.dec_bytes = b"".join(self.dec_docs)
        self.dec_byte_offs = np.cumsum([0] + [len(d) for d in self.dec_docs]).tolist()
        units = [U8.get_string(d) for d in self.dec_docs]
        assert units[0][-1] == 0xFFFD and units[-1][-1] == 0xFFFD and all(u == U8.python_codec(d) for u, d in zip(units, self.dec_docs))
        self.dec_units = [u for p in units for u in p]
        self.dec_unit_offs = np.cumsum([0] + [len(p) for p in units]).tolist()
        # capacities inside a store path, from the oracle's token offsets: the middle of the first piece of 2..4 tokens (an inline quad; a promoted piece in the
        # promoted text), of the longest run of 9..128 tokens (the whole-wave copy), of a piece of more than 1,024 bytes (the giant path)
        self.inside = {"mid": (len(self.ids) // 2) | 1}
        tok = 0
        best_run = 0
        for d in range(self.n):
            tok = self.tok_offs[d]
            for (_a, nbytes, t) in self.items[d]:
                if 2 <= t <= 4 and "quad" not in self.inside:
                    self.inside["quad"] = tok + t // 2
                if 9 <= t <= 128 and nbytes <= 128 and t > best_run:
                    best_run, self.inside["run"] = t, tok + t // 2
                if nbytes > 1024 and "giant" not in self.inside:
                    self.inside["giant"] = tok + t // 2
                tok += t
        # the same points for the decoders: the byte / unit at which that token starts, and one more
        starts = np.cumsum([0] + [len(model.token_text(i, {EOT_ID} if allowed else set())) for i in self.dec_ids])
        ub = SP.units_begun(self.dec_bytes)
        self.inside_bytes = {k: int(starts[v + (len(extra[0]) if v >= self.tok_offs[1] else 0)]) + 1 for k, v in self.inside.items()}
        self.inside_units = {k: int(ub[v]) for k, v in self.inside_bytes.items()}


CAP_KINDS = ("exact", "plus5", "minus1", "zero", "mid", "quad", "run", "giant")


def capacity(kind, need, inside):
    """the capacity of a kind for a result of `need` entries; None: the text has no such store path"""
    if kind in ("exact", "plus5", "minus1", "zero"):
        return {"exact": need, "plus5": need + 5, "minus1": max(need - 1, 0), "zero": 0}[kind]
    if kind not in inside:
        return None
    return max(1, min(inside[kind], need - 1))


# ---- 4. the matrix -----------------------------------------------------------------------------------------------------------------------------------------

# (poison, input phase, offsets' phase, int64 outputs' phase) as indices: every poison with every input phase, and every PAIR of values of any two axes
PAIRWISE = tuple((p, q, (p + q) & 1, ((p >> 1) + (q >> 1) + p) & 1) for p in range(8) for q in range(4))

ENTRIES = ("plain", "special", "begin_end", "begin_counts", "trim_suffix", "trim_prefix", "count", "spans_both", "spans_bytes", "spans_units", "spans_neither", "chunks",
           "decode_utf8", "decode_utf16")
WITH_ALLOWED = ("special", "trim_suffix", "trim_prefix", "count", "spans_both", "spans_bytes", "spans_units", "spans_neither", "chunks", "decode_utf8", "decode_utf16")
NO_CAPACITY = ("count", "spans_neither")               # tkz_count_batch_device takes no id buffer; both span arrays NULL is TKZ_E_ARG at every capacity
INPUT_MATRIX_ENTRIES = ("plain", "decode_utf16")


class Geo:
    """one row of the matrix, as indices into the phase tables above"""

    def __init__(self, poison, in_phase, offs_phase, i64_phase, out_phase, cap="exact", chunk_cap="exact"):
        self.poison, self.in_phase, self.offs_phase, self.i64_phase, self.out_phase, self.cap, self.chunk_cap = poison, in_phase, offs_phase, i64_phase, out_phase, cap, chunk_cap

    def __repr__(self):
        return "poison %02x, input phase %d, offsets' phase %d, int64 phase %d, output phase %d, capacity %s%s" % (
            POISONS[self.poison], self.in_phase, self.offs_phase, self.i64_phase, self.out_phase, self.cap, "" if self.chunk_cap == "exact" else ", chunk capacity " + self.chunk_cap)


def rows(entry, text_name, full=True):
    """output phase x capacity for one entry and text; the input axes by PAIRWISE, from a start that differs from pair to pair.  full=False (the emulated run):
    every capacity kind once, the output phases in turn"""
    salt = 5 * ENTRIES.index(entry) + 11 * TEXT_NAMES.index(text_name)
    kinds = ("exact",) if entry in NO_CAPACITY else CAP_KINDS
    pairs = [(o, k, "exact") for k in kinds for o in range(4)]
    if entry == "chunks":
        pairs += [(o, k, "minus1") for k in ("exact", "minus1") for o in range(4)]
    if not full:
        once = [(k, c) for o, k, c in pairs if o == 0]
        pairs = [((i + salt) % 4, k, c) for i, (k, c) in enumerate(once)]
    return [Geo(*PAIRWISE[(salt + r) % len(PAIRWISE)], out_phase=o, cap=k, chunk_cap=c) for r, (o, k, c) in enumerate(pairs)]


def input_rows(entry, text_name, full=True):
    """poison x input phase in full, at the exact capacity; the output phases in turn.  full=False: every poison and every input phase once"""
    salt = ENTRIES.index(entry) + TEXT_NAMES.index(text_name)
    table = PAIRWISE if full else [PAIRWISE[4 * p + (p + salt) % 4] for p in range(8)]
    return [Geo(*row, out_phase=(r + salt) % 4) for r, row in enumerate(table)]


# ---- 5. the entries ----------------------------------------------------------------------------------------------------------------------------------------

class Env:
    """A library, the oracle, the transport; the models and the encoders of the texts."""

    def __init__(self, lib, O, upload=None):
        self.lib, self.O, self.L = lib, O, lib.L
        self.mem = Memory(upload)
        self.model = CH.Ctx(lib, O, PP.table(), N.CL100K, SPECIALS, upload=upload)
        self.trim = TR.Expect(O, self.model.ovocab, N.CL100K, SPECIALS)
        self._expected, self._encoders = {}, {}

    def expected(self, text, allowed):
        key = (text.name, bool(allowed))
        if key not in self._expected:
            self._expected[key] = Expected(self.model, self.trim, text, [EOT] if allowed else [])
        return self._expected[key]

    def encoder(self, text, shared=False):
        if text.fresh and not shared:
            return self._new(text)
        if text.name not in self._encoders:
            enc = self._encoders[text.name] = self._new(text)
            if text.prepare:
                text.prepare(enc)
        return self._encoders[text.name]

    def _new(self, text):
        enc = N.Encoder(self.model.vocab, N.CL100K)
        for opt, val in text.options:
            enc.set_option(opt, val)
        enc.set_special_tokens(SPECIALS)
        return enc

    # -- arenas --
    def input(self, dtype, data, phase, mod, guard):
        return Arena(self.mem, dtype, len(data), phase, mod, guard, data=data)

    def output(self, dtype, n, phase, guard, mod=16, full=0):
        """full: the entries of the whole result, whatever the capacity"""
        return Arena(self.mem, dtype, n, phase, mod, guard, spill=max(0, full - n) * np.dtype(dtype).itemsize)


class Out:
    """an output of a call: its arena, what a successful call leaves in its first `len(want)` entries"""

    def __init__(self, name, arena, want):
        self.name, self.arena, self.want = name, arena, np.asarray(want, arena.dtype)


def settle(what, status, reported, needed, fits, ins, outs):
    """the assertions of section "geometry matrix" for one call: `reported` / `needed` are tuples (the token total; the chunk entry: and the chunk count)"""
    for a in ins:
        a.read()
        assert a.unchanged(), "%s: an INPUT allocation was written, first at byte %+d of the buffer" % (what, int(np.nonzero(a.now != a.image)[0][0]) - a.off)
    for o in outs:
        o.arena.read()
        assert o.arena.front_ok, "%s: %s: the guard IN FRONT was written, %d bytes before the buffer" % (what, o.name, -o.arena.where())
        assert o.arena.behind_ok, "%s: %s: written at or behind the capacity (%d entries), %d bytes behind the buffer's start" % (what, o.name, o.arena.n, o.arena.where())
    if not fits:
        assert status == N.E_CAPACITY, "%s: status %d, expected TKZ_E_CAPACITY" % (what, status)
        assert reported == needed, "%s: TKZ_E_CAPACITY reports %s, the oracle needs %s" % (what, reported, needed)
        return
    assert status == N.OK, "%s: status %d" % (what, status)
    assert reported == needed, "%s: reports %s, the oracle has %s" % (what, reported, needed)
    for o in outs:
        got, end = o.arena.payload[:len(o.want)], len(o.want)
        if not np.array_equal(got, o.want):
            k = SC.first_diff(got.tolist(), o.want.tolist())
            raise AssertionError("%s: %s differ at %d of %d: got %s, expected %s" % (what, o.name, k, end, got[max(0, k - 3):k + 5].tolist(), o.want[max(0, k - 3):k + 5].tolist()))
        assert o.arena.tail_ok(end), "%s: %s: written behind the result (%d entries) and below the capacity (%d)" % (what, o.name, end, o.arena.n)


def run(env, entry, text, geo):
    """one call of `entry` on `text` in the geometry `geo`.  Returns False when the text has no store path of geo.cap's kind (nothing is run), else True."""
    allowed = entry in WITH_ALLOWED
    exp = env.expected(text, allowed)
    what = "%s on %r: %r" % (entry, text, geo)
    L, e = env.L, exp
    poison = np.uint8(POISONS[geo.poison])
    i64 = I64_PHASES[geo.i64_phase]
    index = np.asarray([0] if allowed else [], np.int32)
    al = (index.ctypes.data if allowed else None, len(index))
    tot, nch = C.c_int64(-1), C.c_int64(-1)

    if entry.startswith("decode"):
        u16 = entry == "decode_utf16"
        want, woffs = (e.dec_units, e.dec_unit_offs) if u16 else (list(e.dec_bytes), e.dec_byte_offs)
        cap = capacity(geo.cap, len(want), e.inside_units if u16 else e.inside_bytes)
        if cap is None:
            return False
        enc = env.encoder(text, shared=True)
        ids = env.input(np.int32, e.dec_ids, IDS_IN_PHASES[geo.in_phase], 16, poison)
        offs = env.input(np.int64, e.dec_offs, I64_PHASES[geo.offs_phase], 16, I64_SENTINEL)
        out = env.output(np.uint16 if u16 else np.uint8, cap, (U16_OUT_PHASES if u16 else U8_OUT_PHASES)[geo.out_phase], UNIT_SENTINEL if u16 else BYTE_SENTINEL, full=len(want))
        ooff = env.output(np.int64, e.n + 1, i64, I64_SENTINEL)
        fn = L.tkz_decode_batch_utf16_device if u16 else L.tkz_decode_batch_device
        st = fn(enc._h, ids.ptr, offs.ptr, e.n, len(e.dec_ids), out.ptr, cap, ooff.ptr, None, C.byref(tot))
        settle(what, st, (tot.value,), (len(want),), len(want) <= cap, [ids, offs], [Out("units" if u16 else "bytes", out, want), Out("offsets", ooff, woffs)])
        return True

    need = len(e.trim[N.TRIM_SUFFIX if entry == "trim_suffix" else N.TRIM_PREFIX][0]) if entry.startswith("trim") else len(e.ids)
    cap = capacity(geo.cap, need, e.inside)
    if cap is None:
        return False
    enc = env.encoder(text)
    w0 = enc.workspace_bytes
    d_bytes = env.input(np.uint8, e.data, BYTES_PHASES[geo.in_phase], 64, poison)
    d_offs = env.input(np.int64, e.offs, I64_PHASES[geo.offs_phase], 16, I64_SENTINEL)
    ins = [d_bytes, d_offs]
    head = (enc._h, d_bytes.ptr, d_offs.ptr, e.n, e.total)
    ooff = env.output(np.int64, e.n + 1, i64, I64_SENTINEL)
    ids = None if entry == "count" else env.output(np.int32, cap, IDS_OUT_PHASES[geo.out_phase], ID_SENTINEL, full=len(e.ids))
    outs = [Out("offsets", ooff, e.tok_offs)] + ([Out("ids", ids, e.ids)] if ids is not None else [])
    needed, fits = (need,), need <= cap
    reported = lambda: (tot.value,)

    if entry == "plain":
        st = L.tkz_encode_batch_device(*head, ids.ptr, cap, ooff.ptr, None, C.byref(tot))
    elif entry == "special":
        st = L.tkz_encode_batch_special_device(*head, *al, ids.ptr, cap, ooff.ptr, None, C.byref(tot))
    elif entry in ("begin_end", "begin_counts"):
        h = C.c_void_p()
        if entry == "begin_counts":
            counts = env.output(np.int64, 3, I64_PHASES[1 - geo.i64_phase], I64_SENTINEL)
            outs.append(Out("counts", counts, [e.n, e.total, need]))
            st = L.tkz_encode_batch_device_begin_counts(*head, ids.ptr, cap, ooff.ptr, None, counts.ptr, C.byref(h))
            assert st != N.OK or L.tkz_pending_counts_device(h) == counts.ptr
        else:
            st = L.tkz_encode_batch_device_begin(*head, ids.ptr, cap, ooff.ptr, None, C.byref(h))
        assert st == N.OK, "%s: _begin returns %d" % (what, st)
        st = L.tkz_encode_batch_device_end(h, C.byref(tot))
    elif entry == "count":
        st = L.tkz_count_batch_device(*head, *al, ooff.ptr, None, C.byref(tot))
    elif entry.startswith("trim"):
        side = N.TRIM_SUFFIX if entry == "trim_suffix" else N.TRIM_PREFIX
        kept, koffs, kb, ku = e.trim[side]
        cb, cu = env.output(np.int64, e.n, I64_PHASES[1 - geo.i64_phase], I64_SENTINEL), env.output(np.int64, e.n, i64, I64_SENTINEL)
        outs = [Out("offsets", ooff, koffs), Out("ids", ids, kept), Out("cut_bytes", cb, kb), Out("cut_units", cu, ku)]
        st = L.tkz_encode_batch_trim_device(*head, *al, side, TRIM_MAX, None, ids.ptr, cap, ooff.ptr, cb.ptr, cu.ptr, None, C.byref(tot))
    elif entry.startswith("spans"):
        # the span arrays at phases that differ from the ids' and from each other
        tb = env.output(np.int32, cap, (IDS_OUT_PHASES[geo.out_phase] + 4) % 16, ID_SENTINEL, full=need) if entry in ("spans_both", "spans_bytes") else None
        tu = env.output(np.int32, cap, (IDS_OUT_PHASES[geo.out_phase] + 8) % 16, ID_SENTINEL, full=need) if entry in ("spans_both", "spans_units") else None
        outs += ([Out("tok_bytes", tb, e.tok_bytes)] if tb else []) + ([Out("tok_units", tu, e.tok_units)] if tu else [])
        st = L.tkz_encode_batch_spans_device(*head, *al, ids.ptr, cap, ooff.ptr, tb.ptr if tb else None, tu.ptr if tu else None, None, C.byref(tot))
        if entry == "spans_neither":                                             # TKZ_E_ARG (tkz.h), and nothing is written anywhere
            assert st == N.E_ARG, "%s: status %d, expected TKZ_E_ARG" % (what, st)
            for a in ins + [ooff, ids]:
                assert a.read().unchanged(), what + ": written by a call that returns TKZ_E_ARG"
            return True
    elif entry == "chunks":
        x = e.chunks
        n_chunks = x.dco[-1]
        ccap = capacity(geo.chunk_cap, n_chunks, {})
        dco = env.output(np.int64, e.n + 1, I64_PHASES[1 - geo.i64_phase], I64_SENTINEL)
        ct = env.output(np.int64, ccap + 1, i64, I64_SENTINEL, full=n_chunks + 1)
        cb = env.output(np.int64, ccap, I64_PHASES[1 - geo.i64_phase], I64_SENTINEL, full=n_chunks)
        cu = env.output(np.int64, ccap, i64, I64_SENTINEL, full=n_chunks)
        outs += [Out("doc_chunk_offsets", dco, x.dco), Out("chunk_tokens", ct, x.ct), Out("chunk_bytes", cb, x.cb), Out("chunk_units", cu, x.cu)]
        st = L.tkz_encode_batch_chunks_device(*head, *al, CHUNK_MAX, ids.ptr, cap, ooff.ptr, dco.ptr, ct.ptr, cb.ptr, cu.ptr, ccap, None, C.byref(tot), C.byref(nch))
        needed, fits = (need, n_chunks), fits and n_chunks <= ccap
        reported = lambda: (tot.value, nch.value)
    else:
        raise AssertionError(entry)
    settle(what, st, reported(), needed, fits, ins, outs)
    if text.fresh:
        assert enc.workspace_bytes > w0, what + ": the lists did not grow -- no attempt was thrown away"
    return True


def run_rows(env, entry, text_name, table):
    """Returns the capacity kinds that ran."""
    text = texts()[text_name]
    return {g.cap for g in table if run(env, entry, text, g)}


# ---- 6. where the text ends --------------------------------------------------------------------------------------------------------------------------------

END_PATTERNS = (N.P1, N.CL100K, N.O200K, N.O200K_DOTNET)
END_POISONS = (0xE4, ord("a"), ord(" "))
TAILS = ("é", "中", "\U0001F600", "  中", " 　　", "12３", "'sé", "\r\n ", "中" * 6)
FOLLOWS = (b"", b"a", b" x")
HEAD_SPLIT = 37                                         # the line of test_pretok_classify.refused_docs: the two-document form cuts behind the first one


def tpos(block):
    """the start of the trailing row that block `block` of k_pretok_rows stages (tkz_pretok_request): 4,032 and 8,000"""
    return (TPC.BLOCK_ROWS * block - 1 + 64) * 64


def head():
    return TPC.refused_docs()[9]                        # the ASCII line, 3 x 4,096 bytes of it


def end_docs(block, tail, full=True):
    """every document head[:start] + tail + follow whose tail starts in [tpos - len - 4, tpos + 17]: the totals take every value of [tpos - 4, tpos + 20].  full=False (the
    emulated run): the starts at which the tail straddles tpos - 1 | tpos or tpos + 15 | tpos + 16, and those at which it ends the text at tpos - 1 .. tpos + 1 and
    tpos + 15 .. tpos + 17"""
    t, tb, base = tpos(block), tail.encode("utf-8"), head()
    assert base[HEAD_SPLIT - 1:HEAD_SPLIT] == b"\n" and len(base) > t + 64
    out = []
    for start in range(t - len(tb) - 4, t + 18):
        for follow in FOLLOWS:
            total = start + len(tb) + len(follow)
            straddles = any(start < edge < start + len(tb) for edge in (t, t + 16))
            ends = not follow and any(total == edge + k for edge in (t, t + 16) for k in (-1, 0, 1))
            if full or straddles or ends:
                out.append(base[:start] + tb + follow)
    return out


class EndEnv:
    """the text-end family on one pattern: gpt2's table, as test_pretok_classify"""

    def __init__(self, lib, O, raw, pattern, upload=None, every_poison=True):
        """every_poison=False (the emulated run): one poison a call, in turn"""
        self.O, self.pattern, self.L, self.every_poison = O, pattern, lib.L, every_poison
        self.mem = Memory(upload)
        self.enc = N.Encoder(N.Vocab(raw, lib), pattern)
        self.oenc = O.Encoder(O.Vocab(raw), pattern)
        self.calls = 0

    def check(self, doc):
        for docs in ([doc], [doc[:HEAD_SPLIT], doc[HEAD_SPLIT:]]):               # a single document, and the last of two: the same bytes, the same end
            data, offs = parity.pack(docs)
            what = "pattern %d, %d bytes in %d documents, ending %r" % (self.pattern, len(data), len(docs), doc[-12:])
            want = parity.oracle_bitmap(self.O, self.pattern, docs)
            got = self.enc.pretokenize(data, offs)
            assert np.array_equal(got, want), what + ": " + parity.explain_bitmap_diff(got, want, docs, offs)
            eids, eoffs = parity.oracle_encode_docs(self.oenc, docs)
            for poison in END_POISONS if self.every_poison else END_POISONS[self.calls % 3:][:1]:
                k = self.calls = self.calls + 1
                d_bytes = Arena(self.mem, np.uint8, len(data), BYTES_PHASES[k % 4], 64, np.uint8(poison), data=data)
                d_offs = Arena(self.mem, np.int64, len(offs), I64_PHASES[k % 2], 16, I64_SENTINEL, data=offs)
                ids = Arena(self.mem, np.int32, len(eids), IDS_OUT_PHASES[(k // 4) % 4], 16, ID_SENTINEL)
                ooff = Arena(self.mem, np.int64, len(offs), I64_PHASES[(k // 2) % 2], 16, I64_SENTINEL)
                tot = C.c_int64(-1)
                st = self.L.tkz_encode_batch_device(self.enc._h, d_bytes.ptr, d_offs.ptr, len(docs), len(data), ids.ptr, len(eids), ooff.ptr, None, C.byref(tot))
                settle("%s, poison %02x" % (what, poison), st, (tot.value,), (len(eids),), True, [d_bytes, d_offs], [Out("offsets", ooff, eoffs), Out("ids", ids, eids)])


# ---- 7. the layout the matrix promises ---------------------------------------------------------------------------------------------------------------------

def check_layout(kernel_header, full):
    """every entry with every capacity kind and all four output phases; every poison and every input phase on the plain entry and one decoder; PAIRWISE covers
    every pair of values of any two of its axes; the text-end totals and tails are what section 6 says"""
    assert re.search(r"\bkRowsPerWave = %d\b" % TPC.BLOCK_ROWS, kernel_header) and re.search(r"\bkSub = %d\b" % SUB, kernel_header)
    assert (tpos(0), tpos(1)) == (4032, 8000)
    sizes = (len(POISONS), 4, 2, 2)
    for a in range(4):
        for b in range(a + 1, 4):
            assert {(r[a], r[b]) for r in PAIRWISE} == {(x, y) for x in range(sizes[a]) for y in range(sizes[b])}, (a, b)
    for entry in ENTRIES:
        seen = set()
        for name in TEXT_NAMES:
            table = rows(entry, name, full)
            seen |= {(g.out_phase, g.cap) for g in table}
            if full:
                assert {(g.out_phase, g.cap) for g in table} >= {(o, k) for o in range(4) for k in (("exact",) if entry in NO_CAPACITY else CAP_KINDS)}, (entry, name)
            if entry == "chunks":
                assert {(g.cap, g.chunk_cap) for g in table} >= {("exact", "exact"), ("exact", "minus1"), ("minus1", "exact"), ("minus1", "minus1")}
        assert {o for o, _ in seen} == {0, 1, 2, 3}, entry
        assert {k for _, k in seen} == set(("exact",) if entry in NO_CAPACITY else CAP_KINDS), entry
    for entry in INPUT_MATRIX_ENTRIES:
        for name in TEXT_NAMES:
            table = input_rows(entry, name, full)
            assert {g.poison for g in table} == set(range(8)) and {g.in_phase for g in table} == set(range(4)), (entry, name)
            if full:
                assert {(g.poison, g.in_phase) for g in table} == {(p, q) for p in range(8) for q in range(4)}
    for t in texts().values():
        assert t.total <= 8 * SUB and b"" in t.docs and t.total > 2 * SUB
    for block in (0, 1):
        t = tpos(block)
        for tail in TAILS:
            n = len(tail.encode("utf-8"))
            docs = end_docs(block, tail, True)
            start = lambda d: d.rindex(tail.encode("utf-8"))
            assert {len(d) for d in docs} >= set(range(t - 4, t + 21)) and {start(d) for d in docs} == set(range(t - n - 4, t + 18)), (block, tail)
            assert all(d[start(d) + n:] in FOLLOWS for d in docs) and {d[start(d) + n:] for d in docs} == set(FOLLOWS)
            few = end_docs(block, tail, False)
            assert 0 < len(few) < len(docs) and set(few) <= set(docs)
            for edge in (t, t + 16):
                assert any(len(d) == edge for d in few) and {edge - start(d) for d in few if start(d) < edge < start(d) + n} == set(range(1, n)), (block, tail, edge)


def check_inside_kinds(env):
    """the texts reach, between them, every capacity kind that is taken from the oracle's token offsets -- and each where it is meant to"""
    has = {name: set(env.expected(t, False).inside) for name, t in texts().items()}
    assert "run" in has["lists"] and "giant" in has["giant"] and "quad" in has["promoted"] and "quad" in has["lists"], has
    assert set().union(*has.values()) == {"mid", "quad", "run", "giant"}
    e = env.expected(texts()["lists"], False)
    runs = sorted({t for items in e.items for _, _, t in items})
    assert 64 in runs and 65 in runs and 18 in runs and 4 in runs, runs
    assert max(n for items in env.expected(texts()["giant"], False).items for _, n, _ in items) > 1024
    s = env.expected(texts()["special"], True)
    assert s.ids.count(EOT_ID) == 4 and s.ids[0] == EOT_ID and s.ids[s.tok_offs[2] - 1] == EOT_ID and EOT_ID not in env.expected(texts()["special"], False).ids
