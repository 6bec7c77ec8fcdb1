"""Host-side mirror of the reference's tokenizer interface for the Encode path, over libtkz.

Names, argument meaning and error behaviour follow
  ITokenizer                     Tokenizer_C#/TokenizerLib/ITokenizer.cs:7-46
  TikTokenizer                   Tokenizer_C#/TokenizerLib/TikTokenizer.cs:20-605
  TokenizerBuilder               Tokenizer_C#/TokenizerLib/TokenizerBuilder.cs:14-214
so that the parity tests read like the reference's own (TikTokenizerUnitTest.cs).  `EncodeBatch` is the
one addition (the reference has no batch API).  What runs where:

  * special-token segmentation (EncodeInternal / FindNextSpecialToken, TikTokenizer.cs:141-170,230-241)
    is host work: every text is cut into plain segments + literal special ids, and ALL plain segments of
    the batch go to the GPU as one document batch (a segment is matched in isolation by the reference
    too: `Regex.Matches(text[start..end])`, TikTokenizer.cs:252);
  * the plain path (TikTokenizer.cs:250-274 + BytePairEncoder.cs:13-76) is the HIP path of libtkz;
  * Decode / DecodeBatch (TikTokenizer.cs:586-604) run on the device too: an id -> bytes gather through the decoder table + a scan;
  * EncodeTrimSuffix / EncodeTrimPrefix (TikTokenizer.cs:288-579) cut at piece granularity: the GPU
    encodes every plain segment with piece granularity (tkz_encode_batch_pieces_utf8: token count and byte span of each
    regex match), the walk over pieces / special tokens that decides where to cut is host work.
"""
import os
import re
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np

from . import _native as N

ENDOFTEXT = "<|endoftext|>"
FIM_PREFIX = "<|fim_prefix|>"
FIM_MIDDLE = "<|fim_middle|>"
FIM_SUFFIX = "<|fim_suffix|>"
ENDOFPROMPT = "<|endofprompt|>"

# the split regexes, verbatim (TokenizerBuilder.cs:112,128; tokenizer_ts/src/tokenizerBuilder.ts:79-89)
REGEX_PATTERN_1 = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"
REGEX_CL100K = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*"
                r"|\s*[\r\n]+|\s+(?!\S)|\s+")
_O2_SUFFIX = r"(?:'s|'S|'t|'T|'re|'RE|'Re|'eR|'ve|'VE|'vE|'Ve|'m|'M|'ll|'lL|'Ll|'LL|'d|'D)?"
REGEX_O200K = "|".join([
    "[^\r\n\\p{L}\\p{N}]?[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]*[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]+" + _O2_SUFFIX,
    "[^\r\n\\p{L}\\p{N}]?[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]+[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]*" + _O2_SUFFIX,
    r"\p{N}{1,3}", r" ?[^\s\p{L}\p{N}]+[\r\n/]*", r"\s*[\r\n]+", r"\s+(?!\S)", r"\s+"])

# TokenizerBuilder.cs:17-66 (and the o200k models of tokenizer_ts/src/tokenizerBuilder.ts)
MODEL_PREFIX_TO_ENCODING = {"gpt-4-": "cl100k_base", "gpt-3.5-turbo-": "cl100k_base", "gpt-4o-": "o200k_base"}
MODEL_TO_ENCODING = {
    "gpt-4o": "o200k_base",
    "gpt-4": "cl100k_base", "gpt-3.5-turbo": "cl100k_base",
    "text-davinci-003": "p50k_base", "text-davinci-002": "p50k_base", "text-davinci-001": "r50k_base",
    "text-curie-001": "r50k_base", "text-babbage-001": "r50k_base", "text-ada-001": "r50k_base",
    "davinci": "r50k_base", "curie": "r50k_base", "babbage": "r50k_base", "ada": "r50k_base",
    "code-davinci-002": "p50k_base", "code-davinci-001": "p50k_base", "code-cushman-002": "p50k_base",
    "code-cushman-001": "p50k_base", "davinci-codex": "p50k_base", "cushman-codex": "p50k_base",
    "text-davinci-edit-001": "p50k_edit", "code-davinci-edit-001": "p50k_edit",
    "text-embedding-ada-002": "cl100k_base",
    "text-similarity-davinci-001": "r50k_base", "text-similarity-curie-001": "r50k_base",
    "text-similarity-babbage-001": "r50k_base", "text-similarity-ada-001": "r50k_base",
    "text-search-davinci-doc-001": "r50k_base", "text-search-curie-doc-001": "r50k_base",
    "text-search-babbage-doc-001": "r50k_base", "text-search-ada-doc-001": "r50k_base",
    "code-search-babbage-code-001": "r50k_base", "code-search-ada-code-001": "r50k_base",
    "gpt2": "gpt2",
}
# encoder -> (regex, rank file name, special tokens)          TokenizerBuilder.cs:109-181
ENCODERS = {
    "cl100k_base": (REGEX_CL100K, "cl100k_base.tiktoken",
                    {ENDOFTEXT: 100257, FIM_PREFIX: 100258, FIM_MIDDLE: 100259, FIM_SUFFIX: 100260, ENDOFPROMPT: 100276}),
    "p50k_base": (REGEX_PATTERN_1, "p50k_base.tiktoken", {ENDOFTEXT: 50256}),
    "p50k_edit": (REGEX_PATTERN_1, "p50k_base.tiktoken", {ENDOFTEXT: 50256, FIM_PREFIX: 50281, FIM_MIDDLE: 50282, FIM_SUFFIX: 50283}),
    "r50k_base": (REGEX_PATTERN_1, "r50k_base.tiktoken", {ENDOFTEXT: 50256}),
    "gpt2": (REGEX_PATTERN_1, "gpt2.tiktoken", {ENDOFTEXT: 50256}),
    "o200k_base": (REGEX_O200K, "o200k_base.tiktoken", {ENDOFTEXT: 199999, ENDOFPROMPT: 200018}),
}
# the engine of the reference that defines each encoder: o200k_base ships only with the TypeScript reference (tokenizer_ts/src/tokenizerBuilder.ts:79-89,
# compiled by `new RegExp(pattern, "gu")`, tikTokenizer.ts:100); everything else is TokenizerBuilder.cs's.  By-name construction follows this table;
# CreateTokenizer with an explicit pattern string keeps the .NET reading (it replaces `new Regex(pattern)`, TikTokenizer.cs:77).
ENCODER_ENGINE = {"o200k_base": "js"}


def host_unicode_classes(ucd=None, n_code_points: int = 0x110000, engine: str = "dotnet"):
    """The class table a host hands to TikTokenizer(unicode_classes=...): class 0..8 of every code point below n_code_points (65536: code units) from
    a `unicodedata`-like module (default: this Python's -- another Unicode version than the 13.0 libtkz is built with).  \\s is .NET's
    ([\\f\\n\\r\\t\\v\\x85\\p{Z}]) or, engine="js", ECMAScript's ([\\t\\n\\v\\f\\r\\ufeff\\p{Zs}\\u2028\\u2029])."""
    import unicodedata
    ucd = ucd or unicodedata
    out = np.zeros(n_code_points, np.uint8)
    code = {"Lu": 1, "Ll": 2, "Lt": 3, "Lm": 4, "Lo": 5, "Mn": 6, "Mc": 6, "Me": 6, "Nd": 7, "Nl": 7, "No": 7, "Zs": 8, "Zl": 8, "Zp": 8}
    for cp in range(n_code_points):
        if 0xD800 <= cp <= 0xDFFF:
            continue
        out[cp] = code.get(ucd.category(chr(cp)), 0)
    # \s beyond \p{Z}: .NET adds [\f\n\r\t\v\x85]; ECMAScript adds [\t\n\v\f\r\ufeff] (U+0085 is NOT white space there)
    for cp in ((9, 10, 11, 12, 13, 0xFEFF) if engine == "js" else (9, 10, 11, 12, 13, 0x85)):
        if cp < n_code_points:
            out[cp] = 8
    return out


def _utf8_like_dotnet(s: str) -> bytes:
    """Encoding.UTF8.GetBytes: a lone surrogate becomes U+FFFD (TikTokenizer.cs:261)."""
    try:
        return s.encode("utf-8")
    except UnicodeEncodeError:
        return s.encode("utf-16-le", "surrogatepass").decode("utf-16-le", "replace").encode("utf-8")


def _has_lone_surrogate(s: str) -> bool:
    try:
        s.encode("utf-8")
        return False
    except UnicodeEncodeError:
        return True


class TikTokenizer:
    """ITokenizer over the MI355X encode path.  Construct through TokenizerBuilder, or directly with the
    bytes of a .tiktoken rank file (the reference takes a Stream, TikTokenizer.cs:60-65)."""

    def __init__(self, tikTokenBpeFile: bytes, specialTokensEncoder: Optional[Dict[str, int]], pattern: str,
                 cacheSize: int = 8192, device: int = 0, lib: Optional[N.Library] = None, host: str = "dotnet",
                 unicode_classes=None, case_equivalence: bool = False, reserve_bytes: int = 0, reserve_docs: int = 0):
        """`host` names the regex engine whose reading of `pattern` is wanted: "dotnet" (the default: `new Regex(pattern,
        RegexOptions.Compiled)`, TikTokenizer.cs:77 -- UTF-16 code units, .NET's \\s) or "js" (`new RegExp(pattern, "gu")`,
        tokenizer_ts/src/tikTokenizer.ts:100 -- code points, ECMAScript's \\s; implemented for the o200k string only, the one
        pattern that exists only in the TypeScript reference).  The two differ on supplementary-plane chars, U+0085 and U+FEFF."""
        self._lib = lib or N.default_library()
        if host not in ("dotnet", "js"):
            raise ValueError("host must be 'dotnet' or 'js'")
        pat = self._lib.L.tkz_pattern_from_regex_engine  # maps the reference's regex text to a scanner, refuses anything else
        import ctypes as C
        out = C.c_int32(0)
        self._lib.check(pat(pattern.encode("utf-8"), N.ENGINE_ECMASCRIPT if host == "js" else N.ENGINE_DOTNET, C.byref(out)))
        self._vocab = N.Vocab(tikTokenBpeFile, self._lib)     # FormatError / DuplicateRankError as in LoadTikTokenBpe + Init
        self._encoder = N.Encoder(self._vocab, out.value, device)
        # The split is whatever the HOST's regex engine makes of the pattern (TikTokenizer.cs:77 compiles it in the running process): `unicode_classes`
        # hands that runtime's classification over (uint8[65536] per code unit, or uint8[1114112] per code point; host_unicode_classes() builds
        # one from a `unicodedata`-like module), `case_equivalence` is .NET >= 7's reading of cl100k's (?i:...) ('ſ is 's).  Default: net6.0's.
        if unicode_classes is not None:
            if host == "js" and len(unicode_classes) == 65536:
                # the ECMAScript reading classifies by CODE POINT: a table of code units leaves the supplementary planes on the built-in Unicode 13.0 data
                import warnings
                warnings.warn("host='js' classifies by code point: a 65536-entry unicode_classes table covers the BMP only, the supplementary planes keep "
                              "libtkz's built-in Unicode 13.0 classes (pass 1114112 entries to override them too)")
            self._encoder.set_unicode_classes(unicode_classes)
        if case_equivalence:
            self._encoder.set_option(N.OPT_CASE_EQUIVALENCE, 1)
        # construction pays, not the first Encode (TokenizerBuilder.cs:210-213): the device workspace of batches of up to reserve_bytes / reserve_docs
        if reserve_bytes > 0:
            self._encoder.reserve(reserve_bytes, max(1, reserve_docs))
        # the reference's LRU piece memo (LRUCache.cs; no effect on results) lives on the device with a fixed size: cacheSize only says
        # whether it is used (the reference's LRUCache of size 0 keeps nothing)
        if cacheSize <= 0:
            self._encoder.set_option(N.OPT_PIECE_MEMO, 0)
        self.SpecialTokensEncoder: Dict[str, int] = dict(specialTokensEncoder or {})
        self.SpecialTokens = set(self.SpecialTokensEncoder)
        # alternation of the escaped literals in registration order (TikTokenizer.cs:78): leftmost match, first alternative wins
        self._special_re = re.compile("|".join(re.escape(k) for k in self.SpecialTokensEncoder)) if self.SpecialTokensEncoder else None
        self._special_on_host = False                         # set when the device's special entries refuse the registered set (UnsupportedError)
        self._fffd_literal = any("\ufffd" in k for k in self.SpecialTokensEncoder)
        if self.SpecialTokensEncoder:
            self._encoder.set_special_tokens(self.SpecialTokensEncoder)      # SpecialTokensDecoder (TikTokenizer.cs:79) for Decode; the device's literal table

    # ---- segmentation (host) ---------------------------------------------------------------------
    def _segments(self, text: str, allowed: Optional[Iterable[str]]):
        """EncodeInternal + FindNextSpecialToken: list of ('t', plain_text, None) / ('s', id, literal)."""
        allowed = set(allowed) if allowed else set()
        if not allowed or self._special_re is None:
            return [("t", text, None)] if text else []
        out = []
        start = 0
        while True:
            find = start
            m = None
            while True:                                       # FindNextSpecialToken (TikTokenizer.cs:230-241)
                m = self._special_re.search(text, find)
                if m is None or m.group(0) in allowed:
                    break
                find = m.start() + 1
            end = m.start() if m else len(text)
            if end > start:
                out.append(("t", text[start:end], None))
            if m is None:
                break
            out.append(("s", self.SpecialTokensEncoder[m.group(0)], m.group(0)))   # EncodeSpecialToken (:215-220)
            start = m.end()
            if start >= len(text):
                break
        return out

    def _resolve_allowed(self, allowedSpecialOrApply):
        if isinstance(allowedSpecialOrApply, bool):           # Encode(string, bool applySpecialTokens = true)  (:193-207)
            return self.SpecialTokens if (allowedSpecialOrApply and self.SpecialTokens) else None
        return allowedSpecialOrApply                          # Encode(string, IReadOnlyCollection<string>)     (:178-185)

    # ---- ITokenizer --------------------------------------------------------------------------------
    def Encode(self, text: str, allowedSpecialOrApply: Union[bool, Sequence[str], None] = True) -> List[int]:
        """With special tokens allowed: ONE call of the device's single-text special entry (tkz_encode_special_utf8), which is one kernel launch for a prompt,
        under the conditions in which EncodeBatchFlat takes the device's special entry; everything else is EncodeBatch of the one text."""
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        if allowed and self._special_re is not None and not self._special_on_host and not (self._fffd_literal and _has_lone_surrogate(text)):
            names = set(allowed)
            index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]       # (registration order = the alternation's)
            try:
                return self._encoder.encode_special(_utf8_like_dotnet(text), index)
            except N.UnsupportedError:
                self._special_on_host = True                  # (EncodeBatchFlat's host segmentation, from here on)
        return self.EncodeBatch([text], allowedSpecialOrApply)[0]

    def EncodeBatch(self, texts: Sequence[str], allowedSpecialOrApply: Union[bool, Sequence[str], None] = True) -> List[List[int]]:
        ids, offs = self.EncodeBatchFlat(texts, allowedSpecialOrApply)
        flat = ids.tolist()
        return [flat[offs[d]:offs[d + 1]] for d in range(len(texts))]

    def EncodeBatchFlat(self, texts: Sequence[str], allowedSpecialOrApply: Union[bool, Sequence[str], None] = True):
        """EncodeBatch without a list per text: (ids int32[total], offsets int64[len(texts) + 1]); text d is ids[offsets[d]:offsets[d+1]].
        When no special token applies (the reference's plain path, TikTokenizer.cs:180-183,196-199) the arrays are the device call's own
        output, untouched; with special tokens allowed likewise: ONE call of the device's special entry on the texts as they are (the literals
        are cut out on the device, tkz_encode_batch_special_utf8).  Only a set of literals the device path does not hold (UnsupportedError), or a text with a
        lone surrogate while a literal holds U+FFFD, is segmented here and spliced."""
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        device_special = not plain and not self._special_on_host
        if device_special and self._fffd_literal:
            # Encoding.UTF8.GetBytes turns a lone surrogate into EF BF BD, which a literal holding U+FFFD would match on bytes but not in the reference's UTF-16 search
            device_special = not any(_has_lone_surrogate(t) for t in texts)
        if plain or device_special:
            segs = [_utf8_like_dotnet(t) for t in texts]
            if not segs:
                return np.zeros(0, np.int32), np.zeros(1, np.int64)
            lens = np.fromiter(map(len, segs), np.int64, len(segs))
            offs = np.zeros(len(segs) + 1, np.int64)
            np.cumsum(lens, out=offs[1:])
            data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
            if plain:
                return self._encoder.encode_batch(data, offs)
            names = set(allowed)
            index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]       # (registration order = the alternation's)
            try:
                return self._encoder.encode_batch_special(data, offs, index)
            except N.UnsupportedError:
                self._special_on_host = True                  # (more than 256 literals, one beyond 128 bytes ...: the host segmentation below, from here on)
        plans = [self._segments(t, allowed) for t in texts]
        segs = [_utf8_like_dotnet(s) for plan in plans for kind, s, _ in plan if kind == "t"]
        if segs:
            data = np.frombuffer(b"".join(segs), np.uint8) if sum(map(len, segs)) else np.zeros(0, np.uint8)
            offs = np.cumsum([0] + [len(s) for s in segs]).astype(np.int64)
            ids, ooff = self._encoder.encode_batch(data, offs)
        else:
            ids, ooff = np.zeros(0, np.int32), np.zeros(1, np.int64)
        n_special = sum(1 for plan in plans for kind, _, _ in plan if kind == "s")
        out = np.empty(len(ids) + n_special, np.int32)
        out_offs = np.zeros(len(texts) + 1, np.int64)
        w, k = 0, 0
        for d, plan in enumerate(plans):
            for kind, v, _ in plan:
                if kind == "s":
                    out[w] = v
                    w += 1
                else:
                    n = int(ooff[k + 1] - ooff[k])
                    out[w:w + n] = ids[ooff[k]:ooff[k + 1]]
                    w += n
                    k += 1
            out_offs[d + 1] = w
        return out, out_offs

    # ---- counts: Encode(...).Count without the ids ---------------------------------------------------
    def CountTokens(self, text: str, allowedSpecialOrApply: Union[bool, Sequence[str], None] = True) -> int:
        """len(Encode(text, allowedSpecialOrApply)) from the device's count entry (tkz_count_utf8: one kernel launch for a prompt, no ids stored or copied), under
        the conditions in which Encode takes the device's entries; where the device special path refuses the registered set, len(Encode(...))."""
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        if plain or not (self._special_on_host or (self._fffd_literal and _has_lone_surrogate(text))):
            names = set(allowed) if not plain else ()
            index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]
            try:
                return self._encoder.count(_utf8_like_dotnet(text), index)
            except N.UnsupportedError:
                self._special_on_host = True
        return len(self.Encode(text, allowedSpecialOrApply))

    def CountTokensBatch(self, texts: Sequence[str], allowedSpecialOrApply: Union[bool, Sequence[str], None] = True) -> List[int]:
        """[len(x) for x in EncodeBatch(texts, allowedSpecialOrApply)] from the device's batch count entry (tkz_count_batch_utf8): only the offsets come back."""
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        if not texts:
            return []
        if plain or not (self._special_on_host or (self._fffd_literal and any(_has_lone_surrogate(t) for t in texts))):
            segs = [_utf8_like_dotnet(t) for t in texts]
            offs = np.zeros(len(segs) + 1, np.int64)
            np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
            data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
            names = set(allowed) if not plain else ()
            index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]
            try:
                return np.diff(self._encoder.count_batch(data, offs, index)).tolist()
            except N.UnsupportedError:
                self._special_on_host = True
        return [len(x) for x in self.EncodeBatch(texts, allowedSpecialOrApply)]

    # ---- token spans: which part of the text is token t -------------------------------------------------
    def EncodeWithOffsets(self, text: str, allowedSpecialOrApply: Union[bool, Sequence[str], None] = True, bytes: bool = False):
        """(ids, starts): Encode(text, allowedSpecialOrApply) and, per token, where its text starts.  starts[t] indexes the `str` as .NET / JavaScript index a
        string -- in UTF-16 CODE UNITS, which is a Python index as long as the text stays inside the BMP --: token t is the units starts[t] .. starts[t + 1], the
        last one ends at the text's length in units.  A token that starts inside a character (byte-level BPE splits emoji and CJK under an English vocabulary) starts
        AFTER that character's units, and a token of continuation bytes only has an empty span.  bytes=True: offsets into text.encode("utf-8") instead, where the
        spans are exactly the tokens' keys.  (HuggingFace's offset_mapping, tiktoken's decode_with_offsets, EncodeToTokens' Offset.)"""
        ids, starts = self.EncodeWithOffsetsBatch([text], allowedSpecialOrApply, bytes)
        return ids[0], starts[0]

    def EncodeWithOffsetsBatch(self, texts: Sequence[str], allowedSpecialOrApply: Union[bool, Sequence[str], None] = True, bytes: bool = False):
        """([ids of text d], [starts of text d]) from ONE call of the device's span entry (tkz_encode_batch_spans_utf8)."""
        if not texts:
            return [], []
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        if not plain and (self._special_on_host or (self._fffd_literal and any(_has_lone_surrogate(t) for t in texts))):
            raise N.UnsupportedError(N.E_UNSUPPORTED, "EncodeWithOffsets: the device's special entries do not hold this set of literals (or a literal holds U+FFFD "
                                                      "and a text a lone surrogate)")
        segs = [_utf8_like_dotnet(t) for t in texts]
        offs = np.zeros(len(segs) + 1, np.int64)
        np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
        data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
        names = set(allowed) if not plain else ()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]
        ids, ooff, tb, tu = self._encoder.encode_batch_spans(data, offs, index, want_bytes=bytes, want_units=not bytes)
        flat, pos = ids.tolist(), (tb if bytes else tu).tolist()
        return [flat[ooff[d]:ooff[d + 1]] for d in range(len(texts))], [pos[ooff[d]:ooff[d + 1]] for d in range(len(texts))]

    # ---- packed rows: framing, rows of the context length, positions and segment starts (include/tkz.h, "Packed rows") ----
    def _frame_id(self, tok) -> int:
        """a framing id: None (none), an int taken as it is, or the literal of a registered special token"""
        if tok is None:
            return -1
        if isinstance(tok, str):
            if tok not in self.SpecialTokensEncoder:
                raise ValueError("not a registered special token: %r" % tok)
            return int(self.SpecialTokensEncoder[tok])
        if int(tok) < 0:
            raise ValueError("a framing id is not negative")
        return int(tok)

    def EncodeBatchPacked(self, texts: Sequence[str], row_len: int, allowedSpecialOrApply: Union[bool, Sequence[str], None] = True, bos=None, eos=None, pad: int = 0):
        """(ids[n_rows, row_len], pos[n_rows, row_len], seg_starts, doc_offsets) as numpy arrays, from ONE device call (tkz_encode_batch_packed_utf8 / _utf16): every
        text's ids -- Encode's for the same arguments -- with `bos` in front and `eos` behind it, the stream cut into rows of row_len and padded with `pad`;
        pos restarts at every document and every row, seg_starts (cu_seqlens) ends with the stream's length, doc_offsets[d] is where text d starts in the stream.
        bos / eos: None, an int, or the literal of a registered special token."""
        if row_len < 1:
            raise ValueError("row_len must be at least 1")
        bos_id, eos_id = self._frame_id(bos), self._frame_id(eos)
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        if not plain and self._special_on_host:
            raise N.UnsupportedError(N.E_UNSUPPORTED, "EncodeBatchPacked: the device's special entries do not hold this set of literals")
        names = set(allowed) if not plain else ()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]
        if not plain and self._fffd_literal and any(_has_lone_surrogate(t) for t in texts):
            # (a literal that holds U+FFFD beside a lone surrogate: only the UTF-16 entry tells the two apart)
            raw = [t.encode("utf-16-le", "surrogatepass") for t in texts]
            offs = np.zeros(len(raw) + 1, np.int64)
            np.cumsum(np.fromiter((len(r) // 2 for r in raw), np.int64, len(raw)), out=offs[1:])
            ids, ooff, pos, seg, _ = self._encoder.encode_batch_packed_utf16(np.frombuffer(b"".join(raw), "<u2"), offs, row_len, index, bos_id, eos_id, pad)
            return ids, pos, seg, ooff
        segs = [_utf8_like_dotnet(t) for t in texts]
        offs = np.zeros(len(segs) + 1, np.int64)
        np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
        data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
        ids, ooff, pos, seg, _ = self._encoder.encode_batch_packed(data, offs, row_len, index, bos_id, eos_id, pad)
        return ids, pos, seg, ooff

    # ---- padded rows: truncation, framing, padding to a common width and the attention mask (include/tkz.h, "Padded rows") ----
    def EncodeBatchPadded(self, texts: Sequence[str], max_length: int, allowedSpecialOrApply: Union[bool, Sequence[str], None] = True, bos=None, eos=None, pad: int = 0,
                          truncation_side: str = "right", padding_side: str = "right", pad_to_multiple_of: int = 1, fixed_width: bool = False, return_pos: bool = False):
        """(ids[n, W], mask[n, W], lens) as numpy arrays -- and pos[n, W] with return_pos -- from ONE device call (tkz_encode_batch_padded_utf8 / _utf16): every
        text's ids -- Encode's for the same arguments -- cut to max_length less the framing (truncation_side "right" keeps the head, "left" the tail), with `bos` in
        front and `eos` behind what is kept, a row a text, padded with `pad` on padding_side to the longest row rounded up to pad_to_multiple_of (at most
        max_length), or to max_length itself with fixed_width.  mask is 1 on content (uint8; .view(bool) is free), lens the content lengths.  bos / eos: None, an
        int, or the literal of a registered special token.  The cut is a plain cut of the id list, not EncodeTrimSuffix's whole-item cut."""
        sides = {"right": 0, "left": 1}
        if truncation_side not in sides or padding_side not in sides:
            raise ValueError("truncation_side and padding_side are 'right' or 'left'")
        bos_id, eos_id = self._frame_id(bos), self._frame_id(eos)
        if max_length < max(1, (bos_id >= 0) + (eos_id >= 0)) or max_length >= 1 << 31:
            raise ValueError("max_length must hold the framing ids, and one id at least")
        if pad_to_multiple_of < 1 or pad_to_multiple_of >= 1 << 31:
            raise ValueError("pad_to_multiple_of must be at least 1")
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        if not plain and self._special_on_host:
            raise N.UnsupportedError(N.E_UNSUPPORTED, "EncodeBatchPadded: the device's special entries do not hold this set of literals")
        names = set(allowed) if not plain else ()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]
        args = (max_length, index, bos_id, eos_id, pad, sides[truncation_side], sides[padding_side], 0 if fixed_width else pad_to_multiple_of, True, return_pos, False)
        if not plain and self._fffd_literal and any(_has_lone_surrogate(t) for t in texts):
            # (a literal that holds U+FFFD beside a lone surrogate: only the UTF-16 entry tells the two apart)
            raw = [t.encode("utf-16-le", "surrogatepass") for t in texts]
            offs = np.zeros(len(raw) + 1, np.int64)
            np.cumsum(np.fromiter((len(r) // 2 for r in raw), np.int64, len(raw)), out=offs[1:])
            ids, mask, pos, lens, _, _, _ = self._encoder.encode_batch_padded_utf16(np.frombuffer(b"".join(raw), "<u2"), offs, *args)
        else:
            segs = [_utf8_like_dotnet(t) for t in texts]
            offs = np.zeros(len(segs) + 1, np.int64)
            np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
            data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
            ids, mask, pos, lens, _, _, _ = self._encoder.encode_batch_padded(data, offs, *args)
        return (ids, mask, lens, pos) if return_pos else (ids, mask, lens)

    # ---- length-bucketed padded rows: sorted by length, a width per mini-batch (include/tkz.h, "Length-bucketed padded rows") ----
    def EncodeBatchBucketed(self, texts: Sequence[str], max_length: int, bucket_rows: int, allowedSpecialOrApply: Union[bool, Sequence[str], None] = True, bos=None, eos=None,
                            pad: int = 0, descending: bool = False, truncation_side: str = "right", padding_side: str = "right", pad_to_multiple_of: int = 1,
                            fixed_width: bool = False, return_pos: bool = False):
        """(buckets, order, rank, lens) from ONE device call (tkz_encode_batch_bucketed_utf8 / _utf16): what EncodeBatchPadded makes of every text, with the texts
        sorted by content length (ascending, or descending; equal lengths keep the texts' order), cut into mini-batches of bucket_rows rows and every mini-batch
        padded to ITS OWN longest row (rounded up to pad_to_multiple_of, at most max_length; max_length itself with fixed_width).  buckets is a list of
        (ids[R_b, W_b], mask[R_b, W_b]) -- and pos[R_b, W_b] with return_pos --, views of one buffer each; row i of bucket b is text order[b * bucket_rows + i],
        rank is the inverse of order, lens the content lengths in the texts' order."""
        sides = {"right": 0, "left": 1}
        if truncation_side not in sides or padding_side not in sides:
            raise ValueError("truncation_side and padding_side are 'right' or 'left'")
        bos_id, eos_id = self._frame_id(bos), self._frame_id(eos)
        if max_length < max(1, (bos_id >= 0) + (eos_id >= 0)) or max_length >= 1 << 31:
            raise ValueError("max_length must hold the framing ids, and one id at least")
        if pad_to_multiple_of < 1 or pad_to_multiple_of >= 1 << 31:
            raise ValueError("pad_to_multiple_of must be at least 1")
        if bucket_rows < 1 or bucket_rows >= 1 << 31:
            raise ValueError("bucket_rows must be at least 1")
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        if not plain and self._special_on_host:
            raise N.UnsupportedError(N.E_UNSUPPORTED, "EncodeBatchBucketed: the device's special entries do not hold this set of literals")
        names = set(allowed) if not plain else ()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]
        args = (max_length, bucket_rows, N.BUCKET_DESCENDING if descending else N.BUCKET_ASCENDING, index, bos_id, eos_id, pad, sides[truncation_side], sides[padding_side],
                0 if fixed_width else pad_to_multiple_of, True, return_pos, False, True)
        if not plain and self._fffd_literal and any(_has_lone_surrogate(t) for t in texts):
            # (a literal that holds U+FFFD beside a lone surrogate: only the UTF-16 entry tells the two apart)
            raw = [t.encode("utf-16-le", "surrogatepass") for t in texts]
            offs = np.zeros(len(raw) + 1, np.int64)
            np.cumsum(np.fromiter((len(r) // 2 for r in raw), np.int64, len(raw)), out=offs[1:])
            r = self._encoder.encode_batch_bucketed_utf16(np.frombuffer(b"".join(raw), "<u2"), offs, *args)
        else:
            segs = [_utf8_like_dotnet(t) for t in texts]
            offs = np.zeros(len(segs) + 1, np.int64)
            np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
            data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
            r = self._encoder.encode_batch_bucketed(data, offs, *args)
        ids, mask, pos, lens, _, order, rank, boffs, widths = r[:9]
        buckets = []
        for b, W in enumerate(widths.tolist()):
            rows = min(bucket_rows, len(texts) - b * bucket_rows)
            cut = slice(int(boffs[b]), int(boffs[b + 1]))
            views = (ids[cut].reshape(rows, W), mask[cut].reshape(rows, W)) + ((pos[cut].reshape(rows, W),) if return_pos else ())
            buckets.append(views)
        return buckets, order, rank, lens

    # ---- token-budget buckets: sorted by length, mini-batches of at most max_tokens positions (include/tkz.h, "Token-budget buckets") ----
    def EncodeBatchBudgeted(self, texts: Sequence[str], max_length: int, max_tokens: int, max_rows: Union[int, None] = None,
                            allowedSpecialOrApply: Union[bool, Sequence[str], None] = True, bos=None, eos=None, pad: int = 0, descending: bool = False,
                            truncation_side: str = "right", padding_side: str = "right", pad_to_multiple_of: int = 1, fixed_width: bool = False, return_pos: bool = False):
        """(buckets, order, rank, lens) from ONE device call (tkz_encode_batch_budgeted_utf8 / _utf16): what EncodeBatchBucketed makes of the texts, with the sorted
        list cut greedily by a TOKEN budget: a mini-batch takes rows while rows * width <= max_tokens (the width of its longest row, rounded as pad_to_multiple_of
        says) and rows <= max_rows (None: no cap).  buckets is a list of (ids[R_b, W_b], mask[R_b, W_b]) -- and pos[R_b, W_b] with return_pos --, views of one buffer
        each; the rows of the buckets, one after the other, are the texts order[0], order[1], ...; rank is the inverse of order, lens the content lengths in the
        texts' order."""
        sides = {"right": 0, "left": 1}
        if truncation_side not in sides or padding_side not in sides:
            raise ValueError("truncation_side and padding_side are 'right' or 'left'")
        bos_id, eos_id = self._frame_id(bos), self._frame_id(eos)
        if max_length < max(1, (bos_id >= 0) + (eos_id >= 0)) or max_length >= 1 << 31:
            raise ValueError("max_length must hold the framing ids, and one id at least")
        if pad_to_multiple_of < 1 or pad_to_multiple_of >= 1 << 31:
            raise ValueError("pad_to_multiple_of must be at least 1")
        if max_tokens < max_length or max_tokens > 1 << 62:
            raise ValueError("max_tokens must hold one row of max_length")
        if max_rows is not None and (max_rows < 1 or max_rows >= 1 << 31):
            raise ValueError("max_rows must be at least 1")
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        if not plain and self._special_on_host:
            raise N.UnsupportedError(N.E_UNSUPPORTED, "EncodeBatchBudgeted: the device's special entries do not hold this set of literals")
        names = set(allowed) if not plain else ()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]
        args = (max_length, max_tokens, max_rows, N.BUCKET_DESCENDING if descending else N.BUCKET_ASCENDING, index, bos_id, eos_id, pad, sides[truncation_side],
                sides[padding_side], 0 if fixed_width else pad_to_multiple_of, True, return_pos, False, True)
        if not plain and self._fffd_literal and any(_has_lone_surrogate(t) for t in texts):
            # (a literal that holds U+FFFD beside a lone surrogate: only the UTF-16 entry tells the two apart)
            raw = [t.encode("utf-16-le", "surrogatepass") for t in texts]
            offs = np.zeros(len(raw) + 1, np.int64)
            np.cumsum(np.fromiter((len(r) // 2 for r in raw), np.int64, len(raw)), out=offs[1:])
            r = self._encoder.encode_batch_budgeted_utf16(np.frombuffer(b"".join(raw), "<u2"), offs, *args)
        else:
            segs = [_utf8_like_dotnet(t) for t in texts]
            offs = np.zeros(len(segs) + 1, np.int64)
            np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
            data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
            r = self._encoder.encode_batch_budgeted(data, offs, *args)
        ids, mask, pos, lens, _, order, rank, boffs, brows, widths = r[:10]
        buckets = []
        for b, W in enumerate(widths.tolist()):
            rows = int(brows[b + 1] - brows[b])
            cut = slice(int(boffs[b]), int(boffs[b + 1]))
            views = (ids[cut].reshape(rows, W), mask[cut].reshape(rows, W)) + ((pos[cut].reshape(rows, W),) if return_pos else ())
            buckets.append(views)
        return buckets, order, rank, lens

    # ---- pair rows: two texts a row, truncation by a strategy, framing, separators, type ids and padding (include/tkz.h, "Pair rows") ----
    def EncodeBatchPairs(self, first: Sequence[str], second: Sequence[str], max_length: int, allowedSpecialOrApply: Union[bool, Sequence[str], None] = True, bos=None, sep=None,
                         sep_count: int = 1, eos=None, pad: int = 0, truncation: str = "longest_first", truncation_side: str = "right", padding_side: str = "right",
                         pad_to_multiple_of: int = 1, fixed_width: bool = False, return_pos: bool = False):
        """(ids[n, W], mask[n, W], type_ids[n, W], lens, kept[n, 2]) as numpy arrays -- and pos[n, W] with return_pos -- from ONE device call
        (tkz_encode_batch_pairs_utf8 / _utf16): row i is `bos` first[i] `sep` x sep_count second[i] `eos`, the two texts' ids -- Encode's for the same arguments --
        cut to max_length less the framing by `truncation` ("longest_first": an id at a time from the longer text, from the second on a tie; "only_first";
        "only_second"), truncation_side "right" keeping the heads and "left" the tails, padded with `pad` on padding_side to the longest row rounded up to
        pad_to_multiple_of (at most max_length), or to max_length itself with fixed_width.  mask is 1 on content, type_ids 1 on the second text's ids and the eos
        (uint8 both), lens the content lengths, kept[i] the ids kept of either text.  bos / sep / eos: None, an int, or the literal of a registered special token;
        sep None means no separator.  The cut is a plain cut of the id lists."""
        sides = {"right": 0, "left": 1}
        strategies = {"longest_first": N.TRUNC_LONGEST_FIRST, "only_first": N.TRUNC_ONLY_FIRST, "only_second": N.TRUNC_ONLY_SECOND}
        if len(first) != len(second):
            raise ValueError("first and second must hold as many texts as each other")
        if truncation_side not in sides or padding_side not in sides:
            raise ValueError("truncation_side and padding_side are 'right' or 'left'")
        if truncation not in strategies:
            raise ValueError("truncation is 'longest_first', 'only_first' or 'only_second'")
        bos_id, sep_id, eos_id = self._frame_id(bos), self._frame_id(sep), self._frame_id(eos)
        if sep_count not in (0, 1, 2):
            raise ValueError("sep_count is 0, 1 or 2")
        if sep_id < 0:
            sep_count = 0
        if max_length < max(1, (bos_id >= 0) + sep_count + (eos_id >= 0)) or max_length >= 1 << 31:
            raise ValueError("max_length must hold the framing ids, and one id at least")
        if pad_to_multiple_of < 1 or pad_to_multiple_of >= 1 << 31:
            raise ValueError("pad_to_multiple_of must be at least 1")
        allowed = self._resolve_allowed(allowedSpecialOrApply)
        plain = not allowed or self._special_re is None
        if not plain and self._special_on_host:
            raise N.UnsupportedError(N.E_UNSUPPORTED, "EncodeBatchPairs: the device's special entries do not hold this set of literals")
        names = set(allowed) if not plain else ()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]
        texts = [t for pair in zip(first, second) for t in pair]          # documents 2p and 2p + 1: the two texts of pair p
        args = (max_length, index, bos_id, sep_id, sep_count, eos_id, pad, strategies[truncation], sides[truncation_side], sides[padding_side],
                0 if fixed_width else pad_to_multiple_of, True, True, return_pos, True, False)
        if not plain and self._fffd_literal and any(_has_lone_surrogate(t) for t in texts):
            # (a literal that holds U+FFFD beside a lone surrogate: only the UTF-16 entry tells the two apart)
            raw = [t.encode("utf-16-le", "surrogatepass") for t in texts]
            offs = np.zeros(len(raw) + 1, np.int64)
            np.cumsum(np.fromiter((len(r) // 2 for r in raw), np.int64, len(raw)), out=offs[1:])
            ids, mask, types, pos, lens, kept = self._encoder.encode_batch_pairs_utf16(np.frombuffer(b"".join(raw), "<u2"), offs, *args)[:6]
        else:
            segs = [_utf8_like_dotnet(t) for t in texts]
            offs = np.zeros(len(segs) + 1, np.int64)
            np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
            data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
            ids, mask, types, pos, lens, kept = self._encoder.encode_batch_pairs(data, offs, *args)[:6]
        return (ids, mask, types, lens, kept, pos) if return_pos else (ids, mask, types, lens, kept)

    # ---- trim variants (TikTokenizer.cs:288-579) --------------------------------------------------
    def _piece_items(self, text: str, allowed):
        """The walk both trim variants share: the text as a list of (n_tokens, ids, utf16_length) items in order --
        one item per regex piece of every plain segment (Regex.Matches(text[start..end]), :290,:485) and one per special
        token (:215-220).  All plain segments go to the GPU in one piece-granular call."""
        plan = self._segments(text, allowed)
        segs = [_utf8_like_dotnet(s) for kind, s, _ in plan if kind == "t"]
        items = []
        if segs:
            data = np.frombuffer(b"".join(segs), np.uint8)
            offs = np.cumsum([0] + [len(s) for s in segs]).astype(np.int64)
            ids, dpo, pbo, pto = self._encoder.encode_batch_pieces(data, offs)
            # UTF-16 length of a piece = chars + 4-byte chars (piece.Length, :295): count lead bytes, 0xF0.. twice
            lead = ((data & 0xC0) != 0x80).astype(np.int64) + (data >= 0xF0).astype(np.int64)
            cum = np.concatenate([[0], np.cumsum(lead)])
            u16 = cum[pbo[1:]] - cum[pbo[:-1]]
        k = 0
        for kind, v, lit in plan:
            if kind == "s":
                items.append((1, [v], len(lit.encode("utf-16-le")) // 2, True))
            else:
                for p in range(int(dpo[k]), int(dpo[k + 1])):
                    items.append((int(pto[p + 1] - pto[p]), ids[pto[p]:pto[p + 1]].tolist(), int(u16[p]), False))
                k += 1
        return items

    @staticmethod
    def _utf16_prefix(text: str, n_units: int, drop: bool = False) -> str:
        """text[..n] / text[n..] with n in UTF-16 code units, as the reference slices a .NET string."""
        raw = text.encode("utf-16-le", "surrogatepass")
        if n_units * 2 >= len(raw):
            return "" if drop else text
        part = raw[2 * n_units:] if drop else raw[:2 * n_units]
        return part.decode("utf-16-le", "surrogatepass")

    def _trim_args(self, a, b):
        # EncodeTrimX(string, IReadOnlyCollection<string> allowedSpecial, int maxTokenCount)       (:394-403, :529-536)
        # EncodeTrimX(string, int maxTokenCount, bool applySpecialTokens = true)                   (:412-429, :545-564)
        if isinstance(a, int) and not isinstance(a, bool):
            apply = True if b is None else bool(b)
            return (self.SpecialTokens if (apply and self.SpecialTokens) else None), int(a)
        if b is None:
            raise TypeError("maxTokenCount is required")
        return (a if a else None), int(b)

    def _trim_batch_device(self, texts: Sequence[str], allowed, max_tokens: int, side: int):
        """The batch on the device's trim entry (tkz_encode_batch_trim_utf8: the literals cut out, the pieces counted, the cut chosen and the kept ids compacted
        there): a list of (ids, text), or None when the host walk has to do it -- a set of literals the device path does not hold (UnsupportedError), a text
        with a lone surrogate while a literal holds U+FFFD, a negative maximum (the reference's prefix variant returns the whole text then)."""
        if max_tokens < 0:
            return None
        plain = not allowed or self._special_re is None
        if not plain and (self._special_on_host or (self._fffd_literal and any(_has_lone_surrogate(t) for t in texts))):
            return None
        if not texts:
            return []
        segs = [_utf8_like_dotnet(t) for t in texts]
        offs = np.zeros(len(segs) + 1, np.int64)
        np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
        data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
        names = set(allowed) if not plain else set()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]           # (registration order = the alternation's)
        try:
            ids, ooff, _, units = self._encoder.encode_batch_trim(data, offs, index, side, max_tokens)
        except N.UnsupportedError:
            self._special_on_host = True
            return None
        flat = ids.tolist()
        drop = side == N.TRIM_PREFIX
        return [(flat[ooff[d]:ooff[d + 1]], self._utf16_prefix(t, int(units[d]), drop=drop)) for d, t in enumerate(texts)]

    def EncodeTrimSuffixBatch(self, texts: Sequence[str], a, b=None):
        """EncodeTrimSuffix for every text, in ONE device call: a list of (ids, text).  The two overload shapes of the single-text method."""
        allowed, max_tokens = self._trim_args(a, b)
        out = self._trim_batch_device(texts, allowed, max_tokens, N.TRIM_SUFFIX)
        return out if out is not None else [self._trim_suffix_host(t, allowed, max_tokens) for t in texts]

    def EncodeTrimPrefixBatch(self, texts: Sequence[str], a, b=None):
        """EncodeTrimPrefix for every text, in ONE device call: a list of (ids, text)."""
        allowed, max_tokens = self._trim_args(a, b)
        out = self._trim_batch_device(texts, allowed, max_tokens, N.TRIM_PREFIX)
        return out if out is not None else [self._trim_prefix_host(t, allowed, max_tokens) for t in texts]

    def _trim_one_device(self, text: str, allowed, max_tokens: int, side: int):
        """ONE text on the device's single-text trim entry (tkz_encode_trim_utf8: one kernel launch for a prompt): (ids, text), or None when the host walk has to
        do it -- exactly the cases of _trim_batch_device."""
        if max_tokens < 0:
            return None
        plain = not allowed or self._special_re is None
        if not plain and (self._special_on_host or (self._fffd_literal and _has_lone_surrogate(text))):
            return None
        names = set(allowed) if not plain else set()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]           # (registration order = the alternation's)
        try:
            ids, _, units = self._encoder.encode_trim(_utf8_like_dotnet(text), index, side, max_tokens)
        except N.UnsupportedError:
            self._special_on_host = True
            return None
        return ids, self._utf16_prefix(text, units, drop=side == N.TRIM_PREFIX)

    def EncodeTrimSuffix(self, text: str, a, b=None):
        """Token ids and the text they cover, cut after the last piece / special token that still fits maxTokenCount."""
        allowed, max_tokens = self._trim_args(a, b)
        out = self._trim_one_device(text, allowed, max_tokens, N.TRIM_SUFFIX)
        return out if out is not None else self._trim_suffix_host(text, allowed, max_tokens)

    def EncodeTrimPrefix(self, text: str, a, b=None):
        """Token ids and the text they cover, cut before the first piece boundary that leaves at most maxTokenCount tokens."""
        allowed, max_tokens = self._trim_args(a, b)
        out = self._trim_one_device(text, allowed, max_tokens, N.TRIM_PREFIX)
        return out if out is not None else self._trim_prefix_host(text, allowed, max_tokens)

    # the host walk over _piece_items: the fallback of the batch methods
    def _trim_suffix_host(self, text: str, allowed, max_tokens: int):
        token_ids: List[int] = []
        token_count = 0
        encode_length = 0
        for n, ids, ulen, is_special in self._piece_items(text, allowed):
            token_count += n                                   # (:298,:313,:328; special: :364)
            if token_count <= max_tokens:
                token_ids.extend(ids)
                encode_length += ulen
            else:
                break                                          # the piece that overflows is dropped with everything after it
            if token_count >= max_tokens:
                break                                          # (:340, :356-359, :375-378)
        return token_ids, self._utf16_prefix(text, encode_length)

    def _trim_prefix_host(self, text: str, allowed, max_tokens: int):
        token_ids: List[int] = []
        token_count = 0
        encode_length = 0
        boundaries = [(0, 0)]                                  # tokenCountMap: cumulative tokens -> cumulative UTF-16 length (:438-441)
        for n, ids, ulen, is_special in self._piece_items(text, allowed):
            token_count += n
            encode_length += ulen
            token_ids.extend(ids)
            boundaries.append((token_count, encode_length))
        if token_count <= max_tokens:                          # TrimPrefix (:463-483)
            return token_ids, text
        prefix_tokens = token_count - max_tokens
        cut_tokens, cut_len = 0, 0
        for tc, el in boundaries:
            if tc >= prefix_tokens:
                cut_tokens, cut_len = tc, el
                break
        return token_ids[cut_tokens:], self._utf16_prefix(text, cut_len, drop=True)

    # ---- token-budget chunks: the repeated-EncodeTrimSuffix loop in one call (include/tkz.h, "Token-budget chunks") ----
    def EncodeChunks(self, text: str, a, b=None):
        """The text cut into chunks of at most maxTokenCount tokens: a list of (ids, text).  The two overload shapes of EncodeTrimSuffix.  While no piece exceeds the
        budget the chunks are what `while rest: ids, part = EncodeTrimSuffix(rest, ...); rest = rest[len(part):]` yields; a piece of more tokens than the budget is
        cut into runs of maxTokenCount tokens (that loop would never end there), its last partial run begins a chunk that goes on with the pieces that follow.  The
        ids concatenate to Encode's, the texts -- sliced in UTF-16 code units, a character cut by a chunk boundary goes to the earlier chunk -- to the input.
        maxTokenCount < 1 is a ValueError."""
        return self.EncodeChunksBatch([text], a, b)[0]

    def EncodeChunksBatch(self, texts: Sequence[str], a, b=None):
        """EncodeChunks for every text, in ONE device call (tkz_encode_batch_chunks_utf8): one list of (ids, text) per text."""
        allowed, max_tokens = self._trim_args(a, b)
        if max_tokens < 1:
            raise ValueError("maxTokenCount must be at least 1")
        if not texts:
            return []
        plain = not allowed or self._special_re is None
        if not plain and (self._special_on_host or (self._fffd_literal and any(_has_lone_surrogate(t) for t in texts))):
            return [self._chunks_host(t, allowed, max_tokens) for t in texts]
        segs = [_utf8_like_dotnet(t) for t in texts]
        offs = np.zeros(len(segs) + 1, np.int64)
        np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
        data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
        names = set(allowed) if not plain else set()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]           # (registration order = the alternation's)
        try:
            ids, _, dco, ct, _, cu = self._encoder.encode_batch_chunks(data, offs, max_tokens, index, want_bytes=False)
        except N.UnsupportedError:
            self._special_on_host = True
            return [self._chunks_host(t, allowed, max_tokens) for t in texts]
        flat, ct, cu = ids.tolist(), ct.tolist(), cu.tolist()
        out = []
        for d, t in enumerate(texts):
            lo, hi = int(dco[d]), int(dco[d + 1])
            raw = t.encode("utf-16-le", "surrogatepass")
            cuts = cu[lo:hi] + [len(raw) // 2]
            out.append([(flat[ct[c]:ct[c + 1]], raw[2 * cuts[c - lo]:2 * cuts[c - lo + 1]].decode("utf-16-le", "surrogatepass")) for c in range(lo, hi)])
        return out

    def _units_of_ids(self, ids) -> int:
        """the UTF-16 units begun in the keys of `ids`: one per non-continuation byte, one more per byte >= 0xF0"""
        data, _ = self._encoder.decode_batch(np.asarray(ids, np.int32), np.asarray([0, len(ids)], np.int64))
        data = np.asarray(data, np.uint8)
        return int(((data & 0xC0) != 0x80).sum() + (data >= 0xF0).sum())

    def _chunks_host(self, text: str, allowed, max_tokens: int):
        """the host walk over _piece_items by the rule of tkz.h: the fallback of EncodeChunksBatch"""
        import bisect
        items = self._piece_items(text, allowed)
        flat: List[int] = []
        tcum, ucum = [0], [0]                                   # tokens and UTF-16 units in front of every item
        for n, ids, ulen, _ in items:
            flat.extend(ids)
            tcum.append(tcum[-1] + n)
            ucum.append(ucum[-1] + ulen)
        total = tcum[-1]
        starts = []                                            # (first token, first unit) of every chunk
        s = p = 0                                              # the chunk starts at token s, in (or at the start of) item p
        while s < total:
            starts.append((s, ucum[p] + (self._units_of_ids(items[p][1][:s - tcum[p]]) if s > tcum[p] else 0)))
            if total - s <= max_tokens:
                break
            k = bisect.bisect_right(tcum, s + max_tokens) - 1   # the last boundary at or below s + max
            if tcum[k] > s:
                s, p = tcum[k], k
            else:
                s += max_tokens                                # (no boundary in reach: inside item p)
        raw = text.encode("utf-16-le", "surrogatepass")
        ends = starts[1:] + [(total, len(raw) // 2)]
        return [(flat[s:e], raw[2 * u:2 * v].decode("utf-16-le", "surrogatepass")) for (s, u), (e, v) in zip(starts, ends)]

    # ---- overlapping token-budget chunks: a chunk size and an overlap (include/tkz.h, "Overlapping token-budget chunks") ----
    def EncodeChunksOverlap(self, text: str, a, b, c=None):
        """EncodeChunks with an overlap: a list of (ids, text) whose consecutive entries share at most `overlap` tokens, and the text of those tokens.  The shapes
        are (text, allowedSpecial, maxTokenCount, overlap) and (text, maxTokenCount, overlap, applySpecialTokens = True).  A chunk is what EncodeTrimSuffix(rest,
        maxTokenCount) returns; the next one starts with what EncodeTrimPrefix(chunk text, overlap) keeps -- one item further on when that is the whole chunk, and
        behind the chunk when a chunk begun there would end where this one does.  overlap = 0 gives EncodeChunks' result.  The texts are slices of the input in
        UTF-16 code units.  maxTokenCount < 1, overlap < 0 and overlap >= maxTokenCount are a ValueError."""
        return self.EncodeChunksOverlapBatch([text], a, b, c)[0]

    def EncodeChunksOverlapBatch(self, texts: Sequence[str], a, b, c=None):
        """EncodeChunksOverlap for every text, in ONE device call (tkz_encode_batch_chunks_overlap_utf8): one list of (ids, text) per text."""
        if isinstance(a, int) and not isinstance(a, bool):
            (allowed, max_tokens), overlap = self._trim_args(a, c), int(b)
        else:
            if c is None:
                raise TypeError("overlap is required")
            (allowed, max_tokens), overlap = self._trim_args(a, b), int(c)
        if max_tokens < 1:
            raise ValueError("maxTokenCount must be at least 1")
        if not 0 <= overlap < max_tokens:
            raise ValueError("overlap must be at least 0 and below maxTokenCount")
        if not texts:
            return []
        plain = not allowed or self._special_re is None
        if not plain and (self._special_on_host or (self._fffd_literal and any(_has_lone_surrogate(t) for t in texts))):
            return [self._chunks_overlap_host(t, allowed, max_tokens, overlap) for t in texts]
        segs = [_utf8_like_dotnet(t) for t in texts]
        offs = np.zeros(len(segs) + 1, np.int64)
        np.cumsum(np.fromiter(map(len, segs), np.int64, len(segs)), out=offs[1:])
        data = np.frombuffer(b"".join(segs), np.uint8) if offs[-1] else np.zeros(0, np.uint8)
        names = set(allowed) if not plain else set()
        index = [i for i, k in enumerate(self.SpecialTokensEncoder) if k in names]           # (registration order = the alternation's)
        try:
            ids, _, dco, ct, ce, _, cu, _, ceu = self._encoder.encode_batch_chunks_overlap(data, offs, max_tokens, overlap, index, want=(False, True, False, True))
        except N.UnsupportedError:
            self._special_on_host = True
            return [self._chunks_overlap_host(t, allowed, max_tokens, overlap) for t in texts]
        flat, ct, ce, cu, ceu = ids.tolist(), ct.tolist(), ce.tolist(), cu.tolist(), ceu.tolist()
        out = []
        for d, t in enumerate(texts):
            raw = t.encode("utf-16-le", "surrogatepass")
            out.append([(flat[ct[k]:ce[k]], raw[2 * cu[k]:2 * ceu[k]].decode("utf-16-le", "surrogatepass")) for k in range(int(dco[d]), int(dco[d + 1]))])
        return out

    def _chunks_overlap_host(self, text: str, allowed, max_tokens: int, overlap: int):
        """the host walk over _piece_items by the rule of tkz.h: the fallback of EncodeChunksOverlapBatch"""
        import bisect
        items = self._piece_items(text, allowed)
        flat: List[int] = []
        tcum, ucum = [0], [0]                                   # tokens and UTF-16 units in front of every item
        for n, ids, ulen, _ in items:
            flat.extend(ids)
            tcum.append(tcum[-1] + n)
            ucum.append(ucum[-1] + ulen)
        total = tcum[-1]

        def end_of(s):                                         # the chunk rule's end for a chunk that starts at s
            if total - s <= max_tokens:
                return total
            k = bisect.bisect_right(tcum, s + max_tokens) - 1
            return tcum[k] if tcum[k] > s else s + max_tokens

        def unit_of(t):                                        # the UTF-16 unit token t starts at
            p = bisect.bisect_right(tcum, t) - 1
            return ucum[p] + (self._units_of_ids(items[p][1][:t - tcum[p]]) if t > tcum[p] else 0) if t < total else ucum[-1]
        out = []
        raw = text.encode("utf-16-le", "surrogatepass")
        s = 0
        while s < total:
            e = end_of(s)
            out.append((flat[s:e], raw[2 * unit_of(s):2 * unit_of(e)].decode("utf-16-le", "surrogatepass")))
            if e == total:
                break
            x = max(e - overlap, s + 1)
            i = bisect.bisect_left(tcum, x)
            n = tcum[i] if tcum[i] <= e else x                 # the first boundary in [x, e], else x inside the item
            s = e if end_of(n) == e else n                     # (a chunk begun at n that ends at e again adds nothing)
        return out

    def Decode(self, tokens: Sequence[int]) -> str:
        """TikTokenizer.cs:586-604: ids that are neither in the vocabulary nor special tokens are dropped; the bytes are decoded as
        UTF-8 (Encoding.UTF8.GetString: malformed sequences become U+FFFD).  One id list is one kernel launch (tkz_decode_utf8)."""
        return self._encoder.decode(self._int32_ids(tokens)).tobytes().decode("utf-8", "replace")

    @staticmethod
    def _int32_ids(tokens):
        flat = np.asarray(list(tokens), dtype=np.int64)
        return np.where((flat < -2**31) | (flat >= 2**31), -1, flat).astype(np.int32)      # (an id outside int is in no table)

    def DecodeBatch(self, batches: Sequence[Sequence[int]]) -> List[str]:
        """Decode for a batch, on the device (tkz_decode_batch: id -> bytes gather through the decoder table + scan)."""
        flat = np.asarray([t for b in batches for t in b], dtype=np.int64)
        flat = np.where((flat < -2**31) | (flat >= 2**31), -1, flat).astype(np.int32)      # (an id outside int is in no table)
        offs = np.cumsum([0] + [len(b) for b in batches]).astype(np.int64)
        data, boffs = self._encoder.decode_batch(flat, offs)
        raw = data.tobytes()
        return [raw[boffs[d]:boffs[d + 1]].decode("utf-8", "replace") for d in range(len(batches))]

    def DecodeUtf16(self, tokens: Sequence[int]) -> str:
        """Decode with Encoding.UTF8.GetString done on the device as well: the same string as Decode."""
        return self._encoder.decode_utf16(self._int32_ids(tokens)).astype("<u2", copy=False).tobytes().decode("utf-16-le")

    def DecodeBatchUtf16(self, batches: Sequence[Sequence[int]]) -> List[str]:
        """DecodeBatch through tkz_decode_batch_utf16: the device hands back the UTF-16 code units of every document (malformed sequences already U+FFFD, one
        per maximal subpart), so the units are well-formed and the conversion below is exact."""
        flat = np.asarray([t for b in batches for t in b], dtype=np.int64)
        flat = np.where((flat < -2**31) | (flat >= 2**31), -1, flat).astype(np.int32)      # (an id outside int is in no table)
        offs = np.cumsum([0] + [len(b) for b in batches]).astype(np.int64)
        units, uoffs = self._encoder.decode_batch_utf16(flat, offs)
        units = units.astype("<u2", copy=False)
        return [units[uoffs[d]:uoffs[d + 1]].tobytes().decode("utf-16-le") for d in range(len(batches))]

    # the raw device encoder, for callers that hold documents in HBM (bench.py)
    @property
    def native(self) -> N.Encoder:
        return self._encoder


class TokenizerBuilder:
    """TokenizerBuilder.cs:14-214 without the HTTP download: rank files are read from a directory
    (`vocab_dir`, default $TKZ_VOCAB_DIR), because the build has no network."""

    @staticmethod
    def _encoder_for_model(modelName: str) -> str:
        enc = MODEL_TO_ENCODING.get(modelName)
        if enc is None:
            for prefix, e in MODEL_PREFIX_TO_ENCODING.items():
                if modelName.startswith(prefix):
                    enc = e
                    break
        if enc is None:
            raise NotImplementedError("Doesn't support this model [%s]" % modelName)       # TokenizerBuilder.cs:96
        return enc

    @staticmethod
    def CreateByModelName(modelName: str, extraSpecialTokens: Optional[Dict[str, int]] = None, vocab_dir: Optional[str] = None, device: int = 0,
                          host: Optional[str] = None, lib: Optional[N.Library] = None):
        return TokenizerBuilder.CreateByEncoderName(TokenizerBuilder._encoder_for_model(modelName), extraSpecialTokens, vocab_dir, device, host, lib)

    @staticmethod
    def CreateByEncoderName(encoderName: str, extraSpecialTokens: Optional[Dict[str, int]] = None, vocab_dir: Optional[str] = None, device: int = 0,
                            host: Optional[str] = None, lib: Optional[N.Library] = None):
        """`host=None` picks the engine of the reference that DEFINES the encoder (ENCODER_ENGINE): o200k_base / gpt-4o exist only in the
        TypeScript reference, whose `new RegExp(pattern, "gu")` matches by code point with ECMAScript's \\s ("js"); every other encoder is the
        C# reference's ("dotnet").  An explicit `host` overrides that (e.g. "dotnet" for a C# host that hands the o200k string to
        TokenizerBuilder.CreateTokenizer(stream, specials, pattern) itself)."""
        if encoderName not in ENCODERS:
            raise NotImplementedError("Doesn't support this encoder [%s]" % encoderName)  # TokenizerBuilder.cs:179
        if host is None:
            host = ENCODER_ENGINE.get(encoderName, "dotnet")
        regex, fname, specials = ENCODERS[encoderName]
        specials = dict(specials)
        if extraSpecialTokens:
            specials.update(extraSpecialTokens)
        d = vocab_dir or os.environ.get("TKZ_VOCAB_DIR") or "."
        path = os.path.join(d, fname)
        if not os.path.exists(path):
            raise FileNotFoundError("%s not found: the reference downloads it at run time (TokenizerBuilder.cs:113,195); "
                                    "place it in vocab_dir / $TKZ_VOCAB_DIR" % path)
        with open(path, "rb") as f:
            return TokenizerBuilder.CreateTokenizer(f.read(), specials, regex, device=device, lib=lib, host=host)

    @staticmethod
    def CreateTokenizer(tikTokenBpeFile: bytes, specialTokensEncoder: Optional[Dict[str, int]], pattern: str, cacheSize: int = 8192,
                        device: int = 0, lib: Optional[N.Library] = None, host: str = "dotnet", unicode_classes=None,
                        case_equivalence: bool = False) -> TikTokenizer:
        return TikTokenizer(tikTokenBpeFile, specialTokensEncoder, pattern, cacheSize, device, lib, host, unicode_classes, case_equivalence)
