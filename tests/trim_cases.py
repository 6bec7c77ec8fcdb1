"""EncodeTrimSuffix / EncodeTrimPrefix for a batch on the device (tkz_encode_batch_trim_utf8 / _device): the expected values and the comparison the
emulated (CPU) and the GPU test modules share.  Every comparison is exact -- kept ids, offsets, cut_bytes, cut_units -- against oracle.TrimOracle's
restatement of TikTokenizer.cs:288-579, text by text."""
import numpy as np

import parity
import special_cases as SC
from tokenizer_amd import _native as N

SIDES = (N.TRIM_SUFFIX, N.TRIM_PREFIX)
IM_START, IM_END = "<|im_start|>", "<|im_end|>"
# the texts of the reference's unit tests (TikTokenizerUnitTest.cs:128-225) and around them
REFERENCE_TEXTS = [IM_START + "Hello World" + IM_END, IM_START + "Hello TempWorld" + IM_END, IM_START + "HelloTemp World" + IM_END,
                   "Hello ⭐ World 😀😀 done" + IM_END + " tail", " 😀", "a 😀 b", "x" + " 😀" * 3]


def utf16_len(s):
    return len(s.encode("utf-16-le", "surrogatepass")) // 2


class Expect:
    """TrimOracle per text, remembered: (kept ids, cut_bytes, cut_units) for (text, allowed, side, max), and the untrimmed token count of (text, allowed)."""

    def __init__(self, O, ovocab, pattern, specials):
        self.oracle = O.TrimOracle(ovocab, pattern, specials)
        self.enc = O.Encoder(ovocab, pattern, specials=specials)
        self._trim, self._count = {}, {}

    def count(self, text, allowed):
        key = (text, tuple(allowed))
        if key not in self._count:
            self._count[key] = len(self.enc.encode(text, list(allowed)))
        return self._count[key]

    def trim(self, text, allowed, side, mx):
        key = (text, tuple(allowed), side, mx)
        if key not in self._trim:
            if side == N.TRIM_SUFFIX:
                ids, kept = self.oracle.encode_trim_suffix(text, list(allowed) or None, mx)
                part = kept                                   # the kept text
            else:
                ids, kept = self.oracle.encode_trim_prefix(text, list(allowed) or None, mx)
                n = utf16_len(text) - utf16_len(kept)         # the dropped text is what is in front of the kept one
                part = text.encode("utf-16-le", "surrogatepass")[:2 * n].decode("utf-16-le", "surrogatepass")
            self._trim[key] = ([int(i) for i in ids], len(part.encode("utf-8")), utf16_len(part))
        return self._trim[key]


def expected(exp, docs, allowed, side, maxima):
    ids, offs, cb, cu = [], [0], [], []
    for d, mx in zip(docs, maxima):
        i, b, u = exp.trim(d, allowed, side, mx)
        ids += i
        offs.append(len(ids))
        cb.append(b)
        cu.append(u)
    return ids, offs, cb, cu


def compare(enc, exp, specials, allowed, docs, side, mx, what="", per_doc=None, call=None):
    """docs: str documents.  mx: the uniform maximum, or -- per_doc -- ignored in favour of one maximum per document.
    call(data, offs, index, side, mx, per_doc) -> (ids, offsets, cut_bytes, cut_units): the entry under test (default: the host entry)."""
    data, offs = parity.pack([d.encode("utf-8") for d in docs])
    index = SC.indices(specials, allowed)
    got = (call or enc.encode_batch_trim)(data, offs, index, side, mx, per_doc)
    maxima = [max(int(m), 0) for m in per_doc] if per_doc is not None else [mx] * len(docs)
    want = expected(exp, docs, allowed, side, maxima)
    for name, g, w in zip(("offsets", "cut_bytes", "cut_units", "ids"), (got[1], got[2], got[3], got[0]), (want[1], want[2], want[3], want[0])):
        g = [int(x) for x in g]
        if g != w:
            k = SC.first_diff(g, w)
            raise AssertionError("%s side %d max %s: %s differ at %d: got %s, expected %s" % (what, side, mx if per_doc is None else "per document", name, k, g[max(0, k - 2):k + 6], w[max(0, k - 2):k + 6]))
    return len(want[0])


def sweep(enc, exp, specials, allowed, docs, side, what=""):
    """Every maximum from 0 to one past the longest document's token count, the whole batch at each (a document that is shorter is kept whole)."""
    top = max([exp.count(d, allowed) for d in docs] + [0]) + 1
    for mx in range(top + 1):
        compare(enc, exp, specials, allowed, docs, side, mx, what)
    return top
