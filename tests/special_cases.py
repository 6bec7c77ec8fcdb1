"""Special tokens on the device (tkz_encode_batch_special_utf8 / _device): the case builders and the comparison the emulated (CPU) and
the GPU test modules share.  Every comparison is bit-exact -- ids and offsets -- against oracle.Encoder(vocab, pattern,
specials=...).encode(text, allowed) per document."""
import random

import numpy as np
import pytest

import parity
import regex_crosscheck as RC
from tokenizer_amd import _native as N
from tokenizer_amd.tokenizer import ENCODERS

EOT = "<|endoftext|>"
# vocabulary (tests/conftest.py: vocab_bytes) -> its special tokens, ids from tokenizer.py: ENCODERS
SPECIAL_SETS = {"gpt2": ENCODERS["gpt2"][2], "synth100k": ENCODERS["cl100k_base"][2], "synth200k": ENCODERS["o200k_base"][2]}
PATTERNS = (1, 2, 3, 4)


def indices(specials, allowed):
    names = list(specials)
    return [names.index(a) for a in allowed if a in names]


def make_encoders(lib, O, vocab, ovocab, pattern, specials):
    enc = N.Encoder(vocab, pattern)
    enc.set_special_tokens(specials)
    return enc, O.Encoder(ovocab, pattern, specials=specials)


def oracle_docs(oenc, docs, allowed):
    ids, offs = [], [0]
    for d in docs:
        ids += oenc.encode(d, list(allowed))
        offs.append(len(ids))
    return ids, offs


def first_diff(got, exp):
    n = min(len(got), len(exp))
    for i in range(n):
        if got[i] != exp[i]:
            return i
    return n


def compare(enc, oenc, specials, allowed, docs, what="", call=None):
    """docs: str documents.  call(data, offs, index) -> (ids, offsets): the entry under test (default: the host entry)."""
    data, offs = parity.pack([d.encode("utf-8") for d in docs])
    index = indices(specials, allowed)
    ids, ooff = (call or enc.encode_batch_special)(data, offs, index)
    eids, eoffs = oracle_docs(oenc, docs, allowed)
    got_offs = [int(x) for x in ooff]
    if got_offs != eoffs:
        d = first_diff(got_offs, eoffs)
        raise AssertionError("%s: offsets differ at document %d: got %s, expected %s; document %r" % (what, d - 1, got_offs[max(0, d - 1):d + 1], eoffs[max(0, d - 1):d + 1], docs[max(0, d - 1)][:200]))
    got = [int(x) for x in ids]
    if got != eids:
        k = first_diff(got, eids)
        d = max(0, int(np.searchsorted(np.asarray(eoffs), k, side="right")) - 1)
        raise AssertionError("%s: ids differ at %d (document %d): got %s, expected %s; document %r" % (what, k, d, got[k:k + 8], eids[k:k + 8], docs[min(d, len(docs) - 1)][:200]))
    return len(eids)


def allowed_choices(specials):
    names = list(specials)
    out = [names, names[:1], []]
    if len(names) > 1:
        out.append(names[1:])                  # a proper subset that leaves the first registered literal out
    return out


def edge_docs(specials, o200k=False):
    """Literals at the start / end of a document, the whole document, back to back, around blanks and newlines, between CJK and emoji, around long pieces, cut
    by a document boundary, beside empty documents; literals that are not allowed simply appear as text under the smaller allowed sets."""
    names = list(specials)
    a = names[0]
    b = names[-1]
    near = [a[:-1], a[1:], a[:-2] + ">", "<|endoftext|", "<|endoftext>", "<endoftext|>"]
    docs = [
        a, a + "hello world", "hello world" + a, a + a, a + b + a, "x" + a + a + a + "y",
        "a   " + a + "b", "a   " + a + "   b", "a\n\n" + a + "\n\nb", "a \n" + a + " \n b", "tab\t\t" + a + "\t\tx", a + " ", " " + a, "  " + a + "  ",
        "don't" + a + "'s it", "12345" + a + "6789", "word" + a + "word", "中文" + a + "中文", "\U0001F600" + a + "\U0001F600⭐" + b, "é" + a + "ß",
        "x" * 1500 + a + "y" * 1500, " " * 1500 + a + " " * 1500, "ab " * 400 + a + "=" * 1200 + a + "q",
        "", a, "", "", "text only, no literal at all", "", b, "",
        "".join(near), " ".join(near), near[3] + a + near[3],
        a[:5], a[5:], a[:-1], ">", "<|", a[2:],             # a literal cut in two by a document boundary: no match
        "the end" + b,
    ]
    if o200k:
        docs += ["a\r\n/" + a + "\r\n/b", "x \r\n\r\n" + a + "\r\n//" + b + "/", "Ab\r\n" + a + "'S", "aB" + a + "Cd\n/" + a]
    return docs


def boundary_docs(lit, boundaries, shifts=None, fill="ab cd "):
    """One document per shift: the literal placed so that it crosses (or touches) byte `boundary` of the BATCH at every offset -- the documents are laid out by
    the caller one per batch.  Returns a list of single-document batches."""
    out = []
    n = len(lit.encode("utf-8"))
    for B in boundaries:
        for k in (shifts if shifts is not None else range(n + 1)):
            pre = B - k
            if pre < 0:
                continue
            body = (fill * (pre // len(fill) + 1))[:pre]
            out.append(body + lit + " tail of the text" + lit)
    return out


def random_docs(rng, specials, n_docs, max_len, kinds=("mix", "runs", "a_mix", "ws", "oth")):
    names = list(specials)
    extra = ["<|endoftext|", EOT[:-1], EOT[1:], EOT[:6] + EOT[7:]]
    docs = []
    alpha = RC.alphabet()
    for _ in range(n_docs):
        n = rng.choice([0, 1, 5, 40, 300, 1000, 1100, 4100]) if rng.random() < 0.6 else rng.randrange(max_len + 1)
        n = min(n, max_len)
        text = parity.gen_text(rng, rng.choice(kinds), n, alpha) if n else ""
        parts, pos = [], 0
        cuts = sorted(rng.randrange(len(text) + 1) for _ in range(rng.choice([0, 1, 1, 2, 5])))
        for c in cuts:
            parts.append(text[pos:c])
            parts.append(rng.choice(names) if rng.random() < 0.7 else rng.choice(extra))
            if rng.random() < 0.2:
                parts.append(rng.choice(names))
            pos = c
        parts.append(text[pos:])
        docs.append("".join(parts))
    return docs


# registration order, overlaps, non-ASCII literals, a literal that is a vocabulary key: (specials, allowed sets, documents)
def order_cases():
    runs = ["a" * n for n in (1, 2, 3, 4, 5, 6, 7, 64, 65, 127, 128, 129, 300)] + ["ab" * n for n in (1, 2, 3, 5, 33, 64, 70)] + ["aabaabaaabab" * 20, "ba" * 40 + "a" * 9 + "b"]
    return [
        ({"<|x": 1001, "<|x|>": 1002}, [["<|x|>"], ["<|x", "<|x|>"], ["<|x"]], ["<|x|>", "a<|x|>b<|x", "<|x<|x|>", "<|<|x|>|>", " <|x|> <|x "]),
        ({"<|x|>": 1002, "<|x": 1001}, [["<|x|>"], ["<|x", "<|x|>"], ["<|x"]], ["<|x|>", "a<|x|>b<|x", "<|x<|x|>", "<|<|x|>|>", " <|x|> <|x "]),
        ({"aa": 2001, "aba": 2002}, [["aa", "aba"], ["aa"], ["aba"]], runs),
        ({"aba": 2002, "aa": 2001}, [["aa", "aba"], ["aa"], ["aba"]], runs),
        ({"<|é中\U0001F600|>": 3001, "中": 3002}, [["<|é中\U0001F600|>", "中"], ["中"], ["<|é中\U0001F600|>"]],
         ["中中中", "x<|é中\U0001F600|>y中", "<|é中\U0001F600|", "é<|é中\U0001F600|>中\U0001F600", "文中文 中 "]),
        ({" the": 4001, "hello": 4002}, [[" the", "hello"], ["hello"]], ["hello the world the", " thehello", "in the theatre hello hellothe"]),
    ]


# ---- special and plain calls side by side: what a call is travels with the call, not with the thread that makes it ----

ROUNDS = 20


def side_by_side_inputs():
    """(a) 8 documents of about 200 bytes, the literal inside each: a plain host call takes the single-launch path.  (b) 160 KiB in 64 documents of 2,560
    bytes, above the single-launch path's 128 KiB: the batch path; a literal across byte 1024 of the batch (a sub-tile edge), one across byte 4096 (a block
    edge), one somewhere in every other document.  ASCII throughout: a character is a byte."""
    rng = random.Random(160)
    words = ["the", "quick", "brown", "fox", "it's", "2024", "tokens", "=>", "x", "  ", "\n", "don't", "Hello", "12345", "(a+b)"]

    def text(n):
        s = ""
        while len(s) < n:
            s += rng.choice(words) + " "
        return s[:n]
    a = [text(90 + 3 * d) + EOT + text(97 - 3 * d) for d in range(8)]
    b = []
    for d in range(64):
        at = {0: 1024 - 6, 1: 4096 - 2560 - 6}.get(d, rng.randrange(2560 - len(EOT)))
        b.append(text(at) + EOT + text(2560 - len(EOT) - at))
    assert all(len(d) == 2560 for d in b) and "".join(b)[1018:1031] == EOT and "".join(b)[4090:4103] == EOT
    return a, b


def check_special_beside_plain(lib, O, vocab, ovocab, pattern, upload=None):
    """Thread A makes special calls (the literal allowed), thread B plain calls of the same buffers, through the host entry and the device entry, ROUNDS times
    on each input: every result is the oracle's for ITS kind of call.  Then, on one thread: a special call that fails its argument check, a plain call, a plain
    _begin, a special call, the _end.  tkz_encoder_special_stats counts the successful special calls and nothing else.
    `upload(np_array) -> (owner, pointer)` as in parity.check_begin_end."""
    import threading
    specials = {EOT: 50256}
    enc, oenc = make_encoders(lib, O, vocab, ovocab, pattern, specials)
    if upload is None:
        upload = lambda arr: (arr, arr.ctypes.data)
    back = lambda o: (o.cpu().numpy() if hasattr(o, "cpu") else o)
    batches = []
    for docs in side_by_side_inputs():
        data, offs = parity.pack([d.encode("utf-8") for d in docs])
        padded = np.zeros(len(data) + 64, np.uint8); padded[:len(data)] = data
        batches.append(dict(data=data, offs=offs, n=len(docs), total=len(data), d_bytes=upload(padded), d_offs=upload(offs.astype(np.int64)),
                            expect={True: oracle_docs(oenc, docs, [EOT]), False: oracle_docs(oenc, docs, [])}))
        assert batches[-1]["expect"][True] != batches[-1]["expect"][False]
    assert batches[0]["total"] <= 2048 and batches[1]["total"] == 160 << 10

    def device_outputs(b):
        return upload(np.zeros(b["total"], np.int32)), upload(np.zeros(b["n"] + 1, np.int64))

    def host_entry(b, special):
        ids, ooff = enc.encode_batch_special(b["data"], b["offs"], [0]) if special else enc.encode_batch(b["data"], b["offs"])
        return ids.tolist(), ooff.tolist()

    def device_entry(b, special, out):
        (ids, p_ids), (ooff, p_ooff) = out
        args = (b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"])
        n = enc.encode_batch_special_device(*args, [0], p_ids, b["total"], p_ooff) if special else enc.encode_batch_device(*args, p_ids, b["total"], p_ooff)
        return back(ids)[:n].tolist(), back(ooff).tolist()

    errors = []

    def work(special):
        outs = [device_outputs(b) for b in batches]          # (each thread its own output buffers)
        try:
            for r in range(ROUNDS):
                for k, b in enumerate(batches):
                    for entry, got in (("host", host_entry(b, special)), ("device", device_entry(b, special, outs[k]))):
                        if got != b["expect"][special]:
                            errors.append("%s entry, %s call, input %s, round %d: not the oracle's result" % (entry, "special" if special else "plain", "ab"[k], r))
        except Exception as ex:          # (a thread's exception would otherwise be lost)
            errors.append(repr(ex))
    small0 = enc.small_path_calls()[0]
    threads = [threading.Thread(target=work, args=(s,)) for s in (True, False)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:5]
    n_special = 2 * 2 * ROUNDS                               # thread A: two entries, two inputs
    assert enc.special_stats()[0] == n_special
    assert enc.small_path_calls()[0] - small0 == ROUNDS      # the plain host calls of (a), and no special call, took the single-launch path

    # one thread, in order
    a, b = batches
    with pytest.raises(N.TkzError) as ei:
        enc.encode_batch_special(a["data"], a["offs"], [1])
    assert ei.value.code == N.E_ARG and "allowed[] holds an index that is not a registered special token" in str(ei.value)
    assert host_entry(b, False) == b["expect"][False]
    out = device_outputs(b)
    h = enc.encode_batch_device_begin(b["d_bytes"][1], b["d_offs"][1], b["n"], b["total"], out[0][1], b["total"], out[1][1])
    assert host_entry(a, True) == a["expect"][True]
    ntok = enc.encode_batch_device_end(h)
    assert (back(out[0][0])[:ntok].tolist(), back(out[1][0]).tolist()) == b["expect"][False]
    assert enc.special_stats()[0] == n_special + 1
