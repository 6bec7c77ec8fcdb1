// A stand-alone driver for a sanitizer build of the host code behind the span entries (tkz_encode_batch_spans_device / _utf8 / _utf16, tkz_encode_spans_utf8 /
// _utf16) and of k_tokspan_mark / k_tokspan_count / k_tokspan_write: tests/test_cpp_spans.py compiles it with the product sources and the CPU SIMT emulator
// (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under -fsanitize=address,undefined and runs it; nothing is loaded into an interpreter.  It walks the
// shapes of tests/spans_cases.py -- a token at every byte, pieces of several tokens across a sub-tile and a word edge, runs of empty documents, crowded miss
// lists on a fresh encoder (the attempt is redone), long and giant pieces, a literal across a sub-tile edge, multi-byte text, the UTF-16 entries with lone
// surrogates, span arrays that are exactly full, one too small and NULL, the argument rows and an empty batch -- twice over one encoder.  Every result is held
// against the encode entry's ids and offsets and against the keys tkz_decode_utf8 returns for the ids: the spans partition every document.  argv: gpt2.tiktoken
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tkz.h"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, tkz_last_error()); return 1; } } while (0)

static uint32_t g_rng = 2463534242u;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }
static const char* kWords[] = {"the", "of", "and", "to", "in", "is", "that", "for", "it", "with", "as", "was", "on", "be", "at", "by", "this", "had", "not", "are"};
static std::string plain(size_t n) { std::string s; while (s.size() < n) { s += kWords[rnd(20)]; s += ' '; } s.resize(n); return s; }
static std::string gib(size_t n, int lo, int hi) {         // consonant strings no vocabulary holds: every piece is a miss of several tokens
    std::string s;
    while (s.size() < n) { s += ' '; for (int k = lo + (int)rnd(hi - lo + 1); k > 0; --k) s += "bcdfghjklmnpqrstvwxz"[rnd(20)]; }
    s.resize(n);
    return s;
}
static int64_t units_begun(const uint8_t* p, int64_t n) { int64_t u = 0; for (int64_t i = 0; i < n; ++i) u += ((p[i] & 0xC0) != 0x80) + (p[i] >= 0xF0); return u; }

struct Batch { std::vector<uint8_t> bytes; std::vector<int64_t> offs{0}; void add(const std::string& d) { bytes.insert(bytes.end(), d.begin(), d.end()); offs.push_back((int64_t)bytes.size()); } };

// the spans of one batch (UTF-8 bytes `text`, byte offsets `offs`) partition every document into the keys of its ids; literal: the allowed special token's id and text
static bool partition(tkz_encoder* e, const uint8_t* text, const std::vector<int64_t>& offs, const std::vector<int32_t>& ids, const std::vector<int64_t>& ooff,
                      const int32_t* tb, const int32_t* tu) {
    uint8_t key[256];
    for (size_t d = 0; d + 1 < offs.size(); ++d) {
        const uint8_t* doc = text + offs[d];
        int64_t pos = 0;
        for (int64_t t = ooff[d]; t < ooff[d + 1]; ++t) {
            int64_t len = 0;
            if (tkz_decode_utf8(e, &ids[(size_t)t], 1, key, sizeof key, &len) != TKZ_OK) return false;
            if (tb && tb[t] != pos) return false;
            if (tu && tu[t] != units_begun(doc, pos)) return false;
            if (pos + len > offs[d + 1] - offs[d] || std::memcmp(doc + pos, key, (size_t)len) != 0) return false;
            pos += len;
        }
        if (pos != offs[d + 1] - offs[d]) return false;
    }
    return true;
}

// the device entry (the emulated build's device memory is host memory) with both arrays, with either one, with a capacity that is exact and one too small; the
// host entry; for a batch of one document the single entry -- against the encode entry's ids and offsets.  allowed: null, or one index
static bool check_batch(tkz_encoder* e, const Batch& b, const int32_t* allowed, int32_t n_allowed) {
    const int64_t n = (int64_t)b.offs.size() - 1, total = b.offs.back();
    void* aligned = nullptr;                                                     // (d_bytes: 16-byte aligned)
    if (tkz_host_alloc((size_t)total + 64, &aligned) != TKZ_OK) return false;
    std::memset(aligned, 0, (size_t)total + 64);
    if (total) std::memcpy(aligned, b.bytes.data(), (size_t)total);
    const uint8_t* d = static_cast<const uint8_t*>(aligned);
    std::vector<int32_t> want_ids((size_t)total + 1), ids((size_t)total + 1, -9);
    std::vector<int64_t> want((size_t)n + 1, -1), got((size_t)n + 1, -2);
    int64_t tw = -1, tg = -2;
    bool ok = (n_allowed ? tkz_encode_batch_special_device(e, d, b.offs.data(), n, total, allowed, n_allowed, want_ids.data(), total, want.data(), nullptr, &tw)
                         : tkz_encode_batch_device(e, d, b.offs.data(), n, total, want_ids.data(), total, want.data(), nullptr, &tw)) == TKZ_OK;
    want_ids.resize((size_t)tw);
    // span arrays of EXACTLY the token count: a store one past the end is the sanitizer's to find
    const size_t room = tw > 0 ? (size_t)tw : 1;                                    // (no tokens: one entry, so that the arrays are not NULL)
    std::vector<int32_t> tb(room), tu(room), xb(room), xu(room);
    ids.assign(room, -9); want_ids.resize(room, -9);
    auto same = [tw](const std::vector<int32_t>& x, const std::vector<int32_t>& y) { return std::equal(x.begin(), x.begin() + tw, y.begin()); };      // (the entries there are)
    ok = ok && tkz_encode_batch_spans_device(e, d, b.offs.data(), n, total, allowed, n_allowed, ids.data(), tw, got.data(), tb.data(), tu.data(), nullptr, &tg) == TKZ_OK;
    ok = ok && tg == tw && got == want && same(ids, want_ids) && partition(e, d, b.offs, ids, got, tb.data(), tu.data());
    ok = ok && tkz_encode_batch_spans_device(e, d, b.offs.data(), n, total, allowed, n_allowed, ids.data(), tw, got.data(), xb.data(), nullptr, nullptr, &tg) == TKZ_OK && same(xb, tb);
    ok = ok && tkz_encode_batch_spans_device(e, d, b.offs.data(), n, total, allowed, n_allowed, ids.data(), tw, got.data(), nullptr, xu.data(), nullptr, &tg) == TKZ_OK && same(xu, tu);
    if (ok && tw > 0) {
        tg = -2;
        ok = tkz_encode_batch_spans_device(e, d, b.offs.data(), n, total, allowed, n_allowed, ids.data(), tw - 1, got.data(), xb.data(), xu.data(), nullptr, &tg) == TKZ_E_CAPACITY && tg == tw;
    }
    std::fill(xb.begin(), xb.end(), -9); std::fill(xu.begin(), xu.end(), -9);
    ok = ok && tkz_encode_batch_spans_utf8(e, d, b.offs.data(), n, allowed, n_allowed, ids.data(), tw, got.data(), xb.data(), xu.data(), &tg) == TKZ_OK;
    ok = ok && tg == tw && got == want && same(ids, want_ids) && same(xb, tb) && same(xu, tu);
    if (ok && n == 1) {
        int64_t one = -1;
        ok = tkz_encode_spans_utf8(e, d, total, allowed, n_allowed, ids.data(), tw, xb.data(), xu.data(), &one) == TKZ_OK && one == tw && same(ids, want_ids) && same(xb, tb) && same(xu, tu);
    }
    tkz_host_free(aligned);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string file = slurp(argv[1]);
    tkz_vocab* v = nullptr; tkz_encoder* e = nullptr;
    REQUIRE(tkz_vocab_from_tiktoken(reinterpret_cast<const uint8_t*>(file.data()), file.size(), &v) == TKZ_OK);
    REQUIRE(tkz_encoder_create(v, TKZ_PATTERN_CL100K, 0, &e) == TKZ_OK);
    const std::string eot = "<|endoftext|>";
    const int32_t sid[1] = {50256}; const int64_t loffs[2] = {0, (int64_t)eot.size()};
    REQUIRE(tkz_encoder_set_special_tokens(e, sid, reinterpret_cast<const uint8_t*>(eot.data()), loffs, 1) == TKZ_OK);
    const int32_t allow[1] = {0};
    for (int round = 0; round < 2; ++round) {
        {   // the FIRST call of the encoder: crowded lists, the attempt is redone with longer ones
            Batch b; const std::string g = gib(30000, 2, 2);
            b.add(g.substr(0, 700)); b.add(g.substr(700, 20000)); b.add(g.substr(20700));
            REQUIRE(check_batch(e, b, nullptr, 0));
        }
        {   // a token at every byte; pieces of several tokens across a sub-tile edge and a word edge
            std::string text; for (int k = 0; k < 140; ++k) text += "a\nb\nc\nd\n";
            Batch b; b.add(text);
            REQUIRE(check_batch(e, b, nullptr, 0));
            for (size_t edge : {size_t(1024), size_t(64)}) { Batch c; c.add(plain(edge - 6) + " zqxjkvbwpmzqxj " + plain(300)); REQUIRE(check_batch(e, c, nullptr, 0)); }
        }
        {   // document starts on the first and last byte of a sub-tile, two in one sub-tile, runs of empty documents, tiny documents, one byte
            Batch b;
            b.add(""); b.add(""); b.add(plain(100)); b.add(plain(200)); b.add(""); b.add(""); b.add("");
            b.add(plain(1024 - b.offs.back() % 1024)); b.add(plain(2047)); b.add(plain(3 * 1024 + 5)); b.add(plain(7)); b.add(""); b.add("");
            REQUIRE(check_batch(e, b, nullptr, 0));
            Batch empties; for (int k = 0; k < 5; ++k) empties.add("");
            REQUIRE(check_batch(e, empties, nullptr, 0));
            Batch none;
            REQUIRE(check_batch(e, none, nullptr, 0));
            Batch tiny; const char* t[] = {"a", " b", "\n", "c d", "qz", " the", "x\n\n", " zqxj"};
            for (int k = 0; k < 2000; ++k) tiny.add(t[rnd(8)]);
            REQUIRE(check_batch(e, tiny, nullptr, 0));
            Batch one; one.add("x");
            REQUIRE(check_batch(e, one, nullptr, 0));
        }
        {   // long misses of 17 .. 128 and of 129 .. 1,024 bytes, a piece of more than 1,024 bytes that ends its document, multi-byte text
            Batch b; b.add(plain(300) + gib(18, 17, 17) + gib(61, 60, 60) + gib(129, 128, 128) + " tail"); b.add(plain(900) + gib(601, 600, 600) + " x" + gib(1025, 1024, 1024));
            b.add(gib(700, 2, 3) + std::string(1500, 'x')); b.add(plain(300)); b.add(plain(500) + gib(3001, 3000, 3000));
            std::string cjk; for (int k = 0; k < 60; ++k) cjk += "\xE6\xBC\xA2\xE5\xAD\x97 caf\xC3\xA9 \xF0\x9F\x98\x80\xF0\x9F\x91\x8D\xF0\x9F\x8F\xBD ";
            b.add(cjk); b.add("\xF0\x9F\x98\x80");
            REQUIRE(check_batch(e, b, nullptr, 0));
        }
        {   // a literal across a sub-tile edge, at the start and the end of a document and twice in a row, allowed and not
            Batch b; b.add(plain(1018) + eot + plain(1500)); b.add(plain(200) + eot); b.add(eot + plain(40)); b.add(eot + eot); b.add(plain(30) + eot.substr(0, 6)); b.add(eot.substr(6));
            REQUIRE(check_batch(e, b, allow, 1) && check_batch(e, b, nullptr, 0));
            Batch one; one.add(plain(900) + eot + plain(700));
            REQUIRE(check_batch(e, one, allow, 1) && check_batch(e, one, nullptr, 0));
        }
        {   // the UTF-16 entries: a lone surrogate, a pair cut by a document boundary, a literal; the units against the transcoded bytes
            std::vector<uint16_t> u; std::vector<int64_t> uo{0};
            auto add = [&](const std::u16string& s) { u.insert(u.end(), s.begin(), s.end()); uo.push_back((int64_t)u.size()); };
            add(u"plain text"); add(u"lone \xD800 high"); add(u"cut \xD83D"); add(u"\xDE00 here"); add(u""); add(u"a <|endoftext|> b \xD83D\xDE00\x6F22");
            const int64_t n = (int64_t)uo.size() - 1;
            std::vector<int32_t> want_ids(u.size() * 3 + 1), ids(u.size() * 3 + 1);
            std::vector<int64_t> want((size_t)n + 1), got((size_t)n + 1);
            int64_t need = 0, tot = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), uo.data(), n, allow, 1, want_ids.data(), (int64_t)want_ids.size(), want.data(), &need) == TKZ_OK);
            std::vector<int32_t> tu((size_t)need, -9);
            ids.resize((size_t)need); want_ids.resize((size_t)need);
            REQUIRE(tkz_encode_batch_spans_utf16(e, u.data(), uo.data(), n, allow, 1, ids.data(), need, got.data(), tu.data(), &tot) == TKZ_OK && tot == need && got == want && ids == want_ids);
            REQUIRE(tkz_encode_batch_spans_utf16(e, u.data(), uo.data(), n, allow, 1, ids.data(), need - 1, got.data(), tu.data(), &tot) == TKZ_E_CAPACITY && tot == need);
            for (int64_t d = 0; d < n; ++d) {
                REQUIRE(got[d] == got[d + 1] || tu[(size_t)got[d]] == 0);
                for (int64_t t = got[d]; t + 1 < got[d + 1]; ++t) REQUIRE(tu[(size_t)t] <= tu[(size_t)t + 1] && tu[(size_t)t + 1] <= uo[d + 1] - uo[d]);
                int64_t a = -1;
                std::vector<int32_t> one_ids((size_t)need + 1), one_u((size_t)need + 1);
                REQUIRE(tkz_encode_spans_utf16(e, u.data() + uo[d], uo[d + 1] - uo[d], allow, 1, one_ids.data(), need, one_u.data(), &a) == TKZ_OK && a == got[d + 1] - got[d]);
                REQUIRE(std::equal(one_u.begin(), one_u.begin() + a, tu.begin() + got[d]) && std::equal(one_ids.begin(), one_ids.begin() + a, ids.begin() + got[d]));
            }
        }
        {   // the argument rows, an empty text, invalid UTF-8
            const uint8_t t[5] = {'h', 'e', 0xFF, 'l', 'o'}; const int64_t o2[2] = {0, 5}; int64_t oo[2] = {7, 7}, n = 7;
            int32_t ids[8], tb[8], tu[8];
            REQUIRE(tkz_encode_spans_utf8(nullptr, t, 2, nullptr, 0, ids, 8, tb, tu, &n) == TKZ_E_ARG && tkz_encode_spans_utf8(e, t, 2, nullptr, 0, ids, 8, tb, tu, nullptr) == TKZ_E_ARG);
            REQUIRE(tkz_encode_spans_utf8(e, t, -1, nullptr, 0, ids, 8, tb, tu, &n) == TKZ_E_ARG && tkz_encode_spans_utf8(e, t, 2, nullptr, 0, ids, 8, nullptr, nullptr, &n) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_spans_utf8(e, t, o2, 1, nullptr, 0, ids, 8, nullptr, tb, tu, &n) == TKZ_E_ARG && tkz_encode_batch_spans_utf8(e, t, nullptr, 1, nullptr, 0, ids, 8, oo, tb, tu, &n) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_spans_utf16(e, reinterpret_cast<const uint16_t*>(t), o2, 1, nullptr, 0, ids, 8, oo, nullptr, &n) == TKZ_E_ARG);
            const int32_t bad[1] = {1}, twice[2] = {0, 0};
            REQUIRE(tkz_encode_spans_utf8(e, t, 2, bad, 1, ids, 8, tb, tu, &n) == TKZ_E_ARG && tkz_encode_batch_spans_utf8(e, t, o2, 1, twice, 2, ids, 8, oo, tb, tu, &n) == TKZ_E_ARG);
            REQUIRE(tkz_encode_spans_utf8(e, t, 5, nullptr, 0, ids, 8, tb, tu, &n) == TKZ_E_INVALID_UTF8);
            n = 7;
            REQUIRE(tkz_encode_spans_utf8(e, nullptr, 0, nullptr, 0, ids, 8, tb, tu, &n) == TKZ_OK && n == 0);
            n = 7;
            REQUIRE(tkz_encode_spans_utf16(e, nullptr, 0, allow, 1, ids, 8, tu, &n) == TKZ_OK && n == 0);
            const int64_t z[3] = {0, 0, 0}; int64_t zo[3] = {5, 5, 5};
            REQUIRE(tkz_encode_batch_spans_utf8(e, nullptr, z, 2, nullptr, 0, ids, 8, zo, tb, tu, &n) == TKZ_OK && zo[0] == 0 && zo[1] == 0 && zo[2] == 0 && n == 0);
        }
    }
    int64_t calls = 0;
    tkz_encoder_spans_calls(e, &calls);
    REQUIRE(calls > 100);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize spans ok (%lld span calls)\n", (long long)calls);
    return 0;
}
