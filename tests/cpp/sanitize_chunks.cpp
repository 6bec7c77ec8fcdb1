// A stand-alone driver for a sanitizer build of the host code behind the chunk entries (tkz_encode_batch_chunks_device / _utf8 / _utf16, tkz_encode_chunks_utf8 /
// _utf16) and of k_chunk_walk / k_chunk_walk_long / k_chunk_unitcount / k_chunk_units: tests/test_cpp_chunks.py compiles it with the product sources and the CPU
// SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under -fsanitize=address,undefined and runs it; nothing is loaded into an interpreter.  It
// walks the shapes of tests/chunk_cases.py -- budgets of 1, 2, 7, 64 and 200 over a chunk at every byte, pieces over the budget, runs of empty documents, 257
// documents, documents at and over the long-document threshold, a literal at a chunk boundary, multi-byte text across a sub-tile edge, the UTF-16 entries with
// lone surrogates, tables that are exactly full, one too small and without the position arrays, the argument rows and an empty batch -- twice over one encoder.
// Every table is held against the encode entry's ids and offsets and against the rule itself, applied to the pieces tkz_encode_batch_pieces_utf8 returns, with the
// byte starts from the keys tkz_decode_utf8 returns for the ids.  argv: gpt2.tiktoken
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
static std::string words(int n) { std::string s; for (int k = 0; k < n; ++k) { if (k) s += ' '; s += kWords[rnd(20)]; } return s; }      // n items of one token
static std::string gib(size_t n, int lo, int hi) {         // consonant strings no vocabulary holds: every piece is a miss of several tokens
    std::string s;
    while (s.size() < n) { s += ' '; for (int k = lo + (int)rnd(hi - lo + 1); k > 0; --k) s += "bcdfghjklmnpqrstvwxz"[rnd(20)]; }
    s.resize(n);
    return s;
}
static int64_t units_begun(const uint8_t* p, int64_t n) { int64_t u = 0; for (int64_t i = 0; i < n; ++i) u += ((p[i] & 0xC0) != 0x80) + (p[i] >= 0xF0); return u; }

struct Batch { std::vector<uint8_t> bytes; std::vector<int64_t> offs{0}; void add(const std::string& d) { bytes.insert(bytes.end(), d.begin(), d.end()); offs.push_back((int64_t)bytes.size()); } };
struct Table { std::vector<int64_t> dco, ct, cb, cu; };

// the rule of tkz.h over the token offsets of the items of every document (piece entry: plain text only), byte starts from the keys of the ids
static bool expected(tkz_encoder* e, const uint8_t* text, const Batch& b, int64_t mx, const std::vector<int32_t>& ids, const std::vector<int64_t>& ooff, Table* T) {
    const int64_t n = (int64_t)b.offs.size() - 1, total = b.offs.back();
    std::vector<int32_t> pids((size_t)total + 1);
    std::vector<int64_t> dpo((size_t)n + 1), pbo((size_t)total + 2), pto((size_t)total + 2);
    int64_t np = 0, need = 0;
    if (total == 0) { T->dco.assign((size_t)n + 1, 0); T->ct.assign(1, 0); T->cb.clear(); T->cu.clear(); return true; }
    if (tkz_encode_batch_pieces_utf8(e, text, b.offs.data(), n, pids.data(), total, dpo.data(), pbo.data(), pto.data(), total + 1, &np, &need) != TKZ_OK) return false;
    // the byte start of every token of the batch
    std::vector<int64_t> tpos((size_t)need + 1);
    uint8_t key[256];
    for (int64_t d = 0; d < n; ++d) {
        int64_t pos = b.offs[d];
        for (int64_t t = ooff[d]; t < ooff[d + 1]; ++t) {
            int64_t len = 0;
            tpos[(size_t)t] = pos;
            if (tkz_decode_utf8(e, &ids[(size_t)t], 1, key, sizeof key, &len) != TKZ_OK) return false;
            pos += len;
        }
        if (pos != b.offs[d + 1]) return false;
    }
    T->dco.assign(1, 0); T->ct.clear(); T->cb.clear(); T->cu.clear();
    for (int64_t d = 0; d < n; ++d) {
        const int64_t end = pto[(size_t)dpo[d + 1]];
        int64_t s = pto[(size_t)dpo[d]];
        while (s < end) {
            T->ct.push_back(s); T->cb.push_back(tpos[(size_t)s] - b.offs[d]); T->cu.push_back(units_begun(text + b.offs[d], tpos[(size_t)s] - b.offs[d]));
            if (end - s <= mx) break;
            int64_t best = s;                                 // the largest item boundary in (s, s + mx]
            for (int64_t p = dpo[d]; p <= dpo[d + 1] && pto[(size_t)p] <= s + mx; ++p) if (pto[(size_t)p] > s) best = pto[(size_t)p];
            s = best > s ? best : s + mx;
        }
        T->dco.push_back((int64_t)T->ct.size());
    }
    T->ct.push_back(need);
    return true;
}

// the device entry (the emulated build's device memory is host memory) with tables of EXACTLY the chunk count -- a store one past the end is the sanitizer's to
// find --, without either position array, one entry short; the host entry; for a batch of one document the single entry.  plain text (no literal allowed)
static bool check_batch(tkz_encoder* e, const Batch& b, int64_t mx) {
    const int64_t n = (int64_t)b.offs.size() - 1, total = b.offs.back();
    void* aligned = nullptr;                                                     // (d_bytes: 16-byte aligned)
    if (tkz_host_alloc((size_t)total + 64, &aligned) != TKZ_OK) return false;
    std::memset(aligned, 0, (size_t)total + 64);
    if (total) std::memcpy(aligned, b.bytes.data(), (size_t)total);
    const uint8_t* d = static_cast<const uint8_t*>(aligned);
    std::vector<int32_t> want_ids((size_t)total + 1);
    std::vector<int64_t> want((size_t)n + 1, -1), got((size_t)n + 1, -2);
    int64_t tw = -1, tg = -2, cg = -2;
    bool ok = tkz_encode_batch_device(e, d, b.offs.data(), n, total, want_ids.data(), total, want.data(), nullptr, &tw) == TKZ_OK;
    Table T;
    ok = ok && expected(e, d, b, mx, want_ids, want, &T);
    if (!ok) { tkz_host_free(aligned); return false; }
    const int64_t nc = (int64_t)T.cb.size();
    const size_t room = tw > 0 ? (size_t)tw : 1, croom = nc > 0 ? (size_t)nc : 1;
    std::vector<int32_t> ids(room, -9);
    std::vector<int64_t> dco((size_t)n + 1, -3), ct((size_t)nc + 1, -3), cb(croom, -3), cu(croom, -3);
    auto same = [](const std::vector<int64_t>& x, const std::vector<int64_t>& y, int64_t k) { return std::equal(y.begin(), y.begin() + k, x.begin()); };
    auto same_ids = [&]() { return std::equal(ids.begin(), ids.begin() + tw, want_ids.begin()); };
    ok = tkz_encode_batch_chunks_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ids.data(), tw, got.data(), dco.data(), ct.data(), cb.data(), cu.data(), nc, nullptr, &tg, &cg) == TKZ_OK;
    ok = ok && tg == tw && cg == nc && got == want && same_ids() && dco == T.dco && ct == T.ct && same(cb, T.cb, nc) && same(cu, T.cu, nc);
    std::fill(ct.begin(), ct.end(), -3);
    ok = ok && tkz_encode_batch_chunks_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ids.data(), tw, got.data(), dco.data(), ct.data(), nullptr, nullptr, nc, nullptr, &tg, &cg) == TKZ_OK && ct == T.ct;
    std::fill(cu.begin(), cu.end(), -3);
    ok = ok && tkz_encode_batch_chunks_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ids.data(), tw, got.data(), dco.data(), ct.data(), nullptr, cu.data(), nc, nullptr, &tg, &cg) == TKZ_OK && same(cu, T.cu, nc);
    if (ok && nc > 0) {
        tg = cg = -2;
        ok = tkz_encode_batch_chunks_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ids.data(), tw, got.data(), dco.data(), ct.data(), cb.data(), cu.data(), nc - 1, nullptr, &tg, &cg) == TKZ_E_CAPACITY && tg == tw && cg == nc;
        ok = ok && tkz_encode_batch_chunks_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ids.data(), tw - 1, got.data(), dco.data(), ct.data(), cb.data(), cu.data(), nc, nullptr, &tg, &cg) == TKZ_E_CAPACITY && tg == tw && cg == nc;
    }
    std::fill(cb.begin(), cb.end(), -3); std::fill(cu.begin(), cu.end(), -3); std::fill(ct.begin(), ct.end(), -3);
    ok = ok && tkz_encode_batch_chunks_utf8(e, d, b.offs.data(), n, nullptr, 0, mx, ids.data(), tw, got.data(), dco.data(), ct.data(), cb.data(), cu.data(), nc, &tg, &cg) == TKZ_OK;
    ok = ok && tg == tw && cg == nc && got == want && same_ids() && dco == T.dco && ct == T.ct && same(cb, T.cb, nc) && same(cu, T.cu, nc);
    if (ok && n == 1) {
        int64_t one = -1, oc = -1;
        std::fill(ct.begin(), ct.end(), -3);
        ok = tkz_encode_chunks_utf8(e, d, total, nullptr, 0, mx, ids.data(), tw, ct.data(), cb.data(), cu.data(), nc, &one, &oc) == TKZ_OK && one == tw && oc == nc && ct == T.ct && same(cb, T.cb, nc);
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
        {   // a chunk at every byte (starts at 1023, 1024, 1025 of the batch); pieces over the budget at the start, in the middle and at the end of a document
            std::string text; for (int k = 0; k < 140; ++k) text += "a\nb\nc\nd\n";
            Batch b; b.add("xy"); b.add(text);
            for (int64_t mx : {1, 2, 7}) REQUIRE(check_batch(e, b, mx));
            Batch g; g.add(gib(400, 5, 14)); g.add(words(5) + gib(40, 9, 9) + " " + words(9)); g.add(words(9) + gib(60, 20, 20)); g.add(""); g.add(gib(20, 19, 19));
            for (int64_t mx : {1, 2, 3, 4, 7}) REQUIRE(check_batch(e, g, mx));
        }
        {   // documents of 0, max and max + 1 tokens, runs of empty documents, no documents, one byte; 255, 256 and 257 documents
            for (int64_t mx : {1, 4}) {
                Batch b; b.add(""); b.add(""); b.add(words((int)mx)); b.add(words((int)mx + 1)); b.add(""); b.add(words(3 * (int)mx)); b.add("x"); b.add(""); b.add("");
                REQUIRE(check_batch(e, b, mx));
            }
            Batch empties; for (int k = 0; k < 5; ++k) empties.add("");
            Batch none;
            REQUIRE(check_batch(e, empties, 3) && check_batch(e, none, 3));
            for (int n : {255, 256, 257}) { Batch b; for (int k = 0; k < n; ++k) b.add(words((int)rnd(10))); REQUIRE(check_batch(e, b, 4)); }
        }
        {   // the long-document form: at, over and far over 1,024 items, a piece over the budget inside; chunks of 63, 64, 65 and 200 items
            Batch b; b.add(words(1024)); b.add(words(1025)); b.add(words(40)); b.add(words(700) + gib(30, 29, 29) + " " + words(700)); b.add(words(2118));
            for (int64_t mx : {4, 63, 64, 65, 200}) REQUIRE(check_batch(e, b, mx));
            Batch one; one.add(words(1500));
            REQUIRE(check_batch(e, one, 64) && check_batch(e, one, 1) && check_batch(e, one, 1 << 20));
        }
        {   // multi-byte text: a 4-byte character across the sub-tile edge in front of a chunk start, CJK
            std::string t; for (int k = 0; k < 511; ++k) t += "a\n";
            t += "\xF0\x9F\x98\x80"; for (int k = 0; k < 8; ++k) t += "a\nb\n";
            std::string cjk; for (int k = 0; k < 60; ++k) cjk += "\xE6\xBC\xA2\xE5\xAD\x97 caf\xC3\xA9 \xF0\x9F\x98\x80\xF0\x9F\x91\x8D\xF0\x9F\x8F\xBD ";
            Batch b; b.add(t); b.add(cjk); b.add("\xF0\x9F\x98\x80");
            for (int64_t mx : {1, 3}) REQUIRE(check_batch(e, b, mx));
        }
        {   // a literal at a chunk boundary, allowed and not: against the special entry's ids, one item of one token
            const std::string text = words(3) + eot + words(9) + eot + eot;
            const int64_t offs[2] = {0, (int64_t)text.size()};
            const uint8_t* t = reinterpret_cast<const uint8_t*>(text.data());
            std::vector<int32_t> want((size_t)text.size()), ids((size_t)text.size());
            int64_t wo[2], go[2], dco[2], need = 0, tot = 0, nc = 0;
            REQUIRE(tkz_encode_batch_special_utf8(e, t, offs, 1, allow, 1, want.data(), (int64_t)want.size(), wo, &need) == TKZ_OK);
            std::vector<int64_t> ct((size_t)need + 1), cb((size_t)need), cu((size_t)need);
            REQUIRE(tkz_encode_batch_chunks_utf8(e, t, offs, 1, allow, 1, 1, ids.data(), need, go, dco, ct.data(), cb.data(), cu.data(), need, &tot, &nc) == TKZ_OK);
            REQUIRE(tot == need && nc == need && go[1] == wo[1] && std::equal(ids.begin(), ids.begin() + need, want.begin()));      // every token a chunk
            for (int64_t c = 0; c < nc; ++c) REQUIRE(ct[(size_t)c] == c && (ids[(size_t)c] != 50256 || c + 1 == nc || cb[(size_t)c + 1] - cb[(size_t)c] == (int64_t)eot.size()));
            REQUIRE(tkz_encode_batch_chunks_utf8(e, t, offs, 1, allow, 1, 4, ids.data(), need, go, dco, ct.data(), cb.data(), cu.data(), need, &tot, &nc) == TKZ_OK);
            REQUIRE(nc == 4 && ct[1] == 4 && ids[3] == 50256 && cb[1] == (int64_t)(text.find(eot) + eot.size()));
        }
        {   // the UTF-16 entries: a lone surrogate, a pair cut by a document boundary, a literal; exact tables
            std::vector<uint16_t> u; std::vector<int64_t> uo{0};
            auto add = [&](const std::u16string& s) { u.insert(u.end(), s.begin(), s.end()); uo.push_back((int64_t)u.size()); };
            add(u"plain text"); add(u"lone \xD800 high zqxjkvb"); add(u"cut \xD83D"); add(u"\xDE00 here"); add(u""); add(u"a <|endoftext|> b \xD83D\xDE00\x6F22");
            const int64_t n = (int64_t)uo.size() - 1;
            std::vector<int32_t> want_ids(u.size() * 3 + 1), ids(u.size() * 3 + 1);
            std::vector<int64_t> want((size_t)n + 1), got((size_t)n + 1), dco((size_t)n + 1);
            int64_t need = 0, tot = 0, nc = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), uo.data(), n, allow, 1, want_ids.data(), (int64_t)want_ids.size(), want.data(), &need) == TKZ_OK);
            ids.resize((size_t)need); want_ids.resize((size_t)need);
            REQUIRE(tkz_encode_batch_chunks_utf16(e, u.data(), uo.data(), n, allow, 1, 2, ids.data(), need, got.data(), dco.data(), got.data(), nullptr, 0, &tot, &nc) == TKZ_E_CAPACITY && tot == need && nc > n);
            std::vector<int64_t> ct((size_t)nc + 1, -3), cu((size_t)nc, -3);
            const int64_t exact = nc;
            REQUIRE(tkz_encode_batch_chunks_utf16(e, u.data(), uo.data(), n, allow, 1, 2, ids.data(), need, got.data(), dco.data(), ct.data(), cu.data(), exact, &tot, &nc) == TKZ_OK);
            REQUIRE(tot == need && nc == exact && got == want && ids == want_ids && ct[(size_t)nc] == need && dco[(size_t)n] == nc);
            for (int64_t d = 0; d < n; ++d) {
                REQUIRE(dco[d] == dco[d + 1] || (cu[(size_t)dco[d]] == 0 && ct[(size_t)dco[d]] == got[d]));
                for (int64_t c = dco[d]; c + 1 < dco[d + 1]; ++c) REQUIRE(cu[(size_t)c] <= cu[(size_t)c + 1] && cu[(size_t)c + 1] <= uo[d + 1] - uo[d] && ct[(size_t)c + 1] - ct[(size_t)c] <= 2 && ct[(size_t)c + 1] > ct[(size_t)c]);
                int64_t a = -1, oc = -1;
                const int64_t k = dco[d + 1] - dco[d];
                std::vector<int32_t> one_ids((size_t)need + 1);
                std::vector<int64_t> one_ct((size_t)k + 1), one_u((size_t)k + 1);
                REQUIRE(tkz_encode_chunks_utf16(e, u.data() + uo[d], uo[d + 1] - uo[d], allow, 1, 2, one_ids.data(), need, one_ct.data(), one_u.data(), k, &a, &oc) == TKZ_OK && a == got[d + 1] - got[d] && oc == k);
                REQUIRE(std::equal(one_u.begin(), one_u.begin() + k, cu.begin() + dco[d]) && std::equal(one_ids.begin(), one_ids.begin() + a, ids.begin() + got[d]));
            }
        }
        {   // the argument rows, an empty text, invalid UTF-8
            const uint8_t t[5] = {'h', 'e', 0xFF, 'l', 'o'}; const int64_t o2[2] = {0, 5}; int64_t oo[2] = {7, 7}, dc[2] = {7, 7}, n = 7, c = 7;
            int32_t ids[8]; int64_t ct[9], cb[8], cu[8];
            REQUIRE(tkz_encode_chunks_utf8(nullptr, t, 2, nullptr, 0, 3, ids, 8, ct, cb, cu, 8, &n, &c) == TKZ_E_ARG && tkz_encode_chunks_utf8(e, t, 2, nullptr, 0, 3, ids, 8, ct, cb, cu, 8, nullptr, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_chunks_utf8(e, t, 2, nullptr, 0, 3, ids, 8, ct, cb, cu, 8, &n, nullptr) == TKZ_E_ARG && tkz_encode_chunks_utf8(e, t, -1, nullptr, 0, 3, ids, 8, ct, cb, cu, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_chunks_utf8(e, t, 2, nullptr, 0, 0, ids, 8, ct, cb, cu, 8, &n, &c) == TKZ_E_ARG && tkz_encode_chunks_utf8(e, t, 2, nullptr, 0, -5, ids, 8, ct, cb, cu, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_chunks_utf8(e, t, 2, nullptr, 0, 3, ids, 8, nullptr, cb, cu, 8, &n, &c) == TKZ_E_ARG && tkz_encode_chunks_utf8(e, t, 2, nullptr, 0, 3, ids, 8, ct, cb, cu, -1, &n, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_chunks_utf8(e, t, o2, 1, nullptr, 0, 3, ids, 8, nullptr, dc, ct, cb, cu, 8, &n, &c) == TKZ_E_ARG && tkz_encode_batch_chunks_utf8(e, t, o2, 1, nullptr, 0, 3, ids, 8, oo, nullptr, ct, cb, cu, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_chunks_utf16(e, reinterpret_cast<const uint16_t*>(t), o2, 1, nullptr, 0, 0, ids, 8, oo, dc, ct, cu, 8, &n, &c) == TKZ_E_ARG);
            const int32_t bad[1] = {1}, twice[2] = {0, 0};
            REQUIRE(tkz_encode_chunks_utf8(e, t, 2, bad, 1, 3, ids, 8, ct, cb, cu, 8, &n, &c) == TKZ_E_ARG && tkz_encode_batch_chunks_utf8(e, t, o2, 1, twice, 2, 3, ids, 8, oo, dc, ct, cb, cu, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_chunks_utf8(e, t, 5, nullptr, 0, 3, ids, 8, ct, cb, cu, 8, &n, &c) == TKZ_E_INVALID_UTF8);
            n = c = 7; ct[0] = 7;
            REQUIRE(tkz_encode_chunks_utf8(e, nullptr, 0, nullptr, 0, 3, ids, 8, ct, cb, cu, 8, &n, &c) == TKZ_OK && n == 0 && c == 0 && ct[0] == 0);
            n = c = 7; ct[0] = 7;
            REQUIRE(tkz_encode_chunks_utf16(e, nullptr, 0, allow, 1, 3, ids, 8, ct, cu, 8, &n, &c) == TKZ_OK && n == 0 && c == 0 && ct[0] == 0);
            const int64_t z[3] = {0, 0, 0}; int64_t zo[3] = {5, 5, 5}, zc[3] = {5, 5, 5};
            REQUIRE(tkz_encode_batch_chunks_utf8(e, nullptr, z, 2, nullptr, 0, 3, ids, 8, zo, zc, ct, cb, cu, 0, &n, &c) == TKZ_OK && zo[2] == 0 && zc[0] == 0 && zc[1] == 0 && zc[2] == 0 && n == 0 && c == 0);
        }
    }
    int64_t calls = 0;
    tkz_encoder_chunks_calls(e, &calls);
    REQUIRE(calls > 100);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize chunks ok (%lld chunk calls)\n", (long long)calls);
    return 0;
}
