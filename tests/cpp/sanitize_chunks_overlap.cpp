// A stand-alone driver for a sanitizer build of the host code behind the overlap chunk entries (tkz_encode_batch_chunks_overlap_device / _utf8 / _utf16,
// tkz_encode_chunks_overlap_utf8 / _utf16) and of k_chunkov_walk / k_chunkov_walk_long / k_chunkov_units: tests/test_cpp_chunks_overlap.py compiles it with the
// product sources and the CPU SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under -fsanitize=address,undefined and runs it; nothing is
// loaded into an interpreter.  It walks the shapes of tests/chunk_overlap_cases.py -- an end at every byte, a batch whose last end is its last byte at a multiple
// of 1,024, pieces over the budget, empty documents, 257 documents, documents at and over the long-document threshold with overlaps under and over a window of 64
// items, multi-byte text across a sub-tile edge, the UTF-16 entries with lone surrogates, tables that are exactly full, one too small and without the position
// arrays, the argument rows and an empty batch -- twice over one encoder.  Every table is held against the encode entry's ids and offsets and against the rule
// itself, applied to the pieces tkz_encode_batch_pieces_utf8 returns, with the byte positions from the keys tkz_decode_utf8 returns for the ids.
// argv: gpt2.tiktoken
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
struct Table { std::vector<int64_t> dco, ct, ce, pos[4]; };      // pos: chunk_bytes, chunk_units, chunk_end_bytes, chunk_end_units

// the rule of tkz.h over the token offsets of the items of every document (piece entry: plain text only), byte positions from the keys of the ids
static bool expected(tkz_encoder* e, const uint8_t* text, const Batch& b, int64_t mx, int64_t ov, const std::vector<int32_t>& ids, const std::vector<int64_t>& ooff, Table* T) {
    const int64_t n = (int64_t)b.offs.size() - 1, total = b.offs.back();
    std::vector<int32_t> pids((size_t)total + 1);
    std::vector<int64_t> dpo((size_t)n + 1), pbo((size_t)total + 2), pto((size_t)total + 2);
    int64_t np = 0, need = 0;
    T->dco.assign(1, 0); T->ct.clear(); T->ce.clear();
    for (auto& p : T->pos) p.clear();
    if (total == 0) { T->dco.assign((size_t)n + 1, 0); return true; }
    if (tkz_encode_batch_pieces_utf8(e, text, b.offs.data(), n, pids.data(), total, dpo.data(), pbo.data(), pto.data(), total + 1, &np, &need) != TKZ_OK) return false;
    std::vector<int64_t> tpos((size_t)need + 1);               // the byte start of every token of the batch
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
    for (int64_t d = 0; d < n; ++d) {
        const int64_t p0 = dpo[d], p1 = dpo[d + 1], end = pto[(size_t)p1];
        auto end_of = [&](int64_t s) {
            if (end - s <= mx) return end;
            int64_t best = s;                                     // the largest item boundary in (s, s + mx]
            for (int64_t p = p0; p <= p1 && pto[(size_t)p] <= s + mx; ++p) if (pto[(size_t)p] > s) best = pto[(size_t)p];
            return best > s ? best : s + mx;
        };
        int64_t s = pto[(size_t)p0];
        while (s < end) {
            const int64_t z = end_of(s), zpos = z < end ? tpos[(size_t)z] : b.offs[d + 1];
            T->ct.push_back(s); T->ce.push_back(z);
            T->pos[0].push_back(tpos[(size_t)s] - b.offs[d]); T->pos[1].push_back(units_begun(text + b.offs[d], tpos[(size_t)s] - b.offs[d]));
            T->pos[2].push_back(zpos - b.offs[d]); T->pos[3].push_back(units_begun(text + b.offs[d], zpos - b.offs[d]));
            if (z == end) break;
            const int64_t x = std::max(z - ov, s + 1);
            int64_t nx = x;                                       // the smallest item boundary in [x, z], else x
            for (int64_t p = p0; p <= p1; ++p) if (pto[(size_t)p] >= x) { if (pto[(size_t)p] <= z) nx = pto[(size_t)p]; break; }
            s = end_of(nx) == z ? z : nx;
        }
        T->dco.push_back((int64_t)T->ct.size());
    }
    return true;
}

// the device entry (the emulated build's device memory is host memory) with tables of EXACTLY the chunk count -- a store one past the end is the sanitizer's to
// find --, with every position array, with none, with the end units alone, one entry short; the host entry; for one document the single entry.  plain text
static bool check_batch(tkz_encoder* e, const Batch& b, int64_t mx, int64_t ov) {
    const int64_t n = (int64_t)b.offs.size() - 1, total = b.offs.back();
    void* aligned = nullptr;                                                     // (d_bytes: 16-byte aligned; NO slack behind the text: an end may be `total`)
    if (tkz_host_alloc((size_t)std::max<int64_t>(total, 16), &aligned) != TKZ_OK) return false;
    if (total) std::memcpy(aligned, b.bytes.data(), (size_t)total);
    const uint8_t* d = static_cast<const uint8_t*>(aligned);
    std::vector<int32_t> want_ids((size_t)total + 1);
    std::vector<int64_t> want((size_t)n + 1, -1), got((size_t)n + 1, -2);
    int64_t tw = -1, tg = -2, cg = -2;
    bool ok = tkz_encode_batch_device(e, d, b.offs.data(), n, total, want_ids.data(), total, want.data(), nullptr, &tw) == TKZ_OK;
    Table T;
    ok = ok && expected(e, d, b, mx, ov, want_ids, want, &T);
    if (!ok) { tkz_host_free(aligned); return false; }
    const int64_t nc = (int64_t)T.ct.size();
    const size_t room = tw > 0 ? (size_t)tw : 1, croom = nc > 0 ? (size_t)nc : 1;
    std::vector<int32_t> ids(room, -9);
    std::vector<int64_t> dco((size_t)n + 1, -3), ct(croom, -3), ce(croom, -3), pos[4];
    for (auto& p : pos) p.assign(croom, -3);
    auto same = [](const std::vector<int64_t>& x, const std::vector<int64_t>& y, int64_t k) { return std::equal(y.begin(), y.begin() + k, x.begin()); };
    auto table = [&](bool all) {
        bool s = tg == tw && cg == nc && got == want && std::equal(ids.begin(), ids.begin() + tw, want_ids.begin()) && dco == T.dco && same(ct, T.ct, nc) && same(ce, T.ce, nc);
        for (int k = 0; all && k < 4; ++k) s = s && same(pos[k], T.pos[k], nc);
        return s;
    };
    ok = tkz_encode_batch_chunks_overlap_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ov, ids.data(), tw, got.data(), dco.data(), ct.data(), ce.data(), pos[0].data(),
                                                pos[1].data(), pos[2].data(), pos[3].data(), nc, nullptr, &tg, &cg) == TKZ_OK && table(true);
    std::fill(ct.begin(), ct.end(), -3); std::fill(ce.begin(), ce.end(), -3);
    ok = ok && tkz_encode_batch_chunks_overlap_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ov, ids.data(), tw, got.data(), dco.data(), ct.data(), ce.data(), nullptr,
                                                      nullptr, nullptr, nullptr, nc, nullptr, &tg, &cg) == TKZ_OK && table(false);
    std::fill(pos[3].begin(), pos[3].end(), -3);
    ok = ok && tkz_encode_batch_chunks_overlap_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ov, ids.data(), tw, got.data(), dco.data(), ct.data(), ce.data(), nullptr,
                                                      nullptr, nullptr, pos[3].data(), nc, nullptr, &tg, &cg) == TKZ_OK && table(true);
    if (ok && nc > 0) {
        tg = cg = -2;
        ok = tkz_encode_batch_chunks_overlap_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ov, ids.data(), tw, got.data(), dco.data(), ct.data(), ce.data(), pos[0].data(),
                                                    pos[1].data(), pos[2].data(), pos[3].data(), nc - 1, nullptr, &tg, &cg) == TKZ_E_CAPACITY && tg == tw && cg == nc;
        ok = ok && tkz_encode_batch_chunks_overlap_device(e, d, b.offs.data(), n, total, nullptr, 0, mx, ov, ids.data(), tw - 1, got.data(), dco.data(), ct.data(), ce.data(),
                                                          pos[0].data(), pos[1].data(), pos[2].data(), pos[3].data(), nc, nullptr, &tg, &cg) == TKZ_E_CAPACITY && tg == tw && cg == nc;
    }
    std::fill(ct.begin(), ct.end(), -3); std::fill(ce.begin(), ce.end(), -3);
    for (auto& p : pos) std::fill(p.begin(), p.end(), -3);
    ok = ok && tkz_encode_batch_chunks_overlap_utf8(e, d, b.offs.data(), n, nullptr, 0, mx, ov, ids.data(), tw, got.data(), dco.data(), ct.data(), ce.data(), pos[0].data(),
                                                    pos[1].data(), pos[2].data(), pos[3].data(), nc, &tg, &cg) == TKZ_OK && table(true);
    if (ok && n == 1) {
        int64_t one = -1, oc = -1;
        std::fill(ct.begin(), ct.end(), -3); std::fill(ce.begin(), ce.end(), -3);
        ok = tkz_encode_chunks_overlap_utf8(e, d, total, nullptr, 0, mx, ov, ids.data(), tw, ct.data(), ce.data(), pos[0].data(), pos[1].data(), pos[2].data(), pos[3].data(), nc,
                                            &one, &oc) == TKZ_OK && one == tw && oc == nc && same(ct, T.ct, nc) && same(ce, T.ce, nc) && same(pos[2], T.pos[2], nc);
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
    const int64_t small[][2] = {{1, 0}, {2, 1}, {3, 1}, {4, 3}, {7, 3}, {7, 6}};
    for (int round = 0; round < 2; ++round) {
        {   // an end at every byte (1023, 1024, 1025 of the batch), the last end at byte 2,048 of a batch of 2,048; pieces over the budget
            std::string text; for (int k = 0; k < 300; ++k) text += "a\nb\nc\nd\n";
            Batch b; b.add("xy"); b.add(text.substr(0, 2046));
            Batch c; c.add(text.substr(0, 384)); c.add("");
            for (const auto& s : small) REQUIRE(check_batch(e, b, s[0], s[1]) && check_batch(e, c, s[0], s[1]));
            Batch g; g.add(gib(400, 5, 14)); g.add(words(5) + gib(40, 9, 9) + " " + words(9)); g.add(words(9) + gib(60, 20, 20)); g.add(""); g.add(gib(20, 19, 19));
            for (const auto& s : small) REQUIRE(check_batch(e, g, s[0], s[1]));
        }
        {   // documents of 0, max and max + 1 tokens, runs of empty documents, no documents, one byte; 255, 256 and 257 documents
            for (const auto& s : small) {
                const int mx = (int)s[0];
                Batch b; b.add(""); b.add(""); b.add(words(mx)); b.add(words(mx + 1)); b.add(""); b.add(words(3 * mx)); b.add("x"); b.add(""); b.add("");
                REQUIRE(check_batch(e, b, s[0], s[1]));
            }
            Batch empties; for (int k = 0; k < 5; ++k) empties.add("");
            Batch none;
            REQUIRE(check_batch(e, empties, 3, 1) && check_batch(e, none, 3, 1));
            for (int n : {255, 256, 257}) { Batch b; for (int k = 0; k < n; ++k) b.add(words((int)rnd(10))); REQUIRE(check_batch(e, b, 4, 2)); }
        }
        {   // the long-document form: at, over and far over 1,024 items, a piece over the budget inside; overlaps of 1, 63, 64 and max - 1 items
            Batch b; b.add(words(1024)); b.add(words(1025)); b.add(words(40)); b.add(words(700) + gib(30, 29, 29) + " " + words(700)); b.add(words(2118));
            const int64_t wide[][2] = {{4, 1}, {50, 7}, {50, 49}, {64, 63}, {65, 64}, {200, 1}, {200, 64}, {200, 199}};
            for (const auto& s : wide) REQUIRE(check_batch(e, b, s[0], s[1]));
            Batch one; one.add(words(1500));
            REQUIRE(check_batch(e, one, 64, 8) && check_batch(e, one, 2, 1) && check_batch(e, one, 1 << 20, 1 << 19));
        }
        {   // multi-byte text: a 4-byte character across the sub-tile edge in front of an end, CJK
            std::string t; for (int k = 0; k < 511; ++k) t += "a\n";
            t += "\xF0\x9F\x98\x80"; for (int k = 0; k < 8; ++k) t += "a\nb\n";
            std::string cjk; for (int k = 0; k < 60; ++k) cjk += "\xE6\xBC\xA2\xE5\xAD\x97 caf\xC3\xA9 \xF0\x9F\x98\x80\xF0\x9F\x91\x8D\xF0\x9F\x8F\xBD ";
            Batch b; b.add(t); b.add(cjk); b.add("\xF0\x9F\x98\x80");
            for (const auto& s : small) REQUIRE(check_batch(e, b, s[0], s[1]));
        }
        {   // the UTF-16 entries: a lone surrogate, a pair cut by a document boundary, a literal; exact tables; the last chunk of a document ends at its length
            std::vector<uint16_t> u; std::vector<int64_t> uo{0};
            auto add = [&](const std::u16string& s) { u.insert(u.end(), s.begin(), s.end()); uo.push_back((int64_t)u.size()); };
            add(u"plain text"); add(u"lone \xD800 high zqxjkvb"); add(u"cut \xD83D"); add(u"\xDE00 here"); add(u""); add(u"a <|endoftext|> b \xD83D\xDE00\x6F22");
            const int64_t n = (int64_t)uo.size() - 1;
            std::vector<int32_t> want_ids(u.size() * 3 + 1), ids(u.size() * 3 + 1);
            std::vector<int64_t> want((size_t)n + 1), got((size_t)n + 1), dco((size_t)n + 1);
            int64_t need = 0, tot = 0, nc = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), uo.data(), n, allow, 1, want_ids.data(), (int64_t)want_ids.size(), want.data(), &need) == TKZ_OK);
            ids.resize((size_t)need); want_ids.resize((size_t)need);
            REQUIRE(tkz_encode_batch_chunks_overlap_utf16(e, u.data(), uo.data(), n, allow, 1, 3, 1, ids.data(), need, got.data(), dco.data(), got.data(), got.data(), nullptr, nullptr,
                                                          0, &tot, &nc) == TKZ_E_CAPACITY && tot == need && nc > n);
            std::vector<int64_t> ct((size_t)nc, -3), ce((size_t)nc, -3), cu((size_t)nc, -3), ceu((size_t)nc, -3);
            const int64_t exact = nc;
            REQUIRE(tkz_encode_batch_chunks_overlap_utf16(e, u.data(), uo.data(), n, allow, 1, 3, 1, ids.data(), need, got.data(), dco.data(), ct.data(), ce.data(), cu.data(),
                                                          ceu.data(), exact, &tot, &nc) == TKZ_OK);
            REQUIRE(tot == need && nc == exact && got == want && ids == want_ids && dco[(size_t)n] == nc);
            for (int64_t d = 0; d < n; ++d) {
                const int64_t c0 = dco[d], c1 = dco[d + 1], k = c1 - c0;
                REQUIRE(k == 0 || (cu[(size_t)c0] == 0 && ct[(size_t)c0] == got[d] && ce[(size_t)c1 - 1] == got[d + 1] && ceu[(size_t)c1 - 1] == uo[d + 1] - uo[d]));
                for (int64_t c = c0; c < c1; ++c) REQUIRE(ce[(size_t)c] - ct[(size_t)c] >= 1 && ce[(size_t)c] - ct[(size_t)c] <= 3 && cu[(size_t)c] <= ceu[(size_t)c]);
                for (int64_t c = c0; c + 1 < c1; ++c)
                    REQUIRE(ct[(size_t)c] < ct[(size_t)c + 1] && ct[(size_t)c + 1] <= ce[(size_t)c] && ce[(size_t)c] - ct[(size_t)c + 1] <= 1 && ce[(size_t)c] < ce[(size_t)c + 1] &&
                            cu[(size_t)c + 1] <= ceu[(size_t)c]);
                int64_t a = -1, oc = -1;
                std::vector<int32_t> one_ids((size_t)need + 1);
                std::vector<int64_t> one_ct((size_t)k + 1), one_ce((size_t)k + 1), one_u((size_t)k + 1), one_eu((size_t)k + 1);
                REQUIRE(tkz_encode_chunks_overlap_utf16(e, u.data() + uo[d], uo[d + 1] - uo[d], allow, 1, 3, 1, one_ids.data(), need, one_ct.data(), one_ce.data(), one_u.data(),
                                                        one_eu.data(), k, &a, &oc) == TKZ_OK && a == got[d + 1] - got[d] && oc == k);
                REQUIRE(std::equal(one_u.begin(), one_u.begin() + k, cu.begin() + c0) && std::equal(one_eu.begin(), one_eu.begin() + k, ceu.begin() + c0) &&
                        std::equal(one_ids.begin(), one_ids.begin() + a, ids.begin() + got[d]));
            }
        }
        {   // the argument rows, an empty text, invalid UTF-8
            const uint8_t t[5] = {'h', 'e', 0xFF, 'l', 'o'}; const int64_t o2[2] = {0, 5}; int64_t oo[2] = {7, 7}, dc[2] = {7, 7}, n = 7, c = 7;
            int32_t ids[8]; int64_t ct[8], ce[8], cb[8], cu[8], eb[8], eu[8];
            auto one = [&](tkz_encoder* enc, int64_t len, int64_t mx, int64_t ov, int64_t* pct, int64_t* pce, int64_t cap, int64_t* pn, int64_t* pc) {
                return tkz_encode_chunks_overlap_utf8(enc, t, len, nullptr, 0, mx, ov, ids, 8, pct, pce, cb, cu, eb, eu, cap, pn, pc);
            };
            REQUIRE(one(nullptr, 2, 3, 1, ct, ce, 8, &n, &c) == TKZ_E_ARG && one(e, 2, 3, 1, ct, ce, 8, nullptr, &c) == TKZ_E_ARG && one(e, 2, 3, 1, ct, ce, 8, &n, nullptr) == TKZ_E_ARG);
            REQUIRE(one(e, -1, 3, 1, ct, ce, 8, &n, &c) == TKZ_E_ARG && one(e, 2, 0, 0, ct, ce, 8, &n, &c) == TKZ_E_ARG && one(e, 2, -5, 0, ct, ce, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(one(e, 2, 3, -1, ct, ce, 8, &n, &c) == TKZ_E_ARG && one(e, 2, 3, 3, ct, ce, 8, &n, &c) == TKZ_E_ARG && one(e, 2, 3, 4, ct, ce, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(one(e, 2, 3, 1, nullptr, ce, 8, &n, &c) == TKZ_E_ARG && one(e, 2, 3, 1, ct, nullptr, 8, &n, &c) == TKZ_E_ARG && one(e, 2, 3, 1, ct, ce, -1, &n, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_chunks_overlap_utf8(e, t, o2, 1, nullptr, 0, 3, 1, ids, 8, nullptr, dc, ct, ce, cb, cu, eb, eu, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_chunks_overlap_utf8(e, t, o2, 1, nullptr, 0, 3, 1, ids, 8, oo, nullptr, ct, ce, cb, cu, eb, eu, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_chunks_overlap_utf16(e, reinterpret_cast<const uint16_t*>(t), o2, 1, nullptr, 0, 3, 3, ids, 8, oo, dc, ct, ce, cu, eu, 8, &n, &c) == TKZ_E_ARG);
            const int32_t bad[1] = {1};
            REQUIRE(tkz_encode_chunks_overlap_utf8(e, t, 2, bad, 1, 3, 1, ids, 8, ct, ce, cb, cu, eb, eu, 8, &n, &c) == TKZ_E_ARG);
            REQUIRE(one(e, 5, 3, 1, ct, ce, 8, &n, &c) == TKZ_E_INVALID_UTF8);
            n = c = 7;
            REQUIRE(tkz_encode_chunks_overlap_utf8(e, nullptr, 0, nullptr, 0, 3, 1, ids, 8, ct, ce, cb, cu, eb, eu, 8, &n, &c) == TKZ_OK && n == 0 && c == 0);
            n = c = 7;
            REQUIRE(tkz_encode_chunks_overlap_utf16(e, nullptr, 0, allow, 1, 3, 1, ids, 8, ct, ce, cu, eu, 8, &n, &c) == TKZ_OK && n == 0 && c == 0);
            const int64_t z[3] = {0, 0, 0}; int64_t zo[3] = {5, 5, 5}, zc[3] = {5, 5, 5};
            REQUIRE(tkz_encode_batch_chunks_overlap_utf8(e, nullptr, z, 2, nullptr, 0, 3, 1, ids, 8, zo, zc, ct, ce, cb, cu, eb, eu, 0, &n, &c) == TKZ_OK && zo[2] == 0 && zc[0] == 0 &&
                    zc[1] == 0 && zc[2] == 0 && n == 0 && c == 0);
        }
    }
    int64_t calls = 0, plain = 0;
    tkz_encoder_chunks_overlap_calls(e, &calls);
    tkz_encoder_chunks_calls(e, &plain);
    REQUIRE(calls > 100 && plain == 0);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize chunks overlap ok (%lld chunk calls)\n", (long long)calls);
    return 0;
}
