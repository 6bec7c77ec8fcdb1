// A stand-alone driver for a sanitizer build of the host code behind the count entries (tkz_count_batch_device / _utf8 / _utf16, tkz_count_utf8 / _utf16) and of
// k_tokcount: compile it with the product sources and the CPU SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under
// -fsanitize=address,undefined and run it; no test runs it.  It walks the shapes of tests/count_cases.py -- sub-tiles without a document start between sub-tiles
// with some, document starts on the first and the last byte of a sub-tile, runs of empty documents, 1,024 records a sub-tile with the only mark at record 3,
// miss lists of fewer than 64, of 65 .. 128 and of more than 128 entries of both kinds, a piece of more than 1,024 bytes, a first call whose lists overflow (the
// attempt is redone), a literal across a sub-tile edge, the single launch, a host call of the batch path, the UTF-16 entries with a lone surrogate, the argument
// rows and an empty batch -- twice over one encoder.  Every result is held against the encode entry's offsets.  argv: gpt2.tiktoken
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tkz.h"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, tkz_last_error()); return 1; } } while (0)

static uint32_t g_rng = 12345;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }
static const char* kWords[] = {"the", "of", "and", "to", "in", "is", "that", "for", "it", "with", "as", "was", "on", "be", "at", "by", "this", "had", "not", "are"};
static std::string plain(size_t n) { std::string s; while (s.size() < n) { s += kWords[rnd(20)]; s += ' '; } s.resize(n); return s; }
static std::string gib(size_t n, int lo, int hi) {         // consonant strings no vocabulary holds: every piece is a miss
    std::string s;
    while (s.size() < n) { s += ' '; for (int k = lo + (int)rnd(hi - lo + 1); k > 0; --k) s += "bcdfghjklmnpqrstvwxz"[rnd(20)]; }
    s.resize(n);
    return s;
}

struct Batch { std::vector<uint8_t> bytes; std::vector<int64_t> offs{0}; void add(const std::string& d) { bytes.insert(bytes.end(), d.begin(), d.end()); offs.push_back((int64_t)bytes.size()); } };

// the device entry (the emulated build's device memory is host memory), the host entry and -- for a batch of one document -- the single entry against the encode
// entries' offsets; allowed: null, or one index
static bool check_batch(tkz_encoder* e, const Batch& b, const int32_t* allowed, int32_t n_allowed) {
    const int64_t n = (int64_t)b.offs.size() - 1, total = b.offs.back();
    std::vector<uint8_t> bytes(b.bytes);
    bytes.resize((size_t)total + 64, 0);
    void* aligned = nullptr;                                                     // (d_bytes: 16-byte aligned)
    if (tkz_host_alloc(bytes.size(), &aligned) != TKZ_OK) return false;
    std::memcpy(aligned, bytes.data(), bytes.size());
    const uint8_t* d = static_cast<const uint8_t*>(aligned);
    std::vector<int32_t> ids((size_t)total + 1);
    std::vector<int64_t> want((size_t)n + 1, -1), got((size_t)n + 1, -2), got_host((size_t)n + 1, -3);
    int64_t tw = -1, tg = -2, th = -3;
    bool ok = true;
    const tkz_status s0 = n_allowed ? tkz_encode_batch_special_device(e, d, b.offs.data(), n, total, allowed, n_allowed, ids.data(), total, want.data(), nullptr, &tw)
                                    : tkz_encode_batch_device(e, d, b.offs.data(), n, total, ids.data(), total, want.data(), nullptr, &tw);
    ok = ok && s0 == TKZ_OK;
    ok = ok && tkz_count_batch_device(e, d, b.offs.data(), n, total, allowed, n_allowed, got.data(), nullptr, &tg) == TKZ_OK && got == want && tg == tw;
    ok = ok && tkz_count_batch_utf8(e, d, b.offs.data(), n, allowed, n_allowed, got_host.data(), &th) == TKZ_OK && got_host == want && th == tw;
    if (ok && n == 1) { int64_t one = -1; ok = tkz_count_utf8(e, d, total, allowed, n_allowed, &one) == TKZ_OK && one == tw; }
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
            Batch b; const std::string g = gib(50000, 2, 2);
            b.add(g.substr(0, 700)); b.add(g.substr(700, 20000)); b.add(g.substr(20700));
            REQUIRE(check_batch(e, b, nullptr, 0));
        }
        {   // marks and skipped sub-tiles, the sub-tile edges, runs of empty documents
            Batch b;
            for (int k = 0; k < 7; ++k) b.add(plain(100));
            b.add(plain(5 * 1024));
            for (int k = 0; k < 9; ++k) b.add(plain(100));
            b.add(plain(1024 - b.offs.back() % 1024));                      // the next one starts on byte 0 of a sub-tile
            b.add(plain(2047)); b.add(plain(1 + 2048 + 1019)); b.add("abcdefghijkl" + plain(300));
            b.add(""); b.add(""); b.add(plain(2051)); b.add(""); b.add(""); b.add("");
            REQUIRE(check_batch(e, b, nullptr, 0));
            Batch empties; for (int k = 0; k < 5; ++k) empties.add("");
            REQUIRE(check_batch(e, empties, nullptr, 0));
            Batch tiny; const char* t[] = {"a", " b", "\n", "c d", "qz", " the", "x\n\n", " zqxj"};
            for (int k = 0; k < 3000; ++k) tiny.add(t[rnd(8)]);
            REQUIRE(check_batch(e, tiny, nullptr, 0));
        }
        {   // 1,024 records a sub-tile: marks behind records 256 and 768, and the only mark of a sub-tile at record 3
            std::string text; for (int k = 0; k < 640; ++k) text += "a\nb\nc\nd\n";
            Batch b; b.add(text.substr(0, 1024 + 258)); b.add(text.substr(1282, 512)); b.add(text.substr(1794, 2049)); b.add(text.substr(3843));
            REQUIRE(check_batch(e, b, nullptr, 0));
            Batch c; c.add(text.substr(0, 2051)); c.add(text.substr(2051));
            REQUIRE(check_batch(e, c, nullptr, 0));
        }
        for (int hits : {5, 2, 0}) {   // per `hits` plain words four short misses and a long one: lists of 65 .. 128 and of more than 128 entries, both kinds
            std::string s;
            while (s.size() < 6000) {
                for (int k = 0; k < hits; ++k) { s += ' '; s += kWords[rnd(20)]; }
                s += gib(12, 2, 2); s += gib(18, 17, 17);
            }
            Batch b; b.add(s.substr(0, 1500)); b.add(s.substr(1500, 1500)); b.add(s.substr(3000)); b.add(" tail of the batch");
            REQUIRE(check_batch(e, b, nullptr, 0));
        }
        {   // a piece of more than 1,024 bytes between crowded sub-tiles, documents behind it
            Batch b; b.add(gib(700, 2, 3) + std::string(1500, 'x')); b.add(gib(2048, 2, 16)); b.add(plain(300)); b.add(plain(500) + " " + std::string(3000, 'y')); b.add(plain(200));
            REQUIRE(check_batch(e, b, nullptr, 0));
        }
        {   // a literal across a sub-tile edge, allowed and not; one document: the single launch, plain and special
            Batch b; b.add(plain(1018) + eot + plain(1500)); b.add(plain(200) + eot); b.add(eot + plain(40));
            REQUIRE(check_batch(e, b, allow, 1) && check_batch(e, b, nullptr, 0));
            Batch one; one.add(plain(900) + eot + plain(700));
            REQUIRE(check_batch(e, one, allow, 1) && check_batch(e, one, nullptr, 0));
            Batch small; small.add(plain(300)); small.add(""); small.add(plain(700));           // a small host batch: the single launch
            REQUIRE(check_batch(e, small, nullptr, 0));
            Batch big; for (int k = 0; k < 64; ++k) big.add(plain(2560));                         // 160 KiB: the batch path
            REQUIRE(check_batch(e, big, nullptr, 0) && check_batch(e, big, allow, 1));
        }
        {   // the UTF-16 entries: a lone surrogate, a pair cut by a document boundary, a literal
            std::vector<uint16_t> u; std::vector<int64_t> uo{0};
            auto add = [&](const std::u16string& s) { u.insert(u.end(), s.begin(), s.end()); uo.push_back((int64_t)u.size()); };
            add(u"plain text"); add(u"lone \xD800 high"); add(u"cut \xD83D"); add(u"\xDE00 here"); add(u""); add(u"a <|endoftext|> b \xD83D\xDE00");
            const int64_t n = (int64_t)uo.size() - 1;
            std::vector<int32_t> ids(u.size() * 3 + 1);
            std::vector<int64_t> want((size_t)n + 1), got((size_t)n + 1);
            int64_t need = 0, tot = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), uo.data(), n, allow, 1, ids.data(), (int64_t)ids.size(), want.data(), &need) == TKZ_OK);
            REQUIRE(tkz_count_batch_utf16(e, u.data(), uo.data(), n, allow, 1, got.data(), &tot) == TKZ_OK && got == want && tot == need);
            REQUIRE(tkz_encode_batch_utf16(e, u.data(), uo.data(), n, ids.data(), (int64_t)ids.size(), want.data(), &need) == TKZ_OK);
            REQUIRE(tkz_count_batch_utf16(e, u.data(), uo.data(), n, nullptr, 0, got.data(), nullptr) == TKZ_OK && got == want);
            for (int64_t d = 0; d < n; ++d) {
                int64_t a = -1, b = -1;
                REQUIRE(tkz_encode_special_utf16(e, u.data() + uo[d], uo[d + 1] - uo[d], allow, 1, ids.data(), (int64_t)ids.size(), &a) == TKZ_OK);
                REQUIRE(tkz_count_utf16(e, u.data() + uo[d], uo[d + 1] - uo[d], allow, 1, &b) == TKZ_OK && a == b);
            }
        }
        {   // the argument rows, an empty text, invalid UTF-8
            const uint8_t t[5] = {'h', 'e', 0xFF, 'l', 'o'}; const int64_t o2[2] = {0, 5}; int64_t oo[2] = {7, 7}, n = 7;
            REQUIRE(tkz_count_utf8(nullptr, t, 2, nullptr, 0, &n) == TKZ_E_ARG && tkz_count_utf8(e, t, 2, nullptr, 0, nullptr) == TKZ_E_ARG);
            REQUIRE(tkz_count_utf8(e, t, -1, nullptr, 0, &n) == TKZ_E_ARG && tkz_count_utf8(e, nullptr, 2, nullptr, 0, &n) == TKZ_E_ARG);
            REQUIRE(tkz_count_batch_utf8(e, t, o2, 1, nullptr, 0, nullptr, nullptr) == TKZ_E_ARG && tkz_count_batch_utf8(e, t, nullptr, 1, nullptr, 0, oo, nullptr) == TKZ_E_ARG);
            REQUIRE(tkz_count_batch_utf8(e, t, o2, -1, nullptr, 0, oo, nullptr) == TKZ_E_ARG && tkz_count_batch_utf8(e, nullptr, o2, 1, nullptr, 0, oo, nullptr) == TKZ_E_ARG);
            const int32_t bad[1] = {1};
            REQUIRE(tkz_count_utf8(e, t, 2, bad, 1, &n) == TKZ_E_ARG && tkz_count_batch_utf8(e, t, o2, 1, bad, 1, oo, nullptr) == TKZ_E_ARG);
            REQUIRE(tkz_count_utf8(e, t, 5, nullptr, 0, &n) == TKZ_E_INVALID_UTF8 && tkz_count_batch_utf8(e, t, o2, 1, nullptr, 0, oo, nullptr) == TKZ_E_INVALID_UTF8);
            n = 7;
            REQUIRE(tkz_count_utf8(e, nullptr, 0, nullptr, 0, &n) == TKZ_OK && n == 0);
            n = 7;
            REQUIRE(tkz_count_utf16(e, nullptr, 0, allow, 1, &n) == TKZ_OK && n == 0);
            const int64_t z[3] = {0, 0, 0}; int64_t zo[3] = {5, 5, 5};
            REQUIRE(tkz_count_batch_utf8(e, nullptr, z, 2, nullptr, 0, zo, &n) == TKZ_OK && zo[0] == 0 && zo[1] == 0 && zo[2] == 0 && n == 0);
        }
    }
    int64_t calls = 0, single = 0;
    tkz_encoder_count_calls(e, &calls, &single);
    REQUIRE(calls > 60 && single > 8 && single < calls);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize count ok (%lld count calls, %lld of them by the single launch)\n", (long long)calls, (long long)single);
    return 0;
}
