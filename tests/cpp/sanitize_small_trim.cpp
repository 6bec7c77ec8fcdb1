// A stand-alone driver for a sanitizer build of the host code behind tkz_encode_trim_utf8 / tkz_encode_trim_utf16: the trim form of the single-launch call (the
// workspace prepared per possible piece, the kept range copied out of the page-locked block), the host transcode with its replaced-byte bitmap, the hand-over to
// the batch trim entries.  Compile it with the product sources and the CPU SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under
// -fsanitize=address,undefined and run it on the CPU; no test runs it.
// Texts that end one byte below, at and above a bitmap word, a sub-tile, 4 KiB and the trim launch's limit of 96 KiB (and at the plain launch's 128 KiB); both sides; maxima 0, 1, a quarter of the
// count, the count and far above; every result beside the batch trim entry's for the same text as one document; a capacity of exactly the kept count and of one
// less; NULL cuts; a text that is handed back; empty input and the error paths; twice over one encoder.  argv: gpt2.tiktoken
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tkz.h"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, tkz_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string file = slurp(argv[1]);
    tkz_vocab* v = nullptr; tkz_encoder* e = nullptr;
    REQUIRE(tkz_vocab_from_tiktoken(reinterpret_cast<const uint8_t*>(file.data()), file.size(), &v) == TKZ_OK);
    REQUIRE(tkz_encoder_create(v, TKZ_PATTERN_P1, 0, &e) == TKZ_OK);
    const std::string lits[3] = {"x\xEF\xBF\xBD", "<|endoftext|>", "<\xEF\xBF\xBD>"};
    const int32_t ids3[3] = {60001, 50256, 60003};
    std::string blob; int64_t loffs[4] = {0, 0, 0, 0};
    for (int i = 0; i < 3; ++i) { blob += lits[i]; loffs[i + 1] = static_cast<int64_t>(blob.size()); }
    REQUIRE(tkz_encoder_set_special_tokens(e, ids3, reinterpret_cast<const uint8_t*>(blob.data()), loffs, 3) == TKZ_OK);
    const int32_t all[3] = {0, 1, 2};
    for (int round = 0; round < 2; ++round) {
        for (int len : {1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 20000, 98303, 98304, 98305, 131072, 131073}) {
            // ASCII filler with the literal in the middle and a 4-byte character in front of the end
            std::string s;
            while (static_cast<int>(s.size()) < len) s.push_back("ab cd "[s.size() % 6]);
            if (len > 40) { s.replace(static_cast<size_t>(len / 2), 13, "<|endoftext|>"); s.replace(static_cast<size_t>(len - 6), 4, "\xF0\x9F\x98\x80"); }
            const int64_t n = static_cast<int64_t>(s.size()), offs[2] = {0, n};
            const uint8_t* text = reinterpret_cast<const uint8_t*>(s.data());
            std::vector<uint16_t> u;                                 // the same text as code units
            for (size_t i = 0; i < s.size(); ++i) { if (static_cast<unsigned char>(s[i]) == 0xF0) { u.push_back(0xD83D); u.push_back(0xDE00); i += 3; } else u.push_back(static_cast<unsigned char>(s[i])); }
            const int64_t nu = static_cast<int64_t>(u.size()), uoffs[2] = {0, nu};
            std::vector<int32_t> a(static_cast<size_t>(n) + 1), b(static_cast<size_t>(n) + 1);
            int64_t count = 0;
            REQUIRE(tkz_encode_special_utf8(e, text, n, all, 3, a.data(), n, &count) == TKZ_OK);
            for (int32_t side : {0, 1})
                for (int64_t mx : {int64_t(0), int64_t(1), count / 4, count, int64_t(1) << 40}) {
                    int64_t na = 0, nb = 0, cba = -1, cua = -1, cbb = -1, cub = -1, oo[2] = {0, 0}, c0 = 0, b0 = 0, c1 = 0, b1 = 0;
                    tkz_encoder_small_path_calls(e, &c0, &b0);
                    REQUIRE(tkz_encode_trim_utf8(e, text, n, all, 3, side, mx, a.data(), n, &na, &cba, &cua) == TKZ_OK);
                    tkz_encoder_small_path_calls(e, &c1, &b1);
                    REQUIRE(c1 - c0 == (n <= 98304 ? 1 : 0) && b1 == b0);      // (kSmallTrimMaxBytes)
                    REQUIRE(tkz_encode_batch_trim_utf8(e, text, offs, 1, all, 3, side, mx, nullptr, b.data(), n, oo, &cbb, &cub, &nb) == TKZ_OK);
                    REQUIRE(na == nb && cba == cbb && cua == cub && std::memcmp(a.data(), b.data(), static_cast<size_t>(na) * 4) == 0);
                    // exactly the kept count fits; one less does not; the cuts may be NULL
                    int64_t nc = 0;
                    REQUIRE(tkz_encode_trim_utf8(e, text, n, all, 3, side, mx, a.data(), na, &nc, nullptr, nullptr) == TKZ_OK && nc == na);
                    if (na > 0) REQUIRE(tkz_encode_trim_utf8(e, text, n, all, 3, side, mx, a.data(), na - 1, &nc, &cba, nullptr) == TKZ_E_CAPACITY && nc == na);
                    // the UTF-16 entry: the same ids, the cut in units
                    int64_t nw = 0, cuw = -1, cux = -1, nx = 0;
                    REQUIRE(tkz_encode_trim_utf16(e, u.data(), nu, all, 3, side, mx, b.data(), n, &nw, &cuw) == TKZ_OK);
                    REQUIRE(nw == na && cuw == cua && std::memcmp(a.data(), b.data(), static_cast<size_t>(na) * 4) == 0);
                    REQUIRE(tkz_encode_batch_trim_utf16(e, u.data(), uoffs, 1, all, 3, side, mx, nullptr, b.data(), n, oo, &cux, &nx) == TKZ_OK && nx == nw && cux == cuw);
                }
        }
        // lone surrogates under literals that hold U+FFFD, the surrogate at the last bit of a bitmap word and the first of the next
        for (int pos : {63, 64, 2047, 2048}) {
            std::vector<uint16_t> u;
            while (static_cast<int>(u.size()) < pos - 1) u.push_back("ab cd "[u.size() % 6]);
            u.push_back('x'); u.push_back(0xD83D); u.push_back(' '); u.push_back('x'); u.push_back(0xFFFD); u.push_back(' '); u.push_back('x'); u.push_back(0xDE00);
            const int64_t nu = static_cast<int64_t>(u.size()), uoffs[2] = {0, nu};
            std::vector<int32_t> a(3 * u.size()), b(3 * u.size());
            for (int32_t side : {0, 1})
                for (int64_t mx : {int64_t(2), int64_t(pos / 3), int64_t(1) << 40}) {
                    int64_t na = 0, nb = 0, cua = -1, cub = -1, oo[2] = {0, 0};
                    REQUIRE(tkz_encode_trim_utf16(e, u.data(), nu, all, 3, side, mx, a.data(), static_cast<int64_t>(a.size()), &na, &cua) == TKZ_OK);
                    REQUIRE(tkz_encode_batch_trim_utf16(e, u.data(), uoffs, 1, all, 3, side, mx, nullptr, b.data(), static_cast<int64_t>(b.size()), oo, &cub, &nb) == TKZ_OK);
                    REQUIRE(na == nb && cua == cub && std::memcmp(a.data(), b.data(), static_cast<size_t>(na) * 4) == 0);
                }
        }
        // a piece of more than 1024 bytes: the kernel hands the call back
        std::string g = "go <|endoftext|>" + std::string(1100, 'q') + " on";
        std::vector<int32_t> out(g.size());
        int64_t n1 = 0, cb = 0, cu = 0, c0 = 0, b0 = 0, c1 = 0, b1 = 0;
        tkz_encoder_small_path_calls(e, &c0, &b0);
        REQUIRE(tkz_encode_trim_utf8(e, reinterpret_cast<const uint8_t*>(g.data()), static_cast<int64_t>(g.size()), all, 3, 0, 2, out.data(), 2, &n1, &cb, &cu) == TKZ_OK);
        tkz_encoder_small_path_calls(e, &c1, &b1);
        REQUIRE(c1 - c0 == 1 && b1 - b0 == 1 && n1 == 2 && cb == 3 && cu == 3);
    }
    int64_t n = 7, cb = 7, cu = 7;
    REQUIRE(tkz_encode_trim_utf8(e, nullptr, 0, all, 3, 0, 5, nullptr, 0, &n, &cb, &cu) == TKZ_OK && n == 0 && cb == 0 && cu == 0);
    REQUIRE(tkz_encode_trim_utf16(e, nullptr, 0, all, 3, 1, 5, nullptr, 0, &n, &cu) == TKZ_OK && n == 0 && cu == 0);
    REQUIRE(tkz_encode_trim_utf8(e, nullptr, 5, all, 3, 0, 5, nullptr, 0, &n, &cb, &cu) == TKZ_E_ARG);
    REQUIRE(tkz_encode_trim_utf16(e, nullptr, -1, all, 3, 0, 5, nullptr, 0, &n, &cu) == TKZ_E_ARG);
    const uint8_t t3[3] = {'a', ' ', 'b'};
    int32_t o3[3];
    const int32_t bad[1] = {3};
    REQUIRE(tkz_encode_trim_utf8(e, t3, 3, all, 3, 2, 5, o3, 3, &n, &cb, &cu) == TKZ_E_ARG && tkz_encode_trim_utf8(e, t3, 3, all, 3, 0, -1, o3, 3, &n, &cb, &cu) == TKZ_E_ARG);
    REQUIRE(tkz_encode_trim_utf8(e, t3, 3, bad, 1, 0, 5, o3, 3, &n, &cb, &cu) == TKZ_E_ARG && tkz_encode_trim_utf8(e, t3, 3, all, 3, 0, 5, o3, 3, nullptr, &cb, &cu) == TKZ_E_ARG);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize small trim ok\n");
    return 0;
}
