// A stand-alone driver for a sanitizer build of the host code behind tkz_encode_special_utf16 / tkz_encode_special_utf8: the host transcode with its
// replaced-byte bitmap, the page-locked block the bitmap travels in, the hand-over to the batch path.  Compile it with the product sources and the CPU SIMT
// emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under -fsanitize=address,undefined and run it on the CPU; no test runs it.
// It puts a lone surrogate, under literals that hold U+FFFD, at the last bit of a bitmap word and the first of the next, at the edges of the literal scan's
// 2 KiB text stage and of a sub-tile, at the very end of the string (the bitmap's last word) and at the single-launch limit (one unit below, at and above
// 128 KiB of UTF-8: the last bitmap word of the block, then the batch path); empty input, the error paths and a capacity failure; twice over one encoder.
// argv: gpt2.tiktoken
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
    const std::string lits[3] = {"x\xEF\xBF\xBD", "x", "<\xEF\xBF\xBD>"};
    const int32_t ids3[3] = {60001, 60002, 60003};
    std::string blob; int64_t loffs[4] = {0, 0, 0, 0};
    for (int i = 0; i < 3; ++i) { blob += lits[i]; loffs[i + 1] = static_cast<int64_t>(blob.size()); }
    REQUIRE(tkz_encoder_set_special_tokens(e, ids3, reinterpret_cast<const uint8_t*>(blob.data()), loffs, 3) == TKZ_OK);
    const int32_t all[3] = {0, 1, 2}, onlyA[1] = {0};
    auto count = [](const std::vector<int32_t>& out, int64_t n, int32_t id) { int a = 0; for (int64_t k = 0; k < n; ++k) a += out[static_cast<size_t>(k)] == id; return a; };
    for (int round = 0; round < 2; ++round) {
        for (int pos : {1, 2, 63, 64, 65, 1023, 1024, 2047, 2048, 2049, 4096, 5000, 131071, 131072, 131073}) {
            // ASCII filler (a unit is a byte), `x` + a lone high half with the surrogate at unit `pos`; then `x` + a real U+FFFD; the string ends in a lone low half
            std::vector<uint16_t> u;
            while (static_cast<int>(u.size()) < pos - 1) u.push_back("ab cd "[u.size() % 6]);
            u.push_back('x'); u.push_back(0xD83D); u.push_back(' '); u.push_back('x'); u.push_back(0xFFFD); u.push_back(' '); u.push_back('x'); u.push_back(0xDE00);
            const int64_t n = static_cast<int64_t>(u.size()), cap = 3 * n;
            std::vector<int32_t> out(static_cast<size_t>(cap));
            int64_t needed = 0, calls0 = 0, back0 = 0, calls1 = 0, back1 = 0;
            tkz_encoder_small_path_calls(e, &calls0, &back0);
            REQUIRE(tkz_encode_special_utf16(e, u.data(), n, onlyA, 1, out.data(), cap, &needed) == TKZ_OK);
            tkz_encoder_small_path_calls(e, &calls1, &back1);
            REQUIRE(calls1 - calls0 == (n + 6 <= 131072 ? 1 : 0) && back1 == back0);      // (three U+FFFD of three bytes each: n + 6 bytes)
            REQUIRE(count(out, needed, 60001) == 1);                     // the real U+FFFD is the literal's, no lone surrogate is
            REQUIRE(tkz_encode_special_utf16(e, u.data(), n, all, 3, out.data(), cap, &needed) == TKZ_OK);
            REQUIRE(count(out, needed, 60001) == 1 && count(out, needed, 60002) == 2);
            const int64_t full = needed;
            REQUIRE(tkz_encode_special_utf16(e, u.data(), n, all, 3, out.data(), full - 1, &needed) == TKZ_E_CAPACITY && needed == full);
            REQUIRE(tkz_encode_special_utf16(e, u.data(), n, nullptr, 0, out.data(), cap, &needed) == TKZ_OK);
            const int32_t bad[1] = {3}, twice[2] = {1, 1};
            REQUIRE(tkz_encode_special_utf16(e, u.data(), n, bad, 1, out.data(), cap, &needed) == TKZ_E_ARG);
            REQUIRE(tkz_encode_special_utf16(e, u.data(), n, twice, 2, out.data(), cap, &needed) == TKZ_E_ARG);
            // the same string without its surrogates, through the UTF-8 entry
            std::string s8;
            for (uint16_t c : u) if (c < 0x80) s8.push_back(static_cast<char>(c));
            REQUIRE(tkz_encode_special_utf8(e, reinterpret_cast<const uint8_t*>(s8.data()), static_cast<int64_t>(s8.size()), all, 3, out.data(), cap, &needed) == TKZ_OK);
            REQUIRE(count(out, needed, 60002) == 3);
        }
        // a piece of more than 1024 bytes beside the literal: the kernel hands the call back, the batch path transcodes the units itself
        std::vector<uint16_t> g(1100, 'q');
        g.push_back('x'); g.push_back(0xDC00); g.push_back('x'); g.push_back(0xFFFD);
        std::vector<int32_t> out(3 * g.size());
        int64_t needed = 0, calls0 = 0, back0 = 0, calls1 = 0, back1 = 0;
        tkz_encoder_small_path_calls(e, &calls0, &back0);
        REQUIRE(tkz_encode_special_utf16(e, g.data(), static_cast<int64_t>(g.size()), all, 3, out.data(), static_cast<int64_t>(out.size()), &needed) == TKZ_OK);
        tkz_encoder_small_path_calls(e, &calls1, &back1);
        REQUIRE(calls1 - calls0 == 1 && back1 - back0 == 1 && count(out, needed, 60001) == 1 && count(out, needed, 60002) == 1);
    }
    int64_t needed = 7;
    REQUIRE(tkz_encode_special_utf16(e, nullptr, 0, all, 3, nullptr, 0, &needed) == TKZ_OK && needed == 0);
    REQUIRE(tkz_encode_special_utf8(e, nullptr, 0, all, 3, nullptr, 0, &needed) == TKZ_OK && needed == 0);
    REQUIRE(tkz_encode_special_utf16(e, nullptr, 5, all, 3, nullptr, 0, &needed) == TKZ_E_ARG);
    REQUIRE(tkz_encode_special_utf16(e, nullptr, -1, all, 3, nullptr, 0, &needed) == TKZ_E_ARG);
    int64_t batches = 0, literals = 0;
    tkz_encoder_special_stats(e, &batches, &literals);
    REQUIRE(batches == 2 * (15 * 3 + 1) + 2 && literals > 0);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize small special u16 ok\n");
    return 0;
}
