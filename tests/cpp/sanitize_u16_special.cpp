// A stand-alone driver for a sanitizer build of the host code behind tkz_encode_batch_special_utf16 / tkz_encode_batch_trim_utf16: compile it with the product
// sources and the CPU SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under -fsanitize=address,undefined and run it; no test runs it.
// It walks the edge positions of tests/u16_special_cases.py -- a lone surrogate at tile, lane-group, bitmap-word and scan-block edges under literals that hold
// U+FFFD --, empty input, the error paths and a capacity failure, twice over one encoder (the workspace's buffers are reused and grown).  argv: gpt2.tiktoken
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
    for (int round = 0; round < 2; ++round)
        for (int pos : {15, 16, 63, 64, 1023, 1024, 2047, 2048, 4094, 4095, 4096, 5000}) {
            // document 0: filler, `x` + a lone high half with the surrogate at unit `pos`; document 1 starts with the low half; document 2 is empty; document 3: `x` + U+FFFD
            std::vector<uint16_t> u; std::vector<int64_t> offs{0};
            u.push_back(0xE9); u.push_back(0x4E2D);
            while (static_cast<int>(u.size()) < pos - 1) u.push_back("ab cd "[u.size() % 6]);
            u.resize(static_cast<size_t>(pos - 1)); u.push_back('x'); u.push_back(0xD83D); offs.push_back(static_cast<int64_t>(u.size()));
            u.push_back(0xDE00); u.push_back('>'); u.push_back(' '); u.push_back('<'); u.push_back(0xDC00); u.push_back('>'); offs.push_back(static_cast<int64_t>(u.size()));
            offs.push_back(static_cast<int64_t>(u.size()));
            u.push_back('a'); u.push_back(' '); u.push_back('x'); u.push_back(0xFFFD); offs.push_back(static_cast<int64_t>(u.size()));
            const int64_t n = static_cast<int64_t>(offs.size()) - 1, cap = 3 * static_cast<int64_t>(u.size());
            std::vector<int32_t> out(static_cast<size_t>(cap)); std::vector<int64_t> oo(static_cast<size_t>(n) + 1), cu(static_cast<size_t>(n));
            int64_t needed = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), offs.data(), n, onlyA, 1, out.data(), cap, oo.data(), &needed) == TKZ_OK);
            int a = 0;
            for (int64_t k = 0; k < oo[3]; ++k) a += out[static_cast<size_t>(k)] == 60001;
            REQUIRE(a == 0);                                             // no lone surrogate is the literal's U+FFFD
            a = 0;
            for (int64_t k = oo[3]; k < needed; ++k) a += out[static_cast<size_t>(k)] == 60001;
            REQUIRE(a == 1);                                             // the real one is
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), offs.data(), n, all, 3, out.data(), cap, oo.data(), &needed) == TKZ_OK);
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), offs.data(), n, all, 3, out.data(), needed - 1, oo.data(), &needed) == TKZ_E_CAPACITY);
            for (int side = 0; side < 2; ++side)
                for (int64_t mx : {int64_t(0), int64_t(2), int64_t(1) << 40}) {
                    const int64_t tcap = mx > cap ? cap : n * mx;
                    REQUIRE(tkz_encode_batch_trim_utf16(e, u.data(), offs.data(), n, all, 3, side, mx, nullptr, out.data(), tcap, oo.data(), cu.data(), &needed) == TKZ_OK);
                    REQUIRE(mx < cap || cu[0] == (side == 0 ? offs[1] : 0));
                }
            const int64_t per_doc[4] = {1, 0, 5, 2};
            REQUIRE(tkz_encode_batch_trim_utf16(e, u.data(), offs.data(), n, onlyA, 1, TKZ_TRIM_PREFIX, 0, per_doc, out.data(), cap, oo.data(), cu.data(), &needed) == TKZ_OK);
            const int64_t bad_doc[4] = {1, -1, 5, 2};
            REQUIRE(tkz_encode_batch_trim_utf16(e, u.data(), offs.data(), n, onlyA, 1, TKZ_TRIM_PREFIX, 0, bad_doc, out.data(), cap, oo.data(), cu.data(), &needed) == TKZ_E_ARG);
            const int32_t bad[1] = {3};
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), offs.data(), n, bad, 1, out.data(), cap, oo.data(), &needed) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_trim_utf16(e, u.data(), offs.data(), n, all, 3, 0, 1, nullptr, out.data(), 0, oo.data(), cu.data(), &needed) == TKZ_E_CAPACITY);
            std::vector<int64_t> broken = offs; broken[1] = offs[2] + 1;
            REQUIRE(tkz_encode_batch_trim_utf16(e, u.data(), broken.data(), n, all, 3, 0, 4, nullptr, out.data(), cap, oo.data(), cu.data(), &needed) == TKZ_E_ARG);
        }
    const int64_t zeros[4] = {0, 0, 0, 0};
    int64_t oo[4] = {7, 7, 7, 7}, cu[3] = {7, 7, 7}, needed = 7;
    REQUIRE(tkz_encode_batch_special_utf16(e, nullptr, zeros, 3, all, 3, nullptr, 0, oo, &needed) == TKZ_OK && oo[3] == 0 && needed == 0);
    REQUIRE(tkz_encode_batch_trim_utf16(e, nullptr, zeros, 3, all, 3, 1, 5, nullptr, nullptr, 0, oo, cu, &needed) == TKZ_OK && cu[2] == 0);
    REQUIRE(tkz_encode_batch_trim_utf16(e, nullptr, zeros, 0, all, 3, 1, 5, nullptr, nullptr, 0, oo, cu, &needed) == TKZ_OK);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize u16 special ok\n");
    return 0;
}
