// A stand-alone driver for a sanitizer build of the host code behind tkz_decode_batch_utf16: compile it with the product sources and the CPU SIMT emulator
// (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under -fsanitize=address,undefined and run it; no test runs it.  It walks the edge positions of
// tests/u8_decode_cases.py -- a 4-byte char and its ill-formed cousins across tile, lane-group, bitmap-word and scan-block edges, in one document, cut by a
// boundary and with an empty document between --, ragged totals, empty input, unknown ids, the error paths and a capacity failure, twice over one encoder
// (the workspace's buffers are reused and grown).  argv: gpt2.tiktoken
#include <cstdio>
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
    REQUIRE(tkz_encoder_create(v, TKZ_PATTERN_CL100K, 0, &e) == TKZ_OK);
    int32_t id_of[256];
    for (int b = 0; b < 256; ++b) { const uint8_t k = static_cast<uint8_t>(b); id_of[b] = tkz_vocab_rank(v, &k, 1); REQUIRE(id_of[b] >= 0); }
    const std::string lit = "<|\xF0\x9F\x98\x80|>";
    const int32_t sid[1] = {60001}; const int64_t loffs[2] = {0, static_cast<int64_t>(lit.size())};
    REQUIRE(tkz_encoder_set_special_tokens(e, sid, reinterpret_cast<const uint8_t*>(lit.data()), loffs, 1) == TKZ_OK);
    const std::vector<std::vector<uint8_t>> probes = {{0xF0, 0x9F, 0x98, 0x80}, {0xF0, 0x9F, 0x98, 0x41}, {0xED, 0xA0, 0x80}, {0xF4, 0x90, 0x80, 0x80}, {0x80, 0x80}};
    for (int round = 0; round < 2; ++round)
        for (int pos : {1, 3, 15, 16, 17, 63, 64, 1023, 1024, 1025, 2048, 4095, 4096, 4097, 5000})
            for (const auto& probe : probes)
                for (int back = 1; back <= 3 && back <= pos; ++back)
                    for (int kind = 0; kind < 3; ++kind) {
                        std::vector<int32_t> ids; std::vector<int64_t> offs{0};
                        for (int q = 0; q < pos - back; ++q) ids.push_back(id_of[static_cast<uint8_t>("na\xC3\xAFve \xE4\xB8\xAD x"[q % 11])]);
                        for (size_t j = 0; j < probe.size(); ++j) {
                            if (static_cast<int>(j) == back && kind >= 1) offs.push_back(static_cast<int64_t>(ids.size()));      // a boundary at the edge
                            if (static_cast<int>(j) == back && kind == 2) offs.push_back(static_cast<int64_t>(ids.size()));      // ... and an empty document
                            ids.push_back(id_of[probe[j]]);
                        }
                        ids.push_back(60001); ids.push_back(-7); ids.push_back(id_of[0xE4]);                                    // a special, an unknown id, a ragged tail
                        offs.push_back(static_cast<int64_t>(ids.size()));
                        const int64_t n = static_cast<int64_t>(offs.size()) - 1, cap = static_cast<int64_t>(ids.size()) + 16;
                        std::vector<uint16_t> out(static_cast<size_t>(cap)); std::vector<int64_t> oo(static_cast<size_t>(n) + 1);
                        int64_t needed = 0;
                        REQUIRE(tkz_decode_batch_utf16(e, ids.data(), offs.data(), n, out.data(), cap, oo.data(), &needed) == TKZ_OK);
                        REQUIRE(oo[0] == 0 && oo[static_cast<size_t>(n)] == needed && needed > 0 && out[static_cast<size_t>(needed) - 1] == 0xFFFD);
                        std::vector<uint16_t> exact(static_cast<size_t>(needed));
                        REQUIRE(tkz_decode_batch_utf16(e, ids.data(), offs.data(), n, exact.data(), needed, oo.data(), &needed) == TKZ_OK);
                        if (needed > 1) REQUIRE(tkz_decode_batch_utf16(e, ids.data(), offs.data(), n, exact.data(), needed - 1, oo.data(), &needed) == TKZ_E_CAPACITY);
                        REQUIRE(tkz_decode_batch_utf16(e, ids.data(), offs.data(), n, nullptr, 0, oo.data(), &needed) == TKZ_E_CAPACITY);
                        std::vector<int64_t> broken = offs; broken[1] = offs[static_cast<size_t>(n)] + 1;                    // (beyond the id count)
                        if (n > 1) REQUIRE(tkz_decode_batch_utf16(e, ids.data(), broken.data(), n, out.data(), cap, oo.data(), &needed) == TKZ_E_ARG);
                    }
    const int64_t zeros[4] = {0, 0, 0, 0};
    int64_t oo[4] = {7, 7, 7, 7}, needed = 7;
    REQUIRE(tkz_decode_batch_utf16(e, nullptr, zeros, 3, nullptr, 0, oo, &needed) == TKZ_OK && oo[0] == 0 && oo[3] == 0 && needed == 0);
    REQUIRE(tkz_decode_batch_utf16(e, nullptr, zeros, 0, nullptr, 0, oo, &needed) == TKZ_OK);
    const int32_t unknown[3] = {-1, 2147483647, 70000}; const int64_t uo[3] = {0, 1, 3};
    uint16_t one[1];
    REQUIRE(tkz_decode_batch_utf16(e, unknown, uo, 2, one, 1, oo, &needed) == TKZ_OK && needed == 0 && oo[2] == 0);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize decode u16 ok\n");
    return 0;
}
