// A stand-alone driver for a sanitizer build of the host code behind tkz_decode_utf8 / tkz_decode_utf16 (k_dec_small): compile it with the product sources and
// the CPU SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under -fsanitize=address,undefined and run it; no test runs it.  It walks the edge
// totals and positions of tests/small_decode_cases.py -- the lane, tile, workgroup-size and capacity edges of the id count; a 4-byte char and its ill-formed
// cousins across the lane-group, word and tile edges of the bytes; a tile beyond the LDS stage; the byte capacity, one byte beyond it (a hand-back) and one id
// beyond the id capacity (the batch route); unknown ids, a special in the sparse table, the argument rows and a capacity failure on every route -- twice over
// one encoder.  Every result is held against the batch entry's.  argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tkz.h"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, tkz_last_error()); return 1; } } while (0)

// both forms of one list at an exact capacity, one item short and with no buffer, against the batch entries; returns false on a difference
static bool check_list(tkz_encoder* e, const std::vector<int32_t>& ids) {
    const int64_t n = static_cast<int64_t>(ids.size()), offs[2] = {0, n};
    int64_t oo[2], needed = 0, got = -1;
    const tkz_status s0 = tkz_decode_batch(e, ids.data(), offs, 1, nullptr, 0, oo, &needed);              // (the size)
    if (s0 != (needed ? TKZ_E_CAPACITY : TKZ_OK)) return false;
    std::vector<uint8_t> want8(static_cast<size_t>(needed) + 1), got8(static_cast<size_t>(needed) + 1);
    if (tkz_decode_batch(e, ids.data(), offs, 1, want8.data(), needed, oo, &needed) != TKZ_OK) return false;
    if (tkz_decode_utf8(e, ids.data(), n, got8.data(), needed, &got) != TKZ_OK || got != needed || want8 != got8) return false;
    if (needed && (tkz_decode_utf8(e, ids.data(), n, got8.data(), needed - 1, &got) != TKZ_E_CAPACITY || got != needed)) return false;
    if (needed && (tkz_decode_utf8(e, ids.data(), n, nullptr, 0, &got) != TKZ_E_CAPACITY || got != needed)) return false;
    int64_t units = 0;
    (void)tkz_decode_batch_utf16(e, ids.data(), offs, 1, nullptr, 0, oo, &units);
    std::vector<uint16_t> want16(static_cast<size_t>(units) + 1), got16(static_cast<size_t>(units) + 1);
    if (tkz_decode_batch_utf16(e, ids.data(), offs, 1, want16.data(), units, oo, &units) != TKZ_OK) return false;
    if (tkz_decode_utf16(e, ids.data(), n, got16.data(), units, &got) != TKZ_OK || got != units || want16 != got16) return false;
    if (units && (tkz_decode_utf16(e, ids.data(), n, got16.data(), units - 1, &got) != TKZ_E_CAPACITY || got != units)) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string file = slurp(argv[1]);
    tkz_vocab* v = nullptr; tkz_encoder* e = nullptr;
    REQUIRE(tkz_vocab_from_tiktoken(reinterpret_cast<const uint8_t*>(file.data()), file.size(), &v) == TKZ_OK);
    REQUIRE(tkz_encoder_create(v, TKZ_PATTERN_CL100K, 0, &e) == TKZ_OK);
    int32_t id_of[256];
    for (int b = 0; b < 256; ++b) { const uint8_t k = static_cast<uint8_t>(b); id_of[b] = tkz_vocab_rank(v, &k, 1); REQUIRE(id_of[b] >= 0); }
    std::string key128;
    for (int k = 0; k < 32; ++k) key128 += "\xC3\x83\xC3\x82";
    const int32_t longest = tkz_vocab_rank(v, reinterpret_cast<const uint8_t*>(key128.data()), 128);        // (gpt2's longest key)
    REQUIRE(longest >= 0);
    const char* fill = "na\xC3\xAFve \xE4\xB8\xAD x";
    auto filler = [&](std::vector<int32_t>& ids, int n) { for (int q = 0; q < n; ++q) ids.push_back(id_of[static_cast<uint8_t>(fill[q % 11])]); };
    const std::vector<std::vector<uint8_t>> probes = {{0xF0, 0x9F, 0x98, 0x80}, {0xF0, 0x9F, 0x98, 0x41}, {0xED, 0xA0, 0x80}, {0xF4, 0x90, 0x80, 0x80}, {0x80, 0x80}};
    for (int table = 0; table < 2; ++table) {
        // the dense table, then an id beyond 2^22: the sparse one; the literal holds a 4-byte char
        const std::string lit = "<|\xF0\x9F\x98\x80|>";
        const int32_t sid[1] = {table ? 5000000 : 60001}; const int64_t loffs[2] = {0, static_cast<int64_t>(lit.size())};
        REQUIRE(tkz_encoder_set_special_tokens(e, sid, reinterpret_cast<const uint8_t*>(lit.data()), loffs, 1) == TKZ_OK);
        for (int round = 0; round < 2; ++round) {
            int64_t c0 = 0, h0 = 0, c1 = 0, h1 = 0;
            tkz_encoder_small_decode_calls(e, &c0, &h0);
            for (int total : {1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 32768, 32769}) {
                std::vector<int32_t> ids;
                filler(ids, total);
                REQUIRE(check_list(e, ids));
            }
            tkz_encoder_small_decode_calls(e, &c1, &h1);
            REQUIRE(c1 - c0 == 14 * 5 && h1 == h0);                                    // (five calls a list; the last list takes the batch route)
            for (int pos : {16, 17, 64, 65, 1008, 1024, 1025, 2064, 4097, 5121})
                for (const auto& probe : probes)
                    for (int back = 1; back <= 3; ++back) {
                        std::vector<int32_t> ids;
                        filler(ids, pos - back);
                        for (uint8_t b : probe) ids.push_back(id_of[b]);
                        filler(ids, 40);
                        ids.push_back(sid[0]); ids.push_back(-7); ids.push_back(id_of[0xE4]);                           // a special, an unknown id, a ragged tail
                        REQUIRE(check_list(e, ids));
                    }
            {   // a tile beyond the stage between staged tiles; the byte capacity exactly; one byte more: a hand-back
                std::vector<int32_t> ids;
                filler(ids, 1024);
                ids.insert(ids.end(), 900, longest);
                filler(ids, 124 + 1033);
                REQUIRE(check_list(e, ids));
                std::vector<int32_t> full(1024, longest);
                tkz_encoder_small_decode_calls(e, &c0, &h0);
                REQUIRE(check_list(e, full));
                tkz_encoder_small_decode_calls(e, &c1, &h1);
                REQUIRE(c1 - c0 == 5 && h1 == h0);
                full.push_back(id_of['x']);
                REQUIRE(check_list(e, full));
                tkz_encoder_small_decode_calls(e, &c0, &h0);
                REQUIRE(c0 - c1 == 5 && h0 - h1 == 5);
            }
            const std::vector<int32_t> unknown = {-1, 2147483647, 70000, 5000001};
            REQUIRE(check_list(e, unknown));
            REQUIRE(check_list(e, std::vector<int32_t>(1100, -3)));
            // the argument rows; no ids
            uint8_t b8[8]; uint16_t b16[8]; int64_t n = 7;
            REQUIRE(tkz_decode_utf8(nullptr, unknown.data(), 4, b8, 8, &n) == TKZ_E_ARG && tkz_decode_utf16(nullptr, unknown.data(), 4, b16, 8, &n) == TKZ_E_ARG);
            REQUIRE(tkz_decode_utf8(e, unknown.data(), 4, b8, 8, nullptr) == TKZ_E_ARG && tkz_decode_utf16(e, unknown.data(), 4, b16, 8, nullptr) == TKZ_E_ARG);
            REQUIRE(tkz_decode_utf8(e, unknown.data(), -1, b8, 8, &n) == TKZ_E_ARG && tkz_decode_utf16(e, unknown.data(), 4, b16, -1, &n) == TKZ_E_ARG);
            REQUIRE(tkz_decode_utf8(e, nullptr, 4, b8, 8, &n) == TKZ_E_ARG && tkz_decode_utf16(e, unknown.data(), 4, nullptr, 8, &n) == TKZ_E_ARG);
            n = 7;
            REQUIRE(tkz_decode_utf8(e, nullptr, 0, nullptr, 0, &n) == TKZ_OK && n == 0);
            n = 7;
            REQUIRE(tkz_decode_utf16(e, nullptr, 0, nullptr, 0, &n) == TKZ_OK && n == 0);
        }
    }
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize small decode ok\n");
    return 0;
}
