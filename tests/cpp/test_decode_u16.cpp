// Drives Decode / DecodeBatch / DecodeUtf16 / DecodeBatchUtf16 of the C++ host mirror (include/tkz_tokenizer.hpp) through the C ABI.  Built by
// tests/test_cpp_decode_u16.py, which writes decode_u16_cases.inc -- the special tokens, and per case the id lists with the bytes and the code units
// the plain reference of tests/u8_decode_cases.py expects -- and puts its directory on the include path.  argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

struct Case {
    const char* name;
    std::vector<std::vector<int32_t>> batches;
    std::vector<std::vector<uint8_t>> bytes;
    std::vector<std::vector<uint16_t>> units;
};
#include "decode_u16_cases.inc"      // static const tkz::SpecialTokens kSpecials; static const std::vector<Case> kCases;

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d (%s): %s\n", __LINE__, name, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const char* name = "setup";
    const std::string cl100k = "(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\\r\\n\\p{L}\\p{N}]?\\p{L}+|\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+";
    tkz::TikTokenizer tok(slurp(argv[1]), kSpecials, cl100k);
    REQUIRE(!kCases.empty());
    size_t docs = 0;
    for (const Case& c : kCases) {
        name = c.name;
        const std::vector<std::string> b = tok.DecodeBatch(c.batches);
        const std::vector<std::u16string> u = tok.DecodeBatchUtf16(c.batches);
        REQUIRE(b.size() == c.batches.size() && u.size() == c.batches.size());
        for (size_t d = 0; d < c.batches.size(); ++d, ++docs) {
            REQUIRE(b[d] == std::string(c.bytes[d].begin(), c.bytes[d].end()));
            REQUIRE(u[d] == std::u16string(c.units[d].begin(), c.units[d].end()));
        }
        if (!c.batches.empty()) {
            REQUIRE(tok.Decode(c.batches[0]) == b[0]);
            REQUIRE(tok.DecodeUtf16(c.batches[0]) == u[0]);
        }
    }
    name = "empty";
    REQUIRE(tok.DecodeBatchUtf16({}).empty() && tok.DecodeBatch({}).empty());
    REQUIRE(tok.DecodeUtf16({}).empty() && tok.Decode({-5, 2147483647}).empty());
    std::printf("cpp decode mirror ok: %zu cases, %zu documents\n", kCases.size(), docs);
    return 0;
}
