// EncodeTrimSuffixBatch / EncodeTrimPrefixBatch of the C++ host mirror (include/tkz_tokenizer.hpp): one device call for the batch gives what the host walk
// over the pieces gives text by text, for every maximum and both overload shapes.  Built by tests/test_emu_trim.py against the emulated library on CPU and
// by tests/test_gpu_trim.py against libtkz.so.  argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string vocab = slurp(argv[1]);
    const std::string p1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    tkz::SpecialTokens specials = {{"<|endoftext|>", 50256}, {"<|im_start|>", 50300}, {"<|im_end|>", 50301}};
    tkz::TikTokenizer tok(vocab, specials, p1);
    const std::vector<std::string> texts = {"<|im_start|>Hello TempWorld \xF0\x9F\x98\x80 \xE6\xBC\xA2\xE5\xAD\x97<|im_end|>", "", "Hello World", "<|im_end|>",
                                            " \xF0\x9F\x98\x80 \xF0\x9F\x98\x80", "a<|endoftext|><|endoftext|>b c d e f", std::string(1500, 'a') + " tail"};
    const std::vector<std::string> all = {"<|endoftext|>", "<|im_start|>", "<|im_end|>"}, one = {"<|im_end|>"}, none;
    for (int mx = -1; mx <= 14; ++mx)
        for (const auto* allowed : {&all, &one, &none}) {
            const auto s = tok.EncodeTrimSuffixBatch(texts, *allowed, mx), p = tok.EncodeTrimPrefixBatch(texts, *allowed, mx);
            REQUIRE(s.size() == texts.size() && p.size() == texts.size());
            for (size_t t = 0; t < texts.size(); ++t) {
                REQUIRE(s[t] == tok.trim_suffix_host(texts[t], *allowed, mx));
                REQUIRE(p[t] == tok.trim_prefix_host(texts[t], *allowed, mx));
                REQUIRE(mx < 0 || static_cast<int>(s[t].first.size()) <= mx);
            }
        }
    REQUIRE(tok.EncodeTrimSuffixBatch(texts, 3) == tok.EncodeTrimSuffixBatch(texts, all, 3));
    REQUIRE(tok.EncodeTrimPrefixBatch(texts, 3, false) == tok.EncodeTrimPrefixBatch(texts, none, 3));
    REQUIRE(tok.EncodeTrimSuffixBatch({}, 3).empty());
    REQUIRE(tok.EncodeTrimSuffix(texts[0], all, 3) == tok.trim_suffix_host(texts[0], all, 3));
    std::printf("cpp trim batch ok\n");
    return 0;
}
