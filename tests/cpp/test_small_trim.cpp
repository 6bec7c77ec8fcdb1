// The single-text trim methods of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeTrimSuffix / EncodeTrimPrefix(std::string, ...) in both overload
// shapes and EncodeTrimSuffixUtf16 / EncodeTrimPrefixUtf16(std::u16string, ...) --, which call tkz_encode_trim_utf8 / _utf16: against the header's own host
// walk (trim_suffix_host etc.), with the route read from tkz_encoder_small_path_calls.  Built by tests/test_cpp_small_trim.py against the emulated library on
// CPU and against libtkz.so on the GPU.  argv: gpt2.tiktoken
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Route { int64_t calls, handed, batches, literals; };
static Route route(const tkz::TikTokenizer& tok) {
    Route r{0, 0, 0, 0};
    tkz_encoder_small_path_calls(tok.native(), &r.calls, &r.handed);
    tkz_encoder_special_stats(tok.native(), &r.batches, &r.literals);
    return r;
}
template <class T> static bool same(const T& a, const T& b) { return a.first == b.first && a.second == b.second; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string vocab = slurp(argv[1]);
    const std::string p1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    const std::string A = "x\xEF\xBF\xBD", B = "x", EOT = "<|endoftext|>", FIM = "<|fim|>";
    tkz::SpecialTokens specials = {{EOT, 50256}, {FIM, 50300}, {A, 60001}, {B, 60002}};
    tkz::TikTokenizer tok(vocab, specials, p1);
    const std::vector<std::string> all = {EOT, FIM, A, B}, eot = {EOT}, none;
    const std::vector<std::string> texts = {
        "Hello <|endoftext|> World<|fim|> and a tail", "<|endoftext|>", "a   <|endoftext|>   b", "plain text, no literal at all",
        "\xE6\xBC\xA2\xE5\xAD\x97<|fim|> \xF0\x9F\x98\x80 \xF0\x9F\x98\x80 ax\xEF\xBF\xBD done", std::string(1500, 'a') + " end<|endoftext|> x", ""};
    for (const auto* allowed : {&all, &eot, &none})
        for (size_t t = 0; t < texts.size(); ++t)
            for (int mx : {0, 1, 2, 3, 5, 9, 1000}) {
                const Route r0 = route(tok);
                const auto s = tok.EncodeTrimSuffix(texts[t], *allowed, mx);
                const auto p = tok.EncodeTrimPrefix(texts[t], *allowed, mx);
                const Route r1 = route(tok);
                REQUIRE(same(s, tok.trim_suffix_host(texts[t], *allowed, mx)));
                REQUIRE(same(p, tok.trim_prefix_host(texts[t], *allowed, mx)));
                // ONE launch each; the 1,500-byte piece is handed back; no text, no launch
                REQUIRE(r1.calls - r0.calls == (texts[t].empty() ? 0 : 2) && r1.handed - r0.handed == (t == 5 ? 2 : 0));
                REQUIRE(r1.batches - r0.batches == (allowed == &none ? 0 : 2));
            }
    {   // the (text, maxTokenCount, applySpecialTokens) shape
        REQUIRE(same(tok.EncodeTrimSuffix(texts[0], 4), tok.EncodeTrimSuffix(texts[0], all, 4)) && same(tok.EncodeTrimPrefix(texts[0], 4, true), tok.EncodeTrimPrefix(texts[0], all, 4)));
        REQUIRE(same(tok.EncodeTrimSuffix(texts[0], 4, false), tok.EncodeTrimSuffix(texts[0], none, 4)) && same(tok.EncodeTrimPrefix(texts[0], 4, false), tok.EncodeTrimPrefix(texts[0], none, 4)));
        const Route r0 = route(tok);
        REQUIRE(same(tok.EncodeTrimPrefix(texts[0], all, -1), tok.trim_prefix_host(texts[0], all, -1)));       // a negative maximum: the host walk
        REQUIRE(route(tok).calls == r0.calls);
    }
    // std::u16string: well-formed text with characters of two units, a real U+FFFD under a literal that holds one, lone surrogates under it
    const char16_t HI = 0xD83D, LO = 0xDE00;
    std::vector<std::u16string> wide = {u"a x", u"a x� b c", u"Hello <|endoftext|> World \U0001F600 \U0001F600 漢字<|fim|> tail", u"", u"tail x", u"x"};
    wide[0] += HI; wide[0] += u" b c";
    wide[4] += HI;
    wide[5] += LO; wide[5] += u"x� y";
    const std::vector<std::string> onlyA = {A};
    for (const auto* allowed : {&all, &onlyA, &eot, &none})
        for (const std::u16string& w : wide)
            for (int mx : {0, 1, 2, 3, 4, 6, 1000}) {
                const Route r0 = route(tok);
                const auto s = tok.EncodeTrimSuffixUtf16(w, *allowed, mx);
                const auto p = tok.EncodeTrimPrefixUtf16(w, *allowed, mx);
                const Route r1 = route(tok);
                REQUIRE(same(s, tok.trim_suffix_host16(w, *allowed, mx)));
                REQUIRE(same(p, tok.trim_prefix_host16(w, *allowed, mx)));
                REQUIRE(r1.calls - r0.calls == (w.empty() ? 0 : 2) && r1.handed == r0.handed);
            }
    // a registered set the device path does not hold: the host walk, from the first call on
    tkz::SpecialTokens many;
    for (int i = 0; i < 300; ++i) many.push_back({"<|s" + std::to_string(i) + "|>", 200000 + i});
    tkz::TikTokenizer tok2(vocab, many, p1);
    const std::string t2 = "a<|s7|>b <|s299|><|s30| and more";
    std::vector<std::string> names;
    for (const auto& m : many) names.push_back(m.first);
    REQUIRE(same(tok2.EncodeTrimSuffix(t2, 4), tok2.trim_suffix_host(t2, names, 4)) && same(tok2.EncodeTrimPrefix(t2, 4), tok2.trim_prefix_host(t2, names, 4)));
    REQUIRE(same(tok2.EncodeTrimSuffixUtf16(u"a<|s7|>b c d", std::vector<std::string>{"<|s7|>"}, 3), tok2.trim_suffix_host16(u"a<|s7|>b c d", std::vector<std::string>{"<|s7|>"}, 3)));
    REQUIRE(route(tok2).batches == 0);
    std::printf("cpp small trim ok\n");
    return 0;
}
