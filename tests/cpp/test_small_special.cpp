// The single-text Encode overloads of the C++ host mirror (include/tkz_tokenizer.hpp) with special tokens -- Encode(std::string, allowedSpecial / bool) and
// EncodeUtf16(std::u16string, allowedSpecial) -- which call tkz_encode_special_utf8 / _utf16: against the header's own host segmentation (EncodeBatch of the one
// text; encode_host16), with the route read from tkz_encoder_small_path_calls and tkz_encoder_special_stats.  Built by tests/test_cpp_small_special.py against
// the emulated library on CPU and against libtkz.so on the GPU.  argv: gpt2.tiktoken
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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string vocab = slurp(argv[1]);
    const std::string p1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    const std::string A = "x\xEF\xBF\xBD", B = "x", EOT = "<|endoftext|>", FIM = "<|fim|>";
    tkz::SpecialTokens specials = {{EOT, 50256}, {FIM, 50300}, {A, 60001}, {B, 60002}};
    tkz::TikTokenizer tok(vocab, specials, p1);
    const std::vector<std::string> all = {EOT, FIM, A, B}, eot = {EOT}, fim_b = {FIM, B}, none, unknown = {"<|nobody|>"};
    const std::vector<std::string> texts = {
        "Hello <|endoftext|> World<|fim|>", "<|endoftext|>", "a   <|endoftext|>   b", "\n\n<|endoftext|>\n", "<|endoftext|><|endoftext|>", "plain text, no literal",
        "x marks the spot <|fim|", "\xE6\xBC\xA2\xE5\xAD\x97<|fim|>\xF0\x9F\x98\x80 ax\xEF\xBF\xBD", std::string(1500, 'a') + " end<|endoftext|>", ""};
    for (const auto* allowed : {&all, &eot, &fim_b, &none, &unknown}) {
        for (size_t t = 0; t < texts.size(); ++t) {
            const Route r0 = route(tok);
            const std::vector<int32_t> got = tok.Encode(texts[t], *allowed);
            const Route r1 = route(tok);
            REQUIRE(got == tok.EncodeBatch({texts[t]}, *allowed)[0]);            // (the header's host segmentation: no special entry, no single launch of its own kind)
            const bool special = allowed != &none && allowed != &unknown;
            REQUIRE(r1.batches - r0.batches == (special ? 1 : 0));
            if (special && !texts[t].empty()) REQUIRE(r1.calls - r0.calls == 1 && r1.handed - r0.handed == (t == 8 ? 1 : 0));      // ONE launch; the 1,500-byte piece is handed back
            int64_t lit = 0;
            for (int32_t id : got) for (const auto& a : *allowed) for (const auto& s : specials) if (s.first == a && s.second == id) ++lit;
            if (special) REQUIRE(r1.literals - r0.literals == lit);
        }
    }
    {   // the bool overloads
        const Route r0 = route(tok);
        REQUIRE(tok.Encode(texts[0]) == tok.Encode(texts[0], all) && tok.Encode(texts[0], true) == tok.Encode(texts[0], all));
        REQUIRE(tok.Encode(texts[0], false) == tok.Encode(texts[0], none));
        const Route r1 = route(tok);
        REQUIRE(r1.batches - r0.batches == 4);
    }
    // std::u16string: well-formed text, a real U+FFFD under a literal that holds one, lone surrogates under it
    const char16_t HI = 0xD83D, LO = 0xDE00;
    std::vector<std::u16string> wide = {u"a x", u"a x� b", u"Hello <|endoftext|> World \U0001F600 漢字<|fim|>", u"", u"tail x", u"x"};
    wide[0] += HI; wide[0] += u" b";
    wide[4] += HI;
    wide[5] += LO; wide[5] += u"x�";
    const std::vector<std::string> onlyA = {A};
    for (const auto* allowed : {&all, &onlyA, &eot, &none})
        for (const std::u16string& w : wide) {
            const Route r0 = route(tok);
            REQUIRE(tok.EncodeUtf16(w, *allowed) == tok.encode_host16(w, *allowed));
            const Route r1 = route(tok);
            if (allowed != &none) REQUIRE(r1.batches - r0.batches == 1 && r1.calls - r0.calls == (w.empty() ? 0 : 1) && r1.handed == r0.handed);
        }
    auto has = [](const std::vector<int32_t>& v, int32_t id) { for (int32_t x : v) if (x == id) return true; return false; };
    REQUIRE(!has(tok.EncodeUtf16(wide[0], onlyA), 60001) && has(tok.EncodeUtf16(wide[0], all), 60002) && !has(tok.EncodeUtf16(wide[0], all), 60001));
    REQUIRE(has(tok.EncodeUtf16(wide[1], onlyA), 60001) && has(tok.EncodeUtf16(wide[5], onlyA), 60001));
    // a registered set the device path does not hold: the host segmentation, from the first call on
    tkz::SpecialTokens many;
    for (int i = 0; i < 300; ++i) many.push_back({"<|s" + std::to_string(i) + "|>", 200000 + i});
    tkz::TikTokenizer tok2(vocab, many, p1);
    const std::string t2 = "a<|s7|>b <|s299|><|s30|";
    const std::vector<int32_t> got2 = tok2.Encode(t2, true);
    REQUIRE(has(got2, 200007) && has(got2, 200299) && !has(got2, 200030) && got2 == tok2.EncodeBatch({t2}, true)[0]);
    REQUIRE(tok2.EncodeUtf16(u"a<|s7|>b", std::vector<std::string>{"<|s7|>"}) == tok2.Encode("a<|s7|>b", std::vector<std::string>{"<|s7|>"}));
    REQUIRE(route(tok2).batches == 0);
    std::printf("cpp small special ok\n");
    return 0;
}
