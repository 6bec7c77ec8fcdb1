// The padded-rows method of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeBatchPadded for std::string and std::u16string --, which calls
// tkz_encode_batch_padded_utf8 / _utf16: held against the rule of tkz.h applied here to the ids EncodeBatch / EncodeBatchUtf16 return for the same arguments
// (those methods are held against the oracle by their own tests), with the calls read from tkz_encoder_padded_calls.  Built by tests/test_cpp_padded.py against
// the emulated library on CPU and against libtkz.so on the GPU.  argv: gpt2.tiktoken
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using Rows = tkz::TikTokenizer::PaddedRows;
static int64_t calls(const tkz::TikTokenizer& tok) { int64_t c = 0; tkz_encoder_padded_calls(tok.native(), &c); return c; }
static std::u16string widen(const std::string& ascii) { return std::u16string(ascii.begin(), ascii.end()); }

// the rule of tkz.h over the ids of every document
static Rows rule(const std::vector<std::vector<int32_t>>& docs, int64_t L, int32_t bos, int32_t eos, int32_t pad, int cut, int side, int64_t M) {
    Rows r;
    const int64_t f = (bos >= 0) + (eos >= 0), n = static_cast<int64_t>(docs.size());
    std::vector<std::vector<int32_t>> content;
    int64_t longest = 0;
    for (const auto& d : docs) {
        const int64_t nd = static_cast<int64_t>(d.size()), k = std::min<int64_t>(nd, L - f);
        std::vector<int32_t> c;
        if (bos >= 0) c.push_back(bos);
        if (cut == TKZ_TRIM_SUFFIX) c.insert(c.end(), d.begin(), d.begin() + k); else c.insert(c.end(), d.end() - k, d.end());
        if (eos >= 0) c.push_back(eos);
        r.total_tokens += nd;
        r.n_cut += nd > L - f;
        r.lens.push_back(static_cast<int32_t>(c.size()));
        longest = std::max<int64_t>(longest, static_cast<int64_t>(c.size()));
        content.push_back(c);
    }
    r.width = longest == 0 ? 0 : (M == 0 ? L : std::min<int64_t>(L, (longest + M - 1) / M * M));
    r.ids.assign(static_cast<size_t>(n * r.width), pad);
    r.pos.assign(r.ids.size(), 0);
    r.mask.assign(r.ids.size(), 0);
    for (int64_t d = 0; d < n; ++d) {
        const int64_t len = static_cast<int64_t>(content[static_cast<size_t>(d)].size()), s = d * r.width + (side == TKZ_PAD_LEFT ? r.width - len : 0);
        for (int64_t j = 0; j < len; ++j) {
            r.ids[static_cast<size_t>(s + j)] = content[static_cast<size_t>(d)][static_cast<size_t>(j)];
            r.pos[static_cast<size_t>(s + j)] = static_cast<int32_t>(j);
            r.mask[static_cast<size_t>(s + j)] = 1;
        }
    }
    return r;
}
static bool same(const Rows& a, const Rows& b) {
    return a.width == b.width && a.total_tokens == b.total_tokens && a.n_cut == b.n_cut && a.ids == b.ids && a.pos == b.pos && a.mask == b.mask && a.lens == b.lens;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string vocab = slurp(argv[1]);
    const std::string p1 = "'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+";
    const std::string EOT = "<|endoftext|>", IMS = "<|im_start|>", IME = "<|im_end|>";
    tkz::SpecialTokens specials = {{EOT, 50256}, {IMS, 50300}, {IME, 50301}};
    tkz::TikTokenizer tok(vocab, specials, p1);
    const std::vector<std::string> all = {EOT, IMS, IME}, only_end = {IME}, none;
    std::string longer;
    for (int k = 0; k < 3000; ++k) longer += (k % 97 == 0) ? EOT : (k % 5 == 0 ? " it's" : (k % 7 == 0 ? " zqxjkv" : " token"));
    const std::string emoji = "\xF0\x9F\x98\x80";
    const std::vector<std::string> texts = {"", "Hello World", IMS + "Hello World" + IME, "", "", IME, " ", std::string(300, 'x'), "a" + IMS, EOT + EOT + "x", emoji,
                                            "caf\xC3\xA9 " + emoji + emoji + " \xE6\xBC\xA2\xE5\xAD\x97", longer, ""};
    const tkz_trim_side cuts[2] = {TKZ_TRIM_SUFFIX, TKZ_TRIM_PREFIX};
    const tkz_pad_side sides[2] = {TKZ_PAD_RIGHT, TKZ_PAD_LEFT};
    for (const auto* allowed : {&all, &only_end, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(texts, *allowed);
        for (int64_t L : {2, 7, 512, 100000}) {
            const int32_t frames[4][2] = {{-1, -1}, {11, -1}, {-1, tok.SpecialTokenId(EOT)}, {11, 50256}};
            int form = 0;
            for (const auto& fr : frames) {
                const int c = form & 1, s = (form >> 1) & 1;      // (the four framing forms over the four pairs of sides, M in turn)
                const int64_t M = (form == 0 ? 0 : form == 1 ? 1 : form == 2 ? 8 : 64);
                ++form;
                const int64_t c0 = calls(tok);
                const Rows got = tok.EncodeBatchPadded(texts, L, *allowed, fr[0], fr[1], -1, cuts[c], sides[s], M);
                REQUIRE(calls(tok) == c0 + 1);
                REQUIRE(same(got, rule(ids, L, fr[0], fr[1], -1, cuts[c], sides[s], M)));
                REQUIRE(same(tok.EncodeBatchPadded(texts, L, *allowed, fr[0], fr[1], 3, cuts[1 - c], sides[1 - s]), rule(ids, L, fr[0], fr[1], 3, cuts[1 - c], sides[1 - s], 1)));
            }
        }
    }
    {   // the worked example of tkz.h: documents of 5, 0 and 2 tokens, bos only, L = 4
        const std::vector<std::string> ex = {" the of and to in", "", " is that"};
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(ex, none);
        REQUIRE(ids[0].size() == 5 && ids[2].size() == 2);
        const int32_t B = 11, P = 77;
        const Rows a = tok.EncodeBatchPadded(ex, 4, none, B, -1, P), b = tok.EncodeBatchPadded(ex, 4, none, B, -1, P, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT);
        REQUIRE(a.width == 4 && a.n_cut == 1 && a.total_tokens == 7 && (a.lens == std::vector<int32_t>{4, 1, 3}) && b.width == 4 && b.lens == a.lens);
        REQUIRE((a.ids == std::vector<int32_t>{B, ids[0][0], ids[0][1], ids[0][2], B, P, P, P, B, ids[2][0], ids[2][1], P}));
        REQUIRE((a.pos == std::vector<int32_t>{0, 1, 2, 3, 0, 0, 0, 0, 0, 1, 2, 0}) && (a.mask == std::vector<uint8_t>{1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 0}));
        REQUIRE((b.ids == std::vector<int32_t>{B, ids[0][2], ids[0][3], ids[0][4], P, P, P, B, P, B, ids[2][0], ids[2][1]}));
        REQUIRE((b.pos == std::vector<int32_t>{0, 1, 2, 3, 0, 0, 0, 0, 0, 0, 1, 2}) && (b.mask == std::vector<uint8_t>{1, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1}));
    }
    {   // no texts; texts that are all empty
        const Rows e0 = tok.EncodeBatchPadded(std::vector<std::string>{}, 4, none, 1, 2);
        REQUIRE(e0.width == 0 && e0.ids.empty() && e0.lens.empty() && e0.total_tokens == 0);
        const Rows e3 = tok.EncodeBatchPadded(std::vector<std::string>{"", "", ""}, 4, none, 1, 2, 5, TKZ_TRIM_SUFFIX, TKZ_PAD_LEFT, 0);
        REQUIRE(same(e3, rule({{}, {}, {}}, 4, 1, 2, 5, TKZ_TRIM_SUFFIX, TKZ_PAD_LEFT, 0)) && e3.width == 4 && e3.ids[0] == 5 && e3.ids[3] == 2);
        const Rows z3 = tok.EncodeBatchPadded(std::vector<std::string>{"", "", ""}, 4);
        REQUIRE(z3.width == 0 && z3.ids.empty() && (z3.lens == std::vector<int32_t>{0, 0, 0}));
    }
    for (int64_t bad : {int64_t(0), int64_t(-1), int64_t(1) << 31}) {            // a maximum length out of range; one the framing does not fit; a framing id below -1
        bool refused = false;
        try { (void)tok.EncodeBatchPadded(texts, bad); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
    }
    {
        bool refused = false;
        try { (void)tok.EncodeBatchPadded(texts, 1, none, 1, 2); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
        refused = false;
        try { (void)tok.EncodeBatchPadded(texts, 8, none, -2); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
        refused = false;
        try { (void)tok.EncodeBatchPadded(texts, 8, none, -1, -1, 0, TKZ_TRIM_SUFFIX, TKZ_PAD_RIGHT, -1); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
    }
    // std::u16string callers: a lone surrogate, a pair, a pair cut by a document boundary, a literal
    std::vector<std::u16string> wide = {widen("Hello World"), widen(IMS + "Hello") + u" \xD83D\xDE00 " + widen(IME), std::u16string(u"lone \xD800 half"), u"", widen(longer),
                                        std::u16string(u"cut \xD83D"), std::u16string(u"\xDE00 here"), std::u16string(u"\xD83D\xDE00")};
    for (const auto* allowed : {&all, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatchUtf16(wide, *allowed);
        for (int64_t L : {5, 2048})
            REQUIRE(same(tok.EncodeBatchPadded(wide, L, *allowed, 11, 50256, 3, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 8), rule(ids, L, 11, 50256, 3, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 8)));
        REQUIRE(same(tok.EncodeBatchPadded(wide, 64, *allowed), rule(ids, 64, -1, -1, 0, TKZ_TRIM_SUFFIX, TKZ_PAD_RIGHT, 1)));
    }
    // a registered set the device path does not hold: no host path, the reference's NotImplementedException; nothing allowed is the plain call
    tkz::SpecialTokens many;
    for (int k = 0; k < 300; ++k) many.push_back({"<|s" + std::to_string(k) + "|>", 200000 + k});
    tkz::TikTokenizer tok2(vocab, many, p1);
    bool refused = false;
    try { (void)tok2.EncodeBatchPadded(std::vector<std::string>{"a<|s7|>b"}, 4, {"<|s7|>"}); } catch (const tkz::NotImplementedError&) { refused = true; }
    REQUIRE(refused && tok2.EncodeBatchPadded(std::vector<std::string>{"a<|s7|>b"}, 64).total_tokens == static_cast<int64_t>(tok2.Encode("a<|s7|>b", false).size()) && calls(tok2) == 1);
    std::printf("cpp padded ok\n");
    return 0;
}
