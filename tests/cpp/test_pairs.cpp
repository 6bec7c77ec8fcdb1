// The pair-rows method of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeBatchPairs for std::string and std::u16string --, which calls
// tkz_encode_batch_pairs_utf8 / _utf16: held against the rule of tkz.h applied here, an id at a time, to the ids EncodeBatch / EncodeBatchUtf16 return for the same
// arguments (those methods are held against the oracle by their own tests), with the calls read from tkz_encoder_pairs_calls.  Built by tests/test_cpp_pairs.py
// against the emulated library on CPU and against libtkz.so on the GPU.  argv: gpt2.tiktoken
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using Rows = tkz::TikTokenizer::PairRows;
using Ids = std::vector<std::vector<int32_t>>;
static int64_t calls(const tkz::TikTokenizer& tok) { int64_t c = 0; tkz_encoder_pairs_calls(tok.native(), &c); return c; }
static std::u16string widen(const std::string& ascii) { return std::u16string(ascii.begin(), ascii.end()); }

// the rule of tkz.h over the ids of the two texts of every pair: the cut an id at a time
static Rows rule(const Ids& first, const Ids& second, int64_t L, int32_t bos, int32_t sep, int s, int32_t eos, int32_t pad, int strategy, int cut, int side, int64_t M) {
    Rows r;
    const int64_t f = (bos >= 0) + s + (eos >= 0), n = static_cast<int64_t>(first.size()), R = L - f;
    std::vector<std::vector<int32_t>> content, types;
    int64_t longest = 0;
    for (int64_t p = 0; p < n; ++p) {
        const auto& A = first[static_cast<size_t>(p)];
        const auto& B = second[static_cast<size_t>(p)];
        int64_t ka = static_cast<int64_t>(A.size()), kb = static_cast<int64_t>(B.size());
        r.total_tokens += ka + kb;
        r.n_cut += ka + kb > R;
        while (ka + kb > R) {
            if (strategy == TKZ_PAIR_LONGEST_FIRST) { if (ka > kb) --ka; else --kb; }
            else if (strategy == TKZ_PAIR_ONLY_FIRST) { if (ka > 0) --ka; else --kb; }
            else { if (kb > 0) --kb; else --ka; }
        }
        std::vector<int32_t> c, t;
        if (bos >= 0) c.push_back(bos);
        if (cut == TKZ_TRIM_SUFFIX) c.insert(c.end(), A.begin(), A.begin() + ka); else c.insert(c.end(), A.end() - ka, A.end());
        for (int k = 0; k < s; ++k) c.push_back(sep);
        t.assign(c.size(), 0);
        if (cut == TKZ_TRIM_SUFFIX) c.insert(c.end(), B.begin(), B.begin() + kb); else c.insert(c.end(), B.end() - kb, B.end());
        if (eos >= 0) c.push_back(eos);
        t.resize(c.size(), 1);
        r.lens.push_back(static_cast<int32_t>(c.size()));
        r.kept.push_back(static_cast<int32_t>(ka));
        r.kept.push_back(static_cast<int32_t>(kb));
        longest = std::max<int64_t>(longest, static_cast<int64_t>(c.size()));
        content.push_back(c);
        types.push_back(t);
    }
    r.width = longest == 0 ? 0 : (M == 0 ? L : std::min<int64_t>(L, (longest + M - 1) / M * M));
    r.ids.assign(static_cast<size_t>(n * r.width), pad);
    r.pos.assign(r.ids.size(), 0);
    r.mask.assign(r.ids.size(), 0);
    r.type_ids.assign(r.ids.size(), 0);
    for (int64_t p = 0; p < n; ++p) {
        const int64_t len = static_cast<int64_t>(content[static_cast<size_t>(p)].size()), at = p * r.width + (side == TKZ_PAD_LEFT ? r.width - len : 0);
        for (int64_t j = 0; j < len; ++j) {
            r.ids[static_cast<size_t>(at + j)] = content[static_cast<size_t>(p)][static_cast<size_t>(j)];
            r.pos[static_cast<size_t>(at + j)] = static_cast<int32_t>(j);
            r.mask[static_cast<size_t>(at + j)] = 1;
            r.type_ids[static_cast<size_t>(at + j)] = static_cast<uint8_t>(types[static_cast<size_t>(p)][static_cast<size_t>(j)]);
        }
    }
    return r;
}
static bool same(const Rows& a, const Rows& b) {
    return a.width == b.width && a.total_tokens == b.total_tokens && a.n_cut == b.n_cut && a.ids == b.ids && a.pos == b.pos && a.mask == b.mask && a.type_ids == b.type_ids &&
           a.lens == b.lens && a.kept == b.kept;
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
    const std::vector<std::string> first = {"", "Hello World", IMS + "Hello World" + IME, "", IME, std::string(300, 'x'), "a" + IMS, emoji, longer, " the of and to in"};
    const std::vector<std::string> second = {"", IME, " ", "Hello World", "", "caf\xC3\xA9 " + emoji + emoji + " \xE6\xBC\xA2\xE5\xAD\x97", EOT + EOT + "x", longer, "short", " is that"};
    const tkz_trim_side cuts[2] = {TKZ_TRIM_SUFFIX, TKZ_TRIM_PREFIX};
    const tkz_pad_side sides[2] = {TKZ_PAD_RIGHT, TKZ_PAD_LEFT};
    const tkz_pair_truncation strategies[3] = {TKZ_PAIR_LONGEST_FIRST, TKZ_PAIR_ONLY_FIRST, TKZ_PAIR_ONLY_SECOND};
    for (const auto* allowed : {&all, &only_end, &none}) {
        const Ids ia = tok.EncodeBatch(first, *allowed), ib = tok.EncodeBatch(second, *allowed);
        for (int64_t L : {4, 7, 512, 100000}) {
            const int32_t frames[4][2] = {{-1, -1}, {11, -1}, {-1, tok.SpecialTokenId(EOT)}, {11, 50256}};
            int form = 0;
            for (const auto& fr : frames) {
                const int c = form & 1, sd = (form >> 1) & 1, s = form % 3;      // (the four framing forms over the four pairs of sides, the separators and M in turn)
                const int64_t M = (form == 0 ? 0 : form == 1 ? 1 : form == 2 ? 8 : 64);
                ++form;
                for (const auto st : strategies) {
                    const int64_t c0 = calls(tok);
                    const Rows got = tok.EncodeBatchPairs(first, second, L, *allowed, fr[0], s ? 50301 : -1, s, fr[1], -1, st, cuts[c], sides[sd], M);
                    REQUIRE(calls(tok) == c0 + 1);
                    REQUIRE(same(got, rule(ia, ib, L, fr[0], 50301, s, fr[1], -1, st, cuts[c], sides[sd], M)));
                }
            }
        }
    }
    {   // the worked example of tkz.h: pairs of (5, 3) and (0, 1) tokens, bos, one separator, eos, L = 8
        const std::vector<std::string> ea = {" the of and to in", ""}, eb = {" is that for", " it"};
        const Ids a = tok.EncodeBatch(ea, none), b = tok.EncodeBatch(eb, none);
        REQUIRE(a[0].size() == 5 && b[0].size() == 3 && b[1].size() == 1);
        const int32_t C = 11, S = 12, E = 13, P = 77;
        const Rows lf = tok.EncodeBatchPairs(ea, eb, 8, none, C, S, 1, E, P);
        REQUIRE(lf.width == 8 && lf.n_cut == 1 && lf.total_tokens == 9 && (lf.lens == std::vector<int32_t>{8, 4}) && (lf.kept == std::vector<int32_t>{3, 2, 0, 1}));
        REQUIRE((lf.ids == std::vector<int32_t>{C, a[0][0], a[0][1], a[0][2], S, b[0][0], b[0][1], E, C, S, b[1][0], E, P, P, P, P}));
        REQUIRE((lf.type_ids == std::vector<uint8_t>{0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 0}) && (lf.mask == std::vector<uint8_t>{1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0}));
        REQUIRE((lf.pos == std::vector<int32_t>{0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 0, 0, 0, 0}));
        const Rows pf = tok.EncodeBatchPairs(ea, eb, 8, none, C, S, 1, E, P, TKZ_PAIR_LONGEST_FIRST, TKZ_TRIM_PREFIX);
        REQUIRE((std::vector<int32_t>(pf.ids.begin(), pf.ids.begin() + 8) == std::vector<int32_t>{C, a[0][2], a[0][3], a[0][4], S, b[0][1], b[0][2], E}));
        const Rows of = tok.EncodeBatchPairs(ea, eb, 8, none, C, S, 1, E, P, TKZ_PAIR_ONLY_FIRST);
        REQUIRE((std::vector<int32_t>(of.ids.begin(), of.ids.begin() + 8) == std::vector<int32_t>{C, a[0][0], a[0][1], S, b[0][0], b[0][1], b[0][2], E}));
        const Rows os = tok.EncodeBatchPairs(ea, eb, 8, none, C, S, 1, E, P, TKZ_PAIR_ONLY_SECOND);
        REQUIRE((std::vector<int32_t>(os.ids.begin(), os.ids.begin() + 8) == std::vector<int32_t>{C, a[0][0], a[0][1], a[0][2], a[0][3], a[0][4], S, E}));
        REQUIRE((std::vector<uint8_t>(os.type_ids.begin(), os.type_ids.begin() + 8) == std::vector<uint8_t>{0, 0, 0, 0, 0, 0, 0, 1}));
    }
    {   // no pairs; pairs that are all empty; no separator id
        const std::vector<std::string> nothing, three = {"", "", ""};
        const Rows e0 = tok.EncodeBatchPairs(nothing, nothing, 4, none, 1, 3, 1, 2);
        REQUIRE(e0.width == 0 && e0.ids.empty() && e0.lens.empty() && e0.kept.empty() && e0.total_tokens == 0);
        const Rows e3 = tok.EncodeBatchPairs(three, three, 5, none, 1, 3, 2, 2, 5, TKZ_PAIR_ONLY_FIRST, TKZ_TRIM_SUFFIX, TKZ_PAD_LEFT, 0);
        REQUIRE(same(e3, rule({{}, {}, {}}, {{}, {}, {}}, 5, 1, 3, 2, 2, 5, TKZ_PAIR_ONLY_FIRST, TKZ_TRIM_SUFFIX, TKZ_PAD_LEFT, 0)) && e3.width == 5 && e3.ids[0] == 5 && e3.ids[4] == 2);
        const Rows z3 = tok.EncodeBatchPairs(three, three, 4);
        REQUIRE(z3.width == 0 && z3.ids.empty() && (z3.lens == std::vector<int32_t>{0, 0, 0}));
        const Rows ns = tok.EncodeBatchPairs(std::vector<std::string>{" the of"}, std::vector<std::string>{" and"}, 8);
        REQUIRE(ns.width == 3 && (ns.type_ids == std::vector<uint8_t>{0, 0, 1}));
    }
    for (int64_t bad : {int64_t(0), int64_t(-1), int64_t(1) << 31}) {            // a maximum length out of range
        bool refused = false;
        try { (void)tok.EncodeBatchPairs(first, second, bad); } catch (const tkz::Error&) { refused = true; }
        REQUIRE(refused);
    }
    {
        const auto refuses = [&](auto&& call) { try { call(); } catch (const tkz::Error&) { return true; } return false; };
        REQUIRE(refuses([&] { (void)tok.EncodeBatchPairs(first, second, 2, none, 1, 3, 1, 2); }));                       // the framing does not fit
        REQUIRE(refuses([&] { (void)tok.EncodeBatchPairs(first, second, 8, none, -2); }));                               // a framing id below -1
        REQUIRE(refuses([&] { (void)tok.EncodeBatchPairs(first, second, 8, none, -1, 3, 3); }));                         // three separators
        REQUIRE(refuses([&] { (void)tok.EncodeBatchPairs(first, second, 8, none, -1, -2, 1); }));                        // a separator id below -1
        REQUIRE(refuses([&] { (void)tok.EncodeBatchPairs(first, second, 8, none, -1, -1, 0, -1, 0, static_cast<tkz_pair_truncation>(3)); }));
        REQUIRE(refuses([&] { (void)tok.EncodeBatchPairs(first, second, 8, none, -1, -1, 0, -1, 0, TKZ_PAIR_LONGEST_FIRST, TKZ_TRIM_SUFFIX, TKZ_PAD_RIGHT, -1); }));
        REQUIRE(refuses([&] { (void)tok.EncodeBatchPairs(first, std::vector<std::string>{"one"}, 8); }));               // as many first texts as second ones
    }
    // std::u16string callers: a lone surrogate, a pair, a pair cut by a document boundary, a literal
    const std::vector<std::u16string> wa = {widen("Hello World"), std::u16string(u"lone \xD800 half"), widen(longer), std::u16string(u"cut \xD83D")};
    const std::vector<std::u16string> wb = {widen(IMS + "Hello") + u" \xD83D\xDE00 " + widen(IME), u"", std::u16string(u"\xD83D\xDE00"), std::u16string(u"\xDE00 here")};
    for (const auto* allowed : {&all, &none}) {
        const Ids ia = tok.EncodeBatchUtf16(wa, *allowed), ib = tok.EncodeBatchUtf16(wb, *allowed);
        for (int64_t L : {6, 2048})
            for (const auto st : strategies)
                REQUIRE(same(tok.EncodeBatchPairs(wa, wb, L, *allowed, 11, 50301, 2, 50256, 3, st, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 8),
                             rule(ia, ib, L, 11, 50301, 2, 50256, 3, st, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 8)));
        REQUIRE(same(tok.EncodeBatchPairs(wa, wb, 64, *allowed), rule(ia, ib, 64, -1, -1, 0, -1, 0, TKZ_PAIR_LONGEST_FIRST, TKZ_TRIM_SUFFIX, TKZ_PAD_RIGHT, 1)));
    }
    // a registered set the device path does not hold: no host path, the reference's NotImplementedException; nothing allowed is the plain call
    tkz::SpecialTokens many;
    for (int k = 0; k < 300; ++k) many.push_back({"<|s" + std::to_string(k) + "|>", 200000 + k});
    tkz::TikTokenizer tok2(vocab, many, p1);
    const std::vector<std::string> one = {"a<|s7|>b"}, other = {"c"};
    bool refused = false;
    try { (void)tok2.EncodeBatchPairs(one, other, 4, {"<|s7|>"}); } catch (const tkz::NotImplementedError&) { refused = true; }
    REQUIRE(refused && tok2.EncodeBatchPairs(one, other, 64).total_tokens == static_cast<int64_t>(tok2.Encode("a<|s7|>b", false).size()) + 1 && calls(tok2) == 1);
    std::printf("cpp pairs ok\n");
    return 0;
}
