// The token-budget method of the C++ host mirror (include/tkz_tokenizer.hpp) -- EncodeBatchBudgeted for std::string and std::u16string --, which calls
// tkz_encode_batch_budgeted_utf8 / _utf16: held against the rule of tkz.h restated here as the sequential greedy loop over the ids EncodeBatch / EncodeBatchUtf16
// return for the same arguments (those methods are held against the oracle by their own tests), with the calls read from tkz_encoder_budgeted_calls.  Built by
// tests/test_cpp_budgeted.py against the emulated library on CPU and against libtkz.so on the GPU.  argv: gpt2.tiktoken
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <numeric>
#include <sstream>

#include "tkz_tokenizer.hpp"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

using Rows = tkz::TikTokenizer::BudgetedRows;
static const int64_t NONE = tkz::TikTokenizer::kNoRowCap;
static int64_t calls(const tkz::TikTokenizer& tok) { int64_t c = 0; tkz_encoder_budgeted_calls(tok.native(), &c); return c; }
static std::u16string widen(const std::string& ascii) { return std::u16string(ascii.begin(), ascii.end()); }

// the rule of tkz.h over the ids of every document: bucket after bucket, row after row
static Rows rule(const std::vector<std::vector<int32_t>>& docs, int64_t L, int64_t T, int64_t B, int order, int32_t bos, int32_t eos, int32_t pad, int cut, int side, int64_t M) {
    Rows r;
    const int64_t f = (bos >= 0) + (eos >= 0), n = static_cast<int64_t>(docs.size());
    std::vector<std::vector<int32_t>> content;
    for (const auto& d : docs) {
        const int64_t nd = static_cast<int64_t>(d.size()), k = std::min<int64_t>(nd, L - f);
        std::vector<int32_t> c;
        if (bos >= 0) c.push_back(bos);
        if (cut == TKZ_TRIM_SUFFIX) c.insert(c.end(), d.begin(), d.begin() + k); else c.insert(c.end(), d.end() - k, d.end());
        if (eos >= 0) c.push_back(eos);
        r.total_tokens += nd;
        r.n_cut += nd > L - f;
        r.lens.push_back(static_cast<int32_t>(c.size()));
        content.push_back(c);
    }
    r.order.resize(static_cast<size_t>(n));
    std::iota(r.order.begin(), r.order.end(), int64_t(0));
    std::stable_sort(r.order.begin(), r.order.end(), [&](int64_t a, int64_t b) {
        return order == TKZ_BUCKET_ASCENDING ? r.lens[static_cast<size_t>(a)] < r.lens[static_cast<size_t>(b)] : r.lens[static_cast<size_t>(a)] > r.lens[static_cast<size_t>(b)];
    });
    r.rank.resize(static_cast<size_t>(n));
    for (int64_t k = 0; k < n; ++k) r.rank[static_cast<size_t>(r.order[static_cast<size_t>(k)])] = k;
    const auto width = [&](int64_t row) {
        const int64_t len = r.lens[static_cast<size_t>(r.order[static_cast<size_t>(row)])];
        return len == 0 ? int64_t(0) : (M == 0 ? L : std::min<int64_t>(L, (len + M - 1) / M * M));
    };
    r.bucket_offsets.push_back(0);
    r.bucket_rows.push_back(0);
    for (int64_t s = 0; s < n;) {
        int64_t e = s + 1;
        while (e < n && e + 1 - s <= B && (e + 1 - s) * width(order == TKZ_BUCKET_ASCENDING ? e : s) <= T) ++e;
        const int64_t W = width(order == TKZ_BUCKET_ASCENDING ? e - 1 : s);
        for (int64_t k = s; k < e; ++k) {
            const auto& c = content[static_cast<size_t>(r.order[static_cast<size_t>(k)])];
            const int64_t len = static_cast<int64_t>(c.size()), s0 = side == TKZ_PAD_LEFT ? W - len : 0;
            for (int64_t j = 0; j < W; ++j) {
                const bool in = j >= s0 && j < s0 + len;
                r.ids.push_back(in ? c[static_cast<size_t>(j - s0)] : pad);
                r.pos.push_back(in ? static_cast<int32_t>(j - s0) : 0);
                r.mask.push_back(in ? 1 : 0);
            }
        }
        r.bucket_widths.push_back(static_cast<int32_t>(W));
        r.bucket_offsets.push_back(static_cast<int64_t>(r.ids.size()));
        r.bucket_rows.push_back(e);
        s = e;
    }
    r.n_buckets = static_cast<int64_t>(r.bucket_widths.size());
    r.total_positions = static_cast<int64_t>(r.ids.size());
    return r;
}
static bool same(const Rows& a, const Rows& b) {
    return a.total_positions == b.total_positions && a.total_tokens == b.total_tokens && a.n_cut == b.n_cut && a.n_buckets == b.n_buckets && a.ids == b.ids && a.pos == b.pos &&
           a.mask == b.mask && a.lens == b.lens && a.order == b.order && a.rank == b.rank && a.bucket_offsets == b.bucket_offsets && a.bucket_rows == b.bucket_rows &&
           a.bucket_widths == b.bucket_widths;
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
    const tkz_bucket_order orders[2] = {TKZ_BUCKET_ASCENDING, TKZ_BUCKET_DESCENDING};
    const int64_t n = static_cast<int64_t>(texts.size());
    for (const auto* allowed : {&all, &only_end, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(texts, *allowed);
        for (int64_t L : {2, 7, 512, 100000}) {
            const int32_t frames[4][2] = {{-1, -1}, {11, -1}, {-1, tok.SpecialTokenId(EOT)}, {11, 50256}};
            const int64_t rows[4] = {NONE, 4, n, 1};
            int form = 0;
            for (const auto& fr : frames) {
                const int c = form & 1, s = (form >> 1) & 1;      // (the four framing forms over the four pairs of sides, M, B and T in turn, both orders)
                const int64_t M = (form == 0 ? 0 : form == 1 ? 1 : form == 2 ? 8 : 64), B = rows[form], T = L * (form == 3 ? n : form + 1) + form;
                ++form;
                for (int o = 0; o < 2; ++o) {
                    const int64_t c0 = calls(tok);
                    const Rows got = tok.EncodeBatchBudgeted(texts, L, T, B, orders[o], *allowed, fr[0], fr[1], -1, cuts[c], sides[s], M);
                    REQUIRE(calls(tok) == c0 + 1);
                    REQUIRE(same(got, rule(ids, L, T, B, orders[o], fr[0], fr[1], -1, cuts[c], sides[s], M)));
                    REQUIRE(got.bucket_rows.front() == 0 && got.bucket_rows.back() == n && got.rows(0) >= 1);
                }
                REQUIRE(same(tok.EncodeBatchBudgeted(texts, L, 3 * L, 3, TKZ_BUCKET_DESCENDING, *allowed, fr[0], fr[1], 3, cuts[1 - c], sides[1 - s]),
                             rule(ids, L, 3 * L, 3, TKZ_BUCKET_DESCENDING, fr[0], fr[1], 3, cuts[1 - c], sides[1 - s], 1)));
            }
        }
    }
    {   // the worked examples of tkz.h: documents of 5, 0, 2, 3 and 2 tokens, eos only, L = 4, T = 9
        const std::vector<std::string> ex = {" the of and to in", "", " is that", " for it with", " as was"};
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatch(ex, none);
        REQUIRE(ids[0].size() == 5 && ids[2].size() == 2 && ids[3].size() == 3 && ids[4].size() == 2);
        const auto &a = ids[0], &c = ids[2], &d = ids[3], &e = ids[4];
        const int32_t X = 9, P = 77;
        const Rows up = tok.EncodeBatchBudgeted(ex, 4, 9, NONE, TKZ_BUCKET_ASCENDING, none, -1, X, P), down = tok.EncodeBatchBudgeted(ex, 4, 9, NONE, TKZ_BUCKET_DESCENDING, none, -1, X, P);
        REQUIRE(up.n_cut == 1 && up.total_tokens == 12 && (up.lens == std::vector<int32_t>{4, 1, 3, 4, 3}) && down.lens == up.lens && up.n_buckets == 2 && down.n_buckets == 2);
        REQUIRE((up.order == std::vector<int64_t>{1, 2, 4, 0, 3}) && (up.rank == std::vector<int64_t>{3, 0, 1, 4, 2}) && (up.bucket_widths == std::vector<int32_t>{3, 4}));
        REQUIRE((up.bucket_rows == std::vector<int64_t>{0, 3, 5}) && (up.bucket_offsets == std::vector<int64_t>{0, 9, 17}) && up.total_positions == 17);
        REQUIRE((up.ids == std::vector<int32_t>{X, P, P, c[0], c[1], X, e[0], e[1], X, a[0], a[1], a[2], X, d[0], d[1], d[2], X}));
        REQUIRE((up.mask == std::vector<uint8_t>{1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}));
        REQUIRE((down.order == std::vector<int64_t>{0, 3, 2, 4, 1}) && (down.rank == std::vector<int64_t>{0, 4, 2, 1, 3}) && (down.bucket_widths == std::vector<int32_t>{4, 3}));
        REQUIRE((down.bucket_rows == std::vector<int64_t>{0, 2, 5}) && (down.bucket_offsets == std::vector<int64_t>{0, 8, 17}) && down.total_positions == 17);
        REQUIRE((down.ids == std::vector<int32_t>{a[0], a[1], a[2], X, d[0], d[1], d[2], X, c[0], c[1], X, e[0], e[1], X, X, P, P}));
        REQUIRE((down.pos == std::vector<int32_t>{0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 0, 1, 2, 0, 0, 0}));
        const Rows two = tok.EncodeBatchBudgeted(ex, 4, 9, 2, TKZ_BUCKET_ASCENDING, none, -1, X, P);
        REQUIRE((two.bucket_rows == std::vector<int64_t>{0, 2, 4, 5}) && (two.bucket_widths == std::vector<int32_t>{3, 4, 4}) && (two.bucket_offsets == std::vector<int64_t>{0, 6, 14, 18}));
        const auto same_as = tok.EncodeBatchBucketed(ex, 4, 2, TKZ_BUCKET_ASCENDING, none, -1, X, P);      // (these are the bucketed entry's buckets)
        REQUIRE(two.ids == same_as.ids && two.mask == same_as.mask && two.bucket_offsets == same_as.bucket_offsets && two.bucket_widths == same_as.bucket_widths);
    }
    {   // no texts; texts that are all empty
        const Rows e0 = tok.EncodeBatchBudgeted(std::vector<std::string>{}, 4, 8, 2, TKZ_BUCKET_ASCENDING, none, 1, 2);
        REQUIRE(e0.total_positions == 0 && e0.ids.empty() && e0.lens.empty() && e0.order.empty() && e0.buckets() == 0 && (e0.bucket_offsets == std::vector<int64_t>{0}) &&
                (e0.bucket_rows == std::vector<int64_t>{0}));
        const Rows e3 = tok.EncodeBatchBudgeted(std::vector<std::string>{"", "", ""}, 4, 8, NONE, TKZ_BUCKET_DESCENDING, none, 1, 2, 5, TKZ_TRIM_SUFFIX, TKZ_PAD_LEFT, 0);
        REQUIRE(same(e3, rule({{}, {}, {}}, 4, 8, NONE, TKZ_BUCKET_DESCENDING, 1, 2, 5, TKZ_TRIM_SUFFIX, TKZ_PAD_LEFT, 0)) && e3.total_positions == 12 && e3.n_buckets == 2 && e3.ids[0] == 5 && e3.ids[3] == 2);
        const Rows z3 = tok.EncodeBatchBudgeted(std::vector<std::string>{"", "", ""}, 4, 4, 2);
        REQUIRE(z3.total_positions == 0 && z3.ids.empty() && (z3.bucket_widths == std::vector<int32_t>{0, 0}) && (z3.order == std::vector<int64_t>{0, 1, 2}) && z3.rows(1) == 1);
    }
    {   // arguments out of range
        const auto refused = [&](int64_t L, int64_t T, int64_t B, int order, int32_t bos, int32_t eos, int64_t M) {
            try { (void)tok.EncodeBatchBudgeted(texts, L, T, B, static_cast<tkz_bucket_order>(order), none, bos, eos, 0, TKZ_TRIM_SUFFIX, TKZ_PAD_RIGHT, M); } catch (const tkz::Error&) { return true; }
            return false;
        };
        REQUIRE(refused(0, 8, 2, 0, -1, -1, 1) && refused(int64_t(1) << 31, int64_t(1) << 40, 2, 0, -1, -1, 1) && refused(1, 8, 2, 0, 1, 2, 1) && refused(8, 8, 2, 0, -2, -1, 1) &&
                refused(8, 8, 2, 0, -1, -1, -1));
        REQUIRE(refused(8, 8, 0, 0, -1, -1, 1) && refused(8, 8, -3, 0, -1, -1, 1) && refused(8, 8, int64_t(1) << 31, 0, -1, -1, 1));
        REQUIRE(refused(8, 7, 2, 0, -1, -1, 1) && refused(8, 0, 2, 0, -1, -1, 1) && refused(8, (int64_t(1) << 62) + 1, 2, 0, -1, -1, 1));
        REQUIRE(!refused(8, 8, 2, 1, -1, -1, 1) && !refused(8, int64_t(1) << 62, NONE, 0, -1, -1, 1));
    }
    // std::u16string callers: a lone surrogate, a pair, a pair cut by a document boundary, a literal
    std::vector<std::u16string> wide = {widen("Hello World"), widen(IMS + "Hello") + u" \xD83D\xDE00 " + widen(IME), std::u16string(u"lone \xD800 half"), u"", widen(longer),
                                        std::u16string(u"cut \xD83D"), std::u16string(u"\xDE00 here"), std::u16string(u"\xD83D\xDE00")};
    for (const auto* allowed : {&all, &none}) {
        const std::vector<std::vector<int32_t>> ids = tok.EncodeBatchUtf16(wide, *allowed);
        for (int64_t L : {5, 2048})
            for (int o = 0; o < 2; ++o)
                REQUIRE(same(tok.EncodeBatchBudgeted(wide, L, 2 * L + 3, 3, orders[o], *allowed, 11, 50256, 3, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 8),
                             rule(ids, L, 2 * L + 3, 3, orders[o], 11, 50256, 3, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 8)));
        REQUIRE(same(tok.EncodeBatchBudgeted(wide, 64, 100, NONE, TKZ_BUCKET_ASCENDING, *allowed), rule(ids, 64, 100, NONE, TKZ_BUCKET_ASCENDING, -1, -1, 0, TKZ_TRIM_SUFFIX, TKZ_PAD_RIGHT, 1)));
    }
    // a registered set the device path does not hold: no host path, the reference's NotImplementedException; nothing allowed is the plain call
    tkz::SpecialTokens many;
    for (int k = 0; k < 300; ++k) many.push_back({"<|s" + std::to_string(k) + "|>", 200000 + k});
    tkz::TikTokenizer tok2(vocab, many, p1);
    bool refused = false;
    try { (void)tok2.EncodeBatchBudgeted(std::vector<std::string>{"a<|s7|>b"}, 4, 4, NONE, TKZ_BUCKET_ASCENDING, {"<|s7|>"}); } catch (const tkz::NotImplementedError&) { refused = true; }
    REQUIRE(refused && tok2.EncodeBatchBudgeted(std::vector<std::string>{"a<|s7|>b"}, 64, 64).total_tokens == static_cast<int64_t>(tok2.Encode("a<|s7|>b", false).size()) && calls(tok2) == 1);
    std::printf("cpp budgeted ok\n");
    return 0;
}
