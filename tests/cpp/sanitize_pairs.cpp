// A stand-alone driver for a sanitizer build of the host code behind the pair entries (tkz_encode_batch_pairs_device / _utf8 / _utf16) and of k_pair_lens /
// k_pair_write: tests/test_cpp_pairs.py compiles it with the product sources and the CPU SIMT emulator (tests/hostemu/Makefile's source list, -DTKZ_HOSTEMU) under
// -fsanitize=address,undefined and runs it; nothing is loaded into an interpreter.  It walks the shapes of tests/pairs_cases.py -- the strategy edges under the four
// framing forms, 0 to 2 separators, both cut and both pad sides, L == f and L == 1, the widths around a multiple and clamped, rows of 1 to 65 columns and across
// tiles, the seam astride a group and a tile edge, n_pairs * W around a tile multiple, empty batches, a literal allowed and not, the UTF-16 entry with lone
// surrogates, the argument rows -- twice over one encoder, with buffers of EXACTLY n_pairs * W, n_pairs, n_docs and n_docs + 1 entries (a store one past the end is
// the sanitizer's to find), one short of them, and without the optional arrays.  Every result is held against the rule of tkz.h applied, an id at a time, to the ids
// and offsets of the matching encode entry.  argv: gpt2.tiktoken
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tkz.h"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, tkz_last_error()); return 1; } } while (0)

static const int64_t K = 1024;                               // kPairTile
static const int32_t SEP = 5;
static uint32_t g_rng = 2463534242u;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }
static const char* kWords[] = {"the", "of", "and", "to", "in", "is", "that", "for", "it", "with", "as", "was", "on", "be", "at", "by", "this", "had", "not", "are"};
static std::string words(int64_t n) { std::string s; for (int64_t k = 0; k < n; ++k) { s += ' '; s += kWords[rnd(20)]; } return s; }      // n tokens

struct Batch {
    std::vector<uint8_t> bytes; std::vector<int64_t> offs{0};
    void add(const std::string& d) { bytes.insert(bytes.end(), d.begin(), d.end()); offs.push_back((int64_t)bytes.size()); }
    void pair(int64_t a, int64_t b) { add(words(a)); add(words(b)); }
};
struct Rows { int64_t total = 0, W = 0, n_cut = 0; std::vector<int32_t> ids, pos, lens, kept; std::vector<uint8_t> mask, types; };
struct Form { int32_t bos, sep, s, eos; int64_t f() const { return (bos >= 0) + s + (eos >= 0); } };

// the rule of tkz.h over the uncut ids and offsets
static Rows rule(const std::vector<int32_t>& ids, const std::vector<int64_t>& O, int64_t L, const Form& F, int32_t pad, int strategy, int cut, int side, int64_t M) {
    Rows r;
    const int64_t nd = (int64_t)O.size() - 1, n = nd / 2, fb = F.bos >= 0, fe = F.eos >= 0, f = F.f(), R = L - f;
    r.total = O[(size_t)nd];
    int64_t longest = 0;
    for (int64_t p = 0; p < n; ++p) {
        int64_t ka = O[(size_t)(2 * p + 1)] - O[(size_t)(2 * p)], kb = O[(size_t)(2 * p + 2)] - O[(size_t)(2 * p + 1)];
        r.n_cut += ka + kb > R;
        while (ka + kb > R) {
            if (strategy == TKZ_PAIR_LONGEST_FIRST) { if (ka > kb) --ka; else --kb; }
            else if (strategy == TKZ_PAIR_ONLY_FIRST) { if (ka > 0) --ka; else --kb; }
            else { if (kb > 0) --kb; else --ka; }
        }
        r.kept.push_back((int32_t)ka); r.kept.push_back((int32_t)kb);
        r.lens.push_back((int32_t)(ka + kb + f));
        longest = std::max(longest, ka + kb + f);
    }
    r.W = longest == 0 ? 0 : (M == 0 ? L : std::min<int64_t>(L, (longest + M - 1) / M * M));
    r.ids.assign((size_t)(n * r.W), pad); r.pos.assign((size_t)(n * r.W), 0); r.mask.assign((size_t)(n * r.W), 0); r.types.assign((size_t)(n * r.W), 0);
    for (int64_t p = 0; p < n; ++p) {
        const int64_t len = r.lens[(size_t)p], ka = r.kept[(size_t)(2 * p)], kb = r.kept[(size_t)(2 * p + 1)];
        const int64_t sa = cut == TKZ_TRIM_SUFFIX ? O[(size_t)(2 * p)] : O[(size_t)(2 * p + 1)] - ka, sb = cut == TKZ_TRIM_SUFFIX ? O[(size_t)(2 * p + 1)] : O[(size_t)(2 * p + 2)] - kb;
        int64_t q = p * r.W + (side == TKZ_PAD_LEFT ? r.W - len : 0), j = 0;
        const auto put = [&](int32_t v, int type) { r.ids[(size_t)q] = v; r.pos[(size_t)q] = (int32_t)j; r.mask[(size_t)q] = 1; r.types[(size_t)q] = (uint8_t)type; ++q; ++j; };
        if (fb) put(F.bos, 0);
        for (int64_t k = 0; k < ka; ++k) put(ids[(size_t)(sa + k)], 0);
        for (int k = 0; k < F.s; ++k) put(F.sep, 0);
        for (int64_t k = 0; k < kb; ++k) put(ids[(size_t)(sb + k)], 1);
        if (fe) put(F.eos, 1);
    }
    return r;
}

// the device entry (the emulated build's device memory is host memory) with buffers of exactly n_pairs * W, n_pairs, n_docs and n_docs + 1 entries; without the
// optional arrays; one entry short; the host entry
static bool check_batch(tkz_encoder* e, const Batch& b, int64_t L, const Form& F, int strategy, int cut, int side, int64_t M) {
    const int64_t nd = (int64_t)b.offs.size() - 1, n = nd / 2, total = b.offs.back();
    void* aligned = nullptr;                                                     // (d_bytes: 16-byte aligned)
    if (tkz_host_alloc((size_t)total + 64, &aligned) != TKZ_OK) return false;
    std::memset(aligned, 0, (size_t)total + 64);
    if (total) std::memcpy(aligned, b.bytes.data(), (size_t)total);
    const uint8_t* d = static_cast<const uint8_t*>(aligned);
    std::vector<int32_t> want_ids((size_t)total + 1);
    std::vector<int64_t> want((size_t)nd + 1, 0);
    int64_t tw = 0;
    bool ok = nd == 0 || tkz_encode_batch_device(e, d, b.offs.data(), nd, total, want_ids.data(), total, want.data(), nullptr, &tw) == TKZ_OK;
    if (!ok) { tkz_host_free(aligned); return false; }
    const Rows R = rule(want_ids, want, L, F, -3, strategy, cut, side, M);
    const int64_t cap = n * R.W;
    std::vector<int32_t> ids((size_t)cap, -9), pos((size_t)cap, -9), lens((size_t)n, -9), kept((size_t)nd, -9);
    std::vector<uint8_t> mask((size_t)cap, 9), types((size_t)cap, 9);
    std::vector<int64_t> offs((size_t)nd + 1, -9);
    int32_t none = 0;                                                            // (an empty vector's data() may be null: the ids and lens pointers are required)
    int32_t* const pi = cap ? ids.data() : &none; int32_t* const pl = n ? lens.data() : &none;
    int64_t T = -1, W = -1, C = -1;
    const auto dev = [&](int64_t c, uint8_t* m, uint8_t* t, int32_t* p, int32_t* k, int64_t* o) {
        return tkz_encode_batch_pairs_device(e, d, b.offs.data(), nd, total, nullptr, 0, F.bos, F.sep, F.s, F.eos, L, strategy, cut, side, -3, M, pi, c, m, t, p, pl, k, o, nullptr, &T, &W, &C);
    };
    ok = dev(cap, mask.data(), types.data(), pos.data(), kept.data(), offs.data()) == TKZ_OK;
    ok = ok && T == R.total && W == R.W && C == R.n_cut && ids == R.ids && pos == R.pos && mask == R.mask && types == R.types && lens == R.lens && kept == R.kept && offs == want;
    std::fill(ids.begin(), ids.end(), -9); std::fill(lens.begin(), lens.end(), -9);
    ok = ok && dev(cap, nullptr, nullptr, nullptr, nullptr, nullptr) == TKZ_OK && ids == R.ids && lens == R.lens && W == R.W;
    std::fill(types.begin(), types.end(), 9); std::fill(kept.begin(), kept.end(), -9);
    ok = ok && dev(cap, nullptr, types.data(), nullptr, kept.data(), nullptr) == TKZ_OK && types == R.types && kept == R.kept;
    if (ok && cap > 0) {
        T = W = C = -2;
        ok = dev(cap - 1, mask.data(), types.data(), pos.data(), kept.data(), offs.data()) == TKZ_E_CAPACITY && T == R.total && W == R.W && C == R.n_cut;
    }
    std::fill(ids.begin(), ids.end(), -9); std::fill(pos.begin(), pos.end(), -9); std::fill(mask.begin(), mask.end(), 9); std::fill(types.begin(), types.end(), 9);
    std::fill(lens.begin(), lens.end(), -9); std::fill(kept.begin(), kept.end(), -9); std::fill(offs.begin(), offs.end(), -9);
    ok = ok && tkz_encode_batch_pairs_utf8(e, d, b.offs.data(), nd, nullptr, 0, F.bos, F.sep, F.s, F.eos, L, strategy, cut, side, -3, M, pi, cap, mask.data(), types.data(), pos.data(), pl,
                                           kept.data(), offs.data(), &T, &W, &C) == TKZ_OK;
    ok = ok && T == R.total && W == R.W && C == R.n_cut && ids == R.ids && pos == R.pos && mask == R.mask && types == R.types && lens == R.lens && kept == R.kept && offs == want;
    tkz_host_free(aligned);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string file = slurp(argv[1]);
    tkz_vocab* v = nullptr; tkz_encoder* e = nullptr;
    REQUIRE(tkz_vocab_from_tiktoken(reinterpret_cast<const uint8_t*>(file.data()), file.size(), &v) == TKZ_OK);
    REQUIRE(tkz_encoder_create(v, TKZ_PATTERN_CL100K, 0, &e) == TKZ_OK);
    const std::string eot = "<|endoftext|>";
    const int32_t sid[1] = {50256}; const int64_t loffs[2] = {0, (int64_t)eot.size()};
    REQUIRE(tkz_encoder_set_special_tokens(e, sid, reinterpret_cast<const uint8_t*>(eot.data()), loffs, 1) == TKZ_OK);
    const int32_t allow[1] = {0};
    const int32_t frames[4][2] = {{-1, -1}, {7, -1}, {-1, 9}, {7, 9}};
    const Form full{7, SEP, 1, 9};
    for (int round = 0; round < 2; ++round) {
        {   // the strategy edges under the four framing forms and 0 .. 2 separators, R odd and even; L == f; L == 1; empty batches
            Batch empties; for (int k = 0; k < 75; ++k) empties.pair(0, 0);
            Batch none;
            for (int64_t L : {int64_t(11), int64_t(12)}) for (const auto& fr : frames) for (int32_t s = 0; s < 3; ++s) {
                const Form F{fr[0], s ? SEP : -1, s, fr[1]};
                const int64_t f = F.f(), R = L - f, h = R / 2, H = R - h;
                const int64_t sizes[10] = {0, 1, h - 1, h, H, H + 1, R - 1, R, R + 1, 3 * L};
                Batch b; for (int64_t a : sizes) for (int64_t c : sizes) b.pair(a, c);
                for (int strategy = 0; strategy < 3; ++strategy) {
                    const int cut = (strategy + s) & 1, side = (int)(L & 1);
                    REQUIRE(check_batch(e, b, L, F, strategy, cut, side, 1) && check_batch(e, b, L, F, strategy, 1 - cut, 1 - side, 1));
                    if (f) REQUIRE(check_batch(e, b, f, F, strategy, cut, side, 1));
                    REQUIRE(check_batch(e, empties, 6, F, strategy, cut, side, side ? 0 : 8));
                }
                REQUIRE(check_batch(e, none, 6, F, 0, 0, 0, 1));
            }
            Batch one; one.pair(3, 2); one.pair(0, 0); one.pair(1, 0); one.pair(0, 4); one.pair(2, 2);
            for (int strategy = 0; strategy < 3; ++strategy) for (int cut = 0; cut < 2; ++cut) REQUIRE(check_batch(e, one, 1, Form{-1, -1, 0, -1}, strategy, cut, cut, 1));
        }
        {   // the width: the longest len a multiple of M, one below it and one above it; a round-up that exceeds L
            for (int64_t M : {int64_t(0), int64_t(1), int64_t(8), int64_t(64)}) {
                const int64_t base = std::max<int64_t>(M, 1) * (24 / std::max<int64_t>(M, 1) + 1);
                for (int64_t longest : {base - 1, base, base + 1}) {
                    Batch b; b.pair(3, 4); b.pair((longest - 3) / 2, longest - 3 - (longest - 3) / 2); b.pair(0, 0); b.pair(9, 8);
                    REQUIRE(check_batch(e, b, 200, full, 0, 0, 0, M) && check_batch(e, b, 200, full, 1, 1, 1, M));
                }
            }
            Batch b; b.pair(40, 30); b.pair(2, 3); b.pair(100, 200);
            const Form two{7, SEP, 2, 9};
            for (int strategy = 0; strategy < 3; ++strategy)
                REQUIRE(check_batch(e, b, 100, two, strategy, 0, 0, 64) && check_batch(e, b, 21, two, strategy, 1, 1, 8) && check_batch(e, b, 63, two, strategy, 0, 1, 64) &&
                        check_batch(e, b, 7, two, strategy, 1, 0, 1000));
        }
        {   // rows of 1 to 65 columns (many rows in a group of 64 positions); a row across tiles; the seam astride an edge; n_pairs * W around a tile multiple
            for (int64_t W : {int64_t(1), int64_t(3), int64_t(7), int64_t(63), int64_t(64), int64_t(65)}) {
                Batch b; for (int64_t p = 0; p < 150; ++p) b.pair((5 * p) % (W + 3), (3 * p) % (W + 2));
                const Form F = W == 1 ? Form{-1, -1, 0, -1} : Form{-1, SEP, 1, 9};
                REQUIRE(check_batch(e, b, W, F, 0, 0, 0, 0) && check_batch(e, b, W, F, 1, 1, 1, 0) && check_batch(e, b, W, F, 2, 0, 1, 0));
            }
            for (int64_t W : {K - 1, K, K + 1, 2 * K + 5}) {
                Batch b; b.pair(W / 2, W); b.pair(5, 2); b.pair(W + 7, 0);
                REQUIRE(check_batch(e, b, W, Form{7, SEP, 1, -1}, 0, 0, 0, 1) && check_batch(e, b, W, Form{7, SEP, 1, -1}, 1, 1, 1, 1));
            }
            for (int64_t seam : {int64_t(63), int64_t(64), int64_t(65), K - 1, K, K + 1}) {
                Batch b; b.pair(seam - 1, 10); b.pair(2, 1); b.pair(seam - 1, 90);
                const Form two{7, SEP, 2, 9};
                REQUIRE(check_batch(e, b, seam + 40, two, 2, 0, 0, 0) && check_batch(e, b, seam + 40, two, 0, 0, 0, 0) && check_batch(e, b, seam + 40, two, 2, 0, 1, 0));
            }
            const int64_t shapes[3][2] = {{23, 89}, {32, 64}, {3, 683}};            // 2K - 1, 2K, 2K + 1
            for (const auto& s : shapes) {
                Batch b; for (int64_t p = 0; p + 1 < s[0]; ++p) b.pair((7 * p) % (s[1] + 2), (3 * p) % 5);
                b.pair(s[1], 2);
                REQUIRE(check_batch(e, b, s[1], Form{-1, SEP, 1, 9}, 0, 0, 0, 1) && check_batch(e, b, s[1], Form{-1, SEP, 1, 9}, 1, 0, 1, 1));
            }
        }
        {   // a literal allowed, with eos set to the same id, and not allowed: against the special entry's ids; the literal at the seam
            const std::string A = words(2) + eot + words(3), B = eot + words(3) + eot;
            const std::string both = A + B + B + A;
            const int64_t offs[5] = {0, (int64_t)A.size(), (int64_t)(A.size() + B.size()), (int64_t)(A.size() + 2 * B.size()), (int64_t)both.size()};
            const uint8_t* t = reinterpret_cast<const uint8_t*>(both.data());
            for (int with = 0; with < 2; ++with) {
                std::vector<int32_t> want((size_t)both.size());
                std::vector<int64_t> wo(5);
                int64_t need = 0;
                REQUIRE(tkz_encode_batch_special_utf8(e, t, offs, 4, allow, with, want.data(), (int64_t)want.size(), wo.data(), &need) == TKZ_OK);
                for (int64_t L : {int64_t(4), int64_t(6), int64_t(7), int64_t(9), int64_t(14)}) for (int strategy = 0; strategy < 3; ++strategy) for (int cut = 0; cut < 2; ++cut) {
                    const Form F{-1, SEP, 1, 50256};
                    const Rows R = rule(want, wo, L, F, 0, strategy, cut, cut, 1);
                    std::vector<int32_t> ids(R.ids.size()), pos(R.ids.size()), lens(2), kept(4);
                    std::vector<uint8_t> mask(R.ids.size()), types(R.ids.size());
                    std::vector<int64_t> oo(5);
                    int64_t T = 0, W = 0, C = 0;
                    REQUIRE(tkz_encode_batch_pairs_utf8(e, t, offs, 4, allow, with, -1, SEP, 1, 50256, L, strategy, cut, cut, 0, 1, ids.data(), (int64_t)ids.size(), mask.data(), types.data(),
                                                        pos.data(), lens.data(), kept.data(), oo.data(), &T, &W, &C) == TKZ_OK);
                    REQUIRE(T == R.total && W == R.W && C == R.n_cut && ids == R.ids && pos == R.pos && mask == R.mask && types == R.types && lens == R.lens && kept == R.kept && oo == wo);
                    if (with && L == 7 && strategy == 0 && cut == 0) REQUIRE(kept[0] == 3 && ids[2] == 50256 && ids[3] == SEP && ids[4] == 50256);      // (the literal either side of the separator)
                }
            }
        }
        {   // the UTF-16 entry: a lone surrogate, a surrogate pair cut by a document boundary, a literal; no units at all
            std::vector<uint16_t> u; std::vector<int64_t> uo{0};
            auto add = [&](const std::u16string& s) { u.insert(u.end(), s.begin(), s.end()); uo.push_back((int64_t)u.size()); };
            add(u"plain text"); add(u"lone \xD800 high zqxjkvb"); add(u"cut \xD83D"); add(u"\xDE00 here"); add(u""); add(u"a <|endoftext|> b \xD83D\xDE00\x6F22");
            const int64_t nd = (int64_t)uo.size() - 1, n = nd / 2;
            std::vector<int32_t> want(u.size() * 3 + 1);
            std::vector<int64_t> wo((size_t)nd + 1);
            int64_t need = 0, T = 0, W = 0, C = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), uo.data(), nd, allow, 1, want.data(), (int64_t)want.size(), wo.data(), &need) == TKZ_OK);
            const Form F{7, SEP, 2, 9};
            const Rows R = rule(want, wo, 9, F, -1, TKZ_PAIR_LONGEST_FIRST, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 4);
            std::vector<int32_t> ids(R.ids.size()), pos(R.ids.size()), lens((size_t)n), kept((size_t)nd);
            std::vector<uint8_t> mask(R.ids.size()), types(R.ids.size());
            std::vector<int64_t> oo((size_t)nd + 1);
            REQUIRE(tkz_encode_batch_pairs_utf16(e, u.data(), uo.data(), nd, allow, 1, 7, SEP, 2, 9, 9, TKZ_PAIR_LONGEST_FIRST, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, -1, 4, ids.data(),
                                                 (int64_t)ids.size() - 1, mask.data(), types.data(), pos.data(), lens.data(), kept.data(), oo.data(), &T, &W, &C) == TKZ_E_CAPACITY);
            REQUIRE(T == R.total && W == R.W && C == R.n_cut);
            REQUIRE(tkz_encode_batch_pairs_utf16(e, u.data(), uo.data(), nd, allow, 1, 7, SEP, 2, 9, 9, TKZ_PAIR_LONGEST_FIRST, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, -1, 4, ids.data(), n * W,
                                                 mask.data(), types.data(), pos.data(), lens.data(), kept.data(), oo.data(), &T, &W, &C) == TKZ_OK);
            REQUIRE(ids == R.ids && pos == R.pos && mask == R.mask && types == R.types && lens == R.lens && kept == R.kept && oo == wo);
            const int64_t z[5] = {0, 0, 0, 0, 0}; int32_t zi[8]; int32_t zp[8]; uint8_t zm[8]; uint8_t zt[8]; int32_t zl[2]; int32_t zk[4]; int64_t zo[5];
            REQUIRE(tkz_encode_batch_pairs_utf16(e, nullptr, z, 4, nullptr, 0, 7, SEP, 1, 9, 4, 0, 0, 0, 6, 4, zi, 8, zm, zt, zp, zl, zk, zo, &T, &W, &C) == TKZ_OK && T == 0 && W == 4 && C == 0);
            REQUIRE(zi[0] == 7 && zi[1] == SEP && zi[2] == 9 && zi[3] == 6 && zi[7] == 6 && zm[2] == 1 && zm[3] == 0 && zt[1] == 0 && zt[2] == 1 && zt[3] == 0 && zp[2] == 2 && zp[3] == 0 &&
                    zl[1] == 3 && zk[3] == 0 && zo[4] == 0);
        }
        {   // the argument rows, invalid UTF-8
            const uint8_t t[5] = {'h', 'e', 0xFF, 'l', 'o'}; const int64_t o1[3] = {0, 1, 2}, o2[3] = {0, 2, 5}, o3[2] = {0, 2}; int64_t oo[3], T = 7, W = 7, C = 7;
            int32_t ids[8], pos[8], lens[1], kept[2]; uint8_t mask[8], types[8];
#define PAIRS(E, OFFS, ND, AL, NAL, BOS, SEPID, S, EOS, ML, ST, CUT, SIDE, MM, IDS, LENS, WP) \
    tkz_encode_batch_pairs_utf8(E, t, OFFS, ND, AL, NAL, BOS, SEPID, S, EOS, ML, ST, CUT, SIDE, 0, MM, IDS, 8, mask, types, pos, LENS, kept, oo, &T, WP, &C)
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_OK && W == lens[0] && W == 4 && T == 2 && C == 0 && kept[0] == 1 && kept[1] == 1);
            REQUIRE(PAIRS(nullptr, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o3, 1, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);                 // an odd n_docs
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -2, SEP, 1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, -2, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, -1, 1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);                  // a separator without an id
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, -1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 3, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, -7, 0, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_OK);                     // (not read without separators)
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 0, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, 7, SEP, 2, 9, 3, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, int64_t(1) << 31, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, -1, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 3, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 2, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, -1, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, -1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, int64_t(1) << 31, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 1, nullptr, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 1, ids, nullptr, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 1, ids, lens, nullptr) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_pairs_utf8(e, t, o1, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 0, 1, ids, 8, nullptr, nullptr, nullptr, lens, nullptr, nullptr, &T, &W, &C) == TKZ_OK);
            REQUIRE(tkz_encode_batch_pairs_device(e, t, o1, 2, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 0, 1, ids, 8, mask, types, pos, lens, kept, oo, nullptr, nullptr, &W, &C) == TKZ_E_ARG);
            const int32_t bad[1] = {1}, twice[2] = {0, 0};
            REQUIRE(PAIRS(e, o1, 2, bad, 1, -1, SEP, 1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o1, 2, twice, 2, -1, SEP, 1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_ARG);
            REQUIRE(PAIRS(e, o2, 2, nullptr, 0, -1, SEP, 1, 9, 6, 0, 0, 0, 1, ids, lens, &W) == TKZ_E_INVALID_UTF8);
#undef PAIRS
        }
    }
    int64_t calls = 0;
    tkz_encoder_pairs_calls(e, &calls);
    REQUIRE(calls > 100);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize pairs ok (%lld pair calls)\n", (long long)calls);
    return 0;
}
