// A stand-alone driver for a sanitizer build of the host code behind the budgeted entries (tkz_encode_batch_budgeted_device / _utf8 / _utf16) and of k_tbk_mark /
// k_tbk_chain / k_tbk_table / k_tbk_write: tests/test_cpp_budgeted.py compiles it with the product sources and the CPU SIMT emulator (tests/hostemu/Makefile's
// source list, -DTKZ_HOSTEMU) under -fsanitize=address,undefined and runs it; nothing is loaded into an interpreter.  It walks the shapes of
// tests/budgeted_cases.py -- the worked examples, one run with a row a bucket, buckets that swallow runs and entries that jump over them, width 0, 1 .. 129 runs
// (the chain looks at 64 at once), documents around the sort's and the marking tile, only B binding, random small batches, empty batches, a literal allowed and
// not, the UTF-16 entry, the argument rows -- twice over one encoder, with buffers of EXACTLY P, n_docs, n_docs + 1, n_buckets and n_buckets + 1 entries (a store
// one past the end is the sanitizer's to find), one short of P and of n_buckets, and without mask, pos, offsets and rank.  Every result is held against the rule of
// tkz.h, restated as the sequential greedy loop over the ids and offsets of the matching encode entry.  argv: gpt2.tiktoken
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "tkz.h"

static std::string slurp(const char* p) { std::ifstream f(p, std::ios::binary); std::stringstream ss; ss << f.rdbuf(); return ss.str(); }
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #c, tkz_last_error()); return 1; } } while (0)

static const int64_t K = 1024, KM = 256;                     // kBktSortTile, kTbkMarkTile
static const int64_t BMAX = (int64_t(1) << 31) - 1, TMAX = int64_t(1) << 62;
static uint32_t g_rng = 2463534242u;
static uint32_t rnd(uint32_t n) { g_rng = g_rng * 1664525u + 1013904223u; return (g_rng >> 8) % n; }
static const char* kWords[] = {"the", "of", "and", "to", "in", "is", "that", "for", "it", "with", "as", "was", "on", "be", "at", "by", "this", "had", "not", "are"};
static std::string words(int64_t n) { std::string s; for (int64_t k = 0; k < n; ++k) { s += ' '; s += kWords[rnd(20)]; } return s; }      // n tokens

struct Batch { std::vector<uint8_t> bytes; std::vector<int64_t> offs{0}; void add(const std::string& d) { bytes.insert(bytes.end(), d.begin(), d.end()); offs.push_back((int64_t)bytes.size()); } };
struct Rows { int64_t total = 0, P = 0, n_cut = 0, nb = 0; std::vector<int32_t> ids, pos, lens, widths; std::vector<uint8_t> mask; std::vector<int64_t> order, rank, boffs, brows; };

// the rule of tkz.h over the uncut ids and offsets: bucket after bucket, row after row
static Rows rule(const std::vector<int32_t>& ids, const std::vector<int64_t>& O, int64_t L, int64_t T, int64_t B, int order, int32_t bos, int32_t eos, int32_t pad, int cut, int side, int64_t M) {
    Rows r;
    const int64_t n = (int64_t)O.size() - 1, fb = bos >= 0, fe = eos >= 0, f = fb + fe;
    r.total = O[(size_t)n];
    for (int64_t d = 0; d < n; ++d) {
        const int64_t nd = O[(size_t)d + 1] - O[(size_t)d], k = std::min<int64_t>(nd, L - f);
        r.lens.push_back((int32_t)(k + f));
        r.n_cut += nd > L - f;
    }
    r.order.resize((size_t)n);
    std::iota(r.order.begin(), r.order.end(), int64_t(0));
    std::stable_sort(r.order.begin(), r.order.end(), [&](int64_t a, int64_t b) { return order == TKZ_BUCKET_ASCENDING ? r.lens[(size_t)a] < r.lens[(size_t)b] : r.lens[(size_t)a] > r.lens[(size_t)b]; });
    r.rank.resize((size_t)n);
    for (int64_t k = 0; k < n; ++k) r.rank[(size_t)r.order[(size_t)k]] = k;
    const auto width = [&](int64_t row) { const int64_t len = r.lens[(size_t)r.order[(size_t)row]]; return len == 0 ? int64_t(0) : (M == 0 ? L : std::min<int64_t>(L, (len + M - 1) / M * M)); };
    r.boffs.push_back(0);
    r.brows.push_back(0);
    for (int64_t s = 0; s < n;) {
        int64_t e = s + 1;
        while (e < n && e + 1 - s <= B && (e + 1 - s) * width(order == TKZ_BUCKET_ASCENDING ? e : s) <= T) ++e;
        const int64_t W = width(order == TKZ_BUCKET_ASCENDING ? e - 1 : s);
        for (int64_t k = s; k < e; ++k) {
            const int64_t d = r.order[(size_t)k], len = r.lens[(size_t)d], kept = len - f, src = cut == TKZ_TRIM_SUFFIX ? O[(size_t)d] : O[(size_t)d + 1] - kept;
            const int64_t s0 = side == TKZ_PAD_LEFT ? W - len : 0;
            for (int64_t c = 0; c < W; ++c) {
                const int64_t j = c - s0;
                const bool in = j >= 0 && j < len;
                r.ids.push_back(!in ? pad : fb && j == 0 ? bos : (fe && j == len - 1 ? eos : ids[(size_t)(src + j - fb)]));
                r.pos.push_back(in ? (int32_t)j : 0);
                r.mask.push_back(in ? 1 : 0);
            }
        }
        r.widths.push_back((int32_t)W);
        r.boffs.push_back((int64_t)r.ids.size());
        r.brows.push_back(e);
        s = e;
    }
    r.P = (int64_t)r.ids.size();
    r.nb = (int64_t)r.widths.size();
    return r;
}

// the device entry (the emulated build's device memory is host memory) with buffers of exactly P, n_docs, n_docs + 1, n_buckets and n_buckets + 1 entries; without
// the optional arrays; one entry short of either capacity; the host entry
static bool check_batch(tkz_encoder* e, const Batch& b, int64_t L, int64_t T, int64_t B, int order, int32_t bos, int32_t eos, int cut, int side, int64_t M) {
    const int64_t n = (int64_t)b.offs.size() - 1, total = b.offs.back();
    void* aligned = nullptr;                                                     // (d_bytes: 16-byte aligned)
    if (tkz_host_alloc((size_t)total + 64, &aligned) != TKZ_OK) return false;
    std::memset(aligned, 0, (size_t)total + 64);
    if (total) std::memcpy(aligned, b.bytes.data(), (size_t)total);
    const uint8_t* d = static_cast<const uint8_t*>(aligned);
    std::vector<int32_t> want_ids((size_t)total + 1);
    std::vector<int64_t> want((size_t)n + 1, 0);
    int64_t tw = 0;
    bool ok = n == 0 || tkz_encode_batch_device(e, d, b.offs.data(), n, total, want_ids.data(), total, want.data(), nullptr, &tw) == TKZ_OK;
    if (!ok) { tkz_host_free(aligned); return false; }
    const Rows R = rule(want_ids, want, L, T, B, order, bos, eos, -3, cut, side, M);
    const int64_t cap = R.P, nb = R.nb;
    // (exactly sized heap blocks, never an empty vector's null data(): a required pointer)
    std::vector<int32_t> ids((size_t)cap), pos((size_t)cap), lens((size_t)n), widths((size_t)nb);
    std::vector<uint8_t> mask((size_t)cap);
    std::vector<int64_t> offs((size_t)n + 1), perm((size_t)n), rank((size_t)n), boffs((size_t)nb + 1), brows((size_t)nb + 1);
    const auto reset = [&] {
        std::fill(ids.begin(), ids.end(), -9); std::fill(pos.begin(), pos.end(), -9); std::fill(lens.begin(), lens.end(), -9); std::fill(widths.begin(), widths.end(), -9);
        std::fill(mask.begin(), mask.end(), 9); std::fill(offs.begin(), offs.end(), -9); std::fill(perm.begin(), perm.end(), -9); std::fill(rank.begin(), rank.end(), -9);
        std::fill(boffs.begin(), boffs.end(), -9); std::fill(brows.begin(), brows.end(), -9);
    };
    int32_t none = 0; int64_t none64 = 0;
    int32_t* const pi = cap ? ids.data() : &none; int32_t* const pl = n ? lens.data() : &none; int32_t* const pw = nb ? widths.data() : &none;
    int64_t* const po = n ? perm.data() : &none64;
    int64_t Tt = -1, P = -1, C = -1, NB = -1;
    reset();
    ok = tkz_encode_batch_budgeted_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, cut, side, -3, M, T, B, order, pi, cap, mask.data(), pos.data(), pl, offs.data(), po,
                                          rank.data(), boffs.data(), brows.data(), pw, nb, nullptr, &Tt, &P, &C, &NB) == TKZ_OK;
    ok = ok && Tt == R.total && P == R.P && C == R.n_cut && NB == R.nb && ids == R.ids && pos == R.pos && mask == R.mask && lens == R.lens && offs == want && perm == R.order &&
         rank == R.rank && boffs == R.boffs && brows == R.brows && widths == R.widths;
    reset();
    ok = ok && tkz_encode_batch_budgeted_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, cut, side, -3, M, T, B, order, pi, cap, nullptr, nullptr, pl, nullptr, po, nullptr,
                                                boffs.data(), brows.data(), pw, nb, nullptr, &Tt, &P, &C, &NB) == TKZ_OK;
    ok = ok && ids == R.ids && lens == R.lens && perm == R.order && boffs == R.boffs && brows == R.brows && widths == R.widths && P == R.P && NB == R.nb;
    if (ok && cap > 0) {
        Tt = P = C = NB = -2;
        ok = tkz_encode_batch_budgeted_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, cut, side, -3, M, T, B, order, pi, cap - 1, mask.data(), pos.data(), pl, offs.data(),
                                              po, rank.data(), boffs.data(), brows.data(), pw, nb, nullptr, &Tt, &P, &C, &NB) == TKZ_E_CAPACITY;
        ok = ok && Tt == R.total && P == R.P && C == R.n_cut && NB == R.nb;
    }
    if (ok && nb > 0) {
        Tt = P = C = NB = -2;
        ok = tkz_encode_batch_budgeted_device(e, d, b.offs.data(), n, total, nullptr, 0, bos, eos, L, cut, side, -3, M, T, B, order, pi, cap, mask.data(), pos.data(), pl, offs.data(),
                                              po, rank.data(), boffs.data(), brows.data(), pw, nb - 1, nullptr, &Tt, &P, &C, &NB) == TKZ_E_CAPACITY;
        ok = ok && Tt == R.total && P == R.P && C == R.n_cut && NB == R.nb;
    }
    reset();
    ok = ok && tkz_encode_batch_budgeted_utf8(e, d, b.offs.data(), n, nullptr, 0, bos, eos, L, cut, side, -3, M, T, B, order, pi, cap, mask.data(), pos.data(), pl, offs.data(), po,
                                              rank.data(), boffs.data(), brows.data(), pw, nb, &Tt, &P, &C, &NB) == TKZ_OK;
    ok = ok && Tt == R.total && P == R.P && C == R.n_cut && NB == R.nb && ids == R.ids && pos == R.pos && mask == R.mask && lens == R.lens && offs == want && perm == R.order &&
         rank == R.rank && boffs == R.boffs && brows == R.brows && widths == R.widths;
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
    const int32_t forms[4][2] = {{-1, -1}, {7, -1}, {-1, 9}, {7, 9}};
    for (int round = 0; round < 2; ++round) {
        {   // the worked examples; the framing forms over both orders, cut sides and pad sides; empty batches
            Batch ex; for (int64_t n : {5, 0, 2, 3, 2}) ex.add(words(n));
            Batch empties; for (int k = 0; k < 75; ++k) empties.add("");
            Batch none;
            for (int order = 0; order < 2; ++order) {
                REQUIRE(check_batch(e, ex, 4, 9, BMAX, order, -1, 9, 0, 0, 1) && check_batch(e, ex, 4, 9, 2, order, -1, 9, 0, 0, 1));
                for (const auto& fr : forms) for (int cut = 0; cut < 2; ++cut) for (int side = 0; side < 2; ++side) {
                    REQUIRE(check_batch(e, ex, 4, 4 + 3 * side + cut, cut ? BMAX : 2, order, fr[0], fr[1], cut, side, side ? 0 : 3));
                    REQUIRE(check_batch(e, empties, 6, 30, cut ? BMAX : 20, order, fr[0], fr[1], cut, side, cut ? 0 : 8));
                }
                REQUIRE(check_batch(e, none, 3, 3, 2, order, 7, 9, 0, 0, 1) && check_batch(e, none, 3, TMAX, BMAX, order, -1, -1, 0, 0, 1));
            }
        }
        {   // one run, a row a bucket; M == 0; only B binds; documents around the sort's and the marking tile
            Batch same; const std::string doc = words(3); for (int64_t d = 0; d < 2 * K + 1; ++d) same.add(doc);
            REQUIRE(check_batch(e, same, 4, 4, BMAX, round, -1, 9, 0, 0, 1) && check_batch(e, same, 5, 15, BMAX, 1 - round, -1, 9, 0, 1, 0));
            Batch b; for (int64_t d = 0; d < 150; ++d) b.add(words((11 * d + d / 7) % 40));
            for (int order = 0; order < 2; ++order)
                for (int64_t B : {int64_t(1), int64_t(64), int64_t(149), int64_t(150), int64_t(151)}) REQUIRE(check_batch(e, b, 30, 150 * 30, B, order, 7, 9, order, order, 8));
            for (int64_t n : {KM - 1, KM, KM + 1, K - 1, K, K + 1}) {
                Batch t; for (int64_t d = 0; d < n; ++d) t.add(words((7 * d + d / 5) % 6));
                REQUIRE(check_batch(e, t, 6, 50, 11, round, -1, 9, 0, 0, 1));
            }
        }
        {   // runs: buckets that swallow runs, entries that jump over them, both bounds binding; width 0 leading and trailing; 1 .. 129 runs
            Batch b;
            for (int64_t n : {1, 1, 2, 2, 3, 3, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 5, 5, 6, 6, 6, 7, 7, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10, 10}) b.add(words(n));
            Batch jump; for (int64_t n : {10, 10, 9, 8}) jump.add(words(n));
            for (int k = 0; k < 30; ++k) jump.add(words(7));
            for (int64_t n : {3, 3, 3, 3, 0, 0, 0}) jump.add(words(n));
            Batch z; for (int64_t n : {2, 0, 0, 1, 0, 0, 0, 4, 0}) z.add(words(n));
            for (int order = 0; order < 2; ++order) {
                REQUIRE(check_batch(e, b, 10, 40, 7, order, -1, -1, 0, 0, 1) && check_batch(e, b, 10, 60, BMAX, order, 7, -1, 1, 1, 1) && check_batch(e, b, 10, 12, BMAX, order, -1, -1, 0, 0, 4));
                REQUIRE(check_batch(e, jump, 10, 40, BMAX, order, -1, -1, 0, 0, 1) && check_batch(e, jump, 10, 25, 6, order, -1, -1, 0, 1, 2));
                REQUIRE(check_batch(e, z, 8, 8, 4, order, -1, -1, 0, 0, 1) && check_batch(e, z, 8, 8, BMAX, order, -1, -1, 0, 1, 1) && check_batch(e, z, 8, 9, 2, order, -1, -1, 0, 0, 0));
            }
            for (int64_t nruns : {1, 63, 64, 65, 129}) {
                Batch t; for (int64_t k = 0; k < nruns; ++k) t.add(words(1 + (k * 37) % nruns));      // (37 is prime to every count: every length once)
                t.add(words(nruns)); t.add(words(1));
                const int64_t L = 131;
                for (int order = 0; order < 2; ++order)
                    REQUIRE(check_batch(e, t, L, L, BMAX, order, -1, 9, 0, 0, 1) && check_batch(e, t, L, 3 * L, 5, order, -1, 9, 0, 0, 1) &&
                            check_batch(e, t, L, (nruns + 2) * L, BMAX, order, -1, 9, 0, 0, 1));
            }
        }
        {   // random small batches
            for (int k = 0; k < 40; ++k) {
                const int64_t L = 1 + rnd(16), n = 1 + rnd(60), M = k % 3 == 0 ? 0 : (k % 3 == 1 ? 1 : 8), T = L + rnd((uint32_t)(9 * L + 1)), B = rnd(3) ? BMAX : 1 + rnd(7);
                Batch t; for (int64_t d = 0; d < n; ++d) t.add(words(rnd(5) ? rnd((uint32_t)L + 4) : 0));
                const int form = L >= 2 ? (int)rnd(4) : (int)rnd(3);
                REQUIRE(check_batch(e, t, L, T, B, k & 1, forms[form][0], forms[form][1], (k >> 1) & 1, (k >> 2) & 1, M));
            }
        }
        {   // a literal allowed and not: against the special entry's ids
            const std::string text = words(2) + eot + words(3);
            const std::string tail = words(3) + eot;
            const std::string both = text + tail;
            const int64_t offs[4] = {0, (int64_t)text.size(), (int64_t)both.size(), (int64_t)both.size()};
            const uint8_t* t = reinterpret_cast<const uint8_t*>(both.data());
            for (int with = 0; with < 2; ++with) {
                std::vector<int32_t> want((size_t)both.size());
                std::vector<int64_t> wo(4);
                int64_t need = 0;
                REQUIRE(tkz_encode_batch_special_utf8(e, t, offs, 3, allow, with, want.data(), (int64_t)want.size(), wo.data(), &need) == TKZ_OK);
                for (int64_t L : {int64_t(3), int64_t(4), int64_t(5), int64_t(8)}) for (int order = 0; order < 2; ++order) {
                    const Rows R = rule(want, wo, L, 2 * L, BMAX, order, -1, 50256, 0, order, order, 1);
                    std::vector<int32_t> ids(R.ids.size()), pos(R.ids.size()), lens(3), widths((size_t)R.nb);
                    std::vector<uint8_t> mask(R.ids.size());
                    std::vector<int64_t> oo(4), perm(3), rank(3), boffs((size_t)R.nb + 1), brows((size_t)R.nb + 1);
                    int64_t T = 0, P = 0, C = 0, NB = 0;
                    REQUIRE(tkz_encode_batch_budgeted_utf8(e, t, offs, 3, allow, with, -1, 50256, L, order, order, 0, 1, 2 * L, BMAX, order, ids.data(), (int64_t)ids.size(), mask.data(),
                                                           pos.data(), lens.data(), oo.data(), perm.data(), rank.data(), boffs.data(), brows.data(), widths.data(), R.nb, &T, &P, &C, &NB) == TKZ_OK);
                    REQUIRE(T == R.total && P == R.P && C == R.n_cut && NB == R.nb && ids == R.ids && pos == R.pos && mask == R.mask && lens == R.lens && oo == wo && perm == R.order &&
                            rank == R.rank && boffs == R.boffs && brows == R.brows && widths == R.widths);
                }
            }
        }
        {   // the UTF-16 entry: a lone surrogate, a pair cut by a document boundary, a literal; no units at all
            std::vector<uint16_t> u; std::vector<int64_t> uo{0};
            auto add = [&](const std::u16string& s) { u.insert(u.end(), s.begin(), s.end()); uo.push_back((int64_t)u.size()); };
            add(u"plain text"); add(u"lone \xD800 high zqxjkvb"); add(u"cut \xD83D"); add(u"\xDE00 here"); add(u""); add(u"a <|endoftext|> b \xD83D\xDE00\x6F22");
            const int64_t n = (int64_t)uo.size() - 1;
            std::vector<int32_t> want(u.size() * 3 + 1);
            std::vector<int64_t> wo((size_t)n + 1);
            int64_t need = 0, T = 0, P = 0, C = 0, NB = 0;
            REQUIRE(tkz_encode_batch_special_utf16(e, u.data(), uo.data(), n, allow, 1, want.data(), (int64_t)want.size(), wo.data(), &need) == TKZ_OK);
            const Rows R = rule(want, wo, 6, 16, 4, TKZ_BUCKET_DESCENDING, 7, 9, -1, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, 4);
            std::vector<int32_t> ids(R.ids.size()), pos(R.ids.size()), lens((size_t)n), widths((size_t)R.nb);
            std::vector<uint8_t> mask(R.ids.size());
            std::vector<int64_t> oo((size_t)n + 1), perm((size_t)n), rank((size_t)n), boffs((size_t)R.nb + 1), brows((size_t)R.nb + 1);
            REQUIRE(tkz_encode_batch_budgeted_utf16(e, u.data(), uo.data(), n, allow, 1, 7, 9, 6, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, -1, 4, 16, 4, TKZ_BUCKET_DESCENDING, ids.data(),
                                                    (int64_t)ids.size() - 1, mask.data(), pos.data(), lens.data(), oo.data(), perm.data(), rank.data(), boffs.data(), brows.data(),
                                                    widths.data(), R.nb, &T, &P, &C, &NB) == TKZ_E_CAPACITY);
            REQUIRE(T == R.total && P == R.P && C == R.n_cut && NB == R.nb);
            REQUIRE(tkz_encode_batch_budgeted_utf16(e, u.data(), uo.data(), n, allow, 1, 7, 9, 6, TKZ_TRIM_PREFIX, TKZ_PAD_LEFT, -1, 4, 16, 4, TKZ_BUCKET_DESCENDING, ids.data(), P,
                                                    mask.data(), pos.data(), lens.data(), oo.data(), perm.data(), rank.data(), boffs.data(), brows.data(), widths.data(), NB, &T, &P, &C,
                                                    &NB) == TKZ_OK);
            REQUIRE(ids == R.ids && pos == R.pos && mask == R.mask && lens == R.lens && oo == wo && perm == R.order && rank == R.rank && boffs == R.boffs && brows == R.brows &&
                    widths == R.widths);
            const int64_t z[4] = {0, 0, 0, 0}; int32_t zi[12]; int32_t zp[12]; uint8_t zm[12]; int32_t zl[3]; int64_t zo[4], zr[3], zk[3], zb[3], zs[3]; int32_t zw[2];
            REQUIRE(tkz_encode_batch_budgeted_utf16(e, nullptr, z, 3, nullptr, 0, 7, 9, 4, 0, 0, 5, 3, 6, BMAX, 0, zi, 12, zm, zp, zl, zo, zr, zk, zb, zs, zw, 2, &T, &P, &C, &NB) == TKZ_OK &&
                    T == 0 && P == 9 && C == 0 && NB == 2);
            REQUIRE(zi[0] == 7 && zi[1] == 9 && zi[2] == 5 && zi[8] == 5 && zm[1] == 1 && zm[2] == 0 && zp[1] == 1 && zl[2] == 2 && zo[3] == 0 && zr[2] == 2 && zk[1] == 1 && zb[1] == 6 &&
                    zb[2] == 9 && zs[1] == 2 && zs[2] == 3 && zw[0] == 3 && zw[1] == 3);
        }
        {   // the argument rows
            const uint8_t t[5] = {'h', 'e', 0xFF, 'l', 'o'}; const int64_t o1[2] = {0, 2}, o2[2] = {0, 5}; int64_t oo[2], T = 7, P = 7, C = 7, NB = 7, perm[1], rank[1], boffs[2], brows[2];
            int32_t ids[8], pos[8], lens[1], widths[1]; uint8_t mask[8];
#define CALL(e_, bos_, eos_, L_, T_, B_, order_, ids_, lens_, perm_, boffs_, brows_, widths_, bcap_, P_, NB_) \
    tkz_encode_batch_budgeted_utf8(e_, t, o1, 1, nullptr, 0, bos_, eos_, L_, 0, 0, 0, 1, T_, B_, order_, ids_, 8, mask, pos, lens_, oo, perm_, rank, boffs_, brows_, widths_, bcap_, &T, P_, &C, NB_)
            REQUIRE(CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_OK && P == lens[0] && widths[0] == lens[0] && boffs[1] == P && brows[1] == 1 && NB == 1);
            REQUIRE(CALL(nullptr, -1, 9, 4, 4, 1, 0, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG);
            REQUIRE(CALL(e, -2, 9, 4, 4, 1, 0, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG && CALL(e, -1, 9, 0, 4, 1, 0, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG);
            REQUIRE(CALL(e, -1, 9, 4, 3, 1, 0, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG && CALL(e, -1, 9, 4, TMAX + 1, 1, 0, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG);
            REQUIRE(CALL(e, -1, 9, 4, TMAX, BMAX, 1, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_OK);
            REQUIRE(CALL(e, -1, 9, 4, 4, 0, 0, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG && CALL(e, -1, 9, 4, 4, BMAX + 1, 0, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG);
            REQUIRE(CALL(e, -1, 9, 4, 4, 1, 2, ids, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG && CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, perm, boffs, brows, widths, -1, &P, &NB) == TKZ_E_ARG);
            REQUIRE(CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, perm, boffs, brows, widths, 0, &P, &NB) == TKZ_E_CAPACITY && NB == 1 && P == lens[0]);
            REQUIRE(CALL(e, -1, 9, 4, 4, 1, 0, nullptr, lens, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG && CALL(e, -1, 9, 4, 4, 1, 0, ids, nullptr, perm, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG);
            REQUIRE(CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, nullptr, boffs, brows, widths, 1, &P, &NB) == TKZ_E_ARG && CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, perm, nullptr, brows, widths, 1, &P, &NB) == TKZ_E_ARG);
            REQUIRE(CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, perm, boffs, nullptr, widths, 1, &P, &NB) == TKZ_E_ARG && CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, perm, boffs, brows, nullptr, 1, &P, &NB) == TKZ_E_ARG);
            REQUIRE(CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, perm, boffs, brows, widths, 1, nullptr, &NB) == TKZ_E_ARG && CALL(e, -1, 9, 4, 4, 1, 0, ids, lens, perm, boffs, brows, widths, 1, &P, nullptr) == TKZ_E_ARG);
#undef CALL
            REQUIRE(tkz_encode_batch_budgeted_utf8(e, t, o1, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, 4, 1, 0, ids, 8, nullptr, nullptr, lens, nullptr, perm, nullptr, boffs, brows, widths, 1, &T, &P, &C, &NB) == TKZ_OK);
            REQUIRE(tkz_encode_batch_budgeted_device(e, t, o1, 1, 2, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, 4, 1, 0, ids, 8, mask, pos, lens, oo, perm, rank, boffs, brows, widths, 1, nullptr, nullptr, &P, &C, &NB) == TKZ_E_ARG);
            const int32_t bad[1] = {1};
            REQUIRE(tkz_encode_batch_budgeted_utf8(e, t, o1, 1, bad, 1, -1, 9, 4, 0, 0, 0, 1, 4, 1, 0, ids, 8, mask, pos, lens, oo, perm, rank, boffs, brows, widths, 1, &T, &P, &C, &NB) == TKZ_E_ARG);
            REQUIRE(tkz_encode_batch_budgeted_utf8(e, t, o2, 1, nullptr, 0, -1, 9, 4, 0, 0, 0, 1, 4, 1, 0, ids, 8, mask, pos, lens, oo, perm, rank, boffs, brows, widths, 1, &T, &P, &C, &NB) == TKZ_E_INVALID_UTF8);
        }
    }
    int64_t calls = 0;
    tkz_encoder_budgeted_calls(e, &calls);
    REQUIRE(calls > 100);
    tkz_encoder_destroy(e);
    tkz_vocab_destroy(v);
    std::printf("sanitize budgeted ok (%lld budgeted calls)\n", (long long)calls);
    return 0;
}
