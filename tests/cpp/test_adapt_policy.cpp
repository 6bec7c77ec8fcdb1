// The promotion / adaptation policy (tokenizer_amd/csrc/tkz_adapt.h) and the choice of what to promote (tkz_promo_select.h), driven without a kernel:
// scripted (bytes, misses, pieces) sequences at the production thresholds (TKZ_ADAPT_* unset), every rule DESIGN.md 6 and the headers' comments state.
//   g++ -std=c++17 -DTKZ_HOSTEMU -I tests/hostemu -I tokenizer_amd/csrc tests/cpp/test_adapt_policy.cpp
#include <cstdio>
#include <string>

#include "tkz_adapt.h"
#include "tkz_promo_select.h"

using tkz::AdaptPolicy;
using Arm = AdaptPolicy::Arm;
using After = AdaptPolicy::After;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failed; fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); } } while (0)

constexpr int64_t MB = int64_t(1) << 20, GB = int64_t(1) << 30;
constexpr int64_t kMinBytes = 8 * MB, kSettle = 64 * MB, kRound = GB, kMinSettled = 256 * MB;      // the defaults of tkz_adapt.h
constexpr size_t kCap = 65536;

// what tkz_api.cpp does around the policy, without the device: arm_learning, after_batch, promote_or_drop
struct Sim {
    AdaptPolicy p;
    size_t n_promoted = 0;
    bool ws_learning = false, opened = false;
    int64_t seen = 0;                                  // the test's own count of the bytes fed
    uint64_t gen = 0;                                  // the generation of the tables the batch in hand took its copy of (arm_learning)
    Arm arm(int64_t total, bool others = false) {
        const Arm a = p.may_learn(total, true, true, true, true, n_promoted, others);
        gen = p.generation();
        if (a != Arm::No) { opened = p.window_armed(a == Arm::YesClearMemo); ws_learning = true; }
        return a;
    }
    After end(int64_t total, double misses, double pieces) {
        const After w = p.batch_ended(total, misses, pieces, ws_learning, n_promoted, gen);
        ws_learning = false; seen += total;
        return w;
    }
    // a batch that was enqueued when the tables were at generation `enqueued_on` (the pipelined host path: two launch sequences ahead) and ends now
    After late(int64_t total, double misses, double pieces, uint64_t enqueued_on) {
        const After w = p.batch_ended(total, misses, pieces, false, n_promoted, enqueued_on);
        seen += total;
        return w;
    }
    After batch(int64_t total, double misses, double pieces) { arm(total); return end(total, misses, pieces); }
    After quiet(int64_t total) { return batch(total, 0, 0); }      // (no pieces: the miss share is not followed, only the bytes count)
    void quiet_until(int64_t at) { while (seen < at) { const bool was = ws_learning; CHECK(quiet(at - seen) == After::Nothing && !was); } }
    void install(int64_t added) { if (added) p.tables_replaced(); p.promotion_installed(added, n_promoted); n_promoted += (size_t)added; }      // (install_key_tables, promote_or_drop)
    void drop() { if (n_promoted) p.tables_replaced(); p.promotions_dropped(); n_promoted = 0; }
    bool stats_are(int64_t promotions, int64_t relearns, int64_t base, int64_t ew, int64_t since_install, int64_t window) {
        int64_t s[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
        p.stats(s);
        const bool ok = s[0] == promotions && s[1] == relearns && s[2] == -7 && s[3] == -7 && s[4] == base && s[5] == ew && s[6] == since_install && s[7] == window;
        if (!ok) fprintf(stderr, "  stats: %lld %lld . . %lld %lld %lld %lld\n", (long long)s[0], (long long)s[1], (long long)s[4], (long long)s[5], (long long)s[6], (long long)s[7]);
        return ok;
    }
};

static void first_window_adapt_on() {
    Sim s;
    CHECK(s.stats_are(0, 0, -1, -1, 0, 0));
    // small batches add up to promo_min_bytes; the first eligible batch opens the window
    for (int k = 1; k <= 7; ++k) {
        CHECK(s.arm(MB) == Arm::Yes && s.opened == (k == 1));
        CHECK(s.end(MB, 100, 1000) == After::WindowContinues);
        CHECK(s.stats_are(0, 0, -1, -1, k * MB, k * MB));       // (a learning batch does not move the miss share's average)
    }
    CHECK(s.arm(MB) == Arm::Yes && !s.opened);
    CHECK(s.end(MB, 100, 1000) == After::Promote);
    CHECK(s.stats_are(0, 0, -1, -1, 8 * MB, 0));
    CHECK(s.arm(MB) == Arm::No);                                 // the slot stays taken while the promotion is built
    s.install(1000);
    CHECK(s.stats_are(1, 0, -1, -1, 0, 0));
    // one batch of the window's size is a window
    Sim t;
    CHECK(t.batch(kMinBytes, 1, 10) == After::Promote);
    Sim u;
    CHECK(u.batch(kMinBytes - 1, 1, 10) == After::WindowContinues && u.batch(1, 0, 0) == After::Promote);
}

static void first_window_adapt_off() {
    Sim s;
    s.p.set_adapt(0);
    CHECK(s.arm(kMinBytes - 1) == Arm::No);                     // only a batch of at least promo_min_bytes learns
    CHECK(s.end(kMinBytes - 1, 500, 1000) == After::Nothing);
    CHECK(s.stats_are(0, 0, -1, -1, kMinBytes - 1, 0));         // (and the miss share is not followed)
    CHECK(s.arm(kMinBytes) == Arm::Yes && s.opened);
    CHECK(s.end(kMinBytes, 500, 1000) == After::Promote);
    s.install(1000);
    const int64_t opened_at = kMinBytes - 1;
    s.quiet_until(opened_at + kRound - 1);
    CHECK(s.arm(kMinBytes) == Arm::No);
    CHECK(s.end(1, 0, 0) == After::Nothing);
    CHECK(s.arm(kMinBytes - 1) == Arm::No);
    CHECK(s.arm(kMinBytes) == Arm::Yes && s.opened);            // the second round, kPromoSecondBytes after the first window began
    CHECK(s.end(kMinBytes, 900, 1000) == After::Promote);      // (no drift rule without TKZ_OPT_ADAPT)
    s.install(1000);
    CHECK(s.stats_are(2, 0, -1, -1, 0, 0));
    s.quiet_until(64 * GB);
    CHECK(s.arm(kMinBytes) == Arm::No);                         // at most kPromoAutoRounds rounds
    Sim t;
    t.p.set_adapt(0); t.p.set_min_bytes(MB);                     // TKZ_OPT_PROMOTE_MIN_BYTES
    CHECK(t.arm(MB - 1) == Arm::No && t.arm(MB) == Arm::Yes);
}

static void round_spacing() {
    Sim s;
    CHECK(s.batch(kMinBytes, 0, 0) == After::Promote);           // the first window opened at byte 0
    s.install(1000);
    // round r + 1 follows the START of round r's window by adapt_round_bytes << min(r - 1, 20)
    int64_t opened_at = 0;
    for (int r = 1; r <= 23; ++r) {
        const int64_t next = opened_at + (kRound << (r - 1 < 20 ? r - 1 : 20));
        s.quiet_until(next - 1);
        CHECK(s.arm(kMinBytes) == Arm::No);
        CHECK(s.end(1, 0, 0) == After::Nothing);
        CHECK(s.arm(kMinBytes) == Arm::Yes && s.opened);
        CHECK(s.end(kMinBytes, 0, 0) == After::Promote);
        s.install(1);                                            // (little: not more than a tenth of what the list held)
        CHECK(s.stats_are(r + 1, 0, -1, -1, 0, 0));
        opened_at = next;
    }
    // back to the 1x gap when a round added MORE than a tenth of what the list held
    Sim t;
    CHECK(t.batch(kMinBytes, 0, 0) == After::Promote);
    t.install(1000);
    t.quiet_until(kRound);
    CHECK(t.batch(kMinBytes, 0, 0) == After::Promote);           // opened at 1 GB
    t.install(100);                                              // exactly a tenth: the gaps go on doubling
    t.quiet_until(3 * GB - 1);
    CHECK(t.arm(kMinBytes) == Arm::No);
    CHECK(t.end(1, 0, 0) == After::Nothing);
    CHECK(t.batch(kMinBytes, 0, 0) == After::Promote);           // opened at 3 GB
    t.install(111);                                              // 1110 > 1100
    t.quiet_until(4 * GB - 1);
    CHECK(t.arm(kMinBytes) == Arm::No);
    CHECK(t.end(1, 0, 0) == After::Nothing);
    CHECK(t.arm(kMinBytes) == Arm::Yes && t.opened);             // 1 GB after 3 GB, not 4 GB after it
}

static void no_window() {
    Sim s;
    const AdaptPolicy& p = s.p;
    CHECK(p.may_learn(MB, true, true, true, true, 0, false) == Arm::Yes);
    CHECK(p.may_learn(MB, false, true, true, true, 0, false) == Arm::No);       // a retry of the batch
    CHECK(p.may_learn(MB, true, false, true, true, 0, false) == Arm::No);       // not a batch of documents
    CHECK(p.may_learn(MB, true, true, false, true, 0, false) == Arm::No);       // the memo is off
    CHECK(p.may_learn(MB, true, true, true, false, 0, false) == Arm::No);       // a promo code would look like a rank
    CHECK(p.may_learn(MB, true, true, true, true, kCap - 1, false) == Arm::Yes);
    CHECK(p.may_learn(MB, true, true, true, true, kCap, false) == Arm::No);     // the list is at its cap
    CHECK(p.may_learn(MB, true, true, true, true, 0, true) == Arm::Yes);        // (other calls only matter when the memo is to be emptied)
    s.p.set_cap(10);                                                             // TKZ_OPT_PROMOTE_CAP
    CHECK(s.p.cap() == 10 && p.may_learn(MB, true, true, true, true, 9, false) == Arm::Yes && p.may_learn(MB, true, true, true, true, 10, false) == Arm::No);
    s.p.set_cap(kCap);
    s.p.set_mode(0);                                                             // TKZ_OPT_PROMOTE 0
    CHECK(s.p.mode() == 0 && s.arm(MB) == Arm::No);
    CHECK(s.end(MB, 500, 1000) == After::Nothing);
    CHECK(s.stats_are(0, 0, -1, -1, MB, 0));                                     // (and the miss share is not followed)
    s.p.set_mode(1);
    CHECK(s.arm(MB) == Arm::Yes && s.opened);
    CHECK(s.arm(MB) == Arm::No);                                                 // the slot is taken
    // a learning batch that ends abnormally gives the slot back; the window it opened stays open
    s.p.learning_abandoned();
    CHECK(s.arm(MB) == Arm::Yes && s.opened);
    CHECK(s.end(MB, 1, 10) == After::WindowContinues);
    // a batch of another call that ends while the slot is taken decides nothing
    CHECK(s.arm(MB) == Arm::Yes && !s.opened);
    CHECK(s.p.batch_ended(GB, 900, 1000, false, 0, s.p.generation()) == After::Nothing);
}

// one window with the miss share `share`, installed; then `steady`-share batches of settle_bytes each
static Sim settled(double window_share, int64_t added) {
    Sim s;
    CHECK(s.batch(kMinBytes, window_share * 1000, 1000) == After::Promote);
    s.install(added);
    return s;
}

static void settle_and_drift() {
    {   // settling: the level is taken settle_bytes after the install, from the average of the batches since
        Sim s = settled(0.25, 1000);
        for (int k = 1; k <= 3; ++k) {
            CHECK(s.batch(16 * MB, 125, 1000) == After::Nothing);
            CHECK(s.stats_are(1, 0, -1, 125000, k * 16 * MB, 0));
        }
        CHECK(s.batch(16 * MB, 125, 1000) == After::Nothing);
        CHECK(s.stats_are(1, 0, 125000, 125000, 64 * MB, 0));
        // the average moves by total / settle_bytes of the distance: 0.125 -> 0.625 by a quarter
        CHECK(s.batch(16 * MB, 625, 1000) == After::Nothing);
        CHECK(s.stats_are(1, 0, 125000, 250000, 80 * MB, 0));
        // nothing within adapt_min_bytes of the install, whatever the share does ...
        for (int k = 6; k <= 15; ++k) CHECK(s.batch(16 * MB, 625, 1000) == After::Nothing);
        // ... then: relearn (the slot is taken until the promotions are dropped; the next window needs the memo emptied)
        CHECK(s.batch(16 * MB, 625, 1000) == After::Relearn);
        CHECK(s.arm(MB) == Arm::No);
        s.drop();
        CHECK(s.stats_are(1, 1, -1, -1, 0, 0));
        CHECK(s.arm(MB) == Arm::YesClearMemo && s.opened);
    }
    {   // the install-time drift rule: a level that settles above window * 1.25 + 0.01 (0.25 -> 0.3225) is another text
        Sim s = settled(0.25, 1000);
        CHECK(s.batch(kSettle, 322, 1000) == After::Nothing);
        CHECK(s.stats_are(1, 0, 322000, 322000, kSettle, 0));
        Sim t = settled(0.25, 1000);
        CHECK(t.batch(kSettle - 1, 323, 1000) == After::Nothing);
        CHECK(t.batch(1, 323, 1000) == After::Relearn);
        // ... asked once: the window's share is spent when the level settles
        Sim u = settled(0.25, 1000);
        CHECK(u.batch(kSettle, 125, 1000) == After::Nothing && u.batch(kSettle, 500, 1000) == After::Nothing && u.batch(kSettle, 500, 1000) == After::Nothing);
    }
    const struct { int misses; After want; } edges[] = {{166, After::Nothing}, {167, After::Relearn},      // above 0.125 * 1.25 + 0.01 = 0.16625
                                                        {84, After::Nothing}, {83, After::Relearn}};       // below 0.125 * 0.75 - 0.01 = 0.08375
    for (const auto& e : edges) {
        Sim s = settled(0.25, 1000);
        CHECK(s.batch(kSettle, 125, 1000) == After::Nothing);            // settles at 0.125
        CHECK(s.batch(kSettle, e.misses, 1000) == After::Nothing && s.batch(kSettle, e.misses, 1000) == After::Nothing);       // 128, 192 MB: too early
        CHECK(s.seen - kMinBytes == kMinSettled - kSettle);
        CHECK(s.batch(kSettle, e.misses, 1000) == e.want);
        if (e.want == After::Relearn) { s.drop(); CHECK(s.stats_are(1, 1, -1, -1, 0, 0)); }
        else CHECK(s.stats_are(1, 0, 125000, e.misses * 1000, kMinSettled, 0));
    }
}

// `n` settle-sized batches at a miss share of 0.125, none of which may ask for a re-learn; a round that comes due among them is installed with `round_adds` pieces.
// Returns the rounds that came due.
static int steady(Sim* s, int n, int64_t round_adds) {
    int rounds = 0;
    for (int k = 1; k <= n; ++k) {
        const After w = s->batch(kSettle, 125, 1000);
        CHECK(w == After::Nothing || w == After::Promote);
        if (w == After::Promote) { s->install(round_adds); ++rounds; }
    }
    return rounds;
}

// the list at 90 % of its cap
static void full_list() {
    for (const int64_t added : {int64_t(58983), int64_t(kCap)}) {      // 58983 * 10 >= 65536 * 9; and the cap itself
        // ONE window filled it: that list is the text's hot pieces as they are now.  Stationary miss share: nothing, for 20 settle-sized batches ...
        // (below the cap itself the second round comes a gigabyte after the first window began, inside these 20 batches; it adds a few pieces, and
        //  that does not make it a list the rounds have filled: the window crossed the mark)
        Sim s = settled(0.25, added);
        CHECK(steady(&s, 20, added < (int64_t)kCap ? 10 : 0) == (added < (int64_t)kCap ? 1 : 0));
        CHECK(s.stats_are(added < (int64_t)kCap ? 2 : 1, 0, 125000, 125000, added < (int64_t)kCap ? 3 * kSettle : 20 * kSettle, 0));      // (the round: the 17th batch)
        // ... and a share outside the band of a quarter and a point is a drift, as for any list: 0.125 * 1.25 + 0.01 = 0.16625, 0.125 * 0.75 - 0.01 = 0.08375
        Sim up = s, down = s, in_hi = s, in_lo = s;
        CHECK(up.batch(kSettle, 167, 1000) == After::Relearn);
        CHECK(down.batch(kSettle, 83, 1000) == After::Relearn);
        CHECK(in_hi.batch(kSettle, 166, 1000) == After::Nothing && in_lo.batch(kSettle, 84, 1000) == After::Nothing);
        up.drop();
        CHECK(up.arm(MB) == Arm::YesClearMemo);
    }
    {   // LATER rounds filled it (two installs and more that added pieces since it was last empty): it starts over, on unchanged text too ...
        Sim s = settled(0.25, 30000);
        s.quiet_until(kRound);
        CHECK(s.batch(kMinBytes, 250, 1000) == After::Promote);          // the second round, a gigabyte after the first window began
        s.install(28983);                                                // (much: the round gap goes back to 1x -- the count of rounds that FILLED the list does not)
        for (int k = 1; k <= 3; ++k) CHECK(s.batch(kSettle, 125, 1000) == After::Nothing);      // (not within adapt_min_bytes of the install)
        CHECK(s.batch(kSettle, 125, 1000) == After::Relearn);
        CHECK(s.arm(MB) == Arm::No);
        s.drop();
        CHECK(s.stats_are(2, 1, -1, -1, 0, 0));
        // ... and the window after that start-over, which fills the list on its own, does not start over again
        CHECK(s.arm(kMinBytes) == Arm::YesClearMemo && s.opened);
        CHECK(s.end(kMinBytes, 250, 1000) == After::Promote);
        s.install(58983);
        CHECK(steady(&s, 20, 10) == 1);
        CHECK(s.stats_are(4, 1, 125000, 125000, 3 * kSettle, 0));
        // one short of 90 %: later rounds or not, nothing
        Sim t = settled(0.25, 30000);
        t.quiet_until(kRound);
        CHECK(t.batch(kMinBytes, 250, 1000) == After::Promote);
        t.install(28982);
        for (int k = 1; k <= 6; ++k) CHECK(t.batch(kSettle, 125, 1000) == After::Nothing);
        // a round that added nothing has filled nothing
        Sim u = settled(0.25, 58983);
        u.quiet_until(kRound);
        CHECK(u.batch(kMinBytes, 250, 1000) == After::Promote);
        u.install(0);
        for (int k = 1; k <= 6; ++k) CHECK(u.batch(kSettle, 125, 1000) == After::Nothing);
    }
}

// batches that ran on tables older than the last install (the pipelined host path enqueues two launch sequences ahead; the install lands on a thread)
static void stale_batches() {
    {   // the issue's case: settled at 0.25, an install, two batches still on the old tables at 0.25, then the new tables' 0.125
        Sim s = settled(0.5, 1000);
        CHECK(s.batch(kSettle, 250, 1000) == After::Nothing);
        CHECK(s.stats_are(1, 0, 250000, 250000, kSettle, 0));
        s.quiet_until(kRound);
        CHECK(s.batch(kMinBytes, 250, 1000) == After::Promote);
        const uint64_t before = s.p.generation();
        s.install(50);
        CHECK(s.p.generation() == before + 1);
        for (int k = 1; k <= 2; ++k) {
            CHECK(s.late(16 * MB, 250, 1000, before) == After::Nothing);
            CHECK(s.stats_are(2, 0, -1, -1, k * 16 * MB, 0));             // their bytes count, their share enters nothing
        }
        CHECK(s.batch(16 * MB, 125, 1000) == After::Nothing);
        CHECK(s.stats_are(2, 0, -1, 125000, 48 * MB, 0));
        CHECK(s.batch(16 * MB, 125, 1000) == After::Nothing);
        CHECK(s.stats_are(2, 0, 125000, 125000, 64 * MB, 0));             // settled at 0.125, not between the two
        for (int k = 1; k <= 20; ++k) CHECK(s.batch(kSettle, 125, 1000) == After::Nothing);
        CHECK(s.stats_are(2, 0, 125000, 125000, 64 * MB + 20 * kSettle, 0));
    }
    {   // what it was without the rule (the same feed with the stale batches handed in as current ones): a level of 0.1875 that 0.125 leaves downwards
        Sim s = settled(0.5, 1000);
        s.quiet_until(kRound);
        CHECK(s.batch(kMinBytes, 250, 1000) == After::Promote);
        s.install(50);
        CHECK(s.batch(16 * MB, 250, 1000) == After::Nothing && s.batch(16 * MB, 250, 1000) == After::Nothing);
        CHECK(s.batch(16 * MB, 125, 1000) == After::Nothing && s.batch(16 * MB, 125, 1000) == After::Nothing);
        CHECK(s.stats_are(2, 0, 195312, 195312, 64 * MB, 0));            // 0.25 -> 0.21875 -> 0.1953125, and 0.1953 * 0.75 - 0.01 = 0.1365 > 0.125
        After w = After::Nothing;
        for (int k = 1; k <= 4 && w == After::Nothing; ++k) w = s.batch(kSettle, 125, 1000);
        CHECK(w == After::Relearn);
    }
    {   // a stale batch after a DROP is stale too; one of the current generation that ends while the slot is taken decides nothing but is followed
        Sim s = settled(0.25, 1000);
        const uint64_t before = s.p.generation();
        s.drop();
        CHECK(s.p.generation() == before + 1);
        CHECK(s.late(GB, 10, 1000, before) == After::Nothing);
        CHECK(s.stats_are(1, 1, -1, -1, GB, 0));
        CHECK(s.late(MB, 10, 1000, s.p.generation()) == After::Nothing);
        CHECK(s.stats_are(1, 1, -1, 10000, GB + MB, 0));
    }
}

// which workspaces of the pool are "another call in flight" for the call that asks (tkz_api.cpp: arm_learning hands the OR of these to may_learn)
static void other_calls() {
    const auto other = AdaptPolicy::other_call_in_flight;                //  (busy, the asker's own, the asker's sibling, a launch sequence in flight on it)
    CHECK(!other(false, false, false, false) && !other(false, false, false, true));      // not leased: nobody's
    CHECK(!other(true, true, false, false) && !other(true, true, false, true));          // the workspace the asking batch runs on
    CHECK(other(true, false, false, false) && other(true, false, false, true));          // leased by another call, whatever runs on it
    CHECK(!other(true, false, true, false));                                              // the asker's sibling with nothing in flight: chunk 0, before chunk 1 is begun
    CHECK(other(true, false, true, true));                                                // ... with a chunk in flight: its kernels probe the memo
}

static void window_against_last_window() {
    const struct { int misses; After want; } edges[] = {{322, After::Promote}, {323, After::Relearn}};      // 0.25 * 1.25 + 0.01 = 0.3225
    for (const auto& e : edges) {
        Sim s = settled(0.25, 1000);
        s.quiet_until(kRound);
        // the second window, in two batches: its share is that of the whole window
        CHECK(s.arm(kMinBytes / 2) == Arm::Yes && s.opened);
        CHECK(s.end(kMinBytes / 2, 0, 1000) == After::WindowContinues);
        CHECK(s.stats_are(1, 0, -1, -1, kRound - kMinBytes / 2, kMinBytes / 2));
        // an open window goes on with the next batch: the round's gap is asked of the batch that OPENS one (it was asked of every batch, counted from the
        // window's own start: a later round's window that was not complete in one batch stalled for another gap)
        CHECK(s.arm(kMinBytes / 2) == Arm::Yes && !s.opened);
        CHECK(s.end(kMinBytes / 2, 2 * e.misses, 1000) == e.want);
        CHECK(s.stats_are(1, 0, -1, -1, kRound, 0));
        if (e.want == After::Promote) continue;
        CHECK(s.arm(MB) == Arm::No);
        s.drop();
        CHECK(s.stats_are(1, 1, -1, -1, 0, 0));
        // the window after a drop has nothing to be compared with
        CHECK(s.batch(kMinBytes, 900, 1000) == After::Promote);
    }
}

// a round that added nothing replaced no table: the settled level stands (a round that comes due on the batches the text changes in must not take it away)
static void empty_round_keeps_the_level() {
    Sim s = settled(0.25, 1000);
    CHECK(s.batch(kSettle, 125, 1000) == After::Nothing);
    CHECK(s.stats_are(1, 0, 125000, 125000, kSettle, 0));
    s.quiet_until(kRound);
    CHECK(s.batch(kMinBytes, 300, 1000) == After::Promote);              // the second round's window, on other text (0.3 <= 0.25 * 1.25 + 0.01: no drift by the windows)
    const uint64_t gen = s.p.generation();
    s.install(0);                                                        // ... whose pieces the memo did not take: nothing to promote
    CHECK(s.p.generation() == gen);
    CHECK(s.stats_are(2, 0, 125000, 125000, kRound, 0));                 // the level and the distance to the last change of the tables as they were
    CHECK(s.batch(kSettle, 300, 1000) == After::Relearn);                // 0.125 -> 0.3 in one settle distance: left, and 256 MB are long past
    s.drop();
    CHECK(s.stats_are(2, 1, -1, -1, 0, 0) && s.arm(MB) == Arm::YesClearMemo);
    // with pieces added the level is taken anew, as ever
    Sim t = settled(0.25, 1000);
    CHECK(t.batch(kSettle, 125, 1000) == After::Nothing);
    t.quiet_until(kRound);
    CHECK(t.batch(kMinBytes, 300, 1000) == After::Promote);
    t.install(1);
    CHECK(t.stats_are(2, 0, -1, -1, 0, 0));
    CHECK(t.batch(kSettle, 300, 1000) == After::Nothing);
    CHECK(t.stats_are(2, 0, 300000, 300000, kSettle, 0));
}

static void memo_clear() {
    {   // a memo three quarters full is emptied before the next window
        Sim s;
        s.p.memo_read_back(3 * 1024 - 1, 4 * 1024);
        CHECK(s.p.may_learn(MB, true, true, true, true, 0, true) == Arm::Yes);
        s.p.memo_read_back(3 * 1024, 4 * 1024);
        // another call in flight: never emptied under it.  (what tkz_api.cpp hands in -- other_calls)
        CHECK(s.arm(MB, true) == Arm::No);
        CHECK(s.arm(MB, false) == Arm::YesClearMemo && s.opened);
        CHECK(s.end(MB, 1, 10) == After::WindowContinues);
        CHECK(s.arm(MB, true) == Arm::Yes && !s.opened);                 // emptied: no longer pending
        Sim off;
        off.p.set_adapt(0);
        off.p.memo_read_back(4 * 1024, 4 * 1024);                        // (only with TKZ_OPT_ADAPT)
        CHECK(off.arm(kMinBytes, true) == Arm::Yes);
    }
    {   // a pipelined host call after a drift, chunk by chunk: chunk 0 finds its sibling idle and empties the memo, chunk 1 -- chunk 0 in flight -- finds the
        // slot taken, chunk 2 continues the window (nothing to empty any more, whatever is in flight)
        const auto other = AdaptPolicy::other_call_in_flight;
        Sim s = settled(0.25, 1000);
        CHECK(s.batch(kSettle, 125, 1000) == After::Nothing);
        for (int k = 1; k <= 2; ++k) CHECK(s.batch(kSettle, 500, 1000) == After::Nothing);
        CHECK(s.batch(kSettle, 500, 1000) == After::Relearn);
        s.drop();
        CHECK(s.arm(MB, other(true, false, true, true)) == Arm::No);                      // (a chunk in flight on the sibling: not now ...)
        CHECK(s.end(MB, 500, 1000) == After::Nothing);
        CHECK(s.arm(MB, other(true, false, true, false)) == Arm::YesClearMemo && s.opened);      // (... the next call's chunk 0)
        CHECK(s.p.may_learn(MB, true, true, true, true, 0, other(true, false, true, true)) == Arm::No);      // chunk 1: the slot is taken
        CHECK(s.end(MB, 500, 1000) == After::WindowContinues);
        CHECK(s.arm(MB, other(true, false, true, true)) == Arm::Yes && !s.opened);        // chunk 2
        s.p.learning_abandoned();
        // two callers: the other call's workspaces are another call's whatever they do
        Sim t;
        t.p.memo_read_back(4, 4);
        CHECK(t.arm(MB, other(true, false, false, false)) == Arm::No);
    }
    {   // could not arm (the device side failed): nothing changed, the memo is still to be emptied
        Sim s;
        s.p.memo_read_back(4, 4);
        CHECK(s.p.may_learn(MB, true, true, true, true, 0, false) == Arm::YesClearMemo);
        CHECK(s.p.may_learn(MB, true, true, true, true, 0, false) == Arm::YesClearMemo);
        CHECK(s.stats_are(0, 0, -1, -1, 0, 0));
    }
    {   // TKZ_OPT_PROMOTE 3: the rounds start over at once, the memo keeps its entries
        Sim s = settled(0.25, 1000);
        CHECK(s.batch(kSettle, 125, 1000) == After::Nothing);
        CHECK(s.arm(MB) == Arm::No);                                     // (the second round is a gigabyte away)
        s.p.reset_by_hand(); s.n_promoted = 0;
        CHECK(s.stats_are(1, 0, -1, -1, 0, 0));
        CHECK(s.arm(MB) == Arm::Yes && s.opened);
        s.p.learning_abandoned();
        s.p.memo_read_back(4, 4);
        s.p.reset_by_hand();                                             // (nor does it take an order to empty the memo back)
        CHECK(s.arm(MB) == Arm::YesClearMemo);
    }
}

// ---- select_promotions ----------------------------------------------------------------------------------------------------------------------

static TkzMemoSlot memo_slot(const std::string& key, uint32_t cnt, uint32_t tok0) {
    TkzMemoSlot m{};
    for (size_t b = 0; b < key.size(); ++b) m.k[b >> 2] |= (uint32_t)(uint8_t)key[b] << (8 * (b & 3));
    m.v[0] = kMemoValid | ((cnt - 1u) << 29) | tok0; m.v[1] = kMemoValid | ((uint32_t)(key.size() - 1) << 27) | (tok0 + 1);
    m.v[2] = kMemoValid | (tok0 + 2); m.v[3] = kMemoValid | (tok0 + 3);
    return m;
}
static void log_record(std::vector<uint32_t>* log, const std::string& key, uint32_t cnt, uint32_t tok0) {
    uint32_t rec[tkz::kLongLogDwords] = {};
    for (size_t b = 0; b < key.size(); ++b) rec[b >> 2] |= (uint32_t)(uint8_t)key[b] << (8 * (b & 3));
    rec[7] = (uint32_t)key.size() | (cnt << 8);
    for (uint32_t t = 0; t < 4; ++t) rec[8 + t] = tok0 + t;
    log->insert(log->end(), rec, rec + tkz::kLongLogDwords);
}
struct List {
    std::vector<tkz::KeyItem> items; std::unordered_set<std::string> keys; std::vector<uint32_t> quads;
    std::string order() const { std::string s; for (const auto& it : items) s += it.key + "|"; return s; }
    bool consistent() const {
        if (quads.size() != items.size() * 4 || keys.size() != items.size()) return false;
        for (size_t i = 0; i < items.size(); ++i) if ((items[i].value & kPromoIdxMask) != i || !(items[i].value & kPromoFlag) || !keys.count(items[i].key)) return false;
        return true;
    }
};

static void selection() {
    std::vector<TkzMemoSlot> memo(8);
    memo[0] = memo_slot("alpha", 2, 100);
    memo[1] = TkzMemoSlot{};                                             // empty
    memo[2] = memo_slot("busy", 1, 200); memo[2].v[0] = kMemoBusy;       // being written
    memo[3] = memo_slot("abc", 1, 300); memo[3].k[0] &= 0x0000FFFFu;     // a zero byte inside the key's length
    memo[4] = memo_slot("beta", 4, 400);
    memo[5] = memo_slot("ab", 1, 500); memo[5].k[1] = 0x41;              // a byte beyond the key's length
    memo[6] = memo_slot("gamma", 3, 600);
    memo[7] = memo_slot("delta", 1, 700);
    const std::vector<uint32_t> hits = {5, 9, 9, 9, 7, 9, 0, 5}, no_log;
    {   // by hits, equal hits in slot order; zero-hit, invalid, busy and incomplete-key slots skipped (the last two kinds still count as valid / not)
        List l;
        const tkz::PromoSelection sel = tkz::select_promotions(memo, &hits, no_log, 100, &l.items, &l.keys, &l.quads);
        CHECK(sel.added == 3 && sel.valid_slots == 6 && l.order() == "beta|alpha|delta|" && l.consistent());
        CHECK(l.items[0].value == (kPromoFlag | (3u << kPromoCntShift) | 0u) && l.items[1].value == (kPromoFlag | (1u << kPromoCntShift) | 1u));
        CHECK(l.quads[0] == 400 && l.quads[3] == 403 && l.quads[4] == 100 && l.quads[5] == 101 && l.quads[6] == 0 && l.quads[7] == 0 && l.quads[8] == 700 && l.quads[9] == 0);
    }
    {   // without hit counters every valid entry counts alike: slot order
        List l;
        const tkz::PromoSelection sel = tkz::select_promotions(memo, nullptr, no_log, 100, &l.items, &l.keys, &l.quads);
        CHECK(sel.added == 4 && sel.valid_slots == 6 && l.order() == "alpha|beta|gamma|delta|" && l.consistent());
    }
    {   // never a key twice: one promoted before, one that sits in two slots; and the cap
        List l;
        l.items.push_back(tkz::KeyItem{"beta", kPromoFlag | 0u}); l.keys.insert("beta"); l.quads.assign(4, 0);
        std::vector<TkzMemoSlot> m2 = memo;
        m2[1] = memo_slot("alpha", 2, 100);
        tkz::PromoSelection sel = tkz::select_promotions(m2, nullptr, no_log, 100, &l.items, &l.keys, &l.quads);
        CHECK(sel.added == 3 && sel.valid_slots == 7 && l.order() == "beta|alpha|gamma|delta|" && l.consistent());
        List c;
        sel = tkz::select_promotions(memo, &hits, no_log, 2, &c.items, &c.keys, &c.quads);
        CHECK(sel.added == 2 && c.order() == "beta|alpha|" && c.consistent());
        sel = tkz::select_promotions(memo, &hits, no_log, 2, &c.items, &c.keys, &c.quads);       // a full list: nothing is looked at
        CHECK(sel.added == 0 && sel.valid_slots == 0 && c.items.size() == 2);
    }
    {   // the long-piece log: seen at least twice, by count then key, up to a quarter of the cap, ahead of the memo's entries
        const std::string k17(17, 'x'), k20 = "\n" + std::string(19, ' '), k28(28, 'y'), once(18, 'o'), known(19, 'k'), short16(16, 's'), long29(28, 'z');
        std::vector<uint32_t> log;
        for (int i = 0; i < 2; ++i) log_record(&log, k17, 2, 1000);
        for (int i = 0; i < 3; ++i) log_record(&log, k28, 4, 2000);
        for (int i = 0; i < 3; ++i) log_record(&log, k20, 1, 3000);
        log_record(&log, once, 1, 4000);
        for (int i = 0; i < 5; ++i) log_record(&log, known, 1, 5000);
        for (int i = 0; i < 5; ++i) log_record(&log, short16, 1, 6000);                  // not a long piece
        for (int i = 0; i < 5; ++i) { log_record(&log, long29, 1, 7000); log[log.size() - tkz::kLongLogDwords + 7] = 29u | (1u << 8); }      // longer than the MID table holds
        for (int i = 0; i < 5; ++i) log_record(&log, std::string(21, 'c'), 5, 8000);     // more than 4 tokens
        List l;
        l.items.push_back(tkz::KeyItem{known, kPromoFlag | 0u}); l.keys.insert(known); l.quads.assign(4, 0);
        tkz::PromoSelection sel = tkz::select_promotions(memo, &hits, log, 100, &l.items, &l.keys, &l.quads);
        CHECK(sel.added == 6 && l.order() == known + "|" + k20 + "|" + k28 + "|" + k17 + "|beta|alpha|delta|" && l.consistent());
        CHECK(l.items[2].value == (kPromoFlag | (3u << kPromoCntShift) | 2u) && l.quads[8] == 2000 && l.quads[11] == 2003 && l.quads[4] == 3000 && l.quads[5] == 0);
        List q;                                                                          // cap 8: two from the log
        sel = tkz::select_promotions(memo, &hits, log, 8, &q.items, &q.keys, &q.quads);
        CHECK(sel.added == 5 && q.order() == known + "|" + k20 + "|beta|alpha|delta|" && q.consistent());
        List r;                                                                          // ... and never past the cap itself
        r.items.assign(7, tkz::KeyItem{"", 0}); r.quads.assign(28, 0);
        sel = tkz::select_promotions(memo, &hits, log, 8, &r.items, &r.keys, &r.quads);
        CHECK(sel.added == 1 && r.items.size() == 8 && r.items[7].key == known);
    }
}

int main() {
    for (const char* v : {"TKZ_ADAPT_SETTLE_BYTES", "TKZ_ADAPT_ROUND_BYTES", "TKZ_ADAPT_MIN_BYTES"})
        if (getenv(v)) { fprintf(stderr, "%s is set: this test checks the production thresholds\n", v); return 2; }
    first_window_adapt_on();
    first_window_adapt_off();
    round_spacing();
    no_window();
    settle_and_drift();
    full_list();
    stale_batches();
    other_calls();
    window_against_last_window();
    empty_round_keeps_the_level();
    memo_clear();
    selection();
    if (g_failed) { fprintf(stderr, "%d check(s) failed\n", g_failed); return 1; }
    printf("adapt policy ok\n");
    return 0;
}
