// tkz_adapt.h -- the promotion / adaptation POLICY of an encoder (TKZ_OPT_PROMOTE, TKZ_OPT_ADAPT): when a learning window opens, when its
// hits are promoted into the key tables, when a drift makes the encoder drop everything and learn again.  Host only and standard headers only: no HIP,
// no encoder, no lock of its own (tkz_api.cpp calls every method with the encoder's mutex held) -- tests/cpp/test_adapt_policy.cpp drives it without a kernel.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace tkz {

constexpr int64_t kPromoSecondBytes = int64_t(1) << 30;      // the second learning round follows the START of the first window by this much text (then 2, 4, 8 ... times)
constexpr int kPromoAutoRounds = 2;                // without TKZ_OPT_ADAPT: the first batch of >= promo_min_bytes, and one more after kPromoSecondBytes more

// The reference's LRUCache evicts and refills for ever (LRUCache.cs:79-121); here the share of pieces that miss the key tables as a whole is followed from
// batch to batch (k_list_stats sums the miss lists: no extra kernel), and when it leaves the level it had after the last promotion the encoder LEARNS AGAIN:
// promotions dropped, memo emptied, the next batches count hits, the hottest pieces of the text as it is NOW are promoted (pieces that stopped hitting are
// simply not chosen again).
class AdaptPolicy {
public:
    enum class Arm { No, Yes, YesClearMemo };                        // YesClearMemo: the memo must be emptied before the window starts
    enum class After { Nothing, WindowContinues, Promote, Relearn };

    int mode() const { return mode_; }
    size_t cap() const { return cap_; }
    void set_mode(int v) { mode_ = v; }                              // TKZ_OPT_PROMOTE 0 / 1
    void set_adapt(int v) { adapt_ = v; }                            // TKZ_OPT_ADAPT
    void set_min_bytes(int64_t v) { min_bytes_ = v; }                // TKZ_OPT_PROMOTE_MIN_BYTES
    void set_cap(size_t v) { cap_ = v; }                             // TKZ_OPT_PROMOTE_CAP
    // {promotions, relearns, -, -, settled miss share * 1e6 or -1, recent miss share * 1e6 or -1, bytes since the last install, bytes of the open window}
    // (tkz_encoder_adapt_stats; entries 2 and 3 are the caller's)
    void stats(int64_t out8[8]) const {
        out8[0] = n_promotions_; out8[1] = n_relearns_;
        out8[4] = base_valid_ ? (int64_t)(base_miss_ * 1e6) : -1; out8[5] = ew_valid_ ? (int64_t)(ew_miss_ * 1e6) : -1;
        out8[6] = bytes_seen_ - bytes_at_install_; out8[7] = learn_bytes_;
    }

    // LEARNING: may this batch of `total` bytes open or continue a window?  The first batches of documents on the batch path (and once more,
    // kPromoSecondBytes later; and again whenever the text has drifted) count the memo's hits per slot.  A learning WINDOW is promo_min_bytes of text: one large
    // batch, or -- TKZ_OPT_ADAPT -- as many smaller ones as it takes (a caller whose batches are 1 MB learns too).
    // (TKZ_OPT_ADAPT: the rounds go on -- a gigabyte after the first window began, then two, four, eight ... gigabytes after the one before: text that
    //  changed without moving the miss share, or right behind a promotion, is still learnt, a round costs one batch that counts hits and ~50 ms of a
    //  host thread; pieces are only ever ADDED by a round -- what empties the list is a drift, or later rounds filling it to its cap: batch_ended)
    // (The gap to the next round is asked of the batch that OPENS a window.  A window that is open goes on with the next batch that may learn: asked of every
    //  batch it counted from the window's own start, so a later round's window that was not complete in one batch -- a chunk of the host pipeline smaller than
    //  the window -- stalled for another gap, and every round took two.)
    // Changes nothing: the caller readies the device side (counters, log, the memo emptied) and then calls window_armed, or -- that failed -- nothing at all.
    Arm may_learn(int64_t total, bool first_attempt, bool may_learn, bool memo_on, bool ranks_fit_promo_code, size_t n_promoted, bool other_calls_in_flight) const {
        const int64_t round_gap = round_bytes_ << std::min(std::max(rounds_ - 1, 0), 20);
        if (!(first_attempt && may_learn && mode_ == 1 && !learning_ && (adapt_ || rounds_ < kPromoAutoRounds) && memo_on && ranks_fit_promo_code &&
              (adapt_ || total >= min_bytes_) && n_promoted < cap_ && (rounds_ == 0 || learn_bytes_ > 0 || bytes_seen_ - bytes_at_promo_ >= round_gap))) return Arm::No;
        // The memo is emptied for a window that follows a drift -- it is full of the old text's pieces and takes no new ones --, and that only while
        // no OTHER call is in flight: an entry never changes once it is valid (tkz_tables.h), which is what makes a hit exact
        if (!memo_clear_pending_) return Arm::Yes;
        return other_calls_in_flight ? Arm::No : Arm::YesClearMemo;
    }
    // ... and what counts as another call in flight for the call that asks: a workspace of the pool that is leased (`busy`), unless it is the asking call's own
    // -- the one the batch runs on, or the SIBLING a pipelined host call leases for its odd chunks while that has no launch sequence in flight (so at chunk
    // 0, before chunk 1 is begun: tkz_api.cpp, HostPipeline).  With a chunk in flight on the sibling its kernels are probing the memo: never emptied then.
    static bool other_call_in_flight(bool busy, bool askers_own, bool askers_sibling, bool sequence_in_flight) {
        return busy && !askers_own && !(askers_sibling && !sequence_in_flight);
    }
    // ... it does: the learning slot is taken.  Returns whether the batch OPENS a window (the hit counters and the log start from zero)
    // (the gigabyte to the second round counts from the START of the first learning window: a job of 5 GB batches learns in its first two)
    bool window_armed(bool memo_emptied) {
        if (memo_emptied) memo_clear_pending_ = false;
        const bool opens = learn_bytes_ == 0;
        if (opens) bytes_at_promo_ = bytes_seen_;
        learning_ = true;
        return opens;
    }
    // a learning batch that ended any other way than through batch_ended gives the slot back
    void learning_abandoned() { learning_ = false; }

    // A batch of `total` bytes has ended; `misses` of its `pieces` regex matches were not found in the key tables as a whole (vocabulary + promoted pieces).
    // Promote: the window is complete, install what it learnt (then promotion_installed).  Relearn: drop every promotion (then promotions_dropped).  The slot
    // stays taken through both: nothing learns meanwhile.  WindowContinues: the slot is free, the window goes on with the next batch.
    // `tables_generation`: generation() as it was when the batch took its copy of the tables.  A batch that ran on tables OLDER than the last install -- the
    // pipelined host path keeps two launch sequences enqueued ahead, and an install lands on a thread behind the batch that completed the window -- has the miss
    // share of the tables before: its bytes count, its share does not enter the average the level settles from (it settled too high, and the first batches
    // on the new tables then "left" it downwards: a re-learn on unchanged text).
    After batch_ended(int64_t total, double misses, double pieces, bool was_learning, size_t n_promoted, uint64_t tables_generation) {
        bytes_seen_ += total;
        if (!was_learning) {
            if (tables_generation != generation_) return After::Nothing;
            if (!left_settled_level(total, misses, pieces, n_promoted)) return After::Nothing;
            learning_ = true;
            return After::Relearn;
        }
        learn_bytes_ += total; win_miss_ += misses; win_pieces_ += pieces;
        if (adapt_ && learn_bytes_ < min_bytes_) { learning_ = false; return After::WindowContinues; }
        learn_bytes_ = 0;
        if (adapt_ && last_window_valid_ && win_pieces_ >= 1 && win_miss_ / win_pieces_ > last_window_miss_ * 1.25 + 0.01) {
            // A window whose miss share is a quarter (and a point) ABOVE the window's before it -- although that one's promotions have been installed since,
            // and promotions only lower the share on unchanged text -- was counted on ANOTHER text, with a memo full of the old one's pieces (it takes no
            // new entry into a full bucket): what it found is a fraction of what a fresh encoder finds (2 k against 9 k pieces on the source text behind 3 GB
            // of synthetic text).  A drift: start over -- this window's counts are dropped with the promotions, the memo is emptied, the next batch begins a window.
            win_miss_ = win_pieces_ = 0;
            return After::Relearn;
        }
        window_valid_ = last_window_valid_ = win_pieces_ >= 1;
        window_miss_ = last_window_miss_ = window_valid_ ? win_miss_ / win_pieces_ : 0;
        win_miss_ = win_pieces_ = 0;
        return After::Promote;
    }
    // the window's promotion is in the key tables (or failed: the tables are as they were): `added` pieces on top of `held_before`
    void promotion_installed(int64_t added, size_t held_before) {
        learning_ = false; ++rounds_; ++n_promotions_;
        if (added > 0 && ++fills_ == 1) first_fill_ = held_before + (size_t)added;
        // A round that found much it did not know -- more than a tenth of what the list held -- is a young encoder, or text that CHANGED without the miss
        // share having had a settled level to leave (the change fell between two installs): the next round then follows a gigabyte later, not
        // 2^rounds gigabytes.  (bench.py's drift leg, synthetic -> real text: the steps beyond 2 GB ran at 0.81 of an encoder that only ever saw
        // the real text, whose second round comes after 1 GB while this one's was 4 GB away.)
        if (adapt_ && rounds_ > 1 && (size_t)added * 10 > held_before) rounds_ = 1;
        // (not start_over: the rounds and the windows go on, and window_miss_ is what the level that settles next is compared with)
        // A round that added NOTHING replaced no table: the settled level stands, and so does the distance to the last change of the tables.  (Taking the level
        // away let a drift go unseen: a round that comes due on the very batches the text changes in -- a memo full of the old text's pieces, nothing new in
        // it to promote -- and the level settled again on the new text, with the old text's promotions and the old text's memo.)
        if (added <= 0) { window_valid_ = false; return; }
        bytes_at_install_ = bytes_seen_; ew_valid_ = base_valid_ = false;
    }
    // the promotions were dropped for a relearn: the next window starts from nothing, on an empty memo
    void promotions_dropped() { learning_ = false; start_over(); memo_clear_pending_ = true; ++n_relearns_; }
    // TKZ_OPT_PROMOTE 3, on an idle encoder (unlike promotions_dropped the memo keeps its entries, and nobody holds the slot)
    void reset_by_hand() { start_over(); }
    // A memo three quarters full takes hardly any new piece (an entry is never replaced; a bucket has two ways): text with many one-off pieces fills it within a
    // gigabyte, and whatever the text turns into afterwards finds it closed -- the reference's LRUCache would have evicted (LRUCache.cs:79-88).  The next learning
    // window therefore starts on an EMPTY memo: the hot pieces are back within the first megabytes of that batch, the one-off ones are gone.
    // (tools/adapt_probe.py ... 1: source text behind 3 GB of synthetic text, the change inside the first promotion's build: 95 GB/s and 2 k new pieces a round
    //  with the full memo, against a fresh encoder's 118 and 9 k.)
    void memo_read_back(uint64_t valid_slots, uint64_t slots) { if (adapt_ && valid_slots * 4 >= slots * 3) memo_clear_pending_ = true; }
    // The key tables on the device were replaced (an install, a drop; with the encoder's mutex held, together with the replacement): batches that took their copy
    // before ran on other tables (batch_ended)
    uint64_t generation() const { return generation_; }
    void tables_replaced() { ++generation_; }

private:
    // the tests' handle on the three distances: their batches are kilobytes
    static int64_t env_bytes(const char* name, int64_t dflt) { const char* v = getenv(name); return v && atoll(v) > 0 ? (int64_t)atoll(v) : dflt; }

    void start_over() {
        rounds_ = 0; fills_ = 0; learn_bytes_ = 0; bytes_at_promo_ = bytes_at_install_ = bytes_seen_;
        ew_valid_ = base_valid_ = window_valid_ = last_window_valid_ = false; win_miss_ = win_pieces_ = 0;
    }
    // TKZ_OPT_ADAPT: a batch that was not a learning batch has ended.  True when the encoder should learn again: the share of pieces that missed, averaged over
    // the recent batches by their bytes, has left the level at which it settled after the last promotion by more than a quarter (and a percentage point) either
    // way -- text whose pieces the promotions no longer answer, or text that a fresh encoder would answer better.  Not within adapt_min_bytes (256 MB) of the last
    // change of the tables: a re-learn costs one window at the speed of an encoder without promotions and two table builds on the host.
    bool left_settled_level(int64_t total, double misses, double pieces, size_t n_promoted) {
        if (!adapt_ || mode_ != 1 || pieces < 1) return false;
        const double rate = misses / pieces, w = std::min(1.0, (double)total / (double)settle_bytes_);
        ew_miss_ = ew_valid_ ? ew_miss_ + (rate - ew_miss_) * w : rate;
        ew_valid_ = true;
        if (learning_ || rounds_ < 1) return false;
        const int64_t since = bytes_seen_ - bytes_at_install_;
        if (!base_valid_) {
            if (since < settle_bytes_) return false;
            base_miss_ = ew_miss_; base_valid_ = true;
            // A change of text that falls between a learning window and the install of what it learnt -- a promotion is built on a host thread, tens of
            // milliseconds, gigabytes of text at this rate -- has no settled level to leave: the level settles on the new text.  But an install only ever ADDS
            // pieces, so on the text it was learnt from the level it leaves is at or below the WINDOW's own miss share; one that is a quarter (and a percentage
            // point) ABOVE it means those promotions answer another text: a drift.  (bench.py's drift leg, 3 GB of synthetic text in 15 ms and real text
            //  behind it: the first install landed ten real batches later, no drift was ever seen, and the encoder ran at 0.77 of a fresh one.)
            const bool drifted = window_valid_ && base_miss_ > window_miss_ * 1.25 + 0.01;
            window_valid_ = false;
            return drifted;
        }
        if (since < min_settled_bytes_) return false;
        // The list is (nearly) full of what SUCCESSIVE rounds have added: start over from the text as it is now.  Not a list that one window filled: that is
        // the text's hot pieces as they are now -- dropping it learns the same list again, a window at the speed of an encoder without promotions and two
        // table builds every adapt_min_bytes, for ever (may_learn opens no further round on a full list; a drift is still seen by the miss share, below).
        // Nor one that a window brought beyond 90 % and a later round added a few pieces to.
        if (fills_ >= 2 && first_fill_ * 10 < cap_ * 9 && n_promoted * 10 >= cap_ * 9) return true;
        return ew_miss_ > base_miss_ * 1.25 + 0.01 || ew_miss_ < base_miss_ * 0.75 - 0.01;
    }

    int mode_ = 1;                         // TKZ_OPT_PROMOTE: 0 never on its own, 1 automatic (default)
    int adapt_ = 1;
    int64_t min_bytes_ = int64_t(8) << 20; // a learning window is this much text
    size_t cap_ = 65536;                   // promoted pieces the key tables hold at most
    // how much text the miss share is averaged over / has to settle for after a promotion, the first gap between rounds, and how soon after an install the encoder may learn again
    int64_t settle_bytes_ = env_bytes("TKZ_ADAPT_SETTLE_BYTES", int64_t(64) << 20);
    int64_t round_bytes_ = env_bytes("TKZ_ADAPT_ROUND_BYTES", kPromoSecondBytes);
    int64_t min_settled_bytes_ = env_bytes("TKZ_ADAPT_MIN_BYTES", int64_t(256) << 20);

    int rounds_ = 0;                       // automatic promotions since the list was last empty (back to 1 after a round that added much)
    int fills_ = 0;                        // ... those of them that added pieces (never set back), and what the list held after the first of them: a list
    size_t first_fill_ = 0;                //     that LATER ROUNDS have filled is one of two fills and more whose first left it below 90 % of the cap
    uint64_t generation_ = 0;              // replacements of the key tables on the device (tables_replaced)
    bool learning_ = false;                // the learning slot: a batch that counts memo hits is in flight, or what it learnt is being installed / dropped
    int64_t bytes_seen_ = 0;               // bytes the batch path has encoded
    int64_t bytes_at_promo_ = 0;           // ... when the last window opened
    int64_t bytes_at_install_ = 0;         // ... when the key tables were last replaced
    int64_t learn_bytes_ = 0;              // bytes of the open window so far (batches smaller than promo_min_bytes add up to one)
    bool memo_clear_pending_ = false;      // the memo is emptied before the next window starts
    double ew_miss_ = 0, base_miss_ = 0;   // miss share of the recent batches; ... as it settled after the last install
    bool ew_valid_ = false, base_valid_ = false;
    double win_miss_ = 0, win_pieces_ = 0; // misses and pieces of the open window ...
    double window_miss_ = 0;               // ... and the miss share of the window the LAST install was learnt in (promotions only lower it on unchanged text)
    bool window_valid_ = false;
    double last_window_miss_ = 0;          // the same, kept for the NEXT window to be compared with
    bool last_window_valid_ = false;
    int64_t n_promotions_ = 0, n_relearns_ = 0;
};

}  // namespace tkz
