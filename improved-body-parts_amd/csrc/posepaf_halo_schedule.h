// posepaf_halo_schedule.h -- the LDS-DMA and LDS-read schedule of k_conv3x3_halo's main loop (posepaf_conv_own.hip), stated ONCE.
// Plain constexpr C++17, no device code: the kernel reads its issue positions and every s_waitcnt immediate from here, a host
// compiler can include it (tests/test_halo_schedule_cpu.py prints and replays the table), and a count that would let a reader
// overtake its load does not compile.
//
// The loop runs in PHASES: one tap of one block of 32 input channels each, NT = 9 (3x3) or 4 (collapsed upsample) taps per block,
// one barrier per phase.  A wave's vector-memory loads inside the loop are LDS-DMA only, and they complete IN ORDER:
// `s_waitcnt vmcnt(N)` returns when at most the last N issued loads are outstanding.  Two things are stated, the rest is derived.
//
// ISSUE.  While block cb is multiplied the halo of block cb + 1 streams into the other halo buffer, NPW pieces per wave (7, or 6
// on the narrower tiles): piece k goes out at tap issue_tap(k) -- nine taps spread them 2-2-1-1(-1) over taps 0..4 so that no tap
// holds the wave's load path for long, four taps have no room for that and issue all at tap 0.  Every tap then issues ONE weight
// slice, after its pieces: the slice of phase ph + AHEAD, into ring slot (ph + AHEAD) % NW.
//
// FIRST READER.  A piece of block cb + 1 is first read by the fragment refill in half B of the LAST tap of block cb (after
// flip_R), so it must have landed when tap NT - 2 ends.  The slice issued in phase q is first read in half B of phase
// q + AHEAD - 1 (as wf[0], wf[1] of the next phase), so it must have landed, and been published by the barrier, when phase
// q + AHEAD - 2 ends.
//
// DERIVED.  KEEP = AHEAD - 2: the slices of this phase and of the KEEP - 1 before it may still be in flight when a phase ends.
// in_flight(tap, halo), the vmcnt immediate at the end of a tap, is the number of loads issued after the most recently issued load
// that is due at or before that tap, counted over the steady-state sequence (a block with a successor, then this block).
// in_window(k, tap): piece k (k >= OPTIONAL: a wave may not own it, and then issues nothing for it) is among those loads, so a
// wave without it waits for one load less.  The last phases of a tile issue no slice and wait for vmcnt(0); that tail is a
// run-time test in the kernel.
//
// The ring slot that phase ph overwrites is the one phase ph - 1 read: its last read (wf[2], wf[3]) is issued at the start of
// that phase's half A and waited for before its half B, and every wave is past the barrier that ended phase ph - 1 before any
// wave issues in phase ph.  Hence NW == AHEAD + 1 and no more.
//
// HISTORY.  These counts were once summed by hand inside the kernel ("the pieces of the last three taps", KEEP = 3 a free
// constant).  That sum is right for nine taps and wrong for four: all pieces go out at tap 0 and are due when tap 2 ends, but the
// sum still counted them there -- vmcnt(3 + NPW) -- and the refill of tap 3 read a halo that was still arriving: wrong pixels,
// under load only, found by tools/collapsed_repeat.py (runs bit-compared).  With the first reader stated here that count fails
// Check::deadlines below.
#pragma once

namespace halo_schedule {

// What is stated and what is derived.  The kernel uses Schedule below: this table with its deadlines checked.
template <int NT_, int NPW_, int AHEAD_, int NW_>
struct Table {
    static constexpr int NT = NT_, NPW = NPW_, AHEAD = AHEAD_, NW = NW_;
    static_assert(NT == 9 || NT == 4, "taps per channel block");
    static_assert(NPW >= 4 && NPW <= 7, "halo pieces per wave");
    static_assert(NW == AHEAD + 1, "the slice of phase ph + AHEAD overwrites the ring slot phase ph - 1 read, and only that one is free");
    static constexpr int KEEP = AHEAD - 2;
    static_assert(KEEP >= 1, "a slice needs a phase to land and a barrier to be published");
    static constexpr int OPTIONAL = 4;    // pieces k >= OPTIONAL exist on some waves only
    static constexpr int SLICE = -1;      // a weight slice, where a load is named by its piece index

    // ---- issue
    static constexpr int issue_tap(int k) { return NT == 9 ? (k < 4 ? k / 2 : k - 2) : 0; }
    static constexpr bool pieces_before_slice = true;   // order inside a tap: pieces in ascending k, then the slice
    // ---- first reader (taps of the issuing block for a piece, phases for a slice; both read in half B) and the deadline it sets
    static constexpr int piece_first_read = NT - 1;
    static constexpr int piece_due = NT - 2;
    static constexpr int slice_first_read(int q) { return q + AHEAD - 1; }
    static constexpr int slice_due(int q) { return q + AHEAD - 2; }

    // The steady-state issue sequence up to the end of `tap`: block 0 (it has a successor, so halo pieces stream), then this block
    // (`halo`: it has one too).  Phases are numbered through: block * NT + tap.  `absent`: bit k set = the wave does not own piece k.
    struct Sequence {
        int n = 0, now = 0;
        int piece[2 * (9 + 7)] = {}, due[2 * (9 + 7)] = {}, first_read[2 * (9 + 7)] = {};
        int last_due = -1;   // index of the most recently issued load that must have landed when phase `now` ends
    };
    static constexpr Sequence sequence(int tap, bool halo, unsigned absent = 0) {
        Sequence s;
        s.now = NT + tap;
        for (int q = 0; q <= s.now; q++)
            for (int turn = 0; turn < 2; turn++) {
                if ((turn == 1) == pieces_before_slice) {
                    s.piece[s.n] = SLICE, s.due[s.n] = slice_due(q), s.first_read[s.n] = slice_first_read(q);
                    s.n++;
                } else if (q < NT || halo) {
                    for (int k = 0; k < NPW; k++)
                        if (issue_tap(k) == q % NT && !((absent >> k) & 1)) {
                            s.piece[s.n] = k, s.due[s.n] = q - q % NT + piece_due, s.first_read[s.n] = q - q % NT + piece_first_read;
                            s.n++;
                        }
                }
            }
        for (int i = 0; i < s.n; i++)
            if (s.due[i] <= s.now) s.last_due = i;
        return s;
    }

    // ---- the vmcnt immediate at the end of `tap`, and whether (optional) piece k is among the loads it leaves outstanding
    static constexpr int in_flight(int tap, bool halo, unsigned absent = 0) {
        const Sequence s = sequence(tap, halo, absent);
        return s.n - 1 - s.last_due;
    }
    static constexpr bool in_window(int k, int tap) {
        const Sequence s = sequence(tap, true);
        for (int i = s.last_due + 1; i < s.n; i++)
            if (s.piece[i] == k) return true;
        return false;
    }
};

// ---- the deadlines, checked against the FIRST READERS (not against the due taps the counts were derived from)
template <class T>
struct Check {
    using Sequence = typename T::Sequence;
    static constexpr int NT = T::NT, NPW = T::NPW, KEEP = T::KEEP, OPTIONAL = T::OPTIONAL;
    // whatever a wait leaves outstanding is first read after the NEXT phase at the earliest -- for every tap, with and without a
    // successor block, and for every set of pieces a wave may not own
    static constexpr bool deadlines() {
        for (int h = 0; h < 2; h++)
            for (int tap = 0; tap < NT; tap++)
                for (unsigned absent = 0; absent < 8; absent++) {
                    const Sequence s = T::sequence(tap, h != 0, absent << OPTIONAL);
                    if (s.last_due < 0) return false;
                    for (int i = s.last_due + 1; i < s.n; i++)
                        if (s.first_read[i] - 1 <= s.now) return false;
                }
        return true;
    }
    // ... and one load more would be one that is read in the next phase
    static constexpr bool tight() {
        for (int h = 0; h < 2; h++)
            for (int tap = 0; tap < NT; tap++) {
                const Sequence s = T::sequence(tap, h != 0);
                if (s.last_due < 0 || s.first_read[s.last_due] - 1 > s.now) return false;
            }
        return true;
    }
    static constexpr bool never_below_keep() {
        for (int h = 0; h < 2; h++)
            for (int tap = 0; tap < NT; tap++)
                for (unsigned absent = 0; absent < 8; absent++)
                    if (T::in_flight(tap, h != 0, absent << OPTIONAL) < KEEP) return false;
        return true;
    }
    // the kernel subtracts one load per absent piece inside the window: that must be the count of the sequence without them
    static constexpr bool window_is_the_absent_count() {
        for (int tap = 0; tap < NT; tap++)
            for (unsigned absent = 0; absent < 8; absent++) {
                int missing = 0;
                for (int k = OPTIONAL; k < OPTIONAL + 3; k++) missing += (((absent << OPTIONAL) >> k) & 1) && T::in_window(k, tap);
                if (T::in_flight(tap, true, absent << OPTIONAL) != T::in_flight(tap, true) - missing) return false;
            }
        return true;
    }
    // a piece is KEEP phases old when it is waited for, like a slice (or goes out with the block's first tap where the block is
    // shorter than that) -- in particular it is issued before its due tap: no wait stalls on a load younger than the ones the loop
    // is built to hide
    static constexpr bool pieces_old_enough() {
        for (int k = 0; k < NPW; k++)
            if (T::piece_due - T::issue_tap(k) < (KEEP < T::piece_due ? KEEP : T::piece_due)) return false;
        return true;
    }
};

template <int NT, int NPW, int AHEAD, int NW>
struct Schedule : Table<NT, NPW, AHEAD, NW> {
    using C = Check<Table<NT, NPW, AHEAD, NW>>;
    static_assert(NPW <= Schedule::OPTIONAL + 3, "three presence flags");
    static_assert(C::pieces_old_enough(), "a halo piece is issued too late for its due tap");
    static_assert(C::deadlines(), "a wait lets a load's first reader run while the load may still be in flight");
    static_assert(C::tight(), "a wait asks for a load that nothing reads in the next phase");
    static_assert(C::never_below_keep(), "a wait asks for one of the last KEEP weight slices");
    static_assert(C::window_is_the_absent_count(), "in_window disagrees with the issue sequence of a wave that does not own a piece");
};

// LDS fragment reads of a wave (ds_read_b128; LDS returns in order, so lgkmcnt is counted like vmcnt).  Issue order, from half B of
// the previous phase on: wf[0], wf[1] of this phase, the PT pixel fragments of this phase in tile order (each after the two MFMAs
// that last used its register), then -- at the start of this phase's half A -- wf[2], wf[3] of this phase.
template <int PT>
struct Reads {
    static constexpr int weights_b = 2, weights_a = 2;                       // wf[0], wf[1] / wf[2], wf[3]
    static constexpr int pixel(int i) { return weights_b + i; }              // position of pixel fragment i
    static constexpr int issued_at_half_a = weights_b + PT + weights_a;
    // before the MFMAs of pixel tile i in half A: everything up to xf[i] landed, the reads after it may be outstanding
    static constexpr int before_tile_a(int i) { return issued_at_half_a - 1 - pixel(i); }
    // before half B (it needs wf[2], wf[3], the last reads of half A): only the next phase's wf[0], wf[1], where a next phase exists
    static constexpr int before_half_b(bool refill) { return refill ? weights_b : 0; }
    static_assert(before_tile_a(PT - 1) == weights_a && before_tile_a(0) == PT - 1 + weights_a, "pixel tiles i + 1 .. PT - 1 and two weight reads");
};

// every instance the kernel has
static_assert(sizeof(Schedule<9, 7, 5, 6>) > 0, "");
static_assert(sizeof(Schedule<9, 6, 5, 6>) > 0, "");
static_assert(sizeof(Schedule<4, 7, 5, 6>) > 0, "");
static_assert(sizeof(Schedule<4, 6, 5, 6>) > 0, "");

}  // namespace halo_schedule
