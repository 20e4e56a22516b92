// Decode-lane bookkeeping of the asynchronous generate (gsv_t2s_generate_start / _finish): which
// lane the next start takes, which started generate holds which lane and KV slot, and what a
// drain leaves valid.  Host-only and free of HIP calls, so tools/lane_book_check.cpp drives it
// under the host sanitizers.
//
// Slots of the decode state: 0 = lane 0 (the engine stream: every synchronous path decodes
// there), 1 = the prefetch (gsv_t2s_prefetch), 2 = lane 1.  Started generates finish in the
// order they were started (a FIFO of at most two).
#pragma once

namespace gsv {

struct LaneBook {
    static constexpr int MAX_LANES = 2, QUEUE = 2, PREFETCH_SLOT = 1;
    int lanes = 1;                      // configured lanes (1 or 2)
    int head = 0, n = 0;                // FIFO of the started generates: entries head .. head + n - 1 (mod QUEUE)
    int q_lane[QUEUE] = {0, 0};         // lane of each entry
    bool q_drained[QUEUE] = {false, false};   // its launch is known to be complete (a drain waited for it)
    unsigned long seq = 0;              // starts so far
    unsigned long started[MAX_LANES] = {0, 0};   // number of the lane's latest start (0: never)
    long launches[MAX_LANES] = {0, 0};  // persistent launches issued on each lane (counters)

    static int slot_of(int lane) { return lane == 0 ? 0 : 2; }
    // decode-state slots a stream needs: the lanes' and the prefetch's (one lane: slot 0, and
    // slot 1 once a prefetch is made)
    int slots(bool prefetch) const { return lanes == 2 ? 3 : prefetch ? 2 : 1; }

    // Only with nothing in flight.  The lane history restarts: the next start takes lane 0.
    bool configure(int l) {
        if (n != 0 || l < 1 || l > MAX_LANES) return false;
        lanes = l;
        started[0] = started[1] = 0;
        return true;
    }
    bool full() const { return n == QUEUE; }
    bool empty() const { return n == 0; }
    int tail() const { return (head + n) % QUEUE; }   // the entry the next start fills
    // The lane whose previous generate was started least recently: with at most two in flight
    // and FIFO finishes, the lane not in use.
    int next_lane() const { return lanes == 2 && started[1] < started[0] ? 1 : 0; }
    bool lane_in_flight(int lane) const {
        for (int i = 0; i < n; ++i)
            if (q_lane[(head + i) % QUEUE] == lane) return true;
        return false;
    }
    // A generate was started on `lane`: returns its entry.
    int push(int lane) {
        const int k = tail();
        q_lane[k] = lane;
        q_drained[k] = false;
        started[lane] = ++seq;
        ++n;
        return k;
    }
    // The oldest started generate is being finished: returns its entry (valid until the next push).
    int pop() {
        const int k = head;
        head = (head + 1) % QUEUE;
        --n;
        return k;
    }
    // Every started launch has completed: the entries stay queued with their results (pinned host
    // memory) and error words valid, and every slot may be overwritten.
    void drained() {
        for (int i = 0; i < n; ++i) q_drained[(head + i) % QUEUE] = true;
    }
    // A synchronous generate runs while started ones stay queued (they were drained): it must not
    // see the queue.  hide() returns what unhide() restores.
    int hide() { const int s = n; n = 0; return s; }
    void unhide(int s) { n = s; }
};

}  // namespace gsv
