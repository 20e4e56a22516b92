// Drives the decode-lane bookkeeping (genie_tts_amd/csrc/lanes.h) through the call sequences the
// engine sees, against a small model of the device: three KV slots, one in-order stream per lane,
// results captured when a launch "completes".  Host code only; built with
// -fsanitize=address,undefined and run by tests/test_lane_book.py.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/lane_book_check.cpp -o lane_book_check && ./lane_book_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../genie_tts_amd/csrc/lanes.h"

using gsv::LaneBook;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

namespace {
// What gen_start / gen_finish / gsv_t2s_generate do with the book, with the device modelled.
struct Model {
    LaneBook lb;
    std::vector<int> slot;          // utterance held by each KV slot (-1: none); resized by growth
    int tmax = 0;
    struct Entry { int utt = -1, result = -1; bool complete = false, err = false; } q[LaneBook::QUEUE];
    int prefetched = -1;            // utterance prefilled into the prefetch slot (launched)
    int reallocs = 0;

    explicit Model(int lanes) { CHECK(lb.configure(lanes)); }

    void complete(int k) {          // the entry's launch ran: its results go to pinned memory
        if (q[k].complete) return;
        q[k].result = slot[LaneBook::slot_of(lb.q_lane[k])];
        q[k].complete = true;
    }
    void run_lane(int lane) {       // a stream is in order: new work on it runs after its earlier launches
        for (int i = 0; i < lb.n; ++i) {
            const int k = (lb.head + i) % LaneBook::QUEUE;
            if (lb.q_lane[k] == lane) complete(k);
        }
    }
    void drain() {
        for (int i = 0; i < lb.n; ++i) complete((lb.head + i) % LaneBook::QUEUE);
        lb.drained();
    }
    void reserve(int slots, int need) {
        if (slots <= (int)slot.size() && need <= tmax) return;
        // re-allocation: nothing may be in flight
        for (int i = 0; i < lb.n; ++i) CHECK(q[(lb.head + i) % LaneBook::QUEUE].complete);
        slot.assign(slots > (int)slot.size() ? slots : slot.size(), -1);
        if (need > tmax) tmax = need;
        prefetched = -1;
        ++reallocs;
    }
    void prefetch(int utt, int need) {
        const int want = lb.slots(true);
        if ((int)slot.size() < want || need > tmax) drain();
        reserve(want, need);
        slot[LaneBook::PREFETCH_SLOT] = utt;   // (launched by the next start; the model runs it at once)
        prefetched = utt;
    }
    void start(int utt, int need, bool err = false, bool persist_ok = true) {
        CHECK(!lb.full());
        const int want = lb.slots(false);
        if (need > tmax || (int)slot.size() < want) drain();
        reserve(want, need);
        const int lane = persist_ok ? lb.next_lane() : 0;
        CHECK(lane >= 0 && lane < lb.lanes);
        const int s = LaneBook::slot_of(lane);
        CHECK(s != LaneBook::PREFETCH_SLOT && s < (int)slot.size());
        if (lb.lanes == 2 && persist_ok) CHECK(!lb.lane_in_flight(lane));   // the lane not in use
        run_lane(lane);
        slot[s] = utt;              // the prefetch slot's copy, or the lane's own prefill
        if (prefetched == utt) prefetched = -1;
        const int k = lb.tail();
        q[k] = Entry{utt, -1, false, err};
        CHECK(lb.push(lane) == k);
        ++lb.launches[lane];
    }
    int generate_sync(int utt, int need) {   // gsv_t2s_generate: drains, decodes on slot 0
        drain();
        reserve(1, need);
        for (int i = 0; i < lb.n; ++i) CHECK(lb.q_drained[(lb.head + i) % LaneBook::QUEUE]);
        slot[0] = utt;
        return slot[0];
    }
    int finish() {
        CHECK(!lb.empty());
        const int k = lb.pop();
        complete(k);
        if (q[k].err) {             // error word set: drain both lanes, re-run synchronously
            drain();
            const int saved = lb.hide();
            CHECK(lb.empty());
            const int r = generate_sync(q[k].utt, tmax);
            lb.unhide(saved);
            return r;
        }
        return q[k].result;
    }
};

// bench.py's Runner.stream: prefetch i+2, start i+1, finish i
void bench_sequence(int lanes, int n) {
    Model m(lanes);
    m.prefetch(1, 200);
    m.start(0, 200);
    for (int i = 0; i < n; ++i) {
        if (i + 1 < n) {
            if (i + 2 < n) m.prefetch(i + 2, 200);
            m.start(i + 1, 200);
            CHECK(m.lb.n == 2);
            if (lanes == 2) CHECK(m.lb.q_lane[m.lb.head] != m.lb.q_lane[(m.lb.head + 1) % 2]);
        }
        CHECK(m.finish() == i);
    }
    CHECK(m.lb.empty());
    CHECK(m.reallocs == 1);
    if (lanes == 2) {
        CHECK(m.lb.launches[0] == (n + 1) / 2 && m.lb.launches[1] == n / 2);
    } else {
        CHECK(m.lb.launches[0] == n && m.lb.launches[1] == 0);
    }
}

// test_async_generate_stream_matches_plain: misses, then a synchronous generate in between
void misses_and_sync(int lanes) {
    Model m(lanes);
    m.start(3, 150);
    m.start(4, 150);
    CHECK(m.finish() == 3);
    CHECK(m.generate_sync(2, 150) == 2);   // waits for the started one; its result stays queued
    CHECK(m.lb.n == 1);
    CHECK(m.finish() == 4);
    m.start(5, 150);                       // the lanes go on alternating after the drain
    m.start(6, 150);
    if (lanes == 2) CHECK(m.lb.q_lane[m.lb.head] != m.lb.q_lane[(m.lb.head + 1) % 2]);
    CHECK(m.finish() == 5);
    CHECK(m.finish() == 6);
    // a start without the persistent path decodes on slot 0 whatever lane is next
    m.start(7, 150);
    m.start(8, 150, false, false);
    CHECK(m.finish() == 7);
    CHECK(m.finish() == 8);
}

// both launches in flight meet the error word: both re-run, the second one's state survives the first's re-run
void error_reruns(int lanes) {
    Model m(lanes);
    m.start(0, 100, true);
    m.start(1, 100, true);
    CHECK(m.finish() == 0);
    CHECK(m.lb.n == 1);
    CHECK(m.finish() == 1);
    m.start(2, 100, true);
    m.start(3, 100);                       // the healthy one's results survive the other's re-run
    CHECK(m.finish() == 2);
    CHECK(m.finish() == 3);
    CHECK(m.lb.empty());
}

// a start that needs more tokens than reserved while the other lane is in flight
void growth(int lanes) {
    Model m(lanes);
    m.start(0, 100);
    m.start(1, 400);
    CHECK(m.reallocs == 2);
    CHECK(m.finish() == 0);
    m.prefetch(2, 900);                    // a prefetch that grows the state drains too
    CHECK(m.reallocs == 3);
    m.start(2, 900);
    CHECK(m.finish() == 1);
    CHECK(m.finish() == 2);
}
}  // namespace

int main() {
    for (int lanes = 1; lanes <= 2; ++lanes) {
        for (int n : {1, 2, 3, 6, 101}) bench_sequence(lanes, n);
        misses_and_sync(lanes);
        error_reruns(lanes);
        growth(lanes);
    }
    LaneBook b;
    CHECK(b.configure(2));
    b.push(b.next_lane());
    CHECK(!b.configure(1));                // never while a generate is in flight
    CHECK(!b.configure(3));
    std::puts("lane book ok");
    return 0;
}
