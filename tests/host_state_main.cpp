// The host state of the forest launch (3d-beats_amd/csrc/rdf_host_state.hpp) driven without a GPU: its contract single-threaded,
// then four threads on two DeviceStates and the registry.  Built and run by tests/test_host_state.py under the thread sanitizer
// and under the address + undefined-behaviour sanitizers; exits non-zero on the first failed check.
#include "rdf_host_state.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <thread>

using namespace rdf_host;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);  \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

static const void *ptr(uintptr_t v) { return reinterpret_cast<const void *>(v); }

static void in_use(DeviceState &ds, int want_stream, int want_graph)
{
    int s = -1, g = -1;
    ds.slots_in_use(&s, &g);
    CHECK(s == want_stream);
    CHECK(g == want_graph);
}

static void check_slot_pool()
{
    SlotPool pool(kSchedSlots);
    for (int i = 0; i < kSchedSlots; ++i) CHECK(pool.take() == i);
    CHECK(pool.take() == -1);
    CHECK(pool.in_use() == kSchedSlots);
    pool.give(5);
    pool.give(9);
    CHECK(pool.in_use() == kSchedSlots - 2);
    CHECK(pool.take() == 9);        // given-back slots first, the most recent first
    CHECK(pool.take() == 5);
    CHECK(pool.take() == -1);
    SlotPool fresh(4);
    CHECK(fresh.take() == 0);
    fresh.give(0);
    CHECK(fresh.take() == 0);       // ... before a fresh one
    CHECK(fresh.take() == 1);
}

static void check_stream_slots()
{
    DeviceStates devices;
    DeviceState &ds = devices.at(0);
    CHECK(&devices.at(0) == &ds);           // made once, never moves
    CHECK(&devices.at(kMaxDevices - 1) != &ds);
    in_use(ds, 0, 0);
    const void *a = ptr(0x1000), *b = ptr(0x2000);
    const int a0 = ds.stream_slot(a, 0), a1 = ds.stream_slot(a, 1), a17 = ds.stream_slot(a, 17), b0 = ds.stream_slot(b, 0);
    const int null0 = ds.stream_slot(nullptr, 0);
    CHECK(std::set<int>({a0, a1, a17, b0, null0}).size() == 5);
    CHECK(ds.stream_slot(a, 0) == a0 && ds.stream_slot(a, 1) == a1 && ds.stream_slot(a, 17) == a17 && ds.stream_slot(b, 0) == b0);
    in_use(ds, 5, 0);
    ds.remember_usable_cus(a, 224);
    ds.remember_usable_cus(b, 32);
    ds.drop_stream(a);                      // its slots of every role and its CU count, nothing else
    in_use(ds, 2, 0);
    int n = 0;
    CHECK(!ds.usable_cus(a, &n));
    CHECK(ds.usable_cus(b, &n) && n == 32);
    CHECK(ds.stream_slot(b, 0) == b0 && ds.stream_slot(nullptr, 0) == null0);
    const int c0 = ds.stream_slot(ptr(0x3000), 0);      // a given-back slot before a fresh one
    CHECK(c0 == a0 || c0 == a1 || c0 == a17);
    in_use(ds, 3, 0);
    // the pool runs out at kSchedSlots; a stream without a slot gets none, again and again, and takes nothing
    for (int i = 3; i < kSchedSlots; ++i) CHECK(ds.stream_slot(ptr(0x10000 + 16 * i), 0) >= 0);
    in_use(ds, kSchedSlots, 0);
    CHECK(ds.stream_slot(ptr(0x9000), 0) == -1);
    CHECK(ds.stream_slot(ptr(0x9000), 0) == -1);
    in_use(ds, kSchedSlots, 0);
    ds.drop_stream(b);
    CHECK(ds.stream_slot(ptr(0x9000), 0) == b0);
    in_use(devices.at(1), 0, 0);            // another device: a state of its own
}

static void check_graph_slots()
{
    DeviceState ds;
    bool say = true;
    CHECK(ds.stream_slot(ptr(0x1000), 0) == 0);
    CHECK(ds.graph_slot(7, &say) == 0 && !say);         // independent of the stream slots
    CHECK(ds.graph_slot(7, &say) == 1 && !say);
    CHECK(ds.graph_slot(8, &say) == 2 && !say);
    in_use(ds, 1, 3);
    CHECK(ds.release_capture(7) == 2);
    in_use(ds, 1, 1);
    CHECK(ds.release_capture(7) == 0);                  // once
    CHECK(ds.release_capture(99) == 0);
    in_use(ds, 1, 1);
    const int again = ds.graph_slot(9, &say);
    CHECK((again == 0 || again == 1) && !say);
    in_use(ds, 1, 2);
    for (int i = 2; i < kGraphSlots; ++i) CHECK(ds.graph_slot(10, &say) >= 0 && !say);
    in_use(ds, 1, kGraphSlots);
    CHECK(ds.graph_slot(11, &say) == -1 && say);        // said the first time only
    CHECK(ds.graph_slot(11, &say) == -1 && !say);
    CHECK(ds.release_capture(11) == 0);
    CHECK(ds.release_capture(10) == kGraphSlots - 2);
    in_use(ds, 1, 2);
    CHECK(ds.release_capture(8) == 1 && ds.release_capture(9) == 1);
    in_use(ds, 1, 0);
}

static void check_caches_and_flag()
{
    DeviceState ds;
    int n = -1;
    const void *k1 = ptr(0x100), *k2 = ptr(0x200);
    CHECK(!ds.occupancy(k1, 4096, &n));
    ds.remember_occupancy(k1, 4096, 5);
    ds.remember_occupancy(k1, 70000, 2);
    ds.remember_occupancy(k2, 4096, 3);
    CHECK(ds.occupancy(k1, 4096, &n) && n == 5);
    CHECK(ds.occupancy(k1, 70000, &n) && n == 2);
    CHECK(ds.occupancy(k2, 4096, &n) && n == 3);
    CHECK(!ds.occupancy(k2, 70000, &n));
    CHECK(!ds.usable_cus(ptr(0x1000), &n));
    ds.remember_usable_cus(ptr(0x1000), 192);
    CHECK(ds.usable_cus(ptr(0x1000), &n) && n == 192);
    CHECK(!ds.usable_cus(ptr(0x2000), &n));

    static unsigned int word = 0, made = 0;
    CHECK(!ds.stale_flag_made() && !ds.take_stale() && ds.stale_flag_if_made().host == nullptr);
    const auto alloc = []() { ++made; StaleFlag f; f.host = f.dev = &word; return f; };
    CHECK(ds.stale_flag(alloc).host == &word && ds.stale_flag(alloc).dev == &word && made == 1);
    CHECK(ds.stale_flag_made() && ds.stale_flag_if_made().dev == &word);
    CHECK(!ds.take_stale());
    word = 0x1234u;             // (a kernel's write)
    CHECK(ds.take_stale());     // true once
    CHECK(!ds.take_stale() && word == 0);
}

static PackedSeen seen(uint32_t exact, uint32_t choice_word, uint32_t generation, const void *info)
{
    return {exact, choice_word, generation, 0.5f, info, 3u, 0u};
}

static void check_registry()
{
    PackedTables t;
    PackedState st;
    const void *a = ptr(0xA000), *b = ptr(0xB000), *c = ptr(0xC000);
    CHECK(!t.find(a, &st));
    // a choice made before the first sight wins over the table's and is the word to write through
    CHECK(t.set_choice(a, 9) == nullptr);
    CHECK(t.find(a, &st) && st.deep_from == 9 && st.exact_nodes == -1);
    CHECK(t.learn(a, seen(0, 13, 77, ptr(0xA800)), &st) == 10u);
    CHECK(st.deep_from == 9 && st.exact_nodes == 0 && st.generation == 77u && st.scale == 0.5f && st.info_dev == ptr(0xA800) &&
          st.deep_min_root == 3u && st.deep_bad_last == 0u);
    CHECK(t.learn(a, seen(0, 10, 77, ptr(0xA800)), &st) == 0u && st.deep_from == 9);     // the table agrees: nothing to write
    CHECK(t.set_choice(a, 0) == ptr(0xA800));
    CHECK(t.learn(a, seen(0, 0, 77, ptr(0xA800)), &st) == 1u && st.deep_from == 0);      // "never" is a choice too
    // a choice found in the info block is adopted when none was made here
    CHECK(t.learn(b, seen(2, 13, 78, ptr(0xB800)), &st) == 0u);
    CHECK(st.deep_from == 12 && st.exact_nodes == 2);
    CHECK(t.learn(c, seen(0xFFFFFFFFu, 0, 79, ptr(0xC800)), &st) == 0u && st.deep_from == -1 && st.exact_nodes == 0x7FFFFFFF);
    CHECK(t.set_choice(c, -1) == ptr(0xC800));
    CHECK(t.find(c, &st) && st.deep_from == -1);
    CHECK(deep_choice_word(-1) == 0u && deep_choice_word(0) == 1u && deep_choice_word(40) == 31u);
    // forget removes one address only
    t.forget(b);
    CHECK(!t.find(b, &st) && t.find(a, &st) && t.find(c, &st));
    t.forget(b);
    CHECK(t.learn(b, seen(0, 0, 80, ptr(0xB800)), &st) == 0u && st.deep_from == -1 && st.generation == 80u);   // read afresh: no old choice
    t.forget_all();
    CHECK(!t.find(a, &st) && !t.find(b, &st) && !t.find(c, &st));
}

// Four threads, a fixed number of mixed operations each, on two DeviceStates and one registry.  Every thread has streams and
// capture ids of its own (as callers do: a stream is destroyed by who made it) and shares the devices, the kernels' occupancy
// entries, the stale flags and the tables with the others.
static void check_threads()
{
    constexpr int kThreads = 4, kOps = 4000;
    DeviceStates devices;
    PackedTables tables;
    static unsigned int words[2];
    words[0] = words[1] = 0u;
    std::atomic<int> raised{0}, taken{0};
    std::vector<std::thread> threads;
    for (int t = 0; t < kThreads; ++t)
        threads.emplace_back([&, t]() {
            uint32_t rng = 12345u + 977u * (uint32_t)t;
            int live_graph[2] = {0, 0};
            for (int op = 0; op < kOps; ++op) {
                rng = rng * 1664525u + 1013904223u;
                const int d = (rng >> 8) & 1, what = (rng >> 12) % 12, v = (rng >> 20) & 7;
                DeviceState &ds = devices.at(d);
                const void *stream = ptr(0x100000u * (uint32_t)(t + 1) + 0x100u * (uint32_t)v);
                const void *table = ptr(0xA0000u + 0x1000u * (uint32_t)v);      // shared by all threads
                const unsigned long long capture = 100ull * (unsigned long long)t + (unsigned long long)(v & 1);
                PackedState st;
                bool say = false;
                int n = 0;
                switch (what) {
                case 0: case 1: CHECK(ds.stream_slot(stream, v & 3) == ds.stream_slot(stream, v & 3)); break;
                case 2: ds.drop_stream(stream); break;
                case 3: if (ds.graph_slot(capture, &say) >= 0) ++live_graph[d]; break;
                case 4: live_graph[d] -= ds.release_capture(capture); break;
                case 5:
                    if (ds.occupancy(ptr(0x100u * (uint32_t)v), 1024 * v, &n)) CHECK(n == v + 1);
                    else ds.remember_occupancy(ptr(0x100u * (uint32_t)v), 1024 * v, v + 1);
                    break;
                case 6:
                    if (ds.usable_cus(stream, &n)) CHECK(n == 32 * (v + 1));
                    else ds.remember_usable_cus(stream, 32 * (v + 1));
                    break;
                case 7:
                    (void)ds.stale_flag([d]() { StaleFlag f; f.host = f.dev = &words[d]; return f; });
                    if (v == 0) { __atomic_store_n(&words[d], 1u, __ATOMIC_RELAXED); ++raised; }     // (a kernel's write)
                    if (ds.take_stale()) { ++taken; tables.forget_all(); }
                    break;
                case 8:
                    if (!tables.find(table, &st) || st.exact_nodes < 0) (void)tables.learn(table, seen(0, (uint32_t)v, 1u + (uint32_t)v, table), &st);
                    CHECK(st.exact_nodes == 0 && st.generation == 1u + (uint32_t)v);
                    break;
                case 9: (void)tables.set_choice(table, v - 1); break;
                case 10: tables.forget(table); break;
                default: ds.slots_in_use(&n, nullptr); CHECK(n >= 0 && n <= kSchedSlots); break;
                }
            }
            // this thread's captures go; what it recorded and what it gave back add up
            for (int d = 0; d < 2; ++d) {
                for (unsigned long long c = 0; c < 2; ++c) live_graph[d] -= devices.at(d).release_capture(100ull * (unsigned long long)t + c);
                CHECK(live_graph[d] == 0);
            }
        });
    for (auto &th : threads) th.join();
    CHECK(taken.load() >= 1 && taken.load() <= raised.load());
    // the slot accounting afterwards: no graph slot is held; the stream slots held are those of the (stream, role) pairs that
    // still have one, each of them stable and distinct; dropping every stream gives them all back
    for (int d = 0; d < 2; ++d) {
        DeviceState &ds = devices.at(d);
        int held = 0;
        ds.slots_in_use(&held, nullptr);
        in_use(ds, held, 0);
        CHECK(held >= 0 && held <= kThreads * 8 * 4);
        for (int t = 0; t < kThreads; ++t)
            for (uint32_t v = 0; v < 8; ++v) ds.drop_stream(ptr(0x100000u * (uint32_t)(t + 1) + 0x100u * v));
        in_use(ds, 0, 0);
        std::set<int> slots;
        for (int i = 0; i < kSchedSlots; ++i) slots.insert(ds.stream_slot(ptr(0x5000000u + 16u * (uint32_t)i), 0));
        CHECK((int)slots.size() == kSchedSlots && *slots.begin() == 0 && *slots.rbegin() == kSchedSlots - 1);
        CHECK(ds.stream_slot(ptr(0x6000000u), 0) == -1);
    }
}

int main()
{
    check_slot_pool();
    check_stream_slots();
    check_graph_slots();
    check_caches_and_flag();
    check_registry();
    check_threads();
    printf("host state ok\n");
    return 0;
}
