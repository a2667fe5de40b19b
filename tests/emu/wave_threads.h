/*
 * wave_threads.h — a small binding of avk_wave.h's emulator interface (avk_emu::gather / lane / yield) in which the 64 lanes of a wave are 64 OS threads that
 * meet at a barrier in every cross-lane primitive.  wave_emu.cpp runs lanes as fibers inside the solver's emulator library; a translation unit that wants to run
 * one small piece of wave code on its own — tests/emu/size_emu.cpp, tests/native/size_check.cpp — includes this header instead (once: it defines the functions),
 * and, having no context switching of its own, it runs under AddressSanitizer as it is.
 *
 * Test infrastructure: never part of libaardvark_amd.so.  Control flow around the primitives must be wave-uniform, as on the device: a lane that arrives at
 * another call site than lane 0 stops the program.
 */
#ifndef AVK_WAVE_THREADS_H
#define AVK_WAVE_THREADS_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

namespace avk_emu {

struct ThreadWave {
    std::mutex mu;
    std::condition_variable cv;
    int waiting = 0;
    uint64_t generation = 0;
    uint64_t slot[2][64];
    uint32_t site[2][64];
    void barrier() {
        std::unique_lock<std::mutex> lock(mu);
        const uint64_t g = generation;
        if (++waiting == 64) {
            waiting = 0, ++generation;
            cv.notify_all();
        } else
            cv.wait(lock, [&] { return generation != g; });
    }
};
static thread_local ThreadWave *tw_wave = nullptr;
static thread_local int tw_lane = 0;
static thread_local unsigned tw_phase = 0;

/* the deposits alternate between two sets of slots: a lane reads the values of primitive p before it enters primitive p + 1, and nobody writes the slots of
 * primitive p again before every lane has passed the barrier of p + 1 */
const uint64_t *gather(uint64_t v, uint32_t site) {
    ThreadWave &w = *tw_wave;
    const unsigned ph = tw_phase++ & 1u;
    w.slot[ph][tw_lane] = v, w.site[ph][tw_lane] = site;
    w.barrier();
    if (w.site[ph][0] != site) {
        fprintf(stderr, "wave_threads: lane %d is at site %u, lane 0 at site %u: divergent use of a cross-lane primitive\n", tw_lane, site, w.site[ph][0]);
        abort();
    }
    return w.slot[ph];
}
int lane() { return tw_lane; }
void yield() { std::this_thread::yield(); }
const uint64_t *quad_gather(uint64_t, uint32_t) {
    fprintf(stderr, "wave_threads: no quad primitives here\n");
    abort();
}

/* fn(lane) on the 64 lanes of one wave */
template <class F> static void run_wave(F &&fn) {
    ThreadWave w;
    std::vector<std::thread> lanes;
    for (int l = 0; l < 64; ++l)
        lanes.emplace_back([&w, &fn, l] {
            tw_wave = &w, tw_lane = l, tw_phase = 0;
            fn(l);
        });
    for (std::thread &t : lanes) t.join();
}

} // namespace avk_emu

#endif /* AVK_WAVE_THREADS_H */
